"""GPU parity: fused chains through an N x K GRID of equal elementwise blocks, K = 2 .. 4 (jh_grid_chain.hip; k_grid_chain).

A' o W o A, (W o A)', W o A, M' o A' o W o A o M ... around a multi-parameter operator are ONE pass each: a lane keeps P(m)_1 .. P(m)_K (and
y_1 .. y_K) in registers and walks the block rows in order.  Every stage rounds where the stage-by-stage composite rounds it (src/Jets.jl:530-540
over JetBlock_df! / df'!, 1010-1057), so every result is BIT-EXACT against the same composite with the planner off (chains.ENABLED = [False]) and
against the oracle's stage loops; many rows of small blocks sum in parts (tolerance; adj_split = 0: ordered, bit-exact)."""
import ctypes as C

import numpy as np
import pytest

from .helpers import DTYPES, assert_bits_equal, u01
from .test_gpu_blockop import _mixed_ops

pytestmark = pytest.mark.gpu


def _grid_kinds(nrow, ncol, mixed):
    if not mixed:
        return [["diag"] * ncol for _ in range(nrow)]
    names = ["diag", "diag_adj", "identity", "scale", "zero"]
    kinds = [[names[(2 * i + 3 * j + i // 4) % 5] for j in range(ncol)] for i in range(nrow)]
    kinds[1] = ["zero"] * ncol                                                   # a whole row of zero blocks: +0 (1022)
    return kinds


class GridRig:
    """An N x K grid A (blocks of n elements) with two weight vectors on its range, two diagonals on its domain (K n elements) and a block-diagonal
    block operator of weights, on the device and in the oracle.  Chains are token lists in APPLICATION order as in tests/test_gpu_chains.py.
    data(tag, n): host arrays in place of the counter generator's U[0,1) streams -- tag ("A", i, j) the coefficients of block (i, j), ("w", k) the
    k-th weights (nrow * n elements), ("c", k) the k-th domain diagonal (ncol * n elements).  kinds: the blocks' kinds (nrow lists of ncol names),
    overriding `mixed`; with_wb=False: no block-diagonal weight operator (nrow^2 children) is built.  The token ("Wb", 0, True) is its adjoint."""

    def __init__(self, J, oracle, dt, nrow, ncol, n, mixed=False, seed=53, data=None, kinds=None, with_wb=True):
        self.J, self.o, self.dt, self.nrow, self.ncol, self.n = J, oracle, dt, nrow, ncol, n
        self.A, self.ora = _mixed_ops(J, oracle, dt, kinds or _grid_kinds(nrow, ncol, mixed), [n] * nrow, [n] * ncol, seed=seed,
                                      coeff=None if data is None else (lambda i, j, nr: data(("A", i, j), nr)))
        R, D = J.range(self.A), J.domain(self.A)
        if data is None:
            self.w = [J.rand(R, seed=seed + 1 + k, stream=0) for k in range(2)]
            self.c = [J.rand(D, seed=seed + 5 + k, stream=0) for k in range(2)]
        else:
            self.w = [J.from_numpy(np.ascontiguousarray(data(("w", k), nrow * n), dtype=dt), R) for k in range(2)]
            self.c = [J.from_numpy(np.ascontiguousarray(data(("c", k), ncol * n), dtype=dt), D) for k in range(2)]
        self.hw = [[b.copy() for b in np.split(w.to_numpy().ravel(order="F"), nrow)] for w in self.w]
        self.hc = [np.split(c.to_numpy().ravel(order="F").copy(), ncol) for c in self.c]
        self.W = [J.JopDiagonal(w) for w in self.w]
        self.M = [J.JopDiagonal(c) for c in self.c]
        spc = J.JetSpace(dt, n)
        rows = []
        for i in range(nrow if with_wb else 0):
            row = [J.JopZeroBlock(spc, spc) for _ in range(nrow)]
            if i % 4 == 3:
                row[i] = J.JopIdentity(spc)
            else:
                d = J.JopDiagonal(self.w[0].arrays[i])
                row[i] = d.H if i % 3 == 1 else d
            rows.append(row)
        self.Wb = J.blockop(rows) if with_wb else None

    def op(self, tok):
        J = self.J
        if tok == "A":
            return self.A
        if tok == "At":
            return self.A.H
        if tok[0] == "W":
            return self.W[tok[1]].H if tok[2] else self.W[tok[1]]
        if tok[0] == "M":
            return self.M[tok[1]].H if tok[2] else self.M[tok[1]]
        if tok[0] == "Wb":
            return self.Wb.H if len(tok) > 2 and tok[2] else self.Wb
        if tok[0] == "s":
            spc = J.range(self.A) if tok[2] == "r" else J.domain(self.A)
            return J.JopLn(dom=spc, rng=spc, df=J.constdiag_df, df_adj=J.constdiag_df_adj, s={"a": tok[1]})
        raise ValueError(tok)

    def compose(self, toks):
        out = self.op(toks[0])
        for t in toks[1:]:
            out = self.J.compose(self.op(t), out)
        return out

    def ora_apply(self, toks, x):
        o, n, dt = self.o, self.n, self.dt
        cur = [b.copy() for b in x]
        for tok in toks:
            if tok == "A":
                cur = o.block_df(self.ora, [np.zeros(n, dt) for _ in range(self.nrow)], cur)
            elif tok == "At":
                cur = o.block_df_adj(self.ora, [np.zeros(n, dt) for _ in range(self.ncol)], cur)
            elif tok[0] in ("W", "M"):
                coef = self.hw[tok[1]] if tok[0] == "W" else self.hc[tok[1]]
                cur = [o.child_mul(o.Block("diag", n, coeff=cf, adjoint=bool(tok[2])), np.zeros(n, dt), b) for cf, b in zip(coef, cur)]
            elif tok[0] == "Wb":
                nxt = []
                for i, b in enumerate(cur):                                    # 0 + product: a block operator of several columns accumulates (1024)
                    if i % 4 == 3:
                        nxt.append(np.zeros(n, dt) + b)
                    else:
                        adj = (i % 3 == 1) != bool(len(tok) > 2 and tok[2])
                        nxt.append(np.zeros(n, dt) + o.child_mul(o.Block("diag", n, coeff=self.hw[0][i], adjoint=adj), np.zeros(n, dt), b))
                cur = nxt
            elif tok[0] == "s":
                cur = o.barr_lincomb([np.empty(n, dt) for _ in cur], [tok[1]], [cur])
            else:
                raise ValueError(tok)
        return cur

    def close(self):
        self.J.close(self.A)
        if self.Wb is not None:
            self.J.close(self.Wb)


CHAINS = {
    "A' o W o A": ["A", ("W", 0, False), "At"],
    "(W o A)'": [("W", 0, True), "At"],
    "W o A": ["A", ("W", 0, False)],
    "M' o A' o W o A o M": [("M", 0, False), "A", ("W", 0, False), "At", ("M", 0, True)],
    "2.5 (A' o W o A)": ["A", ("W", 0, False), "At", ("s", 2.5, "d")],
    "W2 o W1 o A": ["A", ("W", 0, False), ("W", 1, False)],
    "A' o W' o W o A": ["A", ("W", 0, False), ("W", 0, True), "At"],
    "Wb o A": ["A", ("Wb",)],
    "A o M": [("M", 0, False), "A"],                                             # no range-side stage (NW = 0): FORWARD
    "(A o M)'": ["At", ("M", 0, True)],                                          # ADJOINT
    "M' o A' o A o M": [("M", 0, False), "A", "At", ("M", 1, True)],             # NORMAL
}


def _input(J, oracle, rig, toks, dt, seed=91):
    rng_in = toks[0] == "At" or toks[0][0] == "W"
    k = rig.nrow if rng_in else rig.ncol
    hx = [u01(oracle, dt, seed, i, rig.n) for i in range(k)]
    return J.from_numpy(np.concatenate(hx), J.range(rig.A) if rng_in else J.domain(rig.A)), hx


def _both(J, C, x, chains):
    g0, c0 = chains.STATS["grid_chain_calls"], chains.STATS["chain_calls"]
    y1 = J.mul_(J.rand(J.range(C), seed=77, stream=1), C, x)                    # into a DIRTY output
    ran = (chains.STATS["grid_chain_calls"] - g0, chains.STATS["chain_calls"] - c0)
    chains.ENABLED[0] = False
    try:
        y0 = J.mul_(J.rand(J.range(C), seed=78, stream=2), C, x)
    finally:
        chains.ENABLED[0] = True
    return y1.to_numpy().ravel(order="F"), y0.to_numpy().ravel(order="F"), ran


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ncol", [2, 3, 4])
@pytest.mark.parametrize("nrow,n", [(2, 1024), (5, 1027), (9, 4160), (7, 67)])
def test_grid_chains_have_the_bits_of_the_stage_by_stage_composite(Jets, oracle, dt, ncol, nrow, n):
    from jets_jl_amd import chains

    J = Jets
    rig = GridRig(J, oracle, dt, nrow, ncol, n)
    for name, toks in CHAINS.items():
        x, hx = _input(J, oracle, rig, toks, dt)
        y1, y0, ran = _both(J, rig.compose(toks), x, chains)
        assert ran == (1, 1), f"{name}: {ran} (grid, all) fused runs"
        assert_bits_equal(y1, y0, f"{name}: fused vs stage by stage on the device")
        assert_bits_equal(y1, np.concatenate(rig.ora_apply(toks, hx)), f"{name}: fused vs the oracle's stages")
    rig.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ncol", [2, 4])
def test_mixed_kind_grids(Jets, oracle, dt, ncol):
    """Zero blocks, a whole row of zeros, identities, scalars, adjointed diagonals (complex types), and the regularised operator
    [A; lam I] (lam I rows: scalar blocks on the diagonal of the last K rows)."""
    from jets_jl_amd import chains

    J = Jets
    n = 515
    rig = GridRig(J, oracle, dt, 11, ncol, n, mixed=True)
    for name in ("A' o W o A", "(W o A)'", "W o A", "M' o A' o W o A o M", "Wb o A"):
        toks = CHAINS[name]
        x, hx = _input(J, oracle, rig, toks, dt)
        y1, y0, ran = _both(J, rig.compose(toks), x, chains)
        assert ran == (1, 1), name
        assert_bits_equal(y1, y0, f"mixed {name}: fused vs stage by stage")
        assert_bits_equal(y1, np.concatenate(rig.ora_apply(toks, hx)), f"mixed {name}: fused vs the oracle")
    rig.close()
    kinds = [["diag"] * ncol for _ in range(6)] + [["scale" if j == k else "zero" for j in range(ncol)] for k in range(ncol)]
    A, ora = _mixed_ops(J, oracle, dt, kinds, [n] * len(kinds), [n] * ncol, seed=7)
    w = J.rand(J.range(A), seed=3, stream=0)
    Cn = J.compose(A.H, J.compose(J.JopDiagonal(w), A))
    m = J.rand(J.domain(A), seed=4, stream=0)
    y1, y0, ran = _both(J, Cn, m, chains)
    assert ran == (1, 1)
    assert_bits_equal(y1, y0, "regularised A' o W o A")
    J.close(A)


@pytest.mark.parametrize("dt", [np.float32, np.complex128])
def test_sums_of_grid_chains(Jets, oracle, dt):
    from jets_jl_amd import chains

    J = Jets
    rig = GridRig(J, oracle, dt, 6, 3, 1027)
    A, W0, W1 = rig.A, rig.W[0], rig.W[1]
    D = J.domain(A)
    lam2 = J.JopLn(dom=D, rng=D, df=J.constdiag_df, df_adj=J.constdiag_df_adj, s={"a": 0.25})
    cases = [
        (rig.compose(CHAINS["A' o W o A"]) + lam2, D, 2),                  # A' W A + lam^2 I: the chain is the first term, the scalar fused
        (rig.compose(["A", ("W", 0, False)]) - rig.compose(["A", ("W", 1, False)]), D, 2),   # W1 A - W2 A: both terms add themselves
        (rig.compose(["A", ("W", 1, False)]) + rig.compose(["A", ("W", 0, False), ("s", 0.5, "r")]), D, 2),
        # (a bare grid beside them would keep the reference's loop: its forward adds to the temporary as found, 1024)
    ]
    for C, xs, fused in cases:
        x = J.rand(xs, seed=5, stream=1)
        f0 = chains.STATS["sum_terms_fused"]
        y1, y0, ran = _both(J, C, x, chains)
        assert chains.STATS["sum_terms_fused"] - f0 >= fused
        assert ran[0] >= 1
        assert_bits_equal(y1, y0, "sum of grid chains vs stage by stage")
    rig.close()


def _stage_arr(lib_mod, w_ptrs, nrow):
    from jets_jl_amd._ffi import ChainStage, STAGE_DIAG

    arr = (ChainStage * 1)()
    ptrs = (C.c_void_p * nrow)(*w_ptrs)
    arr[0].kind, arr[0].flags, arr[0].a = STAGE_DIAG, 0, 0.0
    arr[0].coeff = C.cast(ptrs, C.POINTER(C.c_void_p))
    return arr, ptrs


@pytest.mark.parametrize("dt", [np.float32, np.complex64])
def test_grid_chain_abi(Jets, oracle, dt):
    """jh_chain_create on a grid for all three types; accumulate 0 / +-1 / +-2 has the stage-by-stage bits; jh_chain_apply_range and
    jh_chain_bidiag_step decline (JH_ERR_UNSUPPORTED) and leave their outputs as they were; grid_chain = 0 restores today's refusal."""
    from jets_jl_amd import chains
    from jets_jl_amd._ffi import CHAIN_ADJOINT, CHAIN_FORWARD, CHAIN_NORMAL, JetsHipError, check, lib

    J = Jets
    nrow, ncol, n = 5, 3, 1027
    rig = GridRig(J, oracle, dt, nrow, ncol, n)
    es = np.dtype(dt).itemsize
    nat = chains.classify(rig.A, None).nat
    mid, keep = _stage_arr(lib, [rig.w[0].ptr + i * n * es for i in range(nrow)], nrow)
    none = (chains.ChainStage * 1)()
    h = {}
    for t in (CHAIN_FORWARD, CHAIN_ADJOINT, CHAIN_NORMAL):
        h[t] = C.c_void_p()
        check(lib.jh_chain_create(nat.handle, t, 0, none, 1, mid, 0, none, C.byref(h[t])))
    R, D = J.range(rig.A), J.domain(rig.A)
    m, d = J.rand(D, seed=11, stream=0), J.rand(R, seed=12, stream=0)
    WA, AtW, AtWA = rig.compose(["A", ("W", 0, False)]), rig.compose([("W", 0, False), "At"]), rig.compose(["A", ("W", 0, False), "At"])
    chains.ENABLED[0] = False
    try:
        ref = {CHAIN_FORWARD: (WA, m, R), CHAIN_ADJOINT: (AtW, d, D), CHAIN_NORMAL: (AtWA, m, D)}
        for t, (Cop, x, spc) in ref.items():
            t_ref = J.mul_(J.zeros(spc), Cop, x).to_numpy().ravel(order="F")
            base = J.rand(spc, seed=13, stream=t)
            hb = base.to_numpy().ravel(order="F")
            for acc in (0, 1, -1, 2, -2):
                out = J.copyto_(J.zeros(spc), base)
                check(lib.jh_chain_apply(h[t], out.handle, x.handle, acc))
                want = {0: t_ref, 1: hb + t_ref, -1: hb - t_ref, 2: np.zeros_like(hb) + t_ref, -2: np.zeros_like(hb) - t_ref}[acc]
                assert_bits_equal(out.to_numpy().ravel(order="F"), want.astype(dt), f"type {t}, accumulate {acc}")
    finally:
        chains.ENABLED[0] = True
    y = J.rand(D, seed=14, stream=0)
    hy = y.to_numpy().copy()
    with pytest.raises(JetsHipError) as e:
        check(lib.jh_chain_apply_range(h[CHAIN_NORMAL], y.handle, m.handle, 0, 0, 4))
    assert e.value.status == 4
    assert_bits_equal(y.to_numpy(), hy, "apply_range left its output alone")
    u, w = J.rand(R, seed=15, stream=0), J.rand(D, seed=16, stream=0)
    hu, hw = u.to_numpy().copy(), w.to_numpy().copy()
    nrm = C.c_double(0)
    with pytest.raises(JetsHipError) as e:
        check(lib.jh_chain_bidiag_step(h[CHAIN_FORWARD], u.handle, m.handle, w.handle, 1.0, 0.0, C.byref(nrm)))
    assert e.value.status == 4
    assert_bits_equal(u.to_numpy(), hu, "bidiag step left u alone")
    assert_bits_equal(w.to_numpy(), hw, "bidiag step left w alone")
    for t in h:
        lib.jh_chain_destroy(h[t])
    J.tune(grid_chain=0)
    try:
        hh = C.c_void_p()
        with pytest.raises(JetsHipError) as e:
            check(lib.jh_chain_create(nat.handle, CHAIN_NORMAL, 0, none, 1, mid, 0, none, C.byref(hh)))
        assert e.value.status == 4
        y_off = J.mul_(J.rand(D, seed=17, stream=0), rig.compose(["A", ("W", 1, False), "At"]), m).to_numpy().ravel(order="F")
    finally:
        J.tune(grid_chain=1)
    y_on = J.mul_(J.rand(D, seed=18, stream=0), rig.compose(["A", ("W", 1, False), "At"]), m).to_numpy().ravel(order="F")
    assert_bits_equal(y_on, y_off, "grid_chain = 0: the stage-by-stage route, the same bits")
    rig.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_every_launch_shape_has_the_same_bits(Jets, oracle, dt):
    """Nontemporal loads on / off (knob nt), one ordered walk / rows in parts (adj_split), and the stages after A' on the folded parts: every
    shape the launcher selects is forced once; the shape counter says which ran."""
    from jets_jl_amd import chains

    J = Jets
    rig = GridRig(J, oracle, dt, 9, 3, 1027)
    seen = set()
    for name in ("A' o W o A", "(W o A)'", "W o A", "2.5 (A' o W o A)"):
        toks = CHAINS[name]
        x, hx = _input(J, oracle, rig, toks, dt)
        want = np.concatenate(rig.ora_apply(toks, hx))
        for nt in (0, 2):
            for split in (0, 3):
                J.tune(nt=nt, adj_split=split)
                try:
                    y = J.mul_(J.rand(J.range(rig.compose(toks)), seed=1, stream=1), rig.compose(toks), x).to_numpy().ravel(order="F")
                    shape = J.tune_get("last_grid_chain_shape")
                finally:
                    J.tune(nt=1, adj_split=-1)
                seen.add(shape)
                assert (shape & 1) == (1 if nt == 2 else 0)
                assert bool(shape & 2) == (split == 3)
                if split == 0 or name == "W o A":
                    assert_bits_equal(y, want, f"{name}, nt {nt}, split {split}")
                else:
                    np.testing.assert_allclose(y, want, rtol=1e-4 if np.dtype(dt).itemsize == 4 else 1e-12, atol=1e-5)
    assert seen >= {0, 1, 2, 3, 6, 7}, seen
    rig.close()


def test_many_rows_of_small_blocks_sum_in_parts(Jets, oracle):
    from jets_jl_amd import chains

    J = Jets
    dt = np.float32
    rig = GridRig(J, oracle, dt, 600, 3, 515)
    toks = CHAINS["A' o W o A"]
    x, hx = _input(J, oracle, rig, toks, dt)
    Cn = rig.compose(toks)
    y1 = J.mul_(J.zeros(J.domain(rig.A)), Cn, x).to_numpy().ravel(order="F")
    assert J.tune_get("last_adj_parts") > 1
    y2 = J.mul_(J.zeros(J.domain(rig.A)), Cn, x).to_numpy().ravel(order="F")
    assert_bits_equal(y1, y2, "deterministic")
    want = np.concatenate(rig.ora_apply(toks, hx))
    np.testing.assert_allclose(y1, want, rtol=1e-4, atol=1e-4)
    J.tune(adj_split=0)
    try:
        y0 = J.mul_(J.zeros(J.domain(rig.A)), Cn, x).to_numpy().ravel(order="F")
    finally:
        J.tune(adj_split=-1)
    assert_bits_equal(y0, want, "adj_split = 0: the ordered walk")
    rig.close()


@pytest.mark.parametrize("dt", [np.float32, np.complex64])
def test_declined_grids_run_stage_by_stage(Jets, oracle, dt):
    """Five block columns, a dense child, a Complex scalar stage: the stage-by-stage composite with the oracle's bits; no grid chain runs for the
    declined grids, and for the Complex scalar only the A' o W o A under it is fused."""
    from jets_jl_amd import chains

    J = Jets
    # K = 5
    n = 260
    A5, ora5 = _mixed_ops(J, oracle, dt, [["diag"] * 5 for _ in range(3)], [n] * 3, [n] * 5, seed=3)
    w = J.rand(J.range(A5), seed=4, stream=0)
    C5 = J.compose(A5.H, J.compose(J.JopDiagonal(w), A5))
    m = J.rand(J.domain(A5), seed=5, stream=0)
    y1, y0, ran = _both(J, C5, m, chains)
    assert ran[0] == 0, "K = 5 is not a grid chain"
    assert_bits_equal(y1, y0, "K = 5")
    hm = np.split(m.to_numpy().ravel(order="F"), 5)
    hw = np.split(w.to_numpy().ravel(order="F"), 3)
    t = oracle.block_df(ora5, [np.zeros(n, dt) for _ in range(3)], hm)
    t = [oracle.child_mul(oracle.Block("diag", n, coeff=c), np.zeros(n, dt), b) for c, b in zip(hw, t)]
    want = np.concatenate(oracle.block_df_adj(ora5, [np.zeros(n, dt) for _ in range(5)], t))
    assert_bits_equal(y1, want, "K = 5 vs the oracle")
    J.close(A5)
    # a dense child: W o A on a 3 x 2 grid of 8-element blocks, dense and diagonal blocks alternating
    nd = 8
    spc = J.JetSpace(dt, nd)
    hd = np.asfortranarray((np.arange(nd * nd).reshape(nd, nd) / (nd * nd)).astype(dt))
    dev, ora = [], []
    for i in range(3):
        drow, orow = [], []
        for j in range(2):
            if (i + j) % 2:
                drow.append(J.JopDense(J.from_numpy(hd)))
                orow.append(oracle.Block("dense", nd, nd, coeff=hd))
            else:
                g = J.rand(spc, seed=9, stream=i + j)
                drow.append(J.JopDiagonal(g))
                orow.append(oracle.Block("diag", nd, coeff=g.to_numpy().ravel(order="F").copy()))
        dev.append(drow)
        ora.append(orow)
    Ad = J.blockop(dev)
    wd = J.rand(J.range(Ad), seed=4, stream=1)
    md = J.rand(J.domain(Ad), seed=2, stream=0)
    y1, y0, ran = _both(J, J.compose(J.JopDiagonal(wd), Ad), md, chains)
    assert ran[0] == 0, "a grid with a dense child is not a grid chain"
    assert_bits_equal(y1, y0, "dense child")
    t = oracle.block_df(ora, [np.zeros(nd, dt) for _ in range(3)], np.split(md.to_numpy().ravel(order="F"), 2))
    hwd = np.split(wd.to_numpy().ravel(order="F"), 3)
    want = np.concatenate([oracle.child_mul(oracle.Block("diag", nd, coeff=c), np.zeros(nd, dt), b) for c, b in zip(hwd, t)])
    assert_bits_equal(y1, want, "dense child vs the oracle")
    J.close(Ad)
    # a Complex scalar stage after A' o W o A: the scalar runs on its own, the run under it is one grid chain
    if np.dtype(dt).kind == "c":
        rig = GridRig(J, oracle, dt, 4, 2, 515)
        D = J.domain(rig.A)
        a = 0.5 + 0.25j
        sc = J.JopLn(dom=D, rng=D, df=J.constdiag_df, df_adj=J.constdiag_df_adj, s={"a": a})
        Cc = J.compose(sc, rig.compose(CHAINS["A' o W o A"]))
        x, hx = _input(J, oracle, rig, CHAINS["A' o W o A"], dt)
        y1, y0, ran = _both(J, Cc, x, chains)
        assert ran[0] == 1, "only A' o W o A under the Complex scalar is a grid chain"
        assert_bits_equal(y1, y0, "Complex scalar stage")
        inner = rig.ora_apply(CHAINS["A' o W o A"], hx)
        want = np.concatenate(oracle.barr_lincomb([np.empty(rig.n, dt) for _ in inner], [a], [inner]))
        assert_bits_equal(y1, want, "Complex scalar stage vs the oracle")
        rig.close()


def _fp64_cgls(A, b, iters):
    x = np.zeros(A.shape[1])
    r = b.copy()
    s = A.T @ r
    p = s.copy()
    g = s @ s
    for _ in range(iters):
        q = A @ p
        al = g / (q @ q)
        x += al * p
        r -= al * q
        s = A.T @ r
        gn = s @ s
        p = s + (gn / g) * p
        g = gn
    return x


def test_solvers_on_a_weighted_grid(Jets, oracle):
    from jets_jl_amd import chains

    J = Jets
    dt = np.float64
    nrow, ncol, n = 6, 3, 64
    rig = GridRig(J, oracle, dt, nrow, ncol, n)
    L = rig.compose(["A", ("W", 0, False)])
    b = J.rand(J.range(L), seed=21, stream=0)
    s0, g0 = chains.STATS["chain_solve_calls"], chains.STATS["grid_chain_calls"]
    res = J.cgnr(L, b, maxiter=10, atol=0.0, btol=0.0)
    assert chains.STATS["chain_solve_calls"] > s0 and chains.STATS["grid_chain_calls"] > g0
    dense = np.zeros((nrow * n, ncol * n))
    for i in range(nrow):
        wi = rig.hw[0][i]
        for k in range(ncol):
            dense[i * n:(i + 1) * n, k * n:(k + 1) * n] = np.diag(wi * rig.ora[i][k].coeff)
    xe = _fp64_cgls(dense, b.to_numpy().ravel(order="F"), 10)
    x = res.x.to_numpy().ravel(order="F")
    assert res.itn == 10
    assert np.linalg.norm(x - xe) / np.linalg.norm(xe) < 1e-9            # (test_gpu_grid_normal.py: the Float64 grid CGNR against the fp64 CGLS)
    for solver in ("lsqr", "cgls"):
        st0, g0, sv0 = chains.STATS["chain_step_calls"], chains.STATS["grid_chain_calls"], chains.STATS["chain_solve_calls"]
        r1 = getattr(J, solver)(L, b, maxiter=8, atol=0.0, btol=0.0)
        # the two passes of every iteration are fused grid chains (FORWARD, then ADJOINT); no one-pass step, no native chain solve
        assert chains.STATS["grid_chain_calls"] - g0 >= 16, f"{solver}: {chains.STATS['grid_chain_calls'] - g0} grid chain calls"
        assert chains.STATS["chain_step_calls"] == st0 and chains.STATS["chain_solve_calls"] == sv0
        chains.ENABLED[0] = False
        try:
            r0 = getattr(J, solver)(L, b, maxiter=8, atol=0.0, btol=0.0)
        finally:
            chains.ENABLED[0] = True
        assert_bits_equal(r1.x.to_numpy(), r0.x.to_numpy(), f"{solver}: two fused grid passes vs stage by stage")
    rig.close()


def test_full_size_weighted_normal_operator_on_64x4_of_256cubed(Jets, oracle):
    """A' o W o A on 64 x 4 of 256^3 Float32 (16 GiB of coefficients, 4 GiB of weights; the range holds 2^32 scalars), the shape of the benchmark,
    launched with the shape and load policy the launcher picks on its own.  Inputs come from the counter-based generator, so the oracle runs on
    regenerated slices (every one of the 64 rows summed in order, bit for bit), and the whole vector is compared with the device's stage-by-stage
    composite (max |difference| == 0), in the pattern of tests/test_gpu_fullsize.py."""
    import math

    from jets_jl_amd import chains

    J = Jets
    nrow, ncol, edge = 64, 4, 256
    n = edge ** 3
    blk = J.JetSpace(np.float32, edge, edge, edge)
    coeff = J.rand(J.JetBSpace([blk] * (nrow * ncol)), seed=1, stream=0)         # block (i, k) = coeff block i K + k
    A = J.blockop([[J.JopDiagonal(coeff.arrays[i * ncol + k]) for k in range(ncol)] for i in range(nrow)])
    w = J.rand(J.range(A), seed=5, stream=0)
    m = J.rand(J.domain(A), seed=2, stream=0)
    C = J.compose(A.H, J.compose(J.JopDiagonal(w), A))
    g0 = chains.STATS["grid_chain_calls"]
    y = J.mul_(J.rand(J.domain(A), seed=7, stream=0), C, m)
    assert chains.STATS["grid_chain_calls"] == g0 + 1
    W = 4096
    for off in (0, (n // 3) // 4 * 4 + 1, n // 2 + 64, n - W):
        ops = [[oracle.Block("diag", W, coeff=oracle.rng_u01(np.float32, 1, 0, (i * ncol + k) * n + off, W)) for k in range(ncol)] for i in range(nrow)]
        hm = [oracle.rng_u01(np.float32, 2, 0, k * n + off, W) for k in range(ncol)]
        t = oracle.block_df(ops, [np.zeros(W, np.float32) for _ in range(nrow)], hm)
        t = [oracle.child_mul(oracle.Block("diag", W, coeff=oracle.rng_u01(np.float32, 5, 0, i * n + off, W)), np.zeros(W, np.float32), t[i])
             for i in range(nrow)]
        ref = oracle.block_df_adj(ops, [np.zeros(W, np.float32) for _ in range(ncol)], t)
        for k in range(ncol):
            assert_bits_equal(y._download(k * n + off, W), ref[k], f"A' o W o A slice at {off} of block column {k}, 64 x 4 of 256^3")
    chains.ENABLED[0] = False
    try:
        y0 = J.mul_(J.zeros(J.domain(A)), C, m)                                  # the stage-by-stage composite on the device
    finally:
        chains.ENABLED[0] = True
    assert chains.STATS["grid_chain_calls"] == g0 + 1
    assert float(J.norm((y - y0).materialize(), math.inf)) == 0.0             # bit-identical on every element
    J.close(A)
