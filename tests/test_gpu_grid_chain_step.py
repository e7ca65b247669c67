"""GPU parity: the one-pass Golub-Kahan step of a FORWARD chain L = R o A o P through an N x K GRID of equal elementwise blocks, K = 2 .. 4
(jh_grid_chain_step.hip behind jh_chain_bidiag_step, knob grid_chain_step = 1), and the native LSQR / CGLS loops that iterate on it
(jh_lsqr_solve_chain, jh_cgls_solve_chain).

The step replaces three calls on the device: the FORWARD grid chain into a zeroed range vector (src/Jets.jl:530-540 over 1010-1032),
jh_lincomb(u, [alpha, beta], [t, u]) and the derived ADJOINT grid chain (1034-1057).  u and w keep their bits (beta == 0: u = alpha t and u is not
read); ||u||^2 is the fp64 sum of the new u.  Many rows of small blocks sum w in parts (tolerance; adj_split = 0: the ordered walk, bit-exact).
Every test sets the knob to 1 and puts the default (0) back."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from .helpers import DTYPES, assert_bits_equal, u01
from .test_gpu_blockop import _mixed_ops
from .test_gpu_grid_chains import GridRig, _fp64_cgls, _stage_arr
from .test_gpu_grid_step import _host_update, _normsq64

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = 4, 1


@contextlib.contextmanager
def _knobs(J, **kw):
    """grid_chain_step = 1 (and the other knobs given) for the body; the defaults afterwards."""
    saved = {k: J.tune_get(k) for k in kw}
    J.tune(grid_chain_step=1, **kw)
    try:
        yield
    finally:
        J.tune(grid_chain_step=0, **saved)


def _flat(x):
    return x.to_numpy().ravel(order="F")


def _guarded(J, dt, n, nblocks, seed):
    """A vector of `nblocks` blocks of n elements between two guard blocks: (the slab, the view of the blocks in the middle)."""
    from jets_jl_amd._ffi import check, lib
    from jets_jl_amd.arrays import BlockArray

    spc = J.JetSpace(dt, n)
    big = J.rand(J.JetBSpace([spc] * (nblocks + 2)), seed=seed, stream=9)
    h = C.c_void_p()
    check(lib.jh_bvec_view(big.handle, 1, nblocks, C.byref(h)))
    return big, BlockArray(h, [spc] * nblocks, np.dtype(dt), owner=big)


def _inputs(J, oracle, rig, dt, beta):
    n = rig.n
    hv = [(u01(oracle, dt, 91, k, n) - dt(0.5)).astype(dt) for k in range(rig.ncol)]
    hu0 = np.concatenate([(u01(oracle, dt, 93, i, n) - dt(0.25)).astype(dt) for i in range(rig.nrow)])
    if beta == 0:
        hu0 = np.full_like(hu0, np.nan)                                         # u is write-only: a NaN must not leak
    return hv, hu0, J.from_numpy(np.concatenate(hv), J.domain(rig.A))


def _check_step(J, oracle, rig, toks, alpha, beta, with_oracle=True):
    """One step at the knobs in force, on guarded vectors, against the device's three calls (and the oracle's stages).  Returns (u, w, ||u||^2, the
    derived ADJOINT grid chain of the new u).  beta == 0: u = alpha t (one product, as the tall chains' step: tests/test_gpu_chain_step.py), and
    where no product is a zero also the bits of jh_lincomb(u, [alpha, 0], [t, u]) on a zeroed u (a product of -0 would come out as +0 there)."""
    from jets_jl_amd import chains
    from jets_jl_amd.arrays import lincomb_

    dt, n, nrow, ncol = rig.dt, rig.n, rig.nrow, rig.ncol
    L = rig.compose(toks)
    R, D = J.range(L), J.domain(L)
    sc = chains.SolverChains(L)
    assert sc.fwd is not None and sc.fwd.grid, "not one FORWARD run through a grid"
    hv, hu0, v = _inputs(J, oracle, rig, dt, beta)
    bigu, u = _guarded(J, dt, n, nrow, 71)
    bigw, w = _guarded(J, dt, n, ncol, 72)                                      # (w: a DIRTY output)
    J.copyto_(u, J.from_numpy(hu0, R))
    gu, gw = bigu.to_numpy().ravel(order="F").copy(), bigw.to_numpy().ravel(order="F").copy()
    s0, g0 = chains.STATS["chain_step_calls"], chains.STATS["grid_chain_calls"]
    nrm2 = sc.step(u, v, w, alpha, beta)
    assert nrm2 is not None, "the library declined the step"
    assert chains.STATS["chain_step_calls"] == s0 + 1 and chains.STATS["grid_chain_calls"] == g0 + 1
    au, aw = bigu.to_numpy().ravel(order="F"), bigw.to_numpy().ravel(order="F")
    hu, hw = au[n:-n].copy(), aw[n:-n].copy()
    for got, was, name in ((au, gu, "u"), (aw, gw, "w")):
        assert_bits_equal(got[:n], was[:n], f"the guard block in front of {name}")
        assert_bits_equal(got[-n:], was[-n:], f"the guard block behind {name}")
    assert not np.isnan(hu.view(np.dtype(dt).type(0).real.dtype)).any(), "a NaN leaked from the old u"
    # the device's three calls: the FORWARD grid chain into zeros, the lincomb, the derived ADJOINT grid chain of the new u
    g0 = chains.STATS["grid_chain_calls"]
    t = J.mul_(J.zeros(R), L, v)
    u2 = J.from_numpy(hu0 if beta != 0 else np.zeros_like(hu0), R)
    if beta != 0:
        lincomb_(u2, [float(alpha), float(beta)], [t, u2])
    else:
        if np.all(_flat(t) != 0):
            assert_bits_equal(hu, _flat(lincomb_(J.zeros(R), [float(alpha), 0.0], [t, u2])), "u vs jh_lincomb(u, [alpha, 0], [t, u])")
        lincomb_(u2, [float(alpha)], [t])
    w2 = J.mul_(J.rand(D, seed=18, stream=5), L.H, J.from_numpy(hu, R))
    assert chains.STATS["grid_chain_calls"] == g0 + 2, "the reference route is two fused grid chains"
    assert_bits_equal(hu, _flat(u2), "u vs the FORWARD grid chain + jh_lincomb")
    if with_oracle:
        tt = rig.ora_apply(toks, hv)
        uref = np.concatenate([_host_update(dt, alpha, beta, tt[i], hu0[i * n:(i + 1) * n]) for i in range(nrow)])
        assert_bits_equal(hu, uref, "u vs the oracle's stages")
    assert nrm2 == pytest.approx(_normsq64(hu), rel=1e-12, abs=0.0)
    sc.close()
    return hu, hw, nrm2, _flat(w2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ncol", [2, 3, 4])
@pytest.mark.parametrize("n", [1024, 1027])
@pytest.mark.parametrize("beta", [0.0, -0.5])
def test_grid_chain_step_has_the_bits_of_the_three_calls(Jets, oracle, dt, ncol, n, beta):
    J = Jets
    rig = GridRig(J, oracle, dt, 5, ncol, n)
    toks = ["A", ("W", 0, np.dtype(dt).kind == "c")]                            # L = W o A; complex types: the conjugated weight
    with _knobs(J, adj_split=0):
        hu, hw, _, wref = _check_step(J, oracle, rig, toks, 1.25, beta)
        assert_bits_equal(hw, wref, "w vs the derived ADJOINT grid chain of the new u")
    rig.close()


STAGE_LISTS = {
    "a * A": ["A", ("s", 0.75, "r")],                                            # NW = 0
    "W1' o W0 o A": ["A", ("W", 0, False), ("W", 1, True)],                      # NW = 2
    "W o A o M": [("M", 0, False), "A", ("W", 0, False)],                        # a domain stage: P before, Q = P^H after
    "a * (W o A)": ["A", ("W", 0, False), ("s", 0.75, "r")],                     # a scalar on the range
}


@pytest.mark.parametrize("dt", [np.float32, np.complex64])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", list(STAGE_LISTS))
def test_stage_lists_and_grids_of_several_kinds(Jets, oracle, dt, mixed, name):
    """NW = 0 / 2, a domain stage, a range scalar; on plain diagonals and on a grid with adjointed diagonals, zero blocks, identities, scalar blocks
    and a whole row of zeros (u_i <- alpha R(0) + beta u_i, nothing added to w)."""
    J = Jets
    rig = GridRig(J, oracle, dt, 11, 4, 515, mixed=True) if mixed else GridRig(J, oracle, dt, 5, 3, 1027)
    with _knobs(J, adj_split=0):
        for beta in (0.0, -0.5):
            hu, hw, _, wref = _check_step(J, oracle, rig, STAGE_LISTS[name], -1.5, beta)
            assert_bits_equal(hw, wref, f"{name}: w vs the derived ADJOINT grid chain")
    rig.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_every_launch_shape(Jets, oracle, dt):
    """Nontemporal loads on / off (knob nt), one ordered walk / rows in parts (adj_split): the counter's bits follow the knobs, u has the same bits
    in every shape, w the bits for the ordered walk and tolerance parity in parts."""
    J = Jets
    rig = GridRig(J, oracle, dt, 9, 3, 1027)
    toks = ["A", ("W", 0, False)]
    base = None
    for nt in (0, 2):
        for split in (0, 3):
            with _knobs(J, nt=nt, adj_split=split):
                hu, hw, nrm2, wref = _check_step(J, oracle, rig, toks, 1.25, -0.5, with_oracle=False)
                shape = J.tune_get("last_grid_chain_step_shape")                # (the step's own counter: the reference chains leave it alone)
            assert (shape & 1) == (1 if nt == 2 else 0), (nt, split, shape)
            assert bool(shape & 2) == (split == 3), (nt, split, shape)
            if base is None:
                base = (hu, hw)
            assert_bits_equal(hu, base[0], f"u, nt {nt}, split {split}")
            if split == 0:
                assert_bits_equal(hw, base[1], f"w, nt {nt}, ordered walk")
                assert_bits_equal(hw, wref, "w vs the derived ADJOINT grid chain")
            else:
                np.testing.assert_allclose(hw, base[1], rtol=1e-4 if np.dtype(dt).itemsize == 4 else 1e-12, atol=1e-5)
    rig.close()


def test_many_rows_of_small_blocks_take_parts_by_themselves(Jets, oracle):
    from jets_jl_amd import chains

    J = Jets
    dt = np.float32
    rig = GridRig(J, oracle, dt, 600, 3, 515)
    L = rig.compose(["A", ("W", 0, False)])
    hv, hu0, v = _inputs(J, oracle, rig, dt, -0.5)
    with _knobs(J):
        sc = chains.SolverChains(L)
        got = []
        for _ in range(2):
            u, w = J.from_numpy(hu0, J.range(L)), J.rand(J.domain(L), seed=3, stream=1)
            nrm2 = sc.step(u, v, w, 1.25, -0.5)
            assert nrm2 is not None
            assert J.tune_get("last_adj_parts") > 1 and (J.tune_get("last_grid_chain_step_shape") & 2)
            got.append((_flat(u), _flat(w), nrm2))
        assert_bits_equal(got[0][0], got[1][0], "u: deterministic")
        assert_bits_equal(got[0][1], got[1][1], "w: deterministic")
        assert got[0][2] == got[1][2]
        sc.close()
    with _knobs(J, adj_split=0):
        sc = chains.SolverChains(L)
        u, w = J.from_numpy(hu0, J.range(L)), J.rand(J.domain(L), seed=3, stream=1)
        assert sc.step(u, v, w, 1.25, -0.5) is not None
        assert_bits_equal(_flat(u), got[0][0], "u: in parts and in order")
        np.testing.assert_allclose(got[0][1], _flat(w), rtol=1e-4, atol=1e-4)   # (the tolerance of the grid chains' many-rows test)
        sc.close()
    rig.close()


def _raw_step(fwd_handle, u, v, w, ranged=False):
    from jets_jl_amd._ffi import lib

    out = C.c_double(-1.0)
    if ranged:
        return lib.jh_chain_bidiag_step_range(fwd_handle, u.handle, v.handle, w.handle, 1.0, -0.5, 0, 4, C.byref(out))
    return lib.jh_chain_bidiag_step(fwd_handle, u.handle, v.handle, w.handle, 1.0, -0.5, C.byref(out))


@pytest.mark.parametrize("dt", [np.float32, np.complex64])
def test_declines_leave_the_outputs_alone(Jets, oracle, dt):
    from jets_jl_amd import chains
    from jets_jl_amd._ffi import CHAIN_ADJOINT, check, lib

    J = Jets
    nrow, ncol, n = 5, 3, 1027
    rig = GridRig(J, oracle, dt, nrow, ncol, n)
    L = rig.compose(["A", ("W", 0, False)])
    R, D = J.range(L), J.domain(L)
    u, v, w = J.rand(R, seed=15, stream=0), J.rand(D, seed=14, stream=0), J.rand(D, seed=16, stream=0)
    hu, hw = _flat(u).copy(), _flat(w).copy()

    def untouched(what):
        assert_bits_equal(_flat(u), hu, f"{what}: u as it was")
        assert_bits_equal(_flat(w), hw, f"{what}: w as it was")

    sc = chains.SolverChains(L)
    assert sc.fwd is not None and sc.fwd.grid
    assert J.tune_get("grid_chain_step") == 0, "the default"
    assert _raw_step(sc.fwd.handle, u, v, w) == UNSUPPORTED                     # knob 0
    untouched("knob 0")
    assert sc.step(u, v, w, 1.0, -0.5) is None                                  # ... and the Python route does not call the library
    with _knobs(J):
        assert _raw_step(sc.fwd.handle, u, v, w, ranged=True) == UNSUPPORTED    # no ranged form under either setting
        untouched("the ranged step")
        # three range-side stages: R and R^H together exceed four
        sc3 = chains.SolverChains(rig.compose(["A", ("W", 0, False), ("W", 1, False), ("s", 0.75, "r")]))
        assert sc3.fwd is not None and sc3.fwd.grid
        assert _raw_step(sc3.fwd.handle, u, v, w) == UNSUPPORTED
        untouched("three range-side stages")
        sc3.close()
        # an ADJOINT-type handle: the existing INVALID
        es = np.dtype(dt).itemsize
        nat = chains.classify(rig.A, None).nat
        mid, keep = _stage_arr(lib, [rig.w[0].ptr + i * n * es for i in range(nrow)], nrow)
        none = (chains.ChainStage * 1)()
        ha = C.c_void_p()
        check(lib.jh_chain_create(nat.handle, CHAIN_ADJOINT, 0, none, 1, mid, 0, none, C.byref(ha)))
        assert _raw_step(ha, u, v, w) == INVALID
        untouched("an ADJOINT handle")
        lib.jh_chain_destroy(ha)
        # K = 5 never builds a grid chain
        A5, _ = _mixed_ops(J, oracle, dt, [["diag"] * 5 for _ in range(3)], [260] * 3, [260] * 5, seed=3)
        sc5 = chains.SolverChains(J.compose(J.JopDiagonal(J.rand(J.range(A5), seed=4, stream=0)), A5))
        assert sc5.fwd is None
        sc5.close()
        J.close(A5)
    sc.close()
    rig.close()


def _fp64_lsqr(A, b, iters):
    """Paige & Saunders' LSQR (damp = 0) in numpy fp64."""
    x = np.zeros(A.shape[1])
    beta = np.linalg.norm(b)
    u = b / beta
    v = A.T @ u
    alpha = np.linalg.norm(v)
    v = v / alpha
    w = v.copy()
    phibar, rhobar = beta, alpha
    for _ in range(iters):
        u = A @ v - alpha * u
        beta = np.linalg.norm(u)
        u = u / beta
        v = A.T @ u - beta * v
        alpha = np.linalg.norm(v)
        v = v / alpha
        rho = np.hypot(rhobar, beta)
        c, s = rhobar / rho, beta / rho
        theta, rhobar = s * alpha, -c * alpha
        phi, phibar = c * phibar, s * phibar
        x = x + (phi / rho) * w
        w = v - (theta / rho) * w
    return x


def _dense(rig):
    nrow, ncol, n = rig.nrow, rig.ncol, rig.n
    dense = np.zeros((nrow * n, ncol * n))
    for i in range(nrow):
        for k in range(ncol):
            dense[i * n:(i + 1) * n, k * n:(k + 1) * n] = np.diag(rig.hw[0][i] * rig.ora[i][k].coeff)
    return dense


def test_solvers_iterate_on_the_step(Jets, oracle, monkeypatch):
    from jets_jl_amd import chains

    J = Jets
    rig = GridRig(J, oracle, np.float64, 6, 3, 64)
    L = rig.compose(["A", ("W", 0, False)])
    b = J.rand(J.range(L), seed=21, stream=0)
    iters = 8
    dense, hb = _dense(rig), b.to_numpy().ravel(order="F")
    want = {"lsqr": _fp64_lsqr(dense, hb, iters), "cgls": _fp64_cgls(dense, hb, iters)}
    for solver in ("lsqr", "cgls"):
        with _knobs(J):
            sv0, st0 = chains.STATS["chain_solve_calls"], chains.STATS["chain_step_calls"]
            r1 = getattr(J, solver)(L, b, maxiter=iters, atol=0.0, btol=0.0)
            assert chains.STATS["chain_solve_calls"] == sv0 + 1, f"{solver}: the native solve on the grid chain"
            assert r1.itn == iters
            x = r1.x.to_numpy().ravel(order="F")
            assert np.linalg.norm(x - want[solver]) / np.linalg.norm(want[solver]) < 1e-9
            monkeypatch.setenv("JETS_LSQR_NATIVE" if solver == "lsqr" else "JETS_CGLS_NATIVE", "0")
            try:
                sv0, st0 = chains.STATS["chain_solve_calls"], chains.STATS["chain_step_calls"]
                r2 = getattr(J, solver)(L, b, maxiter=iters, atol=0.0, btol=0.0)
            finally:
                monkeypatch.undo()
            assert chains.STATS["chain_solve_calls"] == sv0 and chains.STATS["chain_step_calls"] - st0 >= iters, solver
            x2 = r2.x.to_numpy().ravel(order="F")
            assert np.linalg.norm(x2 - want[solver]) / np.linalg.norm(want[solver]) < 1e-9
        # the knob back at 0: the same call advances neither counter
        sv0, st0 = chains.STATS["chain_solve_calls"], chains.STATS["chain_step_calls"]
        getattr(J, solver)(L, b, maxiter=iters, atol=0.0, btol=0.0)
        assert chains.STATS["chain_solve_calls"] == sv0 and chains.STATS["chain_step_calls"] == st0, solver
    rig.close()


def test_float32_damped_warm_start_agrees_with_the_two_pass_route(Jets, oracle):
    J = Jets
    rig = GridRig(J, oracle, np.float32, 6, 3, 64)
    L = rig.compose(["A", ("W", 0, False)])
    b = J.rand(J.range(L), seed=21, stream=0)
    x0 = J.rand(J.domain(L), seed=22, stream=0)
    for solver in ("lsqr", "cgls"):
        with _knobs(J):
            r1 = getattr(J, solver)(L, b, x0=x0, damp=0.1, maxiter=8, atol=0.0, btol=0.0)
        r0 = getattr(J, solver)(L, b, x0=x0, damp=0.1, maxiter=8, atol=0.0, btol=0.0)
        a, c = r1.x.to_numpy().ravel(order="F").astype(np.float64), r0.x.to_numpy().ravel(order="F").astype(np.float64)
        assert np.linalg.norm(a - c) / np.linalg.norm(c) < 1e-5, solver
    rig.close()
