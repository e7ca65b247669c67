"""GPU parity: the ranged forms of the fused chains through an N x K GRID of equal elementwise blocks, K = 2 .. 4 (knob grid_chain_range = 1):
jh_chain_apply_range on an ADJOINT / NORMAL grid chain and jh_chain_bidiag_step_range on a FORWARD one (with grid_chain_step = 1 as well).

On a grid the range is positions [first, first + count) INSIDE a block: one call reads those positions of every block row and writes the K pieces
out_k[first, first + count) and nothing else.  The reference is the whole-vector call on the same handle (jh_chain_apply, jh_chain_bidiag_step):
u always has its bits, out / w have them wherever both walk the rows in one part (adj_split = 0), and agree to the many-rows tolerance of
tests/test_gpu_grid_chain_step.py under the split walk.  Every test sets the knobs and puts the defaults (0) back."""
import ctypes as C

import numpy as np
import pytest

from .helpers import DTYPES, assert_bits_equal, u01
from .test_gpu_grid_chains import GridRig
from .test_gpu_grid_chain_step import _knobs
from .test_gpu_grid_step import _host_update, _normsq64

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = 4, 1
SENTINEL = -777.25
NROW = 5


def _flat(x):
    return x.to_numpy().ravel(order="F")


def _grain(dt) -> int:
    """Elements per 16 bytes: what a range's first element and count are multiples of."""
    return max(1, 16 // np.dtype(dt).itemsize)


def _ranges(dt, n):
    """(three ranges that tile [0, n); a one-pack range, an empty range, the partial last pack alone -- the last full pack where n is on the grid)."""
    g = _grain(dt)
    a, b = (n // 4 // g) * g, (3 * n // 4 // g) * g
    last = (n // g) * g if n % g else n - g
    return [(0, a), (a, b - a), (b, n - b)], [(3 * g, g), (2 * g, 0), (last, n - last)]


def _mask(nblk, n, ranges):
    m = np.zeros(nblk * n, dtype=bool)
    for lo, cnt in ranges:
        for k in range(nblk):
            m[k * n + lo:k * n + lo + cnt] = True
    return m


def _lists(nw, dom, scal):
    """Token lists (application order) of L = R o A o P, adjoint(L) and adjoint(L) o L: R of nw weights (the second conjugated) and a scalar, P = M."""
    R = [("W", 0, False)][:nw] + ([("W", 1, True)] if nw == 2 else []) + ([("s", 0.75, "r")] if scal else [])
    Rh = [(t[0], t[1], not t[2]) if t[0] == "W" else t for t in reversed(R)]
    fwd = ([("M", 0, False)] if dom else []) + ["A"] + R
    adj = Rh + ["At"] + ([("M", 0, True)] if dom else [])
    return fwd, adj, fwd + adj


CONFIGS = {
    "W o A": (1, False, False),
    "a * A": (0, False, True),
    "W1' o W0 o A": (2, False, False),
    "W o A o M": (1, True, False),
    "a * (W o A) o M": (1, True, True),
}


def _handle(J, rig, toks, ctype, cache):
    from jets_jl_amd import chains

    # (a tag per chain type: the cache keys a plan by its tag and the number of stages, and adjoint(L) has as many stages as L)
    h = chains.one_run(chains.stages_of(rig.compose(toks)), cache, f"grid_chain_range_test_{ctype}", ctype)
    assert h is not None and h is not True and h.grid, f"{toks}: not one fused run through the grid"
    return h


def _host_in(oracle, dt, k, n, seed):
    return [(u01(oracle, dt, seed, i, n) - dt(0.5)).astype(dt) for i in range(k)]


def _check_apply(J, rig, h, x, spc, accs, want0=None):
    """Tiled and single ranged applications of `h` into sentinel-filled (accumulate +1: random) outputs against the whole-vector call."""
    dt, n, K = rig.dt, rig.n, rig.ncol
    tile, extra = _ranges(dt, n)
    for acc in accs:
        init = _flat(J.rand(spc, seed=13, stream=acc + 2)) if acc == 1 else np.full(K * n, SENTINEL, dtype=dt)
        whole = _flat(h.apply(J.from_numpy(init.copy(), spc), x, acc))
        if want0 is not None and acc == 0:
            assert_bits_equal(whole, want0, "the whole-vector call vs the oracle's stages")
        out, done = J.from_numpy(init.copy(), spc), []
        for r in tile:
            h.apply_range(out, x, r[0], r[1], acc)
            done.append(r)
            got, m = _flat(out), _mask(K, n, done)
            assert_bits_equal(got[~m], init[~m], f"accumulate {acc}: outside the ranges {done} the output keeps what it held")
            assert_bits_equal(got[m], whole[m], f"accumulate {acc}: ranges {done} vs the whole-vector call")
        assert_bits_equal(_flat(out), whole, f"accumulate {acc}: three ranges vs the whole-vector call")
        if want0 is not None and acc == 0:
            assert_bits_equal(_flat(out), want0, "three ranges vs the oracle's stages")
        for r in extra:
            out = J.from_numpy(init.copy(), spc)
            h.apply_range(out, x, r[0], r[1], acc)
            want, m = init.copy(), _mask(K, n, [r])
            want[m] = whole[m]
            assert_bits_equal(_flat(out), want, f"accumulate {acc}: the range {r} alone")


def _step_whole(h, u, v, w, alpha, beta):
    from jets_jl_amd._ffi import check, lib

    out = C.c_double(-1.0)
    check(lib.jh_chain_bidiag_step(h.handle, u.handle, v.handle, w.handle, float(alpha), float(beta), C.byref(out)))
    return out.value


def _check_step(J, rig, h, hv, hu0, alpha, beta, uref=None, finite=True):
    """Tiled (shares read back, then deferred) and single ranged steps against the whole-vector step on the same handle."""
    from jets_jl_amd._ffi import check, lib

    dt, n, K, N = rig.dt, rig.n, rig.ncol, rig.nrow
    R, D = J.range(rig.A), J.domain(rig.A)
    tile, extra = _ranges(dt, n)
    v = J.from_numpy(np.concatenate(hv), D)
    w0 = np.full(K * n, SENTINEL, dtype=dt)
    u, w = J.from_numpy(hu0.copy(), R), J.from_numpy(w0.copy(), D)
    nrm_whole = _step_whole(h, u, v, w, alpha, beta)
    hu, hw = _flat(u), _flat(w)
    if uref is not None:
        assert_bits_equal(hu, uref, "u of the whole-vector step vs the oracle's stages")
    rd = np.dtype(dt).type(0).real.dtype
    if finite:
        assert not np.isnan(hu.view(rd)).any(), "a NaN leaked from the old u"
        assert nrm_whole == pytest.approx(_normsq64(hu), rel=1e-12, abs=0.0)
    for deferred in (False, True):
        u, w, done, total = J.from_numpy(hu0.copy(), R), J.from_numpy(w0.copy(), D), [], 0.0
        if deferred:
            check(lib.jh_normsq_reset())
        for r in tile:
            share = h.bidiag_step_range(u, v, w, alpha, beta, r[0], r[1], read_normsq=not deferred)
            total += 0.0 if deferred else share
            done.append(r)
            if not deferred:
                gu, gw, mu, mw = _flat(u), _flat(w), _mask(N, n, done), _mask(K, n, done)
                assert_bits_equal(gu[~mu], hu0[~mu], f"outside the ranges {done} u keeps what it held")
                assert_bits_equal(gw[~mw], w0[~mw], f"outside the ranges {done} w keeps its sentinel")
                assert_bits_equal(gu[mu], hu[mu], f"u over the ranges {done} vs the whole-vector step")
        if deferred:
            out = C.c_double(-1.0)
            check(lib.jh_normsq_read(C.byref(out)))
            total = out.value
        assert_bits_equal(_flat(u), hu, "u: three ranges vs the whole-vector step")
        assert_bits_equal(_flat(w), hw, "w: three ranges vs the whole-vector step")
        if finite:
            assert not np.isnan(_flat(u).view(rd)).any(), "a NaN leaked from the old u"
            assert total == pytest.approx(_normsq64(hu), rel=1e-12, abs=0.0), f"the shares of ||u||^2 (deferred: {deferred})"
    for r in extra:
        u, w = J.from_numpy(hu0.copy(), R), J.from_numpy(w0.copy(), D)
        share = h.bidiag_step_range(u, v, w, alpha, beta, r[0], r[1], read_normsq=True)
        wu, ww, mu, mw = hu0.copy(), w0.copy(), _mask(N, n, [r]), _mask(K, n, [r])
        wu[mu], ww[mw] = hu[mu], hw[mw]
        assert_bits_equal(_flat(u), wu, f"u: the range {r} alone")
        assert_bits_equal(_flat(w), ww, f"w: the range {r} alone")
        if finite:
            assert share == pytest.approx(_normsq64(hu[mu]), rel=1e-12, abs=0.0), f"the share of ||u||^2 of the range {r}"
    return hu, hw


def _u0(oracle, rig, beta):
    dt, n = rig.dt, rig.n
    hu0 = np.concatenate([(u01(oracle, dt, 93, i, n) - dt(0.25)).astype(dt) for i in range(rig.nrow)])
    return np.full_like(hu0, np.nan) if beta == 0 else hu0                       # beta == 0: u is write-only, a NaN must not leak


def _run_config(J, oracle, rig, cfg, accs, betas, with_oracle):
    from jets_jl_amd import chains

    dt, n = rig.dt, rig.n
    fwd, adj, nrm = _lists(*cfg)
    cache = chains.ChainCache()
    R, D = J.range(rig.A), J.domain(rig.A)
    with _knobs(J, grid_chain_range=1, adj_split=0):
        g0 = chains.STATS["chain_range_calls"]
        hd, hm = _host_in(oracle, dt, rig.nrow, n, 95), _host_in(oracle, dt, rig.ncol, n, 91)
        ha = _handle(J, rig, adj, chains.CHAIN_ADJOINT, cache)
        _check_apply(J, rig, ha, J.from_numpy(np.concatenate(hd), R), D, accs, np.concatenate(rig.ora_apply(adj, hd)) if with_oracle else None)
        hn = _handle(J, rig, nrm, chains.CHAIN_NORMAL, cache)
        _check_apply(J, rig, hn, J.from_numpy(np.concatenate(hm), D), D, accs, np.concatenate(rig.ora_apply(nrm, hm)) if with_oracle else None)
        hf = _handle(J, rig, fwd, chains.CHAIN_FORWARD, cache)
        for beta in betas:
            hu0, uref = _u0(oracle, rig, beta), None
            if with_oracle:
                tt = rig.ora_apply(fwd, hm)
                uref = np.concatenate([_host_update(dt, 1.25, beta, tt[i], hu0[i * n:(i + 1) * n]) for i in range(rig.nrow)])
            _check_step(J, rig, hf, hm, hu0, 1.25, beta, uref)
        assert chains.STATS["chain_range_calls"] > g0
        assert J.tune_get("last_grid_chain_range_shape") & 2 == 0, "adj_split = 0: the ordered walk"
    cache.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ncol", [2, 3, 4])
@pytest.mark.parametrize("n", [4096, 515])
def test_ranged_grid_chains_have_the_bits_of_the_whole_vector_calls(Jets, oracle, dt, ncol, n):
    """W o A (complex types: the conjugated weight in the adjoint): adjoint, L'L (accumulate 0, +1, -2) and the step (beta 0 over NaN, beta != 0),
    each also against the oracle's stage-by-stage result."""
    rig = GridRig(Jets, oracle, dt, NROW, ncol, n)
    _run_config(Jets, oracle, rig, CONFIGS["W o A"], (0, 1, -2), (0.0, -0.5), with_oracle=True)
    rig.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", [k for k in CONFIGS if k != "W o A"])
def test_stage_lists_and_grids_of_several_kinds(Jets, oracle, dt, mixed, name):
    """NW = 0 / 2, a domain-side diagonal, a scalar stage; plain diagonals, and a grid with adjointed diagonals, zero blocks (a whole row of them),
    identities and scalar blocks -- each also against the oracle's stage-by-stage result, so that a term the ranged and the whole-vector kernel got
    wrong in the same way would show."""
    rig = GridRig(Jets, oracle, dt, NROW, 4, 515, mixed=True) if mixed else GridRig(Jets, oracle, dt, NROW, 3, 515)
    _run_config(Jets, oracle, rig, CONFIGS[name], (0, -2), (-0.5,), with_oracle=True)
    rig.close()


def test_many_rows_of_small_blocks_take_the_split_walk(Jets, oracle):
    """600 x 3 of 515 at the default adj_split: the rows are summed in parts (chosen from the range's pack count).  u keeps its bits; w and y agree
    with the whole-vector calls to the tolerance of tests/test_gpu_grid_chain_step.py's many-rows case; two runs give the same bits."""
    from jets_jl_amd import chains

    J, dt = Jets, np.float32
    rig = GridRig(J, oracle, dt, 600, 3, 515)
    n, K, N = rig.n, rig.ncol, rig.nrow
    fwd, adj, nrm = _lists(1, True, False)
    tile, _ = _ranges(dt, n)
    R, D = J.range(rig.A), J.domain(rig.A)
    cache = chains.ChainCache()
    hd, hm = _host_in(oracle, dt, N, n, 95), _host_in(oracle, dt, K, n, 91)
    d, m = J.from_numpy(np.concatenate(hd), R), J.from_numpy(np.concatenate(hm), D)
    hu0 = _u0(oracle, rig, -0.5)
    with _knobs(J, grid_chain_range=1):
        for toks, ctype, x in ((adj, chains.CHAIN_ADJOINT, d), (nrm, chains.CHAIN_NORMAL, m)):
            h = _handle(J, rig, toks, ctype, cache)
            whole = _flat(h.apply(J.from_numpy(np.full(K * n, SENTINEL, dtype=dt), D), x, 0))
            got = []
            for _ in range(2):
                out = J.from_numpy(np.full(K * n, SENTINEL, dtype=dt), D)
                for lo, cnt in tile:
                    h.apply_range(out, x, lo, cnt, 0)
                    assert J.tune_get("last_adj_parts") > 1 and (J.tune_get("last_grid_chain_range_shape") & 2)
                got.append(_flat(out))
            assert_bits_equal(got[0], got[1], f"chain type {ctype}: deterministic")
            np.testing.assert_allclose(got[0], whole, rtol=1e-4, atol=1e-4)
        hf = _handle(J, rig, fwd, chains.CHAIN_FORWARD, cache)
        u, w = J.from_numpy(hu0.copy(), R), J.from_numpy(np.full(K * n, SENTINEL, dtype=dt), D)
        nrm_whole = _step_whole(hf, u, m, w, 1.25, -0.5)
        hu, hw = _flat(u), _flat(w)
        got = []
        for _ in range(2):
            u, w, total = J.from_numpy(hu0.copy(), R), J.from_numpy(np.full(K * n, SENTINEL, dtype=dt), D), 0.0
            for lo, cnt in tile:
                total += hf.bidiag_step_range(u, m, w, 1.25, -0.5, lo, cnt, read_normsq=True)
                assert J.tune_get("last_adj_parts") > 1 and (J.tune_get("last_grid_chain_range_shape") & 2)
            got.append((_flat(u), _flat(w), total))
        assert_bits_equal(got[0][0], got[1][0], "u: deterministic")
        assert_bits_equal(got[0][1], got[1][1], "w: deterministic")
        assert got[0][2] == got[1][2]
        assert_bits_equal(got[0][0], hu, "u: ranges in parts vs the whole-vector step")
        np.testing.assert_allclose(got[0][1], hw, rtol=1e-4, atol=1e-4)
        assert got[0][2] == pytest.approx(_normsq64(hu), rel=1e-12, abs=0.0)
        assert nrm_whole == pytest.approx(_normsq64(hu), rel=1e-12, abs=0.0)
    cache.close()
    rig.close()


def _special_data(oracle, dt, n, nrow, ncol):
    """GridRig data with NaN, +Inf, -0 and a denormal in the partial last pack and on both sides of the first range boundary."""
    tile, _ = _ranges(dt, n)
    a = tile[1][0]
    pos = [n - 1, n - 2, a, a - 1]
    sp = [np.nan, np.inf, -0.0, np.finfo(dt).smallest_subnormal]

    def data(tag, count):
        seed = {"A": 53, "w": 54, "c": 58}[tag[0]] + 7 * sum(int(t) for t in tag[1:])
        arr = (u01(oracle, dt, seed, 0, count) + dt(0.25)).astype(dt)
        if tag[0] == "A":
            i, j = tag[1], tag[2]
            if (i + j) % 2 == 0:
                arr[pos[(i + j) % 4]] = sp[i % 4]
        else:
            for b in range(count // n):
                arr[b * n + pos[(b + tag[1]) % 4]] = sp[(b + 1) % 4]
        return arr

    def sprinkle(blocks, shift):
        for b, x in enumerate(blocks):
            x[pos[(b + shift) % 4]] = sp[(b + shift + 2) % 4]
        return blocks

    return data, sprinkle


@pytest.mark.parametrize("call", ["adjoint", "normal", "step"])
def test_ieee_special_values_in_the_partial_pack_and_at_a_range_boundary(Jets, oracle, call):
    from jets_jl_amd import chains

    J, dt, n, K = Jets, np.float32, 515, 3
    data, sprinkle = _special_data(oracle, dt, n, NROW, K)
    rig = GridRig(J, oracle, dt, NROW, K, n, data=data)
    fwd, adj, nrm = _lists(1, True, False)
    R, D = J.range(rig.A), J.domain(rig.A)
    cache = chains.ChainCache()
    hd, hm = sprinkle(_host_in(oracle, dt, NROW, n, 95), 0), sprinkle(_host_in(oracle, dt, K, n, 91), 1)
    with _knobs(J, grid_chain_range=1, adj_split=0), np.errstate(all="ignore"):
        if call == "adjoint":
            _check_apply(J, rig, _handle(J, rig, adj, chains.CHAIN_ADJOINT, cache), J.from_numpy(np.concatenate(hd), R), D, (0,))
        elif call == "normal":
            _check_apply(J, rig, _handle(J, rig, nrm, chains.CHAIN_NORMAL, cache), J.from_numpy(np.concatenate(hm), D), D, (0,))
        else:
            hu0 = np.concatenate(sprinkle(np.split(_u0(oracle, rig, -0.5), NROW), 2))
            hu, hw = _check_step(J, rig, _handle(J, rig, fwd, chains.CHAIN_FORWARD, cache), hm, hu0, 1.25, -0.5, finite=False)
            assert np.isnan(hu).any() and np.isnan(hw).any(), "the special values went through"
    cache.close()
    rig.close()


def test_refusals_leave_the_outputs_alone(Jets, oracle):
    from jets_jl_amd import chains
    from jets_jl_amd._ffi import lib

    J, dt, n, K = Jets, np.float32, 515, 3
    rig = GridRig(J, oracle, dt, NROW, K, n)
    fwd, adj, nrm = _lists(1, False, False)
    R, D = J.range(rig.A), J.domain(rig.A)
    cache = chains.ChainCache()
    u, v, w, d = J.rand(R, seed=15, stream=0), J.rand(D, seed=14, stream=0), J.rand(D, seed=16, stream=0), J.rand(R, seed=17, stream=0)
    hu, hw = _flat(u).copy(), _flat(w).copy()
    ha, hn, hf = (_handle(J, rig, t, c, cache) for t, c in ((adj, chains.CHAIN_ADJOINT), (nrm, chains.CHAIN_NORMAL), (fwd, chains.CHAIN_FORWARD)))
    g = _grain(dt)

    def apply_range(h, x, first, count):
        return lib.jh_chain_apply_range(h.handle, w.handle, x.handle, 0, first, count)

    def step_range(first, count):
        out = C.c_double(-1.0)
        return lib.jh_chain_bidiag_step_range(hf.handle, u.handle, v.handle, w.handle, 1.0, -0.5, first, count, C.byref(out))

    def untouched(what):
        assert_bits_equal(_flat(u), hu, f"{what}: u as it was")
        assert_bits_equal(_flat(w), hw, f"{what}: w as it was")

    assert J.tune_get("grid_chain_range") == 0, "the default"
    with _knobs(J):                                                            # grid_chain_step = 1, grid_chain_range = 0
        assert apply_range(ha, d, 0, g) == UNSUPPORTED and apply_range(hn, v, 0, g) == UNSUPPORTED and step_range(0, g) == UNSUPPORTED
        untouched("knob 0")
    J.tune(grid_chain_range=1)                                                  # ... = 1 with grid_chain_step = 0: the step alone declines
    try:
        assert J.tune_get("grid_chain_step") == 0
        assert step_range(0, g) == UNSUPPORTED
        untouched("grid_chain_step = 0")
    finally:
        J.tune(grid_chain_range=0)
    with _knobs(J, grid_chain_range=1):
        for first, count, what in ((1, g, "a misaligned first"), (n - g + 1, g, "first + count > n"), (0, g + 1, "a misaligned count inside the block"),
                                   (n, g, "a piece of the flat domain vector"), (-g, g, "a negative first")):
            assert apply_range(ha, d, first, count) == INVALID, what
            assert apply_range(hn, v, first, count) == INVALID, what
            assert step_range(first, count) == INVALID, what
            untouched(what)
        assert apply_range(hf, v, 0, g) == UNSUPPORTED
        untouched("a FORWARD handle")
        assert apply_range(ha, d, 2 * g, 0) == 0 and step_range(2 * g, 0) == 0
        untouched("an empty range")
    cache.close()
    rig.close()
