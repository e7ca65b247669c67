"""GPU parity: the three ranged calls on an N x K GRID of equal elementwise blocks, K = 2 .. 4, behind the knob grid_range = 1
(jh_blockop_mul_adj_range, jh_blockop_normal_mul_range, jh_blockop_bidiag_step_range: jh_grid_range.hip, jh_grid_normal.hip, jh_grid_step.hip).

On a grid the range [first, first + count) is positions INSIDE a block: one call touches those positions of every u_i and writes the K pieces
w_k[first, first + count) (the adjoint: m_k, A'A: y_k) and nothing else.  u always has the whole-vector call's bits; w / m / y have them where both
walk the rows in one part (adj_split = 0); the many-small-rows split walk per range is tolerance parity (the bound of tests/test_gpu_chain_range.py).
The shares of ||u||^2, added in enqueue order through jh_normsq_reset / jh_normsq_read, are the fp64 sum of the new u to 1e-12 relative (fp64
partials summed in another order: the bound of tests/test_gpu_grid_step.py)."""
import ctypes as C

import numpy as np
import pytest

from .helpers import DTYPES, assert_bits_equal
from .test_gpu_blockop import _mixed_ops
from .test_gpu_grid_step import _flat, _native, _normsq64

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
NROW = 5


@pytest.fixture
def grid_range(Jets):
    """grid_range = 1 and the ordered row walk for the body; the defaults afterwards."""
    Jets.tune(grid_range=1, adj_split=0)
    yield Jets
    Jets.tune(grid_range=0, adj_split=-1)


def _kinds(variant, ncol):
    """plain: all diagonals.  several: the regularised [[A11 A12 ..]; [lam I 0 ..]; [0 lam I ..]; ..] -- K rows of one scalar / identity block each
    under the diagonal rows, one of which holds an adjointed diagonal."""
    top = NROW - ncol if variant == "several" else NROW
    kinds = [["diag"] * ncol for _ in range(top)]
    if variant == "several":
        kinds[0][ncol - 1] = "diag_adj"
        kinds += [[("scale" if r % 2 == 0 else "identity") if k == r else "zero" for k in range(ncol)] for r in range(ncol)]
    return kinds


def _pack(dt):
    return 16 // np.dtype(dt).itemsize


def _three_ranges(dt, n):
    """Three ranges with 16-byte bounds that cover the block; the last ends with it (inside a pack when n is off the 16-byte grid)."""
    pe = _pack(dt)
    a, b = n // 3 // pe * pe, 2 * n // 3 // pe * pe
    return [(0, a), (a, b - a), (b, n - b)]


def _calls(J, A):
    """The three ranged calls and their whole-vector twins on one operator: name -> (ranged(out, in, lo, cnt), whole(out, in)) for the
    adjoint and A'A; the step apart (it updates u as well)."""
    from jets_jl_amd._ffi import lib

    nat = _native(A)
    return nat, {
        "adjoint": (lambda m, d, lo, cnt: lib.jh_blockop_mul_adj_range(nat.handle, m.handle, d.handle, lo, cnt),
                    lambda m, d: lib.jh_blockop_mul_adj(nat.handle, m.handle, d.handle)),
        "normal": (lambda y, m, lo, cnt: lib.jh_blockop_normal_mul_range(nat.handle, y.handle, m.handle, lo, cnt),
                   lambda y, m: lib.jh_blockop_normal_mul(nat.handle, y.handle, m.handle)),
    }


def _step_range(nat, u, v, w, alpha, beta, lo, cnt, out=None):
    from jets_jl_amd._ffi import lib

    return lib.jh_blockop_bidiag_step_range(nat.handle, u.handle, v.handle, w.handle, float(alpha), float(beta), lo, cnt,
                                            None if out is None else C.byref(out))


def _step(nat, u, v, w, alpha, beta):
    from jets_jl_amd._ffi import lib

    out = C.c_double(-1.0)
    assert lib.jh_blockop_bidiag_step(nat.handle, u.handle, v.handle, w.handle, float(alpha), float(beta), C.byref(out)) == 0
    return out.value


def _normsq_read():
    from jets_jl_amd._ffi import lib

    out = C.c_double(-1.0)
    assert lib.jh_normsq_read(C.byref(out)) == 0
    return out.value


def _inside(n, ncol, ranges, rows=None):
    """Boolean masks of the positions the ranges cover: over the flat K n domain, and over the flat N n range."""
    blk = np.zeros(n, dtype=bool)
    for lo, cnt in ranges:
        blk[lo:lo + cnt] = True
    return np.tile(blk, ncol), np.tile(blk, NROW if rows is None else rows)


def _assert_range(got, want, found, mask, what):
    """`got` has the bits of `want` on the mask and of `found` (what the vector held before) off it."""
    assert_bits_equal(got[mask], want[mask], f"{what}: inside the ranges")
    assert_bits_equal(got[~mask], found[~mask], f"{what}: outside the ranges nothing changed")


class Case:
    """One grid, its inputs, and the whole-vector results under adj_split = 0 (computed once per test)."""

    def __init__(self, J, oracle, dt, ncol, n, variant):
        from jets_jl_amd._ffi import lib

        self.J, self.dt, self.ncol, self.n = J, dt, ncol, n
        self.A, _ = _mixed_ops(J, oracle, dt, _kinds(variant, ncol), [n] * NROW, [n] * ncol, seed=53)
        self.nat, self.calls = _calls(J, self.A)
        self.v = J.rand(J.domain(self.A), seed=61, stream=0)
        self.d = J.rand(J.range(self.A), seed=62, stream=0)
        self.hu0 = _flat(J.rand(J.range(self.A), seed=63, stream=0)).copy()
        self.dirty_dom = _flat(J.rand(J.domain(self.A), seed=64, stream=0)).copy()       # the sentinel the outputs are pre-filled with
        self.alpha, self.beta = 1.25, -0.625
        self.want = {}
        for name, (_, whole) in self.calls.items():
            out = self.dom_sentinel()
            assert whole(out, self.d if name == "adjoint" else self.v) == 0
            self.want[name] = _flat(out).copy()
        for beta in (self.beta, 0.0):
            u, w = self.u_found(beta), self.dom_sentinel()
            nrm = _step(self.nat, u, self.v, w, self.alpha, beta)
            self.want["step", beta] = (_flat(u).copy(), _flat(w).copy(), nrm)
        assert lib.jh_normsq_reset() == 0

    def dom_sentinel(self):
        return self.J.from_numpy(self.dirty_dom, self.J.domain(self.A))

    def hu_found(self, beta):
        return np.full_like(self.hu0, np.nan) if beta == 0 else self.hu0                # beta == 0: u is write-only, a NaN must not leak

    def u_found(self, beta):
        return self.J.from_numpy(self.hu_found(beta), self.J.range(self.A))

    def close(self):
        self.J.close(self.A)


def _run_ranges(case, ranges, what):
    """All three calls over `ranges` on sentinel-filled outputs: bits inside, nothing outside; the deferred shares of ||u||^2."""
    from jets_jl_amd._ffi import lib

    dom_in, rng_in = _inside(case.n, case.ncol, ranges)
    for name, (ranged, _) in case.calls.items():
        out = case.dom_sentinel()
        for lo, cnt in ranges:
            assert ranged(out, case.d if name == "adjoint" else case.v, lo, cnt) == 0, f"{what}: {name} [{lo}, {lo + cnt})"
        _assert_range(_flat(out), case.want[name], case.dirty_dom, dom_in, f"{what}: {name}")
    for beta in (case.beta, 0.0):
        u, w = case.u_found(beta), case.dom_sentinel()
        hu_ref, hw_ref, _ = case.want["step", beta]
        assert lib.jh_normsq_reset() == 0
        for lo, cnt in ranges:
            assert _step_range(case.nat, u, case.v, w, case.alpha, beta, lo, cnt) == 0, f"{what}: step [{lo}, {lo + cnt}) beta {beta}"
        total = _normsq_read()
        hu, hw = _flat(u), _flat(w)
        found = case.hu_found(beta)
        assert_bits_equal(hu[rng_in], hu_ref[rng_in], f"{what}: u inside the ranges (beta {beta})")
        assert_bits_equal(hu[~rng_in], found[~rng_in], f"{what}: u outside the ranges (beta {beta})")
        _assert_range(hw, hw_ref, case.dirty_dom, dom_in, f"{what}: w (beta {beta})")
        assert not np.isnan(hu[rng_in].view(hu.real.dtype)).any(), "a NaN of the write-only u leaked"
        assert total == pytest.approx(_normsq64(hu[rng_in]), rel=1e-12, abs=0.0), f"{what}: deferred ||u||^2 (beta {beta})"
    # the shares returned one by one add up too
    u, w = case.u_found(case.beta), case.dom_sentinel()
    shares = []
    for lo, cnt in ranges:
        out = C.c_double(-1.0)
        assert _step_range(case.nat, u, case.v, w, case.alpha, case.beta, lo, cnt, out) == 0
        shares.append(out.value)
    assert sum(shares) == pytest.approx(_normsq64(_flat(u)[rng_in]), rel=1e-12, abs=0.0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ncol", [2, 3, 4])
@pytest.mark.parametrize("n", [4096, 515])
@pytest.mark.parametrize("variant", ["plain", "several"])
def test_ranges_have_the_bits_of_the_whole_vector_calls(grid_range, oracle, dt, ncol, n, variant):
    """N = 5: three ranges that cover the block (the last ends with it -- at 515 elements inside a pack, and every column after the first is
    off the 16-byte grid), one range of a single pack, one empty range."""
    J = grid_range
    case = Case(J, oracle, dt, ncol, n, variant)
    try:
        pe = _pack(dt)
        _run_ranges(case, _three_ranges(dt, n), "three ranges")
        assert J.tune_get("last_grid_range_shape") & 2 == 0, "adj_split = 0: the rows in one part"
        _run_ranges(case, [(n // 2 // pe * pe, pe)], "one pack")
        _run_ranges(case, [(n // 4 // pe * pe, 0)], "an empty range")
        if n % pe:
            _run_ranges(case, [(n // pe * pe, n % pe)], "the partial last pack alone")
    finally:
        case.close()


@pytest.mark.parametrize("nt", [0, 2])
def test_the_nontemporal_rule_is_the_whole_calls(grid_range, oracle, nt):
    """Knob nt = 0 / 2 reaches the ranged kernels (counter bit 0), with the same bits."""
    J = grid_range
    J.tune(nt=nt)
    try:
        case = Case(J, oracle, np.float32, 3, 515, "several")
        _run_ranges(case, _three_ranges(np.float32, 515), f"nt = {nt}")
        assert J.tune_get("last_grid_range_shape") & 1 == (1 if nt == 2 else 0)
        case.close()
    finally:
        J.tune(nt=1)


def test_many_small_rows_take_the_split_walk_per_range(Jets, oracle):
    """600 x 3 of 515 Float32 on the automatic split walk: every range cuts the row sum into parts of its own -- u to the bit, w within the
    split walk's tolerance of the whole-vector call."""
    J = Jets
    dt, nrow, ncol, n = np.float32, 600, 3, 515
    blk = J.JetSpace(dt, n)
    coeff = J.rand(J.JetBSpace([blk] * (nrow * ncol)), seed=1, stream=0)
    A = J.blockop([[J.JopDiagonal(coeff.arrays[i * ncol + k]) for k in range(ncol)] for i in range(nrow)])
    nat = _native(A)
    v = J.rand(J.domain(A), seed=2, stream=0)
    hu0 = _flat(J.rand(J.range(A), seed=3, stream=0)).copy()
    dirty = _flat(J.rand(J.domain(A), seed=4, stream=0)).copy()
    u, w = J.from_numpy(hu0, J.range(A)), J.from_numpy(dirty, J.domain(A))
    _step(nat, u, v, w, 0.5, -0.75)
    hu_ref, hw_ref = _flat(u).copy(), _flat(w).copy()
    tol = (2e-5 if np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4 else 1e-13) * np.sqrt(nrow)
    J.tune(grid_range=1)
    try:
        from jets_jl_amd._ffi import lib

        outs = []
        for _ in range(2):
            u, w = J.from_numpy(hu0, J.range(A)), J.from_numpy(dirty, J.domain(A))
            assert lib.jh_normsq_reset() == 0
            for lo, cnt in _three_ranges(dt, n):
                assert _step_range(nat, u, v, w, 0.5, -0.75, lo, cnt) == 0
                assert J.tune_get("last_grid_range_shape") & 2, "the launcher splits the rows of the range"
            total = _normsq_read()
            outs.append((_flat(u).copy(), _flat(w).copy(), total))
        assert_bits_equal(outs[0][0], hu_ref, "u does not depend on the part count")
        assert_bits_equal(outs[0][1], outs[1][1], "the ranged split walk is deterministic")
        assert np.abs(outs[0][1] - hw_ref).max() <= tol * np.abs(hw_ref).max(), "w: ranges vs the whole-vector call"
        assert outs[0][2] == pytest.approx(_normsq64(hu_ref), rel=1e-12, abs=0.0)
        # the adjoint and A'A per range, against their whole-vector calls
        _, calls = _calls(J, A)
        d = J.from_numpy(hu_ref, J.range(A))
        for name, (ranged, whole) in calls.items():
            ref, out = J.from_numpy(dirty, J.domain(A)), J.from_numpy(dirty, J.domain(A))
            x = d if name == "adjoint" else v
            assert whole(ref, x) == 0
            for lo, cnt in _three_ranges(dt, n):
                assert ranged(out, x, lo, cnt) == 0
                assert J.tune_get("last_grid_range_shape") & 2, name
            href = _flat(ref)
            assert np.abs(_flat(out) - href).max() <= tol * np.abs(href).max(), f"{name}: ranges vs the whole-vector call"
    finally:
        J.tune(grid_range=0)
    J.close(A)


def _expect_untouched(case, status, lo, cnt, what):
    """All three calls return `status` for [lo, lo + cnt) and leave u and the outputs as found."""
    for name, (ranged, _) in case.calls.items():
        out = case.dom_sentinel()
        assert ranged(out, case.d if name == "adjoint" else case.v, lo, cnt) == status, f"{what}: {name}"
        assert_bits_equal(_flat(out), case.dirty_dom, f"{what}: {name}: output untouched")
    u, w = case.u_found(case.beta), case.dom_sentinel()
    out = C.c_double(-1.0)
    assert _step_range(case.nat, u, case.v, w, case.alpha, case.beta, lo, cnt, out) == status, f"{what}: step"
    assert_bits_equal(_flat(u), case.hu0, f"{what}: u untouched")
    assert_bits_equal(_flat(w), case.dirty_dom, f"{what}: w untouched")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_bad_bounds_are_invalid_before_anything_is_touched(grid_range, oracle, dt):
    J = grid_range
    n, pe = 515, _pack(dt)
    case = Case(J, oracle, dt, 3, n, "plain")
    try:
        _expect_untouched(case, INVALID, 1, pe, "first off the 16-byte grid")
        _expect_untouched(case, INVALID, 0, pe + 1, "count off the 16-byte grid inside the block")
        _expect_untouched(case, INVALID, n // pe * pe, n % pe + pe, "beyond the block (inside the flat domain)")
        _expect_untouched(case, INVALID, n, pe, "a position of the flat domain slab, not of a block")
        _expect_untouched(case, INVALID, -pe, pe, "a negative first")
    finally:
        case.close()


def test_knob_at_zero_declines_grids_as_before(Jets, oracle):
    J = Jets
    assert J.tune_get("grid_range") == 0, "the default"
    J.tune(adj_split=0)
    try:
        case = Case(J, oracle, np.float32, 3, 4096, "plain")
        _expect_untouched(case, UNSUPPORTED, 0, 1024, "knob grid_range = 0")
        case.close()
    finally:
        J.tune(adj_split=-1)


def test_the_whole_vector_calls_knobs_hold_for_their_ranged_forms(grid_range, oracle):
    """grid_step = 0 keeps a grid from the ranged step as from jh_blockop_bidiag_step, grid_normal = 0 (and 2 on a grid of several kinds) from the
    ranged A'A as from jh_blockop_normal_mul -- status 4, outputs untouched; the ranged adjoint depends on grid_range alone."""
    J = grid_range
    case = Case(J, oracle, np.float32, 3, 515, "several")
    lo, cnt = 128, 256
    dom_in, _ = _inside(case.n, case.ncol, [(lo, cnt)])

    def declined(name):
        out = case.dom_sentinel()
        if name == "step":
            u = case.u_found(case.beta)
            st = _step_range(case.nat, u, case.v, out, case.alpha, case.beta, lo, cnt)
            if st == UNSUPPORTED:
                assert_bits_equal(_flat(u), case.hu0, "declined step: u untouched")
        else:
            st = case.calls[name][0](out, case.d if name == "adjoint" else case.v, lo, cnt)
        if st == UNSUPPORTED:
            assert_bits_equal(_flat(out), case.dirty_dom, f"declined {name}: output untouched")
        return st

    try:
        for knobs, want in ((dict(grid_step=0), {"step": UNSUPPORTED, "normal": 0, "adjoint": 0}),
                            (dict(grid_normal=0), {"step": 0, "normal": UNSUPPORTED, "adjoint": 0}),
                            (dict(grid_normal=2), {"step": 0, "normal": UNSUPPORTED, "adjoint": 0})):
            J.tune(**knobs)
            try:
                for name, st in want.items():
                    assert declined(name) == st, (knobs, name)
            finally:
                J.tune(grid_step=1, grid_normal=1)
    finally:
        case.close()
