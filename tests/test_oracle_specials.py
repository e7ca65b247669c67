"""CPU: the yardstick of tests/test_gpu_specials_fused.py.  The oracle decides what a fused kernel must give for non-finite and signed-zero data,
so its own behaviour on such data is pinned here against the reference's formulas written out in numpy on the PARTS, in the element's own
precision: a product of two complex numbers is re = ar*br - ai*bi, im = ar*bi + ai*br (Julia's base/complex.jl, no recovery of NaN); a Real
scalar multiplies part by part; a Complex scalar takes the full product even with a zero imaginary part; a block operator of several columns
accumulates `0 + ...` (src/Jets.jl:1024, 1042 / 1049), a one-column one stores; a zero block is skipped and leaves the output scalar as it was
(1022 / 1047).  Input: the special-value mix of tools/check_specials.py.  Also the seam-position generator of the GPU tests against
hand-written cases, so that an off-by-one there cannot make the GPU tests vacuous."""
import numpy as np
import pytest

from oracle import jets_oracle as jo

from .helpers import DTYPES, assert_same_values, load_tool

cs = load_tool("check_specials")
N = 6000


def _rt(dt):
    return np.float32 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64


def _mix(dt, seed, n=N):
    with np.errstate(all="ignore"):
        return cs.specials(np.random.default_rng(seed), dt, n)


def _parts(x):
    rt = _rt(x.dtype)
    return (x.real.astype(rt), x.imag.astype(rt)) if x.dtype.kind == "c" else (x.astype(rt), None)


def _join(dt, re, im):
    if im is None:
        return re.astype(dt)
    out = np.empty(re.shape, dtype=dt)
    out.real, out.imag = re, im
    return out


def _mul(a, b, conj_a=False):
    """a .* b (conj(a) .* b) by the four-multiplication formula, every operation rounded in the element's precision."""
    (ar, ai), (br, bi) = _parts(a), _parts(b)
    with np.errstate(all="ignore"):
        if ai is None:
            return ar * br
        if conj_a:
            ai = -ai
        return _join(a.dtype, ar * br - ai * bi, ar * bi + ai * br)


def _scale(a, x, conj_a=False):
    """`a * x` for a scalar of a's TYPE: a Python float is a Real (part by part), a Python complex a Complex (full product)."""
    rt = _rt(x.dtype)
    xr, xi = _parts(x)
    with np.errstate(all="ignore"):
        if not isinstance(a, complex):
            return _join(x.dtype, rt(a) * xr, None if xi is None else rt(a) * xi)
        ar, ai = rt(a.real), rt(-a.imag if conj_a else a.imag)
        return _join(x.dtype, ar * xr - ai * xi, ar * xi + ai * xr)


def _add(a, b):
    with np.errstate(all="ignore"):
        return a + b


def test_the_mix_holds_every_special_value_and_their_products():
    """The input itself: NaN, both infinities, both zeros, denormals and the largest finite values all occur, in real and imaginary parts."""
    for dt in DTYPES:
        x = _mix(dt, 1).view(_rt(dt))
        fi = np.finfo(_rt(dt))
        assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
        assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
        assert ((x != 0) & (np.abs(x) < fi.tiny)).any() and (np.abs(x) == fi.max).any()


@pytest.mark.parametrize("dt", DTYPES)
def test_child_mul_of_every_kind(dt):
    g, m = _mix(dt, 2), _mix(dt, 3)
    cplx = np.dtype(dt).kind == "c"
    dirty = lambda: np.full(N, 7, dtype=dt)                                  # noqa: E731  (a child mul! overwrites)
    assert_same_values(jo.child_mul(jo.Block("diag", N, coeff=g), dirty(), m), _mul(g, m), "diag")
    assert_same_values(jo.child_mul(jo.Block("diag", N, coeff=g, adjoint=True), dirty(), m), _mul(g, m, conj_a=True), "adjointed diag")
    assert_same_values(jo.child_mul_adj(jo.Block("diag", N, coeff=g), dirty(), m), _mul(g, m, conj_a=True), "adjoint of diag")
    assert_same_values(jo.child_mul(jo.Block("identity", N), dirty(), m), m, "identity")
    for a in (0.75, -1.25, -0.0, np.inf):
        assert_same_values(jo.child_mul(jo.Block("scale", N, scale=a), dirty(), m), _scale(a, m), f"real scale {a}")
        assert_same_values(jo.child_mul(jo.Block("scale", N, scale=a, adjoint=True), dirty(), m), _scale(a, m), f"adjointed real scale {a}")
    if cplx:
        for a in (complex(0.75, 0.0), complex(0.3, -0.25), complex(-1.25, -0.0)):
            assert_same_values(jo.child_mul(jo.Block("scale", N, scale=a), dirty(), m), _scale(a, m), f"Complex scale {a}")
            assert_same_values(jo.child_mul(jo.Block("scale", N, scale=a, adjoint=True), dirty(), m), _scale(a, m, conj_a=True), f"adjointed Complex scale {a}")
        one = _scale(complex(1.0, 0.0), m).view(_rt(dt))
        assert np.isnan(one).sum() > np.isnan(m.view(_rt(dt))).sum(), "a Complex 1 + 0im makes NaN of an infinite part; a Real 1 does not"
        assert_same_values(_scale(1.0, m), m, "a Real 1 keeps every bit")
    out = jo.child_mul(jo.Block("zero", N, N), dirty(), m)
    assert not out.view(_rt(dt)).any() and not np.signbit(out.view(_rt(dt))).any(), "a zero child writes +0, whatever m holds"


def _blocks(dt, n):
    g = [_mix(dt, 10 + k, n) for k in range(4)]
    a = complex(0.3, -0.25) if np.dtype(dt).kind == "c" else 0.3
    return g, a


@pytest.mark.parametrize("dt", DTYPES)
def test_block_df_and_its_adjoint_on_one_column(dt):
    """A one-column operator STORES each row's product (1026); a zero block is skipped, the output row untouched (1022)."""
    n = N
    g, a = _blocks(dt, n)
    ops = [[jo.Block("diag", n, coeff=g[0])], [jo.Block("zero", n, n)], [jo.Block("identity", n)], [jo.Block("scale", n, scale=a)],
           [jo.Block("diag", n, coeff=g[1], adjoint=True)]]
    m = _mix(dt, 20, n)
    d0 = [_mix(dt, 30 + i, n) for i in range(5)]
    out = jo.block_df(ops, [b.copy() for b in d0], [m])
    want = [_mul(g[0], m), d0[1], m, _scale(a, m), _mul(g[1], m, conj_a=True)]
    for i in range(5):
        assert_same_values(out[i], want[i], f"one column, row {i}")
    # the adjoint of several rows accumulates from zeros in row order: 0 + conj(g0) d0 + (skip) + d2 + conj(a) d3 + g1 d4
    d = [_mix(dt, 40 + i, n) for i in range(5)]
    got = jo.block_df_adj(ops, [_mix(dt, 50, n)], d)[0]
    acc = np.zeros(n, dtype=dt)
    for t in (_mul(g[0], d[0], conj_a=True), d[2], _scale(a, d[3], conj_a=True), _mul(g[1], d[4])):
        acc = _add(acc, t)
    assert_same_values(got, acc, "adjoint of a tall operator")
    # a single row: the adjoint stores (1051); a zero block leaves the output as found
    got = jo.block_df_adj([[jo.Block("identity", n)]], [_mix(dt, 51, n)], [d[0]])[0]
    assert_same_values(got, d[0], "adjoint of a 1 x 1 identity stores: -0 stays -0")
    keep = _mix(dt, 52, n)
    assert_same_values(jo.block_df_adj([[jo.Block("zero", n, n)]], [keep.copy()], [d[0]])[0], keep, "adjoint of a 1 x 1 zero block: untouched")


@pytest.mark.parametrize("dt", DTYPES)
def test_block_df_and_its_adjoint_on_several_columns(dt):
    """Several columns ACCUMULATE into the output as found (1024): identity is d + m (a -0 becomes +0 on zeros), zero blocks add nothing."""
    n = N
    g, a = _blocks(dt, n)
    ops = [[jo.Block("diag", n, coeff=g[0]), jo.Block("identity", n), jo.Block("zero", n, n)],
           [jo.Block("zero", n, n), jo.Block("zero", n, n), jo.Block("zero", n, n)],
           [jo.Block("scale", n, scale=a), jo.Block("diag", n, coeff=g[1], adjoint=True), jo.Block("identity", n)]]
    m = [_mix(dt, 60 + j, n) for j in range(3)]
    z = lambda: np.zeros(n, dtype=dt)                                        # noqa: E731
    out = jo.block_df(ops, [z(), z(), z()], m)
    assert_same_values(out[0], _add(_add(z(), _mul(g[0], m[0])), m[1]), "row 0: 0 + g m0 + m1")
    assert_same_values(out[1], z(), "a row of zero blocks: +0 untouched, not 0 * Inf")
    assert_same_values(out[2], _add(_add(_add(z(), _scale(a, m[0])), _mul(g[1], m[1], conj_a=True)), m[2]), "row 2")
    d0 = _mix(dt, 70, n)
    out = jo.block_df(ops, [d0.copy(), d0.copy(), d0.copy()], m)
    assert_same_values(out[1], d0, "a row of zero blocks on a dirty output: untouched")
    assert_same_values(out[0], _add(_add(d0, _mul(g[0], m[0])), m[1]), "a dirty output is added to (1024)")
    d = [_mix(dt, 80 + i, n) for i in range(3)]
    got = jo.block_df_adj(ops, [_mix(dt, 90 + j, n) for j in range(3)], d)
    assert_same_values(got[0], _add(_add(z(), _mul(g[0], d[0], conj_a=True)), _scale(a, d[2], conj_a=True)), "column 0: 0 + conj(g) d0 + conj(a) d2")
    assert_same_values(got[1], _add(_add(z(), d[0]), _mul(g[1], d[2])), "column 1: 0 + d0 + g1 d2")
    assert_same_values(got[2], _add(z(), d[2]), "column 2: 0 + d2 (a -0 of d2 becomes +0)")
    mz = np.full(n, -0.0, dtype=dt)
    got = jo.block_df_adj(ops, [z(), z(), z()], [mz, mz, mz])
    assert not np.signbit(got[2].view(_rt(dt))).any(), "0 + (-0) = +0 where rows are accumulated"


@pytest.mark.parametrize("dt", DTYPES)
def test_barr_lincomb_with_one_and_two_terms(dt):
    n = N
    x, y = [_mix(dt, 100, n), _mix(dt, 101, 37)], [_mix(dt, 102, n), _mix(dt, 103, 37)]
    empty = lambda: [np.empty(n, dtype=dt), np.empty(37, dtype=dt)]          # noqa: E731
    scal = [0.75, -1.25, -0.0] + ([complex(0.75, 0.0), complex(0.5, -2.0)] if np.dtype(dt).kind == "c" else [])
    for a in scal:
        out = jo.barr_lincomb(empty(), [a], [x])
        for k in range(2):
            assert_same_values(out[k], _scale(a, x[k]), f"one term, a = {a!r}")
        for b in scal:
            out = jo.barr_lincomb(empty(), [a, b], [x, y])
            for k in range(2):
                assert_same_values(out[k], _add(_scale(a, x[k]), _scale(b, y[k])), f"two terms, a = {a!r}, b = {b!r}")


# ---------------------------------------------------------------------------------------------------- the seam-position generator
def test_seam_positions_against_hand_written_cases():
    sp = cs.seam_positions
    assert sp("head", 1027, 4) == [0, 1, 2, 3] and sp("head", 134, 2) == [0, 1] and sp("head", 3, 4) == [0, 1, 2]
    # n = 1027 scalars, NS = 4: g = 1024; the last whole pack 1020..1023 and the tail 1024..1026 (the pack loaded from 1023 covers 1023..1026)
    assert sp("overlap", 1027, 4) == [1020, 1021, 1022, 1023, 1024, 1025, 1026]
    assert sp("overlap", 134, 4) == [128, 129, 130, 131, 132, 133]            # 67 complex64 elements: 134 scalars, g = 132
    assert sp("overlap", 3 * 4096 + 17, 2) == [12302, 12303, 12304]           # Float64, g = 12304
    assert sp("overlap", 4120, 4) == [4116, 4117, 4118, 4119]                 # on the grid: the last pack
    assert sp("tile", 2500, 4, tile=1024) == [0, 1023, 1024, 2047, 2048, 2499]
    assert sp("tile", 2048, 4, tile=1024) == [0, 1023, 1024, 2047]
    assert sp("row-ends", 67, 4) == [0, 66]
    assert sp("range-edge", 100, 4, ranges=[(12, 24), (36, 64)]) == [8, 9, 10, 11, 32, 33, 34, 35, 36, 37, 38, 39]
    assert sp("range-edge", 20, 2, ranges=[(0, 8)]) == [8, 9]
    with pytest.raises(ValueError):
        sp("nowhere", 10, 2)


def test_slab_seams_part_rows_and_ranges():
    # blocks at offsets 0, 5, 8, 12, 12, 14: the last scalars of blocks 0, 2, 4; the first of blocks 1 and 5 (block 3 is empty)
    assert cs.slab_seam_positions([5, 3, 4, 0, 2, 1], "block-last") == [4, 11, 13]
    assert cs.slab_seam_positions([5, 3, 4, 0, 2, 1], "block-first") == [5, 14]
    assert cs.slab_seam_positions([5, 3, 0], "block-last") == [4]                    # (the last block has no successor, an empty block owns nothing)
    assert cs.part_edge_rows(10, 3) == [0, 3, 4, 7, 8, 9]                            # rows per part 4: [0, 4), [4, 8), [8, 10)
    assert cs.part_edge_rows(512, 3) == [0, 170, 171, 341, 342, 511]
    assert cs.part_edge_rows(6, 6) == [0, 1, 2, 3, 4, 5]
    for dt, ns, e in ((np.float32, 4, 1), (np.float64, 2, 1), (np.complex64, 4, 2), (np.complex128, 2, 2)):
        assert cs.scalars_per_pack(dt) == ns and cs.scalars_per_elem(dt) == e
        assert cs.tile_sizes(dt) == (256 * ns, 1024 * ns, 2048 * ns)
        for n in (67, 1027, 4120, 12305):
            (lo1, c1), (lo2, c2) = cs.case_ranges(n, dt)
            al = max(1, ns // e)
            assert lo1 % al == 0 and lo2 % al == 0 and lo1 > 0 and lo1 + c1 == lo2 and lo2 + c2 == n and c1 > 0 and c2 > 0
            assert (lo1 * e) % (256 * ns) != 0 and (lo2 * e) % (256 * ns) != 0, "the ranges start on no workgroup tile"
    assert cs.case_ranges(67, np.float32) == [(12, 24), (36, 31)]


def test_poison_and_the_sources_put_the_values_where_the_positions_say():
    x = np.full(8, 1 + 1j, dtype=np.complex64)
    cs.poison(x, [1, 6, 15])
    v = x.view(np.float32)
    assert np.isnan(v[1]) and v[6] == np.inf and v[15] == 0 and np.signbit(v[15])
    assert np.array_equal(np.flatnonzero(v != 1), [1, 6, 15])
    y = np.ones(12, dtype=np.float64)
    cs.poison(y, [0, 3], row_scalars=4, rows=[0, 2])
    assert np.array_equal(np.flatnonzero(y != 1), [0, 3, 8, 11])
    for dt in DTYPES:
        e, n, nrow = cs.scalars_per_elem(dt), 67, 5
        for cls in ("head", "overlap", "tile", "row-ends", "range-edge"):
            src = cs.source_for(dt, cls, n, 3)
            pos = cs.row_positions(cls, n, dt)
            assert pos and max(pos) < n * e
            for tag, rows in ((("A", 2, 0), 1), (("w", 1), nrow), (("x", 0), 1)):
                a = src(tag, rows * n).view(_rt(dt)).reshape(rows, n * e)
                odd = ~np.isfinite(a) | ((a == 0) & np.signbit(a))
                assert np.array_equal(np.flatnonzero(odd.any(axis=0)), pos), (cls, tag)
                assert odd[:, pos].all(), "every row of a slab is poisoned at every position"
                assert ((a >= 0) & (a < 1))[~odd].all()
        for cls in cs.STEP_CLASSES:                      # +Inf alone, real parts alone, in one array: the coefficients (real types) or the old u (complex)
            src = cs.source_for(dt, cls, n, 3)
            hot = ("A", 1, 0) if e == 1 else ("u", 0)
            a = src(hot, n if e == 1 else nrow * n).view(_rt(dt)).reshape(-1, n * e)
            want = [q for q in cs.row_positions(cls.split(",")[0], n, dt) if q % e == 0]
            assert want and all(np.array_equal(np.flatnonzero(row == np.inf), want) and np.isfinite(np.delete(row, want)).all() for row in a)
            cold = [("w", 0), ("v", 0), ("c", 1), ("u", 0) if e == 1 else ("A", 1, 0)]
            assert all(np.isfinite(src(tag, nrow * n).view(_rt(dt))).all() for tag in cold)
        assert cs.inf_only_verdict(dt, "overlap", -0.5, np.array([np.inf], dtype=dt)) is None
        assert cs.inf_only_verdict(dt, cs.STEP_CLASSES[0], -0.5, np.array([1, np.inf], dtype=dt)) is True
        assert cs.inf_only_verdict(dt, cs.STEP_CLASSES[0], -0.5, np.array([np.nan, np.inf], dtype=dt)) is not True
        assert cs.inf_only_verdict(dt, cs.STEP_CLASSES[0], -0.5, np.array([1, 2], dtype=dt)) is not True
        assert (cs.inf_only_verdict(dt, cs.STEP_CLASSES[0], 0.0, np.array([1, 2], dtype=dt)) is None) == (e == 2)
        src = cs.Source(dt, "part-rows", 3, positions=[1, n * e - 1], row_scalars=n * e, rows=[0, 4])
        w = src(("w", 0), nrow * n).view(_rt(dt)).reshape(nrow, n * e)
        assert np.array_equal(np.flatnonzero((~np.isfinite(w) | ((w == 0) & np.signbit(w))).any(axis=1)), [0, 4])
        assert np.isfinite(src(("A", 2, 0), n).view(_rt(dt))).all() and not np.isfinite(src(("A", 4, 0), n).view(_rt(dt))).all()
        free = cs.Source(dt, "order-free", 3)(("x", 0), 5000).view(_rt(dt))
        assert np.abs(free[np.isfinite(free)]).max() <= 1.0, "the split walk's pool holds no +-max"


def test_the_column_source_gives_every_special_value_columns_of_its_own():
    """The split walk's input: summed over all rows, a column holds ONE kind of special value, so clean infinities and finite sums survive."""
    n, nrow, rows = 259, 40, [0, 13, 14, 27, 28, 39]
    for dt in DTYPES:
        rt, e = _rt(dt), cs.scalars_per_elem(dt)
        src = cs.ColumnSource(dt, 3, n, rows, ("w", "u"))
        for t, tag in enumerate((("w", 0), ("u", 0))):
            w = src(tag, nrow * n).reshape(nrow, n)
            re, im = (w.real, w.imag) if e == 2 else (w, np.zeros_like(w))
            assert np.isfinite(im).all() and np.array_equal(np.flatnonzero((~np.isfinite(re)).any(axis=1)), rows)
            for b in range(-(-n // 16)):
                cols = re[:, 16 * b:16 * b + 16]
                if b % 2 != t:
                    assert ((cols >= 0) & (cols < 1) & ~np.signbit(cols)).all(), "the other tag's block is clean"
                    continue
                owner = rows[(b // 2) % len(rows)]
                if cols.shape[1] < 16:                                        # the ragged last block: its first columns only
                    assert np.isnan(cols[owner, 0]) and cols.shape[1] == n % 16
                    continue
                assert np.isnan(cols[owner, 0]) and cols[owner, 1] == np.inf and cols[owner, 2] == -np.inf
                assert cols[owner, 3] == 0 and np.signbit(cols[owner, 3]) and 0 < cols[owner, 4] < np.finfo(rt).tiny
                assert (cols[owner, 5], cols[owner, 6], cols[owner, 7]) == (1, -1, 0)
                others = np.delete(cols[:, :8], owner, axis=0)
                assert ((others >= 0) & (others < 1)).all(), "columns 0 .. 7 are special in the owning row only"
                if 16 * b + 10 < n:
                    assert (cols[rows, 9] == np.inf).all() and cols[rows[0], 10] == np.inf and cols[rows[-1], 10] == -np.inf
                    assert np.isfinite(np.delete(cols[:, 9:11], rows, axis=0)).all() and np.isfinite(cols[rows[1:-1], 10]).all()
                with np.errstate(all="ignore"):
                    tot = cols.sum(axis=0)                                    # what a sum over the rows keeps
                assert np.isnan(tot[0]) and tot[1] == np.inf and tot[2] == -np.inf and np.isfinite(tot[3:8]).all()
                if 16 * b + 10 < n:
                    assert tot[9] == np.inf and np.isnan(tot[10]) and np.isfinite(tot[11:]).all()
        assert np.isfinite(src(("x", 0), n).view(rt)).all() and np.isfinite(src(("A", 13, 0), n).view(rt)).all()
        a = cs.ColumnSource(dt, 3, n, rows, ("A",))
        assert not np.isfinite(a(("A", 13, 2), n).view(rt)).all() and np.isfinite(a(("A", 12, 0), n).view(rt)).all()
    pv = cs.population_verdict
    mixed = np.concatenate([np.ones(30), np.full(25, np.inf), np.full(20, np.nan)])
    assert pv(mixed, True) is True and pv(np.full(100, np.nan), False) is not True and pv(mixed[:50], True) is not True
    assert pv(np.concatenate([np.ones(30), np.full(20, np.nan)]), False) is True and pv(np.concatenate([np.ones(30), np.full(20, np.nan)]), True) is not True


def test_expected_reductions_follow_the_rule():
    assert np.isnan(cs.expect_normsq(np.array([1.0, np.nan, np.inf]))) and cs.expect_normsq(np.array([1.0, -np.inf])) == np.inf
    assert cs.expect_normsq(np.array([3.0, 4.0], dtype=np.float32)) == 25.0 and cs.expect_normsq(np.array([3 + 4j], dtype=np.complex64)) == 25.0
    assert cs.normsq_verdict(float("nan"), np.array([np.nan])) is True and cs.normsq_verdict(1.0, np.array([np.nan])) is not True
    assert cs.normsq_verdict(25.0 * (1 + 1e-13), np.array([3.0, 4.0])) is True and cs.normsq_verdict(25.0 * (1 + 1e-11), np.array([3.0, 4.0])) is not True
    assert cs.normsq_verdict(float("nan"), np.array([3.0, 4.0])) is not True and cs.normsq_verdict(float("inf"), np.array([3.0, 4.0])) is not True
    a, b = np.array([1.0, np.nan, np.inf, 2.0]), np.array([1.0, np.nan, -np.inf, 2.0])
    ok = lambda g, w: True                                                   # noqa: E731
    assert cs.masks_verdict(a, a.copy(), ok) is True and cs.masks_verdict(a, b, ok) is not True
    assert cs.masks_verdict(np.array([1.0, 2.0]), np.array([1.0, np.nan]), ok) is not True
    assert cs.order_free_verdict(a, b) is True and cs.order_free_verdict(a, np.array([1.0, 2.0, np.inf, 2.0])) is not True
    acc = cs.accumulated
    base, t = np.array([-0.0, 1.0], dtype=np.float32), np.array([-0.0, 2.0], dtype=np.float32)
    assert np.signbit(acc(0, base, t)[0]) and np.signbit(acc(1, base, t)[0]) and not np.signbit(acc(2, base, t)[0]) and not np.signbit(acc(-2, base, t)[0])
    assert acc(-1, base, t)[1] == -1.0 and acc(-2, base, t)[1] == -2.0


def test_the_case_list_names_family_chain_dtype_and_class():
    cases = cs.fused_cases()
    ids = [c[0] for c in cases]
    assert len(set(ids)) == len(ids)
    for fam in ("tall chain", "tall composite", "chain step", "grid A'A", "grid chain", "grid step", "block reductions", "split walk", "big blocks"):
        assert any(i.startswith(fam + " | ") for i in ids), fam
    assert all(len(i.split(" | ")) == 4 for i in ids)
    assert cs.adjoint_tokens(["A", ("W", 0, False), ("s", 0.75, "r")]) == [("s", 0.75, "r"), ("W", 0, True), "At"]
