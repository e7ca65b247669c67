"""GPU: every function of the compiled broadcast (jh_bcast.hip, jets.jl_amd/broadcast.py, julia/JetsHIP.jl) against a 50-digit reference,
over its whole domain, with Julia's semantics at the edges.

ACCURACY (tests/golden/bcast_functions.npz, written by tests/golden/make_bcast_functions.py with mpmath): where the reference, rounded to the
element type, is a NORMAL number the result is judged by its relative error alone -- the bar of tests/test_gpu_broadcast.py, 2e-6 (Float32) /
1e-14 (Float64), no atol.  Where it is zero, Inf or NaN the result has that class and sign; where it is subnormal the result has its sign and
is within bar x (smallest normal) of it.  The measured worst case per (function, type), in ulps and with its argument, next to what numpy gets
in the same type on the CPU, is the record profiles/bcast_function_errors.txt (written on first contact with a device, or wherever the
environment variable JETS_BCAST_ERRORS says); the record is not the source of the bar.

BIT FOR BIT: + - * / sqrt floor ceil abs abs2 conj real imag sign max min, subnormal operands and results included; max / min / sign with
Julia's results for NaN and signed zeros.  COMPLEX: z / w, a / w, z / a and abs over magnitudes 2^+-(emax - 2), normwise within 1e-6 / 1e-14
of |z / w|; exp(z) through the overflow threshold with im = +-0.  One mixed expression through the 16-byte kernel (on and off the 16-byte
grid), the one-element-per-lane kernel and the batched kernel under its knobs: the same bits.  Tails, aliasing and sentinels for all four
types; JopElementwise consumers alone and as children of a tall operator.
"""
import math
import os

import numpy as np
import pytest

from .helpers import assert_same_values

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = {np.dtype(np.float32): 2e-6, np.dtype(np.float64): 1e-14}
CBAR = {np.dtype(np.complex64): 1e-6, np.dtype(np.complex128): 1e-14}
TYPES = {"f32": np.float32, "f64": np.float64}
UNARY = ["exp", "exp2", "log", "log2", "log10", "sin", "cos", "tan", "tanh", "sinh", "cosh", "asin", "acos", "atan", "erf"]
BINARY = ["atan2", "hypot", "pow"]
# (function, type, (lowest x0, highest x0)): a subrange where a function misses the bar and the fix is not finished.  At most three; each with
# its measured error in profiles/bcast_function_errors.txt and README.md.
KNOWN_GAPS = []

_erf = np.vectorize(math.erf, otypes=[np.float64])
NUMPY = {"exp": np.exp, "exp2": np.exp2, "log": np.log, "log2": np.log2, "log10": np.log10, "sin": np.sin, "cos": np.cos, "tan": np.tan, "tanh": np.tanh,
         "sinh": np.sinh, "cosh": np.cosh, "asin": np.arcsin, "acos": np.arccos, "atan": np.arctan, "atan2": np.arctan2, "hypot": np.hypot, "pow": np.power,
         "erf": lambda x: _erf(x.astype(np.float64)).astype(x.dtype)}      # (numpy has no erf: the C library's, in double, rounded to the type)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "bcast_functions.npz"))
    return {k: z[k] for k in z.files}


_record = {}


@pytest.fixture(scope="module", autouse=True)
def error_record():
    """Collects the accuracy tests' worst cases and writes the record when the module is done."""
    yield _record
    path = os.environ.get("JETS_BCAST_ERRORS") or os.path.join(ROOT, "profiles", "bcast_function_errors.txt")
    if not _record or (os.path.exists(path) and not os.environ.get("JETS_BCAST_ERRORS")):
        return
    lines = ["Compiled broadcast: worst error per (function, type) over the points of tests/golden/bcast_functions.npz, in ulps of the element type",
             "(reference: mpmath at 50 digits; subnormal references count in units of the smallest subnormal).  `numpy` is the same function in the same",
             "type on the CPU of the machine that ran the test.  bar: 2e-6 = 16.8 ulp (f32), 1e-14 = 45 ulp (f64) relative.  class = results whose class",
             "or sign (zero / Inf / NaN) differs from the correctly rounded reference's.  Written by tests/test_gpu_broadcast_functions.py.", "",
             f"{'function':<9}{'type':<5}{'points':>7}{'device ulp':>12}  {'at':<36}{'worst rel':>10}{'class':>6}{'numpy ulp':>11}  {'at':<36}{'class':>6}"]
    for (fn, ty), r in sorted(_record.items()):
        lines.append(f"{fn:<9}{ty:<5}{r['n']:>7}{r['dev'][0]:>12.3f}  {r['dev'][1]:<36}{r['rel']:>10.2e}{r['dev_class']:>6}{r['np'][0]:>11.3f}  {r['np'][1]:<36}{r['np_class']:>6}")
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


def _run(J, expr, dt, ops, scalars=()):
    vecs = [J.from_numpy(np.ascontiguousarray(o, dtype=o.dtype)) for o in ops]
    out = J.zeros(J.JetSpace(dt, len(ops[0])))
    J.broadcast_(out, expr, vecs, list(scalars))
    return out.to_numpy()


def judge(got, hi, lo, dt):
    """got (element type dt) against the double-double reference (hi, lo): (ok, class_ok, rel, ulps) per point, as the module docstring sets out."""
    dt = np.dtype(dt)
    fi = np.finfo(dt)
    tiny, sub = float(fi.tiny), float(fi.smallest_subnormal)
    g = got.astype(np.float64)
    with np.errstate(all="ignore"):
        ref = hi.astype(dt).astype(np.float64)               # the correctly rounded reference: its class and sign
        normal = np.isfinite(ref) & (np.abs(ref) >= tiny)
        subn = (ref != 0) & (np.abs(ref) < tiny)
        err = np.abs((g - hi) - lo)                          # g - hi is exact where they are close; far apart the rounding does not matter
        rel = np.where(normal, err / np.abs(hi), 0.0)
        rel = np.where(normal & ~np.isfinite(g), np.inf, rel)
        ulp = np.where(normal, np.spacing(np.abs(ref).astype(dt)).astype(np.float64), sub)
        ulps = np.where(normal | subn, err / ulp, 0.0)
        ulps = np.where((normal | subn) & ~np.isfinite(g), np.inf, ulps)
        same_sign = np.signbit(g) == np.signbit(ref)
        class_ok = np.where(np.isnan(ref), np.isnan(g), np.where(np.isinf(ref), g == ref, np.where(ref == 0, (g == 0) & same_sign, True)))
        ok = np.where(normal, rel <= BAR[dt], np.where(subn, same_sign & np.isfinite(g) & (err <= BAR[dt] * tiny), class_ok))
    return ok, class_ok, rel, ulps


def _worst(ulps, ops):
    k = int(np.argmax(ulps))
    return float(ulps[k]), ", ".join(f"{float(o[k])!r}" for o in ops)


@pytest.mark.parametrize("ty", list(TYPES))
@pytest.mark.parametrize("fn", UNARY + BINARY)
def test_function_meets_the_bar_over_its_domain(Jets, golden, error_record, fn, ty):
    dt = TYPES[ty]
    ops64 = [golden[f"{fn}/{ty}/x{k}"] for k in range(2 if fn in BINARY else 1)]
    hi = golden[f"{fn}/{ty}/hi"]
    lo = golden[f"{fn}/{ty}/lo"] if ty == "f64" else np.zeros_like(hi)
    ops = [o.astype(dt) for o in ops64]
    assert all(np.array_equal(o.astype(np.float64), o64, equal_nan=True) for o, o64 in zip(ops, ops64))
    got = _run(Jets, f"{fn}({', '.join(f'x{k}' for k in range(len(ops)))})", dt, ops)
    ok, class_ok, rel, ulps = judge(got, hi, lo, dt)
    with np.errstate(all="ignore"):
        host = NUMPY[fn](*ops).astype(dt)
    _, np_class_ok, _, np_ulps = judge(host, hi, lo, dt)
    error_record[(fn, ty)] = {"n": len(hi), "dev": _worst(ulps, ops64), "rel": float(rel.max()), "dev_class": int((~class_ok).sum()),
                              "np": _worst(np_ulps, ops64), "np_class": int((~np_class_ok).sum())}
    print(f"{fn}/{ty}: device worst {error_record[(fn, ty)]['dev']} ulp, rel {rel.max():.3e}, class mismatches {int((~class_ok).sum())}; numpy {error_record[(fn, ty)]['np']}")
    for gfn, gty, (a, b) in KNOWN_GAPS:
        if (gfn, gty) == (fn, ty):
            ok = ok | ((ops64[0] >= a) & (ops64[0] <= b))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (f"{fn}/{ty}: {bad.size} of {len(hi)} points miss the bar {BAR[np.dtype(dt)]:g}; first: " +
                           "; ".join(f"{fn}({', '.join(repr(float(o[k])) for o in ops64)}) = {got[k]!r}, reference {hi[k]!r} (rel {rel[k]:.3e})" for k in bad[:6]))


def test_known_gaps_stay_within_their_cap():
    assert len(KNOWN_GAPS) <= 3
    assert all(fn in UNARY + BINARY and ty in TYPES and a <= b for fn, ty, (a, b) in KNOWN_GAPS)


@pytest.mark.parametrize("ty", list(TYPES))
def test_exp2_of_every_integer_argument(Jets, ty):
    """exp2(k) for ALL integers from below the smallest subnormal to above the overflow threshold (the fixture holds a stride of them for f64):
    the reference is the exact power of two -- 0 below 2^(emin - 1), Inf from 2^(emax + 1)."""
    dt = TYPES[ty]
    fi = np.finfo(dt)
    k = np.arange(int(np.log2(float(fi.smallest_subnormal))) - 3, int(fi.maxexp) + 3).astype(np.float64)
    with np.errstate(over="ignore"):
        hi = np.ldexp(1.0, k.astype(int))
        hi[k <= np.log2(float(fi.smallest_subnormal)) - 1] = 0.0         # (at emin - 1 the tie goes to the even neighbour: zero, too)
    got = _run(Jets, "exp2(x0)", dt, [k.astype(dt)])
    ok, _, rel, _ = judge(got, hi, np.zeros_like(hi), dt)
    assert ok.all(), f"exp2/{ty}: wrong at integer arguments {k[~ok][:8]}: {got[~ok][:8]}"


@pytest.mark.parametrize("ty", list(TYPES))
def test_pow_with_a_scalar_exponent_is_pow_with_a_vector_exponent(Jets, golden, ty):
    """pow(x0, s0) -- what symmetric.py and JopElementwise write -- gives the bits of pow(x0, x1) (which the accuracy test judges), exponent by exponent."""
    dt = TYPES[ty]
    b, y = golden[f"pow/{ty}/x0"].astype(dt), golden[f"pow/{ty}/x1"].astype(dt)
    want = _run(Jets, "pow(x0, x1)", dt, [b, y])
    for e in np.unique(y):
        sel = y == e
        got = _run(Jets, "pow(x0, s0)", dt, [b[sel]], [dt(e)])
        assert_same_values(got, want[sel], f"pow(x0, {e!r})")


# ---------------------------------------------------------------------------------------------------------------- bit for bit
def _range_values(dt, n, seed):
    """Special values and n values log-uniform over the whole range of dt (subnormals included), both signs."""
    fi = np.finfo(dt)
    big = 2.0 ** fi.nmant
    special = [0.0, -0.0, float(fi.smallest_subnormal), -float(fi.smallest_subnormal), float(fi.tiny) * (1 - float(fi.eps)), -float(fi.tiny) / 2, float(fi.tiny),
               -float(fi.tiny), float(fi.max), -float(fi.max), np.inf, -np.inf, np.nan, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.5, -2.5, 0.49999997, -0.9999999, big, -big,
               big + 1, big / 2 + 0.5, -(big / 2 + 0.5), big * 2 + 2, 3.0, 1e-5, float(fi.eps)]
    rs = np.random.RandomState(seed)
    e = rs.uniform(np.log2(float(fi.smallest_subnormal)), fi.maxexp, n)
    with np.errstate(over="ignore"):
        rnd = (np.exp2(e) * rs.choice([-1.0, 1.0], n)).astype(dt)
        rnd[~np.isfinite(rnd)] = dt(1.25)
    return np.array(special, dtype=dt), rnd


def _jl_max(x, y):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x) | np.isnan(y), x.dtype.type(np.nan), np.where(x > y, x, np.where(y > x, y, np.where(np.signbit(x), y, x))))


def _jl_min(x, y):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x) | np.isnan(y), x.dtype.type(np.nan), np.where(x < y, x, np.where(y < x, y, np.where(np.signbit(x), x, y))))


def _jl_sign(x):
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x.dtype.type(1), np.where(x < 0, x.dtype.type(-1), x))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_arithmetic_rounding_and_selection_are_bit_exact_over_the_whole_range(Jets, dt):
    """+ - * / sqrt floor ceil abs abs2 conj real imag sign max min against numpy's IEEE operations in the same type: every pair of special values
    (signed zeros, subnormals, the largest finite value, infinities, NaN, -0.5, values >= 2^23 / 2^52) and 4000 random pairs over the whole
    exponent range, subnormal operands and results included.  A NaN matches any NaN; everything else bit for bit."""
    sp, rnd = _range_values(dt, 4000, 3)
    x = np.concatenate([np.repeat(sp, len(sp)), rnd])
    y = np.concatenate([np.tile(sp, len(sp)), np.roll(rnd, 1) * dt(0.75)])
    # operands of comparable size too: sums and differences that cancel, quotients near 1, products in range
    x = np.concatenate([x, rnd])
    with np.errstate(all="ignore"):
        y = np.concatenate([y, (rnd * np.random.RandomState(4).uniform(0.5, 2.0, len(rnd)).astype(dt)).astype(dt)])
    vx, vy = Jets.from_numpy(x), Jets.from_numpy(y)
    out = Jets.zeros(Jets.JetSpace(dt, len(x)))
    with np.errstate(all="ignore"):
        cases = {"x0 + x1": x + y, "x0 - x1": x - y, "x0 * x1": x * y, "x0 / x1": x / y, "sqrt(abs(x0))": np.sqrt(np.abs(x)), "floor(x0)": np.floor(x),
                 "ceil(x0)": np.ceil(x), "abs(x0)": np.abs(x), "abs2(x0)": x * x, "conj(x0)": x, "real(x0)": x, "imag(x0) + x1": dt(0) + y, "sign(x0)": _jl_sign(x),
                 "jl_max(x0, x1)": _jl_max(x, y), "jl_min(x0, x1)": _jl_min(x, y), "jl_max(x0, s0)": _jl_max(x, np.full_like(x, 0.0)), "jl_min(x0, s0)": _jl_min(x, np.full_like(x, 0.0))}
    for expr, want in cases.items():
        Jets.broadcast_(out, expr, [vx, vy], [0.0])
        assert_same_values(out.to_numpy(), want.astype(dt), expr)
    # the lazy spelling emits the same functions
    L = Jets.lazy
    Jets.assign_(out, Jets.bc.maximum(L(vx), L(vy)) + Jets.bc.sign(L(vx)) * 0)
    with np.errstate(all="ignore"):
        assert_same_values(out.to_numpy(), (_jl_max(x, y) + _jl_sign(x) * dt(0)).astype(dt), "bc.maximum + bc.sign")
    Jets.assign_(out, Jets.bc.minimum(L(vx), L(vy)))
    assert_same_values(out.to_numpy(), _jl_min(x, y).astype(dt), "bc.minimum")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_max_min_sign_give_julias_results(Jets, dt):
    """The table of the issue, value by value: max / min propagate NaN from either side, order signed zeros; sign keeps NaN and signed zeros."""
    T = dt
    nan, inf = T(np.nan), T(np.inf)
    x = np.array([nan, 2.0, nan, -3.0, -0.0, 0.0, 0.0, -0.0, nan, inf, -inf, nan], dtype=dt)
    y = np.array([2.0, nan, -inf, nan, 0.0, -0.0, -0.0, 0.0, nan, nan, nan, inf], dtype=dt)
    mx = _run(Jets, "jl_max(x0, x1)", dt, [x, y])
    mn = _run(Jets, "jl_min(x0, x1)", dt, [x, y])
    for k in (0, 1, 2, 3, 8, 9, 10, 11):
        assert np.isnan(mx[k]) and np.isnan(mn[k]), f"max / min({x[k]}, {y[k]}) = {mx[k]} / {mn[k]}: Julia gives NaN"
    for k in (4, 5, 6, 7):
        assert mx[k] == 0 and not np.signbit(mx[k]), f"max({x[k]}, {y[k]}) = {mx[k]}: Julia gives 0.0"
        assert mn[k] == 0 and np.signbit(mn[k]), f"min({x[k]}, {y[k]}) = {mn[k]}: Julia gives -0.0"
    s_in = np.array([nan, 0.0, -0.0, inf, -inf, 5e-324 if dt == np.float64 else 1e-45, -2.5], dtype=dt)
    s = _run(Jets, "sign(x0)", dt, [s_in])
    assert np.isnan(s[0]), f"sign(NaN) = {s[0]}: Julia gives NaN"
    assert s[1] == 0 and not np.signbit(s[1]) and s[2] == 0 and np.signbit(s[2]), f"sign(+-0.0) = {s[1]}, {s[2]}: Julia gives 0.0, -0.0"
    assert list(s[3:]) == [1, -1, 1, -1]
    # a clamp written with maximum keeps a NaN of the model vector
    L = Jets.lazy
    m = Jets.from_numpy(np.array([0.25, nan, 0.75, -1.0], dtype=dt))
    c = Jets.assign_(Jets.zeros(Jets.JetSpace(dt, 4)), Jets.bc.minimum(Jets.bc.maximum(L(m), 0.5), 0.7)).to_numpy()
    assert c[0] == T(0.5) and np.isnan(c[1]) and c[2] == T(0.7) and c[3] == T(0.5), f"clamp = {c}"


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_complex_parts_and_abs2_are_bit_exact(Jets, dt):
    rdt = np.float32 if dt == np.complex64 else np.float64
    sp, rnd = _range_values(rdt, 3000, 5)
    re = np.concatenate([np.repeat(sp, len(sp)), rnd])
    im = np.concatenate([np.tile(sp, len(sp)), np.roll(rnd, 7)])
    z = np.empty(len(re), dtype=dt)
    z.real, z.imag = re, im
    vz = Jets.from_numpy(z)
    out = Jets.zeros(Jets.JetSpace(dt, len(z)))

    def cplx(a, b):
        o = np.empty(len(a), dtype=dt)
        o.real, o.imag = a, b
        return o

    zero = np.zeros(len(re), dtype=rdt)
    with np.errstate(all="ignore"):
        cases = {"conj(x0)": cplx(re, -im), "real(x0)": cplx(re, zero), "imag(x0)": cplx(im, zero), "abs2(x0)": cplx(re * re + im * im, zero), "-x0": cplx(-re, -im)}
    for expr, want in cases.items():
        Jets.broadcast_(out, expr, [vz])
        assert_same_values(out.to_numpy(), want, expr)


# ---------------------------------------------------------------------------------------------------------------- complex
def _wide(z):
    """Complex operands as (re, im) in a type with more range and precision than the element type's SQUARES need: complex64 -> float64 parts
    (|z|^2 <= 2^252), complex128 -> x87 long double parts (64-bit significand, 15-bit exponent)."""
    W = np.float64 if z.dtype == np.complex64 else np.longdouble
    assert z.dtype == np.complex64 or (np.finfo(np.longdouble).nmant >= 63 and np.finfo(np.longdouble).maxexp >= 16384)
    return z.real.astype(W), z.imag.astype(W)


def _wide_div(z, w):
    (a, b), (c, d) = _wide(z), _wide(w)
    den = c * c + d * d
    return (a * c + b * d) / den, (b * c - a * d) / den


def _magnitudes(dt, n, seed):
    """n complex values with |z| log-uniform over 2^+-(emax - 2) and any argument; every fifth with re and im 30 orders of magnitude apart."""
    rdt = np.float32 if dt == np.complex64 else np.float64
    emax = np.finfo(rdt).maxexp - 1
    rs = np.random.RandomState(seed)
    mag = np.exp2(rs.uniform(-(emax - 2), emax - 2, n))
    th = rs.uniform(0, 2 * np.pi, n)
    re, im = mag * np.cos(th), mag * np.sin(th)
    k = np.arange(n)
    im = np.where(k % 5 == 0, im * 1e-30, im)
    re = np.where(k % 5 == 1, re * 1e-30, re)
    z = np.empty(n, dtype=dt)
    z.real, z.imag = re.astype(rdt), im.astype(rdt)
    return z


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_complex_division_and_abs_over_the_whole_exponent_range(Jets, dt):
    """z / w, a / w, z / a and abs(z) with |z| and |w| log-uniform over 2^+-(emax - 2): equal huge and equal tiny operands, parts 30 orders apart,
    the two examples of the issue.  Only pairs whose true quotient is a normal number count; the error is normwise, relative to |z / w|."""
    rdt = np.float32 if dt == np.complex64 else np.float64
    fi = np.finfo(rdt)
    n = 3000
    z, w = _magnitudes(dt, n, 11), _magnitudes(dt, n, 12)
    w[:200] = z[:200]                                                      # equal operands, huge and tiny ones among them
    big, small = rdt(2.0) ** (fi.maxexp - 3), rdt(2.0) ** -(fi.maxexp - 3)
    ex = [(1e20 + 1e20j, 1e20 + 1e20j), (1 + 1j, 1e-25 + 1e-25j), (big * (1 + 1j), big * (1 + 1j)), (small * (1 - 1j), small * (1 - 1j)), (1e30 + 1j, 1e-5 + 1e-35j),
          (1e-30 + 1e-30j, 1e-8 - 1e-38j)] if dt == np.complex64 else \
         [(1e200 + 1e200j, 1e200 + 1e200j), (1 + 1j, 1e-200 + 1e-200j), (big * (1 + 1j), big * (1 + 1j)), (small * (1 - 1j), small * (1 - 1j)), (1e300 + 1e270j, 1e-5 + 1e-35j),
          (1e-300 + 1e-300j, 1e-160 - 1e-190j)]
    for k, (a, b) in enumerate(ex):
        z[200 + k], w[200 + k] = dt(a), dt(b)
    a = np.abs(_magnitudes(dt, n, 13).real).astype(rdt) + fi.tiny           # a real operand, same magnitudes
    vz, vw, va = Jets.from_numpy(z), Jets.from_numpy(w), Jets.from_numpy(a)
    out = Jets.zeros(Jets.JetSpace(dt, n))
    W = np.float64 if dt == np.complex64 else np.longdouble
    az = z.copy()
    az.real, az.imag = a, 0
    cases = {"x0 / x1": ([vz, vw], _wide_div(z, w)), "x2 / x1": ([vz, vw, va], _wide_div(az, w)), "x0 / x2": ([vz, vw, va], (z.real.astype(W) / a.astype(W), z.imag.astype(W) / a.astype(W)))}
    for expr, (vecs, (qr, qi)) in cases.items():
        Jets.broadcast_(out, expr, vecs)
        got = out.to_numpy()
        aq = np.hypot(qr, qi)
        use = (aq >= W(fi.tiny)) & (aq <= W(fi.max))
        assert use.sum() > n // 3 and (expr != "x0 / x1" or use[:206].all())
        err = np.hypot(got.real.astype(W) - qr, got.imag.astype(W) - qi) / np.where(use, aq, 1)
        err = np.where(np.isfinite(got.real) & np.isfinite(got.imag), err, np.inf)[use]
        k = int(np.argmax(err))
        print(f"{np.dtype(dt).name} {expr}: worst normwise error {float(err[k]):.3e} over {int(use.sum())} pairs")
        bad = np.flatnonzero(use)[err > CBAR[np.dtype(dt)]]
        assert bad.size == 0, f"{expr}: {bad.size} quotients off by more than {CBAR[np.dtype(dt)]:g}; first: " + "; ".join(f"({z[i]}) / ({w[i]}) [a = {a[i]}] = {got[i]}" for i in bad[:4])
    # a real SCALAR over a complex vector, and the vector over it
    Jets.broadcast_(out, "s0 / x0", [vw], [3.0])
    qr, qi = _wide_div(np.full(n, 3.0, dtype=dt), w)
    aq = np.hypot(qr, qi)
    use = (aq >= W(fi.tiny)) & (aq <= W(fi.max))
    got = out.to_numpy()
    assert np.all(np.hypot(got.real.astype(W) - qr, got.imag.astype(W) - qi)[use] <= CBAR[np.dtype(dt)] * aq[use]), "s0 / x0"
    Jets.broadcast_(out, "abs(x0)", [vz])
    zr, zi = _wide(z)
    want = np.sqrt(zr * zr + zi * zi)
    got = out.to_numpy()
    assert not got.imag.any()
    assert np.all(np.abs(got.real.astype(W) - want) <= BAR[np.dtype(rdt)] * want), "abs(z) over the whole exponent range"


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_complex_exp_through_the_overflow_threshold(Jets, dt):
    """exp(z) is Julia's: complex(exp(re), im) when im is +-0 -- also where exp(re) overflows (no Inf * 0 = NaN) and for re = +-Inf --, else
    exp(re) * (cos(im), sin(im)).  Where exp(re) is finite and |exp(z)| normal the result is within the complex bar normwise (reference: the same
    formula in long double); where exp(re) overflows the element type, each part is Inf with the sign of cos(im) / sin(im), as Inf * cos(im) is."""
    rdt = np.float32 if dt == np.complex64 else np.float64
    fi = np.finfo(rdt)
    over = [89.0, 100.0, 1e4] if rdt == np.float32 else [710.0, 800.0, 1e5]
    under = [-10.0, 0.5, 30.0, 80.0, 88.0] if rdt == np.float32 else [-10.0, 0.5, 80.0, 700.0, 709.5]
    hp = rdt(np.pi / 2)
    ims = [0.0, -0.0, 1e-30, -1e-30, hp, np.nextafter(hp, rdt(2)), np.nextafter(hp, rdt(1)), -hp, 1e5, -1e5, 1.0]
    re = np.repeat(np.array(under + over + [np.inf, -np.inf], dtype=rdt), len(ims))
    im = np.tile(np.array(ims, dtype=rdt), len(under) + len(over) + 2)
    keep = np.isfinite(re) | (im == 0)                       # exp(complex(+-Inf, 0.0)) only
    re, im = re[keep], im[keep]
    z = np.empty(len(re), dtype=dt)
    z.real, z.imag = re, im
    got = _run(Jets, "exp(x0)", dt, [z])
    L = np.longdouble
    with np.errstate(all="ignore"):
        e = np.exp(re.astype(L))
        finite = e <= L(fi.max)
        wr, wi = e * np.cos(im.astype(L)), e * np.sin(im.astype(L))
    for k in range(len(z)):
        what = f"exp({re[k]!r} + {im[k]!r}im) = {got[k]!r}"
        if im[k] == 0:
            assert got.imag[k] == 0 and np.signbit(got.imag[k]) == np.signbit(im[k]), what + ": the imaginary part is the argument's zero"
            if finite[k]:
                assert abs(L(got.real[k]) - e[k]) <= BAR[np.dtype(rdt)] * e[k], what
            else:
                assert got.real[k] == np.inf, what
        elif finite[k]:
            assert np.hypot(L(got.real[k]) - wr[k], L(got.imag[k]) - wi[k]) <= CBAR[np.dtype(dt)] * e[k], what
        else:
            assert np.isinf(got.real[k]) and np.isinf(got.imag[k]) and np.signbit(got.real[k]) == np.signbit(wr[k]) and np.signbit(got.imag[k]) == np.signbit(wi[k]), what


# ---------------------------------------------------------------------------------------------------------------- one expression, three kernels
def _mixed(dt, n, seed):
    rs = np.random.RandomState(seed)
    if np.dtype(dt).kind == "c":
        x = (rs.standard_normal(n) + 1j * rs.standard_normal(n)).astype(dt)
        y = (rs.standard_normal(n) - 1j * rs.standard_normal(n)).astype(dt)
        return "exp(x0) * abs2(x1) + x0 / x1 - conj(x1) * s0 + abs(x0)", x, y, [0.5 - 0.25j]
    x, y = (rs.standard_normal(n) * 3).astype(dt), (rs.standard_normal(n) * 3).astype(dt)
    x[::17], y[::19], x[5], y[5], x[6], y[6] = 0.0, np.nan, -0.0, 0.0, np.inf, -np.inf
    return "pow(abs(x0), s0) * tanh(x1) + jl_max(x0, x1)", x, y, [1.7]


def _ns_e(dt):
    """(scalars per 16-byte pack, scalars per element)."""
    dt = np.dtype(dt)
    return (4 if dt in (np.dtype(np.float32), np.dtype(np.complex64)) else 2), (2 if dt.kind == "c" else 1)


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64, np.complex128])
def test_one_expression_gives_the_same_bits_through_every_kernel(Jets, dt):
    J = Jets
    NS, E = _ns_e(dt)
    n = 1537 * NS // E + 1                                            # 1537 packs and a partial one: 7 tiles of 256 lanes (bands of 3 need >= 6)
    expr, x, y, sc = _mixed(dt, n, 21)
    want = _run(J, expr, dt, [x, y], sc)                              # the 16-byte kernel, operands on the 16-byte grid
    assert np.isfinite(want.view(np.float32 if NS == 4 else np.float64)).sum() > n // 2
    # ... through block views at every scalar offset off the grid (under-aligned packs), each with the partial last pack
    for off in range(1, NS // E + 1):
        R = J.JetBSpace([J.JetSpace(dt, off), J.JetSpace(dt, n), J.JetSpace(dt, 3)])
        pad = lambda h: np.concatenate([np.ones(off, dtype=dt), h, np.ones(3, dtype=dt)])
        u, v, o = J.from_numpy(pad(x), R), J.from_numpy(pad(y), R), J.from_numpy(pad(np.zeros(n, dtype=dt)), R)
        J.broadcast_(J.getblock(o, 1), expr, [J.getblock(u, 1), J.getblock(v, 1)], sc)
        assert_same_values(o.to_numpy(), pad(want), f"view {off} element(s) off the grid")
    # ... the one-element-per-lane kernel: what a vector shorter than one pack takes (complex128: an element IS a pack, that kernel is never taken)
    m = 96
    short = NS // E - 1
    if short:
        R = J.JetBSpace([J.JetSpace(dt, short)] * (m // short))
        u, v, o = J.from_numpy(x[:m], R), J.from_numpy(y[:m], R), J.zeros(R)
        for k in range(m // short):
            J.broadcast_(o.arrays[k], expr, [u.arrays[k], v.arrays[k]], sc)
        assert_same_values(o.to_numpy(), want[:m], "one element per lane")
    # ... the batched kernel: 5 equal items that share x1, under both item orders and two band widths
    count = 5
    R = J.JetBSpace([J.JetSpace(dt, n)] * count)
    u, v = J.from_numpy(np.tile(x, count), R), J.from_numpy(y)
    knobs = (J.tune_get("bcast_item_fast"), J.tune_get("bcast_band"))
    try:
        for item_fast, band in [(0, 1), (1, 1), (1, 3), (0, 3)]:
            J.tune(bcast_item_fast=item_fast, bcast_band=band)
            o = J.zeros(R)
            J.broadcast_many_((o.arrays[k], expr, [u.arrays[k], v], sc) for k in range(count))
            assert_same_values(o.to_numpy(), np.tile(want, count), f"batched, bcast_item_fast={item_fast}, bcast_band={band}")
    finally:
        J.tune(bcast_item_fast=knobs[0], bcast_band=knobs[1])


# ---------------------------------------------------------------------------------------------------------------- tails, aliasing, sentinels
def _muladd(x, y):
    """x*y + x in the element type, every operation rounded (the complex product by its explicit formula, like the prelude's)."""
    if x.dtype.kind != "c":
        return x * y + x
    o = np.empty_like(x)
    o.real = (x.real * y.real - x.imag * y.imag) + x.real
    o.imag = (x.real * y.imag + x.imag * y.real) + x.imag
    return o


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64, np.complex128])
def test_tails_views_and_aliasing_leave_the_neighbours_alone(Jets, dt):
    """Lengths 1 .. 2 NS + 1, 256 NS +- 1 and 512 NS + 3 elements (the partial last pack, one full workgroup and a tail, a second workgroup), as
    views starting 0 .. NS - 1 scalars off the 16-byte grid, out of place and in place (dst is x0); the elements before and after the view are
    sentinels and stay what they were."""
    J = Jets
    NS, E = _ns_e(dt)
    G = 16
    rs = np.random.RandomState(31)
    sentinel = dt(7.25)
    for n in list(range(1, 2 * NS + 2)) + [256 * NS - 1, 256 * NS + 1, 512 * NS + 3]:
        x, y = (rs.standard_normal(n) + 0.5).astype(dt), (rs.standard_normal(n) - 0.25).astype(dt)
        if np.dtype(dt).kind == "c":
            x, y = (x + 1j * rs.standard_normal(n)).astype(dt), (y - 1j * rs.standard_normal(n)).astype(dt)
        want = _muladd(x, y)
        for off in range(max(NS // E, 2)):
            R = J.JetBSpace([J.JetSpace(dt, G + off), J.JetSpace(dt, n), J.JetSpace(dt, G)])
            pad = lambda h: np.concatenate([np.full(G + off, sentinel), h, np.full(G, sentinel)])
            u, v, o = J.from_numpy(pad(x), R), J.from_numpy(pad(y), R), J.from_numpy(pad(np.zeros(n, dtype=dt)), R)
            J.broadcast_(J.getblock(o, 1), "x0*x1 + x0", [J.getblock(u, 1), J.getblock(v, 1)])
            assert o.to_numpy().tobytes() == pad(want).tobytes(), f"n = {n}, {off} off the grid, out of place"
            assert u.to_numpy().tobytes() == pad(x).tobytes()
            J.broadcast_(J.getblock(u, 1), "x0*x1 + x0", [J.getblock(u, 1), J.getblock(v, 1)])
            assert u.to_numpy().tobytes() == pad(want).tobytes(), f"n = {n}, {off} off the grid, in place"


# ---------------------------------------------------------------------------------------------------------------- consumers
@pytest.mark.parametrize("ty", list(TYPES))
@pytest.mark.parametrize("kind", ["tanh", "pow"])
def test_elementwise_operators_alone_and_as_children_of_a_tall_operator(Jets, golden, kind, ty):
    """JopElementwise F and its Jacobian at points of the fixture's domains, as one operator and as the 6 children of a tall block operator (F(m)
    through the batched broadcast), against numpy in long double under the bar of the accuracy tests.
    tanh: s0 * tanh(s1 * x0) with s1 = 2 (the product is exact) and the derivative s0 * s1 / cosh(s1 * x0)^2, for |s1 x0| <= 20 (beyond that the
    derivative leaves Float32's normal range); pow: pow(x0, s0) and s0 * pow(x0, s0 - 1) for bases whose powers stay normal.
    The exponent `s0 - 1` is an operation of the expression, rounded in the element type like every other (1/3 - 1 is not exact); pow is
    ill-conditioned in its exponent by |log x| (208 for the largest Float64 base here), so the reference takes that rounded exponent too: the
    bar measures pow, not the expression's own rounding."""
    J = Jets
    dt = TYPES[ty]
    L = np.longdouble
    rs = np.random.RandomState(41)
    if kind == "tanh":
        m = golden[f"tanh/{ty}/x0"]
        m = m[np.abs(m) <= 10.0]
        f, jac = "s0*tanh(s1*x0)", "s0*s1/(cosh(s1*x0)*cosh(s1*x0))"
        params = [[0.75 + 0.125 * i, 2.0] for i in range(6)]
        F_ref = lambda p, x: L(dt(p[0])) * np.tanh(L(2) * x)
        D_ref = lambda p, x: L(dt(p[0])) * L(2) / np.cosh(L(2) * x) ** 2
    else:
        m = golden[f"pow/{ty}/x0"]
        lim = 20 if ty == "f32" else 300
        m = np.unique(m[(m > 2.0 ** -lim) & (m < 2.0 ** lim)])
        m = np.concatenate([m, np.exp2(rs.uniform(-lim, lim, 300)).astype(dt).astype(np.float64)])
        f, jac = "pow(x0, s0)", "s0*pow(x0, s0 - 1)"
        params = [[s] for s in (2.5, 0.5, 1.5, 3.0, 1.0 / 3.0, 2.0)]
        F_ref = lambda p, x: np.power(x, L(dt(p[0])))
        D_ref = lambda p, x: L(dt(p[0])) * np.power(x, L(dt(dt(p[0]) - dt(1))))
    n = len(m)
    assert n >= 100
    hm = m.astype(dt)
    hd = rs.uniform(0.5, 2.0, n).astype(dt) * rs.choice([-1, 1], n).astype(dt)
    x, d = hm.astype(L), hd.astype(L)
    spc = J.JetSpace(dt, n)
    vm, vd = J.from_numpy(hm), J.from_numpy(hd)

    def check(got, ref, what):
        hi = ref.astype(np.float64)
        lo = (ref - hi.astype(L)).astype(np.float64)
        ok, _, rel, _ = judge(got, hi, lo, dt)
        print(f"{kind}/{ty} {what}: worst relative error {rel.max():.3e}")
        assert ok.all(), f"{kind}/{ty} {what}: {int((~ok).sum())} of {ok.size} points miss the bar; worst relative error {rel.max():.3e}"

    one = J.JopElementwise(spc, f, jac, params[0])
    check((one * vm).to_numpy(), F_ref(params[0], x), "F(m)")
    check((J.jacobian_(one, vm) * vd).to_numpy(), D_ref(params[0], x) * d, "J dm")
    tall = J.blockop([[J.JopElementwise(spc, f, jac, p)] for p in params])
    check((tall * vm).to_numpy(), np.concatenate([F_ref(p, x) for p in params]), "tall F(m)")
    check((J.jacobian_(tall, vm) * vd).to_numpy(), np.concatenate([D_ref(p, x) * d for p in params]), "tall J dm")
