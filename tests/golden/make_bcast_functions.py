#!/usr/bin/env python3
"""High-precision references for the functions of the compiled broadcast (tests/golden/bcast_functions.npz).

    python tests/golden/make_bcast_functions.py          # rewrites bcast_functions.npz next to this script (mpmath, ~20 s)

For every function of FUNCTIONS and each real element type (f32, f64) the file holds

    <fn>/<type>/x0 [, <fn>/<type>/x1]    the operands: exact values of that type, held in float64
    <fn>/<type>/hi                        the 50-digit result rounded to the nearest float64 (ties to even, overflow to Inf,
                                          gradual underflow; zeros and NaN carry their sign / class)
    <fn>/<type>/lo                        f64 only: the 50-digit result minus hi, rounded -- (hi, lo) is a double-double

For f32 `hi` alone is the reference (29 more bits than the type has).  At most MAX_POINTS points per (function, type).
Nothing here is needed on a machine that only RUNS the tests: they read the .npz; tests/test_bcast_function_fixture.py
regenerates every 16th point where mpmath is installed and compares it with the committed file.

DOMAIN RULE.  The reference semantics are Julia's, and inputs stay inside Julia's domain: anything for which Julia throws a
DomainError is left out -- log / log2 / log10 of a negative number, asin / acos outside [-1, 1], a negative base with a
non-integer exponent, sin / cos / tan of an infinity.  -0.0 and NaN operands are left out as well except where a function's
list names them (atan2's signed zeros, hypot(Inf, NaN)): what the kernels do with signed zeros and NaN is tested bit for bit
in tests/test_gpu_broadcast_functions.py, not against this file.

The generator is deterministic: fixed edge lists plus a fill from numpy's RandomState seeded by the (function, type) name,
log-uniform in magnitude (uniform where the interesting domain is an interval of arguments, as for exp and sin).
"""
from __future__ import annotations

import os
import sys
import zlib
from fractions import Fraction

import numpy as np

MAX_POINTS = 400
TYPES = {"f32": np.float32, "f64": np.float64}
UNARY = ["exp", "exp2", "log", "log2", "log10", "sin", "cos", "tan", "tanh", "sinh", "cosh", "asin", "acos", "atan", "erf"]
BINARY = ["atan2", "hypot", "pow"]
FUNCTIONS = UNARY + BINARY
POW_EXPONENTS = [0.0, 0.5, -0.5, 1.0, -1.0, 2.0, 2.5, 3.0, -3.0, 1.0 / 3.0, 10.5, 100.0]


def _mp():
    import mpmath

    mpmath.mp.dps = 50
    return mpmath


# ------------------------------------------------------------------------------------------------------------------ inputs
def _snap(x, dt):
    """The values of x rounded into dt, as float64, first occurrences only (order kept; -0.0 and +0.0 are distinct)."""
    with np.errstate(over="ignore"):
        y = np.asarray(x, dtype=np.float64).astype(dt).astype(np.float64)
    _, first = np.unique(y.view(np.int64), return_index=True)
    return y[np.sort(first)]


def _rs(fn, ty):
    return np.random.RandomState(zlib.crc32(f"{fn}/{ty}".encode()))


def _loguni(rs, lo, hi, n, both_signs=True):
    x = 10.0 ** rs.uniform(np.log10(lo), np.log10(hi), n)
    return x * rs.choice([-1.0, 1.0], n) if both_signs else x


def _around(x, dt, k=2):
    """x rounded into dt and its k neighbours on each side."""
    c = np.asarray(x, dtype=np.float64).astype(dt)
    out = [c]
    up = dn = c
    for _ in range(k):
        up, dn = np.nextafter(up, dt(np.inf)), np.nextafter(dn, dt(-np.inf))
        out += [up, dn]
    return np.concatenate([np.atleast_1d(o) for o in out]).astype(np.float64)


def _exp_points(fn, ty, dt):
    fi, rs = np.finfo(dt), _rs(fn, ty)
    ln = np.log(2.0) if fn == "exp" else 1.0
    lo, hi = ((-104.0, 89.0) if ty == "f32" else (-746.0, 710.0)) if fn == "exp" else ((-151.0, 129.0) if ty == "f32" else (-1076.0, 1025.0))
    sub = float(fi.smallest_subnormal)
    thresholds = [np.log2(float(fi.max)) * ln, np.log2(float(fi.tiny)) * ln, np.log2(sub) * ln, (np.log2(sub) - 1) * ln]
    edges = [0.0, lo, hi, 1.0, -1.0, 0.5, -0.5, float(fi.eps) / 4, -float(fi.eps) / 4, 1e-30, -1e-30]
    parts = [edges] + [_around(t, dt, 3) for t in thresholds]
    if fn == "exp2":       # integer arguments: all of them for f32; f64 keeps those next to the range's ends and a stride (every integer runs in the GPU test itself)
        k = np.arange(-151, 130) if ty == "f32" else np.concatenate([np.arange(-1076, -1060), np.arange(-1030, -1015), np.arange(-12, 13), np.arange(1015, 1026), np.arange(-1060, 1015, 11)])
        parts.append(k.astype(np.float64))
    n_fill = MAX_POINTS - sum(len(p) for p in parts) - 40
    parts += [rs.uniform(lo, hi, n_fill), _loguni(rs, 1e-30, 1.0, 40)]
    return (_snap(np.concatenate(parts), dt),)


def _log_points(fn, ty, dt):
    fi, rs = np.finfo(dt), _rs(fn, ty)
    emin, emax = int(np.log2(float(fi.smallest_subnormal))), int(fi.maxexp) - 1
    ks = np.arange(emin, emax + 1)
    if len(ks) > 290:                                   # f64: both ends and the subnormal border in full, a stride between
        ks = np.unique(np.concatenate([ks[:12], np.arange(-1030, -1015), np.arange(-8, 9), ks[-12:], ks[::9]]))
    eps = float(fi.eps)
    near1 = [1.0 + k * eps for k in range(1, 9)] + [1.0 - k * eps for k in range(1, 9)]
    edges = [0.0, np.inf, 1.0, float(fi.max), float(fi.tiny), float(fi.smallest_subnormal), 2.718281828459045, 10.0, 0.5, 0.9, 1.1]
    fill = _loguni(rs, float(fi.smallest_subnormal) * 4, float(fi.max) / 4, MAX_POINTS - len(ks) - len(near1) - len(edges), both_signs=False)
    return (_snap(np.concatenate([edges, near1, np.ldexp(1.0, ks), fill]), dt),)


def _nearest_two(v, dt):
    """The two floats of dt that bracket the mpmath number v."""
    c = dt(float(v))
    other = np.nextafter(c, dt(np.inf)) if float(c) < v else np.nextafter(c, dt(-np.inf))
    return [float(c), float(other)]


def _trig_points(fn, ty, dt):
    mp, rs = _mp(), _rs(fn, ty)
    pts = []
    for k in list(range(1, 65)) + [-k for k in range(1, 17)]:
        pts += _nearest_two(k * mp.pi / 2, dt)
    big = [1e5, 1e10, 1e22, float(np.finfo(dt).max)]
    edges = [0.0, 1e-30, -1e-30, 0.5, -0.5, 1.0, -1.0] + big + [-b for b in big]
    fill = rs.uniform(-2 * np.pi, 2 * np.pi, MAX_POINTS - len(pts) - len(edges) - 20)
    return (_snap(np.concatenate([edges, pts, fill, _loguni(rs, 1e-30, 1.0, 20)]), dt),)


def _hyperbolic_points(fn, ty, dt):
    fi, rs = np.finfo(dt), _rs(fn, ty)
    top = 100.0 if ty == "f32" else 720.0
    over = np.log(float(fi.max)) + np.log(2.0)          # sinh / cosh overflow just above log(2 max)
    sat = (np.log(2.0 / float(fi.eps)) / 2)             # tanh rounds to 1 beyond about atanh(1 - eps/2)
    parts = [[1e-30, -1e-30, 1.0, -1.0, top, -top, float(fi.tiny), float(fi.eps), 0.5, 22.0, -22.0]]
    for t in (over, sat, np.log(float(fi.max))):
        parts += [_around(t, dt, 2), -_around(t, dt, 2)]
    n_fill = MAX_POINTS - sum(len(p) for p in parts)
    parts += [_loguni(rs, 1e-30, top, n_fill - 120), rs.uniform(-top, top, 120)]
    return (_snap(np.concatenate(parts), dt),)


def _asin_points(fn, ty, dt):
    rs = _rs(fn, ty)
    edges = np.concatenate([_around(1.0, dt, 4), _around(-1.0, dt, 4), [0.5, -0.5, 0.70710678118654752, 0.8660254037844386, 1e-30, -1e-30, 0.0]])
    edges = edges[np.abs(edges) <= 1.0]
    fill = np.concatenate([rs.uniform(-1.0, 1.0, 220), _loguni(rs, 1e-30, 1.0, 80), (1.0 - _loguni(rs, 1e-7 if ty == "f32" else 1e-16, 0.1, 60, False)) * rs.choice([-1.0, 1.0], 60)])
    return (_snap(np.concatenate([edges, fill]), dt),)


def _atan_points(fn, ty, dt):
    fi, rs = np.finfo(dt), _rs(fn, ty)
    edges = [np.inf, -np.inf, float(fi.max), -float(fi.max), float(fi.smallest_subnormal), float(fi.tiny), 1.0, -1.0, 0.0, 2.414213562373095, 0.41421356237309503]
    fill = np.concatenate([_loguni(rs, float(fi.smallest_subnormal), float(fi.max), 280), _loguni(rs, 1e-3, 1e3, 100)])
    return (_snap(np.concatenate([edges, fill]), dt),)


def _erf_points(fn, ty, dt):
    rs = _rs(fn, ty)
    edges = [1e-30, -1e-30, 10.0, -10.0, 1.0, -1.0, 0.5, 0.84375, 1.25, 2.857142857142857, 6.0, 3.92, 5.93, 4.0, -4.0]
    fill = np.concatenate([_loguni(rs, 1e-30, 10.0, 230), rs.uniform(-6.5, 6.5, 150)])
    return (_snap(np.concatenate([edges, fill]), dt),)


def _pairs(y, x, dt):
    """Operand pairs rounded into dt, first occurrences only."""
    with np.errstate(over="ignore"):
        y, x = (np.asarray(a, dtype=np.float64).astype(dt).astype(np.float64) for a in (y, x))
    key = np.stack([y.view(np.int64), x.view(np.int64)], axis=1)
    _, first = np.unique(key, axis=0, return_index=True)
    first = np.sort(first)[:MAX_POINTS]
    return y[first], x[first]


def _atan2_points(fn, ty, dt):
    fi, rs = np.finfo(dt), _rs(fn, ty)
    special = [0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, float(fi.max), -float(fi.tiny), float(fi.smallest_subnormal)]
    ys, xs = [], []
    for a in special:
        for b in special:
            ys.append(a)
            xs.append(b)
    n = MAX_POINTS - len(ys)
    ys = np.concatenate([ys, _loguni(rs, 1e-3, 1e3, n // 2), _loguni(rs, float(fi.tiny), float(fi.max) / 4, n - n // 2)])
    xs = np.concatenate([xs, _loguni(rs, 1e-3, 1e3, n // 2), _loguni(rs, float(fi.tiny), float(fi.max) / 4, n - n // 2)])
    return _pairs(ys, xs, dt)


def _hypot_points(fn, ty, dt):
    fi, rs = np.finfo(dt), _rs(fn, ty)
    emax = int(fi.maxexp) - 1
    big, small = np.ldexp(1.0, emax - 1), np.ldexp(1.0, -(emax - 1))
    ys = [np.inf, np.nan, -np.inf, big, big, 1.5 * big, small, small, 3.0, 0.0, 1.0, float(fi.smallest_subnormal), float(fi.max), float(fi.tiny)]
    xs = [np.nan, np.inf, 1.0, big, small, 1.5 * big, small, -1.5 * small, 4.0, 5.0, float(fi.eps), float(fi.smallest_subnormal), 1.0, float(fi.tiny)]
    n = MAX_POINTS - len(ys)
    e1, e2 = rs.randint(-(emax - 1), emax, n), rs.randint(-(emax - 1), emax, n)
    near = rs.rand(n) < 0.6                              # most pairs within a few binades of each other: both operands matter
    e2 = np.where(near, np.clip(e1 + rs.randint(-3, 4, n), -(emax - 1), emax - 1), e2)
    ys = np.concatenate([ys, np.ldexp(rs.uniform(1.0, 2.0, n), e1) * rs.choice([-1.0, 1.0], n)])
    xs = np.concatenate([xs, np.ldexp(rs.uniform(1.0, 2.0, n), e2) * rs.choice([-1.0, 1.0], n)])
    return _pairs(ys, xs, dt)


def _pow_points(fn, ty, dt):
    fi, rs = np.finfo(dt), _rs(fn, ty)
    emin, emax = int(np.log2(float(fi.smallest_subnormal))), int(fi.maxexp) - 1
    bs, es = [], []
    base_exps = np.unique(np.concatenate([np.linspace(emin, emax, 17).astype(int), [-1, 0, 1]]))
    for y in POW_EXPONENTS:
        for e in base_exps:
            bs.append(float(np.ldexp(rs.uniform(1.0, 2.0), int(e))))
            es.append(y)
        for b in (0.0, 1.0):                             # 0^y for y > 0; 1^y
            if b == 1.0 or y > 0:
                bs.append(b)
                es.append(y)
    for y in (0.0, 1.0, -1.0, 2.0, 3.0, -3.0, 100.0):    # negative bases, integer-valued exponents only (Julia's domain)
        for b in (-1.0, -1.5, -2.0, -0.75, -float(fi.tiny) * 3, -np.ldexp(1.25, emax // 2), -np.ldexp(1.75, emin // 2 + 20), -10.0, -1.0000001):
            bs.append(b)
            es.append(y)
    n = MAX_POINTS - len(bs)
    # results on both sides of overflow and underflow: |y * log2(b)| drawn around the exponent range's ends, and ordinary pairs
    yb = rs.choice([0.5, -0.5, 2.0, 2.5, 3.0, -3.0, 1.0 / 3.0, 10.5, 100.0], n)
    target = np.where(rs.rand(n) < 0.5, rs.uniform(emin - 6, emin + 40, n), rs.uniform(emax - 40, emax + 6, n))
    target = np.where(rs.rand(n) < 0.3, rs.uniform(-30, 30, n), target)
    lb = np.clip(target / yb, emin + 1, emax - 1)
    bs = np.concatenate([bs, np.exp2(lb)])
    es = np.concatenate([es, yb])
    return _pairs(bs, es, dt)


_POINTS = {"exp": _exp_points, "exp2": _exp_points, "log": _log_points, "log2": _log_points, "log10": _log_points, "sin": _trig_points, "cos": _trig_points,
           "tan": _trig_points, "tanh": _hyperbolic_points, "sinh": _hyperbolic_points, "cosh": _hyperbolic_points, "asin": _asin_points, "acos": _asin_points,
           "atan": _atan_points, "erf": _erf_points, "atan2": _atan2_points, "hypot": _hypot_points, "pow": _pow_points}


def points(fn, ty):
    """The operands of (function, type): a tuple of one or two float64 arrays of exact values of the type."""
    ops = _POINTS[fn](fn, ty, TYPES[ty])
    assert all(len(o) == len(ops[0]) for o in ops) and 0 < len(ops[0]) <= MAX_POINTS, (fn, ty, [len(o) for o in ops])
    return ops


# ------------------------------------------------------------------------------------------------------------------ references
def _to_double(v):
    """An mpmath number rounded to the nearest float64 (ties to even; Inf beyond the range; gradual underflow)."""
    mp = _mp()
    if mp.isnan(v):
        return float("nan")
    if mp.isinf(v):
        return float("inf") if v > 0 else float("-inf")
    sign, man, exp, _ = v._mpf_
    if man == 0:
        return 0.0
    q = Fraction(int(man) << exp) if exp >= 0 else Fraction(int(man), 1 << -exp)
    try:
        r = q.numerator / q.denominator                  # int / int: correctly rounded, subnormals included
    except OverflowError:
        r = float("inf")
    return -r if sign else r


def _atan2_ref(mp, y, x):
    import math

    if y == 0 or x == 0 or math.isinf(y) or math.isinf(x):   # IEEE 754 / C99 special operands (Julia's atan(y, x) follows them): a multiple of pi/4
        r = math.atan2(y, x)
        k = round(r / (math.pi / 4))
        return (mp.mpf(k) * mp.pi / 4) if k else r            # (a zero keeps its sign: returned as a float)
    return mp.atan2(mp.mpf(y), mp.mpf(x))


def _pow_ref(mp, b, y):
    if y == 0 or b == 1:
        return mp.mpf(1)
    if b == 0:
        return mp.mpf(0)                                      # (y > 0 only)
    if b < 0:
        assert y == int(y)
        r = mp.power(mp.mpf(-b), mp.mpf(y))
        return -r if int(y) % 2 else r
    return mp.power(mp.mpf(b), mp.mpf(y))


def _hypot_ref(mp, y, x):
    import math

    if math.isinf(y) or math.isinf(x):
        return mp.inf                                         # hypot(Inf, NaN) = Inf
    return mp.sqrt(mp.mpf(y) ** 2 + mp.mpf(x) ** 2)


def reference(fn, *ops):
    """(hi, lo) float64 arrays: the 50-digit value of fn at the operands as a double-double."""
    mp = _mp()
    one = {"exp": mp.exp, "exp2": lambda x: mp.power(2, x), "log": mp.log, "log2": lambda x: mp.log(x) / mp.log(2), "log10": mp.log10, "sin": mp.sin,
           "cos": mp.cos, "tan": mp.tan, "tanh": mp.tanh, "sinh": mp.sinh, "cosh": mp.cosh, "asin": mp.asin, "acos": mp.acos, "atan": mp.atan, "erf": mp.erf}
    two = {"atan2": _atan2_ref, "hypot": _hypot_ref, "pow": _pow_ref}
    n = len(ops[0])
    hi, lo = np.zeros(n), np.zeros(n)
    for i in range(n):
        if fn in one:
            x = float(ops[0][i])
            if fn in ("log", "log2", "log10") and x == 0:
                v = -mp.inf
            elif fn == "exp2" and x == int(x) if np.isfinite(x) else False:
                v = mp.ldexp(mp.mpf(1), int(x))
            else:
                v = one[fn](mp.mpf(x))
        else:
            v = two[fn](mp, float(ops[0][i]), float(ops[1][i]))
        if isinstance(v, float):                              # a signed zero
            hi[i] = v
            continue
        assert v.imag == 0 if hasattr(v, "imag") else True, (fn, [o[i] for o in ops])
        v = mp.mpf(v.real) if hasattr(v, "real") else v
        hi[i] = _to_double(v)
        if np.isfinite(hi[i]) and hi[i] != 0:
            lo[i] = _to_double(v - mp.mpf(float(hi[i])))
    return hi, lo


def cases(stride=1, functions=FUNCTIONS):
    """name -> array, as stored; stride k keeps every k-th point of each (function, type)."""
    out = {}
    for fn in functions:
        for ty in TYPES:
            ops = tuple(o[::stride] for o in points(fn, ty))
            hi, lo = reference(fn, *ops)
            for k, o in enumerate(ops):
                out[f"{fn}/{ty}/x{k}"] = o
            out[f"{fn}/{ty}/hi"] = hi
            if ty == "f64":
                out[f"{fn}/{ty}/lo"] = lo
    return out


PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bcast_functions.npz")

if __name__ == "__main__":
    arrays = cases()
    np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else PATH, **arrays)
    print(f"wrote {len(arrays)} arrays, {sum(len(v) for k, v in arrays.items() if k.endswith('/hi'))} points for {len(FUNCTIONS)} functions x {len(TYPES)} types")
