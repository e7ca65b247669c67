"""GPU parity: the one-pass Golub-Kahan step of an N x K GRID of equal elementwise blocks, K = 2 .. 4 (jh_grid_step.hip behind
jh_blockop_bidiag_step), and the native LSQR / CGLS loops that iterate on it (jh_lsqr_solve, jh_cgls_solve).

The step replaces three calls on the device: jh_blockop_mul into a zeroed range vector (src/Jets.jl:1010-1032), jh_lincomb(u, [alpha, beta], [t, u])
and jh_blockop_mul_adj (1034-1057).  u and w keep their bits (beta == 0: u = alpha t and u is not read); ||u||^2 is the fp64 sum of the new u.
Many rows of small blocks sum w in parts (tolerance; adj_split = 0: the ordered walk, bit-exact)."""
import ctypes as C
import math

import numpy as np
import pytest

from .helpers import DTYPES, assert_bits_equal, u01
from .test_gpu_blockop import _mixed_ops

pytestmark = pytest.mark.gpu

UNSUPPORTED = 4


def _native(A):
    from jets_jl_amd import jetblock as _blk

    return _blk._native_op(A.jet.s["_native"], A.jet.s["ops"], A.jet.rng.eltype())


def _flat(x):
    return x.to_numpy().ravel(order="F")


def _real(dt):
    return np.dtype(dt).type(0).real.dtype.type


def _host_update(dt, alpha, beta, t, u):
    """alpha t + beta u in the element type, part by part (a real scalar against complex data), every product and the sum rounded."""
    rd = _real(dt)
    r = t.view(rd) * rd(alpha)
    if beta != 0:
        r = r + u.view(rd) * rd(beta)
    return r.view(dt)


def _normsq64(x):
    x = np.asarray(x)
    return float(np.sum(x.real.astype(np.float64) ** 2) + (np.sum(x.imag.astype(np.float64) ** 2) if x.dtype.kind == "c" else 0.0))


def _step(nat, u, v, w, alpha, beta):
    from jets_jl_amd._ffi import lib

    out = C.c_double(-1.0)
    st = lib.jh_blockop_bidiag_step(nat.handle, u.handle, v.handle, w.handle, float(alpha), float(beta), C.byref(out))
    return st, out.value


def _device_route(J, A, u, v, alpha, beta):
    """The three calls the step replaces: t = A v into zeros, u <- alpha t + beta u (jh_lincomb), w = A'u.  Returns (t, w); u is updated."""
    from jets_jl_amd.arrays import lincomb_

    t = J.mul_(J.zeros(J.range(A)), A, v)
    lincomb_(u, [float(alpha), float(beta)], [t, u])
    w = J.mul_(J.rand(J.domain(A), seed=17, stream=5), A.H, u)
    return t, w


def _inputs(J, oracle, dt, A, nrow, ncol, n, beta):
    hv = [(u01(oracle, dt, 91, k, n) - dt(0.5)).astype(dt) for k in range(ncol)]
    hu = [(u01(oracle, dt, 93, i, n) - dt(0.25)).astype(dt) for i in range(nrow)]
    v = J.from_numpy(np.concatenate(hv), J.domain(A))
    hu0 = np.concatenate(hu)
    if beta == 0:
        hu0 = np.full_like(hu0, np.nan)                                         # u is write-only: a NaN must not leak
    return hv, hu0, v


def _check_step(J, oracle, A, ora, dt, nrow, ncol, n, alpha, beta):
    """One step at the knobs in force against the oracle's two loops and against the device's three calls; returns (u, w, normsq) as host arrays."""
    nat = _native(A)
    hv, hu0, v = _inputs(J, oracle, dt, A, nrow, ncol, n, beta)
    u = J.from_numpy(hu0, J.range(A))
    w = J.rand(J.domain(A), seed=7, stream=3)                                   # a DIRTY output
    st, nrm2 = _step(nat, u, v, w, alpha, beta)
    assert st == 0, f"jh_blockop_bidiag_step on a {nrow} x {ncol} grid returned {st}"
    hu, hw = _flat(u), _flat(w)
    # the oracle: t from +0 in column order, the update part by part, the adjoint of the new u from +0 in row order
    t = oracle.block_df(ora, [np.zeros(n, dt) for _ in range(nrow)], hv)
    uref = [_host_update(dt, alpha, beta, t[i], hu0[i * n:(i + 1) * n]) for i in range(nrow)]
    wref = oracle.block_df_adj(ora, [np.zeros(n, dt) for _ in range(ncol)], uref)
    assert_bits_equal(hu, np.concatenate(uref), f"u of the grid step vs the oracle ({nrow} x {ncol} of {n}, beta {beta})")
    assert_bits_equal(hw, np.concatenate(wref), f"w of the grid step vs the oracle ({nrow} x {ncol} of {n}, beta {beta})")
    assert nrm2 == pytest.approx(_normsq64(hu), rel=1e-12, abs=0.0)
    # the device's three calls
    u2 = J.from_numpy(hu0 if beta != 0 else np.zeros_like(hu0), J.range(A))
    t2, w2 = _device_route(J, A, u2, v, alpha, beta)
    if beta != 0:
        assert_bits_equal(hu, _flat(u2), "u vs jh_blockop_mul + jh_lincomb")
    else:
        assert_bits_equal(hu, _host_update(dt, alpha, 0, _flat(t2), None), "u vs alpha * (jh_blockop_mul into zeros)")
    w3 = J.mul_(J.rand(J.domain(A), seed=18, stream=5), A.H, J.from_numpy(hu, J.range(A)))
    assert_bits_equal(hw, _flat(w3), "w vs jh_blockop_mul_adj of the new u")
    return hu, hw, nrm2


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ncol", [2, 3, 4])
@pytest.mark.parametrize("nrow,n", [(3, 1024), (7, 1027), (11, 67)])
@pytest.mark.parametrize("beta", [0.0, -0.625])
def test_grid_step_has_the_bits_of_the_three_calls(Jets, oracle, dt, ncol, nrow, n, beta):
    J = Jets
    ops = [[J.JopDiagonal(J.rand(J.JetSpace(dt, n), seed=41, stream=100 * i + k)) for k in range(ncol)] for i in range(nrow)]
    A = J.blockop(ops)
    ora = [[oracle.Block("diag", n, coeff=u01(oracle, dt, 41, 100 * i + k, n)) for k in range(ncol)] for i in range(nrow)]
    J.tune(adj_split=0)
    try:
        got = {}
        for nt in (0, 2):
            J.tune(nt=nt)
            got[nt] = _check_step(J, oracle, A, ora, dt, nrow, ncol, n, 1.25, beta)
            assert J.tune_get("last_grid_step_shape") == (1 if nt == 2 else 0)
        assert_bits_equal(got[0][0], got[2][0], "u: temporal and nontemporal loads")
        assert_bits_equal(got[0][1], got[2][1], "w: temporal and nontemporal loads")
        assert got[0][2] == got[2][2]
    finally:
        J.tune(adj_split=-1, nt=1)
    J.close(A)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ncol", [2, 3, 4])
@pytest.mark.parametrize("nrow,n", [(3, 1024), (7, 1027), (11, 67)])
@pytest.mark.parametrize("beta", [0.0, -0.625])
def test_grid_step_with_blocks_of_several_kinds(Jets, oracle, dt, ncol, nrow, n, beta):
    """The regularised multi-parameter operator: diagonal rows over rows of zero / identity / scalar / adjointed blocks, and one whole row of zeros
    (u_i <- alpha*0 + beta*u_i, nothing added to w)."""
    J = Jets
    names = ["diag", "zero", "identity", "scale", "diag_adj", "diag"]
    kinds = [[("diag" if i < max(1, nrow - ncol - 2) and (i % 5 != 3) else names[(2 * i + 3 * k) % 6]) for k in range(ncol)] for i in range(nrow)]
    kinds[nrow - 1] = ["zero"] * ncol
    A, ora = _mixed_ops(J, oracle, dt, kinds, [n] * nrow, [n] * ncol, seed=43)
    J.tune(adj_split=0)
    try:
        got = {}
        for nt in (0, 2):
            J.tune(nt=nt)
            got[nt] = _check_step(J, oracle, A, ora, dt, nrow, ncol, n, 0.75, beta)
        assert_bits_equal(got[0][0], got[2][0], "u: temporal and nontemporal loads")
        assert_bits_equal(got[0][1], got[2][1], "w: temporal and nontemporal loads")
    finally:
        J.tune(adj_split=-1, nt=1)
    J.close(A)


def _grid_problem(J, oracle, dt, nrow, ncol, n, regularised=False):
    """A grid (optionally [[A]; [lam I, 0 ..]; ...]: K regularisation rows) and its fp64 host matvec / rmatvec."""
    kinds = [["diag"] * ncol for _ in range(nrow)]
    if regularised:
        kinds += [["scale" if k == r else "zero" for k in range(ncol)] for r in range(ncol)]
    A, ora = _mixed_ops(J, oracle, dt, kinds, [n] * len(kinds), [n] * ncol, seed=47)
    dt64 = np.complex128 if np.dtype(dt).kind == "c" else np.float64
    rows = len(kinds)

    def blk(i, k):
        b = ora[i][k]
        if b.kind == "diag":
            return b.coeff.astype(dt64)
        if b.kind == "scale":
            return np.full(n, b.scale if np.dtype(dt64).kind == "c" else b.scale.real, dtype=dt64)
        return np.zeros(n, dtype=dt64)

    coef = [[blk(i, k) for k in range(ncol)] for i in range(rows)]

    def matvec(x):
        xs = np.split(x, ncol)
        return np.concatenate([sum(coef[i][k] * xs[k] for k in range(ncol)) for i in range(rows)])

    def rmatvec(d):
        ds = np.split(d, rows)
        return np.concatenate([sum(np.conj(coef[i][k]) * ds[i] for i in range(rows)) for k in range(ncol)])

    return A, rows, dt64, matvec, rmatvec


@pytest.mark.parametrize("dt,xtol", [(np.float32, 2e-4), (np.float64, 1e-9), (np.complex64, 2e-4), (np.complex128, 1e-9)])
@pytest.mark.parametrize("damp,use_x0", [(0.0, False), (0.3, True)])
@pytest.mark.parametrize("solver", ["lsqr", "cgls"])
def test_native_solves_on_a_grid(Jets, oracle, dt, xtol, damp, use_x0, solver):
    """jh_lsqr_solve / jh_cgls_solve called directly (no fallback can hide) on a regularised 6 x 3 grid, against the fp64 CPU solvers."""
    from oracle.cgls_ref import cgls_fp64
    from oracle.lsqr_ref import lsqr_fp64
    from jets_jl_amd._ffi import LsqrResultC, lib

    J = Jets
    ncol, n, iters = 3, 1500, 10
    A, rows, dt64, matvec, rmatvec = _grid_problem(J, oracle, dt, 6, ncol, n, regularised=True)
    hb = (u01(oracle, dt, 51, 0, rows * n) - dt(0.5)).astype(dt)
    hx0 = (u01(oracle, dt, 52, 0, ncol * n) * dt(0.1)).astype(dt)
    u = J.from_numpy(hb, J.range(A))
    x = J.from_numpy(hx0, J.domain(A)) if use_x0 else J.rand(J.domain(A), seed=9, stream=9)
    res = LsqrResultC()
    hist = (C.c_double * (2 * iters))()
    nat = _native(A)
    if solver == "lsqr":
        st = lib.jh_lsqr_solve(nat.handle, u.handle, x.handle, 1 if use_x0 else 0, damp, 0.0, 0.0, 0.0, iters, 0, C.byref(res), hist)
        xr, info = lsqr_fp64(matvec, rmatvec, hb.astype(dt64), ncol * n, x0=hx0.astype(dt64) if use_x0 else None, damp=damp, atol=0.0, btol=0.0,
                             conlim=0.0, maxiter=iters)
    else:
        st = lib.jh_cgls_solve(nat.handle, u.handle, x.handle, 1 if use_x0 else 0, damp, 0.0, 0.0, iters, 0, C.byref(res), hist)
        xr, info = cgls_fp64(matvec, rmatvec, hb.astype(dt64), ncol * n, x0=hx0.astype(dt64) if use_x0 else None, damp=damp, atol=0.0, btol=0.0,
                             maxiter=iters)
    assert st == 0, f"jh_{solver}_solve on a grid returned {st}"
    assert res.itn == iters == info["itn"] and res.istop == 7
    hx = _flat(x).astype(dt64)
    assert np.linalg.norm(hx - xr) / np.linalg.norm(xr) < xtol
    for k, (_, r_ref, _) in enumerate(info["history"]):
        assert hist[2 * k] == pytest.approx(r_ref, rel=max(10 * xtol, 1e-8))
    J.close(A)


@pytest.mark.parametrize("dt,tol", [(np.float32, 1e-5), (np.float64, 1e-12), (np.complex64, 1e-5)])
@pytest.mark.parametrize("solver", ["lsqr", "cgls"])
def test_jets_solvers_on_a_grid_take_the_native_route(Jets, oracle, dt, tol, solver, monkeypatch):
    """Jets.lsqr / Jets.cgls on a bare grid run jh_*_solve (counter grid_solve_calls); with the native loop off the Python loop runs on the grid step
    (grid_step_calls, LSQR) or the two halves (CGLS), with the same residual history to tolerance."""
    from jets_jl_amd import chains

    J = Jets
    A, rows, _, _, _ = _grid_problem(J, oracle, dt, 5, 2, 900)
    hb = (u01(oracle, dt, 53, 0, rows * 900) - dt(0.5)).astype(dt)
    solve = J.lsqr if solver == "lsqr" else J.cgls
    kw = dict(conlim=0.0) if solver == "lsqr" else {}
    g0, s0 = chains.STATS["grid_solve_calls"], chains.STATS["grid_step_calls"]
    r1 = solve(A, J.from_numpy(hb, J.range(A)), damp=0.2, atol=0.0, btol=0.0, maxiter=8, **kw)
    assert chains.STATS["grid_solve_calls"] == g0 + 1
    monkeypatch.setenv("JETS_LSQR_NATIVE" if solver == "lsqr" else "JETS_CGLS_NATIVE", "0")
    r2 = solve(A, J.from_numpy(hb, J.range(A)), damp=0.2, atol=0.0, btol=0.0, maxiter=8, **kw)
    assert chains.STATS["grid_solve_calls"] == g0 + 1
    if solver == "lsqr":
        assert chains.STATS["grid_step_calls"] == s0 + 8
    assert r1.itn == r2.itn == 8
    for (i1, a1, b1), (i2, a2, b2) in zip(r1.history, r2.history):
        assert i1 == i2 and a1 == pytest.approx(a2, rel=100 * tol) and b1 == pytest.approx(b2, rel=1000 * tol)
    x1, x2 = _flat(r1.x), _flat(r2.x)
    assert np.linalg.norm(x1 - x2) <= 100 * tol * np.linalg.norm(x2)
    J.close(A)


@pytest.mark.parametrize("dt,nrow,ncol,shape", [(np.float32, 600, 3, (515,)), (np.float64, 600, 3, (515,)), (np.complex64, 600, 2, (515,)),
                                                (np.float32, 16384, 2, (32, 32, 32))])
def test_many_small_rows_take_the_split_walk(Jets, oracle, dt, nrow, ncol, shape):
    J = Jets
    blk = J.JetSpace(dt, *shape)
    coeff = J.rand(J.JetBSpace([blk] * (nrow * ncol)), seed=1, stream=0)
    A = J.blockop([[J.JopDiagonal(coeff.arrays[i * ncol + k]) for k in range(ncol)] for i in range(nrow)])
    nat = _native(A)
    v = J.rand(J.domain(A), seed=2, stream=0)

    def run():
        u = J.rand(J.range(A), seed=3, stream=0)
        w = J.rand(J.domain(A), seed=4, stream=0)
        st, nrm2 = _step(nat, u, v, w, 0.5, -0.75)
        assert st == 0
        return u, w, nrm2

    u1, w1, n1 = run()
    assert J.tune_get("last_grid_step_shape") & 2, "the launcher splits the rows"
    u2, w2, n2 = run()
    assert float(J.norm((u1 - u2).materialize(), math.inf)) == 0.0
    assert float(J.norm((w1 - w2).materialize(), math.inf)) == 0.0, "the split walk is deterministic"
    assert n1 == n2
    J.tune(adj_split=0)
    try:
        u0, w0, n0 = run()
        assert J.tune_get("last_grid_step_shape") & 2 == 0
    finally:
        J.tune(adj_split=-1)
    assert float(J.norm((u1 - u0).materialize(), math.inf)) == 0.0, "u does not depend on the part count"
    hw0, hw1 = _flat(w0), _flat(w1)
    eps = 2e-5 if np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4 else 1e-13
    assert np.abs(hw1 - hw0).max() <= eps * np.sqrt(nrow) * np.abs(hw0).max()
    assert n1 == pytest.approx(n0, rel=1e-12)
    J.close(A)


def _expect_declined(J, nat, u, v, w, what):
    hu, hv, hw = _flat(u).copy(), _flat(v).copy(), _flat(w).copy()
    st, _ = _step(nat, u, v, w, 1.0, -0.5)
    assert st == UNSUPPORTED, f"{what}: status {st}"
    assert_bits_equal(_flat(u), hu, f"{what}: u untouched")
    assert_bits_equal(_flat(w), hw, f"{what}: w untouched")
    assert_bits_equal(_flat(v), hv, f"{what}: v untouched")


def test_declined_grids_leave_the_outputs_untouched(Jets, oracle):
    from jets_jl_amd._ffi import LsqrResultC, lib

    J = Jets
    dt, n = np.float32, 515

    def case(A, what):
        u, v, w = J.rand(J.range(A), seed=3, stream=1), J.rand(J.domain(A), seed=4, stream=1), J.rand(J.domain(A), seed=5, stream=1)
        _expect_declined(J, _native(A), u, v, w, what)
        J.close(A)

    case(J.blockop([[J.JopDiagonal(J.rand(J.JetSpace(dt, n), seed=1, stream=10 * i + k)) for k in range(5)] for i in range(4)]), "K = 5")
    hA = u01(oracle, dt, 7, 0, 64 * 64).reshape(64, 64)
    case(J.blockop([[J.JopDense(J.from_numpy(hA)) for _ in range(2)] for _ in range(3)]), "dense children")
    A, _ = _mixed_ops(J, oracle, dt, [["diag", "zero"], ["zero", "diag"], ["diag", "zero"]], [n, n + 4, n], [n, n + 4], seed=5)
    case(A, "ragged blocks")
    case(J.blockop([[J.JopDiagonal(J.rand(J.JetSpace(dt, 3), seed=1, stream=10 * i + k)) for k in range(2)] for i in range(3)]), "12-byte blocks")

    A = J.blockop([[J.JopDiagonal(J.rand(J.JetSpace(dt, n), seed=1, stream=10 * i + k)) for k in range(3)] for i in range(4)])
    nat = _native(A)
    u, w = J.rand(J.range(A), seed=3, stream=1), J.rand(J.domain(A), seed=5, stream=1)
    J.tune(grid_step=0)
    try:
        _expect_declined(J, nat, u, J.rand(J.domain(A), seed=4, stream=1), w, "knob grid_step = 0")
    finally:
        J.tune(grid_step=1)
    # a domain vector one float past its allocation's start (read-only: the step must decline before it reads it)
    big = J.rand(J.JetSpace(dt, 3 * n + 4), seed=4, stream=2)
    data = C.c_void_p()
    nb, ln, dtype = C.c_int64(), C.c_int64(), C.c_int()
    assert lib.jh_bvec_info(big.handle, C.byref(nb), C.byref(ln), C.byref(dtype), C.byref(data)) == 0
    lens = (C.c_int64 * 3)(n, n, n)
    vh = C.c_void_p()
    assert lib.jh_bvec_wrap(C.c_void_p(data.value + 2), 3, lens, dtype.value, C.byref(vh)) == 0
    try:
        hu, hw = _flat(u).copy(), _flat(w).copy()
        out = C.c_double(0)
        assert lib.jh_blockop_bidiag_step(nat.handle, u.handle, vh, w.handle, 1.0, -0.5, C.byref(out)) == UNSUPPORTED
        assert_bits_equal(_flat(u), hu, "misaligned v: u untouched")
        assert_bits_equal(_flat(w), hw, "misaligned v: w untouched")
    finally:
        lib.jh_bvec_destroy(vh)
    v = J.rand(J.domain(A), seed=4, stream=1)
    hu, hw = _flat(u).copy(), _flat(w).copy()
    out = C.c_double(0)
    assert lib.jh_blockop_bidiag_step_range(nat.handle, u.handle, v.handle, w.handle, 1.0, -0.5, 0, 3 * n, C.byref(out)) == UNSUPPORTED
    assert_bits_equal(_flat(u), hu, "ranged step: u untouched")
    assert_bits_equal(_flat(w), hw, "ranged step: w untouched")
    # the partitioned and team solves keep declining grids
    x = J.rand(J.domain(A), seed=6, stream=1)
    hx = _flat(x).copy()
    res = LsqrResultC()
    hist = (C.c_double * 8)()
    arr = lambda h: (C.c_void_p * 1)(h.value if hasattr(h, "value") else h)
    for name, call in (("jh_lsqr_solve_partitioned", lambda: lib.jh_lsqr_solve_partitioned(nat.handle, u.handle, x.handle, 0, 0.0, 0.0, 0.0, 0.0, 4, 0, C.byref(res), hist)),
                       ("jh_cgls_solve_partitioned", lambda: lib.jh_cgls_solve_partitioned(nat.handle, u.handle, x.handle, 0, 0.0, 0.0, 0.0, 4, 0, C.byref(res), hist)),
                       ("jh_lsqr_solve_team", lambda: lib.jh_lsqr_solve_team(1, arr(nat.handle), arr(u.handle), arr(x.handle), 0, 0.0, 0.0, 0.0, 0.0, 4, 0, C.byref(res), hist)),
                       ("jh_cgls_solve_team", lambda: lib.jh_cgls_solve_team(1, arr(nat.handle), arr(u.handle), arr(x.handle), 0, 0.0, 0.0, 0.0, 4, 0, C.byref(res), hist))):
        st = call()
        assert st != 0, f"{name} took a grid"
        if name.endswith("_partitioned"):
            assert st == UNSUPPORTED, f"{name}: status {st}"
        assert_bits_equal(_flat(u), hu, f"{name}: u untouched")
        assert_bits_equal(_flat(x), hx, f"{name}: x untouched")
    J.close(A)


def test_full_size_grid_step_on_64x4_of_256cubed(Jets, oracle):
    """One step on 64 x 4 of 256^3 Float32 (16 GiB of coefficients, a 4 GiB range vector), with the launcher's own choices: slices against the oracle on
    regenerated inputs, the whole u against the device's two-half route (max |difference| == 0), the whole w equal (or, split, to tolerance)."""
    from jets_jl_amd.arrays import lincomb_

    J = Jets
    nrow, ncol, edge = 64, 4, 256
    n = edge ** 3
    alpha, beta = 1.5, -0.625
    blk = J.JetSpace(np.float32, edge, edge, edge)
    coeff = J.rand(J.JetBSpace([blk] * (nrow * ncol)), seed=1, stream=0)         # block (i, k) = coeff block i K + k
    A = J.blockop([[J.JopDiagonal(coeff.arrays[i * ncol + k]) for k in range(ncol)] for i in range(nrow)])
    nat = _native(A)
    v = J.rand(J.domain(A), seed=2, stream=0)
    u = J.rand(J.range(A), seed=3, stream=0)
    w = J.rand(J.domain(A), seed=7, stream=0)
    st, nrm2 = _step(nat, u, v, w, alpha, beta)
    assert st == 0
    split = J.tune_get("last_grid_step_shape") & 2
    W = 4096
    for off in (0, (n // 3) // 4 * 4 + 1, n // 2 + 64, n - W):
        ops = [[oracle.Block("diag", W, coeff=oracle.rng_u01(np.float32, 1, 0, (i * ncol + k) * n + off, W)) for k in range(ncol)] for i in range(nrow)]
        hv = [oracle.rng_u01(np.float32, 2, 0, k * n + off, W) for k in range(ncol)]
        t = oracle.block_df(ops, [np.zeros(W, np.float32) for _ in range(nrow)], hv)
        uref = [_host_update(np.float32, alpha, beta, t[i], oracle.rng_u01(np.float32, 3, 0, i * n + off, W)) for i in range(nrow)]
        for i in (0, 17, nrow - 1):
            assert_bits_equal(u._download(i * n + off, W), uref[i], f"u slice at {off} of row {i}")
        wref = oracle.block_df_adj(ops, [np.zeros(W, np.float32) for _ in range(ncol)], uref)
        for k in range(ncol):
            got = w._download(k * n + off, W)
            if split:
                assert np.abs(got - wref[k]).max() <= 2e-5 * np.sqrt(nrow) * np.abs(wref[k]).max()
            else:
                assert_bits_equal(got, wref[k], f"w slice at {off} of block column {k}")
    u2 = J.rand(J.range(A), seed=3, stream=0)
    t = J.mul_(J.zeros(J.range(A)), A, v)
    lincomb_(u2, [alpha, beta], [t, u2])
    del t
    assert float(J.norm((u - u2).materialize(), math.inf)) == 0.0             # bit-identical on every element
    w2 = J.mul_(J.zeros(J.domain(A)), A.H, u2)
    dw = float(J.norm((w - w2).materialize(), math.inf))
    assert dw == 0.0 if not split else dw <= 2e-5 * np.sqrt(nrow) * float(J.norm(w2, math.inf))
    assert nrm2 == pytest.approx(float(J.norm(u2)) ** 2, rel=1e-6)
    J.close(A)
