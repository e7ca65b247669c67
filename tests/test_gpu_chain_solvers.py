"""GPU: LSQR / CGLS / CGNR on a FORWARD chain -- the weighted least squares users run as `lsqr(W o A o M, b)` (docs/src/index.md:235-246) -- through
jh_lsqr_solve_chain / jh_cgls_solve_chain / jh_cgnr_solve_chain (jh_lsqr.hip) and the Python loop on the chain step (jets.jl_amd/lsqr.py: _Engine).

Against the fp64 CPU solvers (oracle/lsqr_ref.py, oracle/cgls_ref.py) on host copies of the weights and of A at the tolerances of test_gpu_lsqr.py /
test_gpu_cgls.py; the native solve against the Python loop on the chain step (JETS_*_NATIVE=0) and against today's route (JETS_CHAIN_STEP=0);
chains.STATS proves which route ran; a chain the step declines still solves, on the old route."""
import numpy as np
import pytest

from oracle.cgls_ref import cgls_fp64
from oracle.lsqr_ref import lsqr_fp64

from .helpers import u01
from .test_gpu_chains import Rig

pytestmark = pytest.mark.gpu

CHAINS = {
    "W o A": ["A", ("W", 0, False)],
    "W o A o M": [("M", 0, False), "A", ("W", 0, False)],
    "0.75 * (W o A)": ["A", ("W", 0, False), ("s", 0.75, "r")],
    "W2 o W1 o A": ["A", ("W", 0, False), ("W", 1, True)],
    "Wb o A": ["A", ("Wb", 0, False)],
}
TOL = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-10, np.dtype(np.complex64): 1e-4, np.dtype(np.complex128): 1e-10}


def _host_ops(rig, toks, dt64):
    """matvec / rmatvec of the chain in fp64 on host copies of A's rows, the weights and the domain diagonals."""
    nrow, n = rig.nrow, rig.n
    cj = np.conj

    def row(i, x, adj):
        b = rig.ora[i][0]
        if b.kind == "zero":
            return np.zeros(n, dt64)
        if b.kind == "identity":
            return x.copy()
        if b.kind == "scale":
            a = b.scale if np.dtype(dt64).kind == "c" else b.scale.real
            return (cj(a) if adj else a) * x
        c = b.coeff.astype(dt64)
        return (cj(c) if adj != b.adjoint else c) * x

    def wb(k, i, x, adj):
        if i % 4 == 3:
            return x.copy()
        if i % 7 == 5:
            return np.zeros(n, dt64)
        c = rig.hw[k][i].astype(dt64)
        return (cj(c) if (i % 3 == 1) != adj else c) * x

    def apply(tok, cur, adj):
        if tok == "A":
            return [row(i, cur[0], False) for i in range(nrow)] if not adj else [sum(row(i, cur[i], True) for i in range(nrow))]
        kind = tok[0]
        if kind == "W":
            return [(cj(w) if tok[2] != adj else w).astype(dt64) * x for w, x in zip(rig.hw[tok[1]], cur)]
        if kind == "Wb":
            return [wb(tok[1], i, x, tok[2] != adj) for i, x in enumerate(cur)]
        if kind == "M":
            c = rig.hc[tok[1]].astype(dt64)
            return [(cj(c) if tok[2] != adj else c) * cur[0]]
        if kind == "s":
            return [tok[1] * x for x in cur]
        raise ValueError(tok)

    def matvec(x):
        cur = [np.asarray(x, dt64)]
        for t in toks:
            cur = apply(t, cur, False)
        return np.concatenate(cur)

    def rmatvec(y):
        cur = list(np.split(np.asarray(y, dt64), nrow))
        for t in reversed(toks):
            cur = apply(t, cur, True)
        return cur[0]

    return matvec, rmatvec


def _setup(J, oracle, dt, name, nrow=6, n=4096 + 17, kinds="diag"):
    rig = Rig(J, oracle, dt, nrow, n, kinds)
    L = rig.compose(CHAINS[name])
    hb = np.concatenate([u01(oracle, dt, 61, i, n) for i in range(nrow)]) - dt(0.5)
    return rig, L, hb.astype(dt)


def _x(res):
    return res.x.to_numpy().ravel(order="F")


def _run(J, solver, L, hb, **kw):
    b = J.from_numpy(hb, J.range(L))
    f = {"lsqr": J.lsqr, "cgls": J.cgls, "cgnr": J.cgnr}[solver]
    if solver == "lsqr":
        kw.setdefault("conlim", 0.0)
    return f(L, b, atol=0.0, btol=0.0, **kw)


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64])
@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("solver", ["lsqr", "cgls", "cgnr"])
def test_native_chain_solvers_match_the_fp64_cpu_solvers(Jets, oracle, dt, name, solver):
    from jets_jl_amd import chains

    J = Jets
    rig, L, hb = _setup(J, oracle, dt, name, kinds="diag" if name != "Wb o A" else "mixed")
    dt64 = np.complex128 if np.dtype(dt).kind == "c" else np.float64
    matvec, rmatvec = _host_ops(rig, CHAINS[name], dt64)
    iters = 10
    before = chains.STATS["chain_solve_calls"]
    res = _run(J, solver, L, hb, maxiter=iters)
    assert chains.STATS["chain_solve_calls"] == before + 1, f"{solver} on {name}: the native chain solve did not run"
    ref = lsqr_fp64 if solver == "lsqr" else cgls_fp64
    kw = dict(conlim=0.0) if solver == "lsqr" else {}
    xr, info = ref(matvec, rmatvec, hb.astype(dt64), rig.n, atol=0.0, btol=0.0, maxiter=iters, **kw)
    assert res.itn == iters == info["itn"]
    x = _x(res).astype(dt64)
    tol = TOL[np.dtype(dt)] * (10 if solver == "cgnr" else 1)          # (CGNR: the residual by recurrence, accuracy with cond^2)
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) < tol, f"{solver} on {name}"
    rig.close()


@pytest.mark.parametrize("solver", ["lsqr", "cgls", "cgnr"])
@pytest.mark.parametrize("case", ["damp", "x0", "vec"])
def test_damp_warm_start_and_vec(Jets, oracle, solver, case):
    from jets_jl_amd import chains

    J = Jets
    dt, name = np.float64, "W o A o M"
    rig, L, hb = _setup(J, oracle, dt, name)
    matvec, rmatvec = _host_ops(rig, CHAINS[name], np.float64)
    iters = 12
    kw, rkw = {}, {}
    if case == "damp":
        kw = rkw = dict(damp=0.3)
    elif case == "x0":
        hx0 = u01(oracle, dt, 62, 0, rig.n) - 0.5
        kw, rkw = dict(x0=J.from_numpy(hx0, J.domain(L))), dict(x0=hx0)
    before = chains.STATS["chain_solve_calls"]
    if case == "vec":
        b = J.from_numpy(hb, J.range(L))
        f = {"lsqr": J.lsqr, "cgls": J.cgls, "cgnr": J.cgnr}[solver]
        res = f(J.vec_op(L), b, atol=0.0, btol=0.0, maxiter=iters, **(dict(conlim=0.0) if solver == "lsqr" else {}))
    else:
        res = _run(J, solver, L, hb, maxiter=iters, **kw)
    assert chains.STATS["chain_solve_calls"] == before + 1
    ref = lsqr_fp64 if solver == "lsqr" else cgls_fp64
    xr, _ = ref(matvec, rmatvec, hb, rig.n, atol=0.0, btol=0.0, maxiter=iters, **(dict(conlim=0.0) if solver == "lsqr" else {}), **rkw)
    assert np.linalg.norm(_x(res) - xr) / np.linalg.norm(xr) < 1e-9, f"{solver}, {case}"
    rig.close()


@pytest.mark.parametrize("dt", [np.float32, np.complex128])
@pytest.mark.parametrize("kinds", ["diag", "mixed"])
@pytest.mark.parametrize("solver", ["lsqr", "cgls", "cgnr"])
def test_native_vs_python_loop_vs_todays_route(Jets, oracle, monkeypatch, dt, kinds, solver):
    """The native chain solve, the Python loop on the chain step / NORMAL chain (JETS_*_NATIVE=0) and today's route (JETS_CHAIN_STEP=0: the chain into a
    range temporary, then the ADJOINT chain) reach the same x; the counters say which route each took."""
    from jets_jl_amd import chains

    J = Jets
    rig, L, hb = _setup(J, oracle, dt, "W o A o M", nrow=18, n=2051, kinds=kinds)
    iters = 8
    native_env = "JETS_LSQR_NATIVE" if solver == "lsqr" else "JETS_CGLS_NATIVE"
    s0 = dict(chains.STATS)
    x_nat = _x(_run(J, solver, L, hb, maxiter=iters))
    assert chains.STATS["chain_solve_calls"] == s0["chain_solve_calls"] + 1
    monkeypatch.setenv(native_env, "0")
    s1 = dict(chains.STATS)
    x_py = _x(_run(J, solver, L, hb, maxiter=iters))
    assert chains.STATS["chain_solve_calls"] == s1["chain_solve_calls"]
    if solver == "lsqr":
        assert chains.STATS["chain_step_calls"] >= s1["chain_step_calls"] + iters   # lsqr_core on the one-pass chain step
    elif solver == "cgnr":
        assert chains.STATS["chain_calls"] <= s1["chain_calls"] + 1             # A'b once; L'L through the NORMAL chain's hook, not the planner's runs
    else:
        assert chains.STATS["chain_calls"] > s1["chain_calls"]                  # cgls_core's textbook halves on the planner's chains
    monkeypatch.setenv("JETS_CHAIN_STEP", "0")
    monkeypatch.delenv(native_env)
    s2 = dict(chains.STATS)
    x_old = _x(_run(J, solver, L, hb, maxiter=iters))
    assert chains.STATS["chain_solve_calls"] == s2["chain_solve_calls"] and chains.STATS["chain_step_calls"] == s2["chain_step_calls"]
    assert chains.STATS["chain_calls"] > s2["chain_calls"]                      # today's route: the planner's FORWARD / ADJOINT chains
    tol = 1e-4 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else 1e-10
    for what, x in (("python loop", x_py), ("today's route", x_old)):
        assert np.linalg.norm(x - x_nat) / np.linalg.norm(x_nat) < tol, f"{solver}: native vs {what}"
    rig.close()


@pytest.mark.parametrize("solver", ["lsqr", "cgls", "cgnr"])
def test_declined_chain_still_solves_on_the_old_route(Jets, oracle, solver):
    """Three range-side stages: R + R^H exceed one list, jh_*_solve_chain declines before touching anything and the generic loop solves."""
    from jets_jl_amd import chains

    J = Jets
    dt = np.float64
    toks = ["A", ("W", 0, False), ("s", 2.0, "r"), ("W", 1, False)]
    rig = Rig(J, oracle, dt, 5, 1024, "diag")
    L = rig.compose(toks)
    hb = np.concatenate([u01(oracle, dt, 63, i, 1024) for i in range(5)]) - 0.5
    matvec, rmatvec = _host_ops(rig, toks, np.float64)
    before = dict(chains.STATS)
    res = _run(J, solver, L, hb, maxiter=8)
    assert chains.STATS["chain_solve_calls"] == before["chain_solve_calls"]
    assert chains.STATS["chain_step_calls"] == before["chain_step_calls"]
    ref = lsqr_fp64 if solver == "lsqr" else cgls_fp64
    xr, _ = ref(matvec, rmatvec, hb, 1024, atol=0.0, btol=0.0, maxiter=8, **(dict(conlim=0.0) if solver == "lsqr" else {}))
    assert np.linalg.norm(_x(res) - xr) / np.linalg.norm(xr) < 1e-9
    rig.close()
