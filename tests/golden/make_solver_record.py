#!/usr/bin/env python3
"""What the native LSQR / CGLS / CGNR loops of jh_lsqr.hip answer, bit for bit (tests/golden/solver_record.json).

    python tests/golden/make_solver_record.py              # rewrites solver_record.json next to this script (needs an MI355X)
    python tests/golden/make_solver_record.py --stdout     # prints the same record of the library as built, writes nothing

The library is the one the package loads: jets.jl_amd/libjetship.so, or the file the environment variable JETSHIP_LIB names.

One case is one call of an `extern "C"` solver: the stopping rule and the iteration count, the six norms of jh_lsqr_result as hex floats, 16 hex
digits of the SHA-256 of history[0 : 2 itn], of every x and of every overwritten right-hand side, and (plain entry, tall operator) the read-out
last_lsqr_graph / last_cg_graph.
Every solver runs on every path its loops have: plain with the knob lsqr_graph = 0 (the host-driven loop) and with its default (the graph-replayed
device loop), `_partitioned` with force_dist = 1 and a one-rank communicator (the ranged pipelined exchange), `_team` over two contexts of the one
GPU (3 + 5 or 5 + 3 rows), `_chain` on the FORWARD tall chain W o A, and plain on an N x 2 grid of diagonals.  Shapes: 3 and 5 rows of 515 elements
(off the 16-byte pack grid), 3 rows of 49 667 = 3 * 16384 + 515 elements (four exchange ranges, the last of 515 elements); every element type.
Variants: (damp, warm start, maxiter) in the four rows of the orthogonal array over {0, 0.1} x {cold, warm} x {3, 20} -- every pair of values meets; 20
iterations run past one replay pair of the eight-iteration graph.  The cases are a covering list, not the product: per solver and path every type on a
small and on the ranged shape with the variants in turn, one early stop (atol = btol = 1e-3), one b = 0 (the arnorm == 0 return) and two force_maxiter runs on consistent systems: one far past convergence
(1000 iterations allowed: the loops leave when alpha or beta reaches zero, CGNR on the chain through its breakdown exit, istop = 6 with its itn--),
and one on an operator scaled by 1e154, where rho = sqrt(rhobar^2 + beta^2) is not finite in the first iteration: LSQR's istop = 6 exit with its
itn-- (no system of these sizes reaches that exit by underflow: a vector's squares vanish, and alpha or beta with them, before rhobar^2 does).
Refusals are recorded too, with their message and the vectors they must leave alone.

The record is made TWICE in one process and the two must agree; a case whose two runs differ is named under "nondeterministic" and left out of
the bit comparison (at most 5 % may be).  tests/test_gpu_solver_record.py replays the list against the library as built and requires equality,
so the record is regenerated only when a loop's arithmetic or call sequence changes ON PURPOSE -- with the library from BEFORE a change that
claims to keep both.
"""
from __future__ import annotations

import ctypes as C
import gc
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "solver_record.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DTYPES = ("float32", "float64", "complex64", "complex128")
SOLVERS = ("lsqr", "cgls", "cgnr")
PATHS = ("host", "graph", "dist", "team", "chain", "grid")
SHAPES = ((3, 515), (5, 515), (3, 49667))
# (damp, warm, maxiter, tol): the orthogonal array, then the early stop
VARIANTS = ((0.0, 0, 3, 0.0), (0.0, 1, 20, 0.0), (0.1, 0, 20, 0.0), (0.1, 1, 3, 0.0), (0.0, 0, 20, 1e-3))
FORCE_ITERS = 1000
HUGE = 1e154                                     # an operator of this scale: alpha^2 and beta^2 are finite, their sum is not


def cases():
    """A covering list, the same on every run.  Per solver and path: every element type on a small shape (3 and 5 rows in turn) and on the ranged shape,
    the four variants in turn (shifted from one solver and path to the next, so every variant meets every type and shape), then the early stop, b = 0 and
    the two forced runs."""
    out = []
    for k, (path, solver) in enumerate((p, s) for p in PATHS for s in SOLVERS):
        base = {"path": path, "solver": solver}
        for d, dt in enumerate(DTYPES):
            for j, (nrow, n) in enumerate((SHAPES[(d + k) % 2], SHAPES[2])):
                damp, warm, maxiter, tol = VARIANTS[(d + 2 * j + k) % 4]
                out.append(dict(base, nrow=nrow, n=n, dt=dt, kind="solve", damp=damp, warm=warm, maxiter=maxiter, tol=tol))
        damp, warm, maxiter, tol = VARIANTS[4]
        out.append(dict(base, nrow=SHAPES[k % 2][0], n=515, dt=DTYPES[k % 4], kind="solve", damp=damp, warm=warm, maxiter=maxiter, tol=tol))
        out.append(dict(base, nrow=SHAPES[(k + 1) % 2][0], n=515, dt=DTYPES[(k + 1) % 4], kind="zero", damp=0.0, warm=0, maxiter=3, tol=0.0))
        out.append(dict(base, nrow=3, n=515, dt="float32", kind="force", damp=0.0, warm=0, maxiter=FORCE_ITERS, tol=0.0))
        out.append(dict(base, nrow=3, n=515, dt="float64", kind="force", damp=0.0, warm=0, maxiter=5, tol=0.0, scale=HUGE))
    return out


def _host(rng, dt, n, lo=-1.0, hi=1.0):
    a = rng.uniform(lo, hi, n)
    if np.dtype(dt).kind == "c":
        a = a + 0.5j * rng.uniform(-1.0, 1.0, n)
    return a.astype(dt)


def _pattern(dt, n):
    """What a cold-start x holds before the call: fixed, non-zero (the solver zeroes it itself)."""
    a = (np.arange(n) % 7 + 1) * 0.125
    return (a - 1j * (a + 0.5)).astype(dt) if np.dtype(dt).kind == "c" else a.astype(dt)


def _digest(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()[:16]


def _bytes(v) -> bytes:
    return np.ascontiguousarray(v.to_numpy()).tobytes()


class Shard:
    """One operator in the current context: `nrow` diagonals of `n` elements (ncol = 2: an nrow x 2 grid of them; weighted: the FORWARD chain
    W o A), the handle the solvers take, and host copies of a right-hand side, a warm start and a solution to be consistent with."""

    def __init__(self, J, dt, nrow, n, seed, ncol=1, weighted=False, scale=1.0):
        from jets_jl_amd import chains, jetblock

        self.J, self.dt = J, np.dtype(dt).type
        rng = np.random.default_rng([seed, nrow, n, ncol, DTYPES.index(dt)])
        blk = J.JetSpace(self.dt, n)
        self.coeff = J.from_numpy(_host(rng, dt, nrow * ncol * n, 0.5, 1.5) * scale, J.JetBSpace([blk] * (nrow * ncol)))   # moduli in [0.5, 1.6] * scale: well conditioned
        self.A = J.blockop([[J.JopDiagonal(self.coeff.arrays[i * ncol + k]) for k in range(ncol)] for i in range(nrow)])
        self.L, self.cache, self.w = self.A, None, None
        if weighted:
            self.w = J.from_numpy(_host(rng, dt, J.range(self.A).length(), 0.5, 1.5), J.range(self.A))
            self.L = J.compose(J.JopDiagonal(self.w), self.A)
            self.cache = chains.ChainCache()
            h = chains.one_run(chains.stages_of(self.L), self.cache, "solver_record", chains.CHAIN_FORWARD)
            assert isinstance(h, chains.ChainHandle) and not h.grid, "W o A: not one fused tall run"
            self.handle = h.handle
        else:
            self.handle = jetblock._native_op(self.A.jet.s["_native"], self.A.jet.s["ops"], self.A.jet.rng.eltype()).handle
        self.R, self.D = J.range(self.L), J.domain(self.L)
        self.hb = _host(rng, dt, self.R.length())
        dom = np.random.default_rng([n, ncol, DTYPES.index(dt)])             # the domain side is the same in every member of a team
        self.hx0 = (_host(dom, dt, self.D.length()) * 0.1).astype(dt)
        self.hxt = _host(dom, dt, self.D.length()) / scale

    def vectors(self, c):
        """(u, x) of case `c`, fresh."""
        J = self.J
        hb = self.hb
        if c["kind"] == "zero":
            hb = np.zeros_like(hb)
        elif c["kind"] == "force":
            hb = (self.L * J.from_numpy(self.hxt, self.D)).to_numpy()       # consistent: b = L x_true, as the device rounds it
        hx = self.hx0 if c["warm"] else _pattern(self.dt, self.D.length())
        return J.from_numpy(hb, self.R), J.from_numpy(hx, self.D)

    def close(self):
        if self.cache is not None:
            self.cache.close()
        self.J.close(self.A)
        for v in (self.w, self.coeff):
            if v is not None:
                v.close()
        self.w = self.coeff = self.A = self.L = None


def _call(lib, c, entry, ops, us, xs, res, hist):
    """The solver's C call: LSQR takes conlim (0: no limit) between btol and maxiter."""
    fn = getattr(lib, f"jh_{c['solver']}_solve{entry}")
    tol = (c["tol"], c["tol"]) + ((0.0,) if c["solver"] == "lsqr" else ())
    head = (len(ops), _arr(ops), _arr(us), _arr(xs)) if entry == "_team" else (ops[0], us[0].handle, xs[0].handle)
    return fn(*head, c["warm"], c["damp"], *tol, c["maxiter"], 1 if c["kind"] == "force" else 0, C.byref(res), hist)


def _arr(hs):
    return (C.c_void_p * len(hs))(*[getattr(h, "handle", h).value for h in hs])


# the read-out the plain entry of a tall operator resets: replays of the graph (0: a host-driven loop ran); the other entries leave it alone
GRAPH_READOUT = {"lsqr": "last_lsqr_graph", "cgls": "last_cg_graph", "cgnr": "last_cg_graph"}
RESULT = ["istop", "itn", "graph read-out", ["r1norm", "r2norm", "anorm", "acond", "arnorm", "xnorm"], "history", ["x"], ["overwritten rhs"]]
ENTRY = {"host": "", "graph": "", "grid": "", "dist": "_partitioned", "team": "_team", "chain": "_chain"}


def run_case(J, c, shards, contexts):
    """One solve of case `c` on its shards (one, or a team's two, each in its context): what the record holds, RESULT."""
    from jets_jl_amd._ffi import LsqrResultC, check, lib

    us, xs = [], []
    for s, ctx in zip(shards, contexts):
        J.context_use(ctx)
        u, x = s.vectors(c)
        us.append(u)
        xs.append(x)
    J.context_use(contexts[0])
    res, hist = LsqrResultC(), (C.c_double * (2 * c["maxiter"]))()
    check(_call(lib, c, ENTRY[c["path"]], [s.handle for s in shards], us, xs, res, hist))
    out = [res.istop, res.itn, J.tune_get(GRAPH_READOUT[c["solver"]]) if c["path"] in ("host", "graph") else None,
           [float(getattr(res, f)).hex() for f in ("r1norm", "r2norm", "anorm", "acond", "arnorm", "xnorm")],
           _digest(bytes(hist)[:16 * res.itn]), [_digest(_bytes(x)) for x in xs], [_digest(_bytes(u)) for u in us]]
    for v in us + xs:
        v.close()
    return out


def _refusals(J, lib, team_shards, contexts):
    """Calls the loops must decline before they write anything: [name, status, message, vectors unchanged]."""
    from jets_jl_amd._ffi import LsqrResultC

    out = []
    c0 = {"kind": "solve", "warm": 1, "damp": 0.0, "tol": 0.0, "maxiter": 3}

    def attempt(name, solver, entry, ops, us, xs):
        before = [_bytes(v) for v in us + xs]
        res, hist = LsqrResultC(), (C.c_double * 6)()
        st = _call(lib, dict(c0, solver=solver), entry, ops, us, xs, res, hist)
        msg = lib.jh_last_error()
        assert st != 0, f"{name}: accepted"
        out.append({"name": name, "status": st, "message": msg.decode("utf-8", "replace") if msg else "",
                    "unchanged": before == [_bytes(v) for v in us + xs]})

    J.context_use(contexts[0])
    wide = Shard(J, "float32", 2, 515, 7, ncol=5)
    one = Shard(J, "float32", 1, 515, 8)
    for solver in SOLVERS:
        for name, s in (("wide operator", wide), ("one row", one)):
            if s is wide or solver != "lsqr":
                u, x = s.vectors(c0)
                attempt(f"{solver}: {name}", solver, "", [s.handle], [u], [x])
                u.close()
                x.close()
    wide.close()
    one.close()
    us, xs = [], []
    for s, ctx in zip(team_shards, contexts):
        J.context_use(ctx)
        u, x = s.vectors(c0)
        us.append(u)
        xs.append(x)
    J.context_use(contexts[1])
    longer = J.from_numpy(_pattern(np.float32, 516), J.JetSpace(np.float32, 516))
    hs = [s.handle for s in team_shards]
    for solver in SOLVERS:
        J.context_use(contexts[0])
        attempt(f"{solver}: team entry, members swapped", solver, "_team", hs[::-1], us[::-1], xs[::-1])
        attempt(f"{solver}: partitioned entry inside a team", solver, "_partitioned", hs[:1], us[:1], xs[:1])
        attempt(f"{solver}: team entry, member 1's x longer", solver, "_team", hs, us, [xs[0], longer])
    for v in us + xs + [longer]:
        v.close()
    J.context_use(contexts[0])
    return out


def replay(J, todo, refusals=True):
    """Run the cases `todo` path by path (operators are shared inside a path): ([result of every case], [refusals])."""
    from jets_jl_amd import rowpart
    from jets_jl_amd._ffi import lib

    J.init(0)
    home = J.context_current()[0]
    saved = {k: J.tune_get(k) for k in ("lsqr_graph", "force_dist")}
    out, refused = [None] * len(todo), []

    def run_path(path, make, contexts):
        shards = {}
        try:
            for i, c in enumerate(todo):
                if c["path"] == path:
                    key = (c["dt"], c["nrow"], c["n"], c.get("scale", 1.0))
                    if key not in shards:
                        shards[key] = make(*key)
                    out[i] = run_case(J, c, shards[key], contexts)
        finally:
            J.context_use(home)
            for group in shards.values():
                for s, ctx in zip(group, contexts):
                    J.context_use(ctx)
                    s.close()
            J.context_use(home)

    try:
        J.tune(lsqr_graph=0)
        run_path("host", lambda dt, nrow, n, scale: [Shard(J, dt, nrow, n, 1, scale=scale)], [home])
        J.tune(lsqr_graph=saved["lsqr_graph"])
        run_path("graph", lambda dt, nrow, n, scale: [Shard(J, dt, nrow, n, 1, scale=scale)], [home])
        run_path("chain", lambda dt, nrow, n, scale: [Shard(J, dt, nrow, n, 2, weighted=True, scale=scale)], [home])
        run_path("grid", lambda dt, nrow, n, scale: [Shard(J, dt, nrow, n, 3, ncol=2, scale=scale)], [home])
        comm = rowpart.AbiComm(nranks=1, rank=0)
        try:
            J.tune(force_dist=1)
            run_path("dist", lambda dt, nrow, n, scale: [Shard(J, dt, nrow, n, 1, scale=scale)], [home])
        finally:
            J.tune(force_dist=saved["force_dist"])
            comm.close()
        extra = J.context_create(0)
        contexts = [home, extra]
        team = rowpart.Team(contexts)
        try:
            def members(dt, nrow, n, scale=1.0):
                group = []
                for k, ctx in enumerate(contexts):
                    J.context_use(ctx)
                    group.append(Shard(J, dt, nrow if k == 0 else 8 - nrow, n, 4 + k, scale=scale))
                return group

            run_path("team", members, contexts)
            if refusals:
                group = members("float32", 3, 515)
                try:
                    refused = _refusals(J, lib, group, contexts)
                finally:
                    for s, ctx in zip(group, contexts):
                        J.context_use(ctx)
                        s.close()
                    del group
        finally:
            team.close()
            gc.collect()                                                  # the members' vectors and operators die before their contexts
            J.context_use(home)
            J.context_destroy(extra)
    finally:
        J.context_use(home)
        J.tune(**saved)
    return out, refused


def cases_digest(todo) -> str:
    return _digest(json.dumps(todo, sort_keys=True).encode())


def dumps(todo, results, refused, nondet) -> str:
    """The results in the order of cases(), whose digest the header holds: the parameters themselves are not repeated."""
    rows = ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in results)
    refs = ",\n".join("  " + json.dumps(r) for r in refused)
    return f'{{"result": {json.dumps(RESULT)},\n "cases_digest": "{cases_digest(todo)}",\n "nondeterministic": {json.dumps(nondet)},\n "refusals": [\n{refs}\n ],\n "cases": [\n{rows}\n ]}}\n'


if __name__ == "__main__":
    if sys.argv[1:] not in ([], ["--stdout"]):
        raise SystemExit(__doc__)
    import jets_jl_amd as J

    todo = cases()
    first, refused = replay(J, todo)
    second, refused2 = replay(J, todo)
    assert refused == refused2, "the refusals of two runs differ"
    nondet = [i for i, (a, b) in enumerate(zip(first, second)) if a != b]
    text = dumps(todo, first, refused, nondet)
    for i in nondet:
        print("differs between two runs:", todo[i], first[i], second[i], file=sys.stderr)
    if sys.argv[1:]:
        sys.stdout.write(text)
    else:
        with open(OUT, "w", encoding="utf-8") as f:
            f.write(text)
        print(f"{len(todo)} cases, {len(refused)} refusals, {len(nondet)} not deterministic -> {OUT}")
    assert 20 * len(nondet) <= len(todo), f"{len(nondet)} of {len(todo)} cases differ between two runs of one library: more than 5 %"
