"""GPU parity: a row partition whose local operator is a WEIGHTED N x K grid, L = W o A or W o A o M, with the knobs grid_chain_range = 1 and
grid_chain_step = 1 (rowpart._ShardChains, _pipelined_routes, TeamOp): adjoint(L), L'L and the Golub-Kahan step of L run as ranged grid chains
(jh_chain_apply_range / jh_chain_bidiag_step_range over positions inside a block), the K pieces of a finished range exchanged under the next
range's kernel.

(a) one rank, AbiComm, the exchange forced (BENCH_FORCE_DIST=1, JETS_AR_CHUNKS=4): the shard's adjoint, L'L and step have the bits of the unsharded
    fused grid-chain calls under adj_split = 0; LSQR / CGLS / CGNR on the shard agree with the knob-0 route within the 1e-3 of
    tests/test_gpu_grid_range_rowpart.py and allocate no range-sized temporary.
(b) a team of two contexts on the one GPU, five rows split 3 + 2: every member's result is the members' whole-vector results added in rank order."""
import ctypes as C
import gc

import numpy as np
import pytest

from .helpers import assert_bits_equal, u01
from .test_gpu_grid_range_rowpart import _grid
from .test_gpu_grid_step import _flat, _normsq64

pytestmark = pytest.mark.gpu

NCHUNKS = 4


def _weighted(J, oracle, dt, A, with_m, seed, row0=0):
    """L = W o A (o M): W = 0.5 + U[0, 1) on the range (by global row), M = 0.75 + 0.5 U[0, 1) on the domain."""
    nrow, ncol = A.jet.s["ops"].shape
    n = J.domain(A).length() // ncol
    hw = np.concatenate([0.5 + u01(oracle, dt, seed, row0 + i, n) for i in range(nrow)]).astype(dt)
    L = J.compose(J.JopDiagonal(J.from_numpy(hw, J.range(A))), A)
    if with_m:
        hm = np.concatenate([0.75 + 0.5 * u01(oracle, dt, seed + 1, k, n) for k in range(ncol)]).astype(dt)
        L = J.compose(L, J.JopDiagonal(J.from_numpy(hm, J.domain(A))))
    return L


@pytest.fixture
def forced_exchange(Jets, monkeypatch):
    """One rank over the C ABI's communicator with the exchange forced, both knobs at 1 and the ordered row walk."""
    monkeypatch.setenv("BENCH_FORCE_DIST", "1")
    monkeypatch.setenv("JETS_AR_CHUNKS", str(NCHUNKS))
    comm = Jets.rowpart.AbiComm(nranks=1, rank=0)
    Jets.tune(grid_chain_range=1, grid_chain_step=1, adj_split=0)
    try:
        yield comm
    finally:
        Jets.tune(grid_chain_range=0, grid_chain_step=0, adj_split=-1)
        comm.close()


@pytest.mark.parametrize("n", [4096, 515])
@pytest.mark.parametrize("with_m", [False, True])
def test_a_weighted_sharded_grid_applies_range_by_range_with_the_unsharded_bits(Jets, oracle, forced_exchange, n, with_m):
    from jets_jl_amd import chains

    J = Jets
    dt, nrow, ncol = np.float32, 6, 3
    A = _grid(J, oracle, dt, nrow, ncol, (n,), seed=71)
    L = _weighted(J, oracle, dt, A, with_m, seed=61)
    R, D = J.range(L), J.domain(L)
    shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=forced_exchange)
    assert shard.chain_step and shard.fused_normal and shard._chains.grid_n == n
    nranges = len(list(J.rowpart._grid_chunk_bounds(n, NCHUNKS)))
    assert nranges >= 2
    v, d = J.rand(D, seed=72, stream=0), J.rand(R, seed=73, stream=0)
    dirty = _flat(J.rand(D, seed=74, stream=0)).copy()
    sentinel = lambda: J.from_numpy(dirty, D)
    sc = chains.SolverChains(L)                                                  # the unsharded fused grid chains
    assert sc.fwd is not None and sc.fwd.grid
    # adjoint(L)
    want = J.mul_(sentinel(), L.H, d)
    before = (chains.STATS["grid_range_calls"], chains.STATS["grid_chain_calls"])
    got = shard.mul_adj_(sentinel(), d, force_collective=True)
    assert chains.STATS["grid_range_calls"] == before[0] + nranges and chains.STATS["grid_chain_calls"] == before[1] + nranges
    assert_bits_equal(_flat(got), _flat(want), "mul_adj_ of the shard vs the fused ADJOINT grid chain")
    # L'L
    want = J.mul_(sentinel(), J.compose(L.H, L), v)
    before = chains.STATS["grid_range_calls"]
    got = shard.normal_mul_(sentinel(), v, force_collective=True)
    assert chains.STATS["grid_range_calls"] == before + nranges
    assert_bits_equal(_flat(got), _flat(want), "normal_mul_ of the shard vs the fused NORMAL grid chain")
    # the one-pass step
    hu0 = _flat(d).copy()
    u1, w1 = J.from_numpy(hu0, R), sentinel()
    nrm1 = sc.step(u1, v, w1, 0.75, -0.5)
    assert nrm1 is not None
    u2, w2 = J.from_numpy(hu0, R), sentinel()
    before = chains.STATS["grid_range_calls"]
    nrm2 = shard.bidiag_step_(u2, v, w2, 0.75, -0.5, force_collective=True)
    assert chains.STATS["grid_range_calls"] == before + nranges
    assert_bits_equal(_flat(u2), _flat(u1), "bidiag_step_ of the shard: u")
    assert_bits_equal(_flat(w2), _flat(w1), "bidiag_step_ of the shard: w")
    assert nrm2 == pytest.approx(_normsq64(_flat(u1)), rel=1e-12, abs=0.0)
    # knob 0: the previous path -- no grid chain planned, the routes fall back
    J.tune(grid_chain_range=0)
    try:
        assert not shard.chain_step
        before = chains.STATS["grid_range_calls"]
        assert shard.bidiag_step_(J.from_numpy(hu0, R), v, sentinel(), 0.75, -0.5, force_collective=True) is None
        got = shard.mul_adj_(sentinel(), d, force_collective=True)
        assert chains.STATS["grid_range_calls"] == before
        assert_bits_equal(_flat(got), _flat(J.mul_(sentinel(), L.H, d)), "knob 0: the unpipelined adjoint")
    finally:
        J.tune(grid_chain_range=1)
    sc.close()
    shard.close()
    J.close(A)


def _solve_on(J, solver, shard, L, b, iters):
    kw = {} if solver == "cgnr" else {"overwrite_b": True}
    return getattr(J, solver)(shard, J.copyto_(J.zeros(J.range(L)), b), atol=0.0, btol=0.0, maxiter=iters, **kw)


@pytest.mark.parametrize("solver", ["lsqr", "cgls", "cgnr"])
def test_solvers_on_a_weighted_sharded_grid_agree_with_the_knob_0_route(Jets, oracle, forced_exchange, solver):
    """10 iterations on W o A and W o A o M at 6 x 3 of 4096 and of 515 against the same shard with the knob at 0 (an engine built then has no
    `normal` hook and no chain step: the route of a build without the feature) (the two routes sum ||u||^2 in different
    orders: 1e-7 .. 5e-7 relative in Float32, far inside the 1e-3 for solutions).  Then blocks of 4 MiB -- a range vector of 24 MiB: the slab
    cache, which keeps every freed vector of >= 16 MiB, holds nothing after the solve: no range-sized temporary."""
    from jets_jl_amd import chains

    J = Jets
    dt, nrow, ncol = np.float32, 6, 3
    for shape, iters, with_m in (((4096,), 10, False), ((4096,), 10, True), ((515,), 10, False), ((515,), 10, True), ((128, 128, 64), 4, True)):
        A = _grid(J, oracle, dt, nrow, ncol, shape, seed=75)
        L = _weighted(J, oracle, dt, A, with_m, seed=63)
        b = L * J.rand(J.domain(L), seed=76, stream=0)
        shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=forced_exchange)
        assert shard.chain_step and shard.fused_normal
        J.tune(grid_chain_range=0)
        try:
            before = chains.STATS["grid_range_calls"]
            x0 = _flat(_solve_on(J, solver, shard, L, b, iters).x).astype(np.float64)
            assert chains.STATS["grid_range_calls"] == before, "knob 0: no ranged grid-chain call"
        finally:
            J.tune(grid_chain_range=1)
        rhs = J.copyto_(J.zeros(J.range(L)), b)
        kw = {} if solver == "cgnr" else {"overwrite_b": True}
        gc.collect()
        J.synchronize()
        J.trim()
        before = chains.STATS["grid_range_calls"]
        res = getattr(J, solver)(shard, rhs, atol=0.0, btol=0.0, maxiter=iters, **kw)
        calls = chains.STATS["grid_range_calls"] - before
        xs, itn = _flat(res.x).astype(np.float64), res.itn
        del res
        gc.collect()
        J.synchronize()
        cached = J.tune_get("slab_cached_mib")
        J.trim()
        nranges = len(list(J.rowpart._grid_chunk_bounds(int(np.prod(shape)), NCHUNKS)))
        print(f"{solver} on a weighted sharded {nrow} x {ncol} grid of {shape}: itn {itn}, ranged calls {calls}, slab cache {cached} MiB, "
              f"vs knob 0 {np.linalg.norm(xs - x0) / np.linalg.norm(x0):.2e}")
        assert itn >= 4
        assert calls >= nranges * itn, "a ranged grid-chain application per iteration and range"
        assert cached < 16, "no vector of 16 MiB or more was allocated and freed by the solve: no range-sized temporary"
        assert np.linalg.norm(xs - x0) <= 1e-3 * np.linalg.norm(x0), f"{solver}: knob 1 vs knob 0"
        shard.close()
        J.close(A)


@pytest.mark.parametrize("solver", ["lsqr", "cgls", "cgnr"])
def test_a_knob_flipped_to_0_under_a_live_engine_falls_back(Jets, oracle, forced_exchange, solver):
    from jets_jl_amd import chains
    from jets_jl_amd.cgls import cgls_core, cgnr_core
    from jets_jl_amd.lsqr import _engine_for, lsqr_core

    J = Jets
    dt, nrow, ncol, iters = np.float32, 6, 3, 10
    A = _grid(J, oracle, dt, nrow, ncol, (515,), seed=92)
    L = _weighted(J, oracle, dt, A, False, seed=65)
    b = L * J.rand(J.domain(L), seed=93, stream=0)
    shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=forced_exchange)
    core = lambda eng, rhs: {"lsqr": lambda: lsqr_core(eng, rhs, None, 0.0, 0.0, 0.0, 1e8, iters), "cgls": lambda: cgls_core(eng, rhs, None, 0.0, 0.0, 0.0, iters),
                             "cgnr": lambda: cgnr_core(eng, rhs, None, 0.0, 0.0, 0.0, iters)}[solver]()
    eng, rhs, _ = _engine_for(shard, J.copyto_(J.zeros(J.range(L)), b), None)
    x1 = _flat(core(eng, rhs).x).astype(np.float64)
    eng, rhs, _ = _engine_for(shard, J.copyto_(J.zeros(J.range(L)), b), None)      # (built with the knob at 1, as a long-lived engine would be)
    assert eng.chain_step
    J.tune(grid_chain_range=0)
    try:
        before = chains.STATS["grid_range_calls"]
        res = core(eng, rhs)
        assert chains.STATS["grid_range_calls"] == before, "no ranged grid-chain call with the knob at 0"
        xs = _flat(res.x).astype(np.float64)
        assert res.itn >= 4 and np.linalg.norm(xs - x1) <= 1e-3 * np.linalg.norm(x1), f"{solver}: the fallback vs the ranged route"
    finally:
        J.tune(grid_chain_range=1)
    shard.close()
    J.close(A)


def test_a_team_of_two_contexts_runs_weighted_grids_range_by_range(Jets, oracle):
    from jets_jl_amd import rowpart
    from .test_gpu_contexts import _team_contexts

    J = Jets
    J.init(0)
    home = J.context_current()[0]
    ctxs, extra = _team_contexts(J, 2)
    team = rowpart.Team(ctxs)
    try:
        for n in (4096, 515):
            _team_flow(J, oracle, rowpart, team, n)
    finally:
        team.close()
        gc.collect()                                                 # the members' vectors and operators die before their contexts
        J.context_use(home)
        for c in extra:
            J.context_destroy(c)


def _team_flow(J, oracle, rowpart, team, n):
    from jets_jl_amd import chains

    T, scs, As = None, [], []
    knobs = dict(grid_chain_range=1, grid_chain_step=1, adj_split=0)
    try:
        dt, nrow, ncol = np.float32, 5, 3
        parts = [rowpart.partition_rows(nrow, 2, k) for k in range(2)]
        local_ops = []
        for k, _ in team.each():
            J.tune(**knobs)
            As.append(_grid(J, oracle, dt, parts[k].count, ncol, (n,), seed=81, row0=parts[k].first))
            local_ops.append(_weighted(J, oracle, dt, As[k], True, seed=67, row0=parts[k].first))
        T = team.operator(local_ops)
        assert T.chain_step and T.fused_normal
        hv = np.concatenate([u01(oracle, dt, 82, k, n) - dt(0.5) for k in range(ncol)]).astype(dt)
        hu = [u01(oracle, dt, 83, i, n) for i in range(nrow)]
        v = rowpart.TeamVec([J.from_numpy(hv, T.domain()) for _ in team.each()])
        mine = lambda k: np.concatenate(hu[parts[k].first:parts[k].first + parts[k].count])
        # every member's whole-vector fused grid-chain step on its own rows, added on the host in rank order in the element type
        sum_w, want_u, want_n = None, [], 0.0
        for k, _ in team.each():
            scs.append(chains.SolverChains(local_ops[k]))
            uk, wk = J.from_numpy(mine(k), T.ranges()[k]), J.zeros(T.domain())
            nk = scs[k].step(uk, v[k], wk, 0.75, -0.5)
            assert nk is not None
            want_u.append(_flat(uk).copy())
            sum_w = _flat(wk).copy() if sum_w is None else sum_w + _flat(wk)
            want_n += nk
        u = rowpart.TeamVec([J.from_numpy(mine(k), T.ranges()[k]) for k, _ in team.each()])
        w = team.zeros(T.domain())
        nranges = len(list(rowpart._grid_chunk_bounds(n, T.nchunks)))
        assert nranges >= 2
        before = chains.STATS["grid_range_calls"]
        nrm2 = T.bidiag_step_(u, v, w, 0.75, -0.5)
        assert nrm2 is not None and chains.STATS["grid_range_calls"] == before + nranges * 2
        for k, _ in team.each():
            assert_bits_equal(_flat(u[k]), want_u[k], f"team step on a weighted grid: rows of member {k}")
            assert_bits_equal(_flat(w[k]), sum_w, f"team step on a weighted grid: w of member {k} vs the members' steps summed in rank order")
        assert abs(nrm2 - want_n) <= 1e-12 * want_n
        # the knob is per context: members that disagree are an error before any member's u is touched
        for k, _ in team.each():
            J.tune(grid_chain_range=1 if k == 0 else 0)
        try:
            u2 = rowpart.TeamVec([J.from_numpy(mine(k), T.ranges()[k]) for k, _ in team.each()])
            with pytest.raises(ValueError, match="grid_chain_range differs"):
                T.bidiag_step_(u2, v, team.zeros(T.domain()), 0.75, -0.5)
            for k, _ in team.each():
                assert_bits_equal(_flat(u2[k]), mine(k), f"members disagree on the knob: u of member {k} untouched")
        finally:
            for k, _ in team.each():
                J.tune(grid_chain_range=1)
        # adjoint(L) and L'L range by range, the same sum
        for name, ranged in (("adjoint", T.mul_adj_), ("normal", T.normal_mul_)):
            x = u if name == "adjoint" else v
            want = None
            for k, _ in team.each():
                Lk = local_ops[k]
                ok = J.mul_(J.zeros(T.domain()), Lk.H if name == "adjoint" else J.compose(Lk.H, Lk), x[k])
                want = _flat(ok).copy() if want is None else want + _flat(ok)
            out = team.zeros(T.domain())
            before = chains.STATS["grid_range_calls"]
            ranged(out, x)
            assert chains.STATS["grid_range_calls"] == before + nranges * 2, name
            for k, _ in team.each():
                assert_bits_equal(_flat(out[k]), want, f"team {name} on a weighted grid: member {k}")
    finally:
        for k, _ in team.each():
            J.tune(grid_chain_range=0, grid_chain_step=0, adj_split=-1)
            if k < len(scs):
                scs[k].close()
        if T is not None:
            T.close()


def _stats_delta(chains, before):
    return {k: v - before[k] for k, v in chains.STATS.items() if v != before[k]}


@pytest.mark.parametrize("with_m", [False, True])
def test_a_shard_built_under_knob_0_follows_the_knob(Jets, oracle, forced_exchange, with_m):
    """The knob is read per application, also for the shard's NORMAL chain.  A shard built with the knobs at their defaults has an engine with no
    `normal` hook and no chain step -- the engine of a build without the feature: CGNR applies A and A' through a range vector -- and a shard
    built under knob 1 whose knob went back to 0 counts the same calls.  Turning the knob on afterwards puts CGNR on the ranged NORMAL grid chain
    and LSQR / CGLS on the ranged step."""
    from jets_jl_amd import chains
    from jets_jl_amd.lsqr import _ShardEngine

    J = Jets
    dt, nrow, ncol, n, iters = np.float32, 6, 3, 515, 10
    A = _grid(J, oracle, dt, nrow, ncol, (n,), seed=77)
    L = _weighted(J, oracle, dt, A, with_m, seed=69)
    b = L * J.rand(J.domain(L), seed=78, stream=0)
    built_on = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=forced_exchange)
    J.tune(grid_chain_range=0, grid_chain_step=0)
    try:
        shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=forced_exchange)
        for sh in (shard, built_on):
            eng = _ShardEngine(sh)
            assert not sh.fused_normal and not sh.chain_step and not sh.grid_range
            assert not hasattr(eng, "normal") and not eng.chain_step and not eng.grid_range, "knob 0: the engine of a build without the feature"
        deltas, xs0 = [], {}
        for sh in (shard, built_on):
            for solver in ("lsqr", "cgls", "cgnr"):
                before = dict(chains.STATS)
                xs0[solver] = _flat(_solve_on(J, solver, sh, L, b, iters).x).astype(np.float64)
                deltas.append((solver, _stats_delta(chains, before)))
        for (s1, d1), (s2, d2) in zip(deltas[:3], deltas[3:]):
            assert d1 == d2, f"{s1}: built under knob 0 {d1}, built under knob 1 then set to 0 {d2}"
            assert not any(k in d1 for k in ("grid_range_calls", "chain_range_calls", "chain_step_range_calls")), (s1, d1)
    finally:
        J.tune(grid_chain_range=1, grid_chain_step=1)
    assert shard.fused_normal and shard.chain_step, "the shard built under knob 0 follows the knob"
    nranges = len(list(J.rowpart._grid_chunk_bounds(n, NCHUNKS)))
    for solver in ("lsqr", "cgls", "cgnr"):
        before = chains.STATS["grid_range_calls"]
        res = _solve_on(J, solver, shard, L, b, iters)
        assert chains.STATS["grid_range_calls"] - before >= nranges * res.itn, f"{solver}: the ranged grid chains ran"
        xs = _flat(res.x).astype(np.float64)
        assert np.linalg.norm(xs - xs0[solver]) <= 1e-3 * np.linalg.norm(xs0[solver]), f"{solver}: knob 1 vs knob 0"
    shard.close()
    built_on.close()
    J.close(A)


def _team_knobs(J, team, **kw):
    for _ in team.each():
        J.tune(**kw)


def _team_solver_flow(J, oracle, rowpart, team, solver, shape, with_m, iters, check_slabs, nrow=6):
    from jets_jl_amd import chains
    from jets_jl_amd.cgls import cgls_core, cgnr_core
    from jets_jl_amd.lsqr import _engine_for, lsqr_core

    dt, ncol = np.float32, 3
    n = int(np.prod(shape))
    parts = [rowpart.partition_rows(nrow, 2, k) for k in range(2)]
    T = None
    try:
        _team_knobs(J, team, grid_chain_range=1, grid_chain_step=1, adj_split=0)
        local_ops = []
        for k, _ in team.each():
            Ak = _grid(J, oracle, dt, parts[k].count, ncol, shape, seed=85, row0=parts[k].first)
            local_ops.append(_weighted(J, oracle, dt, Ak, with_m, seed=87, row0=parts[k].first))
        T = team.operator(local_ops)
        assert T.chain_step and T.fused_normal
        hx = np.concatenate([u01(oracle, dt, 88, k, n) for k in range(ncol)]).astype(dt)
        b = rowpart.TeamVec([local_ops[k] * J.from_numpy(hx, T.domain()) for k, _ in team.each()])
        rhs = lambda: rowpart.TeamVec([J.copyto_(J.zeros(T.ranges()[k]), b[k]) for k, _ in team.each()])
        kw = {} if solver == "cgnr" else {"overwrite_b": True}
        solve = lambda: getattr(J, solver)(T, rhs(), atol=0.0, btol=0.0, maxiter=iters, **kw)
        x_of = lambda res: _flat(res.x[0]).astype(np.float64)
        nranges = len(list(rowpart._grid_chunk_bounds(n, T.nchunks)))
        # knob 0: the previous route
        _team_knobs(J, team, grid_chain_range=0, grid_chain_step=0)
        before = chains.STATS["grid_range_calls"]
        x0 = x_of(solve())
        assert chains.STATS["grid_range_calls"] == before, "knob 0: no ranged grid-chain call"
        _team_knobs(J, team, grid_chain_range=1, grid_chain_step=1)
        r = rhs()
        gc.collect()
        for _ in team.each():
            J.synchronize()
            J.trim()
        before = chains.STATS["grid_range_calls"]
        res = getattr(J, solver)(T, r, atol=0.0, btol=0.0, maxiter=iters, **kw)
        calls, itn, xs = chains.STATS["grid_range_calls"] - before, res.itn, x_of(res)
        del res
        gc.collect()
        cached = 0
        for _ in team.each():
            J.synchronize()
            cached = max(cached, J.tune_get("slab_cached_mib"))
            J.trim()
        print(f"team {solver}, {shape}, M {with_m}: itn {itn}, ranged calls {calls}, slab cache {cached} MiB, vs knob 0 {np.linalg.norm(xs - x0) / np.linalg.norm(x0):.2e}")
        assert itn >= 4 and calls >= 2 * nranges * itn, "a ranged grid-chain application per member, iteration and range"
        assert np.linalg.norm(xs - x0) <= 1e-3 * np.linalg.norm(x0), f"{solver}: knob 1 vs knob 0"
        if check_slabs:
            assert cached < 16, "no vector of 16 MiB or more was allocated and freed by the solve: no range-sized temporary"
        # the knob flipped to 0 under a live engine: every hook falls back, no wrong iterate
        eng, r2, _ = _engine_for(T, rhs(), None)
        assert eng.chain_step and getattr(eng, "normal", None) is not None
        _team_knobs(J, team, grid_chain_range=0)
        before = chains.STATS["grid_range_calls"]
        core = {"lsqr": lambda: lsqr_core(eng, r2, None, 0.0, 0.0, 0.0, 1e8, iters), "cgls": lambda: cgls_core(eng, r2, None, 0.0, 0.0, 0.0, iters),
                "cgnr": lambda: cgnr_core(eng, r2, None, 0.0, 0.0, 0.0, iters)}[solver]
        res = core()
        assert chains.STATS["grid_range_calls"] == before, "no ranged grid-chain call with the knob at 0"
        xf = x_of(res)
        assert res.itn >= 4 and np.linalg.norm(xf - x0) <= 1e-3 * np.linalg.norm(x0), f"{solver}: the fallback vs the knob-0 route"
    finally:
        _team_knobs(J, team, grid_chain_range=0, grid_chain_step=0, adj_split=-1)
        if T is not None:
            T.close()


@pytest.mark.parametrize("solver", ["lsqr", "cgls", "cgnr"])
def test_solvers_on_a_team_of_weighted_grids(Jets, oracle, solver):
    """10 iterations of LSQR / CGLS / CGNR on a team of two contexts, W o A and W o A o M at 6 x 3 (3 + 3 rows) of 4096 and of 515, against the
    knob-0 route; then 10 x 3 of 4 MiB blocks (a member's range vector: 20 MiB, a domain vector: 12 MiB) for the slab cache, which keeps freed
    vectors of >= 16 MiB; each time also the knob flipped to 0 under a live engine."""
    from jets_jl_amd import rowpart
    from .test_gpu_contexts import _team_contexts

    J = Jets
    J.init(0)
    home = J.context_current()[0]
    ctxs, extra = _team_contexts(J, 2)
    team = rowpart.Team(ctxs)
    try:
        for shape, with_m, iters, slabs, nrow in (((4096,), False, 10, False, 6), ((515,), True, 10, False, 6), ((4096,), True, 10, False, 6),
                                                  ((515,), False, 10, False, 6), ((128, 128, 64), True, 4, True, 10)):
            _team_solver_flow(J, oracle, rowpart, team, solver, shape, with_m, iters, slabs, nrow)
            gc.collect()
    finally:
        team.close()
        gc.collect()
        J.context_use(home)
        for c in extra:
            J.context_destroy(c)
