"""GPU parity: a row partition whose local operator is an N x K GRID, with the knob grid_range = 1 (rowpart._pipelined_routes, TeamOp._ranged): the
ranges are cut over the block length, every range runs the grid's ranged kernel (jh_blockop_mul_adj_range / _normal_mul_range / _bidiag_step_range)
and the K pieces of a finished range are exchanged under the next range's kernel.

(a) one rank, AbiComm, the exchange forced (BENCH_FORCE_DIST=1, as tests/test_gpu_chain_step_range.py): the shard's adjoint, A'A and step have the
    unpartitioned operator's bits under adj_split = 0; LSQR / CGLS / CGNR on the shard iterate on the ranged calls, match the single-process solution
    within that file's 1e-3 and allocate no range-sized temporary.
(b) a team of two contexts on the one GPU, five rows split 3 + 2: every member's w is the members' whole-vector local results added in rank order in
    the element type (the same-device team sum adds the members in rank order), bit for bit."""
import ctypes as C
import gc

import numpy as np
import pytest

from .helpers import assert_bits_equal, u01
from .test_gpu_grid_step import _flat, _native, _normsq64

pytestmark = pytest.mark.gpu

NCHUNKS = 4


def _grid(J, oracle, dt, nrow, ncol, shape, seed, row0=0):
    """A well-conditioned grid of plain diagonals: block (i, k) = 0.2 U[0, 1) + (1 where i % K == k) -- A'A is close to a multiple of I."""
    n = int(np.prod(shape))
    spc = J.JetSpace(dt, *shape)
    return J.blockop([[J.JopDiagonal(J.from_numpy((0.2 * u01(oracle, dt, seed, 100 * (row0 + i) + k, n) + (1.0 if (row0 + i) % ncol == k else 0.0)).astype(dt), spc))
                       for k in range(ncol)] for i in range(nrow)])


@pytest.fixture
def forced_exchange(Jets, monkeypatch):
    """One rank over the C ABI's communicator with the exchange forced, grid_range = 1 and the ordered row walk."""
    monkeypatch.setenv("BENCH_FORCE_DIST", "1")
    monkeypatch.setenv("JETS_AR_CHUNKS", str(NCHUNKS))
    comm = Jets.rowpart.AbiComm(nranks=1, rank=0)
    Jets.tune(grid_range=1, adj_split=0)
    try:
        yield comm
    finally:
        Jets.tune(grid_range=0, adj_split=-1)
        comm.close()


def test_a_sharded_grid_applies_range_by_range_with_the_unpartitioned_bits(Jets, oracle, forced_exchange):
    from jets_jl_amd import chains
    from jets_jl_amd._ffi import lib

    J = Jets
    dt, nrow, ncol, n = np.float32, 6, 3, 4096
    A = _grid(J, oracle, dt, nrow, ncol, (n,), seed=71)
    nat = _native(A)
    shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), A, comm=forced_exchange)
    assert shard.grid_range
    v = J.rand(J.domain(A), seed=72, stream=0)
    d = J.rand(J.range(A), seed=73, stream=0)
    dirty = _flat(J.rand(J.domain(A), seed=74, stream=0)).copy()
    sentinel = lambda: J.from_numpy(dirty, J.domain(A))
    # the adjoint
    want = sentinel()
    assert lib.jh_blockop_mul_adj(nat.handle, want.handle, d.handle) == 0
    before = chains.STATS["grid_range_calls"]
    got = shard.mul_adj_(sentinel(), d, force_collective=True)
    assert chains.STATS["grid_range_calls"] == before + NCHUNKS
    assert_bits_equal(_flat(got), _flat(want), "mul_adj_ of the shard vs jh_blockop_mul_adj")
    # the fused A'A
    want = sentinel()
    assert lib.jh_blockop_normal_mul(nat.handle, want.handle, v.handle) == 0
    before = chains.STATS["grid_range_calls"]
    got = shard.normal_mul_(sentinel(), v, force_collective=True)
    assert chains.STATS["grid_range_calls"] == before + NCHUNKS
    assert_bits_equal(_flat(got), _flat(want), "normal_mul_ of the shard vs jh_blockop_normal_mul")
    # the one-pass step
    hu0 = _flat(d).copy()
    u1, w1, out = J.from_numpy(hu0, J.range(A)), sentinel(), C.c_double(-1.0)
    assert lib.jh_blockop_bidiag_step(nat.handle, u1.handle, v.handle, w1.handle, 0.75, -0.5, C.byref(out)) == 0
    u2, w2 = J.from_numpy(hu0, J.range(A)), sentinel()
    before = chains.STATS["grid_range_calls"]
    nrm2 = shard.bidiag_step_(u2, v, w2, 0.75, -0.5, force_collective=True)
    assert chains.STATS["grid_range_calls"] == before + NCHUNKS
    assert_bits_equal(_flat(u2), _flat(u1), "bidiag_step_ of the shard: u")
    assert_bits_equal(_flat(w2), _flat(w1), "bidiag_step_ of the shard: w")
    assert nrm2 == pytest.approx(_normsq64(_flat(u1)), rel=1e-12, abs=0.0)
    # knob 0: today's path -- the library declines the first range, the routes fall back
    J.tune(grid_range=0)
    try:
        assert not shard.grid_range
        before = chains.STATS["grid_range_calls"]
        assert shard.bidiag_step_(J.from_numpy(hu0, J.range(A)), v, sentinel(), 0.75, -0.5, force_collective=True) is None
        got = shard.mul_adj_(sentinel(), d, force_collective=True)
        assert chains.STATS["grid_range_calls"] == before
        assert lib.jh_blockop_mul_adj(nat.handle, want.handle, d.handle) == 0
        assert_bits_equal(_flat(got), _flat(want), "knob 0: the unpipelined adjoint")
    finally:
        J.tune(grid_range=1)
    shard.close()
    J.close(A)


@pytest.mark.parametrize("solver", ["lsqr", "cgls", "cgnr"])
def test_solvers_on_a_sharded_grid_iterate_on_the_ranged_calls(Jets, oracle, forced_exchange, solver):
    """Exactly JETS_AR_CHUNKS x (itn + 1) ranged calls: JETS_AR_CHUNKS per iteration (LSQR and CGLS: the step; CGNR: A'A) -- the count the ranged route
    is there for -- and one more application, the ranged adjoint for the A'b every one of the three solvers starts with; an iteration that fell back to
    the generic route would be missing from the count.  The single-process solution within 1e-3.  Then blocks of 4 MiB -- a range vector of 24 MiB,
    domain vectors of 12 MiB: the slab cache, which keeps every freed vector of >= 16 MiB, holds nothing after the solve: no range-sized temporary
    beyond u (b's storage) -- while the same solve with the knob at 0 leaves its range temporary there (the check can see one)."""
    from jets_jl_amd import chains

    J = Jets
    dt, nrow, ncol = np.float32, 6, 3
    solve = getattr(J, solver)
    kw = {} if solver == "cgnr" else {"overwrite_b": True}
    for shape, iters in (((4096,), 12), ((128, 128, 64), 4)):
        A = _grid(J, oracle, dt, nrow, ncol, shape, seed=75)
        x_true = J.rand(J.domain(A), seed=76, stream=0)
        b = A * x_true
        single = solve(A, J.copyto_(J.zeros(J.range(A)), b), atol=0.0, btol=0.0, maxiter=iters)
        x1, xt = _flat(single.x).astype(np.float64), _flat(x_true).astype(np.float64)
        del single
        shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), A, comm=forced_exchange)
        assert shard.grid_range
        rhs = J.copyto_(J.zeros(J.range(A)), b)
        gc.collect()
        J.synchronize()
        J.trim()
        before = chains.STATS["grid_range_calls"]
        res = solve(shard, rhs, atol=0.0, btol=0.0, maxiter=iters, **kw)
        calls = chains.STATS["grid_range_calls"] - before
        xs, itn = _flat(res.x).astype(np.float64), res.itn
        del res
        gc.collect()
        J.synchronize()
        cached = J.tune_get("slab_cached_mib")
        J.trim()
        print(f"{solver} on a sharded {nrow} x {ncol} grid of {shape}: itn {itn}, ranged calls {calls}, slab cache {cached} MiB, "
              f"vs single {np.linalg.norm(xs - x1) / np.linalg.norm(x1):.2e}, vs true {np.linalg.norm(xs - xt) / np.linalg.norm(xt):.2e}")
        assert itn >= 4
        assert calls == NCHUNKS * (itn + 1), "JETS_AR_CHUNKS ranged calls per iteration, and the A'b before the first"
        assert cached < 16, "no vector of 16 MiB or more was allocated and freed by the solve: no range-sized temporary"
        assert np.linalg.norm(xs - x1) <= 1e-3 * np.linalg.norm(x1), f"{solver}: shard vs single process"
        range_mib = nrow * int(np.prod(shape)) * 4 >> 20
        if range_mib >= 16:                                              # the positive control: knob 0 is the route through a range temporary
            J.tune(grid_range=0)
            try:
                rhs = J.copyto_(rhs, b)
                before = chains.STATS["grid_range_calls"]
                res = solve(shard, rhs, atol=0.0, btol=0.0, maxiter=iters, **kw)
                x0 = _flat(res.x).astype(np.float64)
                del res
                gc.collect()
                J.synchronize()
                cached = J.tune_get("slab_cached_mib")
                J.trim()
                print(f"{solver}, knob 0: slab cache {cached} MiB (a range vector: {range_mib} MiB)")
                assert chains.STATS["grid_range_calls"] == before, "knob 0: no ranged call"
                assert cached >= range_mib, "the route through the range temporary allocates it (this check sees it)"
                assert np.linalg.norm(x0 - x1) <= 1e-3 * np.linalg.norm(x1), f"{solver}: knob 0 vs single process"
            finally:
                J.tune(grid_range=1)
        shard.close()
        J.close(A)


@pytest.mark.parametrize("solver", ["lsqr", "cgls", "cgnr"])
@pytest.mark.parametrize("case", ["dense blocks", "one exchange range", "knob back at 0"])
def test_solvers_fall_back_where_the_ranged_calls_decline(Jets, oracle, forced_exchange, monkeypatch, solver, case):
    """Knob 1 must run whatever knob 0 ran.  The host takes any native N x (2 .. 4) operator of equal block lengths for a grid and leaves the rest to the
    library, which declines before anything is touched: a 2 x 2 grid of DENSE children; a valid grid with JETS_AR_CHUNKS=1 (no pipelined route at
    all); a shard used after the knob went back to 0.  The solvers then take the generic passes -- the single-process solution within 1e-3, no
    ranged call counted."""
    from jets_jl_amd import chains

    J = Jets
    dt, n, iters = np.float32, 64, 8
    if case == "dense blocks":
        nrow = 2
        mats = [[(np.eye(n) * (1.0 if i == k else 0.25) + 0.05 * u01(oracle, dt, 91, 10 * i + k, n * n).reshape(n, n)).astype(dt) for k in range(2)] for i in range(2)]
        A = J.blockop([[J.JopDense(J.from_numpy(mats[i][k])) for k in range(2)] for i in range(2)])
    else:
        nrow = 6
        A = _grid(J, oracle, dt, nrow, 3, (4096,), seed=92)
    if case == "one exchange range":
        monkeypatch.setenv("JETS_AR_CHUNKS", "1")
    solve = getattr(J, solver)
    x_true = J.rand(J.domain(A), seed=93, stream=0)
    b = A * x_true
    single = solve(A, J.copyto_(J.zeros(J.range(A)), b), atol=0.0, btol=0.0, maxiter=iters)
    x1 = _flat(single.x).astype(np.float64)
    shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), A, comm=forced_exchange)
    assert shard.grid_range, "the host cannot tell: the library declines"
    from jets_jl_amd.cgls import cgls_core, cgnr_core
    from jets_jl_amd.lsqr import _engine_for, lsqr_core

    eng, rhs, _ = _engine_for(shard, J.copyto_(J.zeros(J.range(A)), b), None)      # (built with the knob at 1, as a long-lived engine would be)
    assert eng.grid_range
    if case == "knob back at 0":
        J.tune(grid_range=0)
    try:
        before = chains.STATS["grid_range_calls"]
        core = {"lsqr": lambda: lsqr_core(eng, rhs, None, 0.0, 0.0, 0.0, 1e8, iters), "cgls": lambda: cgls_core(eng, rhs, None, 0.0, 0.0, 0.0, iters),
                "cgnr": lambda: cgnr_core(eng, rhs, None, 0.0, 0.0, 0.0, iters)}[solver]
        res = core()
        xs = _flat(res.x).astype(np.float64)
        assert chains.STATS["grid_range_calls"] == before, "every ranged call was declined on its first range"
        assert res.itn >= 4
        assert np.linalg.norm(xs - x1) <= 1e-3 * np.linalg.norm(x1), f"{solver}, {case}: shard vs single process"
    finally:
        J.tune(grid_range=1)
    shard.close()
    J.close(A)


def test_a_team_of_two_contexts_steps_a_grid_range_by_range(Jets, oracle):
    from jets_jl_amd import rowpart
    from .test_gpu_contexts import _team_contexts

    J = Jets
    J.init(0)
    home = J.context_current()[0]
    ctxs, extra = _team_contexts(J, 2)
    team = rowpart.Team(ctxs)
    try:
        _team_grid_flow(J, oracle, rowpart, team)
    finally:
        team.close()
        gc.collect()                                                 # the members' vectors and operators die before their contexts
        J.context_use(home)
        for c in extra:
            J.context_destroy(c)


def _team_grid_flow(J, oracle, rowpart, team):
    from jets_jl_amd import chains
    from jets_jl_amd._ffi import lib

    T = None
    try:
        dt, nrow, ncol, n = np.float32, 5, 2, 515
        parts = [rowpart.partition_rows(nrow, 2, k) for k in range(2)]
        assert [p.count for p in parts] == [3, 2]
        local_ops = []
        for k, _ in team.each():
            J.tune(grid_range=1, adj_split=0)
            local_ops.append(_grid(J, oracle, dt, parts[k].count, ncol, (n,), seed=81, row0=parts[k].first))
        T = team.operator(local_ops)
        hv = np.concatenate([u01(oracle, dt, 82, k, n) - dt(0.5) for k in range(ncol)]).astype(dt)
        hu = [u01(oracle, dt, 83, i, n) for i in range(nrow)]
        v = rowpart.TeamVec([J.from_numpy(hv, T.domain()) for _ in team.each()])
        mine = lambda k: np.concatenate(hu[parts[k].first:parts[k].first + parts[k].count])
        # every member's whole-vector step on its own rows, added on the host in rank order in the element type
        sum_w, want_u, want_n = None, [], 0.0
        for k, _ in team.each():
            uk, wk, out = J.from_numpy(mine(k), T.ranges()[k]), J.zeros(T.domain()), C.c_double(-1.0)
            assert lib.jh_blockop_bidiag_step(_native(local_ops[k]).handle, uk.handle, v[k].handle, wk.handle, 0.75, -0.5, C.byref(out)) == 0
            want_u.append(_flat(uk).copy())
            sum_w = _flat(wk).copy() if sum_w is None else sum_w + _flat(wk)
            want_n += out.value
        u = rowpart.TeamVec([J.from_numpy(mine(k), T.ranges()[k]) for k, _ in team.each()])
        w = team.zeros(T.domain())
        nranges = len(list(rowpart._grid_chunk_bounds(n, T.nchunks)))
        assert nranges >= 2
        before = chains.STATS["grid_range_calls"]
        nrm2 = T.bidiag_step_(u, v, w, 0.75, -0.5)
        assert nrm2 is not None and chains.STATS["grid_range_calls"] == before + nranges * 2
        for k, _ in team.each():
            assert_bits_equal(_flat(u[k]), want_u[k], f"team step on a grid: rows of member {k}")
            assert_bits_equal(_flat(w[k]), sum_w, f"team step on a grid: w of member {k} vs the members' steps summed in rank order")
        assert abs(nrm2 - want_n) <= 1e-12 * want_n
        # the knob is per context: members that disagree are an error before any member's u is touched
        for k, _ in team.each():
            J.tune(grid_range=1 if k == 0 else 0)
        try:
            u2 = rowpart.TeamVec([J.from_numpy(mine(k), T.ranges()[k]) for k, _ in team.each()])
            with pytest.raises(ValueError, match="grid_range differs"):
                T.bidiag_step_(u2, v, team.zeros(T.domain()), 0.75, -0.5)
            for k, _ in team.each():
                assert_bits_equal(_flat(u2[k]), mine(k), f"members disagree on the knob: u of member {k} untouched")
        finally:
            for k, _ in team.each():
                J.tune(grid_range=1)
        # the adjoint and A'A range by range, the same sum
        for name, whole, ranged in (("adjoint", lambda k, o, x: lib.jh_blockop_mul_adj(_native(local_ops[k]).handle, o.handle, x.handle), T.mul_adj_),
                                    ("normal", lambda k, o, x: lib.jh_blockop_normal_mul(_native(local_ops[k]).handle, o.handle, x.handle), T.normal_mul_)):
            x = u if name == "adjoint" else v
            want = None
            for k, _ in team.each():
                ok = J.zeros(T.domain())
                assert whole(k, ok, x[k]) == 0
                want = _flat(ok).copy() if want is None else want + _flat(ok)
            out = team.zeros(T.domain())
            before = chains.STATS["grid_range_calls"]
            ranged(out, x)
            assert chains.STATS["grid_range_calls"] == before + nranges * 2, name
            for k, _ in team.each():
                assert_bits_equal(_flat(out[k]), want, f"team {name} on a grid: member {k}")
    finally:
        for k, _ in team.each():
            J.tune(grid_range=0, adj_split=-1)
        if T is not None:
            T.close()
