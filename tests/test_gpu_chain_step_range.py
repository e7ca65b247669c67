"""GPU: jh_chain_bidiag_step_range -- the Golub-Kahan step of a FORWARD chain L = R o A o P on an element range of the domain (weighted LSQR / CGLS
over a row partition: src/Jets.jl:530-540 over 1034-1057, the solvers over vec(L) 1138-1154; k_chain_adj MODE 2 with its range bounds).

The bar: ranges that tile the domain give, together, the bits of ONE jh_chain_bidiag_step for u and w (adj_split = 0; u always), their shares of
||u||^2 add up to its normsq to 1e-12 relative (fp64 partials summed in another order: the bound of tests/test_gpu_grid_step.py); a range touches its
columns of u and its elements of w and nothing else; the deferred accumulator holds the sum of the shares; declines leave everything alone.  Then the
routes built on it: a weighted shard (one rank, forced exchange, AbiComm) and a team of contexts with weighted members."""
import gc
import math

import numpy as np
import pytest

from .helpers import DTYPES, assert_bits_equal, rel_err, u01
from .test_gpu_chains import Rig

pytestmark = pytest.mark.gpu

STEP_CHAINS = {
    # name: tokens in application order (tests/test_gpu_chains.py: Rig)
    "W o A": ["A", ("W", 0, False)],
    "W o A o M": [("M", 0, False), "A", ("W", 0, False)],
    "W2 o W1 o A": ["A", ("W", 0, False), ("W", 1, True)],            # two range-side stages
}


def _flat(x):
    return x.to_numpy().ravel(order="F")


def _fwd(rig, toks):
    """(L, its FORWARD ChainHandle, the cache that owns it)"""
    from jets_jl_amd import chains

    L = rig.compose(toks)
    cache = chains.ChainCache()
    h = chains.one_run(chains.stages_of(L), cache, "t", chains.CHAIN_FORWARD)
    assert isinstance(h, chains.ChainHandle), "one fused FORWARD run"
    return L, h, cache


def _ranges(nd, dt, k):
    """k element ranges that tile [0, nd): bounds on the 16-byte grid, the last ends with the vector (inside a pack when nd is off the grid)"""
    es = np.dtype(dt).itemsize
    al = max(1, 16 // es)
    step = -(-(-(-nd // k)) // al) * al
    return [(lo, min(step, nd - lo)) for lo in range(0, nd, step)]


def _whole(J, h, L, u0, v, alpha, beta):
    """ONE jh_chain_bidiag_step: (u, w, normsq)"""
    import ctypes as C

    from jets_jl_amd._ffi import check, lib

    u = J.copyto_(J.zeros(J.range(L)), u0)
    w = J.rand(J.domain(L), seed=55, stream=3)
    out = C.c_double(0)
    check(lib.jh_chain_bidiag_step(h.handle, u.handle, v.handle, w.handle, float(alpha), float(beta), C.byref(out)))
    return _flat(u), _flat(w), out.value


def _inputs(J, oracle, L, dt, nrow, n, seed=93):
    v = J.from_numpy(u01(oracle, dt, seed, 0, n), J.domain(L))
    u0 = J.from_numpy(np.concatenate([u01(oracle, dt, seed + 1, i, n) for i in range(nrow)]), J.range(L))
    return u0, v


def _nan_like(J, x):
    a = x.to_numpy().copy()
    a[...] = np.nan
    return J.from_numpy(a, J.space(x))


def _ranged(J, h, L, u_start, v, alpha, beta, ranges, nrow, n, tag):
    """the step range by range, shares read back; after the FIRST of several ranges everything outside it still holds its old bits"""
    u = J.copyto_(J.zeros(J.range(L)), u_start)
    w = J.rand(J.domain(L), seed=55, stream=3)
    old_u, old_w = _flat(u).reshape(nrow, n).copy(), _flat(w).copy()
    shares = []
    for k, (lo, cnt) in enumerate(ranges):
        shares.append(h.bidiag_step_range(u, v, w, alpha, beta, lo, cnt, read_normsq=True))
        if k == 0 and len(ranges) > 1:
            gu, gw = _flat(u).reshape(nrow, n), _flat(w)
            keep = np.ones(n, dtype=bool)
            keep[lo:lo + cnt] = False
            assert_bits_equal(gu[:, keep].ravel(), old_u[:, keep].ravel(), f"{tag}: columns of u outside the first range")
            assert_bits_equal(gw[keep], old_w[keep], f"{tag}: elements of w outside the first range")
    return _flat(u), _flat(w), shares


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(STEP_CHAINS))
@pytest.mark.parametrize("nrow,n,kinds", [(5, 4096 + 64, "diag"), (7, 1027, "mixed")])
@pytest.mark.parametrize("beta", [0.0, -0.625])
def test_ranges_have_the_bits_of_the_whole_vector_step(Jets, oracle, dt, name, nrow, n, kinds, beta):
    from jets_jl_amd import chains

    J = Jets
    rig = Rig(J, oracle, dt, nrow, n, kinds, with_wb=False)
    L, h, cache = _fwd(rig, STEP_CHAINS[name])
    u0, v = _inputs(J, oracle, L, dt, nrow, n)
    alpha = 1.375
    J.tune(adj_split=0)
    try:
        wu, ww, wn = _whole(J, h, L, u0, v, alpha, beta)
        assert np.isfinite(wn) and wn > 0
        start = _nan_like(J, u0) if beta == 0.0 else u0              # beta == 0: u is write-only, a NaN-filled u must not leak
        for k in (1, 3, 4):
            ranges = _ranges(n, dt, k)
            assert len(ranges) == k
            before = (chains.STATS["chain_range_calls"], chains.STATS["chain_step_range_calls"])
            gu, gw, shares = _ranged(J, h, L, start, v, alpha, beta, ranges, nrow, n, f"{name}, {k} ranges")
            assert chains.STATS["chain_range_calls"] == before[0] + k and chains.STATS["chain_step_range_calls"] == before[1] + k
            assert J.tune_get("last_adj_parts") == 1
            assert_bits_equal(gu, wu, f"{name}, {k} ranges: u vs jh_chain_bidiag_step")
            assert_bits_equal(gw, ww, f"{name}, {k} ranges: w vs jh_chain_bidiag_step")
            got = math.fsum(shares)
            print(f"{name} {np.dtype(dt).name} beta={beta} {k} ranges: shares sum {got!r} whole {wn!r} rel {abs(got - wn) / wn:.3e}")
            assert abs(got - wn) <= 1e-12 * wn, f"{name}, {k} ranges: the shares of ||u||^2"
    finally:
        J.tune(adj_split=-1)
        cache.close()
        rig.close()


@pytest.mark.parametrize("dt", [np.float32, np.complex128])
def test_deferred_norm_is_the_sum_of_the_shares(Jets, oracle, dt):
    """jh_normsq_reset, k ranged steps with normsq == NULL, ONE jh_normsq_read: the shares added in enqueue order -- the additions a host makes of the
    returned shares in that order, so the two sums are the same fp64 number."""
    import ctypes as C

    from jets_jl_amd._ffi import check, lib

    J = Jets
    nrow, n = 6, 3 * 4096 + 17
    rig = Rig(J, oracle, dt, nrow, n, "mixed", with_wb=False)
    L, h, cache = _fwd(rig, STEP_CHAINS["W o A o M"])
    u0, v = _inputs(J, oracle, L, dt, nrow, n)
    ranges = _ranges(n, dt, 4)
    J.tune(adj_split=0)
    try:
        _, _, shares = _ranged(J, h, L, u0, v, -0.5, 2.0, ranges, nrow, n, "read back")
        u = J.copyto_(J.zeros(J.range(L)), u0)
        w = J.zeros(J.domain(L))
        check(lib.jh_normsq_reset())
        for lo, cnt in ranges:
            assert h.bidiag_step_range(u, v, w, -0.5, 2.0, lo, cnt) is None
        out = C.c_double(-1.0)
        check(lib.jh_normsq_read(C.byref(out)))
        want = 0.0
        for s in shares:
            want += s
        print(f"deferred {out.value!r} vs sum of shares {want!r}")
        assert out.value == want
    finally:
        J.tune(adj_split=-1)
        cache.close()
        rig.close()


@pytest.mark.parametrize("dt", [np.float32, np.complex64])
def test_many_small_rows_take_the_split_walk_per_range(Jets, oracle, dt):
    """1024 rows of 64 elements, the launcher's own adj_split: every range cuts w's row sum into parts (each range is launched as a vector of its own
    length) -- u is updated row by row either way (bits), w within the tolerance tests/test_gpu_chain_range.py uses for ranged chains."""
    J = Jets
    nrow, n = 1024, 64
    rig = Rig(J, oracle, dt, nrow, n, "diag", with_wb=False)
    L, h, cache = _fwd(rig, STEP_CHAINS["W o A"])
    u0, v = _inputs(J, oracle, L, dt, nrow, n)
    tol = 2e-5 * np.sqrt(nrow)
    try:
        J.tune(adj_split=0)
        wu, ww, wn = _whole(J, h, L, u0, v, 1.0, -0.25)
        J.tune(adj_split=-1)
        u = J.copyto_(J.zeros(J.range(L)), u0)
        w = J.rand(J.domain(L), seed=55, stream=3)
        shares = []
        for lo, cnt in _ranges(n, dt, 3):
            shares.append(h.bidiag_step_range(u, v, w, 1.0, -0.25, lo, cnt, read_normsq=True))
            assert J.tune_get("last_adj_parts") > 1, "the split walk is taken and reported"
        assert_bits_equal(_flat(u), wu, "u (split walk)")
        err = np.abs(_flat(w) - ww).max() / np.abs(ww).max()
        print(f"{np.dtype(dt).name}: split-walk w max error {err:.3e} (bound {tol:.3e})")
        assert err <= tol
        got = math.fsum(shares)
        assert abs(got - wn) <= 1e-12 * wn
    finally:
        J.tune(adj_split=-1)
        cache.close()
        rig.close()


def _status(fn):
    from jets_jl_amd._ffi import JetsHipError

    try:
        fn()
    except JetsHipError as e:
        return e.status
    return 0


def test_declines_leave_the_outputs_untouched(Jets, oracle):
    from jets_jl_amd import chains
    from .test_gpu_grid_chains import GridRig

    J = Jets
    dt, nrow, n = np.float32, 5, 1027
    rig = Rig(J, oracle, dt, nrow, n, "diag", with_wb=False)
    L, h, cache = _fwd(rig, STEP_CHAINS["W o A"])
    u0, v = _inputs(J, oracle, L, dt, nrow, n)
    u = J.copyto_(J.zeros(J.range(L)), u0)
    w = J.rand(J.domain(L), seed=5, stream=0)
    hu, hw, hv = u.to_numpy().tobytes(), w.to_numpy().tobytes(), v.to_numpy().tobytes()

    def same(tag):
        assert u.to_numpy().tobytes() == hu and w.to_numpy().tobytes() == hw and v.to_numpy().tobytes() == hv, tag

    adj = chains.one_run(chains.stages_of(L.H), cache, "a", chains.CHAIN_ADJOINT)
    assert isinstance(adj, chains.ChainHandle)
    assert _status(lambda: adj.bidiag_step_range(u, v, w, 1.0, 0.5, 0, 4)) == 1              # an ADJOINT handle
    assert _status(lambda: h.bidiag_step_range(u, v, w, 1.0, 0.5, 1, 4)) == 1                # first on no 16-byte boundary
    assert _status(lambda: h.bidiag_step_range(u, v, w, 1.0, 0.5, 0, 6)) == 1                # an end off the grid that is not the vector's end
    assert _status(lambda: h.bidiag_step_range(u, v, w, 1.0, 0.5, 1024, 8)) == 1             # past the end
    assert _status(lambda: h.bidiag_step_range(u, v, w, 1.0, 0.5, -4, 4)) == 1
    assert _status(lambda: h.bidiag_step_range(u, v, v, 1.0, 0.5, 0, 4)) == 1                # w aliases v
    same("invalid arguments")
    assert _status(lambda: h.bidiag_step_range(u, v, w, 1.0, 0.5, 8, 0)) == 0                # count 0: a no-op
    same("count 0")
    L3, h3, cache3 = _fwd(rig, ["A", ("W", 0, False), ("s", 2.0, "r"), ("W", 1, False)])   # R + R^H: six range-side stages
    assert _status(lambda: h3.bidiag_step_range(u, v, w, 1.0, 0.5, 0, 4)) == 4
    same("a three-stage R")
    cache3.close()
    grig = GridRig(J, oracle, dt, 5, 3, n)
    G = grig.compose(["A", ("W", 0, False)])
    gcache = chains.ChainCache()
    gh = chains.one_run(chains.stages_of(G), gcache, "g", chains.CHAIN_FORWARD)
    assert isinstance(gh, chains.ChainHandle) and gh.grid
    gu, gv, gw = J.rand(J.range(G), seed=6, stream=0), J.rand(J.domain(G), seed=7, stream=0), J.rand(J.domain(G), seed=8, stream=0)
    bu, bw = gu.to_numpy().tobytes(), gw.to_numpy().tobytes()
    assert _status(lambda: gh.bidiag_step_range(gu, gv, gw, 1.0, 0.5, 0, 4)) == 4            # a grid chain has no one-pass step
    assert gu.to_numpy().tobytes() == bu and gw.to_numpy().tobytes() == bw
    assert _status(lambda: h.bidiag_step_range(u, v, w, 1.0, 0.5, 1024, 3)) == 0             # the last range may end inside a pack
    gcache.close()
    cache.close()
    rig.close()


@pytest.mark.parametrize("shape", [(256, 0), (512, 2), (512, 4)])
@pytest.mark.parametrize("nt", [0, 2])
@pytest.mark.parametrize("dt", [np.float32, np.complex64, np.float64])
def test_every_launch_shape_the_step_launcher_picks(Jets, oracle, dt, shape, nt):
    """tune(adj_wg, adj_unroll) forces 256 x 1 x 2, 512 x 2 x 1 and 512 x 4 x 1 (ComplexF32: capped to 512 x 2 x 1), nt the loads: three ranges each"""
    J = Jets
    nrow, n = 6, 3 * 4096 + 17
    rig = Rig(J, oracle, dt, nrow, n, "mixed", with_wb=False)
    L, h, cache = _fwd(rig, STEP_CHAINS["W2 o W1 o A"])
    u0, v = _inputs(J, oracle, L, dt, nrow, n)
    J.tune(adj_wg=shape[0], adj_unroll=shape[1], nt=nt, adj_split=0)
    try:
        wu, ww, wn = _whole(J, h, L, u0, v, -0.5, 2.0)
        gu, gw, shares = _ranged(J, h, L, u0, v, -0.5, 2.0, _ranges(n, dt, 3), nrow, n, f"{shape} nt={nt}")
        assert_bits_equal(gu, wu, f"{shape} nt={nt}: u")
        assert_bits_equal(gw, ww, f"{shape} nt={nt}: w")
        assert abs(math.fsum(shares) - wn) <= 1e-12 * wn
    finally:
        J.tune(adj_wg=0, adj_unroll=0, nt=1, adj_split=-1)
        cache.close()
        rig.close()


# ------------------------------------------------------------------ a weighted shard: one rank, forced exchange -------------------------
SHARD_SHAPE = (128, 128, 128)      # 2 Mi elements: four exchange ranges; six rows of 8 MiB: a range vector of 48 MiB (the slab cache keeps >= 16 MiB)


def _well_conditioned(J, nrow):
    def one_plus(x):                                            # coefficients and weights in [1, 2)
        return J.lincomb_(x, [1.0, 1.0], [x, J.ones(J.space(x))])

    spc = J.JetSpace(np.float32, *SHARD_SHAPE)
    A = J.blockop([[J.JopDiagonal(one_plus(J.rand(spc, seed=88, stream=i)))] for i in range(nrow)])
    L = J.JopDiagonal(one_plus(J.rand(J.range(A), seed=89, stream=0))) @ A
    return A, L


@pytest.mark.parametrize("solver", ["lsqr", "cgls"])
def test_solvers_on_a_weighted_shard_take_the_ranged_step(Jets, oracle, monkeypatch, solver):
    """J.lsqr / J.cgls on the shard of W o A (AbiComm, one rank, BENCH_FORCE_DIST=1): JETS_AR_CHUNKS ranged steps per iteration, no range-sized
    temporary (the slab cache, which keeps every freed vector of >= 16 MiB, holds nothing after the solve; device memory is back where it was), the
    single-process solution and the true one within 1e-3; JETS_CHAIN_STEP=0 runs no ranged step and allocates the temporary."""
    from jets_jl_amd import chains

    J = Jets
    nrow, iters, nchunks = 6, 25, 4
    monkeypatch.setenv("BENCH_FORCE_DIST", "1")
    monkeypatch.delenv("JETS_AR_CHUNKS", raising=False)
    monkeypatch.delenv("JETS_CHAIN_STEP", raising=False)
    solve = getattr(J, solver)
    range_mib = nrow * int(np.prod(SHARD_SHAPE)) * 4 >> 20
    comm = J.rowpart.AbiComm(nranks=1, rank=0)
    try:
        A, L = _well_conditioned(J, nrow)
        x_true = J.rand(J.domain(A), seed=87, stream=0)
        b = L * x_true
        single = solve(L, J.copyto_(J.zeros(J.range(A)), b), atol=0.0, btol=0.0, maxiter=iters)
        x1, xt = single.x.to_numpy().astype(np.float64), x_true.to_numpy().astype(np.float64)
        del single
        for chain_step in ("1", "0"):
            monkeypatch.setenv("JETS_CHAIN_STEP", chain_step)
            shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=comm)
            assert shard.chain_step == (chain_step == "1")
            rhs = J.copyto_(J.zeros(J.range(A)), b)
            gc.collect()
            J.synchronize()
            J.trim()
            free0 = J.device_info()["free_mem"]
            before = (chains.STATS["chain_step_range_calls"], chains.STATS["chain_range_calls"])
            res = solve(shard, rhs, atol=0.0, btol=0.0, maxiter=iters, overwrite_b=True)
            steps = chains.STATS["chain_step_range_calls"] - before[0]
            ranged = chains.STATS["chain_range_calls"] - before[1]
            xs = res.x.to_numpy().astype(np.float64)
            itn = res.itn
            del res
            gc.collect()
            J.synchronize()
            cached = J.tune_get("slab_cached_mib")
            J.trim()
            free1 = J.device_info()["free_mem"]
            print(f"{solver} JETS_CHAIN_STEP={chain_step}: itn {itn}, ranged steps {steps}, ranged chains {ranged}, slab cache {cached} MiB, "
                  f"free memory {free0 >> 20} -> {free1 >> 20} MiB")
            assert itn >= 5
            assert ranged >= 3 * itn
            if chain_step == "1":
                assert steps >= nchunks * itn, "JETS_AR_CHUNKS ranged steps per iteration"
                assert cached < 16, "no vector of 16 MiB or more was allocated and freed by the solve: no range-sized temporary"
            else:
                assert steps == 0, "JETS_CHAIN_STEP=0: today's route"
                assert cached >= range_mib, "the route through the range temporary allocates it (this check sees it)"
            assert abs(free1 - free0) < (range_mib << 20) // 2, "device memory is back where it was"
            assert np.linalg.norm(xs - x1) <= 1e-3 * np.linalg.norm(x1), f"{solver}: shard vs single process"
            assert np.linalg.norm(xs - xt) <= 1e-3 * np.linalg.norm(xt), f"{solver}: the weighted solution"
            shard.close()
    finally:
        monkeypatch.delenv("JETS_CHAIN_STEP", raising=False)
        comm.close()


def test_warm_start_on_a_weighted_shard_is_one_ranged_step(Jets, oracle, monkeypatch):
    from jets_jl_amd import chains

    J = Jets
    nrow = 6
    monkeypatch.setenv("BENCH_FORCE_DIST", "1")
    monkeypatch.delenv("JETS_CHAIN_STEP", raising=False)
    comm = J.rowpart.AbiComm(nranks=1, rank=0)
    try:
        A, L = _well_conditioned(J, nrow)
        x_true = J.rand(J.domain(A), seed=87, stream=0)
        b = L * x_true
        x0 = J.lincomb_(J.zeros(J.domain(A)), [0.9], [x_true])
        shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=comm)
        before = chains.STATS["chain_step_range_calls"]
        res = J.lsqr(shard, b, x0=x0, atol=0.0, btol=0.0, maxiter=20)
        assert chains.STATS["chain_step_range_calls"] >= before + 4 * (res.itn + 1)
        xs, xt = res.x.to_numpy().astype(np.float64), x_true.to_numpy().astype(np.float64)
        assert np.linalg.norm(xs - xt) <= 1e-3 * np.linalg.norm(xt)
        shard.close()
    finally:
        comm.close()


# ------------------------------------------------------------------ a team of contexts with weighted members ----------------------------
@pytest.mark.parametrize("nmem", [2, 3])
def test_a_team_with_weighted_members(Jets, oracle, nmem):
    """Two and three contexts on one device, 11 rows split unevenly, every member's local operator W_k o A_k: TeamOp.bidiag_step_ and normal_mul_
    against the one-GPU chain step / NORMAL chain on the whole operator -- u: bits; w and y: the bits of the members' own chains summed in member
    order (adj_split = 0), and the team's all-reduce tolerance of tests/test_gpu_contexts.py (1e-6) against the whole operator's ordered sum --
    and weighted team LSQR / CGLS."""
    from jets_jl_amd import chains, rowpart
    from .test_gpu_contexts import _team_contexts

    J = Jets
    J.init(0)
    home = J.context_current()[0]
    ctxs, extra = _team_contexts(J, nmem)
    team = rowpart.Team(ctxs)
    try:
        _weighted_team_flow(J, oracle, chains, rowpart, team, nmem, home)
    finally:
        team.close()
        gc.collect()                                                 # the members' vectors, operators and chain handles die before their contexts
        J.context_use(home)
        for c in extra:
            J.context_destroy(c)


def _weighted_team_flow(J, oracle, chains, rowpart, team, nmem, home):
    T = None
    try:
        dt, nrow, shape = np.float32, 11, (65, 63, 17)          # 69 615 elements: rows off the 16-byte grid, the last range ends inside a pack
        n = int(np.prod(shape))
        spc = J.JetSpace(dt, *shape)
        parts = [rowpart.partition_rows(nrow, nmem, k) for k in range(nmem)]
        ha = [1.0 + oracle.rng_u01(dt, 1, 0, i * n, n) for i in range(nrow)]
        hw = [1.0 + oracle.rng_u01(dt, 2, 0, i * n, n) for i in range(nrow)]
        local_ops, keep = [], []
        for k, _ in team.each():
            lo, cnt = parts[k].first, parts[k].count
            Ak = J.blockop([[J.JopDiagonal(J.from_numpy(ha[lo + i], spc))] for i in range(cnt)])
            wk = J.from_numpy(np.concatenate(hw[lo:lo + cnt]), J.range(Ak))
            keep.append((Ak, wk))
            local_ops.append(J.JopDiagonal(wk) @ Ak)
        T = team.operator(local_ops)
        assert T.chain_step and T.fused_normal
        J.context_use(home)
        A = J.blockop([[J.JopDiagonal(J.from_numpy(a, spc))] for a in ha])
        L = J.JopDiagonal(J.from_numpy(np.concatenate(hw), J.range(A))) @ A
        sc = chains.SolverChains(L)
        hm = u01(oracle, dt, 3, 0, n)
        hu = [u01(oracle, dt, 4, i, n) for i in range(nrow)]
        J.tune(adj_split=0)
        u1 = J.from_numpy(np.concatenate(hu), J.range(A))
        m1 = J.from_numpy(hm, spc)
        w1 = J.zeros(spc)
        want_n = sc.step(u1, m1, w1, 0.75, -0.5)
        want_y = _flat(sc.normal().apply(J.zeros(spc), m1))
        want_u, want_w = u1.to_numpy(), _flat(w1)
        for k, _ in team.each():
            J.tune(adj_split=0)
        m = rowpart.TeamVec([J.from_numpy(hm, spc) for _ in team.each()])
        u = rowpart.TeamVec([J.from_numpy(np.concatenate(hu[parts[k].first:parts[k].first + parts[k].count]), T.ranges()[k]) for k, _ in team.each()])
        w = team.zeros(T.domain())
        # every member's own one-GPU chain step / NORMAL chain on its rows, added on the host in member order (the team's grouped sum adds the members
        # in rank order): with the ordered walk the team's w and y have THESE bits
        sum_w = sum_y = None
        for k, _ in team.each():
            sck = chains.SolverChains(local_ops[k])
            uk, wk = J.copyto_(J.zeros(T.ranges()[k]), u[k]), J.zeros(spc)
            assert sck.step(uk, m[k], wk, 0.75, -0.5) is not None
            yk = _flat(sck.normal().apply(J.zeros(spc), m[k]))
            sum_w = _flat(wk) if sum_w is None else sum_w + _flat(wk)
            sum_y = yk if sum_y is None else sum_y + yk
            sck.close()
        before = chains.STATS["chain_step_range_calls"]
        nrm2 = T.bidiag_step_(u, m, w, 0.75, -0.5)
        nranges = len(list(rowpart._chunk_bounds(n, T.nchunks)))                                     # (bounds on 64 KiB boundaries: three ranges of 69 615 elements)
        assert nranges >= 2
        assert nrm2 is not None and chains.STATS["chain_step_range_calls"] == before + nranges * nmem
        for k in range(nmem):
            lo, cnt = parts[k].first, parts[k].count
            assert_bits_equal(u[k].to_numpy(), want_u[lo * n:(lo + cnt) * n], f"team step: rows of member {k}")
        gw = [_flat(x) for x in w.members]
        print(f"team of {nmem}: w rel err {rel_err(gw[0], want_w):.3e}, ||u||^2 rel {abs(nrm2 - want_n) / want_n:.3e}")
        assert rel_err(gw[0], want_w) < 1e-6 and all(np.array_equal(gw[k], gw[0]) for k in range(1, nmem))
        assert_bits_equal(gw[0], sum_w, "team step: w vs the members' chain steps summed in member order")
        assert abs(nrm2 - want_n) <= 1e-12 * want_n
        y = team.zeros(T.domain())
        before = chains.STATS["chain_range_calls"]
        T.normal_mul_(y, m)
        assert chains.STATS["chain_range_calls"] == before + nranges * nmem
        gy = [_flat(x) for x in y.members]
        assert rel_err(gy[0], want_y) < 1e-6 and all(np.array_equal(gy[k], gy[0]) for k in range(1, nmem))
        assert_bits_equal(gy[0], sum_y, "team normal: y vs the members' NORMAL chains summed in member order")
        for k, _ in team.each():
            J.tune(adj_split=-1)
        # weighted LSQR over the team against the single-context solve on the whole weighted operator
        J.context_use(home)
        x_true = J.rand(spc, seed=5, stream=0)
        b = L * x_true
        ref = J.lsqr(L, b, maxiter=25, atol=0.0, btol=0.0)
        hb = b.to_numpy()
        bt = rowpart.TeamVec([J.from_numpy(hb[parts[k].first * n:(parts[k].first + parts[k].count) * n], T.ranges()[k]) for k, _ in team.each()])
        before = chains.STATS["chain_step_range_calls"]
        res = J.lsqr(T, bt, maxiter=25, atol=0.0, btol=0.0)
        assert chains.STATS["chain_step_range_calls"] >= before + nranges * nmem * res.itn
        xs, x1, xt = res.x[0].to_numpy().astype(np.float64), ref.x.to_numpy().astype(np.float64), x_true.to_numpy().astype(np.float64)
        assert np.linalg.norm(xs - x1) <= 1e-3 * np.linalg.norm(x1)
        assert np.linalg.norm(xs - xt) <= 1e-3 * np.linalg.norm(xt)
        res_c = J.cgls(T, bt, maxiter=25, atol=0.0, btol=0.0)
        xc = res_c.x[0].to_numpy().astype(np.float64)
        assert np.linalg.norm(xc - xt) <= 1e-3 * np.linalg.norm(xt)
        sc.close()
        del res, res_c, ref
    finally:
        for k, _ in team.each():
            J.tune(adj_split=-1)
        if T is not None:
            T.close()
        J.context_use(home)


# ------------------------------------------------------------------ full size -----------------------------------------------------------
def test_full_size_weighted_step_in_four_ranges(Jets, oracle):
    """256 x 256^3 Float32 with range weights, the launcher's own choices: the step in four ranges against the whole-vector step -- every element of
    u (compared on the device: max |difference| over the 16 Gi-element range vector) and of w."""
    from jets_jl_amd import chains

    J = Jets
    dt, nrow, shape = np.float32, 256, (256, 256, 256)
    n = int(np.prod(shape))
    spc = J.JetSpace(dt, *shape)
    A = J.blockop([[J.JopDiagonal(J.rand(spc, seed=1, stream=i))] for i in range(nrow)])
    w8 = J.rand(J.range(A), seed=2, stream=0)
    L = J.JopDiagonal(w8) @ A
    v = J.rand(J.domain(A), seed=3, stream=0)
    sc = chains.SolverChains(L)
    try:
        assert sc.fwd is not None
        u_whole, w_whole = J.zeros(J.range(A)), J.zeros(J.domain(A))
        nsq = sc.step(u_whole, v, w_whole, 1.0, 0.0)
        assert J.tune_get("last_adj_parts") == 1
        u, w = J.zeros(J.range(A)), J.rand(J.domain(A), seed=9, stream=0)
        shares = []
        before = chains.STATS["chain_step_range_calls"]
        for lo, cnt in _ranges(n, dt, 4):
            shares.append(sc.fwd.bidiag_step_range(u, v, w, 1.0, 0.0, lo, cnt, read_normsq=True))
            assert J.tune_get("last_adj_parts") == 1
        assert chains.STATS["chain_step_range_calls"] == before + 4
        assert_bits_equal(_flat(w), _flat(w_whole), "w: four ranges vs the whole-vector step")
        J.lincomb_(u, [1.0, -1.0], [u, u_whole])                                   # x - x == 0 exactly for finite x of equal bits; any other difference is not 0
        dmax = float(J.norm(u, np.inf))
        print(f"full size: max |u - u_whole| = {dmax!r}; ||u||^2 shares {math.fsum(shares)!r} vs {nsq!r}")
        assert dmax == 0.0
        assert abs(math.fsum(shares) - nsq) <= 1e-12 * nsq
        del u, w, u_whole, w_whole
    finally:
        sc.close()
        J.close(A)
