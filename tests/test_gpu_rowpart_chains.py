"""GPU: weighted shards of the row partition (rowpart.for_device on L = W_loc o A_loc and its kin) -- the adjoint and the normal operator as fused
chains applied range by range (jh_chain_apply_range), each range's all-reduce enqueued behind its kernel; world size 1 with the collective
forced, through the C ABI's communicator (AbiComm) and through torch.distributed's "nccl" backend, as tests/test_gpu_lsqr.py does for plain
shards.  At world size 1 the exchange adds nothing, so every result has the bits of the single-process composite (J.mul_)."""
import numpy as np
import pytest

from .helpers import assert_bits_equal, make_tall_diag

pytestmark = pytest.mark.gpu

SHAPE = (64, 64, 20)            # 81 920 elements: three exchange ranges (64 KiB-aligned bounds)


def _locals(J, oracle, A, nrow):
    """name -> the local composite around the shard's tall operator A"""
    R, D = J.range(A), J.domain(A)
    w = J.rand(R, seed=81, stream=0)
    c = J.rand(D, seed=82, stream=0)
    W, M = J.JopDiagonal(w), J.JopDiagonal(c)
    spc = J.JetSpace(np.float32, *SHAPE)
    rows = []
    for i in range(nrow):
        row = [J.JopZeroBlock(spc, spc) for _ in range(nrow)]
        row[i] = J.JopDiagonal(w.arrays[i])
        rows.append(row)
    Wb = J.blockop(rows)
    return {"W o A": W @ A, "Wb o A": Wb @ A, "W o A o M": W @ A @ M, "a * (W o A)": 0.75 * (W @ A)}


def _check_shard(J, shard, L, A, tag):
    from jets_jl_amd import chains

    d = J.rand(J.range(A), seed=83, stream=0)
    before = chains.STATS["chain_range_calls"]
    mt = shard.mul_adj_(J.rand(J.domain(A), seed=84, stream=0), d, force_collective=True)          # dirty output
    assert chains.STATS["chain_range_calls"] == before + 3, f"{tag}: the adjoint ran as three ranged chains"
    assert_bits_equal(mt.to_numpy(), J.mul_(J.zeros(J.domain(A)), L.H, d).to_numpy(), f"{tag}: pipelined weighted adjoint")
    v = J.rand(J.domain(A), seed=85, stream=0)
    before = chains.STATS["chain_range_calls"]
    yn = shard.normal_mul_(J.rand(J.domain(A), seed=86, stream=0), v, force_collective=True)      # dirty, no tmp_local
    assert chains.STATS["chain_range_calls"] == before + 3, f"{tag}: the normal operator ran as three ranged chains"
    assert_bits_equal(yn.to_numpy(), J.mul_(J.zeros(J.domain(A)), L.H @ L, v).to_numpy(), f"{tag}: pipelined weighted normal")
    fwd = shard.mul_(J.zeros(J.range(A)), v)
    assert_bits_equal(fwd.to_numpy(), (L * v).to_numpy(), f"{tag}: forward (local, no exchange)")


def test_weighted_shards_through_the_abi_communicator(Jets, oracle):
    J = Jets
    nrow = 5
    comm = J.rowpart.AbiComm(nranks=1, rank=0)
    try:
        A, _, _, _ = make_tall_diag(J, oracle, np.float32, nrow, SHAPE)
        for tag, L in _locals(J, oracle, A, nrow).items():
            shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=comm)
            assert shard.fused_normal
            _check_shard(J, shard, L, A, tag)
            shard.close()
    finally:
        comm.close()


def test_weighted_shards_through_torch_distributed(Jets, oracle):
    import os

    import torch
    import torch.distributed as dist

    if dist.is_initialized():
        pytest.skip("a process group already exists")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29537")
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        J = Jets
        nrow = 5
        A, _, _, _ = make_tall_diag(J, oracle, np.float32, nrow, SHAPE)
        for tag, L in _locals(J, oracle, A, nrow).items():
            shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L)
            _check_shard(J, shard, L, A, tag)
            J.synchronize()
            shard.close()
    finally:
        dist.destroy_process_group()


def test_solvers_on_a_weighted_shard(Jets, oracle, monkeypatch):
    """CGNR applies L'L through the shard's normal_mul_ (one fused pass + the ranged exchange per iteration), LSQR and CGLS take the pipelined
    weighted adjoint; all three reach the weighted solution and match the single-process solve on the composite."""
    from jets_jl_amd import chains

    J = Jets
    nrow, iters = 5, 25
    monkeypatch.setenv("BENCH_FORCE_DIST", "1")                 # _ShardEngine: run the exchange with one rank
    comm = J.rowpart.AbiComm(nranks=1, rank=0)

    def one_plus(x):                                            # coefficients and weights in [1, 2): a well-conditioned diagonal system
        return J.lincomb_(x, [1.0, 1.0], [x, J.ones(J.space(x))])

    try:
        spc = J.JetSpace(np.float32, *SHAPE)
        A = J.blockop([[J.JopDiagonal(one_plus(J.rand(spc, seed=88, stream=i)))] for i in range(nrow)])
        L = J.JopDiagonal(one_plus(J.rand(J.range(A), seed=89, stream=0))) @ A
        shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=comm)
        x_true = J.rand(J.domain(A), seed=87, stream=0)
        b = L * x_true
        for solve in (J.cgnr, J.lsqr, J.cgls):
            before = chains.STATS["chain_range_calls"]
            res = solve(shard, b, atol=0.0, btol=0.0, maxiter=iters)
            assert res.itn >= 5                                     # (CGNR's recurrence for ||r|| reaches 0 on this consistent system and stops it)
            assert chains.STATS["chain_range_calls"] >= before + 3 * res.itn, f"{solve.__name__}: the ranged chains ran"
            single = solve(L, b, atol=0.0, btol=0.0, maxiter=iters)
            xs, x1, xt = res.x.to_numpy().astype(np.float64), single.x.to_numpy().astype(np.float64), x_true.to_numpy().astype(np.float64)
            # (Float32 solves; CGNR's two forms differ in arithmetic -- <p, L'L p> on the domain against ||L p||^2 on the range -- and may stop at
            # different iterations once its ||r|| recurrence reaches 0: the solver tolerance of tests/test_gpu_lsqr.py)
            assert np.linalg.norm(xs - x1) <= 1e-3 * np.linalg.norm(x1), f"{solve.__name__}: shard vs single process"
            assert np.linalg.norm(xs - xt) <= 1e-3 * np.linalg.norm(xt), f"{solve.__name__}: the weighted solution"
        shard.close()
    finally:
        comm.close()


def test_full_size_weighted_normal_in_four_ranges(Jets, oracle):
    """256 x 256^3 Float32 with range weights (config 3w's operator): the shard's normal_mul_ -- four ranged NORMAL chains on the fat, nontemporal
    k_chain_adj shape, each all-reduced behind it -- has the bits of the whole-vector chain, and on sampled slices of the domain those of the oracle's
    stage-by-stage chain over all 256 rows."""
    from jets_jl_amd import chains
    from oracle import jets_oracle as jo

    J = Jets
    dt, nrow, shape = np.float32, 256, (256, 256, 256)
    n = int(np.prod(shape))
    spc = J.JetSpace(dt, *shape)
    A = J.blockop([[J.JopDiagonal(J.rand(spc, seed=1, stream=i))] for i in range(nrow)])
    w = J.rand(J.range(A), seed=2, stream=0)
    L = J.JopDiagonal(w) @ A
    m = J.rand(J.domain(A), seed=3, stream=0)
    comm = J.rowpart.AbiComm(nranks=1, rank=0)
    try:
        shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=comm)
        before = chains.STATS["chain_range_calls"]
        y = shard.normal_mul_(J.zeros(J.domain(A)), m, force_collective=True)
        assert chains.STATS["chain_range_calls"] == before + 4
        whole = J.mul_(J.zeros(J.domain(A)), L.H @ L, m)
        got = y.to_numpy().ravel(order="F")
        assert_bits_equal(got, whole.to_numpy().ravel(order="F"), "four ranges vs the whole-vector chain")
        for s0 in (0, n // 4 - 8, n // 2 + 4096, n - 64):                              # slices across range boundaries and at the end
            k = 64
            hm = jo.rng_u01(dt, 3, 0, s0, k)
            acc = np.zeros(k, dtype=dt)
            for i in range(nrow):
                a = jo.rng_u01(dt, 1, i, s0, k)
                wi = jo.rng_u01(dt, 2, 0, i * n + s0, k)
                t = jo.block_df([[jo.Block("diag", k, coeff=a)]], [np.zeros(k, dtype=dt)], [hm])[0]
                t = jo.child_mul(jo.Block("diag", k, coeff=wi), np.zeros(k, dtype=dt), t)      # W
                t = jo.child_mul(jo.Block("diag", k, coeff=wi, adjoint=True), np.zeros(k, dtype=dt), t)   # W'
                acc = acc + jo.block_df_adj([[jo.Block("diag", k, coeff=a)]], [np.zeros(k, dtype=dt)], [t])[0]
            assert_bits_equal(got[s0:s0 + k], acc, f"slice at {s0} vs the oracle")
        shard.close()
        del whole, y
    finally:
        comm.close()
        J.close(A)
