"""CPU, gloo: a WEIGHTED shard of the row partition (rowpart.RowPartitionedOp with L = W_loc o A_loc) -- the weights partitioned with the rows,
the compute engine a numpy test double injected like tests/test_rowpart_gloo.py's.

What is new and runs here: `normal_mul_` without `tmp_local` (the injected `local_normal`, then ONE all-reduce of the domain vector), and
CG on the normal equations through the engine's `normal(y, p)` hook (cgls.cgnr_core: one application of L'L per iteration, no range vector).
The product wiring of the same shard (rowpart.for_device: jh_chain_apply_range + the ranged exchange) is covered on the GPU by
tests/test_gpu_rowpart_chains.py."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rows(dt, first, count, n, seed, shift=0.0):
    from oracle import jets_oracle as jo

    return [jo.rng_u01(dt, seed, 0, (first + i) * n, n) + dt(shift) for i in range(count)]


def _local_adj(a, w, d, n, dt):
    """m = sum_i a_i .* (w_i .* d_i), the rows in order from +0 (src/Jets.jl:1042-1049 after the weights' stage)"""
    m = np.zeros(n, dtype=dt)
    for ai, wi, di in zip(a, w, d):
        m = m + ai * (wi * di)
    return m


def _local_normal(a, w, m, n, dt):
    """y = sum_i a_i .* (w_i .* (w_i .* (a_i .* m))): L'L for L = W o A (W real: W' = W)"""
    y = np.zeros(n, dtype=dt)
    for ai, wi in zip(a, w):
        y = y + ai * (wi * (wi * (ai * m)))
    return y


def _shard(part, n, dt, a, w, calls):
    import torch

    from jets_jl_amd import rowpart

    comm = rowpart.Comm(as_tensor=torch.from_numpy)

    def local_mul(d, L, m):
        for di, ai, wi in zip(d, a, w):
            di[...] = wi * (ai * m)
        return d

    def local_mul_adj(m, L, d):
        m[...] = _local_adj(a, w, d, n, dt)
        return m

    def local_normal(y, L, m):
        calls["normal"] += 1
        y[...] = _local_normal(a, w, m, n, dt)
        return y

    return rowpart.RowPartitionedOp(part, (a, w), comm, local_mul=local_mul, local_mul_adj=local_mul_adj,
                                    local_dot=lambda x, y: sum(float(np.dot(p, q)) for p, q in zip(x, y)),
                                    local_norm=lambda x, p: float(np.linalg.norm(np.concatenate(x), p)), local_normal=local_normal), comm


def _exchange_body(rank, world, nrow, n, out_dir):
    from jets_jl_amd import rowpart

    dt = np.float32
    part = rowpart.partition_rows(nrow, world, rank)
    a = _rows(dt, part.first, part.count, n, 1)
    w = _rows(dt, part.first, part.count, n, 4, 0.25)                 # this rank's rows of the weights only
    d = _rows(dt, part.first, part.count, n, 3)
    m = _rows(dt, 0, 1, n, 2)[0]
    calls = {"normal": 0}
    shard, _ = _shard(part, n, dt, a, w, calls)
    mt = np.full(n, 9.0, dtype=dt)
    shard.mul_adj_(mt, d)                                             # local weighted adjoint + one all-reduce
    yn = np.full(n, 7.0, dtype=dt)                                    # dirty
    assert shard.fused_normal
    shard.normal_mul_(yn, m)                                          # no tmp_local: L'L in one local pass + one all-reduce
    assert calls["normal"] == 1
    np.savez(os.path.join(out_dir, f"x{rank}.npz"), mt=mt, yn=yn, ladj=_local_adj(a, w, d, n, dt), lnrm=_local_normal(a, w, m, n, dt))


def _cgnr_body(rank, world, nrow, n, iters, out_dir):
    from jets_jl_amd import rowpart
    from jets_jl_amd.cgls import cgnr_core

    dt = np.float64
    part = rowpart.partition_rows(nrow, world, rank)
    a = _rows(dt, part.first, part.count, n, 1, 0.05)
    w = _rows(dt, part.first, part.count, n, 6, 0.5)
    b = [x - 0.5 for x in _rows(dt, part.first, part.count, n, 5)]
    calls = {"normal": 0}
    shard, comm = _shard(part, n, dt, a, w, calls)

    class Engine:
        """lsqr._Engine's interface on numpy: range vectors are this rank's rows, domain vectors replicated; the normal operator through the
        shard's normal_mul_ (the hook of a weighted shard, lsqr._ShardEngine.normal)."""

        fwd_calls = 0

        def zeros_dom(self):
            return np.zeros(n, dtype=dt)

        def zeros_rng(self):
            return [np.zeros(n, dtype=dt) for _ in range(part.count)]

        def copy(self, dst, src):
            dst[...] = src
            return dst

        def lincomb(self, dst, coefs, xs):
            dst[...] = sum(c * x for c, x in zip(coefs, xs))
            return dst

        def norm_dom(self, x):
            return float(np.linalg.norm(x))

        def norm_rng(self, x):
            return shard.norm_range(x, 2)

        def fwd(self, u, v, alpha, beta):
            Engine.fwd_calls += 1
            raise AssertionError("cgnr_core with a normal hook applies no forward")

        def adj(self, v, u, alpha, beta):
            tmp = np.zeros(n, dtype=dt)
            shard.mul_adj_(tmp, u)
            v[...] = alpha * tmp + beta * v
            return float(np.linalg.norm(v))

        def normal(self, y, p):
            shard.normal_mul_(y, p)
            return float(np.dot(p, y))

    res = cgnr_core(Engine(), b, None, 0.1, 0.0, 0.0, iters)
    assert calls["normal"] == iters and Engine.fwd_calls == 0
    np.savez(os.path.join(out_dir, f"cgnr{rank}.npz"), x=res.x, itn=res.itn)


def _worker(rank, world, port, out_dir, nrow, n, nrow_s, n_s, iters):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    _exchange_body(rank, world, nrow, n, out_dir)
    _cgnr_body(rank, world, nrow_s, n_s, iters, out_dir)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,nrow,n,nrow_s,n_s,iters", [(2, 6, 1000, 5, 64, 20), (8, 1003, 40, 1003, 16, 6)])
def test_weighted_shard_adjoint_normal_and_cgnr(tmp_path, world, nrow, n, nrow_s, n_s, iters):
    import torch.multiprocessing as mp

    from oracle.cgls_ref import cgls_fp64

    sys.path.insert(0, ROOT)
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), nrow, n, nrow_s, n_s, iters), nprocs=world, join=True)

    # ---- the exchange: replicas identical, the sum of the ranks' local results, the single-process fp64 result within the multi-GPU tolerance
    res = [np.load(tmp_path / f"x{r}.npz") for r in range(world)]
    for r in res[1:]:
        assert r["mt"].tobytes() == res[0]["mt"].tobytes() and r["yn"].tobytes() == res[0]["yn"].tobytes()
    a = np.stack(_rows(np.float32, 0, nrow, n, 1)).astype(np.float64)
    w = np.stack(_rows(np.float32, 0, nrow, n, 4, 0.25)).astype(np.float64)
    d = np.stack(_rows(np.float32, 0, nrow, n, 3)).astype(np.float64)
    m = _rows(np.float32, 0, 1, n, 2)[0].astype(np.float64)
    ref_adj = (a * w * d).sum(0)
    ref_nrm = (a * w * w * a * m).sum(0)
    for key, ref in (("mt", ref_adj), ("yn", ref_nrm)):
        got = res[0][key].astype(np.float64)
        assert np.linalg.norm(got - ref) <= 1e-5 * np.linalg.norm(ref), key
    for key, lk in (("mt", "ladj"), ("yn", "lnrm")):
        fp64_sum = np.sum([r[lk].astype(np.float64) for r in res], axis=0)     # the ranks' ordered local sums, added exactly
        assert np.linalg.norm(res[0][key].astype(np.float64) - fp64_sum) <= 1e-6 * np.linalg.norm(fp64_sum), key

    # ---- CGNR through the normal hook: replicas identical, the iterates of the single-process fp64 CGLS on the weighted operator
    a = np.stack(_rows(np.float64, 0, nrow_s, n_s, 1, 0.05))
    w = np.stack(_rows(np.float64, 0, nrow_s, n_s, 6, 0.5))
    b = np.concatenate([x - 0.5 for x in _rows(np.float64, 0, nrow_s, n_s, 5)])
    aw = a * w
    xr, info = cgls_fp64(lambda v: (aw * v).ravel(), lambda y: (aw * y.reshape(nrow_s, n_s)).sum(0), b, n_s, damp=0.1, atol=0.0, btol=0.0,
                         maxiter=iters)
    sol = [np.load(tmp_path / f"cgnr{r}.npz") for r in range(world)]
    for r in sol[1:]:
        assert r["x"].tobytes() == sol[0]["x"].tobytes(), "replicas differ"
    assert int(sol[0]["itn"]) == info["itn"] == iters
    assert np.linalg.norm(sol[0]["x"] - xr) <= 1e-10 * np.linalg.norm(xr)


def test_a_shard_without_a_fused_normal_still_asks_for_tmp_local():
    """Plain shards keep their routes: no local_normal injected, no tmp_local -> the ValueError as before."""
    sys.path.insert(0, ROOT)
    from jets_jl_amd import rowpart

    class NoComm:
        world = 1

    shard = rowpart.RowPartitionedOp(rowpart.partition_rows(2, 1, 0), None, NoComm(), None, None, None, None)
    assert not shard.fused_normal
    with pytest.raises(ValueError):
        shard.normal_mul_(np.zeros(4), np.zeros(4))


def test_cgnr_core_without_a_hook_keeps_its_recurrence():
    """An engine without `normal` runs A then A' per iteration, as before (the hook is looked up, not required)."""
    sys.path.insert(0, ROOT)
    from jets_jl_amd.cgls import cgnr_core
    from oracle.cgls_ref import cgls_fp64

    rng = np.random.default_rng(5)
    nrow, n = 7, 12
    a = rng.uniform(0.1, 1.0, (nrow, n))
    b = rng.uniform(-0.5, 0.5, nrow * n)
    seen = {"fwd": 0}

    class Eng:
        def zeros_dom(self):
            return np.zeros(n)

        def zeros_rng(self):
            return np.zeros(nrow * n)

        def copy(self, dst, src):
            dst[...] = src
            return dst

        def lincomb(self, dst, coefs, xs):
            dst[...] = sum(c * x for c, x in zip(coefs, xs))
            return dst

        def norm_dom(self, x):
            return float(np.linalg.norm(x))

        norm_rng = norm_dom

        def fwd(self, u, v, alpha, beta):
            seen["fwd"] += 1
            u[...] = alpha * (a * v).ravel() + beta * u
            return float(np.linalg.norm(u))

        def adj(self, v, u, alpha, beta):
            v[...] = alpha * (a * u.reshape(nrow, n)).sum(0) + beta * v
            return float(np.linalg.norm(v))

    res = cgnr_core(Eng(), b, None, 0.0, 0.0, 0.0, 8)
    xr, _ = cgls_fp64(lambda v: (a * v).ravel(), lambda y: (a * y.reshape(nrow, n)).sum(0), b, n, damp=0.0, atol=0.0, btol=0.0, maxiter=8)
    assert seen["fwd"] == 8
    assert np.linalg.norm(res.x - xr) <= 1e-10 * np.linalg.norm(xr)
