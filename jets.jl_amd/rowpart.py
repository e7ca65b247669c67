"""Row partition of a tall block operator across the GPUs of one node.

A tall JopBlock (many block rows x one block column, src/Jets.jl:926-933) shards naturally:
the forward needs no exchange (each range block depends only on m, src/Jets.jl:1015-1031) and the
adjoint is a sum over rows (1045-1053).  One process per GPU; rank g owns the contiguous rows
[first, first+count) -- the slab order of JetBSpace.indices is preserved, so a global block index
maps to (rank, local index) by integer arithmetic.  Domain-side vectors are replicated; the only
data-path collective is ONE all-reduce (RCCL over xGMI via torch.distributed's "nccl" backend) of
the domain vector after the local adjoint, and scalar all-reduces for range-side dot/norm.

The summation order across ranks differs from the sequential reference => tolerance parity at
world_size > 1 (bit-exact at world_size 1).

The compute engine is injected (`local_mul`, `local_mul_adj`, `local_normal`, `as_tensor`) so the sharding and
collective logic can be exercised with world_size-2 gloo tests on CPU against a test double; the
product wiring (`for_device`) uses the HIP path only.
"""
from __future__ import annotations

import builtins
import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable

__all__ = ["RowPartition", "partition_rows", "Comm", "AbiComm", "RowPartitionedOp", "for_device"]


@dataclass(frozen=True)
class RowPartition:
    nrow: int        # global block rows
    world: int
    rank: int
    first: int       # first global row owned by this rank
    count: int       # rows owned

    def owner(self, irow: int) -> int:
        """Rank owning global row `irow`."""
        base, rem = divmod(self.nrow, self.world)
        cut = rem * (base + 1)
        return irow // (base + 1) if irow < cut else rem + (irow - cut) // builtins.max(base, 1)

    def local_index(self, irow: int) -> int:
        return irow - partition_rows(self.nrow, self.world, self.owner(irow)).first


def partition_rows(nrow: int, world: int, rank: int) -> RowPartition:
    """Contiguous chunks; the first nrow % world ranks get one extra row."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    base, rem = divmod(nrow, world)
    count = base + (1 if rank < rem else 0)
    first = rank * base + builtins.min(rank, rem)
    return RowPartition(nrow, world, rank, first, count)


class Comm:
    """Thin wrapper over torch.distributed (backend "nccl" == RCCL on ROCm; "gloo" in CPU tests)."""

    def __init__(self, as_tensor: Callable, stream_ctx: Callable | None = None):
        import torch.distributed as dist

        self._dist = dist
        self._as_tensor = as_tensor
        self._stream_ctx = stream_ctx
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self._views = {}   # id(vector) -> (vector, tensor): the solver all-reduces the same few vectors every iteration

    def all_reduce_sum_(self, x, force: bool = False):
        """In-place sum of a replicated domain vector over all ranks (the adjoint accumulate).
        `force` runs the collective even with one rank (exercises the RCCL path on a one-GPU box)."""
        if self.world == 1 and not (force and self._dist.is_initialized()):
            return x
        hit = self._views.get(id(x))
        if hit is None or hit[0] is not x:
            if len(self._views) > 64:
                self._views.clear()
            hit = (x, self._as_tensor(x))
            self._views[id(x)] = hit
        t = hit[1]
        if self._stream_ctx is not None:
            with self._stream_ctx():
                self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM)
        else:
            self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM)
        return x

    def all_reduce_scalars(self, values, op: str = "sum"):
        """Batched scalar all-reduce (range-side dot / norm^2 / extrema partials), fp64 on the host path."""
        import torch

        if self.world == 1:
            return list(values)
        t = torch.tensor(list(values), dtype=torch.float64)
        backend = self._dist.get_backend()
        if backend == "nccl":
            t = t.cuda()
        red = {"sum": self._dist.ReduceOp.SUM, "max": self._dist.ReduceOp.MAX, "min": self._dist.ReduceOp.MIN}[op]
        self._dist.all_reduce(t, op=red)
        return t.cpu().tolist()

    def barrier(self):
        if self.world > 1:
            self._dist.barrier()


class AbiComm:
    """The same exchange step through the C ABI's own RCCL entry points (jh_comm_*, include/jetship.h) -- what a
    host without torch.distributed (the Julia binding) uses.  `exchange_id` ships rank 0's 128-byte id to the other
    ranks (MPI broadcast, a socket, a file); with one rank it is not needed."""

    def __init__(self, nranks: int = 1, rank: int = 0, exchange_id: Callable | None = None):
        import ctypes as C

        from ._ffi import lib, check
        from . import device as _device

        _device.init()
        self._C, self._lib, self._check = C, lib, check
        ident = C.create_string_buffer(128)
        if rank == 0:
            check(lib.jh_comm_unique_id(ident))
        if nranks > 1:
            if exchange_id is None:
                raise ValueError("exchange_id(bytes_or_None) -> bytes is required for more than one rank")
            ident = C.create_string_buffer(exchange_id(ident.raw if rank == 0 else None), 128)
        check(lib.jh_comm_init_rank(ident, nranks, rank))
        self.world, self.rank = nranks, rank

    def all_reduce_sum_(self, x, force: bool = False):
        if self.world == 1 and not force:
            return x
        self._check(self._lib.jh_comm_allreduce_sum(x.handle))
        return x

    def all_reduce_scalars(self, values, op: str = "sum"):
        vals = list(values)
        buf = (self._C.c_double * len(vals))(*vals)
        self._check(self._lib.jh_comm_allreduce_scalars(buf, len(vals), {"sum": 0, "max": 1, "min": 2}[op]))
        return list(buf)

    def barrier(self):
        self.all_reduce_scalars([0.0])

    def close(self):
        self._check(self._lib.jh_comm_destroy())


class RowPartitionedOp:
    """This rank's shard of a tall block operator plus the exchange step."""

    def __init__(self, part: RowPartition, local_op, comm: Comm, local_mul: Callable, local_mul_adj: Callable,
                 local_dot: Callable, local_norm: Callable, pipelined_adj: Callable | None = None,
                 pipelined_step: Callable | None = None, pipelined_normal: Callable | None = None,
                 local_normal: Callable | None = None, chains=None, grid_n: int | None = None):
        self.part, self.local_op, self.comm = part, local_op, comm
        self._grid_n = grid_n                  # the block length when local_op is an N x (2 .. 4) grid of equal blocks (its ranges are cut over it), else None
        self._mul, self._mul_adj, self._dot, self._norm = local_mul, local_mul_adj, local_dot, local_norm
        self._pipelined_adj = pipelined_adj   # optional: local adjoint and all-reduce pipelined chunk by chunk
        self._pipelined_step = pipelined_step  # optional: one-pass Golub-Kahan step, its w all-reduced chunk by chunk; returns the global ||u||^2
        self._pipelined_normal = pipelined_normal  # optional: the fused A'A, its result all-reduced chunk by chunk
        self._local_normal = local_normal      # optional: this rank's L'L m in one fused pass (a weighted shard's NORMAL chain), no range temporary
        self._chains = chains                  # the device handles a weighted shard's routes hold (released by close())

    @property
    def fused_normal(self) -> bool:
        """normal_mul_ needs no range temporary: a weighted shard (L = W_loc o A_loc, ...) applies L'L as one fused NORMAL chain.  Read per
        application: a run through a grid exists only while the knob grid_chain_range is 1 (_ShardChains.has_normal)."""
        return self._local_normal is not None and (self._chains is None or self._chains.has_normal)

    @property
    def chain_step(self) -> bool:
        """bidiag_step_ runs a weighted shard's one-pass chain step range by range (jh_chain_bidiag_step_range): no range temporary."""
        return self._chains is not None and self._chains.has_step and self._pipelined_step is not None

    @property
    def grid_range(self) -> bool:
        """The local operator is an N x (2 .. 4) grid whose adjoint, A'A and one-pass step run range by range (knob grid_range = 1): the
        ranges are cut over the block length, a finished range's K pieces are exchanged under the next range's kernel."""
        return self._pipelined_step is not None and self._grid_n is not None and _grid_range_on()

    def close(self):
        """Release the chain handles of a weighted shard (the operator itself stays the caller's)."""
        if self._chains is not None:
            self._chains.close()

    def normal_mul_(self, y, m, tmp_local=None, force_collective: bool = False):
        """y = (A'A) m = sum over ALL rows A_i'(A_i m)  (JetComposite_df! over (A', A), src/Jets.jl:530-534, on a row partition): every
        rank's fused A_k'A_k m -- its coefficients read once, no range-side intermediate -- in element ranges
        (jh_blockop_normal_mul_range), the all-reduce of a finished range under the next range's kernel.  Operators without the
        fused kernel run forward then adjoint through `tmp_local` (a range vector of this rank's rows).  A weighted shard (L = W_loc o A_loc,
        a * (W o A), W o A o M: one fused run of the chain planner) runs L'L = A'W'WA as ONE NORMAL chain per range (jh_chain_apply_range), exchanged
        the same way -- or, unpipelined, the whole-vector NORMAL chain and one all-reduce; it needs no `tmp_local`."""
        if self.fused_normal_mul_(y, m, force_collective=force_collective, pipelined_only=tmp_local is not None):
            return y
        if tmp_local is None:
            raise ValueError("normal_mul_: this operator has no fused A'A; pass tmp_local (a range vector of this rank's rows)")
        self.mul_(tmp_local, m)
        return self.mul_adj_(y, tmp_local, force_collective=force_collective)

    def fused_normal_mul_(self, y, m, force_collective: bool = False, pipelined_only: bool = False) -> bool:
        """normal_mul_ where it needs no range temporary: the ranged fused A'A (or NORMAL chain) with its pipelined exchange, else a weighted
        shard's whole-vector NORMAL chain and one all-reduce.  False -- nothing enqueued, y untouched -- when the operator has neither, or the
        library declines the ranged call on its first range: the caller then applies A and A' through a range vector."""
        if self._pipelined_normal is not None and (self.comm.world > 1 or force_collective):
            if self._pipelined_normal(y, self.local_op, m):
                return True
        if pipelined_only or not self.fused_normal:
            return False
        self._local_normal(y, self.local_op, m)
        self.comm.all_reduce_sum_(y, force=force_collective)
        return True

    def bidiag_step_(self, u_local, v, w, alpha: float, beta: float, force_collective: bool = False):
        """u_local <- alpha*(A_local v) + beta*u_local ; w <- sum over ALL ranks of A_local' u_local, the all-reduce of a
        finished chunk of w overlapping the kernel of the next.  Returns the GLOBAL ||u||^2, or None when the local
        operator has no ranged one-pass kernel (the caller then runs the step in one piece).  A weighted shard (L = W_loc o A_loc, ...) runs
        its FORWARD chain's step range by range (jh_chain_bidiag_step_range) the same way."""
        if self._pipelined_step is None or not (self.comm.world > 1 or force_collective):
            return None
        return self._pipelined_step(u_local, v, w, alpha, beta)

    def mul_(self, d_local, m):
        """d_local = A[rows of this rank] m   -- no communication."""
        return self._mul(d_local, self.local_op, m)

    def mul_adj_(self, m, d_local, force_collective: bool = False):
        """m = sum over ALL rows A_i' d_i  -- local ordered sum, then one all-reduce (or, with the device wiring,
        the two pipelined chunk by chunk: all-reduce of chunk k overlaps the kernel of chunk k+1)."""
        if self._pipelined_adj is not None and (self.comm.world > 1 or force_collective):
            if self._pipelined_adj(m, self.local_op, d_local):
                return m
        self._mul_adj(m, self.local_op, d_local)
        return self.comm.all_reduce_sum_(m, force=force_collective)

    def dot_range(self, x_local, y_local) -> float:
        return self.comm.all_reduce_scalars([float(self._dot(x_local, y_local))], "sum")[0]

    def norm_range(self, x_local, p: float = 2) -> float:
        if p == 2:
            return math.sqrt(self.comm.all_reduce_scalars([float(self._norm(x_local, 2)) ** 2], "sum")[0])
        if p == math.inf:
            return self.comm.all_reduce_scalars([float(self._norm(x_local, p))], "max")[0]
        if p == -math.inf:
            return self.comm.all_reduce_scalars([float(self._norm(x_local, p))], "min")[0]
        if p in (0, 1):
            return self.comm.all_reduce_scalars([float(self._norm(x_local, p))], "sum")[0]
        return self.comm.all_reduce_scalars([float(self._norm(x_local, p)) ** p], "sum")[0] ** (1.0 / p)


class _ShardChains:
    """The fused chains of a WEIGHTED shard: a local operator L that the chain planner (chains.py) turns into one run around the shard's
    tall operator -- W_loc o A_loc (W_loc = JopDiagonal of this rank's rows of the weights), a block-diagonal @blockop of weights o A_loc,
    W o A o M, a * (W o A); with the knob grid_chain_range = 1 also around a native N x (2 .. 4) grid of equal blocks.  adjoint(L) is one ADJOINT chain, adjoint(L) o L one NORMAL chain (W' and W read one coefficient stream:
    jh_chain_create's dedupe), L itself one FORWARD chain whose Golub-Kahan step runs range by range (jh_chain_bidiag_step_range: LSQR / CGLS
    on the shard; JETS_CHAIN_STEP=0 keeps the chain into a range temporary, as chains.SolverChains does on one GPU).  Planned here once; the handles live in this object's cache until close().  A bare block operator is not
    weighted: plain shards keep their routes (jh_blockop_*_range)."""

    def __init__(self, L):
        import os

        from . import chains as _chn
        from . import jetblock as _blk
        from .jets import JopLn, JopAdjoint, adjoint, compose, jops_comp

        self._chn = _chn
        self.cache = _chn.ChainCache()
        self._adj = self._nrm = self._nrm_op = self._fwd = None
        if isinstance(L, (JopLn, JopAdjoint)) and not _blk.isblockop(L) and len(jops_comp(L)) >= 2:
            self._nrm_op = compose(adjoint(L), L)
            self._adj = _chn.stages_of(adjoint(L))
            self._nrm = _chn.stages_of(self._nrm_op)
            if os.environ.get("JETS_CHAIN_STEP", "1") != "0":
                self._fwd = _chn.stages_of(L)
        # the block length when the operator inside L is a device-native N x (2 .. 4) grid of equal blocks: its chains' ranged calls take positions
        # inside a block (knob grid_chain_range, read per application: has_adj / has_normal / has_step), the ranges are cut over it
        self.grid_n = None
        self._has_adj = self._planned(self._adj, "rowpart_adj", _chn.CHAIN_ADJOINT)
        self._has_normal = self._planned(self._nrm, "rowpart_normal", _chn.CHAIN_NORMAL)
        self._has_step = self._planned(self._fwd, "rowpart_fwd", _chn.CHAIN_FORWARD)

    def _planned(self, stages, tag, ctype) -> bool:
        """Is the stage list one fused run -- around a tall operator, or through a grid of equal blocks (then grid_n is its block length)?"""
        anchor = None if stages is None else self._chn.run_anchor(stages, self.cache, tag, ctype)
        if anchor is None:
            return False
        if anchor.kind != "grid":
            return True
        n = _grid_block_len(anchor.base)
        if n is None:
            return False
        self.grid_n = n
        return True

    def _grid_on(self, step: bool = False) -> bool:
        """A tall run: yes.  A run through a grid: does the library take its ranged form in the CURRENT context (knob grid_chain_range = 1, the
        default is 0: no grid chain is planned, the shard keeps its previous routes call for call; the step needs grid_chain_step = 1 as well)?"""
        if self.grid_n is None:
            return True
        return _grid_chain_range_on() and (not step or self._chn.grid_step_enabled())

    @property
    def has_adj(self) -> bool:
        return self._has_adj and self._grid_on()

    @property
    def has_normal(self) -> bool:
        return self._has_normal and self._grid_on()

    @property
    def has_step(self) -> bool:
        return self._has_step and self._grid_on(step=True)

    @has_step.setter
    def has_step(self, value: bool):
        self._has_step = bool(value)

    @property
    def normal_planned(self) -> bool:
        """adjoint(L) o L is one fused run, whatever the knobs say now (has_normal says whether it may run in the current context)."""
        return self._has_normal

    def _one_run(self, stages, tag, ctype):
        return self._chn.one_run(stages, self.cache, tag, ctype, grid=self.grid_n is not None)

    def adjoint(self):
        """The ChainHandle of adjoint(L), or None (not one run; the library declined)."""
        return self._one_run(self._adj, "rowpart_adj", self._chn.CHAIN_ADJOINT) if self.has_adj else None

    def normal(self):
        return self._one_run(self._nrm, "rowpart_normal", self._chn.CHAIN_NORMAL) if self.has_normal else None

    def step(self):
        """The FORWARD ChainHandle of L (its ranged Golub-Kahan step: ChainHandle.bidiag_step_range), or None."""
        return self._one_run(self._fwd, "rowpart_fwd", self._chn.CHAIN_FORWARD) if self.has_step else None

    def local_normal(self, y, L, m):
        """y = L'L m on this rank's rows: the whole-vector NORMAL chain (the stage-by-stage chain when the library declines it)."""
        from .jets import mul_

        h = self.normal()
        if h is None:
            return mul_(y, self._nrm_op, m)
        h.apply(y, m)
        self._chn.STATS["chain_calls"] += 1
        return y

    def close(self):
        self.cache.close()


def for_device(part: RowPartition, local_op, comm=None) -> RowPartitionedOp:
    """Product wiring: HIP kernels for the local work, RCCL for the exchange -- through torch.distributed's "nccl"
    backend (default; the all-reduce is ordered against the library's HIP stream with torch.cuda.ExternalStream)
    or through the C ABI's own RCCL entry points when an AbiComm is passed.  Any other `comm` gets the unpipelined routes."""
    from .arrays import dot, norm
    from .jets import mul_, adjoint

    xch = None
    if comm is None:
        xch = _TorchExchange()
        comm = xch.comm
    elif isinstance(comm, AbiComm):
        xch = _AbiExchange()
    sc = _ShardChains(local_op)
    routes = {} if xch is None else _pipelined_routes(xch, local_op, sc)
    return RowPartitionedOp(part, local_op, comm, lambda d, A, m: mul_(d, A, m), lambda m, A, d: mul_(m, adjoint(A), d), dot, norm,
                            local_normal=sc.local_normal if sc.normal_planned else None, chains=sc, grid_n=_grid_block_len(local_op), **routes)


class _TorchExchange:
    """The exchange of the torch.distributed wiring: a range of a vector is all-reduced on RCCL's stream (torch.cuda.ExternalStream of
    the library stream: RCCL's stream waits for the library stream up to there); join makes the library stream wait for every range."""

    def __init__(self):
        import torch
        import torch.distributed as dist

        from . import device as _device

        self._torch, self._dist, self._device = torch, dist, _device
        self._ext = torch.cuda.ExternalStream(_device.stream_handle(), device=torch.device("cuda", _device.init()))
        self.comm = Comm(self._as_tensor, lambda: torch.cuda.stream(self._ext))
        self._views = {}    # id(vector) -> (vector, flat torch view): a solver exchanges the same one or two vectors every iteration
        self._t, self._works = None, []

    def _as_tensor(self, x):
        # RCCL needs a contiguous tensor: hand it the flat 1-D view of the slab (shares memory with x)
        flat = x if len(x.shape) == 1 else x.reshape((x.length(),))
        t = self._torch.as_tensor(flat, device=self._torch.device("cuda", self._device.init()))
        t._jets_owner = flat  # keep the view alive while torch holds the pointer
        return t

    def ready(self) -> bool:
        return self._dist.is_initialized()

    def open(self, x):
        """Start the exchange of `x`, range by range."""
        hit = self._views.get(id(x))
        if hit is None or hit[0] is not x:
            if len(self._views) >= 8:                         # bounded: a view pins its vector (64 MiB at the headline size)
                self._views.clear()
            hit = self._views[id(x)] = (x, self._as_tensor(x))
        self._t, self._works = hit[1], []

    def send(self, lo: int, cnt: int):
        with self._torch.cuda.stream(self._ext):
            self._works.append(self._dist.all_reduce(self._t[lo:lo + cnt], op=self._dist.ReduceOp.SUM, async_op=True))

    def join(self):
        with self._torch.cuda.stream(self._ext):
            for w in self._works:
                w.wait()

    def normsq(self) -> float:
        """The step's global ||u||^2: the one read-back of the library stream's accumulator (kernels only, not the exchange), the join,
        then the scalar all-reduce."""
        from ._ffi import lib, check

        out = C.c_double(0)
        check(lib.jh_normsq_read(C.byref(out)))
        self.join()
        return self.comm.all_reduce_scalars([out.value], "sum")[0]


class _AbiExchange:
    """The exchange of the AbiComm wiring (what a host without torch.distributed gets): the C ABI's own communicator and exchange stream."""

    def __init__(self):
        from ._ffi import lib, check

        self._lib, self._check = lib, check
        self._x = None

    def ready(self) -> bool:
        return True                                           # (with one rank the caller only comes here when forced: validation)

    def open(self, x):
        self._x = x

    def send(self, lo: int, cnt: int):
        self._check(self._lib.jh_comm_allreduce_sum_range(self._x.handle, lo, cnt))

    def join(self):
        self._check(self._lib.jh_comm_join())

    def normsq(self) -> float:
        """The step's global ||u||^2 (jh_comm_allreduce_normsq): kernels and ranged all-reduces are complete on return."""
        out = C.c_double(0)
        self._check(self._lib.jh_comm_allreduce_normsq(C.byref(out)))
        return out.value


def _grid_range_on() -> bool:
    """Does the library take the ranged calls of a grid in the CURRENT context (knob grid_range; the default is 0)?"""
    from .device import tune_get

    return tune_get("grid_range") == 1


def _grid_chain_range_on() -> bool:
    """Does the library take the ranged calls of a chain through a grid in the CURRENT context (knob grid_chain_range; the default is 0)?"""
    from .device import tune_get

    return tune_get("grid_chain_range") == 1


def _grid_block_len(A):
    """The block length n of a device-native N x (2 .. 4) grid of equal blocks, else None: a property of the operator, worked out once where
    the routes are built (it walks the N K children).  Whether the ranged calls take such a grid is the knob's to say (_grid_range_on, read
    per application) and then the library's: it declines before anything is touched, and the callers fall back."""
    from . import jetblock as _blk
    from .jets import domain, range_

    if _blk._grid_native(A) is None:
        return None
    nrow, ncol = A.jet.s["ops"].shape
    n = domain(A).length() // ncol
    if any(domain(op).length() != n or range_(op).length() != n for op in A.jet.s["ops"].ravel()):
        return None
    return n


def _grid_chunk_bounds(n: int, nchunks: int):
    """Ranges of positions inside a block of n elements: bounds on 64 KiB boundaries like _chunk_bounds' where the block is that long, else
    on 64-element (>= 256-byte) ones; the last range ends with the block."""
    step = -(-n // nchunks)
    grain = 16384 if step >= 16384 else 64
    step = -(-step // grain) * grain
    lo = 0
    while lo < n:
        cnt = builtins.min(step, n - lo)
        yield lo, cnt
        lo += cnt


def _pipelined(xch, out, nchunks: int, kernel, finish=None, grid_n=None):
    """kernel(lo, cnt) for every element range of `out`, the exchange of a finished range (xch.send) enqueued behind its kernel, so it
    runs under the next range's kernel; then finish() -- by default xch.join(), and True.  None when the library declines
    (JH_ERR_UNSUPPORTED) before anything was enqueued: the caller then takes its unpipelined route.  A decline after that raises.
    grid_n: `out` is the domain vector of a grid of blocks of grid_n elements -- the ranges are positions inside a block and a finished
    range's exchange is its K pieces (k * grid_n + lo, cnt)."""
    from ._ffi import JetsHipError

    from . import chains as _chn

    xch.open(out)
    done = 0
    bounds = _chunk_bounds(out.length(), nchunks) if grid_n is None else _grid_chunk_bounds(grid_n, nchunks)
    pieces = (0,) if grid_n is None else [k * grid_n for k in builtins.range(out.length() // grid_n)]
    try:
        for lo, cnt in bounds:
            kernel(lo, cnt)
            if grid_n is not None:
                _chn.STATS["grid_range_calls"] += 1
            for at in pieces:
                xch.send(at + lo, cnt)
            done += 1
    except JetsHipError as e:
        if e.status == 4 and done == 0:
            return None
        raise
    if finish is not None:
        return finish()
    xch.join()
    return True


def _pipelined_routes(xch, local_op, sc) -> dict:
    """RowPartitionedOp's pipelined adjoint, fused A'A and one-pass step over the exchange `xch` (_TorchExchange or _AbiExchange), in
    JETS_AR_CHUNKS element ranges."""
    import os

    from ._ffi import lib, check
    from . import jetblock as _blk

    nchunks = int(os.environ.get("JETS_AR_CHUNKS", "4"))
    local_n = _grid_block_len(local_op)

    def grid_n_of(A):
        """The block length to cut over when `A` is a grid and the knob is on (read per application), else None: the flat domain."""
        n = local_n if A is local_op else _grid_block_len(A)
        return n if n is not None and _grid_range_on() else None

    def native_of(A):
        if nchunks <= 1 or not xch.ready() or not _blk.isblockop(A):
            return None
        jt = A.jet
        return _blk._native_op(jt.s.get("_native"), jt.s["ops"], jt.rng.eltype())

    def weighted(out, x, h):
        """A weighted shard's ADJOINT / NORMAL chain range by range (jh_chain_apply_range, accumulate 0: with +-1 every rank would add `out`
        once).  False when there is no handle.  A chain through a grid (knob grid_chain_range = 1): the ranges are positions inside a block, a
        finished range goes out as its K pieces."""
        if nchunks <= 1 or not xch.ready() or h is None:
            return False
        return _pipelined(xch, out, nchunks, lambda lo, cnt: h.apply_range(out, x, lo, cnt, 0), grid_n=h.block_len)

    def pipelined_adj(m, A, d):
        """Local adjoint in `nchunks` element ranges (jh_blockop_mul_adj_range), each range's all-reduce under the next range's kernel.
        Same values as the unpipelined path.  Falsy when the operator has no ranged kernel (then the caller does it in one piece)."""
        nat = native_of(A)
        if nat is None:
            return A is local_op and sc.has_adj and weighted(m, d, sc.adjoint())
        return _pipelined(xch, m, nchunks, lambda lo, cnt: check(lib.jh_blockop_mul_adj_range(nat.handle, m.handle, d.handle, lo, cnt)),
                          grid_n=grid_n_of(A))

    def pipelined_normal(y, A, m):
        """The fused A'A in `nchunks` element ranges (jh_blockop_normal_mul_range), exchanged like the adjoint's."""
        nat = native_of(A)
        if nat is None:
            return A is local_op and sc.has_normal and weighted(y, m, sc.normal())
        return _pipelined(xch, y, nchunks, lambda lo, cnt: check(lib.jh_blockop_normal_mul_range(nat.handle, y.handle, m.handle, lo, cnt)),
                          grid_n=grid_n_of(A))

    def pipelined_step(u, v, w, alpha, beta):
        """jh_blockop_bidiag_step in `nchunks` element ranges, enqueued back to back: every range adds its share of ||u||^2 to a device-side
        accumulator (jh_normsq_reset / normsq == NULL), so the host synchronises ONCE per step, after the last range (xch.normsq), while the
        all-reduces of the finished ranges of w run under the later kernels.  Returns the GLOBAL ||u||^2, or None when the operator has no
        ranged one-pass kernel.  A weighted shard: the same shape over its FORWARD chain's ranged step (jh_chain_bidiag_step_range)."""
        nat = native_of(local_op)
        if nat is None:
            h = sc.step() if nchunks > 1 and xch.ready() and sc.has_step else None
            if h is None:
                return None
            check(lib.jh_normsq_reset())
            r = _pipelined(xch, w, nchunks, lambda lo, cnt: h.bidiag_step_range(u, v, w, alpha, beta, lo, cnt), finish=xch.normsq, grid_n=h.block_len)
            if r is None:                                     # the library declined before anything was touched (R + R^H above four stages): for good
                sc.has_step = False
            return r
        check(lib.jh_normsq_reset())
        return _pipelined(xch, w, nchunks, lambda lo, cnt: check(lib.jh_blockop_bidiag_step_range(
            nat.handle, u.handle, v.handle, w.handle, float(alpha), float(beta), lo, cnt, None)), finish=xch.normsq, grid_n=grid_n_of(local_op))

    return dict(pipelined_adj=pipelined_adj, pipelined_step=pipelined_step, pipelined_normal=pipelined_normal)


def _chunk_bounds(n: int, nchunks: int):
    step = -(-n // nchunks)
    step = -(-step // 16384) * 16384                          # chunk bounds on 64 KiB boundaries
    lo = 0
    while lo < n:
        cnt = builtins.min(step, n - lo)
        yield lo, cnt
        lo += cnt


# ------------------------------------------------------------------ ONE process, several contexts -------------------------
class TeamVec:
    """One vector per member of a single-process team: a RANGE-side TeamVec holds every member's rows, a DOMAIN-side one
    the members' replicas (kept identical by running the same deterministic updates on each)."""

    def __init__(self, members):
        self.members = list(members)

    def __len__(self):
        return len(self.members)

    def __getitem__(self, k):
        return self.members[k]

    def close(self):
        for x in self.members:
            x.close()


class Team:
    """SURVEY section 8e's single-process form: this process holds one context per GPU (`device.context_create` /
    `init(device)`), `jh_comm_init_all` makes them a team, and the exchange step is the members' all-reduces issued between
    jh_comm_group_begin / jh_comm_group_end.  The members may also be several contexts of ONE GPU (then the grouped sum is a
    device kernel: RCCL refuses two ranks on a device) -- which is how the one-GPU test box exercises this flow.

        team = Team([ctx0, ctx1, ...])
        with using_context(team.contexts[k]): A_k = blockop(rows of member k)      # built by the caller, member by member
        T = team.operator([A_0, A_1, ...])
        T.mul_(d, m); T.mul_adj_(m, d); lsqr(T, b)                                  # d, m, b: TeamVec
    """

    def __init__(self, contexts):
        import ctypes as C

        from ._ffi import lib, check

        self.contexts = [int(c) for c in contexts]
        arr = (C.c_int * len(self.contexts))(*self.contexts)
        check(lib.jh_comm_init_all(len(self.contexts), arr))
        self.world = len(self.contexts)
        self._lib, self._check = lib, check

    def each(self):
        """Iterate over (member index, context id) with that context current."""
        from . import device as _device

        for k, ctx in enumerate(self.contexts):
            _device.context_use(ctx)
            yield k, ctx

    def zeros(self, spaces) -> TeamVec:
        """One zero vector per member: `spaces` is one space (replicated, domain side) or one per member (range side)."""
        from .arrays import zeros

        per = spaces if isinstance(spaces, (list, tuple)) else [spaces] * self.world
        return TeamVec([zeros(per[k]) for k, _ in self.each()])

    def group(self):
        return _TeamGroup(self)

    def operator(self, local_ops) -> "TeamOp":
        return TeamOp(self, local_ops)

    def synchronize(self):
        from . import device as _device

        for _ in self.each():
            _device.synchronize()

    def close(self):
        from . import device as _device

        _device.context_use(self.contexts[0])
        self._check(self._lib.jh_comm_destroy())


class _TeamGroup:
    def __init__(self, team):
        self.team = team

    def __enter__(self):
        from . import device as _device

        _device.context_use(self.team.contexts[0])
        self.team._check(self.team._lib.jh_comm_group_begin())
        return self

    def __exit__(self, et, ev, tb):
        from . import device as _device

        _device.context_use(self.team.contexts[0])
        self.team._check(self.team._lib.jh_comm_group_end())
        return False


class TeamOp:
    """A tall block operator whose rows are spread over the members of a Team: member k holds `local_ops[k]` (built in
    its context).  Forward: every member's rows from its replica of m, no exchange (src/Jets.jl:1015-1031).  Adjoint:
    every member's ordered row sum range by range, the grouped all-reduce of a finished range running on the members'
    exchange streams while the next range computes (1045-1053 summed over members: tolerance parity, like any G > 1)."""

    def __init__(self, team: Team, local_ops):
        import os

        from . import jetblock as _blk

        if len(local_ops) != team.world:
            raise ValueError(f"{team.world} members, {len(local_ops)} operators")
        self.team, self.local_ops = team, list(local_ops)
        self.nchunks = builtins.max(1, int(os.environ.get("JETS_AR_CHUNKS", "4")))
        self.one_call = os.environ.get("JETS_TEAM_ONE_CALL", "1") != "0"    # the member loop in C (round 4); 0: spelled out here, call by call
        self._op_handles = None
        self._natives = []
        for A in self.local_ops:
            nat = None
            if _blk.isblockop(A):
                jt = A.jet
                nat = _blk._native_op(jt.s.get("_native"), jt.s["ops"], jt.rng.eltype())
            self._natives.append(nat)
        # members whose local operators are WEIGHTED chains (W_k o A_k, ...: _ShardChains): the one-pass step and the normal operator range by
        # range through each member's own chain handles, which live in that member's context (built on first use there, released by close())
        self._chains = [None if nat is not None else _ShardChains(A) for nat, A in zip(self._natives, self.local_ops)]
        # members that are N x (2 .. 4) grids of equal blocks of ONE length: the ranges are cut over it when the knob grid_range is 1 (_team_grid_n)
        lens = {_grid_block_len(A) for A in self.local_ops}
        self._grid_n = lens.pop() if len(lens) == 1 else None
        # weighted members whose chains run through grids: of ONE block length, or the ranged chain routes decline (a grid handle reads a range as
        # positions inside its block: flat ranges, or another member's block length, are not its ranges)
        clens = {None if sc is None else sc.grid_n for sc in self._chains}
        self._chain_grids = clens != {None}
        self._chain_grids_mixed = self._chain_grids and len(clens) > 1

    def _team_grid_n(self):
        """The block length to cut the ranges over, or None (the flat domain).  Knobs are per context: grid_range is read in EVERY member's
        context, and members that disagree are an error here, before any member's kernel has touched its u."""
        if self._grid_n is None:
            return None
        on = [_grid_range_on() for _ in self.team.each()]
        if any(on) and not all(on):
            raise ValueError(f"knob grid_range differs between the team's contexts ({[int(v) for v in on]}): set it in every member's context")
        return self._grid_n if on[0] else None

    def _team_chain_grid_n(self, step: bool = False):
        """Weighted members whose chains run through grids of ONE block length: that length when the knob grid_chain_range is 1 (the step: and
        grid_chain_step), else None.  The knobs are read in EVERY member's context; members that disagree are an error here, before any member's
        kernel has touched its u."""
        if not self._chain_grids or self._chain_grids_mixed:
            return None
        n = self._chains[0].grid_n
        for name, on in (("grid_chain_range", [_grid_chain_range_on() for _ in self.team.each()]),
                         ("grid_chain_step", [self._chains[0]._chn.grid_step_enabled() for _ in self.team.each()] if step else [True])):
            if any(on) and not all(on):
                raise ValueError(f"knob {name} differs between the team's contexts ({[int(v) for v in on]}): set it in every member's context")
            if not on[0]:
                return None
        return n

    def _every_member(self, attr: str) -> bool:
        """Does every member's _ShardChains have `attr` (has_adj / has_normal / has_step)?  Chains through grids read their knobs: each member's in
        ITS context (knobs are per context); members of mixed kinds or block lengths have no common ranges."""
        if any(sc is None for sc in self._chains) or self._chain_grids_mixed:
            return False
        if not self._chain_grids:
            return all(getattr(sc, attr) for sc in self._chains)
        return all([getattr(self._chains[k], attr) for k, _ in self.team.each()])

    @property
    def chain_step(self) -> bool:
        """Every member is a weighted chain with a ranged one-pass step (jh_chain_bidiag_step_range)."""
        return self._every_member("has_step")

    @property
    def fused_normal(self) -> bool:
        """Every member is a weighted chain whose normal operator is one NORMAL chain (jh_chain_apply_range): normal_mul_ needs no `tmp`."""
        return self._every_member("has_normal")

    def _member_handles(self, which: str):
        """Every member's chain handle (`step` / `normal` of its _ShardChains), each built in its own context; None when one is missing."""
        hs = [getattr(self._chains[k], which)() for k, _ in self.team.each()]
        return None if any(h is None for h in hs) else hs

    def close(self):
        """Release the members' chain handles, each in its member's context (the operators stay the caller's)."""
        for k, _ in self.team.each():
            if self._chains[k] is not None:
                self._chains[k].close()

    def domain(self):
        from .jets import domain

        return domain(self.local_ops[0])

    def ranges(self):
        from .jets import range_

        return [range_(A) for A in self.local_ops]

    def _handles(self, xs):
        import ctypes as C

        return (C.c_void_p * len(xs))(*[x.handle for x in xs])

    def _team_call(self, fn, outs: TeamVec, ins: TeamVec, *extra) -> bool:
        """The whole member loop behind ONE ABI call (jh_team_mul / jh_team_mul_adj / jh_team_normal_mul): False when a member has
        no native operator or the library says 'unsupported' before anything is enqueued (the callers then take the generic path)."""
        from ._ffi import check, JetsHipError

        if any(n is None for n in self._natives):
            return False
        if self._op_handles is None:
            self._op_handles = self._handles(self._natives)
        try:
            check(fn(self.team.world, self._op_handles, self._handles(outs.members), self._handles(ins.members), *extra))
        except JetsHipError as e:
            if e.status != 4:                                  # JH_ERR_UNSUPPORTED comes before anything is enqueued (every member alike)
                raise
            return False
        return True

    def mul_(self, d: TeamVec, m: TeamVec) -> TeamVec:
        from ._ffi import lib
        from .jets import mul_

        if self.one_call and self._team_call(lib.jh_team_mul, d, m):
            return d
        for k, _ in self.team.each():
            mul_(d[k], self.local_ops[k], m[k])
        return d

    def _ranged(self, m: TeamVec, enqueue_range, native: bool = True) -> bool:
        """For every range of the domain: every member's kernel for it, then the members' all-reduces of it in one group.  native=False: the
        kernels are the members' chains' (weighted members), not their block operators'."""
        from ._ffi import lib, check

        if native and any(n is None for n in self._natives):
            return False
        from . import chains as _chn

        # members that are N x (2 .. 4) grids (knob grid_range = 1): ranges of positions inside a block, a finished range's K pieces exchanged
        # (a group per piece: a group holds one collective per member)
        grid_n = self._team_grid_n() if native else self._team_chain_grid_n()
        bounds = _chunk_bounds(m[0].length(), self.nchunks) if grid_n is None else _grid_chunk_bounds(grid_n, self.nchunks)
        pieces = (0,) if grid_n is None else [k * grid_n for k in builtins.range(m[0].length() // grid_n)]
        for lo, cnt in bounds:
            for k, _ in self.team.each():
                enqueue_range(k, lo, cnt)
                if grid_n is not None:
                    _chn.STATS["grid_range_calls"] += 1
            for at in pieces:
                with self.team.group():
                    for k in builtins.range(self.team.world):
                        check(lib.jh_comm_allreduce_sum_range(m[k].handle, at + lo, cnt))
        for _ in self.team.each():
            check(lib.jh_comm_join())
        return True

    def _ranged_chains(self, out: TeamVec, enqueue_range) -> bool:
        """_ranged over the members' chains.  False when the library declines on the first range of member 0, before anything is touched (a
        grid chain with the knob grid_chain_range back at 0): the caller takes its previous route.  A decline after that raises."""
        from ._ffi import JetsHipError

        done = [0]

        def counted(k, lo, cnt):
            enqueue_range(k, lo, cnt)
            done[0] += 1

        try:
            return self._ranged(out, counted, native=False)
        except JetsHipError as e:
            if e.status == 4 and done[0] == 0 and any(sc is not None and sc.grid_n is not None for sc in self._chains):
                return False
            raise

    def mul_adj_(self, m: TeamVec, d: TeamVec) -> TeamVec:
        from ._ffi import lib, check, JetsHipError
        from .jets import mul_, adjoint

        if self.one_call and self._team_call(lib.jh_team_mul_adj, m, d, self.nchunks):
            return m
        # weighted members whose chains run through grids (knob grid_chain_range = 1): adjoint(L_k) as ONE ADJOINT chain per member and range
        if self._team_chain_grid_n() is not None and self._every_member("has_adj"):
            hs = self._member_handles("adjoint")
            if hs is not None and self._ranged_chains(m, lambda k, lo, cnt: hs[k].apply_range(m[k], d[k], lo, cnt, 0)):
                return m
        try:
            if self._ranged(m, lambda k, lo, cnt: check(lib.jh_blockop_mul_adj_range(self._natives[k].handle, m[k].handle, d[k].handle, lo, cnt))):
                return m
        except JetsHipError as e:
            if e.status != 4:                                  # JH_ERR_UNSUPPORTED comes before anything is enqueued (every member alike)
                raise
        for k, _ in self.team.each():
            mul_(m[k], adjoint(self.local_ops[k]), d[k])
        with self.team.group():
            for k in builtins.range(self.team.world):
                check(lib.jh_comm_allreduce_sum(m[k].handle))
        return m

    def normal_mul_(self, y: TeamVec, m: TeamVec, tmp: TeamVec | None = None) -> TeamVec:
        """y = (A'A) m on every member's replica: the members' fused A_k'A_k m range by range, each range summed over the team under
        the next range's kernels; forward then adjoint through `tmp` (a range-side TeamVec) for operators without the fused kernel.  Members that
        are weighted chains (W_k o A_k, ...) apply L_k'L_k as one NORMAL chain per range (jh_chain_apply_range) and need no `tmp`."""
        from ._ffi import lib, check, JetsHipError

        if self.fused_normal_mul_(y, m):
            return y
        if self.one_call and self._team_call(lib.jh_team_normal_mul, y, m, self.nchunks):
            return y
        try:
            if self._ranged(y, lambda k, lo, cnt: check(lib.jh_blockop_normal_mul_range(self._natives[k].handle, y[k].handle, m[k].handle, lo, cnt))):
                return y
        except JetsHipError as e:
            if e.status != 4:
                raise
        if tmp is None:
            raise ValueError("normal_mul_: this operator has no fused A'A; pass tmp (a range-side TeamVec)")
        return self.mul_adj_(y, self.mul_(tmp, m))

    def fused_normal_mul_(self, y: TeamVec, m: TeamVec) -> bool:
        """normal_mul_ where it needs no range temporary: weighted members' L_k'L_k m as ONE NORMAL chain per member and range.  False -- nothing
        enqueued, y untouched -- when the members have no such chains (chains through grids: the knob grid_chain_range at 0 in their contexts) or the
        library declines the first range: the caller then applies A and A' through a range vector."""
        if not self.fused_normal:
            return False
        hs = self._member_handles("normal")
        return hs is not None and self._ranged_chains(y, lambda k, lo, cnt: hs[k].apply_range(y[k], m[k], lo, cnt, 0))

    def bidiag_step_(self, u: TeamVec, v: TeamVec, w: TeamVec, alpha: float, beta: float):
        """One Golub-Kahan step on every member (jh_blockop_bidiag_step_range per range; weighted members: jh_chain_bidiag_step_range) with the ranged exchange of w;
        returns the GLOBAL ||u||^2 -- the host adds the members' deferred accumulators -- or None without a ranged kernel."""
        import ctypes as C

        from ._ffi import lib, check, JetsHipError

        hs = None
        self._team_chain_grid_n(step=True)                     # (weighted grid members: knobs that differ between the contexts raise here, before any u changes)
        if self.chain_step:                                    # weighted members: jh_chain_bidiag_step_range per member and range
            hs = self._member_handles("step")
            if hs is None:
                return None
        elif any(n is None for n in self._natives):
            return None
        for _ in self.team.each():
            check(lib.jh_normsq_reset())
        try:
            if hs is not None:
                self._ranged(w, lambda k, lo, cnt: hs[k].bidiag_step_range(u[k], v[k], w[k], alpha, beta, lo, cnt), native=False)
            else:
                self._ranged(w, lambda k, lo, cnt: check(lib.jh_blockop_bidiag_step_range(
                    self._natives[k].handle, u[k].handle, v[k].handle, w[k].handle, float(alpha), float(beta), lo, cnt, None)))
        except JetsHipError as e:
            if e.status != 4:                                  # JH_ERR_UNSUPPORTED comes before anything is touched (member 0, the first range)
                raise
            if hs is not None:
                for sc in self._chains:
                    sc.has_step = False
            return None
        total = 0.0
        out = C.c_double(0)
        for _ in self.team.each():
            check(lib.jh_normsq_read(C.byref(out)))          # synchronises this member's stream
            total += out.value
        return total
