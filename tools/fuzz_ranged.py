#!/usr/bin/env python3
"""Seeded random differential of the ranged calls and one-pass Golub-Kahan steps against the CPU oracle's stage-by-stage loops.

    python tools/fuzz_ranged.py NCASES [SEED0]            (one MI355X; the families round-robin, seeds SEED0, SEED0 + 1, ...)

Five families: tall_step_range (jh_chain_bidiag_step_range on a tall FORWARD chain), tall_apply_range (jh_chain_apply_range on tall ADJOINT and
NORMAL chains), grid_range (jh_blockop_mul_adj_range / normal_mul_range / bidiag_step_range on a bare N x K grid, knob grid_range), grid_chain_step
(the whole-vector jh_chain_bidiag_step on a grid FORWARD chain, knob grid_chain_step) and grid_chain_range (jh_chain_apply_range and
jh_chain_bidiag_step_range on grid chains, knobs grid_chain_range and grid_chain_step).

draw(family, seed) is pure numpy: element type, K, N, block length (on and off the 16-byte grid, several workgroups ending in a partial pack),
row kinds, stage lists, the row walk (adj_split 0 / forced parts / the launcher's own choice on many rows), a tiling of the block into 1 .. 7
ranges on the 16-byte grid (empty ranges, a one-pack range, the partial last pack alone) applied in a random order, alpha, beta (0: the u found
is all NaN), the shares of ||u||^2 read back or deferred, `accumulate`.  tests/test_random_ranged_cases.py checks on any machine that the
seed list of tests/test_gpu_random_ranged.py covers all of that and that the reference assembled range by range is the whole-vector reference.

run_case(J, oracle, case) builds the operator on the device and in the oracle (the rigs of the chain tests) and yields records
("same", what, got, want) -- bit for bit -- and ("verdict", what, True | text).  The reference is never a device call.  After EVERY ranged call:
inside the ranges done so far u and the output have the oracle's bits, outside them the bits they held before the first call.  Where the rows were
summed in parts (last_adj_parts > 1) the output is held to the bound the project asserts for that family's split walk (check_specials:
_chain_tol, _allclose_ok, _relerr_ok) against the oracle's ORDERED result; u stays bit-exact; two runs give the same bits; the part count is the
launchers' rule (expected_parts).  Shares of ||u||^2: each one, and their sum, within 1e-12 relative of the fp64 sum over the oracle's u.

A range-side list holds at most two stages in the FORWARD and NORMAL chains (the step and the NORMAL program keep R and R^H in four stages), so two
weights leave no room for the scalar; a chain with no stage at all gets the scalar (a bare operator is no chain)."""
import copy
import ctypes as C
import os
import sys
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
import numpy as np

import check_specials as cs

FAMILIES = ("tall_step_range", "tall_apply_range", "grid_range", "grid_chain_step", "grid_chain_range")
DTYPES = ("float32", "float64", "complex64", "complex128")
NSET = (2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 33, 40)
MANY_ROWS = (300, 520)
MANY_BASE = 100000                       # seeds from here on: many rows of short blocks at the launcher's own adj_split
SPLITS = (0, 0, 2, 3, 5)
ALPHAS = (1.25, 1.375, -0.5, 0.75)
BETAS = (0.0, -0.5, -0.625, 1.0)
ACCS = (0, 1, -1, 2, -2)
SCALARS = (0.75, -1.25, 2.5, 0.375)
WG_LANES = 256                           # lanes of one pack per workgroup


def pack_elems(dt):
    """Elements per 16 bytes."""
    return max(1, 16 // np.dtype(dt).itemsize)


def has_ranges(family):
    return family != "grid_chain_step"


def has_step(family):
    return family != "tall_apply_range"


def has_apply(family):
    return family in ("tall_apply_range", "grid_chain_range")


def rows_in_flight(case):
    """DEPTH of the grid kernels: 4 rows per batch at K = 2, 2 at K = 3, 4 (the chains' kernels: 2; tall chains 4, their step 2)."""
    if case["K"] == 1:
        return 2 if case["family"] == "tall_step_range" else 4
    return 4 if case["K"] == 2 and case["family"] == "grid_range" else 2


# ------------------------------------------------------------------------------------------------------------ the generator
def _block_length(rng, p, nmax, many):
    if rng.random() < 0.5:                                                     # on the 16-byte grid; often exactly 1, 2, 3 workgroups
        if not many and rng.random() < 0.4:
            return WG_LANES * p * int(rng.integers(1, 4))
        return p * int(rng.integers(1, nmax // p + 1))
    n = int(rng.integers(p, nmax - p))
    if p > 1 and n % p == 0:
        n += int(rng.integers(1, p))                                           # off the grid wherever the type has one (16-byte elements have none)
    return n


def _tiling(rng, n, p):
    """Ranges (first, count) that tile [0, n), bounds on the 16-byte grid, in the order they are applied."""
    last_pt = (n - 1) // p                                                     # cuts are p * j, 0 <= j <= last_pt: inside the block
    nr = int(rng.integers(1, 8))
    tail, one, dup, perm = rng.random() < 0.35, rng.random() < 0.35, rng.random() < 0.25, rng.random() < 0.8
    special = []
    if tail and last_pt >= 1:
        special.append(last_pt)                                                # the final range: the partial pack alone (on the grid: one pack)
    if one and last_pt >= 1:
        j = int(rng.integers(0, last_pt))
        special += [j, j + 1]                                                  # [p j, p (j + 1)): exactly one pack
    special = [j for j in dict.fromkeys(special) if j > 0]
    nr = max(nr, len(special) + 1)
    cuts = special + [int(j) for j in rng.integers(0, last_pt + 1, size=nr - 1 - len(special))]
    if dup and len(cuts) >= 1 and len(cuts) < 6:
        cuts.append(cuts[int(rng.integers(0, len(cuts)))])                     # a duplicate cut: an empty range
    b = [0] + sorted(p * j for j in cuts) + [n]
    ranges = [(b[i], b[i + 1] - b[i]) for i in range(len(b) - 1)]
    order = rng.permutation(len(ranges)) if perm else np.arange(len(ranges))
    return [ranges[int(i)] for i in order]


def _stages(rng, grid, allow_wb):
    """(fwd, adj, nrm) token lists in application order (tests/test_gpu_chains.py: Rig) of L = R o A o P, adjoint(L), adjoint(L) o L."""
    nw = int(rng.integers(0, 3))
    wb_at = int(rng.integers(0, max(nw, 1))) if rng.random() < 0.3 else -1
    R = []
    for k in range(nw):
        conj = bool(rng.integers(0, 2))
        R.append(("Wb", 0 if grid else k, conj) if (k == wb_at and allow_wb) else ("W", k, conj))
    scal, a, at = rng.random() < 0.5, float(rng.choice(SCALARS)), rng.random()
    dom, mk, mconj = rng.random() < 0.5, int(rng.integers(0, 2)), bool(rng.integers(0, 2))
    if nw == 2:
        scal = False
    if not R and not dom:
        scal = True
    if scal:
        R.insert(int(at * (len(R) + 1)), ("s", a, "r"))
    fwd = ([("M", mk, mconj)] if dom else []) + ["A"] + R
    adj = cs.adjoint_tokens(fwd)
    return fwd, adj, fwd + adj


def draw(family, seed):
    """The case (a dict of plain values) of one family and one seed; seeds >= MANY_BASE: 300 / 520 rows of blocks of at most 600 elements."""
    fam = FAMILIES.index(family)
    rng = np.random.default_rng([fam, seed])
    many, s = seed >= MANY_BASE, seed % MANY_BASE
    grid = family.startswith("grid")
    dtype = DTYPES[s % 4]
    K = 2 + (s // 4) % 3 if grid else 1
    p = pack_elems(dtype)
    n = _block_length(rng, p, 600 if many else 6000, many)
    kinds = str(rng.choice(["plain", "mixed", "regularised"], p=[0.4, 0.4, 0.2])) if grid else str(rng.choice(["plain", "mixed"]))
    pool = MANY_ROWS if many else tuple(N for N in NSET if kinds != "regularised" or N > K)
    N = int(rng.choice(pool))
    split = -1 if many else int(rng.choice(SPLITS))
    ranges = _tiling(rng, n, p)
    alpha, beta, deferred = float(rng.choice(ALPHAS)), float(rng.choice(BETAS)), bool(rng.integers(0, 2))
    if family == "grid_range":
        fwd, adj, nrm = ["A"], ["At"], ["A", "At"]
    else:
        fwd, adj, nrm = _stages(rng, grid, allow_wb=not many)
    return dict(family=family, seed=int(seed), dtype=dtype, K=K, N=N, n=n, kinds=kinds, adj_split=split,
                ranges=ranges if has_ranges(family) else [(0, n)], alpha=alpha, beta=beta, deferred=deferred and has_ranges(family),
                acc=ACCS[(s // 3) % 5], fwd=fwd, adj=adj, nrm=nrm, with_wb=any(t[0] == "Wb" for t in fwd if t != "A"))


SUITE_SEEDS = tuple(range(40)) + (MANY_BASE, MANY_BASE + 1)


def suite_cases():
    """The cases of tests/test_gpu_random_ranged.py: forty seeds per family and two many-rows cases."""
    return [draw(f, s) for f in FAMILIES for s in SUITE_SEEDS]


def case_id(case):
    r = case["ranges"]
    asc = all(r[i][0] + r[i][1] <= r[i + 1][0] for i in range(len(r) - 1))
    walk = {-1: "auto", 0: "ordered"}.get(case["adj_split"], f"parts{case['adj_split']}")
    flags = ("" if asc else "p") + ("e" if any(c == 0 for _, c in r) else "")
    return (f"{case['family']}-s{case['seed']}-{case['dtype']}-{case['N']}x{case['K']}x{case['n']}-{case['kinds']}-{walk}-"
            f"{len(r)}r{flags}-b{case['beta']}-a{case['acc']}")


def expected_parts(case, count):
    """The launchers' rule (pick_adj_parts and what follows it) for a range of `count` elements; None: the launcher's own choice (adj_split -1)."""
    split, N = case["adj_split"], case["N"]
    if split < 0:
        return None
    span, ns = count * cs.scalars_per_elem(case["dtype"]), cs.scalars_per_pack(case["dtype"])
    if split == 0 or N < 4 or span < ns:                                       # (a range shorter than one pack loads from before its start: one part)
        return 1
    parts = min(split, N // 2)
    if parts < 2:
        return 1
    rpp = -(-N // parts)
    return -(-N // rpp)


def mask(nblk, n, ranges):
    """Positions [first, first + count) of each of `nblk` blocks of n elements, over the flat vector."""
    m = np.zeros(nblk * n, dtype=bool)
    for lo, cnt in ranges:
        for k in range(nblk):
            m[k * n + lo:k * n + lo + cnt] = True
    return m


# ------------------------------------------------------------------------------------------------------------ the reference
class _HostSpace:
    def __init__(self, dt, lens):
        self.dt, self.lens = dt, list(lens)

    def length(self):
        return int(sum(self.lens))


class _HostVec:
    def __init__(self, a, spc):
        self.a, self.spc = a, spc

    def to_numpy(self):
        return self.a

    @property
    def arrays(self):
        offs = np.concatenate([[0], np.cumsum(self.spc.lens)]).astype(int)
        return [_HostVec(self.a[offs[i]:offs[i + 1]], _HostSpace(self.spc.dt, [self.spc.lens[i]])) for i in range(len(self.spc.lens))]


class _HostOp:
    def __init__(self, dom, rng):
        self.dom, self.rng = dom, rng

    @property
    def H(self):
        return _HostOp(self.rng, self.dom)


class HostJ:
    """A stand-in for the package that lets the rigs build their ORACLE side with no device: vectors are host arrays, operators know their spaces only."""
    constdiag_df = constdiag_df_adj = None

    def __init__(self, oracle):
        self.o = oracle

    def JetSpace(self, dt, *shape):
        return _HostSpace(dt, [int(np.prod(shape))])

    def rand(self, spc, seed=0, stream=0):
        return _HostVec(self.o.rng_u01(spc.dt, seed, stream, 0, spc.length()), spc)

    def from_numpy(self, a, spc=None):
        return _HostVec(np.asarray(a), spc)

    def JopDiagonal(self, v):
        return _HostOp(v.spc, v.spc)

    def JopZeroBlock(self, dom, rng):
        return _HostOp(dom, rng)

    def JopIdentity(self, spc):
        return _HostOp(spc, spc)

    def JopLn(self, dom=None, rng=None, **kw):
        return _HostOp(dom, rng)

    def blockop(self, rows):
        dt = rows[0][0].dom.dt
        return _HostOp(_HostSpace(dt, [op.dom.length() for op in rows[0]]), _HostSpace(dt, [row[0].rng.length() for row in rows]))

    def range(self, A):
        return A.rng

    def domain(self, A):
        return A.dom

    def close(self, A):
        pass


def _regularised(N, K):
    """[A; lam I] as tests/test_gpu_grid_range.py draws it: N - K rows of diagonals (one block adjointed), then K rows of one scalar / identity block."""
    kinds = [["diag"] * K for _ in range(N - K)]
    kinds[0][K - 1] = "diag_adj"
    return kinds + [[("scale" if r % 2 == 0 else "identity") if k == r else "zero" for k in range(K)] for r in range(K)]


def build_rig(J, oracle, case):
    dt, N, K, n = np.dtype(case["dtype"]).type, case["N"], case["K"], case["n"]
    if K == 1:
        from tests.test_gpu_chains import Rig

        return Rig(J, oracle, dt, N, n, "diag" if case["kinds"] == "plain" else "mixed", with_wb=case["with_wb"])
    from tests.test_gpu_grid_chains import GridRig, _grid_kinds

    kinds = _regularised(N, K) if case["kinds"] == "regularised" else _grid_kinds(N, K, case["kinds"] == "mixed")
    return GridRig(J, oracle, dt, N, K, n, kinds=kinds, with_wb=case["with_wb"])


def _restricted(rig, lo, cnt):
    """The rig's oracle side on positions [lo, lo + cnt) of every block."""
    sub = copy.copy(rig)
    sub.n = cnt
    sub.ora = []
    for row in rig.ora:
        new = []
        for b in row:
            b2 = copy.copy(b)
            b2.nr = b2.nc = cnt
            b2.coeff = None if b.coeff is None else np.asfortranarray(b.coeff[lo:lo + cnt].copy())
            new.append(b2)
        sub.ora.append(new)
    sub.hw = [[b[lo:lo + cnt].copy() for b in w] for w in rig.hw]
    sub.hc = [([b[lo:lo + cnt].copy() for b in c] if isinstance(c, list) else c[lo:lo + cnt].copy()) for c in rig.hc]
    return sub


class Reference:
    """Host inputs of a case and the oracle's results: counter-generator U[0,1) shifted by a constant, as the range tests draw them."""

    def __init__(self, oracle, case, rig):
        from tests.helpers import u01

        self.o, self.case, self.rig = oracle, case, rig
        dt = self.dt = np.dtype(case["dtype"]).type
        N, K, n = case["N"], case["K"], case["n"]
        host = lambda seed, k, shift: [(u01(oracle, dt, seed, i, n) + dt(shift)).astype(dt) for i in range(k)]
        self.hm, self.hd = host(91, K, -0.5), host(95, N, -0.5)
        self.u0 = [np.full(n, np.nan, dtype=dt) for _ in range(N)] if case["beta"] == 0 else host(93, N, -0.25)
        self.dirty = {"adj": np.concatenate(host(97, K, 1.5)), "nrm": np.concatenate(host(98, K, 1.5)), "w": np.concatenate(host(99, K, 1.5))}

    def compute(self, sub=None):
        """{"adj": (W o A o P)' d, "nrm": L'L m, "u": alpha L m + beta u0, "w": L'u} as flat arrays; sub = (lo, cnt): of those positions only."""
        from tests.test_gpu_grid_step import _host_update

        case, dt = self.case, self.dt
        rig = self.rig if sub is None else _restricted(self.rig, *sub)
        cut = (lambda xs: xs) if sub is None else (lambda xs: [b[sub[0]:sub[0] + sub[1]].copy() for b in xs])
        hm, hd, u0 = cut(self.hm), cut(self.hd), cut(self.u0)
        with np.errstate(all="ignore"):
            out = {"adj": np.concatenate(rig.ora_apply(case["adj"], hd)), "nrm": np.concatenate(rig.ora_apply(case["nrm"], hm))}
            t = rig.ora_apply(case["fwd"], hm)
            u = [np.ascontiguousarray(_host_update(dt, case["alpha"], case["beta"], t[i], u0[i])) for i in range(case["N"])]
            out["u"], out["w"] = np.concatenate(u), np.concatenate(rig.ora_apply(case["adj"], u))
        return out


def reference_by_ranges(oracle, case):
    """(whole, assembled): the oracle's whole-vector results and the same results assembled range by range through mask() -- they must be equal."""
    rig = build_rig(HostJ(oracle), oracle, case)
    ref = Reference(oracle, case, rig)
    whole = ref.compute()
    n, nblk = case["n"], {"adj": case["K"], "nrm": case["K"], "w": case["K"], "u": case["N"]}
    parts = {k: np.full_like(v, np.nan) for k, v in whole.items()}
    for lo, cnt in case["ranges"]:
        if cnt == 0:
            continue
        sub = ref.compute((lo, cnt))
        for k in parts:
            parts[k][mask(nblk[k], n, [(lo, cnt)])] = sub[k]
    return whole, parts


# ------------------------------------------------------------------------------------------------------------ the device side
def _flat(x):
    return x.to_numpy().ravel(order="F").copy()


def _walk(J, case, what, lo, cnt, parts, shape_knob):
    want = expected_parts(case, cnt)
    if want is not None:
        ok = parts == want
        yield ("verdict", f"{what} [{lo}, {lo + cnt}): row parts", True if ok else f"{parts} parts, expected {want} (adj_split {case['adj_split']}, N {case['N']})")
    if shape_knob:
        bit = bool(J.tune_get(shape_knob) & 2)
        yield ("verdict", f"{what} [{lo}, {lo + cnt}): {shape_knob} bit 2", True if bit == (parts > 1) else f"bit 2 is {bit} with {parts} parts")


def _output_records(tag, got, init, want, n, nblk, exact, split, tol_ok):
    me, ms = mask(nblk, n, exact), mask(nblk, n, split)
    yield ("same", f"{tag}: outside the ranges done", got[~(me | ms)], init[~(me | ms)])
    yield ("same", f"{tag}: inside, ordered walk", got[me], want[me])
    if split:
        yield ("verdict", f"{tag}: inside, rows in parts", tol_ok(got[ms], want[ms]))


def _sweep_apply(J, case, what, ranged, fresh, init, want, tol_ok, shape_knob, stats):
    n, K, runs = case["n"], case["K"], []
    for rep in (0, 1):
        out, exact, split = fresh(), [], []
        for lo, cnt in case["ranges"]:
            ranged(out, lo, cnt)
            if cnt:
                parts = J.tune_get("last_adj_parts")
                if rep == 0:
                    yield from _walk(J, case, what, lo, cnt, parts, shape_knob)
                    stats["split" if parts > 1 else "ordered"] += 1
                (split if parts > 1 else exact).append((lo, cnt))
            if rep == 0:
                yield from _output_records(f"{what} after [{lo}, {lo + cnt})", _flat(out), init, want, n, K, exact, split, tol_ok)
        runs.append(_flat(out))
    yield ("same", f"{what}: two runs", runs[0], runs[1])


def _sweep_step(J, case, what, ranged, fresh_u, fresh_w, u0, w0, uref, wref, tol_ok, shape_knob, stats):
    from jets_jl_amd._ffi import check, lib

    n, K, N, deferred, runs = case["n"], case["K"], case["N"], case["deferred"], []
    for rep in (0, 1):
        u, w, exact, split, total = fresh_u(), fresh_w(), [], [], 0.0
        if deferred:
            check(lib.jh_normsq_reset())
        for lo, cnt in case["ranges"]:
            share = ranged(u, w, lo, cnt, not deferred)
            if cnt:
                parts = J.tune_get("last_adj_parts")
                if rep == 0:
                    yield from _walk(J, case, what, lo, cnt, parts, shape_knob)
                    stats["split" if parts > 1 else "ordered"] += 1
                (split if parts > 1 else exact).append((lo, cnt))
            if not deferred:
                total += share
            if rep == 0:
                tag = f"{what} after [{lo}, {lo + cnt})"
                gu, mu = _flat(u), mask(N, n, exact + split)
                yield ("same", f"{tag}: u outside the ranges done", gu[~mu], u0[~mu])
                yield ("same", f"{tag}: u inside", gu[mu], uref[mu])
                yield from _output_records(f"{tag}: w", _flat(w), w0, wref, n, K, exact, split, tol_ok)
                if not deferred:
                    yield ("verdict", f"{tag}: its share of ||u||^2", cs.normsq_verdict(share, uref[mask(N, n, [(lo, cnt)])]))
        if deferred:
            out = C.c_double(-1.0)
            check(lib.jh_normsq_read(C.byref(out)))
            total = out.value
        if rep == 0:
            yield ("verdict", f"{what}: the shares of ||u||^2 ({'deferred' if deferred else 'read back'})",
                   cs.normsq_verdict(total, uref[mask(N, n, exact + split)]))
        runs.append((_flat(u), _flat(w), total))
    yield ("same", f"{what}: u, two runs", runs[0][0], runs[1][0])
    yield ("same", f"{what}: w, two runs", runs[0][1], runs[1][1])
    yield ("verdict", f"{what}: ||u||^2, two runs", True if runs[0][2] == runs[1][2] else f"{runs[0][2]!r} vs {runs[1][2]!r}")


KNOBS = {"tall_step_range": {}, "tall_apply_range": {}, "grid_range": dict(grid_range=1), "grid_chain_step": dict(grid_chain_step=1),
         "grid_chain_range": dict(grid_chain_range=1, grid_chain_step=1)}
DEFAULTS = dict(grid_range=0, grid_chain_range=0, grid_chain_step=0, adj_split=-1)


def run_case(J, oracle, case, stats=None):
    """Records of one case.  The knobs it sets go back to their defaults in its own finally (a generator: close() it)."""
    from jets_jl_amd import chains
    from jets_jl_amd._ffi import check, lib

    stats = stats if stats is not None else {"ordered": 0, "split": 0}
    stats.setdefault("ordered", 0), stats.setdefault("split", 0)
    family, dt, N, K, n = case["family"], np.dtype(case["dtype"]).type, case["N"], case["K"], case["n"]
    alpha, beta, acc = case["alpha"], case["beta"], case["acc"]
    rig = build_rig(J, oracle, case)
    cache = chains.ChainCache()
    try:
        ref = Reference(oracle, case, rig)
        want = ref.compute()
        R, D = J.range(rig.A), J.domain(rig.A)
        m, d = J.from_numpy(np.concatenate(ref.hm), D), J.from_numpy(np.concatenate(ref.hd), R)
        u0 = np.concatenate(ref.u0)
        fresh = lambda a, spc: (lambda: J.from_numpy(a.copy(), spc))
        grid, bare = K > 1, family == "grid_range"
        range_knob = {"grid_range": "last_grid_range_shape", "grid_chain_range": "last_grid_chain_range_shape"}.get(family)

        def handle(toks, ctype):
            h = chains.one_run(chains.stages_of(rig.compose(toks)), cache, f"fuzz_ranged_{ctype}", ctype)
            ok = isinstance(h, chains.ChainHandle) and bool(h.grid) == grid
            return h if ok else None

        J.tune(adj_split=case["adj_split"], **KNOBS[family])
        if has_apply(family) or bare:
            tol = cs._allclose_ok(dt) if grid else cs._abs_ok(cs._chain_tol(dt, N))
            for name, toks, ctype, x in (("adjoint", case["adj"], chains.CHAIN_ADJOINT, d), ("normal", case["nrm"], chains.CHAIN_NORMAL, m)):
                key = "adj" if name == "adjoint" else "nrm"
                init = ref.dirty[key]
                if bare:
                    from tests.test_gpu_grid_step import _native

                    nat = _native(rig.A)
                    fn = lib.jh_blockop_mul_adj_range if name == "adjoint" else lib.jh_blockop_normal_mul_range
                    ranged = lambda out, lo, cnt, fn=fn, x=x: check(fn(nat.handle, out.handle, x.handle, lo, cnt))
                    full = want[key]
                else:
                    h = handle(toks, ctype)
                    if h is None:
                        yield ("verdict", f"{name} {toks}: one fused run" + (" through the grid" if grid else ""), "the planner did not fuse the chain")
                        continue
                    ranged = lambda out, lo, cnt, h=h, x=x: h.apply_range(out, x, lo, cnt, acc)
                    full = cs.accumulated(acc, init, want[key])
                yield from _sweep_apply(J, case, name, ranged, fresh(init, D), init, full, tol, range_knob, stats)
        if has_step(family):
            tol = cs._relerr_ok(dt)
            if bare:
                from tests.test_gpu_grid_step import _native

                nat = _native(rig.A)

                def ranged(u, w, lo, cnt, read):
                    out = C.c_double(0.0)
                    check(lib.jh_blockop_bidiag_step_range(nat.handle, u.handle, m.handle, w.handle, alpha, beta, lo, cnt, C.byref(out) if read else None))
                    return out.value if read else None
            else:
                h = handle(case["fwd"], chains.CHAIN_FORWARD)
                if h is None:
                    yield ("verdict", f"step {case['fwd']}: one fused FORWARD run" + (" through the grid" if grid else ""), "the planner did not fuse the chain")
                    return
                if has_ranges(family):
                    ranged = lambda u, w, lo, cnt, read: h.bidiag_step_range(u, m, w, alpha, beta, lo, cnt, read_normsq=read)
                else:
                    def ranged(u, w, lo, cnt, read):                            # the whole-vector step: one "range", the block
                        out = C.c_double(-1.0)
                        check(lib.jh_chain_bidiag_step(h.handle, u.handle, m.handle, w.handle, alpha, beta, C.byref(out)))
                        return out.value
            knob = range_knob if has_ranges(family) else "last_grid_chain_step_shape"
            yield from _sweep_step(J, case, "step", ranged, fresh(u0, R), fresh(ref.dirty["w"], D), u0, ref.dirty["w"], want["u"], want["w"], tol, knob, stats)
    finally:
        J.tune(**DEFAULTS)
        cache.close()
        rig.close()


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes():
        return None
    return f"{int((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(axis=1).sum()) if a.shape == b.shape else '?'} of {a.size} elements differ bitwise"


def main(argv):
    import jets_jl_amd as J
    from oracle import jets_oracle as oracle

    ncases, seed0 = int(argv[1]), int(argv[2]) if len(argv) > 2 else 0
    J.init(0)
    t0, bad = time.time(), 0
    stats = {f: {"cases": 0, "checks": 0, "ordered": 0, "split": 0} for f in FAMILIES}
    for i in range(ncases):
        family = FAMILIES[i % len(FAMILIES)]
        seed = seed0 + i // len(FAMILIES)
        if i // len(FAMILIES) % 25 == 24:
            seed += MANY_BASE                                                  # one case in 25: many rows at the launcher's own adj_split
        case = draw(family, seed)
        st = stats[family]
        st["cases"] += 1
        records = run_case(J, oracle, case, st)
        try:
            for rec in records:
                st["checks"] += 1
                fail = bits_differ(rec[2], rec[3]) if rec[0] == "same" else (None if rec[2] is True else rec[2])
                if fail:
                    bad += 1
                    print(f"MISMATCH {case_id(case)}: {rec[1]}: {fail}", flush=True)
        finally:
            records.close()
        if (i + 1) % 500 == 0:
            print(f"{i + 1} cases, {time.time() - t0:.0f} s", flush=True)
    per = "; ".join(f"{f}: {s['cases']} cases, {s['checks']} checks, {s['ordered']} ordered / {s['split']} split ranged calls" for f, s in stats.items())
    print(f"fuzz_ranged stats: {per}")
    verdict = "all bit-exact / within bound" if not bad else f"{bad} MISMATCHES"
    print(f"fuzz_ranged: {ncases} cases, seeds {seed0} .. {seed0 + (ncases - 1) // len(FAMILIES)}: {verdict}; {time.time() - t0:.0f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
