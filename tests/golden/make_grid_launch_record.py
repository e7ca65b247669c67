#!/usr/bin/env python3
"""How the one-pass grid kernels and the fused chains are LAUNCHED, and the bits they write (tests/golden/grid_launch_record.json).

    python tests/golden/make_grid_launch_record.py              # rewrites grid_launch_record.json next to this script (needs an MI355X)
    python tests/golden/make_grid_launch_record.py --stdout     # prints the same record of the library as built, writes nothing

The library is the one the package loads: jets.jl_amd/libjetship.so, or the file the environment variable JETSHIP_LIB names.

The launchers of jh_grid_normal.hip, jh_grid_range.hip, jh_grid_step.hip, jh_grid_chain_kernels.h, jh_grid_chain_step.hip and
jh_tall_chain_kernels.h choose a split of the block rows into parts (from the knob adj_split, the row count, the workgroups of the call's
range and the device's CU count), a nontemporal policy and a kernel instantiation.  One case is one call: its parameters, the launch
counters the call writes (read back with jh_tune_get) and 16 hex digits of the SHA-256 of every vector it writes.  Inputs come from a seeded
numpy generator; every output is pre-filled with a fixed non-zero pattern, so the hash of a ranged call also says that nothing outside the
range was written.  Blocks of 515 elements are off the 16-byte grid and end in a partial pack; 5 rows walk in order (with a row-loop tail
at every depth of rows in flight), 600 rows take the automatic split, where the part count is re-derived from the rows per part; the range
[512, 515) is shorter than one pack of 32-bit scalars.

The cases are a covering list, not the product: every (call, range, rows, adj_split) that exists, the other parameters chosen so that
every pair of values of two parameters meets in some case.  Two cases are NOT small: one A'A of a grid and one NORMAL tall chain on 256
rows of 262 147 Float32 elements, the smallest shape at which a 256-CU device takes the rule's last clause (one workgroup per CU, up to
two: two parts) -- once per caller of the rule.  They cost 1.3 GB and 1.1 GB of device memory (coefficients, weights and inputs, filled
on the device by the library's counter generator, not uploaded) for the time of the replay; all 224 calls with their operators take about
two seconds on an MI355X.  The number of per-workgroup partial sums a step leaves (last_step_parts) has no name in jh_tune_get: the
step's ||u||^2, folded from them, is hashed instead.  tests/test_gpu_grid_launch_record.py replays the list against the library as
built and requires every counter and every hash to be equal, so the record is regenerated only when a launch rule or a kernel's
arithmetic changes ON PURPOSE -- with the library from BEFORE the change where the change claims to keep both.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import itertools
import json
import os
import random
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "grid_launch_record.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N = 515
DTYPES = ("float32", "float64", "complex64", "complex128")
RANGES = {"whole": None, "head": (0, 128), "rest": (128, 387), "last": (512, 3)}
SPLITS = (-1, 0, 3)
# the parameters of the three families of calls; MAJOR: every combination that exists is a case
MAJOR = ("call", "range", "nrow", "adj_split")
FAMILIES = {
    "grid": {"call": ("normal", "adjoint", "step"), "range": tuple(RANGES), "nrow": (5, 600), "adj_split": SPLITS, "dt": DTYPES,
             "ncol": (2, 3, 4), "mixed": (0, 1), "nt": (0, 2), "beta": (0.0, -0.625)},
    "grid_chain": {"call": ("adjoint", "normal", "forward", "step"), "range": tuple(RANGES), "nrow": (5, 600), "adj_split": SPLITS, "dt": DTYPES,
                   "ncol": (2, 3, 4), "mixed": (0, 1), "nt": (0, 2), "beta": (0.0, -0.625), "nw": (0, 1, 2), "post": (0, 1), "accumulate": (0, 1)},
    "tall_chain": {"call": ("adjoint", "normal", "forward", "step"), "range": tuple(RANGES), "nrow": (5, 600), "adj_split": SPLITS, "dt": DTYPES,
                   "nt": (0, 2), "beta": (0.0, -0.625), "nw": (0, 1, 2), "post": (0, 1), "accumulate": (0, 1)},
}


# 256 rows of 262 147 Float32 elements: 257 workgroups of 256 packs, on a device of 256 CUs one part by pick_adj_parts and two by the rule
BUMP = {"call": "normal", "range": "whole", "nrow": 256, "adj_split": -1, "dt": "float32", "nt": 0, "beta": 0.0, "n": 262147}
BUMP_MINOR = {"ncol": 2, "mixed": 0, "nw": 1, "post": 0, "accumulate": 0}


def _exists(family, c):
    """Does a case with these (some of the) parameters exist?  Each rule reads two parameters, so pairs can be asked too."""
    call, rng = c.get("call"), c.get("range")
    if family == "grid" and call == "adjoint" and rng == "whole":
        return False                                  # the whole-vector adjoint of a grid is the register-tiled general kernel
    if call == "forward" and rng not in (None, "whole"):
        return False                                  # FORWARD chains have no ranged form
    if call == "step" and c.get("accumulate", 0) != 0:
        return False
    if c.get("beta", 0.0) != 0.0 and (call not in (None, "step") or c.get("accumulate", 0) != 0):
        return False                                  # (beta is the step's: one value elsewhere)
    return True


def cases():
    """The covering list, the same on every run: greedy pairwise cover of the minor parameters over the product of the major ones."""
    rnd, out = random.Random(515), []
    for family, axes in FAMILIES.items():
        names = list(axes)
        need = {((a, v), (b, w)) for a, b in itertools.combinations(names, 2) for v in axes[a] for w in axes[b] if _exists(family, {a: v, b: w})}
        for major in itertools.product(*(axes[a] for a in MAJOR)):
            base = dict(zip(MAJOR, major))
            if not _exists(family, base):
                continue
            best, gain = None, -1
            for _ in range(40):
                c = dict(base, **{a: rnd.choice(axes[a]) for a in names if a not in MAJOR})
                if not _exists(family, c):
                    continue
                g = sum(1 for p in itertools.combinations(c.items(), 2) if p in need)
                if g > gain:
                    best, gain = c, g
            need -= set(itertools.combinations(best.items(), 2))
            out.append(dict({"family": family}, **best))
        assert not need, (family, sorted(need)[:5])
        # ... and the one clause of the part rule that blocks of 515 elements cannot reach: a workgroup per CU, up to two, takes TWO parts.  Once
        # per caller of the rule: grid_plan (the five grid launchers share it) and the tall chains' launcher
        if family != "grid_chain":
            out.append(dict({"family": family}, **dict(BUMP, **{a: v for a, v in BUMP_MINOR.items() if a in axes})))
    return out


def _host(rng, dt, n):
    a = rng.uniform(-1.0, 1.0, n)
    if np.dtype(dt).kind == "c":
        a = a + 1j * rng.uniform(-1.0, 1.0, n)
    return a.astype(dt)


def _pattern(dt, n):
    """What every output holds before the call: fixed, non-zero, no two neighbours alike."""
    a = (np.arange(n) % 7 + 1) * 0.125
    return (a - 1j * (a + 0.5)).astype(dt) if np.dtype(dt).kind == "c" else a.astype(dt)


def _digest(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()[:16]


class Rig:
    """One operator -- an N x K grid of blocks of several kinds or of plain diagonals, or (ncol None) a tall operator of diagonals --, two weights on
    its range, a diagonal on its domain, inputs on both sides, and the chain handles made on it."""

    def __init__(self, J, dt, nrow, ncol, mixed, n):
        self.J, self.dt, self.nrow, self.K, self.n = J, np.dtype(dt).type, nrow, ncol or 1, n
        rng, streams = np.random.default_rng([nrow, self.K, mixed, DTYPES.index(dt)]), itertools.count()
        # (the one large operator: the library's counter generator on the device, as reproducible as the host's)
        vec = lambda R: J.from_numpy(_host(rng, dt, R.length()), R) if n == N else J.rand(R, seed=515, stream=next(streams))
        blk = J.JetSpace(self.dt, n)
        self.coeff = vec(J.JetBSpace([blk] * (nrow * self.K)))
        names = ("diag", "diag_adj", "identity", "scale", "zero")
        rows = []
        for i in range(nrow):
            row = []
            for k in range(self.K):
                kind = names[(2 * i + 3 * k + i // 4) % 5] if mixed and i != 1 else ("zero" if mixed else "diag")   # (row 1: all zero blocks)
                if kind in ("diag", "diag_adj"):
                    d = J.JopDiagonal(self.coeff.arrays[i * self.K + k])
                    row.append(d.H if kind == "diag_adj" else d)
                elif kind == "scale":
                    row.append(J.JopLn(dom=blk, rng=blk, df=J.constdiag_df, df_adj=J.constdiag_df_adj, s={"a": 0.3 + (i % 5)}))
                else:
                    row.append(J.JopIdentity(blk) if kind == "identity" else J.JopZeroBlock(blk, blk))
            rows.append(row)
        self.A = J.blockop(rows)
        self.R, self.D = J.range(self.A), J.domain(self.A)
        self.w = [vec(self.R) for _ in range(2)]
        self.c = vec(self.D)
        self.x_rng, self.x_dom = vec(self.R), vec(self.D)
        self.handles, self.caches = {}, []

    def native(self):
        from jets_jl_amd import jetblock

        return jetblock._native_op(self.A.jet.s["_native"], self.A.jet.s["ops"], self.A.jet.rng.eltype())

    def handle(self, call, nw, post):
        """The chain handle of L = R o A o P (forward, step), adjoint(L) or adjoint(L) o L: R of nw weights (the second conjugated; none: a real
        scalar), P the domain diagonal when `post` (its adjoint is the stage after A')."""
        from jets_jl_amd import chains

        key = (call, nw, post)
        if key not in self.handles:
            J = self.J
            W = [J.JopDiagonal(self.w[0]), J.JopDiagonal(self.w[1]).H][:nw]
            if not nw:
                W = [J.JopLn(dom=self.R, rng=self.R, df=J.constdiag_df, df_adj=J.constdiag_df_adj, s={"a": 0.75})]
            L = J.compose(self.A, J.JopDiagonal(self.c)) if post else self.A
            for s in W:
                L = J.compose(s, L)
            op, ctype = {"forward": (L, chains.CHAIN_FORWARD), "step": (L, chains.CHAIN_FORWARD), "adjoint": (L.H, chains.CHAIN_ADJOINT),
                         "normal": (J.compose(L.H, L), chains.CHAIN_NORMAL)}[call]
            cache = chains.ChainCache()
            h = chains.one_run(chains.stages_of(op), cache, f"grid_launch_record_{len(self.caches)}", ctype)
            assert isinstance(h, chains.ChainHandle) and h.grid == (self.K > 1), f"{key}: not one fused run"
            self.caches.append(cache)
            self.handles[key] = h
        return self.handles[key]

    def close(self):
        for c in self.caches:
            c.close()
        self.J.close(self.A)


def _written(c):
    """The launch counters the call of case `c` writes."""
    ranged, fam, call = c["range"] != "whole", c["family"], c["call"]
    if fam == "grid":
        return ["last_adj_parts", "last_adj_launches"] + (["last_grid_range_shape"] if ranged else ["last_grid_step_shape"] if call == "step" else [])
    if fam == "tall_chain":
        return [] if call == "forward" else ["last_adj_parts"]
    if call == "forward":
        return ["last_grid_chain_shape"]
    return ["last_adj_parts", "last_grid_chain_range_shape" if ranged else "last_grid_chain_step_shape" if call == "step" else "last_grid_chain_shape"]


def run_case(J, rig, c):
    """One call of case `c` on its rig: ({counter: value}, [hash of every vector the call writes, of the step's ||u||^2 last])."""
    from jets_jl_amd._ffi import check, lib

    J.tune(adj_split=c["adj_split"], nt=c["nt"])
    r, call, alpha, beta, nrm = RANGES[c["range"]], c["call"], 1.25, c["beta"], C.c_double(-1.0)
    dom = J.from_numpy(_pattern(rig.dt, rig.K * rig.n), rig.D)
    rng = J.from_numpy(_pattern(rig.dt, rig.nrow * rig.n), rig.R) if call in ("step", "forward") else None
    if c["family"] == "grid":
        nat = rig.native().handle
        if call == "step":
            written = [rng, dom]
            check(lib.jh_blockop_bidiag_step(nat, rng.handle, rig.x_dom.handle, dom.handle, alpha, beta, C.byref(nrm)) if r is None else
                  lib.jh_blockop_bidiag_step_range(nat, rng.handle, rig.x_dom.handle, dom.handle, alpha, beta, r[0], r[1], C.byref(nrm)))
        elif call == "normal":
            written = [dom]
            check(lib.jh_blockop_normal_mul(nat, dom.handle, rig.x_dom.handle) if r is None else
                  lib.jh_blockop_normal_mul_range(nat, dom.handle, rig.x_dom.handle, r[0], r[1]))
        else:
            written = [dom]
            check(lib.jh_blockop_mul_adj_range(nat, dom.handle, rig.x_rng.handle, r[0], r[1]))
    else:
        h = rig.handle(call, c["nw"], c["post"])
        if call == "step":
            written = [rng, dom]
            if r is None:
                check(lib.jh_chain_bidiag_step(h.handle, rng.handle, rig.x_dom.handle, dom.handle, alpha, beta, C.byref(nrm)))
            else:
                nrm.value = h.bidiag_step_range(rng, rig.x_dom, dom, alpha, beta, r[0], r[1], read_normsq=True)
        elif call == "forward":
            written = [h.apply(rng, rig.x_dom, c["accumulate"])]
        else:
            x = rig.x_rng if call == "adjoint" else rig.x_dom
            written = [h.apply(dom, x, c["accumulate"]) if r is None else h.apply_range(dom, x, r[0], r[1], c["accumulate"])]
    counters = {name: J.tune_get(name) for name in _written(c)}
    hashes = [_digest(np.ascontiguousarray(v.to_numpy()).tobytes()) for v in written]
    if call == "step":
        hashes.append(_digest(struct.pack("<d", nrm.value)))
    return counters, hashes


def replay(J, todo):
    """Run the cases `todo` (dicts of parameters; rigs are shared and built on first use): [(counters, hashes)] in their order."""
    saved = {k: J.tune_get(k) for k in ("adj_split", "nt", "grid_range", "grid_chain_range", "grid_chain_step")}
    J.tune(grid_range=1, grid_chain_range=1, grid_chain_step=1)
    rigs, out = {}, []
    try:
        for c in todo:
            key = (c["dt"], c["nrow"], c.get("ncol"), c.get("mixed", 0), c.get("n", N))
            if key not in rigs:
                rigs[key] = Rig(J, *key)
            out.append(run_case(J, rigs[key], c))
    finally:
        for rig in rigs.values():
            rig.close()
        J.tune(**saved)
    return out


def dumps(cu_count, todo, results) -> str:
    rows = ",\n".join("  " + json.dumps(dict(c, counters=k, hashes=h)) for c, (k, h) in zip(todo, results))
    return f'{{"cu_count": {cu_count},\n "cases": [\n{rows}\n ]}}\n'


if __name__ == "__main__":
    if sys.argv[1:] not in ([], ["--stdout"]):
        raise SystemExit(__doc__)
    import jets_jl_amd as J

    J.init(0)
    todo = cases()
    text = dumps(J.device_info()["cu_count"], todo, replay(J, todo))
    if sys.argv[1:]:
        sys.stdout.write(text)
    else:
        with open(OUT, "w", encoding="utf-8") as f:
            f.write(text)
        print(f"{len(todo)} cases -> {OUT}")
