#!/usr/bin/env python3
"""IEEE special values (signed zeros, infinities, NaN, denormals, the largest finite values) through every kernel family, against the
CPU oracle, element by element -- bit for bit except for the payload of a NaN.  Prints one line per check; exit status 1 on a mismatch.

    python tools/check_specials.py [elements per block]            (one MI355X; default 4120, 6291456 for the big-block routes)

run_checks: the families of round 3 (tall forward / adjoint / fused A'A, mixed rows, the bare one-pass step, a grid, a sum, dense children,
lincomb, the compiled broadcast).  run_fused_checks: the fused families written since -- tall chains, the chain and grid Golub-Kahan steps,
fused A'A and chains of N x K grids, the per-block reductions, the split walk -- case by case (fused_cases; tests/test_gpu_specials_fused.py
runs the same cases).  Without an argument every small case runs; with a size, run_checks at that size and the one big-block pass.
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np



def specials(rng, dt, n, frac=0.3):
    rt = np.float32 if dt in (np.float32, np.complex64) else np.float64
    fi = np.finfo(rt)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.tiny / 4, -fi.tiny / 8, fi.max, -fi.max, fi.tiny, 1.0, -1.0, fi.eps], dtype=rt)

    def one():
        x = rng.standard_normal(n).astype(rt)
        k = rng.random(n) < frac
        x[k] = rng.choice(pool, size=int(k.sum()))
        return x

    if np.dtype(dt).kind != "c":
        return one()
    out = np.empty(n, dtype=dt)
    out.real, out.imag = one(), one()
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "c":
        rt = np.float32 if a.dtype == np.complex64 else np.float64
        a, b = a.view(rt), b.view(rt)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return f"NaN in different places ({int(na.sum())} vs {int(nb.sum())})"
    it = np.uint32 if a.dtype == np.float32 else np.uint64
    d = a.view(it)[~na] != b.view(it)[~nb]
    return True if not d.any() else f"{int(d.sum())} non-NaN elements differ"




def close_or_better(a, b, rtol):
    """For the one kernel family whose sum is NOT in the reference's order (the dense adjoint: fp64 lanes + wave reduction, tolerance parity):
    a NaN of the device must be a NaN of the oracle (accumulating in fp64 only removes overflow-made Inf - Inf), finite pairs agree to rtol."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "c":
        rt = np.float32 if a.dtype == np.complex64 else np.float64
        a, b = a.view(rt), b.view(rt)
    if (np.isnan(a) & ~np.isnan(b)).any():
        return f"{int((np.isnan(a) & ~np.isnan(b)).sum())} NaNs the oracle does not have"
    both = np.isfinite(a) & np.isfinite(b)
    err = np.abs(a[both].astype(np.float64) - b[both].astype(np.float64))
    scale = np.abs(b[both].astype(np.float64)) + np.finfo(a.dtype).tiny
    return True if (err <= rtol * scale + 1e-30).all() else f"finite values differ by up to {float((err / scale).max()):.1e}"


def run_checks(J, jo, seed=5, n=4096 + 24, dtypes=(np.float32, np.float64, np.complex64, np.complex128)):
    """[(dtype name, what, True | mismatch text)] for every check; J = the product package, jo = the oracle module."""
    from jets_jl_amd._ffi import lib, check

    rng = np.random.default_rng(seed)
    results = []

    def report(dt, what, r):
        results.append((np.dtype(dt).name, what, r))

    with np.errstate(all="ignore"):
        for dt in dtypes:
            nrow = 6
            z = lambda k=1: [np.zeros(n, dtype=dt) for _ in range(k)]
            coeffs = [specials(rng, dt, n) for _ in range(nrow)]
            hm, hd = specials(rng, dt, n), [specials(rng, dt, n) for _ in range(nrow)]
            A = J.blockop([[J.JopDiagonal(J.from_numpy(c))] for c in coeffs])
            ops = [[jo.Block("diag", n, coeff=c)] for c in coeffs]
            m = J.from_numpy(hm)
            ref_d = jo.block_df(ops, z(nrow), [hm])
            report(dt, "tall forward", same((A * m).to_numpy(), np.concatenate(ref_d)))
            dd = J.from_numpy(np.concatenate(hd), J.range(A))
            report(dt, "tall adjoint", same((A.H * dd).to_numpy(), jo.block_df_adj(ops, z(), hd)[0]))
            report(dt, "fused A'A", same(((A.H @ A) * m).to_numpy(), jo.block_df_adj(ops, z(), ref_d)[0]))
            # rows of every elementwise kind, some adjointed
            spc = J.JetSpace(dt, n)
            sc = complex(specials(rng, dt, 1, 0.0)[0])
            sc = sc if np.dtype(dt).kind == "c" else sc.real
            kinds = [J.JopDiagonal(J.from_numpy(coeffs[0])), J.JopIdentity(spc), J.JopZeroBlock(spc, spc), J.JopDiagonal(J.from_numpy(coeffs[1])).H,
                     J.JopLn(dom=spc, rng=spc, df=J.constdiag_df, df_adj=J.constdiag_df_adj, s={"a": sc}), J.JopDiagonal(J.from_numpy(coeffs[2]))]
            okinds = [jo.Block("diag", n, coeff=coeffs[0]), jo.Block("identity", n), jo.Block("zero", n, n), jo.Block("diag", n, coeff=coeffs[1], adjoint=True),
                      jo.Block("scale", n, scale=sc), jo.Block("diag", n, coeff=coeffs[2])]
            B = J.blockop([[k] for k in kinds])
            bops = [[k] for k in okinds]
            report(dt, "mixed rows forward", same((B * m).to_numpy(), np.concatenate(jo.block_df(bops, z(nrow), [hm]))))
            report(dt, "mixed rows adjoint", same((B.H * dd).to_numpy(), jo.block_df_adj(bops, z(), hd)[0]))
            # the one-pass step and the two fused halves
            for name, op, oo in (("all-diagonal", A, ops), ("mixed rows", B, bops)):
                from jets_jl_amd import jetblock
                h = jetblock._native_op(op.jet.s["_native"], op.jet.s["ops"], op.jet.rng.eltype()).handle
                for beta in (0.0, -0.5):
                    u = J.from_numpy(np.concatenate(hd), J.range(op))
                    w = J.zeros(J.domain(op))
                    out = C.c_double(0)
                    check(lib.jh_blockop_bidiag_step(h, u.handle, m.handle, w.handle, 0.75, beta, C.byref(out)))
                    tmp = jo.block_df(oo, z(nrow), [hm])
                    ref_u = jo.barr_lincomb([np.empty(n, dtype=dt) for _ in range(nrow)], [0.75, beta] if beta else [0.75], [tmp, hd] if beta else [tmp])
                    report(dt, f"step u ({name}, beta {beta})", same(u.to_numpy(), np.concatenate(ref_u)))
                    report(dt, f"step w ({name}, beta {beta})", same(w.to_numpy(), jo.block_df_adj(oo, z(), ref_u)[0]))
            # grid with a zero block
            g = [[specials(rng, dt, n) for _ in range(3)] for _ in range(3)]
            G = J.blockop([[J.JopZeroBlock(spc, spc) if (i, j) == (1, 1) else J.JopDiagonal(J.from_numpy(g[i][j])) for j in range(3)] for i in range(3)])
            gops = [[jo.Block("zero", n, n) if (i, j) == (1, 1) else jo.Block("diag", n, coeff=g[i][j]) for j in range(3)] for i in range(3)]
            hx = [specials(rng, dt, n) for _ in range(3)]
            x = J.from_numpy(np.concatenate(hx), J.domain(G))
            report(dt, "grid forward", same((G * x).to_numpy(), np.concatenate(jo.block_df(gops, z(3), hx))))
            report(dt, "grid adjoint", same((G.H * x).to_numpy(), np.concatenate(jo.block_df_adj(gops, z(3), hx))))
            # sum of three tall operators, + - +
            A2 = J.blockop([[J.JopDiagonal(J.from_numpy(c))] for c in coeffs[::-1]])
            A3 = J.blockop([[J.JopDiagonal(J.from_numpy(c))] for c in coeffs[1:] + coeffs[:1]])
            ops2, ops3 = [[jo.Block("diag", n, coeff=c)] for c in coeffs[::-1]], [[jo.Block("diag", n, coeff=c)] for c in coeffs[1:] + coeffs[:1]]
            S = A - A2 + A3
            r1, r2, r3 = jo.block_df(ops, z(nrow), [hm]), jo.block_df(ops2, z(nrow), [hm]), jo.block_df(ops3, z(nrow), [hm])
            ref = [(a - b) + c for a, b, c in zip(r1, r2, r3)]
            ref = [(np.zeros(n, dtype=dt) + a) for a in ref]
            report(dt, "sum forward (+ - +)", same((S * m).to_numpy(), np.concatenate([((np.zeros(n, dtype=dt) + a) - b) + c for a, b, c in zip(r1, r2, r3)])))
            # dense children
            nd = 96
            Md = specials(rng, dt, nd * nd, 0.1).reshape(nd, nd, order="F")
            hv = specials(rng, dt, nd, 0.1)
            D = J.blockop([[J.JopDense(J.from_numpy(np.asfortranarray(Md)))], [J.JopDense(J.from_numpy(np.asfortranarray(Md)))]]) if hasattr(J, "JopDense") else None
            if D is not None:
                dops = [[jo.Block("dense", nd, nd, coeff=np.asfortranarray(Md))], [jo.Block("dense", nd, nd, coeff=np.asfortranarray(Md))]]
                report(dt, "dense forward", same((D * J.from_numpy(hv)).to_numpy(), np.concatenate(jo.block_df(dops, [np.zeros(nd, dtype=dt) for _ in range(2)], [hv]))))
                h2 = [specials(rng, dt, nd, 0.1) for _ in range(2)]
                report(dt, "dense adjoint", close_or_better((D.H * J.from_numpy(np.concatenate(h2), J.range(D))).to_numpy(), jo.block_df_adj(dops, [np.zeros(nd, dtype=dt)], h2)[0],
                                                            1e-4 if dt in (np.float32, np.complex64) else 1e-11))
            # broadcast: a*x + b*y over block arrays
            R = J.range(A)
            X, Y = J.from_numpy(np.concatenate(hd), R), J.from_numpy(np.concatenate(ref_d), R)
            outv = J.zeros(R)
            J.lincomb_(outv, [0.75, -1.25], [X, Y])
            report(dt, "lincomb", same(outv.to_numpy(), np.concatenate(jo.barr_lincomb([np.empty(n, dtype=dt) for _ in range(nrow)], [0.75, -1.25], [hd, ref_d]))))
            J.broadcast_(outv, "s0*x0 + s1*x1", [X, Y], [0.75, -1.25])            # the compiled form of the same expression: real scalars stay real
            report(dt, "compiled broadcast, real scalars", same(outv.to_numpy(), np.concatenate(jo.barr_lincomb([np.empty(n, dtype=dt) for _ in range(nrow)], [0.75, -1.25], [hd, ref_d]))))
            if np.dtype(dt).kind == "c":
                cs = [0.75 + 0.5j, -1.25 - 2j]
                J.lincomb_(outv, cs, [X, Y])
                ref = np.concatenate(jo.barr_lincomb([np.empty(n, dtype=dt) for _ in range(nrow)], cs, [hd, ref_d]))
                report(dt, "lincomb, complex scalars", same(outv.to_numpy(), ref))
                J.broadcast_(outv, "s0*x0 + s1*x1", [X, Y], cs)
                report(dt, "compiled broadcast, complex scalars", same(outv.to_numpy(), ref))
    return results



# =====================================================================================================================================
# The fused families written after round 3: tall chains (jh_chain_apply / jh_chain_apply_range), the chain Golub-Kahan step, fused A'A of
# N x K grids, grid chains, the grid step, the per-block reductions and the split walk.  Two kinds of input: (a) the mix of specials()
# everywhere -- coefficients, weights, domain diagonals and vectors --, (b) "seam poison": finite U[0,1) data with NaN, +Inf and -0 at the
# scalars where lanes overlap or idle (seam_positions).  Every operator is elementwise, so the oracle's stage-by-stage loops say which
# outputs may be non-finite.  A check is a record ("same", what, got, want) -- bit for bit except a NaN's payload -- or
# ("verdict", what, True | text); fused_cases() lists (id, dtype, function) and run_fused_checks() runs them.
POISON = (np.nan, np.inf, -0.0)
SEAM_CLASSES = ("head", "overlap", "tile", "row-ends", "range-edge")
INF_ONLY = ", +Inf only"
STEP_CLASSES = ("head" + INF_ONLY, "overlap" + INF_ONLY)       # for the steps' ||u||^2


def _rt(dt):
    return np.float32 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64


def scalars_per_pack(dt):
    """NS of the kernels: real scalars in one 16-byte pack (a complex element is two scalars)."""
    return 16 // np.dtype(_rt(dt)).itemsize


def scalars_per_elem(dt):
    return 2 if np.dtype(dt).kind == "c" else 1


def seam_positions(cls, n, NS, tile=None, ranges=()):
    """The scalar indices of one row of n scalars that a position class names (sorted):
    head        0 .. NS-1: the pack every idle lane loads (pack_start(ok ? s0 : 0, n))
    overlap     the last NS scalars before g = n - n % NS and the partial tail [g, n): the pack loaded from n - NS overlaps its neighbour
    tile        the first and last scalar of every workgroup tile of `tile` scalars
    row-ends    scalar 0 and scalar n - 1: in a slab of rows, the pack that straddles two rows
    range-edge  the NS scalars just below and just above every [lo, lo + count) of `ranges` (scalars)"""
    if cls == "head":
        p = set(range(0, min(NS, n)))
    elif cls == "overlap":
        g = n - n % NS
        p = set(range(max(g - NS, 0), n))
    elif cls == "tile":
        p = set()
        for t0 in range(0, n, tile):
            p |= {t0, min(t0 + tile, n) - 1}
    elif cls == "row-ends":
        p = {0, n - 1}
    elif cls == "range-edge":
        p = set()
        for lo, cnt in ranges:
            p |= set(range(max(lo - NS, 0), lo)) | set(range(lo + cnt, min(lo + cnt + NS, n)))
    else:
        raise ValueError(cls)
    return sorted(p)


def slab_seam_positions(lens, which):
    """Scalar indices in a slab of blocks of `lens` scalars: "block-last" the last scalar of every even block that has a successor,
    "block-first" the first scalar of every odd block (empty blocks own nothing)."""
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if which == "block-last":
        return [int(offs[i + 1] - 1) for i in range(0, len(lens) - 1, 2) if lens[i] > 0]
    if which == "block-first":
        return [int(offs[i]) for i in range(1, len(lens), 2) if lens[i] > 0]
    raise ValueError(which)


def part_edge_rows(nrow, parts):
    """First and last row of every part of the split walk: rows_per_part = ceil(nrow / parts), part y walks [y, y + 1) * rows_per_part."""
    rpp = -(-nrow // parts)
    rows = set()
    for lo in range(0, nrow, rpp):
        rows |= {lo, min(lo + rpp, nrow) - 1}
    return sorted(rows)


def poison(x, positions, rot=0, row_scalars=None, rows=None, values=POISON):
    """NaN, +Inf, -0 in turn at the scalar `positions` of x (in place; complex x: real and imaginary parts are scalars).  row_scalars: x is
    a slab of rows of that many scalars, every row (or the listed `rows`) gets the positions."""
    v = x.view(_rt(x.dtype))
    vals = np.array(values, dtype=v.dtype)
    if row_scalars is None:
        row_scalars, rws = v.size, [0]
    else:
        rws = range(v.size // row_scalars) if rows is None else [r for r in rows if r < v.size // row_scalars]
    for r in rws:
        for k, q in enumerate(positions):
            v[r * row_scalars + q] = vals[(k + rot + r) % len(vals)]
    return x


def specials_order_free(rng, dt, n, frac=0.3):
    """The split walk's pool: +-0, +-Inf, NaN, denormals, +-1 on U[0,1) data -- no +-max, so no overflow that depends on the row order."""
    rt = _rt(dt)
    fi = np.finfo(rt)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.tiny / 4, -fi.tiny / 8, 1.0, -1.0], dtype=rt)

    def one():
        x = rng.random(n).astype(rt)
        k = rng.random(n) < frac
        x[k] = rng.choice(pool, size=int(k.sum()))
        return x

    if np.dtype(dt).kind != "c":
        return one()
    out = np.empty(n, dtype=dt)
    out.real, out.imag = one(), one()
    return out


class Source:
    """Host arrays for one case, by tag (a tuple of a letter and integers): "mix" specials(), "order-free" specials_order_free(), or finite
    U[0,1) data poisoned at `positions` of every row of `row_scalars` scalars (rows: only those rows of a slab)."""

    def __init__(self, dt, cls, seed, positions=(), row_scalars=None, rows=None, frac=0.3, values=POISON, only=None):
        self.dt, self.cls, self.seed, self.positions, self.row_scalars, self.rows, self.frac = dt, cls, seed, list(positions), row_scalars, rows, frac
        self.values, self.only = values, only                                 # only: the tag letters that are poisoned (None: every array)

    def __call__(self, tag, n):
        key = [ord(tag[0])] + [int(t) for t in tag[1:]]
        rng = np.random.default_rng([self.seed] + key)
        with np.errstate(all="ignore"):
            if self.cls == "mix":
                return specials(rng, self.dt, n, self.frac)
            if self.cls == "order-free":
                return specials_order_free(rng, self.dt, n, self.frac)
            rt = _rt(self.dt)
            if np.dtype(self.dt).kind == "c":
                x = np.empty(n, dtype=self.dt)
                x.real, x.imag = rng.random(n).astype(rt), rng.random(n).astype(rt)
            else:
                x = rng.random(n).astype(rt)
            single = tag[0] == "A" or self.row_scalars is None or n * scalars_per_elem(self.dt) <= self.row_scalars
            if self.only is not None and tag[0] not in self.only:
                return x
            if self.rows is not None and tag[0] == "A":                       # a coefficient block IS one row of the operator
                if tag[1] not in self.rows:
                    return x
            return poison(x, self.positions, rot=sum(key) % 3, row_scalars=None if single else self.row_scalars, rows=None if single else self.rows,
                          values=self.values)


def expect_normsq(u):
    """||u||^2 from the oracle's u: NaN if a scalar is NaN, else Inf if one is Inf, else the fp64 sum of the squares."""
    a = np.ascontiguousarray(u).view(_rt(u.dtype)).astype(np.float64)
    if np.isnan(a).any():
        return float("nan")
    if np.isinf(a).any():
        return float("inf")
    with np.errstate(all="ignore"):
        return float(np.sum(a * a))


def inf_only_verdict(dt, cls, beta, u):
    """A +Inf-only case must stay one: the oracle's new u holds Inf and no NaN (complex types: where the old u is read).  None: not such a case."""
    if not cls.endswith(INF_ONLY) or (scalars_per_elem(dt) == 2 and beta == 0):
        return None
    return True if expect_normsq(u) == np.inf else "DEGRADED CASE: the oracle's u should hold +-Inf and no NaN"


def normsq_verdict(got, u, rtol=1e-12):
    want = expect_normsq(u)
    if np.isnan(want):
        return True if np.isnan(got) else f"||u||^2 = {got}, the oracle's u holds a NaN"
    if np.isinf(want):
        return True if got == np.inf else f"||u||^2 = {got}, expected Inf"
    return True if np.isfinite(got) and abs(got - want) <= rtol * want else f"||u||^2 = {got} vs {want}"


def masks_verdict(got, want, finite_ok):
    """The split walk (another sum order): NaN where the oracle has NaN, the same infinities with the same signs, finite scalars through
    finite_ok(got, want) -> True | text (both with the non-finite scalars set to zero)."""
    g, w = np.ascontiguousarray(got).view(_rt(got.dtype)), np.ascontiguousarray(want).view(_rt(want.dtype))
    if not np.array_equal(np.isnan(g), np.isnan(w)):
        return f"NaN in different places ({int(np.isnan(g).sum())} vs {int(np.isnan(w).sum())})"
    if not np.array_equal(np.isinf(g), np.isinf(w)) or not np.array_equal(np.sign(g[np.isinf(g)]), np.sign(w[np.isinf(w)])):
        return "infinities in different places or of different signs"
    fin = np.isfinite(w)
    return finite_ok(np.where(fin, g, 0).view(got.dtype), np.where(fin, w, 0).view(want.dtype))


def order_free_verdict(fwd, rev):
    """The split walk's condition on the CASE: the oracle with the rows in forward and in reversed order has the same NaN and Inf masks."""
    a, b = np.ascontiguousarray(fwd).view(_rt(fwd.dtype)), np.ascontiguousarray(rev).view(_rt(rev.dtype))
    ok = np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
    return True if ok else "TEST BUG: the oracle's NaN / Inf masks depend on the row order"


LENS = {"mix": (4096 + 24, 1027, 67), "head": (1027, 67), "overlap": (1027, 67, 3 * 4096 + 17), "tile": (3 * 4096 + 17, 4096 + 24),
        "row-ends": (1027, 67), "range-edge": (1027, 3 * 4096 + 17)}
TALL_SHAPES = [(wg, un, nt) for wg, un in ((256, 1), (512, 2), (512, 4)) for nt in (0, 2)]
STEP_KNOBS = [dict(adj_wg=256), dict(adj_wg=512), dict(adj_wg=512, adj_unroll=4), dict(nt=0), dict(nt=2), dict(ua_nt=1)]


def tile_sizes(dt):
    """Workgroup tiles of the forced shapes in scalars: 256 NS, 512 NS U for U = 2, 4."""
    ns = scalars_per_pack(dt)
    return (256 * ns, 512 * ns * 2, 512 * ns * 4)


def case_ranges(n, dt):
    """Two element ranges of a domain of n elements for jh_chain_apply_range: starts on the 16-byte grid (the entry point requires it) but on
    no workgroup tile, the first range inside the vector, the second ends with the vector (inside a pack when n is off the grid)."""
    al = max(1, scalars_per_pack(dt) // scalars_per_elem(dt))
    mid = al * ((n // 2) // al + 1)
    return [(3 * al, mid - 3 * al), (mid, n - mid)]


def row_positions(cls, n, dt):
    """seam_positions of one row of n ELEMENTS for the tall / grid kernels (the tile class: the union over the forced shapes' tiles)."""
    ns, e = scalars_per_pack(dt), scalars_per_elem(dt)
    if cls == "tile":
        return sorted(set().union(*[seam_positions("tile", n * e, ns, tile=t) for t in tile_sizes(dt)]))
    return seam_positions(cls, n * e, ns, ranges=[(lo * e, c * e) for lo, c in case_ranges(n, dt)])


def source_for(dt, cls, n, seed):
    if cls in ("mix", "order-free"):
        return Source(dt, cls, seed)
    if cls.endswith(INF_ONLY):
        # +Inf alone, in real parts alone, in ONE array: no NaN is made, so the new u holds Inf and no NaN and ||u||^2 must be Inf -- a scalar
        # masked out of the sum by a multiplication (0 * Inf) would make it NaN, which the three-valued poison cannot show.  Real types: the
        # operator's coefficients.  Complex types: the old u (a second complex product of Inf + i Inf is NaN, src/Jets.jl's four-multiplication
        # formula; beta * u is part by part), so there the class bites at beta != 0.  The step cases assert that the expected ||u||^2 IS Inf.
        e = scalars_per_elem(dt)
        pos = [q for q in row_positions(cls[:-len(INF_ONLY)], n, dt) if q % e == 0]
        return Source(dt, cls, seed, positions=pos, row_scalars=n * e, values=(np.inf,), only=("A",) if e == 1 else ("u",))
    return Source(dt, cls, seed, positions=row_positions(cls, n, dt), row_scalars=n * scalars_per_elem(dt))


ROW_CONFIGS = (("9 diag rows", 9, "diag"), ("8 mixed rows", 8, "mixed"), ("4 plain + 5 mixed rows", 9, "plain-first"))


def _row_kinds(nrow, name):
    from tests.test_gpu_chains import _kinds

    if name == "plain-first":                                                 # a whole DEPTH batch of plain diagonals, then rows of every kind
        return [["diag"]] * 4 + _kinds(nrow, "mixed")[1:nrow - 3]
    return _kinds(nrow, name)


def accumulated(acc, base, t):
    """What jh_chain_apply leaves: JetSum's broadcast (src/Jets.jl:634, 640) -- +-1 continue from the output, +-2 start from zeros."""
    with np.errstate(all="ignore"):
        return {0: t, 1: base + t, -1: base - t, 2: np.zeros_like(base) + t, -2: np.zeros_like(base) - t}[acc]


TALL_CHAINS = {
    # name: (tokens in application order (tests/test_gpu_chains.py: Rig), chain type)
    "A' o W o A": (["A", ("W", 0, False), "At"], "normal"),
    "(W o A)'": ([("W", 0, True), "At"], "adj"),
    "W o A": (["A", ("W", 0, False)], "fwd"),
    "M' o A' o W o A o M": ([("M", 0, False), "A", ("W", 0, False), "At", ("M", 0, True)], "normal"),
    "A' o (a W) o A": (["A", ("W", 1, False), ("s", -1.25, "r"), "At"], "normal"),
    "a * (W o A)'": ([("W", 0, True), "At", ("s", 0.375, "d")], "adj"),
    "0.75 * (W o A)": (["A", ("W", 0, False), ("s", 0.75, "r")], "fwd"),
    "A' o (2.5 W)' o A, Float64 scalar": (["A", ("s", np.float64(2.5), "r"), ("W", 0, True), "At"], "normal"),
    "3.14 * (A' o W o A), Float64 scalar": (["A", ("W", 0, False), "At", ("s", np.float64(3.14), "d")], "normal"),
    "Wb o A": (["A", ("Wb", 0, False)], "fwd"),
    "Wb' o A": (["A", ("Wb", 1, True)], "fwd"),
    "A' o Wb o A": (["A", ("Wb", 0, False), "At"], "normal"),
    "A o M": ([("M", 0, False), "A"], "fwd"),
    "M o A'": (["At", ("M", 0, False)], "adj"),
}


def adjoint_tokens(toks):
    out = []
    for t in reversed(toks):
        out.append("At" if t == "A" else "A" if t == "At" else t if t[0] in ("s", "I") else (t[0], t[1], not t[2]))
    return out


def _flat(x):
    return x.to_numpy().ravel(order="F")


def tall_chain_case(J, jo, dt, chain, cls, lens=None, shapes=TALL_SHAPES, row_configs=ROW_CONFIGS):
    """jh_chain_apply with accumulate 0 / +-1 / +-2 into an output that holds specials, and jh_chain_apply_range on two ranges, in every forced
    launch shape of k_chain_adj, against the oracle's stage-by-stage chain."""
    from jets_jl_amd import chains
    from tests.test_gpu_chains import Rig

    toks, kind = TALL_CHAINS[chain]
    ctype = {"fwd": chains.CHAIN_FORWARD, "adj": chains.CHAIN_ADJOINT, "normal": chains.CHAIN_NORMAL}[kind]
    for n in lens or LENS[cls.split(",")[0]]:
        for rname, nrow, rkind in row_configs:
            src = source_for(dt, cls, n, 11)
            rig = Rig(J, jo, dt, nrow, n, seed=31, data=src, kinds=_row_kinds(nrow, rkind))
            cache = chains.ChainCache()
            h = chains.one_run(chains.stages_of(rig.compose(toks)), cache, "t", ctype)
            if h is None:
                cache.close()
                rig.close()
                yield ("verdict", f"{chain}, {rname} of {n}: one fused run", "the planner did not fuse the chain")
                continue
            nin, nout = (nrow if kind == "adj" else 1), (nrow if kind == "fwd" else 1)
            hx = [src(("x", i), n) for i in range(nin)]
            x = J.from_numpy(np.concatenate(hx), J.range(rig.A) if kind == "adj" else J.domain(rig.A))
            ospc = J.range(rig.A) if kind == "fwd" else J.domain(rig.A)
            base = src(("o", 0), nout * n)
            with np.errstate(all="ignore"):
                t = np.concatenate(rig.ora_apply(toks, hx))
            for wg, un, nt in shapes:
                J.tune(adj_wg=wg, adj_unroll=un, nt=nt, adj_split=0)
                try:
                    tag = f"{chain}, {rname} of {n}, shape {wg} x {un}, nt {nt}"
                    for acc in (0, 1, -1, 2, -2):
                        out = h.apply(J.from_numpy(base, ospc), x, acc)
                        yield ("same", f"{tag}, accumulate {acc}", _flat(out), accumulated(acc, base, t))
                    if kind != "fwd":
                        for acc in (0, -1):
                            out = J.from_numpy(base, ospc)
                            want = base.copy()
                            for lo, cnt in case_ranges(n, dt):
                                h.apply_range(out, x, lo, cnt, acc)
                                want[lo:lo + cnt] = accumulated(acc, base, t)[lo:lo + cnt]
                            parts = J.tune_get("last_adj_parts")
                            yield ("verdict", f"{tag}: the ordered walk", True if parts == 1 else f"{parts} parts with adj_split = 0")
                            yield ("same", f"{tag}, two ranges, accumulate {acc}", _flat(out), want)
                finally:
                    J.tune(adj_wg=0, adj_unroll=0, nt=1, adj_split=-1)
            cache.close()
            rig.close()


def tall_composite_case(J, jo, dt, chain, cls):
    """Every chain of tests/test_gpu_chains.py: CHAINS through mul!(d, composite, m) into a dirty output, as the planner fuses it."""
    from jets_jl_amd import chains
    from tests.test_gpu_chains import CHAINS, Rig

    toks, runs = CHAINS[chain]
    for n in LENS[cls.split(",")[0]]:
        for rname, nrow, rkind in ROW_CONFIGS[:2]:
            src = source_for(dt, cls, n, 13)
            rig = Rig(J, jo, dt, nrow, n, seed=31, data=src, kinds=_row_kinds(nrow, rkind))
            C_ = rig.compose(toks)
            rng_in = toks[0] == "At" or (toks[0] != "A" and toks[0][0] in ("W", "Wb"))
            hx = [src(("x", i), n) for i in range(nrow if rng_in else 1)]
            x = J.from_numpy(np.concatenate(hx), J.range(rig.A) if rng_in else J.domain(rig.A))
            J.tune(adj_split=0)
            try:
                before = chains.STATS["chain_calls"]
                y = J.mul_(J.from_numpy(src(("o", 0), J.range(C_).length()), J.range(C_)), C_, x)
                ran = chains.STATS["chain_calls"] - before
            finally:
                J.tune(adj_split=-1)
            yield ("verdict", f"{chain}, {rname} of {n}: fused runs", True if ran == runs else f"{ran} fused runs, expected {runs}")
            with np.errstate(all="ignore"):
                want = np.concatenate(rig.ora_apply(toks, hx))
            yield ("same", f"{chain}, {rname} of {n}: the composite vs the oracle's stages", _flat(y), want)
            rig.close()


def chain_step_case(J, jo, dt, chain, cls, lens=None, knobs=STEP_KNOBS, row_configs=ROW_CONFIGS):
    """jh_chain_bidiag_step: u <- alpha L v + beta u, w <- L'u, ||u||^2.  beta == 0: the old u is ALL NaN and must not be read; w is dirty."""
    from jets_jl_amd import chains
    from tests.test_gpu_chain_step import STEP_CHAINS
    from tests.test_gpu_chains import Rig

    toks = STEP_CHAINS[chain]
    alpha = 1.375
    for n in lens or LENS[cls.split(",")[0]]:
        for rname, nrow, rkind in row_configs:
            src = source_for(dt, cls, n, 17)
            rig = Rig(J, jo, dt, nrow, n, seed=31, data=src, kinds=_row_kinds(nrow, rkind))
            L = rig.compose(toks)
            sc = chains.SolverChains(L)
            if sc.fwd is None:
                sc.close()
                rig.close()
                yield ("verdict", f"step of {chain}: one FORWARD run", "the planner did not fuse the chain")
                continue
            hv = src(("v", 0), n)
            v = J.from_numpy(hv, J.domain(L))
            for beta in (0.0, -0.625):
                hu0 = src(("u", 0), nrow * n) if beta else np.full(nrow * n, np.nan, dtype=dt)
                with np.errstate(all="ignore"):
                    tmp = rig.ora_apply(toks, [hv])
                    empty = [np.empty(n, dtype=dt) for _ in range(nrow)]
                    uref = jo.barr_lincomb(empty, [alpha, beta] if beta else [alpha], [tmp, np.split(hu0, nrow)] if beta else [tmp])
                    wref = rig.ora_apply(adjoint_tokens(toks), uref)[0]
                keeps = inf_only_verdict(dt, cls, beta, np.concatenate(uref))
                if keeps is not None:
                    yield ("verdict", f"step of {chain}, {rname} of {n}, beta {beta}: ||u||^2 is expected to be Inf", keeps)
                for kn in knobs:
                    saved = {k: J.tune_get(k) for k in list(kn) + ["adj_unroll", "adj_split"]}
                    J.tune(adj_split=0, **kn)
                    try:
                        u, w = J.from_numpy(hu0, J.range(L)), J.from_numpy(src(("o", 1), n), J.domain(L))
                        nsq = sc.step(u, v, w, alpha, beta)
                    finally:
                        J.tune(**saved)
                    tag = f"step of {chain}, {rname} of {n}, beta {beta}, {kn}"
                    if nsq is None:
                        yield ("verdict", tag, "the library declined the step")
                        continue
                    yield ("same", f"{tag}: u", _flat(u), np.concatenate(uref))
                    yield ("same", f"{tag}: w", _flat(w), wref)
                    yield ("verdict", f"{tag}: ||u||^2", normsq_verdict(nsq, np.concatenate(uref)))
            sc.close()
            rig.close()


def _native(A):
    from jets_jl_amd import jetblock as _blk

    return _blk._native_op(A.jet.s["_native"], A.jet.s["ops"], A.jet.rng.eltype())


def _grid_ops(J, jo, dt, variant, nrow, ncol, n, src, seed=43):
    """plain: all diagonals; mixed: the several-kinds grid of tests/test_gpu_grid_step.py; regularised: [A; lam I]."""
    from tests.test_gpu_blockop import _mixed_ops

    if variant == "plain":
        kinds = [["diag"] * ncol for _ in range(nrow)]
    elif variant == "mixed":
        names = ["diag", "zero", "identity", "scale", "diag_adj", "diag"]
        kinds = [[("diag" if i < max(1, nrow - ncol - 2) and (i % 5 != 3) else names[(2 * i + 3 * k) % 6]) for k in range(ncol)] for i in range(nrow)]
        kinds[nrow - 1] = ["zero"] * ncol
    else:
        kinds = [["diag"] * ncol for _ in range(nrow)] + [["scale" if k == r else "zero" for k in range(ncol)] for r in range(ncol)]
    A, ora = _mixed_ops(J, jo, dt, kinds, [n] * len(kinds), [n] * ncol, seed=seed, coeff=lambda i, j, nr: src(("A", i, j), nr))
    return A, ora, len(kinds)


def grid_normal_case(J, jo, dt, variant, cls):
    """jh_blockop_normal_mul on N x K grids (k_grid_normal; [A; lam I]: k_grid_normal_mixed) against the oracle's two loops."""
    from jets_jl_amd._ffi import lib

    for n in LENS[cls.split(",")[0]]:
        for ncol in (2, 3, 4):
            src = source_for(dt, cls, n, 19)
            A, ora, rows = _grid_ops(J, jo, dt, variant, 7, ncol, n, src)
            hm = [src(("x", j), n) for j in range(ncol)]
            m = J.from_numpy(np.concatenate(hm), J.domain(A))
            with np.errstate(all="ignore"):
                t = jo.block_df(ora, [np.zeros(n, dt) for _ in range(rows)], hm)
                want = np.concatenate(jo.block_df_adj(ora, [np.zeros(n, dt) for _ in range(ncol)], t))
            nat = _native(A)
            for nt in (0, 2):
                J.tune(nt=nt, adj_split=0)
                try:
                    y = J.from_numpy(src(("o", 0), ncol * n), J.domain(A))
                    st = lib.jh_blockop_normal_mul(nat.handle, y.handle, m.handle)
                finally:
                    J.tune(nt=1, adj_split=-1)
                tag = f"A'A of a {variant} {rows} x {ncol} grid of {n}, nt {nt}"
                if st != 0:
                    yield ("verdict", tag, f"jh_blockop_normal_mul returned {st}")
                    continue
                yield ("same", tag, _flat(y), want)
            J.close(A)


GRID_CHAINS = ("A' o W o A", "(W o A)'", "W o A", "M' o A' o W o A o M", "Wb o A", "2.5 (A' o W o A)")


def grid_chain_case(J, jo, dt, chain, variant, cls):
    """k_grid_chain MODE 0 / 1 / 2, the plain-row fast path (plain grids) and the per-kind path (mixed grids)."""
    from jets_jl_amd import chains
    from tests.test_gpu_grid_chains import CHAINS, GridRig

    toks = CHAINS[chain]
    for n in LENS[cls.split(",")[0]]:
        for ncol in (2, 3, 4):
            src = source_for(dt, cls, n, 23)
            nrow = 11 if variant == "mixed" else 9
            rig = GridRig(J, jo, dt, nrow, ncol, n, mixed=variant == "mixed", data=src)
            C_ = rig.compose(toks)
            rng_in = toks[0] == "At" or toks[0][0] == "W"
            hx = [src(("x", i), n) for i in range(nrow if rng_in else ncol)]
            x = J.from_numpy(np.concatenate(hx), J.range(rig.A) if rng_in else J.domain(rig.A))
            with np.errstate(all="ignore"):
                want = np.concatenate(rig.ora_apply(toks, hx))
            for nt in (0, 2):
                J.tune(nt=nt, adj_split=0)
                try:
                    g0 = chains.STATS["grid_chain_calls"]
                    y = J.mul_(J.from_numpy(src(("o", 0), J.range(C_).length()), J.range(C_)), C_, x)
                    ran, shape = chains.STATS["grid_chain_calls"] - g0, J.tune_get("last_grid_chain_shape")
                finally:
                    J.tune(nt=1, adj_split=-1)
                tag = f"{chain} through a {variant} {nrow} x {ncol} grid of {n}, nt {nt}"
                ok = ran == 1 and (shape & 1) == (1 if nt == 2 else 0) and not (shape & 2)
                yield ("verdict", f"{tag}: one grid chain, its shape", True if ok else f"{ran} grid chains, shape {shape}")
                yield ("same", tag, _flat(y), want)
            rig.close()


def grid_step_case(J, jo, dt, variant, cls):
    """The grid Golub-Kahan step behind jh_blockop_bidiag_step: plain, several kinds, [A; lam I]; beta == 0 with an all-NaN old u."""
    import ctypes as C

    from jets_jl_amd._ffi import lib

    alpha = 1.25
    for n in LENS[cls.split(",")[0]]:
        for ncol in (2, 3, 4):
            src = source_for(dt, cls, n, 29)
            A, ora, rows = _grid_ops(J, jo, dt, variant, 7, ncol, n, src)
            hv = [src(("v", k), n) for k in range(ncol)]
            v = J.from_numpy(np.concatenate(hv), J.domain(A))
            nat = _native(A)
            for beta in (0.0, -0.625):
                hu0 = src(("u", 0), rows * n) if beta else np.full(rows * n, np.nan, dtype=dt)
                with np.errstate(all="ignore"):
                    t = jo.block_df(ora, [np.zeros(n, dt) for _ in range(rows)], hv)
                    empty = [np.empty(n, dtype=dt) for _ in range(rows)]
                    uref = jo.barr_lincomb(empty, [alpha, beta] if beta else [alpha], [t, np.split(hu0, rows)] if beta else [t])
                    wref = np.concatenate(jo.block_df_adj(ora, [np.zeros(n, dt) for _ in range(ncol)], uref))
                keeps = inf_only_verdict(dt, cls, beta, np.concatenate(uref))
                if keeps is not None:
                    yield ("verdict", f"step of a {variant} {rows} x {ncol} grid of {n}, beta {beta}: ||u||^2 is expected to be Inf", keeps)
                for nt in (0, 2):
                    J.tune(nt=nt, adj_split=0)
                    try:
                        u, w = J.from_numpy(hu0, J.range(A)), J.from_numpy(src(("o", 1), ncol * n), J.domain(A))
                        out = C.c_double(-1.0)
                        st = lib.jh_blockop_bidiag_step(nat.handle, u.handle, v.handle, w.handle, alpha, beta, C.byref(out))
                    finally:
                        J.tune(nt=1, adj_split=-1)
                    tag = f"step of a {variant} {rows} x {ncol} grid of {n}, beta {beta}, nt {nt}"
                    if st != 0:
                        yield ("verdict", tag, f"jh_blockop_bidiag_step returned {st}")
                        continue
                    yield ("same", f"{tag}: u", _flat(u), np.concatenate(uref))
                    yield ("same", f"{tag}: w", _flat(w), wref)
                    yield ("verdict", f"{tag}: ||u||^2", normsq_verdict(out.value, np.concatenate(uref)))
            J.close(A)


# ---------------------------------------------------------------------------------------------------- per-block reductions
def short_ragged_blocks(dt):
    """The 1,500 blocks of tests/test_gpu_vectors.py: test_per_block_reductions_of_many_short_blocks."""
    rng = np.random.default_rng(5)
    lens = [int(v) for v in rng.integers(0, 700, size=1500)]
    lens[7] = 0
    lens[8] = 4096 // (np.dtype(dt).itemsize // 4)
    return lens


BLOCK_LISTS = {"7 x 1027": lambda dt: [1027] * 7, "4099, 5, 65536, 33, 1027": lambda dt: [4099, 5, 65536, 33, 1027], "1500 short ragged": short_ragged_blocks}


def _block_norm_ref(jo, x, p):
    """norm(x_i, p) of a block: NaN if the block holds one (every fold of the reference keeps it: `max` / `min` answer NaN when they meet one,
    src/Jets.jl:835-838; a sum that meets one is NaN; count_nonzero counts NaN != 0, no NaN comes out), else Inf rules by the fp64 formula."""
    wide = np.complex128 if x.dtype.kind == "c" else np.float64
    with np.errstate(all="ignore"):
        ab = np.abs(x.astype(wide))
        if x.dtype.kind == "c":                                               # |z| of a complex with an infinite part is Inf even beside a NaN part (hypot)
            parts = x.view(_rt(x.dtype)).reshape(-1, 2)
            ab = np.where(np.isinf(parts).any(axis=1), np.inf, ab)
        if ab.size == 0:
            return 0.0
        if p == 0:
            return float(np.count_nonzero(ab))
        if np.isnan(ab).any():
            return float("nan")
        if p == np.inf:
            return float(ab.max())
        if p == -np.inf:
            return float(ab.min())
        return float(ab.sum()) if p == 1 else float((ab ** p).sum() ** (1.0 / p))


def block_reduction_case(J, jo, dt, listname, cls):
    """jh_norm_blocks / jh_dot_blocks, workgroup-per-block and wave-per-block kernels: a poisoned scalar poisons ITS block and no other."""
    lens = BLOCK_LISTS[listname](dt)
    e = scalars_per_elem(dt)
    rng = np.random.default_rng([41, len(lens)])
    rt = _rt(dt)

    def u01n(n):
        if e == 2:
            x = np.empty(n, dtype=dt)
            x.real, x.imag = rng.random(n).astype(rt), rng.random(n).astype(rt)
            return x
        return rng.random(n).astype(rt)

    total = int(sum(lens))
    hx, hy = u01n(total), u01n(total)
    cx, cy = hx.copy(), hy.copy()                                             # the clean values
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if cls == "all-special":
        i = max(range(len(lens)), key=lambda k: (lens[k] <= 1027, lens[k]))   # the longest block of at most 1027 elements
        with np.errstate(all="ignore"):
            hx[offs[i]:offs[i + 1]] = specials(rng, dt, lens[i], frac=1.0)
            hy[offs[i]:offs[i + 1]] = specials(rng, dt, lens[i], frac=1.0)
    else:
        pos = slab_seam_positions([n * e for n in lens], cls)
        poison(hx, pos, rot=0)
        poison(hy, pos, rot=1)
    dirty = np.zeros(len(lens), dtype=bool)                                   # blocks that own a changed scalar (from the data, not the generator)
    for i in range(len(lens)):
        sl = slice(offs[i], offs[i + 1])
        dirty[i] = hx[sl].tobytes() != cx[sl].tobytes() or hy[sl].tobytes() != cy[sl].tobytes()
    yield ("verdict", f"{listname}, {cls}: the case poisons some blocks and not others", True if dirty.any() and not dirty.all() else "vacuous case")
    R = J.JetBSpace([J.JetSpace(dt, n) for n in lens])
    x, y = J.from_numpy(hx, R), J.from_numpy(hy, R)
    tol = 1e-5 if rt == np.float32 else 1e-12
    for wave in (1, 0):
        J.tune(red_blocks_wave=wave)
        try:
            got_n = {p: np.asarray(J.norm_blocks(x, p)).astype(np.float64) for p in (2, 1, 0, np.inf, -np.inf, 3)}
            got_d = np.asarray(J.dot_blocks(x, y)).astype(np.complex128)
        finally:
            J.tune(red_blocks_wave=1)
        for p, got in got_n.items():
            bad = []
            for i in range(len(lens)):
                want = _block_norm_ref(jo, hx[offs[i]:offs[i + 1]], p)
                g = float(got[i])
                if not dirty[i]:
                    clean = _block_norm_ref(jo, cx[offs[i]:offs[i + 1]], p)
                    ok = np.isfinite(g) and abs(g - clean) <= tol * max(abs(clean), 1e-30)
                elif np.isnan(want):
                    ok = np.isnan(g)
                elif np.isinf(want):
                    ok = g == want
                else:
                    ok = np.isfinite(g) and abs(g - want) <= tol * max(abs(want), 1e-30)
                if not ok:
                    bad.append((i, g, want))
            yield ("verdict", f"norm_blocks p = {p}, {listname}, {cls}, red_blocks_wave {wave}", True if not bad else f"{len(bad)} blocks differ, first (block, got, want) {bad[:3]}")
        bad = []
        for i in range(len(lens)):
            sl = slice(offs[i], offs[i + 1])
            with np.errstate(all="ignore"):                                   # dot conjugates its first argument; fp64, part by part (a real type has no imaginary part)
                (xr, xi), (yr, yi) = [((a.real.astype(np.float64), a.imag.astype(np.float64)) if e == 2 else (a.astype(np.float64), None))
                                      for a in ((hx if dirty[i] else cx)[sl], (hy if dirty[i] else cy)[sl])]
                want = complex(np.sum(xr * yr + xi * yi), np.sum(xr * yi - xi * yr)) if e == 2 else complex(np.sum(xr * yr), 0.0)
            g = complex(got_d[i])
            ok = True
            scale = float(np.hypot(*[v if np.isfinite(v) else 0.0 for v in (want.real, want.imag)]))   # (the tolerance of a finite part beside a non-finite one)
            for gp, wp in ((g.real, want.real), (g.imag, want.imag)):
                if np.isnan(wp):
                    ok &= bool(np.isnan(gp))
                elif np.isinf(wp):
                    ok &= gp == wp
                else:
                    ok &= bool(np.isfinite(gp) and abs(gp - wp) <= tol * max(scale, 1e-30))
            if not ok:
                bad.append((i, g, want))
        yield ("verdict", f"dot_blocks, {listname}, {cls}, red_blocks_wave {wave}", True if not bad else f"{len(bad)} blocks differ, first (block, got, want) {bad[:3]}")


# ---------------------------------------------------------------------------------------------------- the split walk
def _rows_reversed(rig, fn):
    """fn() with the rig's oracle rows (operator rows and weights) in reversed order: the other row order of the condition."""
    ora, hw = rig.ora, rig.hw
    rig.ora, rig.hw = ora[::-1], [w[::-1] for w in hw]
    try:
        return fn()
    finally:
        rig.ora, rig.hw = ora, hw


def _chain_tol(dt, nrow):
    """tests/test_gpu_chains.py: test_chains_over_many_small_rows_take_the_split_walk"""
    return (2e-5 if _rt(dt) == np.float32 else 1e-13) * np.sqrt(nrow)


def _abs_ok(tol):
    def ok(g, w):
        err, scale = np.abs(g - w).max(), np.abs(w).max()
        return True if err <= tol * scale else f"finite scalars differ by {err:.3e}, allowed {tol * scale:.3e}"
    return ok


def _allclose_ok(dt):
    """tests/test_gpu_grid_chains.py: test_every_launch_shape_has_the_same_bits (split rows)"""
    def ok(g, w):
        rtol = 1e-4 if _rt(dt) == np.float32 else 1e-12
        bad = np.abs(g - w) > 1e-5 + rtol * np.abs(w)
        return True if not bad.any() else f"{int(bad.sum())} finite scalars outside rtol {rtol}, atol 1e-5"
    return ok


def _relerr_ok(dt):
    """tests/test_gpu_chain_step.py: test_split_walk_of_many_small_rows"""
    def ok(g, w):
        den = np.linalg.norm(w.astype(np.complex128))
        err = np.linalg.norm((g.astype(np.complex128) - w.astype(np.complex128))) / (den if den else 1.0)
        lim = 2e-5 if _rt(dt) == np.float32 else 1e-13
        return True if err < lim else f"relative error {err:.3e} of the finite scalars, allowed {lim}"
    return ok


COLUMN_BLOCK = 16


class ColumnSource:
    """The split walk's second input: finite U[0,1) data, and in the listed `rows` of the arrays whose tag letter is in `tags` (a slab of rows of n
    elements, or the coefficient block ("A", i, j) of row i) every special value has COLUMNS OF ITS OWN, so that the sum over hundreds of rows keeps
    clean infinities and clean finite scalars beside the NaN.  Columns come in blocks of 16 (real parts; imaginary parts stay finite); block b
    belongs to tag b mod len(tags) and to ONE of the rows, which gets NaN, +Inf, -Inf, -0, a denormal, +1, -1, +0 in its columns 0 .. 7: every
    other row of those columns is finite.  Column 9 holds +Inf in EVERY listed row (a sum of +Inf partials from several parts), column 10 +Inf
    in the first listed row and -Inf in the last (Inf - Inf across parts: NaN in any order)."""

    def __init__(self, dt, seed, n, rows, tags):
        self.dt, self.n, self.rows, self.tags, self.clean = dt, n, list(rows), tuple(tags), Source(dt, "clean", seed)
        fi = np.finfo(_rt(dt))
        self.values = {0: np.nan, 1: np.inf, 2: -np.inf, 3: -0.0, 4: fi.tiny / 4, 5: 1.0, 6: -1.0, 7: 0.0}

    def __call__(self, tag, count):
        x = self.clean(tag, count)
        if tag[0] not in self.tags or not self.rows:
            return x
        t, nt, n, rows = self.tags.index(tag[0]), len(self.tags), self.n, self.rows
        re = x.real                                                           # (a view; a real array is its own real part)
        where = {tag[1]: 0} if tag[0] == "A" else {r: r * n for r in rows if (r + 1) * n <= count}
        for r, off in where.items():
            if r not in rows:
                continue
            k = rows.index(r)
            for b in range(-(-n // COLUMN_BLOCK)):
                if b % nt != t:
                    continue
                put = {}
                if rows[(b // nt) % len(rows)] == r:
                    put.update(self.values)
                put[9] = np.inf
                if k == 0:
                    put[10] = np.inf
                if k == len(rows) - 1:
                    put[10] = -np.inf
                for c, v in put.items():
                    if COLUMN_BLOCK * b + c < n:
                        re[off + COLUMN_BLOCK * b + c] = v
        return x


def population_verdict(want, need_inf, least=20):
    """A split-walk case must not be vacuous: the oracle's result holds finite scalars, NaN (and, need_inf, infinities), some tens of each."""
    w = np.ascontiguousarray(want).view(_rt(want.dtype))
    nfin, ninf, nnan = int(np.isfinite(w).sum()), int(np.isinf(w).sum()), int(np.isnan(w).sum())
    ok = nfin >= least and nnan >= least and (ninf >= least or not need_inf)
    return True if ok else f"VACUOUS CASE: the oracle's result holds {nfin} finite, {ninf} infinite, {nnan} NaN scalars; at least {least} of each are needed"


def _split_sources(dt, n, nrow, split, seed, probe, frac, tags, usable=lambda r: True):
    """(name, source, whether clean infinities are required): the sparse order-free mix (frac: so sparse that sums over all rows keep finite
    scalars), and the special values in columns of their own in the first and last row of every part (ColumnSource; usable(row): rows that
    reach the sum).  split = -1: the library picks the part count, probe() runs the clean shape and reads it."""
    yield "order-free mix", Source(dt, "order-free", seed, frac=frac), False
    parts = split if split > 0 else probe()
    rows = [r for r in part_edge_rows(nrow, parts) if usable(r)]
    yield f"special values by column in the first and last row of {parts} parts", ColumnSource(dt, seed, n, rows, tags), True


def split_tall_case(J, jo, dt, chain, split):
    from jets_jl_amd import chains
    from tests.test_gpu_chains import Rig

    toks, kind = TALL_CHAINS[chain]
    ctype = {"adj": chains.CHAIN_ADJOINT, "normal": chains.CHAIN_NORMAL}[kind]
    nrow, n = 512, 259

    def run(src):
        rig = Rig(J, jo, dt, nrow, n, "mixed", seed=31, with_wb=False, data=src)
        cache = chains.ChainCache()
        h = chains.one_run(chains.stages_of(rig.compose(toks)), cache, "t", ctype)
        hx = [src(("x", i), n) for i in range(nrow if kind == "adj" else 1)]
        x = J.from_numpy(np.concatenate(hx), J.range(rig.A) if kind == "adj" else J.domain(rig.A))
        J.tune(adj_split=split)
        try:
            y = _flat(h.apply(J.from_numpy(src(("o", 0), n), J.domain(rig.A)), x, 0))
            parts = J.tune_get("last_adj_parts")
        finally:
            J.tune(adj_split=-1)
        with np.errstate(all="ignore"):
            want = np.concatenate(rig.ora_apply(toks, hx))
            rev = np.concatenate(_rows_reversed(rig, lambda: rig.ora_apply(toks, hx[::-1] if kind == "adj" else hx)))
        cache.close()
        rig.close()
        return y, want, rev, parts

    def probe():
        return run(Source(dt, "clean", 3))[3]

    from tests.test_gpu_chains import _kinds

    kinds = _kinds(nrow, "mixed")
    for sname, src, need_inf in _split_sources(dt, n, nrow, split, 31, probe, 0.0015, ("w",), usable=lambda r: kinds[r][0] != "zero"):
        y, want, rev, parts = run(src)
        tag = f"{chain}, {nrow} rows of {n}, adj_split {split}, {sname}"
        yield ("verdict", f"{tag}: the split walk ran", True if parts > 1 else "one part")
        yield ("verdict", f"{tag}: finite, infinite and NaN results all occur", population_verdict(want, need_inf))
        yield ("verdict", f"{tag}: the case does not depend on the row order", order_free_verdict(want, rev))
        yield ("verdict", tag, masks_verdict(y, want, _abs_ok(_chain_tol(dt, nrow))))


def split_step_case(J, jo, dt, split):
    from jets_jl_amd import chains
    from tests.test_gpu_chains import Rig

    toks = ["A", ("W", 0, False), ("s", 0.75, "r")]
    nrow, n, alpha, beta = 512, 259, 1.0, -0.25

    def run(src):
        rig = Rig(J, jo, dt, nrow, n, "mixed", seed=31, with_wb=False, data=src)
        L = rig.compose(toks)
        sc = chains.SolverChains(L)
        hv, hu0 = src(("v", 0), n), src(("u", 0), nrow * n)
        u, v, w = J.from_numpy(hu0, J.range(L)), J.from_numpy(hv, J.domain(L)), J.from_numpy(src(("o", 1), n), J.domain(L))
        J.tune(adj_split=split)
        try:
            nsq = sc.step(u, v, w, alpha, beta)
            parts = J.tune_get("last_adj_parts")
        finally:
            J.tune(adj_split=-1)
        with np.errstate(all="ignore"):
            tmp = rig.ora_apply(toks, [hv])
            uref = jo.barr_lincomb([np.empty(n, dtype=dt) for _ in range(nrow)], [alpha, beta], [tmp, np.split(hu0, nrow)])
            wref = rig.ora_apply(adjoint_tokens(toks), uref)[0]
            wrev = _rows_reversed(rig, lambda: rig.ora_apply(adjoint_tokens(toks), uref[::-1]))[0]
        got = (_flat(u), _flat(w), nsq)
        sc.close()
        rig.close()
        return got, np.concatenate(uref), wref, wrev, parts

    def probe():
        return run(Source(dt, "clean", 3))[4]

    from tests.test_gpu_chains import _kinds

    kinds = _kinds(nrow, "mixed")
    for sname, src, need_inf in _split_sources(dt, n, nrow, split, 37, probe, 0.0015, ("w", "u"), usable=lambda r: kinds[r][0] != "zero"):
        (u, w, nsq), uref, wref, wrev, parts = run(src)
        tag = f"step of 0.75 * (W o A), {nrow} rows of {n}, adj_split {split}, {sname}"
        yield ("verdict", f"{tag}: the split walk ran", True if parts > 1 else "one part")
        yield ("verdict", f"{tag}: finite, infinite and NaN results all occur", population_verdict(wref, need_inf))
        yield ("verdict", f"{tag}: the case does not depend on the row order", order_free_verdict(wref, wrev))
        yield ("same", f"{tag}: u (independent of the part count)", u, uref)
        yield ("verdict", f"{tag}: w", masks_verdict(w, wref, _relerr_ok(dt)))
        yield ("verdict", f"{tag}: ||u||^2", "the library declined the step" if nsq is None else normsq_verdict(nsq, uref))


def split_grid_case(J, jo, dt, what, split):
    import ctypes as C

    from jets_jl_amd._ffi import lib
    from tests.test_gpu_grid_chains import CHAINS, GridRig

    nrow, ncol, n, alpha, beta = 600, 3, 259, 1.25, -0.625
    toks = CHAINS["A' o W o A"]

    def run(src):
        rig = GridRig(J, jo, dt, nrow, ncol, n, data=src)
        hx = [src(("x", k), n) for k in range(ncol)]
        x = J.from_numpy(np.concatenate(hx), J.domain(rig.A))
        J.tune(adj_split=split)
        try:
            if what == "chain":
                y = _flat(J.mul_(J.from_numpy(src(("o", 0), ncol * n), J.domain(rig.A)), rig.compose(toks), x))
                extra = None
            else:
                hu0 = src(("u", 0), nrow * n)
                u, w = J.from_numpy(hu0, J.range(rig.A)), J.from_numpy(src(("o", 1), ncol * n), J.domain(rig.A))
                out = C.c_double(-1.0)
                st = lib.jh_blockop_bidiag_step(_native(rig.A).handle, u.handle, x.handle, w.handle, alpha, beta, C.byref(out))
                y, extra = _flat(w), (st, _flat(u), out.value)
            parts = J.tune_get("last_adj_parts")
        finally:
            J.tune(adj_split=-1)
        with np.errstate(all="ignore"):
            if what == "chain":
                want = np.concatenate(rig.ora_apply(toks, hx))
                rev = np.concatenate(_rows_reversed(rig, lambda: rig.ora_apply(toks, hx)))
                uref = None
            else:
                t = jo.block_df(rig.ora, [np.zeros(n, dt) for _ in range(nrow)], hx)
                uref = jo.barr_lincomb([np.empty(n, dtype=dt) for _ in range(nrow)], [alpha, beta], [t, np.split(hu0, nrow)])
                want = np.concatenate(jo.block_df_adj(rig.ora, [np.zeros(n, dt) for _ in range(ncol)], uref))
                rev = np.concatenate(jo.block_df_adj(rig.ora[::-1], [np.zeros(n, dt) for _ in range(ncol)], uref[::-1]))
                uref = np.concatenate(uref)
        rig.close()
        return y, want, rev, parts, extra, uref

    def probe():
        return run(Source(dt, "clean", 3))[3]

    for sname, src, need_inf in _split_sources(dt, n, nrow, split, 43, probe, 0.0005, ("w",) if what == "chain" else ("u",)):
        y, want, rev, parts, extra, uref = run(src)
        tag = f"grid {what}, {nrow} x {ncol} of {n}, adj_split {split}, {sname}"
        yield ("verdict", f"{tag}: the split walk ran", True if parts > 1 else "one part")
        yield ("verdict", f"{tag}: finite, infinite and NaN results all occur", population_verdict(want, need_inf))
        yield ("verdict", f"{tag}: the case does not depend on the row order", order_free_verdict(want, rev))
        yield ("verdict", tag, masks_verdict(y, want, _allclose_ok(dt) if what == "chain" else _abs_ok(_chain_tol(dt, nrow))))
        if extra is not None:
            yield ("verdict", f"{tag}: status", True if extra[0] == 0 else f"jh_blockop_bidiag_step returned {extra[0]}")
            yield ("same", f"{tag}: u (independent of the part count)", extra[1], uref)
            yield ("verdict", f"{tag}: ||u||^2", normsq_verdict(extra[2], uref))


# ---------------------------------------------------------------------------------------------------- one big-block pass
def big_case(J, jo, dt, what, n):
    """Rows long enough that the launchers pick the fat shape and nontemporal loads on their own: no knob is touched."""
    one = (("one", 3, "diag"),)
    if what == "tall A' o W o A":
        for rec in tall_composite_big(J, jo, dt, n):
            yield rec
    elif what == "chain step":
        for rec in chain_step_case(J, jo, dt, "W o A", "mix", lens=(n,), knobs=[{}], row_configs=one):
            yield rec
    else:
        from jets_jl_amd import chains
        from tests.test_gpu_grid_chains import CHAINS, GridRig

        src = Source(dt, "mix", 47)
        rig = GridRig(J, jo, dt, 6, 3, n, data=src)
        toks = CHAINS["A' o W o A"]
        hx = [src(("x", k), n) for k in range(3)]
        g0 = chains.STATS["grid_chain_calls"]
        y = J.mul_(J.from_numpy(src(("o", 0), 3 * n), J.domain(rig.A)), rig.compose(toks), J.from_numpy(np.concatenate(hx), J.domain(rig.A)))
        shape = J.tune_get("last_grid_chain_shape")
        yield ("verdict", "big 6 x 3 grid chain: one grid chain", True if chains.STATS["grid_chain_calls"] - g0 == 1 else "not one grid chain")
        yield ("verdict", "big 6 x 3 grid chain: the launcher chose nontemporal loads on its own", True if shape & 1 else f"last_grid_chain_shape = {shape}")
        with np.errstate(all="ignore"):
            want = np.concatenate(rig.ora_apply(toks, hx))
        yield ("same", f"A' o W o A through a 6 x 3 grid of {n}", _flat(y), want)
        rig.close()


def tall_composite_big(J, jo, dt, n):
    from jets_jl_amd import chains
    from tests.test_gpu_chains import Rig

    src = Source(dt, "mix", 53)
    rig = Rig(J, jo, dt, 3, n, "diag", with_wb=False, data=src)
    toks = TALL_CHAINS["A' o W o A"][0]
    hx = [src(("x", 0), n)]
    before = chains.STATS["chain_calls"]
    y = J.mul_(J.from_numpy(src(("o", 0), n), J.domain(rig.A)), rig.compose(toks), J.from_numpy(hx[0], J.domain(rig.A)))
    yield ("verdict", "big tall A' o W o A: one fused run", True if chains.STATS["chain_calls"] - before == 1 else "not one fused run")
    with np.errstate(all="ignore"):
        want = np.concatenate(rig.ora_apply(toks, hx))
    yield ("same", f"A' o W o A, 3 rows of {n}", _flat(y), want)
    rig.close()


ALL_DTYPES = (np.float32, np.float64, np.complex64, np.complex128)
BIG_N = 4 << 20


def fused_cases(big_n=BIG_N):
    """[(id, dtype, function(J, jo) -> records)]: the id names family, chain / variant, element type and input (position) class."""
    from functools import partial as P

    from tests.test_gpu_chain_step import STEP_CHAINS
    from tests.test_gpu_chains import CHAINS

    out = []

    def add(family, name, dt, cls, fn):
        out.append((f"{family} | {name} | {np.dtype(dt).name} | {cls}", dt, fn))

    for dt in ALL_DTYPES:
        for cls in ("mix",) + SEAM_CLASSES:
            for chain, (_, kind) in TALL_CHAINS.items():
                if cls == "range-edge" and kind == "fwd":
                    continue                                                  # (a FORWARD chain has no ranged entry)
                add("tall chain", chain, dt, cls, P(tall_chain_case, dt=dt, chain=chain, cls=cls))
            if cls == "range-edge":
                continue
            if cls in ("mix", "head", "overlap"):
                for chain in CHAINS:
                    add("tall composite", chain, dt, cls, P(tall_composite_case, dt=dt, chain=chain, cls=cls))
            for chain in STEP_CHAINS:
                add("chain step", chain, dt, cls, P(chain_step_case, dt=dt, chain=chain, cls=cls))
            for variant in ("plain", "regularised"):
                add("grid A'A", variant, dt, cls, P(grid_normal_case, dt=dt, variant=variant, cls=cls))
            for variant in ("plain", "mixed"):
                for chain in GRID_CHAINS:
                    add("grid chain", f"{chain}, {variant}", dt, cls, P(grid_chain_case, dt=dt, chain=chain, variant=variant, cls=cls))
            for variant in ("plain", "mixed", "regularised"):
                add("grid step", variant, dt, cls, P(grid_step_case, dt=dt, variant=variant, cls=cls))
        for cls in STEP_CLASSES:
            for chain in STEP_CHAINS:
                add("chain step", chain, dt, cls, P(chain_step_case, dt=dt, chain=chain, cls=cls))
            for variant in ("plain", "mixed", "regularised"):
                add("grid step", variant, dt, cls, P(grid_step_case, dt=dt, variant=variant, cls=cls))
        for listname in BLOCK_LISTS:
            for cls in ("block-last", "block-first", "all-special"):
                add("block reductions", listname, dt, cls, P(block_reduction_case, dt=dt, listname=listname, cls=cls))
        for split in (-1, 3):
            for chain in ("A' o W o A", "(W o A)'"):
                add("split walk", f"tall {chain}", dt, f"adj_split {split}", P(split_tall_case, dt=dt, chain=chain, split=split))
            add("split walk", "chain step", dt, f"adj_split {split}", P(split_step_case, dt=dt, split=split))
            add("split walk", "grid chain", dt, f"adj_split {split}", P(split_grid_case, dt=dt, what="chain", split=split))
            add("split walk", "grid step", dt, f"adj_split {split}", P(split_grid_case, dt=dt, what="step", split=split))
    for dt in (np.float32, np.complex64):
        for what in ("tall A' o W o A", "chain step", "6 x 3 grid chain"):
            add("big blocks", what, dt, "mix", P(big_case, dt=dt, what=what, n=big_n))
    return out


def run_fused_checks(J, jo, select=None, big_n=BIG_N):
    """[(dtype name, what, True | mismatch text)] over fused_cases() (select(id) -> bool picks some): the counterpart of run_checks."""
    results = []
    for cid, dt, fn in fused_cases(big_n):
        if select is not None and not select(cid):
            continue
        bad, count = [], 0
        records = fn(J, jo)
        try:
            for rec in records:
                count += 1
                r = same(rec[2], rec[3]) if rec[0] == "same" else rec[2]
                if r is not True:
                    bad.append(f"{rec[1]}: {r}")
        finally:
            records.close()                                                   # (a case resets the knobs it forces in its own finally)
        results.append((np.dtype(dt).name, cid, True if count and not bad else (f"{len(bad)} of {count} checks; first: {bad[0]}" if bad else "no check ran")))
    return results


if __name__ == "__main__":
    import jets_jl_amd as J
    from oracle import jets_oracle as jo

    J.init(0)
    big = len(sys.argv) > 1
    out = run_checks(J, jo, n=int(sys.argv[1]) if big else 4096 + 24)   # e.g. 6291456: blocks of 24-48 MiB take the big-block routes
    for name, what, r in out:
        print(f"{name:10s} {what:38s} {'ok' if r is True else 'MISMATCH: ' + str(r)}", flush=True)
    # the fused families: every case at the small sizes, or (with a size) the one big-block pass at that size
    fused = run_fused_checks(J, jo, select=(lambda cid: cid.startswith("big blocks")) if big else (lambda cid: not cid.startswith("big blocks")),
                             big_n=int(sys.argv[1]) if big else BIG_N)
    for name, what, r in fused:
        print(f"{what:100s} {'ok' if r is True else 'MISMATCH: ' + str(r)}", flush=True)
    sys.exit(1 if any(r is not True for _, _, r in out + fused) else 0)
