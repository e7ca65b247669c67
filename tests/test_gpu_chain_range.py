"""GPU: jh_chain_apply_range -- the ADJOINT / NORMAL chains on an element range of the domain (the weighted normal equations of a row partition,
src/Jets.jl:530-540 over 1034-1057; jh_tall_chain.hip).

The bar: ranges that tile the domain write, together, the bits of jh_chain_apply (whenever both walk the rows in one part: always here except the
many-small-rows case, which is tolerance parity like every split walk); a range writes its elements and no other; the
whole-vector chain is the oracle's stage-by-stage chain.  All four element types, rows on and off the 16-byte grid, every `accumulate`, the
forced launch shapes, and the documented errors."""
import ctypes as C

import numpy as np
import pytest

from .helpers import DTYPES, assert_bits_equal, u01
from .test_gpu_chains import Rig

pytestmark = pytest.mark.gpu

# name: tokens in application order (tests/test_gpu_chains.py: Rig), chain type
RANGE_CHAINS = {
    "(W o A)'": ([("W", 0, True), "At"], "adj"),
    "A' o W o A": (["A", ("W", 0, False), "At"], "normal"),
    "M' o A' o W o A o M": ([("M", 0, False), "A", ("W", 0, False), "At", ("M", 0, True)], "normal"),
    "A' o (a W) o A": (["A", ("W", 1, False), ("s", -1.25, "r"), "At"], "normal"),
    "a * (W o A)'": ([("W", 0, True), "At", ("s", 0.375, "d")], "adj"),
    "A' o Wb o A": (["A", ("Wb", 0, False), "At"], "normal"),
}


def _es(dt):
    return np.dtype(dt).itemsize


def _range_sets(nd, dt):
    """(name, [(first, count)]) in ELEMENTS: one range, three ranges on the 16-byte grid (the last ends with the vector), a one-pack range, count 0"""
    al = 16 // _es(dt) if _es(dt) < 16 else 1
    step = -(-(-(-nd // 3)) // al) * al
    three = [(lo, min(step, nd - lo)) for lo in range(0, nd, step)]
    return [("one", [(0, nd)]), ("three", three), ("one pack", [(al, al)]), ("empty", [(al, 0)])]


def _handle(J, rig, toks, kind):
    from jets_jl_amd import chains

    C_ = rig.compose(toks)
    cache = chains.ChainCache()
    h = chains.one_run(chains.stages_of(C_), cache, "t", chains.CHAIN_ADJOINT if kind == "adj" else chains.CHAIN_NORMAL)
    assert h is not None, "one fused run"
    return C_, h, cache


def _input(J, oracle, rig, kind, dt, n, nrow, seed=91):
    if kind == "adj":
        hx = [u01(oracle, dt, seed, i, n) for i in range(nrow)]
        return J.from_numpy(np.concatenate(hx), J.range(rig.A)), hx
    hx = [u01(oracle, dt, seed, 0, n)]
    return J.from_numpy(hx[0], J.domain(rig.A)), hx


def _dirty(J, rig, seed):
    return J.rand(J.domain(rig.A), seed=seed, stream=4)


def _check_ranges(J, rig, h, x, nd, dt, tag):
    """every range set x every accumulate: tiles == jh_chain_apply bit for bit, elements outside a range untouched"""
    from jets_jl_amd import chains

    for acc in (0, 1, -1, 2, -2):
        whole = h.apply(_dirty(J, rig, 7), x, acc).to_numpy().ravel(order="F")
        for rname, ranges in _range_sets(nd, dt):
            before = chains.STATS["chain_range_calls"]
            out = _dirty(J, rig, 7)
            dirty = out.to_numpy().ravel(order="F")
            for lo, cnt in ranges:
                h.apply_range(out, x, lo, cnt, acc)
            assert chains.STATS["chain_range_calls"] == before + len(ranges)
            got = out.to_numpy().ravel(order="F")
            covered = np.zeros(nd, dtype=bool)
            for lo, cnt in ranges:
                covered[lo:lo + cnt] = True
            assert_bits_equal(got[covered], whole[covered], f"{tag}: {rname} ranges, accumulate {acc}, vs jh_chain_apply")
            assert_bits_equal(got[~covered], dirty[~covered], f"{tag}: {rname} ranges, accumulate {acc}: elements outside the ranges")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(RANGE_CHAINS))
@pytest.mark.parametrize("nrow,n,kinds", [(5, 4096 + 64, "diag"), (7, 1027, "diag"), (9, 1027, "mixed")])
def test_ranges_have_the_bits_of_the_whole_vector_chain(Jets, oracle, dt, name, nrow, n, kinds):
    J = Jets
    toks, kind = RANGE_CHAINS[name]
    rig = Rig(J, oracle, dt, nrow, n, kinds)
    C_, h, cache = _handle(J, rig, toks, kind)
    x, hx = _input(J, oracle, rig, kind, dt, n, nrow)
    want = np.concatenate(rig.ora_apply(toks, hx))
    assert_bits_equal(h.apply(_dirty(J, rig, 8), x, 0).to_numpy().ravel(order="F"), want, f"{name}: jh_chain_apply vs the oracle's stage-by-stage chain")
    _check_ranges(J, rig, h, x, n, dt, name)
    # the ranged chain vs the oracle, range by range (the oracle's loop: oracle.block_df_adj on the weighted inputs)
    out = _dirty(J, rig, 9)
    for lo, cnt in _range_sets(n, dt)[1][1]:
        h.apply_range(out, x, lo, cnt, 0)
        assert J.tune_get("last_adj_parts") == 1
    assert_bits_equal(out.to_numpy().ravel(order="F"), want, f"{name}: three ranges vs the oracle")
    cache.close()
    rig.close()


@pytest.mark.parametrize("shape", [(256, 0), (512, 2), (512, 4)])
@pytest.mark.parametrize("nt", [0, 2])
@pytest.mark.parametrize("dt", [np.float32, np.complex128])
def test_forced_launch_shapes(Jets, oracle, dt, shape, nt):
    """tune(adj_wg, adj_unroll) picks k_chain_adj's shape (256 x 1 x 4, 512 x 2 x 2, 512 x 4 x 2), nt its loads; adj_split = 0: one part always"""
    J = Jets
    nrow, n = 6, 3 * 4096 + 64
    J.tune(adj_wg=shape[0], adj_unroll=shape[1], nt=nt, adj_split=0)
    try:
        for name in ("A' o W o A", "(W o A)'", "a * (W o A)'"):
            toks, kind = RANGE_CHAINS[name]
            rig = Rig(J, oracle, dt, nrow, n, "mixed", with_wb=False)
            C_, h, cache = _handle(J, rig, toks, kind)
            x, hx = _input(J, oracle, rig, kind, dt, n, nrow)
            want = np.concatenate(rig.ora_apply(toks, hx))
            assert_bits_equal(h.apply(_dirty(J, rig, 8), x, 0).to_numpy().ravel(order="F"), want, f"{name} {shape} nt={nt}: vs the oracle")
            _check_ranges(J, rig, h, x, n, dt, f"{name} {shape} nt={nt}")
            cache.close()
            rig.close()
    finally:
        J.tune(adj_wg=0, adj_unroll=0, nt=1, adj_split=-1)


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64])
def test_many_small_rows_take_the_split_walk_per_range(Jets, oracle, dt):
    """700 rows of 64 elements: every range cuts the row sum into parts (pick_adj_parts on the RANGE's workgroups) -- deterministic, within the
    split walk's tolerance of the whole-vector call and of the oracle; with adj_split = 0 the ranges have the whole-vector chain's bits again."""
    J = Jets
    nrow, n = 700, 64
    rig = Rig(J, oracle, dt, nrow, n, "diag", with_wb=False)
    tol = (2e-5 if np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == "c" else 1) == 4 else 1e-13) * np.sqrt(nrow)
    for name in ("A' o W o A", "a * (W o A)'"):
        toks, kind = RANGE_CHAINS[name]
        C_, h, cache = _handle(J, rig, toks, kind)
        x, hx = _input(J, oracle, rig, kind, dt, n, nrow)
        want = np.concatenate(rig.ora_apply(toks, hx))
        whole = h.apply(_dirty(J, rig, 8), x, 0).to_numpy().ravel(order="F")
        ranges = _range_sets(n, dt)[1][1]
        outs = []
        for _ in range(2):
            out = _dirty(J, rig, 9)
            for lo, cnt in ranges:
                h.apply_range(out, x, lo, cnt, 0)
                assert J.tune_get("last_adj_parts") > 1, "the split walk"
            outs.append(out.to_numpy().ravel(order="F"))
        assert_bits_equal(outs[0], outs[1], f"{name}: the ranged split walk is deterministic")
        scale = np.abs(want).max()
        assert np.abs(outs[0] - whole).max() <= tol * scale, f"{name}: ranges vs the whole-vector call"
        assert np.abs(outs[0] - want).max() <= tol * scale, f"{name}: ranges vs the oracle"
        J.tune(adj_split=0)
        try:
            whole0 = h.apply(_dirty(J, rig, 8), x, 0).to_numpy().ravel(order="F")
            out = _dirty(J, rig, 9)
            for lo, cnt in ranges:
                h.apply_range(out, x, lo, cnt, 0)
                assert J.tune_get("last_adj_parts") == 1
            assert_bits_equal(out.to_numpy().ravel(order="F"), whole0, f"{name}: ordered ranges vs the ordered whole-vector call")
            assert_bits_equal(whole0, want, f"{name}: ordered whole-vector call vs the oracle")
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


def test_errors(Jets, oracle):
    from jets_jl_amd import chains
    from jets_jl_amd._ffi import lib

    J = Jets
    dt, nrow, n = np.float32, 5, 1027
    rig = Rig(J, oracle, dt, nrow, n, "diag", with_wb=False)
    C_, h, cache = _handle(J, rig, RANGE_CHAINS["A' o W o A"][0], "normal")
    x, _ = _input(J, oracle, rig, "normal", dt, n, nrow)
    out = _dirty(J, rig, 3)
    dirty = out.to_numpy().tobytes()
    assert _status(lambda: h.apply_range(out, x, 1, 4, 0)) == 1                     # first on no 16-byte boundary
    assert _status(lambda: h.apply_range(out, x, 0, 6, 0)) == 1                     # an end off the grid that is not the vector's end
    assert _status(lambda: h.apply_range(out, x, 1024, 8, 0)) == 1                  # past the end
    assert _status(lambda: h.apply_range(out, x, -4, 4, 0)) == 1
    assert _status(lambda: h.apply_range(out, x, 0, 4, 3)) == 1                     # accumulate
    assert out.to_numpy().tobytes() == dirty
    assert _status(lambda: h.apply_range(out, x, 1024, 3, 0)) == 0                  # the last range may end inside a pack
    fwd = chains.one_run(chains.stages_of(rig.compose(["A", ("W", 0, False)])), cache, "f", chains.CHAIN_FORWARD)
    assert fwd is not None
    d = J.zeros(J.range(rig.A))
    assert _status(lambda: fwd.apply_range(d, x, 0, 4, 0)) == 4                     # a FORWARD chain needs no exchange
    assert lib.jh_chain_apply_range(None, out.handle, x.handle, 0, 0, 4) == 1          # a null handle
    cache.close()
    rig.close()


def test_a_range_that_needs_the_row_table_resynced_declines_inside_a_capture(Jets, oracle):
    """J(m)' o W o J(m) of SQUARE children: pointing the operator again moves the rows' arrays, and the chain's row table is copied to the device
    on the next application -- which must not happen inside a stream capture: the ranged entry declines (JH_ERR_UNSUPPORTED) there, and resyncs
    outside it with the bits of the whole-vector call."""
    from jets_jl_amd import chains, device
    from jets_jl_amd import jetblock as _blk

    J = Jets
    dt, n, nrow = np.float64, 1027, 5
    spc = J.JetSpace(dt, n)
    F = J.blockop([[J.JopSquare(spc)] if i % 2 == 0 else [J.JopDiagonal(J.rand(spc, seed=40 + i, stream=0))] for i in range(nrow)])
    W = J.JopDiagonal(J.rand(J.range(F), seed=50, stream=0))
    x = J.rand(spc, seed=51, stream=0)
    Jm = J.jacobian_(F, J.rand(spc, seed=60, stream=0))
    cache = chains.ChainCache()
    h = chains.one_run(chains.stages_of(J.compose(J.compose(Jm.H, W), Jm)), cache, "t", chains.CHAIN_NORMAL)
    assert h is not None
    y0 = h.apply(J.zeros(spc), x, 0)
    mo2 = J.rand(spc, seed=61, stream=0)
    Jm2 = J.jacobian_(F, mo2)
    assert _blk._tall_native(Jm2) is not None                                        # (pushes the new point to the native operator)
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p(device.stream_handle())
    out = J.zeros(spc)
    assert hip.hipStreamBeginCapture(stream, 2) == 0                                 # hipStreamCaptureModeRelaxed
    try:
        st = _status(lambda: h.apply_range(out, x, 0, n, 0))
    finally:
        graph = C.c_void_p()
        end = hip.hipStreamEndCapture(stream, C.byref(graph))
        if graph.value:
            hip.hipGraphDestroy(graph)
    assert end == 0
    assert st == 4, "the ranged entry declines a resync inside a capture"
    y1 = h.apply_range(J.zeros(spc), x, 0, n, 0)                                     # outside it: resynced
    y2 = J.mul_(J.zeros(spc), J.compose(J.compose(Jm2.H, W), Jm2), x)
    assert_bits_equal(y1.to_numpy(), y2.to_numpy(), "ranged chain after the resync")
    assert y1.to_numpy().tobytes() != y0.to_numpy().tobytes()
    cache.close()
