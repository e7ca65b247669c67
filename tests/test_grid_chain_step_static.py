"""Static checks of the one-pass step of FORWARD chains through N x K grids (jh_grid_chain_step.hip) that need no GPU: the header documents the
knob and the counter and keeps the sentence the earlier static tests search for, the built library holds k_grid_chain_step in the count DESIGN
states with no scratch and no SGPR spills, chains.py consults the knob, and the Julia binding's step and solvers plan grid chains under it."""
import os
import re
import sys

import pytest

from . import knob_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jets.jl_amd", "libjetship.so")


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


def test_header_documents_the_knob_and_the_counter():
    h = _read("include", "jetship.h")
    doc = h[h.rindex("/*", 0, h.index("typedef struct jh_chain jh_chain;")):h.index("int jh_chain_create(")]
    assert "jh_chain_apply_range and jh_chain_bidiag_step on a grid chain return JH_ERR_UNSUPPORTED" in doc      # the pinned sentence
    assert "GRID CHAIN STEP" in doc and '"grid_chain_step" = 1' in doc and "the default is 0" in doc
    assert '"last_grid_chain_step_shape"' in doc
    assert '"grid_chain_step" (jh_chain_bidiag_step, jh_lsqr_solve_chain and jh_cgls_solve_chain on a FORWARD chain through an N x (2 .. 4) grid' in h   # the knob list
    assert '"last_grid_chain_step_shape" (how the latest grid chain step was launched' in h                           # the counter list


def test_the_library_accepts_the_knob_with_default_zero():
    table = knob_table.rows()                                                   # jh_knobs.def: the field, jh_tune_set and jh_tune_get come from the row
    assert table["grid_chain_step"].kind == "JH_KNOB" and table["last_grid_chain_step_shape"].kind == "JH_COUNTER"   # set and get; the counter is read-only
    assert table["grid_chain_step"].default == 0
    assert "jh_grid_chain_step.hip" in _read("jets.jl_amd", "csrc", "Makefile")


def test_k_grid_chain_step_is_built_without_scratch_or_sgpr_spills():
    if not os.path.exists(LIB):
        pytest.fail("libjetship.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    ks = kernel_resources.kernels(LIB)
    names = kernel_resources.demangle([k["name"] for k in ks])
    mine = [(k, n) for k, n in zip(ks, names) if "k_grid_chain_step<" in n]
    # 4 element types x K = 2 .. 4 x NW = 0 .. 2 x {temporal, nontemporal} x {beta == 0, beta != 0}
    assert len(mine) == 144, len(mine)
    m = re.search(r"(\d+) instantiations of k_grid_chain_step", _read("DESIGN.md"))
    assert m and int(m.group(1)) == len(mine), "DESIGN.md section 3.8d states the instantiation count"
    bad = [(n, k["scratch"], k["sgpr_spills"]) for k, n in mine if k["scratch"] or k["sgpr_spills"]]
    assert not bad, bad
    assert not any("k_grid_step<" in n for _, n in mine)          # a family of its own: the grid step's count of 96 is pinned elsewhere


def test_chains_py_consults_the_knob():
    src = _read("jets.jl_amd", "chains.py")
    assert 'tune_get("grid_chain_step") == 1' in src
    step = src[src.index("    def step(self, u, v, w"):src.index("    def normal_planned(")]
    assert "grid_step_enabled()" in step and "jh_chain_bidiag_step" in step and '"grid_chain_calls"' in step
    assert "grid_step_enabled()" in _read("jets.jl_amd", "lsqr.py")


def _julia_function(src, name):
    start = src.index("function " + name)
    end = src.index("\nend\n", start)
    return src[start:end]


def test_julia_step_and_solvers_plan_grid_chains_under_the_knob():
    jl = _read("julia", "JetsHIP.jl")
    for name in ("bidiag_step!(u::BlockArray{T,<:HipArray{T}}, w::HipArray{T}, A::JopLn", "hip_lsqr!(", "hip_cgls!("):
        body = _julia_function(jl, name)
        assert "grid=false" not in body, name
        assert '_plan_chain(A, T; grid=(tune_get("grid_chain_step") == 1))' in body, name
        t, g, c = body.index("tall_native(A, T)"), body.index("grid_native(A, T)"), body.index("_plan_chain(A, T")
        assert t < g < c, name
