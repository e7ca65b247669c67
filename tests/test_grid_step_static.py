"""Static checks of the one-pass step of N x K grids (jh_grid_step.hip) that need no GPU: the header documents the step, its knob and its counter,
the built library holds k_grid_step with no scratch and no SGPR spills, and the Julia binding's step and solvers consult grid_native."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jets.jl_amd", "libjetship.so")


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


def test_header_documents_the_grid_step_the_knob_and_the_counter():
    h = _read("include", "jetship.h")
    at = h.index("int jh_blockop_bidiag_step(")
    doc = h[h.rindex("/*", 0, at):at]
    assert "GRID STEP" in doc and "N x K grid" in doc and '"grid_step"' in doc and '"last_grid_step_shape"' in doc
    assert '"grid_step" (jh_blockop_bidiag_step, jh_lsqr_solve and jh_cgls_solve on N x (2 .. 4) grids' in h        # the knob list
    assert '"last_grid_step_shape" (how the latest grid step was launched' in h                                       # the counter list
    lsqr = h[h.rindex("/*", 0, h.index("typedef struct {\n    int32_t istop, itn;")):h.index("int jh_lsqr_solve(")]
    assert "jh_lsqr_solve also takes an N x (2 .. 4) grid" in lsqr and "decline grids" in lsqr
    cgls = h[h.rindex("/*", 0, h.index("int jh_cgls_solve(")):h.index("int jh_cgls_solve(")]
    assert "jh_cgls_solve also takes an N x (2 .. 4) grid" in cgls
    assert "jh_chain_apply_range and jh_chain_bidiag_step on a grid chain return JH_ERR_UNSUPPORTED" in h   # grid CHAINS are not stepped


def test_k_grid_step_is_built_without_scratch_or_sgpr_spills():
    if not os.path.exists(LIB):
        pytest.fail("libjetship.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    ks = kernel_resources.kernels(LIB)
    names = kernel_resources.demangle([k["name"] for k in ks])
    mine = [(k, n) for k, n in zip(ks, names) if "k_grid_step<" in n]
    # 4 element types x K = 2 .. 4 x {plain, several kinds} x {temporal, nontemporal} x {beta == 0, beta != 0}
    assert len(mine) == 96, len(mine)
    bad = [(n, k["scratch"], k["sgpr_spills"]) for k, n in mine if k["scratch"] or k["sgpr_spills"]]
    assert not bad, bad


def _julia_function(src, name):
    start = src.index("function " + name)
    end = src.index("\nend\n", start)
    return src[start:end]


def test_julia_step_and_solvers_consult_grid_native():
    jl = _read("julia", "JetsHIP.jl")
    for name in ("bidiag_step!(u::BlockArray{T,<:HipArray{T}}, w::HipArray{T}, A::JopLn", "hip_lsqr!(", "hip_cgls!("):
        body = _julia_function(jl, name)
        t, g, c = body.index("tall_native(A, T)"), body.index("grid_native(A, T)"), body.index("_plan_chain(A, T")
        assert t < g < c, name                  # after tall_native, before the chain planner
