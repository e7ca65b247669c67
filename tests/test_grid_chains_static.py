"""Static checks of the grid chains (jh_grid_chain.hip) that need no GPU: the header documents them, the Julia binding mirrors the planner's
:grid stage, and the ctypes table still binds every jh_chain_* entry point with the header's argument count."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


def test_header_documents_grid_chains_and_the_knob():
    h = _read("include", "jetship.h")
    at = h.index("int jh_chain_create(")
    doc = h[h.rindex("/*", 0, h.index("typedef struct jh_chain jh_chain;")):at]
    assert "GRID CHAINS" in doc and "N x K grid" in doc
    assert "jh_chain_apply_range and jh_chain_bidiag_step on a grid chain return JH_ERR_UNSUPPORTED" in doc
    assert '"grid_chain"' in doc
    assert '"grid_chain" (jh_chain_create on N x (2 .. 4) grids' in h                   # the knob list
    assert '"last_grid_chain_shape"' in h


def _julia_function(src, name):
    start = src.index("function " + name)
    end = src.index("\nend\n", start)
    return src[start:end]


def test_julia_chain_stage_has_a_grid_branch():
    jl = _read("julia", "JetsHIP.jl")
    body = _julia_function(jl, "_chain_stage(")
    assert "kind=:grid" in body and "grid_native(base, T)" in body
    assert "function grid_native(" in jl


def test_julia_segments_accept_grid_where_they_accept_tall():
    jl = _read("julia", "JetsHIP.jl")
    body = _julia_function(jl, "_chain_segments(")
    assert "_anchors(st[j])" in body and "st[k].kind === t.kind" in body
    assert re.search(r"_anchors\(st\) = st\.kind === :tall \|\| st\.kind === :grid", jl)
    assert "t.ndom" in _julia_function(jl, "_chain_sides_ok(")


def test_ffi_binds_every_chain_entry_point_with_the_headers_argument_count():
    h = re.sub(r"/\*.*?\*/", "", _read("include", "jetship.h"), flags=re.S)
    ffi = _read("jets.jl_amd", "_ffi.py")
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(jh_chain_\w+)\s*\(([^)]*)\)\s*;", h)}
    assert {"jh_chain_create", "jh_chain_apply", "jh_chain_apply_range", "jh_chain_destroy", "jh_chain_bidiag_step"} <= set(protos)
    for name, args in protos.items():
        m = re.search(r'"%s":\s*\(_int,\s*\[(.*?)\]\),' % name, ffi)
        assert m, f"{name} is not bound in _ffi.py"
        n_py = len([a for a in re.split(r",\s*(?![^()]*\))", m.group(1)) if a.strip()])
        assert n_py == len([a for a in args.split(",") if a.strip()]), name


def test_the_python_planner_has_a_grid_stage_kind():
    src = _read("jets.jl_amd", "chains.py")
    assert 'Stage("grid", op, R' in src and '"grid_chain_calls"' in src
