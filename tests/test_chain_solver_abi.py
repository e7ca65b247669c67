"""CPU check: the solvers on a FORWARD chain are part of the C ABI -- include/jetship.h declares jh_chain_bidiag_step and jh_lsqr_solve_chain /
jh_cgls_solve_chain / jh_cgnr_solve_chain with the reference lines they stand for (the composite, src/Jets.jl:530-540; the solver loop over vec,
1138-1154), and jets.jl_amd/_ffi.py binds each with the header's argument count."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jetship.h")
NEW = ("jh_chain_bidiag_step", "jh_lsqr_solve_chain", "jh_cgls_solve_chain", "jh_cgnr_solve_chain")


def _header():
    return open(HEADER).read()


def _decl(text, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/jetship.h"
    return m


def _comment_before(text, pos):
    """The block comment that ends closest before `pos` (the entry point's documentation)."""
    end = text.rfind("*/", 0, pos)
    start = text.rfind("/*", 0, end)
    return text[start:end]


def test_header_declares_the_chain_solver_entry_points_with_their_citations():
    text = _header()
    for name in NEW:
        m = _decl(text, name)
        doc = _comment_before(text, m.start())
        assert "530-540" in doc and "1138-1154" in doc, f"{name}: the header comment does not cite src/Jets.jl:530-540 and 1138-1154"
    step = _decl(text, "jh_chain_bidiag_step").group(1)
    assert "const jh_chain *" in step and "double *normsq" in step


def test_ffi_binds_each_entry_point_like_the_header():
    import importlib.util

    spec = importlib.util.spec_from_file_location("_ffi_src", os.path.join(ROOT, "jets.jl_amd", "_ffi.py"))
    src = open(spec.origin).read()
    text = _header()
    for name in NEW:
        m = re.search(r'"' + name + r'":\s*\(_int,\s*\[([^\]]*)\]\)', src)
        assert m, f"_ffi.SYMBOLS does not bind {name}"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        hargs = len([a for a in _decl(text, name).group(1).split(",") if a.strip()])
        assert nargs == hargs, f"{name}: _ffi binds {nargs} arguments, the header declares {hargs}"


def test_abi_version_is_unchanged():
    assert re.search(r"#define JETSHIP_ABI_VERSION 4\b", _header())
