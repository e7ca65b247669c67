"""CPU: which function names the compiled broadcast has for which element type (hiprtc cross-compiles for gfx950 without a device:
jh_bcast_check).  The table is written once, in README.md; here it is held against the code: every name `bc` exports and every
target of the Julia binding's `_cfun` is in it, compiles for the types it lists and is refused -- a JetsHipError that quotes the
expression -- for the others (the functions with no complex definition)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = {"Float32": np.float32, "Float64": np.float64, "ComplexF32": np.complex64, "ComplexF64": np.complex128}
OPERATORS = {"+": "x0 + x1", "-": "x0 - x1 + (-x0)", "*": "x0 * x1", "/": "x0 / x1 + 2 / x0 + x1 / 3"}


def _readme_table():
    """name -> {column: True (exists) / False (refused)} from the marked table of README.md."""
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as f:
        text = f.read()
    body = text[text.index("<!-- bcast-function-table -->"):text.index("<!-- /bcast-function-table -->")]
    rows = [[c.strip() for c in line.strip().strip("|").split("|")] for line in body.splitlines() if line.startswith("|")]
    head, rows = rows[0], rows[2:]
    assert head[1:] == list(COLUMNS)
    table = {}
    for row in rows:
        assert all(c in ("yes", "refused") for c in row[1:]), row
        for name in re.findall(r"`([^`]+)`", row[0]):
            assert name not in table, f"{name} is listed twice"
            table[name] = {col: c == "yes" for col, c in zip(head[1:], row[1:])}
    return table


def _julia_cfun():
    """Julia function name -> emitted C name, from the text of julia/JetsHIP.jl."""
    with open(os.path.join(ROOT, "julia", "JetsHIP.jl"), encoding="utf-8") as f:
        text = f.read()
    m = re.search(r"const _cfun = Dict\{Any,String\}\((.*?)\)\n", text, re.S)
    assert m, "julia/JetsHIP.jl: _cfun not found"
    return dict(re.findall(r"(\S+) => \"([^\"]+)\"", m.group(1)))


def _expression(name):
    """An expression over x0, x1 that uses the table's `name` as the Python side emits it."""
    from jets_jl_amd import bc

    if name in OPERATORS:
        return OPERATORS[name]
    if name in bc.unary:
        return f"{name}(x0)"
    return f"{bc.binary[name]}(x0, x1)"


TABLE = _readme_table()


def test_the_table_lists_every_exported_name_and_every_julia_target():
    from jets_jl_amd import bc

    assert set(TABLE) == set(OPERATORS) | set(bc.unary) | set(bc.binary)
    assert len(bc.unary) == 24 and len(bc.binary) == 5
    for name in list(bc.unary) + list(bc.binary):
        assert callable(getattr(bc, name))
    with pytest.raises(AttributeError):
        bc.no_such_function
    # the Julia binding emits the same device names: an operator as itself, a function under its own name, max / min as the prelude's jl_max / jl_min
    python_emits = set(OPERATORS) | set(bc.unary) | set(bc.binary.values())
    cfun = _julia_cfun()
    assert set(cfun.values()) <= python_emits, set(cfun.values()) - python_emits
    assert cfun["max"] == bc.binary["maximum"] == "jl_max" and cfun["min"] == bc.binary["minimum"] == "jl_min"
    assert all(c == j for j, c in cfun.items() if j not in ("max", "min"))
    assert not any("fmax" in c or "fmin" in c for c in list(cfun.values()) + list(bc.binary.values()))   # C's fmax / fmin drop a NaN operand


@pytest.mark.parametrize("column", list(COLUMNS))
def test_listed_names_compile_and_refused_names_raise(column):
    import jets_jl_amd as J
    from jets_jl_amd._ffi import check, lib
    from jets_jl_amd.spaces import dtype_code

    code = dtype_code(COLUMNS[column])
    have = [n for n in TABLE if TABLE[n][column]]
    refused = [n for n in TABLE if not TABLE[n][column]]
    assert len(have) >= 10
    # every listed name in ONE program (a name the prelude or the device library lacks for this type fails the whole compile, and the log names it);
    # then each alone where the sum did not compile, to say which
    whole = " + ".join(f"({_expression(n)})" for n in have)
    if lib.jh_bcast_check(whole.encode(), code, 2, 0) != 0:
        bad = [n for n in have if lib.jh_bcast_check(_expression(n).encode(), code, 2, 0) != 0]
        raise AssertionError(f"{column}: {bad or whole} does not compile: {lib.jh_last_error()[:600]}")
    for name in refused:
        expr = _expression(name)
        with pytest.raises(J.JetsHipError) as ei:
            check(lib.jh_bcast_check(expr.encode(), code, 2, 0))
        assert f"`{expr}`" in str(ei.value) and "error" in str(ei.value), (name, str(ei.value)[:300])
    # the Julia binding's targets, as _emit prints them
    for jname, cname in _julia_cfun().items():
        expr = OPERATORS[cname] if cname in OPERATORS else f"{cname}(x0, x1)" if jname in ("max", "min") else f"{cname}(x0)"
        table_name = {"max": "maximum", "min": "minimum"}.get(jname, jname)
        rc = lib.jh_bcast_check(expr.encode(), code, 2, 0)
        assert (rc == 0) == TABLE[table_name][column], (jname, column, lib.jh_last_error()[:300])


def test_max_min_take_scalars_literals_and_wide_scalars():
    """jl_max / jl_min where fmax / fmin were used: against a scalar parameter, an integer or floating literal, and a Float64 scalar of a Float32
    program (the wider type's result, like every mixed operation of the prelude)."""
    from jets_jl_amd._ffi import lib

    for code in (0, 1):
        assert lib.jh_bcast_check(b"jl_max(x0, s0) + jl_min(x0, 0) + jl_max(0.5, x0) + jl_min(jl_max(x0, -1), 1)", code, 1, 1) == 0, lib.jh_last_error()
    assert lib.jh_bcast_check_typed(b"jl_max(x0, s0) * jl_min(s0, x0)", 0, 1, 0, 1, 1) == 0, lib.jh_last_error()
