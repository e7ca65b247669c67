"""CPU checks of the knob grid_range (the ranged calls on N x K grids, jh_grid_range.hip): the header describes it, its counter and the grid
meaning of the range next to the three calls, and the library's default is 0."""
import os

from . import knob_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


def _doc_before(h, decl):
    at = h.index(decl)
    return h[h.rindex("/*", 0, at):at]


def test_header_describes_the_knob_the_counter_and_the_range_of_a_grid():
    h = _read("include", "jetship.h")
    doc = _doc_before(h, "int jh_blockop_mul_adj_range(")
    assert "GRID RANGE" in doc and '"grid_range" = 1' in doc and "the default is 0" in doc
    assert "positions INSIDE a block" in doc and "JH_ERR_INVALID" in doc and '"last_grid_range_shape"' in doc
    for decl in ("int jh_blockop_normal_mul_range(", "int jh_blockop_bidiag_step_range("):
        doc = _doc_before(h, decl)
        assert '"grid_range"' in doc and "positions inside a block" in doc, decl
    assert '"grid_range" (jh_blockop_mul_adj_range, jh_blockop_normal_mul_range and jh_blockop_bidiag_step_range on N x (2 .. 4) grids' in h   # the knob list
    assert '"last_grid_range_shape" (how the latest ranged grid call was launched' in h                                                  # the counter list


def test_the_default_is_zero_and_the_counter_is_read_only():
    table = knob_table.rows()                                                   # jh_knobs.def: the field, jh_tune_set and jh_tune_get come from the row
    knob = table["grid_range"]
    assert knob.kind == "JH_KNOB" and knob.default == 0                         # set and get
    assert table["last_grid_range_shape"].kind == "JH_COUNTER"                  # get only
    assert knob.rule == "value == 0 || value == 1" and knob.message == "grid_range must be 0 or 1"
    assert "jh_grid_range.hip" in _read("jets.jl_amd", "csrc", "Makefile")


def test_host_mirror_consults_the_knob():
    src = _read("jets.jl_amd", "rowpart.py")
    assert 'tune_get("grid_range") == 1' in src and '"grid_range_calls"' in src
    assert '"grid_range_calls": 0' in _read("jets.jl_amd", "chains.py")
