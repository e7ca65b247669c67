"""CPU checks of the knob grid_chain_range (the ranged forms of the chains through N x K grids): the header describes it, the meaning of the range
next to both calls and its counter; the library's default is 0; and the row partition plans no grid chain while the knob reads 0."""
import os
import re

from . import knob_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


def _doc_before(h, decl):
    at = h.index(decl)
    return h[h.rindex("/*", 0, at):at]


def test_header_describes_the_knob_the_counter_and_the_range_of_a_grid_chain():
    h = _read("include", "jetship.h")
    doc = _doc_before(h, "typedef struct jh_chain jh_chain;")
    assert 'GRID CHAIN RANGE (knob "grid_chain_range" = 1; the default is 0' in doc
    assert "positions INSIDE a block" in doc and "JH_ERR_INVALID" in doc and '"last_grid_chain_range_shape"' in doc
    assert '"grid_chain_step"' in doc[doc.index("GRID CHAIN RANGE"):], "the step needs both knobs"
    for decl in ("int jh_chain_apply_range(", "int jh_chain_bidiag_step_range("):
        doc = _doc_before(h, decl)
        assert '"grid_chain_range"' in doc and "POSITIONS INSIDE A BLOCK" in doc and "first_elem + count <= n" in doc, decl
        assert re.search(r"default(s)? (is|are) 0", doc), decl
    assert '"grid_chain_range" (jh_chain_apply_range on an ADJOINT / NORMAL chain' in h and "0 -- the default --" in h     # the knob list


def test_the_default_is_zero_and_the_counter_is_read_only():
    table = knob_table.rows()                                                   # jh_knobs.def: the field, jh_tune_set and jh_tune_get come from the row
    knob = table["grid_chain_range"]
    assert knob.kind == "JH_KNOB" and knob.default == 0                         # set and get
    assert table["last_grid_chain_range_shape"].kind == "JH_COUNTER"            # get only
    assert knob.rule == "value == 0 || value == 1" and knob.message == "grid_chain_range must be 0 or 1"
    abi = _read("jets.jl_amd", "csrc", "jh_tall_chain.hip")
    assert "a grid chain has no ranged form (apply the whole vector)" in abi     # the refusals of knob 0, word for word
    assert "a grid chain has no one-pass step (run the FORWARD chain, then the ADJOINT)" in abi


def test_shard_chains_plan_no_grid_chain_while_the_knob_reads_zero(monkeypatch):
    """_ShardChains with its three runs planned through a grid: whether they exist is the knobs' to say, read per application."""
    import sys

    sys.path.insert(0, ROOT)
    import jets_jl_amd  # noqa: F401
    from jets_jl_amd import chains, device, rowpart

    knobs = {"grid_chain_range": 0, "grid_chain_step": 0}
    asked = []

    def tune_get(name):
        asked.append(name)
        return knobs[name]

    monkeypatch.setattr(device, "tune_get", tune_get)
    sc = object.__new__(rowpart._ShardChains)
    sc._chn, sc.cache = chains, chains.ChainCache()
    sc._adj = sc._nrm = sc._fwd = [object()]
    sc._has_adj = sc._has_normal = sc._has_step = True
    made = []
    monkeypatch.setattr(chains, "one_run", lambda stages, cache, tag, ctype, make=True, grid=True: made.append((tag, grid)) or "handle")
    # a run through a grid of blocks of 64 elements
    sc.grid_n = 64
    assert not sc.has_adj and not sc.has_normal and not sc.has_step
    assert sc.adjoint() is None and sc.normal() is None and sc.step() is None and not made, "knob 0: no grid chain is planned or built"
    assert "grid_chain_range" in asked
    knobs["grid_chain_range"] = 1
    assert sc.has_adj and sc.has_normal and not sc.has_step, "the step needs grid_chain_step = 1 as well"
    assert sc.adjoint() == "handle" and sc.normal() == "handle" and sc.step() is None
    knobs["grid_chain_step"] = 1
    assert sc.has_step and sc.step() == "handle"
    assert made == [("rowpart_adj", True), ("rowpart_normal", True), ("rowpart_fwd", True)]
    knobs["grid_chain_range"] = 0                                                # back at 0 under a live shard: read per application
    assert not sc.has_adj and not sc.has_normal and not sc.has_step and sc.step() is None
    sc.has_step = False                                                          # a library decline is for good
    knobs["grid_chain_range"] = 1
    assert not sc.has_step and sc.has_adj
    # a tall run never consults the knobs
    sc.grid_n, sc._has_step = None, True
    del asked[:], made[:]
    assert sc.has_adj and sc.has_normal and sc.has_step and sc.step() == "handle" and not asked
    assert made == [("rowpart_fwd", False)]


def test_a_shard_reads_the_knob_per_application_for_its_normal_operator(monkeypatch):
    """RowPartitionedOp.fused_normal follows the knob after the shard was built, in both directions: a shard built under knob 0 gains the ranged
    NORMAL grid chain when the knob goes to 1, and one built under knob 1 loses every chain route when it goes back to 0 (fused_normal_mul_ then
    returns False with nothing called: the solvers apply A and A' through a range vector, as without the feature)."""
    import sys

    sys.path.insert(0, ROOT)
    import jets_jl_amd  # noqa: F401
    from jets_jl_amd import chains, device, rowpart

    knobs = {"grid_chain_range": 0, "grid_chain_step": 0}
    monkeypatch.setattr(device, "tune_get", lambda name: knobs[name])
    sc = object.__new__(rowpart._ShardChains)
    sc._chn, sc.cache, sc.grid_n = chains, chains.ChainCache(), 64
    sc._has_adj = sc._has_normal = sc._has_step = True
    calls = []

    class OneRank:
        world = 1

        def all_reduce_sum_(self, x, force=False):
            calls.append("all_reduce")
            return x

    shard = rowpart.RowPartitionedOp(None, "L", OneRank(), None, None, None, None, pipelined_normal=lambda y, A, m: calls.append("pipelined") or True,
                                     pipelined_step=lambda *a: 1.0, local_normal=lambda y, A, m: calls.append("local"), chains=sc)
    assert not shard.fused_normal and not shard.chain_step                      # built under knob 0
    assert shard.fused_normal_mul_("y", "m", force_collective=True) is True and calls == ["pipelined"]   # (the route itself consults the knob: stubbed here)
    del calls[:]
    assert shard.fused_normal_mul_("y", "m") is False and not calls, "knob 0, no exchange: neither the local NORMAL chain nor an all-reduce"
    knobs["grid_chain_range"] = knobs["grid_chain_step"] = 1                    # turned on afterwards
    assert shard.fused_normal and shard.chain_step
    assert shard.fused_normal_mul_("y", "m") is True and calls == ["local", "all_reduce"]
    del calls[:]
    knobs["grid_chain_range"] = 0                                                # and back
    assert not shard.fused_normal and not shard.chain_step
    assert shard.fused_normal_mul_("y", "m") is False and not calls


def test_a_team_of_mixed_members_has_no_ranged_chain_routes():
    import sys

    sys.path.insert(0, ROOT)
    from jets_jl_amd import rowpart

    class SC:
        has_adj = has_normal = has_step = True

        def __init__(self, n):
            self.grid_n = n

    T = object.__new__(rowpart.TeamOp)
    for lens, mixed in (((None, None), False), ((64, 64), False), ((64, None), True), ((64, 128), True)):
        T._chains = [SC(n) for n in lens]
        clens = {sc.grid_n for sc in T._chains}
        T._chain_grids, T._chain_grids_mixed = clens != {None}, clens != {None} and len(clens) > 1
        assert T._chain_grids_mixed == mixed
        if mixed:
            assert not T.chain_step and not T.fused_normal and T._team_chain_grid_n() is None
    T._chains = [SC(None), SC(None)]
    T._chain_grids = T._chain_grids_mixed = False
    assert T.chain_step and T.fused_normal                                      # tall weighted members: as before, no knob read


def test_the_knob_is_read_in_one_place_on_the_host():
    src = _read("jets.jl_amd", "rowpart.py")
    assert src.count('tune_get("grid_chain_range")') == 1 and "grid_n=h.block_len" in src
    assert 'tune_get("grid_chain_range")' not in _read("jets.jl_amd", "chains.py")
