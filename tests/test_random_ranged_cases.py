"""CPU: what the seed list of tests/test_gpu_random_ranged.py covers, checked with no device (tools/fuzz_ranged.py: draw is pure numpy).

Every tiling is legal for its entry point and tiles the block; every combination the sweep exists for occurs in every family that has it
(grid_chain_step is the whole-vector step: no ranges, no deferred norm; tall_apply_range has no step: no beta; only the chain applications take
`accumulate`; only grids have K and the regularised layout); at least a quarter of all cases span several workgroups and end in a partial pack;
and the reference agrees with itself: the oracle's results assembled range by range, through the masks the GPU checks use, are the bits of its
whole-vector results."""
import numpy as np
import pytest

from .helpers import assert_bits_equal, load_tool

fr = load_tool("fuzz_ranged")

CASES = fr.suite_cases()
BY_FAMILY = {f: [c for c in CASES if c["family"] == f] for f in fr.FAMILIES}


def _ascending(r):
    return all(r[i][0] + r[i][1] <= r[i + 1][0] for i in range(len(r) - 1))


def test_the_seed_list_is_the_one_the_gpu_test_uses():
    from . import test_gpu_random_ranged as gpu

    assert [fr.case_id(c) for c in gpu.CASES] == [fr.case_id(c) for c in CASES]
    assert len({fr.case_id(c) for c in CASES}) == len(CASES) == len(fr.FAMILIES) * len(fr.SUITE_SEEDS)
    assert len(fr.SUITE_SEEDS) >= 40
    for c in CASES:                                                            # a case is a function of (family, seed) alone: nothing is redrawn
        assert fr.draw(c["family"], c["seed"]) == c


def test_case_sizes_stay_small():
    for c in CASES:
        many = c["seed"] >= fr.MANY_BASE
        assert c["K"] <= 4 and (c["n"] <= 600 and c["N"] in fr.MANY_ROWS and c["adj_split"] == -1 if many else c["n"] <= 6000 and c["N"] <= 40)
        assert c["N"] in fr.MANY_ROWS + fr.NSET and c["n"] >= fr.pack_elems(c["dtype"])


@pytest.mark.parametrize("case", CASES, ids=[fr.case_id(c) for c in CASES])
def test_every_tiling_is_legal_and_tiles_the_block(case):
    n, p = case["n"], fr.pack_elems(case["dtype"])
    assert 1 <= len(case["ranges"]) <= 7
    covered = np.zeros(n, dtype=int)
    for lo, cnt in case["ranges"]:
        assert lo % p == 0 and 0 <= lo and cnt >= 0 and lo + cnt <= n, "starts on the 16-byte grid, inside the block"
        assert cnt % p == 0 or lo + cnt == n, "counts are on the grid, or the range ends the block"
        assert lo < n, "a position inside the block"
        covered[lo:lo + cnt] += 1
    assert (covered == 1).all(), "the union is [0, n) with no overlap"
    for toks in (case["fwd"], case["adj"], case["nrm"]):
        side = [t for t in toks if t not in ("A", "At") and t[0] != "M"]
        assert len(side) <= 4, "R and R^H fit the four range-side stages"


@pytest.mark.parametrize("family", fr.FAMILIES)
def test_every_combination_occurs_in_every_family(family):
    cases = BY_FAMILY[family]
    grid, ranged, step, acc = family.startswith("grid"), fr.has_ranges(family), fr.has_step(family), fr.has_apply(family)

    def some(pred, what):
        assert any(pred(c) for c in cases), f"{family}: no case with {what}"

    pk = lambda c: fr.pack_elems(c["dtype"])
    for dt in fr.DTYPES:
        some(lambda c: c["dtype"] == dt, dt)
    for K in ((2, 3, 4) if grid else (1,)):
        some(lambda c: c["K"] == K, f"K = {K}")
    some(lambda c: c["n"] % pk(c) == 0 and pk(c) > 1, "n on the 16-byte grid")
    some(lambda c: c["n"] % pk(c) != 0, "n off the 16-byte grid")
    some(lambda c: c["n"] in [fr.WG_LANES * pk(c) * k for k in (1, 2, 3)], "n a workgroup multiple")
    some(lambda c: c["n"] > fr.WG_LANES * pk(c) and c["n"] % pk(c) != 0, "several workgroups ending in a partial pack")
    for kinds in ("plain", "mixed") + (("regularised",) if grid else ()):
        some(lambda c: c["kinds"] == kinds, f"{kinds} kinds")
    some(lambda c: c["adj_split"] == 0, "the ordered walk")
    some(lambda c: c["adj_split"] > 0 and (fr.expected_parts(c, c["n"]) or 0) > 1, "forced parts that really split the rows")
    some(lambda c: c["adj_split"] > 0 and c["N"] >= 4 and c["N"] % fr.rows_in_flight(c) != 0, "forced parts with N no multiple of the rows in flight")
    some(lambda c: c["adj_split"] > 0 and c["N"] >= 4 and -(-c["N"] // min(c["adj_split"], c["N"] // 2)) % fr.rows_in_flight(c) != 0,
         "forced parts whose length is no multiple of the rows in flight")
    some(lambda c: c["adj_split"] == -1 and c["N"] in fr.MANY_ROWS, "many rows at the launcher's own adj_split")
    if family != "grid_range":
        some(lambda c: any(t[0] == "W" and t[2] for t in c["fwd"] if t != "A"), "a conjugated weight")
        some(lambda c: sum(t[0] in ("W", "Wb") for t in c["fwd"] if t != "A") == 2, "two range-side weights")
        some(lambda c: sum(t[0] in ("W", "Wb") for t in c["fwd"] if t != "A") == 0, "no range-side weight")
        some(lambda c: any(t[0] == "Wb" for t in c["fwd"] if t != "A"), "the block-diagonal weight operator")
        some(lambda c: any(t[0] == "s" for t in c["fwd"] if t != "A"), "a scalar stage")
        some(lambda c: any(t[0] == "M" for t in c["fwd"] if t != "A"), "a domain-side diagonal")
    if ranged:
        some(lambda c: any(cnt == 0 for _, cnt in c["ranges"]), "an empty range")
        some(lambda c: any(cnt == pk(c) for _, cnt in c["ranges"]), "a one-pack range")
        some(lambda c: any(0 < cnt < pk(c) and lo + cnt == c["n"] for lo, cnt in c["ranges"]), "a final range shorter than one pack")
        some(lambda c: not _ascending(c["ranges"]), "ranges applied out of order")
        some(lambda c: len(c["ranges"]) >= 5, "five ranges or more")
        some(lambda c: len(c["ranges"]) == 1, "one range")
        some(lambda c: any(cnt > fr.WG_LANES * pk(c) and (lo + cnt) % pk(c) != 0 for lo, cnt in c["ranges"]),
             "ONE range of several workgroups that ends in a partial pack")
    if step:
        some(lambda c: c["beta"] == 0, "beta = 0")
        some(lambda c: c["beta"] != 0, "beta != 0")
    if step and ranged:
        some(lambda c: c["deferred"], "deferred ||u||^2")
        some(lambda c: not c["deferred"], "shares of ||u||^2 read back")
    if acc:
        for a in fr.ACCS:
            some(lambda c: c["acc"] == a, f"accumulate {a}")


def test_a_quarter_of_the_cases_span_workgroups_and_end_in_a_partial_pack():
    hit = [c for c in CASES if c["n"] > fr.WG_LANES * fr.pack_elems(c["dtype"]) and c["n"] % fr.pack_elems(c["dtype"]) != 0]
    assert 4 * len(hit) >= len(CASES), f"{len(hit)} of {len(CASES)}"


def test_expected_parts_is_the_launchers_rule():
    case = dict(adj_split=3, N=7, dtype="float32")
    assert fr.expected_parts(case, 8) == 3 and fr.expected_parts(case, 3) == 1                 # rows 3 + 3 + 1; a range shorter than one pack: one part
    assert fr.expected_parts(dict(adj_split=5, N=7, dtype="float64"), 2) == 3                  # min(5, 7 // 2) = 3 parts of 3 + 3 + 1 rows
    assert fr.expected_parts(dict(adj_split=5, N=13, dtype="float64"), 2) == 5                 # 3 rows per part: 3 + 3 + 3 + 3 + 1
    assert fr.expected_parts(dict(adj_split=2, N=3, dtype="float64"), 64) == 1                 # fewer than four rows: ordered
    assert fr.expected_parts(dict(adj_split=0, N=40, dtype="float64"), 64) == 1
    assert fr.expected_parts(dict(adj_split=-1, N=300, dtype="float64"), 64) is None


TEN = [c for f in fr.FAMILIES for c in BY_FAMILY[f][:9] + BY_FAMILY[f][-1:]]


@pytest.mark.parametrize("case", TEN, ids=[fr.case_id(c) for c in TEN])
def test_the_reference_assembled_range_by_range_is_the_whole_vector_reference(oracle, case):
    whole, parts = fr.reference_by_ranges(oracle, case)
    assert set(whole) == {"adj", "nrm", "u", "w"}
    for name in whole:
        assert not np.isnan(whole[name].view(whole[name].real.dtype)).any(), f"{name}: the oracle's result is finite (a NaN of the u found must not be read)"
        assert_bits_equal(parts[name], whole[name], f"{fr.case_id(case)}: {name}")
