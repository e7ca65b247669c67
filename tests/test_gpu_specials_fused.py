"""GPU: IEEE special values (signed zeros, infinities, NaN, denormals, the largest finite values) through the kernel families written after
tools/check_specials.py's first version: the fused tall chains (jh_chain_apply, jh_chain_apply_range, accumulate 0 / +-1 / +-2), the chain
Golub-Kahan step, the fused A'A of N x K grids, the grid chains, the grid step, the per-block reductions and the split walk.

Two kinds of input (tools/check_specials.py): "mix" -- 30 % of the scalars of every coefficient, weight, diagonal and vector drawn from
+-0, +-Inf, NaN, denormals, +-max, tiny, +-1, eps -- and seam poison: finite U[0,1) data with NaN, +Inf and -0 at the scalars where lanes overlap
or idle (the pack an idle lane re-loads, the overlap of a row's partial last pack, workgroup tile edges, row ends inside a slab, the scalars
just outside a range, the first and last row of a part of the split walk).  Every operator is elementwise, so the CPU oracle's stage-by-stage
loops (block_df, block_df_adj, child_mul, barr_lincomb through the rigs of the chain tests) say exactly which outputs may be non-finite: the
comparison is helpers.assert_same_values, bit for bit except a NaN's payload.  The reductions (||u||^2 of the steps, block norms and dots)
are NaN if an owned scalar is NaN, else Inf if one is Inf, else the fp64 sum to the tolerance the project asserts for that quantity elsewhere
(1e-12 for ||u||^2, 1e-5 / 1e-12 for the block reductions); the split walk sums in another order, so there the pool has no +-max and the
case itself is checked to be independent of the row order (the oracle with the rows reversed).  Its two inputs -- a mix so sparse that sums over
hundreds of rows keep finite scalars, and every special value in columns of its own in the first and last row of every part (a sum of +Inf
partials, Inf - Inf across parts) -- must each leave some tens of finite, infinite and NaN scalars in the oracle's result, or the case fails
as vacuous.  The +Inf-only classes of the steps assert that the expected ||u||^2 is Inf, so that they cannot silently turn into NaN cases.

jh_chain_apply_range takes ranges that start on the 16-byte grid; the two ranges of a case start on it but on no workgroup tile, and the
second ends with the vector, inside a pack when the block length is off the grid.

The id of a case names family, chain or variant, element type and input class."""
import pytest

from .helpers import assert_same_values, load_tool

pytestmark = pytest.mark.gpu

cs = load_tool("check_specials")

CASES = cs.fused_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_special_values_through_the_fused_families(Jets, oracle, case):
    cid, dt, fn = case
    count = 0
    records = fn(Jets, oracle)
    try:
        for rec in records:
            count += 1
            if rec[0] == "same":
                assert_same_values(rec[2], rec[3], f"{cid}: {rec[1]}")
            else:
                assert rec[2] is True, f"{cid}: {rec[1]}: {rec[2]}"
    finally:
        records.close()          # a case yields while its forced knobs are set and resets them in its own finally: run that now, not when the traceback dies
    assert count > 0, f"{cid}: no check ran"
