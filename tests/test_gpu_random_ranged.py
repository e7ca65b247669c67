"""GPU: a seeded random differential of the ranged calls and the one-pass Golub-Kahan steps on tall chains, bare N x K grids and grid chains
(jh_chain_bidiag_step_range, jh_chain_apply_range, jh_blockop_{mul_adj,normal_mul,bidiag_step}_range, jh_chain_bidiag_step through a grid) against
the CPU oracle's stage-by-stage loops -- never against a whole-vector device call.

tools/fuzz_ranged.py draws the cases (element type, K, N on both sides of the rows-in-flight multiples, block lengths that span several workgroups
and end in a partial pack, plain / mixed / regularised kinds, stage lists, the ordered walk, forced parts and the launcher's own parts on many
rows, 1 .. 7 ranges with empty, one-pack and partial-pack ranges applied in a random order, alpha, beta = 0 over an all-NaN u, shares of ||u||^2
read back or deferred, every `accumulate`) and runs them: after every ranged call the ranges done so far hold the oracle's bits and everything else
the bits it held before; where the rows are summed in parts the output is within the bound the family's own split-walk test asserts
(tools/check_specials.py: _chain_tol, _allclose_ok, _relerr_ok), u stays bit-exact and two runs agree to the bit.

The id names family, seed, element type, N x K x n, kinds, walk, the number of ranges (p: applied out of order, e: an empty range), beta and
accumulate; tools/fuzz_ranged.py: draw(family, seed) rebuilds the case.  tests/test_random_ranged_cases.py checks what this list covers."""
import pytest

from .helpers import assert_bits_equal, load_tool

pytestmark = pytest.mark.gpu

fr = load_tool("fuzz_ranged")

CASES = fr.suite_cases()


@pytest.mark.parametrize("case", CASES, ids=[fr.case_id(c) for c in CASES])
def test_ranged_calls_and_steps_against_the_oracle(Jets, oracle, case):
    cid = fr.case_id(case)
    count = 0
    records = fr.run_case(Jets, oracle, case)
    try:
        for rec in records:
            count += 1
            if rec[0] == "same":
                assert_bits_equal(rec[2], rec[3], f"{cid}: {rec[1]}")
            else:
                assert rec[2] is True, f"{cid}: {rec[1]}: {rec[2]}"
    finally:
        records.close()          # a case yields while its knobs are set and resets them in its own finally: run that now, not when the traceback dies
    assert count > 0, f"{cid}: no check ran"
