"""GPU: the native LSQR / CGLS / CGNR loops answer what the record holds, bit for bit.

tests/golden/solver_record.json (tests/golden/make_solver_record.py) holds, for every solver on every path of jh_lsqr.hip -- the host-driven loop,
the graph-replayed device loop, the ranged pipelined exchange through `_partitioned` with a one-rank communicator, a team of two contexts through
`_team`, a FORWARD tall chain through `_chain` and an N x 2 grid --, on 3 and 5 rows of 515 elements and 3 rows of 49 667 (four exchange ranges, the
last of 515 elements), in every element type, damped and not, cold and warm, 3 and 20 iterations, an early stop, b = 0 and forced runs into the
istop = 6 exits: istop, itn, the six norms as hex floats, hashes of the history, of x and of the overwritten right-hand side, and the graph
read-outs, as the library answered before the three loops were given one shard scaffold and one Paige-Saunders recurrence.  The replay requires
EQUALITY of all of it, and of the status and message of every recorded refusal, which must leave its vectors alone.  A case that two runs of the
recording library did not answer alike is named in the record and not compared; at most 5 % may be."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_solver_record", os.path.join(GOLDEN, "make_solver_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_solve_and_refusal_answers_what_the_record_holds(Jets):
    gen = _generator()
    with open(os.path.join(GOLDEN, "solver_record.json"), encoding="utf-8") as f:
        record = json.load(f)
    params, recorded = gen.cases(), record["cases"]
    assert record["cases_digest"] == gen.cases_digest(params) and len(recorded) == len(params) >= 200, "the recorded cases are the generator's list"
    assert record["result"] == gen.RESULT
    skip = set(record["nondeterministic"])
    assert 20 * len(skip) <= len(params), "at most 5 % of the cases may be left out of the comparison"
    got, refused = gen.replay(Jets, params)
    got = json.loads(json.dumps(got))
    wrong = [f"{c}: {g}; recorded {r}" for i, (c, g, r) in enumerate(zip(params, got, recorded)) if i not in skip and g != r]
    assert not wrong, f"{len(wrong)} of {len(params) - len(skip)} solves differ from the record:\n" + "\n".join(wrong[:20])
    assert len(record["refusals"]) == 14 and all(r["unchanged"] for r in record["refusals"])
    assert refused == record["refusals"]
    forced = [(c, r) for c, r in zip(params, recorded) if c["kind"] == "force"]
    assert any(r[0] == 6 and 0 < r[1] < c["maxiter"] for c, r in forced), "a breakdown far past convergence is among the forced runs"
    huge = [r for c, r in forced if c["solver"] == "lsqr" and "scale" in c]
    assert len(huge) == len(gen.PATHS) and all((r[0], r[1]) == (6, 0) for r in huge), "LSQR's non-finite-rho exit and its itn--, on every path"
