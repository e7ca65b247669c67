"""GPU: the launch plans and the output bits of the one-pass grid kernels and the fused chains are the recorded ones.

tests/golden/grid_launch_record.json (tests/golden/make_grid_launch_record.py) holds, for a covering list of small calls -- A'A, the ranged
adjoint and the Golub-Kahan step of an N x K grid, the ADJOINT / NORMAL / FORWARD chains and the chain step through a grid and through a tall
operator; 5 and 600 rows of 515 elements, every element type, K = 2 .. 4, adj_split -1 / 0 / 3, nontemporal accesses forced on and off,
whole vectors and three ranges --, the launch counters each call wrote and a hash of every vector it wrote, as the library answered
before the launchers were given one split-walk plan.  The replay requires EQUALITY of every counter and every hash: the part count, the
kernel instantiation and the fold order of a call are part of its result (the split walk is deterministic, not the ordered sum's bits).
The automatic split (adj_split = -1) depends on the device's CU count, which the record holds: on a device with another count those cases
are not compared; on the recorded device (an MI355X) every case is."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_grid_launch_record", os.path.join(GOLDEN, "make_grid_launch_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _params(case):
    return {k: v for k, v in case.items() if k not in ("counters", "hashes")}


def test_every_call_launches_and_writes_what_the_record_holds(Jets):
    gen = _generator()
    with open(os.path.join(GOLDEN, "grid_launch_record.json"), encoding="utf-8") as f:
        record = json.load(f)
    params = [_params(c) for c in record["cases"]]
    assert params == gen.cases() and len(params) >= 200, "the recorded cases are the generator's covering list"
    same_device = Jets.device_info()["cu_count"] == record["cu_count"]
    assert same_device or "MI355X" not in Jets.device_info()["name"], "the record was made on an MI355X: nothing is left out there"
    todo = [c for c in record["cases"] if same_device or c["adj_split"] != -1]
    got = gen.replay(Jets, [_params(c) for c in todo])
    wrong = []
    for c, (counters, hashes) in zip(todo, got):
        if counters != c["counters"] or hashes != c["hashes"]:
            wrong.append(f"{_params(c)}: counters {counters}, hashes {hashes}; recorded {c['counters']}, {c['hashes']}")
    assert not wrong, f"{len(wrong)} of {len(todo)} calls differ from the record:\n" + "\n".join(wrong[:20])
    assert len(todo) == len(record["cases"]) or not same_device
