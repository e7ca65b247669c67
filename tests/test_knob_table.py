"""The context's knobs are one table (jets.jl_amd/csrc/jh_knobs.def) from which the fields of jh_context and the bodies of jh_tune_set /
jh_tune_get are generated.  tests/golden/knob_behaviour.json records what every name answered before the table existed -- its default and,
for a sweep of values on both sides of every bound, whether jh_tune_set took the value, its message when it did not, and what jh_tune_get
read afterwards.  Neither call needs a device (before jh_init they act on the never-ready dummy context), so the record is replayed here
against the library as built, and the table is held level with it."""
import json
import os
import re
import subprocess
import sys

from . import knob_table

ROOT = knob_table.ROOT
GENERATOR = os.path.join(ROOT, "tests", "golden", "make_knob_behaviour.py")
HOWTO = ("a knob is one row of jets.jl_amd/csrc/jh_knobs.def plus its name in NAMES of tests/golden/make_knob_behaviour.py: after adding or changing one "
         "ON PURPOSE, build and run `python tests/golden/make_knob_behaviour.py` to regenerate tests/golden/knob_behaviour.json")


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "knob_behaviour.json"), encoding="utf-8") as f:
        return json.load(f)


def test_the_library_answers_every_name_and_value_as_recorded():
    """The sweep in a fresh child process that never opens a device: "slab_cache" and its kin are process-wide, the dummy context is static."""
    child = subprocess.run([sys.executable, GENERATOR, "--stdout"], capture_output=True, text=True, timeout=60)
    assert child.returncode == 0, child.stderr
    now, then = json.loads(child.stdout), _fixture()
    assert now["probes"] == then["probes"] and len(then["probes"]) >= 32
    assert list(now["knobs"]) == list(then["knobs"]) and len(then["knobs"]) == 85, HOWTO
    for name, rec in then["knobs"].items():
        got = now["knobs"][name]
        assert got["default"] == rec["default"], f"{name}: first jh_tune_get (status, value) {got['default']}, recorded {rec['default']}. {HOWTO}"
        assert got["message"] == rec["message"], f"{name}: refusal {got['message']!r}, recorded {rec['message']!r}. {HOWTO}"
        for k, p in enumerate(then["probes"]):
            assert got["set_status"][k] == rec["set_status"][k], f"jh_tune_set({name!r}, {p}) returned {got['set_status'][k]}, recorded {rec['set_status'][k]}. {HOWTO}"
            assert got["value_after"][k] == rec["value_after"][k], f"after jh_tune_set({name!r}, {p}) jh_tune_get read {got['value_after'][k]}, recorded {rec['value_after'][k]}. {HOWTO}"
        assert len(got["set_status"]) == len(got["value_after"]) == len(then["probes"])


def test_the_table_is_level_with_the_record():
    table, rec = knob_table.rows(), _fixture()["knobs"]
    wide_rw, wide_ro = knob_table.PROCESS_WIDE_SETTABLE, knob_table.PROCESS_WIDE_READ_ONLY
    assert sorted(rec) == sorted(list(table) + list(wide_rw) + list(wide_ro)), f"the recorded names are the table's rows and the five process-wide names. {HOWTO}"
    refuses_every_set = sorted(n for n, r in rec.items() if all(r["set_status"]))
    assert refuses_every_set == sorted(knob_table.counters(table) + list(wide_ro)), f"read-only names are the JH_COUNTER rows and {wide_ro}. {HOWTO}"
    assert all(rec[n]["message"] == f"jh_tune_set: unknown knob '{n}'" for n in refuses_every_set)
    for name, row in table.items():
        assert rec[name]["default"] == [0, row.default], f"{name}: the row's default {row.default}, recorded (status, value) {rec[name]['default']}. {HOWTO}"
        assert rec[name]["message"] == (row.message if row.kind == "JH_KNOB" else f"jh_tune_set: unknown knob '{name}'" if row.kind == "JH_COUNTER" else None), name
    assert len(knob_table.settable(table)) + len(wide_rw) == 64 and len(rec) == 85 and len(refuses_every_set) == 21
    # nothing but the five process-wide names is compared by hand in jh_tune_set / jh_tune_get; the fields exist only through the table
    with open(os.path.join(ROOT, "jets.jl_amd", "csrc", "jh_core.hip"), encoding="utf-8") as f:
        core = f.read()
    by_hand = re.findall(r'strcmp\(name, "([a-z_0-9]+)"\)', core)
    assert sorted(by_hand) == sorted(list(wide_rw) * 2 + list(wide_ro)), by_hand
    assert core.count('#include "jh_knobs.def"') == 2
    with open(os.path.join(ROOT, "jets.jl_amd", "csrc", "jh_internal.h"), encoding="utf-8") as f:
        internal = f.read()
    assert internal.count('#include "jh_knobs.def"') == 1 and not [n for n in table if re.search(rf"\bint64_t {n}\b", internal)]
