"""jets.jl_amd/csrc/jh_knobs.def read as data: the one place a context knob is written down (its name, default, rule for jh_tune_set,
message and meaning), for the static tests that used to look for a knob's field in jh_internal.h and its branches in jh_core.hip."""
from __future__ import annotations

import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEF = os.path.join(ROOT, "jets.jl_amd", "csrc", "jh_knobs.def")

# not fields of a context: explicit branches of jh_tune_set / jh_tune_get next to the table lookup (jh_core.hip)
PROCESS_WIDE_SETTABLE = ("slab_cache", "slab_free_floor_mib")
PROCESS_WIDE_READ_ONLY = ("slab_cached_mib", "slab_probed", "last_alloc_choice")

# kind: JH_KNOB (rule = the check, message = its refusal), JH_KNOB_MAP (rule = the stored expression, never refused), JH_COUNTER (read-only)
Row = collections.namedtuple("Row", "kind name default rule message meaning")
_ROW = re.compile(r"^(JH_KNOB|JH_KNOB_MAP|JH_COUNTER)\((\w+), (-?\d+)(?:, (.*?))?\)\s+// (.+)$")
_CHECK = re.compile(r'^(.*), "((?:[^"\\]|\\.)*)"$')


def rows(path=DEF):
    """{name: Row} in the file's order; a line that starts like a row and is none raises."""
    out = {}
    with open(path, encoding="utf-8") as f:
        for line in f:
            if not line.startswith("JH_"):
                continue
            m = _ROW.match(line.rstrip())
            assert m, f"jh_knobs.def: not a row: {line!r}"
            kind, name, default, rest, meaning = m.groups()
            rule = message = None
            if kind == "JH_KNOB":
                rule, message = _CHECK.match(rest).groups()
            elif kind == "JH_KNOB_MAP":
                rule = rest
            assert (rest is None) == (kind == "JH_COUNTER") and name not in out, line
            out[name] = Row(kind, name, int(default), rule, message, meaning)
    return out


def settable(table=None):
    return [r.name for r in (table or rows()).values() if r.kind != "JH_COUNTER"]


def counters(table=None):
    return [r.name for r in (table or rows()).values() if r.kind == "JH_COUNTER"]
