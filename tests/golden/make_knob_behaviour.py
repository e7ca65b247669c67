#!/usr/bin/env python3
"""What jh_tune_get / jh_tune_set answer for every name and a sweep of values (tests/golden/knob_behaviour.json).

    python tests/golden/make_knob_behaviour.py              # rewrites knob_behaviour.json next to this script
    python tests/golden/make_knob_behaviour.py --stdout     # prints the same record of the library as built, writes nothing

Both calls work before jh_init: they then act on the never-ready dummy context, so the sweep needs no device and this process never
opens one.  Per name the record holds the status and value of a first jh_tune_get (the default) and, for every probe value in order,
the status of jh_tune_set and the value jh_tune_get returns afterwards; the text of jh_last_error() after a refusal is kept once per
name (a name has one message).  The probe values straddle every bound a check uses.

tests/test_knob_table.py replays the sweep against the library as built (in a child process: "slab_cache" and its kin are process-wide)
and compares it with the committed record, so the record is regenerated only when a knob is added or its rule changes ON PURPOSE: add
the row to jets.jl_amd/csrc/jh_knobs.def and the name to NAMES, build, run this script, and read the diff of the json.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "knob_behaviour.json")
LIB = os.environ.get("JETSHIP_LIB", os.path.join(ROOT, "jets.jl_amd", "libjetship.so"))

NAMES = (
    "fwd_group", "fwd_unroll", "fwd_wg", "adj_unroll", "adj_depth", "adj_wg", "fwd_order", "nt", "nt_resident_mib", "slab_cache",
    "slab_cached_mib", "bcast_item_fast", "adj_split", "last_adj_parts", "adj_rows_per_launch", "autotune", "graphs", "small_loop",
    "force_dist", "step_chain", "step_band", "step_chunk", "last_step_chain", "general_xcd", "graph_replays", "last_fwd_rows_per_wg",
    "last_adj_launches", "lsqr_graph", "last_lsqr_graph", "grid_diag", "grid_tile", "sum_group", "bcast_band", "general_band",
    "fwd_ctiles", "sum_adj_group", "general_tile", "general_list", "dense_list", "small_loop_max_kib", "dense_list_split",
    "dense_direct", "dense_grid", "dense_list_shared", "dense_combine", "dense_list_rl_min", "dense_list_cpw", "last_dense_rl",
    "last_general_list", "dense_mixed", "dense_fused", "cgls_trace", "cg_dev", "walk_memory", "alloc_role", "slab_free_floor_mib",
    "slab_probed", "last_alloc_choice", "last_cg_graph", "last_cgls_overlaps", "dense_gw", "dense_fwd_wgs", "last_dense_fused",
    "last_launches", "tall_unaligned", "red_blocks_wave", "adj_bare_chain", "adj_thin_mixed", "grid_normal", "grid_chain",
    "last_grid_chain_shape", "grid_step", "last_grid_step_shape", "grid_chain_step", "last_grid_chain_step_shape", "grid_range",
    "last_grid_range_shape", "grid_chain_range", "last_grid_chain_range_shape", "fwd_anchor", "ua_nt", "tall_f", "wide_twin", "red_wgs",
    "last_fwd_walk",
)
PROBES = (-3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 32, 64, 255, 256, 300, 512, 1024, 2048, 4096, 4097, 65535, 65536, 65537,
          2**20, 2**20 + 1, 2**24 - 1, 2**24, 2**40)
UNSET = -(2**62)          # what the value slot holds before a jh_tune_get: a refused get leaves it there


def sweep(lib_path: str = LIB) -> dict:
    lib = C.CDLL(lib_path)
    lib.jh_tune_set.argtypes, lib.jh_tune_set.restype = [C.c_char_p, C.c_int64], C.c_int
    lib.jh_tune_get.argtypes, lib.jh_tune_get.restype = [C.c_char_p, C.POINTER(C.c_int64)], C.c_int
    lib.jh_last_error.argtypes, lib.jh_last_error.restype = [], C.c_char_p

    def get(name):
        v = C.c_int64(UNSET)
        return [lib.jh_tune_get(name.encode(), C.byref(v)), v.value]

    knobs = {}
    for name in NAMES:
        default, status, value, messages = get(name), [], [], []
        for p in PROBES:
            st = lib.jh_tune_set(name.encode(), p)
            if st != 0:
                msg = lib.jh_last_error().decode()
                if msg not in messages:
                    messages.append(msg)
            status.append(st)
            value.append(get(name)[1])
        assert len(messages) <= 1, (name, messages)        # one message per name: the record keeps it once
        knobs[name] = {"default": default, "message": messages[0] if messages else None, "set_status": status, "value_after": value}
    return {"probes": list(PROBES), "knobs": knobs}


def dumps(record: dict) -> str:
    rows = ",\n".join(f"  {json.dumps(n)}: {json.dumps(k)}" for n, k in record["knobs"].items())
    return f'{{"probes": {json.dumps(record["probes"])},\n "knobs": {{\n{rows}\n }}}}\n'


if __name__ == "__main__":
    if sys.argv[1:] not in ([], ["--stdout"]):
        raise SystemExit(__doc__)
    text = dumps(sweep())
    if sys.argv[1:]:
        sys.stdout.write(text)
    else:
        with open(OUT, "w", encoding="utf-8") as f:
            f.write(text)
        print(f"{len(NAMES)} names x {len(PROBES)} values -> {OUT}")
