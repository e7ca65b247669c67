"""CPU: the C-ABI library loads, exports every symbol include/jetship.h declares, and fails loudly
without a GPU.  No compute calls."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jetship.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char \*)\s*(jh_\w+)\s*\(", text, flags=re.M)))


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    for must in ("jh_init", "jh_last_error", "jh_bvec_create", "jh_getblock_copy", "jh_setblock_copy", "jh_setblock_fill",
                 "jh_fill", "jh_dot", "jh_norm", "jh_extrema", "jh_lincomb", "jh_blockop_create", "jh_blockop_mul",
                 "jh_blockop_mul_adj", "jh_blockop_normal_mul"):
        assert must in syms
    assert len(syms) >= 35


def test_library_exports_every_declared_symbol():
    import jets_jl_amd as J
    from jets_jl_amd._ffi import SYMBOLS

    handle = C.CDLL(J.LIB_PATH)
    declared = declared_symbols()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/jetship.h but not exported by libjetship.so"
    assert sorted(SYMBOLS) == declared, "jets.jl_amd/_ffi.py must bind exactly the symbols the header declares"
    assert handle.jh_abi_version() == 4


def test_library_exports_exactly_the_declared_symbols():
    """Round 6: the library is built with -fvisibility=hidden and a linker version script (csrc/jetship.map) -- its dynamic symbol
    table holds the header's entry points and NOTHING else: no cross-translation-unit helper (round 5 leaked jh_comm_exists, jh_dot_begin, jh_dot_end),
    no C++ template instantiation, no kernel host stub."""
    import subprocess

    import jets_jl_amd as J

    out = subprocess.run(["nm", "-D", "--defined-only", J.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert exported == declared_symbols(), (sorted(set(exported) - set(declared_symbols())), sorted(set(declared_symbols()) - set(exported)))


def test_header_cites_the_reference_for_every_entry_point_group():
    text = open(HEADER).read()
    assert text.count("src/Jets.jl:") >= 25
    for anchor in ("1010-1032", "1034-1057", "834-848", "850-856", "870-878", "880-885", "914", "915", "916", "1112", "530-534"):
        assert anchor in text, f"include/jetship.h should cite src/Jets.jl:{anchor}"


def test_fails_loudly_without_a_gpu():
    import jets_jl_amd as J
    from jets_jl_amd._ffi import lib

    n = C.c_int(-1)
    rc = lib.jh_device_count(C.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible; the no-GPU failure mode is checked on CPU-only boxes")
    with pytest.raises(J.JetsHipError):
        J.init(0)
    h = C.c_void_p()
    lens = (C.c_int64 * 1)(4)
    rc = lib.jh_bvec_create(1, lens, 0, C.byref(h))
    assert rc == 5 and b"jh_init" in lib.jh_last_error()            # JH_ERR_STATE, nothing allocated on the host instead
    with pytest.raises(J.JetsHipError):
        J.zeros(J.JetSpace("float32", 4))


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "jets.jl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert "jets_oracle" not in src and "libjets_oracle" not in src and "from oracle" not in src, f"{f} references the oracle"


def test_every_entry_point_is_mapped_to_the_reference_in_integration_md():
    """INTEGRATION.md section 2 maps the ABI onto the reference: no entry point of include/jetship.h may be missing from it
    (grouped spellings like `jh_event_create/record/elapsed_ms/destroy` count)."""
    import re

    header = open(os.path.join(ROOT, "include", "jetship.h")).read()
    names = sorted(set(re.findall(r"^(?:int|const char \*)\s*(jh_\w+)\(", header, re.M)))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    groups = re.findall(r"`(jh_\w+(?:/\w+)+)`", doc)                 # `jh_a_b/c/d` -> jh_a_b, jh_a_c, jh_a_d
    spelled = set()
    for g in groups:
        head, *rest = g.split("/")
        spelled.add(head)
        stem = head.rsplit("_", 1)[0]
        for r in rest:
            spelled.add(r if r.startswith("jh_") else f"{stem}_{r}")
            if "_" in stem:                                           # `jh_comm_unique_id/init_rank` style: suffix replaces the last TWO words
                spelled.add(f"{stem.rsplit('_', 1)[0]}_{r}")
    missing = [n for n in names if n not in doc and n not in spelled]
    assert len(names) >= 80 and not missing, missing


def test_every_knob_the_library_accepts_is_described_in_the_header():
    """jh_tune_set / jh_tune_get / jh_blockop_tune_* take a NAME: the names the sources know are the interface, so each one
    must appear, quoted, in include/jetship.h's description of the knobs."""
    import re

    from . import knob_table

    hdr = open(os.path.join(ROOT, "include", "jetship.h")).read()
    names = set(knob_table.rows())                                              # the context's knobs and counters: the rows of jh_knobs.def
    import glob

    for f in glob.glob(os.path.join(ROOT, "jets.jl_amd", "csrc", "*.hip")):     # (jh_core.hip: the five process-wide names; jh_tall.hip: the per-operator ones)
        names |= set(re.findall(r'strcmp\(name, "([a-z_0-9]+)"\)', open(f).read()))
    assert set(knob_table.PROCESS_WIDE_SETTABLE + knob_table.PROCESS_WIDE_READ_ONLY) <= names
    assert len(names) > 40
    missing = sorted(n for n in names if f'"{n}"' not in hdr)
    assert not missing, f"knobs without a description in include/jetship.h: {missing}"
