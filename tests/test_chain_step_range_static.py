"""CPU: the ranged Golub-Kahan step of a FORWARD chain (jh_chain_bidiag_step_range) through the layers that need no GPU -- the header documents it and
cites the reference lines it replaces, the built library exports it, the step instantiations of k_chain_adj (MODE 2: the ranged call runs the
whole-vector step's kernels, its bounds are kernel arguments) are as many as before and none has scratch, the Python mirror and the Julia file bind
it."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HEADER = os.path.join(ROOT, "include", "jetship.h")
LIB = os.path.join(ROOT, "jets.jl_amd", "libjetship.so")
JULIA = os.path.join(ROOT, "julia", "JetsHIP.jl")
NAME = "jh_chain_bidiag_step_range"


def test_the_header_documents_the_call():
    text = open(HEADER).read()
    proto = re.search(r"int jh_chain_bidiag_step_range\(([^;]*)\);", text)
    assert proto, "prototype"
    params = re.sub(r"\s+", " ", proto.group(1))
    assert params == ("const jh_chain *fwd, jh_bvec *u, const jh_bvec *v, jh_bvec *w, double alpha, double beta, int64_t first_elem, "
                      "int64_t count, double *normsq")
    doc = text[text.index("/* jh_chain_bidiag_step_range:"):proto.start()]
    for must in ("src/Jets.jl:1138-1154", "530-540", "1034-1057", "16-byte", "count == 0", "jh_normsq_reset", "jh_normsq_read", "JH_ERR_INVALID",
                 "JH_ERR_UNSUPPORTED", "grid chain", "last_adj_parts", "beta == 0"):
        assert must in doc, f"the header's description of {NAME} should mention {must!r}"
    # the sentence about grid chains that other tests read stays as it was
    assert "jh_chain_apply_range and jh_chain_bidiag_step on a grid chain return JH_ERR_UNSUPPORTED before touching" in text


def test_the_library_exports_it_and_the_python_mirror_binds_it():
    import jets_jl_amd as J
    from jets_jl_amd import chains
    from jets_jl_amd._ffi import SYMBOLS

    assert hasattr(ctypes.CDLL(J.LIB_PATH), NAME)
    ret, args = SYMBOLS[NAME]
    assert len(args) == 9
    assert hasattr(chains.ChainHandle, "bidiag_step_range")
    assert "chain_step_range_calls" in chains.STATS


def test_step_instantiations_of_k_chain_adj_have_no_scratch_and_were_not_multiplied():
    import kernel_resources

    ks = [k for k in kernel_resources.kernels(LIB) if "k_chain_adj" in k["name"]]
    names = kernel_resources.demangle([k["name"] for k in ks])
    step = []
    for k, nm in zip(ks, names):
        m = re.search(r"k_chain_adj<([^>]*)>", nm)
        assert m, nm
        targs = [t.strip() for t in m.group(1).split(",")]          # S, E, NS, U, DEPTH, NT, MODE, BLK, NW
        if targs[6] == "2":
            step.append((k, nm))
    assert len(step) == 66, f"{len(step)} step instantiations (66 before the ranged form: its bounds are kernel arguments)"
    bad = [nm for k, nm in step if k["scratch"] > 0]
    assert not bad, bad


def test_the_julia_file_binds_it():
    text = open(JULIA).read()
    assert ":jh_chain_bidiag_step_range, LIB" in text
    assert re.search(r"^function bidiag_step_range!\(", text, re.M)


def test_rowpart_and_the_solvers_take_the_route():
    """the wiring that needs no device: _ShardChains plans the FORWARD run, the engines ask for it, JETS_CHAIN_STEP is the switch"""
    src = {f: open(os.path.join(ROOT, "jets.jl_amd", f)).read() for f in ("rowpart.py", "lsqr.py", "cgls.py", "chains.py")}
    assert "has_step" in src["rowpart.py"] and "JETS_CHAIN_STEP" in src["rowpart.py"] and "bidiag_step_range" in src["rowpart.py"]
    assert "chain_step" in src["lsqr.py"] and "step_cgls" in src["lsqr.py"] and "step_cgls" in src["cgls.py"]
    assert '"chain_step_range_calls"' in src["chains.py"]
