"""CPU: tests/golden/bcast_functions.npz is what tests/golden/make_bcast_functions.py writes (every 16th point of every (function, type)
regenerated with mpmath at 50 digits; skipped where mpmath is not installed), and has the shape the GPU tests rely on."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_bcast_functions", os.path.join(GOLDEN, "make_bcast_functions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_complete_and_holds_exact_values_of_its_type():
    gen = _generator()
    z = np.load(gen.PATH)
    assert os.path.getsize(gen.PATH) < (1 << 19)
    for fn in gen.FUNCTIONS:
        for ty, dt in gen.TYPES.items():
            hi = z[f"{fn}/{ty}/hi"]
            ops = [z[f"{fn}/{ty}/x{k}"] for k in range(2 if fn in gen.BINARY else 1)]
            assert 100 <= len(hi) <= gen.MAX_POINTS and all(o.shape == hi.shape and o.dtype == np.float64 for o in ops)
            for o in ops:
                with np.errstate(over="ignore"):
                    assert np.array_equal(o.astype(dt).astype(np.float64), o, equal_nan=True), f"{fn}/{ty}: an operand is no exact value of the type"
            if ty == "f64":
                lo = z[f"{fn}/{ty}/lo"]
                fin = np.isfinite(hi) & (hi != 0)
                with np.errstate(over="ignore"):
                    half_ulp = np.maximum(np.spacing(np.abs(hi[fin])) / 2, 5e-324)
                assert np.all(np.abs(lo[fin]) <= half_ulp) and not lo[~fin].any()   # a double-double: |lo| <= ulp(hi) / 2
            else:
                assert f"{fn}/{ty}/lo" not in z.files


def test_fixture_is_what_the_generator_writes():
    pytest.importorskip("mpmath")
    gen = _generator()
    z = np.load(gen.PATH)
    again = gen.cases(stride=16)
    assert {k.rsplit("/", 1)[0] for k in again} == {k.rsplit("/", 1)[0] for k in z.files}
    for name, arr in again.items():
        assert arr.tobytes() == z[name][::16].tobytes(), f"{name}: every 16th point regenerated differs from the committed file"
