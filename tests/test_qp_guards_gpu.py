"""GPU: the QP kernel's row loops under one lane mask each (DESIGN §3.3 "Lane guards and spill reloads") against goldens
recorded with the build before the change (tests/golden/qp_guard_steps.npz, written by
tests/golden/make_qp_guard_goldens.py on an MI355X).

No floating-point expression changed, so every output is asserted equal bit for bit: np.array_equal on obj, status,
iters and the collision slack of every step and on X, U of the last step -- the float arrays by their bit patterns --
and the SHA-256 of the raw bytes of X, U of every step (the golden file keeps the earlier steps' big arrays as digests
only).  Every solve of every case ends with status 0 or 1 in the recorded build.

The one-mask form is compiled only into the flag-specialised K = 50 instantiations, and every case here runs a
runtime-flag instantiation: this file pins those kernels at the shapes where a lane mask would go wrong; the changed
device code is pinned by the "flags" goldens of tests/test_qp_insn_gpu.py.

Each case is a Jacobi loop of one cold and two warm steps of 8 agents (tests/qp_guard_cases.py lists the cases and what
each is there for: no idle lane, one, 52; the row mask changed by ineq_last; a free last input; fewer obstacles and no
box; no soft rows; per-lane collision row counts).  The instantiation a solve takes is read back from the library
(scvx_qp_instantiation) and compared with the one the case names."""
import os

import numpy as np
import pytest

import qp_guard_cases as gc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qp_guard_steps.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


def _bits(v):
    """a float array as its bit patterns (equal NaNs compare equal, -0.0 differs from +0.0), others unchanged"""
    return np.ascontiguousarray(v).view(np.uint64) if v.dtype == np.float64 else v


@pytest.mark.parametrize("name,K,inst", gc.CASES)
def test_steps_equal_parent(cuda, golden, name, K, inst):
    assert gc.instantiation(name, K) == inst
    steps = gc.run(cuda, name, K)
    assert len(steps) == gc.STEPS
    assert any((s["status"] == 0).any() for s in steps)
    for s, got in enumerate(steps):
        for k in gc.KEYS:
            key = gc.golden_key(name, K, s, k)
            v = got[k].astype(np.float64) if got[k].dtype.kind == "f" else got[k]
            if key in golden:
                assert v.dtype == golden[key].dtype and v.shape == golden[key].shape, key
                eq = np.array_equal(_bits(v), _bits(golden[key]))
                dmax = float(np.nanmax(np.abs(v.astype(np.float64) - golden[key]))) if not eq else 0.0
                print(f"{name} K={K} step {s} {k}: equal {eq}, max |d| {dmax:.3e}")
                assert eq, (name, K, s, k, dmax)
            else:
                assert k in gc.BIG and s < gc.STEPS - 1, key
            if k in gc.BIG:
                assert np.array_equal(gc.ic.digest(v), golden[key + ".sha256"]), (name, K, s, k, "bytes differ")
        print(f"{name} K={K} step {s}: iters {got['iters'].tolist()}, status {got['status'].tolist()}")
