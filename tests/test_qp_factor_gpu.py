"""GPU: the QP kernel's factor sweep with its reads rescheduled (DESIGN §3.3 "The factor's read batches": one read batch
per phase, the next phase's operands read ahead of the fences) against
goldens recorded with the build before the change (tests/golden/qp_factor_steps.npz, written by
tests/golden/make_qp_factor_goldens.py on an MI355X).

No floating-point expression changed, so every output is asserted equal bit for bit: np.array_equal on obj, status,
iters and the collision slack of every step and on X, U (nu) of the last step, and the SHA-256 of the raw bytes of
X, U (nu) of every step (the golden file keeps the earlier steps' big arrays as digests only).

Each case is a Jacobi loop of one cold and two warm steps of 8 agents at a runtime K (tests/qp_factor_cases.py lists
the cases and what each is there for).  The instantiation a solve takes is read back from the library
(scvx_qp_instantiation: the runtime-K, runtime-flag kernel for every case), and the capacity class through the
workspace bytes per agent, which the golden file records."""
import ctypes
import os

import numpy as np
import pytest

import qp_factor_cases as fc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qp_factor_steps.npz")
GENERIC = 0


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("name,K", fc.CASES)
def test_steps_equal_parent(cuda, golden, name, K):
    from scvx_hip import _lib
    tpl = fc.build(name, K)[2].to_c()
    assert int(_lib.lib().scvx_qp_instantiation(ctypes.byref(tpl))) == GENERIC
    assert fc.ws_bytes(name, K) == int(golden[f"{name}/K{K}/{fc.WS_KEY}"])
    steps = fc.run(cuda, name, K)
    assert len(steps) == fc.STEPS
    assert any((s["status"] == 0).any() for s in steps)
    for s, got in enumerate(steps):
        for k in fc.keys_of(name):
            key = fc.golden_key(name, K, s, k)
            v = got[k].astype(np.float64) if got[k].dtype.kind == "f" else got[k]
            if key in golden:
                eq = np.array_equal(v, golden[key])
                dmax = float(np.abs(v.astype(np.float64) - golden[key]).max()) if not eq else 0.0
                print(f"{name} K={K} step {s} {k}: equal {eq}, max |d| {dmax:.3e}")
                assert eq, (name, K, s, k, dmax)
            if k in fc.BIG:
                assert np.array_equal(fc.ic.digest(v), golden[key + ".sha256"]), (name, K, s, k, "bytes differ")
        print(f"{name} K={K} step {s}: iters {got['iters'].tolist()}, status {got['status'].tolist()}")
