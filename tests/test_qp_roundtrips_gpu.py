"""GPU: the QP kernel after the IPM iteration's workspace round trips were merged and hoisted (the corrector's rhs
reuses the state live from the predictor's step length; one load batch per node phase; the solve passes' operands in
flight across the chains; the predictor's rhs batch issued inside the factor: DESIGN §3.3 "Workspace round trips")
against goldens recorded with the build before that change
(tests/golden/qp_roundtrip_steps.npz, written by tests/golden/make_qp_roundtrip_goldens.py on an MI355X).

Only loads moved: no floating-point expression changed, so every array is expected to be equal bit for bit (each
test prints whether it is).  Asserted: statuses and IPM iteration counts identical, objective 1e-10 relative, X and U
1e-8 absolute (the bounds of tests/test_qp_kspec_gpu.py).  Each case is a Jacobi loop of one cold and two warm steps
(the warm path and both Newton solves of every iteration run), with the K = 50 and the forced runtime-K
instantiation."""
import os

import numpy as np
import pytest

import qp_roundtrip_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qp_roundtrip_steps.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


def _gold(golden, name, inst, step, key):
    same = bool(golden["generic_equals_kspec"][rc.CASES.index(name)])
    return golden[rc.golden_key(name, "kspec" if (same or inst == "kspec") else "generic", step, key)]


@pytest.mark.parametrize("inst", rc.INSTS)
@pytest.mark.parametrize("name", rc.CASES)
def test_steps_match_goldens(cuda, golden, name, inst):
    steps = rc.run(cuda, name, inst == "generic")
    assert len(steps) == rc.STEPS
    assert any((s["status"] == 0).any() for s in steps)
    exact = True
    for s, got in enumerate(steps):
        g = {k: _gold(golden, name, inst, s, k) for k in rc.keys_of(name)}
        eq = all(np.array_equal(got[k], g[k]) for k in rc.keys_of(name))
        exact = exact and eq
        dobj = np.abs(got["obj"] - g["obj"]) / np.maximum(1.0, np.abs(g["obj"]))
        dX, dU = np.abs(got["X"] - g["X"]).max(), np.abs(got["U"] - g["U"]).max()
        dS = np.abs(got["slack_coll"] - g["slack_coll"]).max()
        dN = np.abs(got["nu"] - g["nu"]).max() if "nu" in got else 0.0
        print(f"{name} {inst} step {s}: bitwise equal {eq}, max rel |dobj| {dobj.max():.3e}, |dX| {dX:.3e}, "
              f"|dU| {dU:.3e}, |dslack| {dS:.3e}, |dnu| {dN:.3e}, iters {got['iters'].tolist()}, "
              f"status {got['status'].tolist()}")
        assert np.array_equal(got["status"], g["status"]), (name, inst, s, got["status"], g["status"])
        assert np.array_equal(got["iters"], g["iters"]), (name, inst, s, got["iters"], g["iters"])
        assert dobj.max() <= 1e-10, (name, inst, s, dobj.max())
        assert dX <= 1e-8 and dU <= 1e-8, (name, inst, s, dX, dU)
        assert dS <= 1e-8 and dN <= 1e-8, (name, inst, s, dS, dN)
    print(f"{name} {inst}: bitwise equal over all steps: {exact}")
