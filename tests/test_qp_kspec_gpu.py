"""GPU: the QP kernel's K-specialised instantiations (csrc/qp_inst.hpp QPKSpec: the node count K = 50 at compile
time) against the runtime-K instantiation of the same class, forced with the environment variable
SCVX_QP_GENERIC_K (read by the library at every launch).

Both run the same arithmetic on the same workspace layout, so the results are expected to be equal bit for bit
(each test prints whether they are); the asserted bounds are: statuses and IPM iteration counts identical, objective
1e-10 relative, X and U 1e-8 absolute.  A warm start written by one instantiation must serve the other."""
import os

import numpy as np
import pytest

import scvx_hip
from scvx_hip import workloads

pytestmark = pytest.mark.gpu

ENV = "SCVX_QP_GENERIC_K"
K = 50
BOX = [(0, -12.0, 12.0), (1, -12.0, 12.0)]


def _t(x, cuda, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=cuda, dtype=dtype or torch.float64)


@pytest.fixture
def force_generic():
    """force_generic(flag): the next launches run the runtime-K instantiation (flag) or the library's choice."""
    before = os.environ.get(ENV)

    def set_(flag):
        if flag:
            os.environ[ENV] = "1"
        else:
            os.environ.pop(ENV, None)
    yield set_
    if before is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = before


def _jacobi(cuda, force_generic, sc, spec, generic_per_step, coupling_R=None):
    """Jacobi SCvx steps from the scenario's initial iterate: step 0 cold, the later ones warm from the previous
    step's primal-dual point; generic_per_step[s] picks the instantiation of step s.  Returns every step's outputs."""
    import torch
    N = sc["X"].shape[0]
    X, U, sig = _t(sc["X"], cuda), _t(sc["U"], cuda), _t(sc["sigma"], cuda)
    xi, xf, tr = _t(sc["x_init"], cuda), _t(sc["x_final"], cuda), _t(np.full(N, 0.25), cuda)
    solver = scvx_hip.QPSolver(spec, N, device=cuda)
    warm, steps = None, []
    for generic in generic_per_step:
        disc = scvx_hip.foh_batched("di", X, U, sig)
        rows = cnt = None
        if coupling_R is not None:
            rows, cnt = scvx_hip.collision_rows(X, 0, N, coupling_R, j_max=spec.j_max)
        force_generic(generic)
        out = solver.solve(disc, sig, X, U, xi, xf, tr, rows, cnt, warm=warm)
        torch.cuda.synchronize()
        force_generic(False)
        steps.append({k: v.cpu().numpy().copy() for k, v in out.items()})
        X, U = out["X"].clone(), out["U"].clone()
        warm = (out["status"] == 0).to(torch.int32)
    return steps


def _same(a_steps, b_steps, what):
    exact = True
    for s, (a, b) in enumerate(zip(a_steps, b_steps)):
        assert np.array_equal(a["status"], b["status"]), (what, s, a["status"], b["status"])
        assert np.array_equal(a["iters"], b["iters"]), (what, s, a["iters"], b["iters"])
        dobj = np.abs(a["obj"] - b["obj"]) / np.maximum(1.0, np.abs(b["obj"]))
        dX, dU = np.abs(a["X"] - b["X"]).max(), np.abs(a["U"] - b["U"]).max()
        eq = all(np.array_equal(a[k], b[k]) for k in ("X", "U", "obj", "slack_coll"))
        exact = exact and eq
        print(f"{what} step {s}: bitwise equal {eq}, max rel |dobj| {dobj.max():.3e}, |dX| {dX:.3e}, |dU| {dU:.3e}, "
              f"iters {a['iters'].tolist()}, status {a['status'].tolist()}")
        assert dobj.max() <= 1e-10, (what, s, dobj.max())
        assert dX <= 1e-8 and dU <= 1e-8, (what, s, dX, dU)
    print(f"{what}: bitwise equal over all steps: {exact}")


def _c3():
    sc = workloads.synthetic_di(8, K=K, seed=1, obstacles=8)
    spec = scvx_hip.QPSpec(model="di", K=K, box=BOX, obs=sc["obs"], w_obs=1e6, u_max=1.0, tol=1e-8, max_iter=60)
    return sc, spec


@pytest.fixture(scope="module")
def c3_runs():
    return {}


def _c3_run(cuda, force_generic, cache, pattern):
    if pattern not in cache:
        sc, spec = _c3()
        cache[pattern] = _jacobi(cuda, force_generic, sc, spec, pattern)
    return cache[pattern]


def test_c3_specialised_equals_generic_cold_and_warm(cuda, force_generic, c3_runs):
    spec_ = _c3_run(cuda, force_generic, c3_runs, (False, False, False))
    gen = _c3_run(cuda, force_generic, c3_runs, (True, True, True))
    assert all((s["status"] == 0).any() for s in spec_)
    # the warm re-solves did start warm: fewer iterations than the cold solve
    assert spec_[1]["iters"].mean() < spec_[0]["iters"].mean()
    _same(spec_, gen, "c3 specialised vs generic")


def test_c3_warm_start_crosses_instantiations(cuda, force_generic, c3_runs):
    spec_ = _c3_run(cuda, force_generic, c3_runs, (False, False, False))
    gen = _c3_run(cuda, force_generic, c3_runs, (True, True, True))
    _same(_jacobi(cuda, force_generic, *_c3(), (False, True)), spec_[:2], "c3 specialised then generic vs specialised")
    _same(_jacobi(cuda, force_generic, *_c3(), (True, False)), gen[:2], "c3 generic then specialised vs generic")


def test_c2_class_specialised_equals_generic(cuda, force_generic):
    sc = workloads.synthetic_di(8, K=K, seed=0, obstacles=0)
    spec = scvx_hip.QPSpec(model="di", K=K, box=BOX, obs=[], w_obs=1e6, u_max=None, tol=1e-8, max_iter=60)
    a = _jacobi(cuda, force_generic, sc, spec, (False,))
    b = _jacobi(cuda, force_generic, sc, spec, (True,))
    assert (a[0]["status"] == 0).any()
    _same(a, b, "c2 class")


def test_c4_class_specialised_equals_generic(cuda, force_generic):
    """8 agents on a 2 x 2 x 2 lattice whose straight paths cross: collision rows from collision_rows, j_max = 8."""
    sc = workloads.synthetic_lattice(side=2, K=K, seed=2)
    spec = scvx_hip.QPSpec(model="di", K=K, box=[(0, -50.0, 50.0), (1, -50.0, 50.0)], obs=[], w_obs=1e6, j_max=8,
                           w_coll=1e4, tol=1e-8, max_iter=60)
    a = _jacobi(cuda, force_generic, sc, spec, (False,), coupling_R=2.3)
    b = _jacobi(cuda, force_generic, sc, spec, (True,), coupling_R=2.3)
    assert (a[0]["status"] == 0).any()
    _same(a, b, "c4 class")
