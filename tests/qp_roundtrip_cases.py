"""The Jacobi fixtures of tests/test_qp_roundtrips_gpu.py and of its golden generator
(tests/golden/make_qp_roundtrip_goldens.py): one cold and two warm steps per case, so the warm path and both Newton
solves of every IPM iteration run.

Cases: the three double-integrator fixtures of tests/test_qp_kspec_gpu.py (8 C3 agents, 8 C2 agents, the 2 x 2 x 2
lattice with collision rows) and 4 virtual-control quadrotors (n = 12; w_nu, w_prox, coupling as bench.py c5).  Every
case runs with the library's instantiation (K = 50 at compile time where the class has one) and with the runtime-K
instantiation forced through SCVX_QP_GENERIC_K."""
import os

import numpy as np

ENV = "SCVX_QP_GENERIC_K"
K = 50
STEPS = 3
BOX = [(0, -12.0, 12.0), (1, -12.0, 12.0)]
W_NU, W_PROX = 1e4, 10.0          # bench.py C5_W_NU, C5_W_PROX
KEYS = ("X", "U", "obj", "iters", "status", "slack_coll", "nu")
CASES = ("c3", "c2", "c4", "quad_vc")
INSTS = ("kspec", "generic")


def keys_of(name):
    """nu is recorded where the class carries virtual control (the solver returns zeros otherwise)"""
    return tuple(k for k in KEYS if k != "nu" or name == "quad_vc")


def _t(x, cuda):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=cuda, dtype=torch.float64)


def build(name):
    """-> (model, scenario arrays, QPSpec, coupling radius or None)"""
    import scvx_hip
    from scvx_hip import workloads
    if name == "c3":
        sc = workloads.synthetic_di(8, K=K, seed=1, obstacles=8)
        spec = scvx_hip.QPSpec(model="di", K=K, box=BOX, obs=sc["obs"], w_obs=1e6, u_max=1.0, tol=1e-8, max_iter=60)
        return "di", sc, spec, None
    if name == "c2":
        sc = workloads.synthetic_di(8, K=K, seed=0, obstacles=0)
        spec = scvx_hip.QPSpec(model="di", K=K, box=BOX, obs=[], w_obs=1e6, u_max=None, tol=1e-8, max_iter=60)
        return "di", sc, spec, None
    if name == "c4":
        sc = workloads.synthetic_lattice(side=2, K=K, seed=2)
        spec = scvx_hip.QPSpec(model="di", K=K, box=[(0, -50.0, 50.0), (1, -50.0, 50.0)], obs=[], w_obs=1e6, j_max=8,
                               w_coll=1e4, tol=1e-8, max_iter=60)
        return "di", sc, spec, 2.3
    if name == "quad_vc":
        full = workloads.synthetic_quad(1024, K=K, seed=3, sigma=30.0, obstacles=8)
        sc = {k: np.ascontiguousarray(full[k][:4]) for k in ("X", "U", "x_init", "x_final", "sigma")}
        spec = scvx_hip.QPSpec(model="quad", K=K, box=workloads.QUAD_BOX, obs=full["obs"], w_obs=1e6, j_max=8, w_coll=1e4,
                               tol=1e-8, max_iter=60, w_nu=W_NU, w_prox=W_PROX)
        return "quad", sc, spec, 0.5
    raise KeyError(name)


def run(cuda, name, generic):
    """The case's Jacobi loop from the scenario's initial iterate: step 0 cold, the later ones warm from the previous
    step's primal-dual point.  Returns every step's outputs (numpy, keys_of(name))."""
    import torch
    import scvx_hip
    model, sc, spec, R = build(name)
    N = sc["X"].shape[0]
    X, U, sig = _t(sc["X"], cuda), _t(sc["U"], cuda), _t(sc["sigma"], cuda)
    xi, xf, tr = _t(sc["x_init"], cuda), _t(sc["x_final"], cuda), _t(np.full(N, 0.25), cuda)
    solver = scvx_hip.QPSolver(spec, N, device=cuda)
    before = os.environ.get(ENV)
    warm, steps = None, []
    try:
        if generic:
            os.environ[ENV] = "1"
        else:
            os.environ.pop(ENV, None)
        for _ in range(STEPS):
            disc = scvx_hip.foh_batched(model, X, U, sig)
            rows = cnt = None
            if R is not None:
                rows, cnt = scvx_hip.collision_rows(X, 0, N, R, j_max=spec.j_max)
            out = solver.solve(disc, sig, X, U, xi, xf, tr, rows, cnt, warm=warm)
            torch.cuda.synchronize()
            steps.append({k: out[k].cpu().numpy().copy() for k in keys_of(name)})
            X, U = out["X"].clone(), out["U"].clone()
            warm = (out["status"] == 0).to(torch.int32)
    finally:
        if before is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = before
    return steps


def golden_key(name, inst, step, key):
    return f"{name}/{inst}/{step}/{key}"
