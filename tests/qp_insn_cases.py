"""The Jacobi fixtures of tests/test_qp_insn_gpu.py and of its golden generator (tests/golden/make_qp_insn_goldens.py):
one cold and two warm steps per case, so the warm path and both Newton solves of every IPM iteration run.

Cases (8 agents; 4 for the n = 12 class), each at K = 50 and at a small runtime K (12 for n = 6, 24 for n = 12: the
smallest with K >= 2 n, which the warm start needs):
    c3        <6,3,2,8,0,0>: 8 obstacles, SOC, box on (0, 1), hard terminal -- bench.py c3's template
    c2        <6,3,2,0,0,0>: box on (0, 1), hard terminal                   -- bench.py c2's template
    c4        <6,3,2,0,8,0>: 8 collision rows, box on (0, 1)                -- bench.py c4's template
    quad_vc   <12,4,4,8,8,1>: a virtual-control quadrotor class (no flag-specialised instantiation)
Flag mismatches at K = 50: c3's template with one field changed each.  The class stays <6,3,2,8,0,0>, the host must
take the runtime-flag instantiation (csrc/qp_inst.hpp qp_flags_match compares every field):
    c3_nosoc  no SOC;  c3_obs3  3 of the 8 obstacles;  c3_box  the box on indices (1, 2);  c3_soft  a soft terminal

Instantiations: "flags" the library's own choice (flag- and K-specialised where compiled), "kspec" runtime flags with
K at compile time (SCVX_QP_GENERIC_FLAGS=1), "generic" everything at run time (SCVX_QP_GENERIC_K=1)."""
import os

import numpy as np

ENV_K, ENV_F = "SCVX_QP_GENERIC_K", "SCVX_QP_GENERIC_FLAGS"
STEPS = 3
BOX = [(0, -12.0, 12.0), (1, -12.0, 12.0)]
W_NU, W_PROX = 1e4, 10.0          # bench.py C5_W_NU, C5_W_PROX
KEYS = ("X", "U", "obj", "iters", "status", "slack_coll", "nu")
CLASSES = ("c3", "c2", "c4", "quad_vc")
MISMATCH = ("c3_nosoc", "c3_obs3", "c3_box", "c3_soft")
INSTS = ("flags", "kspec", "generic")


def small_k(name):
    return 24 if name == "quad_vc" else 12


def keys_of(name):
    """nu is recorded where the class carries virtual control (the solver returns zeros otherwise)"""
    return tuple(k for k in KEYS if k != "nu" or name == "quad_vc")


def _t(x, cuda):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=cuda, dtype=torch.float64)


def build(name, K):
    """-> (model, scenario arrays, QPSpec, coupling radius or None)"""
    import scvx_hip
    from scvx_hip import workloads
    if name.startswith("c3"):
        sc = workloads.synthetic_di(8, K=K, seed=1, obstacles=8)
        kw = dict(model="di", K=K, box=BOX, obs=sc["obs"], w_obs=1e6, u_max=1.0, tol=1e-8, max_iter=60)
        if name == "c3_nosoc":
            kw["u_max"] = None
        elif name == "c3_obs3":
            kw["obs"] = sc["obs"][:3]
        elif name == "c3_box":
            kw["box"] = [(1, -12.0, 12.0), (2, -12.0, 12.0)]
        elif name == "c3_soft":
            kw.update(has_final=False, w_final=100.0)
        elif name != "c3":
            raise KeyError(name)
        return "di", sc, scvx_hip.QPSpec(**kw), None
    if name == "c2":
        sc = workloads.synthetic_di(8, K=K, seed=0, obstacles=0)
        spec = scvx_hip.QPSpec(model="di", K=K, box=BOX, obs=[], w_obs=1e6, u_max=None, tol=1e-8, max_iter=60)
        return "di", sc, spec, None
    if name == "c4":
        sc = workloads.synthetic_lattice(side=2, K=K, seed=2)
        spec = scvx_hip.QPSpec(model="di", K=K, box=BOX, obs=[], w_obs=1e6, j_max=8, w_coll=1e4, tol=1e-8, max_iter=60)
        return "di", sc, spec, 2.3
    if name == "quad_vc":
        full = workloads.synthetic_quad(1024, K=K, seed=3, sigma=30.0, obstacles=8)
        sc = {k: np.ascontiguousarray(full[k][:4]) for k in ("X", "U", "x_init", "x_final", "sigma")}
        spec = scvx_hip.QPSpec(model="quad", K=K, box=workloads.QUAD_BOX, obs=full["obs"], w_obs=1e6, j_max=8, w_coll=1e4,
                               tol=1e-8, max_iter=60, w_nu=W_NU, w_prox=W_PROX)
        return "quad", sc, spec, 0.5
    raise KeyError(name)


def run(cuda, name, K, inst):
    """The case's Jacobi loop from the scenario's initial iterate: step 0 cold, the later ones warm from the previous
    step's primal-dual point.  Returns every step's outputs (numpy, keys_of(name))."""
    import torch
    import scvx_hip
    model, sc, spec, R = build(name, K)
    N = sc["X"].shape[0]
    X, U, sig = _t(sc["X"], cuda), _t(sc["U"], cuda), _t(sc["sigma"], cuda)
    xi, xf, tr = _t(sc["x_init"], cuda), _t(sc["x_final"], cuda), _t(np.full(N, 0.25), cuda)
    solver = scvx_hip.QPSolver(spec, N, device=cuda)
    before = {e: os.environ.get(e) for e in (ENV_K, ENV_F)}
    warm, steps = None, []
    try:
        os.environ.pop(ENV_K, None)
        os.environ.pop(ENV_F, None)
        if inst == "generic":
            os.environ[ENV_K] = "1"
        elif inst == "kspec":
            os.environ[ENV_F] = "1"
        elif inst != "flags":
            raise KeyError(inst)
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
        for e, v in before.items():
            if v is None:
                os.environ.pop(e, None)
            else:
                os.environ[e] = v
    return steps


def all_cases():
    """(name, K) of every recorded case"""
    return ([(n, 50) for n in CLASSES] + [(n, small_k(n)) for n in CLASSES] + [(n, 50) for n in MISMATCH])


def golden_key(name, K, inst, step, key):
    return f"{name}/K{K}/{inst}/{step}/{key}"


BIG = ("X", "U", "nu")   # stored in full for the last step only; every step has their digest


def digest(v):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(v).tobytes()).digest(), dtype=np.uint8)


def pack(name, K, inst, step, st, last):
    """the golden file's entries of one step's outputs"""
    out = {}
    for k in keys_of(name):
        v = st[k].astype(np.float64) if st[k].dtype.kind == "f" else st[k]
        if k in BIG:
            out[golden_key(name, K, inst, step, k) + ".sha256"] = digest(v)
        if k not in BIG or last:
            out[golden_key(name, K, inst, step, k)] = v
    return out
