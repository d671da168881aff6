"""The Jacobi fixtures of tests/test_qp_factor_gpu.py and of its golden generator (tests/golden/make_qp_factor_goldens.py):
one cold and two warm steps per case (tests/qp_insn_cases.py's loop), at the shapes where the factor sweep's read
scheduling (DESIGN §3.3 "The factor's read batches") can go wrong and that the goldens of qp_insn_cases do not reach.

Cases (8 agents each; every K is a runtime K, so every case runs the runtime-K, runtime-flag instantiation):
    c3 K = 13, 14   <6,3,2,8,0,0>, qp_insn_cases' c3 scenario.  With its K = 12 these are the three exits of the
                    three-way unrolled stage loop, with the prefetches of stages ts - 3 < 0 and stage 0, which stores no
                    next packet
    uni K = 7, 8    <3,2,2,4,0,0>: the unicycle class -- one repetition per phase, odd n, m = 2
    si K = 7, 8     <3,3,4,8,0,0>: the single-integrator class -- one repetition per phase, n = m = 3, SOC
    di_vc K = 12    <6,3,2,8,0,1>: the double integrator with virtual control; phases 0 and 5 sit around the moved reads
    di_oc K = 12    <6,3,2,8,8,0>: obstacles and collision rows from a 2^3 lattice: the stiff-facet class, whose
                    candidate nodes take the second copy of phase 3 (which issues phase 4's operands too)
K >= 2 n everywhere, which the warm start needs.  The capacity class a case runs on follows from its row counts
(csrc/qp_caps.hpp: the first class that fits); the goldens record the workspace bytes of the class, which differ
between the classes of a model."""
import ctypes

import numpy as np

import qp_insn_cases as ic

STEPS = ic.STEPS
KEYS = ic.KEYS
BIG = ic.BIG
N_AGENTS = 8
CASES = (("c3", 13), ("c3", 14), ("uni", 7), ("uni", 8), ("si", 7), ("si", 8), ("di_vc", 12), ("di_oc", 12))
WS_KEY = "ws_bytes"


def keys_of(name):
    """nu is recorded where the class carries virtual control (the solver returns zeros otherwise)"""
    return tuple(k for k in KEYS if k != "nu" or name == "di_vc")


def _small_model(model, K, seed):
    """Straight lines between seeded end points with a perturbed input guess, as test_qp_gpu.py builds the unicycle
    and single-integrator scenarios (two obstacles near the paths)."""
    rng = np.random.default_rng(seed)
    N, n = N_AGENTS, 3
    a = np.linspace(0, 1, K)[None, :, None]
    p0 = rng.uniform(-8, -5, (N, 1, n))
    p1 = rng.uniform(5, 8, (N, 1, n))
    X = p0 * (1 - a) + p1 * a
    if model == "unicycle":
        X[:, :, 2] = np.pi / 4 + rng.normal(0, 0.1, (N, K))
        U = np.stack([np.full((N, K), 0.8), rng.normal(0, 0.1, (N, K))], -1)
        sig = np.full(N, 24.0)
        obs = [(np.array([0.5, -0.5]), 1.5), (np.array([-3.0, -2.0]), 1.0)]
    else:
        U = np.repeat(((p1 - p0)[:, 0] / 12.0)[:, None, :], K, 1) + rng.normal(0, 0.05, (N, K, 3))
        sig = np.full(N, 12.0)
        obs = [(np.array([0.3, -0.4, 0.2]), 1.5), (np.array([-4.0, -3.0, -4.0]), 1.0)]
    return dict(X=np.ascontiguousarray(X), U=np.ascontiguousarray(U), sigma=sig, obs=obs,
                x_init=X[:, 0, :].copy(), x_final=X[:, -1, :].copy())


def build(name, K):
    """-> (model, scenario arrays, QPSpec, coupling radius or None, trust region)"""
    import scvx_hip
    from scvx_hip import workloads
    if name == "c3":
        model, sc, spec, R = ic.build("c3", K)
        return model, sc, spec, R, 0.25
    if name in ("uni", "si"):
        model = "unicycle" if name == "uni" else "si"
        sc = _small_model(model, K, seed=11 + K)
        spec = scvx_hip.QPSpec(model=model, K=K, pos_dim=2 if name == "uni" else 3, box=[(0, -10, 10), (1, -10, 10)],
                               obs=sc["obs"], w_obs=1e6, u_max=None if name == "uni" else 3.0, tol=1e-8, max_iter=60)
        return model, sc, spec, None, 0.5
    if name == "di_vc":
        sc = workloads.synthetic_di(N_AGENTS, K=K, seed=1, obstacles=8)
        spec = scvx_hip.QPSpec(model="di", K=K, box=ic.BOX, obs=sc["obs"], w_obs=1e6, u_max=1.0, tol=1e-8, max_iter=60,
                               w_nu=ic.W_NU, w_prox=ic.W_PROX)
        return "di", sc, spec, None, 0.25
    if name == "di_oc":
        sc = workloads.synthetic_lattice(side=2, K=K, seed=2, obstacles=8)
        spec = scvx_hip.QPSpec(model="di", K=K, box=ic.BOX, obs=sc["obs"], w_obs=1e6, j_max=8, w_coll=1e4, tol=1e-8,
                               max_iter=60)
        return "di", sc, spec, 2.3, 0.25
    raise KeyError(name)


def ws_bytes(name, K):
    """workspace bytes of one agent of the case's class (the library's own class selection)"""
    from scvx_hip import _lib
    fn = _lib.lib().scvx_qp_workspace_bytes
    fn.restype = ctypes.c_size_t
    tpl = build(name, K)[2].to_c()
    return int(fn(ctypes.byref(tpl), ctypes.c_int(1)))


def run(cuda, name, K):
    """The case's Jacobi loop from the scenario's initial iterate: step 0 cold, the later ones warm from the previous
    step's primal-dual point.  Returns every step's outputs (numpy, keys_of(name))."""
    import torch
    import scvx_hip
    model, sc, spec, R, trv = build(name, K)
    N = sc["X"].shape[0]
    t = lambda x: ic._t(x, cuda)
    X, U, sig = t(sc["X"]), t(sc["U"]), t(sc["sigma"])
    xi, xf, tr = t(sc["x_init"]), t(sc["x_final"]), t(np.full(N, trv))
    solver = scvx_hip.QPSolver(spec, N, device=cuda)
    warm, steps = None, []
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
    return steps


def golden_key(name, K, step, key):
    return f"{name}/K{K}/{step}/{key}"


def pack(name, K, step, st, last):
    """the golden file's entries of one step's outputs: the big arrays in full for the last step only, their SHA-256
    over the raw bytes for every step"""
    out = {}
    for k in keys_of(name):
        v = st[k].astype(np.float64) if st[k].dtype.kind == "f" else st[k]
        if k in BIG:
            out[golden_key(name, K, step, k) + ".sha256"] = ic.digest(v)
        if k not in BIG or last:
            out[golden_key(name, K, step, k)] = v
    return out
