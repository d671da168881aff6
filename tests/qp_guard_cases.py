"""The Jacobi fixtures of tests/test_qp_guards_gpu.py and of its golden generator (tests/golden/make_qp_guard_goldens.py):
one cold and two warm steps of 8 agents per case (tests/qp_insn_cases.py's loop), at the shapes where a lane mask of the
QP kernel's row loops (DESIGN §3.3 "Lane guards and spill reloads") can go wrong and that the goldens of
qp_insn_cases (K = 50, 12) and qp_factor_cases (K = 13, 14) do not reach.

Cases (name, K, the instantiation the host must take: 0 runtime K and flags, 1 K at compile time with runtime flags):
    c3 K = 64            no idle lane; the row mask (t < K - 1) is false in lane 63 only
    c3 K = 63            one idle lane
    c3 K = 12            52 idle lanes, whose out-of-range zeros give inf / NaN in any unguarded reciprocal (the anchor:
                         qp_insn_cases records the same case)
    c3_ineql K = 50, 13  ineq_last: the row mask becomes t < K.  At K = 50 the flags no longer match the compiled ones,
                         so the host must fall to the runtime-flag instantiation (1)
    c3_freeu K = 13      fix_last_input = False (the last input weighted like the others, w_last = 1: with the
                         reference's w_last = 0 the last node's input Hessian is singular)
    c3_obs3 K = 13       3 of the 8 obstacles and no box: the wave-uniform r < n_obs, n_box = 0 guards
    c2 K = 63            no soft rows: the class's one dummy slack group
    c4 K = 63            2^3 lattice, R = 2.3: a per-lane collision row count, whose predicate is not the row mask
                         (lattice seed 3: with qp_insn_cases' seed 2 two of the eight agents end their cold start at
                         K = 63 with a numerical failure)
K >= 2 n everywhere, which the warm start needs.

Every case runs a runtime-flag instantiation (0 or 1).  The one-mask form is compiled only into the flag-specialised
K = 50 instantiations, which tests/test_qp_insn_gpu.py pins bit for bit (its "flags" goldens of c2 / c3 / c4); the cases
here pin the runtime-flag kernels at the shapes where the form would go wrong, for the day it is compiled into them."""
import numpy as np

import qp_insn_cases as ic

STEPS = ic.STEPS
KEYS = tuple(k for k in ic.KEYS if k != "nu")      # no virtual-control class here
BIG = ic.BIG
N_AGENTS = 8
TR = 0.25
GENERIC, KSPEC = 0, 1
CASES = (("c3", 64, GENERIC), ("c3", 63, GENERIC), ("c3", 12, GENERIC), ("c3_ineql", 50, KSPEC),
         ("c3_ineql", 13, GENERIC), ("c3_freeu", 13, GENERIC), ("c3_obs3", 13, GENERIC), ("c2", 63, GENERIC),
         ("c4", 63, GENERIC))


def build(name, K):
    """-> (model, scenario arrays, QPSpec, coupling radius or None)"""
    import scvx_hip
    from scvx_hip import workloads
    if name in ("c3", "c2"):
        return ic.build(name, K)
    if name == "c4":
        sc = workloads.synthetic_lattice(side=2, K=K, seed=3)
        spec = scvx_hip.QPSpec(model="di", K=K, box=ic.BOX, obs=[], w_obs=1e6, j_max=8, w_coll=1e4, tol=1e-8,
                               max_iter=60)
        return "di", sc, spec, 2.3
    sc = workloads.synthetic_di(N_AGENTS, K=K, seed=1, obstacles=8)
    kw = dict(model="di", K=K, box=ic.BOX, obs=sc["obs"], w_obs=1e6, u_max=1.0, tol=1e-8, max_iter=60)
    if name == "c3_ineql":
        kw["ineq_last"] = True
    elif name == "c3_freeu":
        kw.update(fix_last_input=False, w_last=1.0)
    elif name == "c3_obs3":
        kw.update(obs=sc["obs"][:3], box=[])
    else:
        raise KeyError(name)
    return "di", sc, scvx_hip.QPSpec(**kw), None


def instantiation(name, K):
    """the instantiation the library takes for the case's template (scvx_qp_instantiation)"""
    import ctypes
    from scvx_hip import _lib
    tpl = build(name, K)[2].to_c()
    return int(_lib.lib().scvx_qp_instantiation(ctypes.byref(tpl)))


def run(cuda, name, K):
    """The case's Jacobi loop from the scenario's initial iterate: step 0 cold, the later ones warm from the previous
    step's primal-dual point.  Returns every step's outputs (numpy, KEYS)."""
    import torch
    import scvx_hip
    model, sc, spec, R = build(name, K)
    N = sc["X"].shape[0]
    t = lambda x: ic._t(x, cuda)
    X, U, sig = t(sc["X"]), t(sc["U"]), t(sc["sigma"])
    xi, xf, tr = t(sc["x_init"]), t(sc["x_final"]), t(np.full(N, TR))
    solver = scvx_hip.QPSolver(spec, N, device=cuda)
    warm, steps = None, []
    for _ in range(STEPS):
        disc = scvx_hip.foh_batched(model, X, U, sig)
        rows = cnt = None
        if R is not None:
            rows, cnt = scvx_hip.collision_rows(X, 0, N, R, j_max=spec.j_max)
        out = solver.solve(disc, sig, X, U, xi, xf, tr, rows, cnt, warm=warm)
        torch.cuda.synchronize()
        steps.append({k: out[k].cpu().numpy().copy() for k in KEYS})
        X, U = out["X"].clone(), out["U"].clone()
        warm = (out["status"] == 0).to(torch.int32)
    return steps


def golden_key(name, K, step, key):
    return f"{name}/K{K}/{step}/{key}"


def pack(name, K, step, st, last):
    """the golden file's entries of one step's outputs: the big arrays in full for the last step only, their SHA-256
    over the raw bytes for every step"""
    out = {}
    for k in KEYS:
        v = st[k].astype(np.float64) if st[k].dtype.kind == "f" else st[k]
        if k in BIG:
            out[golden_key(name, K, step, k) + ".sha256"] = ic.digest(v)
        if k not in BIG or last:
            out[golden_key(name, K, step, k)] = v
    return out
