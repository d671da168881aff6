"""The fixtures of tests/test_rollout_bitwise_gpu.py and of its golden generator
(tests/golden/make_rollout_parent_goldens.py): every kernel that advances a state by the FOH-input RK4 step
(foh_body.hpp rk4_step), on small fixed-seed inputs.

Shapes: 5 agents with K = 4 (15 segments: no multiple of a wave or a block) and one agent with K = 2 (a single segment,
a single live lane).  Models: the four built-in ones and tests/custom_models.CartPole through hipRTC.  Per model and
shape:
    foh                  foh_batched / DeviceModel.foh (its augmented RK4 does not use the step: a guard)
    nl/{pw,full}/{1,3}   integrate_nonlinear, piecewise and full, 1 and 3 substeps
    dense/S/nsub/{P,L}   rollout_dense at (S, nsub) = (1, 1), (3, 7), (16, 16); built-in models only
    is/*                 intersample_batched: two obstacles, 12 samples, at most 4 minima per slot; n_crit, and the
                         entries below it of t_crit, h0, grad_x, grad_u (the rest zeroed here)"""
import numpy as np

SEED = 7031
SHAPES = ((5, 4), (1, 2))                      # (N, K)
MODELS = ("di", "unicycle", "si", "quad", "cartpole")
FOH_NSUB = 4
NL = ((True, 1), (True, 3), (False, 1), (False, 3))   # (piecewise, nsub)
DENSE = ((1, 1), (3, 7), (16, 16))                    # (S, nsub)
IS_NSUB, IS_SAMPLES, IS_MAX_CRIT = 3, 12, 4
IS_KEYS = ("n_crit", "t_crit", "h0", "grad_x", "grad_u")


def dims(model):
    import scvx_hip
    return (4, 1) if model == "cartpole" else scvx_hip.MODEL_DIMS[model]


def inputs(model, N, K):
    """X (N,K,n), U (N,K,m), sigma (N,): moderate states and inputs (the quadrotor's attitudes stay far from the
    Euler singularity), segments of 1/3 .. 1 time units"""
    n, m = dims(model)
    rng = np.random.default_rng([SEED, MODELS.index(model), N, K])
    return rng.normal(0.0, 0.4, (N, K, n)), rng.normal(0.0, 0.4, (N, K, m)), rng.uniform(1.0, 3.0, N)


def obstacles(model):
    """Two obstacles in the model's position rows, inside the cloud of start states so that roll-outs pass them"""
    pd = 2 if model in ("unicycle", "cartpole") else 3
    return [(np.array([0.1, -0.05, 0.15][:pd]), 0.05), (np.array([-0.2, 0.15, -0.1][:pd]), 0.1)]


def device_model():
    """CartPole with its parameters as launch params (one hipRTC compile per process: DeviceModel caches by source)"""
    import custom_models as cm
    from scvx_hip.rtc import DeviceModel
    mdl = cm.CartPole()
    return DeviceModel.from_sympy(mdl.x_sym, mdl.u_sym, mdl.f_param, p_syms=mdl.p_sym, params=list(mdl.params.values()))


def key(model, N, K):
    return f"{model}/N{N}K{K}"


def pack(out):
    """One float64 vector per model and shape: run()'s arrays raveled in the order of their sorted names (n_crit is
    exact in float64).  A golden of ~150 separate arrays spends a third of its size on headers."""
    return np.concatenate([out[k].astype(np.float64).ravel() for k in sorted(out)])


def run(cuda, model, N, K):
    """-> {name: numpy array} of every recorded output of one model and shape"""
    import torch
    import scvx_hip
    Xn, Un, sn = inputs(model, N, K)
    X, U, sig = (torch.tensor(a, dtype=torch.float64, device=cuda) for a in (Xn, Un, sn))
    dm = device_model() if model == "cartpole" else None
    out = {}
    out["foh"] = (dm.foh(X, U, sig, nsub=FOH_NSUB) if dm else scvx_hip.foh_batched(model, X, U, sig, nsub=FOH_NSUB))
    for pw, nsub in NL:
        out[f"nl/{'pw' if pw else 'full'}/{nsub}"] = (dm.integrate_nonlinear(X, U, sig, pw, nsub=nsub) if dm else
                                                      scvx_hip.integrate_nonlinear(model, X, U, sig, pw, nsub=nsub))
    if dm is None:
        for S, nsub in DENSE:
            out[f"dense/{S}/{nsub}/P"], out[f"dense/{S}/{nsub}/L"] = scvx_hip.rollout_dense(model, X, U, sig, S=S, nsub=nsub)
    res = scvx_hip.intersample_batched(dm or model, X, U, sig, obstacles(model), num_samples=IS_SAMPLES,
                                       max_crit=IS_MAX_CRIT, nsub=IS_NSUB)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    nc = res["n_crit"].cpu().numpy()
    live = np.arange(IS_MAX_CRIT)[None, None, None, :] < nc[..., None]   # (N, K-1, O, max_crit)
    out["is/n_crit"] = nc
    for k in IS_KEYS[1:]:
        v = res[k].cpu().numpy()
        out[f"is/{k}"] = np.where(live if v.ndim == 4 else live[..., None], v, 0.0)
    return out
