"""Multi-agent trajectory analysis -- drop-in for the reference SCvx/utils/analysis.py, computed on the GPU.

Same functions and arguments, numpy in and numpy out: `min_inter_agent_distance` (:10-31),
`min_agent_obstacle_distance` (:34-62), `compute_intersample_clearance` (:64-104).  The pairwise and
obstacle minima run in scvx_pair_min_distance_batched / scvx_obstacle_min_distance_batched instead of the
reference's Python double loop; the dense roll-outs in scvx_rollout_dense_batched, or for a model that is not built
in, in its runtime-compiled form (scvx_hip.rtc.DeviceModel, scvx_rtc_rollout_dense_batched).

Added here (no reference counterpart): `min_inter_agent_separation_continuous`, the closest approach of
any two agents BETWEEN the nodes as well as at them (scvx_hip.fleet_separation), and
`min_agent_obstacle_clearance_continuous`, the same for agents against obstacles
(scvx_hip.fleet_obstacle_clearance).
"""
from typing import List, Sequence, Tuple

import numpy as np

import scvx_hip
from SCvx.discretization.first_order_hold import FirstOrderHold, device_model


def _stack(X_list, device):
    """[(n, K)] * N -> device tensor (N, K, n)."""
    import torch
    X = np.ascontiguousarray(np.stack([np.asarray(x, float).T for x in X_list]))
    return torch.as_tensor(X, dtype=torch.float64, device=device)


def min_inter_agent_distance(X_list: List[np.ndarray], device="cuda") -> Tuple[float, np.ndarray]:
    """(d_min_global, d_mat): d_mat[i, j] = min_k ||X_i[0:3, k] - X_j[0:3, k]|| (rows 0:3 of whatever state is
    given, as the reference), symmetric with a zero diagonal; d_min_global = the minimum over the strictly
    positive entries (ValueError when there are none, as numpy's empty .min())."""
    d_mat = scvx_hip.pair_min_distance(_stack(X_list, device)).cpu().numpy()
    return d_mat[d_mat > 0].min(), d_mat


def min_agent_obstacle_distance(X_list: List[np.ndarray], obstacles: Sequence, robot_radius: float,
                                device="cuda") -> Tuple[float, np.ndarray]:
    """(d_min_global, d_mat): d_mat[i, j] = min_k (||p_i(k) - c_j|| - (robot_radius + r_j)) over rows 0:3;
    d_min_global its minimum (negative when penetrating)."""
    d_mat = scvx_hip.obstacle_min_distance(_stack(X_list, device), list(obstacles), robot_radius).cpu().numpy()
    return d_mat.min(), d_mat


def compute_intersample_clearance(X: np.ndarray, U: np.ndarray, foh, obs_center: np.ndarray, obs_radius: float,
                                  robot_radius: float, margin: float, resolution: int = 50):
    """(tau_cont, h_cont, tau_disc, h_disc): obstacle clearance between and at the nodes of one trajectory.

    This is the behaviour the reference's docstring documents, not the reference's code, which cannot run (it
    calls the three-argument segment roll-out with one argument, analysis.py:90-92): per segment k the samples
    tau = k + t, t in linspace(0, 1, resolution, endpoint=False), of the roll-out from X[:, k] under the FOH input
    at sigma = 1; clearance = ||x[:len(obs_center)] - obs_center|| - (obs_radius + robot_radius + margin) on the
    first len(obs_center) states.  h_disc is the same clearance at the K nodes.

    The roll-outs are scvx_hip.rollout_dense calls on chunks of at most 16 samples (its limit): chunk c of every
    segment starts from the segment's state at its first sample (one integrate_nonlinear roll-out from the node)
    and is sampled at the trajectory's own FOH input restricted to the chunk.  Any model: a user model runs its
    DeviceModel's integrate_nonlinear and rollout_dense."""
    import torch
    X, U = np.asarray(X, float), np.asarray(U, float)
    model = getattr(foh, "_name", None) or device_model(foh.model)
    dev = getattr(foh, "_device", "cuda")
    params = getattr(foh.model, "scvx_params", None)
    user = not isinstance(model, str)   # a DeviceModel
    K, res = X.shape[1], int(resolution)
    c = np.asarray(obs_center, float).reshape(-1)
    pd = c.size
    if not 1 <= pd <= min(3, X.shape[0]) or res < 1:
        raise ValueError("compute_intersample_clearance: obs_center of 1..3 coordinates and resolution >= 1 expected")
    total_radius = obs_radius + robot_radius + margin
    dtp, nsub = foh.dt * 1.0, foh.rollout_nsub(1.0)
    x0, u0, u1 = X[:, :-1].T, U[:, :-1].T, U[:, 1:].T   # (K-1, n), (K-1, m): one virtual agent per segment

    def dev_t(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)

    pos = np.empty((K - 1, res, pd))
    for i0 in range(0, res, 16):
        cnt = min(16, res - i0)
        t0, t1 = i0 / res, (i0 + cnt) / res
        ua, ub = u0 + t0 * (u1 - u0), u0 + t1 * (u1 - u0)
        xs = x0
        if i0:   # the segments' states at t0: a one-interval roll-out over [0, t0 dt] whose end input is u(t0)
            roll = model.integrate_nonlinear if user else (lambda *a, **kw: scvx_hip.integrate_nonlinear(model, *a, **kw))
            out = roll(dev_t(np.stack([x0, x0], 1)), dev_t(np.stack([u0, ua], 1)), dev_t(np.full(K - 1, t0 * dtp)),
                       True, nsub=nsub, params=params)
            xs = out[:, 1].cpu().numpy()
        P, _ = scvx_hip.rollout_dense(model, dev_t(np.stack([xs, xs], 1)), dev_t(np.stack([ua, ub], 1)),
                                      dev_t(np.full(K - 1, (t1 - t0) * dtp)), S=cnt, nsub=nsub, pos_dim=pd,
                                      params=params)
        pos[:, i0:i0 + cnt] = P[:, 0, :cnt, :pd].cpu().numpy()
    t = np.linspace(0, 1, res, endpoint=False)
    tau_cont = (np.arange(K - 1)[:, None] + t[None, :]).reshape(-1)
    h_cont = (np.linalg.norm(pos - c, axis=2) - total_radius).reshape(-1)
    tau_disc = np.arange(K)
    h_disc = np.linalg.norm(X[:pd].T - c.reshape(1, pd), axis=1) - total_radius
    return tau_cont, h_cont, tau_disc, h_disc


def _device_model(foh_or_model, device):
    """(device model, params, device) of a FirstOrderHold, a model object, a built-in device model name or a
    scvx_hip.rtc.DeviceModel.  The device model is a built-in name or a DeviceModel (a FirstOrderHold's own; a model
    object's `scvx_device_model`, else its get_equations() re-traced: first_order_hold.device_model)."""
    if isinstance(foh_or_model, FirstOrderHold):   # resolved at its construction
        return (foh_or_model._name, getattr(foh_or_model.model, "scvx_params", None),
                getattr(foh_or_model, "_device", device))
    if isinstance(foh_or_model, str):
        return foh_or_model, None, device
    if callable(getattr(foh_or_model, "rollout_dense", None)):   # a DeviceModel: its own launch parameters
        return foh_or_model, None, device
    return device_model(foh_or_model), getattr(foh_or_model, "scvx_params", None), device


def _rollout_nsub(model, sig, K):
    """RK4 substeps of the continuous-time functions: exact at the default for the integrators, else at least 16
    (scvx_hip.integrate_nonlinear's default) and at least the FOH's count for the longest interval."""
    if isinstance(model, str) and model in ("di", "si"):
        return None
    return max(16, scvx_hip.default_nsub(model, float(sig.max()), K))


def min_agent_obstacle_clearance_continuous(X_list: List[np.ndarray], U_list: List[np.ndarray], foh_or_model, sigma,
                                            obstacles: Sequence, robot_radius: float, S: int = 8,
                                            device="cuda", pos_dim=None) -> Tuple[float, np.ndarray]:
    """min_agent_obstacle_distance in continuous time (not in the reference): (d_min_global, d_mat) with
    d_mat[i, j] = min over the whole trajectory, between the nodes as well as at them, of
    ||p_i - c_j|| - (robot_radius + r_j); d_min_global its minimum (negative when penetrating).

    X_list / U_list: per agent (n, K) / (m, K); foh_or_model: a FirstOrderHold, a model object, a built-in
    device model name or a scvx_hip.rtc.DeviceModel; sigma: one horizon for all agents or one per agent; obstacles
    [(centre, radius)], centres of up to 3 coordinates.  pos_dim: the leading states that are positions -- required
    for a model that is not built in, scvx_hip.rollout_dense's default otherwise.

    Accuracy: exact for the piecewise-linear interpolant of S samples per segment; within max ||r''|| h^2 / 8 of
    the continuous minimum, h = 1 / ((K-1) S) in normalised time and r = p - c (double integrator:
    ||r''|| <= max(sigma^2 ||u||)).  Never above min_agent_obstacle_distance's matrix: the nodes are samples."""
    import torch
    who = "min_agent_obstacle_clearance_continuous"
    model, params, device = _device_model(foh_or_model, device)
    N = len(X_list)
    if len(U_list) != N:
        raise ValueError(f"{who}: X_list and U_list must have the same length")
    sig = np.broadcast_to(np.asarray(sigma, float), (N,)).copy()
    K = np.asarray(X_list[0]).shape[1]
    out = scvx_hip.fleet_obstacle_clearance(model, _stack(X_list, device), _stack(U_list, device),
                                            torch.as_tensor(sig, device=device), list(obstacles), robot_radius, S=S,
                                            nsub=_rollout_nsub(model, sig, K), pos_dim=pos_dim, params=params)
    return out["min"], out["D"].cpu().numpy()


def min_agent_moving_obstacle_clearance_continuous(X_list: List[np.ndarray], U_list: List[np.ndarray], foh_or_model,
                                                   sigma, tracks: Sequence, robot_radius: float, S: int = 8,
                                                   device="cuda", pos_dim=None) -> Tuple[float, np.ndarray]:
    """min_agent_obstacle_clearance_continuous for obstacles that move (not in the reference): (d_min_global, d_mat)
    with d_mat[i, j] = min over agent i's whole trajectory, on its own clock, of
    ||p_i(t) - q_j(t)|| - (robot_radius + r_j); d_min_global its minimum (negative when penetrating).

    tracks [(knots, (t0, t1), radius)]: track j has n >= 1 knots of up to 3 coordinates equally spaced over the
    real-time window [t0, t1]; it waits at its first knot before t0 and stops at its last after t1; one knot is a
    fixed centre (scvx_hip.obstacle_tracks).  The other arguments as min_agent_obstacle_clearance_continuous.

    Accuracy: exact for the piecewise-linear interpolant of S relative samples per segment; within
    max ||p''|| h^2 / 8 of the continuous minimum, h = 1 / ((K-1) S) in normalised time (double integrator:
    ||p''|| <= max(sigma^2 ||u||)), plus h / 4 times the track's velocity jump (per unit normalised time) for every
    knot that falls strictly inside a sub-interval (scvx_hip.moving_obstacle_scan)."""
    import torch
    who = "min_agent_moving_obstacle_clearance_continuous"
    model, params, device = _device_model(foh_or_model, device)
    N = len(X_list)
    if len(U_list) != N:
        raise ValueError(f"{who}: X_list and U_list must have the same length")
    sig = np.broadcast_to(np.asarray(sigma, float), (N,)).copy()
    K = np.asarray(X_list[0]).shape[1]
    out = scvx_hip.fleet_moving_obstacle_clearance(model, _stack(X_list, device), _stack(U_list, device),
                                                   torch.as_tensor(sig, device=device), tracks, robot_radius, S=S,
                                                   nsub=_rollout_nsub(model, sig, K), pos_dim=pos_dim, params=params)
    return out["min"], out["D"].cpu().numpy()


def min_inter_agent_separation_continuous(X_list: List[np.ndarray], U_list: List[np.ndarray], foh_or_model, sigma,
                                          S: int = 8, device="cuda", pos_dim=None):
    """Closest approach of any two agents in continuous time (not in the reference): (d_min_global, d_seg, info).

    X_list / U_list: per agent (n, K) / (m, K); foh_or_model: a FirstOrderHold, a model object, a built-in
    device model name or a scvx_hip.rtc.DeviceModel; sigma: one horizon for all agents or one per agent; pos_dim: the
    leading states that are positions -- required for a model that is not built in, scvx_hip.rollout_dense's default
    otherwise.  Agents are compared at equal normalised time.  d_seg (N, K-1): per agent and segment the minimum
    distance to any other agent over the segment; info: j (N, K-1) the other agent, tau (N, K-1) the position in the segment where it occurs,
    argmin = (i, j, k, tau) of d_min_global.

    Accuracy: exact for the piecewise-linear interpolant of S samples per segment; within max ||r''|| h^2 / 8 of
    the continuous minimum, h = 1 / ((K-1) S) in normalised time and r the relative position (double integrator:
    ||r''|| <= 2 max(sigma^2 ||u||))."""
    import torch
    model, params, device = _device_model(foh_or_model, device)
    N = len(X_list)
    if len(U_list) != N:
        raise ValueError("min_inter_agent_separation_continuous: X_list and U_list must have the same length")
    sig = np.broadcast_to(np.asarray(sigma, float), (N,)).copy()
    K = np.asarray(X_list[0]).shape[1]
    out = scvx_hip.fleet_separation(model, _stack(X_list, device), _stack(U_list, device),
                                    torch.as_tensor(sig, device=device), S=S, nsub=_rollout_nsub(model, sig, K),
                                    pos_dim=pos_dim, params=params)
    info = dict(j=out["j"].cpu().numpy(), tau=out["tau"].cpu().numpy(), argmin=out["argmin"])
    return out["min"], out["sep"].cpu().numpy(), info
