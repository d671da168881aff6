"""scvx_hip -- MI355X-native batched SCvx inner loop (host side of libscvx_hip.so).

Thin PyTorch-ROCm layer over the C-ABI in include/scvx_hip.h: tensors are device buffers,
kernels run on torch's current HIP stream, nothing falls back to the CPU.

    foh_batched            FirstOrderHold.calculate_discretization for N agents
                           (SCvx/discretization/first_order_hold.py:52-87)
    integrate_nonlinear    FirstOrderHold.integrate_nonlinear_piecewise / _full (:127-155)
    collision_rows         linearized pairwise collision rows (Distributed_opt/dist_scvx_3d.py:93-107)
    collision_check        every reference collision row evaluated at a (culled) solution
    qp_solve_batched       the per-agent trust-region subproblem (dist_scvx_3d.py:51-111)
    QPSpec                 problem template of qp_solve_batched
    SCPSpec / SCPSolver    the SCvx convex subproblem SCProblem (+ AgentSolver ADMM terms)
                           (SCvx/optimization/sc_problem.py:15-83, agent_solver.py:78-102)
    fleet_separation       continuous-time closest approach of every agent to every other (rollout_dense +
                           separation_scan; no reference counterpart)
    intersample_pair_rows  the same scan as QP rows: per (agent, segment) the neighbours that pass too close between
    append_collision_rows  two nodes, appended to collision_rows' node rows (CouplingSpec.intersample_S)
    fleet_obstacle_clearance  continuous-time closest approach of every agent to every obstacle (rollout_dense +
    obstacle_scan          obstacle_scan); the scan's records are the obstacle rows of ObstacleRowsSpec
    pair_min_distance      node-level pairwise / agent-obstacle minimum distances
    obstacle_min_distance  (SCvx/utils/analysis.py:10-62)
"""
import ctypes
import math
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

from . import _lib
from ._lib import MODEL_DIMS, MODEL_IDS, STATUS, QPTemplate, SCPTemplate, ScvxError, check, lib

# RK4 substeps per FOH interval: the smallest count that keeps each model within 1e-7 of the reference's LSODA
# goldens (tests/test_foh_gpu.py, tests/test_foh_oracle.py).  1 is exact for the (linear) integrators; the
# quadrotor holds at 10 (round 5, oracle/foh_ref.c on tests/golden/foh_quad_K50_s5.npz: max relative error 1.2e-7 at
# 8, 7.7e-8 at 9, 5.2e-8 at 10, 9e-10 at 16), the unicycle keeps 16.
DEFAULT_NSUB = {"di": 1, "si": 1, "unicycle": 16, "quad": 10}
# ... at the golden's interval T_pin = sigma / (K - 1).  The RK4 error grows with the interval (the quadrotor at
# sigma = 30, K = 50, six times the golden's interval: 3.8e-6 at 10 substeps, 5.7e-7 at 16, against 256 substeps), so
# for longer intervals the count scales as DEFAULT_NSUB * (T / T_pin)^0.75: the RK4 self-convergence test
# (tests/test_foh_oracle.py: K 30..100, sigma 2..45, attitudes to 0.6 rad) holds 1e-7 with it; C5 (sigma 30, K 50)
# runs 39.  (model: (T_pin, exponent))
NSUB_SCALE = {"quad": (5.0 / 49.0, 0.75)}
QUAD_PARAMS = (1.0, 9.81, 0.02, 0.02, 0.04)

__all__ = ["model_dims", "model_id", "default_nsub", "foh_batched", "jacobi_update", "jacobi_update_global", "integrate_nonlinear", "collision_rows", "collision_check", "qp_solve_batched", "QPSpec", "SCPSpec", "SCPSolver", "slab_update",
           "intersample_batched", "rollout_dense", "separation_scan", "fleet_separation", "pair_min_distance",
           "obstacle_min_distance", "intersample_pair_rows", "append_collision_rows", "obstacle_scan",
           "fleet_obstacle_clearance",
           "disc_stride", "unpack_disc", "ScvxError", "MODEL_DIMS", "DEFAULT_NSUB"]


def _torch():
    import torch
    return torch


def _stream(stream=None):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _dev(t, dtype=None, name="tensor"):
    torch = _torch()
    dtype = dtype or torch.float64
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor on the ROCm device")
    if not t.is_cuda:
        raise ScvxError(f"{name} must live on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def model_dims(model):
    """(n_x, n_u) of a built-in model name or of a runtime-compiled model (scvx_hip.rtc.DeviceModel, `.dims`)."""
    if isinstance(model, str):
        return MODEL_DIMS[model]
    dims = getattr(model, "dims", None)
    if dims is None:
        raise TypeError(f"model must be a built-in name {sorted(MODEL_DIMS)} or a scvx_hip.rtc.DeviceModel")
    return tuple(dims)


def model_id(model):
    """The template's model_id: the built-in id, or SCVX_MODEL_RUNTIME for a runtime-compiled model (the QP and
    SCP kernels are then instantiated for its dimensions at the first solve)."""
    return MODEL_IDS[model] if isinstance(model, str) else _lib.SCVX_MODEL_RUNTIME


def default_nsub(model, sigma=None, K=None):
    """RK4 substeps of the FOH: the built-in table (a user model: its DeviceModel.nsub, 16 by default); with the
    interval known (sigma, K), a model in NSUB_SCALE gets DEFAULT_NSUB * (T / T_pin)^p for intervals T = sigma / (K-1)
    longer than its pinned T_pin (never fewer than the table)."""
    if not isinstance(model, str):
        return int(getattr(model, "nsub", 16))
    base = DEFAULT_NSUB[model]
    if sigma is None or K is None or model not in NSUB_SCALE:
        return base
    t_pin, p = NSUB_SCALE[model]
    T = float(sigma) / (int(K) - 1)
    return max(base, int(math.ceil(base * (T / t_pin) ** p - 1e-9)))


def _auto_nsub(model, sigma, K):
    """default_nsub for a device sigma batch: the longest interval of the batch (one host read of max(sigma), only
    for the models whose count depends on the interval)."""
    if isinstance(model, str) and model not in NSUB_SCALE:
        return DEFAULT_NSUB[model]
    if not isinstance(model, str):
        return default_nsub(model)
    return default_nsub(model, float(sigma.max().item()) if sigma.numel() else 0.0, K)


def _nsub(who, nsub, default):
    """The RK4 substep count of a launch: `nsub` as given (an error below 1; 0 is no request for the default), or for
    None what default() returns (a call, since _auto_nsub may read the device)."""
    if nsub is None:
        return int(default())
    if int(nsub) < 1:
        raise ValueError(f"{who}: nsub >= 1 required, got {nsub}")
    return int(nsub)


def disc_stride(model):
    n, m = model_dims(model)
    return n * (n + 2 * m + 2)


def unpack_disc(disc, model):
    """[..., K-1, n(n+2m+2)] -> (A_bar, B_bar, C_bar, S_bar, z_bar) in the reference's F-order
    column layout (..., n*n, K-1) etc. (first_order_hold.py:20-24, 75-85)."""
    n, m = model_dims(model)
    o = [0, n * n, n * n + n * m, n * n + 2 * n * m, n * n + 2 * n * m + n, n * n + 2 * n * m + 2 * n]
    return tuple(disc[..., o[i]:o[i + 1]].transpose(-1, -2) for i in range(5))


def _params(model, params):
    torch = _torch()
    if model != "quad":
        return None, ctypes.c_void_p(0)
    p = torch.tensor(params if params is not None else QUAD_PARAMS, dtype=torch.float64)
    buf = (ctypes.c_double * 5)(*p.tolist())
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _check_xus(who, model, X, U, sigma):
    """The (X, U, sigma) batch of a model (built-in name or DeviceModel) as every model-templated kernel indexes it:
    X (N,K,n), U (N,K,m), sigma (N,).  Returns (N, K, n, m)."""
    n, m = model_dims(model)
    shp = tuple(X.shape)
    if len(shp) != 3 or shp[2] != n or tuple(U.shape) != (shp[0], shp[1], m) or tuple(sigma.shape) != (shp[0],):
        raise ValueError(f"{who}: X (N,K,{n}), U (N,K,{m}) and sigma (N,) expected; got {shp}, {tuple(U.shape)}, "
                         f"{tuple(sigma.shape)}")
    return shp[0], shp[1], n, m


def _fill_obstacles(t, obstacles, rows=None):
    """n_obs, obs_center, obs_radius of a template (QP, SCP, inter-sample; the caller has checked the count) from
    [(centre, radius)].  rows: the length every centre must have."""
    t.n_obs = len(obstacles)
    for o, (c, r) in enumerate(obstacles):
        if rows is not None and len(c) != rows:
            raise ValueError("obstacle centres must match the projection rows")
        for i in range(len(c)):
            t.obs_center[o][i] = float(c[i])
        t.obs_radius[o] = float(r)


def foh_batched(model, X, U, sigma, nsub=None, params=None, out=None, stream=None):
    """X (N,K,n), U (N,K,m), sigma (N,) float64 device tensors -> disc (N,K-1,n(n+2m+2)).  nsub None: default_nsub
    for the batch's longest interval (for the quadrotor this reads max(sigma) on the host; pass nsub to avoid it)."""
    torch = _torch()
    N, K, n, m = _check_xus("foh_batched", model, X, U, sigma)
    if K < 2:
        raise ValueError("foh_batched: K >= 2 required")
    nsub = _nsub("foh_batched", nsub, lambda: _auto_nsub(model, sigma, K))
    if out is None:
        out = torch.empty((N, K - 1, disc_stride(model)), dtype=torch.float64, device=X.device)
    if N == 0:      # nothing to launch (an empty tensor has no device pointer for the C-ABI's null checks)
        return out
    keep, pp = _params(model, params)
    rc = lib().scvx_foh_batched(MODEL_IDS[model], pp, K, N, _dev(X, name="X"), _dev(U, name="U"),
                                _dev(sigma, name="sigma"), nsub, _dev(out, name="out"), _stream(stream))
    check(rc, "scvx_foh_batched")
    return out


def integrate_nonlinear(model, X, U, sigma, piecewise, nsub=16, params=None, out=None, stream=None):
    """Batched FirstOrderHold.integrate_nonlinear_piecewise (piecewise=True) / _full (False)."""
    torch = _torch()
    N, K, n, m = _check_xus("integrate_nonlinear", model, X, U, sigma)
    if K < 2:
        raise ValueError("integrate_nonlinear: K >= 2 required")
    nsub = _nsub("integrate_nonlinear", nsub, lambda: 16)
    if out is None:
        out = torch.empty_like(X)
    if N == 0:
        return out
    keep, pp = _params(model, params)
    rc = lib().scvx_integrate_nonlinear_batched(MODEL_IDS[model], pp, K, N, _dev(X, name="X"), _dev(U, name="U"),
                                                _dev(sigma, name="sigma"), nsub, int(bool(piecewise)),
                                                _dev(out, name="out"), _stream(stream))
    check(rc, "scvx_integrate_nonlinear_batched")
    return out


def collision_rows(X_all, i0, n_local, R, j_max, pos_dim=3, cull_radius=0.0, rows=None, count=None, stream=None):
    """Rows (g, b) of dist_scvx_3d.py:93-107 for local agents [i0, i0+n_local) of X_all (N_total,K,n)."""
    torch = _torch()
    N_total, K, n = X_all.shape
    if rows is None:
        rows = torch.zeros((n_local, K, j_max, pos_dim + 1), dtype=torch.float64, device=X_all.device)
    if count is None:
        count = torch.zeros((n_local, K), dtype=torch.int32, device=X_all.device)
    rc = lib().scvx_collision_rows_batched(K, pos_dim, n, N_total, _dev(X_all, name="X_all"), int(i0), int(n_local),
                                           float(R), float(cull_radius), int(j_max), _dev(rows, name="rows"),
                                           _dev(count, torch.int32, "count"), _stream(stream))
    check(rc, "scvx_collision_rows_batched")
    return rows, count


def collision_rows_indexed(X_all, idx, R, j_max, pos_dim=3, cull_radius=0.0, rows=None, count=None, stream=None):
    """Rows of dist_scvx_3d.py:93-107 for the agents idx (device int32, distinct, in [0, N_total)) of X_all
    (scvx_collision_rows_indexed): rows [len(idx)][K][j_max][pos_dim+1], count [len(idx)][K]; rows / count
    may be larger buffers whose leading len(idx) entries are written."""
    torch = _torch()
    N_total, K, n = X_all.shape
    n_sel = int(idx.shape[0])
    if rows is None:
        rows = torch.zeros((n_sel, K, j_max, pos_dim + 1), dtype=torch.float64, device=X_all.device)
    if count is None:
        count = torch.zeros((n_sel, K), dtype=torch.int32, device=X_all.device)
    if rows.shape[0] < n_sel or tuple(rows.shape[1:]) != (K, j_max, pos_dim + 1) or count.shape[0] < n_sel:
        raise ValueError("collision_rows_indexed: rows / count too small")
    rc = lib().scvx_collision_rows_indexed(K, pos_dim, n, N_total, _dev(X_all, name="X_all"), _dev(idx, torch.int32, "idx"),
                                           n_sel, float(R), float(cull_radius), int(j_max), _dev(rows, name="rows"),
                                           _dev(count, torch.int32, "count"), _stream(stream))
    check(rc, "scvx_collision_rows_indexed")
    return rows, count


def collision_check(X_all, i0, X_new, slack, R, pos_dim=3, tol=1e-7, viol=None, vmax=None, stream=None):
    """Evaluate EVERY reference collision row (dist_scvx_3d.py:93-107) of local agents
    [i0, i0+N_local) at a solution X_new (N_local,K,n) with shared slacks slack (N_local,K), linearised
    at X_all (N_total,K,n).  Returns device tensors viol (N_local,K) int32 = rows violated by more
    than tol, vmax (N_local,K) = largest row value (scvx_collision_check_batched)."""
    torch = _torch()
    N_total, K, n = X_all.shape
    n_local = X_new.shape[0]
    if tuple(X_new.shape) != (n_local, K, n) or tuple(slack.shape) != (n_local, K):
        raise ValueError("collision_check: X_new (N_local,K,n) and slack (N_local,K) expected")
    if viol is None:
        viol = torch.empty((n_local, K), dtype=torch.int32, device=X_all.device)
    if vmax is None:
        vmax = torch.empty((n_local, K), dtype=torch.float64, device=X_all.device)
    rc = lib().scvx_collision_check_batched(K, pos_dim, n, N_total, _dev(X_all, name="X_all"), int(i0), int(n_local),
                                            float(R), _dev(X_new, name="X_new"), _dev(slack, name="slack"), float(tol),
                                            _dev(viol, torch.int32, "viol"), _dev(vmax, name="vmax"), _stream(stream))
    check(rc, "scvx_collision_check_batched")
    return viol, vmax


@dataclass
class QPSpec:
    """Template of the batched trust-region subproblem (include/scvx_hip.h scvx_qp_template)."""
    model: str = "di"
    K: int = 50
    pos_dim: int = 3
    has_final: bool = True
    fix_last_input: bool = True
    ineq_last: bool = False
    w_last: float = 0.0
    box: Sequence[Tuple[int, float, float]] = ()
    obs: Sequence[Tuple[Sequence[float], float]] = ()
    w_obs: float = 1e6
    j_max: int = 0
    w_coll: float = 1e4
    u_max: Optional[float] = None
    max_iter: int = 60
    # relative stopping tolerance (primal / dual residual and gap); 1e-8 is Clarabel's default
    # (tol_feas = tol_gap_rel = tol_gap_abs = 1e-8), the solver dist_scvx_3d.py:110 calls
    tol: float = 1e-8
    # soft terminal state (build-side option for nonlinear models; the reference's subproblem has the
    # hard row d_{T-1} + x_{T-1} == x_des): with has_final=False and w_final > 0 the objective gains
    # w_final ||x_{K-1} - x_final||^2, so the subproblem stays feasible whatever the linearisation
    w_final: float = 0.0
    # virtual control (the SCvx subproblem form of SCvx/optimization/sc_problem.py:60-68, build-side option for
    # nonlinear models under the Jacobi update): nu_t in every dynamics row, + w_nu sum_t ||nu_t||_1; the
    # subproblem is then feasible for any linearisation point.  Quadrotor (and one DI) classes only.
    w_nu: float = 0.0
    # proximal term w_prox sum_t ||x_t - xbar_t||^2: a soft trust region on the states (the hard trust region
    # of dist_scvx_3d.py:84 bounds the inputs only)
    w_prox: float = 0.0

    def to_c(self):
        n, m = model_dims(self.model)
        if self.w_final < 0 or (self.w_final > 0 and self.has_final):
            raise ValueError("QPSpec: w_final > 0 (soft terminal) needs has_final=False")
        t = QPTemplate()
        t.model_id, t.n_x, t.n_u, t.K, t.pos_dim = model_id(self.model), n, m, self.K, self.pos_dim
        t.has_final, t.fix_last_input, t.ineq_last = int(self.has_final), int(self.fix_last_input), int(self.ineq_last)
        t.w_last = self.w_last
        if len(self.box) > _lib.SCVX_MAX_BOX or len(self.obs) > _lib.SCVX_MAX_OBS:
            raise ValueError("too many box constraints / obstacles")
        t.n_box = len(self.box)
        for i, (bi, lo, hi) in enumerate(self.box):
            t.box_idx[i], t.box_lo[i], t.box_hi[i] = int(bi), float(lo), float(hi)
        _fill_obstacles(t, self.obs)
        t.w_obs, t.j_max, t.w_coll = float(self.w_obs), int(self.j_max), float(self.w_coll)
        t.has_soc = int(self.u_max is not None)
        t.u_max = 0.0 if self.u_max is None else float(self.u_max)
        t.max_iter, t.tol = int(self.max_iter), float(self.tol)
        t.w_final = float(self.w_final)
        if self.w_nu < 0 or self.w_prox < 0:
            raise ValueError("QPSpec: w_nu and w_prox must be >= 0")
        t.w_nu, t.w_prox = float(self.w_nu), float(self.w_prox)
        return t


class QPSolver:
    """Reusable batched solver: holds the C template and a device workspace for N agents."""

    def __init__(self, spec: QPSpec, N: int, device="cuda"):
        torch = _torch()
        self.spec, self.N = spec, N
        self.ctpl = spec.to_c()
        nbytes = lib().scvx_qp_workspace_bytes(ctypes.byref(self.ctpl), N)
        self.workspace = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)
        n, m = model_dims(spec.model)
        K = spec.K
        self.X = torch.empty((N, K, n), dtype=torch.float64, device=device)
        self.U = torch.empty((N, K, m), dtype=torch.float64, device=device)
        self.slack = torch.empty((N, K), dtype=torch.float64, device=device)
        self.nu = torch.zeros((N, K - 1, n), dtype=torch.float64, device=device)   # zeros unless w_nu > 0
        self.obj = torch.empty(N, dtype=torch.float64, device=device)
        self.status = torch.empty(N, dtype=torch.int32, device=device)
        self.iters = torch.empty(N, dtype=torch.int32, device=device)
        self._dummy = torch.zeros(1, dtype=torch.float64, device=device)
        self._dummy_i = torch.zeros(1, dtype=torch.int32, device=device)
        # slots [0, _state_n) hold a solve's primal-dual state (solve(n=...) always fills a leading prefix):
        # a warm flag on any other slot would start the IPM from uninitialised workspace, so it is cleared
        self._state_n = 0
        self._order_tail = self._order_bulk = None   # dispatch_lists' buffers
        self.last_entry = None

    def _check_shapes(self, disc, sigma, Xref, Uref, x_init, x_final, tr, coll_rows, coll_count, N=None):
        """Host-side shape checks: the kernel indexes every buffer with the template's compile-time
        dimensions, so a mis-shaped tensor would be read out of bounds on the device."""
        spec, N = self.spec, (self.N if N is None else N)
        n, m = model_dims(spec.model)
        K = spec.K
        want = {"disc": (disc, (N, K - 1, disc_stride(spec.model))), "sigma": (sigma, (N,)),
                "Xref": (Xref, (N, K, n)), "Uref": (Uref, (N, K, m)), "x_init": (x_init, (N, n)),
                "tr": (tr, (N,))}
        if spec.has_final or spec.w_final > 0:
            if x_final is None:
                raise ValueError("QPSolver.solve: the template has a terminal condition; x_final is required")
            want["x_final"] = (x_final, (N, n))
        if spec.j_max > 0:
            if coll_rows is None or coll_count is None:
                raise ValueError(f"QPSolver.solve: spec.j_max={spec.j_max} needs coll_rows and coll_count "
                                 "(scvx_hip.collision_rows)")
            want["coll_rows"] = (coll_rows, (N, K, spec.j_max, spec.pos_dim + 1))
            want["coll_count"] = (coll_count, (N, K))
        for name, (t, shp) in want.items():
            if tuple(t.shape) != shp:
                raise ValueError(f"QPSolver.solve: {name} has shape {tuple(t.shape)}, expected {shp}")

    supports_order = True
    supports_split = True

    def dispatch_lists(self, thr, T, short_per_tail=0, stream=None):
        """The dispatch lists of the next solve from the IPM iteration counts this solver's last full solve left in
        its `iters` buffer (scvx_qp_dispatch_select: one launch, no host sync): (order_tail (T,), order_bulk (N,)),
        int32 device tensors reused by every call.  The agents sorted longest-first (stable); the first
        min(T, #{iters >= thr}) go to the tail list -- with short_per_tail > 0 at most #{iters < thr} /
        short_per_tail of them: the bulk workgroups each tail workgroup displaces must be short solves -- the rest
        to the bulk list, unused entries are _lib.SCVX_QP_ORDER_SKIP.  T = 0: (None, the whole sort) -- the order of
        solve(order=...)."""
        torch = _torch()
        T = int(T)
        if not 0 <= T <= self.N:
            raise ValueError(f"QPSolver.dispatch_lists: T={T} outside [0, {self.N}]")
        if self._state_n < self.N:
            raise ValueError("QPSolver.dispatch_lists: no full solve yet (the iteration counts are not set)")
        if self._order_bulk is None:
            self._order_bulk = torch.empty(self.N, dtype=torch.int32, device=self.iters.device)
        if T > 0 and (self._order_tail is None or self._order_tail.numel() != T):
            self._order_tail = torch.empty(T, dtype=torch.int32, device=self.iters.device)
        tail = self._order_tail if T > 0 else None
        rc = lib().scvx_qp_dispatch_select(self.N, _dev(self.iters, torch.int32), int(thr), T, int(short_per_tail),
                                           int(self.spec.max_iter),
                                           _dev(tail, torch.int32) if T > 0 else None,
                                           _dev(self._order_bulk, torch.int32), _stream(stream))
        check(rc, "scvx_qp_dispatch_select")
        return tail, self._order_bulk

    def solve(self, disc, sigma, Xref, Uref, x_init, x_final, tr, coll_rows=None, coll_count=None, stream=None, n=None,
              warm=None, order=None, order_tail=None, reserve="whole"):
        """n (<= N): solve only n agents (the inputs' leading dimension); the outputs are the leading n rows
        of the solver's buffers.  warm (N,) int32 device tensor or None: agents with warm != 0 start from the
        primal-dual point of their previous solve by THIS solver (the same agent slot), e.g. the previous
        SCvx iteration's status == 0.  order (n,) int32 device tensor or None: the dispatch order, a
        permutation of range(n) (scvx_qp_solve_batched_ordered; results do not depend on it).  order_tail (T,)
        int32 device tensor: the split launch (scvx_qp_solve_batched_split) -- these agents in a launch of their
        own whose workgroups keep a compute unit to themselves (reserve "whole") or share it with one other
        ("half"), `order` then the bulk list (dispatch_lists gives both).  Returns dict of device tensors (views of
        reused buffers)."""
        torch = _torch()
        n = self.N if n is None else int(n)
        if not 0 <= n <= self.N:
            raise ValueError(f"QPSolver.solve: n={n} outside [0, {self.N}]")
        self._check_shapes(disc, sigma, Xref, Uref, x_init, x_final, tr, coll_rows, coll_count, N=n)
        if self.spec.j_max == 0:
            coll_rows, coll_count = self._dummy, self._dummy_i
        xf = x_final if x_final is not None else self._dummy
        if n == 0:
            return {k: v[:0] for k, v in self._outputs().items()}
        if warm is not None and tuple(warm.shape) != (n,):
            raise ValueError(f"QPSolver.solve: warm has shape {tuple(warm.shape)}, expected ({n},)")
        if warm is not None and n > self._state_n:   # slots never solved by this solver start cold
            warm = warm.clone()
            warm[self._state_n:] = 0
        if order is not None and (tuple(order.shape) != (n,) or order.dtype != torch.int32):
            raise ValueError(f"QPSolver.solve: order must be an int32 ({n},) permutation, got "
                             f"{tuple(order.shape)} {order.dtype}")
        split = ()
        if order_tail is not None:
            if order is None:
                raise ValueError("QPSolver.solve: order_tail needs order, the bulk list (dispatch_lists)")
            if order_tail.dim() != 1 or not 1 <= order_tail.numel() <= n or order_tail.dtype != torch.int32:
                raise ValueError(f"QPSolver.solve: order_tail must be an int32 (T,) list with 1 <= T <= {n}, got "
                                 f"{tuple(order_tail.shape)} {order_tail.dtype}")
            if reserve not in _lib.SCVX_QP_RESERVE:
                raise ValueError(f"QPSolver.solve: reserve must be 'whole' or 'half', not {reserve!r}")
            split = (_dev(order_tail, torch.int32, "order_tail"), int(order_tail.numel()),
                     _lib.SCVX_QP_RESERVE[reserve])
        entry = "scvx_qp_solve_batched_split" if split else "scvx_qp_solve_batched_ordered"
        rc = getattr(lib(), entry)(
            ctypes.byref(self.ctpl), n, _dev(disc, name="disc"), _dev(sigma, name="sigma"),
            _dev(Xref, name="Xref"), _dev(Uref, name="Uref"), _dev(x_init, name="x_init"), _dev(xf, name="x_final"),
            _dev(tr, name="tr"), _dev(coll_rows, name="coll_rows"), _dev(coll_count, torch.int32, "coll_count"),
            _dev(self.X), _dev(self.U), _dev(self.slack), _dev(self.nu), _dev(self.obj), _dev(self.status, torch.int32),
            _dev(self.iters, torch.int32), _dev(warm, torch.int32, "warm") if warm is not None else None,
            _dev(order, torch.int32, "order") if order is not None else None, *split,
            _dev(self.workspace), ctypes.c_size_t(self.workspace.numel() * 8), _stream(stream))
        check(rc, entry)
        self.last_entry = entry   # (diagnostics: the entry point the last solve went through)
        self._state_n = max(self._state_n, n)
        out = self._outputs()
        return out if n == self.N else {k: v[:n] for k, v in out.items()}

    def _outputs(self):
        return dict(X=self.X, U=self.U, slack_coll=self.slack, nu=self.nu, obj=self.obj, status=self.status,
                    iters=self.iters)


def qp_solve_batched(spec: QPSpec, disc, sigma, Xref, Uref, x_init, x_final, tr, coll_rows=None, coll_count=None):
    """One-shot batched solve (allocates a QPSolver); returns dict of device tensors (copies)."""
    s = QPSolver(spec, Xref.shape[0], device=Xref.device)
    out = s.solve(disc, sigma, Xref, Uref, x_init, x_final, tr, coll_rows, coll_count)
    return {k: v.clone() for k, v in out.items()}


@dataclass
class SCPSpec:
    """Template of the batched SCProblem solve (include/scvx_hip.h scvx_scp_template).  The
    constraint data come from the model (SCvx/models/*.scp_constraints())."""
    model: str = "unicycle"
    K: int = 100
    pos_dim: int = 2
    has_final: bool = True
    pin_u_first: bool = True
    pin_u_last: bool = True
    u_bounds: Sequence[Tuple[int, Optional[float], Optional[float]]] = ()
    u_soc: Optional[float] = None
    x_bounds: Sequence[Tuple[int, float, float]] = ()
    obs: Sequence[Tuple[Sequence[float], float]] = ()   # (center, total clearance r_o)
    w_nu: float = 1e4
    w_slack: float = 1e6
    w_sigma: float = 100.0
    n_nbr: int = 0
    rho: float = 0.0
    d_min: float = 1.0
    w_coll: float = 1e5
    max_iter: int = 100
    tol: float = 1e-9
    reg: float = 1e-10
    # Nash best-response terms (scvx_scp_game_solve_batched; game_model.py:68-126)
    game: bool = False
    sigma_fixed: bool = False
    w_u2: float = 0.0
    w_du: float = 0.0
    w_dth: float = 0.0
    theta_idx: int = -1
    w_in: float = 0.0
    n_slab: int = 0
    r_slab: float = 0.0
    # launch mapping of this template's solves: 0 = automatic (two waves per agent when K > 64 and the launch
    # leaves SIMDs idle), 1 or 2 forced -- per template, so concurrent callers never share it
    waves_per_agent: int = 0

    def to_c(self):
        n, m = model_dims(self.model)
        t = SCPTemplate()
        t.model_id, t.n_x, t.n_u, t.K, t.pos_dim = model_id(self.model), n, m, int(self.K), int(self.pos_dim)
        t.has_final, t.pin_u_first, t.pin_u_last = int(self.has_final), int(self.pin_u_first), int(self.pin_u_last)
        if len(self.u_bounds) > _lib.SCVX_MAX_BOX or len(self.x_bounds) > _lib.SCVX_MAX_BOX:
            raise ValueError("too many bound constraints")
        if len(self.obs) > _lib.SCVX_MAX_OBS or self.n_nbr > _lib.SCVX_MAX_NBR:
            raise ValueError("too many obstacles / neighbours")
        t.n_ubound = len(self.u_bounds)
        for b, (j, lo, hi) in enumerate(self.u_bounds):
            t.ub_idx[b] = int(j)
            t.ub_has_lo[b], t.ub_has_hi[b] = int(lo is not None), int(hi is not None)
            t.ub_lo[b] = 0.0 if lo is None else float(lo)
            t.ub_hi[b] = 0.0 if hi is None else float(hi)
        t.has_soc = int(self.u_soc is not None)
        t.u_max = 0.0 if self.u_soc is None else float(self.u_soc)
        t.n_xbound = len(self.x_bounds)
        for b, (i, lo, hi) in enumerate(self.x_bounds):
            t.xb_idx[b], t.xb_lo[b], t.xb_hi[b] = int(i), float(lo), float(hi)
        _fill_obstacles(t, self.obs)
        t.w_nu, t.w_slack, t.w_sigma = float(self.w_nu), float(self.w_slack), float(self.w_sigma)
        t.n_nbr, t.rho, t.d_min, t.w_coll = int(self.n_nbr), float(self.rho), float(self.d_min), float(self.w_coll)
        t.max_iter, t.tol, t.reg = int(self.max_iter), float(self.tol), float(self.reg)
        if self.game:
            if self.n_nbr:
                raise ValueError("game template: no ADMM neighbour terms")
            if self.n_slab > _lib.SCVX_MAX_NBR:
                raise ValueError("too many slab neighbours")
            t.game, t.sigma_fixed = 1, int(self.sigma_fixed)
            t.w_u2, t.w_du, t.w_dth, t.w_in = float(self.w_u2), float(self.w_du), float(self.w_dth), float(self.w_in)
            t.theta_idx, t.n_slab, t.r_slab = int(self.theta_idx), int(self.n_slab), float(self.r_slab)
        else:
            t.theta_idx = -1
        if self.waves_per_agent not in (0, 1, 2):
            raise ValueError("waves_per_agent must be 0, 1 or 2")
        t.waves_per_agent = int(self.waves_per_agent)
        return t


class SCPSolver:
    """Reusable batched SCProblem solver (scvx_scp_solve_batched): C template, device workspace and
    output buffers for N agents."""

    def __init__(self, spec: SCPSpec, N: int, device="cuda"):
        torch = _torch()
        self.spec, self.N = spec, N
        self.ctpl = spec.to_c()
        nbytes = lib().scvx_scp_workspace_bytes(ctypes.byref(self.ctpl), N)
        self.workspace = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)
        n, m = model_dims(spec.model)
        K, f64 = spec.K, torch.float64
        self.X = torch.empty((N, K, n), dtype=f64, device=device)
        self.U = torch.empty((N, K, m), dtype=f64, device=device)
        self.nu = torch.empty((N, K - 1, n), dtype=f64, device=device)
        self.sigma = torch.empty(N, dtype=f64, device=device)
        self.s_obs = torch.empty((N, max(len(spec.obs), 1), K), dtype=f64, device=device)
        self.s_nbr = torch.empty((N, max(spec.n_nbr, 1), K), dtype=f64, device=device)
        self.obj = torch.empty(N, dtype=f64, device=device)
        self.status = torch.empty(N, dtype=torch.int32, device=device)
        self.iters = torch.empty(N, dtype=torch.int32, device=device)
        self._dummy = torch.zeros(1, dtype=f64, device=device)

    def _call(self, entry, inputs, optional, outputs, stream):
        """Marshal one solve for the C entry point `entry`: the template and N, the seven inputs solve() and
        solve_game() share, the entry point's three optional tensors as (name, tensor or None) (None: the dummy
        buffer), its output buffers, the workspace and the stream."""
        names = ("disc", "Xref", "Uref", "sigma_ref", "tr", "x_init", "x_final")
        args = [_dev(t, name=k) for k, t in zip(names, inputs)]
        args += [_dev(self._dummy if t is None else t, name=k) for k, t in optional]
        args += [_dev(t, t.dtype) for t in outputs]
        rc = getattr(lib(), entry)(ctypes.byref(self.ctpl), self.N, *args, _dev(self.workspace),
                                   ctypes.c_size_t(self.workspace.numel() * 8), _stream(stream))
        check(rc, entry)

    def solve(self, disc, Xref, Uref, sigma_ref, tr, x_init, x_final, nbr_pos=None, nbr_Y=None, nbr_Lam=None,
              stream=None):
        """disc (N,K-1,n(n+2m+2)), Xref (N,K,n), Uref (N,K,m), sigma_ref (N,), tr (N,), x_init/x_final (N,n);
        nbr_* (N,n_nbr,K,pos_dim) when spec.n_nbr > 0.  Returns dict of device tensors (reused buffers)."""
        if self.spec.n_nbr > 0 and (nbr_pos is None or nbr_Y is None or nbr_Lam is None):
            raise ValueError("ADMM terms need nbr_pos, nbr_Y and nbr_Lam")
        self._call("scvx_scp_solve_batched", (disc, Xref, Uref, sigma_ref, tr, x_init, x_final),
                   (("nbr_pos", nbr_pos), ("nbr_Y", nbr_Y), ("nbr_Lam", nbr_Lam)),
                   (self.X, self.U, self.nu, self.sigma, self.s_obs, self.s_nbr, self.obj, self.status, self.iters),
                   stream)
        return dict(X=self.X, U=self.U, nu=self.nu, sigma=self.sigma, s_obs=self.s_obs[:, :len(self.spec.obs)],
                    s_nbr=self.s_nbr[:, :self.spec.n_nbr], obj=self.obj, status=self.status, iters=self.iters)

    def solve_game(self, disc, Xref, Uref, sigma_ref, tr, x_init, x_final, X_prev=None, slab_z=None, slab_P=None,
                   stream=None):
        """Nash best responses (scvx_scp_game_solve_batched; spec.game must be set): inputs as solve(),
        plus X_prev (N,K,n) when spec.w_in > 0 and slab_z / slab_P (N,n_slab,K,pos_dim) when
        spec.n_slab > 0.  Returns dict of device tensors (reused buffers)."""
        sp_ = self.spec
        if not sp_.game:
            raise ValueError("solve_game needs a game template (SCPSpec.game=True)")
        N, K, pd = self.N, sp_.K, sp_.pos_dim
        if sp_.w_in > 0 and (X_prev is None or tuple(X_prev.shape) != tuple(self.X.shape)):
            raise ValueError(f"X_prev {tuple(self.X.shape)} required (inertia_weight > 0)")
        if sp_.n_slab > 0:
            shp = (N, sp_.n_slab, K, pd)
            if slab_z is None or slab_P is None or tuple(slab_z.shape) != shp or tuple(slab_P.shape) != shp:
                raise ValueError(f"slab_z / slab_P {shp} required")
        self._call("scvx_scp_game_solve_batched", (disc, Xref, Uref, sigma_ref, tr, x_init, x_final),
                   (("X_prev", X_prev), ("slab_z", slab_z), ("slab_P", slab_P)),
                   (self.X, self.U, self.nu, self.sigma, self.s_obs, self.obj, self.status, self.iters), stream)
        return dict(X=self.X, U=self.U, nu=self.nu, sigma=self.sigma, s_obs=self.s_obs[:, :len(sp_.obs)],
                    obj=self.obj, status=self.status, iters=self.iters)


def slab_update(p, P, pos_dim, z=None, stream=None):
    """ACS slab normals for every (agent, neighbour, node) in one launch (scvx_slab_update_batched;
    GameUnicycleModel.update_slabs, game_model.py:54-66): z = d/||d||, d = p[a,k,:pos_dim] - P[a,j,k],
    0 where ||d|| < 1e-6.  p (N,K,n) float64, P (N,n_slab,K,pos_dim); returns z like P."""
    torch = _torch()
    N, K, n = p.shape
    if P.dim() != 4 or P.shape[0] != N or P.shape[2] != K or P.shape[3] != pos_dim:
        raise ValueError(f"slab_update: P (N={N}, n_slab, K={K}, pos_dim={pos_dim}) expected")
    if z is None:
        z = torch.empty_like(P)
    elif tuple(z.shape) != tuple(P.shape):
        raise ValueError("slab_update: z must have P's shape")
    rc = lib().scvx_slab_update_batched(N, P.shape[1], K, pos_dim, n, _dev(p, name="p"), _dev(P, name="P"),
                                        _dev(z, name="z"), _stream(stream))
    check(rc, "scvx_slab_update_batched")
    return z


def admm_consensus(X_new, nbr, rho, Y, Lam, pos_dim, primal=None, dual=None, stream=None, check_index=True):
    """ADMM consensus / dual update of every (agent, neighbour slot) in one launch
    (scvx_admm_consensus_batched; the host loop of SCvx/optimization/admm_coordinator.py:80-96).
    X_new (N,K,n) float64, nbr (N,n_nbr) int32 neighbour indices, Y / Lam (N,n_nbr,K,pos_dim) updated in
    place.  Returns device tensors primal, dual (N,n_nbr): ||p_j - Y_new||_F, ||Y_new - Y_old||_F.
    check_index=False skips the range check of nbr (a device -> host read) for callers that built nbr
    themselves (the coordinators validate it once)."""
    torch = _torch()
    N, K, n = X_new.shape
    n_nbr = nbr.shape[1] if nbr.dim() == 2 else 0
    shp = (N, n_nbr, K, pos_dim)
    if tuple(nbr.shape) != (N, n_nbr) or tuple(Y.shape) != shp or tuple(Lam.shape) != shp:
        raise ValueError(f"admm_consensus: nbr (N,n_nbr), Y / Lam {shp} expected")
    if not 1 <= pos_dim <= n:
        raise ValueError("admm_consensus: pos_dim out of range")
    if check_index and n_nbr and (int(nbr.min()) < 0 or int(nbr.max()) >= N):
        raise ValueError("admm_consensus: neighbour index out of range")
    if primal is None:
        primal = torch.empty((N, n_nbr), dtype=torch.float64, device=X_new.device)
    if dual is None:
        dual = torch.empty((N, n_nbr), dtype=torch.float64, device=X_new.device)
    rc = lib().scvx_admm_consensus_batched(N, n_nbr, K, pos_dim, n, _dev(X_new, name="X_new"),
                                           _dev(nbr, torch.int32, "nbr"), float(rho), _dev(Y, name="Y"),
                                           _dev(Lam, name="Lam"), _dev(primal, name="primal"), _dev(dual, name="dual"),
                                           _stream(stream))
    check(rc, "scvx_admm_consensus_batched")
    return primal, dual


def jacobi_update(status, X_sol, U_sol, X, U, tr, prev_cost, grow=False, tr_max=float("inf"), X_out=None, U_out=None,
                  tie_rtol=0.0, stream=None):
    """Fused bookkeeping of one Jacobi SCvx iteration, per-agent trust-region rule
    (scvx_jacobi_update_batched): failed agents (status 2) keep (X, U), the others take (X_sol, U_sol);
    tr halves where sum_{t<K-1} ||u_t||^2 rose above prev_cost (1 + tie_rtol), then a failed agent's radius halves
    (or doubles up to tr_max with grow=True); prev_cost <- the new cost.  tr / prev_cost are updated in
    place; returns (X_out, U_out) (fresh tensors unless given)."""
    torch = _torch()
    N, K, n = X.shape
    m = U.shape[2]
    if (tuple(X_sol.shape) != (N, K, n) or tuple(U.shape) != (N, K, m) or tuple(U_sol.shape) != (N, K, m)
            or tuple(status.shape) != (N,) or tuple(tr.shape) != (N,) or tuple(prev_cost.shape) != (N,)):
        raise ValueError("jacobi_update: X / X_sol (N,K,n), U / U_sol (N,K,m), status / tr / prev_cost (N,)")
    X_out = torch.empty_like(X) if X_out is None else X_out
    U_out = torch.empty_like(U) if U_out is None else U_out
    if tuple(X_out.shape) != (N, K, n) or tuple(U_out.shape) != (N, K, m):
        raise ValueError("jacobi_update: X_out / U_out shapes")
    rc = lib().scvx_jacobi_update_batched(N, K, n, m, _dev(status, torch.int32, "status"), _dev(X_sol, name="X_sol"),
                                          _dev(U_sol, name="U_sol"), _dev(X, name="X"), _dev(U, name="U"),
                                          _dev(X_out, name="X_out"), _dev(U_out, name="U_out"), _dev(tr, name="tr"),
                                          _dev(prev_cost, name="prev_cost"), int(bool(grow)), float(tr_max),
                                          float(tie_rtol), _stream(stream))
    check(rc, "scvx_jacobi_update_batched")
    return X_out, U_out


def jacobi_update_global(status, X_sol, U_sol, X, U, tr, prev_total, grow=False, tr_max=float("inf"), X_out=None,
                         U_out=None, all_reduce=None, stream=None):
    """Fused bookkeeping of one Jacobi SCvx iteration under the reference's global trust-region rule
    (Distributed_opt/dist_scvx_3d.py:242-252; scvx_jacobi_update_costs_batched + scvx_jacobi_global_rule): failed agents
    (status 2) keep (X, U), the others take (X_sol, U_sol); every radius halves when the summed cost
    sum_i sum_{t<K-1} ||u_t||^2 exceeds prev_total (strict), then a failed agent's radius halves (or doubles up to
    tr_max with grow=True); prev_total (a (1,) device tensor) <- the total.  all_reduce: a callable that sums a (1,)
    device tensor over the ranks in place (torch.distributed.all_reduce), for agents sharded over ranks.  Returns
    (X_out, U_out)."""
    torch = _torch()
    N, K, n = X.shape
    m = U.shape[2]
    if (tuple(X_sol.shape) != (N, K, n) or tuple(U.shape) != (N, K, m) or tuple(U_sol.shape) != (N, K, m)
            or tuple(status.shape) != (N,) or tuple(tr.shape) != (N,) or tuple(prev_total.shape) != (1,)):
        raise ValueError("jacobi_update_global: X / X_sol (N,K,n), U / U_sol (N,K,m), status / tr (N,), prev_total (1,)")
    X_out = torch.empty_like(X) if X_out is None else X_out
    U_out = torch.empty_like(U) if U_out is None else U_out
    cost = torch.empty((N,), dtype=torch.float64, device=X.device)
    L, st = lib(), _stream(stream)
    rc = L.scvx_jacobi_update_costs_batched(N, K, n, m, _dev(status, torch.int32, "status"), _dev(X_sol, name="X_sol"),
                                            _dev(U_sol, name="U_sol"), _dev(X, name="X"), _dev(U, name="U"),
                                            _dev(X_out, name="X_out"), _dev(U_out, name="U_out"), _dev(cost, name="cost"),
                                            st)
    check(rc, "scvx_jacobi_update_costs_batched")
    s32, ptr = _dev(status, torch.int32, "status"), _dev(tr, name="tr")
    pt = _dev(prev_total, name="prev_total")
    if all_reduce is None:
        rc = L.scvx_jacobi_global_rule(N, 1, s32, _dev(cost, name="cost"), None, None, ptr, pt, int(bool(grow)),
                                       float(tr_max), st)
    else:
        total = torch.empty((1,), dtype=torch.float64, device=X.device)
        rc = L.scvx_jacobi_global_rule(N, 0, s32, _dev(cost, name="cost"), None, _dev(total, name="total"), None, None,
                                       0, 0.0, st)
        check(rc, "scvx_jacobi_global_rule")
        all_reduce(total)
        rc = L.scvx_jacobi_global_rule(N, 2, s32, None, _dev(total, name="total"), None, ptr, pt, int(bool(grow)),
                                       float(tr_max), st)
    check(rc, "scvx_jacobi_global_rule")
    return X_out, U_out


def intersample_batched(model, X, U, sigma, obstacles, proj=None, dt=1.0, seg_dt=None, num_samples=100, eps=1e-4,
                        tol=1e-6, max_crit=8, nsub=None, params=None, stream=None):
    """Inter-sample obstacle minima for every (agent, segment, obstacle) (scvx_intersample_batched;
    SCvx/utils/intersample_collision.py as called per segment by SCvx/models/game_si_model.py:156-176).

    model: a built-in model name, or a scvx_hip.rtc.DeviceModel (any user model: scvx_rtc_intersample_batched,
    the same scan on its runtime-compiled f).  X (N,K,n), U (N,K,m), sigma (N,) float64 device tensors;
    obstacles [(center (pd,), radius)]; proj (pd, n) projection T (default: the first pd state rows); dt as
    find_critical_times; seg_dt = FirstOrderHold.dt (default 1/(K-1)).  Returns device tensors n_crit (N,K-1,O)
    int32 and t_crit / h0 (N,K-1,O,max_crit), grad_x (...,n), grad_u (...,m); entries past n_crit are unset."""
    import numpy as np
    torch = _torch()
    rt = not isinstance(model, str)
    N, K, n, m = _check_xus("intersample_batched", model, X, U, sigma)
    O = len(obstacles)
    if O > _lib.SCVX_MAX_OBS:
        raise ValueError("too many obstacles")
    if n > _lib.SCVX_IS_MAX_STATE:
        raise ValueError(f"intersample_batched: n_x {n} > {_lib.SCVX_IS_MAX_STATE}")
    pd = len(np.asarray(obstacles[0][0]).reshape(-1)) if O else 1
    Tm = np.eye(n)[:pd] if proj is None else np.asarray(proj, float).reshape(pd, n)
    t = _lib.IntersampleTemplate()
    t.model_id, t.proj_rows = model_id(model), pd
    _fill_obstacles(t, [(np.asarray(c, float).reshape(-1), r) for c, r in obstacles], rows=pd)
    for i in range(pd):
        for j in range(n):
            t.proj[i * _lib.SCVX_IS_MAX_STATE + j] = float(Tm[i, j])
    t.dt, t.seg_dt = float(dt), float(1.0 / (K - 1) if seg_dt is None else seg_dt)
    t.eps, t.tol, t.num_samples, t.max_crit = float(eps), float(tol), int(num_samples), int(max_crit)
    # default substeps: the FOH's for this segment length T = seg_dt * sigma (default_nsub; the quadrotor's count
    # grows with T, so max(sigma) is read on the host for it)
    t.nsub = int(nsub or (model.nsub if rt else
                          (default_nsub(model, t.seg_dt * float(sigma.max().item()), 2) if model in NSUB_SCALE and N
                           else DEFAULT_NSUB[model])))
    dev = X.device
    f64 = torch.float64
    shp = (N, K - 1, max(O, 1))
    out = dict(n_crit=torch.zeros(shp, dtype=torch.int32, device=dev),
               t_crit=torch.zeros(shp + (max_crit,), dtype=f64, device=dev),
               h0=torch.zeros(shp + (max_crit,), dtype=f64, device=dev),
               grad_x=torch.zeros(shp + (max_crit, n), dtype=f64, device=dev),
               grad_u=torch.zeros(shp + (max_crit, m), dtype=f64, device=dev))
    bufs = (_dev(X, name="X"), _dev(U, name="U"), _dev(sigma, name="sigma"), _dev(out["n_crit"], torch.int32),
            _dev(out["t_crit"]), _dev(out["h0"]), _dev(out["grad_x"]), _dev(out["grad_u"]), _stream(stream))
    if rt:
        pa, npar = model._pp(params)
        rc = lib().scvx_rtc_intersample_batched(model._h.ptr, pa.ctypes.data, npar, ctypes.byref(t), K, N, *bufs)
        check(rc, "scvx_rtc_intersample_batched")
    else:
        keep, pp = _params(model, params)
        rc = lib().scvx_intersample_batched(ctypes.byref(t), pp, K, N, *bufs)
        check(rc, "scvx_intersample_batched")
        del keep
    return {k: v[:, :, :O] for k, v in out.items()}


def _rollout_dense_args(who, model, X, U, sigma, S, pos_dim):
    """The arguments of a dense roll-out, built-in (rollout_dense) or runtime-compiled (DeviceModel.rollout_dense),
    checked before any device access -> (N, K, S, pos_dim).  pos_dim None: 2 for the unicycle, 3 for the other
    built-in models; a user model has no default (which of its states are positions is the caller's knowledge: the
    kinematic car's third state is a heading)."""
    N, K, n, m = _check_xus(who, model, X, U, sigma)
    if K < 2:
        raise ValueError(f"{who}: K >= 2 required")
    if pos_dim is None:
        if not isinstance(model, str):
            raise ValueError(f"{who}: pos_dim is required for a user model (the number of leading states that are "
                             f"positions, 1 <= pos_dim <= {min(3, n)})")
        pos_dim = 2 if model == "unicycle" else 3
    S, pos_dim = int(S), int(pos_dim)
    if not 1 <= S <= 16 or not 1 <= pos_dim <= min(3, n):
        raise ValueError(f"{who}: 1 <= S <= 16 and 1 <= pos_dim <= {min(3, n)} required, got S={S}, "
                         f"pos_dim={pos_dim}")
    return N, K, S, pos_dim


def rollout_dense(model, X, U, sigma, S=8, nsub=None, pos_dim=None, params=None, stream=None):
    """Dense samples of every segment's nonlinear roll-out (scvx_rollout_dense_batched): X (N,K,n), U (N,K,m),
    sigma (N,) float64 device tensors -> (P, L), P (N,K-1,S+1,3) the first pos_dim states at tau = s/S of each
    segment (zeros past pos_dim), L (N,K-1) the polyline length of those samples.  Restarts at every node, as
    integrate_nonlinear(piecewise=True).  RK4 with sub = ceil(nsub / S) steps between samples; nsub None:
    default_nsub for the batch's longest interval (exact for "di" / "si").  pos_dim None: 2 for the unicycle,
    else 3.  model: a built-in name, or a scvx_hip.rtc.DeviceModel (any user model: its own rollout_dense, the same
    kernel body on its runtime-compiled f; pos_dim is then required and nsub None means the model's nsub)."""
    torch = _torch()
    if not isinstance(model, str):
        roll = getattr(model, "rollout_dense", None)
        if roll is None:
            raise NotImplementedError("rollout_dense: the model must be a built-in name or offer rollout_dense "
                                      "(scvx_hip.rtc.DeviceModel)")
        return roll(X, U, sigma, S=S, nsub=nsub, pos_dim=pos_dim, params=params, stream=stream)
    N, K, S, pos_dim = _rollout_dense_args("rollout_dense", model, X, U, sigma, S, pos_dim)
    nsub = _nsub("rollout_dense", nsub, lambda: _auto_nsub(model, sigma, K))
    P = torch.empty((N, K - 1, S + 1, 3), dtype=torch.float64, device=X.device)
    L = torch.empty((N, K - 1), dtype=torch.float64, device=X.device)
    if N == 0:
        return P, L
    keep, pp = _params(model, params)
    rc = lib().scvx_rollout_dense_batched(MODEL_IDS[model], pp, K, N, _dev(X, name="X"), _dev(U, name="U"),
                                          _dev(sigma, name="sigma"), S, -(-nsub // S), pos_dim, _dev(P, name="P"),
                                          _dev(L, name="L"), _stream(stream))
    check(rc, "scvx_rollout_dense_batched")
    del keep
    return P, L


def _check_samples(who, P_all, L_all, i0, n_local, k_max=None):
    """The dense-sample arguments of the pair-scan entry points -> (N_total, K-1, S, i0, n_local); k_max: the
    entry point's upper bound on K, if it has one."""
    if P_all.dim() != 4 or P_all.shape[3] != 3 or P_all.shape[2] < 2 or tuple(L_all.shape) != tuple(P_all.shape[:2]):
        raise ValueError(f"{who}: P_all (N_total,K-1,S+1,3) and L_all (N_total,K-1) expected")
    N_total, Km1, S = P_all.shape[0], P_all.shape[1], P_all.shape[2] - 1
    i0, n_local = int(i0), int(n_local)
    if S > 16 or Km1 < 1 or (k_max and Km1 >= k_max) or i0 < 0 or n_local < 0 or i0 + n_local > N_total:
        raise ValueError(f"{who}: S <= 16, {f'2 <= K <= {k_max}' if k_max else 'K >= 2'} and 0 <= i0, "
                         f"i0 + n_local <= N_total required; got S={S}, K-1={Km1}, i0={i0}, n_local={n_local}, "
                         f"N_total={N_total}")
    return N_total, Km1, S, i0, n_local


def separation_scan(P_all, L_all, i0, n_local, stream=None, prune=True):
    """Continuous-time closest approach of local agents [i0, i0+n_local) to every other agent of P_all
    (N_total,K-1,S+1,3) / L_all (N_total,K-1) (rollout_dense's outputs) at equal normalised time
    (scvx_separation_scan_batched).  Per (local agent, segment), device tensors: sep the minimum chord distance
    (+inf when there is no other agent), j the other agent and s the sub-interval it occurs in (-1, -1 then),
    alpha its position in the sub-interval, tau = (s + alpha) / S its position in the segment (nan when j < 0).
    First minimum in the order j, then s.  Exact for the piecewise-linear interpolant of the samples: within
    max ||r''|| h^2 / 8 of the continuous minimum, h = 1 / ((K-1) S) in normalised time, r the relative position.
    prune=False (tests) disables the skip of far neighbours; the outputs are bit-identical."""
    torch = _torch()
    N_total, Km1, S, i0, n_local = _check_samples("separation_scan", P_all, L_all, i0, n_local)
    dev = P_all.device
    sep = torch.empty((n_local, Km1), dtype=torch.float64, device=dev)
    arg = torch.empty((n_local, Km1, 2), dtype=torch.int32, device=dev)
    alpha = torch.empty((n_local, Km1), dtype=torch.float64, device=dev)
    rc = lib().scvx_separation_scan_batched(Km1 + 1, S, N_total, _dev(P_all, name="P_all"), _dev(L_all, name="L_all"),
                                            i0, n_local, _dev(sep, name="sep"), _dev(arg, torch.int32, "arg"),
                                            _dev(alpha, name="alpha"), 0 if prune else 1, _stream(stream))
    check(rc, "scvx_separation_scan_batched")
    j, s = arg[..., 0], arg[..., 1]
    tau = torch.where(j >= 0, (s.to(torch.float64) + alpha) / S, torch.full_like(alpha, float("nan")))
    return dict(sep=sep, j=j, s=s, alpha=alpha, tau=tau)


def fleet_separation(model, X, U, sigma, S=8, nsub=None, pos_dim=None, params=None, stream=None):
    """rollout_dense + separation_scan of a whole fleet: how close any two agents come, between the nodes as
    well as at them.  Returns separation_scan's dict plus P, L (the samples), agent_min (N,) each agent's
    minimum over its segments, min (float) the fleet's minimum and argmin = (i, j, k, tau) where it occurs
    (None for a single agent).  model: a built-in name or a DeviceModel (pos_dim required), as rollout_dense; the
    scan reads only the samples.  The accuracy statement of separation_scan applies; for the double integrator
    ||r''|| <= 2 max(sigma^2 ||u||) in normalised time."""
    P, L = rollout_dense(model, X, U, sigma, S=S, nsub=nsub, pos_dim=pos_dim, params=params, stream=stream)
    out = separation_scan(P, L, 0, X.shape[0], stream=stream)
    out.update(P=P, L=L, agent_min=out["sep"].min(dim=1).values)
    flat = int(out["sep"].argmin().item())
    i, k = divmod(flat, X.shape[1] - 1)
    out["min"] = float(out["sep"][i, k].item())
    out["argmin"] = (i, int(out["j"][i, k].item()), k, float(out["tau"][i, k].item())) if X.shape[0] > 1 else None
    return out


def intersample_pair_rows(P_all, L_all, i0, n_local, R, cull, J=2, stream=None, prune=True):
    """Inter-sample collision records of local agents [i0, i0+n_local) on the dense samples P_all
    (N_total,K-1,S+1,3) / L_all (N_total,K-1) of rollout_dense (scvx_intersample_pair_rows_batched): per (agent,
    segment) the J neighbours whose chord closest approach lies strictly between the two nodes (0 < alpha' < 1), is
    closer than cull and is not zero, nearest first, ties to the lower j.  Returns device tensors rec
    (n_local,K-1,J,4) = (g, v) with g = c / dist the unit relative position at the closest approach and
    v = 2R - dist, nbr (n_local,K-1,J) int32 the neighbour (-1 past count), alpha (n_local,K-1,J) = alpha' and count
    (n_local,K-1) int32.  prune=False (tests) disables the skip of far neighbours; the outputs are bit-identical."""
    torch = _torch()
    N_total, Km1, S, i0, n_local = _check_samples("intersample_pair_rows", P_all, L_all, i0, n_local, k_max=64)
    J = int(J)
    if not 1 <= J <= 8 or not float(cull) > 0.0:
        raise ValueError(f"intersample_pair_rows: 1 <= J <= 8 and cull > 0 required, got J={J}, cull={cull}")
    dev = P_all.device
    rec = torch.empty((n_local, Km1, J, 4), dtype=torch.float64, device=dev)
    nbr = torch.empty((n_local, Km1, J), dtype=torch.int32, device=dev)
    alpha = torch.empty((n_local, Km1, J), dtype=torch.float64, device=dev)
    count = torch.empty((n_local, Km1), dtype=torch.int32, device=dev)
    rc = lib().scvx_intersample_pair_rows_batched(Km1 + 1, S, N_total, _dev(P_all, name="P_all"),
                                                  _dev(L_all, name="L_all"), i0, n_local, float(R), float(cull), J,
                                                  _dev(rec, name="rec"), _dev(nbr, torch.int32, "nbr"),
                                                  _dev(alpha, name="alpha"), _dev(count, torch.int32, "count"),
                                                  0 if prune else 1, _stream(stream))
    check(rc, "scvx_intersample_pair_rows_batched")
    return dict(rec=rec, nbr=nbr, alpha=alpha, count=count)


def append_collision_rows(X_all, i0, rec, count_seg, rows, count, pos_dim=3, idx=None, overflow=None, check_index=True,
                          stream=None):
    """Append the records of intersample_pair_rows behind the node rows of collision_rows
    (scvx_collision_rows_append_batched): a record of segment k becomes the rows (g, b = v + g . pbar_t) at nodes
    t = k and t = k+1, pbar = X_all (N_total,K,n) the current iterate; per node segment t's records first, then
    segment t-1's, none at node K-1.  rows (>= n,K,j_max,pos_dim+1) and count (>= n,K) int32 are updated in place
    (their leading n entries); rows past j_max are dropped and counted in overflow (a (1,) int32 device tensor that
    accumulates; a zeroed one is made when None).  idx None: the n = rec.shape[0] agents i0, i0+1, ...; idx (device
    int32): agent a is global agent idx[a], as collision_rows_indexed, and reads rec / count_seg [idx[a] - i0]
    (check_index=False skips the range check of idx, a device -> host read).  Returns (rows, count, overflow)."""
    torch = _torch()
    N_total, K, n_x = X_all.shape
    i0, pos_dim = int(i0), int(pos_dim)
    if rec.dim() != 4 or tuple(rec.shape[1:2] + rec.shape[3:]) != (K - 1, 4) or tuple(count_seg.shape) != tuple(rec.shape[:2]):
        raise ValueError(f"append_collision_rows: rec (n,{K - 1},J,4) and count_seg (n,{K - 1}) expected")
    n_rec, J = int(rec.shape[0]), int(rec.shape[2])
    n = n_rec if idx is None else int(idx.shape[0])
    if not 1 <= J <= 8 or not 2 <= K <= 64 or not 1 <= pos_dim <= min(3, n_x) or i0 < 0 or i0 + n_rec > N_total:
        raise ValueError(f"append_collision_rows: 1 <= J <= 8, 2 <= K <= 64, 1 <= pos_dim <= {min(3, n_x)} and "
                         f"0 <= i0, i0 + n <= N_total required; got J={J}, K={K}, pos_dim={pos_dim}, i0={i0}")
    if rows.dim() != 4 or rows.shape[0] < n or tuple(rows.shape[1:2] + rows.shape[3:]) != (K, pos_dim + 1) or \
            count.dim() != 2 or count.shape[0] < n or count.shape[1] != K or not 1 <= rows.shape[2] <= 32:
        raise ValueError(f"append_collision_rows: rows (>= {n},{K},j_max <= 32,{pos_dim + 1}) and count (>= {n},{K}) expected")
    if idx is not None and check_index and n and (int(idx.min()) < i0 or int(idx.max()) >= i0 + n_rec):
        raise ValueError("append_collision_rows: idx outside the agents [i0, i0 + rec.shape[0]) the records cover")
    if overflow is None:
        overflow = torch.zeros((1,), dtype=torch.int32, device=X_all.device)
    rc = lib().scvx_collision_rows_append_batched(K, pos_dim, n_x, N_total, _dev(X_all, name="X_all"), i0,
                                                  _dev(idx, torch.int32, "idx") if idx is not None else None, n, J,
                                                  _dev(rec, name="rec"), _dev(count_seg, torch.int32, "count_seg"),
                                                  int(rows.shape[2]), _dev(rows, name="rows"),
                                                  _dev(count, torch.int32, "count"),
                                                  _dev(overflow, torch.int32, "overflow"), _stream(stream))
    check(rc, "scvx_collision_rows_append_batched")
    return rows, count, overflow


def _obstacle_arrays(who, obstacles, device):
    """[(centre, total radius)] -> device tensors centers (O,3), rho (O,); centres shorter than 3 are zero-padded
    (P holds zeros past pos_dim).  A pair of tensors (centers, rho) made here before passes through."""
    import numpy as np
    torch = _torch()
    if isinstance(obstacles, tuple) and len(obstacles) == 2 and all(isinstance(t, torch.Tensor) for t in obstacles):
        if obstacles[0].dim() != 2 or obstacles[0].shape[1] != 3 or tuple(obstacles[1].shape) != (obstacles[0].shape[0],) \
                or not obstacles[0].shape[0]:
            raise ValueError(f"{who}: centers (O,3) and rho (O,) with O >= 1 expected")
        return obstacles
    obstacles = list(obstacles)
    if not obstacles:
        raise ValueError(f"{who}: at least one obstacle required")
    c = np.zeros((len(obstacles), 3))
    for o, (ctr, _) in enumerate(obstacles):
        ctr = np.asarray(ctr, float).reshape(-1)
        if not 1 <= ctr.size <= 3:
            raise ValueError(f"{who}: obstacle centres must have 1..3 coordinates")
        c[o, :ctr.size] = ctr
    r = np.array([float(r) for _, r in obstacles])
    return torch.as_tensor(c, device=device), torch.as_tensor(r, device=device)


def obstacle_scan(P, obstacles, cull=None, J=0, analysis=True, stream=None):
    """Continuous-time closest approach of every agent to every obstacle on the dense samples P (N,K-1,S+1,3) of
    rollout_dense (scvx_obstacle_scan_batched).  obstacles: [(centre, total radius rho)], at least one, any number;
    centres shorter than 3 are zero-padded to match P's zero columns past pos_dim.  Device tensors: dist (N,K-1,O)
    every obstacle's minimum chord distance to its centre on every segment and alpha (N,K-1,O) its position in the
    segment, alpha' = (s + a) / S (analysis=False leaves both out).  Exact for the piecewise-linear interpolant of
    the samples: within max ||r''|| h^2 / 8 of the continuous minimum, h = 1 / ((K-1) S) in normalised time,
    r = p - c.
    J in 1..8 adds the records of the obstacle rows (K <= 64): per (agent, segment) the J obstacles of largest
    v = rho - dist among those with v > -cull (cull None: the largest rho), 0 < alpha' < 1 and dist > 0, in
    descending (v, then ascending o) order: rec (N,K-1,J,4) = (g, v) with g = c / dist the unit direction from the
    centre at the closest approach, obs (N,K-1,J) int32 the obstacle (-1 past count), rec_alpha (N,K-1,J) = alpha'
    and count (N,K-1) int32 -- the layout of intersample_pair_rows, so append_collision_rows takes them as they are."""
    torch = _torch()
    if P.dim() != 4 or P.shape[3] != 3 or P.shape[2] < 2 or P.shape[1] < 1:
        raise ValueError("obstacle_scan: P (N,K-1,S+1,3) with K >= 2 and S >= 1 expected")
    N, Km1, S = P.shape[0], P.shape[1], P.shape[2] - 1
    J = int(J)
    if S > 16 or not 0 <= J <= 8 or (J and Km1 >= 64) or not (J or analysis):
        raise ValueError(f"obstacle_scan: S <= 16 and 0 <= J <= 8 required (records: K <= 64; J = 0 needs "
                         f"analysis=True); got S={S}, J={J}, K={Km1 + 1}")
    dev = P.device
    cd, rd = _obstacle_arrays("obstacle_scan", obstacles, dev)
    O = cd.shape[0]
    cull = float(rd.max().item()) if cull is None else float(cull)
    if J and not cull > 0.0:
        raise ValueError(f"obstacle_scan: cull > 0 required, got {cull}")
    out = {}
    if analysis:
        out["dist"] = torch.empty((N, Km1, O), dtype=torch.float64, device=dev)
        out["alpha"] = torch.empty((N, Km1, O), dtype=torch.float64, device=dev)
    if J:
        out["rec"] = torch.empty((N, Km1, J, 4), dtype=torch.float64, device=dev)
        out["obs"] = torch.empty((N, Km1, J), dtype=torch.int32, device=dev)
        out["rec_alpha"] = torch.empty((N, Km1, J), dtype=torch.float64, device=dev)
        out["count"] = torch.empty((N, Km1), dtype=torch.int32, device=dev)
    ptr = lambda k, dt=None: _dev(out[k], dt, k) if k in out else None  # noqa: E731
    rc = lib().scvx_obstacle_scan_batched(Km1 + 1, S, N, _dev(P, name="P"), O, _dev(cd, name="centers"),
                                          _dev(rd, name="rho"), cull, J, ptr("dist"), ptr("alpha"), ptr("rec"),
                                          ptr("obs", torch.int32), ptr("rec_alpha"), ptr("count", torch.int32),
                                          _stream(stream))
    check(rc, "scvx_obstacle_scan_batched")
    return out


def fleet_obstacle_clearance(model, X, U, sigma, obstacles, robot_radius=0.0, S=8, nsub=None, pos_dim=None,
                             params=None, stream=None):
    """rollout_dense + obstacle_scan of a whole fleet, the counterpart of fleet_separation: how close any agent
    comes to any obstacle, between the nodes as well as at them.  obstacles: [(centre, radius r_o)].  Returns clear
    (N,K-1,O) = dist - (r_o + robot_radius) per segment, tau (N,K-1,O) where in the segment it occurs, D (N,O) the
    minimum over the segments (the continuous-time form of obstacle_min_distance's matrix), agent_min (N,), min
    (float) and argmin = (i, o, k, tau) where it occurs, plus P, L (the samples).  model: a built-in name or a
    DeviceModel (pos_dim required), as rollout_dense.  The accuracy statement of
    separation_scan applies with r = p - c the position relative to the (fixed) centre; for the double integrator
    ||r''|| <= max(sigma^2 ||u||) in normalised time."""
    torch = _torch()
    obstacles = list(obstacles)
    P, L = rollout_dense(model, X, U, sigma, S=S, nsub=nsub, pos_dim=pos_dim, params=params, stream=stream)
    sc = obstacle_scan(P, obstacles, stream=stream)
    total = torch.as_tensor([float(r) + float(robot_radius) for _, r in obstacles], dtype=torch.float64,
                            device=X.device)
    clear = sc["dist"] - total
    out = dict(clear=clear, tau=sc["alpha"], P=P, L=L, D=clear.min(dim=1).values)
    out["agent_min"] = out["D"].min(dim=1).values
    O = clear.shape[2]
    flat = int(clear.argmin().item())
    i, rest = divmod(flat, clear.shape[1] * O)
    k, o = divmod(rest, O)
    out["min"] = float(clear[i, k, o].item())
    out["argmin"] = (i, o, k, float(sc["alpha"][i, k, o].item()))
    return out


class ObstacleTracks(tuple):
    """(knots (O,M_max,3), n_knots (O,) int32, window (O,2), rho (O,)) device tensors made and validated by
    obstacle_tracks; passes through it unchanged."""
    __slots__ = ()


def obstacle_tracks(tracks, device):
    """Moving obstacles [(knots, (t0, t1), rho)] -> ObstacleTracks, the device arrays of moving_obstacle_scan.
    Track o: n_o >= 1 knots of 1..3 coordinates each (zero-padded like the static centres), equally spaced over the
    real-time window [t0, t1]; rho the total radius.  One knot: a fixed centre, the window is ignored (None will do).
    Two or more need t1 > t0: q(t) = c_m + (u - m)(c_{m+1} - c_m) with u = clamp((t - t0) / (t1 - t0), 0, 1) (n - 1),
    m = min(floor(u), n - 2) -- the obstacle waits at its first knot before t0 and stops at its last after t1; a
    constant-velocity intruder is two knots.  Validated here, on the host; an ObstacleTracks made before passes
    through."""
    import numpy as np
    torch = _torch()
    if isinstance(tracks, ObstacleTracks):
        return tracks
    tracks = list(tracks)
    if not tracks:
        raise ValueError("obstacle_tracks: at least one track required")
    ks = []
    for kn, _, _ in tracks:
        kn = np.asarray(kn, float)
        kn = kn.reshape(1, -1) if kn.ndim == 1 else kn
        if kn.ndim != 2 or kn.shape[0] < 1 or not 1 <= kn.shape[1] <= 3 or not np.isfinite(kn).all():
            raise ValueError("obstacle_tracks: a track's knots must be (n >= 1, 1..3 coordinates), finite")
        ks.append(kn)
    O, M = len(ks), max(k.shape[0] for k in ks)
    knots, win = np.zeros((O, M, 3)), np.zeros((O, 2))
    win[:, 1] = 1.0
    for o, (kn, (_, w, _)) in enumerate(zip(ks, tracks)):
        knots[o, :kn.shape[0], :kn.shape[1]] = kn
        if kn.shape[0] >= 2:
            t0, t1 = (float(x) for x in w)
            if not (np.isfinite(t0) and np.isfinite(t1) and t1 > t0):
                raise ValueError(f"obstacle_tracks: track {o} has {kn.shape[0]} knots and needs a window t1 > t0, "
                                 f"got ({t0}, {t1})")
            win[o] = t0, t1
    rho = np.array([float(r) for _, _, r in tracks])
    if not np.isfinite(rho).all():
        raise ValueError("obstacle_tracks: rho must be finite")
    return ObstacleTracks((torch.as_tensor(knots, device=device),
                           torch.as_tensor(np.array([k.shape[0] for k in ks], np.int32), device=device),
                           torch.as_tensor(win, device=device), torch.as_tensor(rho, device=device)))


def moving_obstacle_scan(P, sigma, tracks, cull=None, J=0, analysis=True, node_rows=True, stream=None):
    """obstacle_scan against obstacles that move (scvx_moving_obstacle_scan_batched).  P (N,K-1,S+1,3) the dense
    samples of rollout_dense, sigma (N,) the agents' final times: agent i lives on its own clock, sample s of segment
    k is at t = sigma_i (k S + s) / ((K-1) S).  tracks: [(knots, (t0, t1), rho)] or an ObstacleTracks
    (obstacle_tracks).  The chords run on the relative samples d_s = p_s - q_o(t_s).  Returns obstacle_scan's dict --
    dist, alpha (N,K-1,O) with analysis; rec, obs, rec_alpha, count with J in 1..8 (K <= 64; cull None: the largest
    rho) -- plus, with J >= 1 and node_rows, the node records the QP kernel cannot hold for a centre that moves: per
    segment's first node (sample 0; node K-1 gets none) the J obstacles of largest v = rho - |d_0| with v > -cull and
    |d_0| > 0, descending (v, then ascending o): node_rec (N,K-1,J,4) = (d_0 / |d_0|, v), node_obs (N,K-1,J) int32
    (-1 past the count), node_count (N,K-1) int32; append_node_rows takes them as they are.  With one knot per track
    every output is obstacle_scan's bit for bit.
    Accuracy.  The scan is exact for the piecewise-linear interpolant of the relative samples r = p - q.  On a
    sub-interval of length h = 1 / ((K-1) S) (normalised time) on which r is twice differentiable the interpolant is
    within max ||r''|| h^2 / 8 of r.  q is piecewise linear: r'' = p'' except at a knot time, where r' jumps by the
    change dv of the obstacle's velocity (per unit normalised time).  Such a jump at a point a of (0, h) adds the
    term -dv max(0, t - a) to r, which is farthest from its own chord at t = a: ||dv|| a (h - a) / h <= ||dv|| h / 4.
    Hence: within max ||p''|| h^2 / 8 + (h / 4) sum ||dv|| of the continuous minimum, the sum over the knots that
    fall strictly inside one sub-interval (the first and the last knot, where the obstacle starts and stops,
    included)."""
    torch = _torch()
    if P.dim() != 4 or P.shape[3] != 3 or P.shape[2] < 2 or P.shape[1] < 1:
        raise ValueError("moving_obstacle_scan: P (N,K-1,S+1,3) with K >= 2 and S >= 1 expected")
    N, Km1, S = P.shape[0], P.shape[1], P.shape[2] - 1
    J = int(J)
    if S > 16 or not 0 <= J <= 8 or (J and Km1 >= 64) or not (J or analysis):
        raise ValueError(f"moving_obstacle_scan: S <= 16 and 0 <= J <= 8 required (records: K <= 64; J = 0 needs "
                         f"analysis=True); got S={S}, J={J}, K={Km1 + 1}")
    if tuple(sigma.shape) != (N,):
        raise ValueError(f"moving_obstacle_scan: sigma ({N},) expected")
    dev = P.device
    kd, nd, wd, rd = obstacle_tracks(tracks, dev)
    if kd.dim() != 3 or kd.shape[2] != 3 or not kd.shape[0] or not kd.shape[1] or tuple(nd.shape) != (kd.shape[0],) \
            or tuple(wd.shape) != (kd.shape[0], 2) or tuple(rd.shape) != (kd.shape[0],):
        raise ValueError("moving_obstacle_scan: knots (O,M_max,3), n_knots (O,), window (O,2), rho (O,) expected")
    O, M = kd.shape[0], kd.shape[1]
    cull = float(rd.max().item()) if cull is None else float(cull)
    if J and not cull > 0.0:
        raise ValueError(f"moving_obstacle_scan: cull > 0 required, got {cull}")
    out = {}
    if analysis:
        out["dist"] = torch.empty((N, Km1, O), dtype=torch.float64, device=dev)
        out["alpha"] = torch.empty((N, Km1, O), dtype=torch.float64, device=dev)
    if J:
        out["rec"] = torch.empty((N, Km1, J, 4), dtype=torch.float64, device=dev)
        out["obs"] = torch.empty((N, Km1, J), dtype=torch.int32, device=dev)
        out["rec_alpha"] = torch.empty((N, Km1, J), dtype=torch.float64, device=dev)
        out["count"] = torch.empty((N, Km1), dtype=torch.int32, device=dev)
        if node_rows:
            out["node_rec"] = torch.empty((N, Km1, J, 4), dtype=torch.float64, device=dev)
            out["node_obs"] = torch.empty((N, Km1, J), dtype=torch.int32, device=dev)
            out["node_count"] = torch.empty((N, Km1), dtype=torch.int32, device=dev)
    ptr = lambda k, dt=None: _dev(out[k], dt, k) if k in out else None  # noqa: E731
    i32 = torch.int32
    rc = lib().scvx_moving_obstacle_scan_batched(Km1 + 1, S, N, _dev(P, name="P"), _dev(sigma, name="sigma"), O, M,
                                                 _dev(kd, name="knots"), _dev(nd, i32, "n_knots"),
                                                 _dev(wd, name="window"), _dev(rd, name="rho"), cull, J, ptr("dist"),
                                                 ptr("alpha"), ptr("rec"), ptr("obs", i32), ptr("rec_alpha"),
                                                 ptr("count", i32), ptr("node_rec"), ptr("node_obs", i32),
                                                 ptr("node_count", i32), _stream(stream))
    check(rc, "scvx_moving_obstacle_scan_batched")
    return out


def append_node_rows(X_all, i0, node_rec, node_count, rows, count, pos_dim=3, idx=None, overflow=None,
                     check_index=True, stream=None):
    """Append the node records of moving_obstacle_scan behind the rows a node already has
    (scvx_node_rows_append_batched): record r of node_rec[a][t] becomes the row (g, b = v + g . pbar_t) at node t,
    pbar = X_all (N_total,K,n) the current iterate; none at node K-1.  rows, count, overflow, idx and check_index as
    append_collision_rows.  Returns (rows, count, overflow)."""
    torch = _torch()
    N_total, K, n_x = X_all.shape
    i0, pos_dim = int(i0), int(pos_dim)
    if node_rec.dim() != 4 or tuple(node_rec.shape[1:2] + node_rec.shape[3:]) != (K - 1, 4) or \
            tuple(node_count.shape) != tuple(node_rec.shape[:2]):
        raise ValueError(f"append_node_rows: node_rec (n,{K - 1},J,4) and node_count (n,{K - 1}) expected")
    n_rec, J = int(node_rec.shape[0]), int(node_rec.shape[2])
    n = n_rec if idx is None else int(idx.shape[0])
    if not 1 <= J <= 8 or not 2 <= K <= 64 or not 1 <= pos_dim <= min(3, n_x) or i0 < 0 or i0 + n_rec > N_total:
        raise ValueError(f"append_node_rows: 1 <= J <= 8, 2 <= K <= 64, 1 <= pos_dim <= {min(3, n_x)} and "
                         f"0 <= i0, i0 + n <= N_total required; got J={J}, K={K}, pos_dim={pos_dim}, i0={i0}")
    if rows.dim() != 4 or rows.shape[0] < n or tuple(rows.shape[1:2] + rows.shape[3:]) != (K, pos_dim + 1) or \
            count.dim() != 2 or count.shape[0] < n or count.shape[1] != K or not 1 <= rows.shape[2] <= 32:
        raise ValueError(f"append_node_rows: rows (>= {n},{K},j_max <= 32,{pos_dim + 1}) and count (>= {n},{K}) expected")
    if idx is not None and check_index and n and (int(idx.min()) < i0 or int(idx.max()) >= i0 + n_rec):
        raise ValueError("append_node_rows: idx outside the agents [i0, i0 + node_rec.shape[0]) the records cover")
    if overflow is None:
        overflow = torch.zeros((1,), dtype=torch.int32, device=X_all.device)
    rc = lib().scvx_node_rows_append_batched(K, pos_dim, n_x, N_total, _dev(X_all, name="X_all"), i0,
                                             _dev(idx, torch.int32, "idx") if idx is not None else None, n, J,
                                             _dev(node_rec, name="node_rec"),
                                             _dev(node_count, torch.int32, "node_count"), int(rows.shape[2]),
                                             _dev(rows, name="rows"), _dev(count, torch.int32, "count"),
                                             _dev(overflow, torch.int32, "overflow"), _stream(stream))
    check(rc, "scvx_node_rows_append_batched")
    return rows, count, overflow


def fleet_moving_obstacle_clearance(model, X, U, sigma, tracks, robot_radius=0.0, S=8, nsub=None, pos_dim=None,
                                    params=None, stream=None):
    """rollout_dense + moving_obstacle_scan of a whole fleet, the counterpart of fleet_obstacle_clearance for
    obstacles that move: tracks [(knots, (t0, t1), radius r_o)] (obstacle_tracks).  Returns clear (N,K-1,O) =
    dist - (r_o + robot_radius) per segment, tau (N,K-1,O) where in the segment it occurs, D (N,O) the minimum over
    the segments, agent_min (N,), min (float) and argmin = (i, o, k, tau), plus P, L (the samples).  model: a built-in
    name or a DeviceModel (pos_dim required), as rollout_dense; the scan reads only the samples.  Accuracy: that of
    moving_obstacle_scan -- within max ||p''|| h^2 / 8 plus h / 4 times the obstacle's velocity jump (per unit
    normalised time, sigma_i times the real one) for every knot strictly inside a sub-interval; for the double
    integrator ||p''|| <= max(sigma^2 ||u||), and a constant-velocity track whose window covers the horizon has no
    jump."""
    torch = _torch()
    tr = obstacle_tracks(tracks, X.device)
    P, L = rollout_dense(model, X, U, sigma, S=S, nsub=nsub, pos_dim=pos_dim, params=params, stream=stream)
    sc = moving_obstacle_scan(P, sigma, tr, stream=stream)
    clear = sc["dist"] - (tr[3] + float(robot_radius))
    out = dict(clear=clear, tau=sc["alpha"], P=P, L=L, D=clear.min(dim=1).values)
    out["agent_min"] = out["D"].min(dim=1).values
    O = clear.shape[2]
    flat = int(clear.argmin().item())
    i, rest = divmod(flat, clear.shape[1] * O)
    k, o = divmod(rest, O)
    out["min"] = float(clear[i, k, o].item())
    out["argmin"] = (i, o, k, float(sc["alpha"][i, k, o].item()))
    return out


def pair_min_distance(X, rows=None, stream=None):
    """min_inter_agent_distance's matrix (SCvx/utils/analysis.py:10-31) on the device: X (N,K,n) -> D (N,N),
    D[i,j] = min_k ||X[i,k,:rows] - X[j,k,:rows]||, symmetric with a zero diagonal.  rows None: min(3, n), the
    reference's rows 0:3 of whatever state it is given (scvx_pair_min_distance_batched)."""
    torch = _torch()
    if X.dim() != 3 or X.shape[1] < 1:
        raise ValueError("pair_min_distance: X (N,K,n) expected")
    N, K, n = X.shape
    rows = min(3, n) if rows is None else int(rows)
    if not 1 <= rows <= min(3, n):
        raise ValueError(f"pair_min_distance: 1 <= rows <= {min(3, n)} required, got {rows}")
    D = torch.empty((N, N), dtype=torch.float64, device=X.device)
    rc = lib().scvx_pair_min_distance_batched(K, n, rows, N, _dev(X, name="X"), _dev(D, name="D"), _stream(stream))
    check(rc, "scvx_pair_min_distance_batched")
    return D


def obstacle_min_distance(X, obstacles, robot_radius, stream=None):
    """min_agent_obstacle_distance's matrix (SCvx/utils/analysis.py:34-62) on the device: X (N,K,n >= 3),
    obstacles [(centre (3,), radius)] -> D (N,M), D[i,o] = min_k (||X[i,k,:3] - c_o|| - (robot_radius + r_o))
    (scvx_obstacle_min_distance_batched)."""
    import numpy as np
    torch = _torch()
    if X.dim() != 3 or X.shape[1] < 1 or X.shape[2] < 3:
        raise ValueError("obstacle_min_distance: X (N,K,n) with n >= 3 expected")
    N, K, n = X.shape
    M = len(obstacles)
    c = np.array([np.asarray(c, float).reshape(-1) for c, _ in obstacles], float).reshape(M, -1)
    if M and c.shape[1] != 3:
        raise ValueError("obstacle_min_distance: obstacle centres must have 3 coordinates")
    D = torch.empty((N, M), dtype=torch.float64, device=X.device)
    if M == 0:
        return D
    cd = torch.as_tensor(np.ascontiguousarray(c), device=X.device)
    rd = torch.as_tensor(np.array([float(r) for _, r in obstacles]), device=X.device)
    rc = lib().scvx_obstacle_min_distance_batched(K, n, N, _dev(X, name="X"), M, _dev(cd, name="centers"),
                                                  _dev(rd, name="radii"), float(robot_radius), _dev(D, name="D"),
                                                  _stream(stream))
    check(rc, "scvx_obstacle_min_distance_batched")
    return D
