"""Batched Jacobi SCvx outer iteration over N agents, device-resident.

Semantics follow the reference's data-parallel SCvx driver Distributed_opt/dist_scvx_3d.py:
  * x_traj_opt (:31-118): every agent solves its trust-region subproblem against the PREVIOUS
    iterate of all other agents (Jacobi), and X_traj is updated only after all solves (:113-118);
  * cost_fcn (:131-138): cost = sum_t ||u_t||^2 over t < T-1;
  * outer loop (:242-252): if the cost increased, trust_region /= 2.
with the build's FOH discretization (SCvx/discretization/first_order_hold.py) in place of the
one-off ZOH (:9-28, :231), so one SCvx iteration = FOH -> [all-gather + collision rows] -> QP ->
update/bookkeeping.  Multi-GPU: agents are sharded contiguously over ranks; the only data-path
collective is one all_gather of the states per iteration (RCCL over xGMI), needed only when
collision coupling is on, plus one scalar all_reduce for the global trust-region rule.
"""
import dataclasses
import os
from dataclasses import dataclass
from typing import Optional, Sequence

from . import (ObstacleTracks, QPSolver, QPSpec, append_collision_rows, append_node_rows, collision_check, collision_rows,
               collision_rows_indexed, default_nsub, fleet_moving_obstacle_clearance, fleet_obstacle_clearance,
               fleet_separation, foh_batched, intersample_pair_rows, jacobi_update, jacobi_update_global, model_dims,
               moving_obstacle_scan, obstacle_scan, obstacle_tracks, rollout_dense)

# The split QP launch of JacobiSCvx (dispatch_order="lpt", every agent resident): the measured settings of
# profiles/split_sweep.txt (DESIGN §3.3 "Split launch").  SPLIT_DEFAULT: what an unset SCVX_QP_SPLIT stands for ("1": on
# where the driver's rule applies, "0": the single launch).
SPLIT_THR, SPLIT_T, SPLIT_RESERVE, SPLIT_DEFAULT = 7, 64, "whole", "1"


def balanced_order(iters, world):
    """An agent order for `world` contiguous shards (rank r owns order[r*n:(r+1)*n]) in which every shard gets
    the same mix of per-agent IPM iteration counts (e.g. the last step's `iters`): agents sorted by
    iterations (descending; ties by index) are dealt to the shards in serpentine order (0..W-1, W-1..0, ...),
    and each shard keeps its agents in ascending index order.  Under the Jacobi update every agent solves
    against the previous iterate of all others (Distributed_opt/dist_scvx_3d.py:93-118), so which rank solves
    which agent does not change any subproblem: the order only moves work between ranks.  A shard's QP launch
    lasts as long as its slowest SIMD's waves, so spreading the long solves evens out the ranks once a GPU holds
    more agents than SIMDs."""
    import numpy as np
    iters = np.asarray(iters)
    N = iters.size
    if N % world:
        raise ValueError(f"balanced_order: {N} agents do not shard over {world} ranks")
    idx = np.lexsort((np.arange(N), -iters))
    rank_of = np.empty(N, np.int64)
    for k, a in enumerate(idx):
        rd, ps = divmod(k, world)
        rank_of[a] = ps if rd % 2 == 0 else world - 1 - ps
    return np.concatenate([np.nonzero(rank_of == r)[0] for r in range(world)])


class HipBackend:
    """The product compute path: the libscvx_hip.so kernels (no CPU fallback)."""

    def foh(self, model, X, U, sigma, nsub, out):
        if isinstance(model, str):
            return foh_batched(model, X, U, sigma, nsub=nsub, out=out)
        return model.foh(X, U, sigma, nsub=nsub, out=out)   # a runtime-compiled model (scvx_hip.rtc.DeviceModel)

    def collision_rows(self, X_all, i0, n_local, R, j_max, pos_dim, cull, rows, count):
        return collision_rows(X_all, i0, n_local, R, j_max, pos_dim, cull, rows, count)

    def collision_rows_indexed(self, X_all, idx, R, j_max, pos_dim, cull, rows, count):
        return collision_rows_indexed(X_all, idx, R, j_max, pos_dim, cull, rows, count)

    def collision_check(self, X_all, i0, X_new, slack, R, pos_dim, tol):
        return collision_check(X_all, i0, X_new, slack, R, pos_dim, tol)

    def intersample_pair_rows(self, model, X, U, sigma, S, nsub, pos_dim, R, cull, J):
        """(rec, count_seg) of every agent of the iterate (X, U): the dense roll-out, then the pair-rows scan."""
        P, L = rollout_dense(model, X, U, sigma, S=S, nsub=nsub, pos_dim=pos_dim)
        self.samples = (S, P)   # for obstacle_rows of the same step (the driver hands it on and clears it)
        out = intersample_pair_rows(P, L, 0, X.shape[0], R, cull, J)
        return out["rec"], out["count"]

    def obstacle_rows(self, model, X, U, sigma, S, nsub, pos_dim, obstacles, cull, J, P=None):
        """(rec, count_seg) of the obstacle rows of every agent of the iterate (X, U): the dense roll-out (P: the
        samples of this very iterate at the same S, when the step already has them), then the obstacle scan.  The
        obstacles' device arrays are made once per list object."""
        if P is None:
            P, _ = rollout_dense(model, X, U, sigma, S=S, nsub=nsub, pos_dim=pos_dim)
            self.samples = (S, P)   # for moving_obstacle_rows of the same step
        cached = getattr(self, "_obs_dev", None)
        if cached is None or cached[0] is not obstacles or cached[1][0].device != X.device:
            from . import _obstacle_arrays
            cached = self._obs_dev = (obstacles, _obstacle_arrays("obstacle_rows", obstacles, X.device))
        out = obstacle_scan(P, cached[1], cull=cull, J=J, analysis=False)
        return out["rec"], out["count"]

    def moving_obstacle_rows(self, model, X, U, sigma, S, nsub, pos_dim, tracks, cull, J, P=None):
        """(rec, count_seg, node_rec, node_count) of the moving-obstacle rows of every agent of the iterate (X, U) on
        this rank's own clocks sigma: the dense roll-out (P: as obstacle_rows), then the moving-obstacle scan.  The
        tracks' device arrays are made once per list object."""
        if P is None:
            P, _ = rollout_dense(model, X, U, sigma, S=S, nsub=nsub, pos_dim=pos_dim)
        cached = getattr(self, "_trk_dev", None)
        if cached is None or cached[0] is not tracks or cached[1][0].device != X.device:
            cached = self._trk_dev = (tracks, obstacle_tracks(tracks, X.device))
        out = moving_obstacle_scan(P, sigma, cached[1], cull=cull, J=J, analysis=False)
        return out["rec"], out["count"], out["node_rec"], out["node_count"]

    def append_collision_rows(self, X_all, i0, idx, rec, count_seg, rows, count, pos_dim, overflow):
        return append_collision_rows(X_all, i0, rec, count_seg, rows, count, pos_dim, idx=idx, overflow=overflow,
                                     check_index=False)   # idx comes from this rank's own agents

    def append_node_rows(self, X_all, i0, idx, node_rec, node_count, rows, count, pos_dim, overflow):
        return append_node_rows(X_all, i0, node_rec, node_count, rows, count, pos_dim, idx=idx, overflow=overflow,
                                check_index=False)

    def qp_solver(self, spec, N, device):
        return QPSolver(spec, N, device=device)

    def jacobi_update(self, status, X_sol, U_sol, X, U, tr, prev_cost, grow, tr_max, tie_rtol=0.0):
        return jacobi_update(status, X_sol, U_sol, X, U, tr, prev_cost, grow=grow, tr_max=tr_max, tie_rtol=tie_rtol)

    def jacobi_update_global(self, status, X_sol, U_sol, X, U, tr, prev_total, grow, tr_max, all_reduce=None):
        return jacobi_update_global(status, X_sol, U_sol, X, U, tr, prev_total, grow=grow, tr_max=tr_max,
                                    all_reduce=all_reduce)


@dataclass
class CouplingSpec:
    """Collision coupling of dist_scvx_3d.py:93-107.  The QP keeps the spec.j_max nearest rows per
    node; with check=True every dropped row is evaluated at the solution (collision_check) and the
    agents that violate one are re-solved with the j_max_hi nearest rows.  The culled problem is a
    relaxation of the reference's, so a solution that satisfies every row IS the reference's; agents
    still violating after the re-solve (more binding neighbours than j_max_hi) are counted in
    JacobiSCvx.last_check["overflow"].

    intersample_S > 0 adds continuous-time rows (single rank): every step the iterate is rolled out with
    intersample_S samples per segment, the intersample_J neighbours per (agent, segment) that pass closer than
    intersample_cull strictly between two nodes each become two node rows, and these are appended behind the node
    rows.  QPSpec.j_max (and j_max_hi in the re-solve) is then the total capacity per node: the node-level rows
    get j_max - 2 intersample_J of it.  Build-side option; the reference constrains the nodes only."""
    R: float = 2.3              # agent radius (dist_scvx_3d.py:211); rows use 2R
    cull_radius: float = 0.0    # <= 0: every neighbour (exact reference semantics)
    check: bool = True          # evaluate every reference row at the solution
    j_max_hi: int = 32          # nearest rows of the re-solve (the largest QP capacity class)
    check_tol: float = 1e-7     # row violation threshold (metres)
    intersample_S: int = 0      # dense samples per segment of the continuous-time rows; 0: off, nothing changes
    intersample_J: int = 2      # neighbours kept per (agent, segment)
    intersample_cull: float = 0.0   # pairs farther apart than this give no row; <= 0: 3R


@dataclass
class ObstacleRowsSpec:
    """Continuous-time obstacle rows, JacobiSCvx(..., obstacle_rows=ObstacleRowsSpec()).  The QP's own
    obstacle rows (QPSpec.obs) hold at the nodes only; with this option every step rolls the iterate out with S
    samples per segment, the J obstacles per (agent, segment) whose surface the chords come closest to strictly
    between two nodes (within cull of it) each become two node rows g.(p_t - pbar_t) >= v - S_t, and these are
    appended behind whatever collision rows the node already has (node rows, then pair records, then obstacle
    records).  They share the node's collision slack and w_coll; the QP kernel is not touched (no slack group of
    its own at w_obs, no chord row inside the QP).  QPSpec.j_max is the total capacity per node: the node-level
    collision rows get j_max - 2 intersample_J - 2 J of it.  Works with or without a CouplingSpec, at any world
    size (per agent and local: no collective).  Any model with a dense roll-out: the built-in ones and every
    scvx_hip.rtc.DeviceModel (the samples are its first QPSpec.pos_dim states).  Build-side option; the reference's Jacobi
    driver constrains the nodes only."""
    S: int = 8                  # dense samples per segment
    J: int = 2                  # obstacles kept per (agent, segment)
    cull: float = 0.0           # obstacles whose surface stays farther than this give no row; <= 0: the largest rho
    obstacles: Optional[Sequence] = None   # [(centre, total radius rho)]; None: QPSpec.obs, the node rows' list


@dataclass
class MovingObstaclesSpec:
    """Moving obstacles, JacobiSCvx(..., moving_obstacles=MovingObstaclesSpec(tracks)): things that move
    along a known track and are not ours to plan.  tracks: [(knots, (t0, t1), total radius rho)]
    (scvx_hip.obstacle_tracks), in real time; every agent meets them on its own clock sigma_i.  Every step rolls the
    iterate out with S samples per segment and scans the relative samples p - q_o(t): per node t < K-1 the J tracks
    closest to their surface at the node (within cull of it) give one node row each -- the QP kernel holds node rows
    for fixed centres only -- and per segment the J tracks that come closest strictly between two nodes give two node
    rows each, as the static obstacle records do.  Per node they follow whatever rows the node already has: collision
    node rows, pair records, static obstacle records, then the moving node rows, then the moving segment records.
    They take 3 J of QPSpec.j_max per node (J node rows, 2 J from the two adjoining segments), share the node's
    collision slack and w_coll, and leave the QP kernel untouched.  Works with or without a CouplingSpec and
    obstacle_rows, at any world size (per agent and local: this rank's sigma, no collective), for any model with a
    dense roll-out."""
    tracks: Sequence            # [(knots, (t0, t1), rho)], at least one
    S: int = 8                  # dense samples per segment
    J: int = 2                  # tracks kept per node and per (agent, segment)
    cull: float = 0.0           # tracks whose surface stays farther than this give no row; <= 0: the largest rho


class JacobiSCvx:
    """Device-resident Jacobi SCvx for this rank's agents [i0, i0 + N_local) of N_total.

    on_fail: what a failed subproblem (status 2) does to its agent's trust radius -- "halve" (the
             default) or "grow" (x2, at most tr_max, default tr0: an infeasible trust-region subproblem is the trust
             region being too small to reach x_final, the usual SCP remedy; for nonlinear models).
    tr_rule: "global" -- one trust region for all agents, halved when the total cost rises
             (dist_scvx_3d.py:248-252); "per_agent" -- the same rule applied to each agent's own
             cost (independent agents, configs C2/C3).
    tie_rtol: per-agent rule only -- an agent's radius halves when its cost exceeds the previous one by
             more than this relative margin (default 1e-9).  A converged agent's successive costs agree
             only to rounding, so the reference's strict test would halve its radius on the rounding of
             the cost sum, differently for every summation order (the per-agent rule is this build's; the
             reference's global rule keeps the strict test).
    fused_update: the bookkeeping in csrc/jacobi.hip (default): the per-agent rule in one launch, the global rule in two
             (per-agent costs, then one workgroup sums them in a fixed order and applies the strict test; at world > 1
             the local total is all-reduced in between); False runs the same rules as tensor ops.
    warm_start: each agent's QP starts from the primal-dual point of its previous solve when that one was
             optimal (QPSolver.solve(warm=...), include/scvx_hip.h): the next subproblem is the same agent's
             re-linearised at that solution.  The optimum and the stopping rule are unchanged; C3 needs
             ~2.4x fewer IPM iterations.  False: every solve starts cold (CVXOPT-style).
    warm_max_status: the previous solve qualifies when its status is <= this (0: optimal only; 1: also
             optimal_inaccurate, whose iterate meets the reduced tolerances).
    dispatch_order: "lpt" (default) -- when the agents outnumber the resident waves (one per SIMD: 4 x the
             GPU's CUs; C4), each QP launch deals them longest-first by their previous solve's IPM iterations
             (QPSolver.solve(order=...)), so a slot that frees up takes the next-longest solve (C4 85 -> 93
             SCvx-it/s); "none" -- always agent order, one launch.  Results do not depend on it.
             With every agent resident at once (C3, C5) an order alone gains nothing (dealing the long solves first
             only moves them onto shared CUs: C3 780 -> 764), but the launch lasts as long as its slowest wave, and
             the slowest agents are the same from step to step: where the agents outnumber the CUs, "lpt" launches
             the QP kernel twice (QPSolver.solve(order_tail=...), scvx_qp_solve_batched_split) -- the up to split_T
             agents whose last solve took at least split_thr IPM iterations on compute units they share with nobody
             (split_reserve "whole") or with one workgroup ("half"), everyone else as before, longest first.  A
             step in which no agent reached split_thr launches no tail agent, nor does one without
             split_short_per_tail shorter solves per tail agent (default: what a tail workgroup displaces, 3 or 1).
             The lists come from one selection launch (QPSolver.dispatch_lists), which also orders the
             agents-outnumber-waves case.  Built-in models and tr_rule="global" only (under the per-agent rule most
             steps have no tail and the fixed cost of two launches is all that is left: c3 -1.4 %).  The environment
             variable SCVX_QP_SPLIT=0 turns the split off (2: on also under the per-agent rule and where the agents
             do not outnumber the CUs); SCVX_QP_SPLIT_THR / _T / _RESERVE override the three settings (DESIGN §3.3
             "Split launch").
    obstacle_rows: an ObstacleRowsSpec adds continuous-time obstacle rows to every subproblem (see there); None
             (default): off, nothing changes.  The rows share the node's collision slack and w_coll; the QP kernel is
             not touched.
    moving_obstacles: a MovingObstaclesSpec adds node rows and continuous-time rows against obstacles that move along
             known tracks (see there); None (default): off, nothing changes.
    """

    def __init__(self, spec: QPSpec, x_init, x_final, sigma, tr0: float, coupling: Optional[CouplingSpec] = None,
                 tr_rule: str = "per_agent", group=None, nsub: Optional[int] = None, backend=None,
                 on_fail: str = "halve", tr_max: Optional[float] = None, fused_update: bool = True,
                 tie_rtol: float = 1e-9, warm_start: bool = True, warm_max_status: int = 0,
                 dispatch_order: str = "lpt", obstacle_rows: Optional["ObstacleRowsSpec"] = None,
                 split_thr: Optional[int] = None, split_T: Optional[int] = None,
                 split_reserve: Optional[str] = None, split_short_per_tail: Optional[int] = None,
                 moving_obstacles: Optional["MovingObstaclesSpec"] = None):
        import torch
        self.torch = torch
        self.backend = backend or HipBackend()
        self.spec = spec
        self.N = x_init.shape[0]
        self.device = x_init.device
        self.x_init, self.x_final, self.sigma = x_init, x_final, sigma
        self.coupling = coupling
        self.tr_rule = tr_rule
        if on_fail not in ("halve", "grow"):
            raise ValueError(f"on_fail must be 'halve' or 'grow', not {on_fail!r}")
        self.on_fail, self.tr_max = on_fail, float(tr0 if tr_max is None else tr_max)
        self.fused_update = fused_update
        self.tie_rtol = float(tie_rtol)
        self.warm_start = warm_start and spec.K >= 2 * model_dims(spec.model)[0]
        self.warm = None   # (N,) int32 device: the previous solve of the agent qualifies as a warm start
        self._warm_buf = None
        self.warm_max_status = int(warm_max_status)
        if dispatch_order not in ("lpt", "none"):
            raise ValueError(f"dispatch_order must be 'lpt' or 'none', not {dispatch_order!r}")
        self.dispatch_order = dispatch_order
        self.order = None  # (N,) int32 device: the next launch's dispatch order (longest previous solve first)
        cus = self._cu_count()
        resident = 4 * cus if cus else self.N
        self._lpt = dispatch_order == "lpt" and self.N > resident
        env = os.environ.get
        self.split_thr = int(env("SCVX_QP_SPLIT_THR") or (SPLIT_THR if split_thr is None else split_thr))
        self.split_T = min(int(env("SCVX_QP_SPLIT_T") or (SPLIT_T if split_T is None else split_T)), self.N)
        self.split_reserve = env("SCVX_QP_SPLIT_RESERVE") or (SPLIT_RESERVE if split_reserve is None else split_reserve)
        if self.split_reserve not in ("whole", "half"):
            raise ValueError(f"split_reserve must be 'whole' or 'half', not {self.split_reserve!r}")
        # a tail workgroup displaces the other three of its CU (one, sharing half of it) into a second round: the
        # selection forms a tail only while that many short solves per tail agent exist (0: no such limit)
        self.split_short_per_tail = int((3 if self.split_reserve == "whole" else 1) if split_short_per_tail is None
                                        else split_short_per_tail)
        # agents that do not outnumber the CUs share none: nothing to reserve (C2).  Under the per-agent rule every
        # agent's radius settles on its own and the counts level out at 5-6: most steps have no tail and would only pay
        # the two launches' fixed cost (c3: -1.4 %), so the split is for the global rule.  SCVX_QP_SPLIT=2 asks for it
        # in both cases.
        mode = env("SCVX_QP_SPLIT", SPLIT_DEFAULT)
        self._split = (dispatch_order == "lpt" and not self._lpt and bool(cus) and self.split_T >= 1
                       and isinstance(spec.model, str) and mode != "0"
                       and ((self.N > cus and tr_rule == "global") or mode == "2"))
        self.order_tail = None  # (split_T,) int32 device: the next launch's tail list (split launch)
        self.group = group
        # RK4 substeps of the FOH: default_nsub for this run's longest interval (one host read of max(sigma) here,
        # none per step; the quadrotor's count grows with the interval)
        self.nsub = nsub or default_nsub(spec.model, float(sigma.max().item()) if self.N else None, spec.K)
        self.solver = self.backend.qp_solver(spec, self.N, self.device)
        self.tr = torch.full((self.N,), float(tr0), dtype=torch.float64, device=self.device)
        self.prev_cost = torch.full((self.N,), float("inf"), dtype=torch.float64, device=self.device)
        self.prev_total = torch.full((1,), float("inf"), dtype=torch.float64, device=self.device)
        self.disc = None
        self.last_check = None
        self.world = 1
        self.rank = 0
        if group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(group)
            self.rank = torch.distributed.get_rank(group)
        self.i0 = self.rank * self.N
        self.N_total = self.N * self.world
        if coupling is not None:
            n, _ = model_dims(spec.model)
            self.X_all = torch.empty((self.N_total, spec.K, n), dtype=torch.float64, device=self.device)
            self.rows = torch.zeros((self.N, spec.K, spec.j_max, spec.pos_dim + 1), dtype=torch.float64,
                                    device=self.device)
            self.count = torch.zeros((self.N, spec.K), dtype=torch.int32, device=self.device)
        self._hi = None   # re-solve buffers of the full-row check (allocated at the first violation)
        self._is = None   # continuous-time rows (CouplingSpec.intersample_S > 0): settings and buffers
        if coupling is not None and coupling.intersample_S > 0:
            if self.world > 1:
                raise NotImplementedError("CouplingSpec.intersample_S at world > 1 needs the all-gather of the dense "
                                          "samples P (and L) across ranks before the scan, which is not implemented")
            S, J = int(coupling.intersample_S), int(coupling.intersample_J)
            if not 1 <= S <= 16 or not 1 <= J <= 8:
                raise ValueError(f"CouplingSpec: 1 <= intersample_S <= 16 and 1 <= intersample_J <= 8 required, got "
                                 f"{S}, {J}")
            j_node = spec.j_max - 2 * J
            if j_node < 1:   # (the re-solve runs only at j_max_hi > j_max, which then leaves room as well)
                raise ValueError(f"CouplingSpec.intersample_S > 0: QPSpec.j_max = {spec.j_max} is the total capacity "
                                 f"per node and must leave at least one node-level row next to the 2 x intersample_J = "
                                 f"{2 * J} continuous-time rows")
            cull = float(coupling.intersample_cull) if coupling.intersample_cull > 0 else 3.0 * coupling.R
            self._is = dict(S=S, J=J, per_node=2 * J, cull=cull, j_node=j_node, rec=None, count_seg=None,
                            rows_node=torch.zeros((self.N, spec.K, j_node, spec.pos_dim + 1), dtype=torch.float64,
                                                  device=self.device),
                            overflow=torch.zeros((1,), dtype=torch.int32, device=self.device))
        self._ob = None   # continuous-time obstacle rows (obstacle_rows): settings and buffers
        if obstacle_rows is not None:
            if not isinstance(spec.model, str) and not callable(getattr(spec.model, "rollout_dense", None)):
                raise NotImplementedError("obstacle_rows: the model offers no dense roll-out (rollout_dense): a built-in "
                                          "model name or a scvx_hip.rtc.DeviceModel is needed")
            S, J = int(obstacle_rows.S), int(obstacle_rows.J)
            if not 1 <= S <= 16 or not 1 <= J <= 8:
                raise ValueError(f"ObstacleRowsSpec: 1 <= S <= 16 and 1 <= J <= 8 required, got {S}, {J}")
            obstacles = list(spec.obs if obstacle_rows.obstacles is None else obstacle_rows.obstacles)
            if not obstacles:
                raise ValueError("ObstacleRowsSpec: no obstacles (neither in the option nor in QPSpec.obs)")
            J_pair = self._is["J"] if self._is is not None else 0
            j_node = spec.j_max - 2 * J_pair - 2 * J
            if j_node < (1 if coupling is not None else 0):
                raise ValueError(f"obstacle_rows: QPSpec.j_max = {spec.j_max} is the total capacity per node and must "
                                 f"hold the 2 x J = {2 * J} obstacle rows"
                                 + (f", the 2 x intersample_J = {2 * J_pair} pair rows" if J_pair else "")
                                 + (" and at least one node-level row" if coupling is not None else ""))
            cull = float(obstacle_rows.cull) if obstacle_rows.cull > 0 else max(float(r) for _, r in obstacles)
            self._ob = dict(S=S, J=J, per_node=2 * J, cull=cull, obstacles=obstacles, j_node=j_node, rec=None,
                            count_seg=None, overflow=torch.zeros((1,), dtype=torch.int32, device=self.device))
            if coupling is None:   # independent agents: the driver owns the rows, all of them obstacle rows
                self.rows = torch.zeros((self.N, spec.K, spec.j_max, spec.pos_dim + 1), dtype=torch.float64,
                                        device=self.device)
                self.count = torch.zeros((self.N, spec.K), dtype=torch.int32, device=self.device)
            elif self._is is not None:
                self._is["j_node"] = j_node
                self._is["rows_node"] = self._is["rows_node"][:, :, :j_node].contiguous()
            else:
                self._ob["rows_node"] = torch.zeros((self.N, spec.K, j_node, spec.pos_dim + 1), dtype=torch.float64,
                                                    device=self.device)
        self._mv = None   # moving obstacles (moving_obstacles): settings and buffers
        if moving_obstacles is not None:
            if not isinstance(spec.model, str) and not callable(getattr(spec.model, "rollout_dense", None)):
                raise NotImplementedError("moving_obstacles: the model offers no dense roll-out (rollout_dense): a "
                                          "built-in model name or a scvx_hip.rtc.DeviceModel is needed")
            S, J = int(moving_obstacles.S), int(moving_obstacles.J)
            if not 1 <= S <= 16 or not 1 <= J <= 8:
                raise ValueError(f"MovingObstaclesSpec: 1 <= S <= 16 and 1 <= J <= 8 required, got {S}, {J}")
            if spec.K > 64:
                raise ValueError(f"MovingObstaclesSpec: K <= 64 required (the records' limit), got {spec.K}")
            tracks = moving_obstacles.tracks
            if not isinstance(tracks, ObstacleTracks):
                tracks = list(tracks)
                if not tracks:
                    raise ValueError("MovingObstaclesSpec: no tracks")
            rmax = float(obstacle_tracks(tracks, "cpu")[3].max().item())   # (a list is validated here, on the host)
            earlier = self._records()
            j_node = spec.j_max - sum(s["per_node"] for s in earlier) - 3 * J
            if j_node < (1 if coupling is not None else 0):
                raise ValueError(f"moving_obstacles: QPSpec.j_max = {spec.j_max} is the total capacity per node and "
                                 f"must hold the 3 x J = {3 * J} moving-obstacle rows (J node rows, 2 J from the two "
                                 f"adjoining segments)"
                                 + "".join(f", the {s['per_node']} {n} rows" for s, n in
                                           ((self._is, "pair"), (self._ob, "obstacle")) if s is not None)
                                 + (" and at least one node-level row" if coupling is not None else ""))
            cull = float(moving_obstacles.cull) if moving_obstacles.cull > 0 else rmax
            self._mv = dict(S=S, J=J, per_node=3 * J, cull=cull, tracks=tracks, j_node=j_node, rec=None, count_seg=None,
                            node_rec=None, node_count=None,
                            overflow=torch.zeros((1,), dtype=torch.int32, device=self.device))
            for s in earlier:   # the node-level share shrinks for every set
                s["j_node"] = j_node
                if "rows_node" in s:
                    s["rows_node"] = s["rows_node"][:, :, :j_node].contiguous()
            if coupling is None:
                if not earlier:   # independent agents: the driver owns the rows, none of them node-level
                    self.rows = torch.zeros((self.N, spec.K, spec.j_max, spec.pos_dim + 1), dtype=torch.float64,
                                            device=self.device)
                    self.count = torch.zeros((self.N, spec.K), dtype=torch.int32, device=self.device)
            elif not earlier:
                self._mv["rows_node"] = torch.zeros((self.N, spec.K, j_node, spec.pos_dim + 1), dtype=torch.float64,
                                                    device=self.device)

    def _cu_count(self):
        """Compute units of this driver's GPU (0: no GPU -- stub backends; every dispatch option is then off)"""
        if self.device.type != "cuda":
            return 0
        return int(self.torch.cuda.get_device_properties(self.device).multi_processor_count)

    def _records(self):
        """The record sets appended behind the node rows, in order: pair records, static obstacle records, moving
        obstacles.  Each states the rows it may add to a node (per_node) and is appended by _append."""
        return [s for s in (self._is, self._ob, self._mv) if s is not None]

    def _append(self, s, X_all, i0, idx, rows, count):
        """The appends of record set s behind the count rows of every node: a moving-obstacle set's node rows first
        (one row per record), then a set's segment records (two rows per record).  idx: the re-solve's agents."""
        if s.get("node_rec") is not None:
            self.backend.append_node_rows(X_all, i0, idx, s["node_rec"], s["node_count"], rows, count,
                                          self.spec.pos_dim, s["overflow"])
        return self.backend.append_collision_rows(X_all, i0, idx, s["rec"], s["count_seg"], rows, count,
                                                  self.spec.pos_dim, s["overflow"])

    def _hi_buffers(self):
        """Rows, counts and a QPSolver at j_max_hi sized for all N local agents, allocated once: a re-solve
        uses their leading n_bad entries (QPSolver.solve(n=...))."""
        if self._hi is None:
            torch, spec, c = self.torch, self.spec, self.coupling
            spec_hi = dataclasses.replace(spec, j_max=c.j_max_hi)
            self._hi = dict(rows=torch.zeros((self.N, spec.K, c.j_max_hi, spec.pos_dim + 1), dtype=torch.float64,
                                             device=self.device),
                            count=torch.zeros((self.N, spec.K), dtype=torch.int32, device=self.device),
                            solver=self.backend.qp_solver(spec_hi, self.N, self.device))
            if self._records():   # the node-level share of j_max_hi, before the continuous-time rows join it
                j_node = c.j_max_hi - sum(s["per_node"] for s in self._records())
                self._hi["rows_node"] = torch.zeros((self.N, spec.K, j_node, spec.pos_dim + 1), dtype=torch.float64,
                                                    device=self.device)
        return self._hi

    def _enforce_all_rows(self, X_all, X, U, out):
        """Make the culled coupling exact: evaluate every reference row at the solution, re-solve the
        violating agents with the j_max_hi nearest rows (computed for those agents only), count what still
        violates (overflow)."""
        torch, spec, c = self.torch, self.spec, self.coupling
        ok = out["status"] != 2

        def violators():
            viol, _ = self.backend.collision_check(X_all, self.i0, out["X"], out["slack_coll"], c.R, spec.pos_dim,
                                                   c.check_tol)
            return (viol.sum(dim=1) > 0) & ok

        bad = violators()
        n_bad = int(bad.sum().item())   # one host read per SCvx iteration
        self.last_check = {"violated": n_bad, "resolved": 0, "overflow": n_bad}
        if n_bad == 0 or spec.j_max >= c.j_max_hi:
            return out
        idx = bad.nonzero().flatten()
        hi = self._hi_buffers()
        gidx = (idx + self.i0).to(torch.int32)
        if not self._records():
            self.backend.collision_rows_indexed(X_all, gidx, c.R, c.j_max_hi, spec.pos_dim, c.cull_radius, hi["rows"],
                                                hi["count"])
        else:   # j_max_hi less every set's rows per node, then the step's own records of those agents, set by set
            j_node = c.j_max_hi - sum(s["per_node"] for s in self._records())
            self.backend.collision_rows_indexed(X_all, gidx, c.R, j_node, spec.pos_dim, c.cull_radius,
                                                hi["rows_node"], hi["count"])
            hi["rows"][:n_bad, :, :j_node].copy_(hi["rows_node"][:n_bad])
            for s in self._records():
                self._append(s, X_all, self.i0, gidx, hi["rows"], hi["count"])
        g = lambda t: t.index_select(0, idx).contiguous()  # noqa: E731
        o2 = hi["solver"].solve(g(self.disc), g(self.sigma), g(X), g(U), g(self.x_init), g(self.x_final), g(self.tr),
                                hi["rows"][:n_bad], hi["count"][:n_bad], n=n_bad)
        out = {k: v.clone() for k, v in out.items()}
        for k in ("X", "U", "slack_coll", "nu", "obj", "status", "iters"):
            out[k].index_copy_(0, idx, o2[k])
        ok = out["status"] != 2
        still = int(violators().sum().item())
        self.last_check.update(resolved=n_bad - still, overflow=still)
        return out

    def gather_states(self, X, async_op=False):
        """All-gather the local states (N,K,n) into X_all (N_total,K,n) -- RCCL over xGMI.  async_op: return
        a handle whose wait() makes the current stream wait for the collective (overlap with the FOH)."""
        if self.world == 1:
            self.X_all.copy_(X)
            return None if async_op else self.X_all
        work = self.torch.distributed.all_gather_into_tensor(self.X_all, X.contiguous(), group=self.group,
                                                             async_op=async_op)
        return work if async_op else self.X_all

    def separation(self, X, U, S=8):
        """Continuous-time closest approach of every agent to every other at the iterate (X, U)
        (scvx_hip.fleet_separation: S samples per segment, the FOH's substep count, the template's pos_dim) --
        the between-nodes check the node-level collision rows cannot give.  Single rank only."""
        if self.world > 1:
            raise NotImplementedError("JacobiSCvx.separation at world > 1 needs the all-gather of the dense samples P "
                                      "(and L) across ranks before the scan, which is not implemented")
        return fleet_separation(self.spec.model, X, U, self.sigma, S=S, nsub=self.nsub, pos_dim=self.spec.pos_dim)

    def obstacle_clearance(self, X, U, S=8):
        """Continuous-time clearance of every agent to every obstacle at the iterate (X, U)
        (scvx_hip.fleet_obstacle_clearance: S samples per segment, the FOH's substep count, the template's pos_dim)
        -- the between-nodes check the node-level obstacle rows cannot give.  The obstacles are the obstacle_rows
        option's, else QPSpec.obs; their radii are total radii (robot_radius = 0).  Per agent and local: any world."""
        obstacles = self._ob["obstacles"] if self._ob is not None else list(self.spec.obs)
        return fleet_obstacle_clearance(self.spec.model, X, U, self.sigma, obstacles, 0.0, S=S, nsub=self.nsub,
                                        pos_dim=self.spec.pos_dim)

    def moving_obstacle_clearance(self, X, U, S=8):
        """Continuous-time clearance of every agent to every moving obstacle of the moving_obstacles option at the
        iterate (X, U), each agent on its own clock (scvx_hip.fleet_moving_obstacle_clearance: S samples per segment,
        the FOH's substep count, the template's pos_dim; the radii are total radii).  Per agent and local: any world."""
        if self._mv is None:
            raise ValueError("JacobiSCvx.moving_obstacle_clearance needs the moving_obstacles option (its tracks)")
        return fleet_moving_obstacle_clearance(self.spec.model, X, U, self.sigma, self._mv["tracks"], 0.0, S=S,
                                               nsub=self.nsub, pos_dim=self.spec.pos_dim)

    def _mark(self, marks, name):
        """Record a timing event named `name` on the current (launch) stream (marks: list or None)."""
        if marks is not None:
            e = self.torch.cuda.Event(enable_timing=True)
            e.record(self.torch.cuda.current_stream())
            marks.append((name, e))

    def step(self, X, U, marks=None):
        """One SCvx iteration; returns the new (X, U) and the raw solver outputs.
        marks: optional list; (stage, event) pairs are appended on the launch stream -- "start", then
        the end of "foh", "gather" (all-gather), "rows" (collision rows), "isrows" (with CouplingSpec.intersample_S > 0: dense
        roll-out, pair-rows scan and append), "obsrows" (with obstacle_rows: dense roll-out unless shared, obstacle scan and
        append), "movrows" (with moving_obstacles: dense roll-out unless shared, moving-obstacle scan, node-row and record
        appends), "qp" (the QP kernel),
        "check" (full-row check + re-solve) and "update" (bookkeeping); a stage's time is the
        difference to the previous mark."""
        torch = self.torch
        spec = self.spec
        self._mark(marks, "start")
        # the state all-gather (RCCL, its own stream) is issued first and overlaps the FOH launch
        work = self.gather_states(X, async_op=True) if self.coupling is not None else None
        self.disc = self.backend.foh(spec.model, X, U, self.sigma, self.nsub, self.disc)
        self._mark(marks, "foh")
        rows = count = X_all = None
        if self.coupling is not None:
            if work is not None:
                work.wait()
            X_all = self.X_all
            self._mark(marks, "gather")
            if not self._records():
                rows, count = self.backend.collision_rows(X_all, self.i0, self.N, self.coupling.R, spec.j_max,
                                                          spec.pos_dim, self.coupling.cull_radius, self.rows, self.count)
                self._mark(marks, "rows")
            else:
                # the node rows take j_max - 2 (J_pair + J_obs) slots of every node; the continuous-time rows of the
                # current iterate (two per record: the segment's two nodes) follow them
                first = self._records()[0]
                j_node, rows_node = first["j_node"], first["rows_node"]
                self.backend.collision_rows(X_all, self.i0, self.N, self.coupling.R, j_node, spec.pos_dim,
                                            self.coupling.cull_radius, rows_node, self.count)
                self.rows[:, :, :j_node].copy_(rows_node)
                rows, count = self.rows, self.count
                self._mark(marks, "rows")
            if self._is is not None:
                s = self._is
                s["rec"], s["count_seg"] = self.backend.intersample_pair_rows(
                    spec.model, X, U, self.sigma, s["S"], self.nsub, spec.pos_dim, self.coupling.R, s["cull"], s["J"])
                s["overflow"].zero_()
                rows, count, _ = self._append(s, X_all, self.i0, None, self.rows, self.count)
                self._mark(marks, "isrows")
        # the dense samples of this iterate, by sample count: a set's roll-out serves the later sets of the step
        have = {}

        def take_samples():
            made = getattr(self.backend, "samples", None)
            if made is not None:
                have[made[0]] = made[1]
                self.backend.samples = None

        take_samples()
        i0_rows = self.i0 if self.coupling is not None else 0
        if self.coupling is None and self._records():   # independent agents: no node rows, the iterate is its own X_all
            self.count.zero_()
            X_all = X if X.is_contiguous() else X.contiguous()
        if self._ob is not None:
            s = self._ob
            share = {"P": have[s["S"]]} if s["S"] in have else {}
            s["rec"], s["count_seg"] = self.backend.obstacle_rows(
                spec.model, X, U, self.sigma, s["S"], self.nsub, spec.pos_dim, s["obstacles"], s["cull"], s["J"], **share)
            take_samples()
            s["overflow"].zero_()
            rows, count, _ = self._append(s, X_all, i0_rows, None, self.rows, self.count)
            self._mark(marks, "obsrows")
        if self._mv is not None:
            s = self._mv
            share = {"P": have[s["S"]]} if s["S"] in have else {}
            s["rec"], s["count_seg"], s["node_rec"], s["node_count"] = self.backend.moving_obstacle_rows(
                spec.model, X, U, self.sigma, s["S"], self.nsub, spec.pos_dim, s["tracks"], s["cull"], s["J"], **share)
            s["overflow"].zero_()
            rows, count, _ = self._append(s, X_all, i0_rows, None, self.rows, self.count)
            self._mark(marks, "movrows")
        kw = {"order": self.order} if self.order is not None else {}
        if self.order_tail is not None:
            kw.update(order_tail=self.order_tail, reserve=self.split_reserve)
        out = self.solver.solve(self.disc, self.sigma, X, U, self.x_init, self.x_final, self.tr, rows, count,
                                warm=self.warm, **kw)
        if self.warm_start:   # one launch: the comparison written straight into the int32 flag buffer
            if self._warm_buf is None:
                self._warm_buf = torch.empty((self.N,), dtype=torch.int32, device=self.device)
            self.warm = torch.le(out["status"], self.warm_max_status, out=self._warm_buf)
        if self._lpt and getattr(self.solver, "supports_order", False):
            if getattr(self.solver, "supports_split", False):   # one launch: the stable longest-first sort
                self.order = self.solver.dispatch_lists(self.spec.max_iter + 1, 0)[1]
            else:
                self.order = torch.argsort(out["iters"], descending=True, stable=True).to(torch.int32)
        elif self._split and getattr(self.solver, "supports_split", False):
            self.order_tail, self.order = self.solver.dispatch_lists(self.split_thr, self.split_T,
                                                                     self.split_short_per_tail)
        self._mark(marks, "qp")
        if self.coupling is not None and self.coupling.check:
            out = self._enforce_all_rows(X_all, X, U, out)
            if self._is is not None:
                # continuous-time rows that did not fit a node's capacity, in this step's solve and re-solve (none
                # by construction: the node rows leave 2J slots free)
                self.last_check["is_overflow"] = int(self._is["overflow"].item())
            if self._ob is not None:   # the same for the obstacle rows
                self.last_check["obs_overflow"] = int(self._ob["overflow"].item())
            if self._mv is not None:   # and for the moving obstacles' rows
                self.last_check["mov_overflow"] = int(self._mv["overflow"].item())
            self._mark(marks, "check")
        # an agent whose subproblem failed numerically (status 2) rejects the step: it keeps its
        # iterate (its output may be non-finite and would otherwise reach every other agent through
        # the collision all-gather) and halves its own trust radius so the next subproblem differs.
        # The reference aborts the whole run instead (cvxpy raises SolverError, dist_scvx_3d.py:110).
        fused = getattr(self.backend, "jacobi_update", None)
        if self.fused_update and self.tr_rule == "per_agent" and fused is not None:
            # one launch for the update, the cost rule and the failure rule (csrc/jacobi.hip)
            Xn, Un = fused(out["status"], out["X"], out["U"], X, U, self.tr, self.prev_cost, self.on_fail == "grow",
                           self.tr_max, self.tie_rtol)
            self._mark(marks, "update")
            return Xn, Un, out
        fused_g = getattr(self.backend, "jacobi_update_global", None)
        if self.fused_update and self.tr_rule == "global" and fused_g is not None:
            ar = None
            if self.world > 1:
                ar = lambda t: torch.distributed.all_reduce(t, group=self.group)  # noqa: E731
            Xn, Un = fused_g(out["status"], out["X"], out["U"], X, U, self.tr, self.prev_total, self.on_fail == "grow",
                             self.tr_max, all_reduce=ar)
            self._mark(marks, "update")
            return Xn, Un, out
        failed = out["status"] == 2
        ok = (~failed)[:, None, None]
        Xn, Un = torch.where(ok, out["X"], X), torch.where(ok, out["U"], U)
        # cost_fcn (dist_scvx_3d.py:131-138) and the trust-region halving rule (:250-252)
        cost = (Un[:, :-1, :] * Un[:, :-1, :]).sum(dim=(1, 2))
        if self.tr_rule == "global":
            total = cost.sum().reshape(1)
            if self.world > 1:
                torch.distributed.all_reduce(total, group=self.group)
            shrink = (total > self.prev_total).to(torch.float64)
            self.tr.mul_(1.0 - 0.5 * shrink)
            self.prev_total.copy_(total)
        else:
            shrink = (cost > self.prev_cost * (1.0 + self.tie_rtol)).to(torch.float64)
            self.tr.mul_(1.0 - 0.5 * shrink)
            self.prev_cost.copy_(cost)
        if self.on_fail == "grow":
            self.tr.mul_(1.0 + failed.to(torch.float64)).clamp_(max=self.tr_max)
        else:
            self.tr.mul_(1.0 - 0.5 * failed.to(torch.float64))
        self._mark(marks, "update")
        return Xn, Un, out
