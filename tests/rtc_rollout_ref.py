"""TEST INFRASTRUCTURE ONLY -- the dense roll-out (csrc/foh_body.hpp rollout_dense_body) restated in numpy for ANY
model given as its f(x, u), the models of the run-time roll-out's tests, and the margins of their row-record
fixture.

  * dense_rk4_f: separation_ref.dense_rk4 with the model's f as an argument: sample s of a segment by s*sub RK4
    steps of T/(S sub) from the node, through oracle.intersample_np._rollout (the kernel's step sequence); the
    length is separation_ref.polyline_length;
  * the models: tests/custom_models.py's KinematicCar (launch parameter L) and TripleInt3D, and two tiny ones
    written as C expressions, n_x = 2 (f = [x1, u0 - p0 x1]) and n_x = 1 (f = [u0 - p0 x0]), each with its numpy f;
  * retraced(name): the DeviceModel re-traced from the drop-in double integrator / unicycle (from_callables);
  * ROWS / row_margins: the obstacle of the row-record test and the project's margin rule
    (tests/test_collision_ref_cpu.py: GAP = 1e-9) for the selections on an iterate of the head-on fixture.

Layouts are the kernels': X (N,K,n), U (N,K,m), sigma (N,), P (N,K-1,S+1,3), L (N,K-1)."""
import functools

import numpy as np

import custom_models as cm
import intersample_rows_ref as ir
import obstacle_rows_ref as orf
import separation_ref as sr
from oracle import intersample_np

GAP = 1e-9
SHAPES = [(5, 4), (70, 2)]                 # (N, K): 15 lanes of one block; one segment per agent, 64 + 6 lanes
S_NSUB = [(1, 1), (3, 7), (16, 16)]
P_TINY = 0.4                               # p[0] of the two tiny models


def dense_rk4_f(f, X, U, sigma, S, sub, pos_dim):
    """P, L of the roll-out of x' = f(x, u) by the kernel's step sequence (separation_ref.dense_rk4 for any f)."""
    N, K, _ = X.shape
    P = np.zeros((N, K - 1, S + 1, 3))
    for a in range(N):
        T = float(sigma[a]) / (K - 1)
        for k in range(K - 1):
            P[a, k, 0, :pos_dim] = X[a, k, :pos_dim]
            for s in range(1, S + 1):
                x = intersample_np._rollout(f, X[a, k], U[a, k], U[a, k + 1], T, s / S, s * sub)
                P[a, k, s, :pos_dim] = x[:pos_dim]
    return P, sr.polyline_length(P)


# ------------------------------------------------------------------ the models: numpy f and DeviceModel
def car_f(L):
    return lambda x, u: np.array([x[3] * np.cos(x[2]), x[3] * np.sin(x[2]), x[3] * np.tan(u[1]) / L, u[0]])


def triple_f(c=cm.TripleInt3D.params["c"]):
    return lambda x, u: np.concatenate([x[3:6], x[6:9] - c * x[3:6], u])


def tiny2_f(p=P_TINY):
    return lambda x, u: np.array([x[1], u[0] - p * x[1]])


def tiny1_f(p=P_TINY):
    return lambda x, u: np.array([u[0] - p * x[0]])


@functools.lru_cache(maxsize=None)
def device_model(name):
    """car (from_sympy, launch parameter L = 2.5), triple (from_callables), tiny2 / tiny1 (C expressions, p[0])."""
    from scvx_hip.rtc import DeviceModel
    if name == "car":
        m = cm.KinematicCar()
        return DeviceModel.from_sympy(m.x_sym, m.u_sym, m.f_param, p_syms=m.p_sym, params=[2.5])
    if name == "triple":
        m = cm.TripleInt3D()
        return DeviceModel.from_callables(*m.get_equations(), m.n_x, m.n_u)
    if name == "tiny2":
        return DeviceModel(2, 1, ["x[1]", "u[0] - p[0]*x[1]"], A=["0", "1", "0", "-p[0]"], B=["0", "1"],
                           params=[P_TINY], name="tiny2")
    if name == "tiny1":
        return DeviceModel(1, 1, ["u[0] - p[0]*x[0]"], A=["-p[0]"], B=["1"], params=[P_TINY], name="tiny1")
    raise KeyError(name)


MODEL_F = {"car": lambda: car_f(2.5), "triple": triple_f, "tiny2": tiny2_f, "tiny1": tiny1_f}
# (model, pos_dim) of the samples-against-the-restatement test
CASES = [("car", 2), ("triple", 3), ("tiny2", 1), ("tiny2", 2), ("tiny1", 1)]


@functools.lru_cache(maxsize=None)
def retraced(name):
    """The drop-in "di" / "unicycle" model re-traced into a DeviceModel: the built-in kernels' dynamics through
    hipRTC."""
    from scvx_hip.rtc import DeviceModel
    from SCvx.models.double_integrator_model import DoubleIntegratorModel
    from SCvx.models.unicycle_model import UnicycleModel
    m = {"di": DoubleIntegratorModel, "unicycle": UnicycleModel}[name]()
    return DeviceModel.from_callables(*m.get_equations(), m.n_x, m.n_u)


DIMS = {"car": (4, 2), "triple": (9, 3), "tiny2": (2, 1), "tiny1": (1, 1)}


def inputs(name, N, K, seed=3):
    """Random (X, U, sigma) of a model, every entry bounded away from zero (as separation_ref.random_fleet's speeds:
    the polyline lengths stay well above rounding): states of magnitude 0.5 .. 1.5; inputs 0.3 .. 0.6 for the car
    (a steering angle) and 1 .. 2 for the others, whose f = u - p x can then not cancel."""
    n, m = DIMS[name]
    rng = np.random.default_rng(seed + 17 * N + K)

    def mag(lo, hi, shape):
        return rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)

    lo, hi = (0.3, 0.6) if name == "car" else (1.0, 2.0)
    return mag(0.5, 1.5, (N, K, n)), mag(lo, hi, (N, K, m)), rng.uniform(1.0, 3.0, N)


@functools.lru_cache(maxsize=None)
def reference(name, N, K, S, nsub, pos_dim):
    """The restatement's (P, L) of inputs(name, N, K) at the model's default parameters (computed once, read-only)."""
    X, U, sig = inputs(name, N, K)
    P, L = dense_rk4_f(MODEL_F[name](), X, U, sig, S, -(-nsub // S), pos_dim)
    P.setflags(write=False)
    L.setflags(write=False)
    return P, L


def clearance_rollout_f(f, X, U, dt, nsub, center, total_radius, resolution):
    """separation_ref.clearance_rollout for any f: h_cont of SCvx.utils.analysis.compute_intersample_clearance by the
    same chunked RK4 (chunks of 16 samples; the state at a chunk's start by nsub steps from the node)."""
    c = np.asarray(center, float).reshape(-1)
    pd, K, res = c.size, X.shape[1], resolution
    h = np.empty((K - 1, res))
    for k in range(K - 1):
        xk, u0, u1 = X[:, k], U[:, k], U[:, k + 1]
        for i0 in range(0, res, 16):
            cnt = min(16, res - i0)
            t0, t1 = i0 / res, (i0 + cnt) / res
            ua, ub = u0 + t0 * (u1 - u0), u0 + t1 * (u1 - u0)
            xs = intersample_np._rollout(f, xk, u0, ua, t0 * dt, 1.0, nsub) if i0 else np.array(xk, float)
            sub = -(-nsub // cnt)
            for s in range(cnt):
                x = intersample_np._rollout(f, xs, ua, ub, (t1 - t0) * dt, s / cnt, s * sub) if s else xs
                h[k, i0 + s] = np.linalg.norm(x[:pd] - c) - total_radius
    return h.reshape(-1)


# ------------------------------------------------------------------ the row-record fixture
# the pair rows are the head-on fixture's own (R, the driver's cull = 3R, J); the obstacle stands above the
# crossing at the origin, its surface within `cull` of both paths
ROWS = dict(S=ir.HEAD_ON["S"], R=ir.HEAD_ON["R"], pair_cull=3.0 * ir.HEAD_ON["R"], J=ir.HEAD_ON["J"],
            obstacles=[((0.0, 0.0, 2.2), 1.0)], obs_cull=2.0)


def _inner_margin(D, Sx, A, S):
    """How far the decision `0 < alpha' < 1` is from turning over, for relative positions D (..., S+1, 3) and the
    selected (s, a): inside, the distance of alpha' = (s + a) / S from 0 and 1; at an end of the segment (a clipped
    to 0 in the first chord or to 1 in the last), how far the chord's unclipped parameter -d0.e / e.e lies outside
    [0, 1]."""
    al = (Sx + A) / S
    d0 = np.take_along_axis(D, Sx[..., None, None], axis=-2)[..., 0, :]
    d1 = np.take_along_axis(D, Sx[..., None, None] + 1, axis=-2)[..., 0, :]
    e = d1 - d0
    with np.errstate(divide="ignore", invalid="ignore"):   # an agent against itself: masked by the caller
        t = -(d0 * e).sum(-1) / (e * e).sum(-1)
    inner = (al > 0.0) & (al < 1.0)
    return np.where(inner, np.minimum(al, 1.0 - al), np.maximum(-t, t - 1.0))


def row_margins(X, U, sig):
    """The margin rule on the iterate (X, U) of the head-on fixture, on the restatement's samples: every distance
    that takes part in the pair-rows and the obstacle-rows selection is more than GAP (relative) away from its cull
    threshold and from the next candidate's, and every decision "strictly between two nodes" is more than GAP
    from turning over (_inner_margin).  A change of the samples of 1e-12 cannot then change a count.  Returns (pair count,
    obstacle count) per (agent, segment)."""
    r = ROWS
    S = r["S"]
    P, _ = sr.dense_closed_form("di", X, U, sig, S, 3)
    scale = np.abs(P).max()
    # pairs: dist against cull
    Q, Sx, A, _ = ir.pair_minima(P)
    d = np.sqrt(Q)
    other = ~np.eye(P.shape[0], dtype=bool)[:, :, None] & np.ones_like(Q, bool)
    cand = ir.candidates(Q, Sx, A, S, r["pair_cull"])
    assert cand.any() and (~cand & other).any()
    assert (np.abs(d[other] - r["pair_cull"]) > GAP * scale).all()
    D = P[None, :] - P[:, None]                 # [j, i] = p_i - p_j, as pair_minima's first axis is j
    assert (_inner_margin(D, Sx, A, S)[other] > GAP).all() and (d[other] > GAP * scale).all()
    ds = np.sort(np.where(cand, d, np.inf), axis=0)
    both = np.isfinite(ds[1]) if ds.shape[0] > 1 else np.zeros(ds.shape[1:], bool)
    assert (ds[1][both] - ds[0][both] > GAP * scale).all()
    # obstacles: v = rho - dist against -cull
    c, rho = orf.pad_centers(r["obstacles"])
    Qo, So, Ao, _ = orf.obstacle_minima(P, c)
    V = orf.values(Qo, rho)
    cando = orf.candidates(Qo, So, Ao, S, rho, r["obs_cull"])
    assert cando.any() and (~cando).any()
    assert (np.abs(V + r["obs_cull"]) > GAP * scale).all()
    Do = P[None, :] - c[:, None, None, None, :]
    assert (_inner_margin(Do, So, Ao, S) > GAP).all() and (np.sqrt(Qo) > GAP * scale).all()
    vs = -np.sort(np.where(cando, -V, np.inf), axis=0)
    if vs.shape[0] > 1:
        both = np.isfinite(vs[1])
        assert (vs[0][both] - vs[1][both] > GAP * scale).all()
    return np.minimum(cand.sum(0), r["J"]), np.minimum(cando.sum(0), r["J"])
