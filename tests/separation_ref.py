"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the fleet separation analysis (csrc/separation.hip).

  * dense samples of every segment's roll-out two ways: the closed-form cubic / quadratic of the double /
    single integrator, and fixed-step RK4 with the kernel's `sub` steps between samples through
    oracle/models_np.py and oracle/intersample_np._rollout (imported, not edited);
  * the chord scan with the kernel's first-minimum rule (j ascending, s ascending, strictly smaller);
  * a brute-force continuous truth for the double integrator: the cubic on a fine grid;
  * the node-level minima of the reference's SCvx/utils/analysis.py:10-62, vectorised.

Layouts are the kernels': X (N,K,n), U (N,K,m), sigma (N,), P (N,K-1,S+1,3), L (N,K-1)."""
import numpy as np

from oracle import intersample_np, models_np


def polyline_length(P):
    return np.sqrt((np.diff(P, axis=2) ** 2).sum(-1)).sum(-1)


def dense_closed_form(model, X, U, sigma, S, pos_dim=3):
    """P, L for "di" (p0 + v0 t + u0 t^2/2 + du t^3/(6T)) and "si" (p0 + u0 t + du t^2/(2T)), t = s/S T."""
    N, K, _ = X.shape
    T = (np.asarray(sigma, float) / (K - 1))[:, None, None, None]
    t = (np.arange(S + 1) / S)[None, None, :, None] * T
    u0, du = U[:, :-1, None, :], (U[:, 1:] - U[:, :-1])[:, :, None, :]
    p0 = X[:, :-1, None, 0:3]
    if model == "di":
        p = p0 + X[:, :-1, None, 3:6] * t + u0 * t ** 2 / 2.0 + du * t ** 3 / (6.0 * T)
    elif model == "si":
        p = p0 + u0 * t + du * t ** 2 / (2.0 * T)
    else:
        raise ValueError(model)
    P = np.zeros((N, K - 1, S + 1, 3))
    P[..., :pos_dim] = p[..., :pos_dim]
    P[:, :, 0, :pos_dim] = X[:, :-1, :pos_dim]
    return P, polyline_length(P)


def dense_rk4(model, X, U, sigma, S, sub, pos_dim):
    """P, L by RK4 from the node with s*sub steps of T/(S sub) up to sample s (the kernel's step sequence)."""
    f = models_np.MODELS[model][2]()[0]
    N, K, _ = X.shape
    P = np.zeros((N, K - 1, S + 1, 3))
    for a in range(N):
        T = float(sigma[a]) / (K - 1)
        for k in range(K - 1):
            P[a, k, 0, :pos_dim] = X[a, k, :pos_dim]
            for s in range(1, S + 1):
                x = intersample_np._rollout(f, X[a, k], U[a, k], U[a, k + 1], T, s / S, s * sub)
                P[a, k, s, :pos_dim] = x[:pos_dim]
    return P, polyline_length(P)


def chord(d0, d1):
    """(alpha, dist^2) of the closest approach of d0 + a (d1 - d0), a in [0, 1], to the origin (last axis = xyz)."""
    e = d1 - d0
    ee = (e * e).sum(-1)
    de = (d0 * e).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        al = np.where(ee == 0.0, 0.0, np.clip(-de / np.where(ee == 0.0, 1.0, ee), 0.0, 1.0))
    c = d0 + al[..., None] * e
    return al, (c * c).sum(-1)


def chord_scan(P, i0=0, n_local=None):
    """sep, j, s, alpha (n_local, K-1) of local agents [i0, i0+n_local): first minimum over j ascending, then s."""
    N, Km1, S1, _ = P.shape
    n_local = N - i0 if n_local is None else n_local
    Pi = P[i0:i0 + n_local]
    best = np.full((n_local, Km1), np.inf)
    bj = np.full((n_local, Km1), -1)
    bs = np.full((n_local, Km1), -1)
    ba = np.zeros((n_local, Km1))
    me = np.arange(i0, i0 + n_local)[:, None]
    for j in range(N):
        d = Pi - P[j][None]
        for s in range(S1 - 1):
            al, q = chord(d[:, :, s], d[:, :, s + 1])
            take = (q < best) & (me != j)
            best, bj, bs, ba = np.where(take, q, best), np.where(take, j, bj), np.where(take, s, bs), np.where(take, al, ba)
    return np.sqrt(best), bj, bs, ba


def chord_dist(P, i, k, j, s, alpha):
    """||d0 + alpha (d1 - d0)|| of the reported (j, s, alpha) for arrays i, k, j, s, alpha of one shape."""
    d0 = P[i, k, s] - P[j, k, s]
    d1 = P[i, k, s + 1] - P[j, k, s + 1]
    c = d0 + alpha[..., None] * (d1 - d0)
    return np.sqrt((c * c).sum(-1))


def di_truth(X, U, sigma, M=2000):
    """Per (agent, segment) the minimum over j != i of ||p_i - p_j|| on M+1 points of the segment's exact cubic,
    at equal normalised time."""
    P, _ = dense_closed_form("di", X, U, sigma, M)
    N = X.shape[0]
    out = np.full((N, X.shape[1] - 1), np.inf)
    for i in range(N):
        d = np.sqrt(((P[i][None] - P) ** 2).sum(-1)).min(-1)   # (N, K-1)
        d[i] = np.inf
        out[i] = d.min(0)
    return out


def di_chord_bound(U, sigma, K, S):
    """max ||r''|| h^2 / 8 with ||r''|| <= 2 max(sigma^2 ||u||) and h = 1 / ((K-1) S) (normalised time)."""
    a = (np.asarray(sigma, float)[:, None] ** 2 * np.sqrt((U ** 2).sum(-1))).max()
    return 2.0 * a * (1.0 / ((K - 1) * S)) ** 2 / 8.0


def pair_min_distance(X, rows=3):
    """d_mat of min_inter_agent_distance (analysis.py:10-31): min_k ||X_i[k,:rows] - X_j[k,:rows]||."""
    p = X[:, :, :rows]
    return np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)).min(-1)


def obstacle_min_distance(X, centers, radii, robot_radius):
    """d_mat of min_agent_obstacle_distance (analysis.py:34-62)."""
    d = np.sqrt(((X[:, None, :, 0:3] - np.asarray(centers, float)[None, :, None, :]) ** 2).sum(-1))
    return (d - (robot_radius + np.asarray(radii, float))[None, :, None]).min(-1)


def clearance_rollout(model, X, U, dt, nsub, center, total_radius, resolution):
    """h_cont of SCvx.utils.analysis.compute_intersample_clearance by the same chunked RK4: X (n,K), U (m,K);
    chunk starts i0 = 0, 16, ..: the state at t0 = i0/res by nsub steps from the node, then sample s of the
    chunk by s*sub steps of the chunk's own interval, sub = ceil(nsub / chunk length)."""
    f = models_np.MODELS[model][2]()[0]
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


def random_fleet(model, N, K, seed):
    """Random inputs (X, U, sigma) with positions in a +-6 box and speeds bounded away from zero (so that the
    polyline lengths are well above rounding).  "di" / "si": positions uniform in the box.  "unicycle" (planar:
    N agents uniform in a 12 x 12 square come within 0.05 of each other): each agent jitters by +-0.1 around its
    own cell of a randomly permuted 15 x 15 grid of pitch 0.8 and moves at most 0.25 per segment, so any two
    stay 0.1 apart."""
    rng = np.random.default_rng(seed)
    n, m, _ = models_np.MODELS[model]

    def mag(shape):
        return rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)

    if model == "unicycle":
        cell = rng.permutation(225)[:N]
        ctr = -5.6 + 0.8 * np.stack([cell % 15, cell // 15], 1)
        X = np.empty((N, K, 3))
        X[:, :, :2] = ctr[:, None, :] + rng.uniform(-0.1, 0.1, (N, K, 2))
        X[:, :, 2] = rng.uniform(-np.pi, np.pi, (N, K))
        U = np.stack([rng.uniform(0.6, 1.0, (N, K)), rng.uniform(-1.0, 1.0, (N, K))], 2)
        return X, U, rng.uniform(0.8, 1.0, N)
    X = rng.uniform(-6.0, 6.0, (N, K, n))
    if model == "di":
        X[:, :, 3:] = mag((N, K, 3))
    return X, mag((N, K, m)), rng.uniform(1.0, 3.0, N)
