"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the continuous-time obstacle scan and rows
(csrc/obstacle_rows.hip), built on tests/separation_ref.py (dense_closed_form, chord).

  * obstacle_minima: every obstacle's own chord closest approach per (agent, segment), the first minimum over the
    S sub-intervals (replaced only when strictly smaller): dist^2, s, a, c;
  * candidates / obstacle_rows: the kernel's candidate rule (v = rho - dist > -cull, 0 < alpha' < 1, dist > 0) and
    its top-J selection in descending (v, then ascending o) order;
  * the fixture of DESIGN §3.8 (one agent whose straight line passes an obstacle between two nodes), the figures its
    tests assert and a CPU backend's hook for scvx_hip.scvx.JacobiSCvx.

Layouts are the kernel's: P (N,K-1,S+1,3), centers (O,3), rho (O,), dist / alpha (N,K-1,O), rec (N,K-1,J,4) =
(g, v), obs / rec_alpha (N,K-1,J), count (N,K-1).  The appended node rows are intersample_rows_ref.append_rows'."""
import numpy as np

import separation_ref as sr


def pad_centers(obstacles):
    """[(centre, rho)] -> centers (O,3) zero-padded, rho (O,)."""
    c = np.zeros((len(obstacles), 3))
    for o, (ctr, _) in enumerate(obstacles):
        ctr = np.asarray(ctr, float).reshape(-1)
        c[o, :ctr.size] = ctr
    return c, np.array([float(r) for _, r in obstacles])


def obstacle_minima(P, centers):
    """Q, s, a (O, N, K-1) and c (O, N, K-1, 3): obstacle o (first axis) against every (agent, segment)."""
    N, Km1, S1, _ = P.shape
    O = len(centers)
    Q = np.full((O, N, Km1), np.inf)
    Sx = np.zeros((O, N, Km1), int)
    A = np.zeros((O, N, Km1))
    C = np.zeros((O, N, Km1, 3))
    for o in range(O):
        d = P - np.asarray(centers[o], float)[None, None, None, :]
        for s in range(S1 - 1):
            d0, d1 = d[:, :, s], d[:, :, s + 1]
            al, q = sr.chord(d0, d1)
            take = q < Q[o]
            Q[o], Sx[o], A[o] = np.where(take, q, Q[o]), np.where(take, s, Sx[o]), np.where(take, al, A[o])
            C[o] = np.where(take[..., None], d0 + al[..., None] * (d1 - d0), C[o])
    return Q, Sx, A, C


def scan(P, centers):
    """dist, alpha (N, K-1, O) of scvx_obstacle_scan_batched's analysis outputs."""
    Q, Sx, A, _ = obstacle_minima(P, centers)
    S = P.shape[2] - 1
    return np.moveaxis(np.sqrt(Q), 0, -1), np.moveaxis((Sx + A) / S, 0, -1)


def values(Q, rho):
    """v = rho_o - dist (O, N, K-1)."""
    return np.asarray(rho, float)[:, None, None] - np.sqrt(Q)


def candidates(Q, Sx, A, S, rho, cull):
    """v > -cull, 0 < alpha' < 1, dist > 0."""
    inner = ((Sx > 0) | (A > 0.0)) & ((Sx < S - 1) | (A < 1.0))
    return inner & (Q > 0.0) & (values(Q, rho) > -cull)


def obstacle_rows(P, centers, rho, cull, J):
    """rec, obs, rec_alpha, count of scvx_obstacle_scan_batched, and sel (N,K-1,J) the selected sub-interval s
    (-1 past count)."""
    N, Km1, S1, _ = P.shape
    S = S1 - 1
    Q, Sx, A, C = obstacle_minima(P, centers)
    V = values(Q, rho)
    cand = candidates(Q, Sx, A, S, rho, cull)
    rec = np.zeros((N, Km1, J, 4))
    obs = np.full((N, Km1, J), -1, np.int32)
    alpha = np.zeros((N, Km1, J))
    sel = np.full((N, Km1, J), -1)
    count = np.zeros((N, Km1), np.int32)
    for a in range(N):
        for k in range(Km1):
            os_ = np.nonzero(cand[:, a, k])[0]
            os_ = os_[np.lexsort((os_, -V[os_, a, k]))][:J]     # descending v, then ascending o
            count[a, k] = os_.size
            for r, o in enumerate(os_):
                dist = np.sqrt(Q[o, a, k])
                rec[a, k, r, :3] = C[o, a, k] / dist
                rec[a, k, r, 3] = rho[o] - dist
                obs[a, k, r] = o
                alpha[a, k, r] = (Sx[o, a, k] + A[o, a, k]) / S
                sel[a, k, r] = Sx[o, a, k]
    return rec, obs, alpha, count, sel


def di_clearance_truth(X, U, sigma, centers, rho, M=2000):
    """(N, K-1, O): min over M+1 points of each segment's exact cubic of ||p - c_o|| - rho_o."""
    P, _ = sr.dense_closed_form("di", X, U, sigma, M)
    d = np.stack([np.sqrt(((P - np.asarray(c, float)) ** 2).sum(-1)).min(2) for c in centers], -1)
    return d - np.asarray(rho, float)[None, None, :]


# ------------------------------------------------------------------ the fixture
FIXTURE = dict(K=8, sigma=7.0, S=8, J=1, cull=1.0, iters=10, tr0=4.0, j_max=4, obs=[((0.0, 0.0, 0.0), 0.7)],
               box=[(0, -20.0, 20.0)], w_coll=1e4, tol=1e-10)


def fixture(far=False, apart=100.0):
    """One double integrator at rest at (-6, 0.05, 0) -> (6, 0.05, 0), straight-line warm start with U = 0: with
    K = 8 the origin lies between nodes 3 and 4, and the obstacle of total radius 0.7 there is passed between them.
    far: a second agent, the same `apart` further along z (no obstacle within reach).  X (N,K,6), U (N,K,3),
    sigma (N,)."""
    K, N = FIXTURE["K"], 2 if far else 1
    a = np.linspace(0, 1, K)
    X = np.zeros((N, K, 6))
    X[:, :, 0] = -6.0 + 12.0 * a
    X[:, :, 1] = 0.05
    if far:
        X[1, :, 2] = apart
    return X, np.zeros((N, K, 3)), np.full(N, FIXTURE["sigma"])


def run_fixture(T, backend, on, far=False, obstacles=None, iters=None, marks=None):
    """FIXTURE["iters"] steps of JacobiSCvx (no coupling) on the fixture with the obstacle rows on or off at the same
    QPSpec.j_max.  One agent: the global rule.  far (two agents): the per-agent rule with the strict test
    (tie_rtol = 0), which is the global rule of each agent on its own -- under the shared rule the fixture agent's
    cost would move the far agent's trust radius.  obstacles: the option's own list (None: QPSpec.obs).  T: numpy ->
    tensor on the backend's device.  Returns numpy X, U, sigma, the last step's solver outputs and the driver."""
    import scvx_hip
    from scvx_hip.scvx import JacobiSCvx, ObstacleRowsSpec
    f = FIXTURE
    X0, U0, sig = fixture(far)
    spec = scvx_hip.QPSpec(model="di", K=f["K"], box=f["box"], obs=f["obs"], j_max=f["j_max"], w_coll=f["w_coll"],
                           tol=f["tol"], max_iter=80)
    opt = ObstacleRowsSpec(S=f["S"], J=f["J"], cull=f["cull"], obstacles=obstacles) if on else None
    rule = dict(tr_rule="per_agent", tie_rtol=0.0) if far else dict(tr_rule="global")
    drv = JacobiSCvx(spec, T(X0[:, 0]), T(X0[:, -1]), T(sig), f["tr0"], backend=backend, obstacle_rows=opt, **rule)
    X, U = T(X0), T(U0)
    rows = T(np.zeros((X0.shape[0], f["K"], f["j_max"], 4)))
    for _ in range(f["iters"] if iters is None else iters):
        if on:
            Xn, Un, out = drv.step(X, U, marks=marks)
        else:   # j_max > 0 without any row source: the solver takes empty rows (the option-off run of the same class)
            Xn, Un, out = _step_with_empty_rows(drv, X, U, rows, marks)
        X, U = Xn.clone(), Un.clone()
    return X.cpu().numpy(), U.cpu().numpy(), sig, {k: v.cpu().numpy() for k, v in out.items()}, drv


def _step_with_empty_rows(drv, X, U, rows, marks=None):
    """JacobiSCvx.step with the option off at j_max > 0 and no coupling: the driver hands the solver no rows, the
    template wants some -- the driver's own solver is wrapped for the call so that it gets zero rows per node."""
    import torch
    solver = drv.solver
    count = torch.zeros(rows.shape[:2], dtype=torch.int32, device=rows.device)

    class _Empty:
        supports_order = getattr(solver, "supports_order", False)

        def solve(self, disc, sigma, Xr, Ur, xi, xf, tr, r, c, **kw):
            return solver.solve(disc, sigma, Xr, Ur, xi, xf, tr, rows, count, **kw)

    drv.solver = _Empty()
    try:
        return drv.step(X, U, marks=marks)
    finally:
        drv.solver = solver


def fixture_figures(X, U, sig, out):
    """(continuous clearance on 2000 points per segment of the exact cubic, node clearance, chord bound, worst
    status, largest slack) of agent 0 against the fixture's obstacle."""
    c, rho = pad_centers(FIXTURE["obs"])
    cont = di_clearance_truth(X[:1], U[:1], sig[:1], c, rho, M=2000).min()
    node = sr.obstacle_min_distance(X[:1], c, rho, 0.0).min()
    return (cont, node, sr.di_chord_bound(U[:1], sig[:1], FIXTURE["K"], FIXTURE["S"]), int(out["status"].max()),
            float(np.abs(out["slack_coll"]).max()))


def cpu_obstacle_rows(model, X, U, sigma, S, nsub, pos_dim, obstacles, cull, J):
    """The HipBackend hook of the same name on numpy arrays ("di": the closed-form samples are its roll-out)."""
    P, _ = sr.dense_closed_form(model, X, U, sigma, S, pos_dim)
    c, rho = pad_centers(obstacles)
    rec, _, _, count, _ = obstacle_rows(P, c, rho, cull, J)
    return rec, count
