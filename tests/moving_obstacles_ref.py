"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the moving-obstacle scan and node rows
(csrc/moving_obstacles.hip), built on tests/obstacle_rows_ref.py and tests/separation_ref.py.

  * pad_tracks / track_eval: a track's position q_o(t) from its knots, window and the kernel's expressions
    (w = (n - 1) / (t1 - t0) divided once, u = clamp((t - t0) w, 0, n - 1), m = min(floor(u), n - 2));
  * clock: every agent's own sample times t = (sigma_i / ((K-1) S)) (k S + s);
  * relative: the relative samples P - Q_o(t); the moving scan on (P, tracks) IS the static restatement
    (obstacle_rows_ref) on them against a centre at the origin -- minima, scan;
  * both candidate rules and the top-J order: segment_records (v = rho - dist > -cull, 0 < alpha' < 1, dist > 0) and
    node_records (sample 0: v = rho - |d_0| > -cull, |d_0| > 0), descending (v, then ascending o);
  * append_node_rows: one row per node record behind the rows already present;
  * the fixtures of DESIGN §3.9 (A: an intruder crossing the path between two nodes; B: one that is at a node when
    the agent is), the figures their tests assert and a CPU backend's hooks for scvx_hip.scvx.JacobiSCvx.

Layouts are the kernel's: P (N,K-1,S+1,3), knots (O,M,3), n_knots (O,), window (O,2), rho (O,), dist / alpha
(N,K-1,O), rec / node_rec (N,K-1,J,4) = (g, v), obs / node_obs (N,K-1,J), count / node_count (N,K-1)."""
import numpy as np

import obstacle_rows_ref as orf
import separation_ref as sr


def pad_tracks(tracks):
    """[(knots, (t0, t1), rho)] -> knots (O,M,3) zero-padded, n_knots (O,), window (O,2) ((0, 1) for one knot), rho."""
    ks = [np.atleast_2d(np.asarray(k, float)) for k, _, _ in tracks]
    M = max(k.shape[0] for k in ks)
    knots, win = np.zeros((len(ks), M, 3)), np.tile([0.0, 1.0], (len(ks), 1))
    for o, (k, (_, w, _)) in enumerate(zip(ks, tracks)):
        knots[o, :k.shape[0], :k.shape[1]] = k
        if k.shape[0] > 1:
            win[o] = w
    return knots, np.array([k.shape[0] for k in ks]), win, np.array([float(r) for _, _, r in tracks])


def random_tracks(n, pd=3, seed=11, box=6.0, horizon=(1.0, 3.0)):
    """n tracks with 1, 2 and 5 knots in turn, knots uniform in +-box (pd coordinates; track 0, the one a list of one
    consists of, in the fleet's own +-6), rho uniform in 0.5..1.5, for
    agents whose sigma lies in `horizon` (separation_ref.random_fleet's).  Of the windows, track 1 starts after t = 0
    (and lasts beyond every horizon), track 2 stops before the shortest sigma, track 4 covers every agent's horizon;
    the rest are drawn inside (0, horizon[1]).  The first O of them are the same tracks for every O."""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.5, 1.5, n)
    fixed = {1: (0.25 * horizon[0], 1.5 * horizon[1]), 2: (0.0, 0.5 * horizon[0]), 4: (-0.5, 1.25 * horizon[1])}
    out = []
    for o in range(n):
        kn = rng.uniform(-1.0, 1.0, ((1, 2, 5)[o % 3], 3))[:, :pd] * (box if o else 6.0)
        t0, t1 = np.sort(rng.uniform(0.0, horizon[1], 2))
        out.append((kn, fixed.get(o, (float(t0), float(t1) + 0.1)), float(rho[o])))
    return out


def edge_params(D):
    """The unclamped chord parameter -d0.e / e.e of every (track, agent, segment)'s first and last chord (nan where
    the chord has no length): a minimum there is `inner` or not by the sign of the first and of 1 - the last."""
    def par(d0, d1):
        e = d1 - d0
        ee = (e * e).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(ee > 0.0, -(d0 * e).sum(-1) / ee, np.nan)
    return par(D[..., 0, :], D[..., 1, :]), par(D[..., -2, :], D[..., -1, :])


def track_eval(kn, n, win, t):
    """q(t) (..., 3) of one track: kn (M,3), n knots, win (t0, t1), t any shape."""
    t = np.asarray(t, float)
    if n == 1:
        return np.broadcast_to(kn[0], t.shape + (3,)).copy()
    w = (n - 1) / (win[1] - win[0])
    u = np.clip((t - win[0]) * w, 0.0, float(n - 1))
    m = np.clip(np.floor(u).astype(int), 0, n - 2)
    return kn[m] + (u - m)[..., None] * (kn[m + 1] - kn[m])


def clock(sigma, K, S):
    """t (N, K-1, S+1): sample s of segment k of agent i, in real time."""
    dt = np.asarray(sigma, float) / ((K - 1) * S)
    idx = (np.arange(K - 1)[:, None] * S + np.arange(S + 1)[None, :]).astype(float)
    return dt[:, None, None] * idx[None]


def relative(P, sigma, trk):
    """D (O, N, K-1, S+1, 3) = P - Q_o(t), trk = pad_tracks' tuple."""
    knots, n, win, _ = trk
    t = clock(sigma, P.shape[1] + 1, P.shape[2] - 1)
    return np.stack([P - track_eval(knots[o], n[o], win[o], t) for o in range(len(n))])


def minima(P, sigma, trk):
    """Q, s, a (O, N, K-1) and c (O, N, K-1, 3): obstacle_rows_ref.obstacle_minima of every track's relative samples
    against a centre at the origin."""
    parts = [orf.obstacle_minima(D, np.zeros((1, 3))) for D in relative(P, sigma, trk)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def scan(P, sigma, trk):
    """dist, alpha (N, K-1, O) of the analysis outputs."""
    Q, Sx, A, _ = minima(P, sigma, trk)
    return np.moveaxis(np.sqrt(Q), 0, -1), np.moveaxis((Sx + A) / (P.shape[2] - 1), 0, -1)


def _top(V, cand, J):
    """Per (agent, segment): the candidates o of largest V[o], descending (V, then ascending o), at most J."""
    _, N, Km1 = V.shape
    out = [[None] * Km1 for _ in range(N)]
    for a in range(N):
        for k in range(Km1):
            os_ = np.nonzero(cand[:, a, k])[0]
            out[a][k] = os_[np.lexsort((os_, -V[os_, a, k]))][:J]
    return out


def segment_records(P, sigma, trk, cull, J):
    """rec, obs, rec_alpha, count, and sel (N,K-1,J) the selected sub-interval (-1 past count)."""
    rho = trk[3]
    N, Km1, S = P.shape[0], P.shape[1], P.shape[2] - 1
    Q, Sx, A, C = minima(P, sigma, trk)
    V = orf.values(Q, rho)
    top = _top(V, orf.candidates(Q, Sx, A, S, rho, cull), J)
    rec, obs, alpha = np.zeros((N, Km1, J, 4)), np.full((N, Km1, J), -1, np.int32), np.zeros((N, Km1, J))
    sel, count = np.full((N, Km1, J), -1), np.zeros((N, Km1), np.int32)
    for a in range(N):
        for k in range(Km1):
            count[a, k] = top[a][k].size
            for r, o in enumerate(top[a][k]):
                dist = np.sqrt(Q[o, a, k])
                rec[a, k, r, :3], rec[a, k, r, 3] = C[o, a, k] / dist, rho[o] - dist
                obs[a, k, r], alpha[a, k, r], sel[a, k, r] = o, (Sx[o, a, k] + A[o, a, k]) / S, Sx[o, a, k]
    return rec, obs, alpha, count, sel


def node_values(P, sigma, trk):
    """d_0 (O, N, K-1, 3) the relative position at every segment's first node, and v = rho - |d_0| (O, N, K-1)."""
    d0 = relative(P, sigma, trk)[:, :, :, 0]
    return d0, trk[3][:, None, None] - np.sqrt((d0 * d0).sum(-1))


def node_candidates(d0, V, cull):
    return ((d0 * d0).sum(-1) > 0.0) & (V > -cull)


def node_records(P, sigma, trk, cull, J):
    """node_rec, node_obs, node_count."""
    N, Km1 = P.shape[:2]
    d0, V = node_values(P, sigma, trk)
    top = _top(V, node_candidates(d0, V, cull), J)
    rec, obs, count = np.zeros((N, Km1, J, 4)), np.full((N, Km1, J), -1, np.int32), np.zeros((N, Km1), np.int32)
    for a in range(N):
        for k in range(Km1):
            count[a, k] = top[a][k].size
            for r, o in enumerate(top[a][k]):
                dist = np.sqrt((d0[o, a, k] ** 2).sum())
                rec[a, k, r, :3], rec[a, k, r, 3], obs[a, k, r] = d0[o, a, k] / dist, trk[3][o] - dist, o
    return rec, obs, count


def append_node_rows(X_all, i0, idx, node_rec, node_count, rows, count, pos_dim):
    """scvx_node_rows_append_batched on copies: (rows, count, overflow).  idx None: agents i0 + a."""
    rows, count = rows.copy(), count.copy()
    K, j_max = X_all.shape[1], rows.shape[2]
    n = node_rec.shape[0] if idx is None else len(idx)
    overflow = 0
    for a in range(n):
        gi = i0 + a if idx is None else int(idx[a])
        ra = gi - i0
        for t in range(K - 1):
            m = int(count[a, t])
            for r in range(int(node_count[ra, t])):
                if m >= j_max:
                    overflow += 1
                    continue
                g, v = node_rec[ra, t, r, :3], node_rec[ra, t, r, 3]
                b = v
                for d in range(pos_dim):             # left to right, as the kernel
                    b = b + g[d] * X_all[gi, t, d]
                rows[a, t, m, :pos_dim], rows[a, t, m, pos_dim] = g[:pos_dim], b
                m += 1
            count[a, t] = m
    return rows, count, overflow


def di_truth(X, U, sigma, trk, M=2000):
    """(N, K-1, O): min over M+1 points of each segment's exact cubic of ||p(t) - q_o(t)|| - rho_o, every agent on
    its own clock."""
    P, _ = sr.dense_closed_form("di", X, U, sigma, M)
    D = relative(P, sigma, trk)
    return np.moveaxis(np.sqrt((D * D).sum(-1)).min(-1), 0, -1) - trk[3][None, None, :]


def node_clearance(X, sigma, trk):
    """(N, K, O): ||p_t - q_o(sigma_i t / (K-1))|| - rho_o at every node."""
    K = X.shape[1]
    t = np.asarray(sigma, float)[:, None] * np.arange(K)[None, :] / (K - 1)
    knots, n, win, rho = trk
    return np.stack([np.sqrt(((X[:, :, :3] - track_eval(knots[o], n[o], win[o], t)) ** 2).sum(-1)) - rho[o]
                     for o in range(len(n))], -1)


# ------------------------------------------------------------------ the fixtures
FIXTURE = dict(orf.FIXTURE, obs=())
RHO = 0.7
# A: the intruder of radius 0.7 starts at (0, -3.5, 0) and moves at (0, 1, 0): it crosses the agent's line at the
# origin at t = 3.5, half way between nodes 3 and 4 (sigma = 7, K = 8).  Two knots, the window is the horizon.
TRACKS_A = [(np.array([[0.0, -3.5, 0.0], [0.0, 3.5, 0.0]]), (0.0, 7.0), RHO)]
NODE_B = 4


def tracks_b(X_off):
    """B: a constant-velocity track across the converged option-off path X_off (1,K,6), perpendicular to it (the path
    runs along x: the track along y at speed 1), through node NODE_B's position at node NODE_B's time."""
    f = FIXTURE
    p, t = X_off[0, NODE_B, :3], f["sigma"] * NODE_B / (f["K"] - 1)
    return [(np.stack([p + np.array([0.0, -t, 0.0]), p + np.array([0.0, f["sigma"] - t, 0.0])]), (0.0, f["sigma"]), RHO)]


def run_fixture(T, backend, on, tracks, far=False, iters=None, marks=None):
    """FIXTURE["iters"] steps of JacobiSCvx (no coupling, QPSpec.obs empty) on obstacle_rows_ref.fixture with the moving
    obstacles on or off at the same QPSpec.j_max; rules as obstacle_rows_ref.run_fixture.  Returns numpy X, U, sigma, the
    last step's solver outputs and the driver."""
    import scvx_hip
    from scvx_hip.scvx import JacobiSCvx, MovingObstaclesSpec
    f = FIXTURE
    X0, U0, sig = orf.fixture(far)
    spec = scvx_hip.QPSpec(model="di", K=f["K"], box=f["box"], obs=f["obs"], j_max=f["j_max"], w_coll=f["w_coll"],
                           tol=f["tol"], max_iter=80)
    opt = MovingObstaclesSpec(tracks, S=f["S"], J=f["J"], cull=f["cull"]) if on else None
    rule = dict(tr_rule="per_agent", tie_rtol=0.0) if far else dict(tr_rule="global")
    drv = JacobiSCvx(spec, T(X0[:, 0]), T(X0[:, -1]), T(sig), f["tr0"], backend=backend, moving_obstacles=opt, **rule)
    X, U = T(X0), T(U0)
    rows = T(np.zeros((X0.shape[0], f["K"], f["j_max"], 4)))
    for _ in range(f["iters"] if iters is None else iters):
        if on:
            Xn, Un, out = drv.step(X, U, marks=marks)
        else:
            Xn, Un, out = orf._step_with_empty_rows(drv, X, U, rows, marks)
        X, U = Xn.clone(), Un.clone()
    return X.cpu().numpy(), U.cpu().numpy(), sig, {k: v.cpu().numpy() for k, v in out.items()}, drv


def fixture_figures(X, U, sig, out, tracks):
    """(continuous clearance on 2000 points per segment of the exact cubic minus the exact line, node clearances (K,),
    chord bound, worst status, largest slack) of agent 0 against the fixture's track."""
    trk = pad_tracks(tracks)
    cont = di_truth(X[:1], U[:1], sig[:1], trk, M=2000).min()
    node = node_clearance(X[:1], sig[:1], trk)[0].min(-1)
    # a constant-velocity track over the whole horizon has no velocity jump: r'' = p'', inside di_chord_bound's
    # ||r''|| <= 2 max(sigma^2 ||u||)
    bound = sr.di_chord_bound(U[:1], sig[:1], FIXTURE["K"], FIXTURE["S"])
    return cont, node, bound, int(out["status"].max()), float(np.abs(out["slack_coll"]).max())


def mov_overflow(drv):
    """The step's rows that did not fit: last_check["mov_overflow"] where the step has a check stage, else the counter
    it is read from."""
    if drv.last_check is not None:
        return drv.last_check["mov_overflow"]
    return int(drv._mv["overflow"].item())


COUPLED = dict(obs=[((-0.9, 0.9, 0.0), 0.5)],
               # an obstacle drifting along agent 0's path, 0.6 to its side
               tracks=[(np.array([[-3.0, 0.9, 0.0], [-2.0, 0.9, 0.0]]), (0.0, 7.0), 0.5)])


def coupled_step(T, backend, marks=None):
    """Two steps on intersample_rows_ref.head_on with a CouplingSpec (check=True), pair records, static obstacle records
    and moving obstacles, J = 1 each at j_max = 8 (one node-level row left).  Returns the driver, the last step's
    iterate (numpy) and its solver outputs.  (The warm start is at rest at every node: its roll-out does not move, the
    first step has no pair or static record.)"""
    import intersample_rows_ref as ir
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx, MovingObstaclesSpec, ObstacleRowsSpec
    X0, U0, sig = ir.head_on()
    spec = scvx_hip.QPSpec(model="di", K=8, box=[(0, -20.0, 20.0)], obs=COUPLED["obs"], j_max=8, w_coll=1e4, tol=1e-10,
                           max_iter=80)
    drv = JacobiSCvx(spec, T(X0[:, 0]), T(X0[:, -1]), T(sig), 4.0, tr_rule="global", backend=backend,
                     coupling=CouplingSpec(R=1.0, check=True, intersample_S=8, intersample_J=1),
                     obstacle_rows=ObstacleRowsSpec(S=8, J=1, cull=1.0),
                     moving_obstacles=MovingObstaclesSpec(COUPLED["tracks"], S=8, J=1, cull=1.0))
    X, U = T(X0), T(U0)
    for _ in range(2):
        Xp = X
        X, U, out = drv.step(X, U, marks=marks)
        X, U = X.clone(), U.clone()
    return drv, Xp.cpu().numpy(), out


def check_coupled_rows(drv, Xp):
    """drv.count and drv.rows after coupled_step against the restatement: per node the one neighbour's node row, then
    the pair records, the static obstacle records, the moving node rows and the moving segment records, each appended
    by its restatement from the step's own records (g bit for bit, b within 1e-13)."""
    import intersample_rows_ref as ir
    n = lambda t: t.cpu().numpy()  # noqa: E731
    rows_d, count_d = n(drv.rows), n(drv.count)
    cs = [n(s["count_seg"]) for s in (drv._is, drv._ob, drv._mv)]
    nc = n(drv._mv["node_count"])
    assert all(c.sum() > 0 for c in cs) and nc.sum() > 0
    rows = np.zeros_like(rows_d)
    rows[:, :-1, 0] = rows_d[:, :-1, 0]                       # the node-level row of the one neighbour
    count = np.zeros_like(count_d)
    count[:, :-1] = 1
    for s in (drv._is, drv._ob):
        rows, count, over = ir.append_rows(Xp, 0, None, n(s["rec"]), n(s["count_seg"]), rows, count, 3)
        assert over == 0
    rows, count, over = append_node_rows(Xp, 0, None, n(drv._mv["node_rec"]), nc, rows, count, 3)
    assert over == 0
    rows, count, over = ir.append_rows(Xp, 0, None, n(drv._mv["rec"]), cs[2], rows, count, 3)
    assert over == 0
    assert np.array_equal(count_d, count)
    live = np.arange(rows.shape[2])[None, None, :] < count[:, :, None]
    assert np.array_equal(rows_d[live][:, :3], rows[live][:, :3]) and np.abs(rows_d[live][:, 3] - rows[live][:, 3]).max() <= 1e-13
    # where a node has all five kinds the moving node row sits behind the static record and ahead of the moving one
    want = np.zeros_like(count)
    want[:, :-1] = 1 + cs[0] + cs[1] + nc + cs[2]
    want[:, 1:-1] += (cs[0] + cs[1] + cs[2])[:, :-1]
    assert np.array_equal(count, want)


def cpu_moving_obstacle_rows(model, X, U, sigma, S, nsub, pos_dim, tracks, cull, J):
    """The HipBackend hook of the same name on numpy arrays ("di": the closed-form samples are its roll-out)."""
    P, _ = sr.dense_closed_form(model, X, U, sigma, S, pos_dim)
    trk = pad_tracks(tracks)
    rec, _, _, count, _ = segment_records(P, sigma, trk, cull, J)
    nrec, _, ncount = node_records(P, sigma, trk, cull, J)
    return rec, count, nrec, ncount
