"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the continuous-time collision rows (csrc/intersample_rows.hip),
built on tests/separation_ref.py (dense_closed_form, chord).

  * pair_minima: every pair's own chord closest approach per segment, the first minimum over the S sub-intervals
    (replaced only when strictly smaller): dist^2, s, a, c;
  * candidates / pair_rows: the kernel's candidate rule and its top-J selection in ascending (dist, j) order;
  * append_rows: the two node rows of every record behind the node rows already present;
  * head_on: the two-agent fixture of DESIGN §3.7 and a CPU backend's two hooks for scvx_hip.scvx.JacobiSCvx.

Layouts are the kernels': P (N,K-1,S+1,3), rec (n,K-1,J,4) = (g, v), nbr / alpha (n,K-1,J), count (n,K-1);
rows (n,K,j_max,pos_dim+1), count (n,K)."""
import numpy as np

import separation_ref as sr


def pair_minima(P, i0=0, n_local=None):
    """Q, s, a (N, n_local, K-1) and c (N, n_local, K-1, 3) of local agent i against every j (first axis)."""
    N, Km1, S1, _ = P.shape
    n_local = N - i0 if n_local is None else n_local
    Pi = P[i0:i0 + n_local]
    Q = np.full((N, n_local, Km1), np.inf)
    Sx = np.zeros((N, n_local, Km1), int)
    A = np.zeros((N, n_local, Km1))
    C = np.zeros((N, n_local, Km1, 3))
    for j in range(N):
        d = Pi - P[j][None]
        for s in range(S1 - 1):
            d0, d1 = d[:, :, s], d[:, :, s + 1]
            al, q = sr.chord(d0, d1)
            take = q < Q[j]
            Q[j], Sx[j], A[j] = np.where(take, q, Q[j]), np.where(take, s, Sx[j]), np.where(take, al, A[j])
            C[j] = np.where(take[..., None], d0 + al[..., None] * (d1 - d0), C[j])
    return Q, Sx, A, C


def candidates(Q, Sx, A, S, cull, i0=0):
    """dist < cull (on the squares), 0 < alpha' < 1, dist > 0, j != i."""
    N, n_local, _ = Q.shape
    other = np.arange(N)[:, None, None] != (i0 + np.arange(n_local))[None, :, None]
    inner = ((Sx > 0) | (A > 0.0)) & ((Sx < S - 1) | (A < 1.0))
    return other & inner & (Q > 0.0) & (Q < cull * cull)


def pair_rows(P, i0, n_local, R, cull, J):
    """rec, nbr, alpha, count of scvx_intersample_pair_rows_batched."""
    N, Km1, S1, _ = P.shape
    S = S1 - 1
    Q, Sx, A, C = pair_minima(P, i0, n_local)
    cand = candidates(Q, Sx, A, S, cull, i0)
    rec = np.zeros((n_local, Km1, J, 4))
    nbr = np.full((n_local, Km1, J), -1, np.int32)
    alpha = np.zeros((n_local, Km1, J))
    count = np.zeros((n_local, Km1), np.int32)
    for a in range(n_local):
        for k in range(Km1):
            js = np.nonzero(cand[:, a, k])[0]
            js = js[np.lexsort((js, Q[js, a, k]))][:J]     # ascending (dist, j)
            count[a, k] = js.size
            for r, j in enumerate(js):
                dist = np.sqrt(Q[j, a, k])
                rec[a, k, r, :3] = C[j, a, k] / dist
                rec[a, k, r, 3] = 2.0 * R - dist
                nbr[a, k, r] = j
                alpha[a, k, r] = (Sx[j, a, k] + A[j, a, k]) / S
    return rec, nbr, alpha, count


def append_rows(X_all, i0, idx, rec, count_seg, rows, count, pos_dim):
    """scvx_collision_rows_append_batched on copies: (rows, count, overflow).  idx None: agents i0 + a."""
    rows, count = rows.copy(), count.copy()
    K = X_all.shape[1]
    j_max = rows.shape[2]
    n = rec.shape[0] if idx is None else len(idx)
    overflow = 0
    for a in range(n):
        gi = i0 + a if idx is None else int(idx[a])
        ra = gi - i0
        for t in range(K - 1):
            m = int(count[a, t])
            for k in ([t, t - 1] if t else [t]):
                for r in range(int(count_seg[ra, k])):
                    if m >= j_max:
                        overflow += 1
                        continue
                    g, v = rec[ra, k, r, :3], rec[ra, k, r, 3]
                    b = v
                    for d in range(pos_dim):             # left to right, as the kernel
                        b = b + g[d] * X_all[gi, t, d]
                    rows[a, t, m, :pos_dim], rows[a, t, m, pos_dim] = g[:pos_dim], b
                    m += 1
            count[a, t] = m
    return rows, count, overflow


# ------------------------------------------------------------------ the head-on fixture
HEAD_ON = dict(K=8, sigma=7.0, R=1.0, S=8, J=1, iters=25, tr0=4.0, j_max=8, box=[(0, -20.0, 20.0)], w_coll=1e4,
               tol=1e-10)


def head_on(copies=1, apart=100.0):
    """Two double integrators crossing almost head-on between two nodes: starts (-+6, +-0.3, 0), goals
    (+-6, +-0.3, +-0.2), at rest, straight-line warm start with U = 0 (workloads.synthetic_di's).  copies > 1
    repeats the pair `apart` further along z.  Returns X (N,K,6), U (N,K,3), sigma (N,)."""
    K = HEAD_ON["K"]
    p0 = np.array([[-6.0, 0.3, 0.0], [6.0, -0.3, 0.0]])
    pf = np.array([[6.0, 0.3, 0.2], [-6.0, -0.3, -0.2]])
    a = np.linspace(0, 1, K)
    X = np.zeros((2 * copies, K, 6))
    for c in range(copies):
        X[2 * c:2 * c + 2, :, 0:3] = p0[:, None, :] * (1 - a)[None, :, None] + pf[:, None, :] * a[None, :, None]
        X[2 * c:2 * c + 2, :, 2] += apart * c
    return X, np.zeros((2 * copies, K, 3)), np.full(2 * copies, HEAD_ON["sigma"])


def run_head_on(T, backend, on, copies=1):
    """HEAD_ON["iters"] steps of JacobiSCvx (global rule, strict halving test, no check stage) on the fixture, with
    the continuous-time rows on or off at the same QPSpec.j_max.  T: numpy -> tensor on the backend's device.
    Returns numpy X, U, sigma, the last step's solver outputs and the driver."""
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx
    h = HEAD_ON
    X0, U0, sig = head_on(copies)
    spec = scvx_hip.QPSpec(model="di", K=h["K"], box=h["box"], j_max=h["j_max"], w_coll=h["w_coll"], tol=h["tol"],
                           max_iter=80)
    cpl = CouplingSpec(R=h["R"], check=False, intersample_S=h["S"] if on else 0, intersample_J=h["J"])
    drv = JacobiSCvx(spec, T(X0[:, 0]), T(X0[:, -1]), T(sig), h["tr0"], coupling=cpl, tr_rule="global", backend=backend)
    X, U = T(X0), T(U0)
    for _ in range(h["iters"]):
        Xn, Un, out = drv.step(X, U)
        X, U = Xn.clone(), Un.clone()
    return X.cpu().numpy(), U.cpu().numpy(), sig, {k: v.cpu().numpy() for k, v in out.items()}, drv


def head_on_figures(X, U, sig, out):
    """(continuous minimum on 2000 points per segment, node minimum, chord bound, worst status, largest slack)."""
    D = sr.pair_min_distance(X)
    node = D[~np.eye(D.shape[0], dtype=bool)].min()
    return (sr.di_truth(X, U, sig, M=2000).min(), node, sr.di_chord_bound(U, sig, HEAD_ON["K"], HEAD_ON["S"]),
            int(out["status"].max()), float(np.abs(out["slack_coll"]).max()))


def cpu_intersample_pair_rows(model, X, U, sigma, S, nsub, pos_dim, R, cull, J):
    """The HipBackend hook of the same name on numpy arrays ("di": the closed-form samples are its roll-out)."""
    P, _ = sr.dense_closed_form(model, X, U, sigma, S, pos_dim)
    rec, _, _, count = pair_rows(P, 0, X.shape[0], R, cull, J)
    return rec, count
