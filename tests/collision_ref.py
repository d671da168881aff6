"""Plain reference of the collision rows and the full-row check (csrc/collision.hip), in extended precision.

Vectorised numpy in np.longdouble over all neighbours of one (global agent, node); no pruning, no tiles, no
bounds: Distributed_opt/dist_scvx_3d.py:93-107 as written,

    row j:   g = (p_i - p_j) / |p_i - p_j|,   b = 2R - |p_i - p_j| + g . p_i        (b - g . p_t <= S_t)
    check j: v = (2R - |p_i - p_j|) - (p_i - p_j) . dp / |p_i - p_j| - S,           dp = p_new - p_i

with the culling of include/scvx_hip.h: a neighbour is eligible when j != i and, if cull > 0, |p_i - p_j| < cull
strictly.  A coincident neighbour gives NaN (0/0), as the reference's.

assert_rows_valid is the acceptance rule of a kept set: it does not depend on the kernel's row order or on how the
kernel breaks exact distance ties."""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
SENTINEL = -7.25e77      # what the callers pre-fill `rows` with; no row holds it


def _positions(X_all, t, pos_dim):
    return np.asarray(X_all)[:, t, :pos_dim].astype(LD)


def rows_ref(X_all, gi, t, R, pos_dim, cull):
    """The eligible neighbours of global agent gi at node t, ascending in index: idx (E,), their squared
    distances d2 (E,), norms nr (E,) and rows g (E, pos_dim), b (E,), all np.longdouble."""
    P = _positions(X_all, t, pos_dim)
    pi = P[gi]
    diff = pi - P
    d2 = (diff * diff).sum(axis=1)
    nr = np.sqrt(d2)
    elig = np.ones(P.shape[0], bool)
    elig[gi] = False
    if cull > 0:
        elig &= nr < LD(cull)
    idx = np.nonzero(elig)[0]
    diff, d2, nr = diff[idx], d2[idx], nr[idx]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = diff / nr[:, None]
        b = 2 * LD(R) - nr + (g * pi).sum(axis=1)
    return SimpleNamespace(idx=idx, d2=d2, nr=nr, g=g, b=b)


def check_ref(X_all, gi, t, X_new_a, S, R, pos_dim, scale=False):
    """All N_total - 1 row values v of global agent gi at node t (neighbour-index order, np.longdouble) at the
    solved positions X_new_a (K, n_x) of that agent and its slack S.  scale=True: also the magnitude
    max_j (2R + nr_j + |(p_i - p_j) . dp| / nr_j + |S|) the rounding of a double evaluation is proportional to
    (0 for an empty or all-NaN row set)."""
    P = _positions(X_all, t, pos_dim)
    pi = P[gi]
    dp = np.asarray(X_new_a)[t, :pos_dim].astype(LD) - pi
    diff = np.delete(pi - P, gi, axis=0)
    nr = np.sqrt((diff * diff).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        proj = (diff * dp).sum(axis=1) / nr
        v = (2 * LD(R) - nr) - proj - LD(S)
        if not scale:
            return v
        mag = 2 * abs(LD(R)) + nr + np.abs(proj) + abs(LD(S))
    mag = mag[~np.isnan(mag)]
    return v, (float(mag.max()) if mag.size else 0.0)


def kept_gap(ref, j_max):
    """Relative gap between the j_max-th and the (j_max+1)-th nearest eligible squared distance (inf when
    every eligible neighbour is kept): the selection is unambiguous in double when this exceeds rounding."""
    if ref.d2.size <= j_max:
        return np.inf
    d = np.sort(ref.d2)
    return float((d[j_max] - d[j_max - 1]) / d[j_max])


def cull_gap(X_all, gi, t, pos_dim, cull):
    """Smallest relative distance of a neighbour's |p_i - p_j| to cull."""
    P = _positions(X_all, t, pos_dim)
    diff = np.delete(P[gi] - P, gi, axis=0)
    if diff.shape[0] == 0:
        return np.inf
    nr = np.sqrt((diff * diff).sum(axis=1))
    return float(np.abs(nr - LD(cull)).min() / LD(cull))


def _row_matches(got, ref, p_i, R):
    """(count, E) boolean: got row r is reference row e within the derived tolerances."""
    pd = ref.g.shape[1]
    gg, gb = got[:, None, :pd].astype(LD), got[:, None, pd].astype(LD)
    with np.errstate(invalid="ignore"):
        tol_b = 16 * EPS * (2 * abs(LD(R)) + ref.nr + np.abs(ref.g * np.asarray(p_i, LD)[:pd]).sum(axis=1))
        ok = (np.abs(gg - ref.g[None]) <= 8 * EPS).all(axis=2) & (np.abs(gb - ref.b[None]) <= tol_b[None])
    # a coincident neighbour: NaN in every entry of both, and nothing else is NaN
    nan_ref = np.isnan(ref.g).all(axis=1) & np.isnan(ref.b)
    nan_got = np.isnan(got).all(axis=1)
    return ok | (nan_got[:, None] & nan_ref[None, :])


def _distinct_assignment(M):
    """A matching of every row of boolean M (count, E) to a distinct column (Kuhn), or None."""
    cols = [np.nonzero(r)[0] for r in M]
    if all(len(c) == 1 for c in cols):          # the usual case: one candidate each
        flat = [int(c[0]) for c in cols]
        return flat if len(set(flat)) == len(flat) else None
    owner = {}

    def place(r, seen):
        for c in cols[r]:
            c = int(c)
            if c in seen:
                continue
            seen.add(c)
            if c not in owner or place(owner[c], seen):
                owner[c] = r
                return True
        return False

    for r in range(M.shape[0]):
        if not place(r, set()):
            return None
    inv = {r: c for c, r in owner.items()}
    return [inv[r] for r in range(M.shape[0])]


def assert_rows_valid(got_rows, got_count, ref, j_max, p_i, R, where=""):
    """got_rows (j_max, pos_dim + 1) pre-filled with SENTINEL by the caller, got_count: one (agent, node) of the
    kernel's output; ref = rows_ref(...) of it; p_i the agent's position.  Returns the kept neighbour indices."""
    got_rows = np.asarray(got_rows)
    E = ref.idx.size
    n = int(got_count)
    assert n == min(j_max, E), f"{where}: count {n}, eligible {E}, j_max {j_max}"
    got = got_rows[:n]
    M = _row_matches(got, ref, p_i, R)
    assert M.any(axis=1).all(), f"{where}: rows {np.nonzero(~M.any(axis=1))[0]} are no eligible neighbour's row"
    kept = _distinct_assignment(M)
    assert kept is not None, f"{where}: the kept rows are not those of distinct neighbours"
    if n < E:
        mask = np.zeros(E, bool)
        mask[kept] = True
        far, near = ref.d2[mask].max(), ref.d2[~mask].min()
        assert far <= near, f"{where}: kept |d|^2 {float(far)!r} but dropped {float(near)!r}"
    tail = got_rows[n:]
    assert (tail == SENTINEL).all(), f"{where}: slots behind count were written"
    return ref.idx[np.asarray(kept, dtype=np.int64)]
