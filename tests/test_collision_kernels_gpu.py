"""GPU: collision_rows_kernel and collision_check_kernel (csrc/collision.hip) against the plain extended-precision
reference (tests/collision_ref.py) at the edges of their pruning: several LDS tiles and a padded last chunk, blocks
that straddle a tile boundary, the wave-local bound tau, the [blo, bhi) block-mate exclusion at i0 > 0, every JM
template class, fewer eligible neighbours than j_max, culling (strict), exact distance ties, pos_dim 1 and 2 with
junk in the other state components, K = 2 and 64, a coincident pair, the indexed form, relabelled agents, slack and
step extremes of the check, fleets of 1 and 2, and the argument checks of the three entry points.

The fixtures (tests/collision_cases.py) are proven tie-free / margin-safe on the reference alone by
tests/test_collision_ref_cpu.py, so the kept set and the violation count are compared exactly; row values within
    |dg_d| <= 8 eps,   |db| <= 16 eps (2R + |d| + sum_d |g_d p_i,d|),   eps = 2^-52
(a row is a handful of IEEE double operations with one sqrt and one divide per component) and the largest check
value within 16 eps max_j (2R + |d_j| + |(p_i - p_j) . dp| / |d_j| + |S|)."""
import numpy as np
import pytest

import collision_cases as cc
import collision_ref as cr
import scvx_hip

pytestmark = pytest.mark.gpu

EMPTY_VMAX = -1e300     # vmax of an agent without neighbours (include/scvx_hip.h, scvx_collision_check_batched)


def _t(x, cuda, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=cuda, dtype=dtype or torch.float64)


def _launch_rows(cuda, X, R, j_max, pos_dim, cull, i0=0, n_local=None, idx=None):
    """rows pre-filled with the sentinel, count with -7 (the kernel writes every count entry)."""
    import torch
    n = len(idx) if idx is not None else n_local
    K = X.shape[1]
    rows = torch.full((n, K, j_max, pos_dim + 1), cr.SENTINEL, dtype=torch.float64, device=cuda)
    count = torch.full((n, K), -7, dtype=torch.int32, device=cuda)
    if idx is not None:
        scvx_hip.collision_rows_indexed(_t(X, cuda), _t(idx, cuda, torch.int32), R, j_max, pos_dim, cull, rows, count)
    else:
        scvx_hip.collision_rows(_t(X, cuda), i0, n, R, j_max, pos_dim, cull, rows, count)
    return rows.cpu().numpy(), count.cpu().numpy()


def _launch_case(cuda, c):
    return _launch_rows(cuda, c["X"], c["R"], c["j_max"], c["pos_dim"], c["cull"], c["i0"], c["n_local"], c["idx"])


def _validate(c, rows, cnt):
    """Every (local agent, node) of a case against the reference; returns the kept neighbour indices."""
    X, K, pd = c["X"], c["X"].shape[1], c["pos_dim"]
    kept = {}
    for a, gi in enumerate(cc.agents_of(c)):
        for t in range(K - 1):
            kept[a, t] = cr.assert_rows_valid(rows[a, t], cnt[a, t], cc.row_ref(c, gi, t), c["j_max"], X[gi, t, :pd],
                                              c["R"], where=f"{c['name']} agent {gi} node {t}")
    assert (cnt[:, K - 1] == 0).all()
    assert (rows[:, K - 1] == cr.SENTINEL).all()
    return kept


def _as_sets(rows, cnt):
    """Per (agent, node) the kept rows in a canonical order (bitwise comparison of sets; no NaN rows)."""
    out = {}
    for a in range(rows.shape[0]):
        for t in range(rows.shape[1]):
            r = rows[a, t, :cnt[a, t]]
            out[a, t] = r[np.lexsort(r.T)]
    return out


@pytest.mark.parametrize("name", list(cc.ROW_CASES))
def test_rows_match_reference(cuda, name):
    c = cc.ROW_CASES[name]
    rows, cnt = _launch_case(cuda, c)
    kept = _validate(c, rows, cnt)
    X = c["X"]
    if name.startswith("lattice"):
        # node 0 numbers the sites in raster order: 62 is the centre (6 neighbours at 1, 12 at sqrt 2, 8 at sqrt 3,
        # 6 at exactly 2), 0 a corner (3, 3, 1, 3)
        d2 = lambda a: sorted(((X[a, 0, :3] - X[kept[a, 0], 0, :3]) ** 2).sum(axis=1).tolist())  # noqa: E731
        want = {"lattice_j8": ([1.0] * 6 + [2.0] * 2, [1.0] * 3 + [2.0] * 3 + [3.0] + [4.0]),
                "lattice_j4": ([1.0] * 4, [1.0] * 3 + [2.0]),
                "lattice_cull2_j8": ([1.0] * 6 + [2.0] * 2, [1.0] * 3 + [2.0] * 3 + [3.0]),
                "lattice_cull2_j32": ([1.0] * 6 + [2.0] * 12 + [3.0] * 8, [1.0] * 3 + [2.0] * 3 + [3.0])}[name]
        assert d2(62) == want[0] and d2(0) == want[1]
    if name == "cull_none":
        assert (cnt == 0).all() and (rows == cr.SENTINEL).all()
    if name == "coincident":
        a40, a41 = 40 - c["i0"], 41 - c["i0"]
        for a, other in ((a40, 41), (a41, 40)):
            assert cnt[a, 1] == c["j_max"] and other in kept[a, 1]
            nan = np.isnan(rows[a, 1])
            assert nan.all(axis=1).sum() == 1 and nan.any(axis=1).sum() == 1      # that row: NaN in g (and b)
        nan_rows = np.isnan(rows).any(axis=3)
        nan_rows[[a40, a41], 1] = False
        assert not nan_rows.any()


@pytest.mark.parametrize("name", ["indexed", "indexed_cull"])
def test_indexed_rows_equal_the_contiguous_launch(cuda, name):
    c = cc.ROW_CASES[name]
    rows, cnt = _launch_case(cuda, c)
    full, cfull = _launch_rows(cuda, c["X"], c["R"], c["j_max"], c["pos_dim"], c["cull"], 0, cc.N_TILES)
    got, want = _as_sets(rows, cnt), _as_sets(full, cfull)
    for a, gi in enumerate(c["idx"]):
        np.testing.assert_array_equal(cnt[a], cfull[gi])
        for t in range(c["X"].shape[1]):
            np.testing.assert_array_equal(got[a, t], want[int(gi), t])


def test_rows_do_not_depend_on_the_agent_numbering(cuda):
    """Relabelling the agents changes every wave's block-mates (tau) and every tile's content, not the kept sets."""
    X = cc.multi_tile()
    perm = np.random.default_rng(105).permutation(cc.N_TILES)
    rows, cnt = _launch_rows(cuda, X, cc.R, 8, 3, 0.0, 0, cc.N_TILES)
    rows_p, cnt_p = _launch_rows(cuda, X[perm], cc.R, 8, 3, 0.0, 0, cc.N_TILES)
    want, got = _as_sets(rows, cnt), _as_sets(rows_p, cnt_p)
    np.testing.assert_array_equal(cnt_p, cnt[perm])
    for a in range(cc.N_TILES):
        for t in range(X.shape[1]):
            np.testing.assert_array_equal(got[a, t], want[int(perm[a]), t])


def _launch_check(cuda, c, X=None, X_new=None, S=None):
    import torch
    X = c["X"] if X is None else X
    X_new, S = (c["X_new"] if X_new is None else X_new), (c["S"] if S is None else S)
    viol = torch.full(S.shape, -7, dtype=torch.int32, device=cuda)
    vmax = torch.full(S.shape, cr.SENTINEL, dtype=torch.float64, device=cuda)
    scvx_hip.collision_check(_t(X, cuda), c["i0"], _t(X_new, cuda), _t(S, cuda), c["R"], c["pos_dim"], c["tol"],
                             viol, vmax)
    return viol.cpu().numpy(), vmax.cpu().numpy()


@pytest.mark.parametrize("name", list(cc.CHECK_CASES))
def test_check_matches_reference(cuda, name):
    c = cc.CHECK_CASES[name]
    viol, vmax = _launch_check(cuda, c)
    K = c["X"].shape[1]
    saw_nan = False
    for a in range(c["n_local"]):
        for t in range(K - 1):
            v, mag = cr.check_ref(c["X"], c["i0"] + a, t, c["X_new"][a], c["S"][a, t], c["R"], c["pos_dim"], scale=True)
            nan = np.isnan(v)
            where = (name, a, t)
            assert viol[a, t] == int(((v > c["tol"]) | nan).sum()), where
            if nan.any():
                saw_nan = True
                assert np.isnan(vmax[a, t]), where
            elif v.size:
                assert abs(cr.LD(vmax[a, t]) - v.max()) <= 16 * cr.EPS * mag, (where, vmax[a, t], float(v.max()))
            else:
                assert vmax[a, t] == EMPTY_VMAX, where
    assert (viol[:, K - 1] == 0).all() and (vmax[:, K - 1] == 0).all()
    assert saw_nan == (name == "coincident_shard")
    if name == "slack1e3":
        assert (viol == 0).all()


def test_check_does_not_depend_on_the_agent_numbering(cuda):
    c = cc.CHECK_CASES["tiles_all"]
    perm = np.random.default_rng(106).permutation(cc.N_TILES)
    viol, vmax = _launch_check(cuda, c)
    viol_p, vmax_p = _launch_check(cuda, c, c["X"][perm], c["X_new"][perm], c["S"][perm])
    np.testing.assert_array_equal(viol_p, viol[perm])
    np.testing.assert_array_equal(vmax_p, vmax[perm])
    assert viol.max() > 0 and (viol == 0).any()


def test_argument_checks(cuda):
    """SCVX_EINVAL without a launch (the outputs keep their fill) for every argument outside its range; N_local = 0
    is OK and writes nothing.  The buffers are sized for the largest value tried."""
    import torch
    L = scvx_hip.lib()
    N, K, nx, pd, jm = 8, 4, 6, 3, 8
    X = torch.randn((N, 65, nx), dtype=torch.float64, device=cuda)
    X_new = torch.randn((N, 65, nx), dtype=torch.float64, device=cuda)
    S = torch.zeros((N, 65), dtype=torch.float64, device=cuda)
    idx = torch.arange(N, dtype=torch.int32, device=cuda)
    rows = torch.full((N, 65, 33, 4), cr.SENTINEL, dtype=torch.float64, device=cuda)
    cnt = torch.full((N, 65), -7, dtype=torch.int32, device=cuda)
    viol = torch.full((N, 65), -7, dtype=torch.int32, device=cuda)
    vmax = torch.full((N, 65), cr.SENTINEL, dtype=torch.float64, device=cuda)
    p = lambda t: t.data_ptr()  # noqa: E731

    def batched(K=K, pd=pd, nx=nx, N=N, i0=0, nl=N, jm=jm):
        return L.scvx_collision_rows_batched(K, pd, nx, N, p(X), i0, nl, 0.5, 0.0, jm, p(rows), p(cnt), None)

    def indexed(K=K, pd=pd, nx=nx, N=N, nl=N, jm=jm, i0=None):
        return L.scvx_collision_rows_indexed(K, pd, nx, N, p(X), p(idx), nl, 0.5, 0.0, jm, p(rows), p(cnt), None)

    def check(K=K, pd=pd, nx=nx, N=N, i0=0, nl=N, jm=None):
        return L.scvx_collision_check_batched(K, pd, nx, N, p(X), i0, nl, 0.5, p(X_new), p(S), 1e-7, p(viol), p(vmax),
                                              None)

    bad = [dict(K=1), dict(K=65), dict(pd=0), dict(pd=4), dict(pd=3, nx=2)]
    for f in (batched, indexed, check):
        for kw in bad:
            assert f(**kw) == -1, (f.__name__, kw)            # SCVX_EINVAL
    for f in (batched, indexed):
        for jmax in (0, 33):
            assert f(jm=jmax) == -1, (f.__name__, jmax)
    for f in (batched, check):
        for kw in (dict(i0=1, nl=N), dict(i0=N, nl=1), dict(i0=-1, nl=1)):
            assert f(**kw) == -1, (f.__name__, kw)
    for f in (batched, indexed, check):
        assert f(nl=0) == 0, f.__name__
    torch.cuda.synchronize()
    assert (rows == cr.SENTINEL).all() and (cnt == -7).all() and (viol == -7).all() and (vmax == cr.SENTINEL).all()
    # and the in-range call does launch
    assert batched() == 0 and indexed() == 0 and check() == 0
    torch.cuda.synchronize()
    assert (cnt.flatten()[:N * K] != -7).all() and (viol.flatten()[:N * K] != -7).all()
