"""CPU: the extended-precision reference of the collision kernels (tests/collision_ref.py) and the fixtures of
tests/test_collision_kernels_gpu.py (tests/collision_cases.py), proven on the reference alone.

  * the reference against oracle/problems.collision_rows, the double-precision restatement of
    dist_scvx_3d.py:93-107, in exact mode;
  * the fixture conditions: on every random fixture the selection, the cull test and the violation count are
    decided by margins far above double rounding, so a failure on the GPU is the kernel's, never a flaky tie;
  * the coverage conditions: every fixture really contains the situation it is there for;
  * the acceptance rule (assert_rows_valid) rejects each kind of wrong kept set."""
import numpy as np
import pytest

import collision_cases as cc
import collision_ref as cr
from oracle import problems as pb

GAP = 1e-9


@pytest.mark.parametrize("pos_dim,seed", [(3, 143), (2, 7), (1, 8)])
def test_reference_matches_the_double_restatement(pos_dim, seed):
    X = cc.cloud(N=33, seed=seed, pos_dim=pos_dim, junk=pos_dim < 3)
    trajs = [X[i] for i in range(X.shape[0])]
    for gi in (0, 7, 32):
        want = pb.collision_rows(trajs, gi, cc.R, pos_dim)
        for t in range(X.shape[1] - 1):
            ref = cr.rows_ref(X, gi, t, cc.R, pos_dim, 0.0)
            assert ref.idx.tolist() == [j for j in range(33) if j != gi]
            w = want[t]
            assert np.abs(w[:, :pos_dim] - ref.g).max() <= 8 * cr.EPS
            tol_b = 16 * cr.EPS * (2 * cc.R + ref.nr + np.abs(ref.g * X[gi, t, :pos_dim]).sum(axis=1))
            assert (np.abs(w[:, pos_dim] - ref.b) <= tol_b).all()
            # the check's row value at dp, S is the row at the moved point: b - g . p_new - S
            X_new = X[gi] + 0.1
            v = cr.check_ref(X, gi, t, X_new, 0.25, cc.R, pos_dim)
            v_rows = ref.b - (ref.g * X_new[t, :pos_dim]).sum(axis=1) - 0.25
            assert float(np.abs(v - v_rows).max()) <= 1e-15 * (1 + float(np.abs(ref.b).max()))


def test_reference_culls_strictly():
    X = cc.lattice()
    centre = 62                                   # site (0, 0, 0) at node 0
    assert (X[centre, 0, :3] == 0).all()
    ref = cr.rows_ref(X, centre, 0, cc.R, 3, 2.0)
    d2 = np.sort(ref.d2.astype(np.float64))
    assert d2.tolist() == [1.0] * 6 + [2.0] * 12 + [3.0] * 8      # the 6 at distance exactly 2 are out
    assert cr.rows_ref(X, centre, 0, cc.R, 3, 0.0).idx.size == 124
    assert cr.rows_ref(X, 0, 0, cc.R, 3, 2.0).idx.size == 7       # a corner: 3 + 3 + 1


@pytest.mark.parametrize("name", [n for n, c in cc.ROW_CASES.items() if c["random"]])
def test_row_fixture_conditions(name):
    c = cc.ROW_CASES[name]
    K = c["X"].shape[1]
    for gi in cc.agents_of(c):
        for t in range(K - 1):
            ref = cc.row_ref(c, gi, t)
            assert cr.kept_gap(ref, c["j_max"]) > GAP, (name, gi, t)
            if c["cull"] > 0:
                assert cr.cull_gap(c["X"], gi, t, c["pos_dim"], c["cull"]) > GAP, (name, gi, t)


def test_permutation_fixture_is_tie_free_for_every_agent():
    """The permutation-invariance tests launch all 1100 agents of the multi-tile fixture."""
    X = cc.multi_tile()
    for gi in range(cc.N_TILES):
        for t in range(X.shape[1] - 1):
            assert cr.kept_gap(cr.rows_ref(X, gi, t, cc.R, 3, 0.0), 8) > GAP, (gi, t)


@pytest.mark.parametrize("name", list(cc.CHECK_CASES))
def test_check_fixture_conditions(name):
    c = cc.CHECK_CASES[name]
    K = c["X"].shape[1]
    for a in range(c["n_local"]):
        for t in range(K - 1):
            v = cr.check_ref(c["X"], c["i0"] + a, t, c["X_new"][a], c["S"][a, t], c["R"], c["pos_dim"])
            v = v[~np.isnan(v)]
            if v.size:
                assert float(np.abs(v - c["tol"]).min()) > GAP, (name, a, t)


def test_check_fixtures_count_something():
    """The shard fixture has nodes with and without violated rows, and rows the distance bound can skip."""
    c = cc.CHECK_CASES["tiles_shard"]
    n = np.array([[int((cr.check_ref(c["X"], c["i0"] + a, t, c["X_new"][a], c["S"][a, t], c["R"], 3) > c["tol"]).sum())
                   for t in range(c["X"].shape[1] - 1)] for a in range(c["n_local"])])
    assert (n == 0).any() and (n >= 3).any(), np.bincount(n.ravel())
    c = cc.CHECK_CASES["slack1e3"]
    assert all((cr.check_ref(c["X"], c["i0"] + a, 0, c["X_new"][a], c["S"][a, 0], c["R"], 3) < -900).all()
               for a in range(c["n_local"]))


def _eligible(c):
    K = c["X"].shape[1]
    return np.array([[cc.row_ref(c, gi, t).idx.size for t in range(K - 1)] for gi in cc.agents_of(c)])


def test_cull_fixtures_cover_every_count():
    for name in ("cull", "pd1_junk_cull", "pd2_junk_cull", "indexed_cull"):
        c = cc.ROW_CASES[name]
        E = _eligible(c)
        assert (E == 0).any() and ((E > 0) & (E < c["j_max"])).any() and (E > c["j_max"]).any(), (name, np.bincount(E.ravel()))
    assert (_eligible(cc.ROW_CASES["cull_none"]) == 0).all()
    E = _eligible(cc.ROW_CASES["lattice_cull2_j8"])
    assert E.min() == 7 and E.max() == 26              # corners and interior sites
    assert all((_eligible(cc.ROW_CASES[f"short_n{n}"]) == n - 1).all() for n in (1, 2, 5))
    assert (_eligible(cc.ROW_CASES["exact_n33"]) == 32).all()


def test_multi_tile_fixture_reaches_every_tile():
    c = cc.ROW_CASES["multi_tile"]
    last_tile = two_tiles = loose = tight = 0
    X = c["X"]
    for gi in cc.agents_of(c):
        for t in range(X.shape[1] - 1):
            ref = cc.row_ref(c, gi, t)
            order = np.argsort(ref.d2, kind="stable")[:c["j_max"]]
            kept = ref.idx[order]
            last_tile += kept[0] >= 1024
            two_tiles += len(set((kept // 512).tolist())) >= 2
            # tau: the j_max-th nearest of the agent's block-mates, against its true j_max-th nearest
            b0 = c["i0"] + (gi - c["i0"]) // 64 * 64
            mates = (ref.idx >= b0) & (ref.idx < min(b0 + 64, c["i0"] + c["n_local"]))
            dm = np.sort(ref.d2[mates])
            if dm.size >= c["j_max"]:
                ratio = float(dm[c["j_max"] - 1] / ref.d2[order[-1]])
                tight += ratio < 4.0
                loose += ratio > 100.0
    assert last_tile >= 5 and two_tiles >= 50 and loose >= 20 and tight >= 20, (last_tile, two_tiles, loose, tight)
    # the blocks of the shard straddle the tile boundary, and the last one has 2 live lanes
    assert c["i0"] < 512 < c["i0"] + 64 and c["n_local"] % 64 == 2
    assert cc.N_TILES % 512 % 8 == 4
    idx = cc.indexed_agents()
    assert len(set(idx.tolist())) == 70 and (np.diff(idx) < 0).any() and idx.max() >= 1024


def test_coincident_fixtures_hold_one_pair():
    for X in (cc.ROW_CASES["coincident"]["X"], cc.CHECK_CASES["coincident_shard"]["X"]):
        ref = cr.rows_ref(X, 40, 1, cc.R, 3, 0.0)
        assert np.isnan(ref.g).all(axis=1).sum() == 1 and ref.idx[np.isnan(ref.b)].tolist() == [41]
        assert not np.isnan(cr.rows_ref(X, 40, 0, cc.R, 3, 0.0).g).any()
        assert not np.isnan(cr.rows_ref(X, 39, 1, cc.R, 3, 0.0).g).any()


def _kernel_like(ref, keep, j_max, pd):
    rows = np.full((j_max, pd + 1), cr.SENTINEL)
    rows[:len(keep), :pd] = ref.g[keep].astype(np.float64)
    rows[:len(keep), pd] = ref.b[keep].astype(np.float64)
    return rows


def test_acceptance_rule_rejects_wrong_sets():
    X, gi, t, j_max = cc.cloud(), 30, 0, 8
    ref = cr.rows_ref(X, gi, t, cc.R, 3, 0.0)
    p_i = X[gi, t, :3]
    order = np.argsort(ref.d2, kind="stable")
    good = order[:j_max][::-1]                                          # any row order
    kept = cr.assert_rows_valid(_kernel_like(ref, good, j_max, 3), j_max, ref, j_max, p_i, cc.R)
    assert sorted(kept.tolist()) == sorted(ref.idx[good].tolist())
    bad = {"a farther neighbour kept": (np.r_[order[:j_max - 1], order[j_max]], j_max),
           "one neighbour twice": (np.r_[order[:j_max - 1], order[0]], j_max),
           "short count": (order[:j_max - 1], j_max - 1)}
    for why, (keep, n) in bad.items():
        with pytest.raises(AssertionError):
            cr.assert_rows_valid(_kernel_like(ref, keep, j_max, 3), n, ref, j_max, p_i, cc.R)
            pytest.fail(why)
    rows = _kernel_like(ref, good, j_max, 3)
    rows[3, 1] += 32 * cr.EPS                                           # a row off by more than its rounding
    with pytest.raises(AssertionError):
        cr.assert_rows_valid(rows, j_max, ref, j_max, p_i, cc.R)
    d = np.sqrt(ref.d2[order])
    few = cr.rows_ref(X, gi, t, cc.R, 3, float((d[3] + d[4]) / 2))     # fewer eligible than j_max
    assert few.idx.size == 4
    rows = _kernel_like(few, np.arange(few.idx.size), j_max, 3)
    cr.assert_rows_valid(rows, few.idx.size, few, j_max, p_i, cc.R)
    rows[few.idx.size, 0] = 0.0                                         # a slot behind count written
    with pytest.raises(AssertionError):
        cr.assert_rows_valid(rows, few.idx.size, few, j_max, p_i, cc.R)
    # a coincident neighbour's NaN row is that neighbour's row; its twin rows at a third agent are two neighbours
    Xc = cc.ROW_CASES["coincident"]["X"]
    for gi in (40, 39):
        ref = cr.rows_ref(Xc, gi, 1, cc.R, 3, 0.0)
        keep = np.argsort(ref.d2, kind="stable")[:32]
        rows = _kernel_like(ref, keep, 32, 3)
        assert np.isnan(rows).any() == (gi == 40)
        kept = cr.assert_rows_valid(rows, 32, ref, 32, Xc[gi, 1, :3], cc.R)
        assert {40, 41} - {gi} <= set(kept.tolist()) and len(set(kept.tolist())) == 32
        other = np.argmax(~np.isin(ref.idx[keep], (40, 41)))
        rows[np.argmax(ref.idx[keep] == 41)] = rows[other]              # the twin's row replaced by another's
        with pytest.raises(AssertionError):
            cr.assert_rows_valid(rows, 32, ref, 32, Xc[gi, 1, :3], cc.R)
    # exact ties: any 2 of the lattice's 12 second neighbours, but all 6 first neighbours
    L = cc.lattice()
    ref = cr.rows_ref(L, 62, 0, cc.R, 3, 0.0)
    first, second = np.nonzero(ref.d2 == 1)[0], np.nonzero(ref.d2 == 2)[0]
    for pick in (second[:2], second[-2:]):
        cr.assert_rows_valid(_kernel_like(ref, np.r_[first, pick], 8, 3), 8, ref, 8, L[62, 0, :3], cc.R)
    with pytest.raises(AssertionError):
        cr.assert_rows_valid(_kernel_like(ref, np.r_[first[:5], second[:3]], 8, 3), 8, ref, 8, L[62, 0, :3], cc.R)
