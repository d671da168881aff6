"""Moving obstacles on the GPU (csrc/moving_obstacles.hip) against their numpy restatement
(tests/moving_obstacles_ref.py), and the Jacobi driver with them on.

Kernel shapes: separation_ref.random_fleet("di", 70, 5, 3), so N (K-1) = 280 lanes: four full workgroups of 64 and
one of 24; every agent has its own sigma in 1..3.  S = 3 and 16, pos_dim 2 and 3 (planar knots, zero-padded).
Tracks from moving_obstacles_ref.random_tracks(19, pd, 12, box): 1, 2 and 5 knots in turn in one list, rho uniform
in 0.5..1.5; track 1 starts after t = 0, track 2 stops before the shortest sigma, track 4's window covers every
agent's horizon; O = 1, 5 and 19 (the first O of them); J = 1, 2 and 8 (every list class).  cull = 4.5, the static
test's.  The knots are uniform in +-9 at pos_dim 3 and +-16 at pos_dim 2: inside the fleet's own +-6 every node has a
track within cull + rho and no node list is empty (in the plane none within +-12 either).  The samples are the kernel's
own (rollout_dense), the restatement runs on the same P and sigma, and the comparison's conditions are asserted on the
restatement: lists with more candidates than J, partly filled and empty ones (segment and node lists), a penetrating
candidate in both, no v within 1e-9 of -cull, no two v of a list within 1e-9 of each other, no unclamped chord
parameter within 1e-9 of 0 on a first chord or of 1 on a last one -- so the 1e-12 comparison (the figure of
tests/test_obstacle_rows_gpu.py for this same arithmetic: GPU against the same algorithm on the CPU) never compares two
different selections."""
import functools

import numpy as np
import pytest

import moving_obstacles_ref as mo
import obstacle_rows_ref as orf
import separation_ref as sr

pytestmark = pytest.mark.gpu
N, K, SEED, CULL, TSEED, BOX = 70, 5, 3, 4.5, 12, {2: 16.0, 3: 9.0}
CASES = [(pd, S, O, J) for pd in (2, 3) for S in (3, 16) for O in (1, 5, 19) for J in (1, 2, 8)]


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda:0")


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def tracks(pd, O):
    return mo.random_tracks(19, pd, TSEED, BOX[pd])[:O]


@functools.lru_cache(maxsize=None)
def _samples(pd, S):
    """The kernel's own samples (device and host) and the fleet."""
    import scvx_hip
    X, U, sig = sr.random_fleet("di", N, K, SEED)
    assert len(set(sig.tolist())) == N                                          # every agent on a clock of its own
    Pd, _ = scvx_hip.rollout_dense("di", _t(X), _t(U), _t(sig), S=S, pos_dim=pd)
    return X, U, sig, Pd, Pd.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _minima(pd, S, O):
    trk = mo.pad_tracks(tracks(pd, O))
    X, U, sig, _, P = _samples(pd, S)
    return trk, mo.minima(P, sig, trk), mo.node_values(P, sig, trk)


@functools.lru_cache(maxsize=None)
def _ref(pd, S, O, J):
    X, U, sig, _, P = _samples(pd, S)
    trk = _minima(pd, S, O)[0]
    return mo.segment_records(P, sig, trk, CULL, J), mo.node_records(P, sig, trk, CULL, J)


@functools.lru_cache(maxsize=None)
def _gpu(pd, S, O, J):
    import scvx_hip
    X, U, sig, Pd, _ = _samples(pd, S)
    return scvx_hip.moving_obstacle_scan(Pd, _t(sig), tracks(pd, O), cull=CULL, J=J)


@pytest.mark.parametrize("pd,S", [(pd, S) for pd in (2, 3) for S in (3, 16)])
def test_the_inputs_cover_full_partial_and_empty_lists(cuda, pd, S):
    """On the restatement (O = 19), for the segment lists and the node lists: lists with more candidates than J = 1
    and 2, lists partly filled at J = 2 and 8, empty lists, penetrating candidates; and the three windows."""
    trk, (Q, Sx, A, C), (d0, NV) = _minima(pd, S, 19)
    sig = _samples(pd, S)[2]
    n, nn = orf.candidates(Q, Sx, A, S, trk[3], CULL).sum(0), mo.node_candidates(d0, NV, CULL).sum(0)
    print(f"pos_dim={pd} S={S}: up to {n.max()} / {nn.max()} candidates per segment / node list, "
          f"{int((n == 0).sum())} / {int((nn == 0).sum())} of {n.size} lists empty")
    for c in (n, nn):
        assert (c > 2).any() and (c == 1).any() and (c == 0).any()
    assert (orf.values(Q, trk[3])[orf.candidates(Q, Sx, A, S, trk[3], CULL)] > 0).any()
    assert (NV[mo.node_candidates(d0, NV, CULL)] > 0).any()
    nk, win = trk[1], trk[2]
    assert sorted(set(nk.tolist())) == [1, 2, 5]
    assert win[1, 0] > 0 and nk[1] > 1 and win[2, 1] < sig.min() and nk[2] > 1
    assert win[4, 0] <= 0 and win[4, 1] >= sig.max() and nk[4] > 1


@pytest.mark.parametrize("pd,S,O,J", CASES)
def test_scan_and_records_match_the_restatement(cuda, pd, S, O, J):
    X, U, sig, _, P = _samples(pd, S)
    trk, (Q, Sx, A, C), (d0, NV) = _minima(pd, S, O)
    rho = trk[3]
    # the conditions of the comparison, on the CPU side
    V = orf.values(Q, rho)
    inner = orf.candidates(Q, Sx, A, S, rho, np.inf)
    cand, ncand = orf.candidates(Q, Sx, A, S, rho, CULL), mo.node_candidates(d0, NV, CULL)
    assert np.abs(V[inner] + CULL).min() > 1e-9 and np.abs(NV + CULL).min() > 1e-9   # nothing at the cull threshold
    for vals, cd in ((V, cand), (NV, ncand)):                                     # kept or dropped: no two v tie
        vs = np.sort(np.where(cd, vals, np.inf), axis=0)
        with np.errstate(invalid="ignore"):
            gaps = np.diff(vs, axis=0)
        assert O == 1 or gaps[np.isfinite(gaps)].min(initial=np.inf) > 1e-9
    u0, u1 = mo.edge_params(mo.relative(P, sig, trk))                            # inner or not: nothing on the edge
    assert np.nanmin(np.abs(u0)) > 1e-9 and np.nanmin(np.abs(u1 - 1.0)) > 1e-9
    (rec_r, obs_r, al_r, cnt_r, sel_r), (nrec_r, nobs_r, ncnt_r) = _ref(pd, S, O, J)
    dist_r, alpha_r = mo.scan(P, sig, trk)
    g = _np(_gpu(pd, S, O, J))
    scale = np.abs(P).max()
    e_rec, e_al = np.abs(g["rec"] - rec_r).max() / scale, np.abs(g["rec_alpha"] - al_r).max()
    e_nrec = np.abs(g["node_rec"] - nrec_r).max() / scale
    e_d, e_a = np.abs(g["dist"] - dist_r).max() / scale, np.abs(g["alpha"] - alpha_r).max()
    print(f"pos_dim={pd} S={S} O={O} J={J}: (g, v) {e_rec:.2e}, node (g, v) {e_nrec:.2e}, dist {e_d:.2e} of the position "
          f"scale, alpha' {max(e_al, e_a):.2e}; segment lists: {int((cand.sum(0) > J).sum())} over J, "
          f"{int((cnt_r == 0).sum())} empty; node lists: {int((ncand.sum(0) > J).sum())} over J, "
          f"{int((ncnt_r == 0).sum())} empty")
    assert g["dist"].shape == (N, K - 1, O) and g["rec"].shape == g["node_rec"].shape == (N, K - 1, J, 4)
    assert np.array_equal(g["count"], cnt_r) and np.array_equal(g["obs"], obs_r)
    assert np.array_equal(g["node_count"], ncnt_r) and np.array_equal(g["node_obs"], nobs_r)
    assert e_rec <= 1e-12 and e_nrec <= 1e-12 and e_d <= 1e-12 and e_al <= 1e-12 and e_a <= 1e-12
    # the selected sub-interval: s = floor(alpha' S) (read away from the samples, where alpha' S is an integer)
    kept = obs_r >= 0
    frac = al_r * S - sel_r
    mid = kept & (frac > 1e-9) & (frac < 1 - 1e-9)
    assert mid.any() and np.array_equal(np.floor(g["rec_alpha"][mid] * S), sel_r[mid])
    assert not g["rec"][..., pd:3].any() and not g["node_rec"][..., pd:3].any()   # zeros past pos_dim
    # v is rho minus the scan's own distance to that track, bit for bit
    a, k, r = np.nonzero(kept)
    assert np.array_equal(g["rec"][a, k, r, 3], rho[g["obs"][a, k, r]] - g["dist"][a, k, g["obs"][a, k, r]])


@pytest.mark.parametrize("pd,S,O,J", [(2, 3, 19, 1), (3, 16, 19, 8), (3, 3, 5, 2), (2, 16, 1, 2)])
def test_one_knot_tracks_are_the_static_scan_bit_for_bit(cuda, pd, S, O, J):
    import scvx_hip
    X, U, sig, Pd, _ = _samples(pd, S)
    rng = np.random.default_rng(11)
    c, rho = rng.uniform(-6.0, 6.0, (19, 3)), rng.uniform(0.5, 1.5, 19)
    obs = [(c[o, :pd].copy(), float(rho[o])) for o in range(O)]
    # (the window of a one-knot track is not read: any will do)
    mov = _np(scvx_hip.moving_obstacle_scan(Pd, _t(sig), [(ctr, (3.0, 1.0) if o % 2 else None, r)
                                                         for o, (ctr, r) in enumerate(obs)], cull=CULL, J=J))
    sta = _np(scvx_hip.obstacle_scan(Pd, obs, cull=CULL, J=J))
    assert int(sta["count"].sum()) > 0
    for key in ("dist", "alpha", "rec", "obs", "rec_alpha", "count"):
        assert np.array_equal(mov[key], sta[key]), key


@pytest.mark.parametrize("pd,S,O,J", [(2, 3, 19, 1), (3, 16, 19, 8), (3, 3, 5, 2), (2, 16, 1, 2)])
def test_a_slice_and_each_group_alone_are_the_full_call_bit_for_bit(cuda, pd, S, O, J):
    import torch
    import scvx_hip
    X, U, sig, Pd, _ = _samples(pd, S)
    sd, trk = _t(sig), scvx_hip.obstacle_tracks(tracks(pd, O), "cuda:0")
    full = _np(_gpu(pd, S, O, J))
    part = _np(scvx_hip.moving_obstacle_scan(Pd[17:57], sd[17:57], trk, cull=CULL, J=J))
    assert sorted(part) == sorted(full) and len(full) == 9
    for key in full:
        assert np.array_equal(part[key], full[key][17:57]), key
    # the groups alone: analysis only (J = 0), segment records only, segment and node records
    ana = _np(scvx_hip.moving_obstacle_scan(Pd, sd, trk))
    recs = _np(scvx_hip.moving_obstacle_scan(Pd, sd, trk, cull=CULL, J=J, analysis=False, node_rows=False))
    both = _np(scvx_hip.moving_obstacle_scan(Pd, sd, trk, cull=CULL, J=J, analysis=False))
    assert sorted(ana) == ["alpha", "dist"] and sorted(recs) == ["count", "obs", "rec", "rec_alpha"]
    assert sorted(both) == ["count", "node_count", "node_obs", "node_rec", "obs", "rec", "rec_alpha"]
    for got in (ana, recs, both):
        for key in got:
            assert np.array_equal(got[key], full[key]), key
    # the node group alone is reached through the C entry point only
    nrec = torch.empty((N, K - 1, J, 4), dtype=torch.float64, device="cuda:0")
    nobs = torch.empty((N, K - 1, J), dtype=torch.int32, device="cuda:0")
    ncnt = torch.empty((N, K - 1), dtype=torch.int32, device="cuda:0")
    rc = scvx_hip.lib().scvx_moving_obstacle_scan_batched(
        K, S, N, Pd.data_ptr(), sd.data_ptr(), O, trk[0].shape[1], trk[0].data_ptr(), trk[1].data_ptr(),
        trk[2].data_ptr(), trk[3].data_ptr(), CULL, J, None, None, None, None, None, None, nrec.data_ptr(),
        nobs.data_ptr(), ncnt.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    for key, got in (("node_rec", nrec), ("node_obs", nobs), ("node_count", ncnt)):
        assert np.array_equal(got.cpu().numpy(), full[key]), key


@pytest.mark.parametrize("pd", [2, 3])
def test_fleet_clearance_against_the_closed_form_truth(cuda, pd):
    """Roll-out plus scan at S = 8 against the exact cubic minus the exact line on 2000 points per segment, constant-
    velocity tracks whose window covers every horizon (no velocity jump: r'' = p''): within the chord bound of it,
    and never above the node-level minimum (the nodes are samples)."""
    import scvx_hip
    X, U, sig = sr.random_fleet("di", N, K, SEED)
    rng = np.random.default_rng(5)
    trs = [(rng.uniform(-6.0, 6.0, (2, 3))[:, :pd], (-0.5, 3.5), float(r)) for r in rng.uniform(0.5, 1.5, 19)]
    rr, S = 0.3, 8
    out = scvx_hip.fleet_moving_obstacle_clearance("di", _t(X), _t(U), _t(sig), trs, robot_radius=rr, S=S, pos_dim=pd)
    trk = mo.pad_tracks(trs)
    Xp, Up = X.copy(), U.copy()
    Xp[:, :, pd:3], Xp[:, :, 3 + pd:6], Up[:, :, pd:] = 0.0, 0.0, 0.0           # the truth of the first pd coordinates
    truth = mo.di_truth(Xp, Up, sig, trk, M=2000) - rr
    bound = sr.di_chord_bound(Up, sig, K, S)
    clear = out["clear"].cpu().numpy()
    print(f"pos_dim={pd}: clearance vs truth: {np.abs(clear - truth).max():.2e} (bound {bound:.2e}), min {out['min']:.4f}")
    assert clear.shape == (N, K - 1, 19) and out["tau"].shape == (N, K - 1, 19)
    assert (truth >= clear - bound - 1e-12).all()                                # within the chord bound below it
    assert (truth <= clear + bound + sr.di_chord_bound(Up, sig, K, 2000) + 1e-12).all()
    D = out["D"].cpu().numpy()
    # (nodes 0..K-2 are samples; the random fleet's node K-1 is not where its last segment's roll-out ends)
    node = mo.node_clearance(Xp, sig, trk)[:, :-1].min(1) - rr
    assert D.shape == (N, 19) and (D <= node + 1e-12).all() and (D < node - 1e-3).any()
    assert np.array_equal(D, clear.min(1)) and np.array_equal(out["agent_min"].cpu().numpy(), D.min(1))
    i, o, k, tau = out["argmin"]
    assert out["min"] == clear.min() == clear[i, k, o] and tau == float(out["tau"][i, k, o].item()) and 0 <= tau <= 1


def test_analysis_wrapper_returns_the_matrix(cuda):
    import scvx_hip
    from SCvx.utils import analysis
    X, U, sig = sr.random_fleet("di", 6, K, SEED)
    trs = tracks(3, 5)
    d_min, d_mat = analysis.min_agent_moving_obstacle_clearance_continuous([x.T for x in X], [u.T for u in U], "di", sig,
                                                                           trs, 0.3, S=8)
    out = scvx_hip.fleet_moving_obstacle_clearance("di", _t(X), _t(U), _t(sig), trs, robot_radius=0.3, S=8)
    assert d_mat.shape == (6, 5) and np.array_equal(d_mat, out["D"].cpu().numpy()) and d_min == d_mat.min() == out["min"]


@pytest.mark.parametrize("pd", [2, 3])
def test_append_node_rows_matches_the_restatement(cuda, pd):
    """The plain and the idx form: g bit for bit, b within 1e-13 (the figure of the pair records' append); rows that
    do not fit j_max are counted and not written."""
    import torch
    import scvx_hip
    X, U, sig, Pd, P = _samples(pd, 3)
    g = _gpu(pd, 3, 19, 2)
    nrec, ncnt = g["node_rec"].cpu().numpy(), g["node_count"].cpu().numpy()
    rng = np.random.default_rng(2)
    for j_max, idx in ((4, None), (2, None), (4, np.array([5, 66, 2, 40, 40], np.int32))):
        n = N if idx is None else len(idx)
        rows0, count0 = rng.normal(size=(n, K, j_max, pd + 1)), rng.integers(0, 3, (n, K)).astype(np.int32)
        want_r, want_c, want_o = mo.append_node_rows(X, 0, idx, nrec, ncnt, rows0, count0, pd)
        rows, count = _t(rows0), _t(count0, torch.int32)
        _, _, over = scvx_hip.append_node_rows(_t(X), 0, g["node_rec"], g["node_count"], rows, count, pos_dim=pd,
                                               idx=None if idx is None else _t(idx, torch.int32))
        assert int(over.item()) == want_o and (want_o > 0) == (j_max == 2)
        assert np.array_equal(count.cpu().numpy(), want_c)
        got = rows.cpu().numpy()
        assert np.array_equal(got[..., :pd], want_r[..., :pd]) and np.abs(got[..., pd] - want_r[..., pd]).max() <= 1e-13
    with pytest.raises(ValueError):
        scvx_hip.append_node_rows(_t(X), 0, g["node_rec"], g["node_count"], rows, count, pos_dim=pd,
                                  idx=_t(np.array([70], np.int32), torch.int32))


def test_wrapper_and_driver_reject_bad_arguments(cuda):
    import scvx_hip
    from scvx_hip.scvx import JacobiSCvx, MovingObstaclesSpec
    X, U, sig, Pd, _ = _samples(3, 3)
    sd, trs = _t(sig), tracks(3, 5)
    for kw in (dict(J=9), dict(J=-1), dict(J=1, cull=0.0), dict(J=0, analysis=False)):
        with pytest.raises(ValueError):
            scvx_hip.moving_obstacle_scan(Pd, sd, trs, **kw)
    two = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    for bad in ([], [(two, (1.0, 1.0), 0.5)], [(two, (2.0, 1.0), 0.5)]):           # empty; t1 <= t0 with two knots
        with pytest.raises(ValueError):
            scvx_hip.moving_obstacle_scan(Pd, sd, bad)
    with pytest.raises(ValueError):
        scvx_hip.moving_obstacle_scan(Pd[..., :2], sd, trs)
    with pytest.raises(ValueError):                                                # S = 17
        scvx_hip.moving_obstacle_scan(_t(np.zeros((2, 4, 18, 3))), sd[:2], trs)
    with pytest.raises(ValueError):                                                # records need K <= 64
        scvx_hip.moving_obstacle_scan(_t(np.zeros((1, 64, 4, 3))), sd[:1], trs, J=1)
    assert scvx_hip.moving_obstacle_scan(_t(np.zeros((1, 64, 4, 3))), sd[:1], trs)["dist"].shape == (1, 64, 5)
    # cull None: the largest rho
    a = _np(scvx_hip.moving_obstacle_scan(Pd, sd, trs, J=2))
    b = _np(scvx_hip.moving_obstacle_scan(Pd, sd, trs, cull=max(r for _, _, r in trs), J=2))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    X0, U0, s0 = orf.fixture()

    def mk(j_max, trs=mo.TRACKS_A, **kw):
        return JacobiSCvx(scvx_hip.QPSpec(model="di", K=8, j_max=j_max), _t(X0[:, 0]), _t(X0[:, -1]), _t(s0), 4.0,
                          moving_obstacles=MovingObstaclesSpec(trs, **kw))

    assert mk(6)._mv["j_node"] == 0
    with pytest.raises(ValueError, match="capacity"):
        mk(5)                                                                      # cannot hold 3 J = 6
    for kw in (dict(S=17), dict(J=9)):
        with pytest.raises(ValueError):
            mk(32, **kw)
    with pytest.raises(ValueError):
        mk(8, trs=[])
    with pytest.raises(ValueError, match="t1 > t0"):
        mk(8, trs=[(two, (1.0, 1.0), 0.5)])


# ------------------------------------------------------------------ the driver
@functools.lru_cache(maxsize=None)
def _fixture_a(on):
    marks = []
    return mo.run_fixture(_t, None, on, mo.TRACKS_A, far=True, marks=marks) + (marks,)


@functools.lru_cache(maxsize=None)
def _tracks_b():
    return mo.tracks_b(_fixture_a(False)[0])


@functools.lru_cache(maxsize=None)
def _fixture_b(on):
    return mo.run_fixture(_t, None, on, _tracks_b(), far=True)


def test_fixture_a_bites_without_the_rows(cuda):
    """Fixture A of tests/test_moving_obstacles_cpu.py plus a second agent 100 away in z, on the kernels, 10
    iterations: no rows, the nodes clear the intruder and the curve passes deep inside it between two nodes."""
    X, U, sig, out, drv, marks = _fixture_a(False)
    cont, node, bound, st, slack = mo.fixture_figures(X, U, sig, out, mo.TRACKS_A)
    print(f"A off: continuous clearance {cont:.4f}, node clearance {node.min():.4f}, status {st}, slack {slack:.1e}")
    assert cont <= -0.5
    assert node.min() > 0 and st == 0
    assert "movrows" not in [m for m, _ in marks]


def test_fixture_a_clears_the_intruder_in_continuous_time_with_the_rows(cuda):
    X, U, sig, out, drv, marks = _fixture_a(True)
    cont, node, bound, st, slack = mo.fixture_figures(X, U, sig, out, mo.TRACKS_A)
    print(f"A on: continuous clearance {cont:.6f} (bound {bound:.2e}), node clearance {node.min():.6f}, status {st}, "
          f"slack {slack:.1e}")
    assert cont >= -bound
    assert st == 0
    assert slack < 1e-12
    assert mo.mov_overflow(drv) == 0
    assert [m for m, _ in marks].count("movrows") == mo.FIXTURE["iters"]
    # JacobiSCvx.moving_obstacle_clearance sees the same curve
    mc = drv.moving_obstacle_clearance(_t(X), _t(U), S=mo.FIXTURE["S"])
    assert abs(mc["D"][0, 0].item() - cont) <= bound and mc["D"][1, 0].item() > 90.0


def test_fixture_b_sits_on_the_node_without_the_rows(cuda):
    X, U, sig, out, drv = _fixture_b(False)
    cont, node, bound, st, slack = mo.fixture_figures(X, U, sig, out, _tracks_b())
    print(f"B off: node {mo.NODE_B} clearance {node[mo.NODE_B]:.6f}, continuous clearance {cont:.4f}")
    assert abs(node[mo.NODE_B] + mo.RHO) <= 1e-12 and st == 0


def test_fixture_b_clears_the_node_with_the_rows(cuda):
    X, U, sig, out, drv = _fixture_b(True)
    cont, node, bound, st, slack = mo.fixture_figures(X, U, sig, out, _tracks_b())
    print(f"B on: node clearance {node.min():.2e}, continuous clearance {cont:.6f} (bound {bound:.2e}), status {st}, "
          f"slack {slack:.1e}")
    assert node.min() >= -slack - 1e-9
    assert cont >= -bound
    assert st == 0
    assert mo.mov_overflow(drv) == 0


def test_the_far_agent_is_untouched(cuda):
    """No track within the far agent's reach: its X and U are bit-identical to the run with the option off at the
    same QPSpec.j_max (the fixture agent's are not)."""
    Xoff, Uoff = _fixture_a(False)[:2]
    Xon, Uon = _fixture_a(True)[:2]
    assert np.array_equal(Xon[1], Xoff[1]) and np.array_equal(Uon[1], Uoff[1])
    assert not np.array_equal(Xon[0], Xoff[0])


def test_tracks_out_of_reach_change_nothing(cuda):
    """Every track beyond cull: three steps are bit-identical to the option off."""
    far = [(np.array([[50.0, 50.0, 50.0], [51.0, 50.0, 50.0]]), (0.0, 7.0), 0.7), ((-50.0, 50.0, 0.0), None, 0.7)]
    on = mo.run_fixture(_t, None, True, far, far=True, iters=3)
    off = mo.run_fixture(_t, None, False, far, far=True, iters=3)
    assert int(on[4]._mv["count_seg"].sum()) == 0 and int(on[4]._mv["node_count"].sum()) == 0
    assert int(on[4].count.max()) == 0
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert not np.array_equal(on[0], orf.fixture(far=True)[0])


def test_a_coupled_step_with_all_record_kinds(cuda):
    """CouplingSpec with check=True, pair records, static obstacle records and moving obstacles in one node's rows:
    drv.count and the rows buffer are the restatement's order and content; the dense samples are shared (equal S);
    no overflow."""
    marks = []
    drv, Xp, out = mo.coupled_step(_t, None, marks=marks)
    assert [m for m, _ in marks][:7] == ["start", "foh", "gather", "rows", "isrows", "obsrows", "movrows"]
    assert int(out["status"].max()) == 0
    assert drv.last_check["is_overflow"] == drv.last_check["obs_overflow"] == drv.last_check["mov_overflow"] == 0
    assert getattr(drv.backend, "samples", None) is None                         # handed on and cleared
    mo.check_coupled_rows(drv, Xp)
