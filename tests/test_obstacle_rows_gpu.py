"""Continuous-time obstacle scan and rows on the GPU (csrc/obstacle_rows.hip) against their numpy restatement
(tests/obstacle_rows_ref.py), and the Jacobi driver with them on.

Kernel shapes: separation_ref.random_fleet("di", 70, 5, 3), so N (K-1) = 280 lanes: four full workgroups of 64 and
one of 24.  S = 3 and 16, pos_dim 2 and 3 (planar centres, zero-padded).  Obstacles from default_rng(11): centres
uniform in +-6, rho uniform in 0.5..1.5; O = 1, 5 and 19 (more than SCVX_MAX_OBS = 16: the list is a device array,
not a template field); J = 1, 2 and 8 (every list class).  cull = 4.5, the pair test's (1.5 leaves no list of
more than two candidates at pos_dim 3; 4.5 gives up to five, margins to the threshold >= 7.7e-3, gaps between the v
of a list >= 8.9e-4).  The samples are the kernel's own
(rollout_dense), the restatement runs on the same P, and the fixture's conditions are asserted on the restatement:
lists with more candidates than J, partly filled and empty ones, no candidate within 1e-9 of the cull threshold and
no two v of a list within 1e-9 of each other -- so the 1e-12 comparison (the figure of tests/test_intersample_rows_gpu.py
for this same arithmetic: GPU against the same algorithm on the CPU) never compares two different selections."""
import functools

import numpy as np
import pytest

import intersample_rows_ref as ir
import obstacle_rows_ref as orf
import separation_ref as sr

pytestmark = pytest.mark.gpu
N, K, SEED, CULL = 70, 5, 3, 4.5
CASES = [(pd, S, O, J) for pd in (2, 3) for S in (3, 16) for O in (1, 5, 19) for J in (1, 2, 8)]


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda:0")


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def obstacles(pd, O):
    """[(centre of pd coordinates, rho)]: the first O of the 19 drawn."""
    rng = np.random.default_rng(11)
    c, rho = rng.uniform(-6.0, 6.0, (19, 3)), rng.uniform(0.5, 1.5, 19)
    return [(c[o, :pd].copy(), float(rho[o])) for o in range(O)]


@functools.lru_cache(maxsize=None)
def _samples(pd, S):
    """The kernel's own samples (device and host)."""
    import scvx_hip
    X, U, sig = sr.random_fleet("di", N, K, SEED)
    Pd, _ = scvx_hip.rollout_dense("di", _t(X), _t(U), _t(sig), S=S, pos_dim=pd)
    return X, U, sig, Pd, Pd.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _minima(pd, S, O):
    c, rho = orf.pad_centers(obstacles(pd, O))
    return c, rho, orf.obstacle_minima(_samples(pd, S)[4], c)


@functools.lru_cache(maxsize=None)
def _ref(pd, S, O, J):
    c, rho, _ = _minima(pd, S, O)
    return orf.obstacle_rows(_samples(pd, S)[4], c, rho, CULL, J)


@functools.lru_cache(maxsize=None)
def _gpu(pd, S, O, J):
    import scvx_hip
    return scvx_hip.obstacle_scan(_samples(pd, S)[3], obstacles(pd, O), cull=CULL, J=J)


@pytest.mark.parametrize("pd,S", [(pd, S) for pd in (2, 3) for S in (3, 16)])
def test_the_inputs_cover_full_partial_and_empty_lists(cuda, pd, S):
    """On the restatement (O = 19): lists with more candidates than J = 1 and 2, lists partly filled at J = 2 and 8,
    empty lists, penetrating candidates."""
    c, rho, (Q, Sx, A, C) = _minima(pd, S, 19)
    n = orf.candidates(Q, Sx, A, S, rho, CULL).sum(0)
    print(f"pos_dim={pd} S={S}: up to {n.max()} candidates per list, {int((n == 0).sum())} of {n.size} lists empty")
    assert (n > 2).any() and (n == 1).any() and (n == 0).any() and n.max() < 8
    V = orf.values(Q, rho)
    assert (V[orf.candidates(Q, Sx, A, S, rho, CULL)] > 0).any()


@pytest.mark.parametrize("pd,S,O,J", CASES)
def test_scan_and_records_match_the_restatement(cuda, pd, S, O, J):
    P = _samples(pd, S)[4]
    c, rho, (Q, Sx, A, C) = _minima(pd, S, O)
    # the conditions of the comparison, on the CPU side
    V = orf.values(Q, rho)
    inner = orf.candidates(Q, Sx, A, S, rho, np.inf)
    cand = orf.candidates(Q, Sx, A, S, rho, CULL)
    assert np.abs(V[inner] + CULL).min() > 1e-9                                  # nothing at the cull threshold
    vs = np.sort(np.where(cand, V, np.inf), axis=0)                              # a list's candidates, ascending
    with np.errstate(invalid="ignore"):
        gaps = np.diff(vs, axis=0)
    assert O == 1 or gaps[np.isfinite(gaps)].min(initial=np.inf) > 1e-9          # kept or dropped: no two v tie
    rec_r, obs_r, al_r, cnt_r, sel_r = _ref(pd, S, O, J)
    dist_r, alpha_r = orf.scan(P, c)
    g = _np(_gpu(pd, S, O, J))
    scale = np.abs(P).max()
    e_rec, e_al = np.abs(g["rec"] - rec_r).max() / scale, np.abs(g["rec_alpha"] - al_r).max()
    e_d, e_a = np.abs(g["dist"] - dist_r).max() / scale, np.abs(g["alpha"] - alpha_r).max()
    print(f"pos_dim={pd} S={S} O={O} J={J}: (g, v) {e_rec:.2e}, dist {e_d:.2e} of the position scale, alpha' "
          f"{max(e_al, e_a):.2e}; lists: {int((cand.sum(0) > J).sum())} over J, {int((cnt_r == 0).sum())} empty")
    assert g["dist"].shape == (N, K - 1, O) and g["rec"].shape == (N, K - 1, J, 4)
    assert np.array_equal(g["count"], cnt_r) and np.array_equal(g["obs"], obs_r)
    assert e_rec <= 1e-12 and e_al <= 1e-12 * scale and e_d <= 1e-12 and e_a <= 1e-12 * scale
    # the selected sub-interval: s = floor(alpha' S) (read away from the samples, where alpha' S is an integer)
    kept = obs_r >= 0
    frac = al_r * S - sel_r
    mid = kept & (frac > 1e-9) & (frac < 1 - 1e-9)
    assert mid.any() and np.array_equal(np.floor(g["rec_alpha"][mid] * S), sel_r[mid])
    assert not g["rec"][..., pd:3].any()                                         # zeros past pos_dim
    # v is rho minus the scan's own distance to that obstacle, bit for bit
    a, k, r = np.nonzero(kept)
    assert np.array_equal(g["rec"][a, k, r, 3], rho[g["obs"][a, k, r]] - g["dist"][a, k, g["obs"][a, k, r]])


@pytest.mark.parametrize("pd,S,O,J", [(2, 3, 19, 1), (3, 16, 19, 8), (3, 3, 5, 2), (2, 16, 1, 2)])
def test_a_slice_is_the_matching_rows_bit_for_bit(cuda, pd, S, O, J):
    import scvx_hip
    Pd = _samples(pd, S)[3]
    full = _np(_gpu(pd, S, O, J))
    part = _np(scvx_hip.obstacle_scan(Pd[17:57], obstacles(pd, O), cull=CULL, J=J))
    for key in ("dist", "alpha", "rec", "obs", "rec_alpha", "count"):
        assert np.array_equal(part[key], full[key][17:57]), key
    # the groups alone: analysis only (J = 0), records only
    ana = _np(scvx_hip.obstacle_scan(Pd, obstacles(pd, O)))
    recs = _np(scvx_hip.obstacle_scan(Pd, obstacles(pd, O), cull=CULL, J=J, analysis=False))
    assert sorted(ana) == ["alpha", "dist"] and sorted(recs) == ["count", "obs", "rec", "rec_alpha"]
    for key in full:
        assert np.array_equal((ana if key in ana else recs)[key], full[key]), key


def test_wrapper_rejects_bad_arguments(cuda):
    import scvx_hip
    Pd = _samples(3, 3)[3]
    for kw in (dict(J=9), dict(J=-1), dict(J=1, cull=0.0), dict(J=0, analysis=False)):
        with pytest.raises(ValueError):
            scvx_hip.obstacle_scan(Pd, obstacles(3, 5), **kw)
    with pytest.raises(ValueError):
        scvx_hip.obstacle_scan(Pd, [])
    with pytest.raises(ValueError):
        scvx_hip.obstacle_scan(Pd[..., :2], obstacles(3, 5))
    # cull None: the largest rho
    obs5 = obstacles(3, 5)
    a = _np(scvx_hip.obstacle_scan(Pd, obs5, J=2))
    b = _np(scvx_hip.obstacle_scan(Pd, obs5, cull=max(r for _, r in obs5), J=2))
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("pd", [2, 3])
def test_fleet_obstacle_clearance_against_the_closed_form_truth(cuda, pd):
    """Roll-out plus scan at S = 8 against the exact cubic on 2000 points per segment: within the chord bound of it
    (r = p - c), and never above the node-level minimum (the nodes are samples)."""
    import scvx_hip
    X, U, sig = sr.random_fleet("di", N, K, SEED)
    obs, rr, S = obstacles(pd, 19), 0.3, 8
    out = scvx_hip.fleet_obstacle_clearance("di", _t(X), _t(U), _t(sig), obs, robot_radius=rr, S=S, pos_dim=pd)
    c, r = orf.pad_centers(obs)
    Xp, Up = X.copy(), U.copy()
    Xp[:, :, pd:3], Xp[:, :, 3 + pd:6], Up[:, :, pd:] = 0.0, 0.0, 0.0           # the truth of the first pd coordinates
    truth = orf.di_clearance_truth(Xp, Up, sig, c, r + rr, M=2000)
    bound = sr.di_chord_bound(Up, sig, K, S)
    clear = out["clear"].cpu().numpy()
    print(f"pos_dim={pd}: clearance vs truth: {np.abs(clear - truth).max():.2e} (bound {bound:.2e}), min {out['min']:.4f}")
    assert clear.shape == (N, K - 1, 19) and out["tau"].shape == (N, K - 1, 19)
    assert (truth >= clear - bound - 1e-12).all()                                # within the chord bound below it
    assert (truth <= clear + bound + sr.di_chord_bound(Up, sig, K, 2000) + 1e-12).all()
    D = out["D"].cpu().numpy()
    # (nodes 0..K-2 are samples; the random fleet's node K-1 is not where its last segment's roll-out ends)
    node = sr.obstacle_min_distance(Xp[:, :-1], c, r, rr)
    assert D.shape == (N, 19) and (D <= node + 1e-12).all() and (D < node - 1e-3).any()
    assert np.array_equal(D, clear.min(1)) and np.array_equal(out["agent_min"].cpu().numpy(), D.min(1))
    i, o, k, tau = out["argmin"]
    assert out["min"] == clear.min() == clear[i, k, o] and tau == float(out["tau"][i, k, o].item()) and 0 <= tau <= 1


def test_analysis_wrapper_returns_the_matrix(cuda):
    """SCvx.utils.analysis.min_agent_obstacle_clearance_continuous: (d_min_global, d_mat (N, M)) of the reference's
    signature style, equal to fleet_obstacle_clearance."""
    import scvx_hip
    from SCvx.utils import analysis
    X, U, sig = sr.random_fleet("di", 6, K, SEED)
    obs = obstacles(3, 5)
    d_min, d_mat = analysis.min_agent_obstacle_clearance_continuous([x.T for x in X], [u.T for u in U], "di", sig, obs,
                                                                    0.3, S=8)
    out = scvx_hip.fleet_obstacle_clearance("di", _t(X), _t(U), _t(sig), obs, robot_radius=0.3, S=8)
    assert d_mat.shape == (6, 5) and np.array_equal(d_mat, out["D"].cpu().numpy()) and d_min == d_mat.min() == out["min"]


# ------------------------------------------------------------------ the driver
@functools.lru_cache(maxsize=None)
def _fixture(on):
    marks = []
    return orf.run_fixture(_t, None, on, far=True, marks=marks) + (marks,)


def test_fixture_bites_without_the_rows(cuda):
    """The fixture of tests/test_obstacle_rows_cpu.py plus a second agent 100 away in z, on the kernels, 10
    iterations: node rows only, the nodes clear the obstacle and the curve passes deep inside it."""
    X, U, sig, out, drv, marks = _fixture(False)
    cont, node, bound, st, slack = orf.fixture_figures(X, U, sig, out)
    print(f"off: continuous clearance {cont:.4f}, node clearance {node:.4f}, status {st}, slack {slack:.1e}")
    assert cont <= -0.6
    assert node > 0 and st == 0
    assert "obsrows" not in [m for m, _ in marks]


def test_fixture_clears_the_obstacle_in_continuous_time_with_the_rows(cuda):
    X, U, sig, out, drv, marks = _fixture(True)
    cont, node, bound, st, slack = orf.fixture_figures(X, U, sig, out)
    print(f"on: continuous clearance {cont:.6f} (bound {bound:.2e}), node clearance {node:.6f}, status {st}, "
          f"slack {slack:.1e}")
    assert abs(cont) <= bound
    assert st == 0
    assert slack < 1e-12
    assert [m for m, _ in marks].count("obsrows") == orf.FIXTURE["iters"]
    assert int(drv._ob["overflow"].item()) == 0
    # JacobiSCvx.obstacle_clearance sees the same curve
    oc = drv.obstacle_clearance(_t(X), _t(U), S=orf.FIXTURE["S"])
    assert abs(oc["D"][0, 0].item() - cont) <= bound and oc["D"][1, 0].item() > 90.0


def test_the_far_agent_is_untouched(cuda):
    """No obstacle within the far agent's reach: its X and U are bit-identical to the run with the option off at the
    same QPSpec.j_max (the fixture agent's are not)."""
    Xoff, Uoff = _fixture(False)[:2]
    Xon, Uon = _fixture(True)[:2]
    assert np.array_equal(Xon[1], Xoff[1]) and np.array_equal(Uon[1], Uoff[1])
    assert not np.array_equal(Xon[0], Xoff[0])


def test_nothing_in_reach_changes_nothing(cuda):
    """Every obstacle of the option's list beyond cull: three steps are bit-identical to the option off."""
    on = orf.run_fixture(_t, None, True, far=True, obstacles=[((50.0, 50.0, 50.0), 0.7)], iters=3)
    off = orf.run_fixture(_t, None, False, far=True, iters=3)
    assert int(on[4]._ob["count_seg"].sum()) == 0 and int(on[4].count.max()) == 0
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert not np.array_equal(on[0], orf.fixture(far=True)[0])


def test_a_coupled_step_with_both_record_kinds(cuda):
    """CouplingSpec with check=True, pair records and obstacle records in one node's rows: node row, pair records,
    obstacle records; the dense samples are shared (equal S); no overflow."""
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx, ObstacleRowsSpec
    X0, U0, sig = ir.head_on()
    obs = [((-0.9, 0.9, 0.0), 0.5)]
    spec = scvx_hip.QPSpec(model="di", K=8, box=[(0, -20.0, 20.0)], obs=obs, j_max=8, w_coll=1e4, tol=1e-10, max_iter=80)
    drv = JacobiSCvx(spec, _t(X0[:, 0]), _t(X0[:, -1]), _t(sig), 4.0, tr_rule="global",
                     coupling=CouplingSpec(R=1.0, check=True, intersample_S=8, intersample_J=1),
                     obstacle_rows=ObstacleRowsSpec(S=8, J=1, cull=1.0))
    X, U = _t(X0), _t(U0)
    marks = []
    for _ in range(2):   # (the warm start is at rest at every node: its roll-out does not move, the first step has no record)
        Xp = X
        X, U, out = drv.step(X, U, marks=marks)
        X, U = X.clone(), U.clone()
    assert [m for m, _ in marks][:6] == ["start", "foh", "gather", "rows", "isrows", "obsrows"]
    assert int(out["status"].max()) == 0
    assert drv.last_check["is_overflow"] == 0 and drv.last_check["obs_overflow"] == 0
    assert getattr(drv.backend, "samples", None) is None                         # handed on and cleared
    cs_p, cs_o = drv._is["count_seg"].cpu().numpy(), drv._ob["count_seg"].cpu().numpy()
    assert cs_p.sum() > 0 and cs_o.sum() > 0
    want = 1 + cs_p + cs_o
    want[:, 1:] += (cs_p + cs_o)[:, :-1]
    assert np.array_equal(drv.count.cpu().numpy()[:, :7], want)
    rec =drv._ob["rec"].cpu().numpy()
    a, k = np.argwhere(cs_o > 0)[0]
    row = drv.rows.cpu().numpy()[a, k, 1 + cs_p[a, k]]                             # node k: segment k's records first
    p = Xp.cpu().numpy()[a, k, :3]
    assert np.array_equal(row[:3], rec[a, k, 0, :3]) and abs(row[3] - rec[a, k, 0, 3] - row[:3] @ p) < 1e-13
