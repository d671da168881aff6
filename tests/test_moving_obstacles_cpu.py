"""Moving obstacles without a device: the numpy restatement's own properties (tests/moving_obstacles_ref.py), the
exported symbols and the C-ABI's argument rejection, the driver's option checks, and the fixtures of DESIGN §3.9 end
to end through scvx_hip.scvx.JacobiSCvx with the CPU restatements (oracle/) behind the backend hooks."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import moving_obstacles_ref as mo
import obstacle_rows_ref as orf
import separation_ref as sr
from test_obstacle_rows_cpu import CpuBackend as _StaticCpuBackend

CULL, S, J, K, N = 4.5, 4, 2, 5, 24


class CpuBackend(_StaticCpuBackend):
    """The static tests' CPU backend plus the two moving-obstacle hooks on the numpy restatement."""

    def moving_obstacle_rows(self, model, X, U, sigma, S, nsub, pos_dim, tracks, cull, J):
        out = mo.cpu_moving_obstacle_rows(model, X.numpy(), U.numpy(), sigma.numpy(), S, nsub, pos_dim, tracks, cull, J)
        return tuple(torch.from_numpy(o) for o in out)

    def append_node_rows(self, X_all, i0, idx, node_rec, node_count, rows, count, pos_dim, overflow):
        r, c, over = mo.append_node_rows(X_all.numpy(), i0, None if idx is None else idx.numpy(), node_rec.numpy(),
                                         node_count.numpy(), rows.numpy(), count.numpy(), pos_dim)
        rows.copy_(torch.from_numpy(r))
        count.copy_(torch.from_numpy(c))
        overflow += over
        return rows, count, overflow


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _fleet():
    X, U, sig = sr.random_fleet("di", N, K, 3)
    P, _ = sr.dense_closed_form("di", X, U, sig, S)
    trk = mo.pad_tracks(mo.random_tracks(19, box=9.0))
    return X, sig, P, trk, mo.segment_records(P, sig, trk, CULL, J), mo.node_records(P, sig, trk, CULL, J)


def test_track_evaluation():
    kn = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 4.0, 0.0]])
    q = mo.track_eval(kn, 3, (1.0, 3.0), np.array([-1.0, 1.0, 1.5, 2.0, 2.5, 3.0, 9.0]))
    assert np.allclose(q[:, 0], [0, 0, 1, 2, 2, 2, 2]) and np.allclose(q[:, 1], [0, 0, 0, 0, 2, 4, 4])   # waits, stops
    assert np.array_equal(mo.track_eval(kn, 1, (0.0, 1.0), np.array([0.3, 7.0])), np.zeros((2, 3)))      # one knot
    t = mo.clock(np.array([2.0, 3.0]), 5, 4)
    assert t.shape == (2, 4, 5) and t[0, 0, 0] == 0 and abs(t[1, 3, 4] - 3.0) < 1e-15 and abs(t[0, 2, 1] - 2 * 9 / 16) < 1e-15
    assert np.array_equal(t[:, :-1, -1], t[:, 1:, 0])                                  # a node's two samples agree


def test_records_are_sorted_unit_and_strictly_between_the_nodes():
    X, sig, P, trk, (rec, obs, alpha, count, sel), (nrec, nobs, ncount) = _fleet()
    rho = trk[3]
    Q, Sx, A, C = mo.minima(P, sig, trk)
    V = orf.values(Q, rho)
    cand = orf.candidates(Q, Sx, A, S, rho, CULL)
    d0, NV = mo.node_values(P, sig, trk)
    ncand = mo.node_candidates(d0, NV, CULL)
    for c, cd in ((count, cand), (ncount, ncand)):                                  # the cases are covered
        assert (c == J).any() and ((c > 0) & (c < J)).any() and (c == 0).any() and (cd.sum(0) > J).any()
        assert np.array_equal(c, np.minimum(cd.sum(0), J))
    assert (rec[..., 3] > 0).any() and (nrec[..., 3] > 0).any()                     # penetrations
    dist, al = mo.scan(P, sig, trk)
    for a in range(N):
        for k in range(K - 1):
            for r_, o_, n, vals, cd in ((rec, obs, count[a, k], V, cand), (nrec, nobs, ncount[a, k], NV, ncand)):
                os_, v = o_[a, k, :n], r_[a, k, :n, 3]
                assert (os_ >= 0).all() and len(set(os_.tolist())) == n and (v > -CULL).all()
                assert all((-v[r], os_[r]) < (-v[r + 1], os_[r + 1]) for r in range(n - 1))   # descending v, then o
                assert np.abs(np.linalg.norm(r_[a, k, :n, :3], axis=1) - 1.0).max(initial=0.0) <= 1e-15
                rest = np.setdiff1d(np.nonzero(cd[:, a, k])[0], os_)                 # nothing nearer was left out
                assert n == 0 or rest.size == 0 or vals[rest, a, k].max() <= v.min()
                assert (o_[a, k, n:] == -1).all() and not r_[a, k, n:].any()
            n = count[a, k]
            assert ((alpha[a, k, :n] > 0) & (alpha[a, k, :n] < 1)).all() and not alpha[a, k, n:].any()
            for r in range(n):                                                      # v = rho - dist of the scan
                o = obs[a, k, r]
                assert rec[a, k, r, 3] == rho[o] - dist[a, k, o] and alpha[a, k, r] == al[a, k, o]
            for r in range(ncount[a, k]):                                           # the node record is sample 0's
                o = nobs[a, k, r]
                assert np.abs(nrec[a, k, r, :3] * (rho[o] - nrec[a, k, r, 3]) - d0[o, a, k]).max() <= 1e-14 * 16


def test_the_scan_is_the_minimum_over_the_relative_polyline():
    """dist is the distance from the origin to the polyline of the relative samples p_s - q_o(t_s): no point of a fine
    subdivision of its chords is nearer."""
    X, sig, P, trk, _, _ = _fleet()
    dist, al = mo.scan(P, sig, trk)
    D = mo.relative(P, sig, trk)
    t = np.linspace(0, 1, 65)[None, None, None, None, :, None]
    pts = (D[:, :, :, :-1, None, :] * (1 - t) + D[:, :, :, 1:, None, :] * t).reshape(len(trk[1]), N, K - 1, -1, 3)
    fine = np.moveaxis(np.sqrt((pts ** 2).sum(-1)).min(-1), 0, -1)
    assert (dist <= fine + 1e-13).all() and (fine - dist).max() < 1e-2
    assert ((al >= 0) & (al <= 1)).all()


def test_one_knot_tracks_are_the_static_restatement():
    X, sig, P, _, _, _ = _fleet()
    c, rho = np.random.default_rng(11).uniform(-6.0, 6.0, (19, 3)), np.random.default_rng(12).uniform(0.5, 1.5, 19)
    trk = mo.pad_tracks([(c[o], None, rho[o]) for o in range(19)])
    for got, want in zip(mo.segment_records(P, sig, trk, CULL, J), orf.obstacle_rows(P, c, rho, CULL, J)):
        assert np.array_equal(got, want)
    for got, want in zip(mo.scan(P, sig, trk), orf.scan(P, c)):
        assert np.array_equal(got, want)


def test_exports_and_bad_arguments_are_rejected_without_a_device():
    from scvx_hip import _lib
    L = _lib.lib()
    for name in ("scvx_moving_obstacle_scan_batched", "scvx_node_rows_append_batched"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert _lib.SCVX_HIP_VERSION == 7 == L.scvx_version()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(K=5, S=8, N=4, P=p, sig=p, O=3, M=2, kn=p, nk=p, win=p, rho=p, cull=1.0, J=2, dist=p, alpha=p, rec=p,
                obs=p, ra=p, count=p, nrec=p, nobs=p, ncount=p)

    def call(**kw):
        a = dict(good, **kw)
        return L.scvx_moving_obstacle_scan_batched(*[a[k] for k in good], None)

    none4 = dict(rec=None, obs=None, ra=None, count=None)
    none3 = dict(nrec=None, nobs=None, ncount=None)
    for kw in (dict(K=1), dict(S=0), dict(S=17), dict(O=0), dict(M=0), dict(J=-1), dict(J=9), dict(cull=0.0),
               dict(cull=-1.0), dict(K=65), dict(N=-1), dict(P=None), dict(sig=None), dict(kn=None), dict(nk=None),
               dict(win=None), dict(rho=None),
               dict(dist=None), dict(alpha=None),                                  # half an analysis group
               dict(rec=None), dict(obs=None), dict(ra=None), dict(count=None),    # part of a record group
               dict(nrec=None), dict(nobs=None), dict(ncount=None),                # part of the node group
               dict(J=0),                                                          # records given, none asked for
               dict(J=0, **none4), dict(J=0, **none3),
               dict(J=2, **none4, **none3),                                        # records asked for, none given
               dict(J=0, dist=None, alpha=None, **none4, **none3)):                # nothing asked for
        assert call(**kw) == -1 and b"bad args" in L.scvx_last_error(), kw
    assert call(N=0) == 0                                                           # nothing to do: no launch
    assert call(N=0, **none4) == 0 and call(N=0, **none3) == 0                      # each record group alone
    assert call(N=0, J=0, **none4, **none3) == 0 and call(N=0, K=65, J=0, **none4, **none3) == 0
    assert call(N=0, dist=None, alpha=None) == 0

    g2 = dict(K=5, pd=3, nx=6, Nt=4, X=p, i0=0, idx=None, Nl=4, J=2, rec=p, cnt=p, j_max=4, rows=p, count=p, over=p)

    def call2(**kw):
        a = dict(g2, **kw)
        return L.scvx_node_rows_append_batched(*[a[k] for k in g2], None)

    for kw in (dict(K=1), dict(K=65), dict(pd=0), dict(pd=4), dict(pd=3, nx=2), dict(Nt=-1), dict(Nl=-1), dict(i0=-1),
               dict(i0=5), dict(i0=1), dict(J=0), dict(J=9), dict(j_max=0), dict(j_max=33), dict(X=None),
               dict(rec=None), dict(cnt=None), dict(rows=None), dict(count=None), dict(over=None)):
        assert call2(**kw) == -1 and b"bad args" in L.scvx_last_error(), kw
    assert call2(Nl=0) == 0


def test_obstacle_tracks_helper_and_wrapper_checks():
    import scvx_hip
    tr = scvx_hip.obstacle_tracks([((1.0, 2.0), None, 0.4), ([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0]], (0.5, 2.5), 1.2)], "cpu")
    kn, n, win, rho = tr
    assert kn.shape == (2, 2, 3) and n.tolist() == [1, 2] and n.dtype == torch.int32 and rho.tolist() == [0.4, 1.2]
    assert kn[0].tolist() == [[1.0, 2.0, 0.0], [0.0, 0.0, 0.0]] and win[1].tolist() == [0.5, 2.5]
    assert scvx_hip.obstacle_tracks(tr, "cpu") is tr                               # passes through
    two = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    for bad in ([], [(two, (1.0, 1.0), 0.5)], [(two, (2.0, 1.0), 0.5)], [(two, (0.0, float("nan")), 0.5)],
                [(np.zeros((2, 4)), (0.0, 1.0), 0.5)], [(np.zeros((0, 3)), (0.0, 1.0), 0.5)]):
        with pytest.raises(ValueError):
            scvx_hip.obstacle_tracks(bad, "cpu")
    P, sig = torch.zeros((2, 4, 9, 3), dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    for kw in (dict(J=9), dict(J=-1), dict(J=1, cull=0.0), dict(J=0, analysis=False)):
        with pytest.raises(ValueError):
            scvx_hip.moving_obstacle_scan(P, sig, tr, **kw)
    for args in ((P[..., :2], sig, tr), (torch.zeros((2, 4, 18, 3), dtype=torch.float64), sig, tr), (P, sig[:1], tr),
                 (P, sig, []), (P, sig, [(two, (1.0, 0.0), 0.5)])):
        with pytest.raises(ValueError):
            scvx_hip.moving_obstacle_scan(*args)
    with pytest.raises(ValueError):                                                # records need K <= 64
        scvx_hip.moving_obstacle_scan(torch.zeros((1, 64, 9, 3), dtype=torch.float64), sig[:1], tr, J=1)


def test_driver_option_checks():
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx, MovingObstaclesSpec, ObstacleRowsSpec
    X, U, sig = orf.fixture(far=True)
    obs = orf.FIXTURE["obs"]
    tracks = mo.TRACKS_A

    def mk(j_max, coupling=None, orows=None, tracks=tracks, K=8, **kw):
        return JacobiSCvx(scvx_hip.QPSpec(model="di", K=K, j_max=j_max, obs=obs), _T(X[:, 0]), _T(X[:, -1]), _T(sig), 4.0,
                          coupling=coupling, backend=CpuBackend(), obstacle_rows=orows,
                          moving_obstacles=MovingObstaclesSpec(tracks, **kw) if tracks is not None else None)

    d = MovingObstaclesSpec(tracks)
    assert (d.S, d.J, d.cull) == (8, 2, 0.0)
    assert mk(0, tracks=None)._mv is None
    on = mk(6)                                                                      # without coupling: 6 - 3 x 2 = 0
    assert on._mv["j_node"] == 0 and on._mv["cull"] == 0.7 and on._mv["per_node"] == 6
    assert on.rows.shape == (2, 8, 6, 4) and on.count.shape == (2, 8) and on.coupling is None
    assert mk(6, cull=2.5)._mv["cull"] == 2.5
    with pytest.raises(ValueError, match="capacity"):
        mk(5)                                                                       # 5 < 3 x 2
    with pytest.raises(ValueError, match="capacity"):
        mk(6, CouplingSpec(R=1.0))                                                  # coupling wants a node row too
    c = mk(7, CouplingSpec(R=1.0))
    assert c._mv["j_node"] == 1 and c._mv["rows_node"].shape == (2, 8, 1, 4)
    ob = mk(8, orows=ObstacleRowsSpec(S=8, J=1), J=2)                               # 8 - 2 - 6 = 0, no coupling
    assert ob._ob["j_node"] == ob._mv["j_node"] == 0 and [s["per_node"] for s in ob._records()] == [2, 6]
    with pytest.raises(ValueError, match="capacity"):
        mk(7, orows=ObstacleRowsSpec(S=8, J=1), J=2)
    al = mk(8, CouplingSpec(R=1.0, intersample_S=8, intersample_J=1), ObstacleRowsSpec(S=8, J=1), J=1)
    assert al._is["j_node"] == al._ob["j_node"] == al._mv["j_node"] == 1 and al._is["rows_node"].shape == (2, 8, 1, 4)
    assert [s["per_node"] for s in al._records()] == [2, 2, 3]
    with pytest.raises(ValueError, match="capacity"):
        mk(7, CouplingSpec(R=1.0, intersample_S=8, intersample_J=1), ObstacleRowsSpec(S=8, J=1), J=1)
    co = mk(8, CouplingSpec(R=1.0), ObstacleRowsSpec(S=8, J=1), J=1)
    assert co._ob["rows_node"].shape == (2, 8, 3, 4) and "rows_node" not in co._mv
    for kw in (dict(S=17), dict(S=0), dict(J=9), dict(J=0)):
        with pytest.raises(ValueError):
            mk(32, **kw)
    with pytest.raises(ValueError, match="no tracks"):
        mk(8, tracks=[])
    with pytest.raises(ValueError, match="t1 > t0"):
        mk(8, tracks=[(tracks[0][0], (2.0, 2.0), 0.7)])
    with pytest.raises(ValueError, match="K <= 64"):
        JacobiSCvx(scvx_hip.QPSpec(model="di", K=65, j_max=8), _T(X[:, 0]), _T(X[:, -1]), _T(sig), 4.0,
                   backend=CpuBackend(), moving_obstacles=MovingObstaclesSpec(tracks))

    class UserModel:   # a runtime-compiled model without a dense roll-out
        dims, nsub = (6, 3), 4

    with pytest.raises(NotImplementedError, match="built-in"):
        JacobiSCvx(scvx_hip.QPSpec(model=UserModel(), K=8, j_max=8), _T(X[:, 0]), _T(X[:, -1]), _T(sig), 4.0,
                   backend=CpuBackend(), moving_obstacles=MovingObstaclesSpec(tracks))
    import unittest.mock as um
    with um.patch("torch.distributed.is_initialized", return_value=True), \
            um.patch("torch.distributed.get_world_size", return_value=2), \
            um.patch("torch.distributed.get_rank", return_value=1):
        assert mk(6).world == 2                                                     # local: any world size


def test_append_node_rows_restatement():
    X, sig, P, trk, _, (nrec, nobs, ncount) = _fleet()
    rows0, count0 = np.zeros((N, K, 3, 4)), np.zeros((N, K), np.int32)
    count0[::2, :-1] = 2                                                            # every other agent has one slot left
    rows, count, over = mo.append_node_rows(X, 0, None, nrec, ncount, rows0, count0, 3)
    assert np.array_equal(count[:, :-1], np.minimum(count0[:, :-1] + ncount, 3)) and not count[:, -1].any()
    assert over == int((count0[:, :-1] + ncount - count[:, :-1]).sum()) and over > 0
    a, k = np.argwhere((ncount == J) & (count0[:, :-1] == 0))[0]
    for r in range(J):
        assert np.array_equal(rows[a, k, r, :3], nrec[a, k, r, :3])
        assert abs(rows[a, k, r, 3] - nrec[a, k, r, 3] - nrec[a, k, r, :3] @ X[a, k, :3]) < 1e-13
    idx = np.array([5, 2, 9])                                                       # the re-solve's form
    r2, c2, _ = mo.append_node_rows(X, 0, idx, nrec, ncount, rows0[:3], count0[1:4] * 0, 3)
    assert np.array_equal(c2[:, :-1], ncount[idx]) and np.array_equal(r2[0, :, 0], mo.append_node_rows(
        X, 0, None, nrec, ncount, rows0, count0 * 0, 3)[0][5, :, 0])


# ------------------------------------------------------------------ the fixtures
@functools.lru_cache(maxsize=None)
def _fixture_a(on):
    return mo.run_fixture(_T, CpuBackend(), on, mo.TRACKS_A)


@functools.lru_cache(maxsize=None)
def _fixture_b(on):
    return mo.run_fixture(_T, CpuBackend(), on, mo.tracks_b(_fixture_a(False)[0]))


def test_fixture_a_bites_without_the_rows():
    """No rows: every node ends clear of the intruder and the curve passes deep inside it between two nodes."""
    X, U, sig, out, drv = _fixture_a(False)
    cont, node, bound, st, slack = mo.fixture_figures(X, U, sig, out, mo.TRACKS_A)
    print(f"A off: continuous clearance {cont:.4f}, node clearance {node.min():.4f}, status {st}, slack {slack:.1e}")
    assert cont <= -0.5
    assert node.min() > 0 and st == 0


def test_fixture_a_clears_the_intruder_in_continuous_time_with_the_rows():
    X, U, sig, out, drv = _fixture_a(True)
    cont, node, bound, st, slack = mo.fixture_figures(X, U, sig, out, mo.TRACKS_A)
    print(f"A on: continuous clearance {cont:.6f} (bound {bound:.2e}), node clearance {node.min():.6f}, status {st}, "
          f"slack {slack:.1e}")
    assert cont >= -bound
    assert st == 0
    assert slack < 1e-12
    assert mo.mov_overflow(drv) == 0


def test_fixture_b_sits_on_the_node_without_the_rows():
    X, U, sig, out, drv = _fixture_b(False)
    tracks = mo.tracks_b(_fixture_a(False)[0])
    cont, node, bound, st, slack = mo.fixture_figures(X, U, sig, out, tracks)
    print(f"B off: node {mo.NODE_B} clearance {node[mo.NODE_B]:.6f}, continuous clearance {cont:.4f}")
    assert abs(node[mo.NODE_B] + mo.RHO) <= 1e-12 and st == 0


def test_fixture_b_clears_the_node_with_the_rows():
    X, U, sig, out, drv = _fixture_b(True)
    tracks = mo.tracks_b(_fixture_a(False)[0])
    cont, node, bound, st, slack = mo.fixture_figures(X, U, sig, out, tracks)
    print(f"B on: node clearance {node.min():.2e}, continuous clearance {cont:.6f} (bound {bound:.2e}), status {st}, "
          f"slack {slack:.1e}")
    assert node.min() >= -slack - 1e-9
    assert cont >= -bound
    assert st == 0
    assert mo.mov_overflow(drv) == 0


def test_a_coupled_step_appends_all_five_kinds_in_order():
    drv, Xp, out = mo.coupled_step(_T, CpuBackend())
    assert int(out["status"].max()) == 0
    assert drv.last_check["is_overflow"] == drv.last_check["obs_overflow"] == drv.last_check["mov_overflow"] == 0
    mo.check_coupled_rows(drv, Xp)
