"""Continuous-time obstacle rows without a device: the numpy restatement's own properties
(tests/obstacle_rows_ref.py), the C-ABI's argument rejection, the driver's option checks, and the fixture of
DESIGN §3.8 end to end through scvx_hip.scvx.JacobiSCvx with the CPU restatements (oracle/) behind the backend
hooks."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import intersample_rows_ref as ir
import obstacle_rows_ref as orf
import separation_ref as sr
from oracle import qp_cpu
from test_distributed_cpu import OracleBackend, _CpuQP

CULL, S, J, K, N, O = 4.5, 4, 2, 5, 24, 19


class _CpuObsQP(_CpuQP):
    """The CPU twin with the template's obstacles (the parent's template leaves them out)."""

    def __init__(self, spec):
        self.tpl = qp_cpu.make_template(6, 3, spec.K, box=spec.box, obs=spec.obs, w_obs=spec.w_obs, j_max=spec.j_max,
                                        w_coll=spec.w_coll, tol=spec.tol, max_iter=spec.max_iter)


class CpuBackend(OracleBackend):
    """OracleBackend with obstacles in the QP, plus the hooks of both kinds of continuous-time rows on the numpy
    restatements."""

    def qp_solver(self, spec, N, device):
        return _CpuObsQP(spec)

    def intersample_pair_rows(self, model, X, U, sigma, S, nsub, pos_dim, R, cull, J):
        rec, count = ir.cpu_intersample_pair_rows(model, X.numpy(), U.numpy(), sigma.numpy(), S, nsub, pos_dim, R,
                                                  cull, J)
        return torch.from_numpy(rec), torch.from_numpy(count)

    def obstacle_rows(self, model, X, U, sigma, S, nsub, pos_dim, obstacles, cull, J):
        rec, count = orf.cpu_obstacle_rows(model, X.numpy(), U.numpy(), sigma.numpy(), S, nsub, pos_dim, obstacles,
                                           cull, J)
        return torch.from_numpy(rec), torch.from_numpy(count)

    def append_collision_rows(self, X_all, i0, idx, rec, count_seg, rows, count, pos_dim, overflow):
        r, c, over = ir.append_rows(X_all.numpy(), i0, None if idx is None else idx.numpy(), rec.numpy(),
                                    count_seg.numpy(), rows.numpy(), count.numpy(), pos_dim)
        rows.copy_(torch.from_numpy(r))
        count.copy_(torch.from_numpy(c))
        overflow += over
        return rows, count, overflow


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def random_obstacles(n, seed=11):
    rng = np.random.default_rng(seed)
    return rng.uniform(-6.0, 6.0, (n, 3)), rng.uniform(0.5, 1.5, n)


@functools.lru_cache(maxsize=None)
def _fleet():
    X, U, sig = sr.random_fleet("di", N, K, 3)
    P, _ = sr.dense_closed_form("di", X, U, sig, S)
    c, rho = random_obstacles(O)
    return X, P, c, rho, orf.obstacle_rows(P, c, rho, CULL, J)


def test_records_are_sorted_unit_and_strictly_between_the_nodes():
    X, P, c, rho, (rec, obs, alpha, count, sel) = _fleet()
    Q, Sx, A, C = orf.obstacle_minima(P, c)
    V = orf.values(Q, rho)
    cand = orf.candidates(Q, Sx, A, S, rho, CULL)
    assert (count == J).any() and ((count > 0) & (count < J)).any() and (count == 0).any()   # the cases are covered
    assert (cand.sum(0) > J).any() and (rec[..., 3] > 0).any()                  # lists that overflow; penetrations
    assert np.array_equal(count, np.minimum(cand.sum(0), J))
    dist, al = orf.scan(P, c)
    for a in range(N):
        for k in range(K - 1):
            n = count[a, k]
            os_ = obs[a, k, :n]
            v = rec[a, k, :n, 3]
            assert (os_ >= 0).all() and len(set(os_.tolist())) == n
            assert all((-v[r], os_[r]) < (-v[r + 1], os_[r + 1]) for r in range(n - 1))   # descending v, then o
            assert ((alpha[a, k, :n] > 0) & (alpha[a, k, :n] < 1)).all() and (v > -CULL).all()
            assert np.abs(np.linalg.norm(rec[a, k, :n, :3], axis=1) - 1.0).max(initial=0.0) <= 1e-15
            rest = np.setdiff1d(np.nonzero(cand[:, a, k])[0], os_)                   # nothing nearer was left out
            assert n == 0 or rest.size == 0 or V[rest, a, k].max() <= v.min()
            assert (obs[a, k, n:] == -1).all() and not rec[a, k, n:].any() and not alpha[a, k, n:].any()
            for r in range(n):                                                      # v = rho - dist of the scan
                assert v[r] == rho[os_[r]] - dist[a, k, os_[r]] and alpha[a, k, r] == al[a, k, os_[r]]
                # g points from the centre to the closest point of the selected chord
                s = sel[a, k, r]
                t = alpha[a, k, r] * S - s
                p = P[a, k, s] + t * (P[a, k, s + 1] - P[a, k, s])
                assert np.abs(c[os_[r]] + rec[a, k, r, :3] * dist[a, k, os_[r]] - p).max() <= 1e-13 * 8


def test_the_scan_is_the_minimum_over_the_polyline():
    """dist is the distance from the centre to the polyline of the samples: no point of a fine subdivision of the
    chords is nearer, and the reported point attains it."""
    X, P, c, rho, _ = _fleet()
    dist, al = orf.scan(P, c)
    t = np.linspace(0, 1, 65)[None, None, None, :, None]
    pts = (P[:, :, :-1, None, :] * (1 - t) + P[:, :, 1:, None, :] * t).reshape(N, K - 1, -1, 3)
    fine = np.sqrt(((pts[:, :, :, None, :] - c[None, None, None]) ** 2).sum(-1)).min(2)
    assert (dist <= fine + 1e-13).all() and (fine - dist).max() < 1e-2
    assert ((al >= 0) & (al <= 1)).all()


def test_two_appended_rows_imply_the_chord_row():
    """Rows g.dp_t >= v at both nodes of a segment give g.((1 - a') dp_k + a' dp_{k+1}) >= v: the first-order image
    of the closest point clears rho.  Random displacements that satisfy both rows, with and without slack to spare."""
    _, _, _, _, (rec, obs, alpha, count, _) = _fleet()
    rng = np.random.default_rng(0)
    seen = 0
    for a, k in zip(*np.nonzero(count)):
        for r in range(count[a, k]):
            g, v, al = rec[a, k, r, :3], rec[a, k, r, 3], alpha[a, k, r]
            for _ in range(8):
                dp = rng.normal(size=(2, 3))
                dp += ((v - dp @ g) + rng.choice([0.0, 1.0]) * rng.uniform(0, 1, 2))[:, None] * g[None, :]
                assert (dp @ g >= v - 1e-14).all()
                assert g @ ((1 - al) * dp[0] + al * dp[1]) >= v - 1e-14
                seen += 1
    assert seen > 100


def test_bad_arguments_are_rejected_without_a_device():
    from scvx_hip import _lib
    L = _lib.lib()
    assert "scvx_obstacle_scan_batched" in _lib.EXPORTS and hasattr(L, "scvx_obstacle_scan_batched")
    assert _lib.SCVX_HIP_VERSION == 7 == L.scvx_version()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = L.scvx_obstacle_scan_batched
    good = dict(K=5, S=8, N=4, P=p, O=3, c=p, rho=p, cull=1.0, J=2, dist=p, alpha=p, rec=p, obs=p, ra=p, count=p)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["K"], a["S"], a["N"], a["P"], a["O"], a["c"], a["rho"], a["cull"], a["J"], a["dist"], a["alpha"],
                  a["rec"], a["obs"], a["ra"], a["count"], None)

    none4 = dict(rec=None, obs=None, ra=None, count=None)
    for kw in (dict(K=1), dict(S=0), dict(S=17), dict(O=0), dict(J=-1), dict(J=9), dict(cull=0.0), dict(cull=-1.0),
               dict(K=65), dict(N=-1), dict(P=None), dict(c=None), dict(rho=None),
               dict(dist=None), dict(alpha=None),                                  # half an analysis group
               dict(rec=None), dict(obs=None), dict(ra=None), dict(count=None),    # part of a record group
               dict(J=0),                                                          # records given, none asked for
               dict(J=2, **none4),                                                 # records asked for, none given
               dict(J=0, dist=None, alpha=None, **none4)):                         # nothing asked for
        assert call(**kw) == -1 and b"bad args" in L.scvx_last_error(), kw
    assert call(N=0) == 0                                                           # nothing to do: no launch
    assert call(N=0, J=0, **none4) == 0 and call(N=0, K=65, J=0, **none4) == 0      # K <= 64 binds the records only
    assert call(N=0, dist=None, alpha=None) == 0


def test_driver_option_checks():
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx, ObstacleRowsSpec
    X, U, sig = orf.fixture(far=True)
    obs = orf.FIXTURE["obs"]

    def mk(j_max, coupling=None, obs=obs, **kw):
        return JacobiSCvx(scvx_hip.QPSpec(model="di", K=8, j_max=j_max, obs=obs), _T(X[:, 0]), _T(X[:, -1]), _T(sig), 4.0,
                          coupling=coupling, backend=CpuBackend(), obstacle_rows=ObstacleRowsSpec(**kw) if kw else None)

    d = ObstacleRowsSpec()
    assert (d.S, d.J, d.cull, d.obstacles) == (8, 2, 0.0, None)
    assert mk(0)._ob is None and mk(8, CouplingSpec(R=1.0))._ob is None
    on = mk(4, S=8)                                                                 # without coupling: 4 - 2 x 2 = 0
    assert on._ob["j_node"] == 0 and on._ob["cull"] == 0.7 and on._ob["obstacles"] == list(obs)
    assert on.rows.shape == (2, 8, 4, 4) and on.count.shape == (2, 8) and on.coupling is None
    two = [((1.0, 2.0), 0.4), ((0.0, 0.0, 1.0), 1.2)]
    assert mk(4, S=8, obstacles=two)._ob["cull"] == 1.2 and mk(4, S=8, cull=2.5)._ob["cull"] == 2.5
    with pytest.raises(ValueError, match="capacity"):
        mk(3, S=8)                                                                  # 3 < 2 x 2
    with pytest.raises(ValueError, match="capacity"):
        mk(4, CouplingSpec(R=1.0), S=8)                                             # coupling wants a node row too
    c = mk(5, CouplingSpec(R=1.0), S=8)
    assert c._ob["j_node"] == 1 and c._ob["rows_node"].shape == (2, 8, 1, 4)
    both = mk(8, CouplingSpec(R=1.0, intersample_S=8, intersample_J=1), S=8)
    assert both._ob["j_node"] == both._is["j_node"] == 2 and both._is["rows_node"].shape == (2, 8, 2, 4)
    with pytest.raises(ValueError, match="capacity"):
        mk(8, CouplingSpec(R=1.0, intersample_S=8, intersample_J=2), S=8)           # 8 - 4 - 4 leaves no node row
    with pytest.raises(ValueError):
        mk(8, S=17)
    with pytest.raises(ValueError):
        mk(8, S=8, J=9)
    with pytest.raises(ValueError, match="no obstacles"):
        mk(8, obs=(), S=8)

    class UserModel:   # a runtime-compiled model: no dense roll-out
        dims, nsub = (6, 3), 4

    with pytest.raises(NotImplementedError, match="built-in"):
        JacobiSCvx(scvx_hip.QPSpec(model=UserModel(), K=8, j_max=4, obs=obs), _T(X[:, 0]), _T(X[:, -1]), _T(sig), 4.0,
                   backend=CpuBackend(), obstacle_rows=ObstacleRowsSpec())
    import unittest.mock as um
    with um.patch("torch.distributed.is_initialized", return_value=True), \
            um.patch("torch.distributed.get_world_size", return_value=2), \
            um.patch("torch.distributed.get_rank", return_value=1):
        assert mk(4, S=8).world == 2                                                # local: any world size


def test_a_coupled_step_appends_node_rows_then_pair_then_obstacle_records():
    """Two steps with a CouplingSpec, both record kinds and check=True on the twin: per node the node row of the one
    neighbour, then the pair records, then the obstacle records; no overflow."""
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx, ObstacleRowsSpec
    X0, U0, sig = ir.head_on()
    obs = [((-0.9, 0.9, 0.0), 0.5)]
    spec = scvx_hip.QPSpec(model="di", K=8, box=[(0, -20.0, 20.0)], obs=obs, j_max=8, w_coll=1e4, tol=1e-10, max_iter=80)
    drv = JacobiSCvx(spec, _T(X0[:, 0]), _T(X0[:, -1]), _T(sig), 4.0, tr_rule="global", backend=CpuBackend(),
                     coupling=CouplingSpec(R=1.0, check=True, intersample_S=8, intersample_J=1),
                     obstacle_rows=ObstacleRowsSpec(S=8, J=1, cull=1.0))
    X, U = _T(X0), _T(U0)
    for _ in range(2):   # (the warm start is at rest at every node: its roll-out does not move, the first step has no record)
        Xp, Up = X, U
        X, U, out = drv.step(X, U)
        X, U = X.clone(), U.clone()
    X0 = Xp.numpy()                                                                 # the last step's iterate
    assert int(out["status"].max()) == 0
    assert drv.last_check["is_overflow"] == 0 and drv.last_check["obs_overflow"] == 0
    cs_p, cs_o = drv._is["count_seg"].numpy(), drv._ob["count_seg"].numpy()
    assert cs_p.sum() > 0 and cs_o.sum() > 0
    want = np.zeros((2, 8), int)
    want[:, :7] = 1 + cs_p + cs_o
    want[:, 1:7] += (cs_p + cs_o)[:, :-1]
    assert np.array_equal(drv.count.numpy(), want)
    # the obstacle rows are the last ones of their node: g of the record, b = v + g . pbar
    rec = drv._ob["rec"].numpy()
    a, k = np.argwhere(cs_o > 0)[0]
    m = 1 + cs_p[a, k]                                                              # node k: segment k's records first
    row = drv.rows.numpy()[a, k, m]
    assert np.array_equal(row[:3], rec[a, k, 0, :3]) and abs(row[3] - rec[a, k, 0, 3] - row[:3] @ X0[a, k, :3]) < 1e-13


@functools.lru_cache(maxsize=None)
def _fixture(on):
    return orf.run_fixture(_T, CpuBackend(), on)


def test_fixture_bites_without_the_rows():
    """Node rows only: every node ends clear of the obstacle and the curve still passes deep inside it between two
    nodes."""
    X, U, sig, out, drv = _fixture(False)
    cont, node, bound, st, slack = orf.fixture_figures(X, U, sig, out)
    print(f"off: continuous clearance {cont:.4f}, node clearance {node:.4f}, status {st}, slack {slack:.1e}")
    assert cont <= -0.6
    assert node > 0 and st == 0


def test_fixture_clears_the_obstacle_in_continuous_time_with_the_rows():
    X, U, sig, out, drv = _fixture(True)
    cont, node, bound, st, slack = orf.fixture_figures(X, U, sig, out)
    print(f"on: continuous clearance {cont:.6f} (bound {bound:.2e}), node clearance {node:.6f}, status {st}, "
          f"slack {slack:.1e}")
    assert abs(cont) <= bound
    assert st == 0
    assert slack < 1e-12
    assert drv.coupling is None and int(drv._ob["overflow"].item()) == 0
