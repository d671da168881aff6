"""Continuous-time collision rows without a device: the numpy restatement's own properties
(tests/intersample_rows_ref.py), the C-ABI's argument rejection, the driver's option checks, and the head-on
fixture of DESIGN §3.7 end to end through scvx_hip.scvx.JacobiSCvx with the CPU restatements (oracle/) behind
the backend hooks."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import intersample_rows_ref as ir
import separation_ref as sr
from test_distributed_cpu import OracleBackend

R, CULL, S, J, K, N = 1.0, 4.5, 4, 3, 5, 24


class CpuBackend(OracleBackend):
    """OracleBackend plus the two hooks of the continuous-time rows, on the numpy restatement."""

    def intersample_pair_rows(self, model, X, U, sigma, S, nsub, pos_dim, R, cull, J):
        rec, count = ir.cpu_intersample_pair_rows(model, X.numpy(), U.numpy(), sigma.numpy(), S, nsub, pos_dim, R,
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


@functools.lru_cache(maxsize=None)
def _fleet():
    X, U, sig = sr.random_fleet("di", N, K, 3)
    P, _ = sr.dense_closed_form("di", X, U, sig, S)
    return X, P, ir.pair_rows(P, 0, N, R, CULL, J)


def test_records_are_sorted_unit_and_strictly_between_the_nodes():
    X, P, (rec, nbr, alpha, count) = _fleet()
    Q, Sx, A, C = ir.pair_minima(P)
    cand = ir.candidates(Q, Sx, A, S, CULL)
    assert (count > 0).any() and (count == J).any() and (count == 0).any()       # the fixture covers the cases
    assert np.array_equal(count, np.minimum(cand.sum(0), J))
    for a in range(N):
        for k in range(K - 1):
            n = count[a, k]
            js = nbr[a, k, :n]
            d = 2.0 * R - rec[a, k, :n, 3]
            assert (js >= 0).all() and (js != a).all() and len(set(js.tolist())) == n
            assert all((d[r], js[r]) < (d[r + 1], js[r + 1]) for r in range(n - 1))    # ascending (dist, j)
            assert ((alpha[a, k, :n] > 0) & (alpha[a, k, :n] < 1)).all() and (d > 0).all() and (d < CULL).all()
            assert np.abs(np.linalg.norm(rec[a, k, :n, :3], axis=1) - 1.0).max(initial=0.0) <= 1e-15
            rest = np.setdiff1d(np.nonzero(cand[:, a, k])[0], js)                    # nothing closer was left out
            assert n == 0 or rest.size == 0 or np.sqrt(Q[rest, a, k]).min() >= d.max()
            assert (nbr[a, k, n:] == -1).all() and not rec[a, k, n:].any() and not alpha[a, k, n:].any()
            # the record is the pair's chord closest approach: dist equals the scan's distance to that neighbour
            for r in range(n):
                assert abs(np.sqrt(Q[js[r], a, k]) - d[r]) <= 1e-15 * CULL


def test_two_appended_rows_imply_the_chord_row():
    """Rows g.dp_t >= v at both nodes of a segment give g.((1 - a') dp_k + a' dp_{k+1}) >= v: the first-order image
    of the closest point clears 2R.  Random displacements that satisfy both rows, with and without slack to spare."""
    _, _, (rec, nbr, alpha, count) = _fleet()
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


def test_append_writes_two_rows_per_record_and_none_at_the_last_node():
    X, _, (rec, nbr, alpha, count_seg) = _fleet()
    j_max = 2 * J + 2
    rows0 = np.zeros((N, K, j_max, 4))
    cnt0 = np.zeros((N, K), np.int32)
    cnt0[:, :K - 1] = 2
    rows0[:, :K - 1, :2] = 7.0
    rows, cnt, over = ir.append_rows(X, 0, None, rec, count_seg, rows0, cnt0, 3)
    assert over == 0 and (cnt[:, K - 1] == 0).all() and not rows[:, K - 1].any()
    want = 2 + count_seg.copy()
    want[:, 1:] += count_seg[:, :-1]
    assert np.array_equal(cnt[:, :K - 1], want)
    # two rows per record, but for the last segment's: their second node is K-1
    assert cnt.sum() == 2 * N * (K - 1) + 2 * count_seg.sum() - count_seg[:, -1].sum()
    assert (rows[:, :K - 1, :2] == 7.0).all()                                       # the node rows are kept
    for a, t in [(a, t) for a in range(N) for t in range(K - 1)]:
        m = 2
        for k in ([t, t - 1] if t else [t]):                                       # segment t first, then t-1
            for r in range(count_seg[a, k]):
                g, v = rec[a, k, r, :3], rec[a, k, r, 3]
                assert np.array_equal(rows[a, t, m, :3], g)
                # b - g.p <= S at p = pbar_t reads v <= S: the row is violated by exactly the deficit
                assert abs((rows[a, t, m, 3] - g @ X[a, t, :3]) - v) <= 1e-14 * (1 + np.abs(X[a, t, :3]).max())
                m += 1
    # a capacity too small: what does not fit is counted, never written; indexed form reads rec at idx - i0
    small, cs, over = ir.append_rows(X, 0, None, rec, count_seg, rows0[:, :, :3].copy(), cnt0, 3)
    assert over == int(np.maximum(want - 3, 0).sum()) > 0 and cs.max() == 3
    idx = np.array([5, 2, 9])
    ri, ci, _ = ir.append_rows(X, 0, idx, rec, count_seg, rows0[:3].copy(), cnt0[:3].copy(), 3)
    assert np.array_equal(ri, rows[idx]) and np.array_equal(ci, cnt[idx])


def test_bad_arguments_are_rejected_without_a_device():
    from scvx_hip import _lib
    L = _lib.lib()
    for name in ("scvx_intersample_pair_rows_batched", "scvx_collision_rows_append_batched"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    pr, ap = L.scvx_intersample_pair_rows_batched, L.scvx_collision_rows_append_batched
    good = dict(K=5, S=8, N=4, i0=0, n=4, R=1.0, cull=3.0, J=2, flags=0)

    def pair(**kw):
        a = dict(good, **kw)
        return pr(a["K"], a["S"], a["N"], p, p, a["i0"], a["n"], a["R"], a["cull"], a["J"], p, p, p, p, a["flags"], None)

    for kw in (dict(K=1), dict(K=65), dict(S=0), dict(S=17), dict(J=0), dict(J=9), dict(cull=0.0), dict(cull=-1.0),
               dict(i0=2), dict(i0=-1), dict(n=-1), dict(flags=2)):
        assert pair(**kw) == -1 and b"bad args" in L.scvx_last_error(), kw
    assert pr(5, 8, 4, None, p, 0, 4, 1.0, 3.0, 2, p, p, p, p, 0, None) == -1
    assert pair(n=0) == 0                                                           # nothing to do: no launch
    for args in ((1, 3, 6, 4, p, 0, None, 4, 2, p, p, 8, p, p, p, None), (5, 4, 6, 4, p, 0, None, 4, 2, p, p, 8, p, p, p, None),
                 (5, 3, 6, 4, p, 1, None, 4, 2, p, p, 8, p, p, p, None), (5, 3, 6, 4, p, 0, None, 4, 9, p, p, 8, p, p, p, None),
                 (5, 3, 6, 4, p, 0, None, 4, 2, p, p, 33, p, p, p, None), (5, 3, 6, 4, p, 0, None, 4, 2, p, p, 8, p, p, None, None)):
        assert ap(*args) == -1 and b"bad args" in L.scvx_last_error(), args
    assert ap(5, 3, 6, 4, p, 0, None, 0, 2, p, p, 8, p, p, p, None) == 0


def test_driver_option_checks():
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx
    X, U, sig = ir.head_on()
    mk = lambda j_max, **kw: JacobiSCvx(scvx_hip.QPSpec(model="di", K=8, j_max=j_max), _T(X[:, 0]), _T(X[:, -1]),   # noqa: E731
                                       _T(sig), 4.0, coupling=CouplingSpec(R=1.0, **kw), backend=CpuBackend())
    off = mk(8)
    assert off._is is None and CouplingSpec().intersample_S == 0 and CouplingSpec().intersample_J == 2
    on = mk(8, intersample_S=8)
    assert on._is["j_node"] == 4 and on._is["cull"] == 3.0 and on._is["rows_node"].shape == (2, 8, 4, 4)
    assert mk(8, intersample_S=8, intersample_cull=2.5)._is["cull"] == 2.5
    with pytest.raises(ValueError, match="capacity"):
        mk(4, intersample_S=8)                                                      # 4 - 2 x 2 leaves no node row
    with pytest.raises(ValueError, match="capacity"):
        mk(8, intersample_S=8, intersample_J=4)
    with pytest.raises(ValueError):
        mk(8, intersample_S=17)
    import unittest.mock as um
    with um.patch("torch.distributed.is_initialized", return_value=True), \
            um.patch("torch.distributed.get_world_size", return_value=2), \
            um.patch("torch.distributed.get_rank", return_value=0):
        with pytest.raises(NotImplementedError, match="all-gather"):
            mk(8, intersample_S=8)
        assert mk(8).world == 2                                                     # off: nothing changes


@functools.lru_cache(maxsize=None)
def _head_on(on):
    return ir.run_head_on(_T, CpuBackend(), on)


def test_head_on_fixture_bites_without_the_rows():
    """Node rows only: every node ends 2R apart and the agents still pass well inside 2R between two nodes."""
    X, U, sig, out, drv = _head_on(False)
    cont, node, bound, st, slack = ir.head_on_figures(X, U, sig, out)
    print(f"off: continuous minimum {cont:.4f}, node minimum {node:.4f}, status {st}, slack {slack:.1e}")
    assert cont < 0.5 * 2 * ir.HEAD_ON["R"]
    assert node >= 2 * ir.HEAD_ON["R"] - 1e-7 and st == 0


def test_head_on_fixture_clears_2R_in_continuous_time_with_the_rows():
    X, U, sig, out, drv = _head_on(True)
    cont, node, bound, st, slack = ir.head_on_figures(X, U, sig, out)
    print(f"on: continuous minimum {cont:.6f} (bound {bound:.2e}), node minimum {node:.6f}, status {st}, "
          f"slack {slack:.1e}")
    R2 = 2 * ir.HEAD_ON["R"]
    assert cont >= R2 - bound - 1e-6
    assert st == 0
    assert slack < 1e-6
    assert node >= R2 - 1e-7
