"""Continuous-time collision rows on the GPU (csrc/intersample_rows.hip) against their numpy restatement
(tests/intersample_rows_ref.py), and the Jacobi driver with them on.

Kernel shapes: separation_ref.random_fleet("di") at N = 70 (two 64-agent blocks, the second with 6 agents; three
staged tiles of 32 neighbours, the last with 6), K = 5, S = 3 and 16, pos_dim 2 and 3, J = 2 and 8 (the smallest
and the largest list class).  R = 1 and cull = 4.5 with seed 1 give, in every case, (agent, segment) pairs with
more than J candidates and pairs with none, no candidate within 1e-9 of cull and no tie within 1e-9 at the J-th
place: the test asserts all of that on the restatement, so that the 1e-12 comparison (the figure of the separation
tests: GPU against the same algorithm on the CPU) is never a comparison of two different selections."""
import functools

import numpy as np
import pytest

import intersample_rows_ref as ir
import separation_ref as sr

pytestmark = pytest.mark.gpu
N, K, SEED, R, CULL = 70, 5, 1, 1.0, 4.5
CASES = [(pd, S, J) for pd in (2, 3) for S in (3, 16) for J in (2, 8)]


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda:0")


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _samples(pd, S):
    """The kernel's own samples (device and host) and the restatement's pair minima on them."""
    import scvx_hip
    X, U, sig = sr.random_fleet("di", N, K, SEED)
    Pd, Ld = scvx_hip.rollout_dense("di", _t(X), _t(U), _t(sig), S=S, pos_dim=pd)
    P = Pd.cpu().numpy()
    return X, Pd, Ld, P, ir.pair_minima(P)


@functools.lru_cache(maxsize=None)
def _ref(pd, S, J):
    return ir.pair_rows(_samples(pd, S)[3], 0, N, R, CULL, J)


@functools.lru_cache(maxsize=None)
def _gpu(pd, S, J):
    import scvx_hip
    _, Pd, Ld, _, _ = _samples(pd, S)
    return scvx_hip.intersample_pair_rows(Pd, Ld, 0, N, R, CULL, J=J)


@pytest.mark.parametrize("pd,S,J", CASES)
def test_pair_rows_match_the_restatement(cuda, pd, S, J):
    _, _, _, P, (Q, Sx, A, C) = _samples(pd, S)
    # the fixture's conditions, on the CPU side
    d = np.sqrt(Q)
    inner = ir.candidates(Q, Sx, A, S, np.inf)
    cand = ir.candidates(Q, Sx, A, S, CULL)
    n = cand.sum(0)
    assert (n > J).any() and (n == 0).any()
    assert np.abs(d[inner] - CULL).min() > 1e-9
    ds = np.sort(np.where(cand, d, np.inf), axis=0)
    more = np.isfinite(ds[J])
    assert (ds[J][more] - ds[J - 1][more]).min() > 1e-9
    rec_r, nbr_r, al_r, cnt_r = _ref(pd, S, J)
    g = _np(_gpu(pd, S, J))
    scale = np.abs(P).max()
    e_rec, e_al = np.abs(g["rec"] - rec_r).max() / scale, np.abs(g["alpha"] - al_r).max()
    print(f"pos_dim={pd} S={S} J={J}: (g, v) {e_rec:.2e} of the position scale, alpha' {e_al:.2e}; "
          f"{int((n > J).sum())} lists full, {int((n == 0).sum())} empty")
    assert np.array_equal(g["count"], cnt_r) and np.array_equal(g["nbr"], nbr_r)
    assert e_rec <= 1e-12 and e_al <= 1e-12 * scale
    assert not g["rec"][..., pd:3].any()                                 # zeros past pos_dim


@pytest.mark.parametrize("pd,S,J", CASES)
def test_outputs_do_not_depend_on_the_launch_geometry(cuda, pd, S, J):
    import scvx_hip
    _, Pd, Ld, _, _ = _samples(pd, S)
    full = _np(_gpu(pd, S, J))
    shard = _np(scvx_hip.intersample_pair_rows(Pd, Ld, 17, 40, R, CULL, J=J))
    unpruned = _np(scvx_hip.intersample_pair_rows(Pd, Ld, 0, N, R, CULL, J=J, prune=False))
    for key in ("rec", "nbr", "alpha", "count"):
        assert np.array_equal(shard[key], full[key][17:57]), key        # a shard is the matching rows, bit for bit
        assert np.array_equal(unpruned[key], full[key]), key             # the skip changes nothing


@pytest.mark.parametrize("pd,J", [(2, 2), (3, 8)])
def test_append_is_exact_against_the_restatement(cuda, pd, J):
    import torch
    import scvx_hip
    S = 3
    X = _samples(pd, S)[0]
    out = _gpu(pd, S, J)
    rec, cseg = out["rec"].cpu().numpy(), out["count"].cpu().numpy()
    rng = np.random.default_rng(4)
    for j_max in (2 + 2 * J, 3):                                         # roomy; too small: rows are dropped
        cnt0 = np.zeros((N, K), np.int32)
        cnt0[:, :K - 1] = rng.integers(0, 3, (N, K - 1))
        rows0 = rng.normal(size=(N, K, j_max, pd + 1))
        rows_r, cnt_r, over_r = ir.append_rows(X, 0, None, rec, cseg, rows0, cnt0, pd)
        rows, cnt, over = scvx_hip.append_collision_rows(_t(X), 0, out["rec"], out["count"], _t(rows0),
                                                         _t(cnt0, torch.int32), pos_dim=pd)
        assert np.array_equal(rows.cpu().numpy(), rows_r) and np.array_equal(cnt.cpu().numpy(), cnt_r)
        assert int(over.item()) == over_r and (over_r > 0) == (j_max == 3)
        assert cnt_r.max() <= j_max and (cnt_r[:, K - 1] == 0).all()
        # the counter accumulates over launches
        scvx_hip.append_collision_rows(_t(X), 0, out["rec"], out["count"], _t(rows0), _t(cnt0, torch.int32),
                                       pos_dim=pd, overflow=over)
        assert int(over.item()) == 2 * over_r
    # indexed form on a shard's records: agent a is idx[a], its records sit at idx[a] - i0
    sh = scvx_hip.intersample_pair_rows(_samples(pd, S)[1], _samples(pd, S)[2], 17, 40, R, CULL, J=J)
    idx = np.array([40, 17, 56, 30, 31], np.int32)
    j_max = 1 + 2 * J
    cnt0 = np.ones((8, K), np.int32)
    cnt0[:, K - 1] = 0
    rows0 = rng.normal(size=(8, K, j_max, pd + 1))                        # larger buffers: leading len(idx) entries
    rows_r, cnt_r, over_r = ir.append_rows(X, 17, idx, sh["rec"].cpu().numpy(), sh["count"].cpu().numpy(), rows0,
                                           cnt0, pd)
    rows, cnt, over = scvx_hip.append_collision_rows(_t(X), 17, sh["rec"], sh["count"], _t(rows0),
                                                     _t(cnt0, torch.int32), pos_dim=pd, idx=_t(idx, torch.int32))
    assert np.array_equal(rows.cpu().numpy(), rows_r) and np.array_equal(cnt.cpu().numpy(), cnt_r)
    assert int(over.item()) == over_r == 0 and cnt_r[:5].max() > 1
    assert np.array_equal(rows_r[5:], rows0[5:])
    with pytest.raises(ValueError, match="idx outside"):
        scvx_hip.append_collision_rows(_t(X), 17, sh["rec"], sh["count"], _t(rows0), _t(cnt0, torch.int32), pos_dim=pd,
                                       idx=_t(np.array([16], np.int32), torch.int32))
    with pytest.raises(ValueError):
        scvx_hip.intersample_pair_rows(_samples(pd, S)[1], _samples(pd, S)[2], 0, N, R, 0.0)


def test_nothing_in_reach_changes_nothing(cuda):
    """Four agents more than cull = 3R apart at all times: a step with the continuous-time rows on returns X and U
    bit-identical to the option off at the same QPSpec.j_max (the three node rows fit the node share either way)."""
    import torch
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx
    Kd = 8
    p0 = np.array([[0.0, 0, 0], [30, 0, 0], [0, 30, 0], [0, 0, 30]])
    pf = p0 + np.array([[3.0, 1, -2], [-2, 3, 1], [1, -2, 3], [2, 2, 2]])
    a = np.linspace(0, 1, Kd)
    X0 = np.zeros((4, Kd, 6))
    X0[:, :, :3] = p0[:, None] * (1 - a)[None, :, None] + pf[:, None] * a[None, :, None]
    sig = np.full(4, 7.0)
    res = []
    for S in (0, 8):
        spec = scvx_hip.QPSpec(model="di", K=Kd, box=[(0, -40.0, 40.0)], j_max=8, tol=1e-10)
        drv = JacobiSCvx(spec, _t(X0[:, 0]), _t(X0[:, -1]), _t(sig), 4.0, tr_rule="global",
                         coupling=CouplingSpec(R=1.0, intersample_S=S))
        X, U = _t(X0), _t(np.zeros((4, Kd, 3)))
        marks = []
        for _ in range(2):
            X, U, out = drv.step(X, U, marks=marks)
            X, U = X.clone(), U.clone()
        assert ("isrows" in [m for m, _ in marks]) == (S > 0)
        assert drv.last_check.get("is_overflow", -1) == (0 if S else -1) and int(out["status"].max()) == 0
        if S:
            assert int(drv._is["count_seg"].sum()) == 0 and int(drv.count.max()) == 3
        res.append((X, U))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], _t(X0))


def test_head_on_fixture_end_to_end(cuda):
    """The fixture of tests/test_intersample_rows_cpu.py on the kernels, two copies of the pair 100 apart (N = 4):
    off, the agents pass inside half of 2R between two nodes; on, the continuous minimum clears 2R up to the chord
    bound of DESIGN §3.6."""
    R2 = 2 * ir.HEAD_ON["R"]
    X, U, sig, out, _ = ir.run_head_on(_t, None, False, copies=2)
    cont, node, bound, st, slack = ir.head_on_figures(X, U, sig, out)
    print(f"off: continuous minimum {cont:.4f}, node minimum {node:.4f}, status {st}, slack {slack:.1e}")
    assert cont < 0.5 * R2
    X, U, sig, out, drv = ir.run_head_on(_t, None, True, copies=2)
    cont, node, bound, st, slack = ir.head_on_figures(X, U, sig, out)
    print(f"on: continuous minimum {cont:.6f} (bound {bound:.2e}), node minimum {node:.6f}, status {st}, "
          f"slack {slack:.1e}")
    assert cont >= R2 - bound - 1e-6
    assert st == 0
    assert slack < 1e-6
    assert node >= R2 - 1e-7
    assert int(drv._is["overflow"].item()) == 0


def test_the_constructed_swap_is_no_longer_left_inside_2R(cuda):
    """The pair of tests/test_separation_gpu.py that swaps places between two nodes (node-level minimum 2.0,
    continuous 0.1; here R = 1, so the node rows are content with it): after the fixture's 25 iterations with the
    rows on, JacobiSCvx.separation finds it no closer than 2R minus the chord bound."""
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx
    Ks, S = 5, 8
    X0, sig = np.zeros((2, Ks, 6)), np.full(2, 2.0)
    t = np.arange(Ks) / (Ks - 1)
    for a, sgn in ((0, 1.0), (1, -1.0)):
        X0[a, :, 0], X0[a, :, 1], X0[a, :, 2] = sgn * (-3.0 + 8.0 * t), 0.05 * sgn, 20.0
        X0[a, :, 3:] = [sgn * 8.0 / sig[a], 0.0, 0.0]
    spec = scvx_hip.QPSpec(model="di", K=Ks, j_max=8, w_coll=1e4, tol=1e-10, max_iter=80)
    drv = JacobiSCvx(spec, _t(X0[:, 0]), _t(X0[:, -1]), _t(sig), 4.0, tr_rule="global",
                     coupling=CouplingSpec(R=1.0, check=False, intersample_S=S, intersample_J=1))
    X, U = _t(X0), _t(np.zeros((2, Ks, 3)))
    before = drv.separation(X, U, S=S)["min"]
    for _ in range(ir.HEAD_ON["iters"]):
        X, U, out = drv.step(X, U)
        X, U = X.clone(), U.clone()
    after = drv.separation(X, U, S=S)["min"]
    bound = sr.di_chord_bound(U.cpu().numpy(), sig, Ks, S)
    print(f"swap: separation {before:.4f} -> {after:.6f} (bound {bound:.2e})")
    assert abs(before - 0.1) < 1e-9 and int(out["status"].max()) == 0
    assert after >= 2.0 - bound - 1e-6
