"""Fleet separation analysis on the GPU (csrc/separation.hip) against its numpy restatement
(tests/separation_ref.py), a brute-force continuous truth and the reference-generated goldens
(tests/golden/analysis_*.npz).

Shapes: N = 200 agents (above one 64-agent block and above one staged tile of 32 neighbours, a multiple of
neither), K = 5, S = 3 and 16, pos_dim 3 (double / single integrator) and 2 (unicycle); random inputs in a
+-6 box (separation_ref.random_fleet), whose minimum separation the helper checks to be >= 0.05 so that the
relative tolerances below are not eaten by cancellation.  1e-12 relative is the project's figure for GPU
against the same algorithm on the CPU."""
import functools
import os

import numpy as np
import pytest

import separation_ref as sr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N, K = 200, 5
POS_DIM = {"di": 3, "si": 3, "unicycle": 2}
CASES = [("di", 3), ("di", 16), ("unicycle", 3), ("unicycle", 16)]


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda:0")


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items() if hasattr(v, "cpu")}


@functools.lru_cache(maxsize=None)
def _inputs(model):
    return sr.random_fleet(model, N, K, 1)


@functools.lru_cache(maxsize=None)
def _gpu_rollout(model, S):
    import scvx_hip
    X, U, sig = _inputs(model)
    return scvx_hip.rollout_dense(model, _t(X), _t(U), _t(sig), S=S)


@functools.lru_cache(maxsize=None)
def _ref_scan(model, S):
    """The helper's chord scan of the kernel's own samples (computed once per case)."""
    P = _gpu_rollout(model, S)[0].cpu().numpy()
    out = sr.chord_scan(P)
    assert out[0].min() >= 0.05, out[0].min()
    return (P,) + out


@pytest.mark.parametrize("model,S", CASES + [("si", 3), ("si", 16)])
def test_rollout_dense_matches_the_helper(cuda, model, S):
    import scvx_hip
    X, U, sig = _inputs(model)
    P, L = (t.cpu().numpy() for t in _gpu_rollout(model, S))
    pd = POS_DIM[model]
    if model == "unicycle":
        Pr, Lr = sr.dense_rk4(model, X, U, sig, S, -(-scvx_hip.DEFAULT_NSUB[model] // S), pd)
    else:
        Pr, Lr = sr.dense_closed_form(model, X, U, sig, S, pd)
    assert P.shape == (N, K - 1, S + 1, 3) and L.shape == (N, K - 1)
    scale = np.abs(Pr).max()
    eP, eL = np.abs(P - Pr).max() / scale, (np.abs(L - Lr) / Lr).max()
    print(f"{model} S={S}: P {eP:.2e} of the position scale, L {eL:.2e} relative")
    assert eP <= 1e-12 and eL <= 1e-12
    assert np.array_equal(P[:, :, 0, :pd], X[:, :-1, :pd])          # sample 0 is the node, exactly
    assert not P[..., pd:].any()                                      # zeros past pos_dim


@pytest.mark.parametrize("model,S", CASES)
def test_separation_scan_matches_the_helper(cuda, model, S):
    import scvx_hip
    Pd, Ld = _gpu_rollout(model, S)
    P, sep_r, j_r, s_r, al_r = _ref_scan(model, S)
    full = scvx_hip.separation_scan(Pd, Ld, 0, N)
    sub = scvx_hip.separation_scan(Pd, Ld, 37, 70)
    for out, i0, n in ((full, 0, N), (sub, 37, 70)):
        g = _np(out)
        ref = sep_r[i0:i0 + n]
        e = (np.abs(g["sep"] - ref) / ref).max()
        print(f"{model} S={S} i0={i0}: sep {e:.2e} relative")
        assert e <= 1e-12
        assert ((g["j"] >= 0) & (g["j"] < N) & (g["j"] != np.arange(i0, i0 + n)[:, None])).all()
        assert ((g["s"] >= 0) & (g["s"] < S) & (g["alpha"] >= 0) & (g["alpha"] <= 1)).all()
        ii, kk = np.meshgrid(np.arange(i0, i0 + n), np.arange(K - 1), indexing="ij")
        back = sr.chord_dist(P, ii, kk, g["j"], g["s"], g["alpha"])
        assert (np.abs(back - g["sep"]) / g["sep"]).max() <= 1e-12
        assert np.allclose(g["tau"], (g["s"] + g["alpha"]) / S, rtol=0, atol=1e-15)
    f, s = _np(full), _np(sub)
    for key in ("sep", "j", "s", "alpha"):                          # a shard is the matching rows, bit for bit
        assert np.array_equal(s[key], f[key][37:107]), key


@pytest.mark.parametrize("model,S", CASES)
def test_pruned_and_unpruned_scans_are_bit_identical(cuda, model, S):
    import scvx_hip
    Pd, Ld = _gpu_rollout(model, S)
    a, b = _np(scvx_hip.separation_scan(Pd, Ld, 0, N)), _np(scvx_hip.separation_scan(Pd, Ld, 0, N, prune=False))
    for key in ("sep", "j", "s", "alpha"):
        assert np.array_equal(a[key], b[key]), key


def test_degenerate_pairs(cuda):
    import scvx_hip
    X = np.zeros((2, K, 6))
    X[:, :, 0:3] = [1.5, -2.0, 0.25]
    U, sig = np.zeros((2, K, 3)), np.array([1.0, 2.0])
    same = _np(scvx_hip.fleet_separation("di", _t(X), _t(U), _t(sig), S=8))
    assert np.array_equal(same["sep"], np.zeros((2, K - 1)))         # e.e == 0: alpha = 0, no 0/0
    assert np.isfinite(same["alpha"]).all() and np.isfinite(same["tau"]).all()
    X[1, :, 0] += 1.0
    apart = _np(scvx_hip.fleet_separation("di", _t(X), _t(U), _t(sig), S=8))
    assert np.array_equal(apart["sep"], np.ones((2, K - 1)))
    assert np.array_equal(apart["j"], np.array([[1] * (K - 1), [0] * (K - 1)]))
    one = scvx_hip.fleet_separation("di", _t(X[:1]), _t(U[:1]), _t(sig[:1]), S=8)
    assert one["argmin"] is None and one["min"] == np.inf
    one = _np(one)
    assert np.isposinf(one["sep"]).all() and (one["j"] == -1).all() and (one["s"] == -1).all()


def test_continuous_truth_and_a_crossing_between_nodes(cuda):
    """70 double integrators, S = 16: per-segment sep within max ||r''|| h^2 / 8 (+1e-12) of the exact cubics on
    2000 points per segment (a multiple of S, so the truth's grid holds every sample).  Agents 0 and 1 swap
    places at constant speed, 0.1 apart where they pass at tau = 0.375 (the middle of segment 1), far from
    everybody else: the node-level minimum is 2, and no node-level check sees the pass."""
    import scvx_hip
    n, S = 70, 16
    X, U, sig = (a[:n].copy() for a in _inputs("di"))
    t = np.arange(K) / (K - 1)
    for a, sgn in ((0, 1.0), (1, -1.0)):
        sig[a], U[a] = 2.0, 0.0
        X[a, :, 0], X[a, :, 1], X[a, :, 2] = sgn * (-3.0 + 8.0 * t), 0.05 * sgn, 20.0
        X[a, :, 3:] = [sgn * 8.0 / sig[a], 0.0, 0.0]
    out = scvx_hip.fleet_separation("di", _t(X), _t(U), _t(sig), S=S)
    g = _np(out)
    truth = sr.di_truth(X, U, sig, M=2000)
    bound = sr.di_chord_bound(U, sig, K, S)
    err = np.abs(g["sep"] - truth).max()
    print(f"worst scan-vs-truth error {err:.3e}, bound {bound:.3e}")
    assert err <= bound + 1e-12
    node = scvx_hip.pair_min_distance(_t(X)).cpu().numpy()
    assert node[0, 1] - truth[0, 1] > bound and node[0, 1] > 2.0
    assert abs(g["sep"][0, 1] - 0.1) <= bound + 1e-12 and g["sep"][0, 1] < node[0, 1] - bound
    assert g["j"][0, 1] == 1 and g["j"][1, 1] == 0
    assert abs(g["tau"][0, 1] - 0.5) <= 1.0 / S
    assert np.array_equal(g["agent_min"], g["sep"].min(1))
    i, j, k, tau = out["argmin"]
    assert out["min"] == g["sep"].min() == g["sep"][i, k] and g["j"][i, k] == j and g["tau"][i, k] == tau


@pytest.mark.parametrize("name", ["di", "unicycle"])
def test_node_level_minima_match_the_reference_goldens(cuda, name):
    import scvx_hip
    from SCvx.utils.analysis import min_agent_obstacle_distance, min_inter_agent_distance
    g = np.load(os.path.join(HERE, "golden", f"analysis_{name}.npz"))
    X_list = [x for x in g["X"]]
    obstacles = [(g["obs_center"][o], float(g["obs_radius"][o])) for o in range(len(g["obs_radius"]))]
    rr = float(g["robot_radius"])
    Xd = _t(g["X"].transpose(0, 2, 1))
    D = scvx_hip.pair_min_distance(Xd).cpu().numpy()
    O = scvx_hip.obstacle_min_distance(Xd, obstacles, rr).cpu().numpy()
    d_min, d_mat = min_inter_agent_distance(X_list)
    o_min, o_mat = min_agent_obstacle_distance(X_list, obstacles, rr)
    assert np.array_equal(D, d_mat) and np.array_equal(O, o_mat)
    assert np.abs(D - g["d_mat"]).max() <= 1e-12 * np.abs(g["d_mat"]).max()
    assert np.array_equal(D, D.T) and not np.diag(D).any()
    assert ((D == 0).sum() > len(X_list)) == (name == "unicycle")    # the coincident pair is an exact zero
    assert abs(d_min - float(g["d_min"])) <= 1e-12 * float(g["d_min"])
    assert np.abs(O - g["o_mat"]).max() <= 1e-12 * np.abs(g["o_mat"]).max()
    assert abs(o_min - float(g["o_min"])) <= 1e-12 * abs(float(g["o_min"]))
    with pytest.raises(ValueError):                                   # no strictly positive entry
        min_inter_agent_distance([X_list[0], X_list[0]])


@pytest.mark.parametrize("model", ["si", "unicycle"])
def test_compute_intersample_clearance(cuda, model):
    from SCvx.discretization.first_order_hold import FirstOrderHold
    from SCvx.models.single_integrator_model import SingleIntegratorModel
    from SCvx.models.unicycle_model import UnicycleModel
    from SCvx.utils.analysis import compute_intersample_clearance
    Kc, res = 6, 50
    Xa, Ua, _ = sr.random_fleet(model, 1, Kc, 5)
    X, U = Xa[0].T.copy(), Ua[0].T.copy()
    foh = FirstOrderHold({"si": SingleIntegratorModel, "unicycle": UnicycleModel}[model](), Kc)
    center = np.array([0.5, -1.0, 0.3])[:POS_DIM[model]]
    total = 1.0 + 0.25 + 0.05   # obs_radius + robot_radius + margin, summed as the function does
    tau_c, h_c, tau_d, h_d = compute_intersample_clearance(X, U, foh, center, 1.0, 0.25, 0.05, resolution=res)
    ref = sr.clearance_rollout(model, X, U, foh.dt, foh.rollout_nsub(1.0), center, total, res)
    assert tau_c.shape == h_c.shape == (res * (Kc - 1),) and np.array_equal(tau_d, np.arange(Kc))
    assert np.array_equal(tau_c, (np.arange(Kc - 1)[:, None] + np.linspace(0, 1, res, endpoint=False)).reshape(-1))
    e = np.abs(h_c - ref).max() / np.abs(ref).max()
    print(f"{model}: h_cont {e:.2e} relative")
    assert e <= 1e-12
    assert np.array_equal(h_d, np.linalg.norm(X[:len(center)].T - center, axis=1) - total)
    assert np.array_equal(h_c[::res], h_d[:-1])                      # t = 0 of every segment is the node


def test_jacobi_scvx_separation_equals_fleet_separation(cuda):
    import torch
    import scvx_hip
    from scvx_hip.scvx import JacobiSCvx
    n = 8
    X, U, sig = (_t(a[:n]) for a in _inputs("di"))
    spec = scvx_hip.QPSpec(model="di", K=K)
    drv = JacobiSCvx(spec, X[:, 0].contiguous(), X[:, -1].contiguous(), sig, tr0=0.5)
    a, b = drv.separation(X, U, S=8), scvx_hip.fleet_separation("di", X, U, sig, S=8)
    for key in ("sep", "j", "s", "alpha", "P", "L", "agent_min"):
        assert torch.equal(a[key], b[key]), key
    assert a["min"] == b["min"] and a["argmin"] == b["argmin"]
    drv.world = 2
    with pytest.raises(NotImplementedError, match="all-gather"):
        drv.separation(X, U)


def test_continuous_separation_drop_in(cuda):
    """SCvx.utils.analysis.min_inter_agent_separation_continuous (numpy in and out) is fleet_separation, whether
    the model is named, given as a model object or through its FirstOrderHold."""
    import scvx_hip
    from SCvx.discretization.first_order_hold import FirstOrderHold
    from SCvx.models.double_integrator_model import DoubleIntegratorModel
    from SCvx.utils.analysis import min_inter_agent_separation_continuous
    n = 8
    X, U, sig = (a[:n] for a in _inputs("di"))
    ref = scvx_hip.fleet_separation("di", _t(X), _t(U), _t(sig), S=8)
    X_list, U_list = [x.T for x in X], [u.T for u in U]
    model = DoubleIntegratorModel()
    for how in ("di", model, FirstOrderHold(model, K)):
        d_min, d_seg, info = min_inter_agent_separation_continuous(X_list, U_list, how, sig, S=8)
        assert d_min == ref["min"] and info["argmin"] == ref["argmin"]
        assert np.array_equal(d_seg, ref["sep"].cpu().numpy()) and np.array_equal(info["j"], ref["j"].cpu().numpy())
        assert np.array_equal(info["tau"], ref["tau"].cpu().numpy())
    with pytest.raises(ValueError):
        min_inter_agent_separation_continuous(X_list, U_list[:-1], "di", sig)
