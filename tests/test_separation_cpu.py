"""Fleet separation analysis without a device: the C-ABI revision and symbols, argument rejection before any
GPU call, and the numpy restatement (tests/separation_ref.py) against the reference-generated goldens
(tests/golden/analysis_*.npz, made by tests/golden/make_analysis_goldens.py) and against its own brute-force
continuous truth."""
import ctypes
import os
import re

import numpy as np
import pytest

import separation_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NEW = ("scvx_rollout_dense_batched", "scvx_separation_scan_batched", "scvx_pair_min_distance_batched",
       "scvx_obstacle_min_distance_batched")


def test_abi_revision_and_symbols():
    from scvx_hip import _lib
    hdr = open(os.path.join(REPO, "include", "scvx_hip.h")).read()
    assert int(re.search(r"#define SCVX_HIP_VERSION (\d+)", hdr).group(1)) == 7
    L = _lib.lib()
    assert _lib.SCVX_HIP_VERSION == 7 == L.scvx_version()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name


def test_bad_arguments_are_rejected_without_a_device():
    from scvx_hip import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()   # a non-null address; a rejected call never reads it
    p = ctypes.cast(buf, ctypes.c_void_p)

    def bad(rc, code=-1):
        assert rc == code, (rc, L.scvx_last_error())
        assert L.scvx_last_error()

    roll = L.scvx_rollout_dense_batched
    for S in (0, 17):
        bad(roll(0, None, 5, 4, p, p, p, S, 1, 3, p, p, None))
    bad(roll(0, None, 5, 4, p, p, p, 8, 1, 4, p, p, None))      # pos_dim 4
    bad(roll(0, None, 5, 4, p, p, p, 8, 1, 0, p, p, None))
    bad(roll(0, None, 5, 4, p, p, p, 8, 0, 3, p, p, None))      # sub 0
    bad(roll(0, None, 1, 4, p, p, p, 8, 1, 3, p, p, None))      # K 1
    for hole in range(5):                                        # each null buffer
        a = [p] * 5
        a[hole] = None
        bad(roll(0, None, 5, 4, a[0], a[1], a[2], 8, 1, 3, a[3], a[4], None))
    bad(roll(_lib.SCVX_MODEL_RUNTIME, None, 5, 4, p, p, p, 8, 1, 3, p, p, None), -2)
    bad(roll(77, None, 5, 4, p, p, p, 8, 1, 3, p, p, None), -2)

    scan = L.scvx_separation_scan_batched
    for S in (0, 17):
        bad(scan(5, S, 4, p, p, 0, 4, p, p, p, 0, None))
    bad(scan(5, 8, 4, p, p, 2, 3, p, p, p, 0, None))            # i0 + N_local > N_total
    bad(scan(5, 8, 4, p, p, -1, 2, p, p, p, 0, None))
    bad(scan(5, 8, 4, p, p, 0, 4, p, p, p, 2, None))            # unknown flag
    for hole in range(5):
        a = [p] * 5
        a[hole] = None
        bad(scan(5, 8, 4, a[0], a[1], 0, 4, a[2], a[3], a[4], 0, None))

    pair = L.scvx_pair_min_distance_batched
    bad(pair(5, 6, 4, 4, p, p, None))                           # rows 4
    bad(pair(5, 2, 3, 4, p, p, None))                           # rows > n_x
    bad(pair(5, 6, 3, 4, None, p, None))
    bad(pair(5, 6, 3, 4, p, None, None))

    obst = L.scvx_obstacle_min_distance_batched
    bad(obst(5, 2, 4, p, 3, p, p, 0.1, p, None))                # n_x < 3
    bad(obst(5, 6, 4, None, 3, p, p, 0.1, p, None))
    bad(obst(5, 6, 4, p, 3, None, p, 0.1, p, None))
    bad(obst(5, 6, 4, p, 3, p, None, 0.1, p, None))
    bad(obst(5, 6, 4, p, 3, p, p, 0.1, None, None))


def test_wrappers_validate_shapes_before_the_device():
    import torch
    import scvx_hip
    X, U, sig = torch.zeros(4, 5, 6, dtype=torch.float64), torch.zeros(4, 5, 3, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        scvx_hip.rollout_dense("di", X, U, sig, S=17)
    with pytest.raises(ValueError):
        scvx_hip.rollout_dense("di", X, U, sig, pos_dim=4)
    with pytest.raises(ValueError):
        scvx_hip.rollout_dense("si", X, U, sig)
    with pytest.raises(ValueError):
        scvx_hip.separation_scan(torch.zeros(4, 4, 9, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64), 0, 4)
    with pytest.raises(ValueError):
        scvx_hip.separation_scan(torch.zeros(4, 4, 9, 3, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64), 2, 3)
    with pytest.raises(ValueError):
        scvx_hip.pair_min_distance(X, rows=4)
    with pytest.raises(ValueError):
        scvx_hip.obstacle_min_distance(X, [([0.0, 0.0], 1.0)], 0.1)
    with pytest.raises(scvx_hip.ScvxError):    # host tensors: no CPU fallback
        scvx_hip.rollout_dense("di", X, U, sig)
    with pytest.raises(scvx_hip.ScvxError):
        scvx_hip.pair_min_distance(X)


@pytest.mark.parametrize("name", ["di", "unicycle"])
def test_helper_reproduces_the_reference_goldens(name):
    g = np.load(os.path.join(HERE, "golden", f"analysis_{name}.npz"))
    X = np.ascontiguousarray(g["X"].transpose(0, 2, 1))   # (N, n, K) -> (N, K, n)
    d = sr.pair_min_distance(X)
    assert np.abs(d - g["d_mat"]).max() <= 1e-12 * np.abs(g["d_mat"]).max()
    assert d[d > 0].min() == pytest.approx(float(g["d_min"]), rel=1e-12)
    assert ((d == 0).sum() > X.shape[0]) == (name == "unicycle")   # the coincident pair
    o = sr.obstacle_min_distance(X, g["obs_center"], g["obs_radius"], float(g["robot_radius"]))
    assert np.abs(o - g["o_mat"]).max() <= 1e-12 * np.abs(g["o_mat"]).max()
    assert o.min() == pytest.approx(float(g["o_min"]), rel=1e-12)


def test_helper_chord_scan_is_within_the_derived_bound_of_the_truth():
    """12 random double integrators, K = 6, S = 4: |chord scan - brute-force cubic| <= max ||r''|| h^2 / 8."""
    K, S = 6, 4
    X, U, sig = sr.random_fleet("di", 12, K, 3)
    P, L = sr.dense_closed_form("di", X, U, sig, S)
    sep, j, s, al = sr.chord_scan(P)
    truth = sr.di_truth(X, U, sig, M=2000)
    bound = sr.di_chord_bound(U, sig, K, S)
    err = np.abs(sep - truth).max()
    print(f"worst chord-vs-truth error {err:.3e}, bound {bound:.3e}")
    assert err <= bound + 1e-12
    ii, kk = np.meshgrid(np.arange(12), np.arange(K - 1), indexing="ij")
    assert np.abs(sr.chord_dist(P, ii, kk, j, s, al) - sep).max() <= 1e-12 * sep.max()
    # the two roll-out restatements agree (the double integrator's RK4 is exact)
    P2, L2 = sr.dense_rk4("di", X, U, sig, S, 1, 3)
    assert np.abs(P - P2).max() <= 1e-12 * np.abs(P).max() and np.abs(L - L2).max() <= 1e-12 * L.max()
