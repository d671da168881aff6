"""The fixture of tests/test_pair_scan_bitwise_gpu.py, of its golden generator
(tests/golden/make_pair_scan_goldens.py) and of tests/test_pair_scan_fixture_cpu.py: separation_scan and
intersample_pair_rows (the two kernels built on csrc/pair_scan.hpp) on one small fleet.

Samples: separation_ref.random_fleet("di", 70, 5, seed=1) -- two agent blocks (the second with 6 lanes), three staged
tiles (the last with 6 neighbours: a chunk and a half) -- as closed-form dense samples at S = 16, agent 68's
overwritten with agent 5's: a coincident pair (distance 0 in every segment), and for every other agent two neighbours
at exactly equal distance.  S = 1, 2, 8 are the exact sub-samples P16[:, :, ::16 // S].  P16 itself is kept in the
golden file, so the inputs do not depend on the numpy build.

Cases, each pruned and unpruned, on the agent ranges (i0, n_local) = (0, 70) and (17, 40):
    scan/S<S>/...          separation_scan: sep, arg = (j, s), alpha
    rows/S<S>/J<J>/...     intersample_pair_rows at R = 1, cull = 5.5, J = 1 (list class 2, J below it), 3 (class 4, J
                           below it), 8 (class 8, full): rec, nbr, alpha, count, unused slots included
cull = 5.5 and not the 4.5 of tests/test_intersample_rows_gpu.py: at 4.5, S = 2 and S = 8 have no (agent, segment) with
more than 8 candidates."""
import hashlib

import numpy as np

import separation_ref as sr

N, K, SEED = 70, 5, 1
TWIN, TWIN_OF = 68, 5
S_ALL = (1, 2, 8, 16)
S_FULL = 8                                   # the S whose output arrays the golden keeps in full
RANGES = ((0, 70), (17, 40))                 # (i0, n_local)
J_ALL = (1, 3, 8)
R, CULL = 1.0, 5.5


def make_p16():
    """P16 (70,4,17,3) as described above (the generator's; tests read the golden's copy)."""
    X, U, sig = sr.random_fleet("di", N, K, SEED)
    P16, _ = sr.dense_closed_form("di", X, U, sig, 16)
    P16[TWIN] = P16[TWIN_OF]
    return P16


def samples(P16, S):
    """P (70,4,S+1,3) and L (70,4) at S sub-intervals."""
    P = np.ascontiguousarray(P16[:, :, ::16 // S])
    return P, sr.polyline_length(P)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def run(cuda, P16, S):
    """-> {name: numpy array} of every output array of every case at S, in a fixed order."""
    import torch
    import scvx_hip
    Pn, Ln = samples(P16, S)
    P, L = (torch.tensor(a, dtype=torch.float64, device=cuda) for a in (Pn, Ln))
    out = {}
    for i0, n in RANGES:
        for prune in (True, False):
            tag = f"i{i0}n{n}/{'pruned' if prune else 'unpruned'}"
            sc = scvx_hip.separation_scan(P, L, i0, n, prune=prune)
            out[f"scan/S{S}/{tag}/sep"] = sc["sep"]
            out[f"scan/S{S}/{tag}/arg"] = torch.stack((sc["j"], sc["s"]), dim=-1)
            out[f"scan/S{S}/{tag}/alpha"] = sc["alpha"]
            for J in J_ALL:
                rw = scvx_hip.intersample_pair_rows(P, L, i0, n, R, CULL, J=J, prune=prune)
                for key in ("rec", "nbr", "alpha", "count"):
                    out[f"rows/S{S}/J{J}/{tag}/{key}"] = rw[key]
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}
