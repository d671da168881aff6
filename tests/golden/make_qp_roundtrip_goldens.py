"""Writes tests/golden/qp_roundtrip_steps.npz: every step's outputs (X, U, obj, iters, status, slack_coll; nu for the
virtual-control case) of the Jacobi fixtures in tests/qp_roundtrip_cases.py, for tests/test_qp_roundtrips_gpu.py.

Run it on an MI355X with the library whose results are the reference -- the commit before the IPM iteration's
workspace round trips were merged (DESIGN §3.3 "Workspace round trips"):
    SCVX_HIP_LIB=<that build's libscvx_hip.so> python tests/golden/make_qp_roundtrip_goldens.py
The K = 50 instantiation's steps are stored under <case>/kspec/<step>/<key>; the runtime-K instantiation's are stored
under <case>/generic/... only where they differ from it (they run the same arithmetic, so normally nowhere: the
file then says so in `generic_equals_kspec`)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "dynamic-programming-multiagent-trajectory-optimiziation_amd"), REPO,
                os.path.dirname(HERE)]


def main():
    import torch
    import qp_roundtrip_cases as rc
    cuda = torch.device("cuda:0")
    out, same = {}, []
    for name in rc.CASES:
        spec_, gen = rc.run(cuda, name, False), rc.run(cuda, name, True)
        eq = all(np.array_equal(a[k], b[k]) for a, b in zip(spec_, gen) for k in rc.keys_of(name))
        same.append(eq)
        for inst, steps in (("kspec", spec_),) + ((() if eq else (("generic", gen),))):
            for s, st in enumerate(steps):
                for k in rc.keys_of(name):
                    v = st[k]
                    out[rc.golden_key(name, inst, s, k)] = v.astype(np.float64) if v.dtype.kind == "f" else v
        print(f"{name}: generic bitwise equal to kspec {eq}; iters per step {[st['iters'].tolist() for st in spec_]}, "
              f"status {[st['status'].tolist() for st in spec_]}")
    out["generic_equals_kspec"] = np.array(same)
    path = os.path.join(HERE, "qp_roundtrip_steps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
