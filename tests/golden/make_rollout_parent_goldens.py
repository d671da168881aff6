"""Writes tests/golden/rollout_parent.npz: the outputs of every kernel that takes the FOH-input RK4 state step
(integrate_nonlinear, rollout_dense, intersample_batched; foh_batched as a guard) on the fixtures of
tests/rollout_bitwise_cases.py, for tests/test_rollout_bitwise_gpu.py.

Run it on an MI355X with the library whose results are the reference -- the commit before the three copies of the
step became foh_body.hpp's rk4_step:
    SCVX_HIP_LIB=<that build's libscvx_hip.so> python tests/golden/make_rollout_parent_goldens.py
One vector per model and shape is stored under <model>/N<N>K<K> (rollout_bitwise_cases.key, .pack)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "dynamic-programming-multiagent-trajectory-optimiziation_amd"), REPO,
                os.path.dirname(HERE)]


def main():
    import torch
    import rollout_bitwise_cases as rc
    cuda = torch.device("cuda:0")
    out = {}
    for model in rc.MODELS:
        for N, K in rc.SHAPES:
            got = rc.run(cuda, model, N, K)
            out[rc.key(model, N, K)] = rc.pack(got)
            print(f"{model} N={N} K={K}: {len(got)} arrays, {sum(v.nbytes for v in got.values())} bytes, "
                  f"inter-sample minima {int(got['is/n_crit'].sum())} (most per slot {int(got['is/n_crit'].max())})")
    path = os.path.join(HERE, "rollout_parent.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
