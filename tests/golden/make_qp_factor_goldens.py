"""Writes tests/golden/qp_factor_steps.npz: every step's outputs (X, U, obj, iters, status, slack_coll; nu for the
virtual-control case) of the Jacobi fixtures in tests/qp_factor_cases.py, for tests/test_qp_factor_gpu.py.

Run it on an MI355X with the library whose results are the reference -- the commit before the factor sweep's reads were
rescheduled (DESIGN §3.3 "The factor's read batches"):
    SCVX_HIP_LIB=<that build's libscvx_hip.so> python tests/golden/make_qp_factor_goldens.py
Every case has a runtime K, so that library runs its runtime-K, runtime-flag instantiation on each (checked).  Next to
the outputs the file keeps the workspace bytes per agent of the class each case ran on (<case>/K<K>/ws_bytes).

To keep the file small, the float arrays X, U and nu are stored in full for the last step only; for every step the
file holds their SHA-256 over the raw bytes (`.../<key>.sha256`), which is what bit-for-bit equality needs."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "dynamic-programming-multiagent-trajectory-optimiziation_amd"), REPO,
                os.path.dirname(HERE)]


def main():
    import torch
    import qp_factor_cases as fc
    from scvx_hip import _lib
    cuda = torch.device("cuda:0")
    out = {}
    for name, K in fc.CASES:
        tpl = fc.build(name, K)[2].to_c()
        inst = int(_lib.lib().scvx_qp_instantiation(ctypes.byref(tpl)))
        assert inst == 0, (name, K, inst)
        steps = fc.run(cuda, name, K)
        for s, st in enumerate(steps):
            out.update(fc.pack(name, K, s, st, last=s == len(steps) - 1))
        out[f"{name}/K{K}/{fc.WS_KEY}"] = np.array(fc.ws_bytes(name, K), dtype=np.int64)
        print(f"{name} K={K}: {fc.ws_bytes(name, K)} workspace bytes per agent; iters per step "
              f"{[st['iters'].tolist() for st in steps]}, status {[st['status'].tolist() for st in steps]}", flush=True)
    path = os.environ.get("QP_FACTOR_GOLDEN_OUT") or os.path.join(HERE, "qp_factor_steps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
