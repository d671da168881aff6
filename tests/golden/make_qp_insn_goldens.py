"""Writes tests/golden/qp_insn_steps.npz: every step's outputs (X, U, obj, iters, status, slack_coll; nu for the
virtual-control case) of the Jacobi fixtures in tests/qp_insn_cases.py, for tests/test_qp_insn_gpu.py.

Run it on an MI355X with the library whose results are the reference -- the commit before the QP kernel got its
compile-time problem flags (DESIGN §3.3 "Non-arithmetic instructions"):
    SCVX_HIP_LIB=<that build's libscvx_hip.so> python tests/golden/make_qp_insn_goldens.py
That library has two instantiations per class: K = 50 at compile time (its own choice at K = 50) and the runtime-K one
(SCVX_QP_GENERIC_K=1; the only one at another K).  Its own choice is stored under <case>/K<K>/parent/<step>/<key>; the
forced runtime-K steps are stored under <case>/K<K>/generic/... only where they differ from it (they run the same
arithmetic, so normally nowhere: the file then says so in `generic_equals_parent`).

To keep the file small, the float arrays X, U and nu are stored in full for the last step only; for every step the
file holds their SHA-256 over the raw bytes (`.../<key>.sha256`), which is what bit-for-bit equality needs.  Every
step feeds the next, so the last step's arrays are also where a deviation shows in size."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "dynamic-programming-multiagent-trajectory-optimiziation_amd"), REPO,
                os.path.dirname(HERE)]


def main():
    import torch
    import qp_insn_cases as ic
    cuda = torch.device("cuda:0")
    out, same = {}, []
    for name, K in ic.all_cases():
        own, gen = ic.run(cuda, name, K, "flags"), ic.run(cuda, name, K, "generic")
        eq = all(np.array_equal(a[k], b[k]) for a, b in zip(own, gen) for k in ic.keys_of(name))
        same.append(eq)
        for inst, steps in (("parent", own),) + ((() if eq else (("generic", gen),))):
            for s, st in enumerate(steps):
                out.update(ic.pack(name, K, inst, s, st, last=s == len(steps) - 1))
        print(f"{name} K={K}: generic bitwise equal to the library's choice {eq}; iters per step "
              f"{[st['iters'].tolist() for st in own]}, status {[st['status'].tolist() for st in own]}", flush=True)
    out["generic_equals_parent"] = np.array(same)
    path = os.environ.get("QP_INSN_GOLDEN_OUT") or os.path.join(HERE, "qp_insn_steps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
