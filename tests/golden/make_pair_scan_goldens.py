"""Writes tests/golden/pair_scan_parent.npz: the outputs of separation_scan and intersample_pair_rows on the fixture of
tests/pair_scan_cases.py, for tests/test_pair_scan_bitwise_gpu.py.

Run it on an MI355X with the library whose results are the reference -- the commit before the two kernels' common
part became csrc/pair_scan.hpp:
    SCVX_HIP_LIB=<that build's libscvx_hip.so> python tests/golden/make_pair_scan_goldens.py

The file holds P16 (the input samples), `names` and `sha256` (one SHA-256 over the raw bytes per output array of
every case, which is what bit-for-bit equality needs), and the arrays themselves for the pruned cases at S = 8 under
their names, so that a mismatch can be located.  The unpruned arrays are not kept a second time: the generator
requires them equal to the pruned ones byte for byte (with P16 they would take the file past the largest golden here)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "dynamic-programming-multiagent-trajectory-optimiziation_amd"), REPO,
                os.path.dirname(HERE)]


def main():
    import torch
    import pair_scan_cases as pc
    cuda = torch.device("cuda:0")
    P16 = pc.make_p16()
    out, names, digests = {"P16": P16}, [], []
    for S in pc.S_ALL:
        got = pc.run(cuda, P16, S)
        for name, v in got.items():
            names.append(name)
            digests.append(np.frombuffer(pc.sha(v), np.uint8))
            if "/unpruned/" in name:
                assert pc.sha(v) == pc.sha(got[name.replace("/unpruned/", "/pruned/")]), name
            elif S == pc.S_FULL:
                out[name] = v
        cnt = got[f"rows/S{S}/J8/i0n70/pruned/count"]
        print(f"S={S}: {len(got)} arrays, {sum(v.nbytes for v in got.values())} bytes; J=8 lists full "
              f"{int((cnt == 8).sum())}, empty {int((cnt == 0).sum())} of {cnt.size}", flush=True)
    out["names"], out["sha256"] = np.array(names), np.stack(digests)
    path = os.environ.get("PAIR_SCAN_GOLDEN_OUT") or os.path.join(HERE, "pair_scan_parent.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
