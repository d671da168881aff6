"""Times the moving-obstacle scan (csrc/moving_obstacles.hip) on the GPU next to the static obstacle scan
(scvx_obstacle_scan_batched) and the dense roll-out of the same process, at the C3 shape (1024 double integrators,
K = 50; bench.make_workload's trajectories) and the C4 shape (4096 agents on the 16^3 lattice;
workloads.synthetic_lattice), both with every node given the straight line's constant velocity (the workloads' own
trajectories stand still between the nodes: tools/obstacle_rows_time.py).  8 tracks of 2 knots: the shape's 8
obstacles (workloads' obs_seed 11), each moving one diameter along x over the horizon; the static scan runs on their
first knots.  S = 8, J = 2, cull = the largest radius.  Device lists throughout (what the driver's backend passes
after its first step).  HIP events around each launch, median of 20 launches after 5 warm-ups, the kernels alternating
in one process (tools/separation_time.py's loop).  Prints one JSON line per (shape, kernel) with the ratios to the
static scan of the same outputs and to rollout_dense: the spread between runs on shared machines exceeds the spread
between kernels, so the ratios are the figures to keep.  "_5_knots": the same tracks with three knots inserted (the
per-lane gather of the knots instead of the wave-uniform loads).
usage: python tools/moving_obstacles_time.py [S [J]]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dynamic-programming-multiagent-trajectory-optimiziation_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import scvx_hip  # noqa: E402
from scvx_hip import workloads  # noqa: E402
from separation_time import timed  # noqa: E402


def main(S=8, J=2):
    S, J = int(S), int(J)
    dev = torch.device("cuda:0")
    shapes = {"c3": workloads.synthetic_di(1024, K=bench.K, seed=1, sigma=bench.SIGMA, obstacles=bench.N_OBS),
              "c4": workloads.synthetic_lattice(side=16, K=bench.K, seed=2, sigma=bench.SIGMA, obstacles=bench.N_OBS)}
    for name, sc in shapes.items():
        Xh = sc["X"].copy()
        Xh[:, :, 3:6] = ((Xh[:, -1, 0:3] - Xh[:, 0, 0:3]) / sc["sigma"][:, None])[:, None, :]
        X, U, sig = torch.tensor(Xh, device=dev), torch.tensor(sc["U"], device=dev), torch.tensor(sc["sigma"], device=dev)
        N, K = X.shape[0], X.shape[1]
        obs = [(np.asarray(c, float), float(r)) for c, r in sc["obs"]]
        cull, T = max(r for _, r in obs), float(sc["sigma"].max())
        ends = [(c, c + np.array([2.0 * r, 0.0, 0.0])) for c, r in obs]
        tr2 = scvx_hip.obstacle_tracks([(np.stack(e), (0.0, T), r) for e, (_, r) in zip(ends, obs)], dev)
        tr5 = scvx_hip.obstacle_tracks([(np.linspace(e[0], e[1], 5), (0.0, T), r) for e, (_, r) in zip(ends, obs)], dev)
        obs_dev = scvx_hip._obstacle_arrays("moving_obstacles_time", obs, dev)
        P, _ = scvx_hip.rollout_dense("di", X, U, sig, S=S)
        a = scvx_hip.moving_obstacle_scan(P, sig, tr2, cull=cull, J=J)
        mov = lambda tr, **kw: (lambda: scvx_hip.moving_obstacle_scan(P, sig, tr, cull=cull, **kw))  # noqa: E731
        t = timed({"rollout_dense": lambda: scvx_hip.rollout_dense("di", X, U, sig, S=S),
                   "obstacle_scan_records": lambda: scvx_hip.obstacle_scan(P, obs_dev, cull=cull, J=J, analysis=False),
                   "moving_scan_records": mov(tr2, J=J, analysis=False, node_rows=False),
                   "moving_scan_records_and_node_rows": mov(tr2, J=J, analysis=False),
                   "moving_scan_records_and_node_rows_5_knots": mov(tr5, J=J, analysis=False),
                   "obstacle_scan_analysis": lambda: scvx_hip.obstacle_scan(P, obs_dev),
                   "moving_scan_analysis": mov(tr2),
                   "moving_scan_analysis_5_knots": mov(tr5)})
        for k, ms in t.items():
            static = t["obstacle_scan_analysis" if "analysis" in k else "obstacle_scan_records"]
            print(json.dumps(dict(shape=name, N=N, K=K, S=S, J=J, O=len(obs), cull=round(cull, 4), kernel=k,
                                  median_ms=round(ms, 4), ratio_to_static_scan=round(ms / static, 3),
                                  ratio_to_rollout=round(ms / t["rollout_dense"], 3))), flush=True)
        print(json.dumps(dict(shape=name, records=int(a["count"].sum().item()),
                              node_records=int(a["node_count"].sum().item()),
                              min_clearance=round(float((a["dist"] - tr2[3]).min().item()), 4))), flush=True)


if __name__ == "__main__":
    main(*sys.argv[1:3])
