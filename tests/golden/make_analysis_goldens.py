"""Generate the trajectory-analysis golden vectors by running the REFERENCE implementation here.

Run (container only; /root/reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_analysis_goldens.py

Imported unmodified from the reference: SCvx/utils/analysis.py (min_inter_agent_distance,
min_agent_obstacle_distance).  Outputs: small .npz fixtures (inputs + expected outputs) next to this script:

    analysis_di.npz        70 double-integrator states (n = 6), K = 5, 3 obstacles
    analysis_unicycle.npz  70 unicycle states (n = 3: the heading is row 2 of the reference's rows 0:3 and
                           enters its norms), K = 5, 3 obstacles; agents 11 and 40 coincide at node 2, so
                           d_mat has an off-diagonal zero and d_min_global exercises the reference's "> 0" rule
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from SCvx.utils.analysis import min_agent_obstacle_distance, min_inter_agent_distance  # noqa: E402  (reference)


def run_case(name, X, obstacles, robot_radius):
    """X (N, n, K): the reference's per-agent (n, K) arrays."""
    X_list = [x for x in X]
    d_min, d_mat = min_inter_agent_distance(X_list)
    o_min, o_mat = min_agent_obstacle_distance(X_list, obstacles, robot_radius)
    np.savez(os.path.join(HERE, f"analysis_{name}.npz"), X=X, obs_center=np.array([c for c, _ in obstacles], float),
             obs_radius=np.array([r for _, r in obstacles], float), robot_radius=robot_radius, d_min=d_min,
             d_mat=d_mat, o_min=o_min, o_mat=o_mat)
    print(name, "d_min", d_min, "zeros off the diagonal", int((d_mat == 0).sum()) - len(X_list), "o_min", o_min)


def main():
    rng = np.random.default_rng(2024)
    N, K = 70, 5
    obstacles = [([0.5, -1.0, 0.3], 1.0), ([-3.0, 2.0, 1.0], 0.7), ([4.0, 4.0, -2.0], 1.5)]
    X = rng.uniform(-6.0, 6.0, (N, 6, K))
    run_case("di", X, obstacles, 0.25)
    X = rng.uniform(-6.0, 6.0, (N, 3, K))
    X[:, 2] = rng.uniform(-np.pi, np.pi, (N, K))
    X[40, :, 2] = X[11, :, 2]
    run_case("unicycle", X, obstacles, 0.25)


if __name__ == "__main__":
    main()
