"""GPU: the QP kernel's runtime-K instantiation at the node counts where the workspace layout can go wrong, against
the CPU twin (oracle.qp_cpu): K = 12 (the minimum a warm start allows, K >= 2 n_x), K = 13 (odd: the bases of the
packet and factor-block regions fall on odd elements) and K = 64 (every lane owns a node: no out-of-range lanes).
The c2 class (no obstacles, no input cone) and the C3 class (8 obstacles, cone, box), 4 agents each; bounds as
tests/test_qp_gpu.py, kernel against twin: status equal, objective 1e-8 relative, X and U 1e-6 absolute."""
import numpy as np
import pytest

import scvx_hip
from oracle import qp_cpu
from scvx_hip import workloads

pytestmark = pytest.mark.gpu

BOX = [(0, -12.0, 12.0), (1, -12.0, 12.0)]
N = 4


def _t(x, cuda):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=cuda, dtype=torch.float64)


@pytest.mark.parametrize("c3", [False, True], ids=["c2", "c3"])
@pytest.mark.parametrize("K", [12, 13, 64])
def test_generic_kernel_matches_twin_at_edge_node_counts(cuda, K, c3):
    sc = workloads.synthetic_di(N, K=K, seed=3, obstacles=8 if c3 else 0)   # seed 3: an obstacle row is active
    umax = 1.0 if c3 else None
    X, U, sig = _t(sc["X"], cuda), _t(sc["U"], cuda), _t(sc["sigma"], cuda)
    disc = scvx_hip.foh_batched("di", X, U, sig)
    spec = scvx_hip.QPSpec(model="di", K=K, box=BOX, obs=sc["obs"], w_obs=1e6, u_max=umax, tol=1e-10, max_iter=80)
    tr = np.full(N, 0.25)
    out = scvx_hip.qp_solve_batched(spec, disc, sig, X, U, _t(sc["x_init"], cuda), _t(sc["x_final"], cuda), _t(tr, cuda))
    tpl = qp_cpu.make_template(6, 3, K, box=BOX, obs=sc["obs"], w_obs=1e6, u_max=umax, tol=1e-10, max_iter=80)
    cpu = qp_cpu.solve_batched(tpl, disc.cpu().numpy(), sc["sigma"], sc["X"], sc["U"], sc["x_init"], sc["x_final"], tr)
    st = out["status"].cpu().numpy()
    assert (cpu["status"] == 0).all(), cpu["status"]
    assert np.array_equal(st, cpu["status"]), (st, cpu["status"])
    og, Xg, Ug = out["obj"].cpu().numpy(), out["X"].cpu().numpy(), out["U"].cpu().numpy()
    dobj = np.abs(og - cpu["obj"]) / np.maximum(1.0, np.abs(cpu["obj"]))
    dX, dU = np.abs(Xg - cpu["X"]).max(), np.abs(Ug - cpu["U"]).max()
    print(f"K={K} c3={c3}: max rel |dobj| {dobj.max():.3e}, |dX| {dX:.3e}, |dU| {dU:.3e}, iters "
          f"{out['iters'].cpu().numpy().tolist()} (twin {cpu['iters'].tolist()})")
    assert dobj.max() <= 1e-8
    assert dX < 1e-6 and dU < 1e-6
