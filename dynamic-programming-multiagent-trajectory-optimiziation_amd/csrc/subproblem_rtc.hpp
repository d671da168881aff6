// Launchers of the runtime-compiled subproblem kernels (csrc/subproblem_rtc.hip): templates with
// model_id = SCVX_MODEL_RUNTIME (user models; n_x, n_u from the template).
#pragma once
#include <hip/hip_runtime.h>

#include "qp_layout.hpp"
#include "scp_layout.hpp"

namespace scvx {
// Limits of the runtime-compiled classes, shared by the solve entry points (qp_check, scp_launch) and
// scvx_rtc_subproblem_compile, so a class that compiles is one that launches.  nullptr when the class is served.
// QP: qp_class_error (qp_layout.hpp).
// SCP: the node vector z = [xi | g | game states | u | nu] within the kernel's 16 (n_x <= 8)
inline const char* rtc_scp_class_error(int nx, int nu, int ne) {
    if (nx < 1 || nx > 8 || nu < 1 || ne < 0 || 2 * nx + SCP_NG + ne + nu > 16)
        return "scp: runtime model needs 2 n_x + n_u + 4 (+ game states) <= 16";
    return nullptr;
}
// the QP kernel for class QPCfg<n_x, n_u, nb, no, nc, vc> (compiled at the first use)
int rtc_qp_launch(const QPArgs& a, int nb, int no, int nc, int vc, hipStream_t st);
// the SCP kernel scp_ipm_kernel<n_x, n_u, ne, nw>
int rtc_scp_launch(const SCPArgs& a, int ne, int nw, hipStream_t st);
}  // namespace scvx
