// Argument block and node-block layout of the SCProblem kernel (csrc/scp_kernel.hpp), shared by the kernel and the
// host code that sizes its workspace and launches it (no kernel body here).
// (Also compiled at run time for user models: csrc/subproblem_rtc.hip.)
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#include "scvx_hip.h"

namespace scvx {

constexpr int SCP_NG = 4;
constexpr int SCP_KMAX = 256;

struct SCPArgs {
    scvx_scp_template T;
    int N;
    const double *disc, *Xref, *Uref, *sigma_ref, *tr, *x_init, *x_final, *nbr_pos, *nbr_Y, *nbr_Lam;
    const double *X_prev, *slab_z, *slab_P;  // Nash best response (T.game)
    double *X, *U, *nu, *sigma, *s_obs, *s_nbr, *obj;
    int32_t *status, *iters;
    double* ws;
    long long ws_agent;
};

// node-block layout (doubles); counts are runtime (rows depend on the template)
struct SCPLay {
    int RH, NS, Q, RL, ROWS, stride;
    int o_rows, o_q, o_P, o_At, o_Bt, o_ct, o_z, o_sig, o_s, o_lam, o_wl, o_sw, o_lt, o_H, o_f, o_rd, o_rc, o_rsig,
        o_t, o_rho, o_rhs, o_dz, o_dsig, o_ds, o_dl, o_dsa, o_dla, o_y, o_yp, o_rp, o_K, o_Pr, o_pv, o_kv, o_LD, o_nh,
        o_zb, o_sgb, o_Acl, o_g, o_w, o_e;
};

// augmented game states: u~_k = u_{k-1} (m), th~_k = th_{k-1} (1 when the model has a heading)
__host__ __device__ inline int scp_ne(const scvx_scp_template& T) {
    return T.game ? T.n_u + (T.theta_idx >= 0 ? 1 : 0) : 0;
}

__host__ __device__ inline SCPLay scp_layout(const scvx_scp_template& T) {
    const int n = T.n_x, m = T.n_u;
    const int NXA = n + SCP_NG + scp_ne(T), NUA = m + n, NZ = NXA + NUA;
    SCPLay L{};
    int sides = 0;
    for (int b = 0; b < T.n_ubound; ++b) sides += (T.ub_has_lo[b] ? 1 : 0) + (T.ub_has_hi[b] ? 1 : 0);
    L.RH = (1 << n) + (1 << m) + (1 << n) + sides + 2 * T.n_xbound + 3 + (T.game ? T.n_slab : 0);
    L.NS = T.n_obs + T.n_nbr;
    L.Q = T.has_soc ? m + 1 : 0;
    L.RL = L.RH + 2 * L.NS + L.Q;
    L.ROWS = L.RH + L.NS + L.Q;
    int o = 0;
    auto take = [&](int sz) { const int r = o; o += sz; return r; };
    L.o_rows = take(L.ROWS * (NZ + 1));
    L.o_q = take(NZ);
    L.o_P = take(NZ * NZ);
    L.o_At = take(NXA * NXA);
    L.o_Bt = take(NXA * NUA);
    L.o_ct = take(NXA);
    L.o_z = take(NZ);
    L.o_sig = take(L.NS);
    L.o_s = take(L.RL);
    L.o_lam = take(L.RL);
    L.o_wl = take(L.RH + 2 * L.NS);
    L.o_sw = take(L.Q + 1);
    L.o_lt = take(L.RL);
    L.o_H = take(NZ * NZ);
    L.o_f = take(NZ);
    L.o_rd = take(NZ);
    L.o_rc = take(L.RL);
    L.o_rsig = take(L.NS);
    L.o_t = take(L.RL);
    L.o_rho = take(L.RL);
    L.o_rhs = take(L.NS);
    L.o_dz = take(NZ);
    L.o_dsig = take(L.NS);
    L.o_ds = take(L.RL);
    L.o_dl = take(L.RL);
    L.o_dsa = take(L.RL);
    L.o_dla = take(L.RL);
    L.o_y = take(NXA);
    L.o_yp = take(NXA);
    L.o_rp = take(NXA);
    L.o_K = take(NUA * NXA);
    L.o_Pr = take(NXA * NXA);
    L.o_pv = take(NXA);
    L.o_kv = take(NUA);
    L.o_LD = take(NUA * NUA);
    L.o_nh = take(1);
    L.o_zb = take(NZ);       // best iterate (z, soft slacks) once the reduced tolerances hold
    L.o_sgb = take(L.NS);
    L.o_Acl = take(NXA * NXA);  // closed-loop Acl = At + Bt K (row-major), LQ chain offsets g, w, e
    L.o_g = take(NXA);
    L.o_w = take(NXA);
    L.o_e = take(NXA);
    L.stride = (o + 7) & ~7;
    if (L.stride < 64) L.stride = 64;  // the junk block after the K node blocks holds one slot per lane
    return L;
}

}  // namespace scvx
