// Continuous-time (inter-sample) agent-obstacle clearance and obstacle rows for the Jacobi QP (gfx950, float64): the
// chords of the pair scan (csrc/pair_scan.hpp) against points that do not move.
//
//   obstacle_scan_kernel   per (agent, segment k): every obstacle's closest approach over the segment's S chords
//                          (dist, alpha'), and the J obstacles that come closest to their surface strictly between
//                          the two nodes, as records (g, v, o, alpha') in the layout of intersample_pair_rows_kernel
//
// One lane per (agent, segment), 64 lanes to a workgroup, the lane's own S+1 samples in registers; no LDS, no
// barrier.  All lanes walk the same obstacles o = 0..O-1 (the loop index is wave-uniform, centre and radius are
// uniform loads), each lane its S chords in ascending s.  Per obstacle d_s = p_s - c_o and the first minimum over the
// chords of chord_closest(d_s, d_{s+1}), replaced only when strictly smaller: (q, s, a); dist = sqrt(q),
// alpha' = (s + a) / S, v = rho_o - dist.  The obstacle is a candidate when v > -cull, 0 < alpha' < 1 (a minimum at
// a node belongs to the node rows) and dist > 0 (no direction otherwise: dropped).  Per (agent, segment) the J
// candidates of largest v are kept in descending (v, then ascending o) order: obstacles are walked o ascending and a
// candidate moves ahead of a kept one only when its v is strictly larger, so the output does not depend on the
// launch geometry.  The list (v, o, s, a) lives in registers; the insertion is a chain of selects, no branch.  c is
// recomputed once at the end from the selected (s, a) by chord_point, the statement the chords use, so the written
// dist is the selected one bit for bit.  Record: g = c / dist, v = rho_o - dist; scvx_collision_rows_append_batched
// turns it into the two node rows g.(p_t - pbar_t) >= v - S_t unchanged.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.hpp"
#include "pair_scan.hpp"
#include "scvx_hip.h"

namespace scvx {

template <int S, int JM>
__global__ __launch_bounds__(64) void obstacle_scan_kernel(long long lanes, const double* __restrict__ P, int O,
                                                           const double* __restrict__ centers,
                                                           const double* __restrict__ rho, double cull, int J,
                                                           double* __restrict__ dist, double* __restrict__ alpha,
                                                           double* __restrict__ rec, int32_t* __restrict__ obs,
                                                           double* __restrict__ rec_alpha,
                                                           int32_t* __restrict__ count) {
    constexpr int W = (S + 1) * 3;
    const long long l = (long long)blockIdx.x * 64 + threadIdx.x;   // (agent, segment) = l / (K-1), l % (K-1)
    if (l >= lanes) return;                                         // no barrier below
    const double* own = P + l * W;
    double p[W];
#pragma unroll
    for (int e = 0; e < W; ++e) p[e] = own[e];
    // the kept list, descending in (v, then ascending o); empty slots hold -inf
    double kv[JM], ka[JM];
    int ko[JM], ks[JM];
#pragma unroll
    for (int r = 0; r < JM; ++r) { kv[r] = -INFINITY; ka[r] = 0.0; ko[r] = -1; ks[r] = 0; }
#pragma unroll 1
    for (int o = 0; o < O; ++o) {
        const double c0 = centers[o * 3LL], c1 = centers[o * 3LL + 1], c2 = centers[o * 3LL + 2], ro = rho[o];
        double bq = INFINITY, ba = 0.0;
        int bs = 0;
        double d0[3] = {p[0] - c0, p[1] - c1, p[2] - c2};
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const double d1[3] = {p[(s + 1) * 3] - c0, p[(s + 1) * 3 + 1] - c1, p[(s + 1) * 3 + 2] - c2};
            const Approach m = chord_closest(d0, d1);
            const bool take = m.q < bq;
            bq = take ? m.q : bq;
            ba = take ? m.al : ba;
            bs = take ? s : bs;
            d0[0] = d1[0]; d0[1] = d1[1]; d0[2] = d1[2];
        }
        const double ds = sqrt(bq);
        if (dist) {
            dist[l * O + o] = ds;
            alpha[l * O + o] = ((double)bs + ba) / (double)S;
        }
        if (rec) {
            // strictly between the nodes: not (s = 0, a = 0) and not (s = S-1, a = 1)
            const bool inner = (bs > 0 || ba > 0.0) && (bs < S - 1 || ba < 1.0);
            const double v = ro - ds;
            // no candidate: -inf, which is strictly larger than nothing and so moves nothing
            const double vv = (inner && bq > 0.0 && v > -cull) ? v : -INFINITY;
#pragma unroll
            for (int r = JM - 1; r > 0; --r) {
                const bool shift = vv > kv[r - 1], here = !shift && vv > kv[r];
                kv[r] = shift ? kv[r - 1] : (here ? vv : kv[r]);
                ka[r] = shift ? ka[r - 1] : (here ? ba : ka[r]);
                ko[r] = shift ? ko[r - 1] : (here ? o : ko[r]);
                ks[r] = shift ? ks[r - 1] : (here ? bs : ks[r]);
            }
            const bool first = vv > kv[0];
            kv[0] = first ? vv : kv[0];
            ka[0] = first ? ba : ka[0];
            ko[0] = first ? o : ko[0];
            ks[0] = first ? bs : ks[0];
        }
    }
    if (!rec) return;
    int n = 0;
#pragma unroll
    for (int r = 0; r < JM; ++r) {
        if (r >= J) break;
        double* out = rec + (l * J + r) * 4;
        if (ko[r] < 0) {  // unused slots are written too: the whole output is deterministic
            out[0] = out[1] = out[2] = out[3] = 0.0;
            obs[l * J + r] = -1;
            rec_alpha[l * J + r] = 0.0;
            continue;
        }
        ++n;
        // the samples s, s+1 of the selected chord come from memory again: no run-time index into registers
        const int s = ks[r];
        const double al = ka[r];
        const double* q = own + s * 3;
        const double* c = centers + ko[r] * 3LL;
        const double d0[3] = {q[0] - c[0], q[1] - c[1], q[2] - c[2]};
        const double d1[3] = {q[3] - c[0], q[4] - c[1], q[5] - c[2]};
        double cp[3];
        chord_point(d0, d1[0] - d0[0], d1[1] - d0[1], d1[2] - d0[2], al, cp);
        const double ds = sqrt(sq3(cp[0], cp[1], cp[2]));
        out[0] = cp[0] / ds;
        out[1] = cp[1] / ds;
        out[2] = cp[2] / ds;
        out[3] = rho[ko[r]] - ds;
        obs[l * J + r] = ko[r];
        rec_alpha[l * J + r] = ((double)s + al) / (double)S;
    }
    count[l] = n;
}

template <int S>
static int launch_obstacle_scan(long long lanes, const double* P, int O, const double* centers, const double* rho,
                                double cull, int J, double* dist, double* alpha, double* rec, int32_t* obs,
                                double* rec_alpha, int32_t* count, hipStream_t st) {
    const dim3 grid((unsigned)((lanes + 63) / 64));
#define SCVX_OBS_LAUNCH(JM)                                                                                  \
    hipLaunchKernelGGL((obstacle_scan_kernel<S, JM>), grid, dim3(64), 0, st, lanes, P, O, centers, rho, cull, J, \
                       dist, alpha, rec, obs, rec_alpha, count)
    if (J <= 2) {   // J = 0 (analysis only) runs the smallest list class with the list switched off
        SCVX_OBS_LAUNCH(2);
    } else if (J <= 4) {
        SCVX_OBS_LAUNCH(4);
    } else {
        SCVX_OBS_LAUNCH(8);
    }
#undef SCVX_OBS_LAUNCH
    return check_launch("obstacle_scan_kernel");
}

}  // namespace scvx

using namespace scvx;

extern "C" int scvx_obstacle_scan_batched(int K, int S, int N, const double* P, int O, const double* centers,
                                          const double* rho, double cull, int J, double* dist, double* alpha,
                                          double* rec, int32_t* obs, double* rec_alpha, int32_t* count,
                                          void* stream) {
    const bool ana = dist && alpha, ana_none = !dist && !alpha;
    const bool recs = rec && obs && rec_alpha && count, recs_none = !rec && !obs && !rec_alpha && !count;
    if (K < 2 || S < 1 || S > 16 || N < 0 || O < 1 || J < 0 || J > 8 || !P || !centers || !rho ||
        !(ana || ana_none) || !(recs || recs_none) || (ana_none && recs_none) || recs != (J >= 1) ||
        (recs && (K > 64 || !(cull > 0.0))))
        return set_error(SCVX_EINVAL, "obstacle_scan: bad args");
    const long long lanes = (long long)N * (K - 1);
    if (lanes == 0) return SCVX_OK;
    if ((lanes + 63) / 64 > 0x7fffffffLL) return set_error(SCVX_EINVAL, "obstacle_scan: bad args (N (K-1) too large)");
    return dispatch_S(S, "obstacle_scan", [&](auto tag) {
        return launch_obstacle_scan<decltype(tag)::S>(lanes, P, O, centers, rho, cull, J, dist, alpha, rec, obs,
                                                      rec_alpha, count, (hipStream_t)stream);
    });
}
