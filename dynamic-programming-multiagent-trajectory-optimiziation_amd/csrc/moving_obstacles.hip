// Moving obstacles for the Jacobi QP (gfx950, float64): the obstacle scan of obstacle_rows.hip against centres that
// follow a track in real time, and the node rows the QP kernel offers for fixed centres only.
//
//   moving_obstacle_scan_kernel   per (agent, segment k): every obstacle's closest approach over the segment's S
//                                 chords of the RELATIVE samples p_s - q_o(t_s) (dist, alpha'), the J obstacles that
//                                 come closest to their surface strictly between the two nodes as records
//                                 (g, v, o, alpha'), and the J that are closest at the segment's first node as node
//                                 records (g, v, o)
//   node_rows_append_kernel       each node record becomes one node row, behind the rows already present
//
// Track o: n_o knots [M_max][3], equally spaced over the real-time window [t0_o, t1_o]; the obstacle waits at its
// first knot before t0 and at its last after t1 (track_point).  One knot: a fixed centre, the window is not read.
// Agent i lives on its own clock: sample s of segment k is at t = sigma_i (k S + s) / ((K-1) S), formed as
// dt_i (k S + s) with dt_i = sigma_i / ((K-1) S) divided once per lane; (n_o - 1) / (t1 - t0) is divided once per
// obstacle, so a sample costs no division.
//
// The frame is obstacle_scan_kernel's: one lane per (agent, segment), 64 lanes to a workgroup, the lane's own S+1
// samples in registers, no LDS, no barrier, the obstacle loop wave-uniform, the kept lists select chains in
// registers, unused slots written.  The walk is that kernel's too -- first minimum over the chords of chord_closest
// (pair_scan.hpp), replaced only when strictly smaller, c recomputed at the end through chord_point from the selected
// (s, a) -- so a record's dist is the scan's bit for bit, and with one knot per obstacle d_s = p_s - c_0 exactly: the
// outputs are the static scan's bit for bit.  Tracks of one or two knots (a fixed centre, a constant-velocity
// intruder) read their knots through wave-uniform loads; longer ones gather the two knots around each sample's time
// per lane.  Both run track_point's expressions.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.hpp"
#include "pair_scan.hpp"
#include "scvx_hip.h"

namespace scvx {

// a track's per-obstacle constants: n clamped into 1..M_max (nothing is read outside the obstacle's own knots
// whatever n_knots holds), t0 and w = (n - 1) / (t1 - t0); one knot: t0 = w = 0, the window is not read
struct Track { const double* kn; int n; double t0, w; };
__device__ __forceinline__ Track track_of(const double* __restrict__ knots, const int32_t* __restrict__ n_knots,
                                          const double* __restrict__ window, int M_max, int o) {
    Track tr;
    tr.kn = knots + (long long)o * M_max * 3;
    tr.n = min(max((int)n_knots[o], 1), M_max);
    tr.t0 = tr.n > 1 ? window[o * 2LL] : 0.0;
    tr.w = tr.n > 1 ? (double)(tr.n - 1) / (window[o * 2LL + 1] - tr.t0) : 0.0;
    return tr;
}

// u = clamp((t - t0) w, 0, n - 1): the position along the knots at the lane's sample time t = dt idx.  Product,
// difference and product are rounded one by one (contraction off): the walk and the recomputation at the end, which
// the compiler schedules differently, then agree bit for bit, and a host restatement reproduces them
__device__ __forceinline__ double track_param(const Track& tr, double dt, int idx) {
#pragma clang fp contract(off)
    const double t = dt * (double)idx;
    const double x = t - tr.t0;
    return fmin(fmax(x * tr.w, 0.0), (double)(tr.n - 1));
}

// q(t) = c_m + (u - m)(c_{m+1} - c_m), m = min(floor(u), n - 2); one knot: c_0 exactly (u = 0, c_{m+1} = c_m)
__device__ __forceinline__ void track_point(const Track& tr, double dt, int idx, double (&q)[3]) {
    const double u = track_param(tr, dt, idx);
    const int m = max(min((int)u, tr.n - 2), 0);
    const double fr = u - (double)m;
    const double* a = tr.kn + m * 3;
    const double* b = tr.kn + min(m + 1, tr.n - 1) * 3;
#pragma unroll
    for (int e = 0; e < 3; ++e) q[e] = fma(fr, b[e] - a[e], a[e]);
}

// sorted insertion of (vv, o, s, a) into a list kept descending in (v, then ascending o): a candidate moves ahead of
// a kept one only when strictly larger; vv = -inf moves nothing
template <int JM>
__device__ __forceinline__ void keep_insert(double (&kv)[JM], double (&ka)[JM], int (&ko)[JM], int (&ks)[JM], double vv,
                                            int o, int s, double a) {
#pragma unroll
    for (int r = JM - 1; r > 0; --r) {
        const bool shift = vv > kv[r - 1], here = !shift && vv > kv[r];
        kv[r] = shift ? kv[r - 1] : (here ? vv : kv[r]);
        ka[r] = shift ? ka[r - 1] : (here ? a : ka[r]);
        ko[r] = shift ? ko[r - 1] : (here ? o : ko[r]);
        ks[r] = shift ? ks[r - 1] : (here ? s : ks[r]);
    }
    const bool first = vv > kv[0];
    kv[0] = first ? vv : kv[0];
    ka[0] = first ? a : ka[0];
    ko[0] = first ? o : ko[0];
    ks[0] = first ? s : ks[0];
}

template <int S, int JM>
__global__ __launch_bounds__(64) void moving_obstacle_scan_kernel(
    long long lanes, int K, const double* __restrict__ P, const double* __restrict__ sigma, int O, int M_max,
    const double* __restrict__ knots, const int32_t* __restrict__ n_knots, const double* __restrict__ window,
    const double* __restrict__ rho, double cull, int J, double* __restrict__ dist, double* __restrict__ alpha,
    double* __restrict__ rec, int32_t* __restrict__ obs, double* __restrict__ rec_alpha, int32_t* __restrict__ count,
    double* __restrict__ node_rec, int32_t* __restrict__ node_obs, int32_t* __restrict__ node_count) {
    constexpr int W = (S + 1) * 3;
    const long long l = (long long)blockIdx.x * 64 + threadIdx.x;   // (agent, segment) = l / (K-1), l % (K-1)
    if (l >= lanes) return;                                         // no barrier below
    const long long ag = l / (K - 1);
    const int k = (int)(l - ag * (K - 1));
    const double dt = sigma[ag] / (double)((K - 1) * S);            // the lane's clock: sample s is at dt (k S + s)
    const int s0 = k * S;
    const double* own = P + l * W;
    double p[W];
#pragma unroll
    for (int e = 0; e < W; ++e) p[e] = own[e];
    // the kept lists, descending in (v, then ascending o); empty slots hold -inf.  Segment records: (v, o, s, a);
    // node records: (v, o)
    double kv[JM], ka[JM], nv[JM];
    int ko[JM], ks[JM], no[JM];
#pragma unroll
    for (int r = 0; r < JM; ++r) { kv[r] = nv[r] = -INFINITY; ka[r] = 0.0; ko[r] = no[r] = -1; ks[r] = 0; }
#pragma unroll 1
    for (int o = 0; o < O; ++o) {
        const Track tr = track_of(knots, n_knots, window, M_max, o);   // wave-uniform
        const double ro = rho[o];
        double bq = INFINITY, ba = 0.0, q0 = 0.0;
        int bs = 0;
        // the walk of obstacle_scan_kernel on d_s = p_s - q(t_s); point(s, q) is track_point at the lane's t_s
        auto walk = [&](auto&& point) {
            double q[3];
            point(0, q);
            double d0[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
            q0 = sq3(d0[0], d0[1], d0[2]);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                point(s + 1, q);
                const double d1[3] = {p[(s + 1) * 3] - q[0], p[(s + 1) * 3 + 1] - q[1], p[(s + 1) * 3 + 2] - q[2]};
                const Approach m = chord_closest(d0, d1);
                const bool take = m.q < bq;
                bq = take ? m.q : bq;
                ba = take ? m.al : ba;
                bs = take ? s : bs;
                d0[0] = d1[0]; d0[1] = d1[1]; d0[2] = d1[2];
            }
        };
        if (tr.n <= 2) {
            // m = 0 for every sample: both knots through uniform loads, c_1 - c_0 once (track_point's expressions)
            const double* b = tr.kn + (tr.n - 1) * 3;
            const double c0 = tr.kn[0], c1 = tr.kn[1], c2 = tr.kn[2];
            const double e0 = b[0] - c0, e1 = b[1] - c1, e2 = b[2] - c2;
            walk([&](int s, double (&q)[3]) {
                const double fr = track_param(tr, dt, s0 + s);   // u - m with m = 0
                q[0] = fma(fr, e0, c0); q[1] = fma(fr, e1, c1); q[2] = fma(fr, e2, c2);
            });
        } else {
            walk([&](int s, double (&q)[3]) { track_point(tr, dt, s0 + s, q); });
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
            keep_insert<JM>(kv, ka, ko, ks, (inner && bq > 0.0 && v > -cull) ? v : -INFINITY, o, bs, ba);
        }
        if (node_rec) {   // the segment's first node: sample 0
            const double v = ro - sqrt(q0);
            const double vv = (q0 > 0.0 && v > -cull) ? v : -INFINITY;
#pragma unroll
            for (int r = JM - 1; r > 0; --r) {
                const bool shift = vv > nv[r - 1], here = !shift && vv > nv[r];
                nv[r] = shift ? nv[r - 1] : (here ? vv : nv[r]);
                no[r] = shift ? no[r - 1] : (here ? o : no[r]);
            }
            const bool first = vv > nv[0];
            nv[0] = first ? vv : nv[0];
            no[0] = first ? o : no[0];
        }
    }
    if (rec) {
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
            const double* x = own + s * 3;
            const Track tr = track_of(knots, n_knots, window, M_max, ko[r]);
            double qa[3], qb[3];
            track_point(tr, dt, s0 + s, qa);
            track_point(tr, dt, s0 + s + 1, qb);
            const double d0[3] = {x[0] - qa[0], x[1] - qa[1], x[2] - qa[2]};
            const double d1[3] = {x[3] - qb[0], x[4] - qb[1], x[5] - qb[2]};
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
    if (node_rec) {
        int n = 0;
#pragma unroll
        for (int r = 0; r < JM; ++r) {
            if (r >= J) break;
            double* out = node_rec + (l * J + r) * 4;
            if (no[r] < 0) {
                out[0] = out[1] = out[2] = out[3] = 0.0;
                node_obs[l * J + r] = -1;
                continue;
            }
            ++n;
            const Track tr = track_of(knots, n_knots, window, M_max, no[r]);
            double q[3];
            track_point(tr, dt, s0, q);
            const double d0[3] = {own[0] - q[0], own[1] - q[1], own[2] - q[2]};
            const double ds = sqrt(sq3(d0[0], d0[1], d0[2]));
            out[0] = d0[0] / ds;
            out[1] = d0[1] / ds;
            out[2] = d0[2] / ds;
            out[3] = rho[no[r]] - ds;
            node_obs[l * J + r] = no[r];
        }
        node_count[l] = n;
    }
}

// One lane per (local agent a, node t < K-1): behind the count[a][t] rows already present, the node records of
// segment t (its first node is node t).  Row (g, b) in the form the QP consumes, b - g' p_t <= S_t:
// b = v + g . pbar_t, summed left to right without contraction so that a host restatement reproduces it exactly
// (collision_rows_append_kernel's statement).  Rows that do not fit j_max are counted, never written.
__global__ __launch_bounds__(256) void node_rows_append_kernel(int K, int pd, int nx, int N_local,
                                                               const double* __restrict__ X_all, int i0,
                                                               const int32_t* __restrict__ idx, int J,
                                                               const double* __restrict__ node_rec,
                                                               const int32_t* __restrict__ node_count, int j_max,
                                                               double* __restrict__ rows, int32_t* __restrict__ count,
                                                               int32_t* __restrict__ overflow) {
#pragma clang fp contract(off)
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long long)N_local * (K - 1)) return;
    const long long a = tid / (K - 1);
    const int t = (int)(tid - a * (K - 1));
    const long long gi = idx ? (long long)idx[a] : i0 + a;
    const long long o = (gi - i0) * (K - 1) + t;  // the agent's slot in node_rec / node_count
    const double* p = X_all + (gi * K + t) * nx;
    double* out = rows + (a * K + t) * (long long)j_max * (pd + 1);
    int n = count[a * K + t], over = 0;
    const int m = min(max((int)node_count[o], 0), J);
    for (int r = 0; r < m; ++r) {
        if (n >= j_max) { ++over; continue; }
        const double* q = node_rec + (o * J + r) * 4;
        double b = q[3];
        for (int d = 0; d < pd; ++d) {
            out[n * (pd + 1) + d] = q[d];
            b = b + q[d] * p[d];
        }
        out[n * (pd + 1) + pd] = b;
        ++n;
    }
    count[a * K + t] = n;
    if (over) atomicAdd(overflow, over);
}

template <int S>
static int launch_moving_scan(long long lanes, int K, const double* P, const double* sigma, int O, int M_max,
                              const double* knots, const int32_t* n_knots, const double* window, const double* rho,
                              double cull, int J, double* dist, double* alpha, double* rec, int32_t* obs,
                              double* rec_alpha, int32_t* count, double* node_rec, int32_t* node_obs,
                              int32_t* node_count, hipStream_t st) {
    const dim3 grid((unsigned)((lanes + 63) / 64));
#define SCVX_MOV_LAUNCH(JM)                                                                                        \
    hipLaunchKernelGGL((moving_obstacle_scan_kernel<S, JM>), grid, dim3(64), 0, st, lanes, K, P, sigma, O, M_max, \
                       knots, n_knots, window, rho, cull, J, dist, alpha, rec, obs, rec_alpha, count, node_rec,   \
                       node_obs, node_count)
    if (J <= 2) {   // J = 0 (analysis only) runs the smallest list class with the lists switched off
        SCVX_MOV_LAUNCH(2);
    } else if (J <= 4) {
        SCVX_MOV_LAUNCH(4);
    } else {
        SCVX_MOV_LAUNCH(8);
    }
#undef SCVX_MOV_LAUNCH
    return check_launch("moving_obstacle_scan_kernel");
}

}  // namespace scvx

using namespace scvx;

extern "C" int scvx_moving_obstacle_scan_batched(int K, int S, int N, const double* P, const double* sigma, int O,
                                                 int M_max, const double* knots, const int32_t* n_knots,
                                                 const double* window, const double* rho, double cull, int J,
                                                 double* dist, double* alpha, double* rec, int32_t* obs,
                                                 double* rec_alpha, int32_t* count, double* node_rec,
                                                 int32_t* node_obs, int32_t* node_count, void* stream) {
    const bool ana = dist && alpha, ana_none = !dist && !alpha;
    const bool recs = rec && obs && rec_alpha && count, recs_none = !rec && !obs && !rec_alpha && !count;
    const bool nodes = node_rec && node_obs && node_count, nodes_none = !node_rec && !node_obs && !node_count;
    if (K < 2 || S < 1 || S > 16 || N < 0 || O < 1 || M_max < 1 || J < 0 || J > 8 || !P || !sigma || !knots ||
        !n_knots || !window || !rho || !(ana || ana_none) || !(recs || recs_none) || !(nodes || nodes_none) ||
        (ana_none && recs_none && nodes_none) || (recs || nodes) != (J >= 1) ||
        ((recs || nodes) && (K > 64 || !(cull > 0.0))))
        return set_error(SCVX_EINVAL, "moving_obstacle_scan: bad args");
    const long long lanes = (long long)N * (K - 1);
    if (lanes == 0) return SCVX_OK;
    if ((lanes + 63) / 64 > 0x7fffffffLL || (long long)(K - 1) * S > 0x7fffffffLL)
        return set_error(SCVX_EINVAL, "moving_obstacle_scan: bad args (N (K-1) too large)");
    return dispatch_S(S, "moving_obstacle_scan", [&](auto tag) {
        return launch_moving_scan<decltype(tag)::S>(lanes, K, P, sigma, O, M_max, knots, n_knots, window, rho, cull, J,
                                                    dist, alpha, rec, obs, rec_alpha, count, node_rec, node_obs,
                                                    node_count, (hipStream_t)stream);
    });
}

extern "C" int scvx_node_rows_append_batched(int K, int pos_dim, int n_x, int N_total, const double* X_all, int i0,
                                             const int32_t* idx, int N_local, int J, const double* node_rec,
                                             const int32_t* node_count, int j_max, double* rows, int32_t* count,
                                             int32_t* overflow, void* stream) {
    if (K < 2 || K > 64 || pos_dim < 1 || pos_dim > 3 || pos_dim > n_x || N_total < 0 || N_local < 0 || i0 < 0 ||
        i0 > N_total || (!idx && i0 + (long long)N_local > N_total) || J < 1 || J > 8 || j_max < 1 || j_max > 32 ||
        !X_all || !node_rec || !node_count || !rows || !count || !overflow)
        return set_error(SCVX_EINVAL, "node_rows_append: bad args");
    if (N_local == 0) return SCVX_OK;
    const long long total = (long long)N_local * (K - 1);
    hipLaunchKernelGGL(node_rows_append_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, K, pos_dim, n_x, N_local, X_all, i0, idx, J, node_rec, node_count, j_max,
                       rows, count, overflow);
    return check_launch("node_rows_append_kernel");
}
