// Continuous-time (inter-sample) agent-agent collision rows for the Jacobi QP (gfx950, float64): the pair scan of
// separation.hip, turned from a diagnosis into constraints.
//
//   intersample_pair_rows_kernel   per (local agent i, segment k): the J neighbours that come closest strictly
//                                  between the two nodes, as records (g, v, j, alpha')       (the hot path)
//   collision_rows_append_kernel   each record becomes two node rows, behind the node rows of collision.hip
//
// Mapping, tile staging and the chords of a pair are csrc/pair_scan.hpp's, the ones separation_scan_kernel runs.  A
// pair's closest approach on segment k is the first minimum over its S chords (replaced only when strictly
// smaller): c its relative position there, dist = |c|, alpha' = (s + a) / S.  The pair is a
// candidate when dist < cull, 0 < alpha' < 1 (a minimum at a node belongs to the node rows) and dist > 0 (no
// direction otherwise: dropped).  Per (i, k) the J candidates of smallest dist are kept in ascending (dist, j)
// order -- neighbours are scanned j ascending and a candidate moves ahead of a kept one only when strictly
// closer -- so the output does not depend on the launch geometry.  Record: g = c / dist, v = 2R - dist.
//
// Each lane keeps its sorted top-J list (dist^2, j, s, a) in registers; the insertion runs under a wave ballot with
// the running bound "the J-th kept dist^2" (as collision_rows_kernel); c is recomputed once at the end by
// approach_point, the statement the chords use, so dist^2 comes out bit for bit as selected.
//
// Chunk skip: a neighbour whose bound |d(s=0)| - (L_i + L_j) is cull (1 + PS_SKIP_MARGIN) or more is no candidate.
// The threshold is fixed (the scan's moves with the kept minimum): each lane tests the neighbours of a tile once,
// into a bit mask, a chunk is skipped when a wave ballot finds no lane needing any of its neighbours, and the
// outputs are bit-identical to the unpruned kernel (flags bit 0, tests only).
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.hpp"
#include "pair_scan.hpp"
#include "scvx_hip.h"

namespace scvx {

template <int S, int JM, bool PRUNE>
__global__ __launch_bounds__(64) void intersample_pair_rows_kernel(int K, int N_total, int N_local,
                                                                   const double* __restrict__ P_all,
                                                                   const double* __restrict__ L_all, int i0, double R,
                                                                   double cull, int J,
                                                                   double* __restrict__ rec, int32_t* __restrict__ nbr,
                                                                   double* __restrict__ alpha,
                                                                   int32_t* __restrict__ count) {
    constexpr int W = (S + 1) * 3;
    __shared__ double tile[PS_TJ * W];
    __shared__ double tileL[PS_TJ];
    const int lane = threadIdx.x;
    const int k = blockIdx.y;  // segment, < K-1
    const long long a = (long long)blockIdx.x * 64 + lane;
    const bool live = a < N_local;
    const long long gi = live ? i0 + a : -1;
    double pi[W], Li = 0.0;
#pragma unroll
    for (int e = 0; e < W; ++e) pi[e] = live ? P_all[(gi * (K - 1) + k) * W + e] : 0.0;
    if (PRUNE && live) Li = L_all[gi * (K - 1) + k];
    // the kept list, ascending in (dist^2, j); empty slots hold +inf
    double kq[JM], ka[JM];
    int kj[JM], ks[JM];
#pragma unroll
    for (int r = 0; r < JM; ++r) { kq[r] = INFINITY; ka[r] = 0.0; kj[r] = -1; ks[r] = 0; }
    const double cull2 = cull * cull;
    double bound = cull2;  // a candidate enters only below min(cull^2, the J-th kept dist^2)
    for (int j0 = 0; j0 < N_total; j0 += PS_TJ) {
        const int nt = stage_tile<S, PRUNE>(tile, tileL, P_all, L_all, j0, N_total, K, k, lane);
        // the skip test of the whole tile at once, one bit per neighbour: 32 independent chains whose LDS reads
        // overlap (made chunk by chunk, each test waited for its own reads with nothing else to issue)
        uint32_t needmask = 0;
        if (PRUNE) {
#pragma unroll
            for (int jj = 0; jj < PS_TJ; ++jj) {
                const double* pj = tile + jj * W;
                const double x0 = pi[0] - pj[0], x1 = pi[1] - pj[1], x2 = pi[2] - pj[2];
                const double r = (cull + Li + tileL[jj]) * (1.0 + PS_SKIP_MARGIN);
                needmask |= (sq3(x0, x1, x2) >= r * r) ? 0u : (1u << jj);
            }
            needmask = live ? needmask : 0u;
        }
        for (int jb = 0; jb < nt; jb += PS_CH) {
            if (PRUNE && !__builtin_amdgcn_ballot_w64(((needmask >> jb) & ((1u << PS_CH) - 1u)) != 0u)) continue;
#pragma unroll 1
            for (int c = 0; c < PS_CH; ++c) {
                const int j = j0 + jb + c;
                const bool ok = live && j < N_total && j != gi;
                // the pair's own first minimum over its S chords
                double bq = INFINITY, ba = 0.0;
                int bs = 0;
                const double* pj = tile + (jb + c) * W;
                double d0[3];
                rel_pos(pi, pj, 0, d0);
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    double d1[3];
                    rel_pos(pi, pj, s + 1, d1);
                    const Approach m = chord_closest(d0, d1);
                    const bool take = m.q < bq;
                    bq = take ? m.q : bq;
                    ba = take ? m.al : ba;
                    bs = take ? s : bs;
                    d0[0] = d1[0]; d0[1] = d1[1]; d0[2] = d1[2];
                }
                // strictly between the nodes: not (s = 0, a = 0) and not (s = S-1, a = 1)
                const bool inner = (bs > 0 || ba > 0.0) && (bs < S - 1 || ba < 1.0);
                const bool ins = ok && inner && bq > 0.0 && bq < bound;
                if (!__builtin_amdgcn_ballot_w64(ins)) continue;
                if (ins) {
                    // sorted insertion behind every kept entry that is not farther (ties keep the lower j ahead)
#pragma unroll
                    for (int r = JM - 1; r > 0; --r) {
                        const bool shift = bq < kq[r - 1], here = !shift && bq < kq[r];
                        kq[r] = shift ? kq[r - 1] : (here ? bq : kq[r]);
                        ka[r] = shift ? ka[r - 1] : (here ? ba : ka[r]);
                        kj[r] = shift ? kj[r - 1] : (here ? j : kj[r]);
                        ks[r] = shift ? ks[r - 1] : (here ? bs : ks[r]);
                    }
                    const bool first = bq < kq[0];
                    kq[0] = first ? bq : kq[0];
                    ka[0] = first ? ba : ka[0];
                    kj[0] = first ? j : kj[0];
                    ks[0] = first ? bs : ks[0];
#pragma unroll
                    for (int r = 0; r < JM; ++r) bound = (r == J - 1) ? fmin(cull2, kq[r]) : bound;
                }
            }
        }
    }
    if (!live) return;
    const long long o = a * (K - 1) + k;
    int n = 0;
#pragma unroll
    for (int r = 0; r < JM; ++r) {
        if (r >= J) break;
        double* out = rec + (o * J + r) * 4;
        if (kj[r] < 0) {  // unused slots are written too: the whole output is deterministic
            out[0] = out[1] = out[2] = out[3] = 0.0;
            nbr[o * J + r] = -1;
            alpha[o * J + r] = 0.0;
            continue;
        }
        ++n;
        const int s = ks[r];
        const double al = ka[r];
        double cp[3];
        approach_point(P_all + (gi * (K - 1) + k) * W + s * 3,
                       P_all + ((long long)kj[r] * (K - 1) + k) * W + s * 3, al, cp);
        const double dist = sqrt(sq3(cp[0], cp[1], cp[2]));
        out[0] = cp[0] / dist;
        out[1] = cp[1] / dist;
        out[2] = cp[2] / dist;
        out[3] = 2.0 * R - dist;
        nbr[o * J + r] = kj[r];
        alpha[o * J + r] = ((double)s + al) / (double)S;
    }
    count[o] = n;
}

// One lane per (local agent a, node t < K-1): behind the count[a][t] rows already present, the records of
// segment t (the row at the segment's first node), then those of segment t-1 (its second node).  Row (g, b) in
// the form the QP consumes, b - g' p_t <= S_t: b = v + g . pbar_t, summed left to right without contraction so
// that a host restatement reproduces it exactly.  Rows that do not fit j_max are counted, never written.
__global__ __launch_bounds__(256) void collision_rows_append_kernel(int K, int pd, int nx, int N_local,
                                                                    const double* __restrict__ X_all, int i0,
                                                                    const int32_t* __restrict__ idx, int J,
                                                                    const double* __restrict__ rec,
                                                                    const int32_t* __restrict__ count_seg, int j_max,
                                                                    double* __restrict__ rows,
                                                                    int32_t* __restrict__ count,
                                                                    int32_t* __restrict__ overflow) {
#pragma clang fp contract(off)
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long long)N_local * (K - 1)) return;
    const long long a = tid / (K - 1);
    const int t = (int)(tid - a * (K - 1));
    const long long gi = idx ? (long long)idx[a] : i0 + a;
    const long long ra = gi - i0;  // the agent's slot in rec / count_seg
    const double* p = X_all + (gi * K + t) * nx;
    double* out = rows + (a * K + t) * (long long)j_max * (pd + 1);
    int n = count[a * K + t], over = 0;
    for (int side = 0; side < 2; ++side) {
        const int k = t - side;
        if (k < 0) break;
        const long long o = ra * (K - 1) + k;
        const int m = count_seg[o];
        for (int r = 0; r < m; ++r) {
            if (n >= j_max) { ++over; continue; }
            const double* q = rec + (o * J + r) * 4;
            double b = q[3];
            for (int d = 0; d < pd; ++d) {
                out[n * (pd + 1) + d] = q[d];
                b = b + q[d] * p[d];
            }
            out[n * (pd + 1) + pd] = b;
            ++n;
        }
    }
    count[a * K + t] = n;
    if (over) atomicAdd(overflow, over);
}

template <int S>
static int launch_pair_rows(int K, int N_total, const double* P_all, const double* L_all, int i0, int N_local, double R,
                            double cull, int J, double* rec, int32_t* nbr, double* alpha, int32_t* count, int flags,
                            hipStream_t st) {
    const dim3 grid((unsigned)((N_local + 63) / 64), (unsigned)(K - 1));
#define SCVX_ISR_LAUNCH(JM)                                                                                        \
    if (flags & 1)                                                                                                 \
        hipLaunchKernelGGL((intersample_pair_rows_kernel<S, JM, false>), grid, dim3(64), 0, st, K, N_total,        \
                           N_local, P_all, L_all, i0, R, cull, J, rec, nbr, alpha, count);                         \
    else                                                                                                           \
        hipLaunchKernelGGL((intersample_pair_rows_kernel<S, JM, true>), grid, dim3(64), 0, st, K, N_total,         \
                           N_local, P_all, L_all, i0, R, cull, J, rec, nbr, alpha, count)
    if (J <= 2) {
        SCVX_ISR_LAUNCH(2);
    } else if (J <= 4) {
        SCVX_ISR_LAUNCH(4);
    } else {
        SCVX_ISR_LAUNCH(8);
    }
#undef SCVX_ISR_LAUNCH
    return check_launch("intersample_pair_rows_kernel");
}

}  // namespace scvx

using namespace scvx;

extern "C" int scvx_intersample_pair_rows_batched(int K, int S, int N_total, const double* P_all, const double* L_all,
                                                  int i0, int N_local, double R, double cull, int J, double* rec,
                                                  int32_t* nbr, double* alpha, int32_t* count, int flags,
                                                  void* stream) {
    if (!pair_scan_args_ok(K, 64, S, N_total, N_local, i0, flags, P_all, L_all) || J < 1 || J > 8 || !(cull > 0.0) ||
        !(R == R) || !rec || !nbr || !alpha || !count)
        return set_error(SCVX_EINVAL, "intersample_pair_rows: bad args");
    if (N_local == 0) return SCVX_OK;
    return dispatch_S(S, "intersample_pair_rows", [&](auto tag) {
        return launch_pair_rows<decltype(tag)::S>(K, N_total, P_all, L_all, i0, N_local, R, cull, J, rec, nbr, alpha,
                                                  count, flags, (hipStream_t)stream);
    });
}

extern "C" int scvx_collision_rows_append_batched(int K, int pos_dim, int n_x, int N_total, const double* X_all, int i0,
                                                  const int32_t* idx, int N_local, int J, const double* rec,
                                                  const int32_t* count_seg, int j_max, double* rows, int32_t* count,
                                                  int32_t* overflow, void* stream) {
    if (K < 2 || K > 64 || pos_dim < 1 || pos_dim > 3 || pos_dim > n_x || N_total < 0 || N_local < 0 || i0 < 0 ||
        i0 > N_total || (!idx && i0 + (long long)N_local > N_total) || J < 1 || J > 8 || j_max < 1 || j_max > 32 ||
        !X_all || !rec || !count_seg || !rows || !count || !overflow)
        return set_error(SCVX_EINVAL, "collision_rows_append: bad args");
    if (N_local == 0) return SCVX_OK;
    const long long total = (long long)N_local * (K - 1);
    hipLaunchKernelGGL(collision_rows_append_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, K, pos_dim, n_x, N_local, X_all, i0, idx, J, rec, count_seg, j_max, rows,
                       count, overflow);
    return check_launch("collision_rows_append_kernel");
}
