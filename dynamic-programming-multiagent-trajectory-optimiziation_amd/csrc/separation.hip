// Fleet separation analysis (gfx950, float64): how close any two agents of a finished run come, at the
// nodes and between them.
//
//   rollout_dense_kernel      dense samples of every segment's nonlinear roll-out (positions + polyline length)
//   separation_scan_kernel    continuous-time agent-agent closest approach on those samples (the hot path)
//   pair_min_kernel           node-level pairwise minimum distance, SCvx/utils/analysis.py:10-31
//   obstacle_min_kernel       node-level agent-obstacle clearance, SCvx/utils/analysis.py:34-62
//
// The scan's mapping, tile staging and chord closest approach are csrc/pair_scan.hpp's, shared with the collision rows
// (intersample_rows.hip); its accuracy: within max ||r''|| h^2 / 8 of the true minimum (h = the sub-interval, r the
// relative position).  Here: the selection and the skip rule.
//
// Selection: squared distances (one sqrt at the end), replaced only on strictly smaller, in the order j ascending,
// s ascending: the first minimum, whatever the launch geometry.
//
// Chunk skip: when the bound |d(s=0)| - (L_i + L_j), held back by PS_SKIP_MARGIN, exceeds the lane's current
// minimum (or the sample-0 distance to a block mate, which the final minimum cannot exceed) for every neighbour of a
// chunk in every lane (wave ballot), the chunk is skipped: none of its candidates could have been the first minimum, so
// the outputs are bit-identical to the unpruned scan (flags bit 0 selects it, for the test of exactly that).  Measured
// 4.4x faster at the C4 shape and 1.7x at C3.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "common.hpp"
#include "models.hpp"
#include "pair_scan.hpp"
#include "scvx_hip.h"

namespace scvx {

// one lane per (agent, segment): rollout_dense_body (foh_body.hpp), shared with the runtime-compiled user models
template <class Mdl>
__global__ __launch_bounds__(64) void rollout_dense_kernel(const double* __restrict__ X, const double* __restrict__ U,
                                                           const double* __restrict__ sigma, double* __restrict__ P,
                                                           double* __restrict__ L, int K, int N, int S, int sub,
                                                           int pd, ModelParams Pm) {
    rollout_dense_body<Mdl>(X, U, sigma, P, L, K, N, S, sub, pd, Pm);
}

template <int S, bool PRUNE>
__global__ __launch_bounds__(64) void separation_scan_kernel(int K, int N_total, int N_local,
                                                             const double* __restrict__ P_all,
                                                             const double* __restrict__ L_all, int i0,
                                                             double* __restrict__ sep, int32_t* __restrict__ arg,
                                                             double* __restrict__ alpha) {
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
    double best = INFINITY, balpha = 0.0;
    int bj = -1, bs = -1;
    // an upper bound of the lane's final minimum before the scan has met a near neighbour: the sample-0 distance
    // to the closest other agent of this block (index neighbours are often spatial neighbours, e.g. on a lattice)
    double ub = INFINITY;
    if (PRUNE) {
        __shared__ double blk[64 * 3];
#pragma unroll
        for (int d = 0; d < 3; ++d) blk[lane * 3 + d] = pi[d];
        __syncthreads();
        const int nb = (int)min(64LL, N_local - (long long)blockIdx.x * 64);
        for (int l = 0; l < nb; ++l) {
            const double x0 = pi[0] - blk[l * 3], x1 = pi[1] - blk[l * 3 + 1], x2 = pi[2] - blk[l * 3 + 2];
            ub = l == lane ? ub : fmin(ub, sq3(x0, x1, x2));
        }
    }
    for (int j0 = 0; j0 < N_total; j0 += PS_TJ) {
        const int nt = stage_tile<S, PRUNE>(tile, tileL, P_all, L_all, j0, N_total, K, k, lane);
        for (int jb = 0; jb < nt; jb += PS_CH) {
            if (PRUNE) {
                // d(s=0)^2 > ((sqrt(min(best, ub)) + L_i + L_j) (1 + margin))^2: every chord of the pair is longer
                // than the kept minimum or than the block mate's that will replace it (strictly: a coincident
                // block mate, ub = 0 and L = 0, is itself not skipped)
                const double sb = sqrt(fmin(best, ub));
                bool need = false;
#pragma unroll
                for (int c = 0; c < PS_CH; ++c) {
                    const double* pj = tile + (jb + c) * W;
                    const double x0 = pi[0] - pj[0], x1 = pi[1] - pj[1], x2 = pi[2] - pj[2];
                    const double r = (sb + Li + tileL[jb + c]) * (1.0 + PS_SKIP_MARGIN);
                    need |= !(sq3(x0, x1, x2) > r * r);
                }
                if (!__builtin_amdgcn_ballot_w64(need && live)) continue;
            }
            // one neighbour at a time: its S sub-intervals are independent work enough, and unrolling the chunk as
            // well would hold PS_CH sets of samples in registers next to the lane's own (spills at S >= 8)
#pragma unroll 1
            for (int c = 0; c < PS_CH; ++c) {
                const int j = j0 + jb + c;
                const bool ok = live && j < N_total && j != gi;
                const double* pj = tile + (jb + c) * W;
                double d0[3];
                rel_pos(pi, pj, 0, d0);
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    double d1[3];
                    rel_pos(pi, pj, s + 1, d1);
                    const Approach m = chord_closest(d0, d1);
                    const bool take = ok && m.q < best;
                    best = take ? m.q : best;
                    balpha = take ? m.al : balpha;
                    bj = take ? j : bj;
                    bs = take ? s : bs;
                    d0[0] = d1[0]; d0[1] = d1[1]; d0[2] = d1[2];
                }
            }
        }
    }
    if (!live) return;
    const long long o = a * (K - 1) + k;
    sep[o] = sqrt(best);
    arg[o * 2] = bj;
    arg[o * 2 + 1] = bs;
    alpha[o] = balpha;
}

// D[i][j] = min_k ||X_i[0:rows, k] - X_j[0:rows, k]||.  One workgroup (256 threads) per 64 x 64 tile of pairs:
// lane = j of the tile, each of the 4 waves takes 16 of the tile's i.  The node positions of both agent blocks
// are staged in LDS a chunk of PM_KC nodes at a time: the j block as [node][row][agent] (consecutive lanes on
// consecutive doubles), the i block as [node][agent][row], read as broadcasts.  (a - b)^2 == (b - a)^2 in
// floating point and the rows are summed in one order, so D is symmetric with an exact zero diagonal although
// every entry is computed on its own.
constexpr int PM_KC = 8;

__global__ __launch_bounds__(256) void pair_min_kernel(int K, int nx, int rows, int N, const double* __restrict__ X,
                                                       double* __restrict__ D) {
    __shared__ double Pj[PM_KC * 3 * 64];
    __shared__ double Pi[PM_KC * 64 * 3];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long long ib = (long long)blockIdx.y * 64, jb = (long long)blockIdx.x * 64;
    double m2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) m2[r] = INFINITY;
    for (int k0 = 0; k0 < K; k0 += PM_KC) {
        const int nk = min(PM_KC, K - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < nk * 3 * 64; e += 256) {
            const int kk = e / 192, rem = e - kk * 192;
            {   // j block: e = (kk, d, agent)
                const int d = rem / 64, ag = rem - d * 64;
                Pj[e] = (d < rows && jb + ag < N) ? X[((jb + ag) * K + k0 + kk) * nx + d] : 0.0;
            }
            {   // i block: e = (kk, agent, d)
                const int ag = rem / 3, d = rem - ag * 3;
                Pi[e] = (d < rows && ib + ag < N) ? X[((ib + ag) * K + k0 + kk) * nx + d] : 0.0;
            }
        }
        __syncthreads();
        for (int kk = 0; kk < nk; ++kk) {
            const double q0 = Pj[(kk * 3 + 0) * 64 + tx], q1 = Pj[(kk * 3 + 1) * 64 + tx], q2 = Pj[(kk * 3 + 2) * 64 + tx];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double* p = Pi + (kk * 64 + ty * 16 + r) * 3;
                const double d0 = p[0] - q0, d1 = p[1] - q1, d2 = p[2] - q2;
                m2[r] = fmin(m2[r], fma(d2, d2, fma(d1, d1, d0 * d0)));
            }
        }
    }
    const long long j = jb + tx;
    if (j >= N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long i = ib + ty * 16 + r;
        if (i < N) D[i * N + j] = sqrt(m2[r]);
    }
}

// D[i][o] = min_k (||X_i[0:3, k] - c_o|| - (robot_radius + r_o)); one lane per (agent, obstacle)
__global__ __launch_bounds__(256) void obstacle_min_kernel(int K, int nx, int N, const double* __restrict__ X,
                                                           int n_obs, const double* __restrict__ centers,
                                                           const double* __restrict__ radii, double robot_radius,
                                                           double* __restrict__ D) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long long)N * n_obs) return;
    const long long i = tid / n_obs;
    const int o = (int)(tid - i * n_obs);
    const double c0 = centers[o * 3], c1 = centers[o * 3 + 1], c2 = centers[o * 3 + 2];
    double m2 = INFINITY;
    for (int k = 0; k < K; ++k) {
        const double* p = X + (i * K + k) * nx;
        const double d0 = p[0] - c0, d1 = p[1] - c1, d2 = p[2] - c2;
        m2 = fmin(m2, fma(d2, d2, fma(d1, d1, d0 * d0)));
    }
    // sqrt and the subtraction of a constant are monotone, so the minimum commutes with them
    D[tid] = sqrt(m2) - (robot_radius + radii[o]);
}

template <class Mdl>
static int launch_rollout_dense(const double* X, const double* U, const double* sigma, double* P, double* L, int K,
                                int N, int S, int sub, int pd, const ModelParams& Pm, hipStream_t st) {
    if (const char* bad = rollout_dense_check(K, N, S, sub, pd, Mdl::N, X, U, sigma, P, L))
        return set_error(SCVX_EINVAL, bad);
    if (N == 0) return SCVX_OK;
    const long long total = (long long)N * (K - 1);
    hipLaunchKernelGGL(rollout_dense_kernel<Mdl>, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, X, U, sigma, P,
                       L, K, N, S, sub, pd, Pm);
    return check_launch("rollout_dense_kernel");
}

template <int S>
static int launch_scan(int K, int N_total, const double* P_all, const double* L_all, int i0, int N_local, double* sep,
                       int32_t* arg, double* alpha, int flags, hipStream_t st) {
    const dim3 grid((unsigned)((N_local + 63) / 64), (unsigned)(K - 1));
    if (flags & 1)
        hipLaunchKernelGGL((separation_scan_kernel<S, false>), grid, dim3(64), 0, st, K, N_total, N_local, P_all, L_all,
                           i0, sep, arg, alpha);
    else
        hipLaunchKernelGGL((separation_scan_kernel<S, true>), grid, dim3(64), 0, st, K, N_total, N_local, P_all, L_all,
                           i0, sep, arg, alpha);
    return check_launch("separation_scan_kernel");
}

}  // namespace scvx

using namespace scvx;

extern "C" int scvx_rollout_dense_batched(int model_id, const double* params, int K, int N, const double* X,
                                          const double* U, const double* sigma, int S, int sub, int pos_dim, double* P,
                                          double* L, void* stream) {
    // the rules that need no model first (n_x = 0), so that a bad argument is SCVX_EINVAL whatever the model id; the
    // launcher repeats the check with the model's n_x
    if (const char* bad = rollout_dense_check(K, N, S, sub, pos_dim, 0, X, U, sigma, P, L))
        return set_error(SCVX_EINVAL, bad);
    if (model_id == SCVX_MODEL_RUNTIME)
        return set_error(SCVX_EUNSUPPORTED,
                         "rollout_dense: a runtime-compiled model goes through scvx_rtc_rollout_dense_batched");
    const ModelParams Pm = model_params(model_id, params);
    return dispatch_model(model_id, "rollout_dense", [&](auto tag) {
        return launch_rollout_dense<typename decltype(tag)::type>(X, U, sigma, P, L, K, N, S, sub, pos_dim, Pm,
                                                                  (hipStream_t)stream);
    });
}

extern "C" int scvx_separation_scan_batched(int K, int S, int N_total, const double* P_all, const double* L_all, int i0,
                                            int N_local, double* sep, int32_t* arg, double* alpha, int flags,
                                            void* stream) {
    if (!pair_scan_args_ok(K, INT_MAX, S, N_total, N_local, i0, flags, P_all, L_all) || !sep || !arg || !alpha)
        return set_error(SCVX_EINVAL, "separation_scan: bad args");
    if (N_local == 0) return SCVX_OK;
    return dispatch_S(S, "separation_scan", [&](auto tag) {
        return launch_scan<decltype(tag)::S>(K, N_total, P_all, L_all, i0, N_local, sep, arg, alpha, flags,
                                             (hipStream_t)stream);
    });
}

extern "C" int scvx_pair_min_distance_batched(int K, int n_x, int rows, int N, const double* X, double* D,
                                              void* stream) {
    if (K < 1 || n_x < 1 || rows < 1 || rows > 3 || rows > n_x || N < 0 || !X || !D)
        return set_error(SCVX_EINVAL, "pair_min_distance: bad args");
    if (N == 0) return SCVX_OK;
    const unsigned nb = (unsigned)((N + 63) / 64);
    if (nb > 65535) return set_error(SCVX_EUNSUPPORTED, "pair_min_distance: more than 65535 x 64 agents");
    hipLaunchKernelGGL(pair_min_kernel, dim3(nb, nb), dim3(256), 0, (hipStream_t)stream, K, n_x, rows, N, X, D);
    return check_launch("pair_min_kernel");
}

extern "C" int scvx_obstacle_min_distance_batched(int K, int n_x, int N, const double* X, int n_obs,
                                                  const double* centers, const double* radii, double robot_radius,
                                                  double* D, void* stream) {
    if (K < 1 || n_x < 3 || N < 0 || n_obs < 0 || !X || !D || (n_obs > 0 && (!centers || !radii)))
        return set_error(SCVX_EINVAL, "obstacle_min_distance: bad args");
    if (N == 0 || n_obs == 0) return SCVX_OK;
    const long long total = (long long)N * n_obs;
    hipLaunchKernelGGL(obstacle_min_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, K,
                       n_x, N, X, n_obs, centers, radii, robot_radius, D);
    return check_launch("obstacle_min_kernel");
}
