// Dispatch lists of the split QP launch (include/scvx_hip.h scvx_qp_dispatch_select): a stable counting sort of
// the agents by their previous solve's IPM iterations, descending, cut into a tail list (the first agents with
// iters >= thr, at most T, and at most one per short_per_tail agents below thr) and a bulk list (everyone else, in the
// sorted order).  One workgroup, no atomics: the result is the same on every run.
//
// Agent i belongs to chunk c = i / 64 (one wave pass).  cnt[c][k] counts the chunk's agents with key k; an exclusive
// scan over the chunks per key, then over the keys from the largest down, gives every agent its position:
//   pos(i) = #{key > k_i} + #{j in earlier chunks, key = k_i} + #{j < i in the same chunk, key = k_i}.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "scvx_hip.h"
#include "wave_ops.hpp"

namespace scvx {
namespace {
constexpr int kSelThreads = 1024;
constexpr int kSelTable = 12288;   // ints of LDS for cnt[chunks][bins]

__global__ __launch_bounds__(kSelThreads) void qp_dispatch_select_kernel(int N, const int32_t* __restrict__ iters,
                                                                         int thr, int T, int short_per_tail,
                                                                         int max_iter,
                                                                         int32_t* __restrict__ order_tail,
                                                                         int32_t* __restrict__ order_bulk) {
    extern __shared__ int sel_lds[];
    const int B = max_iter + 1, chunks = (N + WAVE - 1) / WAVE;
    int* cnt = sel_lds;              // [chunks][B]
    int* start = cnt + chunks * B;   // [B]: agents with a larger key
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, waves = kSelThreads / WAVE;
    for (int e = tid; e < chunks * B; e += kSelThreads) cnt[e] = 0;
    __syncthreads();
    // per chunk: the count of every key that occurs in it (one ballot per distinct key)
    for (int c = wave; c < chunks; c += waves) {
        const int i = c * WAVE + lane;
        const int k = i < N ? min(max((int)iters[i], 0), max_iter) : -1;
        unsigned long long todo = __ballot(k >= 0);
        while (todo) {
            const int kk = __shfl(k, __ffsll((long long)todo) - 1);
            const unsigned long long m = __ballot(k == kk);
            if (lane == 0) cnt[c * B + kk] = __popcll(m);
            todo &= ~m;
        }
    }
    __syncthreads();
    // per key: exclusive scan of the counts over the chunks; the key's total lands in start[]
    for (int k = tid; k < B; k += kSelThreads) {
        int run = 0;
        for (int c = 0; c < chunks; ++c) {
            const int v = cnt[c * B + k];
            cnt[c * B + k] = run;
            run += v;
        }
        start[k] = run;
    }
    __syncthreads();
    // start[k] = #{key > k}; n_q = #{key >= thr}
    int above = 0, n_q = 0;
    for (int k = B - 1; k >= 0; --k) {   // (every thread walks the B totals: B broadcast reads; B <= the block size)
        const int v = start[k];
        if (k >= thr) n_q += v;
        if (k > tid) above += v;
    }
    __syncthreads();
    if (tid < B) start[tid] = above;
    __syncthreads();
    // every running tail workgroup displaces short_per_tail bulk workgroups into a second round: only as many tail
    // agents as there are agents below thr to displace (a batch whose agents all qualify has no tail)
    const int n_tail = short_per_tail > 0 ? min(min(T, n_q), (N - n_q) / short_per_tail) : min(T, n_q);
    for (int c = wave; c < chunks; c += waves) {
        const int i = c * WAVE + lane;
        const int k = i < N ? min(max((int)iters[i], 0), max_iter) : -1;
        unsigned long long todo = __ballot(k >= 0);
        const unsigned long long below = (1ull << lane) - 1ull;
        int rank = 0;
        while (todo) {
            const int kk = __shfl(k, __ffsll((long long)todo) - 1);
            const unsigned long long m = __ballot(k == kk);
            if (k == kk) rank = __popcll(m & below);
            todo &= ~m;
        }
        if (k >= 0) {
            const int pos = start[k] + cnt[c * B + k] + rank;
            if (pos < n_tail) order_tail[pos] = i;
            else order_bulk[pos - n_tail] = i;
        }
    }
    for (int e = n_tail + tid; e < T; e += kSelThreads) order_tail[e] = SCVX_QP_ORDER_SKIP;
    for (int e = N - n_tail + tid; e < N; e += kSelThreads) order_bulk[e] = SCVX_QP_ORDER_SKIP;
}
}  // namespace
}  // namespace scvx

using namespace scvx;

extern "C" int scvx_qp_dispatch_select(int N, const int32_t* iters, int thr, int T, int short_per_tail, int max_iter,
                                       int32_t* order_tail, int32_t* order_bulk, void* stream) {
    if (N < 0 || T < 0 || T > N || max_iter < 1 || short_per_tail < 0)
        return set_error(SCVX_EINVAL, "qp dispatch: 0 <= T <= N, short_per_tail >= 0, max_iter >= 1");
    if (N == 0) return SCVX_OK;
    if (!iters || !order_bulk || (T > 0 && !order_tail)) return set_error(SCVX_EINVAL, "qp dispatch: null buffer");
    const long long B = (long long)max_iter + 1, chunks = ((long long)N + WAVE - 1) / WAVE;
    if (B > kSelThreads || chunks * B > kSelTable)
        return set_error(SCVX_EUNSUPPORTED, "qp dispatch: max_iter > 1023 or ceil(N / 64) * (max_iter + 1) > 12288 (the count table)");
    const size_t lds = sizeof(int) * (size_t)(chunks * B + B);
    hipLaunchKernelGGL(qp_dispatch_select_kernel, dim3(1), dim3(kSelThreads), lds, (hipStream_t)stream, N, iters, thr, T,
                       short_per_tail, max_iter, order_tail, order_bulk);
    return check_launch("qp_dispatch_select_kernel");
}
