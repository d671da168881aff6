// The pair scan's core (gfx950, float64), stated once for separation_scan_kernel (separation.hip, the diagnosis) and
// intersample_pair_rows_kernel (intersample_rows.hip, the collision rows): a record's dist and alpha' are bit for bit
// the scan's closest approach of the same pair because both run the expressions below.
//
// Frame: one workgroup of 64 lanes per (segment k, block of 64 local agents), lane = local agent, its own S+1 samples
// in registers.  All lanes walk the same neighbours j = 0..N_total-1: a tile of PS_TJ neighbours' samples is staged in
// LDS per workgroup (stage_tile) and read back as broadcasts, PS_CH neighbours to a chunk.
// Chords: agents are compared at EQUAL normalised time.  Between two samples the relative position is d0 + a e,
// e = d1 - d0, a in [0, 1]; chord_closest is its clamped projection, exact for the piecewise-linear interpolant.  A
// kernel walks a pair's S chords in order (d1 becomes the next d0) and applies its own selection to their (s, a, q).
// Skip tests: a pair stays within L_i + L_j (the segments' polyline lengths) of d(s=0), so none of its chords is
// shorter than |d(s=0)| - (L_i + L_j).  A kernel compares sq3 of the sample-0 difference with
// ((its reach + L_i + L_j) (1 + PS_SKIP_MARGIN))^2; the reach is its own rule.
// The own-sample load, the chord walk and the sample-0 difference stay in the kernels: as functions of this header
// they changed the compiled code (occupancy, +1..4 % time).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "common.hpp"

namespace scvx {

constexpr int PS_TJ = 32;  // neighbours staged per LDS tile: 32 x 51 doubles = 12.75 KiB at S = 16
constexpr int PS_CH = 4;   // neighbours per chunk (the unit of a skip); a tile is a whole number of chunks
// d(s=0), L and the reach each carry a few ulp (1e-16 relative to the pair's distance): four orders below the margin
constexpr double PS_SKIP_MARGIN = 1e-12;

// |x|^2 in one order everywhere: a chord's |e|^2 and |c|^2, |d(s=0)|^2 of the skip tests and of the block-mate bound
__device__ __forceinline__ double sq3(double x0, double x1, double x2) { return fma(x2, x2, fma(x1, x1, x0 * x0)); }

// d = the relative position of a pair at sample s (pi, pj: the samples of the two agents' segment)
__device__ __forceinline__ void rel_pos(const double* pi, const double* pj, int s, double (&d)[3]) {
    d[0] = pi[s * 3] - pj[s * 3]; d[1] = pi[s * 3 + 1] - pj[s * 3 + 1]; d[2] = pi[s * 3 + 2] - pj[s * 3 + 2];
}

// c = d0 + al e, the relative position at al of the chord from d0 along e
__device__ __forceinline__ void chord_point(const double (&d0)[3], double e0, double e1, double e2, double al,
                                            double (&c)[3]) {
    c[0] = fma(al, e0, d0[0]); c[1] = fma(al, e1, d0[1]); c[2] = fma(al, e2, d0[2]);
}

// the closest approach of the chord d0 -> d1 to the origin: al the clamped minimiser of |d0 + a (d1 - d0)| on [0, 1],
// q the squared distance there
struct Approach { double al, q; };
__device__ __forceinline__ Approach chord_closest(const double (&d0)[3], const double (&d1)[3]) {
    const double e0 = d1[0] - d0[0], e1 = d1[1] - d0[1], e2 = d1[2] - d0[2];
    const double ee = sq3(e0, e1, e2);
    const double de = fma(d0[2], e2, fma(d0[1], e1, d0[0] * e0));
    const double al = ee == 0.0 ? 0.0 : fmin(fmax(-de / ee, 0.0), 1.0);
    double c[3];
    chord_point(d0, e0, e1, e2, al, c);
    return {al, sq3(c[0], c[1], c[2])};
}

// c of a reported (s, al): qi, qj point at sample s of the two agents (sample s+1 follows)
__device__ __forceinline__ void approach_point(const double* qi, const double* qj, double al, double (&c)[3]) {
    double d0[3], d1[3];
    rel_pos(qi, qj, 0, d0);
    rel_pos(qi, qj, 1, d1);
    chord_point(d0, d1[0] - d0[0], d1[1] - d0[1], d1[2] - d0[2], al, c);
}

// stages neighbours j0 .. j0 + PS_TJ - 1 of segment k (tile [PS_TJ][W], tileL [PS_TJ] with PRUNE) between two
// barriers and returns how many exist; slots past that hold zeros and are never selected (the kernels test
// j < N_total)
template <int S, bool PRUNE>
__device__ __forceinline__ int stage_tile(double* tile, double* tileL, const double* __restrict__ P_all,
                                          const double* __restrict__ L_all, int j0, int N_total, int K, int k,
                                          int lane) {
    constexpr int W = (S + 1) * 3;
    const int nt = min(PS_TJ, N_total - j0);
    __syncthreads();
    for (int e = lane; e < PS_TJ * W; e += 64) {
        const int jj = e / W;
        tile[e] = jj < nt ? P_all[((long long)(j0 + jj) * (K - 1) + k) * W + (e - jj * W)] : 0.0;
    }
    if (PRUNE && lane < PS_TJ) tileL[lane] = lane < nt ? L_all[(long long)(j0 + lane) * (K - 1) + k] : 0.0;
    __syncthreads();
    return nt;
}

// host side: the arguments both entry points share (K_max: the caller's upper bound on K)
inline bool pair_scan_args_ok(int K, int K_max, int S, int N_total, int N_local, int i0, int flags, const double* P_all,
                              const double* L_all) {
    return K >= 2 && K <= K_max && S >= 1 && S <= 16 && N_total >= 0 && N_local >= 0 && i0 >= 0 &&
           i0 + (long long)N_local <= N_total && !(flags & ~1) && P_all && L_all;
}

// host side: the one switch from a run-time S in 1..16 to a compile-time one (as dispatch_model, models.hpp).  Calls
// fn(STag<S>{}) and returns its result; any other S is SCVX_EINVAL "<who>: bad args"
template <int S_>
struct STag { static constexpr int S = S_; };
template <class Fn>
inline int dispatch_S(int S, const char* who, Fn&& fn) {
    switch (S) {
#define PS_CASE(s) case s: return fn(STag<s>{});
        PS_CASE(1) PS_CASE(2) PS_CASE(3) PS_CASE(4) PS_CASE(5) PS_CASE(6) PS_CASE(7) PS_CASE(8)
        PS_CASE(9) PS_CASE(10) PS_CASE(11) PS_CASE(12) PS_CASE(13) PS_CASE(14) PS_CASE(15) PS_CASE(16)
#undef PS_CASE
        default: return set_error(SCVX_EINVAL, (std::string(who) + ": bad args").c_str());
    }
}

}  // namespace scvx
