// The element-parallel phases of the QP kernel's factor sweep (csrc/qp_ipm.hpp): packed per-lane descriptors, their
// decoded forms and the phase that evaluates them.  The kernel builds the descriptors; nothing here knows its state.
// (Also compiled at run time for user models: csrc/subproblem_rtc.hip.)
#pragma once
#include "qp_access.hpp"
#include "wave_ops.hpp"

namespace scvx {

// packed phase descriptors (all operands are contiguous LDS vectors; the stage packet always sits at
// F_RING, so every offset is stage-invariant):
//   operand = LDS offset (15 bits)
//   output  = LDS offset | accumulate << 15 | (global column + 1) << 17
//   base    = LDS offset | kind << 16   (kind 0: none, 1: always, 2: last stage)

// One lane's repetition of a factor phase, decoded once per sweep (the offsets are stage-invariant)
struct QPRep {
    int L, R, B, O, G;   // LDS operand / base / output offsets; byte voffset of the global store
    double b1, b2, acc;  // base multipliers (every stage, last stage only); 1 if the output accumulates
};
// lsink: LDS sink (outputs that go nowhere in LDS, and accumulating outputs, which live in registers
// during the sweep); jnk: the junk slot of the stage block
__device__ __forceinline__ QPRep qp_decode(const int (&d)[4], int one, int lsink, int jnk) {
    QPRep q;
    q.L = d[0] & 0x7FFF;
    q.R = d[1] & 0x7FFF;
    const int bk = d[3] >> 16;
    q.B = bk ? (d[3] & 0x7FFF) : one;
    q.b1 = bk == 1 ? 1.0 : 0.0;
    q.b2 = bk == 2 ? 1.0 : 0.0;
    const int O = d[2];
    const bool on = O >= 0, acc = on && ((O >> 15) & 1);
    q.O = (on && !acc) ? (O & 0x7FFF) : lsink;
    q.acc = acc ? 1.0 : 0.0;
    const int g = on ? (O >> 17) - 1 : -1;
    q.G = (g >= 0 ? g : jnk) * 8;
    return q;
}

template <int KK>
__device__ __forceinline__ double qp_dot(const double* lds, int L, int R) {
    const double* lp = lds + L;
    const double* rp = lds + R;
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        if (k & 1) acc1 = fma(lp[k], rp[k], acc1); else acc0 = fma(lp[k], rp[k], acc0);
    }
    return acc0 + acc1;
}

// Read scheduling of the phases (DESIGN §3.3 "The factor's read batches").  A stage is a chain of dependent LDS
// round trips (issue to use: 50-60 cycles), so what counts is how many read batches sit exposed behind a fence:
//   FS_A  one read batch per phase: the base and operand reads of every repetition are issued first, pinned in use
//         order (the waits stay progressive), then the trees run -- not one batch per repetition
//   FS_C  operands whose sources are final before the previous phase are read before its fence (phase 2's and
//         phase 4's L and base; only R is the previous phase's output), in the split form of FS_A
// (diagnostics builds: -DQP_FS_STEPS=<bits A = 1, C = 2> builds a step alone, tools/build_variant.sh)
#ifndef QP_FS_STEPS
#define QP_FS_STEPS 3
#endif
constexpr int QP_FS_A = 1, QP_FS_C = 2;
// The steps of a class <nx, nu, nb, no, nc> (the kernel's FSM).  The n = 12 classes keep their compact phases
// (qp_phase_c) as they are.  Two classes compile at the limit of the register file and the allocator's result moves
// by a few words with any change of the stage: each keeps the steps under which its scratch size and spill count do
// not exceed those without any step (profiles/factor_static_table.md lists every class before and after).
constexpr int qp_fs_mask(int nx, int nu, int nb, int no, int nc) {
    int m = nx > 8 ? 0 : QP_FS_STEPS;
    if (nx == 3 && nu == 2 && nc == 32) m = 0;                       // <3,2,4,16,32,0>: either step, 2368 -> 2384 B scratch
    if (nx == 6 && nb == 2 && no == 0 && nc == 16) m &= QP_FS_A;     // <6,3,2,0,16,0>: with C, 20 -> 22 VGPR spills
    return m;
}

// the value is in its register here (a read issued before must have landed; reads after stay after)
__device__ __forceinline__ void qp_pin(double& v) { asm volatile("" : "+v"(v)); }

// One lane's operands of a phase, in registers between their issue and the trees
template <int KK, int NREP>
struct QPOps {
    double l[NREP][KK], r[NREP][KK], b[NREP];
};
// Issues the phase's reads.  SEL 3: everything, in use order; 1: L and the base (sources final before the previous
// phase's fence: the caller says which phase wrote them last); 2: R, behind that fence.
template <int SEL, int KK, int NREP>
__device__ __forceinline__ void qp_phase_issue(const double* lds, const QPRep (&d)[NREP], QPOps<KK, NREP>& o) {
#pragma unroll
    for (int r = 0; r < NREP; ++r) {
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            if (SEL & 1) o.l[r][k] = lds[d[r].L + k];
            if (SEL & 2) o.r[r][k] = lds[d[r].R + k];
        }
        if (SEL & 1) o.b[r] = lds[d[r].B];
    }
}
// The trees (qp_dot's: even terms in acc0, odd ones in acc1, acc0 + acc1, then the base) and the writes of a phase
// whose reads are out.
template <int KK, int NREP, int ALO, int AHI>
__device__ __forceinline__ void qp_phase_finish(double* lds, const QPRep (&d)[NREP], double blast, const QPBuf& wb, int fbo,
                                                double (&areg)[NREP], QPOps<KK, NREP>& o) {
    double val[NREP];
#pragma unroll
    for (int r = 0; r < NREP; ++r) {
        double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            qp_pin(o.l[r][k]);
            qp_pin(o.r[r][k]);
            if (k & 1) acc1 = fma(o.l[r][k], o.r[r][k], acc1); else acc0 = fma(o.l[r][k], o.r[r][k], acc0);
        }
        qp_pin(o.b[r]);
        val[r] = fma(o.b[r], d[r].b1 + blast * d[r].b2, acc0 + acc1);
    }
#pragma unroll
    for (int r = 0; r < NREP; ++r) {
        lds[d[r].O] = val[r];
        if (WAVE * r < AHI && WAVE * r + WAVE > ALO) areg[r] = fma(d[r].acc, val[r], areg[r]);
        wb.st(d[r].G, fbo, val[r]);
    }
}

// One element-parallel phase of the factor sweep: every lane evaluates its NREP repetitions
// (out = base + sum_k L[k] R[k]), writes each to its LDS slot and its global column, and adds the
// accumulating ones (M, xe: summed over the stages) into registers -- no LDS read-modify-write on the
// sweep's chain.
// (outputs [ALO, AHI) of the phase may accumulate: only the repetitions covering them keep a register sum)
template <int FSM, int KK, int NREP, int ALO = 0, int AHI = WAVE * NREP>
__device__ __forceinline__ void qp_phase(double* lds, const QPRep (&d)[NREP], double blast, const QPBuf& wb, int fbo,
                                         double (&areg)[NREP]) {
    if constexpr ((FSM & QP_FS_A) != 0) {
        QPOps<KK, NREP> o;
        qp_phase_issue<3>(lds, d, o);
        qp_phase_finish<KK, NREP, ALO, AHI>(lds, d, blast, wb, fbo, areg, o);
    } else {   // one read batch per repetition
        double val[NREP];
#pragma unroll
        for (int r = 0; r < NREP; ++r)
            val[r] = fma(lds[d[r].B], d[r].b1 + blast * d[r].b2, qp_dot<KK>(lds, d[r].L, d[r].R));
#pragma unroll
        for (int r = 0; r < NREP; ++r) {
            lds[d[r].O] = val[r];
            if (WAVE * r < AHI && WAVE * r + WAVE > ALO) areg[r] = fma(d[r].acc, val[r], areg[r]);
            wb.st(d[r].G, fbo, val[r]);
        }
    }
}

// Compact repetition (n = 12 classes): the base / accumulate flags packed in F (bits 0-1: base kind 0 none,
// 1 every stage, 2 last stage; bit 2: accumulating output) instead of three doubles, and the accumulating
// outputs keep their LDS target in O (written every stage, overwritten by the register sum after the
// sweep; nothing reads V_M / V_XE during it).  20 repetitions x 6 instead of 11 registers at NX = 12.
// Packed in three registers (round 4: the six-int form held 120 registers across the n = 12 sweep, which
// spilled to scratch inside the stage loop): L | R << 16, B | O << 16, G | F << 16 (LDS offsets < 2^15
// doubles, the global byte offset within a stage block < 2^16).
struct QPRepC {
    int LR, BO, GF;
    __device__ __forceinline__ int L() const { return LR & 0xFFFF; }
    __device__ __forceinline__ int R() const { return LR >> 16; }
    __device__ __forceinline__ int B() const { return BO & 0xFFFF; }
    __device__ __forceinline__ int O() const { return BO >> 16; }
    __device__ __forceinline__ int G() const { return GF & 0xFFFF; }
    __device__ __forceinline__ int F() const { return GF >> 16; }
};
__device__ __forceinline__ QPRepC qp_decode_c(const int (&d)[4], int one, int lsink, int jnk) {
    QPRepC q;
    const int L = d[0] & 0x7FFF, R = d[1] & 0x7FFF;
    const int bk = d[3] >> 16;
    const int B = bk ? (d[3] & 0x7FFF) : one;
    const int O = d[2];
    const bool on = O >= 0, acc = on && ((O >> 15) & 1);
    const int Oo = on ? (O & 0x7FFF) : lsink;
    const int g = on ? (O >> 17) - 1 : -1;
    const int G = (g >= 0 ? g : jnk) * 8;
    const int F = bk | (acc ? 4 : 0);
    q.LR = L | (R << 16);
    q.BO = B | (Oo << 16);
    q.GF = G | (F << 16);
    return q;
}
// as qp_phase; outputs [ALO, AHI) of the phase may accumulate (only those repetitions keep a register sum)
template <int KK, int NREP, int ALO, int AHI>
__device__ __forceinline__ void qp_phase_c(double* lds, const QPRepC* d, double blast, const QPBuf& wb,
                                           int fbo, double (&areg)[NREP]) {
    const QPRepC* q = d;
    double val[NREP];
#pragma unroll
    for (int r = 0; r < NREP; ++r) {
        const int bk = q[r].F() & 3;
        const double bm = (bk == 1 ? 1.0 : 0.0) + blast * (bk == 2 ? 1.0 : 0.0);
        val[r] = fma(lds[q[r].B()], bm, qp_dot<KK>(lds, q[r].L(), q[r].R()));
    }
#pragma unroll
    for (int r = 0; r < NREP; ++r) {
        lds[q[r].O()] = val[r];
        if (WAVE * r < AHI && WAVE * r + WAVE > ALO) areg[r] = fma((q[r].F() & 4) ? 1.0 : 0.0, val[r], areg[r]);
        wb.st(q[r].G(), fbo, val[r]);
    }
}

}  // namespace scvx
