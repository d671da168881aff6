// Workspace access and optimiser fences of the batched QP kernel (csrc/qp_ipm.hpp): the raw-buffer accessor of an
// agent's workspace, the opaque-value helpers and the barrier rows' fast division.  Nothing here knows the kernel's
// state.  (Also compiled at run time for user models: csrc/subproblem_rtc.hip.)
#pragma once
#include "qp_layout.hpp"

namespace scvx {

// Agent workspace accessor: raw buffer loads/stores with the lane part of the address in one
// VGPR (voffset) and the column part as a (rematerialisable) SGPR constant (soffset), so no
// per-column 64-bit address is ever materialised in vector registers.
typedef unsigned int qp_u2 __attribute__((ext_vector_type(2)));
typedef unsigned int qp_u4 __attribute__((ext_vector_type(4)));
// Every memory op of the factor sweep is unconditional: lanes with nothing to store write to the
// junk slot of the stage block, and prefetch loads of padding / structurally zero packet elements
// read past the end of the workspace (0).  A load or store under a divergent branch makes the
// compiler's vmcnt accounting fall back to vmcnt(0), which drains the packet prefetches issued
// stages ahead (measured: most of the factor's per-stage time).
struct QPBuf {
    __amdgpu_buffer_rsrc_t rs;
#ifdef QP_BYTE_TRACE
    // diagnostics build (tools/qp_bytes_trace.py): workspace bytes this lane requested since the last region stamp
    // (lanes without a node address QP_OOB and move nothing); the stamps fold them into the trace buffer per region
    mutable double nby = 0.0;
    __device__ __forceinline__ void cnt(int voff, int soff, double b) const {
        nby += (voff < QP_OOB && soff < QP_OOB) ? b : 0.0;
    }
#else
    __device__ __forceinline__ void cnt(int, int, double) const {}
#endif
    __device__ __forceinline__ double ld(int voff, int soff) const {
        soff = __builtin_amdgcn_readfirstlane(soff);  // uniform by construction
        cnt(voff, soff, 8.0);
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0));
    }
    __device__ __forceinline__ void st(int voff, int soff, double v) const {
        soff = __builtin_amdgcn_readfirstlane(soff);
        cnt(voff, soff, 8.0);
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(qp_u2, v), rs, voff, soff, 0);
    }
    __device__ __forceinline__ qp_u4 ld4(int voff, int soff) const {
        soff = __builtin_amdgcn_readfirstlane(soff);
        cnt(voff, soff, 16.0);
        return __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
    }
    __device__ __forceinline__ void st4(int voff, int soff, qp_u4 v) const {
        soff = __builtin_amdgcn_readfirstlane(soff);
        cnt(voff, soff, 16.0);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, voff, soff, 0);
    }
    // A byte offset known at compile time (the K-specialised instantiations: qp_ipm_kernel's KC) is split: its low
    // 12 bits join voffset, where the backend folds a constant addend into the instruction's immediate field, and
    // the 4 KB window above them is the soffset -- one scalar constant shared by every access of the window, no
    // scalar arithmetic per access.  `coff` is the whole constant part of the address (a constant added to `voff`
    // by the caller would overflow the immediate field and cost a vector add).  The range check sees
    // voffset + immediate: a lane without a node (voffset = QP_OOB) stays wholly out of range.
    // The lane offset is made opaque first (not volatile: equal ones still merge): the optimiser otherwise pushes
    // the constant through the select that forms it (node ? t * 8 : QP_OOB) and keeps one precomputed vector
    // register per accessed column live across the whole kernel.
    static constexpr int IMM = 0xFFF;
    static __device__ __forceinline__ int vopq(int v) {
        asm("" : "+v"(v));
        return v;
    }
    __device__ __forceinline__ double ldk(int voff, int coff) const {
        cnt(voff, coff, 8.0);
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, vopq(voff) + (coff & IMM), coff & ~IMM, 0));
    }
    __device__ __forceinline__ qp_u4 ld4k(int voff, int coff) const {
        cnt(voff, coff, 16.0);
        return __builtin_amdgcn_raw_buffer_load_b128(rs, vopq(voff) + (coff & IMM), coff & ~IMM, 0);
    }
    __device__ __forceinline__ void stk(int voff, int coff, double v) const {
        cnt(voff, coff, 8.0);
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(qp_u2, v), rs, vopq(voff) + (coff & IMM), coff & ~IMM, 0);
    }
};
// keep a value opaque to the optimiser (volatile: re-derived where it is used, never hoisted)
__device__ __forceinline__ int qp_opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
// a double made opaque where it is defined (not volatile: it orders nothing).  A product pinned this way stays rounded
// on its own: the backend cannot contract it into a sum that consumes it.
__device__ __forceinline__ double qp_rounded(double v) {
    asm("" : "+v"(v));
    return v;
}
// 1.0 if a == b else 0.0, opaque to the optimiser: selecting an array element by a runtime
// index with this mask stays arithmetic (a compare/select chain is turned back into a
// dynamically indexed private array, i.e. scratch memory)
__device__ __forceinline__ double qp_mask(int a, int b) {
    int m = a == b ? 1 : 0;
    asm("" : "+v"(m));
    return (double)m;
}
// a + b that is never contracted with a product feeding it.  fma(1.0, c, g) rounds c before the sum; written c + g,
// the backend would fuse a c = x * y into fma(x, y, g) and round once (floating-point contraction is on for the
// rest of the kernel), so the compile-time form of a masked accumulation goes through this.
__device__ __forceinline__ double qp_add_nc(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
// a / b for the per-row barrier quantities (l / s, the rows' Newton terms): the hardware reciprocal, two Newton
// steps and a product (~1.5 ulp, six instructions) instead of the correctly rounded division sequence (eleven,
// with a longer dependent chain); these run once per row per phase on every node
__device__ __forceinline__ double qp_div(double a, double b) {
#ifdef QP_EXACT_DIV   // diagnostics build (tools/qp_div_accuracy.py): the correctly rounded division of round 4
    return a / b;
#endif
    double r = __builtin_amdgcn_rcp(b);
    r = fma(fma(-b, r, 1.0), r, r);
    r = fma(fma(-b, r, 1.0), r, r);
    return a * r;
}

}  // namespace scvx
