// Tuning constants of the QP interior point shared by the kernel (csrc/qp_ipm.hpp) and its CPU twin
// (oracle/scvx_cpu.cpp): plain C++, no HIP, so both sides compile this one definition.
#pragma once

namespace scvx {

// warm start: floor of every slack and dual of the previous iterate (scaled units)
constexpr double QP_WARM_ETA = 1e-3;
// ... except that a row's dual floor is min(QP_WARM_ETA, QP_WARM_KAPPA / s) at its recomputed slack s: a row far from
// active (box rows, obstacle rows away from the trajectory: s ~ 1..10) keeps a dual near its last, tiny value instead
// of 1e-3, so the start's complementarity s lambda is ~1e-5 there, not ~1e-2.  The warm solve starts ~100x closer
// to the end game: on the CPU twin over the bench's 25 steps, the slowest agent's IPM iterations summed over the
// timed steps fall 171 -> 132 (per-agent rule) and 240 -> 201 (global rule), seeds 2 and 3 alike
constexpr double QP_WARM_KAPPA = 1e-5;
// stiff trust-region facet: its barrier weight D = lambda / s above QP_STIFF x the largest diagonal entry of the rest
// of the stage's input Hessian Rhat
constexpr double QP_STIFF = 1e6;
// fraction-to-boundary of the end game (affine step >= 0.99).  In the warm-started Jacobi loop almost every
// solve is an end game from its first iteration: each step is a full Newton step up to this fraction, so
// the gap falls by 1 / (1 - QP_TAU_END) per iteration.  0.999 took the C3 bulk 5 iterations, 1 - 1e-5 takes
// it 3 (1 - 1e-6 lengthened the tail: measured on the twin over the bench's 25 steps)
constexpr double QP_TAU_END = 0.99999;

}  // namespace scvx
