// Instantiation helper: one translation unit per model (parallel builds).
#pragma once
#include "qp_caps.hpp"
#include "qp_ipm.hpp"

namespace scvx {

// K-specialised instantiations (qp_ipm_kernel's KC): the classes below are also compiled with the node count as a
// constant, in a translation unit of their own (qp_inst_di_k50.hip).  K = 50 is the reference's horizon
// (dist_scvx_3d.py) and fixed for the life of a problem; the three classes are the double-integrator ones without
// coupling rows, with obstacles, and with 8 collision rows.
template <class C> struct QPKSpec { static constexpr int K = 0; };
template <> struct QPKSpec<QPCfg<6, 3, 2, 0, 0, 0>> { static constexpr int K = 50; };
template <> struct QPKSpec<QPCfg<6, 3, 2, 8, 0, 0>> { static constexpr int K = 50; };
template <> struct QPKSpec<QPCfg<6, 3, 2, 0, 8, 0>> { static constexpr int K = 50; };
extern template int qp_launch<QPCfg<6, 3, 2, 0, 0, 0>, 50>(const QPArgs&, hipStream_t);
extern template int qp_launch<QPCfg<6, 3, 2, 8, 0, 0>, 50>(const QPArgs&, hipStream_t);
extern template int qp_launch<QPCfg<6, 3, 2, 0, 8, 0>, 50>(const QPArgs&, hipStream_t);
// true: every solve runs the runtime-K instantiation (environment variable SCVX_QP_GENERIC_K set to anything but
// "" or "0"; read at every launch, so one process can compare the two instantiations).  qp_capi.hip
bool qp_force_generic_k();

// Flag-specialised instantiations (qp_ipm_kernel's F, qp_ipm.hpp QPFlags): the three K = 50 classes above are also
// compiled with the problem flags of the templates that bench.py c2 / c3 / c4 launch (the reference's subproblem,
// dist_scvx_3d.py: hard terminal state, last input fixed, no rows at the last node, a box on x and y; c3 adds the
// input cone and 8 obstacles, c4 the collision rows), in qp_inst_di_k50f.hip.
//                                                     FIN FIXU INEQL SOC COLL NOBS NBOX B0 B1
template <class C> struct QPFSpec { using F = QPFlagsRT; };
template <> struct QPFSpec<QPCfg<6, 3, 2, 0, 0, 0>> { using F = QPFlags<1, 1, 0, 0, 0, 0, 2, 0, 1>; };
template <> struct QPFSpec<QPCfg<6, 3, 2, 8, 0, 0>> { using F = QPFlags<1, 1, 0, 1, 0, 8, 2, 0, 1>; };
template <> struct QPFSpec<QPCfg<6, 3, 2, 0, 8, 0>> { using F = QPFlags<1, 1, 0, 0, 1, 0, 2, 0, 1>; };
extern template int qp_launch<QPCfg<6, 3, 2, 0, 0, 0>, 50, QPFSpec<QPCfg<6, 3, 2, 0, 0, 0>>::F>(const QPArgs&, hipStream_t);
extern template int qp_launch<QPCfg<6, 3, 2, 8, 0, 0>, 50, QPFSpec<QPCfg<6, 3, 2, 8, 0, 0>>::F>(const QPArgs&, hipStream_t);
extern template int qp_launch<QPCfg<6, 3, 2, 0, 8, 0>, 50, QPFSpec<QPCfg<6, 3, 2, 0, 8, 0>>::F>(const QPArgs&, hipStream_t);
// true: no solve runs a flag-specialised instantiation (SCVX_QP_GENERIC_FLAGS, read like SCVX_QP_GENERIC_K)
bool qp_force_generic_flags();

// true where the template states, field for field, what F fixes at compile time: the kernel reads none of these
// fields in that instantiation, so each one it would have read is compared here.  (has_final / fix_last_input /
// ineq_last / has_soc are truth values in the kernel; j_max enters the flags only as j_max > 0, the row count per
// node stays run-time data; w_final, w_prox and w_nu must be off: QPFlags has no soft terminal, proximal term or
// virtual control.)
template <class F>
bool qp_flags_match(const scvx_qp_template& T) {
    if (!F::spec) return false;
    if ((T.has_final != 0) != (F::has_final != 0)) return false;
    if ((T.fix_last_input != 0) != (F::fix_last_input != 0)) return false;
    if ((T.ineq_last != 0) != (F::ineq_last != 0)) return false;
    if ((T.has_soc != 0) != (F::has_soc != 0)) return false;
    if ((T.j_max > 0) != (F::has_coll != 0)) return false;
    if (T.n_obs != F::n_obs || T.n_box != F::n_box) return false;
    for (int b = 0; b < F::n_box; ++b)
        if (T.box_idx[b] != F::box_idx(b)) return false;
    if (T.w_final > 0.0 || T.w_prox > 0.0 || T.w_nu > 0.0) return false;
    return true;
}

// The instantiation of class C a solve of template T runs (`tracing`: a diagnostics buffer is set, scvx_qp_set_trace):
//   QP_INST_GENERIC  K and the flags at run time
//   QP_INST_K        K at compile time where the template's K matches a compiled one
//   QP_INST_KF       K and the flags at compile time: T matches the class's QPFSpec as well (qp_flags_match) and no
//                    trace is set (that instantiation carries no diagnostics)
enum { QP_INST_GENERIC = 0, QP_INST_K = 1, QP_INST_KF = 2 };
template <class C>
int qp_select(const scvx_qp_template& T, bool tracing) {
    if (QPKSpec<C>::K == 0 || T.K != QPKSpec<C>::K || qp_force_generic_k()) return QP_INST_GENERIC;
    using F = typename QPFSpec<C>::F;
    constexpr bool lever = (QP_INSN_STEPS & 1) != 0;
    if (lever && (!tracing || QP_SPEC_TRACE) && !qp_force_generic_flags() && qp_flags_match<F>(T)) return QP_INST_KF;
    return QP_INST_K;
}

template <class C>
int qp_launch_class(const QPArgs& a, hipStream_t st) {
    if constexpr (QPKSpec<C>::K > 0) {
        const int inst = qp_select<C>(a.T, a.trace != nullptr);
        if constexpr (QPFSpec<C>::F::spec) {
            if (inst == QP_INST_KF) return qp_launch<C, QPKSpec<C>::K, typename QPFSpec<C>::F>(a, st);
        }
        if (inst != QP_INST_GENERIC) return qp_launch<C, QPKSpec<C>::K>(a, st);
    }
    return qp_launch<C>(a, st);
}

// launch class `idx` of the table (compile-time list of QPCfg)
template <int NX, int NU, int IDX, int NB, int NO, int NC, int VC, int... REST>
struct QPDispatch {
    static int launch(int idx, const QPArgs& a, hipStream_t st) {
        if (idx == IDX) return qp_launch_class<QPCfg<NX, NU, NB, NO, NC, VC>>(a, st);
        return QPDispatch<NX, NU, IDX + 1, REST...>::launch(idx, a, st);
    }
    static int select(int idx, const scvx_qp_template& T, bool tracing) {
        if (idx == IDX) return qp_select<QPCfg<NX, NU, NB, NO, NC, VC>>(T, tracing);
        return QPDispatch<NX, NU, IDX + 1, REST...>::select(idx, T, tracing);
    }
};
template <int NX, int NU, int IDX, int NB, int NO, int NC, int VC>
struct QPDispatch<NX, NU, IDX, NB, NO, NC, VC> {
    static int launch(int idx, const QPArgs& a, hipStream_t st) {
        if (idx == IDX) return qp_launch_class<QPCfg<NX, NU, NB, NO, NC, VC>>(a, st);
        return set_error(SCVX_EUNSUPPORTED, "qp: no row-capacity class");
    }
    static int select(int idx, const scvx_qp_template& T, bool tracing) {
        return idx == IDX ? qp_select<QPCfg<NX, NU, NB, NO, NC, VC>>(T, tracing) : QP_INST_GENERIC;
    }
};

}  // namespace scvx
