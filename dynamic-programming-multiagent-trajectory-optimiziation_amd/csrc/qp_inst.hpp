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

// the class's K-specialised instantiation where the template's K matches one, else the runtime-K one
template <class C>
int qp_launch_class(const QPArgs& a, hipStream_t st) {
    if constexpr (QPKSpec<C>::K > 0) {
        if (a.T.K == QPKSpec<C>::K && !qp_force_generic_k()) return qp_launch<C, QPKSpec<C>::K>(a, st);
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
};
template <int NX, int NU, int IDX, int NB, int NO, int NC, int VC>
struct QPDispatch<NX, NU, IDX, NB, NO, NC, VC> {
    static int launch(int idx, const QPArgs& a, hipStream_t st) {
        if (idx == IDX) return qp_launch_class<QPCfg<NX, NU, NB, NO, NC, VC>>(a, st);
        return set_error(SCVX_EUNSUPPORTED, "qp: no row-capacity class");
    }
};

}  // namespace scvx
