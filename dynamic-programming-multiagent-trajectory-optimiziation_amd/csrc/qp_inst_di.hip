// QP kernel instantiations for the di model (n=6, m=3); classes: qp_caps.hpp SCVX_CAPS_DI.
#include "qp_inst.hpp"

namespace scvx {

// Pins of the layout (qp_layout.hpp): the factor block and the K = 50 LDS bytes of three classes, worked out from the
// formulas as they stood before the layout was stated once (DESIGN §3.3 quotes the first pair).  With
// even(x) = x rounded up to even; base = 2 n^2 + 4 n m + m^2 + n, the LDS packet without D and the facet weights;
// LDS(K) = l_var + K n + (K + 1) n + (n <= 8 ? 8 n^2 : 0), l_var = even(f_end + 2 n^2 + 8 n + 5) + 16 + (n <= 8 ? 128 NR : 0),
// f_end = even(packet + 5 n^2 + 5 n m + m^2 + max(n, 8) + 4 NV n):
//  <6,3,2,8,0,0> (C3, obstacles): blocks 18 18 9+1 18 36 36 6 36 = 178, junk slot -> even(179) = 180;
//      packet 159, f_end = even(159 + 279 + 8) = 446, NR = 8 + 4 + 8 + 8 = 28, l_var = even(571) + 16 + 3584 = 4172,
//      LDS(50) = 4172 + 300 + 306 + 288 = 5066 doubles = 40528 B
//  <6,3,2,0,8,0> (coupled, stiff facets: PM = 2, NFD = 8 + 2 + 3 = 13): 178 + Gamma 12 + Gamma_kappa 12 +
//      (W 6 | C^-1 4 | indices 2) = 214, junk slot -> even(215) = 216;
//      packet 159 + 13 = 172, f_end = even(172 + 279 + 8) = 460, NR = 8 + 4 + 8 + 1 = 21,
//      l_var = even(585) + 16 + 2688 = 3290, LDS(50) = 3290 + 606 + 288 = 4184 doubles = 33472 B
//  <12,4,4,8,8,1> (quadrotor, virtual control: NV = 12): blocks 48 48 16 48 144 144 12 144 = 604, + 4 x 144 = 1180,
//      junk slot -> even(1181) = 1182;
//      packet 288 + 192 + 16 + 12 + 12 = 520, f_end = even(520 + 720 + 240 + 16 + 12 + 576) = 2084,
//      l_var = even(2084 + 288 + 96 + 5) + 16 = 2490 (rows in workspace columns), LDS(50) = 2490 + 600 + 612 = 3702
//      doubles = 29616 B
static_assert(QPCfg<6, 3, 2, 8, 0, 0>::L.FBS == 180 && QPCfg<6, 3, 2, 8, 0, 0>::L.lds_doubles(50) * 8 == 40528, "layout moved");
static_assert(QPCfg<6, 3, 2, 0, 8, 0>::L.FBS == 216 && QPCfg<6, 3, 2, 0, 8, 0>::L.lds_doubles(50) * 8 == 33472, "layout moved");
static_assert(QPCfg<12, 4, 4, 8, 8, 1>::L.FBS == 1182 && QPCfg<12, 4, 4, 8, 8, 1>::L.lds_doubles(50) * 8 == 29616, "layout moved");

int qp_launch_di(int idx, const QPArgs& a, hipStream_t st) {
    return QPDispatch<6, 3, 0, SCVX_CAPS_DI>::launch(idx, a, st);
}
// the instantiation qp_launch_di takes for class idx (QP_INST_*), without launching
int qp_select_di(int idx, const scvx_qp_template& T, bool tracing) {
    return QPDispatch<6, 3, 0, SCVX_CAPS_DI>::select(idx, T, tracing);
}

}  // namespace scvx
