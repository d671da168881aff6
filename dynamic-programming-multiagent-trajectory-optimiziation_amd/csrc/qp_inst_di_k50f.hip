// QP kernel instantiations for the di model (n=6, m=3) with K = 50 and the problem flags at compile time
// (qp_inst.hpp QPFSpec: the templates of bench.py c2 / c3 / c4); their runtime-flag twins are in qp_inst_di_k50.hip.
#include "qp_inst.hpp"

namespace scvx {

template int qp_launch<QPCfg<6, 3, 2, 0, 0, 0>, 50, QPFSpec<QPCfg<6, 3, 2, 0, 0, 0>>::F>(const QPArgs&, hipStream_t);
template int qp_launch<QPCfg<6, 3, 2, 8, 0, 0>, 50, QPFSpec<QPCfg<6, 3, 2, 8, 0, 0>>::F>(const QPArgs&, hipStream_t);
template int qp_launch<QPCfg<6, 3, 2, 0, 8, 0>, 50, QPFSpec<QPCfg<6, 3, 2, 0, 8, 0>>::F>(const QPArgs&, hipStream_t);

}  // namespace scvx
