// QP kernel instantiations for the di model (n=6, m=3) with the node count K = 50 at compile time
// (qp_inst.hpp QPKSpec); their runtime-K twins are in qp_inst_di.hip.
#include "qp_inst.hpp"

namespace scvx {

template int qp_launch<QPCfg<6, 3, 2, 0, 0, 0>, 50>(const QPArgs&, hipStream_t);
template int qp_launch<QPCfg<6, 3, 2, 8, 0, 0>, 50>(const QPArgs&, hipStream_t);
template int qp_launch<QPCfg<6, 3, 2, 0, 8, 0>, 50>(const QPArgs&, hipStream_t);

}  // namespace scvx
