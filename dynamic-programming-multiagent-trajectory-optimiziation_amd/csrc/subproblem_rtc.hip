// Runtime-compiled subproblem kernels for user models (hipRTC, the library's own ARCH).
//
// The FOH of any model is runtime-compiled from its expressions (csrc/foh_rtc.hip).  The convex subproblems
// that consume it -- the trust-region QP of Distributed_opt/dist_scvx_3d.py:51-111 (csrc/qp_ipm.hpp) and the
// SCProblem LP/SOCP of SCvx/optimization/sc_problem.py:15-83 (csrc/scp_kernel.hpp) -- do not depend on the
// model's dynamics, only on its dimensions (n_x, n_u) and the template's row counts.  A template with
// model_id = SCVX_MODEL_RUNTIME is therefore served by the same kernel source, instantiated by hipRTC for
// exactly its (n_x, n_u, rows) at the first solve: the headers are embedded in the library as text at build
// time (csrc/rtc_common.hip), so built-in and user classes run one kernel.  Code objects are cached
// per instantiation for the life of the process (and per device once loaded); a compile costs ~10 s once per process.
// This file names the instantiations and keeps that cache; compiling, loading and launching are the library's hipRTC
// layer (csrc/rtc_common.hpp).
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "rtc_common.hpp"
#include "scvx_hip.h"
#include "subproblem_rtc.hpp"
#include "wave_ops.hpp"

namespace {

constexpr const char* kWho = "subproblem rtc";

struct Instance {
    std::vector<char> code;
    std::string lowered, log;
    scvx::rtc::Modules mods;  // never unloaded: an instance lives for the process
};

std::mutex g_mu;
std::map<std::string, std::unique_ptr<Instance>> g_cache;

// the instantiation of a QP class <nx, nu, nb, no, nc, vc> / an SCP class <nx, nu, ne, nw>
struct Inst {
    std::string key, expr;
    const char* header;
};
Inst qp_inst(int nx, int nu, int nb, int no, int nc, int vc) {
    const std::string cls = std::to_string(nx) + ", " + std::to_string(nu) + ", " + std::to_string(nb) + ", " +
                            std::to_string(no) + ", " + std::to_string(nc) + ", " + std::to_string(vc);
    return {"qp<" + cls + ">", "scvx::qp_ipm_kernel<scvx::QPCfg<" + cls + ">>", "qp_ipm.hpp"};
}
Inst scp_inst(int nx, int nu, int ne, int nw) {
    const std::string cls = std::to_string(nx) + ", " + std::to_string(nu) + ", " + std::to_string(ne) + ", " +
                            std::to_string(nw);
    return {"scp<" + cls + ">", "scvx::scp_ipm_kernel<" + cls + ">", "scp_kernel.hpp"};
}

// the compiled instance of `i`, compiled at its first use (the compiler's log cut to 2000 characters in the error)
int compile_inst(const Inst& i, Instance** out) {
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_cache.find(i.key);
    if (it == g_cache.end()) {
        auto inst = std::make_unique<Instance>();
        if (int rc = scvx::rtc::compile(kWho, std::string("#include \"") + i.header + "\"\n", "scvx_subproblem_rtc.hip",
                                        i.expr.c_str(), &inst->code, &inst->log, &inst->lowered, 2000))
            return rc;
        it = g_cache.emplace(i.key, std::move(inst)).first;
    }
    *out = it->second.get();
    return SCVX_OK;
}

int launch(const Inst& i, void** args, unsigned grid, unsigned block, size_t lds, hipStream_t st) {
    if (lds > 65536) return scvx::set_error(SCVX_EUNSUPPORTED, "subproblem rtc: class needs more than 64 KiB of LDS");
    Instance* in = nullptr;
    if (int rc = compile_inst(i, &in)) return rc;
    hipFunction_t f = nullptr;
    if (int rc = in->mods.function(kWho, in->code, in->lowered.c_str(), &f)) return rc;
    return scvx::rtc::launch(kWho, f, grid, block, lds, st, args);
}

}  // namespace

namespace scvx {

int rtc_qp_launch(const QPArgs& a, int nb, int no, int nc, int vc, hipStream_t st) {
    const int nx = a.T.n_x, nu = a.T.n_u;
    const size_t lds = sizeof(double) * (size_t)qp_layout(nx, nu, nb, no, nc, vc).lds_doubles(a.T.K);
    QPArgs copy = a;
    void* args[] = {&copy};
    return launch(qp_inst(nx, nu, nb, no, nc, vc), args, (unsigned)a.N, WAVE, lds, st);
}

int rtc_scp_launch(const SCPArgs& a, int ne, int nw, hipStream_t st) {
    SCPArgs copy = a;
    double* ws = a.ws;
    const double* disc = a.disc;
    void* args[] = {&copy, &ws, &disc};   // scp_ipm_kernel(SCPArgs a, double* ws_all, const double* disc_all)
    return launch(scp_inst(a.T.n_x, a.T.n_u, ne, nw), args, (unsigned)a.N, WAVE * nw, 0, st);
}

}  // namespace scvx

extern "C" int scvx_rtc_subproblem_compile(int kind, const int* cls, int ncls, size_t* code_bytes) {
    if (!cls || (kind == 0 && ncls != 6) || (kind == 1 && ncls != 4) || kind < 0 || kind > 1)
        return scvx::set_error(SCVX_EINVAL, "scvx_rtc_subproblem_compile: kind 0 takes 6 class ints, kind 1 takes 4");
    for (int i = 0; i < ncls; ++i)
        if (cls[i] < 0 || cls[i] > 64) return scvx::set_error(SCVX_EINVAL, "scvx_rtc_subproblem_compile: class out of range");
    // the solve entry points' own limits (qp_layout.hpp, subproblem_rtc.hpp), checked before a ~10 s compile
    const char* bad = kind == 0 ? scvx::qp_class_error(cls[0], cls[1], cls[2], cls[3], cls[4], cls[5], 2)
                                : scvx::rtc_scp_class_error(cls[0], cls[1], cls[2]);
    if (bad) return scvx::set_error(SCVX_EUNSUPPORTED, bad);
    const Inst i = kind == 0 ? qp_inst(cls[0], cls[1], cls[2], cls[3], cls[4], cls[5])
                             : scp_inst(cls[0], cls[1], cls[2], cls[3]);
    Instance* in = nullptr;
    if (int rc = compile_inst(i, &in)) return rc;
    if (code_bytes) *code_bytes = in->code.size();
    return SCVX_OK;
}
