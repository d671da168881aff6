// The hipRTC layer of csrc/rtc_common.hpp.  The headers that run-time compiles may include -- the integrator bodies
// user models are compiled against (foh_rtc.hip) and everything the subproblem kernels include
// (subproblem_rtc.hip) -- are embedded here as text at build time: the Makefile's RTC_HEADERS is the one list of
// them, build/rtc_headers.inc the table it generates ({include name, text} per header).
#include "rtc_common.hpp"

#ifndef SCVX_OFFLOAD_ARCH
#define SCVX_OFFLOAD_ARCH "gfx950"
#endif
#include <hip/hiprtc.h>

#include <cstring>

#include "common.hpp"

namespace scvx {
namespace rtc {
namespace {

struct Header {
    const char* name;
    const char* text;
};
const Header kHeaders[] = {
#include "rtc_headers.inc"
};
constexpr int kNumHeaders = (int)(sizeof(kHeaders) / sizeof(kHeaders[0]));

int fail(int code, const char* who, const std::string& what) {
    return set_error(code, (std::string(who) + ": " + what).c_str());
}

}  // namespace

int compile(const char* who, const std::string& src, const char* name, const char* expr, std::vector<char>* code,
            std::string* log, std::string* lowered, size_t log_cut) {
    const char *hsrc[kNumHeaders], *hname[kNumHeaders];
    for (int i = 0; i < kNumHeaders; ++i) { hsrc[i] = kHeaders[i].text; hname[i] = kHeaders[i].name; }
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), name, kNumHeaders, hsrc, hname) != HIPRTC_SUCCESS)
        return fail(SCVX_EINVAL, who, "hiprtcCreateProgram failed");
    if (expr) hiprtcAddNameExpression(prog, expr);
    const char* opts[] = {"--offload-arch=" SCVX_OFFLOAD_ARCH, "-O3", "-std=c++17"};
    const hiprtcResult rc = hiprtcCompileProgram(prog, 3, opts);
    size_t ls = 0;
    log->clear();
    if (hiprtcGetProgramLogSize(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        log->resize(ls);
        hiprtcGetProgramLog(prog, &(*log)[0]);
        log->resize(std::strlen(log->c_str()));
    }
    std::string err;
    if (rc != HIPRTC_SUCCESS) {
        err = std::string("compile") + (expr ? std::string(" of ") + expr : "") + " failed: " +
              hiprtcGetErrorString(rc) + "\n" + log->substr(0, log_cut);
    } else {
        const char* low = nullptr;
        if (expr && lowered && (hiprtcGetLoweredName(prog, expr, &low) != HIPRTC_SUCCESS || !low)) {
            err = "kernel name not found";
        } else {
            if (low) *lowered = low;
            size_t cs = 0;
            hiprtcGetCodeSize(prog, &cs);
            code->resize(cs);
            hiprtcGetCode(prog, code->data());
            if (cs == 0) err = "empty code object";
        }
    }
    hiprtcDestroyProgram(&prog);
    return err.empty() ? SCVX_OK : fail(SCVX_EINVAL, who, err);
}

int Modules::function(const char* who, const std::vector<char>& code, const char* name, hipFunction_t* f) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(SCVX_ELAUNCH, who, "no HIP device");
    std::lock_guard<std::mutex> g(mu_);
    Loaded& L = loaded_[dev];
    if (!L.mod) {
        const hipError_t e = hipModuleLoadData(&L.mod, code.data());
        if (e != hipSuccess) {
            loaded_.erase(dev);
            return fail(SCVX_ELAUNCH, who, std::string("hipModuleLoadData: ") + hipGetErrorString(e));
        }
    }
    auto it = L.fn.find(name);
    if (it == L.fn.end()) {
        hipFunction_t fn = nullptr;
        if (hipModuleGetFunction(&fn, L.mod, name) != hipSuccess)
            return fail(SCVX_ELAUNCH, who, std::string("kernel ") + name + " missing from the code object");
        it = L.fn.emplace(name, fn).first;
    }
    *f = it->second;
    return SCVX_OK;
}

void Modules::unload_all() {
    std::lock_guard<std::mutex> g(mu_);
    if (loaded_.empty()) return;  // nothing was launched: no HIP call (a model compiled on a host without a GPU)
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto& kv : loaded_) {
        (void)hipSetDevice(kv.first);
        (void)hipModuleUnload(kv.second.mod);
    }
    (void)hipSetDevice(cur);
    loaded_.clear();
}

int launch(const char* what, hipFunction_t f, unsigned grid, unsigned block, size_t lds, hipStream_t st, void** args) {
    const hipError_t e = hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, (unsigned)lds, st, args, nullptr);
    if (e != hipSuccess)
        return set_error(SCVX_ELAUNCH, (std::string(what) + " launch: " + hipGetErrorString(e)).c_str());
    return SCVX_OK;
}

}  // namespace rtc
}  // namespace scvx
