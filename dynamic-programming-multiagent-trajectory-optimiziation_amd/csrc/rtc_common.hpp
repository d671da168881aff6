// The library's one hipRTC layer (csrc/rtc_common.hip): the embedded header table, compile, the per-device module
// and function cache, launch.  Its users keep what is theirs: csrc/foh_rtc.hip generates a user model's source and
// owns the scvx_rtc_model handle, csrc/subproblem_rtc.hip names the QP / SCP instantiations and caches them by key.
//
// Every function reports through set_error with the caller's prefix `who` ("rtc", "subproblem rtc") and returns the
// code: SCVX_EINVAL for a failed compile, SCVX_ELAUNCH for a failed load or launch.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace scvx {
namespace rtc {

// Compiles `src` (program `name`) for the library's own target (the Makefile's ARCH: a code object loads where the
// library runs) with every embedded header visible; needs no GPU.  expr (or nullptr): a name expression, whose
// lowered name goes to *lowered.  *log receives the compiler's log whatever the outcome; a failed compile's message
// carries its first log_cut characters.
int compile(const char* who, const std::string& src, const char* name, const char* expr, std::vector<char>* code,
            std::string* log, std::string* lowered = nullptr, size_t log_cut = std::string::npos);

// The modules of one code object: loaded on a device at the first request there (hipModuleLoadData), functions
// looked up once per device and name.  Thread-safe.
class Modules {
  public:
    int function(const char* who, const std::vector<char>& code, const char* name, hipFunction_t* f);
    void unload_all();  // every module, on its own device
  private:
    struct Loaded {
        hipModule_t mod = nullptr;
        std::map<std::string, hipFunction_t> fn;
    };
    std::mutex mu_;
    std::map<int, Loaded> loaded_;  // device -> module
};

// hipModuleLaunchKernel of a one-dimensional grid; a failure is reported as "<what> launch: <HIP's error string>"
int launch(const char* what, hipFunction_t f, unsigned grid, unsigned block, size_t lds, hipStream_t st, void** args);

}  // namespace rtc
}  // namespace scvx
