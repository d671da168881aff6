// C-ABI of the batched trust-region QP (include/scvx_hip.h): argument checks, row-capacity class
// selection (qp_caps.hpp), workspace sizing and the launch of the matching qp_ipm_kernel
// instantiation (qp_inst_*.hip).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>

#include "common.hpp"
#include "qp_caps.hpp"
#include "qp_layout.hpp"
#include "scvx_hip.h"
#include "subproblem_rtc.hpp"
#include "wave_ops.hpp"

namespace scvx {
int qp_launch_di(int idx, const QPArgs& a, hipStream_t st);
int qp_launch_unicycle(int idx, const QPArgs& a, hipStream_t st);
int qp_launch_si(int idx, const QPArgs& a, hipStream_t st);
int qp_launch_quad(int idx, const QPArgs& a, hipStream_t st);
int qp_select_di(int idx, const scvx_qp_template& T, bool tracing);
// SCVX_QP_GENERIC_K (qp_inst.hpp): the runtime-K instantiation also where a K-specialised one exists
bool qp_force_generic_k() {
    const char* e = std::getenv("SCVX_QP_GENERIC_K");
    return e && e[0] && !(e[0] == '0' && !e[1]);
}
// SCVX_QP_GENERIC_FLAGS (qp_inst.hpp): the runtime-flag instantiation also where a flag-specialised one matches
bool qp_force_generic_flags() {
    const char* e = std::getenv("SCVX_QP_GENERIC_FLAGS");
    return e && e[0] && !(e[0] == '0' && !e[1]);
}

// Split launch (scvx_qp_solve_batched_split).  Per device: one non-blocking side stream and the fork / join events
// (timing disabled), created at the first split launch and kept for the life of the process.
namespace {
struct SplitDev {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    int lds_cu = 0, lds_wg = 0;   // LDS bytes per compute unit / per workgroup
    int cus = 0;                  // compute units
    bool ok = false, tried = false;
};
constexpr int kMaxDev = 64;
SplitDev g_split[kMaxDev];
std::mutex g_split_mu;
// kernels whose dynamic-LDS limit has been raised to `bytes` (the attribute is set once per kernel and size)
struct SplitAttr { const void* fn; int bytes; };
SplitAttr g_split_attr[32];
int g_split_nattr = 0;
// workgroups of kernel `fn` (one wave, `lds` bytes) a compute unit holds at once, asked once per kernel and size
struct SplitOcc { const void* fn; size_t lds; int blocks; };
SplitOcc g_split_occ[32];
int g_split_nocc = 0;

int split_blocks_per_cu(const void* fn, size_t lds) {
    for (int i = 0; i < g_split_nocc; ++i)
        if (g_split_occ[i].fn == fn && g_split_occ[i].lds == lds) return g_split_occ[i].blocks;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, WAVE, lds) != hipSuccess) {
        (void)hipGetLastError();
        nb = 0;
    }
    if (g_split_nocc < 32) g_split_occ[g_split_nocc++] = {fn, lds, nb};
    return nb;
}

SplitDev* split_dev() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return nullptr;
    SplitDev& d = g_split[dev];
    if (!d.tried) {
        d.tried = true;
        int cu = 0, wg = 0;
        d.ok = hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
               hipDeviceGetAttribute(&cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess &&
               hipDeviceGetAttribute(&wg, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
               hipStreamCreateWithFlags(&d.side, hipStreamNonBlocking) == hipSuccess &&
               hipEventCreateWithFlags(&d.fork, hipEventDisableTiming) == hipSuccess &&
               hipEventCreateWithFlags(&d.join, hipEventDisableTiming) == hipSuccess;
        d.lds_cu = cu; d.lds_wg = wg;
        if (!d.ok) (void)hipGetLastError();
    }
    return d.ok ? &d : nullptr;
}
}  // namespace

// The tail's LDS request: WHOLE -- what is left next to it does not hold one more QP workgroup (lds bytes each);
// HALF -- it holds one and a half, so exactly one fits whatever the allocation granule.  0: no such request exists
// (the kernel's own request already is that large, or exceeds the workgroup limit).
static int split_tail_lds(int reserve, size_t lds, int lds_cu, int lds_wg) {
    const long long room = reserve == SCVX_QP_RESERVE_HALF ? (long long)lds + (long long)lds / 2 : (long long)lds / 2;
    long long req = (long long)lds_cu - room;
    if (req > lds_wg) req = lds_wg;
    if (req < (long long)lds || (long long)lds_cu - req >= (reserve == SCVX_QP_RESERVE_HALF ? 2 : 1) * (long long)lds)
        return 0;
    return (int)(req & ~15LL);
}

int qp_launch_split(const void* fn, const QPArgs& a, size_t lds, hipStream_t st) {
    std::lock_guard<std::mutex> lock(g_split_mu);
    QPArgs bulk = a;
    bulk.tail_n = 0; bulk.order_tail = nullptr;
    void* kargs[] = {(void*)&bulk};
    SplitDev* d = split_dev();
    const int tail_lds = d ? split_tail_lds(a.tail_reserve, lds, d->lds_cu, d->lds_wg) : 0;
    // The split is for a launch whose workgroups are all resident at once (then it lasts as long as its slowest one):
    // where the kernel's registers and LDS let fewer share the compute units, the agents run in rounds already and
    // reserved compute units only lengthen the queue, so they are dealt in one launch.
    bool split = d && tail_lds > 0 && (long long)a.N <= (long long)d->cus * split_blocks_per_cu(fn, lds);
    if (split && tail_lds > 65536) {
        bool have = false;
        for (int i = 0; i < g_split_nattr; ++i) have = have || (g_split_attr[i].fn == fn && g_split_attr[i].bytes >= tail_lds);
        if (!have) {
            split = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, tail_lds) == hipSuccess;
            if (split && g_split_nattr < 32) g_split_attr[g_split_nattr++] = {fn, tail_lds};
        }
    }
    if (split) {
        // fork: both launches come behind everything already on `st`.  The tail must reach the compute units first (a
        // tail workgroup that finds them full waits until one has drained completely: the step then takes 1.36 ms
        // instead of 1.10, DESIGN §3.3 "Split launch"), so it is the tail that stays on `st`, where it starts as soon
        // as its predecessor ends, and the bulk that crosses to the side stream, which costs it the ~7 us of the
        // event hand-over.
        QPArgs tail = bulk;
        tail.order = a.order_tail;
        void* targs[] = {(void*)&tail};
        split = hipEventRecord(d->fork, st) == hipSuccess && hipStreamWaitEvent(d->side, d->fork, 0) == hipSuccess &&
                hipLaunchKernel(fn, dim3(a.tail_n), dim3(WAVE), targs, (size_t)tail_lds, st) == hipSuccess;
    }
    if (!split) {
        // no side stream, no such LDS request or a refused tail launch: every agent in one launch, in agent order
        (void)hipGetLastError();
        bulk.order = nullptr;
        (void)hipLaunchKernel(fn, dim3(a.N), dim3(WAVE), kargs, lds, st);
        return check_launch("qp_ipm_kernel");
    }
    if (hipLaunchKernel(fn, dim3(a.N), dim3(WAVE), kargs, lds, d->side) != hipSuccess)
        return check_launch("qp_ipm_kernel (bulk)");
    // join: whatever follows on `st` comes behind both launches
    if (hipEventRecord(d->join, d->side) != hipSuccess || hipStreamWaitEvent(st, d->join, 0) != hipSuccess)
        return check_launch("qp_ipm_kernel (split join)");
    return check_launch("qp_ipm_kernel");
}
}  // namespace scvx

using namespace scvx;

namespace {
double* g_trace = nullptr;
int g_trace_agent = 0, g_trace_cap = 0;

constexpr int kCapsDI[] = {SCVX_CAPS_DI};
constexpr int kCapsUni[] = {SCVX_CAPS_UNICYCLE};
constexpr int kCapsSI[] = {SCVX_CAPS_SI};
constexpr int kCapsQuad[] = {SCVX_CAPS_QUAD};

struct ModelTable {
    int nx, nu;
    const int* caps;
    int ncaps;
    int (*launch)(int, const QPArgs&, hipStream_t);
    int (*select)(int, const scvx_qp_template&, bool);   // nullptr: the model has runtime-K instantiations only
};

// model table entry for the template (nullptr: unknown model / dimensions)
const ModelTable* model_of(const scvx_qp_template& T) {
    static const ModelTable tab[] = {
        {6, 3, kCapsDI, (int)(sizeof(kCapsDI) / sizeof(int) / QP_CAPS_W), qp_launch_di, qp_select_di},
        {3, 2, kCapsUni, (int)(sizeof(kCapsUni) / sizeof(int) / QP_CAPS_W), qp_launch_unicycle, nullptr},
        {3, 3, kCapsSI, (int)(sizeof(kCapsSI) / sizeof(int) / QP_CAPS_W), qp_launch_si, nullptr},
        {12, 4, kCapsQuad, (int)(sizeof(kCapsQuad) / sizeof(int) / QP_CAPS_W), qp_launch_quad, nullptr},
    };
    const int ids[] = {SCVX_MODEL_DOUBLE_INTEGRATOR, SCVX_MODEL_UNICYCLE, SCVX_MODEL_SINGLE_INTEGRATOR, SCVX_MODEL_QUADROTOR};
    for (int i = 0; i < 4; ++i)
        if (T.model_id == ids[i] && T.n_x == tab[i].nx && T.n_u == tab[i].nu) return &tab[i];
    return nullptr;
}

// the kernel class of a template: a compiled row-capacity class of a built-in model (mt, cls), or -- for
// model_id = SCVX_MODEL_RUNTIME -- the exact class (n_x, n_u, n_box, n_obs, j_max, VC) compiled at run time
struct QPClass {
    const ModelTable* mt = nullptr;
    int cls = -1;
    bool rt = false;
    int nx = 0, nu = 0, nb = 0, no = 0, nc = 0, vc = 0;
};

// validates the template; on success sets the class
int qp_check(const scvx_qp_template* T, int N, QPClass& c) {
    if (!T || N < 0) return set_error(SCVX_EINVAL, "qp: null template");
    if (T->K < 2 || T->K > WAVE) return set_error(SCVX_EUNSUPPORTED, "qp: K must be in [2, 64]");
    if (T->pos_dim < 1 || T->pos_dim > 3 || T->pos_dim > T->n_x) return set_error(SCVX_EINVAL, "qp: pos_dim");
    if (T->n_box < 0 || T->n_box > SCVX_MAX_BOX || T->n_obs < 0 || T->n_obs > SCVX_MAX_OBS || T->j_max < 0)
        return set_error(SCVX_EINVAL, "qp: box/obstacle/collision counts");
    for (int b = 0; b < T->n_box; ++b)
        if (T->box_idx[b] < 0 || T->box_idx[b] >= T->n_x) return set_error(SCVX_EINVAL, "qp: box index");
    if (T->max_iter < 1) return set_error(SCVX_EINVAL, "qp: max_iter");
    if (T->w_nu < 0.0 || T->w_prox < 0.0) return set_error(SCVX_EINVAL, "qp: w_nu / w_prox must be >= 0");
    c = QPClass{};
    c.nx = T->n_x; c.nu = T->n_u;
    if (T->model_id == SCVX_MODEL_RUNTIME) {
        // the kernel's limits (qp_layout.hpp, shared with scvx_rtc_subproblem_compile)
        if (const char* bad = qp_class_error(T->n_x, T->n_u, T->n_box, T->n_obs, T->j_max, T->w_nu > 0.0 ? 1 : 0, T->K))
            return set_error(SCVX_EUNSUPPORTED, bad);
        c.rt = true;
        c.nb = T->n_box; c.no = T->n_obs; c.nc = T->j_max; c.vc = T->w_nu > 0.0 ? 1 : 0;
        return SCVX_OK;
    }
    c.mt = model_of(*T);
    if (!c.mt) return set_error(SCVX_EUNSUPPORTED, "qp: model id / dimensions");
    c.cls = qp_pick_caps(c.mt->caps, c.mt->ncaps, *T);
    if (c.cls < 0)
        return set_error(SCVX_EUNSUPPORTED, T->w_nu > 0.0
            ? "qp: no virtual-control class for this model / row counts (w_nu > 0: quad n_box <= 4, n_obs <= 16, j_max <= 32; di n_box <= 2, n_obs <= 8, no coupling)"
            : "qp: more box / obstacle / collision rows than the largest capacity class (j_max <= 32, n_obs <= 16)");
    const int* cp = c.mt->caps + QP_CAPS_W * c.cls;
    c.nb = cp[0]; c.no = cp[1]; c.nc = cp[2]; c.vc = cp[3];
    return SCVX_OK;
}

size_t ws_bytes(const QPClass& c, int N, int K) {
    return sizeof(double) * (size_t)N * (size_t)qp_layout(c.nx, c.nu, c.nb, c.no, c.nc, c.vc).ws_doubles(K);
}
}  // namespace

// Diagnostics hook (not part of the solve contract): subsequent scvx_qp_solve_batched launches write
// 8 doubles per IPM iteration of agent `agent` into the device buffer (pres, dres, gap, pobj,
// alpha_aff, alpha, sigma, mu), then 4 doubles (factor cycles, solve cycles, total cycles, fail code).
// agent < 0: one double per agent instead, its exit code (0 converged, 1 start-point factorization,
// 2 terminal Schur complement, 3 non-finite residual, 4 non-finite direction, 5 iteration cap,
// 6 stall at reduced accuracy).
extern "C" int scvx_qp_set_trace(double* buf, int agent, int cap) {
    g_trace = buf; g_trace_agent = agent; g_trace_cap = buf ? cap : 0;
    return SCVX_OK;
}

// Diagnostics query (host only, no launch): which instantiation of its class a solve of `tpl` runs right now -- the
// environment overrides and a trace set by scvx_qp_set_trace included.  0: K and the problem flags at run time;
// 1: K at compile time; 2: K and the flags at compile time (csrc/qp_inst.hpp qp_select, the function the launch
// itself calls).  Negative: the template's error code.
extern "C" int scvx_qp_instantiation(const scvx_qp_template* tpl) {
    QPClass c;
    const int rc = qp_check(tpl, 1, c);
    if (rc != SCVX_OK) return rc < 0 ? rc : -rc;
    if (c.rt || !c.mt->select) return 0;
    return c.mt->select(c.cls, *tpl, g_trace != nullptr);
}

extern "C" size_t scvx_qp_workspace_bytes(const scvx_qp_template* tpl, int N) {
    QPClass c;
    if (N <= 0 || qp_check(tpl, N, c) != SCVX_OK) return 0;
    return ws_bytes(c, N, tpl->K);
}

// the solve behind the three entry points: order_tail / T / reserve are those of scvx_qp_solve_batched_split
// (T = 0: one launch)
static int qp_solve(const scvx_qp_template* tpl, int N, const double* disc, const double* sigma, const double* Xref,
                    const double* Uref, const double* x_init, const double* x_final, const double* tr,
                    const double* coll_rows, const int32_t* coll_count, double* X, double* U, double* slack_coll,
                    double* nu, double* obj, int32_t* status, int32_t* iters, const int32_t* warm,
                    const int32_t* order, const int32_t* order_tail, int T, int reserve, void* workspace,
                    size_t workspace_bytes, void* stream) {
    QPClass c;
    int rc = qp_check(tpl, N, c);
    if (rc != SCVX_OK) return rc;
    if (N == 0) return SCVX_OK;
    if (!disc || !sigma || !Xref || !Uref || !x_init || !tr || !X || !U || !slack_coll || !obj || !status || !iters)
        return set_error(SCVX_EINVAL, "qp: null buffer");
    if ((tpl->has_final || tpl->w_final > 0.0) && !x_final) return set_error(SCVX_EINVAL, "qp: x_final required");
    if (tpl->w_final < 0.0 || (tpl->w_final > 0.0 && tpl->has_final))
        return set_error(SCVX_EINVAL, "qp: w_final > 0 (soft terminal) needs has_final = 0");
    if (tpl->j_max > 0 && (!coll_rows || !coll_count)) return set_error(SCVX_EINVAL, "qp: collision rows required");
    if (tpl->w_nu > 0.0 && !nu) return set_error(SCVX_EINVAL, "qp: nu output required (w_nu > 0)");
    if (warm && tpl->K < 2 * tpl->n_x) return set_error(SCVX_EUNSUPPORTED, "qp: warm start needs K >= 2 n_x");
    const size_t need = ws_bytes(c, N, tpl->K);
    if (!workspace || workspace_bytes < need) return set_error(SCVX_EWORKSPACE, "qp: workspace too small");
    QPArgs a{};
    a.T = *tpl;
    a.N = N;
    a.disc = disc; a.sigma = sigma; a.Xref = Xref; a.Uref = Uref; a.x_init = x_init; a.x_final = x_final;
    a.tr = tr; a.coll_rows = coll_rows; a.coll_count = coll_count; a.warm = warm;
    a.X = X; a.U = U; a.slack_coll = slack_coll; a.nu = nu; a.obj = obj; a.status = status; a.iters = iters;
    a.ws = (double*)workspace;
    a.ws_agent = (long long)(need / sizeof(double) / (size_t)N);
    a.trace = g_trace; a.trace_agent = g_trace_agent; a.trace_cap = g_trace_cap;
    a.order = order;
    if (c.rt) {   // the runtime-compiled classes keep the single launch (the two lists of a split: agent order)
        if (T > 0) a.order = nullptr;
        return rtc_qp_launch(a, c.nb, c.no, c.nc, c.vc, (hipStream_t)stream);
    }
    a.order_tail = order_tail; a.tail_n = T; a.tail_reserve = reserve;
    return c.mt->launch(c.cls, a, (hipStream_t)stream);
}

extern "C" int scvx_qp_solve_batched_ordered(const scvx_qp_template* tpl, int N, const double* disc,
                                             const double* sigma, const double* Xref, const double* Uref,
                                             const double* x_init, const double* x_final, const double* tr,
                                             const double* coll_rows, const int32_t* coll_count, double* X, double* U,
                                             double* slack_coll, double* nu, double* obj, int32_t* status,
                                             int32_t* iters, const int32_t* warm, const int32_t* order,
                                             void* workspace, size_t workspace_bytes, void* stream) {
    return qp_solve(tpl, N, disc, sigma, Xref, Uref, x_init, x_final, tr, coll_rows, coll_count, X, U, slack_coll, nu,
                    obj, status, iters, warm, order, nullptr, 0, 0, workspace, workspace_bytes, stream);
}

extern "C" int scvx_qp_solve_batched_split(const scvx_qp_template* tpl, int N, const double* disc, const double* sigma,
                                           const double* Xref, const double* Uref, const double* x_init,
                                           const double* x_final, const double* tr, const double* coll_rows,
                                           const int32_t* coll_count, double* X, double* U, double* slack_coll,
                                           double* nu, double* obj, int32_t* status, int32_t* iters,
                                           const int32_t* warm, const int32_t* order_bulk, const int32_t* order_tail,
                                           int T, int reserve, void* workspace, size_t workspace_bytes, void* stream) {
    if (N > 0 && (!order_bulk || !order_tail)) return set_error(SCVX_EINVAL, "qp split: null order list");
    if (T < 1 || T > (N > 0 ? N : 1)) return set_error(SCVX_EINVAL, "qp split: 1 <= T <= N required");
    if (reserve != SCVX_QP_RESERVE_WHOLE && reserve != SCVX_QP_RESERVE_HALF)
        return set_error(SCVX_EINVAL, "qp split: reserve must be SCVX_QP_RESERVE_WHOLE or SCVX_QP_RESERVE_HALF");
    return qp_solve(tpl, N, disc, sigma, Xref, Uref, x_init, x_final, tr, coll_rows, coll_count, X, U, slack_coll, nu,
                    obj, status, iters, warm, order_bulk, order_tail, T, reserve, workspace, workspace_bytes, stream);
}

extern "C" int scvx_qp_solve_batched(const scvx_qp_template* tpl, int N, const double* disc, const double* sigma,
                                     const double* Xref, const double* Uref, const double* x_init,
                                     const double* x_final, const double* tr, const double* coll_rows,
                                     const int32_t* coll_count, double* X, double* U, double* slack_coll,
                                     double* nu, double* obj, int32_t* status, int32_t* iters,
                                     const int32_t* warm, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return scvx_qp_solve_batched_ordered(tpl, N, disc, sigma, Xref, Uref, x_init, x_final, tr, coll_rows, coll_count,
                                         X, U, slack_coll, nu, obj, status, iters, warm, nullptr, workspace,
                                         workspace_bytes, stream);
}
