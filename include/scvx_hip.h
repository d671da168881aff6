/*
 * libscvx_hip.so -- C-ABI of the MI355X-native batched SCvx inner loop.
 *
 * Every pointer argument of a compute entry point is a CALLER-OWNED DEVICE buffer (e.g. a
 * PyTorch-ROCm tensor's data_ptr()); `stream` is a hipStream_t (NULL = default stream).  The
 * library never allocates caller-visible memory, never synchronises the stream and never throws:
 * every function returns SCVX_OK (0) or a negative SCVX_E* code, with a message available from
 * scvx_last_error().  Per-agent solver outcomes are reported in `status` arrays
 * (SCVX_STATUS_*), which the Python layer maps to CVXPY status strings.
 *
 * Layouts are agent-major (agent = outermost index) so that one agent's data is contiguous:
 *   X      [N][K][n]        == per agent the reference's X (n,K) in order='F'
 *   U      [N][K][m]
 *   disc   [N][K-1][n*(n+2m+2)]   per interval vec_F(A_k) | vec_F(B_k) | vec_F(C_k) | S_k | z_k
 *          == columns k of the reference's (A_bar, B_bar, C_bar, S_bar, z_bar)
 *          (SCvx/discretization/first_order_hold.py:20-24, 75-85).
 */
#ifndef SCVX_HIP_H
#define SCVX_HIP_H

#ifndef __HIPCC_RTC__  /* hipRTC (runtime-compiled kernels of user models) provides size_t itself */
#include <stddef.h>
#endif
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCVX_HIP_VERSION 7   /* 7: fleet separation analysis (scvx_rollout_dense_batched, scvx_separation_scan_batched,
                                  scvx_pair_min_distance_batched, scvx_obstacle_min_distance_batched); the
                                  inter-sample collision rows (scvx_intersample_pair_rows_batched,
                                  scvx_collision_rows_append_batched) and the obstacle scan
                                  (scvx_obstacle_scan_batched) were added to it without a bump: purely
                                  additive, no existing argument list changed; likewise the split QP launch
                                  (scvx_qp_dispatch_select, scvx_qp_solve_batched_split) and the dense roll-out
                                  of a runtime-compiled model (scvx_rtc_rollout_dense_batched) and the moving
                                  obstacles (scvx_moving_obstacle_scan_batched, scvx_node_rows_append_batched) */

#define SCVX_OK 0
#define SCVX_EINVAL (-1)
#define SCVX_EUNSUPPORTED (-2)
#define SCVX_ELAUNCH (-3)
#define SCVX_EWORKSPACE (-4)

/* model ids (csrc/models.hpp) */
#define SCVX_MODEL_DOUBLE_INTEGRATOR 0 /* n=6,  m=3  Distributed_opt/dist_scvx_3d.py:10-21 */
#define SCVX_MODEL_UNICYCLE 1          /* n=3,  m=2  SCvx/models/unicycle_model.py:54-63   */
#define SCVX_MODEL_SINGLE_INTEGRATOR 2 /* n=3,  m=3  SCvx/models/single_integrator_model.py:54-57 */
#define SCVX_MODEL_QUADROTOR 3         /* n=12, m=4  build-defined           */
/* any other model: n_x / n_u taken from the template; the subproblem kernels (QP, SCP) are compiled for
   those dimensions at the first solve (hipRTC) -- the user-model path of scvx_rtc_model_create */
#define SCVX_MODEL_RUNTIME 255

/* per-agent solver status (maps to cvxpy.OPTIMAL / OPTIMAL_INACCURATE / ...) */
#define SCVX_STATUS_OPTIMAL 0
#define SCVX_STATUS_MAX_ITER 1
#define SCVX_STATUS_NUMERICAL 2

int scvx_version(void);
const char* scvx_last_error(void);

/*
 * Batched FOH discretization.  Replaces FirstOrderHold.calculate_discretization
 * (SCvx/discretization/first_order_hold.py:52-87) for N agents in one launch.
 *   X [N][K][n], U [N][K][m], sigma [N]  ->  out [N][K-1][n*(n+2m+2)]
 * nsub = RK4 substeps per interval (1 is exact for the double integrator).
 * params: for the quadrotor five doubles in host memory, mass, g, Jx, Jy, Jz, or NULL for the defaults
 * (1, 9.81, 0.02, 0.02, 0.04); ignored (may be NULL) for the other models.
 */
int scvx_foh_batched(int model_id, const double* params, int K, int N, const double* X, const double* U,
                     const double* sigma, int nsub, double* out, void* stream);

/*
 * Batched nonlinear roll-outs: FirstOrderHold.integrate_nonlinear_piecewise (piecewise=1) and
 * integrate_nonlinear_full (piecewise=0) (first_order_hold.py:127-155).  Xout [N][K][n].
 */
int scvx_integrate_nonlinear_batched(int model_id, const double* params, int K, int N, const double* X,
                                     const double* U, const double* sigma, int nsub, int piecewise,
                                     double* Xout, void* stream);

/* ------------------------------------------------------------------------------------------
 * Runtime-compiled user models (hipRTC).  The reference's FirstOrderHold(model, K) integrates ANY
 * BaseModel through its numpy f/A/B callables (SCvx/discretization/first_order_hold.py:13-50,
 * 89-125; SCvx/models/base_model.py:16-24).  Here a user model is given as C expressions and
 * compiled for gfx950 at run time into the same RK4 forward-sensitivity kernel the built-in models
 * use (csrc/foh_body.hpp); no CPU path exists.
 *
 * Expressions are HIP C++ double expressions in x[0..n_x), u[0..n_u), p[0..SCVX_MAX_MODEL_PARAMS)
 * (the params array of the launch) and any name the prelude defines:
 *   f_exprs  n_x entries         f_i(x, u)
 *   A_exprs  n_x*n_x, row-major  dA_ij = d f_i / d x_j
 *   B_exprs  n_x*n_u, row-major  dB_ij = d f_i / d u_j
 * A NULL entry, "" or "0" is a structural zero (skipped in the generated matrix-vector products).
 * prelude: optional statements (e.g. `const double c2 = cos(x[2]);`) evaluated before the
 * expressions in each of f, A and B.  n_x <= 16, n_u <= 8.
 *
 * scvx_rtc_model_create compiles (no GPU needed); the code object is loaded on the calling
 * thread's current device at the first launch.  On a compile error it returns SCVX_EINVAL with
 * *out set to a model that holds only the generated source and the compiler log (read them with
 * scvx_rtc_model_source / _log, then destroy it; launches on it fail); other errors leave *out NULL.
 * ------------------------------------------------------------------------------------------ */
#define SCVX_MAX_MODEL_PARAMS 16
#define SCVX_RTC_MAX_NX 16
#define SCVX_RTC_MAX_NU 8
typedef struct scvx_rtc_model scvx_rtc_model;

int scvx_rtc_model_create(int n_x, int n_u, const char* const* f_exprs, const char* const* A_exprs,
                          const char* const* B_exprs, const char* prelude, scvx_rtc_model** out);
/* generated HIP source (for inspection) and the last compile log; buffers are the model's */
const char* scvx_rtc_model_source(const scvx_rtc_model* model);
const char* scvx_rtc_model_log(const scvx_rtc_model* model);
int scvx_rtc_model_destroy(scvx_rtc_model* model);

/* as scvx_foh_batched / scvx_integrate_nonlinear_batched; params: n_params <= SCVX_MAX_MODEL_PARAMS
 * doubles (host memory, copied into the launch), p[i] = 0 beyond n_params */
int scvx_rtc_foh_batched(const scvx_rtc_model* model, const double* params, int n_params, int K, int N,
                         const double* X, const double* U, const double* sigma, int nsub, double* out,
                         void* stream);
int scvx_rtc_integrate_nonlinear_batched(const scvx_rtc_model* model, const double* params, int n_params,
                                         int K, int N, const double* X, const double* U, const double* sigma,
                                         int nsub, int piecewise, double* Xout, void* stream);

/* Compile (no GPU needed) the subproblem kernel a SCVX_MODEL_RUNTIME template is served by, into the
 * process-wide code-object cache the first solve would fill (a warm-up / a build check of user classes):
 *   kind 0  the trust-region QP (scvx_qp_solve_batched), cls = {n_x, n_u, n_box, n_obs, j_max class, VC}
 *   kind 1  the SCProblem (scvx_scp_solve_batched),       cls = {n_x, n_u, n_extra, waves per agent}
 * (the class ints of csrc/qp_capi.hip / csrc/scp_ipm.hip).  *code_bytes (optional) = code-object size.
 * SCVX_EINVAL with the compiler log in scvx_last_error() on a compile error. */
int scvx_rtc_subproblem_compile(int kind, const int* cls, int ncls, size_t* code_bytes);

/* ------------------------------------------------------------------------------------------
 * Batched trust-region subproblem (one per agent), the convex solve the reference hands to
 * CVXPY+Clarabel in Distributed_opt/dist_scvx_3d.py:51-111 (x_traj_opt), written in absolute
 * variables x_t = xbar_t + d_t, u_t = ubar_t + w_t:
 *
 *   min  sum_{t<K-1} ||u_t||^2 + w_last ||u_{K-1}||^2 + w_coll sum_t S_t + w_obs sum_{t,o} s_{t,o}
 *   s.t. x_0 = x_init                                                    (:73, d_0 = 0)
 *        x_{t+1} = A_t x_t + B_t u_t + C_t u_{t+1} + S_t sigma + z_t      (:80-83; FOH form)
 *        x_{K-1} = x_final                     if has_final               (:74)
 *        u_{K-1} = ubar_{K-1}                  if fix_last_input          (:63, unused w row)
 *   for nodes t < K-1 (and t = K-1 if ineq_last):
 *        ||u_t - ubar_t||_1 <= tr                                        (:84)
 *        box_lo[i] <= x_t[box_idx[i]] <= box_hi[i]                         (:87-90)
 *        b_j - g_j' p_t <= S_t (j < coll_count[t]),  S_t >= 0           (:93-107, shared slack)
 *        a_o' (p_t - c_o) >= r_o - s_{t,o},  s_{t,o} >= 0,
 *           a_o = (pbar_t - c_o)/(||pbar_t - c_o|| + 1e-6)   (single_integrator_model.py:113-126)
 *        ||u_t||_2 <= u_max                    if has_soc                 (single_integrator_model.py:103-104)
 * with p_t = x_t[0:pos_dim].  With w_nu > 0 (virtual control, the SCvx subproblem form of
 * SCvx/optimization/sc_problem.py:60-68) every dynamics row carries nu_t (t < K-1):
 *        x_{t+1} = A_t x_t + B_t u_t + C_t u_{t+1} + S_t sigma + z_t + nu_t,
 * and the objective gains the exact penalty w_nu sum_t ||nu_t||_1 (node-separable; the reference's
 * SCProblem prices max_t ||nu_t||_1, scvx_scp_solve_batched below), so the subproblem stays feasible
 * whatever the linearisation point (nonlinear models under the Jacobi update).  With w_prox > 0 the
 * objective also gains w_prox sum_t ||x_t - xbar_t||^2, a soft trust region on the states (the trust
 * region above bounds only the inputs, which leaves the states of a long integrator chain free).  Solved by a batched primal-dual interior-point method (Mehrotra
 * predictor-corrector, Nesterov-Todd scaling for the SOC) whose KKT systems are factored by a
 * Riccati recursion over the K nodes.
 * ------------------------------------------------------------------------------------------ */
#define SCVX_MAX_BOX 4
#define SCVX_MAX_OBS 16

typedef struct scvx_qp_template {
    int32_t model_id;       /* only used for n_x/n_u consistency checks */
    int32_t n_x, n_u, K;
    int32_t pos_dim;        /* 2 or 3 */
    int32_t has_final;
    int32_t fix_last_input;
    int32_t ineq_last;
    double w_last;
    int32_t n_box;
    int32_t box_idx[SCVX_MAX_BOX];
    double box_lo[SCVX_MAX_BOX];
    double box_hi[SCVX_MAX_BOX];
    int32_t n_obs;
    double obs_center[SCVX_MAX_OBS][3];
    double obs_radius[SCVX_MAX_OBS];
    double w_obs;
    int32_t j_max;          /* collision rows per node (0 = no coupling) */
    double w_coll;
    int32_t has_soc;
    double u_max;
    int32_t max_iter;
    double tol;
    double w_final;         /* has_final = 0 and w_final > 0: soft terminal w_final ||x_{K-1} - x_final||^2 */
    double w_nu;            /* > 0: virtual control nu_t with penalty w_nu sum_t ||nu_t||_1 (0: none) */
    double w_prox;          /* > 0: proximal term w_prox sum_t ||x_t - xbar_t||^2 (a soft state trust region) */
} scvx_qp_template;

/*
 * Inputs (device, agent-major):
 *   disc [N][K-1][n(n+2m+2)], sigma [N], Xref [N][K][n], Uref [N][K][m], x_init [N][n],
 *   x_final [N][n] (ignored unless has_final or w_final > 0), tr [N],
 *   coll_rows [N][K][j_max][pos_dim+1] rows (g, b), coll_count [N][K] (both ignored if j_max=0)
 * Outputs (device):
 *   X [N][K][n], U [N][K][m], slack_coll [N][K] (S_t, zeros if j_max = 0),
 *   nu [N][K-1][n] (virtual control; required iff w_nu > 0, may be NULL otherwise), obj [N],
 *   status [N], iters [N]
 * warm [N] (device int32, may be NULL): agents with warm[a] != 0 start from the primal-dual point their
 *   previous solve left in this workspace (same template, same agent slot): z, the multipliers and the
 *   inequality duals are kept, the slacks recomputed from the new rows, every slack / dual floored
 *   inside its cone.  The optimum and the stopping rule are unchanged; the Jacobi SCvx loop, which
 *   re-solves each agent re-linearised at its own solution, needs ~2.4x fewer IPM iterations (C3).
 *   Requires K >= 2 n_x.  warm = NULL (or all 0): the CVXOPT-style cold start.
 * workspace: caller-owned device scratch of at least scvx_qp_workspace_bytes(tpl, N) bytes.
 * Limits: 2 <= K <= 64 (one node per lane), n_u <= 4, <= 64 inequality rows per node.
 */
int scvx_qp_solve_batched(const scvx_qp_template* tpl, int N, const double* disc, const double* sigma,
                          const double* Xref, const double* Uref, const double* x_init, const double* x_final,
                          const double* tr, const double* coll_rows, const int32_t* coll_count, double* X,
                          double* U, double* slack_coll, double* nu, double* obj, int32_t* status, int32_t* iters,
                          const int32_t* warm, void* workspace, size_t workspace_bytes, void* stream);

/* scvx_qp_solve_batched with a dispatch order (replaces the same call, qp_capi.hip; the reference has no
 * counterpart -- its agents' subproblems are solved one by one, dist_scvx_3d.py:110): workgroup b solves agent
 * order[b] (device int32 [N], a permutation of 0..N-1; NULL = agent b).  A non-permutation is undefined
 * behaviour: an entry outside [0, N) is replaced by b, which can duplicate an agent (two workgroups then share
 * its workspace and outputs) and leave another unsolved.
 * Workgroups start in index order as slots free up, so when the agents outnumber the resident waves the
 * longest solves dealt first shorten the launch (JacobiSCvx orders by the last step's IPM iterations).
 * Results do not depend on the order. */
int scvx_qp_solve_batched_ordered(const scvx_qp_template* tpl, int N, const double* disc, const double* sigma,
                                  const double* Xref, const double* Uref, const double* x_init,
                                  const double* x_final, const double* tr, const double* coll_rows,
                                  const int32_t* coll_count, double* X, double* U, double* slack_coll, double* nu,
                                  double* obj, int32_t* status, int32_t* iters, const int32_t* warm,
                                  const int32_t* order, void* workspace, size_t workspace_bytes, void* stream);

/* An order entry with this value makes its workgroup return before it reads or writes anything (every other entry
 * outside [0, N) falls back to the workgroup's index, as above). */
#define SCVX_QP_ORDER_SKIP (-2147483647 - 1)
/* tail reservation of scvx_qp_solve_batched_split: the tail workgroup's LDS request leaves room for no other QP
 * workgroup on its compute unit (WHOLE) or for exactly one (HALF) */
#define SCVX_QP_RESERVE_WHOLE 1
#define SCVX_QP_RESERVE_HALF 2

/* The two order lists of scvx_qp_solve_batched_split from the previous solve's IPM iteration counts (one workgroup,
 * deterministic, no host synchronisation; csrc/qp_dispatch.hip).  iters device int32 [N], clamped to [0, max_iter].
 * All agents sorted by descending count, ties by ascending index (a stable counting sort): the first n_tail of them go to
 * order_tail [T], the rest to order_bulk [N], in that order; the unused entries of both lists are SCVX_QP_ORDER_SKIP.
 * n_tail = min(T, #{iters >= thr}), and with short_per_tail > 0 also at most #{iters < thr} / short_per_tail: every
 * running tail workgroup displaces that many bulk workgroups into a second round (three with
 * SCVX_QP_RESERVE_WHOLE on a compute unit of four, one with _HALF), which pays only while those are short solves -- a
 * batch whose agents all reach thr gets no tail.  short_per_tail = 0: no such limit.  T = 0 (order_tail may be NULL):
 * order_bulk is the whole sort, the longest-first order of scvx_qp_solve_batched_ordered.  Limits: 0 <= T <= N,
 * 1 <= max_iter <= 1023, and ceil(N / 64) * (max_iter + 1) <= 12288 (the count table in LDS), else SCVX_EUNSUPPORTED. */
int scvx_qp_dispatch_select(int N, const int32_t* iters, int thr, int T, int short_per_tail, int max_iter,
                            int32_t* order_tail, int32_t* order_bulk, void* stream);

/* scvx_qp_solve_batched_ordered as two launches of the same kernel (qp_capi.hip): the agents of order_tail
 * (device int32 [T]) on a library-owned non-blocking side stream, submitted first and with the LDS request of
 * `reserve` (the kernel does not use the extra LDS), so each of them has a compute unit to itself or shares it with
 * one workgroup instead of three; the agents of order_bulk (device int32 [N]) on `stream` with the usual request.
 * Between them the two lists name every agent once (scvx_qp_dispatch_select); the rest is SCVX_QP_ORDER_SKIP.  The side
 * stream waits for everything enqueued on `stream` before the call, and `stream` waits for both launches after it (two
 * events, no host synchronisation).  Not to be called under stream capture.  Every output is what the single launch
 * writes, bit for bit: the same instruction stream runs on the same data.  A runtime-compiled class
 * (SCVX_MODEL_RUNTIME) and a refused tail launch solve every agent in one launch instead. */
int scvx_qp_solve_batched_split(const scvx_qp_template* tpl, int N, const double* disc, const double* sigma,
                                const double* Xref, const double* Uref, const double* x_init, const double* x_final,
                                const double* tr, const double* coll_rows, const int32_t* coll_count, double* X,
                                double* U, double* slack_coll, double* nu, double* obj, int32_t* status,
                                int32_t* iters, const int32_t* warm, const int32_t* order_bulk,
                                const int32_t* order_tail, int T, int reserve, void* workspace,
                                size_t workspace_bytes, void* stream);

/* Bytes of caller-owned device scratch scvx_qp_solve_batched needs for N agents. */
size_t scvx_qp_workspace_bytes(const scvx_qp_template* tpl, int N);

/* Diagnostics hook: later solves write 8 doubles per IPM iteration of agent `agent`
 * (pres, dres, gap, pobj, alpha_aff, alpha, sigma, mu) into device buffer `buf` (cap iterations).
 * buf = NULL disables.  Not needed for normal use. */
int scvx_qp_set_trace(double* buf, int agent, int cap);

/*
 * Pairwise collision linearization for the Jacobi coupling (Distributed_opt/dist_scvx_3d.py:93-107):
 * for local agents i0..i0+N_local-1 of the all-gathered states X_all [N_total][K][n_x] and nodes
 * t < K-1, rows (g, b) with g = (p_i - p_j)/|p_i - p_j|, b = 2R - |p_i - p_j| + g' p_i, i.e.
 * b - g' p_t <= S_t.  cull_radius <= 0 keeps every neighbour; otherwise only |p_i - p_j| < cull_radius.
 * At most j_max rows per node (largest 2R - |.| kept).  rows [N_local][K][j_max][pos_dim+1],
 * count [N_local][K].
 */
int scvx_collision_rows_batched(int K, int pos_dim, int n_x, int N_total, const double* X_all, int i0,
                                int N_local, double R, double cull_radius, int j_max, double* rows,
                                int32_t* count, void* stream);

/*
 * The same rows for an arbitrary subset of agents: local agent a (< N_sel) is global agent idx[a] of X_all
 * (idx: device int32 [N_sel], distinct values in [0, N_total)).  rows [N_sel][K][j_max][pos_dim+1],
 * count [N_sel][K].  Used for the agents the full-row check below found violating.
 */
int scvx_collision_rows_indexed(int K, int pos_dim, int n_x, int N_total, const double* X_all, const int32_t* idx,
                                int N_sel, double R, double cull_radius, int j_max, double* rows, int32_t* count,
                                void* stream);

/*
 * A-posteriori check of the reference's FULL collision row set at a solution (replaces nothing in the
 * reference, which always solves with every row: Distributed_opt/dist_scvx_3d.py:93-107).  For every
 * local agent i, node t < K-1 and every j != i of X_all (the linearisation point):
 *     v = (2R - |pbar_i - pbar_j|) - g_ij' (p_t - pbar_i) - S_t,   g_ij = (pbar_i - pbar_j)/|.|
 * with p_t = X_new[i][t][0:pos_dim], S_t = slack[i][t].  Outputs viol [N_local][K] = #{j : v > tol}
 * and vmax [N_local][K] = max_j v (0 at t = K-1).  A coincident neighbour's row is NaN (the reference's
 * 0/0): it is counted in viol and makes vmax NaN.  A fleet of one (N_total = 1) has no row: viol = 0 and
 * vmax = -1e300, the maximum's start value, below every row value (finite, so a reduction over agents
 * stays finite).  A culled solve (j_max < N_total-1) is the
 * reference's solution iff no row is violated: the culled problem is a relaxation of the full one.
 */
int scvx_collision_check_batched(int K, int pos_dim, int n_x, int N_total, const double* X_all, int i0,
                                 int N_local, double R, const double* X_new, const double* slack, double tol,
                                 int32_t* viol, double* vmax, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batched SCvx convex subproblem: the reference's SCProblem (SCvx/optimization/sc_problem.py:15-83)
 * with the constraints of its models (unicycle_model.py:88-114, single_integrator_model.py:80-126)
 * and, when n_nbr > 0, the ADMM terms of AgentSolver (agent_solver.py:78-102, si_agent_solver.py:70-92):
 *
 *   min  w_nu ||nu||_{1,ind} + w_slack sum_{o,k} s'_{o,k} + w_sigma sigma
 *        + sum_j [ sum Lam_j o (p - Y_j) + rho/2 ||p - Y_j||_F^2 + w_coll sum_k S_{j,k} ]
 *   s.t. x_{k+1} = A_k x_k + B_k u_k + C_k u_{k+1} + S_k sigma + z_k + nu_k      (:53-68)
 *        ||X - Xref||_{1,ind} + ||U - Uref||_{1,ind} + |sigma - sigma_ref| <= tr    (:71-74)
 *        sigma >= 0; x_0 = x_init; x_{K-1} = x_final (has_final); u_0 = 0 (pin_u_first);
 *        u_{K-1} = 0 (pin_u_last); ub_lo <= u_k[ub_idx] <= ub_hi; xb_lo <= x_k[xb_idx] <= xb_hi;
 *        ||u_k||_2 <= u_max (has_soc); a_{o,k}'(p_k - c_o) >= r_o - s'_{o,k}, s' >= 0 with
 *        a_{o,k} = (pbar_k - c_o)/(||pbar_k - c_o|| + 1e-6);  a_{j,k}'(p_k - Y_{j,k}) + S_{j,k} >= d_min,
 *        S >= 0 with a_{j,k} = (pbar_k - P_{j,k})/(||pbar_k - P_{j,k}|| + 1e-6) (multi_agent_model.py:61-79),
 * p_k = x_k[0:pos_dim], ||M||_{1,ind} = max_k ||M[:,k]||_1 (the induced norm cvx.norm(M, 1) computes).
 * Solved by a primal-dual interior-point method (Mehrotra, Nesterov-Todd SOC scaling) whose Newton
 * systems go through a Riccati recursion with (sigma, tau_x, tau_u, tau_nu) as augmented states.
 * Supported models: unicycle (n=3, m=2), single integrator (n=3, m=3).  K <= 256.
 * ------------------------------------------------------------------------------------------ */
#define SCVX_MAX_NBR 32

typedef struct scvx_scp_template {
    int32_t model_id;
    int32_t n_x, n_u, K;
    int32_t pos_dim;
    int32_t has_final;      /* X[:,-1] == x_final (requires pin_u_last) */
    int32_t pin_u_first;    /* U[:,0] == 0  */
    int32_t pin_u_last;     /* U[:,-1] == 0 */
    int32_t n_ubound;
    int32_t ub_idx[SCVX_MAX_BOX];
    int32_t ub_has_lo[SCVX_MAX_BOX];
    int32_t ub_has_hi[SCVX_MAX_BOX];
    double ub_lo[SCVX_MAX_BOX];
    double ub_hi[SCVX_MAX_BOX];
    int32_t has_soc;
    double u_max;
    int32_t n_xbound;
    int32_t xb_idx[SCVX_MAX_BOX];
    double xb_lo[SCVX_MAX_BOX];
    double xb_hi[SCVX_MAX_BOX];
    int32_t n_obs;
    double obs_center[SCVX_MAX_OBS][3];
    double obs_radius[SCVX_MAX_OBS];   /* total clearance r_o (obstacle + robot radius [+ margin]) */
    double w_nu, w_slack, w_sigma;
    int32_t n_nbr;
    double rho, d_min, w_coll;
    int32_t max_iter;
    double tol;
    double reg;             /* primal regularisation of the Newton systems (scaled units), e.g. 1e-10 */
    /* Nash best-response terms (scvx_scp_game_solve_batched; zero for SCProblem / AgentSolver) */
    int32_t game;           /* 1: the terms below are active */
    int32_t sigma_fixed;    /* sigma == sigma_ref (agent_best_response.py:77) */
    double w_u2;            /* control_weight       * ||U||_F^2                       (game_model.py:88) */
    double w_du;            /* control_rate_weight  * sum_k ||u_{k+1} - u_k||^2       (:91-93) */
    double w_dth;           /* curvature_weight     * sum_k (x_{k+1}[th] - x_k[th])^2 (:94-96) */
    int32_t theta_idx;      /* state index of th (unicycle 2), -1: no curvature state */
    double w_in;            /* inertia_weight       * ||X - X_prev||_F^2              (:99-100) */
    int32_t n_slab;         /* slab rows z_{j,k}'(p_k - P_{j,k}) >= r_slab per node (:121-124), <= SCVX_MAX_NBR */
    double r_slab;          /* collision_radius */
    /* launch mapping of this template's solves (version 4; version 5 dropped the process-wide default setter):
     * 0 = automatic -- two waves per agent when K > 64 and the launch leaves SIMDs idle (2 N <= 4 x CUs), so the
     * node phases of a K <= 128 agent run in one pass; 1 or 2 waves per agent forced */
    int32_t waves_per_agent;
} scvx_scp_template;

/*
 * Inputs (device, agent-major): disc [N][K-1][n(n+2m+2)], Xref [N][K][n], Uref [N][K][m],
 *   sigma_ref [N], tr [N], x_init [N][n], x_final [N][n],
 *   nbr_pos / nbr_Y / nbr_Lam [N][n_nbr][K][pos_dim]  (neighbour reference positions X_ref_j[0:pd],
 *   consensus Y_j, duals Lambda_j; ignored when n_nbr = 0).
 * Outputs (device): X [N][K][n], U [N][K][m], nu [N][K-1][n], sigma [N], s_obs [N][n_obs][K],
 *   s_nbr [N][n_nbr][K], obj [N] (the reference objective at the solution), status [N], iters [N].
 */
int scvx_scp_solve_batched(const scvx_scp_template* tpl, int N, const double* disc, const double* Xref,
                           const double* Uref, const double* sigma_ref, const double* tr, const double* x_init,
                           const double* x_final, const double* nbr_pos, const double* nbr_Y, const double* nbr_Lam,
                           double* X, double* U, double* nu, double* sigma, double* s_obs, double* s_nbr, double* obj,
                           int32_t* status, int32_t* iters, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of caller-owned device scratch scvx_scp_solve_batched / scvx_scp_game_solve_batched need for
 * N agents (depends on the game fields: the game kernel carries extra Riccati states). */
size_t scvx_scp_workspace_bytes(const scvx_scp_template* tpl, int N);



/* ------------------------------------------------------------------------------------------
 * Batched Nash best response: AgentBestResponse.setup/solve (SCvx/optimization/agent_best_response.py:
 * 35-113, si_agent_best_response.py:36-127) = the SCProblem above (without ADMM terms) plus the
 * GameUnicycleModel / GameSIModel cost and slab constraints (game_model.py:68-126,
 * game_si_model.py:90-136) and sigma == sigma_ref:
 *
 *   + w_u2 ||U||_F^2 + w_du sum_k ||u_{k+1} - u_k||^2 + w_dth sum_k (th_{k+1} - th_k)^2
 *   + w_in ||X - X_prev||_F^2,      s.t.  z_{j,k}'(p_k - P_{j,k}) >= r_slab   (j < n_slab, every k)
 *
 * The cross-node terms ride on augmented Riccati states u~_k = u_{k-1}, th~_k = th_{k-1}.
 * Extra inputs (device): X_prev [N][K][n] (read when w_in > 0), slab_z / slab_P
 * [N][n_slab][K][pos_dim] (the slab normals z and neighbour positions P).  obj includes the game
 * cost and w_sigma sigma_ref.  Requires tpl->game = 1 and tpl->n_nbr = 0; models as above.
 * ------------------------------------------------------------------------------------------ */
int scvx_scp_game_solve_batched(const scvx_scp_template* tpl, int N, const double* disc, const double* Xref,
                                const double* Uref, const double* sigma_ref, const double* tr,
                                const double* x_init, const double* x_final, const double* X_prev,
                                const double* slab_z, const double* slab_P, double* X, double* U, double* nu,
                                double* sigma, double* s_obs, double* obj, int32_t* status, int32_t* iters,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Slab normals of the ACS dual update (GameUnicycleModel.update_slabs, game_model.py:54-66 /
 * game_si_model.py:69-88): z[a][j][k] = d / ||d|| with d = p[a][k] - P[a][j][k], 0 when ||d|| < 1e-6.
 * p [N][K][n_x] (positions = the first pos_dim states), P [N][n_slab][K][pos_dim], z likewise. */
int scvx_slab_update_batched(int N, int n_slab, int K, int pos_dim, int n_x, const double* p, const double* P,
                             double* z, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batched inter-sample obstacle clearance: SCvx/utils/intersample_collision.py (make_segment_f
 * :104-126, h_i :7-26, find_critical_times :29-67, linearize_h :70-101) for every (agent, segment k,
 * obstacle) of N agents, as called per segment by SCvx/models/game_si_model.py:156-176.
 * For segment k of agent a: x(t) rolls out dx/dtau = f(x, u_k + tau/dt_phys (u_{k+1} - u_k)) from
 * X[a][k] to tau = t dt_phys (dt_phys = seg_dt * sigma[a]; FirstOrderHold._dx); h(t) = ||proj x(t) -
 * c_o|| - r_o; the interior minima t* in (0, dt) of h are located by the reference's scan
 * (num_samples central differences phi with step eps on [eps, dt - eps], bisection to tol, phi2 > 0);
 * at each t*: h0 = h(t*), grad_x = central differences of h w.r.t. x_k, grad_u = 0 (the segment
 * roll-out ignores u_k, as in the reference).
 * ------------------------------------------------------------------------------------------ */
#define SCVX_IS_MAX_PROJ 3
#define SCVX_IS_MAX_STATE 12

typedef struct scvx_intersample_template {
    int32_t model_id;
    int32_t n_obs;
    double obs_center[SCVX_MAX_OBS][SCVX_IS_MAX_PROJ];
    double obs_radius[SCVX_MAX_OBS];
    int32_t proj_rows;                                   /* rows of T (projection), <= 3 */
    double proj[SCVX_IS_MAX_PROJ * SCVX_IS_MAX_STATE];   /* T row-major, row stride SCVX_IS_MAX_STATE */
    double dt;            /* find_critical_times' dt (normalised segment length; the reference passes 1.0) */
    double seg_dt;        /* FirstOrderHold.dt = 1 / (K_foh - 1) */
    double eps;           /* central-difference step (reference 1e-4) */
    double tol;           /* bisection tolerance (reference 1e-6) */
    int32_t num_samples;  /* scan points (reference 100) */
    int32_t max_crit;     /* minima stored per (agent, segment, obstacle) */
    int32_t nsub;         /* RK4 steps per roll-out */
} scvx_intersample_template;

/*
 * Inputs (device): X [N][K][n], U [N][K][m], sigma [N]; params as scvx_foh_batched.
 * Outputs (device): n_crit [N][K-1][n_obs] (minima found; only the first max_crit are stored),
 *   t_crit / h0 [N][K-1][n_obs][max_crit], grad_x [..][max_crit][n], grad_u [..][max_crit][m].
 */
int scvx_intersample_batched(const scvx_intersample_template* tpl, const double* params, int K, int N,
                             const double* X, const double* U, const double* sigma, int32_t* n_crit,
                             double* t_crit, double* h0, double* grad_x, double* grad_u, void* stream);

/* scvx_intersample_batched for a runtime-compiled user model (scvx_rtc_model_create; n_x <= SCVX_IS_MAX_STATE):
 * the same scan on the model's own f, so the inter-sample search of any BaseModel runs on the GPU (the reference's
 * SCvx/utils/intersample_collision.py:104-126 integrates model.get_equations()'s f with odeint for any model).
 * tpl->model_id is ignored; params / n_params as scvx_rtc_foh_batched.  (version 5) */
int scvx_rtc_intersample_batched(const scvx_rtc_model* model, const double* params, int n_params,
                                 const scvx_intersample_template* tpl, int K, int N, const double* X, const double* U,
                                 const double* sigma, int32_t* n_crit, double* t_crit, double* h0, double* grad_x,
                                 double* grad_u, void* stream);

/* ------------------------------------------------------------------------------------------
 * ADMM consensus / dual update of the multi-agent coordinators: replaces the host loop of
 * SCvx/optimization/admm_coordinator.py:80-96 (si_admm_coordinator.py:91-102).  For agent i and
 * neighbour slot s (j = nbr[i][s]), p_j = X_new[j][:, 0:pos_dim]:
 *     Y_new = (Y + p_j) / 2;  Lam += rho (p_j - Y_new);
 *     primal[i][s] = ||p_j - Y_new||_F;  dual[i][s] = ||Y_new - Y||_F   (admm_utils.py:20-38)
 * Device buffers: X_new [N][K][n_x], nbr [N][n_nbr] int32, Y / Lam [N][n_nbr][K][pos_dim] (updated in
 * place; the layout of scvx_scp_solve_batched's nbr_Y / nbr_Lam), primal / dual [N][n_nbr].  The
 * element updates are bit-identical to the reference's numpy expressions.
 */
int scvx_admm_consensus_batched(int N, int n_nbr, int K, int pos_dim, int n_x, const double* X_new,
                                const int32_t* nbr, double rho, double* Y, double* Lam, double* primal,
                                double* dual, void* stream);

/* ------------------------------------------------------------------------------------------
 * Bookkeeping of one Jacobi SCvx iteration with the per-agent trust-region rule (the tensor ops of
 * scvx_hip/scvx.py JacobiSCvx.step, fused): per agent i, (X_out[i], U_out[i]) = (X_sol[i], U_sol[i]) if
 * status[i] != 2, else (X[i], U[i]) (Distributed_opt/dist_scvx_3d.py:113-118; X_out may alias X);
 * cost = sum_{t<K-1} ||U_out[i][t]||^2
 * (cost_fcn, :131-138); tr[i] *= 0.5 if cost > prev_cost[i] (1 + tie_rtol) (:248-252, per agent;
 * tie_rtol >= 0, e.g. 1e-9: successive costs of a converged agent agree only to rounding, so the
 * reference's strict test (tie_rtol = 0) would halve on the rounding of the sum); a failed agent's
 * radius then halves (grow = 0) or doubles (grow = 1; every radius is then capped at tr_max);
 * prev_cost[i] = cost.
 * Device buffers: status [N] int32, X_sol / X / X_out [N][K][n_x], U_sol / U / U_out [N][K][n_u],
 * tr / prev_cost [N] (updated in place).
 */
int scvx_jacobi_update_batched(int N, int K, int n_x, int n_u, const int32_t* status, const double* X_sol,
                               const double* U_sol, const double* X, const double* U, double* X_out, double* U_out,
                               double* tr, double* prev_cost, int grow, double tr_max, double tie_rtol,
                               void* stream);

/*
 * The same bookkeeping under the reference's GLOBAL trust-region rule (Distributed_opt/dist_scvx_3d.py:242-252:
 * one radius, halved when the summed cost_fcn rises; ABI 6), in two calls:
 *   scvx_jacobi_update_costs_batched: X_out / U_out as scvx_jacobi_update_batched, cost[i] = sum_{t<K-1}
 *     ||U_out[i][t]||^2; the radii are not touched.
 *   scvx_jacobi_global_rule: total = sum_i cost[i] (fixed summation order); mode 0 writes it to total_out only (a
 *     rank's share, to be all-reduced by the caller), mode 1 sums and applies, mode 2 applies *total_in (the
 *     all-reduced total).  Apply: tr[i] *= 0.5 for every agent if total > *prev_total (the reference's strict test),
 *     then a failed agent's radius halves (grow = 0) or doubles (grow = 1, capped at tr_max); *prev_total = total
 *     (and *total_out when given).
 * Device buffers: cost / tr [N], status [N] int32, total_in / total_out / prev_total one double each.
 */
int scvx_jacobi_update_costs_batched(int N, int K, int n_x, int n_u, const int32_t* status, const double* X_sol,
                                     const double* U_sol, const double* X, const double* U, double* X_out,
                                     double* U_out, double* cost, void* stream);
int scvx_jacobi_global_rule(int N, int mode, const int32_t* status, const double* cost, const double* total_in,
                            double* total_out, double* tr, double* prev_total, int grow, double tr_max, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fleet separation analysis (version 7; csrc/separation.hip): how close any two agents of a finished run
 * come, at the nodes (SCvx/utils/analysis.py:10-62) and between them (no reference counterpart).
 * ------------------------------------------------------------------------------------------ */

/*
 * Dense samples of every segment's nonlinear roll-out: for agent a and segment k < K-1 the roll-out from
 * X[a][k] under the FOH input u_k + tau/dt (u_{k+1} - u_k), dt = sigma[a]/(K-1) (the piecewise semantics of
 * scvx_integrate_nonlinear_batched: restart at every node), sampled at tau_s = s/S dt, s = 0..S.  Fixed-step
 * RK4 with `sub` steps between consecutive samples (exact for the double and the single integrator).
 *   X [N][K][n], U [N][K][m], sigma [N]  ->  P [N][K-1][S+1][3]  the first pos_dim states, zeros past pos_dim
 *                                            L [N][K-1]          polyline length of those samples
 * Limits: K >= 2, N >= 0 (N == 0: SCVX_OK, no launch), 1 <= S <= 16, sub >= 1, 1 <= pos_dim <= min(3, n), no null
 * buffer; anything else is SCVX_EINVAL.  A model id names a built-in model: SCVX_MODEL_RUNTIME returns
 * SCVX_EUNSUPPORTED here, a runtime-compiled model has the handle-based form below.  params as scvx_foh_batched.
 */
int scvx_rollout_dense_batched(int model_id, const double* params, int K, int N, const double* X, const double* U,
                               const double* sigma, int S, int sub, int pos_dim, double* P, double* L, void* stream);

/* scvx_rollout_dense_batched for a runtime-compiled user model (scvx_rtc_model_create): the same kernel body
 * (csrc/foh_body.hpp rollout_dense_body) on the model's own f, with the same argument rules (n = the model's n_x,
 * which may be 1 or 2) and the same outputs, so the separation scan, the obstacle scan and the continuous-time rows
 * built on P / L serve any model.  params / n_params as scvx_rtc_foh_batched.  (added to version 7) */
int scvx_rtc_rollout_dense_batched(const scvx_rtc_model* model, const double* params, int n_params, int K, int N,
                                   const double* X, const double* U, const double* sigma, int S, int sub,
                                   int pos_dim, double* P, double* L, void* stream);

/*
 * Continuous-time closest approach on those samples.  For local agents [i0, i0 + N_local) of P_all
 * [N_total][K-1][S+1][3] / L_all [N_total][K-1] (all-gathered, as X_all of scvx_collision_rows_batched) and
 * every segment k: the minimum over j != i and sub-intervals s < S, at equal normalised time, of the chord
 * closest approach
 *     d0 = p_i(s) - p_j(s), d1 = p_i(s+1) - p_j(s+1), e = d1 - d0,
 *     a = 0 if e.e == 0 else clamp(-d0.e / e.e, 0, 1),   dist = ||d0 + a e||.
 * Outputs: sep [N_local][K-1], arg [N_local][K-1][2] int32 = (j, s), alpha [N_local][K-1] = a.  The scan runs
 * j ascending, then s ascending, and a candidate replaces the kept one only when strictly smaller: the first
 * minimum.  N_total == 1: sep = +inf, arg = (-1, -1).  Exact for the piecewise-linear interpolant of the
 * samples; within max ||r''|| h^2 / 8 of the continuous minimum (r the relative position, h the sub-interval).
 * flags: 0; bit 0 (tests only) disables the skip of neighbours whose |d(s=0)| - (L_i + L_j) cannot be
 * strictly smaller than the kept minimum -- the outputs are bit-identical either way.
 */
int scvx_separation_scan_batched(int K, int S, int N_total, const double* P_all, const double* L_all, int i0,
                                 int N_local, double* sep, int32_t* arg, double* alpha, int flags, void* stream);

/* min_inter_agent_distance (SCvx/utils/analysis.py:10-31): D [N][N] = min_k ||X_i[0:rows, k] - X_j[0:rows, k]||
 * over the K nodes of X [N][K][n_x]; symmetric, zero diagonal.  rows <= 3 (the reference takes rows 0:3 of
 * whatever state it is given, the unicycle's heading included). */
int scvx_pair_min_distance_batched(int K, int n_x, int rows, int N, const double* X, double* D, void* stream);

/* min_agent_obstacle_distance (analysis.py:34-62): D [N][n_obs] = min_k (||X_i[0:3, k] - c_o|| - (robot_radius +
 * r_o)); centers [n_obs][3], radii [n_obs] (device).  n_x >= 3. */
int scvx_obstacle_min_distance_batched(int K, int n_x, int N, const double* X, int n_obs, const double* centers,
                                       const double* radii, double robot_radius, double* D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Continuous-time (inter-sample) collision rows for the Jacobi QP (csrc/intersample_rows.hip):
 * the pair scan above fed back into the subproblem.  Two entry points added to revision 7; no existing
 * argument list changed.
 * ------------------------------------------------------------------------------------------ */

/*
 * Per local agent i in [i0, i0 + N_local) and segment k < K-1, the J neighbours that come closest strictly
 * between the two nodes, on the samples P_all [N_total][K-1][S+1][3] / L_all [N_total][K-1] of
 * scvx_rollout_dense_batched.  A pair's closest approach on the segment is the chord formula of
 * scvx_separation_scan_batched over its own S sub-intervals (first minimum over s, replaced only when strictly
 * smaller): (s, a), c = d0 + a e, dist = ||c||, alpha' = (s + a) / S.  The pair is a candidate when
 *     dist < cull,   0 < alpha' < 1 (a minimum at a node belongs to the node rows),   dist > 0
 * (coincident chords have no direction and are dropped; the comparisons are made on dist^2 against cull^2).
 * The J candidates of smallest dist are kept, ties to the lower j, and written in ascending (dist, j) order:
 *     rec   [N_local][K-1][J][4]   g = c / dist (3 doubles, zeros past pos_dim as P_all), v = 2R - dist
 *     nbr   [N_local][K-1][J]      int32 j            alpha [N_local][K-1][J]   alpha'
 *     count [N_local][K-1]         int32 records kept; slots past it hold zeros, nbr -1
 * The output does not depend on the launch geometry: a shard (i0, N_local) returns the matching rows of the full
 * launch bit for bit.  flags: 0; bit 0 (tests only) disables the skip of neighbours with
 * ||d(s=0)|| - (L_i + L_j) >= cull (1 + 1e-12), which cannot be candidates -- bit-identical outputs either way.
 * Limits: K <= 64, 1 <= S <= 16, 1 <= J <= 8, cull > 0.
 */
int scvx_intersample_pair_rows_batched(int K, int S, int N_total, const double* P_all, const double* L_all, int i0,
                                       int N_local, double R, double cull, int J, double* rec, int32_t* nbr,
                                       double* alpha, int32_t* count, int flags, void* stream);

/*
 * Append those records to the node rows of scvx_collision_rows_batched / _indexed.  A record of segment k becomes
 * two node rows, at node k and at node k+1, each g'(p_t - pbar_t) >= v - S_t, i.e. in the QP's form
 * b - g' p_t <= S_t with b = v + g' pbar_t, pbar_t = X_all[i][t][0:pos_dim] (summed left to right, unfused).
 * Shifting both end nodes along g by the deficit shifts every point of the node chord by as much, so the
 * first-order image of the closest point clears 2R.  For local agent a and node t < K-1, behind the count[a][t]
 * rows already present: segment t's records first, then segment t-1's.  No row at node K-1.  Never writes past
 * j_max rows per node; *overflow (one device int32, accumulated, zeroed by the caller) counts the rows that did
 * not fit.  idx NULL: local agent a is global agent i0 + a and reads rec / count_seg [a].  idx (device int32
 * [N_local], as scvx_collision_rows_indexed): local agent a is global agent idx[a] and reads rec / count_seg
 * [idx[a] - i0], which the caller guarantees to lie inside those buffers.
 *   rows [N_local][K][j_max][pos_dim+1], count [N_local][K] (in / out), rec [.][K-1][J][4], count_seg [.][K-1].
 */
int scvx_collision_rows_append_batched(int K, int pos_dim, int n_x, int N_total, const double* X_all, int i0,
                                       const int32_t* idx, int N_local, int J, const double* rec,
                                       const int32_t* count_seg, int j_max, double* rows, int32_t* count,
                                       int32_t* overflow, void* stream);

/* ------------------------------------------------------------------------------------------
 * Continuous-time agent-obstacle clearance and obstacle rows for the Jacobi QP (csrc/obstacle_rows.hip,
 * DESIGN §3.8).  One entry point added to revision 7; no existing argument list changed.
 * ------------------------------------------------------------------------------------------ */

/*
 * Per agent and segment k < K-1 of the samples P [N][K-1][S+1][3] of scvx_rollout_dense_batched, against the
 * obstacles centers [O][3] / rho [O] (device; rho the total radius, obstacle plus robot; O >= 1, no upper limit):
 * obstacle o's closest approach on the segment is the chord formula of scvx_separation_scan_batched with
 * d_s = p_s - c_o over the S sub-intervals (first minimum over s, replaced only when strictly smaller): (s, a),
 * c = d0 + a e, dist = ||c||, alpha' = (s + a) / S, v = rho_o - dist.
 * Analysis outputs (both or neither):
 *     dist  [N][K-1][O]   alpha [N][K-1][O] = alpha'
 * Record outputs (all four with 1 <= J <= 8, none with J = 0).  Obstacle o is a candidate when
 *     v > -cull,   0 < alpha' < 1 (a minimum at a node belongs to the node rows),   dist > 0;
 * the J candidates of largest v are kept, ties to the lower o, and written in descending (v, then ascending o)
 * order in the layout of scvx_intersample_pair_rows_batched, so that scvx_collision_rows_append_batched turns
 * them into node rows g'(p_t - pbar_t) >= v - S_t unchanged:
 *     rec   [N][K-1][J][4]   g = c / dist (3 doubles, zeros past pos_dim when P and the centres hold zeros there), v
 *     obs   [N][K-1][J]      int32 o            rec_alpha [N][K-1][J]   alpha'
 *     count [N][K-1]         int32 records kept; slots past it hold zeros, obs -1
 * Every (agent, segment) is computed on its own: a slice of P returns the matching rows of the full launch bit
 * for bit.  Limits: K >= 2, 1 <= S <= 16, 0 <= J <= 8; with records K <= 64 (the append's) and cull > 0.
 */
int scvx_obstacle_scan_batched(int K, int S, int N, const double* P, int O, const double* centers, const double* rho,
                               double cull, int J, double* dist, double* alpha, double* rec, int32_t* obs,
                               double* rec_alpha, int32_t* count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Moving obstacles: tracked centres in the clearance scan and the QP rows (csrc/moving_obstacles.hip,
 * DESIGN §3.9).  Two entry points added to revision 7; no existing argument list changed.
 * ------------------------------------------------------------------------------------------ */

/*
 * scvx_obstacle_scan_batched against centres that move.  Track o (device arrays): n_knots[o] in 1..M_max knots
 * knots [O][M_max][3] (zero-padded past the position dimension, entries past n_knots[o] unread), equally spaced
 * over the real-time window window [O][2] = (t0, t1), t1 > t0; total radius rho [O].  Its position is
 *     one knot:   q_o(t) = c_0 (the window is not read)
 *     otherwise:  u = clamp((t - t0) w, 0, n - 1), w = (n - 1) / (t1 - t0), m = min(floor(u), n - 2),
 *                 q_o(t) = c_m + (u - m)(c_{m+1} - c_m):  at rest at c_0 before t0 and at c_{n-1} after t1.
 * The caller guarantees n_knots and the window rule (the entry point reads no device memory; the kernel clamps
 * n_knots into 1..M_max so that nothing outside the arrays is read).  Agent i lives on its own clock: sample s of
 * segment k of P [N][K-1][S+1][3] is at t = sigma[i] (k S + s) / ((K-1) S), formed as (sigma[i] / ((K-1) S)) (k S + s).
 * Obstacle o's closest approach on a segment is the chord formula of scvx_obstacle_scan_batched on the relative
 * samples d_s = p_s - q_o(t_s): exact for the piecewise-linear interpolant of the relative samples.  With one knot
 * per obstacle every output is scvx_obstacle_scan_batched's bit for bit.
 * Analysis outputs (both or neither):   dist [N][K-1][O], alpha [N][K-1][O] = alpha'.
 * Segment records (all four or none): scvx_obstacle_scan_batched's rec, obs, rec_alpha, count under its rule
 *     v = rho_o - dist > -cull,   0 < alpha' < 1,   dist > 0;   the J of largest v, descending (v, then ascending o).
 * Node records (all three or none), which the QP kernel cannot hold for a centre that moves: for the segment's first
 * node (sample 0; node K-1 gets none) the J obstacles of largest v = rho_o - ||d_0|| with v > -cull and
 * ||d_0|| > 0, in the same order:
 *     node_rec [N][K-1][J][4] = (d_0 / ||d_0||, v)   node_obs [N][K-1][J] int32 o   node_count [N][K-1] int32
 * (slots past the count hold zeros, obs -1).  J >= 1 exactly when segment or node records are asked for.  Every
 * (agent, segment) is computed on its own: a slice of P and sigma returns the matching rows bit for bit.
 * Limits: K >= 2, 1 <= S <= 16, O >= 1, M_max >= 1, 0 <= J <= 8; with records K <= 64 and cull > 0.
 */
int scvx_moving_obstacle_scan_batched(int K, int S, int N, const double* P, const double* sigma, int O, int M_max,
                                      const double* knots, const int32_t* n_knots, const double* window,
                                      const double* rho, double cull, int J, double* dist, double* alpha, double* rec,
                                      int32_t* obs, double* rec_alpha, int32_t* count, double* node_rec,
                                      int32_t* node_obs, int32_t* node_count, void* stream);

/*
 * Append those node records: for local agent a and node t < K-1, behind the count[a][t] rows already present, record
 * r of node_rec[.][t] becomes the row g'(p_t - pbar_t) >= v - S_t, i.e. (g, b = v + g' pbar_t), pbar_t =
 * X_all[i][t][0:pos_dim] (summed left to right, unfused).  No row at node K-1.  Arguments, idx form, j_max and
 * *overflow as scvx_collision_rows_append_batched.
 *   rows [N_local][K][j_max][pos_dim+1], count [N_local][K] (in / out), node_rec [.][K-1][J][4], node_count [.][K-1].
 */
int scvx_node_rows_append_batched(int K, int pos_dim, int n_x, int N_total, const double* X_all, int i0,
                                  const int32_t* idx, int N_local, int J, const double* node_rec,
                                  const int32_t* node_count, int j_max, double* rows, int32_t* count,
                                  int32_t* overflow, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCVX_HIP_H */
