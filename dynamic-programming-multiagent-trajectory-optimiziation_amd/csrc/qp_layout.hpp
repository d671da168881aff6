// Per-agent memory layout of the batched QP kernel (csrc/qp_ipm.hpp), stated once for host and device: the capacity
// class <NX, NU, NB, NO, NC, VC> fixes every offset of the LDS packet, the global packet, the factor block, the
// workspace columns and the LDS regions.  The kernel reads them from QPCfg<...>::L at compile time; the host asks
// qp_layout(...) of the same six numbers for the workspace and LDS sizes, so a runtime-compiled class (user models,
// csrc/subproblem_rtc.hip), which has no QPCfg instantiation on the host, is sized by the formulas its kernel indexes.
// Also holds the kernel's argument block and the limits of a class (qp_class_error).
// Host, device and hipRTC clean: nothing but scvx_hip.h is included.
#pragma once
#include "scvx_hip.h"

namespace scvx {

struct QPArgs {
    scvx_qp_template T;
    int N;
    const double* disc;
    const double* sigma;
    const double* Xref;
    const double* Uref;
    const double* x_init;
    const double* x_final;
    const double* tr;
    const double* coll_rows;
    const int32_t* coll_count;
    const int32_t* warm; // per agent: start from the state this workspace holds from the agent's last solve
    double* X;
    double* U;
    double* slack_coll;
    double* nu;          // virtual control [N][K-1][n] (w_nu > 0 classes)
    double* obj;
    int32_t* status;
    int32_t* iters;
    double* ws;          // workspace
    long long ws_agent;  // doubles per agent
    double* trace;       // optional per-iteration diagnostics of agent `trace_agent` (or nullptr)
    int trace_agent, trace_cap;
    const int32_t* order;  // optional dispatch order: workgroup b solves agent order[b] (nullptr: agent b)
    // host side only (the split launch, qp_capi.hip qp_launch_split; the kernel reads none of them): tail_n > 0 runs
    // the agents of order_tail[tail_n] in a launch of their own with the LDS request of tail_reserve, `order` the rest
    const int32_t* order_tail;
    int tail_n, tail_reserve;
};

// byte offset of every access of a lane without a node (t >= K): beyond num_records of any workspace
constexpr int QP_OOB = 0x40000000;
// chunked solve chains (NX <= 8): the K-1 transitions are cut into QP_NCH chunks, one per 8-lane group; a
// chunk holds at most QP_CLM transitions (K <= 64)
constexpr int QP_NCH = 8, QP_CLM = 8;
// solve-chain prefetch depth (stages of Acl / offsets held in registers ahead of the chain)
constexpr int QP_CPF = 4;

constexpr int qp_dstr(int nx, int nu) { return nx * (nx + 2 * nu + 2); }
// stiff trust-region facets (the coupled classes, n <= 8, 2 <= m <= 4; see QPLay::STF): the 2^m facet weights, their
// folded sum (diagonal and upper off-diagonals of sum_f D_f g_f g_f') and their maximum ride in the packet; at most
// m-1 of them stay explicit per stage
constexpr bool qp_stf(int nx, int nu, int nc) { return nx <= 8 && nu >= 2 && nu <= 4 && nc > 0; }
constexpr int qp_pm(int nx, int nu, int nc) { return qp_stf(nx, nu, nc) ? nu - 1 : 0; }
constexpr int qp_nfd(int nx, int nu, int nc) { return qp_stf(nx, nu, nc) ? (1 << nu) + 2 + nu * (nu - 1) / 2 : 0; }
constexpr int qp_even(int x) { return (x + 1) & ~1; }

// Every member is a function of the class alone (filled by qp_layout below); only lds_doubles / ws_doubles take K.
struct QPLay {
    int NX, NU, NB, NO, NC, VC;
    // VC = 1: the virtual-control class (scvx_qp_template.w_nu > 0): nu_t in every dynamics row, priced
    // w_nu ||nu_t||_1 through its epigraph -e <= nu <= e.  nu is eliminated inside each Riccati stage
    // (G = D + P_{t+1}, D = the node's nu curvature after e is eliminated), e and the 2 n rows per node
    // live in workspace columns, not in the LDS row state.
    int NV, NVA;   // NV = VC ? NX : 0; NVA = max(NV, 1) (array bounds)
    int NZ, NQ, NTR;
    int NS;        // soft halfspace rows
    int NG;        // slack groups (one per obstacle, one shared)
    int R_BOX, R_OBS, R_COL, R_GRP, NR;
    int DSTR;
    // stiff trust-region facets (STF: the coupled classes, n <= 8 and 2 <= m <= 4): the node's R leaves the 2^m
    // facets' D g g' out; their weights D_f, their folded sum and max ride in the packet (P_FD) and factor phase 3
    // folds them back into Rhat, all but at most PM = m-1 stiff ones, which stay explicit stage unknowns (Woodbury;
    // see the factor).  The uncoupled classes (C3) fold the facets into R as before: no stiff facet has failed a
    // C3 solve, and the stage work costs ~13 % of an IPM iteration there (round 5 A/B).
    bool STF;
    int NFD, PM, PMA;
    // packet: the facet weights | their folded sum (diagonal, upper off-diagonals) | their maximum
    int NFO;
    // factor packet [t][PKT]: node Hessian Q|S|R, e, then the constant A (column-major) | Bt
    // column-major | Bt row-major | C_{t-1} (column-major).  Every dot product of the factor
    // phases then reads two contiguous LDS vectors.
    int P_Q, P_S, P_R, P_E, P_A, P_BT, P_BTR, P_C, P_D, P_FD, PKT;
    // global packet (compact, n <= 8): Q diagonal | Q position-block off-diagonals (0,1) (0,2) (1,2) |
    // S | R upper packed | e | A (column-major) | Bt (column-major) | C_{t-1} (column-major) | D -- expanded to
    // the LDS packet layout by the factor's prefetch through a per-lane gather table (qp_gsrc)
    int G_QD, G_QO, G_S, G_R, G_E, G_A, G_BT, G_C, G_D, G_FD;
    // n = 12 (DPK): the global packet has the LDS layout element for element.  The compact form needs a per-lane
    // gather table of PFN offsets live across the factor sweep; at n = 12 the register allocator spilled it to
    // scratch, and every reload waited for the packet prefetches in flight.  The dense prefetch is one
    // contiguous load per 64 elements; Q's structural zeros are written once per solve (setup), with the
    // constant A | Bt | Bt row-major | C_{t-1}; the node phase writes Q's nonzeros (both triangles), S, R (both
    // halves), e, D.  (n <= 8 keeps the compact form: its 3-entry table costs nothing, the dense packet's extra
    // traffic does: C3 780 -> 742 SCvx-it/s, A/B round 4.)
    bool DPK;
    int GPK;
    // global packet index of the node-phase outputs e, D and of the constant blocks
    int gE, gD, gS, gA, gBT, gC, gFD;
    // factor outputs: stage-major blocks [t][FBS] (coalesced stores from the element-parallel factor; each
    // lane-parallel pass reads its own stage's block).  Every sub-block starts on an even element (one padding double
    // after a sub-block of odd size; the small block W | C^-1 | indices stays contiguous) and the block size is even:
    // with the 16-byte region bases of ws_doubles the lane-parallel passes read a sub-block two doubles per load
    // (C3: 178 -> 180 doubles)
    int B_K;      // K      NU x NX
    int B_KAP;    // kappa  NU x NX
    int B_LD;     // LDL' of Rhat: L[i][j] (i > j), 1/d_i on the diagonal
    int B_W2;     // W2 = Bt' Pi_{t+1}  NU x NX
    int B_P;      // P_t
    int B_PI;     // Pi_t
    int B_U;      // P_{t+1} e_t
    int B_ACL;    // Acl_t = A_t + Bt_t K_t (row-major)
    // virtual control (VC): G^-1 P_{t+1}, G^-1 Pi_{t+1}, G^-1 (column-major), the chain matrix
    // Acl~ = G^-1 D Acl (row-major)
    int B_YP, B_YPI, B_GI, B_ACL2;
    int B_CH;     // what the solve chains read
    // stiff facets (STF): Gamma = -C^-1 G' R0^-1 Sh and Gamma_kappa = -C^-1 G' R0^-1 W2 (PM x NX, row-major: the
    // multiplier steps nu = Gamma xi + Gamma_kappa mu + gamma0), then W = R0^-1 G (NU x PM), C^-1 (PM x PM) and the
    // stiff facets' indices (PM, -1 = empty slot)
    int B_GAM, B_GAK, B_WS, B_CI, B_SF;
    int NSMB;     // W | C^-1 | indices: one small block
    int B_JNK;    // junk slot (stores of lanes without an output)
    int FBS;
    // stage-minor workspace columns (K doubles each: one per node)
    int C_DT;     // disc, transposed: A (col-major) | B | C | S | z
    int C_BT;     // Bt_t (row-major)
    int C_SOFT;   // soft rows (g0, g1, g2, b)
    int C_GRP;    // per group: Hpa/Haa (3), 1/Haa
    int C_RD;     // dual residual (x, u part)
    int C_R1A;    // group part of the current Newton rhs
    int C_CP;     // predictor products ds_a dl_a per row
    int C_UB;     // reference input ubar_t
    // node state
    int C_Z, C_Y, C_SQ, C_LQ, C_AV;
    // SOC scaling of the current iteration: w (NQ), eta, W lam (NQ), rc (NQ), rho (NQ)
    int C_WV, C_ETA, C_LTQ, C_RCQ, C_RHO;
    // virtual control state (lanes t < K-1): nu, e, slacks s1 s2 and duals l1 l2 of the rows nu - e <= 0,
    // -nu - e <= 0, the e part of the Newton rhs, the predictor products of the two rows, the dual residual
    // (nu, e parts)
    int C_VN, C_VE, C_VS, C_VL, C_VRE, C_VCP, C_VRD;
    // warm start: the row duals lambda_r at the last iterate (NR), and y_init (lanes 0..NX-1) / y_fin (lanes
    // NX..2NX-1) in one column (needs K >= 2 NX: the host checks)
    int C_WL, C_WY;
    // row slacks / duals: LDS [r][lane] for n <= 8; for the n = 12 classes workspace columns (their 49 rows
    // took 50 KB of LDS per agent, two waves per CU; in columns the class runs four)
    bool ROWG;
    int C_RS, C_RL, NCOL;
    // n = 12 classes: the factor's per-lane phase descriptors, [repetition][lane] x 16 bytes (QPRepC + pad), after
    // the factor blocks (agent-independent, rewritten at each sweep; see the factor sweep): NREP repetitions
    int NREP;
    // LDS (doubles, compile-time offsets except the K-sized blocks at the end):
    // factor: the current stage's packet, P', Pi' (col-major), T1, T2 (col-major), W1, W2 (col-major), Qh,
    // Sh (col-major), Rh, [K | kappa] (col-major), sink,
    // virtual control: G^-1 P, G^-1 Pi (column-major), Z = G^-1 D (row-major), Acl (column-major)
    int F_RING, F_PP, F_PIP, F_T1, F_T2, F_W1, F_W2, F_QH, F_SH, F_RH, F_KK, F_SINK, F_YP, F_YPI, F_Z, F_ACLC, F_END;
    int L_M, L_PI0, L_XE, L_XI0, L_R2F, L_YI, L_YF, L_DYI, L_DYF, L_PIV, L_ONE, L_FLAG, L_ST, L_S, L_L, L_VAR;
    // row slacks s / duals lambda [r][lane]; then K-sized: chain offsets g/f [K][NX], chain vectors [K+1][NX];
    // then (chunked solve chains, NX <= 8) the chunk transition matrices Phi_c [QP_NCH][NX][NX]
    bool CHK;

    constexpr int lds_doubles(int K) const { return L_VAR + K * NX + (K + 1) * NX + (CHK ? QP_NCH * NX * NX : 0); }
    // descriptor table of the n = 12 classes (doubles)
    constexpr int dtab_doubles() const { return DPK ? NREP * 64 * 2 : 0; }
    // per agent: columns [c][K], packets [K][GPK], factor blocks [K][FBS], each region from a 16-byte boundary (the
    // column and the packet region rounded up to an even number of doubles: odd K) -- only the K nodes: lanes >= K
    // address past the end of the buffer (loads read 0, stores are dropped), so the agent's footprint is
    // what its nodes touch (C3: 1024 agents x 233 KB stay inside the 256 MB Infinity Cache); then the descriptor table
    constexpr long long ws_doubles(int K) const {
        return (long long)qp_even(K * NCOL) + qp_even(K * GPK) + (long long)K * FBS + dtab_doubles();
    }
};

constexpr QPLay qp_layout(int nx, int nu, int nb, int no, int nc, int vc) {
    QPLay L{};
    L.NX = nx; L.NU = nu; L.NB = nb; L.NO = no; L.NC = nc; L.VC = vc;
    L.NV = vc ? nx : 0; L.NVA = L.NV > 0 ? L.NV : 1;
    L.NZ = nx + nu; L.NQ = nu + 1; L.NTR = 1 << nu;
    L.NS = no + nc;
    L.NG = no + (nc > 0 ? 1 : 0);
    L.R_BOX = L.NTR; L.R_OBS = L.NTR + 2 * nb; L.R_COL = L.R_OBS + no; L.R_GRP = L.R_COL + nc;
    L.NR = L.R_GRP + L.NG;
    L.DSTR = qp_dstr(nx, nu);
    L.STF = qp_stf(nx, nu, nc);
    L.NFD = qp_nfd(nx, nu, nc); L.PM = qp_pm(nx, nu, nc); L.PMA = L.PM > 0 ? L.PM : 1;
    L.NFO = nu * (nu - 1) / 2;
    const int NV = L.NV, PM = L.PM, NZ = L.NZ, NQ = L.NQ, NR = L.NR, NS = L.NS, NG = L.NG;
    int o = 0;
    auto take = [&](int sz) { const int r = o; o += sz; return r; };
    // a sub-block that starts on an even element
    auto take2 = [&](int sz) { o = qp_even(o); return take(sz); };

    // LDS packet
    o = 0;
    L.P_Q = take(nx * nx); L.P_S = take(nx * nu); L.P_R = take(nu * nu); L.P_E = take(nx);
    L.P_A = take(nx * nx); L.P_BT = take(nx * nu); L.P_BTR = take(nx * nu); L.P_C = take(nx * nu);
    L.P_D = take(NV); L.P_FD = take(L.NFD);
    L.PKT = o;
    // global packet
    o = 0;
    L.G_QD = take(nx); L.G_QO = take(3); L.G_S = take(nx * nu); L.G_R = take(nu * (nu + 1) / 2); L.G_E = take(nx);
    L.G_A = take(nx * nx); L.G_BT = take(nx * nu); L.G_C = take(nx * nu); L.G_D = take(NV); L.G_FD = take(L.NFD);
    L.DPK = nx > 8;
    L.GPK = L.DPK ? L.PKT : o;
    L.gE = L.DPK ? L.P_E : L.G_E; L.gD = L.DPK ? L.P_D : L.G_D; L.gS = L.DPK ? L.P_S : L.G_S;
    L.gA = L.DPK ? L.P_A : L.G_A; L.gBT = L.DPK ? L.P_BT : L.G_BT; L.gC = L.DPK ? L.P_C : L.G_C;
    L.gFD = L.DPK ? L.P_FD : L.G_FD;
    // factor block
    o = 0;
    L.B_K = take2(nu * nx); L.B_KAP = take2(nu * nx); L.B_LD = take2(nu * nu); L.B_W2 = take2(nu * nx);
    L.B_P = take2(nx * nx); L.B_PI = take2(nx * nx); L.B_U = take2(nx); L.B_ACL = take2(nx * nx);
    L.B_YP = take2(NV * nx); L.B_YPI = take2(NV * nx); L.B_GI = take2(NV * nx); L.B_ACL2 = take2(NV * nx);
    L.B_CH = NV > 0 ? L.B_ACL2 : L.B_ACL;
    L.B_GAM = take2(PM * nx); L.B_GAK = take2(PM * nx);
    L.B_WS = take2(nu * PM); L.B_CI = take(PM * PM); L.B_SF = take(PM);
    L.NSMB = nu * PM + PM * PM + PM;
    L.B_JNK = take(1);
    L.FBS = qp_even(o);
    // workspace columns
    o = 0;
    L.C_DT = take(L.DSTR); L.C_BT = take(nx * nu); L.C_SOFT = take(4 * NS); L.C_GRP = take(4 * NG);
    L.C_RD = take(NZ); L.C_R1A = take(NG); L.C_CP = take(NR); L.C_UB = take(nu);
    L.C_Z = take(NZ); L.C_Y = take(nx); L.C_SQ = take(NQ); L.C_LQ = take(NQ); L.C_AV = take(NG);
    L.C_WV = take(NQ); L.C_ETA = take(1); L.C_LTQ = take(NQ); L.C_RCQ = take(NQ); L.C_RHO = take(NQ);
    L.C_VN = take(NV); L.C_VE = take(NV); L.C_VS = take(2 * NV); L.C_VL = take(2 * NV); L.C_VRE = take(NV);
    L.C_VCP = take(2 * NV); L.C_VRD = take(2 * NV);
    L.C_WL = take(NR); L.C_WY = take(1);
    L.ROWG = nx > 8;
    L.C_RS = take(L.ROWG ? NR : 0); L.C_RL = take(L.ROWG ? NR : 0);
    L.NCOL = o;
    // the factor phases' repetitions per lane: phase 1, phases 2 and 3, phase 4 (the kernel asserts its own count)
    L.NREP = (2 * nx * nx + 2 * nx * nu + 2 * nx + 63) / 64 + (nx * nx + nu * nx + nu * nu + 63) / 64 +
             (4 * nx * nx + 63) / 64;
    // LDS
    o = 0;
    L.F_RING = take(L.PKT); L.F_PP = take(nx * nx); L.F_PIP = take(nx * nx); L.F_T1 = take(nx * nx);
    L.F_T2 = take(nx * nu); L.F_W1 = take(nx * nx); L.F_W2 = take(nu * nx); L.F_QH = take(nx * nx);
    L.F_SH = take(nu * nx); L.F_RH = take(nu * nu); L.F_KK = take(2 * nu * nx); L.F_SINK = take(nx > 8 ? nx : 8);
    L.F_YP = take(NV * nx); L.F_YPI = take(NV * nx); L.F_Z = take(NV * nx); L.F_ACLC = take(NV * nx);
    L.F_END = qp_even(o);
    o = L.F_END;
    L.L_M = take(nx * nx); L.L_PI0 = take(nx * nx); L.L_XE = take(nx); L.L_XI0 = take(nx); L.L_R2F = take(nx);
    L.L_YI = take(nx); L.L_YF = take(nx); L.L_DYI = take(nx); L.L_DYF = take(nx); L.L_PIV = take(nx);
    L.L_ONE = take(1); L.L_FLAG = take(4);
    L.L_ST = take2(16); L.L_S = take(nx > 8 ? 0 : NR * 64); L.L_L = take(nx > 8 ? 0 : NR * 64);
    L.L_VAR = o;
    L.CHK = nx <= 8;
    return L;
}

// global packet element of LDS packet element e (-1: a structural zero).  The layout is a template argument (a
// reference to a constexpr QPLay, QPCfg<...>::L), not `this`: the kernel calls it at a runtime e, and every offset
// must still be a constant expression there
template <const QPLay& L>
constexpr int qp_gsrc(int e) {
    if (L.DPK) return e;
    if (e < L.P_S) {
        const int i = e / L.NX, j = e % L.NX;
        if (i == j) return L.G_QD + i;
        if (i < 3 && j < 3) return L.G_QO + i + j - 1;  // (0,1) -> 0, (0,2) -> 1, (1,2) -> 2
        return -1;
    }
    if (e < L.P_R) return L.G_S + (e - L.P_S);
    if (e < L.P_E) {
        const int i = (e - L.P_R) / L.NU, j = (e - L.P_R) % L.NU, p = i < j ? i : j, q = i < j ? j : i;
        return L.G_R + p * L.NU - p * (p - 1) / 2 + (q - p);
    }
    if (e < L.P_A) return L.G_E + (e - L.P_E);
    if (e < L.P_BT) return L.G_A + (e - L.P_A);
    if (e < L.P_BTR) return L.G_BT + (e - L.P_BT);
    if (e < L.P_C) {
        const int i = (e - L.P_BTR) / L.NU, j = (e - L.P_BTR) % L.NU;
        return L.G_BT + j * L.NX + i;
    }
    if (e < L.P_D) return L.G_C + (e - L.P_C);
    if (e < L.P_FD) return L.G_D + (e - L.P_D);
    return L.G_FD + (e - L.P_FD);
}

// Limits of a class, for the classes compiled into the library (QPCfg asserts it) and the runtime-compiled ones
// (qp_check and scvx_rtc_subproblem_compile call it, so a class that compiles is one that launches).  nullptr when
// the class is served.  The 3 x 3 position block (n_x >= 3), the solve chains' 16-lane broadcast and the virtual
// control's Gauss-Jordan over 4 n_x lanes (n_x <= 16), 2^n_u trust-region facets (n_u <= 4), j_max <= 32, and the
// class's LDS within lds_max bytes at K (a caller without a K checks the smallest, K = 2): 64 KiB for a
// runtime-compiled class, which is launched without raising the kernel's dynamic LDS limit; QP_LDS_DEVICE for the
// classes compiled into the library (qp_launch raises the limit: the largest row capacities need ~90 KiB).
constexpr int QP_LDS_DEVICE = 160 * 1024;   // gfx950: LDS per workgroup
constexpr const char* qp_class_error(int nx, int nu, int nb, int no, int nc, int vc, int K, int lds_max = 65536) {
    if (nx < 3 || nx > 16 || nu < 1 || nu > 4) return "qp: runtime model needs 3 <= n_x <= 16 and 1 <= n_u <= 4";
    if (nb < 0 || nb > SCVX_MAX_BOX || no < 0 || no > SCVX_MAX_OBS || nc < 0 || nc > 32 || vc < 0 || vc > 1)
        return "qp: runtime class needs n_box <= 4, n_obs <= 16, j_max <= 32";
    if (8LL * qp_layout(nx, nu, nb, no, nc, vc).lds_doubles(K) > lds_max)
        return "qp: runtime class needs more than 64 KiB of LDS";
    return nullptr;
}

}  // namespace scvx
