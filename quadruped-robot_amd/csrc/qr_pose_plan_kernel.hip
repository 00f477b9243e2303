// ============================================================================
// Walk pose planner, one 64-lane wavefront per robot:
//   qrPosePlanner::Update                               quadruped/src/planner/qr_pose_planner.cpp:72-233
//   QpSolver                                            :236-279
//   ComputeG / GradientF / GradientG / HessianF / HessianG   :282-443 (ComputeF's value is never read and is not built)
//   ResetBasePose                                       include/quadruped/planner/qr_pose_planner.h:311-320
//   solve_quadprog_test                                 quadruped/extern/QuadProgpp/src/QuadProg++.cc:52-450, 849-1149
// An SQP of `loops` (20) iterations; each assembles a 6-variable QP with 3N (9 or 12) inequality rows in fp32 exactly as the reference
// writes it (contraction off, products and sums in the order stated below) and solves it in fp64 from the fp32 data with QuadProg++'s
// Goldfarb-Idnani iteration restated step for step: same factorisation, same Givens updates of J and R, same decisions, same operation
// order, so x, the working set A[] and the slot-ordered multipliers u are those of the compiled solver bit for bit.
//
// What the reference does and this kernel keeps:
//   - legs are taken in counter-clockwise order, slot c = leg {0, 2, 3, 1}[c] (ToCounterClockOrder);
//   - rBH is the planner's own constant, not the robot's hip offsets;
//   - rSP_ = 2/3 mean(stance feet) + 1/3 mean(all feet), z = bodyHight; ProjectV is the identity;
//   - with four stance feet the convexity test of :138-168 may erase one vertex;
//   - the QP matrix is GG[i][j] = (hessF - hessGSum)(j, i); QuadProg++'s Cholesky reads GG[i][j] for j >= i only, so the QP solved is
//     the mirrored LOWER triangle of the fp32 matrix hessF - hessGSum (as qr_vmc_kernel.hip records for its QP);
//   - u is indexed by working-set slot: Lambda(i) = u[i] for i < 3N, whatever slot i last held (0.0 where it never held anything);
//   - Lambda is memory (0.1 x 12 at construction, truncated to 3N by an Update).
// rBCOM = 0: rICOMoffset and every term multiplied by it are +-0 for finite inputs.  Those terms are added to accumulators that start at
// +0 (so never hold -0) or enter the QP only as products summed from +0, hence dropping them is bit-identical in every output; a
// non-finite quaternion, base position, foot position or ground pitch -- for which it would not be -- is flagged QRGPU_PP_NAN up front.
// Readings that could not be checked against a compiled qr_pose_planner.cpp (Eigen is not available): 3-term dot products and 3x3
// products are (a0 b0 + a1 b1) + a2 b2; a 4-term mean is ((a + b) + (c + d)) / 4; a float matrix divided by a double scalar divides by
// the scalar narrowed to float; pow(giNorm, 3) is the correctly rounded double cube.
//
// Lanes: the per-leg blocks (one lane per polygon vertex), the 36 matrix entries, the 3N constraint rows and the six rows of J are
// spread over lanes; the serial parts of the active set (Cholesky, R, the step lengths) run on one lane or uniformly on all.  Everything
// a later phase reads is in LDS; PP_SYNC separates the phases.  No scratch.
// QR_POSE_PLAN_HOST compiles the same statement for the host with the lanes as a loop (a CPU build to step through with a debugger).
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_wave_helpers.h"
#include "qr_kernels.h"

namespace qrgpu {

#ifdef QR_POSE_PLAN_HOST
#define PP_LANES(cond) for (int lane = 0; lane < 64; ++lane) if (cond)
#define PP_SYNC() ((void)0)
#define PP_FN inline
#else
#define PP_LANES(cond) if (cond)
#define PP_SYNC() wave_sync()
#define PP_FN __device__ __forceinline__
#endif

struct PoseWork {
    // fp32 planner state
    float q[4], rIB[3], src[3], rIF[12], rBF[12], rBH[12], rSP[3], vert[12], g[12], lam[12];
    int valid[4], contact[4];
    int N, flags, lsize;
    // per-vertex blocks of one SQP iteration
    float Sn[4][9], Dn[4][9], Hn[4][36], gfh[4][3], gft[4][3];
    float Mf[36], gradF[6], gradG[72], Gv[12];
    // fp64 QP
    double G[36], J[36], R[36], x[6], z[6], d[6], np[6], r[12], u[12], s[12], xold[6], uold[12];
    double rc[6], rs[6], rx[6];
    int rskip[6], rcol[6], nrot;
    int A[13], Aold[13];
    int iq, qpflags;
};

namespace {

PP_FN double pp_distance(double a, double b)
{
#pragma clang fp contract(off)
    const double a1 = __builtin_fabs(a), b1 = __builtin_fabs(b);
    if (a1 > b1) { const double t = b1 / a1; return a1 * __builtin_sqrt(1.0 + t * t); }
    if (b1 > a1) { const double t = a1 / b1; return b1 * __builtin_sqrt(1.0 + t * t); }
    return a1 * __builtin_sqrt(2.0);
}

// the rotations recorded in W.rc / rs / rx / rskip / rcol applied to columns (c, c + 1) of row k of J
PP_FN void pp_rotate_J_row(PoseWork &W, int k)
{
#pragma clang fp contract(off)
    for (int e = 0; e < W.nrot; ++e) {
        if (W.rskip[e]) continue;
        const int c = W.rcol[e];
        const double cc = W.rc[e], ss = W.rs[e], xny = W.rx[e];
        const double t1 = W.J[6 * k + c], t2 = W.J[6 * k + c + 1];
        const double a = t1 * cc + t2 * ss;
        W.J[6 * k + c] = a;
        W.J[6 * k + c + 1] = xny * (t1 + a) - t2;
    }
}

// delete_constraint (QuadProg++.cc:963-1046) for constraint l.  Returns false when l is not in the working set (the reference throws).
PP_FN bool pp_delete_constraint(PoseWork &W, int lane, int &iq, int l)
{
#pragma clang fp contract(off)
    const double DEPS = 2.220446049250313e-16;
    int qq = -1;
    for (int i = 0; i < iq; ++i) if (qq < 0 && W.A[i] == l) qq = i;
    if (qq < 0) return false;
    const int iq0 = iq;
    PP_LANES(lane == 0) {
        for (int i = qq; i < iq0 - 1; ++i) {
            W.A[i] = W.A[i + 1];
            W.u[i] = W.u[i + 1];
            for (int j = 0; j < 6; ++j) W.R[6 * j + i] = W.R[6 * j + i + 1];
        }
        W.A[iq0 - 1] = W.A[iq0];
        W.u[iq0 - 1] = W.u[iq0];
        W.A[iq0] = 0;
        W.u[iq0] = 0.0;
        for (int j = 0; j < iq0; ++j) W.R[6 * j + iq0 - 1] = 0.0;
        const int nq = iq0 - 1;
        int nrot = 0;
        for (int j = qq; j < nq; ++j) {
            double cc = W.R[6 * j + j], ss = W.R[6 * (j + 1) + j];
            const double h = pp_distance(cc, ss);
            W.rcol[nrot] = j;
            if (__builtin_fabs(h) < DEPS) { W.rskip[nrot++] = 1; continue; }
            cc = cc / h;
            ss = ss / h;
            W.R[6 * (j + 1) + j] = 0.0;
            if (cc < 0.0) { W.R[6 * j + j] = -h; cc = -cc; ss = -ss; }
            else W.R[6 * j + j] = h;
            const double xny = ss / (1.0 + cc);
            for (int k = j + 1; k < nq; ++k) {
                const double t1 = W.R[6 * j + k], t2 = W.R[6 * (j + 1) + k];
                const double a = t1 * cc + t2 * ss;
                W.R[6 * j + k] = a;
                W.R[6 * (j + 1) + k] = xny * (t1 + a) - t2;
            }
            W.rskip[nrot] = 0; W.rc[nrot] = cc; W.rs[nrot] = ss; W.rx[nrot] = xny;
            ++nrot;
        }
        W.nrot = nrot;
    }
    PP_SYNC();
    iq = iq0 - 1;
    if (iq > 0) {
        PP_LANES(lane < 6) pp_rotate_J_row(W, lane);
        PP_SYNC();
    }
    return true;
}

// add_constraint (:892-961).  Returns false when the new column is dependent (iq has been incremented all the same, as in the reference).
PP_FN bool pp_add_constraint(PoseWork &W, int lane, int &iq, double &R_norm)
{
#pragma clang fp contract(off)
    const double DEPS = 2.220446049250313e-16;
    const int iq0 = iq;
    PP_LANES(lane == 0) {
        int nrot = 0;
        for (int j = 5; j >= iq0 + 1; --j) {
            double cc = W.d[j - 1], ss = W.d[j];
            const double h = pp_distance(cc, ss);
            W.rcol[nrot] = j - 1;
            if (__builtin_fabs(h) < DEPS) { W.rskip[nrot++] = 1; continue; }
            W.d[j] = 0.0;
            ss = ss / h;
            cc = cc / h;
            if (cc < 0.0) { cc = -cc; ss = -ss; W.d[j - 1] = -h; }
            else W.d[j - 1] = h;
            W.rskip[nrot] = 0; W.rc[nrot] = cc; W.rs[nrot] = ss; W.rx[nrot] = ss / (1.0 + cc);
            ++nrot;
        }
        W.nrot = nrot;
        for (int i = 0; i < iq0 + 1; ++i) W.R[6 * i + iq0] = W.d[i];
    }
    PP_SYNC();
    PP_LANES(lane < 6) pp_rotate_J_row(W, lane);
    PP_SYNC();
    iq = iq0 + 1;
    const double dl = W.d[iq - 1];
    if (__builtin_fabs(dl) <= DEPS * R_norm) return false;
    R_norm = R_norm > __builtin_fabs(dl) ? R_norm : __builtin_fabs(dl);
    return true;
}

// solve_quadprog_test with n = 6, p = 0, m inequality rows.  In: W.Mf (fp32 hessF - hessGSum), W.gradF, W.gradG, W.Gv.  Out: W.x, W.u,
// W.A, W.iq, W.qpflags (QRGPU_PP_NOT_PD: the Cholesky would throw, nothing else is valid; QRGPU_PP_INFEASIBLE: +inf was returned;
// QRGPU_PP_MAXITER: a bound the reference does not have).
PP_FN void pp_solve_quadprog(PoseWork &W, int lane, int m)
{
#pragma clang fp contract(off)
    const double DEPS = 2.220446049250313e-16, INF = __builtin_inf();
#define CI(j, i) ((double)W.gradG[6 * (i) + (j)])
#define CI0(i) ((double)W.Gv[i])
    PP_LANES(lane < 36) { const int i = lane / 6, j = lane - 6 * i; W.G[lane] = (double)W.Mf[6 * j + i]; W.R[lane] = 0.0; }
    PP_LANES(lane >= 36 && lane < 36 + 12) W.u[lane - 36] = 0.0;
    PP_LANES(lane >= 48 && lane < 48 + 13) W.A[lane - 48] = 0;
    PP_SYNC();
    double c1 = 0.0;
    for (int i = 0; i < 6; ++i) c1 += W.G[7 * i];
    // cholesky_decomposition (:1079-1110), then x = -G^-1 g0 (cholesky_solve :1112-1149)
    PP_LANES(lane == 0) {
        int bad = 0;
        for (int i = 0; i < 6 && !bad; ++i) {
            for (int j = i; j < 6; ++j) {
                double sum = W.G[6 * i + j];
                for (int k = i - 1; k >= 0; --k) sum -= W.G[6 * i + k] * W.G[6 * j + k];
                if (i == j) {
                    if (sum <= 0.0) { bad = 1; break; }
                    W.G[7 * i] = __builtin_sqrt(sum);
                } else W.G[6 * j + i] = sum / W.G[7 * i];
            }
            for (int k = i + 1; k < 6 && !bad; ++k) W.G[6 * i + k] = W.G[6 * k + i];
        }
        W.qpflags = bad ? QRGPU_PP_NOT_PD : 0;
        W.iq = 0;
    }
    PP_SYNC();
    if (W.qpflags & QRGPU_PP_NOT_PD) return;
    // J = L^-T, row i by forward elimination of e_i (:143-151)
    PP_LANES(lane < 6) {
        double y[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double v = (i == lane) ? 1.0 : 0.0;
            if (i == 0) v = v / W.G[0];
            else {
#pragma unroll
                for (int j = 0; j < 6; ++j) if (j < i) v -= W.G[6 * i + j] * y[j];
                v = v / W.G[7 * i];
            }
            y[i] = v;
            W.J[6 * lane + i] = v;
        }
    }
    PP_LANES(lane == 6) {
        double y[6], xx[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double v = (double)W.gradF[i];
            if (i == 0) v = v / W.G[0];
            else {
#pragma unroll
                for (int j = 0; j < 6; ++j) if (j < i) v -= W.G[6 * i + j] * y[j];
                v = v / W.G[7 * i];
            }
            y[i] = v;
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double v = y[i];
            if (i < 5) {
#pragma unroll
                for (int j = 0; j < 6; ++j) if (j > i) v -= W.G[6 * i + j] * xx[j];
            }
            v = v / W.G[7 * i];
            xx[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) W.x[i] = -xx[i];
    }
    PP_SYNC();
    double c2 = 0.0;
    for (int i = 0; i < 6; ++i) c2 += W.J[7 * i];
    double R_norm = 1.0;
    int iq = 0, ip = 0, guard = 0, flags = 0;
    unsigned excl = 0;                                                        // bit i: iaexcl[i] == false
    double ss = 0.0;
    bool done = false;
    while (!done) {                                                           // l1
        PP_LANES(lane < m) {
            double sum = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) sum += CI(j, lane) * W.x[j];
            sum += CI0(lane);
            W.s[lane] = sum;
        }
        PP_LANES(lane >= 16 && lane < 16 + 12) W.uold[lane - 16] = W.u[lane - 16];
        PP_LANES(lane >= 32 && lane < 32 + 13) W.Aold[lane - 32] = W.A[lane - 32];
        PP_LANES(lane >= 48 && lane < 48 + 6) W.xold[lane - 48] = W.x[lane - 48];
        PP_SYNC();
        double psi = 0.0;
        for (int i = 0; i < m; ++i) { const double v = W.s[i]; psi += (v < 0.0) ? v : 0.0; }
        if (__builtin_fabs(psi) <= m * DEPS * c1 * c2 * 100.0) break;
        ss = 0.0; ip = 0; excl = 0;
        bool to_l1 = false;
        while (!done && !to_l1) {                                             // l2
            unsigned active = 0;
            for (int k = 0; k < iq; ++k) active |= 1u << W.A[k];
            for (int i = 0; i < m; ++i) {
                const double v = W.s[i];
                if (v < ss && !((active >> i) & 1u) && !((excl >> i) & 1u)) { ss = v; ip = i; }
            }
            if (ss >= 0.0) { done = true; break; }
            const int ipc = ip, iqc = iq;
            PP_LANES(lane < 6) W.np[lane] = CI(lane, ipc);
            PP_LANES(lane == 6) { W.u[iqc] = 0.0; W.A[iqc] = ipc; }
            PP_SYNC();
            for (;;) {                                                        // l2a
                if (++guard > 200) { flags |= QRGPU_PP_MAXITER | QRGPU_PP_INFEASIBLE; done = true; break; }
                const int iqa = iq;
                PP_LANES(lane < 6) {
                    double sum = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; ++j) sum += W.J[6 * j + lane] * W.np[j];
                    W.d[lane] = sum;
                }
                PP_SYNC();
                PP_LANES(lane < 6) {
                    double v = 0.0;
                    for (int j = iqa; j < 6; ++j) v += W.J[6 * lane + j] * W.d[j];
                    W.z[lane] = v;
                }
                PP_LANES(lane == 6) {
                    for (int i = iqa - 1; i >= 0; --i) {
                        double sum = 0.0;
                        for (int j = i + 1; j < iqa; ++j) sum += W.R[6 * i + j] * W.r[j];
                        W.r[i] = (W.d[i] - sum) / W.R[7 * i];
                    }
                }
                PP_SYNC();
                int l = 0;
                double t1 = INF;
                for (int k = 0; k < iq; ++k) {
                    const double rk = W.r[k];
                    if (rk > 0.0) { const double qv = W.u[k] / rk; if (qv < t1) { t1 = qv; l = W.A[k]; } }
                }
                double zz = 0.0, znp = 0.0;
                for (int k = 0; k < 6; ++k) { zz += W.z[k] * W.z[k]; znp += W.z[k] * W.np[k]; }
                double t2;
                if (__builtin_fabs(zz) > DEPS) { t2 = -W.s[ip] / znp; if (t2 < 0) t2 = INF; }
                else t2 = INF;
                const double tmin = (t2 < t1) ? t2 : t1;                      // std::min(t1, t2)
                if (tmin >= INF) { flags |= QRGPU_PP_INFEASIBLE; done = true; break; }
                if (t2 >= INF) {                                              // step in dual space
                    PP_LANES(lane <= iqa) { if (lane < iqa) W.u[lane] -= tmin * W.r[lane]; else W.u[lane] += tmin; }
                    PP_SYNC();
                    if (!pp_delete_constraint(W, lane, iq, l)) { flags |= QRGPU_PP_MAXITER | QRGPU_PP_INFEASIBLE; done = true; break; }
                    continue;
                }
                PP_LANES(lane <= iqa) { if (lane < iqa) W.u[lane] -= tmin * W.r[lane]; else W.u[lane] += tmin; }
                PP_LANES(lane >= 16 && lane < 22) W.x[lane - 16] += tmin * W.z[lane - 16];
                PP_SYNC();
                if (__builtin_fabs(tmin - t2) < DEPS) {                       // full step
                    if (iq >= 6) { flags |= QRGPU_PP_MAXITER | QRGPU_PP_INFEASIBLE; done = true; break; }      // cannot happen: z = 0 with six rows
                    if (!pp_add_constraint(W, lane, iq, R_norm)) {
                        excl |= 1u << ip;
                        if (!pp_delete_constraint(W, lane, iq, ip)) { flags |= QRGPU_PP_MAXITER | QRGPU_PP_INFEASIBLE; done = true; break; }
                        const int iqn = iq;
                        PP_LANES(lane < iqn) { W.A[lane] = W.Aold[lane]; W.u[lane] = W.uold[lane]; }
                        PP_LANES(lane >= 16 && lane < 22) W.x[lane - 16] = W.xold[lane - 16];
                        PP_SYNC();
                        break;                                                // goto l2 (ss and ip keep their values)
                    }
                    to_l1 = true;
                    break;
                }
                if (!pp_delete_constraint(W, lane, iq, l)) { flags |= QRGPU_PP_MAXITER | QRGPU_PP_INFEASIBLE; done = true; break; }
                const int ipp = ip;                                           // partial step: s[ip] = CI x + ci0
                PP_LANES(lane == 0) {
                    double sum = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) sum += CI(k, ipp) * W.x[k];
                    W.s[ipp] = sum + CI0(ipp);
                }
                PP_SYNC();
            }
        }
    }
    const int iqe = iq, fl = flags;
    PP_LANES(lane == 0) { W.iq = iqe; W.qpflags = fl; }
    PP_SYNC();
#undef CI
#undef CI0
}

}  // namespace

// One robot.  ev: 1 Update, 2 ResetBasePose.  Arrays are [row][n]; g_out may be null.
PP_FN void pose_plan_robot(PoseWork &W, int lane, int rid, int n, const qrgpu_pose_plan_desc &D, int ev, int reset, const float *g_est_in, const float *g_est_out,
                           const float *g_ground, const float *g_rpy, const float *g_walk, float *g_state, float *g_cmd, float *g_out, int *g_flags)
{
#pragma clang fp contract(off)
    const size_t Ns = (size_t)n;
#define ROW(p, f) (p)[(size_t)(f) * Ns + rid]
    // ---- inputs: slot c holds leg {0, 2, 3, 1}[c]
    PP_LANES(lane < 4) {
        const int leg = (lane == 0) ? 0 : (lane == 1) ? 2 : (lane == 2) ? 3 : 1;
        const float q[4] = {ROW(g_est_in, 6), ROW(g_est_in, 7), ROW(g_est_in, 8), ROW(g_est_in, 9)};
        const float bp[3] = {ROW(g_est_out, 36), ROW(g_est_out, 37), ROW(g_est_out, 38)};
        const float p[3] = {ROW(g_est_out, 12 + 3 * leg), ROW(g_est_out, 13 + 3 * leg), ROW(g_est_out, 14 + 3 * leg)};
        float w[3];
        invert_rigid_transform(q, bp, p, w);
#pragma unroll
        for (int k = 0; k < 3; ++k) { W.rIF[3 * lane + k] = w[k]; W.rBF[3 * lane + k] = p[k]; W.rBH[3 * lane + k] = D.rBH[3 * leg + k]; }
        W.contact[lane] = ((int)ROW(g_walk, 8 + leg) == 1) ? 1 : 0;
        W.q[lane] = (lane == 0) ? q[0] : (lane == 1) ? q[1] : (lane == 2) ? q[2] : q[3];
        if (lane < 3) { const float b = (lane == 0) ? bp[0] : (lane == 1) ? bp[1] : bp[2]; W.rIB[lane] = b; W.src[lane] = b; }
    }
    PP_LANES(lane >= 16 && lane < 28) W.lam[lane - 16] = reset ? 0.1f : ROW(g_state, lane - 16);
    PP_SYNC();
    if (ev == 2) {                                                            // ResetBasePose
        PP_LANES(lane == 0) {
            const float mx = ((W.rIF[0] + W.rIF[3]) + (W.rIF[6] + W.rIF[9])) / 4.f;
            const float my = ((W.rIF[1] + W.rIF[4]) + (W.rIF[7] + W.rIF[10])) / 4.f;
            const float dest[6] = {mx, my, D.body_height, 0.f, 0.f, 0.f};
            int fl = 0;
            if (!(__builtin_isfinite(mx) && __builtin_isfinite(my))) fl = QRGPU_PP_NAN;
            if (!fl) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { ROW(g_cmd, 7 + k) = W.src[k]; ROW(g_cmd, 10 + k) = ROW(g_rpy, k); }
#pragma unroll
                for (int k = 0; k < 6; ++k) { ROW(g_cmd, 13 + k) = dest[k]; ROW(g_cmd, 19 + k) = 0.f; ROW(g_state, 20 + k) = dest[k]; }
            }
            g_flags[rid] = fl;
        }
        return;
    }
    // ---- Update: contacts, support polygon, g (:74-174)
    PP_LANES(lane == 0) {
        int fl = 0, cnt = 0;
        float sp[3] = {0.f, 0.f, 0.f};
        bool fin = __builtin_isfinite(ROW(g_ground, 7));
#pragma unroll
        for (int k = 0; k < 4; ++k) fin = fin && __builtin_isfinite(W.q[k]);
#pragma unroll
        for (int k = 0; k < 12; ++k) fin = fin && __builtin_isfinite(W.rIF[k]) && __builtin_isfinite(W.rBF[k]);
        if (!fin) fl |= QRGPU_PP_NAN;
        for (int c = 0; c < 4; ++c) {
            if (!W.contact[c]) continue;
            const float hb[3] = {W.rBH[3 * c], W.rBH[3 * c + 1], W.rBH[3 * c + 2]};
            float t[3];
            transform_vec_by_quat(W.q, hb, t);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float r = W.rIF[3 * c + k];
                W.vert[3 * cnt + k] = r;
                sp[k] += r;
                W.g[3 * cnt + k] = (W.rIB[k] + t[k]) - r;
            }
            W.valid[cnt] = c;
            ++cnt;
        }
        int N = cnt;
        if (cnt < 3) fl |= QRGPU_PP_FEW_CONTACTS;
        else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float center = ((W.rIF[k] + W.rIF[3 + k]) + (W.rIF[6 + k] + W.rIF[9 + k])) / 4.f;
                const float mean = sp[k] / (float)cnt;
                W.rSP[k] = mean * 2.f / 3.f + center / 3.f;
            }
            W.rSP[2] = D.body_height;
            if (cnt == 4) {                                                   // convexity (:138-168)
                int invalid = -1;
                for (int s = 1; s <= 2 && invalid < 0; ++s) {
                    const int dst = (s + 2) % 4;
                    const float *cp = W.vert + 3 * (s - 1), *cn = W.vert + 3 * (s + 1), *sr = W.vert + 3 * s, *ds = W.vert + 3 * dst;
                    if ((ds[0] - sr[0]) * (cp[1] - sr[1]) - (ds[1] - sr[1]) * (cp[0] - sr[0]) > 0) invalid = s - 1;
                    else if ((ds[0] - sr[0]) * (cn[1] - sr[1]) - (ds[1] - sr[1]) * (cn[0] - sr[0]) < 0) invalid = s + 1;
                }
                if (invalid >= 0) {
                    for (int v = invalid; v < 3; ++v) {
                        W.valid[v] = W.valid[v + 1];
#pragma unroll
                        for (int k = 0; k < 3; ++k) { W.vert[3 * v + k] = W.vert[3 * v + 3 + k]; W.g[3 * v + k] = W.g[3 * v + 3 + k]; }
                    }
                    N = 3;
                    fl |= QRGPU_PP_NONCONVEX;
                }
            }
            // Lambda.conservativeResize(3N): entries it does not have yet are uninitialised in the reference, 0.1 here
            int ls = reset ? 12 : (int)ROW(g_state, 12);
            ls = ls < 0 ? 0 : (ls > 12 ? 12 : ls);
            if (3 * N > ls) {
                fl |= QRGPU_PP_LAMBDA_GROWN;
                for (int i = ls; i < 3 * N; ++i) W.lam[i] = 0.1f;
            }
        }
        W.N = N;
        W.flags = fl;
    }
    PP_SYNC();
    const int N = W.N, m = 3 * N;
    if (W.flags & (QRGPU_PP_FEW_CONTACTS | QRGPU_PP_NAN)) {
        PP_LANES(lane == 0) g_flags[rid] = W.flags;
        return;
    }
    const int loops = D.loops < 1 ? 1 : (D.loops > QRGPU_POSE_MAX_LOOPS ? QRGPU_POSE_MAX_LOOPS : D.loops);
    for (int loop = 0; loop < loops; ++loop) {
        // ---- per-vertex blocks: ComputeGradientF / HessianF / G / GradientG / HessianG (:282-443)
        PP_LANES(lane < N) {
            const int c = W.valid[lane];
            const float bf[3] = {W.rBF[3 * c], W.rBF[3 * c + 1], W.rBF[3 * c + 2]};
            const float hb[3] = {W.rBH[3 * c], W.rBH[3 * c + 1], W.rBH[3 * c + 2]};
            const float fi[3] = {W.rIF[3 * c], W.rIF[3 * c + 1], W.rIF[3 * c + 2]};
            const float b[3] = {W.rIB[0], W.rIB[1], W.rIB[2]};
            const float g[3] = {W.g[3 * lane], W.g[3 * lane + 1], W.g[3 * lane + 2]};
            const float q[4] = {W.q[0], W.q[1], W.q[2], W.q[3]};
            float r[3], h[3], S[3][3], Sh[3][3], M[3][3], P1[3][3], P2[3][3];
            transform_vec_by_quat(q, bf, r);
            transform_vec_by_quat(q, hb, h);
            const float dv[3] = {b[0] - fi[0], b[1] - fi[1], b[2] - fi[2]};
            vector_to_skew_mat(r, S);
            vector_to_skew_mat(h, Sh);
            vector_to_skew_mat(dv, M);                                        // vectorToSkewMat(rIB) - vectorToSkewMat(rIF.col(i)), entry by entry
            mat3_mul(M, S, P1);
            mat3_mul(S, M, P2);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                W.gfh[lane][k] = (b[k] + r[k]) - fi[k];
                W.gft[lane][k] = dot3(S[k], dv[0], dv[1], dv[2]);
#pragma unroll
                for (int j = 0; j < 3; ++j) { W.Sn[lane][3 * k + j] = S[k][j]; W.Dn[lane][3 * k + j] = (P1[k][j] + P2[k][j]) / 2.f; }
            }
            const float g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
            const float gn = sqrtf(g2);
            const float gn3 = (float)(((double)gn * (double)gn) * (double)gn);
            float diff[3][3], h00[3][3], DS[3][3], T0[3][3], dG[3], gh[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) { diff[k][j] = g[k] * g[j]; h00[k][j] = ((k == j) ? 1.f : 0.f) / gn - diff[k][j] / gn3; }
            mat3_mul(diff, Sh, DS);
            mat3_mul(h00, Sh, T0);
            mat3_mul(M, Sh, P1);
            mat3_mul(Sh, M, P2);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                dG[j] = (((-g[0]) * Sh[0][j] + (-g[1]) * Sh[1][j]) + (-g[2]) * Sh[2][j]) / gn;
                gh[j] = (g2 > 0.f) ? g[j] / gn : g[j];                       // normalize() leaves a zero vector alone
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    W.Hn[lane][6 * k + j] = h00[k][j];
                    W.Hn[lane][6 * k + 3 + j] = (-Sh[k][j]) / gn + DS[k][j] / gn3;
                    W.Hn[lane][6 * (3 + k) + j] = -T0[j][k];
                    W.Hn[lane][6 * (3 + k) + 3 + j] = (((P1[k][j] + P2[k][j]) / 2.f) / 2.f - dG[k] * dG[j]) / gn;
                }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float a = gh[j], bq = ((-gh[0]) * Sh[0][j] + (-gh[1]) * Sh[1][j]) + (-gh[2]) * Sh[2][j];
                W.gradG[6 * (N + lane) + j] = a; W.gradG[6 * (N + lane) + 3 + j] = bq;
                W.gradG[6 * (2 * N + lane) + j] = -a; W.gradG[6 * (2 * N + lane) + 3 + j] = -bq;
            }
            W.Gv[N + lane] = gn - D.l_min;
            W.Gv[2 * N + lane] = D.l_max - gn;
        }
        PP_LANES(lane == 8) {                                                 // the shrunk polygon's half planes (ComputeG :392-435)
            float O[3], V[4][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (N == 3) O[k] = ((W.vert[k] + W.vert[3 + k]) + W.vert[6 + k]) / 3.f;
                else O[k] = (((W.vert[k] + W.vert[3 + k]) + W.vert[6 + k]) + W.vert[9 + k]) / 4.f;
            }
            const float sh = 1 - D.eps;
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int k = 0; k < 3; ++k) V[v][k] = (v < N) ? O[k] + sh * (W.vert[3 * v + k] - O[k]) : 0.f;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (v < N) {
                    float a0, a1, bs;
                    // row v: from vertex v to vertex v + 1 (cyclic)
                    const bool last = v == N - 1;
                    const float *P = V[v];
                    float Q0, Q1;
                    if (last) { Q0 = V[0][0]; Q1 = V[0][1]; }
                    else { Q0 = V[(v + 1) & 3][0]; Q1 = V[(v + 1) & 3][1]; }
                    a0 = Q1 - P[1]; a1 = P[0] - Q0; bs = P[0] * Q1 - Q0 * P[1];
                    W.gradG[6 * v] = a0; W.gradG[6 * v + 1] = a1; W.gradG[6 * v + 2] = 0.f;
                    W.gradG[6 * v + 3] = 0.f; W.gradG[6 * v + 4] = 0.f; W.gradG[6 * v + 5] = 0.f;
                    W.Gv[v] = ((a0 * W.rIB[0] + a1 * W.rIB[1]) + 0.f * W.rIB[2]) - bs;
                }
            }
        }
        PP_SYNC();
        // ---- hessF - hessGSum (36 lanes), gradientF (6 lanes)
        PP_LANES(lane < 36) {
            const int r = lane / 6, c = lane - 6 * r;
            float hf = 0.f, hg = 0.f;
            if (r < 3 && c < 3) {
                const float id = (r == c) ? 1.f : 0.f;
                for (int v = 0; v < N; ++v) hf += id;
                hf += D.omega * id;
            } else if (r < 3) { for (int v = 0; v < N; ++v) hf -= W.Sn[v][3 * r + (c - 3)]; }
            else if (c < 3) { for (int v = 0; v < N; ++v) hf += W.Sn[v][3 * (r - 3) + c]; }
            else { for (int v = 0; v < N; ++v) hf += W.Dn[v][3 * (r - 3) + (c - 3)]; }
            hf *= 2.f;
            for (int v = 0; v < N; ++v) hg += W.lam[N + v] * W.Hn[v][lane];
            for (int v = 0; v < N; ++v) hg += W.lam[2 * N + v] * (-W.Hn[v][lane]);
            W.Mf[lane] = hf - hg;
        }
        PP_LANES(lane >= 36 && lane < 42) {
            const int k = lane - 36;
            float a = 0.f;
            if (k < 3) {
                for (int v = 0; v < N; ++v) a += W.gfh[v][k];
                a += D.omega * (W.rIB[k] - W.rSP[k]);
            } else for (int v = 0; v < N; ++v) a += W.gft[v][k - 3];
            W.gradF[k] = a * 2.f;
        }
        PP_SYNC();
        pp_solve_quadprog(W, lane, m);
        if (W.qpflags & QRGPU_PP_NOT_PD) {
            PP_LANES(lane == 0) g_flags[rid] = W.flags | QRGPU_PP_NOT_PD;
            return;
        }
        // ---- the step (:194-211)
        if (g_out) {
            PP_LANES(lane < 6) ROW(g_out, 7 * loop + lane) = (float)W.x[lane];
            PP_LANES(lane == 6) ROW(g_out, 7 * loop + 6) = (float)W.iq;
            if (loop == 0) {
                PP_LANES(lane >= 16 && lane < 28) ROW(g_out, 154 + lane - 16) = (lane - 16 < m) ? (float)W.u[lane - 16] : 0.f;
                PP_LANES(lane >= 32 && lane < 44) ROW(g_out, 166 + lane - 32) = (lane - 32 < W.iq) ? (float)W.A[lane - 32] : -1.f;
            }
        }
        PP_LANES(lane == 0) {
            W.flags |= W.qpflags;
            float so3[3], dq[4], nq[4];
            const float q[4] = {W.q[0], W.q[1], W.q[2], W.q[3]};
#pragma unroll
            for (int k = 0; k < 3; ++k) { W.rIB[k] += (float)W.x[k]; so3[k] = (float)W.x[3 + k]; }
            so3_to_quat(so3, dq);
            concatenation_two_quats(dq, q, nq);
#pragma unroll
            for (int k = 0; k < 4; ++k) W.q[k] = nq[k];
        }
        PP_LANES(lane >= 16 && lane < 16 + m) W.lam[lane - 16] = (float)W.u[lane - 16];
        PP_SYNC();
        PP_LANES(lane < 4) {                                                  // rBF = RigidTransform(0, quat, rIF - rIB)
            const float q[4] = {W.q[0], W.q[1], W.q[2], W.q[3]};
            const float z3[3] = {0.f, 0.f, 0.f};
            const float p[3] = {W.rIF[3 * lane] - W.rIB[0], W.rIF[3 * lane + 1] - W.rIB[1], W.rIF[3 * lane + 2] - W.rIB[2]};
            float o[3];
            rigid_transform(q, z3, p, o);
#pragma unroll
            for (int k = 0; k < 3; ++k) W.rBF[3 * lane + k] = o[k];
        }
        PP_LANES(lane >= 8 && lane < 8 + N) {                                 // g = rIB + quat rBH - rIF
            const int v = lane - 8, c = W.valid[v];
            const float q[4] = {W.q[0], W.q[1], W.q[2], W.q[3]};
            const float hb[3] = {W.rBH[3 * c], W.rBH[3 * c + 1], W.rBH[3 * c + 2]};
            float t[3];
            transform_vec_by_quat(q, hb, t);
#pragma unroll
            for (int k = 0; k < 3; ++k) W.g[3 * v + k] = (W.rIB[k] + t[k]) - W.rIF[3 * c + k];
        }
        PP_SYNC();
    }
    // ---- ending (:217-227)
    PP_LANES(lane == 0) {
        const float q[4] = {W.q[0], W.q[1], W.q[2], W.q[3]};
        float rpy[3];
        quat_to_rpy(q, rpy);
        rpy[1] = (float)((double)(rpy[1] + ROW(g_ground, 7)) / 2.0);
        const float dest[6] = {W.rIB[0], W.rIB[1], W.rIB[2], rpy[0], rpy[1], rpy[2]};
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 6; ++k) fin = fin && __builtin_isfinite(dest[k]);
        int fl = W.flags;
        if (!fin) fl |= QRGPU_PP_NAN;
        else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { ROW(g_cmd, 7 + k) = W.src[k]; ROW(g_cmd, 10 + k) = ROW(g_rpy, k); ROW(g_state, 13 + k) = W.rIB[k]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) ROW(g_state, 16 + k) = q[k];
#pragma unroll
            for (int k = 0; k < 6; ++k) { ROW(g_cmd, 13 + k) = dest[k]; ROW(g_state, 20 + k) = dest[k]; }
            for (int i = 0; i < m; ++i) ROW(g_state, i) = W.lam[i];
            ROW(g_state, 12) = (float)m;
        }
        if (g_out) {
            for (int i = 0; i < 12; ++i) ROW(g_out, 140 + i) = (i < m) ? W.lam[i] : 0.f;
            int mask = 0;
            for (int v = 0; v < N; ++v) mask |= 1 << W.valid[v];
            ROW(g_out, 152) = (float)N;
            ROW(g_out, 153) = (float)mask;
        }
        g_flags[rid] = fl;
    }
#undef ROW
}

#ifndef QR_POSE_PLAN_HOST
// event: 0 none, 1 Update, 2 ResetBasePose, 3 Update where a leg has legState SWING and curLegState STANCE (qr_locomotion_controller.cpp:81-89);
// g_event (may be null) overrides it per robot with 0 / 1 / 2.  reset: every robot's state is first put into the constructed state (:31-69).
__global__ void __launch_bounds__(64) qr_pose_plan_kernel(int n, qrgpu_pose_plan_desc D, int event, const int *__restrict__ g_event, int reset,
                                                          const float *__restrict__ g_est_in, const float *__restrict__ g_est_out,
                                                          const float *__restrict__ g_ground, const float *__restrict__ g_rpy,
                                                          const float *__restrict__ g_walk, float *__restrict__ g_state, float *__restrict__ g_cmd,
                                                          float *__restrict__ g_out, int *__restrict__ g_flags, StageResetArgs SR)
{
    const int lane = threadIdx.x;
    const int rid = xcd_robot_index(blockIdx.x, n);
    if (rid < 0) return;
    const size_t Ns = (size_t)n;
    // the robot's own reset, uniform over its wavefront
    if (!reset && stage_masked(SR, rid)) reset = 1;
    int ev = g_event ? g_event[rid] : event;
    if (!g_event && event == 3) {
        ev = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if ((int)g_walk[(size_t)(12 + l) * Ns + rid] == 0 && (int)g_walk[(size_t)(16 + l) * Ns + rid] == 1) ev = 1;
    }
    if (ev != 1 && ev != 2) ev = 0;
    if (reset && lane < QRGPU_POSE_STATE_ROWS) {                                 // the constructor (:31-69)
        float v = 0.f;
        if (lane < 12) v = 0.1f;
        else if (lane == 12) v = 12.f;
        else if (lane < 16) v = g_est_out[(size_t)(36 + lane - 13) * Ns + rid];
        else if (lane == 16) v = 1.f;
        else if (lane >= 20 && lane < 23) v = g_est_out[(size_t)(36 + lane - 20) * Ns + rid];
        g_state[(size_t)lane * Ns + rid] = v;
    }
    if (reset) {                                                              // those stores land before lane 0's stores to the same rows at the end
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (ev == 0) return;
    __shared__ PoseWork W;
    pose_plan_robot(W, lane, rid, n, D, ev, reset, g_est_in, g_est_out, g_ground, g_rpy, g_walk, g_state, g_cmd, g_out, g_flags);
}

#endif

}  // namespace qrgpu
