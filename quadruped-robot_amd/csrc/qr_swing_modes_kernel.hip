// ============================================================================
// Swing-leg controller of the walk and position modes and the lift-off memory of all four modes, one thread per robot:
//   qrRaibertSwingLegController::Reset / Update / GetAction    quadruped/src/controllers/qr_swing_leg_controller.cpp:60-101, 104-229, 241-461
//   qrFootholdPlanner::Reset / UpdateOnce                       quadruped/src/planner/qr_foothold_planner.cpp:49-109
//   qrFootStepper (gap-crossing step plan, CheckSolution's QP)  quadruped/src/planner/qr_foot_stepper.cpp:31-202, 483-525
//   qrFootBSplinePatternGenerator + tinynurbs                   quadruped/src/controllers/qr_foot_trajectory_generator.cpp:30-163, 276-343,
//                                                               extern/tinynurbs/include/tinynurbs/core/{basis.h:25-70,163-240, evaluate.h:66-99}
// The per-robot memory (lift-off points, footholds, walk trajectories, the swingJointAnglesVelocities map, the stepper's plan queue) is
// one [QRGPU_SWING_STATE_FLOATS][n] float array; its rows are listed in include/qrgpu.h.  Every operation is the reference's, in its order
// and float / double mix, contraction off.  The reference's unqualified abs on floats (UpdateSpline :100/:105/:123, SwingFootTrajectory
// :298, StepGenerator :150) is read as std::abs(float).  The B-spline has degree 3 and the fixed knot vector of :44-47, so its basis is
// unrolled and stays in registers; the plan queue lives in the state array (a runtime-indexed private array would land in scratch).
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_wave_helpers.h"
#include "qr_kernels.h"

namespace qrgpu {

namespace {

// state rows (include/qrgpu.h, QRGPU_SWING_STATE_FLOATS)
constexpr int SS_LOCAL = 0, SS_GLOBAL = 12, SS_FH = 24, SS_SRC = 36, SS_TGT = 48, SS_H = 60, SS_BUILT = 64, SS_QANG = 65, SS_QVEL = 77, SS_MAP = 89,
              SS_OFF = 90, SS_PFLAGS = 102, SS_HEAD = 103, SS_TAIL = 104, SS_PLAN = 105;
// d_swing_flags bits (QRGPU_SW_*)
constexpr int SW_NO_TRAJ = 1, SW_PHASE = 2, SW_PLAN_EXIT = 4, SW_PLAN_EMPTY = 8, SW_PLAN_FULL = 16;
constexpr float MAXIMUM_STEP = 0.001f;                                       // config/qr_config.h:43

// the stepper's fixed knot vector, (float)(k / 6) as the constructor writes it (:44-47)
__device__ __forceinline__ float knot_at(int k)
{
    return k <= 3 ? 0.f : k == 4 ? (float)(0.3 / 6) : k == 5 ? (float)(1.3 / 6) : k == 6 ? (float)(2.5 / 6) : k == 7 ? (float)(3.0 / 6)
         : k == 8 ? (float)(4.0 / 6) : 1.f;
}

// SwingFootTrajectory(BSpline) + qrFootBSplinePatternGenerator::SetParameters / UpdateSpline / GenerateTrajectory at u, from the stored
// source, target and height: position and d/du (per unit phase) in the frame of source and target.
__device__ __forceinline__ void bspline_point(const float src[3], const float tgt[3], float height, float u, float pos[3], float vel[3])
{
#pragma clang fp contract(off)
    const float TX[9] = {-10.f, -10.3f, -13.f, -15.f, 0.f, 11.f, 10.5f, 10.2f, 10.f};
    const float TZ[9] = {0.f, 0.2f, 2.f, 7.f, 7.8f, 8.f, 4.f, 1.f, 0.f};
    const float dx = tgt[0] - src[0], dy = tgt[1] - src[1], dz = tgt[2] - src[2];
    const float theta = atan2f(dy, dx);
    const float s = sinf(theta), c = cosf(theta);
    const float e0 = (c * (dx * 100.f) + s * (dy * 100.f)) + 0.f * (dz * 100.f);
    const float e2 = (0.f * (dx * 100.f) + 0.f * (dy * 100.f)) + 1.f * (dz * 100.f);
    const float appex = height * 100.f;
    const float xRatio = fabsf(e0 - 0.f) / 20.f;
    float cx[9], cz[9];
    if (e2 >= 0.f) {                                                        // walk up (:101-117)
        const float zr = appex - (e2 - 0.f);
        const float zRatio = fabsf(appex) / 8.f, xm = (e0 + 0.f) / 2;
#pragma unroll
        for (int k = 0; k < 9; ++k) { cx[k] = TX[k] * xRatio + xm; cz[k] = TZ[k] * zRatio + 0.f; }
        cz[8] = e2;
        cz[7] = cz[8] + TZ[7] / 8 * zr;
        cz[6] = cz[8] + TZ[6] / 8 * zr;
        cz[5] = cz[8] + TZ[5] / 8 * zr;
    } else {                                                                // walk down (:119-133)
        const float zl = appex - (0.f - e2);
        const float zRatio = fabsf(appex) / 8.f, xm = (e0 + 0.f) / 2;
#pragma unroll
        for (int k = 0; k < 9; ++k) { cx[k] = TX[k] * xRatio + xm; cz[k] = TZ[k] * zRatio + e2; }
        cz[0] = 0.f;
        cz[1] = (float)((double)cz[0] + 0.2 / 8 * (double)zl);
        cz[2] = (float)((double)cz[0] + 2.0 / 8 * (double)zl);
        cz[3] = (float)((double)cz[0] + 7.0 / 8 * (double)zl);
    }
    // tinynurbs findSpan (degree 3, n = 8; the knots inside the domain are distinct, so the binary search is a count)
    int span;
    if (u > 1.f - 1.1920929e-07f) span = 8;
    else if (u < 0.f + 1.1920929e-07f) span = 3;
    else span = 3 + (u >= knot_at(4)) + (u >= knot_at(5)) + (u >= knot_at(6)) + (u >= knot_at(7)) + (u >= knot_at(8));
    // bsplineDerBasis (NURBS Book A2.3), deg 3, one derivative
    float left[4], right[4], ndu[4][4];
    ndu[0][0] = 1.f;
#pragma unroll
    for (int j = 1; j <= 3; ++j) {
        left[j] = u - knot_at(span + 1 - j);
        right[j] = knot_at(span + j) - u;
        float saved = 0.f;
#pragma unroll
        for (int r = 0; r < j; ++r) {
            ndu[j][r] = right[r + 1] + left[j - r];
            const float temp = ndu[r][j - 1] / ndu[j][r];
            ndu[r][j] = saved + right[r + 1] * temp;
            saved = left[j - r] * temp;
        }
        ndu[j][j] = saved;
    }
    float d0[4], d1[4];
#pragma unroll
    for (int j = 0; j <= 3; ++j) d0[j] = ndu[j][3];
#pragma unroll
    for (int r = 0; r <= 3; ++r) {                                          // k = 1 only: a(s1, .) is a(0, .) = {1}, a(s2, .) the new row
        const float a10 = 1.f;
        float d = 0.f, a0 = 0.f, a1 = 0.f;
        const int rk = r - 1, pk = 2;
        if (r >= 1) { a0 = a10 / ndu[pk + 1][rk]; d = a0 * ndu[rk][pk]; }
        if (r <= pk) { a1 = -a10 / ndu[pk + 1][r]; d += a1 * ndu[r][pk]; }
        d1[r] = d;
    }
#pragma unroll
    for (int j = 0; j <= 3; ++j) d1[j] *= 3.f;
    // curveDerivatives: sum of ders(k, j) * P[span - 3 + j]; y of every control point is zero
    float px = 0.f, pz = 0.f, vx = 0.f, vz = 0.f;
#pragma unroll
    for (int j = 0; j <= 3; ++j) {
        float qx = 0.f, qz = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) if (k == span - 3 + j) { qx = cx[k]; qz = cz[k]; }
        px += d0[j] * qx; pz += d0[j] * qz;
        vx += d1[j] * qx; vz += d1[j] * qz;
    }
    px = px / 100; pz = pz / 100; vx = vx / 100; vz = vz / 100;
    // RTheta^T p + Tp, RTheta^T v; RTheta = [[c, s, 0], [-s, c, 0], [0, 0, 1]]
    pos[0] = ((c * px + -s * 0.f) + 0.f * pz) + src[0];
    pos[1] = ((s * px + c * 0.f) + 0.f * pz) + src[1];
    pos[2] = ((0.f * px + 0.f * 0.f) + 1.f * pz) + src[2];
    vel[0] = (c * vx + -s * 0.f) + 0.f * vz;
    vel[1] = (s * vx + c * 0.f) + 0.f * vz;
    vel[2] = (0.f * vx + 0.f * 0.f) + 1.f * vz;
}

// solve_quadprog (QuadProg++.cc:55-420) for CheckSolution's problem: n = 1, G = 1, g0 = 0, no equalities, six inequalities
// ci[k] x + ci0[k] >= 0 with ci[k] = +-1.  For n = 1, J stays 1 and at most one constraint is active; the Goldfarb-Idnani steps reduce to
// the loop below, operation for operation.  Returns x as the solver leaves it (also when it reports infeasibility).
__device__ __forceinline__ double quadprog_1d(const double ci[6], const double ci0[6])
{
#pragma clang fp contract(off)
    double x = -0.0;
    int act = -1;
    for (int it = 0; it < 12; ++it) {
        double s[6], psi = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) { double sum = 0.0; sum += ci[k] * x; sum += ci0[k]; s[k] = sum; psi += fmin(0.0, sum); }
        if (fabs(psi) <= 6 * 2.220446049250313e-16 * 1.0 * 1.0 * 100.0) return x;
        double ss = 0.0;
        int ip = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) if (s[k] < ss && k != act) { ss = s[k]; ip = k; }
        if (ss >= 0.0) return x;
        double cip = 0.0, sip = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) if (k == ip) { cip = ci[k]; sip = s[k]; }
        if (act >= 0) {                                                       // z = 0: only a dual step, which drops the active one
            double cact = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) if (k == act) cact = ci[k];
            const double r = (0.0 + 1.0 * cip) / (0.0 + 1.0 * cact);
            if (!(r > 0.0)) return x;                                          // t1 = t2 = inf: infeasible
            act = -1;
        }
        const double z = 0.0 + 1.0 * (0.0 + 1.0 * cip);
        double t2 = -sip / (0.0 + z * cip);
        if (t2 < 0) return x;
        x += t2 * z;
        act = ip;
    }
    return x;
}

// qrFootStepper::CheckSolution (:85-116)
__device__ __forceinline__ double check_solution(const qrgpu_swing_mode_desc &M, const float cx[4], double front, double back, float fd, float fw, float bd, float bw)
{
#pragma clang fp contract(off)
    const float delta = M.foothold_delta;
    double ci[6], b[6], ci0[6];
    ci[0] = 1.0; ci[5] = -1.0;
    b[0] = -(double)delta;
    b[5] = -1. * (double)(MAXIMUM_STEP - delta);
#pragma unroll
    for (int i = 1; i < 5; ++i) {
        ci[i] = i <= 2 ? front : back;
        const double gd = i <= 2 ? fd : bd, gw = i <= 2 ? fw : bw;
        b[i] = -ci[i] * ((double)delta - (gd + gw / 2.0 * ci[i]) + (double)cx[i - 1]);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) ci0[i] = -b[i];
    const double deltaX = quadprog_1d(ci, ci0);
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if ((int)(deltaX * ci[i] * 10000) < (int)(b[i] * 10000)) return MAXIMUM_STEP;
    return deltaX;
}

// qrFootStepper::StepGenerator (:118-179); gaitFlag is bit 2 of *pflags
__device__ __forceinline__ int step_generator(const qrgpu_swing_mode_desc &M, const float cx[4], float des[4], int *pflags)
{
#pragma clang fp contract(off)
    const float delta = M.foothold_delta;
    float dn[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) { dn[l] = cx[l] + delta; des[l] = delta; }
    for (int g = 0; g < M.n_gaps; ++g) {
        const float gd = M.gap_distance[g], gw = M.gap_width;
        float fd = gd, bd = gd;
        if (g > 0) bd = M.gap_distance[g - 1];
        if (g < M.n_gaps - 1) fd = M.gap_distance[g + 1];
        float deltaX = MAXIMUM_STEP;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if (fabsf(dn[l] - gd) <= gw / 2) {
                if (l <= 1) fd = gd; else bd = gd;
#pragma unroll
                for (int i = -1; i <= 1; i += 2)
#pragma unroll
                    for (int j = -1; j <= 1; j += 2) {
                        const float x = (float)check_solution(M, cx, (double)i, (double)j, fd, gw, bd, gw);
                        deltaX = fabsf(x) < fabsf(deltaX) ? x : deltaX;
                    }
                const float step = delta + deltaX;
#pragma unroll
                for (int k = 0; k < 4; ++k) des[k] = step;
                if ((double)step < 0.001 || step >= MAXIMUM_STEP) {
                    if (*pflags & 2) return -2;
                    *pflags |= 2;
                    return -1;
                }
                return 0;
            }
        }
    }
    if (*pflags & 2) {                                                        // recovery of the cross gait
        for (int g = 0; g < M.n_gaps; ++g) {
            const float gd = M.gap_distance[g], gw = M.gap_width;
            if (fabs((double)cx[0] + (double)delta / 2.0 - (double)gd) <= (double)(gw / 2) || fabs((double)cx[3] + (double)delta / 2.0 - (double)gd) <= (double)(gw / 2))
                return 0;
        }
        des[0] = (float)((double)delta / 2.0); des[1] = delta; des[2] = delta; des[3] = (float)((double)delta / 2.0);
        *pflags &= ~2;
    }
    return 0;
}

}  // namespace

// Reset (reset != 0) and Update of the swing-leg controller and its foothold planner: the lift-off memory of every mode, the footholds
// and walk trajectories of the position and walk modes.  Optionally writes the lift-off rows the ADVANCED_TROT / VELOCITY kernels read.
__global__ void __launch_bounds__(64) qr_swing_update_kernel(int n, qrgpu_swing_mode_desc M, int reset, int stop, const float *__restrict__ g_est_in,
                                                             const float *__restrict__ g_est_out, const float *__restrict__ g_gait_out, float *__restrict__ g_st,
                                                             float *__restrict__ g_swing_in, float *__restrict__ g_swing_vel_in, float *__restrict__ g_fe_in,
                                                             int *__restrict__ g_flags, StageResetArgs SR)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
    // the lane's own reset level: the call's scalar reset wins, then the bound level of a masked robot
    if (!reset && stage_masked(SR, i)) reset = SR.level;
#define ST(f) g_st[(size_t)(f) * N + i]
    const float q[4] = {g_est_in[6 * N + i], g_est_in[7 * N + i], g_est_in[8 * N + i], g_est_in[9 * N + i]};
    const float bp[3] = {g_est_out[36 * N + i], g_est_out[37 * N + i], g_est_out[38 * N + i]};
    float Rq[3][3];                                                           // invertRigidTransform's rotation (Eigen)
    quat_to_rot(q[0], q[1], q[2], q[3], Rq);
    // feet in the base frame and GetFootPositionsInWorldFrame (:222-230), read per leg (a runtime leg index must not select a private array)
#define LOC(l, r) g_est_out[(size_t)(12 + 3 * (l) + (r)) * N + i]
#define WLD(l, r) (dot3(Rq[r], LOC(l, 0), LOC(l, 1), LOC(l, 2)) + bp[r])
    int flags = reset ? 0 : g_flags[i];
    const bool side = M.mode == 0 || M.mode == 3;                             // the rows of the VELOCITY / ADVANCED_TROT kernels
    if (reset) {
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float lc = LOC(l, r), wd = WLD(l, r);
                ST(SS_LOCAL + 3 * l + r) = lc;
                ST(SS_GLOBAL + 3 * l + r) = wd;
                if (M.mode == 1) ST(SS_FH + 3 * l + r) = (r == 0 && (l == 0 || l == 3)) ? (float)((double)wd - 0.05) : wd;
                else if (M.mode == 2) ST(SS_FH + 3 * l + r) = wd;
                else if (reset == 2) ST(SS_FH + 3 * l + r) = 0.f;
                ST(SS_OFF + 3 * l + r) = 0.f;                                 // qrFootholdPlanner::Reset: desiredFootholdsOffset = 0
                if (side && g_swing_in) g_swing_in[(size_t)(12 + 3 * l + r) * N + i] = wd;
                if (side && g_swing_vel_in) g_swing_vel_in[(size_t)(8 + 3 * l + r) * N + i] = lc;
            }
        if (side && g_fe_in) { g_fe_in[62 * N + i] = bp[0]; g_fe_in[63 * N + i] = bp[1]; }   // firstSwingBaseState
        ST(SS_MAP) = 0.f;                                                     // swingJointAnglesVelocities.clear()
        if (reset == 2) {                                                     // a constructed controller: no trajectory, an unplanned stepper
            ST(SS_BUILT) = 0.f; ST(SS_PFLAGS) = 0.f; ST(SS_HEAD) = 0.f; ST(SS_TAIL) = 0.f;
        }
    }
    float Rb[3][3];                                                           // stateDataFlow.baseRMat
    base_rmat(q, Rb);
    int built = (int)ST(SS_BUILT);
    for (int l = 0; l < 4; ++l) {
        const int nst = (int)g_gait_out[(size_t)(8 + l) * N + i], cur = (int)g_gait_out[(size_t)(16 + l) * N + i];
        bool lift;
        if (M.mode == 1) lift = (nst == 0 || nst == 4) && cur == 1 && !stop;
        else if (M.mode == 2) lift = (nst == 8 || nst == 4) && cur == 6 && !stop;
        else lift = nst == 0 && nst != cur;
        if (!lift) continue;
        const float lc[3] = {LOC(l, 0), LOC(l, 1), LOC(l, 2)};
        float wd[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) { ST(SS_LOCAL + 3 * l + r) = lc[r]; wd[r] = WLD(l, r); }
        if (side) {
            float g[3];                                                       // Rb * local: a rotation only (:186)
#pragma unroll
            for (int r = 0; r < 3; ++r) { g[r] = dot3(Rb[r], lc[0], lc[1], lc[2]); ST(SS_GLOBAL + 3 * l + r) = g[r]; }
            if (g_swing_in)
#pragma unroll
                for (int r = 0; r < 3; ++r) g_swing_in[(size_t)(12 + 3 * l + r) * N + i] = g[r];
            if (g_swing_vel_in)
#pragma unroll
                for (int r = 0; r < 3; ++r) g_swing_vel_in[(size_t)(8 + 3 * l + r) * N + i] = lc[r];
            if (M.mode == 3 && g_fe_in) { g_fe_in[62 * N + i] = bp[0]; g_fe_in[63 * N + i] = bp[1]; }
            continue;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) ST(SS_GLOBAL + 3 * l + r) = wd[r];
        // qrFootholdPlanner::UpdateOnce: position mode at leg 0 for all legs, walk mode for this leg
        if (M.mode == 2 || l == 0) {
            float off0[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) off0[k] = M.foothold_delta;            // nextFootholdsOffset row 0 (rows 1, 2 stay zero)
            if (M.terrain == 2) {                                             // GetFootholdsInWorldFrame, STAIRS (:181-202)
                if (M.mode == 2) ST(SS_FH + 3 * l) = ST(SS_FH + 3 * l) + 0.1f;
            } else if (M.n_gaps > 0) {                                        // GetOptimalFootholdsOffset (:483-525)
                int pf = (int)fminf(fmaxf(ST(SS_PFLAGS), 0.f), 3.f);
                // head / tail address the queue: clamped, so that a state array that never saw reset = 2 cannot index outside it
                int tail = (int)fminf(fmaxf(ST(SS_TAIL), 0.f), (float)QRGPU_SWING_MAX_PLAN);
                int head = (int)fminf(fmaxf(ST(SS_HEAD), 0.f), (float)tail);
                if (!(pf & 1)) {
                    head = 0; tail = 0;
                    float cx[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) cx[k] = ST(SS_FH + 3 * k);
                    const float lastD = M.gap_distance[M.n_gaps - 1];
                    while ((double)cx[3] < (double)lastD + (double)M.gap_width / 2.0) {
                        float des[4];
                        const int f = step_generator(M, cx, des, &pf);
                        if (f == -2) { flags |= SW_PLAN_EXIT; break; }        // exit(-1) in the reference
                        if (f == -1) {
                            if (tail > head) {
                                ST(SS_PLAN + 4 * (tail - 1)) = (float)((double)ST(SS_PLAN + 4 * (tail - 1)) + (double)M.foothold_delta / 2.0);
                                ST(SS_PLAN + 4 * (tail - 1) + 3) = (float)((double)ST(SS_PLAN + 4 * (tail - 1) + 3) + (double)M.foothold_delta / 2.0);
                            } else {
                                flags |= SW_PLAN_EMPTY;                      // steps.back() on an empty queue
                            }
                            cx[0] = (float)((double)cx[0] + (double)M.foothold_delta / 2.0);
                            cx[3] = (float)((double)cx[3] + (double)M.foothold_delta / 2.0);
                        } else {
                            if (tail >= QRGPU_SWING_MAX_PLAN) { flags |= SW_PLAN_FULL; break; }
#pragma unroll
                            for (int k = 0; k < 4; ++k) { ST(SS_PLAN + 4 * tail + k) = des[k]; cx[k] = cx[k] + des[k]; }
                            ++tail;
                        }
                    }
                    pf |= 1;
                }
                if (tail > head) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) off0[k] = ST(SS_PLAN + 4 * head + k);
                    ++head;
                }
                ST(SS_PFLAGS) = (float)pf; ST(SS_HEAD) = (float)head; ST(SS_TAIL) = (float)tail;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) { ST(SS_OFF + 3 * k) = off0[k]; ST(SS_OFF + 3 * k + 1) = 0.f; ST(SS_OFF + 3 * k + 2) = 0.f; }
        }
        if (M.mode == 1) {
#pragma unroll
            for (int r = 0; r < 3; ++r) ST(SS_FH + 3 * l + r) = ST(SS_FH + 3 * l + r) + ST(SS_OFF + 3 * l + r);
        } else {                                                              // walk: SwingFootTrajectory(BSpline, source, target, 1, 0.15)
            float src[3], tgt[3];
            if (M.is_sim) {
#pragma unroll
                for (int r = 0; r < 3; ++r) { src[r] = wd[r]; tgt[r] = ST(SS_FH + 3 * l + r); }
                tgt[2] = src[2] + ST(SS_OFF + 3 * l + 2);
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) src[r] = lc[r];
                tgt[0] = l <= 1 ? 0.30f : -0.17f;
                tgt[1] = (float)(-0.145 * ((l & 1) ? -1.0 : 1.0));
                tgt[2] = -0.32f;
            }
            const float lo = 0.15f + fabsf(tgt[2] - src[2]);                 // std::min(0.2f, std::max(0.1f, maxClearance + |dz|)) (:298)
            const float mx = (0.1f < lo) ? lo : 0.1f;
            const float hh = (mx < 0.2f) ? mx : 0.2f;
#pragma unroll
            for (int r = 0; r < 3; ++r) { ST(SS_SRC + 3 * l + r) = src[r]; ST(SS_TGT + 3 * l + r) = tgt[r]; }
            ST(SS_H + l) = hh;
            built |= 1 << l;
        }
    }
    ST(SS_BUILT) = (float)built;
    g_flags[i] = flags;
#undef ST
#undef LOC
#undef WLD
}

// GetAction of the position and walk modes: swing-leg selection, trajectory point, frame change, leg IK, J^-1 v, and the command loop over
// the swingJointAnglesVelocities map (entries of legs that swung earlier and are flagged now re-emit their last targets).
// g_out rows: foot position in the base frame[12], foot velocity in the base frame[12], joint angles[12], joint velocities[12], command[4].
__global__ void __launch_bounds__(64) qr_swing_action_kernel(int n, qrgpu_swing_mode_desc M, qrgpu_estimator_desc D, int stop, const float *__restrict__ g_est_in,
                                                             const float *__restrict__ g_est_out, const float *__restrict__ g_gait_out,
                                                             const float *__restrict__ g_gait_state, float *__restrict__ g_st, float *__restrict__ g_out,
                                                             int *__restrict__ g_flags)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
#define ST(f) g_st[(size_t)(f) * N + i]
#define OUT(f) g_out[(size_t)(f) * N + i]
#define GO(f) g_gait_out[(size_t)(f) * N + i]
    const float q[4] = {g_est_in[6 * N + i], g_est_in[7 * N + i], g_est_in[8 * N + i], g_est_in[9 * N + i]};
    const float bp[3] = {g_est_out[36 * N + i], g_est_out[37 * N + i], g_est_out[38 * N + i]};
    const float zero3[3] = {0.f, 0.f, 0.f};
    int flags = g_flags[i];
    int map = (int)ST(SS_MAP);
    const int built = (int)ST(SS_BUILT);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        bool swing;
        if (M.mode == 2) {
            const int det = (int)GO(20 + l), des = (int)GO(8 + l);
            swing = !(det == 1 || det == 2 || des != 8 || stop);
        } else {
            const int ls = (int)GO(12 + l);
            swing = !((ls == 1 && g_gait_state[(size_t)(20 + l) * N + i] != 0.f) || ls == 2);
        }
        if (!swing) continue;
        float pb[3], vb[3] = {0.f, 0.f, 0.f};
        if (M.mode == 1) {                                                    // XYLinear_ZParabola in the world frame, warped phase
            const float st[3] = {ST(SS_GLOBAL + 3 * l), ST(SS_GLOBAL + 3 * l + 1), ST(SS_GLOBAL + 3 * l + 2)};
            const float tg[3] = {ST(SS_FH + 3 * l), ST(SS_FH + 3 * l + 1), ST(SS_FH + 3 * l + 2)};
            float pw[3] = {0.f, 0.f, 0.f};
            swing_parabola_point(swing_warp_phase(GO(4 + l)), st, tg, pw);
            rigid_transform(q, bp, pw, pb);
        } else {
            if (!((built >> l) & 1)) { flags |= SW_NO_TRAJ; continue; }        // the reference would read an unbuilt generator
            const float u = GO(4 + l) - 0.f;
            if ((double)u < -1e-3 || (double)u >= (double)1.f + 1e-3) { flags |= SW_PHASE; continue; }   // the reference throws (:352-354)
            const float src[3] = {ST(SS_SRC + 3 * l), ST(SS_SRC + 3 * l + 1), ST(SS_SRC + 3 * l + 2)};
            const float tgt[3] = {ST(SS_TGT + 3 * l), ST(SS_TGT + 3 * l + 1), ST(SS_TGT + 3 * l + 2)};
            float p[3], v[3];
            bspline_point(src, tgt, ST(SS_H + l), u, p, v);
            if (M.is_sim) { rigid_transform(q, bp, p, pb); rigid_transform(q, zero3, v, vb); }
            else {
#pragma unroll
                for (int r = 0; r < 3; ++r) { pb[r] = p[r]; vb[r] = v[r]; }
            }
        }
        const float sh = D.hip_l * ((l & 1) ? 1.f : -1.f);
        float ang[3], Ji[3][3];
        leg_ik(pb, &D.hip_offset[3 * l], sh, D.upper_l, D.lower_l, ang);
        leg_jacobian_inverse(ang, sh, D.upper_l, D.lower_l, Ji);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            float a = ang[r];
            if (a != a) a = g_est_in[(size_t)(17 + 3 * l + r) * N + i];        // a NaN angle keeps the current one (:415-418)
            ST(SS_QANG + 3 * l + r) = a;
            ST(SS_QVEL + 3 * l + r) = (Ji[r][0] * vb[0] + Ji[r][1] * vb[1]) + Ji[r][2] * vb[2];
            OUT(3 * l + r) = pb[r];
            OUT(12 + 3 * l + r) = vb[r];
            OUT(24 + 3 * l + r) = a;
            OUT(36 + 3 * l + r) = ST(SS_QVEL + 3 * l + r);
        }
        map |= 1 << l;
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) {                                             // the command loop (:427-459)
        bool cmd = false;
        if ((map >> l) & 1) {
            if (M.mode == 2) cmd = (int)GO(8 + l) == 8 && (int)GO(20 + l) != 2;
            else cmd = (int)GO(12 + l) == 0;
        }
        OUT(48 + l) = cmd ? 1.f : 0.f;
        if (cmd)
#pragma unroll
            for (int r = 0; r < 3; ++r) { OUT(24 + 3 * l + r) = ST(SS_QANG + 3 * l + r); OUT(36 + 3 * l + r) = ST(SS_QVEL + 3 * l + r); }
    }
    ST(SS_MAP) = (float)map;
    g_flags[i] = flags;
#undef ST
#undef OUT
#undef GO
}

}  // namespace qrgpu
