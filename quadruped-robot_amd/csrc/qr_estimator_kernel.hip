// ============================================================================
// Base velocity estimator + the leg kinematics it reads, one thread per robot (first part):
//   qrRobot::UpdateDataFlow              quadruped/src/robots/qr_robot.cpp:62-72, 187-197   (foot Jacobians, positions, velocities)
//   qrRobotVelocityEstimator::Update     quadruped/src/estimators/qr_robot_velocity_estimator.cpp:77-133
//   qrRobotPoseEstimator::Update         quadruped/src/estimators/qr_robot_pose_estimator.cpp:68-165   (stance-foot height, planar odometry)
//   qrMovingWindowFilter                 quadruped/include/quadruped/estimators/qr_moving_window_filter.hpp:150-186, 236-263
//   TinyEKF<3,3>                         quadruped/extern/TinyEKF/src/TinyEKF.h:103-124, tiny_ekf.c:17-93, 292-332
// A streaming kernel with per-robot memory: the Kalman state, the two Neumaier window sums and their ring buffers live in a
// [field][robot] array of doubles of which one tick touches 32 header fields and 6 ring slots.  Every operation of the filters is
// the reference's, in its order and type, contraction off: with equal foot kinematics the outputs are bit-identical to the CPU
// restatement (whose Kalman step is bit-identical to the reference's compiled TinyEKF); sinf / cosf of the leg kinematics differ
// from libm in the last bit, which is what the tolerance of tests/test_gpu_estimator.py covers.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_wave_helpers.h"
#include "qr_kernels.h"

namespace qrgpu {

namespace {
#pragma clang fp contract(off)
__device__ __forceinline__ void mulmat3(const double *a, const double *b, double *c)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double acc = 0;
#pragma unroll
            for (int l = 0; l < 3; ++l) acc += a[3 * i + l] * b[3 * l + j];
            c[3 * i + j] = acc;
        }
}
// Inverse of a symmetric positive-definite 3x3 (row-major) through its Cholesky factor, written out entry by entry.
// Returns 1 when a pivot is not positive.  The Kalman step is compared bit for bit with the reference's compiled filter
// (tests/test_oracle_estimator.py), whose inverse runs factor -> inverse of the factor -> product of the inverse factors; bit identity
// needs those roundings in that sequence, so every statement below is one IEEE operation (contraction off) in that dependency order,
// including the `0.0 -` / `0.0 +` starts of the accumulated sums.
__device__ __forceinline__ int spd3_inverse(const double *A, double *inv)
{
#pragma clang fp contract(off)
    // factor A = L L^T: d0..d2 the diagonal of L, l10 l20 l21 below it
    if (A[0] <= 0) return 1;
    const double d0 = sqrt(A[0]);
    const double l10 = A[1] / d0, l20 = A[2] / d0;
    const double s11 = A[4] - l10 * l10;
    if (s11 <= 0) return 1;
    const double d1 = sqrt(s11);
    const double l21 = (A[5] - l10 * l20) / d1;
    const double s22 = (A[8] - l21 * l21) - l20 * l20;
    if (s22 <= 0) return 1;
    const double d2 = sqrt(s22);
    // K = L^-1 (lower triangular), column by column
    const double k00 = 1 / d0;
    const double k10 = (0.0 - l10 * k00) / d1;
    const double k20 = ((0.0 - l20 * k00) - l21 * k10) / d2;
    const double k11 = 1 / d1;
    const double k21 = (0.0 - l21 * k11) / d2;
    const double k22 = 1 / d2;
    // A^-1 = K^T K, upper triangle then mirrored
    const double i00 = (k00 * k00 + k10 * k10) + k20 * k20;
    const double i01 = (0.0 + k10 * k11) + k20 * k21;
    const double i02 = 0.0 + k20 * k22;
    const double i11 = k11 * k11 + k21 * k21;
    const double i12 = 0.0 + k21 * k22;
    const double i22 = k22 * k22;
    inv[0] = i00; inv[1] = i01; inv[2] = i02;
    inv[3] = i01; inv[4] = i11; inv[5] = i12;
    inv[6] = i02; inv[7] = i12; inv[8] = i22;
    return 0;
}

// Neumaier update of (sum, corr) by v
template <typename T> __device__ __forceinline__ void neumaier(T &sum, T &corr, T v)
{
#pragma clang fp contract(off)
    const T ns = sum + v;
    const T as = sum < 0 ? -sum : sum, av = v < 0 ? -v : v;
    if (as >= av) corr += (sum - ns) + v;
    else corr += (v - ns) + sum;
    sum = ns;
}
}  // namespace

#define EST_LAST 0
#define EST_X 1
#define EST_P 4
#define EST_VB 13
#define EST_VSUM 16
#define EST_VCORR 19
#define EST_VCNT 22
#define EST_VHEAD 23
#define EST_ASUM 24
#define EST_ACORR 27
#define EST_ACNT 30
#define EST_AHEAD 31
#define EST_POSE 32          /* x, y, theta, absoluteHight */
#define EST_AWIN 36
#define EST_VWIN 96

// Glue between the estimators and the tick, one thread per robot: what MPCStanceLegController::SolveDenseMPC (:385-399) and
// qrWbcLocomotionController::UpdateModel (:136-156) read from qrRobot / stateDataFlow, laid out as the tick's mpc_state[28] and
// fb_state[37].  foot2ComInWorldFrame = baseRMat * (footPositionsInBaseFrame - comOffset); rpy is an input (GetBaseRollPitchYaw).
__global__ void __launch_bounds__(64) qr_pack_state_kernel(int n, float c0, float c1, float c2, const float *__restrict__ g_in, const float *__restrict__ g_est,
                                                           const float *__restrict__ g_rpy, float *__restrict__ g_mpc, float *__restrict__ g_fb)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
#define IN(f) g_in[(size_t)(f) * N + i]
#define ES(f) g_est[(size_t)(f) * N + i]
    const float e0 = IN(6), e1 = IN(7), e2 = IN(8), e3 = IN(9);
    float R[3][3];
    R[0][0] = 1 - 2 * (e2 * e2 + e3 * e3); R[0][1] = 2 * (e1 * e2 - e0 * e3); R[0][2] = 2 * (e1 * e3 + e0 * e2);
    R[1][0] = 2 * (e1 * e2 + e0 * e3); R[1][1] = 1 - 2 * (e1 * e1 + e3 * e3); R[1][2] = 2 * (e2 * e3 - e0 * e1);
    R[2][0] = 2 * (e1 * e3 - e0 * e2); R[2][1] = 2 * (e2 * e3 + e0 * e1); R[2][2] = 1 - 2 * (e1 * e1 + e2 * e2);
    if (g_mpc) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            g_mpc[(size_t)r * N + i] = ES(36 + r);                 // basePosition
            g_mpc[(size_t)(3 + r) * N + i] = ES(3 + r);            // baseVInWorldFrame
            g_mpc[(size_t)(10 + r) * N + i] = ES(9 + r);           // baseWInWorldFrame
            g_mpc[(size_t)(25 + r) * N + i] = g_rpy[(size_t)r * N + i];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) g_mpc[(size_t)(6 + r) * N + i] = IN(6 + r);
#pragma unroll
        for (int leg = 0; leg < 4; ++leg) {
            const float p0 = ES(12 + 3 * leg) - c0, p1 = ES(13 + 3 * leg) - c1, p2 = ES(14 + 3 * leg) - c2;
#pragma unroll
            for (int r = 0; r < 3; ++r) g_mpc[(size_t)(13 + 3 * leg + r) * N + i] = R[r][0] * p0 + R[r][1] * p1 + R[r][2] * p2;
        }
    }
    if (g_fb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) g_fb[(size_t)r * N + i] = IN(6 + r);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            g_fb[(size_t)(4 + r) * N + i] = ES(36 + r);
            g_fb[(size_t)(7 + r) * N + i] = IN(10 + r);            // omegaBody = GetBaseRollPitchYawRate
            g_fb[(size_t)(10 + r) * N + i] = ES(6 + r);            // GetBaseVelocityInBaseFrame
        }
#pragma unroll
        for (int r = 0; r < 12; ++r) { g_fb[(size_t)(13 + r) * N + i] = IN(17 + r); g_fb[(size_t)(25 + r) * N + i] = IN(29 + r); }
    }
#undef IN
#undef ES
}

// Swing-leg targets of the MPC/WBC mode (ADVANCED_TROT, horizontal terrain), one thread per robot:
//   qrRaibertSwingLegController::GetAction      quadruped/src/controllers/qr_swing_leg_controller.cpp:362-398, 408-424
//   qrFootParabolaPatternGenerator / qrQuadraticSpline   quadruped/src/controllers/qr_foot_trajectory_generator.cpp:187-215, quadruped/src/utils/qr_geometry.cpp:157-190
//   leg inverse kinematics                      quadruped/src/robots/qr_robot.cpp:106-124, 200-219
// Writes, for the legs flagged as swinging only: rows 15-50 of wbc_cmd (pFoot_des, vFoot_des, aFoot_des), the foot target in the
// world frame (an input of the MPC front-end) and the joint angle / velocity targets of the swing-leg position command.
__global__ void __launch_bounds__(64) qr_swing_kernel(int n, qrgpu_estimator_desc D, const float *__restrict__ g_in, float *__restrict__ g_cmd, float *__restrict__ g_tgt_world,
                                                      float *__restrict__ g_qdes)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
#define IN(f) g_in[(size_t)(f) * N + i]
    const float e0 = IN(39), e1 = IN(40), e2 = IN(41), e3 = IN(42);
    float R[3][3];                                                        // body -> world
    R[0][0] = 1 - 2 * (e2 * e2 + e3 * e3); R[0][1] = 2 * (e1 * e2 - e0 * e3); R[0][2] = 2 * (e1 * e3 + e0 * e2);
    R[1][0] = 2 * (e1 * e2 + e0 * e3); R[1][1] = 1 - 2 * (e1 * e1 + e3 * e3); R[1][2] = 2 * (e2 * e3 - e0 * e1);
    R[2][0] = 2 * (e1 * e3 - e0 * e2); R[2][1] = 2 * (e2 * e3 + e0 * e1); R[2][2] = 1 - 2 * (e1 * e1 + e2 * e2);
    const float bp[3] = {IN(36), IN(37), IN(38)}, bv[3] = {IN(43), IN(44), IN(45)};
#pragma unroll
    for (int leg = 0; leg < 4; ++leg) {
        if (IN(leg) == 0.f) continue;
        const float phase = IN(4 + leg), swingDur = IN(8 + leg);
        const float st[3] = {IN(12 + 3 * leg), IN(13 + 3 * leg), IN(14 + 3 * leg)}, tg[3] = {IN(24 + 3 * leg), IN(25 + 3 * leg), IN(26 + 3 * leg)};
        if (g_tgt_world) {
#pragma unroll
            for (int r = 0; r < 3; ++r) g_tgt_world[(size_t)(3 * leg + r) * N + i] = (R[r][0] * tg[0] + R[r][1] * tg[1] + R[r][2] * tg[2]) + bp[r];
        }
        float pw[3] = {0.f, 0.f, 0.f};
        swing_parabola_point(phase, st, tg, pw);
        float vb[3] = {0.f, 0.f, 0.f};
        if ((double)phase < 1.0) {
#pragma unroll
            for (int r = 0; r < 3; ++r) vb[r] = 0.f / swingDur;
        }
        if (g_cmd) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                g_cmd[(size_t)(15 + 3 * leg + r) * N + i] = (R[r][0] * pw[0] + R[r][1] * pw[1] + R[r][2] * pw[2]) + bp[r];
                g_cmd[(size_t)(27 + 3 * leg + r) * N + i] = bv[r] + vb[r];
                g_cmd[(size_t)(39 + 3 * leg + r) * N + i] = 0.f;
            }
        }
        if (g_qdes) {
            const float sh = D.hip_l * ((leg & 1) ? 1.f : -1.f);
            float ang[3], Ji[3][3];
            leg_ik(pw, &D.hip_offset[3 * leg], sh, D.upper_l, D.lower_l, ang);
            leg_jacobian_inverse(ang, sh, D.upper_l, D.lower_l, Ji);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float a = ang[r];
                if (a != a) a = IN(46 + 3 * leg + r);                     // unreachable target: keep the current angle (:415-418)
                g_qdes[(size_t)(3 * leg + r) * N + i] = a;
                g_qdes[(size_t)(12 + 3 * leg + r) * N + i] = Ji[r][0] * vb[0] + Ji[r][1] * vb[1] + Ji[r][2] * vb[2];
            }
        }
    }
#undef IN
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Which legs swing + where they should land: qrRaibertSwingLegController::Update (default branch, QS/controllers/
// qr_swing_leg_controller.cpp:211-236) and qrFootholdPlanner::ComputeHeuristicFootHold (QS/planner/qr_foothold_planner.cpp:110-239) on
// flat ground (dR = baseRMat).  One thread per robot; same operation order as oracle/qr_oracle_swing.cpp (footholds), contraction off.
// g_in [46][n] (include/qrgpu.h fh_in); rows 0-15 come from the gait kernel's arrays instead when those are given (legState and
// allowSwitchLegState are rows 16-23 of gait_state, normalizedPhase / swingTimeRemaining rows 4-7 / 20-23 of gait_out).
// Writes rows 0-3 of swing_in for every leg, rows 4-7 and 24-35 for the swinging ones.
__global__ void __launch_bounds__(64) qr_foothold_kernel(int n, qrgpu_foothold_desc D, const float *__restrict__ g_in, const float *__restrict__ g_gait_state,
                                                         const float *__restrict__ g_gait_out, float *__restrict__ g_swing)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
#define FI(f) g_in[(size_t)(f) * N + i]
    const float e0 = FI(33), e1 = FI(34), e2 = FI(35), e3 = FI(36);
    float R[3][3];                                                        // baseRMat: body -> world (= dR on flat ground)
    R[0][0] = 1 - 2 * (e2 * e2 + e3 * e3); R[0][1] = 2 * (e1 * e2 - e0 * e3); R[0][2] = 2 * (e1 * e3 + e0 * e2);
    R[1][0] = 2 * (e1 * e2 + e0 * e3); R[1][1] = 1 - 2 * (e1 * e1 + e3 * e3); R[1][2] = 2 * (e2 * e3 - e0 * e1);
    R[2][0] = 2 * (e1 * e3 - e0 * e2); R[2][1] = 2 * (e2 * e3 + e0 * e1); R[2][2] = 1 - 2 * (e1 * e1 + e2 * e2);
    const float vdes[3] = {FI(16), FI(17), FI(18)}, wdes = FI(19), hdes = FI(20);
    const float roll = FI(37);
    const float vb[3] = {FI(40), FI(41), FI(42)}, w[3] = {FI(43), FI(44), FI(45)};
    const float dh2 = hdes - D.foot_clearance;
    const float c = cosf(roll), sn = sinf(roll);
#pragma unroll
    for (int leg = 0; leg < 4; ++leg) {
        const int st = (int)(g_gait_state ? g_gait_state[(size_t)(16 + leg) * N + i] : FI(leg));
        const float allow = g_gait_state ? g_gait_state[(size_t)(20 + leg) * N + i] : FI(4 + leg);
        const bool skip = (st == 1 && allow != 0.f) || st == 2;
        g_swing[(size_t)leg * N + i] = skip ? 0.f : 1.f;
        if (skip) continue;
        const float side = (leg & 1) ? 1.f : -1.f;
        const float ho[3] = {D.hip_offset[3 * leg], D.hip_offset[3 * leg + 1], D.hip_offset[3 * leg + 2]};
        const float twist[3] = {-ho[1], ho[0], 0.f};
        const float cr[3] = {w[1] * ho[2] - w[2] * ho[1], w[2] * ho[0] - w[0] * ho[2], w[0] * ho[1] - w[1] * ho[0]};
        const float hv0[3] = {vb[0] + cr[0], vb[1] + cr[1], vb[2] + cr[2]};
        float hv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) hv[r] = (R[r][0] * hv0[0] + R[r][1] * hv0[1]) + R[r][2] * hv0[2];
        hv[2] = 0.f;
        const float tv[3] = {vdes[0] + wdes * twist[0], vdes[1] + wdes * twist[1], vdes[2] + wdes * twist[2]};
        float ftp[3], phase;
        if (allow == 0.f) {
            const float hp[3] = {D.default_hip_position[3 * leg], D.default_hip_position[3 * leg + 1], D.default_hip_position[3 * leg + 2]};
            const float d[3] = {FI(21 + 3 * leg) - hp[0], FI(22 + 3 * leg) - hp[1], FI(23 + 3 * leg) - hp[2]};
            float t[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) t[r] = (R[r][0] * d[0] + R[r][1] * d[1]) + R[r][2] * d[2];
            if ((double)t[1] > 0.01 + 0.00 * (double)(-side)) t[1] = (float)((double)t[1] - 0.005);
            else if ((double)t[1] < -0.01 + 0.00 * (double)side) t[1] = (float)((double)t[1] + 0.005);
            t[2] = (float)((double)t[2] - 0.02);
#pragma unroll
            for (int r = 0; r < 3; ++r) ftp[r] = ((R[0][r] * t[0] + R[1][r] * t[1]) + R[2][r] * t[2]) + hp[r];
            phase = 1.0f;
        } else {
            const float s = g_gait_out ? g_gait_out[(size_t)(20 + leg) * N + i] : FI(8 + leg);
            float u[3], dP[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) u[r] = tv[r] * s - D.swing_kp[r] * (tv[r] - hv[r]);
#pragma unroll
            for (int r = 0; r < 3; ++r) dP[r] = (R[0][r] * u[0] + R[1][r] * u[1]) + R[2][r] * u[2];
            const float th = 0.2f;
            dP[0] = dP[0] < -th ? -th : (dP[0] > th ? th : dP[0]);
            dP[1] = dP[1] < -th ? -th : (dP[1] > th ? th : dP[1]);
            dP[2] = 0.f;
            const float iy = D.hip_l * side;
            const float rr[3] = {(0.f * 1.f + 0.f * iy) + 0.f * 0.f, (0.f * 0.f + c * iy) + sn * 0.f, (0.f * 0.f + -sn * iy) + c * 0.f};
            const float a[3] = {ho[0], ho[1], 0.f};
#pragma unroll
            for (int r = 0; r < 3; ++r) ftp[r] = (dP[r] + a[r]) + rr[r];
#pragma unroll
            for (int r = 0; r < 3; ++r) ftp[r] -= (R[0][r] * 0.f + R[1][r] * 0.f) + R[2][r] * dh2;
            phase = g_gait_out ? g_gait_out[(size_t)(4 + leg) * N + i] : FI(12 + leg);
        }
        g_swing[(size_t)(4 + leg) * N + i] = phase;
#pragma unroll
        for (int r = 0; r < 3; ++r) g_swing[(size_t)(24 + 3 * leg + r) * N + i] = ftp[r];
    }
#undef FI
}

// Swing-leg action of the velocity mode (the trot of the force-balance path), one thread per robot:
//   qrRaibertSwingLegController::GetAction, VELOCITY_LOCOMOTION case    quadruped/src/controllers/qr_swing_leg_controller.cpp:285-309, 408-424
//   SwingFootTrajectory::GenerateTrajectoryPoint(phaseModule = true)   quadruped/src/controllers/qr_foot_trajectory_generator.cpp:322-343
// g_in [53][n]: swing flag[4], normalizedPhase[4], phaseSwitchFootLocalPos[12], estimated base velocity (base frame)[3], yaw rate,
// desiredSpeed[3], desiredTwistingSpeed, dR[9] (baseRInControlFrame, row-major: rows 22-30 of the ground kernel's output), quat_wxyz[4],
// motor angles[12].  g_out [48][n], for the flagged legs: footTargetPosition[12] (base frame), footPositionInBaseFrame[12], joint angle
// targets[12], joint velocity targets[12].
__global__ void __launch_bounds__(64) qr_swing_velocity_kernel(int n, qrgpu_estimator_desc D, qrgpu_swing_velocity_desc V, const float *__restrict__ g_in, float *__restrict__ g_out)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
#define IN(f) g_in[(size_t)(f) * N + i]
    const float e0 = IN(37), e1 = IN(38), e2 = IN(39), e3 = IN(40);
    float Rwb[3][3];                                                      // world -> body = baseRMat^T
    Rwb[0][0] = 1 - 2 * (e2 * e2 + e3 * e3); Rwb[1][0] = 2 * (e1 * e2 - e0 * e3); Rwb[2][0] = 2 * (e1 * e3 + e0 * e2);
    Rwb[0][1] = 2 * (e1 * e2 + e0 * e3); Rwb[1][1] = 1 - 2 * (e1 * e1 + e3 * e3); Rwb[2][1] = 2 * (e2 * e3 - e0 * e1);
    Rwb[0][2] = 2 * (e1 * e3 - e0 * e2); Rwb[1][2] = 2 * (e2 * e3 + e0 * e1); Rwb[2][2] = 1 - 2 * (e1 * e1 + e2 * e2);
    float dR[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) dR[k] = IN(28 + k);
    const float bvel[3] = {IN(20), IN(21), IN(22)}, yawDot = IN(23), sp[3] = {IN(24), IN(25), IN(26)}, twist = IN(27);
#pragma unroll
    for (int leg = 0; leg < 4; ++leg) {
        if (IN(leg) == 0.f) continue;
        const float ho[3] = {V.hip_position_com[3 * leg], V.hip_position_com[3 * leg + 1], V.hip_position_com[3 * leg + 2]};
        const float tw[3] = {-ho[1], ho[0], 0.f};
        float hv[3], hh[3], tgtv[3], u[3], tg[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) hv[r] = bvel[r] + yawDot * tw[r];
#pragma unroll
        for (int r = 0; r < 3; ++r) hh[r] = (dR[3 * r] * hv[0] + dR[3 * r + 1] * hv[1]) + dR[3 * r + 2] * hv[2];
        hh[2] = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) tgtv[r] = sp[r] + twist * tw[r];
#pragma unroll
        for (int r = 0; r < 3; ++r) u[r] = hh[r] * V.stance_duration[leg] / 2.0f - V.swing_kp[r] * (tgtv[r] - hh[r]);
        const float dh[3] = {0.f, 0.f, V.desired_height};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float a = (dR[r] * u[0] + dR[3 + r] * u[1]) + dR[6 + r] * u[2];
            const float b = (Rwb[r][0] * dh[0] + Rwb[r][1] * dh[1]) + Rwb[r][2] * dh[2];
            const float off = (r < 2) ? ho[r] : 0.f;
            tg[r] = (a + off) - b;
        }
        const float st[3] = {IN(8 + 3 * leg), IN(9 + 3 * leg), IN(10 + 3 * leg)};
        const float inputPhase = IN(4 + leg);
        const float phase = swing_warp_phase(inputPhase);
        float pw[3] = {0.f, 0.f, 0.f};
        swing_parabola_point(phase, st, tg, pw);
#pragma unroll
        for (int r = 0; r < 3; ++r) { g_out[(size_t)(3 * leg + r) * N + i] = tg[r]; g_out[(size_t)(12 + 3 * leg + r) * N + i] = pw[r]; }
        const float sh = D.hip_l * ((leg & 1) ? 1.f : -1.f);
        float ang[3], Ji[3][3];
        leg_ik(pw, &D.hip_offset[3 * leg], sh, D.upper_l, D.lower_l, ang);
        // J^-1 * (the generator's zero velocity): zero, or NaN where the Jacobian is (an unreachable target), as the reference's product is
        leg_jacobian_inverse(ang, sh, D.upper_l, D.lower_l, Ji);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            float a = ang[r];
            if (a != a) a = IN(41 + 3 * leg + r);                         // unreachable target: keep the current angle (:415-418)
            g_out[(size_t)(24 + 3 * leg + r) * N + i] = a;
            g_out[(size_t)(36 + 3 * leg + r) * N + i] = Ji[r][0] * 0.f + Ji[r][1] * 0.f + Ji[r][2] * 0.f;
        }
    }
#undef IN
}

// The stage kernels with memory, compiled twice: as they always were, and in their per-robot form (suffix _pr, qrgpu_set_stage_reset).
#define QR_STAGE_PR 0
#include "qr_estimator_stages.inc.h"
#undef QR_STAGE_PR
#define QR_STAGE_PR 1
#include "qr_estimator_stages.inc.h"
#undef QR_STAGE_PR

}  // namespace qrgpu
