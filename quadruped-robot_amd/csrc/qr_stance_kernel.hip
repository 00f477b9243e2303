// ============================================================================
// Stance front-end and motor commands of the force-balance modes (VELOCITY, POSITION, WALK, ADVANCED_TROT without MPC), one thread per robot:
//   TorqueStanceLegController::UpdateFRatio / UpdateDesCommand   quadruped/src/controllers/balance_controller/qr_torque_stance_leg_controller.cpp:89-172, 174-477
//   TorqueStanceLegController::GetAction (motor-command tail)    :503-541
//   qrLocomotionController::GetAction (swing / stance merge)     quadruped/src/controllers/qr_locomotion_controller.cpp:128-147
//   qrComAdjuster::Update (POSITION)                             quadruped/src/planner/qr_com_adjuster.cpp:61-108, include/quadruped/planner/qr_com_adjuster.h:55-59
//   qrPosePlanner::GetIntermediateBasePose + qrSegment::GetPoint include/quadruped/planner/qr_pose_planner.h:327-365, utils/qr_geometry.h:73-81
//   ComputeContactForce's Rcb / g / surfaceNormal                quadruped/src/controllers/balance_controller/qr_qp_torque_optimizer.cpp:202-221, 319-336
// Every array is [field][robot]; no LDS, no scratch.  Every operation is the reference's, in its order and float / double mix (double
// literals promote, assignment narrows), contraction off; the unqualified abs on floats (:355, :386) is std::abs(float).
// Branches of the reference that cannot be reached, and are therefore not built:
//   - VELOCITY sets computeForceInWorldFrame = false at :235 before :262 and :337 read it: the world-frame forms of :337-342 never run and
//     :262 always does;
//   - the rotation-error branch :456-468 needs computeForceInWorldFrame in a mode other than ADVANCED_TROT: only WALK reaches it;
//   - com2FootInWorld (:216) is never used;
//   - WALK's legJointq (:403-420) enters the command as 0.0 * legJointq (:519): the command's position is written as 0 and the leg
//     inverse kinematics behind it is not computed.
// The walk branch of UpdateFRatio is qr_walk_gait_kernel's; here only N, moveBasePhase (:145) and the robot->stop override (:95-102) are
// taken from its output.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_wave_helpers.h"
#include "qr_kernels.h"

namespace qrgpu {

namespace {

// one vertex of qrComAdjuster::Update's support polygon (:82-103)
__device__ __forceinline__ void com_vertex(const float p[3], const float pCw[3], const float pCcw[3], float phi, float phiCw, float phiCcw, float out[3])
{
#pragma clang fp contract(off)
    const float rest = 1 - phi;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float vCw = p[r] * phi + pCw[r] * rest;
        const float vCcw = p[r] * phi + pCcw[r] * rest;
        out[r] = ((phi * p[r] + phiCcw * vCcw) + phiCw * vCw) / ((phi + phiCcw) + phiCw);
    }
}

}  // namespace

// UpdateFRatio + UpdateDesCommand.  g_st [1][n]: heightInControlFrame as the pose estimator keeps it (est_out row 39 is NaN while no foot
// is in stance).  g_cmd [28][n]: stateDes(2), stateDes 6..8, stateDes 9..11, the pose planner's source[6], dest[6], twist[6],
// GetDesiredComPose().tail(3).  Outputs (each may be null): g_vmc_in [37][n] complete, g_ratio [8][n], g_out [33][n] = stateCur[12],
// stateDes[12], ddqDes[6], N, moveBasePhase, computeForceInWorldFrame.
__global__ void __launch_bounds__(64) qr_stance_update_kernel(int n, qrgpu_stance_desc S, float current_time, int stop, int reset, const float *__restrict__ g_est_in,
                                                              const float *__restrict__ g_est_out, const float *__restrict__ g_ground,
                                                              const float *__restrict__ g_rpy, const float *__restrict__ g_gait_out,
                                                              const float *__restrict__ g_gait_state, const float *__restrict__ g_cmd, float *__restrict__ g_st,
                                                              float *__restrict__ g_vmc_in, float *__restrict__ g_ratio, float *__restrict__ g_out, StageResetArgs SR)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
    // the lane's own reset level and clock: the call's scalar reset wins, then the bound level of a masked robot
    if (!reset && stage_masked(SR, i)) reset = SR.level;
    current_time = stage_time(SR, i, current_time);
#define EI(f) g_est_in[(size_t)(f) * N + i]
#define EO(f) g_est_out[(size_t)(f) * N + i]
#define GR(f) g_ground[(size_t)(f) * N + i]
#define GO(f) g_gait_out[(size_t)(f) * N + i]
#define CM(f) g_cmd[(size_t)(f) * N + i]
    // ---- UpdateFRatio (:89-172)
    float cont[4], fmn[4], fmx[4];
    int Nc = 0;
    float mbp = 1.f;
    if (stop) {
#pragma unroll
        for (int l = 0; l < 4; ++l) { cont[l] = 1.f; fmn[l] = 0.01f; fmx[l] = 10.f; }
        Nc = 4;
    } else if (S.mode != 2) {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const int desired = (int)GO(8 + l);
            bool flag;
            if (S.mode == 0) flag = desired == 1;
            else flag = (desired == 1 && g_gait_state[(size_t)(20 + l) * N + i] != 0.f) || (int)GO(12 + l) == 2;
            cont[l] = flag ? 1.f : 0.f; fmn[l] = 0.01f; fmx[l] = 10.f;
            if (flag) ++Nc;
        }
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            cont[l] = GO(29 + l); fmn[l] = GO(33 + l); fmx[l] = GO(37 + l);
            if (cont[l] != 0.f) ++Nc;
            if ((int)GO(20 + l) == 0) mbp = GO(28);                          // a leg planned to swing: the generator's moveBasePhase (:145)
        }
    }
    // ---- the pose estimator's height memory (qr_robot_pose_estimator.cpp:50, :139-147)
    float hmem = reset ? S.body_height : g_st[i];
    { const float h = EO(39); if (h == h) hmem = h; }
    g_st[i] = hmem;
    // ---- UpdateDesCommand (:174-477)
    const float q[4] = {EI(6), EI(7), EI(8), EI(9)};
    const float bp[3] = {EO(36), EO(37), EO(38)};
    const float gr[3] = {GR(6), GR(7), GR(8)};
    const float cq[4] = {GR(9), GR(10), GR(11), GR(12)};
    const float zero3[3] = {0.f, 0.f, 0.f};
    float Rc[3][3], Rb[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Rc[r][c] = GR(13 + 3 * r + c);
    base_rmat(q, Rb);
    float cp[3] = {0.f, 0.f, bp[2]};                                          // robotComPosition
    float cr[3] = {g_rpy[i], g_rpy[N + i], g_rpy[2 * N + i]};                 // robotComRpy
    float cv[3] = {EO(6), EO(7), EO(8)};                                      // robotComVelocity
    float cw[3] = {EI(10), EI(11), EI(12)};                                   // robotComRpyRate
    float dp[3] = {0.f, 0.f, 0.f}, dr[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f}, dw[3] = {0.f, 0.f, 0.f};
    const bool sloped = S.terrain >= 2;
    const bool world = S.mode == 2 || (S.mode == 3 && S.force_in_world);
    // into the control frame: first into the world, then RigidTransform by the control frame's orientation
    auto to_control = [&](float v[3]) {
        float t[3];
        invert_rigid_transform(q, zero3, v, t);
        rigid_transform(cq, zero3, t, v);
    };
    auto to_world = [&](float v[3]) {
        float t[3];
        invert_rigid_transform(q, zero3, v, t);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2];
    };
    auto control_rpy = [&](float out[3]) {                                    // rotationMatrixToRPY(Rcb^T): r = Rcb
        float Rcb[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Rcb[r][c] = GR(22 + 3 * r + c);
        rotmat_t_to_rpy(Rcb, out);
    };
    if (S.mode == 0) {                                                        // VELOCITY (:233-268, :323-343)
        if (sloped) {
            float qi[4], t[3];
            quat_inverse(cq, qi);
            transform_vec_by_quat(qi, cp, t);
            cp[0] = 0.0f; cp[1] = 0.0f; cp[2] = t[2];
            to_control(cv);
            control_rpy(cr);
            to_control(cw);
        } else {
            float t[3];
            invert_rigid_transform(q, zero3, cv, t);
            float u[3];
            invert_rigid_transform(q, zero3, cw, u);
            cr[2] = 0.0f;
            rigid_transform(cq, zero3, t, cv);
            rigid_transform(cq, zero3, u, cw);
        }
        dp[2] = S.desired_height;
        dr[0] = -gr[0]; dr[2] = -gr[2];
        dv[0] = CM(1); dv[1] = CM(2); dv[2] = CM(3);
        dw[0] = CM(4); dw[1] = CM(5); dw[2] = CM(6);
    } else if (S.mode == 3) {                                                 // ADVANCED_TROT (:270-295, :345-400)
        if (world) {
            to_world(cv);
            to_world(cw);
            // comAdjuster->Update is not called in this mode (qr_locomotion_controller.cpp:118-121): comPosInBaseFrame is Reset's zero
            dp[0] = dot3(Rb[0], 0.f, 0.f, 0.f) + bp[0];
            dp[1] = dot3(Rb[1], 0.f, 0.f, 0.f) + bp[1];
            dp[2] = CM(0);
            float pitch = gr[1];
            const float pitchMax = 0.5f;
            if (fabsf(pitch) < 0.1f) pitch = 0;
            else if (pitch > pitchMax) pitch = pitchMax;
            else if (pitch < -pitchMax) pitch = -pitchMax;
            dr[1] = pitch;
            float scaleFactor = 1;
            const float fx0 = EO(12), fx1 = EO(15);
            const float footX = (fx1 < fx0) ? fx1 : fx0;
            if (footX < 0.1f) { const float t = footX / 0.1f; scaleFactor = (0.1f < t) ? t : 0.1f; }
            dv[0] = scaleFactor * CM(1); dv[1] = scaleFactor * CM(2); dv[2] = scaleFactor * CM(3);
            if (pitch < 0.1f && dv[2] > 0.01f) dp[2] += 0.04f * fabsf(pitch / pitchMax);
            dw[0] = CM(4); dw[1] = CM(5); dw[2] = CM(6);
        } else {
            cr[2] = 0.f;
            if (sloped) {
                cp[2] = hmem;
                to_control(cv);
                control_rpy(cr);
                to_control(cw);
            }
            dp[2] = S.desired_height * fabsf(cosf(gr[1]));
            dp[2] = (float)((double)cp[2] * 0.7 + (double)dp[2] * 0.3);
            dr[0] = -gr[0]; dr[2] = -gr[2];
            dv[0] = dot3(Rc[0], S.desired_speed[0], S.desired_speed[1], 0.f);
            dv[1] = dot3(Rc[1], S.desired_speed[0], S.desired_speed[1], 0.f);
            dv[2] = dot3(Rc[2], S.desired_speed[0], S.desired_speed[1], 0.f);
            dw[2] = S.desired_twisting_speed;
        }
    } else if (S.mode == 2) {                                                 // WALK (:197-208, :297-302, :402-433)
        float phase;
        if (!stop) {
            phase = (float)((double)mbp * 1.0);
            if ((double)phase > 1.0) phase = 1.0;
        } else {
            const float dt = current_time - S.pose_reset_time;
            phase = dt / 5.0f;
            if ((double)phase > 1.0) phase = 1.0;
        }
        if ((double)phase > 1.0) phase = 1.0;                                 // qrSegment::GetPoint
        else if ((double)phase < 0.0) phase = 0.0;
        const float rest = (float)(1.0 - (double)phase);
        float pose[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) pose[k] = phase * CM(13 + k) + rest * CM(7 + k);
        cp[0] = bp[0]; cp[1] = bp[1];
        to_world(cv);
        to_world(cw);
        dp[0] = pose[0]; dp[1] = pose[1]; dp[2] = pose[2];
        dr[0] = pose[3]; dr[1] = pose[4]; dr[2] = pose[5];
        { const float mn = (0.35f < dr[1]) ? 0.35f : dr[1]; dr[1] = (-0.35f < mn) ? mn : -0.35f; }
        dv[0] = CM(19); dv[1] = CM(20); dv[2] = CM(21);
        dw[0] = CM(22); dw[1] = CM(23); dw[2] = CM(24);
    } else {                                                                  // POSITION (:304-311, :435-447)
        float w[4];
        const double den = (double)1.0f * sqrt(2.0);                          // delta * sqrt(2)
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const int ls = (int)GO(12 + l);
            const float ph = GO(4 + l);
            float contactK, swingK;
            if (ls == 1 || ls == 3) {
                contactK = (float)(0.5 * (erf((double)ph / den) + erf((1.0 - (double)ph) / den)));
                swingK = 0.f;
            } else {
                swingK = (float)(0.5 * ((2.0 + erf((double)(-ph) / den)) + erf(((double)ph - 1.0) / den)));
                contactK = 0.f;
            }
            w[l] = contactK + swingK;
        }
        const float p0[3] = {EO(12), EO(13), EO(14)}, p1[3] = {EO(15), EO(16), EO(17)}, p2[3] = {EO(18), EO(19), EO(20)}, p3[3] = {EO(21), EO(22), EO(23)};
        float v0[3], v1[3], v2[3], v3[3];                                     // ADJEST_LEG: leg 0 (cw 2, ccw 1), 1 (0, 3), 2 (3, 0), 3 (1, 2)
        com_vertex(p0, p2, p1, w[0], w[2], w[1], v0);
        com_vertex(p1, p0, p3, w[1], w[0], w[3], v1);
        com_vertex(p2, p3, p0, w[2], w[3], w[0], v2);
        com_vertex(p3, p1, p2, w[3], w[1], w[2], v3);
        dp[0] = ((v0[0] + v1[0]) + (v2[0] + v3[0])) / 4.f;                    // rowwise().mean()
        dp[1] = ((v0[1] + v1[1]) + (v2[1] + v3[1])) / 4.f;
        dp[2] = S.desired_height;
        dv[0] = S.desired_speed[0]; dv[1] = S.desired_speed[1];
        dr[0] = CM(25); dr[1] = CM(26); dr[2] = CM(27);
    }
    float dq[6], ddq[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { dq[k] = dp[k] - cp[k]; dq[3 + k] = dr[k] - cr[k]; ddq[k] = dv[k] - cv[k]; ddq[3 + k] = dw[k] - cw[k]; }
    if (S.mode == 2) {                                                        // R (dR^T -> rpy) and R ((W_des)^ - (W_cur)^)v (:456-468)
        float A[3][3], B[3][3], dRt[3][3], e[3];
        rpy_to_rotmat(cr, A);                                                 // robotR = A^T
        rpy_to_rotmat(dr, B);                                                 // desiredRobotRT
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) dRt[c][r] = (B[r][0] * A[c][0] + B[r][1] * A[c][1]) + B[r][2] * A[c][2];   // dR = B robotR, stored transposed
        rotmat_t_to_rpy(dRt, e);
        const float a[3] = {dot3(B[0], dw[0], dw[1], dw[2]), dot3(B[1], dw[0], dw[1], dw[2]), dot3(B[2], dw[0], dw[1], dw[2])};
        const float b[3] = {dot3(A[0], cw[0], cw[1], cw[2]), dot3(A[1], cw[0], cw[1], cw[2]), dot3(A[2], cw[0], cw[1], cw[2])};
        // matToSkewVec(vectorToSkewMat(a) - vectorToSkewMat(b))
        const float s[3] = {0.5f * ((a[0] - b[0]) - (-a[0] - -b[0])), 0.5f * ((a[1] - b[1]) - (-a[1] - -b[1])), 0.5f * ((a[2] - b[2]) - (-a[2] - -b[2]))};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            dq[3 + r] = (A[0][r] * e[0] + A[1][r] * e[1]) + A[2][r] * e[2];
            ddq[3 + r] = (A[0][r] * s[0] + A[1][r] * s[1]) + A[2][r] * s[2];
        }
    }
    float acc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float a = S.kp[k] * dq[k] + S.kd[k] * ddq[k];
        a = (S.max_ddq[k] < a) ? S.max_ddq[k] : a;                            // cwiseMin(maxDdq).cwiseMax(minDdq)
        a = (a < S.min_ddq[k]) ? S.min_ddq[k] : a;
        acc[k] = a;
    }
    if (g_out) {
#define OUT(f) g_out[(size_t)(f) * N + i]
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            OUT(k) = cp[k]; OUT(3 + k) = cr[k]; OUT(6 + k) = cv[k]; OUT(9 + k) = cw[k];
            OUT(12 + k) = dp[k]; OUT(15 + k) = dr[k]; OUT(18 + k) = dv[k]; OUT(21 + k) = dw[k];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) OUT(24 + k) = acc[k];
        OUT(30) = (float)Nc; OUT(31) = mbp; OUT(32) = world ? 1.f : 0.f;
#undef OUT
    }
    if (g_ratio) {
#pragma unroll
        for (int l = 0; l < 4; ++l) { g_ratio[(size_t)l * N + i] = fmn[l]; g_ratio[(size_t)(4 + l) * N + i] = fmx[l]; }
    }
    if (g_vmc_in) {
#define VI(f) g_vmc_in[(size_t)(f) * N + i]
#pragma unroll
        for (int k = 0; k < 12; ++k) VI(k) = EO(12 + k);
#pragma unroll
        for (int k = 0; k < 6; ++k) VI(12 + k) = acc[k];
#pragma unroll
        for (int l = 0; l < 4; ++l) VI(18 + l) = cont[l];
        const float g9 = (float)9.8;
        if (world) {                                                          // rotMat, g, GetAction's direction vectors (qr_qp_torque_optimizer.cpp:319-336)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) VI(22 + 3 * r + c) = Rb[r][c];
            VI(31) = 0.f; VI(32) = 0.f; VI(33) = g9;
            VI(34) = 0.f; VI(35) = 0.f; VI(36) = 1.f;
        } else if (!sloped) {                                                 // PLANE / PLUM_PILES (:215-216)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) VI(22 + 3 * r + c) = r == c ? 1.f : 0.f;
            VI(31) = 0.f; VI(32) = 0.f; VI(33) = g9;
            VI(34) = 0.f; VI(35) = 0.f; VI(36) = 1.f;
        } else {                                                              // Rcb = Rc^T baseRMat, g = Rc^T g, the pitched normal (:218-220)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) VI(22 + 3 * r + c) = (Rc[0][r] * Rb[0][c] + Rc[1][r] * Rb[1][c]) + Rc[2][r] * Rb[2][c];
                VI(31 + r) = (Rc[0][r] * 0.f + Rc[1][r] * 0.f) + Rc[2][r] * g9;
            }
            VI(34) = -sinf(gr[1]); VI(35) = 0.f; VI(36) = cosf(gr[1]);
        }
#undef VI
    }
#undef EI
#undef EO
#undef GR
#undef GO
#undef CM
}

// The motor-command tail of TorqueStanceLegController::GetAction (:503-541) and the merge of qrLocomotionController::GetAction
// (qr_locomotion_controller.cpp:128-147).  g_cmd [60][n]: p[12], Kp[12], d[12], Kd[12], tua[12].  WALK reads contacts (rows 18-21 of
// g_vmc_in), N and moveBasePhase (rows 30, 31 of g_stance_out).  g_swing_q [24][n] joint angle and velocity targets and g_swing_flag [4][n]
// (both may be null): a flagged leg's motors become {q, kp, qd, kd, 0} (qr_swing_leg_controller.cpp:456-458).
__global__ void __launch_bounds__(64) qr_stance_command_kernel(int n, qrgpu_stance_desc S, int stop, const float *__restrict__ g_vmc_in,
                                                               const float *__restrict__ g_stance_out, const float *__restrict__ g_tau,
                                                               const float *__restrict__ g_swing_q, const float *__restrict__ g_swing_flag,
                                                               float *__restrict__ g_cmd)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
    int Nc = 0;
    float mbp = 0.f;
    if (S.mode == 2) { Nc = (int)g_stance_out[(size_t)30 * N + i]; mbp = g_stance_out[(size_t)31 * N + i]; }
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const bool swing = g_swing_q && g_swing_flag && g_swing_flag[(size_t)l * N + i] != 0.f;
        int kind = 0;                                                         // 0: {0, 0, 0, 0, tau}
        if (S.mode == 2) {
            if (g_vmc_in[(size_t)(18 + l) * N + i] != 0.f) kind = 1;
            else if ((Nc < 4 && (double)mbp < 0.7) || stop) kind = 2;
            else kind = 3;
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const int j = 3 * l + m;
            float p = 0.f, kp = 0.f, d = 0.f, kd = 0.f, tau = g_tau[(size_t)j * N + i];
            if (kind == 1) { kp = (float)(0.0 * (double)S.motor_kp[j]); d = (float)0.0; kd = (float)(0.5 * (double)S.motor_kd[j]); }   // p = 0.0 * legJointq
            else if (kind == 2) kd = (float)((double)S.motor_kd[j] * 0.0);
            else if (kind == 3) tau = 0.f;
            if (swing) { p = g_swing_q[(size_t)j * N + i]; kp = S.motor_kp[j]; d = g_swing_q[(size_t)(12 + j) * N + i]; kd = S.motor_kd[j]; tau = 0.f; }
            g_cmd[(size_t)j * N + i] = p; g_cmd[(size_t)(12 + j) * N + i] = kp; g_cmd[(size_t)(24 + j) * N + i] = d;
            g_cmd[(size_t)(36 + j) * N + i] = kd; g_cmd[(size_t)(48 + j) * N + i] = tau;
        }
    }
}

}  // namespace qrgpu
