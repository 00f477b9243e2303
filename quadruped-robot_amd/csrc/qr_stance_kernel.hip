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

// The stage kernels with memory, compiled twice: as they always were, and in their per-robot form (suffix _pr, qrgpu_set_stage_reset).
#define QR_STAGE_PR 0
#include "qr_stance_update.inc.h"
#undef QR_STAGE_PR
#define QR_STAGE_PR 1
#include "qr_stance_update.inc.h"
#undef QR_STAGE_PR

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
