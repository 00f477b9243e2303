// The data-flow stage of the velocity mode (the force-balance trot: LocomotionMode::VELOCITY_LOCOMOTION, TorqueStanceLegController and the VELOCITY case
// of the swing controller), per robot: what qr_velocity_flow_kernel (qr_velocity_flow_kernel.hip) runs per lane.  Copies, compares and integer bit
// operations in float32, nothing else.  The function is __host__ __device__: the same text compiles for a CPU check against tests/velocity_flow_ref.py
// (tests/stubs/velocity_flow_host.hip).  include/qrgpu.h states the rules.
//   qrRaibertSwingLegController::Reset        quadruped/src/controllers/qr_swing_leg_controller.cpp:100 (the map is cleared)
//   qrRaibertSwingLegController::Update       :218-229, the default branch: swingFootIds
//   qrRaibertSwingLegController::GetAction    :256-258 (motor angles, yaw rate, estimated velocity), :271-276 (dR and robotBaseR on horizontal terrain),
//                                             :294 (stateDes 6-8, 11), :306 (normalizedPhase), :408-424 (the map's entries), :446-448 (the VELOCITY flag)
//   qrRobotVelocityEstimator::Update          quadruped/src/estimators/qr_robot_velocity_estimator.cpp:126-131: estimatedVelocity is left in the base
//                                             frame, the value robot->baseVelocityInBaseFrame receives: rows 6-8 of est_out (qr_estimator_kernel.hip)
// The values of swingJointAnglesVelocities are not kept here: they are rows 24-47 of qrgpu_swing_velocity_batch's output, which that kernel writes for the
// flagged legs alone, so the array keeps a leg's last targets as the map does (d_swing_q of qrgpu_stance_command_batch is that d_out + 24 * n).
// Row k of an array lies at p[k * S]: the kernel passes the robot's column and S = n, a packed record has S = 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#ifndef QR_HD
#define QR_HD __host__ __device__ __forceinline__
#endif

namespace qrgpu {
namespace velocity_flow {

enum { TERRAIN_STAIRS = 2 };                                                   // TerrainType: PLANE 0 and PLUM_PILES 1 are "horizontal" (:271)

// ein / eout / gnd / go / gs / des: est_in, est_out, ground_out (read on terrain >= 2 alone, else may be null), gait_out, gait_state, state_des.
// sv / eiw / mem / flag: swing_vel_in, est_in again (or another array), the entries (bit per leg), swing_flag; each may be null, flag needs mem.
// eiw may be ein: the rows written there (41-44) are not among the rows read (6-9, 12, 17-28), and every load is made before the first store.
QR_HD void velocity_inputs(int terrain, bool rst, size_t S, const float *ein, const float *eout, const float *gnd, const float *go, const float *gs,
                           const float *des, float *sv, float *eiw, int *mem, float *flag)
{
    const float LEG_SWING = 0.f, LEG_STANCE = 1.f, LEG_EARLY_CONTACT = 2.f;    // LegState, config/qr_enum_types.h, as the gait kernel writes them
    float phase[4], want[4], leg[4], allow[4], vb[3], sp[4], R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, ang[12];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        phase[a] = go[(size_t)(4 + a) * S]; want[a] = go[(size_t)(8 + a) * S]; leg[a] = go[(size_t)(12 + a) * S]; allow[a] = gs[(size_t)(20 + a) * S];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { vb[a] = eout[(size_t)(6 + a) * S]; sp[a] = des[(size_t)(6 + a) * S]; }
    sp[3] = des[11 * S];
    const float yaw_rate = ein[12 * S];
#pragma unroll
    for (int k = 0; k < 12; ++k) ang[k] = ein[(size_t)(17 + k) * S];
    if (terrain >= TERRAIN_STAIRS) {                                           // dR = baseRInControlFrame, robotBaseR = baseRMat (:275)
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = gnd[(size_t)(22 + k) * S];
#pragma unroll
        for (int a = 0; a < 4; ++a) q[a] = ein[(size_t)(6 + a) * S];
    }
    const int had = mem ? *mem : 0;                                            // loaded whatever rst says
    int ids = 0;                                                               // swingFootIds
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const bool skip = (leg[l] == LEG_STANCE && allow[l] != 0.f) || leg[l] == LEG_EARLY_CONTACT;
        if (!skip) ids |= 1 << l;
    }
    const int entries = (rst ? 0 : (had & 0xf)) | ids;                         // Reset() clears the map, GetAction adds every leg of swingFootIds
    if (sv) {
#pragma unroll
        for (int l = 0; l < 4; ++l) { sv[(size_t)l * S] = ((ids >> l) & 1) ? 1.f : 0.f; sv[(size_t)(4 + l) * S] = phase[l]; }
#pragma unroll
        for (int a = 0; a < 3; ++a) sv[(size_t)(20 + a) * S] = vb[a];
        sv[23 * S] = yaw_rate;
#pragma unroll
        for (int a = 0; a < 4; ++a) sv[(size_t)(24 + a) * S] = sp[a];
#pragma unroll
        for (int k = 0; k < 9; ++k) sv[(size_t)(28 + k) * S] = R[k];
#pragma unroll
        for (int a = 0; a < 4; ++a) sv[(size_t)(37 + a) * S] = q[a];
#pragma unroll
        for (int k = 0; k < 12; ++k) sv[(size_t)(41 + k) * S] = ang[k];
    }
    if (eiw) {
#pragma unroll
        for (int a = 0; a < 4; ++a) eiw[(size_t)(41 + a) * S] = want[a];
    }
    if (mem) *mem = entries;
    if (flag) {
#pragma unroll
        for (int l = 0; l < 4; ++l) flag[(size_t)l * S] = (((entries >> l) & 1) && want[l] == LEG_SWING) ? 1.f : 0.f;
    }
}

}  // namespace velocity_flow
}  // namespace qrgpu
