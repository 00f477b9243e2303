// The two per-robot maps of the cadenced tick (qrgpu_tick_cadence_batch, include/qrgpu.h), per robot: what qr_cadence_kernel (qr_cadence_kernel.hip)
// runs per lane.  float32 as the MPC kernel's output phase is; the rotation matrix with contraction off (quat_to_rot), the two contractions as
// mpc_outputs writes them (no pragma of their own: the build's fast-honor-pragmas rule).  Every function is __host__ __device__: the same text
// compiles for a CPU check against tests/cadence_ref.py (tests/stubs/cadence_host.hip, which makes the __device__ helpers of qr_wave_helpers.h host
// functions too).
//   MPCStanceLegController::GetAction         quadruped/src/controllers/mpc/qr_mpc_stance_leg_controller.cpp:129-156, :402-409  (f_ff = -R^T f, kept
//                                             between solves; every tick maps the kept force through the CURRENT Jacobian)
//   qrRobot::MapContactForceToJointTorques    quadruped/src/robots/qr_robot.cpp:148-172, :196-207 (AnalyticalLegJacobian^T f)
// Row k of an array lies at p[k * S]: the kernel passes the robot's column and S = n, a packed record has S = 1.
#pragma once
#include "qr_wave_helpers.h"
#include "qr_rigid_body.h"

namespace qrgpu {
namespace cadence {

// ---- a robot that has just been solved: hold = f_ff = -R^T f, R = Quaternion(quat).toRotationMatrix() of the state the solve read.  quat: rows w, x, y, z
// (rows 6-9 of d_mpc_state); force, hold: 12 rows, 3 * leg + axis.  The expression is mpc_outputs' (qr_mpc_kernel.hip).
QR_HD void hold_from_force(size_t S, const float *quat, const float *force, float *__restrict__ hold)
{
    float R[3][3], f[12];
    quat_to_rot(quat[0], quat[S], quat[2 * S], quat[3 * S], R);
#pragma unroll
    for (int k = 0; k < 12; ++k) f[k] = force[(size_t)k * S];
#pragma unroll
    for (int leg = 0; leg < 4; ++leg) {
        const float fx = f[3 * leg], fy = f[3 * leg + 1], fz = f[3 * leg + 2];
#pragma unroll
        for (int i = 0; i < 3; ++i) hold[(size_t)(3 * leg + i) * S] = (-R[0][i]) * fx + (-R[1][i]) * fy + (-R[2][i]) * fz;
    }
}

// ---- a robot that is not solved this tick: tau = J(q)^T hold on all four legs, q the joint angles of NOW (rows 13-24 of d_fb_state), hold the base-frame
// force kept from the robot's last solve.  Leg geometry of the robot's type; odd legs (FL, RL) carry +hip_l.  Raw: the torque tail comes after the
// stance / swing merge (qr_wbc_kernel).
QR_HD void held_torque(float hip_l, float upper_l, float lower_l, size_t S, const float *q, const float *hold, float *__restrict__ tau)
{
    float a[12], f[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { a[k] = q[(size_t)k * S]; f[k] = hold[(size_t)k * S]; }
#pragma unroll
    for (int leg = 0; leg < 4; ++leg) {
        const float sh = hip_l * ((leg & 1) ? 1.f : -1.f);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float J0, J1, J2;
            leg_jacobian_column(j, a[3 * leg], a[3 * leg + 1], a[3 * leg + 2], sh, upper_l, lower_l, J0, J1, J2);
            tau[(size_t)(3 * leg + j) * S] = J0 * f[3 * leg] + J1 * f[3 * leg + 1] + J2 * f[3 * leg + 2];
        }
    }
}

}  // namespace cadence
}  // namespace qrgpu
