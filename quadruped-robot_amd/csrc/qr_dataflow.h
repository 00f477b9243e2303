// The three stages between the trot's kernels, per robot: what qr_command_kernel, qr_trot_inputs_kernel and qr_mpc_command_kernel
// (qr_dataflow_kernel.hip) run per lane.  float32 where the reference is float32, its double literals promoting where they do there; contraction
// off.  Every function is __host__ __device__: the same text compiles for a CPU check against tests/dataflow_ref.py (tests/stubs/dataflow_host.hip,
// which makes the __device__ helpers of qr_wave_helpers.h host functions too).  include/qrgpu.h states the rules.
//   qrDesiredStateCommand::Update             quadruped/src/controllers/qr_desired_state_command.cpp:164-265   (members: qr_desired_state_command.hpp)
//   qrRobot::GetFootPositionsInWorldFrame     quadruped/src/robots/qr_robot.cpp:222-230
//   TorqueStanceLegController::UpdateFRatio   quadruped/src/controllers/balance_controller/qr_torque_stance_leg_controller.cpp:103-124 (the contacts
//                                             MPCStanceLegController::Run reads, qr_mpc_stance_leg_controller.cpp:161, :212)
//   MPCStanceLegController::GetAction         quadruped/src/controllers/mpc/qr_mpc_stance_leg_controller.cpp:129-156
//   qrRaibertSwingLegController::GetAction    quadruped/src/controllers/qr_swing_leg_controller.cpp:419, :426-459
//   qrLocomotionController::GetAction         quadruped/src/controllers/qr_locomotion_controller.cpp:128-147
//   qrFSMStateLocomotion::Run, UpdateLegCMD   quadruped/src/fsm/qr_fsm_state_locomotion.cpp:140-157, controllers/wbc/qr_wbc_locomotion_controller.cpp:205-217
// Row k of an array lies at p[k * S]: the kernel passes the robot's column and S = n, a packed record has S = 1.
#pragma once
#include "qr_wave_helpers.h"
#include "qr_rigid_body.h"

namespace qrgpu {
namespace dataflow {

enum { RC_HARD_CODE = 0, RC_JOY_TROT = 1, RC_JOY_ADVANCED_TROT = 2, RC_JOY_WALK = 3, RC_JOY_STAND = 4 };     // RC_MODE, config/qr_enum_types.h:101-113
enum { LEG_SWING = 0, LEG_STANCE = 1, LEG_EARLY_CONTACT = 2, LEG_USERDEFINED_SWING = 4 };                    // LegState, config/qr_enum_types.h

// robotics::math::clip<float> (utils/qr_algebra.h:57-65): a NaN passes
QR_HD float clipf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
// A value as loaded, or +0 under a reset (keep = 0): the load stays unconditional (qr_observe.h: kept)
QR_HD float kept(float x, unsigned keep) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & keep); }

// ---- qrDesiredStateCommand::Update.  joy rows: joyCmdVx, Vy, Vz, RollRate, PitchRate, YawRate, joycmdBodyHeight, joyCtrlState; st rows: filteredVel,
// filteredOmega.  rst: the robot starts from a zero column.  Any output may be null.  The joy rows are the caller's and are not written: the zeros
// the JOY_STAND / else branches assign to the joyCmd members (:214-219, :235-240) are overwritten by the next JoyCallback there.
QR_HD void command_update(const qrgpu_command_desc &D, bool rst, size_t S, const float *joy, float *__restrict__ st, float *__restrict__ des,
                          float *__restrict__ fe, float *__restrict__ fh, float *__restrict__ sv, float *__restrict__ sc)
{
#pragma clang fp contract(off)
    const unsigned keep = rst ? 0u : 0xffffffffu;
    float j[8], f[6];
#pragma unroll
    for (int k = 0; k < 8; ++k) j[k] = joy[(size_t)k * S];
#pragma unroll
    for (int k = 0; k < 6; ++k) f[k] = kept(st[(size_t)k * S], keep);
    const float m = j[7];
    const int mode = (m >= 0.f && m <= 7.f) ? (int)m : 7;                     // anything that is no RC_MODE takes the else branch, as EXIT does
    if (mode == RC_JOY_TROT || mode == RC_JOY_ADVANCED_TROT || mode == RC_JOY_WALK) {
        // filtered * (1.0 - filterFactor) + cmd * filterFactor (:223-230): the double factor is narrowed to the vector's scalar, products and sum float
        const float a = (float)(1.0 - (double)D.filter_factor);
#pragma unroll
        for (int k = 0; k < 6; ++k) f[k] = f[k] * a + j[k] * D.filter_factor;
    } else if (mode == RC_HARD_CODE) {
#pragma unroll
        for (int k = 0; k < 6; ++k) f[k] = j[k];                              // vDesInBodyFrame, wDesInBodyFrame (:232-233)
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) f[k] = 0.f;                               // JOY_STAND, BODY_UP, BODY_DOWN, EXIT (:220-221, :241-242)
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) st[(size_t)k * S] = f[k];
    float d[12];
    const float zero = 0.f;                                                    // stateDes.setZero() (:171)
    d[0] = D.dt * zero; d[1] = D.dt * zero;                                    // dt * stateDes(6), (7): entries of the vector just zeroed (:245-246)
    d[2] = j[6];
    d[3] = 0.f;
    d[4] = clipf(f[4] * D.dt, D.min_pitch, D.max_pitch);
    d[5] = D.dt * zero;                                                        // dt * stateDes(11), zero as well (:251)
    d[6] = clipf(f[0], D.min_velx, D.max_velx);
    d[7] = clipf(f[1], D.min_vely, D.max_vely);
    d[8] = 0.f; d[9] = 0.f; d[10] = 0.f;
    d[11] = clipf(f[5], D.min_yawrate, D.max_yawrate);
    if ((double)d[6] < -0.01) d[2] = (float)((double)j[6] * 0.85);             // walking back (:262-263)
    if (des) {
#pragma unroll
        for (int k = 0; k < 12; ++k) des[(size_t)k * S] = d[k];
    }
    if (fe) {                                                                  // stateDes 2, 3, 4, 6, 7, 11
        fe[0] = d[2]; fe[S] = d[3]; fe[2 * S] = d[4]; fe[3 * S] = d[6]; fe[4 * S] = d[7]; fe[5 * S] = d[11];
    }
    if (fh) { fh[16 * S] = d[6]; fh[17 * S] = d[7]; fh[18 * S] = d[8]; fh[19 * S] = d[11]; fh[20 * S] = d[2]; }
    if (sv) { sv[23 * S] = d[6]; sv[24 * S] = d[7]; sv[25 * S] = d[8]; sv[26 * S] = d[11]; }
    if (sc) { sc[0] = d[2]; sc[S] = d[6]; sc[2 * S] = d[7]; sc[3 * S] = d[8]; sc[4 * S] = d[9]; sc[5 * S] = d[10]; sc[6 * S] = d[11]; }
}

// contacts[leg] of UpdateFRatio outside the walk mode and robot->stop: (desired STANCE and allowSwitchLegState) or legState EARLY_CONTACT
QR_HD bool leg_contact(float desired, float allow, float leg) { return ((int)desired == LEG_STANCE && allow != 0.f) || (int)leg == LEG_EARLY_CONTACT; }

// ---- the getters between the stages.  ein / eout / rpy / go / gs: est_in, est_out, d_rpy, gait_out, gait_state (gs is read for fe alone).  eiw is est_in
// again (or another array, or null): the rows written there (41-44) are not among the rows read (6-12, 17-28), and every load is made before the
// first store.
QR_HD void trot_inputs(size_t S, const float *ein, const float *eout, const float *rpy, const float *go, const float *gs, float *fe, float *fh, float *sw, float *eiw)
{
#pragma clang fp contract(off)
    float q[4], w[3], ang[12], vw[3], vb[3], fp[12], bp[3], r[3], des[4], leg[4], allow[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int a = 0; a < 4; ++a) { q[a] = ein[(size_t)(6 + a) * S]; des[a] = go[(size_t)(8 + a) * S]; leg[a] = go[(size_t)(12 + a) * S]; }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        w[a] = ein[(size_t)(10 + a) * S]; vw[a] = eout[(size_t)(3 + a) * S]; vb[a] = eout[(size_t)(6 + a) * S]; bp[a] = eout[(size_t)(36 + a) * S];
        r[a] = rpy[(size_t)a * S];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) { ang[k] = ein[(size_t)(17 + k) * S]; fp[k] = eout[(size_t)(12 + k) * S]; }
    if (fe) {
#pragma unroll
        for (int a = 0; a < 4; ++a) allow[a] = gs[(size_t)(20 + a) * S];
    }
    if (fe) {
#pragma unroll
        for (int a = 0; a < 3; ++a) fe[(size_t)(6 + a) * S] = bp[a];
        fe[9 * S] = r[2];
#pragma unroll
        for (int a = 0; a < 4; ++a) { fe[(size_t)(10 + a) * S] = q[a]; fe[(size_t)(38 + a) * S] = leg_contact(des[a], allow[a], leg[a]) ? 1.f : 0.f; }
#pragma unroll
        for (int l = 0; l < 4; ++l) {                                          // invertRigidTransform(basePosition, baseOrientation, footPositionsInBaseFrame)
            float pw[3];
            invert_rigid_transform(q, bp, fp + 3 * l, pw);
            fe[(size_t)(14 + 3 * l) * S] = pw[0]; fe[(size_t)(15 + 3 * l) * S] = pw[1]; fe[(size_t)(16 + 3 * l) * S] = pw[2];
        }
    }
    if (fh) {
#pragma unroll
        for (int k = 0; k < 12; ++k) fh[(size_t)(21 + k) * S] = fp[k];
#pragma unroll
        for (int a = 0; a < 4; ++a) fh[(size_t)(33 + a) * S] = q[a];
#pragma unroll
        for (int a = 0; a < 3; ++a) { fh[(size_t)(37 + a) * S] = r[a]; fh[(size_t)(40 + a) * S] = vb[a]; fh[(size_t)(43 + a) * S] = w[a]; }
    }
    if (sw) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { sw[(size_t)(36 + a) * S] = bp[a]; sw[(size_t)(43 + a) * S] = vw[a]; }
#pragma unroll
        for (int a = 0; a < 4; ++a) sw[(size_t)(39 + a) * S] = q[a];
#pragma unroll
        for (int k = 0; k < 12; ++k) sw[(size_t)(46 + k) * S] = ang[k];
    }
    if (eiw) {
#pragma unroll
        for (int a = 0; a < 4; ++a) eiw[(size_t)(41 + a) * S] = des[a];
    }
}

// ---- the motor command of the MPC mode.  tau [12], qdes [24] (angles, velocities), sw rows 0-3 (the legs swing_targets computed: they get an entry in
// swingJointAnglesVelocities, :419), go / gs: gait_out, gait_state, mem: the entries, bit per leg.  A leg with an entry whose flag of :450-452 holds
// carries {q, kp, qd, kd, tua}; every other motor {0, 100 on the abad of an EARLY_CONTACT leg else 0, 0, stance_kd, tau}.  tua of a swing command is 0
// plus the abad compensation qrFSMStateLocomotion::Run adds to every motor (epilogue bit 0), clipped (bit 1) -- unless the leg is in contact_state,
// where UpdateLegCMD overwrites tua with the WBC's torque, which is d_tau.  d_tau itself carries the epilogue from the tick already.
QR_HD void mpc_command(const qrgpu_mpc_command_desc &D, bool rst, size_t S, const float *tau, const float *qdes, const float *sw, const float *go, const float *gs,
                       int *__restrict__ mem, float *__restrict__ cmd)
{
#pragma clang fp contract(off)
    float t[12], qa[12], qv[12], flag[4], des[4], leg[4], cur[4], allow[4];
#pragma unroll
    for (int k = 0; k < 12; ++k) { t[k] = tau[(size_t)k * S]; qa[k] = qdes[(size_t)k * S]; qv[k] = qdes[(size_t)(12 + k) * S]; }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        flag[a] = sw[(size_t)a * S]; des[a] = go[(size_t)(8 + a) * S]; leg[a] = go[(size_t)(12 + a) * S]; cur[a] = go[(size_t)(16 + a) * S];
        allow[a] = gs[(size_t)(20 + a) * S];
    }
    const int had = *mem;                                                      // loaded whatever rst says (qr_observe.h: kept)
    int entries = rst ? 0 : (had & 0xf);
#pragma unroll
    for (int l = 0; l < 4; ++l) if (flag[l] != 0.f) entries |= 1 << l;
    *mem = entries;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int ls = (int)leg[l];
        const bool swing = ((entries >> l) & 1) && (ls == LEG_SWING || ls == LEG_USERDEFINED_SWING || ((int)cur[l] == LEG_SWING && allow[l] == 0.f));
        const bool contact = leg_contact(des[l], allow[l], leg[l]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int mtr = 3 * l + a;
            float c[5];
            if (swing) {
                c[0] = qa[mtr]; c[1] = D.kp[mtr]; c[2] = qv[mtr]; c[3] = D.kd[mtr];
                c[4] = contact ? t[mtr] : torque_epilogue(0.f, mtr, true, D.epilogue);
            } else {
                c[0] = 0.f; c[1] = (ls == LEG_EARLY_CONTACT && a == 0) ? D.early_contact_abad_kp : 0.f; c[2] = 0.f; c[3] = D.stance_kd; c[4] = t[mtr];
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) cmd[(size_t)(12 * k + mtr) * S] = c[k];
        }
    }
}

}  // namespace dataflow
}  // namespace qrgpu
