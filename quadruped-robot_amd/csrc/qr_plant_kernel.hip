// ============================================================================
// The plant of a batch of quadrupeds: what turns the torque of tick t into the state of tick t + 1.  gfx950 (MI355X) only.
//
//   qr_fwd_dyn_kernel     forward dynamics of the floating-base model (base, 12 links, 12 rotors): FloatingBaseModel::runABA with
//                         _externalForces, QS/dynamics/floating_base_model.cpp:876-947 -- "never called" on the reference's controller path,
//                         which leaves the plant to Gazebo
//   qr_plant_step_kernel  one control tick of `substeps` sub-steps: the Gazebo joint controller's motor law, a ground contact law of OUR OWN (the
//                         reference has none), the forward dynamics, semi-implicit Euler; the state lives in fp64 registers across the sub-steps
//   qr_plant_step_terrain_kernel  the same tick on a height field chosen per robot (qr_terrain.h), with a world-frame wrench on the base held for
//                         the tick
//   (qr_plant_step_body_kernel, the terrain tick with knee and trunk contact and joint limits, is qr_plant_body_kernel.hip's; what the plant kernels
//   share on the device -- the quad's sums, who_am_i, forward_dynamics, the LDS column, and the named pieces of the tick that the terrain and the
//   body kernel call: state in, motor law, integrator, state check, plant_out -- is qr_plant_quad.h)
//
// Four lanes per robot, one per leg (the way qr_wbc_kernel walks the tree), sixteen robots per 64-lane wavefront, one wavefront per workgroup.
// A leg's articulated inertia and bias force reach the base through two __shfl_xor steps inside the quad; every lane of the quad then solves
// the base's 6 x 6 system (the same arithmetic on the same bits: the four copies of the base state never part).  No scratch, no
// runtime-indexed local array: the algebra of qr_plant_math.h is structs of scalars, and the recursion over a leg's joints is a loop whose
// carried values sit in a lane-private column of LDS (72 doubles a lane, 36 KiB a workgroup).  The four lanes of a robot are live or idle together: an
// idle quad (robot index beyond the batch) computes on the last robot's inputs and stores nothing.
// fp64 arithmetic on the fp32 inputs, as in the WBC kernel; the rotors' velocity-product terms, which that kernel drops, are kept.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_wave_helpers.h"
#include "qr_kernels.h"
#include "qr_plant_math.h"
#include "qr_plant_quad.h"
#include "qr_terrain.h"

namespace qrgpu {

using namespace plant;

__global__ void __launch_bounds__(64) qr_fwd_dyn_kernel(int n, const WbcConst *__restrict__ types, const int *__restrict__ type_id, int type_ready,
                                                        const float *__restrict__ g_state, const float *__restrict__ g_tau, const float *__restrict__ g_ff,
                                                        float *__restrict__ g_nudot, int *__restrict__ g_status)
{
    Who w = who_am_i(n, types, type_id, type_ready);
    const WbcConst &K = *w.K;
    const size_t N = (size_t)n;
    const int i = w.robot, leg = w.leg, j = 3 * leg;
    real qw = ROW(g_state, 0), qx = ROW(g_state, 1), qy = ROW(g_state, 2), qz = ROW(g_state, 3);
    unit_quat(qw, qx, qy, qz, w.flags);
    const frame3 R = quat_to_rot(qw, qx, qy, qz);
    sv6 v0;
    v0.a = mk(ROW(g_state, 7), ROW(g_state, 8), ROW(g_state, 9));
    v0.l = mk(ROW(g_state, 10), ROW(g_state, 11), ROW(g_state, 12));
    const real q0 = ROW(g_state, 13 + j), q1 = ROW(g_state, 14 + j), q2 = ROW(g_state, 15 + j);
    const real qd0 = ROW(g_state, 25 + j), qd1 = ROW(g_state, 26 + j), qd2 = ROW(g_state, 27 + j);
    const real tau0 = ROW(g_tau, j), tau1 = ROW(g_tau, j + 1), tau2 = ROW(g_tau, j + 2);
    v3 f = mk(0, 0, 0);
    if (g_ff) f = mk(ROW(g_ff, j), ROW(g_ff, j + 1), ROW(g_ff, j + 2));
    QR_PL_STASH();
    v3 foot, foot_vel;
    leg_start(K, leg, st, q0, q1, q2, qd0, qd1, qd2, v0, foot, foot_vel);
    sv6 afb;
    real qdd0, qdd1, qdd2;
    forward_dynamics(K, leg, st, R, v0, qd0, qd1, qd2, tau0, tau1, tau2, mulT(R, f), afb, qdd0, qdd1, qdd2);
    int bad = !(finite3(afb.a) && finite3(afb.l) && isfinite(qdd0) && isfinite(qdd1) && isfinite(qdd2));
    if (quad_or(bad)) w.flags |= QRGPU_PL_NONFINITE;
    if (!w.live) return;
    ROW(g_nudot, 6 + j) = (float)qdd0; ROW(g_nudot, 7 + j) = (float)qdd1; ROW(g_nudot, 8 + j) = (float)qdd2;
    if (leg == 0) { ROW(g_nudot, 0) = (float)afb.a.x; ROW(g_nudot, 1) = (float)afb.a.y; ROW(g_nudot, 2) = (float)afb.a.z; }
    if (leg == 1) { ROW(g_nudot, 3) = (float)afb.l.x; ROW(g_nudot, 4) = (float)afb.l.y; ROW(g_nudot, 5) = (float)afb.l.z; }
    if (leg == 2 && g_status) g_status[i] = w.flags;
}


// The three step kernels (the two here and qr_plant_step_body_kernel) are one control tick: the state in, per sub-step the motor law, the contact
// forces, the forward dynamics and the integrator, then the state check, the state out and the outputs.  The terrain and the body kernel call the
// steps they share as the named pieces of qr_plant_quad.h.  THIS kernel keeps them written out, state_check apart: with any other piece called, or
// with more of them, its launch measured 80 to 200 ns over what it was (five sittings a side; DESIGN 4.6, "One tick, three kernels").  A change to
// a piece of qr_plant_quad.h is made here too.
__global__ void __launch_bounds__(64) qr_plant_step_kernel(int n, qrgpu_plant_params P, const WbcConst *__restrict__ types, const int *__restrict__ type_id,
                                                           int type_ready, float *g_state, const float *__restrict__ g_cmd, float *__restrict__ g_out,
                                                           float *__restrict__ g_mpc, float *__restrict__ g_est, int *__restrict__ g_status)
{
    Who w = who_am_i(n, types, type_id, type_ready);
    const WbcConst &K = *w.K;
    const size_t N = (size_t)n;
    const int i = w.robot, leg = w.leg, j = 3 * leg;
    // the state: read once
    real qw = ROW(g_state, 0), qx = ROW(g_state, 1), qy = ROW(g_state, 2), qz = ROW(g_state, 3);
    unit_quat(qw, qx, qy, qz, w.flags);
    v3 pos = mk(ROW(g_state, 4), ROW(g_state, 5), ROW(g_state, 6));
    sv6 v0;
    v0.a = mk(ROW(g_state, 7), ROW(g_state, 8), ROW(g_state, 9));
    v0.l = mk(ROW(g_state, 10), ROW(g_state, 11), ROW(g_state, 12));
    real q0 = ROW(g_state, 13 + j), q1 = ROW(g_state, 14 + j), q2 = ROW(g_state, 15 + j);
    real qd0 = ROW(g_state, 25 + j), qd1 = ROW(g_state, 26 + j), qd2 = ROW(g_state, 27 + j);
    const real cp0 = ROW(g_cmd, j), cp1 = ROW(g_cmd, j + 1), cp2 = ROW(g_cmd, j + 2);
    const real kp0 = ROW(g_cmd, 12 + j), kp1 = ROW(g_cmd, 13 + j), kp2 = ROW(g_cmd, 14 + j);
    const real cd0 = ROW(g_cmd, 24 + j), cd1 = ROW(g_cmd, 25 + j), cd2 = ROW(g_cmd, 26 + j);
    const real kd0 = ROW(g_cmd, 36 + j), kd1 = ROW(g_cmd, 37 + j), kd2 = ROW(g_cmd, 38 + j);
    const real ff0 = ROW(g_cmd, 48 + j), ff1 = ROW(g_cmd, 49 + j), ff2 = ROW(g_cmd, 50 + j);
    const real h = (real)P.dt / (real)P.substeps;
    const real ck = P.contact_k, ca = P.contact_a, mu = P.mu, v_eps = P.v_eps, ground_z = P.ground_z, tau_max = P.tau_max;

    QR_PL_STASH();
    v3 f_w = mk(0, 0, 0), acc = mk(0, 0, 0);
    sv6 afb; afb.a = afb.l = mk(0, 0, 0);
    real fn = 0, tau0 = 0, tau1 = 0, tau2 = 0, qdd0 = 0, qdd1 = 0, qdd2 = 0;
#pragma unroll 1
    for (int s = 0; s < P.substeps; ++s) {
        const frame3 R = quat_to_rot(qw, qx, qy, qz);
        tau0 = clip(kp0 * (cp0 - q0) + kd0 * (cd0 - qd0) + ff0, tau_max);
        tau1 = clip(kp1 * (cp1 - q1) + kd1 * (cd1 - qd1) + ff1, tau_max);
        tau2 = clip(kp2 * (cp2 - q2) + kd2 * (cd2 - qd2) + ff2, tau_max);
        // the foot point: position and velocity in the world
        v3 foot, foot_vel;
        leg_start(K, leg, st, q0, q1, q2, qd0, qd1, qd2, v0, foot, foot_vel);
        const v3 p_w = pos + mul(R, foot), v_w = mul(R, foot_vel);
        f_w = contact_force(ground_z, ck, ca, mu, v_eps, p_w, v_w, fn);
        forward_dynamics(K, leg, st, R, v0, qd0, qd1, qd2, tau0, tau1, tau2, mulT(R, f_w), afb, qdd0, qdd1, qdd2);
        acc = (afb.l + cross(v0.a, v0.l)) + mulT(R, mk(0, 0, QR_PL_GRAVITY));      // what an accelerometer at the base origin reads over this sub-step
        // semi-implicit Euler: rates first, then positions with the new rates
        v0 = v0 + h * afb;
        qd0 += h * qdd0; qd1 += h * qdd1; qd2 += h * qdd2;
        q0 += h * qd0; q1 += h * qd1; q2 += h * qd2;
        pos = pos + h * mul(R, v0.l);
        // quat <- normalise(quat (x) exp(h omega_body))
        const v3 hw = h * v0.a;
        const real th = sqrt(dot(hw, hw));
        const real cw = cos(0.5 * th), sc = th < 1e-8 ? 0.5 : sin(0.5 * th) / th;
        const v3 e = sc * hw, qv = mk(qx, qy, qz);
        const real nw = qw * cw - dot(qv, e);
        const v3 nv = (qw * e + cw * qv) + cross(qv, e);
        qw = nw; qx = nv.x; qy = nv.y; qz = nv.z;
        const real inv = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
        qw *= inv; qx *= inv; qy *= inv; qz *= inv;
    }
    state_check(w.flags, qw, qx, qy, qz, pos, v0, q0, q1, q2, qd0, qd1, qd2);
    if (!w.live) return;

    // the state: written once.  Rows of the base go out from the lane of leg 0, a leg's joints from its own lane.
    const float fq[4] = {(float)qw, (float)qx, (float)qy, (float)qz};
    ROW(g_state, 13 + j) = (float)q0; ROW(g_state, 14 + j) = (float)q1; ROW(g_state, 15 + j) = (float)q2;
    ROW(g_state, 25 + j) = (float)qd0; ROW(g_state, 26 + j) = (float)qd1; ROW(g_state, 27 + j) = (float)qd2;
    if (leg == 0) {
        ROW(g_state, 0) = fq[0]; ROW(g_state, 1) = fq[1]; ROW(g_state, 2) = fq[2]; ROW(g_state, 3) = fq[3];
        ROW(g_state, 4) = (float)pos.x; ROW(g_state, 5) = (float)pos.y; ROW(g_state, 6) = (float)pos.z;
        ROW(g_state, 7) = (float)v0.a.x; ROW(g_state, 8) = (float)v0.a.y; ROW(g_state, 9) = (float)v0.a.z;
        ROW(g_state, 10) = (float)v0.l.x; ROW(g_state, 11) = (float)v0.l.y; ROW(g_state, 12) = (float)v0.l.z;
    }
    if (leg == 2 && g_status) g_status[i] = w.flags;
    // the foot of the state just written
    const frame3 R = quat_to_rot(qw, qx, qy, qz);
    v3 foot_b, foot_vel;
    leg_start(K, leg, st, q0, q1, q2, qd0, qd1, qd2, v0, foot_b, foot_vel);
    const v3 foot_w = pos + mul(R, foot_b);
    const float contact = fn > (real)P.contact_threshold ? 1.f : 0.f;
    if (g_out) {
        ROW(g_out, j) = (float)f_w.x; ROW(g_out, j + 1) = (float)f_w.y; ROW(g_out, j + 2) = (float)f_w.z;
        ROW(g_out, 12 + j) = (float)foot_w.x; ROW(g_out, 13 + j) = (float)foot_w.y; ROW(g_out, 14 + j) = (float)foot_w.z;
        ROW(g_out, 24 + leg) = contact;
        ROW(g_out, 28 + j) = (float)tau0; ROW(g_out, 29 + j) = (float)tau1; ROW(g_out, 30 + j) = (float)tau2;
        ROW(g_out, 46 + j) = (float)qdd0; ROW(g_out, 47 + j) = (float)qdd1; ROW(g_out, 48 + j) = (float)qdd2;
        if (leg == 0) { ROW(g_out, 40) = (float)afb.a.x; ROW(g_out, 41) = (float)afb.a.y; ROW(g_out, 42) = (float)afb.a.z; }
        if (leg == 1) { ROW(g_out, 43) = (float)afb.l.x; ROW(g_out, 44) = (float)afb.l.y; ROW(g_out, 45) = (float)afb.l.z; }
    }
    if (g_mpc) {      // the ground truth in qrgpu_pack_state_batch's conventions
        const v3 r = mul(R, foot_b - mk(P.com_offset[0], P.com_offset[1], P.com_offset[2]));
        ROW(g_mpc, 13 + j) = (float)r.x; ROW(g_mpc, 14 + j) = (float)r.y; ROW(g_mpc, 15 + j) = (float)r.z;
        if (leg == 0) {
            ROW(g_mpc, 0) = (float)pos.x; ROW(g_mpc, 1) = (float)pos.y; ROW(g_mpc, 2) = (float)pos.z;
            ROW(g_mpc, 6) = fq[0]; ROW(g_mpc, 7) = fq[1]; ROW(g_mpc, 8) = fq[2]; ROW(g_mpc, 9) = fq[3];
        }
        if (leg == 1) {
            const v3 vw = mul(R, v0.l), ww = mul(R, v0.a);
            ROW(g_mpc, 3) = (float)vw.x; ROW(g_mpc, 4) = (float)vw.y; ROW(g_mpc, 5) = (float)vw.z;
            ROW(g_mpc, 10) = (float)ww.x; ROW(g_mpc, 11) = (float)ww.y; ROW(g_mpc, 12) = (float)ww.z;
        }
        if (leg == 2) {
            float rpy[3];
            quat_to_rpy(fq, rpy);
            ROW(g_mpc, 25) = rpy[0]; ROW(g_mpc, 26) = rpy[1]; ROW(g_mpc, 27) = rpy[2];
        }
    }
    if (g_est) {      // rows 0-40 of est_in, qrRobotA1Sim::ReceiveObservation's quantities without its filters; rows 41-53 are other kernels'
        ROW(g_est, 13 + leg) = contact;
        ROW(g_est, 17 + j) = (float)q0; ROW(g_est, 18 + j) = (float)q1; ROW(g_est, 19 + j) = (float)q2;
        ROW(g_est, 29 + j) = (float)qd0; ROW(g_est, 30 + j) = (float)qd1; ROW(g_est, 31 + j) = (float)qd2;
        if (leg == 0) {
            ROW(g_est, 0) = (float)acc.x; ROW(g_est, 1) = (float)acc.y; ROW(g_est, 2) = (float)acc.z;
            ROW(g_est, 3) = (float)acc.x; ROW(g_est, 4) = (float)acc.y; ROW(g_est, 5) = (float)acc.z;
        }
        if (leg == 1) {
            ROW(g_est, 6) = fq[0]; ROW(g_est, 7) = fq[1]; ROW(g_est, 8) = fq[2]; ROW(g_est, 9) = fq[3];
            ROW(g_est, 10) = (float)v0.a.x; ROW(g_est, 11) = (float)v0.a.y; ROW(g_est, 12) = (float)v0.a.z;
        }
    }
}

// The tick on a height field chosen per robot, with a wrench on the base.  Its own: one surface sample under the foot, the contact law in the
// surface's frame, the base wrench, OFF_FIELD.  The state write and the mpc_state / est_in writes stand written out here, in the body kernel and
// in the flat one: called as pieces they cost this kernel 80 ns a launch and the body kernel 120.
__global__ void __launch_bounds__(64) qr_plant_step_terrain_kernel(int n, qrgpu_plant_params P, qrgpu_terrain_desc T, const WbcConst *__restrict__ types,
                                                                   const int *__restrict__ type_id, int type_ready, const float *__restrict__ g_height,
                                                                   const int *__restrict__ g_field, const float *__restrict__ g_push, float *g_state,
                                                                   const float *__restrict__ g_cmd, float *__restrict__ g_out, float *__restrict__ g_tout,
                                                                   float *__restrict__ g_mpc, float *__restrict__ g_est, int *__restrict__ g_status)
{
    Who w = who_am_i(n, types, type_id, type_ready);
    const WbcConst &K = *w.K;
    const size_t N = (size_t)n;
    const int i = w.robot, leg = w.leg, j = 3 * leg;
    real qw, qx, qy, qz, q0, q1, q2, qd0, qd1, qd2;
    v3 pos;
    sv6 v0;
    state_in(g_state, N, i, j, w.flags, qw, qx, qy, qz, pos, v0, q0, q1, q2, qd0, qd1, qd2);
    const Cmd cmd = cmd_in(g_cmd, N, i, j);
    const real h = (real)P.dt / (real)P.substeps;
    const real ck = P.contact_k, ca = P.contact_a, mu = P.mu, v_eps = P.v_eps, ground_z = P.ground_z, tau_max = P.tau_max;
    const float *field = field_in(T, g_height, g_field, i, w.flags);
    const real gx0 = T.x0, gy0 = T.y0, cell = T.cell;
    v3 push_f, push_m;
    push_in(g_push, N, i, push_f, push_m);
    bool off_field = false;

    QR_PL_STASH();
    v3 f_w = mk(0, 0, 0), acc = mk(0, 0, 0);
    sv6 afb; afb.a = afb.l = mk(0, 0, 0);
    real fn = 0, tau0 = 0, tau1 = 0, tau2 = 0, qdd0 = 0, qdd1 = 0, qdd2 = 0;
#pragma unroll 1
    for (int s = 0; s < P.substeps; ++s) {
        const frame3 R = quat_to_rot(qw, qx, qy, qz);
        // the foot point: position and velocity in the world
        v3 foot, foot_vel;
        leg_start(K, leg, st, q0, q1, q2, qd0, qd1, qd2, v0, foot, foot_vel);
        const v3 p_w = pos + mul(R, foot), v_w = mul(R, foot_vel);
        // the ground under the foot, sampled here, where the fewest values are live; the push in the base frame of this sub-step
        const terrain::Sample g = terrain::sample(field, T.nx, T.ny, gx0, gy0, cell, p_w.x, p_w.y);
        f_w = terrain::contact_force(g.z + ground_z, terrain::normal_of(g.zx, g.zy), ck, ca, mu, v_eps, p_w, v_w, fn);
        off_field = g.off && fn > 0.0;
        // The motor law after the sample, not before it as in the flat kernel: the law reads only q and qd, which the sample does not change, and
        // three fewer doubles are live across the sample.  (With every shared step called as a piece the other order spilled two VGPRs; in the
        // present text it does not, and this order is the one whose launch times were measured.)
        motor_law(cmd, q0, q1, q2, qd0, qd1, qd2, tau_max, tau0, tau1, tau2);
        sv6 wrench; wrench.a = mulT(R, push_m); wrench.l = mulT(R, push_f);
        forward_dynamics<true>(K, leg, st, R, v0, qd0, qd1, qd2, tau0, tau1, tau2, mulT(R, f_w), afb, qdd0, qdd1, qdd2, wrench);
        acc = accelerometer(R, v0, afb);
        integrate(R, h, afb, qdd0, qdd1, qdd2, qw, qx, qy, qz, pos, v0, q0, q1, q2, qd0, qd1, qd2);
    }
    state_check(w.flags, qw, qx, qy, qz, pos, v0, q0, q1, q2, qd0, qd1, qd2);
    if (quad_or(off_field)) w.flags |= QRGPU_PL_OFF_FIELD;
    if (!w.live) return;

    // the state: written once.  Rows of the base go out from the lane of leg 0, a leg's joints from its own lane.
    const float fq[4] = {(float)qw, (float)qx, (float)qy, (float)qz};
    ROW(g_state, 13 + j) = (float)q0; ROW(g_state, 14 + j) = (float)q1; ROW(g_state, 15 + j) = (float)q2;
    ROW(g_state, 25 + j) = (float)qd0; ROW(g_state, 26 + j) = (float)qd1; ROW(g_state, 27 + j) = (float)qd2;
    if (leg == 0) {
        ROW(g_state, 0) = fq[0]; ROW(g_state, 1) = fq[1]; ROW(g_state, 2) = fq[2]; ROW(g_state, 3) = fq[3];
        ROW(g_state, 4) = (float)pos.x; ROW(g_state, 5) = (float)pos.y; ROW(g_state, 6) = (float)pos.z;
        ROW(g_state, 7) = (float)v0.a.x; ROW(g_state, 8) = (float)v0.a.y; ROW(g_state, 9) = (float)v0.a.z;
        ROW(g_state, 10) = (float)v0.l.x; ROW(g_state, 11) = (float)v0.l.y; ROW(g_state, 12) = (float)v0.l.z;
    }
    if (leg == 2 && g_status) g_status[i] = w.flags;
    // the foot of the state just written
    const frame3 R = quat_to_rot(qw, qx, qy, qz);
    v3 foot_b, foot_vel;
    leg_start(K, leg, st, q0, q1, q2, qd0, qd1, qd2, v0, foot_b, foot_vel);
    const v3 foot_w = pos + mul(R, foot_b);
    const float contact = fn > (real)P.contact_threshold ? 1.f : 0.f;
    ground_out(g_tout, N, i, leg, field, T, ground_z, foot_w);
    plant_out(g_out, N, i, leg, (float)f_w.x, (float)f_w.y, (float)f_w.z, foot_w, contact, (float)tau0, (float)tau1, (float)tau2, afb, qdd0, qdd1, qdd2);
    if (g_mpc) {      // the ground truth in qrgpu_pack_state_batch's conventions
        const v3 r = mul(R, foot_b - mk(P.com_offset[0], P.com_offset[1], P.com_offset[2]));
        ROW(g_mpc, 13 + j) = (float)r.x; ROW(g_mpc, 14 + j) = (float)r.y; ROW(g_mpc, 15 + j) = (float)r.z;
        if (leg == 0) {
            ROW(g_mpc, 0) = (float)pos.x; ROW(g_mpc, 1) = (float)pos.y; ROW(g_mpc, 2) = (float)pos.z;
            ROW(g_mpc, 6) = fq[0]; ROW(g_mpc, 7) = fq[1]; ROW(g_mpc, 8) = fq[2]; ROW(g_mpc, 9) = fq[3];
        }
        if (leg == 1) {
            const v3 vw = mul(R, v0.l), ww = mul(R, v0.a);
            ROW(g_mpc, 3) = (float)vw.x; ROW(g_mpc, 4) = (float)vw.y; ROW(g_mpc, 5) = (float)vw.z;
            ROW(g_mpc, 10) = (float)ww.x; ROW(g_mpc, 11) = (float)ww.y; ROW(g_mpc, 12) = (float)ww.z;
        }
        if (leg == 2) {
            float rpy[3];
            quat_to_rpy(fq, rpy);
            ROW(g_mpc, 25) = rpy[0]; ROW(g_mpc, 26) = rpy[1]; ROW(g_mpc, 27) = rpy[2];
        }
    }
    if (g_est) {      // rows 0-40 of est_in, qrRobotA1Sim::ReceiveObservation's quantities without its filters; rows 41-53 are other kernels'
        ROW(g_est, 13 + leg) = contact;
        ROW(g_est, 17 + j) = (float)q0; ROW(g_est, 18 + j) = (float)q1; ROW(g_est, 19 + j) = (float)q2;
        ROW(g_est, 29 + j) = (float)qd0; ROW(g_est, 30 + j) = (float)qd1; ROW(g_est, 31 + j) = (float)qd2;
        if (leg == 0) {
            ROW(g_est, 0) = (float)acc.x; ROW(g_est, 1) = (float)acc.y; ROW(g_est, 2) = (float)acc.z;
            ROW(g_est, 3) = (float)acc.x; ROW(g_est, 4) = (float)acc.y; ROW(g_est, 5) = (float)acc.z;
        }
        if (leg == 1) {
            ROW(g_est, 6) = fq[0]; ROW(g_est, 7) = fq[1]; ROW(g_est, 8) = fq[2]; ROW(g_est, 9) = fq[3];
            ROW(g_est, 10) = (float)v0.a.x; ROW(g_est, 11) = (float)v0.a.y; ROW(g_est, 12) = (float)v0.a.z;
        }
    }
}

}  // namespace qrgpu
