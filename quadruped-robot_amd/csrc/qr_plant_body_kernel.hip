// ============================================================================
// The plant with a body: qr_plant_step_terrain_kernel's tick (qr_plant_kernel.hip) for a robot that touches the ground with sixteen points -- four
// feet, four knees, the eight corners of its trunk -- and whose joints have stops.  gfx950 (MI355X) only.  include/qrgpu.h states the law
// (qrgpu_plant_step_body_batch).
//
// The shape is the plant's: four lanes per robot, sixteen robots per wavefront, the joint loop, the lane-private column of LDS, no barrier.  A
// lane owns its leg's foot and knee and the two trunk corners on its leg's side.  It takes its four points ONE AFTER ANOTHER, in a loop that is
// not unrolled, before the inward pass, where the fewest values are live: a surface sample is sixteen loads and their weights, and four of them
// live at once do not fit beside the state.  What the loop leaves: the foot force and the knee force (they enter the knee link's external force)
// and the corners' wrench on the base, which is summed over the quad and joins the push.
// The step body is the terrain kernel's, written a third time (profiles/terrain_isa_compare.txt: a body shared through a template moved the
// flat kernel's register allocation); what the three share by call is qr_plant_quad.h, qr_plant_math.h, qr_terrain.h.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_wave_helpers.h"
#include "qr_kernels.h"
#include "qr_plant_math.h"
#include "qr_plant_quad.h"
#include "qr_plant_body.h"
#include "qr_terrain.h"

namespace qrgpu {

using namespace plant;

// The second column: foot force, knee force (world) at 0; f_n of the bottom and the top corner at 6; the motor's torque at 8; tau_lim at 11.
#define QR_PB_OUT_FORCE 0
#define QR_PB_OUT_FN    6
#define QR_PB_OUT_TAU   8
#define QR_PB_OUT_TLIM  11
#define QR_PB_OUT_SLOTS 14
#define KEEP(slot) keep[(slot) * 64]
// what the last sub-step met, per lane
#define QR_PB_HIT_FOOT  1
#define QR_PB_HIT_KNEE  2
#define QR_PB_HIT_TRUNK 4
#define QR_PB_HIT_LIMIT 8

__device__ __forceinline__ sv6 quad_sum(sv6 v) { sv6 o; o.a = quad_sum(v.a); o.l = quad_sum(v.l); return o; }

// forward_dynamics<true> with a force at the knee: leg_inward_body in the place of leg_inward.
__device__ __forceinline__ void forward_dynamics_body(const WbcConst &K, int leg, const Stash &st, const frame3 &R, sv6 v0, real qd0, real qd1, real qd2, real tau0,
                                                      real tau1, real tau2, v3 f_b, v3 fk_b, sv6 wrench_b, sv6 &afb, real &qdd0, real &qdd1, real &qdd2)
{
    abi IA;
    sv6 pA;
    leg_inward_body(K, leg, st, qd0, qd1, qd2, tau0, tau1, tau2, f_b, fk_b, IA, pA);
#pragma unroll
    for (int i = 0; i < 6; ++i) { IA.I[i] = quad_sum(IA.I[i]); IA.M[i] = quad_sum(IA.M[i]); }
    IA.h0 = quad_sum(IA.h0); IA.h1 = quad_sum(IA.h1); IA.h2 = quad_sum(IA.h2);
    pA.a = quad_sum(pA.a); pA.l = quad_sum(pA.l);
    abi IA0; sv6 pA0;
    base_start(K, v0, IA0, pA0);
    pA0 = pA0 + (-1.0) * wrench_b;
    sv6 a0;
    base_solve(IA0 + IA, pA0 + pA, R, afb, a0);
    leg_outward(K, leg, st, a0, qdd0, qdd1, qdd2);
}

__global__ void __launch_bounds__(64) qr_plant_step_body_kernel(int n, qrgpu_plant_params P, qrgpu_terrain_desc T, const WbcConst *__restrict__ types,
                                                                const qrgpu_plant_body_desc *__restrict__ bodies, const int *__restrict__ type_id, int type_ready,
                                                                const float *__restrict__ g_height, const int *__restrict__ g_field,
                                                                const float *__restrict__ g_push, float *g_state, const float *__restrict__ g_cmd,
                                                                float *__restrict__ g_out, float *__restrict__ g_tout, float *__restrict__ g_bout,
                                                                float *__restrict__ g_mpc, float *__restrict__ g_est, int *__restrict__ g_status)
{
    Who w = who_am_i(n, types, type_id, type_ready);
    const WbcConst &K = *w.K;
    const qrgpu_plant_body_desc &B = bodies[w.K - types];          // the type's body: the slot of its model constants
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
    const real h = (real)P.dt / (real)P.substeps;
    const real ck = P.contact_k, ca = P.contact_a, mu = P.mu, v_eps = P.v_eps, ground_z = P.ground_z, tau_max = P.tau_max;

    // the robot's field (an id outside the stack: field 0, flagged) and the wrench on its base, world frame: force at the base origin, moment
    int fid = g_field ? g_field[i] : 0;
    if (fid < 0 || fid >= T.n_fields) { fid = 0; w.flags |= QRGPU_PL_BAD_FIELD; }
    const float *field = g_height + (size_t)fid * ((size_t)T.nx * (size_t)T.ny);
    const real gx0 = T.x0, gy0 = T.y0, cell = T.cell;
    bool off_field = false;

    QR_PL_STASH();
    // What only the outputs read -- the forces, the corners' f_n and the torques of the last sub-step -- waits in a second lane-private column, as the
    // float32 it goes out as: sixteen values a lane, 4 KiB a workgroup, so that four workgroups still share a CU's LDS.  Kept in registers across
    // the inward pass they spilled to scratch.  The flags are taken in fp64, where the values are made.
    __shared__ float out_lds[QR_PB_OUT_SLOTS * 64];
    float *const keep = out_lds + threadIdx.x;
    const real thr = (real)P.contact_threshold;
    int hits = 0;
    v3 acc = mk(0, 0, 0);
    sv6 afb; afb.a = afb.l = mk(0, 0, 0);
    real qdd0 = 0, qdd1 = 0, qdd2 = 0;
#pragma unroll 1
    for (int s = 0; s < P.substeps; ++s) {
        const frame3 R = quat_to_rot(qw, qx, qy, qz);
        // The motor command of this leg's joints (p, Kp, d, Kd, tua) and the push are read again at every sub-step, through pointers the compiler cannot
        // see through: held in registers across the inward pass, their 21 doubles were what spilled.  They are inputs, not the state.
        const float *cmd = g_cmd, *push = g_push;
        asm volatile("" : "+s"(cmd), "+s"(push));
        const real cp0 = ROW(cmd, j), cp1 = ROW(cmd, j + 1), cp2 = ROW(cmd, j + 2);
        const real kp0 = ROW(cmd, 12 + j), kp1 = ROW(cmd, 13 + j), kp2 = ROW(cmd, 14 + j);
        const real cd0 = ROW(cmd, 24 + j), cd1 = ROW(cmd, 25 + j), cd2 = ROW(cmd, 26 + j);
        const real kd0 = ROW(cmd, 36 + j), kd1 = ROW(cmd, 37 + j), kd2 = ROW(cmd, 38 + j);
        const real ff0 = ROW(cmd, 48 + j), ff1 = ROW(cmd, 49 + j), ff2 = ROW(cmd, 50 + j);
        real tau0 = clip(kp0 * (cp0 - q0) + kd0 * (cd0 - qd0) + ff0, tau_max);
        real tau1 = clip(kp1 * (cp1 - q1) + kd1 * (cd1 - qd1) + ff1, tau_max);
        real tau2 = clip(kp2 * (cp2 - q2) + kd2 * (cd2 - qd2) + ff2, tau_max);
        KEEP(QR_PB_OUT_TAU) = (float)tau0; KEEP(QR_PB_OUT_TAU + 1) = (float)tau1; KEEP(QR_PB_OUT_TAU + 2) = (float)tau2;
        // the stops: added after the motor's clip
        const real tl0 = limit_torque(q0, qd0, B.q_lo[0], B.q_hi[0], B.limit_k, B.limit_a);
        const real tl1 = limit_torque(q1, qd1, B.q_lo[1], B.q_hi[1], B.limit_k, B.limit_a);
        const real tl2 = limit_torque(q2, qd2, B.q_lo[2], B.q_hi[2], B.limit_k, B.limit_a);
        KEEP(QR_PB_OUT_TLIM) = (float)tl0; KEEP(QR_PB_OUT_TLIM + 1) = (float)tl1; KEEP(QR_PB_OUT_TLIM + 2) = (float)tl2;
        hits = (tl0 != 0.0 || tl1 != 0.0 || tl2 != 0.0) ? QR_PB_HIT_LIMIT : 0;
        tau0 += tl0; tau1 += tl1; tau2 += tl2;
        v3 foot, foot_vel, knee, knee_vel;
        leg_start_body(K, leg, st, q0, q1, q2, qd0, qd1, qd2, v0, foot, foot_vel, knee, knee_vel);
        // the lane's four points, one after another: the ground under each, its force; what stays is two forces and the corners' wrench
        v3 f_b = mk(0, 0, 0), fk_b = mk(0, 0, 0);
        sv6 corners; corners.a = corners.l = mk(0, 0, 0);
        off_field = false;
#pragma unroll 1
        for (int k = 0; k < QR_PB_POINTS; ++k) {
            v3 p_b, v_b;
            lane_point(B, leg, k, v0, foot, foot_vel, knee, knee_vel, p_b, v_b);
            const v3 p_w = pos + mul(R, p_b), v_w = mul(R, v_b);
            const terrain::Sample g = terrain::sample(field, T.nx, T.ny, gx0, gy0, cell, p_w.x, p_w.y);
            real fnk;
            const v3 fw = terrain::contact_force(g.z + ground_z, terrain::normal_of(g.zx, g.zy), ck, ca, mu, v_eps, p_w, v_w, fnk);
            off_field = off_field || (g.off && fnk > 0.0);
            const v3 fb = mulT(R, fw);
            const bool hit = fnk > thr;
            if (k == QR_PB_FOOT) { f_b = fb; if (hit) hits |= QR_PB_HIT_FOOT; }
            else if (k == QR_PB_KNEE) { fk_b = fb; if (hit) hits |= QR_PB_HIT_KNEE; }
            else { corners = corners + corner_wrench(p_b, fb); if (hit) hits |= QR_PB_HIT_TRUNK; }
            if (k <= QR_PB_KNEE) { KEEP(QR_PB_OUT_FORCE + 3 * k) = (float)fw.x; KEEP(QR_PB_OUT_FORCE + 3 * k + 1) = (float)fw.y; KEEP(QR_PB_OUT_FORCE + 3 * k + 2) = (float)fw.z; }
            else KEEP(QR_PB_OUT_FN + k - QR_PB_BOTTOM) = (float)fnk;
        }
        // the base wrench: the push in the base frame of this sub-step and the eight corners' forces
        v3 push_f = mk(0, 0, 0), push_m = mk(0, 0, 0);
        if (push) { push_f = mk(ROW(push, 0), ROW(push, 1), ROW(push, 2)); push_m = mk(ROW(push, 3), ROW(push, 4), ROW(push, 5)); }
        sv6 wrench; wrench.a = mulT(R, push_m); wrench.l = mulT(R, push_f);
        wrench = wrench + quad_sum(corners);
        forward_dynamics_body(K, leg, st, R, v0, qd0, qd1, qd2, tau0, tau1, tau2, f_b, fk_b, wrench, afb, qdd0, qdd1, qdd2);
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
    const int bad = !(isfinite(qw) && isfinite(qx) && isfinite(qy) && isfinite(qz) && finite3(pos) && finite3(v0.a) && finite3(v0.l) && isfinite(q0) && isfinite(q1) &&
                      isfinite(q2) && isfinite(qd0) && isfinite(qd1) && isfinite(qd2));
    if (quad_or(bad)) w.flags |= QRGPU_PL_NONFINITE;
    if (quad_or(off_field)) w.flags |= QRGPU_PL_OFF_FIELD;
    const int any = quad_or(hits);
    if (any & QR_PB_HIT_TRUNK) w.flags |= QRGPU_PL_TRUNK_CONTACT;
    if (any & QR_PB_HIT_KNEE) w.flags |= QRGPU_PL_KNEE_CONTACT;
    if (any & QR_PB_HIT_LIMIT) w.flags |= QRGPU_PL_JOINT_LIMIT;
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
    if (g_bout) {      // of the last sub-step: knee force, knee contact, the two corners' normal forces, the stops' torques
        ROW(g_bout, j) = KEEP(QR_PB_OUT_FORCE + 3); ROW(g_bout, j + 1) = KEEP(QR_PB_OUT_FORCE + 4); ROW(g_bout, j + 2) = KEEP(QR_PB_OUT_FORCE + 5);
        ROW(g_bout, 12 + leg) = (hits & QR_PB_HIT_KNEE) ? 1.f : 0.f;
        ROW(g_bout, 16 + 2 * leg) = KEEP(QR_PB_OUT_FN); ROW(g_bout, 17 + 2 * leg) = KEEP(QR_PB_OUT_FN + 1);
        ROW(g_bout, 24 + j) = KEEP(QR_PB_OUT_TLIM); ROW(g_bout, 25 + j) = KEEP(QR_PB_OUT_TLIM + 1); ROW(g_bout, 26 + j) = KEEP(QR_PB_OUT_TLIM + 2);
    }
    // the foot of the state just written
    const frame3 R = quat_to_rot(qw, qx, qy, qz);
    v3 foot_b, foot_vel;
    leg_start(K, leg, st, q0, q1, q2, qd0, qd1, qd2, v0, foot_b, foot_vel);
    const v3 foot_w = pos + mul(R, foot_b);
    const float contact = (hits & QR_PB_HIT_FOOT) ? 1.f : 0.f;
    if (g_tout) {      // the ground under the foot of the state just written
        const terrain::Sample g = terrain::sample(field, T.nx, T.ny, gx0, gy0, cell, foot_w.x, foot_w.y);
        const v3 nrm = terrain::normal_of(g.zx, g.zy);
        ROW(g_tout, leg) = (float)(g.z + ground_z);
        ROW(g_tout, 4 + j) = (float)nrm.x; ROW(g_tout, 5 + j) = (float)nrm.y; ROW(g_tout, 6 + j) = (float)nrm.z;
    }
    if (g_out) {
        ROW(g_out, j) = KEEP(QR_PB_OUT_FORCE); ROW(g_out, j + 1) = KEEP(QR_PB_OUT_FORCE + 1); ROW(g_out, j + 2) = KEEP(QR_PB_OUT_FORCE + 2);
        ROW(g_out, 12 + j) = (float)foot_w.x; ROW(g_out, 13 + j) = (float)foot_w.y; ROW(g_out, 14 + j) = (float)foot_w.z;
        ROW(g_out, 24 + leg) = contact;
        ROW(g_out, 28 + j) = KEEP(QR_PB_OUT_TAU); ROW(g_out, 29 + j) = KEEP(QR_PB_OUT_TAU + 1); ROW(g_out, 30 + j) = KEEP(QR_PB_OUT_TAU + 2);      // the motor's torque; the stops' are g_bout's
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

}  // namespace qrgpu
