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
// What the tick has in common with the terrain kernel's -- state in, command read, motor law, integrator, state check, push read, plant_out,
// terrain_out -- is the named pieces of qr_plant_quad.h; what stands in this kernel is its own (the stops, the four-point loop,
// forward_dynamics_body, the second LDS column, g_bout, the hit flags) and the state write and the mpc_state / est_in writes, which are the
// terrain kernel's text: called as pieces they measured 120 ns a launch over the kernel as it was.
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
    real qw, qx, qy, qz, q0, q1, q2, qd0, qd1, qd2;
    v3 pos;
    sv6 v0;
    state_in(g_state, N, i, j, w.flags, qw, qx, qy, qz, pos, v0, q0, q1, q2, qd0, qd1, qd2);
    const real h = (real)P.dt / (real)P.substeps;
    const real ck = P.contact_k, ca = P.contact_a, mu = P.mu, v_eps = P.v_eps, ground_z = P.ground_z, tau_max = P.tau_max;
    const float *field = field_in(T, g_height, g_field, i, w.flags);
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
        // The motor command of this leg's joints and the push are read again at every sub-step, through pointers the compiler cannot see through:
        // held in registers across the inward pass, their 21 doubles were what spilled.  They are inputs, not the state.
        const float *cmd = g_cmd, *push = g_push;
        asm volatile("" : "+s"(cmd), "+s"(push));
        real tau0, tau1, tau2;
        motor_law(cmd_in(cmd, N, i, j), q0, q1, q2, qd0, qd1, qd2, tau_max, tau0, tau1, tau2);
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
        v3 push_f, push_m;
        push_in(push, N, i, push_f, push_m);
        sv6 wrench; wrench.a = mulT(R, push_m); wrench.l = mulT(R, push_f);
        wrench = wrench + quad_sum(corners);
        forward_dynamics_body(K, leg, st, R, v0, qd0, qd1, qd2, tau0, tau1, tau2, f_b, fk_b, wrench, afb, qdd0, qdd1, qdd2);
        acc = accelerometer(R, v0, afb);
        integrate(R, h, afb, qdd0, qdd1, qdd2, qw, qx, qy, qz, pos, v0, q0, q1, q2, qd0, qd1, qd2);
    }
    state_check(w.flags, qw, qx, qy, qz, pos, v0, q0, q1, q2, qd0, qd1, qd2);
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
    ground_out(g_tout, N, i, leg, field, T, ground_z, foot_w);
    // the foot's force and the motor's torque come from the column; the stops' torques are g_bout's
    plant_out(g_out, N, i, leg, KEEP(QR_PB_OUT_FORCE), KEEP(QR_PB_OUT_FORCE + 1), KEEP(QR_PB_OUT_FORCE + 2), foot_w, contact, KEEP(QR_PB_OUT_TAU), KEEP(QR_PB_OUT_TAU + 1),
              KEEP(QR_PB_OUT_TAU + 2), afb, qdd0, qdd1, qdd2);
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
