// What qr_plant_step_body_kernel (qr_plant_body_kernel.hip) has beyond the terrain plant: the sixteen contact points of a robot -- per leg the
// foot, the knee and the two trunk corners on the leg's side -- the joint-limit law, and a leg's inward pass that takes a force at the knee.
// fp64.  Every function is __host__ __device__: the same text compiles for a CPU check against tests/body_contact_ref.py
// (tests/stubs/plant_body_host.hip).  include/qrgpu.h states the law (qrgpu_plant_step_body_batch).
#pragma once
#include "qr_plant_math.h"

namespace qrgpu {
namespace plant {

// A lane's points, in the order it takes them.
#define QR_PB_FOOT   0
#define QR_PB_KNEE   1
#define QR_PB_BOTTOM 2      // trunk corner (sx hx, sy hy, -hz)
#define QR_PB_TOP    3      // trunk corner (sx hx, sy hy, +hz)
#define QR_PB_POINTS 4

// The stop of a joint: one-sided, continuous in the state, zero inside [lo, hi].
QR_HD real limit_torque(real q, real qd, real lo, real hi, real k, real a)
{
    if (q > hi) return -fmax(0.0, k * (q - hi) * (1.0 + a * qd));
    if (q < lo) return fmax(0.0, k * (lo - q) * (1.0 - a * qd));
    return 0.0;
}

// leg_start that also hands out the knee point -- the origin of the knee link's frame -- and its velocity, base frame.
QR_HD void leg_start_body(const WbcConst &K, int leg, const Stash &st, real q0, real q1, real q2, real qd0, real qd1, real qd2, sv6 v0, v3 &foot, v3 &foot_vel,
                          v3 &knee, v3 &knee_vel)
{
    const real s0 = sin(q0), c0 = cos(q0), s1 = sin(q1), c1 = cos(q1), s2 = sin(q2), c2 = cos(q2);
    st.at(QR_PL_ST_TRIG) = s0; st.at(QR_PL_ST_TRIG + 1) = c0; st.at(QR_PL_ST_TRIG + 2) = s1; st.at(QR_PL_ST_TRIG + 3) = c1;
    st.at(QR_PL_ST_TRIG + 4) = s2; st.at(QR_PL_ST_TRIG + 5) = c2;
    const Joint X1 = leg_joint(K, leg, 0, s0, c0), X2 = leg_joint(K, leg, 1, s1, c1), X3 = leg_joint(K, leg, 2, s2, c2);
    sv6 v1 = to_child(X1, v0); v1.a.x += qd0;
    sv6 v2 = to_child(X2, v1); v2.a.y += qd1;
    sv6 v3s = to_child(X3, v2); v3s.a.y += qd2;
    st.put(QR_PL_ST_V, v0); st.put(QR_PL_ST_V + 6, v1); st.put(QR_PL_ST_V + 12, v2); st.put(QR_PL_ST_V + 18, v3s);
    const v3 pf = leg_foot_in_knee(K, leg);
    foot = X1.r + mul(X1.R, X2.r + mul(X2.R, X3.r + mul(X3.R, pf)));
    foot_vel = mul(X1.R, mul(X2.R, mul(X3.R, v3s.l + cross(v3s.a, pf))));
    knee = X1.r + mul(X1.R, X2.r + mul(X2.R, X3.r));
    knee_vel = mul(X1.R, mul(X2.R, mul(X3.R, v3s.l)));
}

// The trunk corner on leg's side, base frame: trunk_center + (sx hx, sy hy, -+hz) with leg_joint's signs.
QR_HD v3 trunk_corner(const qrgpu_plant_body_desc &B, int leg, bool top)
{
    const real sx = leg < 2 ? 1.0 : -1.0, sy = (leg & 1) ? 1.0 : -1.0;
    return mk((real)B.trunk_center[0] + sx * (real)B.trunk_half[0], (real)B.trunk_center[1] + sy * (real)B.trunk_half[1],
              (real)B.trunk_center[2] + (top ? (real)B.trunk_half[2] : -(real)B.trunk_half[2]));
}

// Point k of a lane: position and velocity in the base frame.  A corner moves with the base: v + omega x c.
QR_HD void lane_point(const qrgpu_plant_body_desc &B, int leg, int k, sv6 v0, v3 foot, v3 foot_vel, v3 knee, v3 knee_vel, v3 &p, v3 &v)
{
    if (k == QR_PB_FOOT) { p = foot; v = foot_vel; return; }
    if (k == QR_PB_KNEE) { p = knee; v = knee_vel; return; }
    p = trunk_corner(B, leg, k == QR_PB_TOP);
    v = v0.l + cross(v0.a, p);
}

// The wrench on the base of a force f_b at the corner c, both in the base frame: (moment about the base origin; force).
QR_HD sv6 corner_wrench(v3 c, v3 f_b) { sv6 w; w.a = cross(c, f_b); w.l = f_b; return w; }

// leg_inward with a second external force on the knee link: fk_b, base frame, acting at the link's origin -- in link coordinates a pure force, no
// moment.  With fk_b = 0 it is leg_inward.
QR_HD void leg_inward_body(const WbcConst &K, int leg, const Stash &st, real qd0, real qd1, real qd2, real tau0, real tau1, real tau2, v3 f_b, v3 fk_b, abi &IA,
                           sv6 &pA)
{
    const v3 zero = mk(0, 0, 0);
#pragma unroll
    for (int i = 0; i < 6; ++i) { IA.I[i] = 0; IA.M[i] = 0; }
    IA.h0 = IA.h1 = IA.h2 = zero;
    pA.a = pA.l = zero;
    // both external forces act on the knee link: into its frame
    v3 f3 = f_b, fk3 = fk_b;
#pragma unroll
    for (int jnt = 0; jnt < 3; ++jnt) {
        const frame3 Rj = leg_joint(K, leg, jnt, st.at(QR_PL_ST_TRIG + 2 * jnt), st.at(QR_PL_ST_TRIG + 2 * jnt + 1)).R;
        f3 = mulT(Rj, f3); fk3 = mulT(Rj, fk3);
    }
    sv6 fx; fx.a = cross(leg_foot_in_knee(K, leg), f3); fx.l = f3 + fk3;
#pragma unroll 1
    for (int jnt = 2; jnt >= 0; --jnt) {
        const Joint X = leg_joint(K, leg, jnt, st.at(QR_PL_ST_TRIG + 2 * jnt), st.at(QR_PL_ST_TRIG + 2 * jnt + 1));
        v3 axr, rot;
        leg_rotor(leg, jnt, axr, rot);
        const real qd = jnt == 0 ? qd0 : jnt == 1 ? qd1 : qd2, tau = jnt == 0 ? tau0 : jnt == 1 ? tau1 : tau2;
        LegJoint J;
        leg_joint_inward(J, X, rbi_load(leg_link(K, leg, jnt)), leg_axis(jnt), st.get(QR_PL_ST_V + 6 * (jnt + 1)), st.get(QR_PL_ST_V + 6 * jnt), axr, rot, K.k_rot, qd, tau,
                         fx, IA, pA);
        fx.a = fx.l = zero;
        st.put(QR_PL_ST_J + 14 * jnt, J.c); st.put(QR_PL_ST_J + 14 * jnt + 6, J.Ut);
        st.at(QR_PL_ST_J + 14 * jnt + 12) = J.u; st.at(QR_PL_ST_J + 14 * jnt + 13) = J.inv_d;
    }
}

}  // namespace plant
}  // namespace qrgpu
