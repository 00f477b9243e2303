// What is the plant kernels' own (qr_plant_kernel.hip) on top of the shared algebra of qr_rigid_body.h: the column-vector rotation, articulated-body
// inertias, the articulated-body forward dynamics of one leg and the contact law.  fp64 throughout.  Every function is __host__ __device__: the
// same text compiles for a CPU check against the float64 mechanics of tests/rigid_body_ref.py.
//
// Coordinates: Featherstone's link coordinates.  A link's frame sits at its joint, so a link's inertia is a constant and its joint axis a unit
// vector; what passes between a link and its parent goes through the joint's transform (a rotation about a coordinate axis and a constant
// offset).  A rotor is fixed in its joint's PARENT and its inertia is isotropic, so it is handled in the parent's coordinates, where its place,
// axis and inertia are constants too.  The recursion is FloatingBaseModel::runABA (QS/dynamics/floating_base_model.cpp:876-947) with its rotor
// terms (:895-900, :914-922).
//   motion vector (a; l): angular velocity; velocity of the body-fixed point that passes the frame's origin
//   force vector  (a; l): moment about the frame's origin; force
#pragma once
#include "qr_device_types.h"
#include "qr_rigid_body.h"

namespace qrgpu {
namespace plant {

// Rotor data BuildDynamicModel gives every robot (QS/robots/qr_robot_a1_sim.cpp:184-189, :243) beyond what WbcConst carries: float literals, widened.
#define QR_PL_ROTOR_MASS   ((double)1e-8f)
#define QR_PL_ABAD_ROTOR_X ((double)0.14f)
#define QR_PL_ABAD_ROTOR_Y ((double)0.047f)
#define QR_PL_HIP_ROTOR_Y  ((double)0.04f)
#define QR_PL_GRAVITY      9.81

// Rotation matrix as three column vectors c0 c1 c2 (a frame's axes in its parent's coordinates); a product with a vector is summed
// b.x c0 + (b.y c1 + b.z c2).  (The WBC chains' xform3 is row-major and sums (a0 b0 + a1 b1) + a2 b2: the two are kept apart.)
struct frame3 { v3 c0, c1, c2; };
QR_HD v3 mul(const frame3 &R, v3 b) { return b.x * R.c0 + (b.y * R.c1 + b.z * R.c2); }
QR_HD v3 mulT(const frame3 &R, v3 b) { return mk(dot(R.c0, b), dot(R.c1, b), dot(R.c2, b)); }
QR_HD frame3 mul(const frame3 &A, const frame3 &B) { frame3 C; C.c0 = mul(A, B.c0); C.c1 = mul(A, B.c1); C.c2 = mul(A, B.c2); return C; }
QR_HD frame3 rot_x(real s, real c) { frame3 R; R.c0 = mk(1, 0, 0); R.c1 = mk(0, c, s); R.c2 = mk(0, -s, c); return R; }
QR_HD frame3 rot_y(real s, real c) { frame3 R; R.c0 = mk(c, 0, -s); R.c1 = mk(0, 1, 0); R.c2 = mk(s, 0, c); return R; }
// body-to-world rotation of a unit quaternion (w, x, y, z)
QR_HD frame3 quat_to_rot(real w, real x, real y, real z)
{
    frame3 R;
    R.c0 = mk(1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y));
    R.c1 = mk(2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x));
    R.c2 = mk(2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y));
    return R;
}

// the axis `ax` through the point `p` as a motion vector
QR_HD sv6 axis_at(v3 ax, v3 p) { sv6 o; o.a = ax; o.l = cross(p, ax); return o; }

// s (a b^T + b a^T) added to a symmetric matrix
QR_HD void sym_add_outer2(real I[6], real s, v3 a, v3 b)
{
    I[0] += s * 2 * a.x * b.x; I[1] += s * 2 * a.y * b.y; I[2] += s * 2 * a.z * b.z;
    I[3] += s * (a.x * b.y + a.y * b.x); I[4] += s * (a.x * b.z + a.z * b.x); I[5] += s * (a.y * b.z + a.z * b.y);
}
// A rotor: mass m at the point c with the isotropic inertia k 1 (the same in every frame).
QR_HD rbi rbi_rotor(real m, real k, v3 c)
{
    rbi o; o.m = m; o.h = m * c;
    const real cc = dot(c, c);
    o.I[0] = k + m * (cc - c.x * c.x); o.I[1] = k + m * (cc - c.y * c.y); o.I[2] = k + m * (cc - c.z * c.z);
    o.I[3] = -m * c.x * c.y; o.I[4] = -m * c.x * c.z; o.I[5] = -m * c.y * c.z;
    return o;
}

// Articulated-body inertia [[I, H], [H^T, M]]: I, M symmetric (xx yy zz xy xz yz), H full with columns h0 h1 h2.
struct abi { real I[6]; v3 h0, h1, h2; real M[6]; };
QR_HD abi abi_of(const rbi &a)
{
    abi o;
#pragma unroll
    for (int i = 0; i < 6; ++i) { o.I[i] = a.I[i]; o.M[i] = 0; }
    o.M[0] = o.M[1] = o.M[2] = a.m;
    // [h]x: columns h x e_k
    o.h0 = mk(0, a.h.z, -a.h.y); o.h1 = mk(-a.h.z, 0, a.h.x); o.h2 = mk(a.h.y, -a.h.x, 0);
    return o;
}
QR_HD abi operator+(const abi &a, const abi &b)
{
    abi o;
#pragma unroll
    for (int i = 0; i < 6; ++i) { o.I[i] = a.I[i] + b.I[i]; o.M[i] = a.M[i] + b.M[i]; }
    o.h0 = a.h0 + b.h0; o.h1 = a.h1 + b.h1; o.h2 = a.h2 + b.h2;
    return o;
}
QR_HD sv6 abi_mul(const abi &A, sv6 v)
{
    sv6 o;
    o.a = sym_mul(A.I, v.a) + (v.l.x * A.h0 + (v.l.y * A.h1 + v.l.z * A.h2));
    o.l = mk(dot(A.h0, v.a), dot(A.h1, v.a), dot(A.h2, v.a)) + sym_mul(A.M, v.l);
    return o;
}
// A - u u^T / d
QR_HD abi abi_downdate(const abi &A, sv6 u, real inv_d)
{
    abi o = A;
    sym_add_outer2(o.I, -0.5 * inv_d, u.a, u.a);
    sym_add_outer2(o.M, -0.5 * inv_d, u.l, u.l);
    o.h0 = o.h0 - (inv_d * u.l.x) * u.a; o.h1 = o.h1 - (inv_d * u.l.y) * u.a; o.h2 = o.h2 - (inv_d * u.l.z) * u.a;
    return o;
}

// x = A^-1 b for the base's symmetric positive definite 6 x 6 articulated inertia: Cholesky, fully unrolled (constant indices only).
QR_HD sv6 abi_solve(const abi &A, sv6 b)
{
    real a[6][6], x[6] = {b.a.x, b.a.y, b.a.z, b.l.x, b.l.y, b.l.z};
    a[0][0] = A.I[0]; a[1][1] = A.I[1]; a[2][2] = A.I[2]; a[1][0] = A.I[3]; a[2][0] = A.I[4]; a[2][1] = A.I[5];
    a[3][0] = A.h0.x; a[3][1] = A.h0.y; a[3][2] = A.h0.z; a[4][0] = A.h1.x; a[4][1] = A.h1.y; a[4][2] = A.h1.z; a[5][0] = A.h2.x; a[5][1] = A.h2.y; a[5][2] = A.h2.z;
    a[3][3] = A.M[0]; a[4][4] = A.M[1]; a[5][5] = A.M[2]; a[4][3] = A.M[3]; a[5][3] = A.M[4]; a[5][4] = A.M[5];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        real s = a[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= a[j][k] * a[j][k];
        const real ljj = sqrt(s), inv = 1.0 / ljj;
        a[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            real t = a[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= a[i][k] * a[j][k];
            a[i][j] = t * inv;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        real t = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= a[i][k] * x[k];
        x[i] = t / a[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        real t = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) t -= a[k][i] * x[k];
        x[i] = t / a[i][i];
    }
    sv6 o; o.a = mk(x[0], x[1], x[2]); o.l = mk(x[3], x[4], x[5]);
    return o;
}

// R A R^T of a full 3 x 3 matrix given by its columns.
QR_HD frame3 rot_conj(const frame3 &R, const frame3 &A)
{
    const v3 b0 = mul(R, A.c0), b1 = mul(R, A.c1), b2 = mul(R, A.c2);
    frame3 o;
    o.c0 = R.c0.x * b0 + (R.c1.x * b1 + R.c2.x * b2);
    o.c1 = R.c0.y * b0 + (R.c1.y * b1 + R.c2.y * b2);
    o.c2 = R.c0.z * b0 + (R.c1.z * b1 + R.c2.z * b2);
    return o;
}
QR_HD frame3 sym_full(const real I[6]) { frame3 o; o.c0 = mk(I[0], I[3], I[4]); o.c1 = mk(I[3], I[1], I[5]); o.c2 = mk(I[4], I[5], I[2]); return o; }
QR_HD void full_sym(const frame3 &A, real I[6])
{
    I[0] = A.c0.x; I[1] = A.c1.y; I[2] = A.c2.z; I[3] = 0.5 * (A.c1.x + A.c0.y); I[4] = 0.5 * (A.c2.x + A.c0.z); I[5] = 0.5 * (A.c2.y + A.c1.z);
}

// A joint's transform: the child frame sits at r in the parent and is turned by R (child -> parent).
struct Joint { frame3 R; v3 r; };
QR_HD sv6 to_child(const Joint &X, sv6 v) { sv6 o; o.a = mulT(X.R, v.a); o.l = mulT(X.R, v.l - cross(X.r, v.a)); return o; }      // motion vectors
QR_HD sv6 to_parent(const Joint &X, sv6 f) { sv6 o; o.l = mul(X.R, f.l); o.a = mul(X.R, f.a) + cross(X.r, o.l); return o; }       // force vectors
// X^T A X of an articulated inertia: turned by R, then moved by r:  M' = R M R^T,  H_p = R H R^T + [r]x M',  I_p = R I R^T - (R H R^T) [r]x + [r]x H_p^T
QR_HD abi to_parent(const Joint &X, const abi &A)
{
    const frame3 I = rot_conj(X.R, sym_full(A.I)), M = rot_conj(X.R, sym_full(A.M));
    frame3 H; H.c0 = A.h0; H.c1 = A.h1; H.c2 = A.h2;
    H = rot_conj(X.R, H);
    const v3 r = X.r;
    frame3 Hp; Hp.c0 = H.c0 + cross(r, M.c0); Hp.c1 = H.c1 + cross(r, M.c1); Hp.c2 = H.c2 + cross(r, M.c2);
    // H [r]x: column k = H (r x e_k);   [r]x Hp^T: column k = r x (row k of Hp)
    frame3 Ip;
    Ip.c0 = (I.c0 - mul(H, mk(0, r.z, -r.y))) + cross(r, mk(Hp.c0.x, Hp.c1.x, Hp.c2.x));
    Ip.c1 = (I.c1 - mul(H, mk(-r.z, 0, r.x))) + cross(r, mk(Hp.c0.y, Hp.c1.y, Hp.c2.y));
    Ip.c2 = (I.c2 - mul(H, mk(r.y, -r.x, 0))) + cross(r, mk(Hp.c0.z, Hp.c1.z, Hp.c2.z));
    abi o;
    full_sym(Ip, o.I); full_sym(M, o.M);
    o.h0 = Hp.c0; o.h1 = Hp.c1; o.h2 = Hp.c2;
    return o;
}

// ---- one leg ------------------------------------------------------------------------------------------------------------------------------
// The recursion runs as a LOOP over the three joints (abad about x, hip and knee about y), not unrolled: written out, the three joints' work is
// one basic block whose live values need more than the 512 registers of a lane, and the compiler spills to scratch.  What lives from one joint
// to the next, and from the inward pass to the outward one, is kept in a per-lane store -- on the device a column of LDS, on the host an
// array -- and a joint's constants are selected by its number.
struct Stash {
    real *p; int stride;
    QR_HD real &at(int slot) const { return p[slot * stride]; }
    QR_HD void put(int slot, sv6 v) const { at(slot) = v.a.x; at(slot + 1) = v.a.y; at(slot + 2) = v.a.z; at(slot + 3) = v.l.x; at(slot + 4) = v.l.y; at(slot + 5) = v.l.z; }
    QR_HD sv6 get(int slot) const { sv6 v; v.a = mk(at(slot), at(slot + 1), at(slot + 2)); v.l = mk(at(slot + 3), at(slot + 4), at(slot + 5)); return v; }
};
#define QR_PL_ST_TRIG  0      // sin, cos of joint j at 2 j
#define QR_PL_ST_V     6      // velocity of the base (0) and of link j (1 + j), each in its own coordinates, at 6 k
#define QR_PL_ST_J     30     // joint j at 14 j: c [6] (link coordinates), Ut [6] (parent coordinates), u, 1 / d
#define QR_PL_ST_SLOTS 72

QR_HD Joint leg_joint(const WbcConst &K, int leg, int jnt, real s, real c)
{
    const real sx = leg < 2 ? 1.0 : -1.0, sy = (leg & 1) ? 1.0 : -1.0;
    const bool x = jnt == 0;
    Joint X;
    X.R.c0 = mk(x ? 1.0 : c, 0, x ? 0.0 : -s); X.R.c1 = mk(0, x ? c : 1.0, x ? s : 0.0); X.R.c2 = mk(x ? 0.0 : s, x ? -s : 0.0, c);      // rot_x / rot_y
    X.r = jnt == 0 ? mk(sx * K.abad_loc[0], sy * K.abad_loc[1], K.abad_loc[2]) : jnt == 1 ? mk(0, sy * K.hip_l, 0) : mk(0, 0, -K.upper_l);
    return X;
}
QR_HD v3 leg_axis(int jnt) { return jnt == 0 ? mk(1, 0, 0) : mk(0, 1, 0); }
// A joint's rotor in the joint's parent: its axis is the joint's, but the hip rotor's frame is Rz(pi) of its parent (:300-302), so it turns about
// the parent's -y; the knee rotor sits at the hip link's origin.
QR_HD void leg_rotor(int leg, int jnt, v3 &axis, v3 &at)
{
    const real sx = leg < 2 ? 1.0 : -1.0, sy = (leg & 1) ? 1.0 : -1.0;
    axis = jnt == 0 ? mk(1, 0, 0) : jnt == 1 ? mk(0, -1, 0) : mk(0, 1, 0);
    at = jnt == 0 ? mk(sx * QR_PL_ABAD_ROTOR_X, sy * QR_PL_ABAD_ROTOR_Y, 0) : jnt == 1 ? mk(0, sy * QR_PL_HIP_ROTOR_Y, 0) : mk(0, 0, 0);
}
QR_HD const real *leg_link(const WbcConst &K, int leg, int jnt)
{
    const int side = leg & 1;                                               // 0: right legs, the mirrored bodies; the knee link is mirrored on no leg
    return K.rb[jnt == 0 ? QR_RB_ABAD + side : jnt == 1 ? QR_RB_HIP + side : QR_RB_KNEE];
}
QR_HD v3 leg_foot_in_knee(const WbcConst &K, int leg) { return mk(0, (leg & 1) ? -K.foot_y : K.foot_y, -K.lower_l); }      // +y on the mirrored (right) legs

// Start of a leg's evaluation: the joints' sines and cosines and the links' velocities go to the store.  -> the foot point's position and
// velocity in the base frame.
QR_HD void leg_start(const WbcConst &K, int leg, const Stash &st, real q0, real q1, real q2, real qd0, real qd1, real qd2, sv6 v0, v3 &foot, v3 &foot_vel)
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
}

// What the outward pass of a leg needs from its inward pass, per joint: c in the link's coordinates, Ut in the parent's.
struct LegJoint { sv6 c, Ut; real u, inv_d; };

// One joint of the inward pass.  In: IA, pA = what the link's children handed to it (zero at the knee), in the link's coordinates; I = the link's
// inertia, v = its velocity, ax = its joint axis, X = its joint; v_parent = the parent's velocity, axr / rot = the rotor's axis and place in the parent;
// f_ext = the external force on the link.  Out: IA, pA = what the link and its rotor hand to the parent, in the parent's coordinates.
QR_HD void leg_joint_inward(LegJoint &J, const Joint &X, const rbi &I, v3 ax, sv6 v, sv6 v_parent, v3 axr, v3 rot, real k_rot, real qd, real tau, sv6 f_ext,
                            abi &IA, sv6 &pA)
{
    sv6 S; S.a = ax; S.l = mk(0, 0, 0);
    const sv6 Srot = axis_at(axr, rot);
    const sv6 vj = qd * S, vjr = qd * Srot;
    J.c = crm(v, vj);
    const sv6 vr = v_parent + vjr, crot = crm(vr, vjr);
    const rbi Irot = rbi_rotor(QR_PL_ROTOR_MASS, k_rot, rot);
    const abi IAl = abi_of(I) + IA;
    const sv6 pAl = (crf(v, rbi_mul(I, v)) + pA) + (-1.0) * f_ext;
    const sv6 pArot = crf(vr, rbi_mul(Irot, vr));
    const sv6 U = abi_mul(IAl, S), Urot = rbi_mul(Irot, Srot);
    J.inv_d = 1.0 / (dot(S, U) + dot(Srot, Urot));
    J.u = tau - dot(S, pAl) - dot(Srot, pArot) - dot(U, J.c) - dot(Urot, crot);
    J.Ut = to_parent(X, U) + Urot;
    IA = abi_downdate(to_parent(X, IAl) + abi_of(Irot), J.Ut, J.inv_d);
    pA = (to_parent(X, pAl + abi_mul(IAl, J.c)) + (pArot + rbi_mul(Irot, crot))) + (J.u * J.inv_d) * J.Ut;
}

// Inward pass of one leg, after leg_start: -> IA, pA = what it adds to the base's articulated inertia and bias force, base coordinates.
// f_b: the force on the foot point, base frame.
QR_HD void leg_inward(const WbcConst &K, int leg, const Stash &st, real qd0, real qd1, real qd2, real tau0, real tau1, real tau2, v3 f_b, abi &IA, sv6 &pA)
{
    const v3 zero = mk(0, 0, 0);
#pragma unroll
    for (int i = 0; i < 6; ++i) { IA.I[i] = 0; IA.M[i] = 0; }
    IA.h0 = IA.h1 = IA.h2 = zero;
    pA.a = pA.l = zero;
    // the external force acts on the knee link: into its frame
    v3 f3 = f_b;
#pragma unroll
    for (int jnt = 0; jnt < 3; ++jnt) f3 = mulT(leg_joint(K, leg, jnt, st.at(QR_PL_ST_TRIG + 2 * jnt), st.at(QR_PL_ST_TRIG + 2 * jnt + 1)).R, f3);
    sv6 fx; fx.a = cross(leg_foot_in_knee(K, leg), f3); fx.l = f3;
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

// Outward pass: the leg's three joint accelerations from the base's spatial acceleration (gravity's fictitious part included).
QR_HD void leg_outward(const WbcConst &K, int leg, const Stash &st, sv6 a, real &qdd0, real &qdd1, real &qdd2)
{
#pragma unroll 1
    for (int jnt = 0; jnt < 3; ++jnt) {
        const int b = QR_PL_ST_J + 14 * jnt;
        const real qdd = (st.at(b + 12) - dot(st.get(b + 6), a)) * st.at(b + 13);
        if (jnt == 2) { qdd2 = qdd; break; }
        a = to_child(leg_joint(K, leg, jnt, st.at(QR_PL_ST_TRIG + 2 * jnt), st.at(QR_PL_ST_TRIG + 2 * jnt + 1)), a) + st.get(b);
        if (jnt == 0) { a.a.x += qdd; qdd0 = qdd; } else { a.a.y += qdd; qdd1 = qdd; }
    }
}

// The base: its own inertia and velocity-product force, to which the four legs' contributions are added.
QR_HD void base_start(const WbcConst &K, sv6 v0, abi &IA, sv6 &pA)
{
    const rbi I0 = rbi_load(K.rb[QR_RB_BASE]);
    IA = abi_of(I0);
    pA = crf(v0, rbi_mul(I0, v0));
}
// afb = d/dt of the components of (omega_body, v_body); a0 = afb + gravity's fictitious acceleration, what the legs' outward pass takes.
QR_HD void base_solve(const abi &IA, sv6 pA, const frame3 &R, sv6 &afb, sv6 &a0)
{
    sv6 ag; ag.a = mk(0, 0, 0); ag.l = mulT(R, mk(0, 0, QR_PL_GRAVITY));
    const sv6 rhs = -1.0 * (pA + abi_mul(IA, ag));
    afb = abi_solve(IA, rhs);
    a0 = ag + afb;
}

// The contact law (ours; the reference leaves the ground to its simulator): a flat ground at ground_z, a spring-damper normal force that never
// pulls, and friction regularised at v_eps.  Both are continuous in the state.  p, v: the foot point's world position and velocity.
QR_HD v3 contact_force(real ground_z, real k, real a, real mu, real v_eps, v3 p, v3 v, real &fn)
{
    const real depth = ground_z - p.z;
    fn = 0.0;
    if (depth > 0.0) fn = fmax(0.0, k * depth * (1.0 - a * v.z));
    const real s = -mu * fn / sqrt(v.x * v.x + v.y * v.y + v_eps * v_eps);
    return mk(s * v.x, s * v.y, fn);
}

}  // namespace plant
}  // namespace qrgpu
