// The WBC kernel's rigid-body chains (K8-K10) as functions: per leg the link frames, the contact Jacobian, composite inertias, mass-matrix
// columns and gravity (what wave 0 of qr_wbc_kernel walks), velocities, bias accelerations, foot position / velocity, Jcdqd and Coriolis (wave 1),
// and the two base blocks that collect the legs' contributions.  They take the type's constants, the state, the joints' sines and cosines and
// output pointers -- on the device the kernel's LDS arrays -- and know nothing of lanes, waves or fences: the kernel decides who calls what and
// fences in between; tests/stubs/wbc_rigid_body_host.hip calls them from plain loops on the CPU.  fp64 on the fp32 inputs.
// Rotor bodies: see the head of qr_wbc_kernel.hip.
#pragma once
#include "qr_device_types.h"
#include "qr_rigid_body.h"

namespace qrgpu {

// Coordinate transform, row-major m[row][col]; a product's entry is summed (a0 b0 + a1 b1) + a2 b2.  (The plant's frame3 holds three column
// vectors and sums b.x c0 + (b.y c1 + b.z c2): the two are kept apart.)
struct xform3 { real m[3][3]; };
QR_HD v3 mul(const xform3 &A, v3 b)
{
    return mk(A.m[0][0] * b.x + A.m[0][1] * b.y + A.m[0][2] * b.z, A.m[1][0] * b.x + A.m[1][1] * b.y + A.m[1][2] * b.z,
              A.m[2][0] * b.x + A.m[2][1] * b.y + A.m[2][2] * b.z);
}
QR_HD v3 mulT(const xform3 &A, v3 b)
{
    return mk(A.m[0][0] * b.x + A.m[1][0] * b.y + A.m[2][0] * b.z, A.m[0][1] * b.x + A.m[1][1] * b.y + A.m[2][1] * b.z,
              A.m[0][2] * b.x + A.m[1][2] * b.y + A.m[2][2] * b.z);
}
QR_HD xform3 mul(const xform3 &A, const xform3 &B)
{
    xform3 C;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C.m[i][j] = A.m[i][0] * B.m[0][j] + A.m[i][1] * B.m[1][j] + A.m[i][2] * B.m[2][j];
    return C;
}
QR_HD xform3 transpose(const xform3 &A)
{
    xform3 C;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C.m[i][j] = A.m[j][i];
    return C;
}
// coordinateRotation (QI/utils/qr_se3.h:72-89): the coordinate-transform (transposed) matrix.
QR_HD xform3 coord_rot_sc(int axis, real s, real c)
{
    xform3 R;
    if (axis == 0)      { R = {{{1, 0, 0}, {0, c, s}, {0, -s, c}}}; }
    else if (axis == 1) { R = {{{c, 0, -s}, {0, 1, 0}, {s, 0, c}}}; }
    else                { R = {{{c, s, 0}, {-s, c, 0}, {0, 0, 1}}}; }
    return R;
}
// quaternionToRotationMatrix (:186-203): world -> body.
QR_HD xform3 quat_to_rot_wb(const real *q)
{
    const real e0 = q[0], e1 = q[1], e2 = q[2], e3 = q[3];
    xform3 R;
    R.m[0][0] = 1 - 2 * (e2 * e2 + e3 * e3); R.m[1][0] = 2 * (e1 * e2 - e0 * e3); R.m[2][0] = 2 * (e1 * e3 + e0 * e2);
    R.m[0][1] = 2 * (e1 * e2 + e0 * e3); R.m[1][1] = 1 - 2 * (e1 * e1 + e3 * e3); R.m[2][1] = 2 * (e2 * e3 - e0 * e1);
    R.m[0][2] = 2 * (e1 * e3 - e0 * e2); R.m[1][2] = 2 * (e2 * e3 + e0 * e1); R.m[2][2] = 1 - 2 * (e1 * e1 + e2 * e2);
    return R;
}
// Express a child-frame inertia in the parent frame: X^T I X with X = (E, r)  (createSXform(E, r)).
QR_HD rbi rbi_to_parent(const rbi &a, const xform3 &E, v3 r)
{
    rbi o;
    o.m = a.m;
    const v3 hr = mulT(E, a.h);                    // E^T h
    o.h = hr + a.m * r;
    // Ibar' = E^T Ibar E - [r]x[hr]x - [h']x[r]x
    xform3 I; I.m[0][0] = a.I[0]; I.m[1][1] = a.I[1]; I.m[2][2] = a.I[2];
    I.m[0][1] = I.m[1][0] = a.I[3]; I.m[0][2] = I.m[2][0] = a.I[4]; I.m[1][2] = I.m[2][1] = a.I[5];
    xform3 Ir = mul(transpose(E), mul(I, E));
    // -[a]x[b]x = (a.b) 1 - b a^T
    auto add_outer = [&](v3 a_, v3 b_) {
        const real ab = dot(a_, b_);
        const real av[3] = {a_.x, a_.y, a_.z}, bv[3] = {b_.x, b_.y, b_.z};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Ir.m[i][j] += (i == j ? ab : 0.0) - bv[i] * av[j];
    };
    add_outer(r, hr);
    add_outer(o.h, r);
    o.I[0] = Ir.m[0][0]; o.I[1] = Ir.m[1][1]; o.I[2] = Ir.m[2][2];
    o.I[3] = 0.5 * (Ir.m[0][1] + Ir.m[1][0]); o.I[4] = 0.5 * (Ir.m[0][2] + Ir.m[2][0]); o.I[5] = 0.5 * (Ir.m[1][2] + Ir.m[2][1]);
    return o;
}
QR_HD sv6 xmotion(const xform3 &E, v3 r, sv6 v) { sv6 o; o.a = mul(E, v.a); o.l = mul(E, v.l - cross(r, v.a)); return o; }   // X v
QR_HD sv6 xforceT(const xform3 &E, v3 r, sv6 f) { sv6 o; o.l = mulT(E, f.l); o.a = mulT(E, f.a) + cross(r, o.l); return o; }   // X^T f

// Layouts: A 18 x 18 (zeroed by the caller), JcA 4 x (3 x 18) (zeroed by the caller), Gv / Cv 18, Jcd / pGC / vGC 4 x 3, legB 4 x 16: what a leg
// hands to the base (its composite inertia seen from the base at 0-9: wave 0; its force at 10-15: wave 1); sS / sC: sin / cos of the twelve joint angles.
struct LegFrames { v3 r_a, r_h, r_k, loc; xform3 Ea, Eh, Ek, Eabs_a, Eabs_h, Eabs_k; };
QR_HD LegFrames leg_frames(const WbcConst &K, const xform3 &Rwb, const real *sS, const real *sC, int leg)
{
    LegFrames F;
    const int side = leg & 1;           // side 0: right (legs 0,2; sideSign<0), 1: left
    const real sx = (leg < 2) ? 1.0 : -1.0, sy = side ? 1.0 : -1.0;
    F.r_a = mk(sx * K.abad_loc[0], sy * K.abad_loc[1], K.abad_loc[2]);
    F.r_h = mk(0.0, sy * K.hip_l, 0.0);
    F.r_k = mk(0.0, 0.0, -K.upper_l);
    F.loc = mk(0.0, side ? -K.foot_y : K.foot_y, -K.lower_l);
    F.Ea = coord_rot_sc(0, sS[3 * leg], sC[3 * leg]); F.Eh = coord_rot_sc(1, sS[3 * leg + 1], sC[3 * leg + 1]); F.Ek = coord_rot_sc(1, sS[3 * leg + 2], sC[3 * leg + 2]);
    // absolute rotations (world -> link)
    F.Eabs_a = mul(F.Ea, Rwb); F.Eabs_h = mul(F.Eh, F.Eabs_a); F.Eabs_k = mul(F.Ek, F.Eabs_h);
    return F;
}

// One leg of the mass-matrix side: contact Jacobian -> JcA, composite inertias -> legB[0:10], the leg's columns of H -> A, gravity -> Gv.
QR_HD void wbc_leg_inertia_chain(const WbcConst &K, const xform3 &Rwb, const real *sS, const real *sC, int leg, real *A, real *JcA, real *Gv, real *legB)
{
    const v3 ex = mk(1, 0, 0), ey = mk(0, 1, 0);
    const int side = leg & 1;
    const LegFrames F = leg_frames(K, Rwb, sS, sC, leg);
    const v3 r_a = F.r_a, r_h = F.r_h, r_k = F.r_k, loc = F.loc;
    const xform3 &Ea = F.Ea, &Eh = F.Eh, &Ek = F.Ek, &Eabs_a = F.Eabs_a, &Eabs_h = F.Eabs_h, &Eabs_k = F.Eabs_k;
    // contact Jacobian columns: world velocity of the foot per unit generalized velocity
    {
        real *J = JcA + 54 * leg;
        const v3 lk = loc;                               // foot in knee frame
        const v3 lh = r_k + mulT(Ek, lk);                // foot in hip frame
        const v3 la = r_h + mulT(Eh, lh);                // foot in abad frame
        const v3 lb = r_a + mulT(Ea, la);                // foot in base frame
        const v3 ck_ = mulT(Eabs_k, cross(ey, lk)), ch_ = mulT(Eabs_h, cross(ey, lh)), ca_ = mulT(Eabs_a, cross(ex, la));
        const int c0 = 6 + 3 * leg;
        J[0 * 18 + c0] = ca_.x; J[1 * 18 + c0] = ca_.y; J[2 * 18 + c0] = ca_.z;
        J[0 * 18 + c0 + 1] = ch_.x; J[1 * 18 + c0 + 1] = ch_.y; J[2 * 18 + c0 + 1] = ch_.z;
        J[0 * 18 + c0 + 2] = ck_.x; J[1 * 18 + c0 + 2] = ck_.y; J[2 * 18 + c0 + 2] = ck_.z;
        // base: angular columns Rbw (e_i x lb), linear columns Rbw e_i
        const v3 e[3] = {mk(1, 0, 0), mk(0, 1, 0), mk(0, 0, 1)};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const v3 ang = mulT(Rwb, cross(e[i], lb)), lin = mulT(Rwb, e[i]);
            J[0 * 18 + i] = ang.x; J[1 * 18 + i] = ang.y; J[2 * 18 + i] = ang.z;
            J[0 * 18 + 3 + i] = lin.x; J[1 * 18 + 3 + i] = lin.y; J[2 * 18 + 3 + i] = lin.z;
        }
    }
    // composite inertias (rotor constants are folded into the *_eff parents on the host)
    const rbi ICk = rbi_load(K.rb[QR_RB_KNEE]);
    const rbi Ih_e = rbi_load(K.rb[QR_RB_HIP_EFF + side]);
    const rbi Ia_e = rbi_load(K.rb[QR_RB_ABAD_EFF + side]);
    const rbi ICh = rbi_add(Ih_e, rbi_to_parent(ICk, Ek, r_k));
    const rbi ICa = rbi_add(Ia_e, rbi_to_parent(ICh, Eh, r_h));
    const rbi ICa_b = rbi_to_parent(ICa, Ea, r_a);
    real *LB = legB + 16 * leg;
    LB[0] = ICa_b.m; LB[1] = ICa_b.h.x; LB[2] = ICa_b.h.y; LB[3] = ICa_b.h.z;
#pragma unroll
    for (int i = 0; i < 6; ++i) LB[4 + i] = ICa_b.I[i];
    // mass-matrix columns (massMatrix :774-806)
    const real kr = K.k_rot;
    const int ja = 6 + 3 * leg, jh = ja + 1, jk = ja + 2;
    auto base_col = [&](int j, sv6 f) {     // f expressed in the base frame
        const real fv[6] = {f.a.x, f.a.y, f.a.z, f.l.x, f.l.y, f.l.z};
#pragma unroll
        for (int i = 0; i < 6; ++i) { A[i * 18 + j] = fv[i]; A[j * 18 + i] = fv[i]; }
    };
    {   // knee
        sv6 S; S.a = ey; S.l = mk(0, 0, 0);
        sv6 f = rbi_mul(ICk, S);
        A[jk * 18 + jk] = f.a.y + kr;
        f = xforceT(Ek, r_k, f); f.a.y += kr;                 // + Xuprot^T (Irot Srot): knee rotor, E_rot = 1
        A[jh * 18 + jk] = A[jk * 18 + jh] = f.a.y;
        f = xforceT(Eh, r_h, f);
        A[ja * 18 + jk] = A[jk * 18 + ja] = f.a.x;
        f = xforceT(Ea, r_a, f);
        base_col(jk, f);
    }
    {   // hip
        sv6 S; S.a = ey; S.l = mk(0, 0, 0);
        sv6 f = rbi_mul(ICh, S);
        A[jh * 18 + jh] = f.a.y + kr;
        f = xforceT(Eh, r_h, f); f.a.x += kr * K.hiprot_ex; f.a.y += kr * K.hiprot_ey;   // hip rotor: E_rot = Rz(pi)
        A[ja * 18 + jh] = A[jh * 18 + ja] = f.a.x;
        f = xforceT(Ea, r_a, f);
        base_col(jh, f);
    }
    {   // abad
        sv6 S; S.a = ex; S.l = mk(0, 0, 0);
        sv6 f = rbi_mul(ICa, S);
        A[ja * 18 + ja] = f.a.x + kr;
        f = xforceT(Ea, r_a, f); f.a.x += kr;
        base_col(ja, f);
    }
    // gravity (:607-626): ag_i = [0; E_abs_i g], G[i] = -S_i . (IC_i ag_i) = -axis . (h_i x a_i)
    {
        const v3 gw = mk(0, 0, -9.81);
        const v3 g_a = mul(Eabs_a, gw), g_h = mul(Eabs_h, gw), g_k = mul(Eabs_k, gw);
        Gv[ja] = -cross(ICa.h, g_a).x;
        Gv[jh] = -cross(ICh.h, g_h).y;
        Gv[jk] = -cross(ICk.h, g_k).y;
    }
}

// Base block of H and G from the base's own inertia and the four legs' legB[0:10].
QR_HD void wbc_base_block(const WbcConst &K, const xform3 &Rwb, const real *legB, real *A, real *Gv)
{
    rbi IC5 = rbi_load(K.rb[QR_RB_BASE_EFF]);
    for (int l = 0; l < 4; ++l) IC5 = rbi_add(IC5, rbi_load(legB + 16 * l));
    // H[0:6,0:6] = IC5 as a 6x6
    const real I6[3][3] = {{IC5.I[0], IC5.I[3], IC5.I[4]}, {IC5.I[3], IC5.I[1], IC5.I[5]}, {IC5.I[4], IC5.I[5], IC5.I[2]}};
    const real hx[3][3] = {{0, -IC5.h.z, IC5.h.y}, {IC5.h.z, 0, -IC5.h.x}, {-IC5.h.y, IC5.h.x, 0}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            A[i * 18 + j] = I6[i][j];
            A[i * 18 + 3 + j] = hx[i][j];
            A[(3 + i) * 18 + j] = hx[j][i];
            A[(3 + i) * 18 + 3 + j] = (i == j) ? IC5.m : 0.0;
        }
    // G[0:6] = -IC5 [0; a5],  a5 = Rwb g
    const v3 a5 = mul(Rwb, mk(0, 0, -9.81));
    const v3 gt = cross(IC5.h, a5);
    Gv[0] = -gt.x; Gv[1] = -gt.y; Gv[2] = -gt.z; Gv[3] = -IC5.m * a5.x; Gv[4] = -IC5.m * a5.y; Gv[5] = -IC5.m * a5.z;
}

// One leg of the velocity side: foot position / velocity -> pGC / vGC, Jcdqd -> Jcd, the leg's Coriolis rows -> Cv, its force on the base -> legB[10:16].
// pos, bv, qdj: the state's position, base velocity (angular; linear, body frame) and twelve joint rates.
QR_HD void wbc_leg_velocity_chain(const WbcConst &K, const xform3 &Rwb, const real *pos, const real *bv, const real *qdj, const real *sS, const real *sC, int leg,
                                  real *pGC, real *vGC, real *Jcd, real *Cv, real *legB)
{
    const v3 ex = mk(1, 0, 0), ey = mk(0, 1, 0);
    const int side = leg & 1;
    const LegFrames F = leg_frames(K, Rwb, sS, sC, leg);
    const v3 r_a = F.r_a, r_h = F.r_h, r_k = F.r_k, loc = F.loc;
    const xform3 &Ea = F.Ea, &Eh = F.Eh, &Ek = F.Ek, &Eabs_a = F.Eabs_a, &Eabs_h = F.Eabs_h, &Eabs_k = F.Eabs_k;
    const real d0 = qdj[3 * leg], d1 = qdj[3 * leg + 1], d2 = qdj[3 * leg + 2];
    // velocities, bias accelerations
    sv6 v5; v5.a = mk(bv[0], bv[1], bv[2]); v5.l = mk(bv[3], bv[4], bv[5]);
    sv6 va = xmotion(Ea, r_a, v5); sv6 vJa; vJa.a = d0 * ex; vJa.l = mk(0, 0, 0); va.a = va.a + vJa.a;
    sv6 ca = crm(va, vJa);
    sv6 vh = xmotion(Eh, r_h, va); sv6 vJh; vJh.a = d1 * ey; vJh.l = mk(0, 0, 0); vh.a = vh.a + vJh.a;
    sv6 ch = crm(vh, vJh);
    sv6 vk = xmotion(Ek, r_k, vh); sv6 vJk; vJk.a = d2 * ey; vJk.l = mk(0, 0, 0); vk.a = vk.a + vJk.a;
    sv6 ck = crm(vk, vJk);
    sv6 aa = ca;
    sv6 ah = xmotion(Eh, r_h, aa); ah.a = ah.a + ch.a; ah.l = ah.l + ch.l;
    sv6 ak = xmotion(Ek, r_k, ah); ak.a = ak.a + ck.a; ak.l = ak.l + ck.l;
    // Foot position / velocity exactly as forwardKinematics does it (:506-521): through the bottom-left
    // block of Xa and invertSXform / sXFormPoint, which use E^T as E^-1.  With the float-rounded (not
    // exactly unit) quaternion of the state this differs from the textbook sum of offsets by O(|q|^2-1) * 1 m,
    // which the foot task's Kp = 500 would turn into 1e-5 N m.
    {
        auto skewm = [](v3 r) { xform3 S = {{{0, -r.z, r.y}, {r.z, 0, -r.x}, {-r.y, r.x, 0}}}; return S; };
        auto neg = [](const xform3 &A_) { xform3 C_; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C_.m[i][j] = -A_.m[i][j]; return C_; };
        auto addm = [](const xform3 &A_, const xform3 &B_) { xform3 C_; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C_.m[i][j] = A_.m[i][j] + B_.m[i][j]; return C_; };
        auto unskew = [](const xform3 &M_) { return mk(0.5 * (M_.m[2][1] - M_.m[1][2]), 0.5 * (M_.m[0][2] - M_.m[2][0]), 0.5 * (M_.m[1][0] - M_.m[0][1])); };   // matToSkewVec
        const v3 p5 = mk(pos[0], pos[1], pos[2]);
        const xform3 B5 = neg(mul(Rwb, skewm(p5)));                                              // createSXform(R, pos) bottom-left
        const xform3 Ba = addm(mul(neg(mul(Ea, skewm(r_a))), Rwb), mul(Ea, B5));                 // Xup[a] * Xa[5]
        const xform3 Bh = addm(mul(neg(mul(Eh, skewm(r_h))), Eabs_a), mul(Eh, Ba));
        const xform3 Bk = addm(mul(neg(mul(Ek, skewm(r_k))), Eabs_h), mul(Ek, Bh));
        const xform3 E = Eabs_k, Et = transpose(Eabs_k);
        const v3 r1 = (-1.0) * unskew(mul(Et, Bk));                                          // invertSXform: r
        const v3 Er1 = mul(E, r1);
        const xform3 BLi = mul(Et, skewm(Er1));                                                  // Xai bottom-left = -E^T [-E r]x
        const v3 rp = (-1.0) * unskew(mul(E, BLi));                                          // translationFromSXform(Xai)
        const v3 pf = mul(Et, loc - rp);                                                     // sXFormPoint
        const v3 wS = mul(Et, vk.a);
        const v3 vS = mul(BLi, vk.a) + mul(Et, vk.l);
        const v3 vf = vS + cross(wS, pf);                                                    // spatialToLinearVelocity
        pGC[3 * leg] = pf.x; pGC[3 * leg + 1] = pf.y; pGC[3 * leg + 2] = pf.z;
        vGC[3 * leg] = vf.x; vGC[3 * leg + 1] = vf.y; vGC[3 * leg + 2] = vf.z;
    }
    // Jcdqd = Rai [ (a_lin + a_ang x loc) + w x (v_lin + w x loc) ]
    {
        const v3 t = (ak.l + cross(ak.a, loc)) + cross(vk.a, vk.l + cross(vk.a, loc));
        const v3 jd = mulT(Eabs_k, t);
        Jcd[3 * leg] = jd.x; Jcd[3 * leg + 1] = jd.y; Jcd[3 * leg + 2] = jd.z;
    }
    // Coriolis (:633-665) with link inertias
    {
        const rbi Ik = rbi_load(K.rb[QR_RB_KNEE]), Ih = rbi_load(K.rb[QR_RB_HIP + side]), Ia = rbi_load(K.rb[QR_RB_ABAD + side]);
        const int ja = 6 + 3 * leg, jh = ja + 1, jk = ja + 2;
        sv6 fk = rbi_mul(Ik, ak); { sv6 c = crf(vk, rbi_mul(Ik, vk)); fk.a = fk.a + c.a; fk.l = fk.l + c.l; }
        sv6 fh = rbi_mul(Ih, ah); { sv6 c = crf(vh, rbi_mul(Ih, vh)); fh.a = fh.a + c.a; fh.l = fh.l + c.l; }
        sv6 fa = rbi_mul(Ia, aa); { sv6 c = crf(va, rbi_mul(Ia, va)); fa.a = fa.a + c.a; fa.l = fa.l + c.l; }
        Cv[jk] = fk.a.y;
        { sv6 t = xforceT(Ek, r_k, fk); fh.a = fh.a + t.a; fh.l = fh.l + t.l; }
        Cv[jh] = fh.a.y;
        { sv6 t = xforceT(Eh, r_h, fh); fa.a = fa.a + t.a; fa.l = fa.l + t.l; }
        Cv[ja] = fa.a.x;
        sv6 t = xforceT(Ea, r_a, fa);
        real *LB = legB + 16 * leg;
        LB[10] = t.a.x; LB[11] = t.a.y; LB[12] = t.a.z; LB[13] = t.l.x; LB[14] = t.l.y; LB[15] = t.l.z;
    }
}

// Base block of C: fvp5 = v5 x* (I5 v5) (avp5 = 0) plus the four legs' legB[10:16].
QR_HD void wbc_base_coriolis(const WbcConst &K, const real *bv, const real *legB, real *Cv)
{
    sv6 fb; fb.a = mk(0, 0, 0); fb.l = mk(0, 0, 0);
    for (int l = 0; l < 4; ++l) { const real *LB = legB + 16 * l; fb.a = fb.a + mk(LB[10], LB[11], LB[12]); fb.l = fb.l + mk(LB[13], LB[14], LB[15]); }
    const rbi I5 = rbi_load(K.rb[QR_RB_BASE]);
    sv6 v5; v5.a = mk(bv[0], bv[1], bv[2]); v5.l = mk(bv[3], bv[4], bv[5]);
    const sv6 c5 = crf(v5, rbi_mul(I5, v5));
    Cv[0] = c5.a.x + fb.a.x; Cv[1] = c5.a.y + fb.a.y; Cv[2] = c5.a.z + fb.a.z;
    Cv[3] = c5.l.x + fb.l.x; Cv[4] = c5.l.y + fb.l.y; Cv[5] = c5.l.z + fb.l.z;
}

}  // namespace qrgpu
