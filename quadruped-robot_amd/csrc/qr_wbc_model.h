// BuildDynamicModel (QS/robots/qr_robot_a1_sim.cpp:176-343; the Lite3 file is a literal copy) reduced to the rigid-body parameters of WbcConst.
// Literals are the reference's float literals, evaluated in double.  Host only: the library's qrgpu_wbc_setup and the CPU build of the WBC's
// rigid-body chains (tests/stubs/wbc_rigid_body_host.hip) include it.
#pragma once
#include <cmath>
#include "qr_device_types.h"

namespace qrgpu {

struct RB { double m, h[3], I[6]; };     // I: xx yy zz xy xz yz about the frame origin
inline RB make_rb(double m, const double c[3], const double Ic[9])
{   // SpatialInertia(mass, com, inertia), QI/dynamics/spatial.hpp:390-398: Ibar = I + m [c]x[c]x^T
    RB r; r.m = m;
    for (int i = 0; i < 3; ++i) r.h[i] = m * c[i];
    const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    double Ib[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Ib[i][j] = Ic[3 * i + j] + m * ((i == j ? cc : 0.0) - c[i] * c[j]);
    r.I[0] = Ib[0][0]; r.I[1] = Ib[1][1]; r.I[2] = Ib[2][2]; r.I[3] = Ib[0][1]; r.I[4] = Ib[0][2]; r.I[5] = Ib[1][2];
    return r;
}
inline RB flip_y(const RB &a)
{   // flipAlongAxis(Y), spatial.hpp:505-534: mirror y
    RB r = a;
    r.h[1] = -a.h[1];
    r.I[3] = -a.I[3];
    r.I[5] = -a.I[5];
    return r;
}
inline RB add_rb(const RB &a, const RB &b)
{
    RB r; r.m = a.m + b.m;
    for (int i = 0; i < 3; ++i) r.h[i] = a.h[i] + b.h[i];
    for (int i = 0; i < 6; ++i) r.I[i] = a.I[i] + b.I[i];
    return r;
}
inline void store_rb(double *dst, const RB &r)
{
    dst[0] = r.m; dst[1] = r.h[0]; dst[2] = r.h[1]; dst[3] = r.h[2];
    for (int i = 0; i < 6; ++i) dst[4 + i] = r.I[i];
}
inline void build_wbc_const(const qrgpu_model_desc &d, WbcConst &K)
{
    auto F = [](double x) { return (double)(float)x; };      // the reference's literals are floats
    const double u = F(1e-6);
    const double abadI[9] = {F(469.2) * u, F(-9.4) * u, F(-0.342) * u, F(-9.4) * u, F(807.5) * u, F(-0.466) * u, F(-0.342) * u, F(-0.466) * u, F(552.9) * u};
    const double abadC[3] = {F(-0.0033), 0, 0};
    const double hipI[9] = {F(5529) * u, F(4.825) * u, F(343.9) * u, F(4.825) * u, F(5139.3) * u, F(22.4) * u, F(343.9) * u, F(22.4) * u, F(1367.8) * u};
    const double hipC[3] = {F(-0.003237), F(-0.022327), F(-0.027326)};
    const double kneeI[9] = {F(2998) * u, 0, F(-141.2) * u, 0, F(3014) * u, 0, F(-141.2) * u, 0, F(32.4) * u};
    const double kneeC[3] = {F(0.006435), 0, F(-0.107)};
    const double bodyI[9] = {F(15853) * u, 0, 0, 0, F(37799) * u, 0, 0, 0, F(45654) * u};
    const double zero3[3] = {0, 0, 0};
    const double m_abad = F(0.696), m_hip = F(1.013), m_knee = F(0.166), m_body = 6.0;
    const RB abadL = make_rb(m_abad, abadC, abadI), hipL = make_rb(m_hip, hipC, hipI), knee = make_rb(m_knee, kneeC, kneeI);
    const RB abadR = flip_y(abadL), hipR = flip_y(hipL);
    const RB base = make_rb(m_body, zero3, bodyI);
    // rotors (:193-198, :244-247): mass 1e-8, inertia (1e-2 * 1e-6) * identity  (setIdentity() overrides 33/33/63)
    const double k_rot = (double)(float)(F(1e-2) * 1e-6), m_rot = F(1e-8);
    auto rotor_at = [&](double x, double y, double z) {
        const double c[3] = {x, y, z};
        const double I[9] = {k_rot, 0, 0, 0, k_rot, 0, 0, 0, k_rot};
        return make_rb(m_rot, c, I);
    };
    RB base_eff = base;
    const double arx = F(0.14), ary = F(0.047);
    for (int leg = 0; leg < 4; ++leg) base_eff = add_rb(base_eff, rotor_at((leg < 2 ? 1 : -1) * arx, ((leg & 1) ? 1 : -1) * ary, 0.0));
    const double hry = F(0.04);
    const RB abadR_eff = add_rb(abadR, rotor_at(0, -hry, 0)), abadL_eff = add_rb(abadL, rotor_at(0, hry, 0));
    const RB hipR_eff = add_rb(hipR, rotor_at(0, 0, 0)), hipL_eff = add_rb(hipL, rotor_at(0, 0, 0));
    store_rb(K.rb[QR_RB_BASE], base);          store_rb(K.rb[QR_RB_BASE_EFF], base_eff);
    store_rb(K.rb[QR_RB_ABAD + 0], abadR);     store_rb(K.rb[QR_RB_ABAD + 1], abadL);
    store_rb(K.rb[QR_RB_ABAD_EFF + 0], abadR_eff); store_rb(K.rb[QR_RB_ABAD_EFF + 1], abadL_eff);
    store_rb(K.rb[QR_RB_HIP + 0], hipR);       store_rb(K.rb[QR_RB_HIP + 1], hipL);
    store_rb(K.rb[QR_RB_HIP_EFF + 0], hipR_eff); store_rb(K.rb[QR_RB_HIP_EFF + 1], hipL_eff);
    store_rb(K.rb[QR_RB_KNEE], knee);
    K.abad_loc[0] = F(0.1805); K.abad_loc[1] = F(0.047); K.abad_loc[2] = 0.0;
    K.hip_l = d.hip_l; K.upper_l = d.upper_l; K.lower_l = d.lower_l; K.foot_y = F(0.004);
    K.k_rot = k_rot;
    const double pi_f = (double)(float)M_PI;                   // coordinateRotation(Z, float(M_PI)) (:299)
    K.hiprot_ex = -std::sin(pi_f); K.hiprot_ey = std::cos(pi_f);
    const double total = m_body + 4.0 * (m_abad + m_hip + m_knee);                  // totalNonRotorMass()
    K.max_fz = (double)(float)total * (double)9.81f;
    K.kp_pos = d.kp_body_pos; K.kd_pos = d.kd_body_pos; K.kp_ori = d.kp_body_ori; K.kd_ori = d.kd_body_ori;
    K.kp_foot = d.kp_foot; K.kd_foot = d.kd_foot;
    K.w_fb = d.weight_fb; K.w_fr = d.weight_fr; K.mu = d.mu;
}

}  // namespace qrgpu
