// Cross-lane helpers for wave64 on gfx950: DPP row all-reduce + v_readlane combine (no LDS traffic, no
// ds_bpermute), uniform broadcasts, fast reciprocal.  Shared by the MPC and WBC kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace qrgpu {

// 1/x by v_rcp_f64 + two Newton steps (<= 1 ulp-ish; the active-set step lengths do not need IEEE division)
__device__ __forceinline__ double fast_rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return r;
}

// 1/x by v_rcp_f64 (4.6e-8 relative, scratch/ubench/rcp.hip) + one Newton step: 2.2e-15 relative -- for the pivots of a sweep, whose
// reciprocal sits on the dependent chain of every step
__device__ __forceinline__ double fast_rcp1(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return r;
}

// ---- cross-lane helpers (wave64) ---------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ double dpp_d(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// srclane must be wave-uniform
__device__ __forceinline__ double readlane_d(double v, int srclane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), srclane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), srclane);
    return __hiloint2double(hi, lo);
}
// All-reduce inside each 16-lane row: xor 1, xor 2 (quad_perm), rotate by 4 and 8 (row_ror); then
// the four row results are combined through v_readlane.  Result is wave-uniform.
__device__ __forceinline__ double wave_min_d(double v)
{
    v = fmin(v, dpp_d<0xB1>(v));      // quad_perm [1,0,3,2]
    v = fmin(v, dpp_d<0x4E>(v));      // quad_perm [2,3,0,1]
    v = fmin(v, dpp_d<0x124>(v));     // row_ror:4
    v = fmin(v, dpp_d<0x128>(v));     // row_ror:8
    const double a = readlane_d(v, 0), b = readlane_d(v, 16), c = readlane_d(v, 32), d = readlane_d(v, 48);
    return fmin(fmin(a, b), fmin(c, d));
}
__device__ __forceinline__ double wave_sum_d(double v)
{
    v += dpp_d<0xB1>(v);
    v += dpp_d<0x4E>(v);
    v += dpp_d<0x124>(v);
    v += dpp_d<0x128>(v);
    return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}
// lowest lane whose predicate holds (or -1); uniform
__device__ __forceinline__ int first_lane(bool pred)
{
    const unsigned long long m = __ballot(pred);
    return m ? (int)__builtin_ctzll(m) : -1;
}


// Column j of the analytic leg Jacobian (AnalyticalLegJacobian, quadruped/src/robots/qr_robot.cpp:148-172) in fp32.
__device__ __forceinline__ void leg_jacobian_column(int j, float t0, float t1, float t2, float sh, float lu, float ll, float &J0, float &J1, float &J2)
{
    const float lEff = sqrtf(lu * lu + ll * ll + 2 * lu * ll * cosf(t2));
    const float tEff = t1 + t2 / 2;
    if (j == 0) {
        J0 = 0;
        J1 = -sh * sinf(t0) + lEff * cosf(t0) * cosf(tEff);
        J2 = sh * cosf(t0) + lEff * sinf(t0) * cosf(tEff);
    } else if (j == 1) {
        J0 = -lEff * cosf(tEff);
        J1 = -lEff * sinf(t0) * sinf(tEff);
        J2 = lEff * sinf(tEff) * cosf(t0);
    } else {
        J0 = ll * lu * sinf(t2) * sinf(tEff) / lEff - lEff * cosf(tEff) / 2;
        J1 = -ll * lu * sinf(t0) * sinf(t2) * cosf(tEff) / lEff - lEff * sinf(t0) * sinf(tEff) / 2;
        J2 = ll * lu * sinf(t2) * cosf(t0) * cosf(tEff) / lEff + lEff * sinf(tEff) * cosf(t0) / 2;
    }
}

// ---- swing-leg helpers shared by the swing kernels (qr_estimator_kernel.hip, qr_swing_modes_kernel.hip); fp32, contraction off -------

// SwingFootTrajectory::GenerateTrajectoryPoint's phase warp (phaseModule = true), qr_foot_trajectory_generator.cpp:328-335
__device__ __forceinline__ float swing_warp_phase(float inputPhase)
{
#pragma clang fp contract(off)
    if (inputPhase <= 0.5f) return (float)(0.8 * sin((double)inputPhase * 3.14159265358979323846));
    return (float)(0.8 + ((double)inputPhase - 0.5) * 0.4);
}

// qrFootParabolaPatternGenerator::GenerateTrajectory with height 0.1 (qr_foot_trajectory_generator.cpp:187-215, qr_geometry.cpp:157-190):
// XY linear, Z parabola through max(z_start, z_end) + 0.1 at phase 0.5.  pw is left untouched outside [-1e-3, 1 + 1e-3) and z for phase < 0.
__device__ __forceinline__ void swing_parabola_point(float phase, const float st[3], const float tg[3], float pw[3])
{
#pragma clang fp contract(off)
    if (!((double)phase < 0.0 - 1e-3) && !((double)phase >= 0.0 + 1.0 + 1e-3)) {
        pw[0] = (1 - phase) * st[0] + phase * tg[0];
        pw[1] = (1 - phase) * st[1] + phase * tg[1];
        const float mid = (tg[2] > st[2] ? tg[2] : st[2]) + 0.1f;
        if (!(phase < 0.f)) {
            const float d1 = mid - st[2], d2 = tg[2] - st[2];
            const float d3 = (float)(0.25 - 0.5);
            const float ca = (d1 - d2 * 0.5f) / d3;
            const float cb = (float)(((double)d2 * 0.25 - (double)d1) / (double)d3);
            pw[2] = (float)((double)ca * ((double)phase * (double)phase) + (double)(cb * phase) + (double)st[2]);
        }
    }
}

// Leg inverse kinematics, qrRobot::FootPositionInHipFrameToJointAngle (quadruped/src/robots/qr_robot.cpp:106-124) of the foot position p
// in the base frame minus the hip offset ho; sh = hipLength * (-1 for right legs, +1 for left legs)
__device__ __forceinline__ void leg_ik(const float p[3], const float ho[3], float sh, float lu, float ll, float ang[3])
{
#pragma clang fp contract(off)
    const float x = p[0] - ho[0], y = p[1] - ho[1], z = p[2] - ho[2];
    const float tK = -acosf(((x * x + y * y + z * z) - (sh * sh + lu * lu + ll * ll)) / (2 * ll * lu));
    const float l = sqrtf(lu * lu + ll * ll + 2 * lu * ll * cosf(tK));
    const float tH = asinf(-x / l) - tK / 2;
    const float c1 = sh * y - l * cosf(tH + tK / 2) * z;
    const float s1 = l * cosf(tH + tK / 2) * y + sh * z;
    ang[0] = atan2f(s1, c1); ang[1] = tH; ang[2] = tK;
}

// AnalyticalLegJacobian(...).inverse() (qr_robot.cpp:148-172, 200-219): the adjugate over the determinant
__device__ __forceinline__ void leg_jacobian_inverse(const float ang[3], float sh, float lu, float ll, float Ji[3][3])
{
#pragma clang fp contract(off)
    float J[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) leg_jacobian_column(j, ang[0], ang[1], ang[2], sh, lu, ll, J[0][j], J[1][j], J[2][j]);
    const float det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    const float id = 1.f / det;
    Ji[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * id; Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id; Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
    Ji[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) * id; Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id; Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
    Ji[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * id; Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id; Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
}

}  // namespace qrgpu
