// Cross-lane helpers for wave64 on gfx950: DPP row all-reduce + v_readlane combine (no LDS traffic, no
// ds_bpermute), uniform broadcasts, fast reciprocal; the wave fence, the write-through store, the robot-type rule and the torque tail every
// kernel shares.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/qrgpu.h"

namespace qrgpu {

// The fence between the lanes of one wavefront: what a lane stored to LDS in front of it, the wave's other lanes read behind it.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A plain store, or -- `through`: another launch reads the value while this one still runs -- an agent-scope one (global_store ... sc1, written
// through to memory).
template <typename T> __device__ __forceinline__ void st_through(T *p, T v, bool through)
{
    if (through) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *p = v;
}

// A robot whose type id is out of range or names a type that was never set up (bit t of type_ready: type t was) is computed with the first
// valid type and flagged: -> true, tyid replaced.
__device__ __forceinline__ bool resolve_type(int &tyid, int type_ready)
{
    const bool bad_type = tyid < 0 || tyid >= QRGPU_MAX_TYPES || !((type_ready >> (tyid & (QRGPU_MAX_TYPES - 1))) & 1);
    if (bad_type) tyid = __builtin_ctz(type_ready | (1 << QRGPU_MAX_TYPES));
    return bad_type;
}

// K14 torque tail: bit 0 of `epilogue` = the +-0.9 N m abad compensation of qrFSMStateLocomotion::Run (QS/fsm/qr_fsm_state_locomotion.cpp:141-151),
// on the motors the caller says it survives on (comp); bit 1 = the +-23 N m clip of qrSafetyChecker::CheckForceFeedForward
// (QS/fsm/qr_safety_checker.cpp:48-66); legCmd.tua is a double there.
__device__ __forceinline__ float torque_epilogue(float tau, int motor, bool comp, int epilogue)
{
    double t = (double)tau;
    if (comp && (epilogue & 1) && motor % 3 == 0) t += (double)(((motor / 3) & 1) ? 0.9f : -0.9f);     // tua_ * pow(-1, (leg + 1) % 2)
    if (epilogue & 2) t = t > 23.0 ? 23.0 : (t < -23.0 ? -23.0 : t);
    return (float)t;
}

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

// ---- rotation helpers shared by the swing-mode and stance kernels (robotics::math, include/quadruped/utils/qr_se3.h); fp32 with the
// reference's float / double mix, contraction off.  3x3 matrices are row-major R[row][col]; a product's entry is (a0 b0 + a1 b1) + a2 b2.

// Eigen::Quaternion<float>::toRotationMatrix (w, x, y, z)
__device__ __forceinline__ void quat_to_rot(float w, float x, float y, float z, float R[3][3])
{
#pragma clang fp contract(off)
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0][0] = 1.f - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1.f - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1.f - (txx + tyy);
}

__device__ __forceinline__ float dot3(const float a[3], const float b0, const float b1, const float b2)
{
#pragma clang fp contract(off)
    return (a[0] * b0 + a[1] * b1) + a[2] * b2;
}

// robotics::math::RigidTransform(t, q, p) = q.inverse() p + q.inverse() (-t)  (include/quadruped/utils/qr_se3.h:459-466)
__device__ __forceinline__ void rigid_transform(const float q[4], const float t[3], const float p[3], float out[3])
{
#pragma clang fp contract(off)
    const float n2 = (q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]);
    float Ri[3][3];
    quat_to_rot(q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2, Ri);
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = dot3(Ri[r], p[0], p[1], p[2]) + dot3(Ri[r], -t[0], -t[1], -t[2]);
}

// stateDataFlow.baseRMat = quaternionToRotationMatrix(q)^T (qr_se3.h:186-203, qr_robot.cpp:70): base -> world
__device__ __forceinline__ void base_rmat(const float q[4], float R[3][3])
{
#pragma clang fp contract(off)
    const float e0 = q[0], e1 = q[1], e2 = q[2], e3 = q[3];
    R[0][0] = 1 - 2 * (e2 * e2 + e3 * e3); R[0][1] = 2 * (e1 * e2 - e0 * e3); R[0][2] = 2 * (e1 * e3 + e0 * e2);
    R[1][0] = 2 * (e1 * e2 + e0 * e3); R[1][1] = 1 - 2 * (e1 * e1 + e3 * e3); R[1][2] = 2 * (e2 * e3 - e0 * e1);
    R[2][0] = 2 * (e1 * e3 - e0 * e2); R[2][1] = 2 * (e2 * e3 + e0 * e1); R[2][2] = 1 - 2 * (e1 * e1 + e2 * e2);
}

// robotics::math::invertRigidTransform(t, q, p) = q p + t (qr_se3.h:442-449; Eigen's Quaternion::toRotationMatrix)
__device__ __forceinline__ void invert_rigid_transform(const float q[4], const float t[3], const float p[3], float out[3])
{
#pragma clang fp contract(off)
    float R[3][3];
    quat_to_rot(q[0], q[1], q[2], q[3], R);
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = dot3(R[r], p[0], p[1], p[2]) + t[r];
}

// TransformVecByQuat(quat, r_b) = (2 q0 q0 - 1) r_b + 2 q0 [q_]x r_b + 2 q_ (q_ . r_b) (qr_se3.h:473-479)
__device__ __forceinline__ void transform_vec_by_quat(const float q[4], const float rb[3], float out[3])
{
#pragma clang fp contract(off)
    const float q0 = q[0], v0 = q[1], v1 = q[2], v2 = q[3];
    const float a = 2 * q0 * q0 - 1, s = 2 * q0;
    const float M[3][3] = {{s * 0.f, s * -v2, s * v1}, {s * v2, s * 0.f, s * -v0}, {s * -v1, s * v0, s * 0.f}};
    const float d = (v0 * rb[0] + v1 * rb[1]) + v2 * rb[2];
    const float w[3] = {2 * v0, 2 * v1, 2 * v2};
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = (a * rb[r] + dot3(M[r], rb[0], rb[1], rb[2])) + w[r] * d;
}

// quatInverse (qr_se3.h:307-313)
__device__ __forceinline__ void quat_inverse(const float q[4], float out[4])
{
#pragma clang fp contract(off)
    const float n2 = (q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]);
    out[0] = q[0] / n2; out[1] = -q[1] / n2; out[2] = -q[2] / n2; out[3] = -q[3] / n2;
}

__device__ __forceinline__ void mat3_mul(const float A[3][3], const float B[3][3], float C[3][3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[r][c] = (A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c];
}

// rpyToRotMat = Rx(roll) Ry(pitch) Rz(yaw) of coordinateRotation's coordinate-transform matrices (qr_se3.h:71-89, 108-116)
__device__ __forceinline__ void rpy_to_rotmat(const float rpy[3], float M[3][3])
{
#pragma clang fp contract(off)
    const float sr = sinf(rpy[0]), cr = cosf(rpy[0]), sp = sinf(rpy[1]), cp = cosf(rpy[1]), sy = sinf(rpy[2]), cy = cosf(rpy[2]);
    const float X[3][3] = {{1.f, 0.f, 0.f}, {0.f, cr, sr}, {0.f, -sr, cr}};
    const float Y[3][3] = {{cp, 0.f, -sp}, {0.f, 1.f, 0.f}, {sp, 0.f, cp}};
    const float Z[3][3] = {{cy, sy, 0.f}, {-sy, cy, 0.f}, {0.f, 0.f, 1.f}};
    float XY[3][3];
    mat3_mul(X, Y, XY);
    mat3_mul(XY, Z, M);
}

// rotationMatrixToRPY(R) = quatToRPY(rotationMatrixToQuaternion(R)) (qr_se3.h:145-178, 209-223, 255-262), given r = R^T: the matrix
// rotationMatrixToQuaternion works on after its own transpose
__device__ __forceinline__ void rotmat_t_to_rpy(const float r[3][3], float rpy[3])
{
#pragma clang fp contract(off)
    float q0, q1, q2, q3;
    const float tr = (r[0][0] + r[1][1]) + r[2][2];
    if ((double)tr > 0.0) {
        const float S = (float)(sqrt((double)tr + 1.0) * 2.0);
        q0 = (float)(0.25 * (double)S); q1 = (r[2][1] - r[1][2]) / S; q2 = (r[0][2] - r[2][0]) / S; q3 = (r[1][0] - r[0][1]) / S;
    } else if (r[0][0] > r[1][1] && r[0][0] > r[2][2]) {
        const float S = (float)(sqrt(1.0 + (double)r[0][0] - (double)r[1][1] - (double)r[2][2]) * 2.0);
        q0 = (r[2][1] - r[1][2]) / S; q1 = (float)(0.25 * (double)S); q2 = (r[0][1] + r[1][0]) / S; q3 = (r[0][2] + r[2][0]) / S;
    } else if (r[1][1] > r[2][2]) {
        const float S = (float)(sqrt(1.0 + (double)r[1][1] - (double)r[0][0] - (double)r[2][2]) * 2.0);
        q0 = (r[0][2] - r[2][0]) / S; q1 = (r[0][1] + r[1][0]) / S; q2 = (float)(0.25 * (double)S); q3 = (r[1][2] + r[2][1]) / S;
    } else {
        const float S = (float)(sqrt(1.0 + (double)r[2][2] - (double)r[0][0] - (double)r[1][1]) * 2.0);
        q0 = (r[1][0] - r[0][1]) / S; q1 = (r[0][2] + r[2][0]) / S; q2 = (r[1][2] + r[2][1]) / S; q3 = (float)(0.25 * (double)S);
    }
    const float as = (float)fmin(-2. * (double)(q1 * q3 - q0 * q2), .99999);
    rpy[2] = atan2f(2 * (q1 * q2 + q0 * q3), ((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3);
    rpy[1] = asinf(as);
    rpy[0] = atan2f(2 * (q2 * q3 + q0 * q1), ((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3);
}

// vectorToSkewMat / crossMatrix (qr_se3.h:95-103, 121-130)
__device__ __forceinline__ void vector_to_skew_mat(const float v[3], float m[3][3])
{
    m[0][0] = 0.f; m[0][1] = -v[2]; m[0][2] = v[1];
    m[1][0] = v[2]; m[1][1] = 0.f; m[1][2] = -v[0];
    m[2][0] = -v[1]; m[2][1] = v[0]; m[2][2] = 0.f;
}

// so3ToQuat (qr_se3.h:402-418): theta in float, the half angle and its sine / cosine in double
__device__ __forceinline__ void so3_to_quat(const float so3[3], float q[4])
{
#pragma clang fp contract(off)
    const float theta = sqrtf((so3[0] * so3[0] + so3[1] * so3[1]) + so3[2] * so3[2]);
    if (fabs((double)theta) < 1.e-6) { q[0] = 1.f; q[1] = 0.f; q[2] = 0.f; q[3] = 0.f; return; }
    const double h = (double)theta / 2., sh = sin(h);
    q[0] = (float)cos(h);
    q[1] = (float)((double)(so3[0] / theta) * sh);
    q[2] = (float)((double)(so3[1] / theta) * sh);
    q[3] = (float)((double)(so3[2] / theta) * sh);
}

// ConcatenationTwoQuats(q, p) = (q0 p0 - q_.p_, q0 p_ + p0 q_ + [q_]x p_) (qr_se3.h:484-494)
__device__ __forceinline__ void concatenation_two_quats(const float q[4], const float p[4], float out[4])
{
#pragma clang fp contract(off)
    float S[3][3];
    vector_to_skew_mat(q + 1, S);
    out[0] = q[0] * p[0] - ((q[1] * p[1] + q[2] * p[2]) + q[3] * p[3]);
#pragma unroll
    for (int r = 0; r < 3; ++r) out[1 + r] = (q[0] * p[1 + r] + p[0] * q[1 + r]) + dot3(S[r], p[1], p[2], p[3]);
}

// quatToRPY (qr_se3.h:209-223)
__device__ __forceinline__ void quat_to_rpy(const float q[4], float rpy[3])
{
#pragma clang fp contract(off)
    const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const float as = (float)fmin(-2. * (double)(q1 * q3 - q0 * q2), .99999);
    rpy[2] = atan2f(2 * (q1 * q2 + q0 * q3), ((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3);
    rpy[1] = asinf(as);
    rpy[0] = atan2f(2 * (q2 * q3 + q0 * q1), ((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3);
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
