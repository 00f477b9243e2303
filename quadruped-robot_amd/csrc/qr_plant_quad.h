// What the plant kernels (qr_plant_kernel.hip, qr_plant_body_kernel.hip) share on the device: the quad of four lanes that is one robot -- who it is,
// sums and flags across it, the forward dynamics across it -- the lane's column of LDS, and the steps of a control tick that the terrain and the
// body step kernel have in common, as named pieces: the state in, the command read and the motor law, the integrator, the state check, plant_out,
// the field, push and terrain_out.  What a kernel's tick has of its own stands in that kernel's sub-step loop.  The flat step kernel calls
// state_check alone and keeps the rest written out, and the state write and the mpc_state / est_in writes are written out in all three: each is a
// measured choice (launch times), not a style.  Device only: the algebra that also runs on a CPU is qr_plant_math.h's.
#pragma once
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_wave_helpers.h"
#include "qr_plant_math.h"
#include "qr_terrain.h"

namespace qrgpu {

using namespace plant;

#define QR_PL_QUADS 16     // robots per wavefront

__device__ __forceinline__ real quad_sum(real v)
{
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v;
}
__device__ __forceinline__ v3 quad_sum(v3 v) { return mk(quad_sum(v.x), quad_sum(v.y), quad_sum(v.z)); }
__device__ __forceinline__ int quad_or(int v)
{
    v |= __shfl_xor(v, 1);
    v |= __shfl_xor(v, 2);
    return v;
}
__device__ __forceinline__ bool finite3(v3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// Which robot, which constants: the WBC kernel's rule for a type that was never set up (computed with the first valid type, flagged).
struct Who { int robot, leg, flags; bool live; const WbcConst *K; };
__device__ __forceinline__ Who who_am_i(int n, const WbcConst *types, const int *type_id, int type_ready)
{
    Who w;
    const int robot = blockIdx.x * QR_PL_QUADS + (threadIdx.x >> 2);
    w.live = robot < n;
    w.robot = w.live ? robot : n - 1;
    w.leg = threadIdx.x & 3;
    int tyid = type_id ? type_id[w.robot] : 0;
    const bool bad_type = resolve_type(tyid, type_ready);
    w.flags = bad_type ? QRGPU_PL_BAD_TYPE : 0;
    w.K = types + (tyid & (QRGPU_MAX_TYPES - 1));
    return w;
}

// The quaternion normalised in fp64; a zero or non-finite one is flagged and replaced by the identity.
__device__ __forceinline__ void unit_quat(real &w, real &x, real &y, real &z, int &flags)
{
    const real nn = w * w + x * x + y * y + z * z;
    if (!(nn > 0.0) || !isfinite(nn)) { flags |= QRGPU_PL_QUAT_ZERO; w = 1.0; x = y = z = 0.0; return; }
    const real inv = 1.0 / sqrt(nn);
    w *= inv; x *= inv; y *= inv; z *= inv;
}

// Forward dynamics of one robot across its quad, after leg_start: this lane's leg in, the base's and this leg's accelerations out.
// WRENCH: an external wrench on the base (moment about its origin; force), base frame, enters the base's bias force.
template <bool WRENCH = false>
__device__ __forceinline__ void forward_dynamics(const WbcConst &K, int leg, const Stash &st, const frame3 &R, sv6 v0, real qd0, real qd1, real qd2, real tau0,
                                                 real tau1, real tau2, v3 f_b, sv6 &afb, real &qdd0, real &qdd1, real &qdd2, sv6 wrench_b = sv6())
{
    abi IA;
    sv6 pA;
    leg_inward(K, leg, st, qd0, qd1, qd2, tau0, tau1, tau2, f_b, IA, pA);
#pragma unroll
    for (int i = 0; i < 6; ++i) { IA.I[i] = quad_sum(IA.I[i]); IA.M[i] = quad_sum(IA.M[i]); }
    IA.h0 = quad_sum(IA.h0); IA.h1 = quad_sum(IA.h1); IA.h2 = quad_sum(IA.h2);
    pA.a = quad_sum(pA.a); pA.l = quad_sum(pA.l);
    abi IA0; sv6 pA0;
    base_start(K, v0, IA0, pA0);
    if (WRENCH) pA0 = pA0 + (-1.0) * wrench_b;
    sv6 a0;
    base_solve(IA0 + IA, pA0 + pA, R, afb, a0);
    leg_outward(K, leg, st, a0, qdd0, qdd1, qdd2);
}

// A lane's column of the workgroup's LDS: what a leg keeps between its joints (qr_plant_math.h).  Lane-private: no barrier stands anywhere.
#define QR_PL_STASH() __shared__ real stash_lds[QR_PL_ST_SLOTS * 64]; Stash st; st.p = stash_lds + threadIdx.x; st.stride = 64

#define ROW(p, f) (p)[(size_t)(f) * N + i]

__device__ __forceinline__ real clip(real x, real lim) { return fmin(fmax(x, -lim), lim); }

// ---- The pieces of a control tick.  N, i, j: the batch size, the lane's robot and the first joint row of its leg (3 * leg), as ROW reads them.

// The state as a lane holds it across the sub-steps is thirteen loose values, passed to the pieces by name: the base (qw qx qy qz, pos, v0: the same
// bits in the four lanes of a quad) and this lane's leg (q0 q1 q2, qd0 qd1 qd2).  The long argument lists are a measured compromise: with the
// thirteen in one struct hipcc leaves one multiply-add of the terrain and of the body kernel unfused, so their rounding differs from the same
// text written out in the kernel.  Do not tidy them into a struct without comparing outputs bit for bit.

// The motor command of a leg's joints: p, Kp, d, Kd, tua.
struct Cmd { real cp0, cp1, cp2, kp0, kp1, kp2, cd0, cd1, cd2, kd0, kd1, kd2, ff0, ff1, ff2; };

// The state: read once, rows 0-12 and this leg's joint rows widened to fp64, the quaternion normalised.
__device__ __forceinline__ void state_in(const float *g_state, size_t N, int i, int j, int &flags, real &qw, real &qx, real &qy, real &qz, v3 &pos, sv6 &v0,
                                         real &q0, real &q1, real &q2, real &qd0, real &qd1, real &qd2)
{
    qw = ROW(g_state, 0); qx = ROW(g_state, 1); qy = ROW(g_state, 2); qz = ROW(g_state, 3);
    unit_quat(qw, qx, qy, qz, flags);
    pos = mk(ROW(g_state, 4), ROW(g_state, 5), ROW(g_state, 6));
    v0.a = mk(ROW(g_state, 7), ROW(g_state, 8), ROW(g_state, 9));
    v0.l = mk(ROW(g_state, 10), ROW(g_state, 11), ROW(g_state, 12));
    q0 = ROW(g_state, 13 + j); q1 = ROW(g_state, 14 + j); q2 = ROW(g_state, 15 + j);
    qd0 = ROW(g_state, 25 + j); qd1 = ROW(g_state, 26 + j); qd2 = ROW(g_state, 27 + j);
}

__device__ __forceinline__ Cmd cmd_in(const float *g_cmd, size_t N, int i, int j)
{
    Cmd c;
    c.cp0 = ROW(g_cmd, j); c.cp1 = ROW(g_cmd, j + 1); c.cp2 = ROW(g_cmd, j + 2);
    c.kp0 = ROW(g_cmd, 12 + j); c.kp1 = ROW(g_cmd, 13 + j); c.kp2 = ROW(g_cmd, 14 + j);
    c.cd0 = ROW(g_cmd, 24 + j); c.cd1 = ROW(g_cmd, 25 + j); c.cd2 = ROW(g_cmd, 26 + j);
    c.kd0 = ROW(g_cmd, 36 + j); c.kd1 = ROW(g_cmd, 37 + j); c.kd2 = ROW(g_cmd, 38 + j);
    c.ff0 = ROW(g_cmd, 48 + j); c.ff1 = ROW(g_cmd, 49 + j); c.ff2 = ROW(g_cmd, 50 + j);
    return c;
}

// The Gazebo joint controller's motor law, clipped.
__device__ __forceinline__ void motor_law(const Cmd &c, real q0, real q1, real q2, real qd0, real qd1, real qd2, real tau_max, real &tau0, real &tau1,
                                          real &tau2)
{
    tau0 = clip(c.kp0 * (c.cp0 - q0) + c.kd0 * (c.cd0 - qd0) + c.ff0, tau_max);
    tau1 = clip(c.kp1 * (c.cp1 - q1) + c.kd1 * (c.cd1 - qd1) + c.ff1, tau_max);
    tau2 = clip(c.kp2 * (c.cp2 - q2) + c.kd2 * (c.cd2 - qd2) + c.ff2, tau_max);
}

// What an accelerometer at the base origin reads over a sub-step: before the integrator, on the rates the accelerations were computed from.
__device__ __forceinline__ v3 accelerometer(const frame3 &R, const sv6 &v0, const sv6 &afb)
{
    return (afb.l + cross(v0.a, v0.l)) + mulT(R, mk(0, 0, QR_PL_GRAVITY));
}

// One sub-step of semi-implicit Euler: rates first, then positions with the new rates.  R is the rotation the accelerations were computed in.
__device__ __forceinline__ void integrate(const frame3 &R, real h, const sv6 &afb, real qdd0, real qdd1, real qdd2, real &qw, real &qx, real &qy, real &qz,
                                          v3 &pos, sv6 &v0, real &q0, real &q1, real &q2, real &qd0, real &qd1, real &qd2)
{
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

// The state check: one non-finite value in any lane of the quad flags the robot.
__device__ __forceinline__ void state_check(int &flags, real qw, real qx, real qy, real qz, v3 pos, sv6 v0, real q0, real q1, real q2, real qd0, real qd1,
                                            real qd2)
{
    const int bad = !(isfinite(qw) && isfinite(qx) && isfinite(qy) && isfinite(qz) && finite3(pos) && finite3(v0.a) && finite3(v0.l) && isfinite(q0) &&
                      isfinite(q1) && isfinite(q2) && isfinite(qd0) && isfinite(qd1) && isfinite(qd2));
    if (quad_or(bad)) flags |= QRGPU_PL_NONFINITE;
}

// plant_out, of the last sub-step: the foot's force (world) and the motor's torque as the float32 they go out as, nu-dot.
__device__ __forceinline__ void plant_out(float *g_out, size_t N, int i, int leg, float fx, float fy, float fz, v3 foot_w, float contact, float tau0, float tau1,
                                          float tau2, sv6 afb, real qdd0, real qdd1, real qdd2)
{
    if (!g_out) return;
    const int j = 3 * leg;
    ROW(g_out, j) = fx; ROW(g_out, j + 1) = fy; ROW(g_out, j + 2) = fz;
    ROW(g_out, 12 + j) = (float)foot_w.x; ROW(g_out, 13 + j) = (float)foot_w.y; ROW(g_out, 14 + j) = (float)foot_w.z;
    ROW(g_out, 24 + leg) = contact;
    ROW(g_out, 28 + j) = tau0; ROW(g_out, 29 + j) = tau1; ROW(g_out, 30 + j) = tau2;
    ROW(g_out, 46 + j) = (float)qdd0; ROW(g_out, 47 + j) = (float)qdd1; ROW(g_out, 48 + j) = (float)qdd2;
    if (leg == 0) { ROW(g_out, 40) = (float)afb.a.x; ROW(g_out, 41) = (float)afb.a.y; ROW(g_out, 42) = (float)afb.a.z; }
    if (leg == 1) { ROW(g_out, 43) = (float)afb.l.x; ROW(g_out, 44) = (float)afb.l.y; ROW(g_out, 45) = (float)afb.l.z; }
}

// ---- What the terrain and the body kernel add to the pieces above.

// The robot's field: an id outside the stack is field 0, flagged.
__device__ __forceinline__ const float *field_in(const qrgpu_terrain_desc &T, const float *g_height, const int *g_field, int i, int &flags)
{
    int fid = g_field ? g_field[i] : 0;
    if (fid < 0 || fid >= T.n_fields) { fid = 0; flags |= QRGPU_PL_BAD_FIELD; }
    return g_height + (size_t)fid * ((size_t)T.nx * (size_t)T.ny);
}

// The wrench on the robot's base, world frame: force at the base origin, moment.  None given: zero.
__device__ __forceinline__ void push_in(const float *g_push, size_t N, int i, v3 &push_f, v3 &push_m)
{
    push_f = mk(0, 0, 0); push_m = mk(0, 0, 0);
    if (g_push) { push_f = mk(ROW(g_push, 0), ROW(g_push, 1), ROW(g_push, 2)); push_m = mk(ROW(g_push, 3), ROW(g_push, 4), ROW(g_push, 5)); }
}

// terrain_out: the ground under the foot of the state just written, its height and normal.
__device__ __forceinline__ void ground_out(float *g_tout, size_t N, int i, int leg, const float *field, const qrgpu_terrain_desc &T, real ground_z, v3 foot_w)
{
    if (!g_tout) return;
    const int j = 3 * leg;
    const terrain::Sample g = terrain::sample(field, T.nx, T.ny, (real)T.x0, (real)T.y0, (real)T.cell, foot_w.x, foot_w.y);
    const v3 nrm = terrain::normal_of(g.zx, g.zy);
    ROW(g_tout, leg) = (float)(g.z + ground_z);
    ROW(g_tout, 4 + j) = (float)nrm.x; ROW(g_tout, 5 + j) = (float)nrm.y; ROW(g_tout, 6 + j) = (float)nrm.z;
}

}  // namespace qrgpu
