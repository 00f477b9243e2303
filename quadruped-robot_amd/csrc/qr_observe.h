// A robot's sensor front-end: what qr_observe_kernel (qr_observe_kernel.hip) runs per lane -- qrRobot*::ReceiveObservation's filters, yaw logic and
// quaternion, UpdateDataFlow's foot positions, the sensor noise.  float32 where the reference is float32, its double literals promoting where they do
// there; contraction off.  Every function is __host__ __device__: the same text compiles for a CPU check against tests/observe_ref.py
// (tests/stubs/observe_host.hip, which makes the __device__ helpers of qr_wave_helpers.h host functions too).  include/qrgpu.h states the rules
// (qrgpu_observe_batch).
//   qrRobotA1Sim::ReceiveObservation      quadruped/src/robots/qr_robot_a1_sim.cpp:606-670   (qrRobotSim: qr_robot_sim.cpp:547-)
//   qrRobotA1::ReceiveObservation         quadruped/src/robots/qr_robot_a1.cpp:140-193
//   the filters, their Reset              quadruped/src/robots/qr_robot.cpp:30-37, :55-58
//   qrMovingWindowFilter<float, N>        quadruped/include/quadruped/estimators/qr_moving_window_filter.hpp:139-189
// Row k of an array lies at p[k * S]: the kernel passes the robot's column and S = n, a packed record has S = 1.
#pragma once
#include "qr_wave_helpers.h"
#include "qr_episode.h"

namespace qrgpu {
namespace observe {

// ---- d_obs_state rows.  A filter of dimension D and window W at base b: sum[D] b, correction[D] b + D, count b + 2 D, head b + 2 D + 1, the ring
// b + 2 D + 2 + D * slot + axis.  count = the deque's length, head = the slot the next push writes (once the window is full: the oldest sample's).
enum { COUNT = 0, YAW = 1, ACC = 2, GYRO = 25, RPY = 48, QD = 71, ROWS = QRGPU_OBSERVE_STATE_ROWS, ROWS_MV = QRGPU_OBSERVE_STATE_ROWS_MV };
static_assert(ROWS == QD && ROWS_MV == QD + 26 + 12 * 20, "d_obs_state layout");

// the reference's constants: M_PI of <cmath>, M_2PI of qr_ctypes.h:51 (not 2 pi)
#define QR_OBS_PI  3.14159265358979323846
#define QR_OBS_2PI 6.28318530718

// NeumaierSum (qr_moving_window_filter.hpp:151-165), one component
QR_HD void neumaier(float &sum, float &corr, float v)
{
#pragma clang fp contract(off)
    const float ns = sum + v;
    if (fabsf(sum) >= fabsf(v)) corr += (sum - ns) + v; else corr += (v - ns) + sum;
    sum = ns;
}
// CalculateAverage (:176-189), one component: cnt = the deque's length before the call, old = valueDeque[0] (read only when cnt >= W).
// -> the average; the length after the call is min(cnt + 1, W)
template <int W> QR_HD float push(float &sum, float &corr, int cnt, float old, float v)
{
#pragma clang fp contract(off)
    int len = cnt;
    if (cnt >= W) { neumaier(sum, corr, -old); len = cnt - 1; }
    neumaier(sum, corr, v);
    return (sum + corr) / (float)(len + 1);
}
// A value as loaded, or +0 under a reset (keep = 0): the load itself stays unconditional -- a select on the reset flag lets the compiler move the
// load behind a branch on it, and the flag comes from a load of its own (the mask word)
QR_HD float kept(float x, unsigned keep) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & keep); }
// A count or head row as read: an integer in [0, hi], anything else (a column that was never reset) is taken as 0 -- the head addresses memory.
QR_HD int small_int(float x, int hi) { return (x >= 0.f && x <= (float)hi) ? (int)x : 0; }

// the yaw fold (qr_robot_a1_sim.cpp:624-628, :636-640): float against the double constants
QR_HD float fold_yaw(float y)
{
#pragma clang fp contract(off)
    if ((double)y >= QR_OBS_PI) y = (float)((double)y - QR_OBS_2PI);
    else if ((double)y <= -QR_OBS_PI) y = (float)((double)y + QR_OBS_2PI);
    return y;
}

// rpyToQuat (qr_se3.h:228-235) = rotationMatrixToQuaternion(rpyToRotMat(rpy)) (:145-178), Scalar float: the trace and S as rotmat_t_to_rpy reads them
QR_HD void rpy_to_quat(const float rpy[3], float q[4])
{
#pragma clang fp contract(off)
    float M[3][3], r[3][3];
    rpy_to_rotmat(rpy, M);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) r[a][b] = M[b][a];
    const float tr = (r[0][0] + r[1][1]) + r[2][2];
    if ((double)tr > 0.0) {
        const float S = (float)(sqrt((double)tr + 1.0) * 2.0);
        q[0] = (float)(0.25 * (double)S); q[1] = (r[2][1] - r[1][2]) / S; q[2] = (r[0][2] - r[2][0]) / S; q[3] = (r[1][0] - r[0][1]) / S;
    } else if (r[0][0] > r[1][1] && r[0][0] > r[2][2]) {
        const float S = (float)(sqrt(1.0 + (double)r[0][0] - (double)r[1][1] - (double)r[2][2]) * 2.0);
        q[0] = (r[2][1] - r[1][2]) / S; q[1] = (float)(0.25 * (double)S); q[2] = (r[0][1] + r[1][0]) / S; q[3] = (r[0][2] + r[2][0]) / S;
    } else if (r[1][1] > r[2][2]) {
        const float S = (float)(sqrt(1.0 + (double)r[1][1] - (double)r[0][0] - (double)r[2][2]) * 2.0);
        q[0] = (r[0][2] - r[2][0]) / S; q[1] = (r[0][1] + r[1][0]) / S; q[2] = (float)(0.25 * (double)S); q[3] = (r[1][2] + r[2][1]) / S;
    } else {
        const float S = (float)(sqrt(1.0 + (double)r[2][2] - (double)r[0][0] - (double)r[1][1]) * 2.0);
        q[0] = (r[1][0] - r[0][1]) / S; q[1] = (r[0][2] + r[2][0]) / S; q[2] = (r[1][2] + r[2][1]) / S; q[3] = (float)(0.25 * (double)S);
    }
}

// FootPositionsInBaseFrame, one leg (qr_robot.cpp:127-146, :174-183; the formula of qr_estimator_kernel, qr_estimator_kernel.hip)
QR_HD void foot_position(const qrgpu_observe_desc &D, int leg, float t0, float t1, float t2, float p[3])
{
#pragma clang fp contract(off)
    const float sh = D.hip_l * ((leg & 1) ? 1.f : -1.f);
    const float lu = D.upper_l, ll = D.lower_l;
    const float legDist = sqrtf(lu * lu + ll * ll + 2 * lu * ll * cosf(t2));
    const float eff = t1 + t2 / 2;
    const float offX = -legDist * sinf(eff), offZ = -legDist * cosf(eff), offY = sh;
    p[0] = offX + D.hip_offset[3 * leg + 0];
    p[1] = cosf(t0) * offY - sinf(t0) * offZ + D.hip_offset[3 * leg + 1];
    p[2] = sinf(t0) * offY + cosf(t0) * offZ + D.hip_offset[3 * leg + 2];
}

// block k of robot `robot`'s noise at loop count `step` under `seed`: key (seed, robot), counter (step, k, 0x0b5e7, 0)
QR_HD episode::Words noise_block(unsigned seed, unsigned robot, unsigned step, unsigned k) { return episode::philox(step, k, 0x0b5e7u, 0u, seed, robot); }
// row += amplitude * s, s = 2 u - 1 (exact in float): one float product, one float sum
QR_HD float noised(float x, float amplitude, unsigned w)
{
#pragma clang fp contract(off)
    return x + amplitude * (float)episode::symmetric(w);
}
QR_HD void noise3(float x[3], float amplitude, const episode::Words &w)
{
    x[0] = noised(x[0], amplitude, w.w0); x[1] = noised(x[1], amplitude, w.w1); x[2] = noised(x[2], amplitude, w.w2);
}
QR_HD void noise12(const qrgpu_observe_desc &D, unsigned robot, unsigned step, unsigned first_block, float amplitude, float x[12])
{
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const episode::Words w = noise_block(D.seed, robot, step, first_block + (unsigned)b);
        x[4 * b + 0] = noised(x[4 * b + 0], amplitude, w.w0); x[4 * b + 1] = noised(x[4 * b + 1], amplitude, w.w1);
        x[4 * b + 2] = noised(x[4 * b + 2], amplitude, w.w2); x[4 * b + 3] = noised(x[4 * b + 3], amplitude, w.w3);
    }
}

// A 3-vector filter's header as loaded; under a reset: as constructed
struct Filt3 { float sum[3], corr[3]; int cnt, head; };
QR_HD Filt3 load3(const float *st, size_t S, int base, unsigned keep)
{
    Filt3 f;
#pragma unroll
    for (int a = 0; a < 3; ++a) { f.sum[a] = kept(st[(size_t)(base + a) * S], keep); f.corr[a] = kept(st[(size_t)(base + 3 + a) * S], keep); }
    f.cnt = small_int(kept(st[(size_t)(base + 6) * S], keep), 5); f.head = small_int(kept(st[(size_t)(base + 7) * S], keep), 4);
    return f;
}
QR_HD void old3(const float *st, size_t S, int base, const Filt3 &f, float old[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) old[a] = st[(size_t)(base + 8 + 3 * f.head + a) * S];
}
// CalculateAverage of v with the oldest sample `old`; header and the pushed sample go back to the state
QR_HD void average3(float *st, size_t S, int base, Filt3 &f, const float old[3], const float v[3], float avg[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        avg[a] = push<5>(f.sum[a], f.corr[a], f.cnt, old[a], v[a]);
        st[(size_t)(base + a) * S] = f.sum[a]; st[(size_t)(base + 3 + a) * S] = f.corr[a];
        st[(size_t)(base + 8 + 3 * f.head + a) * S] = v[a];
    }
    f.cnt = f.cnt >= 5 ? 5 : f.cnt + 1; f.head = (f.head + 1) % 5;
    st[(size_t)(base + 6) * S] = (float)f.cnt; st[(size_t)(base + 7) * S] = (float)f.head;
}

// ---- one robot, one call.  rst: the robot starts from a zero column (the call's scalar reset, or its mask word under a binding).  raw rows 0-40 as
// the plant writes them; prev: est_out of the previous tick or null; est may be raw itself: every raw row is loaded before the first store.
// rows = the rows of st the caller allocated (ROWS or ROWS_MV, by D.filter_motor_velocity).  gin, tick may be null.
// Loads come first and do not wait for one another: raw rows, the filters' headers, the previous yaw, the counter, prev; then the ring slots the
// headers name (one per axis); then arithmetic and stores.  No && or early exit between loads (qr_episode.h: state_finite).
QR_HD void step(const qrgpu_observe_desc &D, bool rst, unsigned robot, unsigned stepno, size_t S, const float *raw, const float *prev, float *__restrict__ st,
                float *est, float *__restrict__ rpy_out, float *__restrict__ gin, unsigned *__restrict__ tick)
{
#pragma clang fp contract(off)
    const bool mv = D.filter_motor_velocity != 0;
    const unsigned keep = rst ? 0u : 0xffffffffu;
    float acc[3], quat[4], gyro[3], ct[4], q[12], qd[12];
#pragma unroll
    for (int a = 0; a < 3; ++a) { acc[a] = raw[(size_t)a * S]; gyro[a] = raw[(size_t)(10 + a) * S]; }
#pragma unroll
    for (int a = 0; a < 4; ++a) { quat[a] = raw[(size_t)(6 + a) * S]; ct[a] = raw[(size_t)(13 + a) * S]; }
#pragma unroll
    for (int j = 0; j < 12; ++j) { q[j] = raw[(size_t)(17 + j) * S]; qd[j] = raw[(size_t)(29 + j) * S]; }
    Filt3 fa = load3(st, S, ACC, keep), fg = load3(st, S, GYRO, keep), fr = load3(st, S, RPY, keep);
    const float yaw_prev = kept(st[(size_t)YAW * S], keep);
    const unsigned count = __builtin_bit_cast(unsigned, kept(st[(size_t)COUNT * S], keep)) + 1u;
    float bp[3] = {0.f, 0.f, D.base_height};                                  // qrRobot::Reset: basePosition (qr_robot.cpp:53)
    if (prev) {
        bp[0] = kept(prev[(size_t)36 * S], keep); bp[1] = kept(prev[(size_t)37 * S], keep);
        bp[2] = __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, prev[(size_t)38 * S]) & keep) | (__builtin_bit_cast(unsigned, D.base_height) & ~keep));
    }
    float vs[12], vc[12];
    int vcnt = 0, vhead = 0;
    if (mv) {
#pragma unroll
        for (int j = 0; j < 12; ++j) { vs[j] = kept(st[(size_t)(QD + j) * S], keep); vc[j] = kept(st[(size_t)(QD + 12 + j) * S], keep); }
        vcnt = small_int(kept(st[(size_t)(QD + 24) * S], keep), 20); vhead = small_int(kept(st[(size_t)(QD + 25) * S], keep), 19);
    }
    // the slots the headers name
    float oa[3], og[3], orp[3], ov[12];
    old3(st, S, ACC, fa, oa); old3(st, S, GYRO, fg, og); old3(st, S, RPY, fr, orp);
    if (mv) {
#pragma unroll
        for (int j = 0; j < 12; ++j) ov[j] = st[(size_t)(QD + 26 + 12 * vhead + j) * S];
    }
    // a reset robot's column is zero before the call writes to it: the slots this call does not touch, too
    if (rst) {
        const int rows = mv ? ROWS_MV : ROWS;
        for (int k = 0; k < rows; ++k) st[(size_t)k * S] = 0.f;
    }
    // ---- noise (OURS): blocks 0 acc, 1 gyro, 2-4 q, 5-7 qd; an amplitude of 0 leaves the rows' bits alone
    if (D.acc_noise != 0.f) noise3(acc, D.acc_noise, noise_block(D.seed, robot, stepno, 0u));
    if (D.gyro_noise != 0.f) noise3(gyro, D.gyro_noise, noise_block(D.seed, robot, stepno, 1u));
    if (D.q_noise != 0.f) noise12(D, robot, stepno, 2u, D.q_noise, q);
    if (D.qd_noise != 0.f) noise12(D, robot, stepno, 5u, D.qd_noise, qd);
    // ---- accelerometer and its window of 5 (qr_robot_a1_sim.cpp:615-618)
    float facc[3];
    average3(st, S, ACC, fa, oa, acc, facc);
    // ---- roll, pitch, yaw (:620-640; qr_robot_a1.cpp:155-162): state.imu.rpy = quatToRPY of the raw quaternion
    float rpy[3];
    quat_to_rpy(quat, rpy);
    const float cy = fold_yaw(rpy[2] - D.yaw_offset);
    rpy[2] = cy;
    if (D.filter_rpy) {
        if ((double)fabsf(yaw_prev - cy) >= QR_OBS_PI) {                       // rpyFilter.Reset() (:630-632): abs read as std::abs(float)
#pragma unroll
            for (int a = 0; a < 3; ++a) fr.sum[a] = fr.corr[a] = 0.f;
            fr.cnt = 0; fr.head = 0;
        }
        const float in[3] = {rpy[0], rpy[1], cy};
        average3(st, S, RPY, fr, orp, in, rpy);
        rpy[2] = fold_yaw(rpy[2]);
    }
    st[(size_t)YAW * S] = rpy[2];
    float bq[4];
    rpy_to_quat(rpy, bq);                                                     // baseOrientation (:648; qr_robot_a1.cpp:163)
    // ---- gyro (:642-645)
    float fgyro[3];
    average3(st, S, GYRO, fg, og, gyro, fgyro);
    // ---- motor velocities: motorVFilter, window 20 (qr_robot_a1.cpp:176), or as read
    float fqd[12];
    if (mv) {
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            fqd[j] = push<20>(vs[j], vc[j], vcnt, ov[j], qd[j]);
            st[(size_t)(QD + j) * S] = vs[j]; st[(size_t)(QD + 12 + j) * S] = vc[j];
            st[(size_t)(QD + 26 + 12 * vhead + j) * S] = qd[j];
        }
        st[(size_t)(QD + 24) * S] = (float)(vcnt >= 20 ? 20 : vcnt + 1); st[(size_t)(QD + 25) * S] = (float)((vhead + 1) % 20);
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) fqd[j] = qd[j];
    }
    st[(size_t)COUNT * S] = __builtin_bit_cast(float, count);
    // ---- est_in rows 0-40; 41-53 belong to the gait and the ground stage
#pragma unroll
    for (int a = 0; a < 3; ++a) { est[(size_t)a * S] = acc[a]; est[(size_t)(3 + a) * S] = facc[a]; est[(size_t)(10 + a) * S] = fgyro[a]; rpy_out[(size_t)a * S] = rpy[a]; }
#pragma unroll
    for (int a = 0; a < 4; ++a) { est[(size_t)(6 + a) * S] = bq[a]; est[(size_t)(13 + a) * S] = ct[a]; }
#pragma unroll
    for (int j = 0; j < 12; ++j) { est[(size_t)(17 + j) * S] = q[j]; est[(size_t)(29 + j) * S] = fqd[j]; }
    // ---- the ground stage's input: contacts, FootPositionsInBaseFrame(motorAngles) (UpdateDataFlow, qr_robot.cpp:68), basePosition, baseOrientation
    if (gin) {
#pragma unroll
        for (int a = 0; a < 4; ++a) { gin[(size_t)a * S] = ct[a]; gin[(size_t)(19 + a) * S] = bq[a]; }
#pragma unroll
        for (int leg = 0; leg < 4; ++leg) {
            float p[3];
            foot_position(D, leg, q[3 * leg], q[3 * leg + 1], q[3 * leg + 2], p);
            gin[(size_t)(4 + 3 * leg) * S] = p[0]; gin[(size_t)(5 + 3 * leg) * S] = p[1]; gin[(size_t)(6 + 3 * leg) * S] = p[2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) gin[(size_t)(16 + a) * S] = bp[a];
    }
    if (tick) *tick = count * D.tick_ms;
}

}  // namespace observe
}  // namespace qrgpu
