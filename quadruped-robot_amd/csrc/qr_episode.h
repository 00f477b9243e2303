// A robot's episode step: when its episode ends, the random numbers of its next spawn, the spawn itself.  What qr_episode_kernel
// (qr_episode_kernel.hip) runs per lane.  fp64 on the fp32 arrays.  Every function is __host__ __device__: the same text compiles for a CPU check
// against tests/episode_ref.py (tests/stubs/episode_host.hip).  include/qrgpu.h states the rules (qrgpu_episode_step_batch).  The ground is
// qr_terrain.h's: terrain::sample and terrain::normal_of, no second sampler.
#pragma once
#include "qr_device_types.h"
#include "qr_terrain.h"

namespace qrgpu {
namespace episode {

// ---- Philox-4x32-10 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1) -> four words
struct Words { unsigned w0, w1, w2, w3; };
QR_HD Words philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * (unsigned long long)c0, p1 = 0xCD9E8D57ull * (unsigned long long)c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Words o = {c0, c1, c2, c3};
    return o;
}
// block k of robot `robot`'s episode `epi` under `seed`: key (seed, robot), counter (epi, k, 0, 0)
QR_HD Words block(unsigned seed, unsigned robot, unsigned epi, unsigned k) { return philox(epi, k, 0u, 0u, seed, robot); }
// u = (word >> 8) 2^-24 in [0, 1), exact in float, widened;  s = 2 u - 1 in [-1, 1)
QR_HD real uniform(unsigned w) { return (real)((float)(w >> 8) * 5.9604644775390625e-08f); }
QR_HD real symmetric(unsigned w) { return 2.0 * uniform(w) - 1.0; }

// ---- the ground under a point: the robot's field (or none: flat at ground_z)
struct Ground { bool has; const float *field; int nx, ny; real x0, y0, cell, ground_z; };
QR_HD Ground ground_of(bool has, const qrgpu_terrain_desc &T, const float *height, int fid, float ground_z)
{
    Ground g;
    g.has = has; g.nx = T.nx; g.ny = T.ny; g.x0 = T.x0; g.y0 = T.y0; g.cell = T.cell; g.ground_z = ground_z;
    g.field = has ? height + (size_t)fid * ((size_t)T.nx * (size_t)T.ny) : nullptr;
    return g;
}

// Are the robot's 37 state rows all finite?  row k lies at state[k * stride] (the kernel: stride n, the robot's column; a packed record: 1).
// & and not &&: a short-circuit would make each row's load wait for the verdict on the row before it -- a chain of memory latencies.
QR_HD bool state_finite(const float *state, size_t stride)
{
    int fin = 1;
#pragma unroll
    for (int k = 0; k < 37; ++k) { const float x = state[(size_t)k * stride]; fin &= (int)(x - x == 0.0f); }      // (Inf - Inf and NaN - NaN are NaN)
    return fin != 0;
}

// the bound R_zz is held against: cos(tilt_max); a tilt_max of pi or more bounds nothing (R_zz >= -1 > -2)
inline double cos_tilt_of(float tilt_max) { return tilt_max >= 3.14159265f ? -2.0 : cos((double)tilt_max); }

// ---- termination.  q, p: the quaternion and the base position as read; finite: all 37 rows are finite.  deb, ticks: the robot's debounce and tick
// counters, advanced here.  -> reason bits (QRGPU_EP_STATUS .. QRGPU_EP_FORCED); rzz, clearance, margin: the continuous criteria (0 when not judged).
struct Verdict { int reason; real rzz, clearance, margin; };
QR_HD Verdict decide(const qrgpu_episode_desc &D, real cos_tilt, const Ground &G, int plant_status, int tick_status, int forced, bool finite,
                     real qw, real qx, real qy, real qz, real px, real py, real pz, int &deb, int &ticks)
{
    Verdict v;
    v.reason = 0; v.rzz = 0.0; v.clearance = 0.0; v.margin = 0.0;
    deb = (plant_status & D.status_mask) ? (deb < 0x7fffffff ? deb + 1 : deb) : 0;
    ticks = ticks < 0x7fffffff ? ticks + 1 : ticks;
    if (deb >= D.status_ticks) v.reason |= QRGPU_EP_STATUS;
    if (tick_status & D.tick_mask) v.reason |= QRGPU_EP_TICK_STATUS;
    if (D.max_ticks > 0 && ticks >= D.max_ticks) v.reason |= QRGPU_EP_TIMEOUT;
    if (forced) v.reason |= QRGPU_EP_FORCED;
    if (!finite) { v.reason |= QRGPU_EP_NONFINITE; return v; }
    const real n2 = (qw * qw + qx * qx) + (qy * qy + qz * qz);
    v.rzz = n2 > 0.0 ? 1.0 - 2.0 * (qx * qx + qy * qy) / n2 : 1.0;       // a zero quaternion is read as the identity, as the plant reads it
    if (v.rzz < cos_tilt) v.reason |= QRGPU_EP_TILT;
    real zg = G.ground_z;
    if (G.has) {
        zg += terrain::sample(G.field, G.nx, G.ny, G.x0, G.y0, G.cell, px, py).z;
        const real m = D.field_margin;
        const real x1 = G.x0 + (real)(G.nx - 1) * G.cell, y1 = G.y0 + (real)(G.ny - 1) * G.cell;
        v.margin = fmin(fmin(px - (G.x0 + m), (x1 - m) - px), fmin(py - (G.y0 + m), (y1 - m) - py));
        if (v.margin < 0.0) v.reason |= QRGPU_EP_OFF_FIELD;
    }
    v.clearance = pz - zg;
    if (v.clearance < (real)D.min_clearance) v.reason |= QRGPU_EP_HEIGHT;
    return v;
}

// ---- spawn of robot `robot`'s episode `epi`: table d_spawn [4][n_spawn] (x, y, yaw, reserved)
struct Spawn { real qw, qx, qy, qz, x, y, z, yaw, vx, vy; real q[12]; };
QR_HD Spawn spawn(const qrgpu_episode_desc &D, const Ground &G, const float *table, int n_spawn, unsigned robot, unsigned epi)
{
    Spawn s;
    const Words b0 = block(D.seed, robot, epi, 0u), b1 = block(D.seed, robot, epi, 1u);
    int row = (int)floor(uniform(b0.w0) * (real)n_spawn);
    row = row > n_spawn - 1 ? n_spawn - 1 : row;
    s.x = (real)table[row] + (real)D.xy_jitter * symmetric(b0.w1);
    s.y = (real)table[(size_t)n_spawn + row] + (real)D.xy_jitter * symmetric(b0.w2);
    s.yaw = (real)table[2 * (size_t)n_spawn + row] + (real)D.yaw_jitter * symmetric(b0.w3);
    s.vx = (real)D.v_jitter * symmetric(b1.w0);
    s.vy = (real)D.v_jitter * symmetric(b1.w1);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const Words w = block(D.seed, robot, epi, 2u + (unsigned)b);
        s.q[4 * b + 0] = (real)D.q_spawn[4 * b + 0] + (real)D.q_jitter * symmetric(w.w0);
        s.q[4 * b + 1] = (real)D.q_spawn[4 * b + 1] + (real)D.q_jitter * symmetric(w.w1);
        s.q[4 * b + 2] = (real)D.q_spawn[4 * b + 2] + (real)D.q_jitter * symmetric(w.w2);
        s.q[4 * b + 3] = (real)D.q_spawn[4 * b + 3] + (real)D.q_jitter * symmetric(w.w3);
    }
    // the ground at the spawn point, the base spawn_height along its normal
    real zg = G.ground_z;
    v3 n = mk(0.0, 0.0, 1.0);
    if (G.has) {
        const terrain::Sample g = terrain::sample(G.field, G.nx, G.ny, G.x0, G.y0, G.cell, s.x, s.y);
        zg += g.z;
        n = terrain::normal_of(g.zx, g.zy);
    }
    const real h = D.spawn_height;
    s.z = zg + h * n.z;
    s.x += h * n.x; s.y += h * n.y;
    // attitude: (the shortest rotation of e_z onto n) (x) (yaw about z) -- the base z axis is n; level: the yaw alone
    const real c = cos(0.5 * s.yaw), sn = sin(0.5 * s.yaw);
    real a0 = 1.0, a1 = 0.0, a2 = 0.0;
    if (D.align_to_slope) { a0 = 1.0 + n.z; a1 = -n.y; a2 = n.x; }
    real w = a0 * c, x = a1 * c + a2 * sn, y = a2 * c - a1 * sn, z = a0 * sn;
    real inv = 1.0 / sqrt((w * w + x * x) + (y * y + z * z));
    if (w < 0.0) inv = -inv;
    s.qw = w * inv; s.qx = x * inv; s.qy = y * inv; s.qz = z * inv;
    return s;
}

// ---- bookkeeping: the rows of d_ep_state (ticks .. n_time) and of d_ep_stats (sx .. run_min) of one robot
struct Book { int ticks, epi, deb, last, n_fail, n_time; real sx, sy, sz, syaw, len, dx, dy, last_min, run_min; };
// a call that judged the clearance
QR_HD void note_clearance(Book &b, bool finite, real clearance) { if (finite) b.run_min = fmin(b.run_min, clearance); }
// the episode ends with `reason` at base position (px, py)
QR_HD void close_episode(Book &b, int reason, bool finite, real px, real py)
{
    if (reason == QRGPU_EP_TIMEOUT) ++b.n_time; else ++b.n_fail;
    b.last = reason; b.len = (real)b.ticks; b.last_min = b.run_min;
    b.dx = finite ? px - b.sx : 0.0; b.dy = finite ? py - b.sy : 0.0;
    ++b.epi;
}
// the next one starts at s
QR_HD void open_episode(Book &b, const Spawn &s, real spawn_height)
{
    b.ticks = 0; b.deb = 0;
    b.sx = s.x; b.sy = s.y; b.sz = s.z; b.syaw = s.yaw; b.run_min = spawn_height;
}

}  // namespace episode
}  // namespace qrgpu
