// ============================================================================
// qr_episode_kernel: per-robot termination, reset and spawn (qrgpu_episode_step_batch, include/qrgpu.h); the arithmetic is qr_episode.h's.
//
// One lane per robot, 64 lanes (one wavefront) per workgroup.  Every array is [row][n], robot index fastest: each load and store of a wavefront is
// one coalesced row segment.  A lane reads its status words and counters, reads its 37 state rows once (finite?  quaternion and position kept),
// decides, and -- where the episode ends -- closes the statistics, draws the spawn (five Philox blocks, sixteen plain global loads of the
// L2-resident field) and writes state, prev_ori and the motor command.  No LDS, no barrier, no runtime-indexed local array.  A lane past n stores
// nothing.
// Compaction of the reset robots: one __ballot per wavefront, a lane's slot = population count of the ballot below the lane, ONE atomic add per
// wavefront that has a reset (by its first reset lane, the base handed round with __shfl): the list's order across wavefronts is unspecified.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_kernels.h"
#include "qr_episode.h"

namespace qrgpu {

__global__ void __launch_bounds__(64) qr_episode_kernel(int n, qrgpu_episode_desc D, double cos_tilt, int reset_all, float ground_z, int has_terrain, qrgpu_terrain_desc T,
                                                        const float *__restrict__ g_height, const int *__restrict__ g_field, const float *__restrict__ g_spawn,
                                                        int n_spawn, const int *__restrict__ g_pstatus, const int *__restrict__ g_tstatus,
                                                        const int *__restrict__ g_force, float *__restrict__ g_state, float *__restrict__ g_prev,
                                                        float *__restrict__ g_cmd, int *__restrict__ g_st, float *__restrict__ g_stats, int *__restrict__ g_done,
                                                        int *__restrict__ g_list, int *__restrict__ g_count)
{
    const int lane = (int)threadIdx.x;
    const int r = (int)blockIdx.x * 64 + lane;
    const bool live = r < n;
    const size_t N = (size_t)n, i = (size_t)(live ? r : n - 1);
    bool reset = false;
    if (live) {
        int flags = 0, fid = 0;
        if (has_terrain) {
            fid = g_field ? g_field[i] : 0;
            if (fid < 0 || fid >= T.n_fields) { fid = 0; flags = QRGPU_EP_BAD_FIELD; }
        }
        const episode::Ground G = episode::ground_of(has_terrain != 0, T, g_height, fid, ground_z);
        episode::Book b;
        memset(&b, 0, sizeof(b));
        int reason = QRGPU_EP_FORCED;
        real px = 0, py = 0;
        bool finite = true;
        if (!reset_all) {
            b.ticks = g_st[i]; b.epi = g_st[N + i]; b.deb = g_st[2 * N + i];
            b.run_min = g_stats[8 * N + i];
            const real qw = g_state[i], qx = g_state[N + i], qy = g_state[2 * N + i], qz = g_state[3 * N + i];
            px = g_state[4 * N + i]; py = g_state[5 * N + i];
            const real pz = g_state[6 * N + i];
            finite = episode::state_finite(g_state + i, N);
            const episode::Verdict v = episode::decide(D, cos_tilt, G, g_pstatus ? g_pstatus[i] : 0, g_tstatus ? g_tstatus[i] : 0, g_force ? g_force[i] : 0,
                                                       finite, qw, qx, qy, qz, px, py, pz, b.deb, b.ticks);
            reason = v.reason;
            episode::note_clearance(b, finite, v.clearance);
        }
        reset = reason != 0;
        g_done[i] = reason | flags;
        if (!reset) {
            g_st[i] = b.ticks; g_st[2 * N + i] = b.deb;
            g_stats[8 * N + i] = (float)b.run_min;
        } else {
            if (!reset_all) {                                  // close the episode that ends here
                b.n_fail = g_st[4 * N + i]; b.n_time = g_st[5 * N + i];
                b.sx = g_stats[i]; b.sy = g_stats[N + i];
                episode::close_episode(b, reason, finite, px, py);
            }
            const episode::Spawn s = episode::spawn(D, G, g_spawn, n_spawn, (unsigned)r, (unsigned)b.epi);
            episode::open_episode(b, s, (real)D.spawn_height);
            g_st[i] = b.ticks; g_st[N + i] = b.epi; g_st[2 * N + i] = b.deb; g_st[3 * N + i] = b.last; g_st[4 * N + i] = b.n_fail; g_st[5 * N + i] = b.n_time;
            g_stats[i] = (float)b.sx; g_stats[N + i] = (float)b.sy; g_stats[2 * N + i] = (float)b.sz; g_stats[3 * N + i] = (float)b.syaw;
            g_stats[4 * N + i] = (float)b.len; g_stats[5 * N + i] = (float)b.dx; g_stats[6 * N + i] = (float)b.dy; g_stats[7 * N + i] = (float)b.last_min;
            g_stats[8 * N + i] = (float)b.run_min;
            g_state[i] = (float)s.qw; g_state[N + i] = (float)s.qx; g_state[2 * N + i] = (float)s.qy; g_state[3 * N + i] = (float)s.qz;
            g_state[4 * N + i] = (float)s.x; g_state[5 * N + i] = (float)s.y; g_state[6 * N + i] = (float)s.z;
#pragma unroll
            for (int k = 7; k < 13; ++k) g_state[(size_t)k * N + i] = 0.f;
            g_state[10 * N + i] = (float)s.vx; g_state[11 * N + i] = (float)s.vy;
#pragma unroll
            for (int k = 0; k < 12; ++k) { g_state[(size_t)(13 + k) * N + i] = (float)s.q[k]; g_state[(size_t)(25 + k) * N + i] = 0.f; }
            if (g_prev) { g_prev[i] = 0.f; g_prev[N + i] = 0.f; g_prev[2 * N + i] = 0.f; }
            if (g_cmd) {
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    g_cmd[(size_t)k * N + i] = (float)s.q[k]; g_cmd[(size_t)(12 + k) * N + i] = D.kp; g_cmd[(size_t)(24 + k) * N + i] = 0.f;
                    g_cmd[(size_t)(36 + k) * N + i] = D.kd; g_cmd[(size_t)(48 + k) * N + i] = 0.f;
                }
            }
        }
    }
    // the robots reset in this call, compacted (every lane of the wavefront is here)
    const unsigned long long m = __ballot(reset);
    if (g_count && m != 0ull) {
        const int first = __ffsll((long long)m) - 1;
        int base = 0;
        if (lane == first) base = atomicAdd(g_count, __popcll(m));
        base = __shfl(base, first);
        if (reset && g_list) g_list[base + __popcll(m & ((1ull << lane) - 1ull))] = r;
    }
}

}  // namespace qrgpu
