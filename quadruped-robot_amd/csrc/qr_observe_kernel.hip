// ============================================================================
// qr_observe_kernel: the robot classes' sensor front-end, qrRobot*::ReceiveObservation (qrgpu_observe_batch, include/qrgpu.h); the arithmetic is
// qr_observe.h's.
//
// One lane per robot, 64 lanes (one wavefront) per workgroup.  Every array is [row][n], robot index fastest: each load and store of a wavefront is
// one coalesced row segment; a filter's ring is [slot][axis][n], so a tick touches one slot per axis.  A lane loads its mask word, its 41 raw rows,
// the filters' headers, the previous yaw, the counter and the previous base position without waiting for any of them, then the ring slots the
// headers name, then computes and stores: two memory latencies, the second for the slots.  g_est_in may be g_raw (no __restrict__ on the pair):
// every raw row is in registers before the first store.  The stage-reset binding comes as an argument always (a null mask: unbound); only its mask
// is read.  No LDS, no barrier, no cross-lane traffic.  A lane past n does nothing.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_kernels.h"
#include "qr_observe.h"

namespace qrgpu {

__global__ void __launch_bounds__(64) qr_observe_kernel(int n, qrgpu_observe_desc D, int reset, unsigned step, StageResetArgs SR, const float *g_raw, const float *g_prev,
                                                        float *__restrict__ g_st, float *g_est_in, float *__restrict__ g_rpy, float *__restrict__ g_ground_in,
                                                        unsigned *__restrict__ g_tick)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    // the mask word's load is the first of the lane's loads, not a gate in front of them: no branch on the binding -- unbound, the lane reads a word of
    // its own raw column instead and holds it against bits 0
    const unsigned *mp = SR.mask ? (const unsigned *)SR.mask + i : (const unsigned *)g_raw + i;
    const unsigned bits = SR.mask ? SR.bits : 0u;
    const bool rst = (reset != 0) | ((*mp & bits) != 0u);
    observe::step(D, rst, (unsigned)i, step, (size_t)n, g_raw + i, g_prev ? g_prev + i : nullptr, g_st + i, g_est_in + i, g_rpy + i,
                  g_ground_in ? g_ground_in + i : nullptr, g_tick ? g_tick + i : nullptr);
}

}  // namespace qrgpu
