// ============================================================================
// qr_gait_kernel, qr_gait_select_kernel, qr_stage_clock_kernel: the open-loop gait generator with one gait for the launch and with the gait chosen per
// robot, and the stage clock that restarts where a mask says (qrgpu_gait_update_batch, qrgpu_gait_select_update_batch, qrgpu_stage_clock_batch,
// include/qrgpu.h); the arithmetic is qr_gait.h's, written once for both gait kernels and for the CPU check.
//
// One lane per robot, 64 lanes (one wavefront) per workgroup.  Every array is [row][n], robot index fastest: each load and store of a wavefront is
// one coalesced row segment.  qr_gait_kernel takes its one gait by value in the kernel arguments: uniform, read with scalar loads.  The gait table of
// qr_gait_select_kernel lies in device memory (the context's copy): a lane reads the 19 words of its entry with its own index, plain global loads -- a
// table passed by value in the kernel arguments and indexed per lane would be copied to private memory first.  A lane loads its state column, its
// selection and its mask word up front, not behind a branch on the mask; a reset then overrides what its level does not keep.
// No LDS, no barrier, no cross-lane traffic, no scratch.  A lane past n does nothing.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_kernels.h"
#include "qr_gait.h"

namespace qrgpu {

// State [52][n] floats (rows in qr_gait.h); `fresh` = QRGPU_GAIT_RESET_LIVE applies Reset(0) to the running generator first, any other non-zero
// value starts from a generator as constructed (the state's content is not read).  Rows 48-51 are neither read nor written.
__global__ void __launch_bounds__(64) qr_gait_kernel(int n, qrgpu_gait_desc D, float currentTime, int stop, int fresh, const float *__restrict__ g_contact,
                                                     float *__restrict__ st, float *__restrict__ g_out, float *__restrict__ g_fe, StageResetArgs SR)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    // the lane's own reset level and clock: the call's scalar reset wins, then the bound level of a masked robot
    const bool masked = stage_masked(SR, i);
    const int level = fresh ? fresh : masked ? SR.level : 0;
    gait::fixed_update(D, level, stage_time(SR, i, currentTime), stop, (size_t)n, g_contact + i, st + i, g_out ? g_out + i : nullptr,
                       g_fe ? g_fe + i : nullptr);
}

__global__ void __launch_bounds__(64) qr_gait_select_kernel(int n, const qrgpu_gait_desc *__restrict__ g_table, int n_gaits, const float *__restrict__ g_sel,
                                                            float currentTime, int stop, int fresh, const float *__restrict__ g_contact,
                                                            float *__restrict__ st, float *__restrict__ g_out, float *__restrict__ g_fe,
                                                            float *__restrict__ g_sw, int *__restrict__ g_flags, StageResetArgs SR)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    // the lane's own reset level and clock: the call's scalar reset wins, then the bound level of a masked robot
    const bool masked = stage_masked(SR, i);
    const float sel = g_sel[i];
    const int level = fresh ? fresh : masked ? SR.level : 0;
    gait::select_update(g_table, n_gaits, sel, level, stage_time(SR, i, currentTime), stop, (size_t)n, g_contact + i, st + i, g_out ? g_out + i : nullptr,
                        g_fe ? g_fe + i : nullptr, g_sw ? g_sw + i : nullptr, g_flags ? g_flags + i : nullptr);
}

__global__ void __launch_bounds__(64) qr_stage_clock_kernel(int n, const int *__restrict__ g_mask, unsigned bits, const int *__restrict__ g_ticks,
                                                            int *__restrict__ g_origin, int *__restrict__ g_local)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    gait::stage_clock(g_mask[i], bits, g_ticks[i], g_origin + i, g_local + i);
}

}  // namespace qrgpu
