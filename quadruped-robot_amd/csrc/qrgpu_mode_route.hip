// ============================================================================
// libqrgpu.so host side: the locomotion mode per robot (qr_mode_route_kernel.hip) -- the route from each robot's mode to its chain, the binding the
// cadenced tick and the force-balance QP launch read it through, the merge of the two chains' motor commands -- and the default route table.
// Every launching entry point is "check the arguments, one launch on the context's stream" (qrgpu_dataflow.hip); the route zeroes its three counters
// on the stream first.
// ============================================================================
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>

#include "qrgpu_ctx.h"

static int mr_bad(qrgpu_ctx *c, const char *call, const char *what)
{
    if (c) c->err = std::string(call) + ": " + what;
    return QRGPU_ERR_BAD_ARG;
}

static bool mr_chain_ok(int v) { return v >= QRGPU_CHAIN_NONE && v <= QRGPU_CHAIN_FORCE_BALANCE; }

extern "C" {

void qrgpu_mode_route_desc_default(qrgpu_mode_route_desc *d)
{   // qr_fsm_state_locomotion.cpp:78-158: JOY_TROT runs the force-balance chain, JOY_ADVANCED_TROT the MPC chain; the POSITION and WALK chains are not closed
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->chain_of_mode[QRGPU_MODE_VELOCITY] = QRGPU_CHAIN_FORCE_BALANCE;
    d->chain_of_mode[QRGPU_MODE_POSITION] = QRGPU_CHAIN_NONE;
    d->chain_of_mode[QRGPU_MODE_WALK] = QRGPU_CHAIN_NONE;
    d->chain_of_mode[QRGPU_MODE_ADVANCED_TROT] = QRGPU_CHAIN_MPC;
    d->fallback_chain = QRGPU_CHAIN_MPC;
}

int qrgpu_mode_route_batch(qrgpu_ctx *c, int n, const qrgpu_mode_route_desc *desc, const float *d_mode_sel, const int *d_plan, int *d_chain, int *d_route_flags,
                           int *d_chain_count)
{
    static const char *const me = "qrgpu_mode_route_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return mr_bad(c, me, "n");
    if (!desc) return mr_bad(c, me, "desc");
    for (int m = 0; m < 4; ++m)
        if (!mr_chain_ok(desc->chain_of_mode[m])) return mr_bad(c, me, "desc->chain_of_mode");
    if (!mr_chain_ok(desc->fallback_chain)) return mr_bad(c, me, "desc->fallback_chain");
    if (!d_mode_sel) return mr_bad(c, me, "d_mode_sel");
    if (!d_chain) return mr_bad(c, me, "d_chain");
    c->ov_chain = false;                                             // another launch of the context: the next overlapped tick is not chained
    HIPCHK(c, hipSetDevice(c->device));
    if (d_chain_count) HIPCHK(c, hipMemsetAsync(d_chain_count, 0, 3 * sizeof(int), c->stream));
    hipLaunchKernelGGL(qr_mode_route_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, *desc, d_mode_sel, d_plan, d_chain, d_route_flags, d_chain_count);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

int qrgpu_set_mode_route(qrgpu_ctx *c, const int *d_chain)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    c->mode_chain = d_chain;
    return QRGPU_OK;
}

int qrgpu_mode_command_batch(qrgpu_ctx *c, int n, const int *d_chain, const float *d_cmd_mpc, const float *d_cmd_fb, const int *d_status_mpc, const int *d_status_fb,
                             float *d_motor_cmd, int *d_status)
{
    static const char *const me = "qrgpu_mode_command_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return mr_bad(c, me, "n");
    if (!d_chain) return mr_bad(c, me, "d_chain");
    if (!d_cmd_mpc) return mr_bad(c, me, "d_cmd_mpc");
    if (!d_cmd_fb) return mr_bad(c, me, "d_cmd_fb");
    if (!d_motor_cmd) return mr_bad(c, me, "d_motor_cmd");
    c->ov_chain = false;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_mode_command_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, d_chain, d_cmd_mpc, d_cmd_fb, d_status_mpc, d_status_fb, d_motor_cmd,
                       d_status);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

}  // extern "C"
