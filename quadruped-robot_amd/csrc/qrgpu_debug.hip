// ============================================================================
// libqrgpu.so host side: diagnostics.  The undocumented qrgpu_debug_* read-outs (cycle stamps, list lengths, counters, the timeline buffer of
// -DQR_TIMELINE builds: its layout is QR_TL_* in qr_device_types.h), the cross-lane self-test and the executed-arithmetic counters.
// ============================================================================
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>

#include "qrgpu_ctx.h"

extern "C" {

int qrgpu_debug_cycles(qrgpu_ctx *c, long long *host_out /* [n][8] or NULL to disable */, int n)
{   // undocumented diagnostic: phase cycle stamps of the last MPC launch (enable by calling once with NULL first; NULL with n < 0 switches them off again)
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!host_out && n < 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(c->d_dbg_cycles);
        (void)hipFree(c->d_dbg_cycles_wbc);
        c->d_dbg_cycles = nullptr; c->d_dbg_cycles_wbc = nullptr;
        return QRGPU_OK;
    }
    if (!c->d_dbg_cycles) {
        HIPCHK(c, hipMalloc(&c->d_dbg_cycles, sizeof(long long) * 16 * (size_t)c->max_batch));
        HIPCHK(c, hipMalloc(&c->d_dbg_cycles_wbc, sizeof(long long) * 16 * (size_t)(c->max_batch + 8)));
        return QRGPU_OK;
    }
    if (host_out && n < 0) {   // n < 0: fetch the WBC kernel's stamps instead (indexed by workgroup)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(host_out, c->d_dbg_cycles_wbc, sizeof(long long) * 16 * (size_t)(-n), hipMemcpyDeviceToHost));
        return QRGPU_OK;
    }
    if (host_out) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipMemcpy(host_out, c->d_dbg_cycles, sizeof(long long) * 16 * (size_t)n, hipMemcpyDeviceToHost)); }
    return QRGPU_OK;
}

int qrgpu_debug_lists(qrgpu_ctx *c, int *host_out /* [8]: rescue list lengths (both parities), planned list lengths (both parities), "go" count and the
                                                      plan epoch of a planned launch whose gate gave up, the tick epoch of a WBC gate that gave up, the context's plan epoch */)
{   // undocumented diagnostic: how many robots the last MPC launches handed to the trailing list launch / planned for the next call; which gates gave up
    if (!c || !host_out) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // (the lane the context's last launch ran on; the give-up words are rings indexed by epoch: the latest epoch in each is reported)
    const Lane &L = c->lane[c->ov_chain ? c->ov_lane_last : 0];
    HIPCHK(c, hipMemcpy(host_out, L.d_rescue, 2 * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(host_out + 2, L.d_pre, 2 * sizeof(int), hipMemcpyDeviceToHost));
    int ring[1 + QR_ABORT_RING];
    HIPCHK(c, hipMemcpy(ring, L.d_go, sizeof(ring), hipMemcpyDeviceToHost));
    host_out[4] = ring[0]; host_out[5] = 0;
    for (int i = 1; i <= QR_ABORT_RING; ++i) if (ring[i] > host_out[5]) host_out[5] = ring[i];
    HIPCHK(c, hipMemcpy(ring, c->d_gate_abort, QR_ABORT_RING * sizeof(int), hipMemcpyDeviceToHost));
    host_out[6] = 0;
    for (int i = 0; i < QR_ABORT_RING; ++i) if (ring[i] > host_out[6]) host_out[6] = ring[i];
    host_out[7] = L.plan_epoch;
    return QRGPU_OK;
}

int qrgpu_debug_counters(qrgpu_ctx *c, int *host_out /* [12]: device count / host total of main_started, wbc_finished, tick_done, lane_done of lanes 1 and 2, epoch */)
{   // undocumented diagnostic: the cumulative counters the gates and joins poll, as the device and the host see them
    if (!c || !host_out) return QRGPU_ERR_BAD_ARG;
    (void)hipDeviceSynchronize();
    memset(host_out, 0, 12 * sizeof(int));
    HIPCHK(c, hipMemcpy(host_out + 0, c->d_main_started, sizeof(int), hipMemcpyDeviceToHost)); host_out[1] = (int)c->main_started_total;
    HIPCHK(c, hipMemcpy(host_out + 2, c->d_wbc_finished, sizeof(int), hipMemcpyDeviceToHost)); host_out[3] = (int)c->wbc_finished_total;
    HIPCHK(c, hipMemcpy(host_out + 4, c->d_tick_done, sizeof(int), hipMemcpyDeviceToHost)); host_out[5] = (int)c->tick_done_total;
    for (int l = 1; l <= 2; ++l)
        if (c->lane[l].d_lane_done) { HIPCHK(c, hipMemcpy(host_out + 4 + 2 * l, c->lane[l].d_lane_done, sizeof(int), hipMemcpyDeviceToHost)); host_out[5 + 2 * l] = (int)c->lane[l].lane_done_total; }
    host_out[10] = (int)c->tick_epoch;
    if (!c->d_join_dbg) { HIPCHK(c, hipMalloc(&c->d_join_dbg, 16 * 8 * sizeof(long long))); HIPCHK(c, hipMemset(c->d_join_dbg, 0, 16 * 8 * sizeof(long long))); }
    else {
        long long h[16 * 8];
        HIPCHK(c, hipMemcpy(h, c->d_join_dbg, sizeof(h), hipMemcpyDeviceToHost));
        for (int i = 0; i < 16; ++i) if (h[8 * i]) fprintf(stderr, "  join[%d]: start %lld dur %.1f us expect %lld lane_expect %lld seen %lld lane_seen %lld gave_up %lld\n", i, h[8 * i], (h[8 * i + 1] - h[8 * i]) / 100.0, h[8 * i + 2], h[8 * i + 3], h[8 * i + 4], h[8 * i + 5], h[8 * i + 6]);
    }
    return QRGPU_OK;
}

int qrgpu_debug_gate2(qrgpu_ctx *c, long long *host_out /* [64][2]: when the gate in front of a chained tick's launches came up / opened, by epoch & 63 */)
{
    if (!c || !c->d_timeline || !host_out) return QRGPU_ERR_BAD_ARG;
    (void)hipDeviceSynchronize();
    HIPCHK(c, hipMemcpy(host_out, c->d_timeline + QR_TL_GATES, sizeof(long long) * (QR_TL_GATES_N + QR_TL_PLANNED_N), hipMemcpyDeviceToHost));      // [64][2] gate up / open, then [64][2] planned launch first start / last end
    return QRGPU_OK;
}

int qrgpu_debug_timeline_solves(qrgpu_ctx *c, long long *host_out /* [2][16][1024]: per epoch & 15 and robot: (publish time << 8 | launch kind), (cross-tick wait << 8 | kind | 8 gave up) */)
{
    if (!c || !c->d_timeline || !host_out) return QRGPU_ERR_BAD_ARG;
    (void)hipDeviceSynchronize();
    HIPCHK(c, hipMemcpy(host_out, c->d_timeline + QR_TL_SOLVES, sizeof(long long) * QR_TL_SOLVES_N, hipMemcpyDeviceToHost));
    return QRGPU_OK;
}

int qrgpu_debug_timeline_plans(qrgpu_ctx *c, long long *host_out /* [64][64] list length each planned workgroup read, then [64] the length each tick's planning left */)
{
    if (!c || !c->d_timeline || !host_out) return QRGPU_ERR_BAD_ARG;
    (void)hipDeviceSynchronize();
    HIPCHK(c, hipMemcpy(host_out, c->d_timeline + QR_TL_PLANS, sizeof(long long) * QR_TL_PLANS_N, hipMemcpyDeviceToHost));
    return QRGPU_OK;
}

int qrgpu_debug_timeline_trace(qrgpu_ctx *c, long long *host_out /* [16][1024] what happened to each robot in each epoch & 15 (QR_TRACE bits) */)
{
    if (!c || !c->d_timeline || !host_out) return QRGPU_ERR_BAD_ARG;
    (void)hipDeviceSynchronize();
    HIPCHK(c, hipMemcpy(host_out, c->d_timeline + QR_TL_TRACE, sizeof(long long) * QR_TL_TRACE_N, hipMemcpyDeviceToHost));
    return QRGPU_OK;
}

int qrgpu_debug_words(qrgpu_ctx *c, unsigned *solved, unsigned *wbc_done, int n)
{   // undocumented diagnostic: the per-robot epoch words of the overlapped tick
    if (!c || n <= 0 || n > c->max_batch) return QRGPU_ERR_BAD_ARG;
    (void)hipDeviceSynchronize();
    if (solved) HIPCHK(c, hipMemcpy(solved, c->d_solved, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost));
    if (wbc_done) HIPCHK(c, hipMemcpy(wbc_done, c->d_wbc_done, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost));
    return QRGPU_OK;
}

int qrgpu_debug_timeline(qrgpu_ctx *c, long long *host_out /* [65][8] (row 64, entry 0: the last tick's epoch), or NULL to switch on and reset */)
{   // undocumented diagnostic: per pipelined tick (ring of 64, indexed by the tick's epoch & 63) on the shared 100 MHz clock:
    // 0 first / 1 last start of a main-pass workgroup, 2 last solve published, 3 first WBC workgroup, 4 last WBC workgroup done,
    // 5 trailing list launch started, 6 ended, 7 second WBC pass ended (0 / LLONG_MAX where nothing was recorded)
    if (!c) return QRGPU_ERR_BAD_ARG;
#ifndef QR_TIMELINE
    c->err = "qrgpu_debug_timeline: the stamps are compiled in only with -DQR_TIMELINE (QRGPU_EXTRA_FLAGS)";
    return QRGPU_ERR_NOT_SETUP;
#endif
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->wbc_stream));
    if (!c->d_timeline) { HIPCHK(c, hipMalloc(&c->d_timeline, sizeof(long long) * QR_TL_WORDS)); HIPCHK(c, hipMemset(c->d_timeline, 0, sizeof(long long) * QR_TL_WORDS)); }
    {   // (the planned launch's first start is an atomicMin)
        long long ext[QR_TL_PLANNED_N];
        for (int e = 0; e < 64; ++e) { ext[2 * e] = 0x7fffffffffffffffLL; ext[2 * e + 1] = 0; }
        HIPCHK(c, hipMemcpy(c->d_timeline + QR_TL_PLANNED, ext, sizeof(ext), hipMemcpyHostToDevice));
    }
    if (!c->d_tlr) HIPCHK(c, hipMalloc(&c->d_tlr, sizeof(int) * 4 * (size_t)c->max_batch));
    if (host_out) HIPCHK(c, hipMemcpy(host_out, c->d_timeline + QR_TL_TICKS, sizeof(long long) * QR_TL_TICKS_N, hipMemcpyDeviceToHost));
    long long init[QR_TL_TICKS_N];
    for (int e = 0; e < 64; ++e) for (int k = 0; k < 8; ++k) init[e * 8 + k] = (k == 0 || k == 3 || k == 5) ? 0x7fffffffffffffffLL : 0;
    HIPCHK(c, hipMemcpy(c->d_timeline + QR_TL_TICKS, init, sizeof(init), hipMemcpyHostToDevice));
    if (host_out) host_out[QR_TL_TICKS_N] = (long long)c->tick_epoch;
    return QRGPU_OK;
}

int qrgpu_debug_timeline_robots(qrgpu_ctx *c, int *host_out /* [4][n]: WBC started, flag seen, WBC done, the solve's flag raised */, int n)
{   // undocumented diagnostic: per-robot moments of the last pipelined tick (after qrgpu_debug_timeline switched the stamps on)
    if (!c || !c->d_tlr || !host_out || n <= 0 || n > c->max_batch) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->wbc_stream));
    HIPCHK(c, hipMemcpy(host_out, c->d_tlr, sizeof(int) * 3 * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(host_out + 3 * (size_t)n, c->d_ftime, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    return QRGPU_OK;
}

int qrgpu_selftest(qrgpu_ctx *c, double *host_out256)
{   // cross-lane helper self-test (tests/test_gpu_mpc.py::test_wave_helpers)
    if (!c || !host_out256) return QRGPU_ERR_BAD_ARG;
    DeviceScratch d;
    HIPCHK(c, hipMalloc(&d.p, 256 * sizeof(double)));
    hipLaunchKernelGGL(qr_selftest_kernel, dim3(1), dim3(64), 0, c->stream, (double *)d.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(host_out256, d.p, 256 * sizeof(double), hipMemcpyDeviceToHost));
    return QRGPU_OK;
}

int qrgpu_enable_flop_count(qrgpu_ctx *c, int on)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (on && !c->d_flops) HIPCHK(c, hipMalloc(&c->d_flops, sizeof(double) * 4 * (size_t)c->max_batch));
    c->flops_on = on != 0;
    c->flops_n = 0;
    return QRGPU_OK;
}

int qrgpu_mpc_flop_counts(qrgpu_ctx *c, double out[4])
{
    if (!c || !out) return QRGPU_ERR_BAD_ARG;
    if (!c->d_flops || c->flops_n <= 0) return QRGPU_ERR_NOT_SETUP;
    std::vector<double> h(4 * (size_t)c->flops_n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h.data(), c->d_flops, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = out[3] = 0.0;
    for (int i = 0; i < c->flops_n; ++i) for (int k = 0; k < 4; ++k) out[k] += h[4 * (size_t)i + k];
    return QRGPU_OK;
}

}  // extern "C"
