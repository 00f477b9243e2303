// ============================================================================
// libqrgpu.so host side: the open-loop gait generator with the gait chosen per robot and the stage clock that restarts where a mask says
// (qr_gait_kernel.hip), and the default gait table.  Every entry point is "check the arguments, one launch on the context's stream".
// ============================================================================
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>

#include "qrgpu_ctx.h"

static int gs_bad(qrgpu_ctx *c, const char *call, const char *what)
{
    if (c) c->err = std::string(call) + ": " + what;
    return QRGPU_ERR_BAD_ARG;
}

template <typename... KArgs, typename... Args>
static int gs_launch(qrgpu_ctx *c, void (*kernel)(KArgs...), int n, Args... args)
{
    c->ov_chain = false;                                             // another launch of the context: the next overlapped tick is not chained
    hipLaunchKernelGGL(kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, args...);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

extern "C" {

void qrgpu_gait_table_default(qrgpu_gait_desc table[5])
{   // config/a1_sim/openloop_gait_generator.yaml: advanced_trot (the gait the generator is constructed with), trot, advanced_trot, walk, stand
    if (!table) return;
    for (int e = 0; e < 5; ++e) qrgpu_gait_desc_default(&table[e]);          // [0], [2]; every entry: all legs start in STANCE, wait_time
    const struct { int e; float stance, duty, phase[4], threshold; } blocks[] = {{QRGPU_FSM_GAIT_TROT, 0.3f, 0.6f, {0.5f, 0.f, 0.f, 0.5f}, 0.5f},
                                                                                 {QRGPU_FSM_GAIT_WALK, 7.5f, 0.75f, {0.5f, 0.f, 0.75f, 0.25f}, 0.1f},
                                                                                 {QRGPU_FSM_GAIT_STAND, 0.3f, 1.f, {0.f, 0.f, 0.f, 0.f}, 0.1f}};
    for (const auto &b : blocks) {
        qrgpu_gait_desc &d = table[b.e];
        for (int l = 0; l < 4; ++l) { d.stance_duration[l] = b.stance; d.duty_factor[l] = b.duty; d.initial_leg_phase[l] = b.phase[l]; }
        d.contact_detection_phase_threshold = b.threshold; d.advanced_trot = 0;
    }
}

int qrgpu_gait_select_update_batch(qrgpu_ctx *c, int n, const qrgpu_gait_desc *table, int n_gaits, const float *d_gait_sel, float current_time, int robot_stop,
                                   int reset, const float *d_contact, float *d_gait_state, float *d_gait_out, float *d_fe_in, float *d_swing_in, int *d_gait_flags)
{
    static const char *const me = "qrgpu_gait_select_update_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return gs_bad(c, me, "n");
    if (!table) return gs_bad(c, me, "table");
    if (n_gaits < 1 || n_gaits > QRGPU_MAX_GAITS) return gs_bad(c, me, "n_gaits");
    if (!d_gait_sel) return gs_bad(c, me, "d_gait_sel");
    if (!d_contact) return gs_bad(c, me, "d_contact");
    if (!d_gait_state) return gs_bad(c, me, "d_gait_state");
    if (reset != 0 && reset != QRGPU_GAIT_RESET_CONSTRUCT && reset != QRGPU_GAIT_RESET_LIVE) return gs_bad(c, me, "reset");
    for (int e = 0; e < n_gaits; ++e)
        for (int l = 0; l < 4; ++l) {                                  // USERDEFINED_SWING legs are not built
            if (!(table[e].duty_factor[l] > 0.001f)) return gs_bad(c, me, "table: duty_factor");
            if (!(table[e].stance_duration[l] > 0.f)) return gs_bad(c, me, "table: stance_duration");
        }
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_gait_table) HIPCHK(c, hipMalloc((void **)&c->d_gait_table, sizeof(c->gait_table_host)));
    const size_t bytes = sizeof(qrgpu_gait_desc) * (size_t)n_gaits;
    if (c->gait_table_n != n_gaits || memcmp(c->gait_table_host, table, bytes) != 0) {
        // another table: the launches queued so far read the old one, so the copy is queued behind them on the stream, from the context's own memory
        memcpy(c->gait_table_host, table, bytes);
        c->gait_table_n = 0;
        HIPCHK(c, hipMemcpyAsync(c->d_gait_table, c->gait_table_host, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->gait_table_n = n_gaits;
    }
    return gs_launch(c, qr_gait_select_kernel, n, (const qrgpu_gait_desc *)c->d_gait_table, n_gaits, d_gait_sel, current_time, robot_stop ? 1 : 0, reset, d_contact,
                     d_gait_state, d_gait_out, d_fe_in, d_swing_in, d_gait_flags,
                     stage_args(c, QRGPU_GAIT_RESET_CONSTRUCT, QRGPU_GAIT_RESET_LIVE));
}

int qrgpu_stage_clock_batch(qrgpu_ctx *c, int n, const int *d_mask, unsigned bits, const int *d_ticks, int *d_origin, int *d_local)
{
    static const char *const me = "qrgpu_stage_clock_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return gs_bad(c, me, "n");
    if (!d_mask) return gs_bad(c, me, "d_mask");
    if (bits == 0u) return gs_bad(c, me, "bits");
    if (!d_ticks) return gs_bad(c, me, "d_ticks");
    if (!d_origin) return gs_bad(c, me, "d_origin");
    if (!d_local) return gs_bad(c, me, "d_local");
    HIPCHK(c, hipSetDevice(c->device));
    return gs_launch(c, qr_stage_clock_kernel, n, d_mask, bits, d_ticks, d_origin, d_local);
}

}  // extern "C"
