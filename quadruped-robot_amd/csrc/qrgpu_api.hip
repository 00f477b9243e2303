// ============================================================================
// libqrgpu.so host side: the C ABI of include/qrgpu.h on top of the HIP runtime.
// No torch, no CPU compute path: every solve is a kernel launch on gfx950.
// This file: context and lane lifetime, the setters, *_setup, the MPC / WBC / VMC batch entry points, the
// single-robot calls and the memory, timing and mark utilities.  The per-robot stages: qrgpu_stages.hip; diagnostics: qrgpu_debug.hip;
// the MPC launch and the tick: qrgpu_mpc.hip, qrgpu_tick.hip.
// ============================================================================
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "qrgpu_ctx.h"
#include "qr_wbc_model.h"

// The side stream carries the planned list launch -- a few workgroups that each need a whole CU -- beside the main pass.  Highest priority,
// so that they are placed while the CUs are still empty: at default priority the main pass's workgroups fill every CU first and a listed
// robot starts 80-160 us late, which is then the end of the launch.
hipError_t create_side_stream(hipStream_t *s)
{
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
        return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest);
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

static void lane_destroy(Lane &L);

// A lane's buffers, counters and (lanes 1, 2) streams.  Counters start at zero and are never cleared.  A lane is either complete (d_order set)
// or empty: one that fails half way is taken down again.
int lane_create(qrgpu_ctx *c, Lane &L, bool own_stream, bool masked)
{
    if (L.d_order) return QRGPU_OK;
    L.own_stream = own_stream; L.masked = own_stream && masked;     // (what lane_destroy goes by, should this fail half way)
    const size_t nb = (size_t)c->max_batch;
    auto zalloc = [](auto **p, size_t bytes) { return hipMalloc((void **)p, bytes) == hipSuccess && hipMemset(*p, 0, bytes) == hipSuccess; };
    bool ok = hipMalloc(&L.d_order, sizeof(int) * 2 * nb) == hipSuccess && zalloc(&L.d_rescue, sizeof(int) * (nb + 2)) && zalloc(&L.d_pre, sizeof(int) * (2 * nb + 4)) &&
              zalloc(&L.d_skip, nb) && hipHostMalloc((void **)&L.h_pre_count, 4 * sizeof(int), hipHostMallocMapped) == hipSuccess &&
              hipHostGetDevicePointer((void **)&L.d_pre_hint, L.h_pre_count, 0) == hipSuccess && zalloc(&L.d_started, sizeof(int)) &&
              ((own_stream && !masked) || masked || create_side_stream(&L.side_stream) == hipSuccess) && zalloc(&L.d_done_flag, sizeof(unsigned) * nb) && zalloc(&L.d_qhead, 16 * sizeof(int)) &&
              zalloc(&L.d_planned_done, sizeof(int)) && zalloc(&L.d_go, (1 + QR_ABORT_RING) * sizeof(int)) && zalloc(&L.d_lane_done, sizeof(int)) && zalloc(&L.d_main_done, sizeof(int)) && zalloc(&L.d_rescue_taken, 4 * sizeof(int)) &&
              hipMalloc(&L.d_cmd_tick, sizeof(float) * 12 * nb) == hipSuccess &&
              hipEventCreateWithFlags(&L.ev_fork, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&L.ev_join, hipEventDisableTiming) == hipSuccess;
    if (ok && own_stream) {
        const uint32_t words = (uint32_t)((c->num_cu + 31) / 32);
        ok = (masked ? (hipExtStreamCreateWithCUMask(&L.stream, words, c->mask16_main) == hipSuccess && hipExtStreamCreateWithCUMask(&L.side_stream, words, c->mask16_side) == hipSuccess)
                     : hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking) == hipSuccess);
    }
    if (ok && masked) ok = hipMemset(L.d_rescue + 2, 0xff, sizeof(int) * nb) == hipSuccess;      // (an entry reads -1 until it is written: MpcLaunch::rescue_taken)
    if (ok) { L.h_pre_count[0] = L.h_pre_count[1] = L.h_pre_count[2] = L.h_pre_count[3] = 0; }       // ([2] of lane 0: a pipelined tick's join gave up waiting)
    (void)hipDeviceSynchronize();          // (the fills went to the default stream: none of the context's streams waits for that one)
    if (!ok) lane_destroy(L);
    return ok ? QRGPU_OK : QRGPU_ERR_ALLOC;
}
static void lane_destroy(Lane &L)
{
    if (L.stream && L.own_stream) { (void)hipStreamSynchronize(L.stream); }
    if (L.side_stream && (!L.own_stream || L.masked)) { (void)hipStreamSynchronize(L.side_stream); hipStreamDestroy(L.side_stream); }     // (lanes 1, 2 borrow lane 0's)
    if (L.stream && L.own_stream) hipStreamDestroy(L.stream);
    (void)hipHostFree(L.h_pre_count);
    for (void *p : {(void *)L.d_order, (void *)L.d_rescue, (void *)L.d_pre, (void *)L.d_skip, (void *)L.d_started, (void *)L.d_done_flag, (void *)L.d_qhead,
                    (void *)L.d_planned_done, (void *)L.d_go, (void *)L.d_lane_done, (void *)L.d_main_done, (void *)L.d_rescue_taken, (void *)L.d_cmd_tick})
        (void)hipFree(p);                                      // (null: a no-op)
    if (L.ev_fork) hipEventDestroy(L.ev_fork);
    if (L.ev_join) hipEventDestroy(L.ev_join);
    L = Lane{};
}

int upload_wbc(qrgpu_ctx *c)
{
    if (!c->wbc_dirty) return QRGPU_OK;
    HIPCHK(c, hipMemcpyAsync(c->d_wbc, c->wbc_host, sizeof(WbcConst) * QRGPU_MAX_TYPES, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->wbc_dirty = false;
    return QRGPU_OK;
}

int launch_wbc(qrgpu_ctx *c, int n, const int *d_type, const float *d_state, const float *d_cmd, float *d_prev, float *d_tau, float *d_qdes, int *d_status,
               const WbcOpts &o)
{
    if (!batch_ok(c, n) || !d_state) return QRGPU_ERR_BAD_ARG;
    if (!o.dbg && (!d_cmd || !d_prev || !d_tau)) return QRGPU_ERR_BAD_ARG;
    if (!(d_type ? ready_mask(c->wbc_ready) != 0 : c->wbc_ready[0])) return QRGPU_ERR_NOT_SETUP;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = upload_wbc(c);
    if (rc) return rc;
    const hipStream_t ws = o.stream ? o.stream : c->stream;
    if (!o.pipe.wbc_done) c->ov_chain = false;        // (any WBC launch but an overlapped tick's: the next overlapped tick waits for the context's stream)
    {
        TimerScope ts(c, 1, ws, !o.pipe.second && o.timed);          // (the second pass of a pipelined tick is not "the WBC launch" of the timing API)
        // (inspection outputs and cycle stamps are compiled into qr_wbc_kernel_dbg only)
        hipLaunchKernelGGL((o.dbg || o.qp || c->d_dbg_cycles_wbc) ? qr_wbc_kernel_dbg : qr_wbc_kernel, dim3(o.grid_wgs > 0 ? o.grid_wgs : 8 * ((n + 7) / 8)), dim3(128), 0, ws, n, c->d_wbc, d_type, d_state,
                           d_cmd ? d_cmd : d_state, d_prev, d_tau, d_qdes, d_status, o.dbg, o.merge, o.status_or, (long long *)c->d_dbg_cycles_wbc, o.fr,
                           ready_mask(c->wbc_ready), o.epilogue, o.qp, o.pipe);
    }
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

// The force-balance QP launch (the VMC entry points below; qrgpu_stance_tick_batch in qrgpu_stages.hip).
int launch_vmc(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_vmc_in, const float *d_ratio, const float *d_q, float *d_force,
               float *d_tau, int *d_status)
{
    if (!batch_ok(c, n) || !d_vmc_in || !d_force) return QRGPU_ERR_BAD_ARG;
    if (d_tau && !d_q) return QRGPU_ERR_BAD_ARG;
    if (!(d_type_id ? ready_mask(c->vmc_ready) != 0 : c->vmc_ready[0])) return QRGPU_ERR_NOT_SETUP;
    HIPCHK(c, hipSetDevice(c->device));
    VmcLaunch P = c->vmc;
    P.n = n; P.ratio = d_ratio; P.type_ready = ready_mask(c->vmc_ready);
    P.chain = c->mode_chain;                                         // (qrgpu_set_mode_route; null: every robot)
    hipLaunchKernelGGL(qr_vmc_kernel, dim3(8 * ((n + 7) / 8)), dim3(64), 0, c->stream, P, d_type_id, d_vmc_in, d_q, d_force, d_tau, d_status);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

extern "C" {

void qrgpu_model_desc_default(qrgpu_model_desc *d)
{
    d->hip_l = 0.08505f; d->upper_l = 0.2f; d->lower_l = 0.2f;
    d->body_size[0] = 0.267f; d->body_size[1] = 0.194f; d->body_size[2] = 0.114f;
    d->kp_body_pos = 100.f; d->kd_body_pos = 10.f; d->kp_body_ori = 100.f; d->kd_body_ori = 10.f;
    d->kp_foot = 500.f; d->kd_foot = 10.f; d->weight_fb = 0.1f; d->weight_fr = 1.f; d->mu = 0.4f;
}

// Once per process: any QRGPU_* variable of the environment that is neither a supported switch (include/qrgpu.h) nor bench.py's own (QRGPU_BENCH_*)
// is reported on the standard error -- a laboratory switch without QRGPU_LAB=1 is ignored, a misspelt one never did anything.
extern char **environ;
static void warn_unknown_env()
{
    static std::once_flag once;
    std::call_once(once, [] {
        static const char *supported[] = {QRGPU_SUPPORTED_ENV};
        static const char *labs[] = {QRGPU_LAB_ENV};
        const bool lab_on = lab_env("QRGPU_LAB") != nullptr;
        for (char **e = environ; e && *e; ++e) {
            if (strncmp(*e, "QRGPU_", 6) != 0 || strncmp(*e, "QRGPU_BENCH_", 12) == 0) continue;
            const char *eq = strchr(*e, '=');
            const std::string name(*e, eq ? (size_t)(eq - *e) : strlen(*e));
            bool ok = false, is_lab = false;
            for (const char *s_ : supported) if (name == s_) ok = true;
            for (const char *s_ : labs) if (name == s_) is_lab = true;
            if (ok || (is_lab && lab_on)) continue;
            if (is_lab) fprintf(stderr, "libqrgpu: %s is a laboratory switch: ignored unless QRGPU_LAB=1 is set (include/qrgpu.h lists the supported ones)\n", name.c_str());
            else fprintf(stderr, "libqrgpu: %s is not an environment switch of this library (include/qrgpu.h lists the supported ones): ignored\n", name.c_str());
        }
    });
}

int qrgpu_create(int device_id, int max_batch, int horizon_max, qrgpu_ctx **out)
{
    if (!out || max_batch <= 0 || horizon_max <= 0 || horizon_max > QRGPU_MAX_HORIZON) return QRGPU_ERR_BAD_ARG;
    warn_unknown_env();
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return QRGPU_ERR_NO_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return QRGPU_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return QRGPU_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return QRGPU_ERR_NO_DEVICE;     // kernels are built for gfx950 only
    qrgpu_ctx *c = new qrgpu_ctx();
    c->device = device_id; c->max_batch = max_batch; c->horizon_max = horizon_max;
    c->name = prop.name; c->num_cu = prop.multiProcessorCount;
    c->lds_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    if (c->lds_per_cu <= 0) c->lds_per_cu = 160 * 1024;
    const size_t in1 = 28 + 12 * QRGPU_MAX_HORIZON + 4 * QRGPU_MAX_HORIZON + 12 + 37 + 67 + 3;
    static_assert(28 + 12 * QRGPU_MAX_HORIZON + 4 * QRGPU_MAX_HORIZON + 12 + 37 + 67 + 3 <= 512, "staging layout");
    c->zero_copy = !qr_env().single_copies;
    bool stage_ok;
    if (c->zero_copy) {
        // [0, 512) floats in, [512, 576) floats out, [576, 580) status / type words
        void *dp = nullptr;
        stage_ok = hipHostMalloc(&c->h_stage, 640 * sizeof(float), hipHostMallocMapped) == hipSuccess &&
                   hipHostGetDevicePointer(&dp, c->h_stage, 0) == hipSuccess;
        if (stage_ok) {
            memset(c->h_stage, 0, 640 * sizeof(float));
            c->h_in1 = (float *)c->h_stage; c->h_out1 = c->h_in1 + 512; c->h_st1 = (int *)(c->h_in1 + 576);
            c->d_in1 = (float *)dp; c->d_out1 = c->d_in1 + 512; c->d_st1 = (int *)(c->d_in1 + 576);
        }
    } else {
        stage_ok = hipMalloc(&c->d_in1, in1 * sizeof(float)) == hipSuccess && hipMalloc(&c->d_out1, 64 * sizeof(float)) == hipSuccess &&
                   hipMalloc(&c->d_st1, 4 * sizeof(int)) == hipSuccess;
    }
    auto zalloc = [](auto **p, size_t bytes) { return hipMalloc((void **)p, bytes) == hipSuccess && hipMemset(*p, 0, bytes) == hipSuccess; };
    bool ok = stage_ok && hipMalloc(&c->d_wbc, sizeof(WbcConst) * QRGPU_MAX_TYPES) == hipSuccess;
    const size_t nb = (size_t)max_batch;
    ok = ok && zalloc(&c->d_body, sizeof(qrgpu_plant_body_desc) * QRGPU_MAX_TYPES);
    ok = ok && zalloc(&c->d_cost[0], sizeof(int) * nb) && zalloc(&c->d_cost[1], sizeof(int) * nb) && hipMalloc(&c->d_warm, (size_t)QR_WARM_STRIDE * nb) == hipSuccess &&
         hipStreamCreateWithFlags(&c->wbc_stream, hipStreamNonBlocking) == hipSuccess &&
         zalloc(&c->d_main_started, sizeof(int)) && zalloc(&c->d_tick_done, sizeof(int)) && zalloc(&c->d_gate_abort, QR_ABORT_RING * sizeof(int)) &&
         zalloc(&c->d_wbc_finished, sizeof(int)) && zalloc(&c->d_solved, sizeof(unsigned) * nb) && zalloc(&c->d_wbc_done, sizeof(unsigned) * nb) &&
         hipMalloc(&c->d_ftime, sizeof(int) * nb) == hipSuccess;
    // lane 0 always; lanes 1 and 2 (streams of their own) when overlapped ticks are first switched on (qrgpu_set_tick_overlap)
    ok = ok && lane_create(c, c->lane[0], false) == QRGPU_OK;
    if (!ok) {
        qrgpu_destroy(c);
        return QRGPU_ERR_ALLOC;
    }
    // The compute stream is the context's own (non-blocking) unless the caller names one (qrgpu_set_stream; NULL there = the default stream).  On the
    // default stream two contexts of one process serialise each other's launches: 16.9 against 34.7 M WBC calls/s for two contexts of 512 robots.
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) == hipSuccess) c->stream = c->own_stream;
    c->lane[0].stream = c->stream;
    (void)hipDeviceSynchronize();          // (the fills of the counters above went to the default stream: none of the context's streams waits for that one)
    memset(&c->mpc, 0, sizeof(c->mpc));
    memset(c->wbc_host, 0, sizeof(c->wbc_host));
    *out = c;
    return QRGPU_OK;
}

void qrgpu_destroy(qrgpu_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->wbc_stream) (void)hipStreamSynchronize(c->wbc_stream);
    qrgpu_comm_destroy(c);
    for (int l = 0; l < QR_LANES; ++l) lane_destroy(c->lane[l]);         // (synchronises the lanes' own and side streams first)
    for (int k = 0; k < 2; ++k) for (auto &e : c->ev[k]) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    for (auto &e : c->marks) hipEventDestroy(e);
    if (c->wbc_stream) hipStreamDestroy(c->wbc_stream);
    if (c->wbc_stream_hi) { (void)hipStreamSynchronize(c->wbc_stream_hi); hipStreamDestroy(c->wbc_stream_hi); }
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    for (int k = 0; k < 2; ++k) if (c->ev_call[k]) hipEventDestroy(c->ev_call[k]);
    if (c->h_stage) (void)hipHostFree(c->h_stage);              // (zero copy: d_in1, d_out1 and d_st1 point into this block)
    else for (void *p : {(void *)c->d_in1, (void *)c->d_out1, (void *)c->d_st1}) (void)hipFree(p);
    for (void *p : {(void *)c->d_wbc, (void *)c->d_body, (void *)c->d_gait_table, (void *)c->d_mode_masks, (void *)c->d_cost[0], (void *)c->d_cost[1], (void *)c->d_warm, (void *)c->d_flops, (void *)c->d_main_started, (void *)c->d_ftime,
                    (void *)c->d_wbc_finished, (void *)c->d_gate_abort, (void *)c->d_solved, (void *)c->d_wbc_done, (void *)c->d_gather_done, (void *)c->d_tick_done,
                    (void *)c->d_timeline, (void *)c->d_tlr, (void *)c->d_sinv_spill, c->d_dbg_cycles, c->d_dbg_cycles_wbc, (void *)c->d_join_dbg})
        (void)hipFree(p);                                      // (null: a no-op)
    delete c;
}

// another population: the dispatch order, the plan and the smoothed costs of every lane mean nothing any more
static void forget_history(qrgpu_ctx *c)
{
    for (auto &L : c->lane) { L.lpt_n = 0; L.plan_n = 0; }
    c->cost_n[0] = c->cost_n[1] = 0;
    c->ov_hold = 0;
}
int qrgpu_set_lpt_schedule(qrgpu_ctx *c, int on)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    c->lpt = on != 0;
    forget_history(c);
    return QRGPU_OK;
}
int qrgpu_set_warm_start(qrgpu_ctx *c, int on)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    c->warm = on != 0;
    c->warm_n = 0;                 // forget what is stored
    return QRGPU_OK;
}
int qrgpu_mpc_set_hessian_mode(qrgpu_ctx *c, int mode)
{
    if (!c || (mode != QRGPU_HESSIAN_F32 && mode != QRGPU_HESSIAN_BF16X3)) return QRGPU_ERR_BAD_ARG;
    c->mpc.hess_mode = mode;
    return QRGPU_OK;
}
int qrgpu_set_planned_list(qrgpu_ctx *c, int on, int big_nls)
{
    if (!c || big_nls < 0) return QRGPU_ERR_BAD_ARG;
    c->planned = on != 0;
    c->big_nls = big_nls;
    for (auto &L : c->lane) L.plan_n = 0;
    return QRGPU_OK;
}
int qrgpu_set_tick_pipeline(qrgpu_ctx *c, int on)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    c->pipeline = on != 0;
    return QRGPU_OK;
}
int qrgpu_set_rescue_pass(qrgpu_ctx *c, int on)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    c->rescue = on != 0;
    for (auto &L : c->lane) L.plan_n = 0;
    return QRGPU_OK;
}
int qrgpu_set_stream(qrgpu_ctx *c, void *s) { if (!c) return QRGPU_ERR_BAD_ARG; c->stream = (hipStream_t)s; c->lane[0].stream = c->stream; c->ov_chain = false; return QRGPU_OK; }
void *qrgpu_get_stream(qrgpu_ctx *c) { return c ? (void *)c->stream : nullptr; }
const char *qrgpu_last_error(const qrgpu_ctx *c) { return c ? c->err.c_str() : "null context"; }
int qrgpu_device_info(const qrgpu_ctx *c, char *name, int len, int *lds)
{
    if (!c) return 0;
    if (name && len > 0) { strncpy(name, c->name.c_str(), len - 1); name[len - 1] = 0; }
    if (lds) *lds = c->lds_per_cu;
    return c->num_cu;
}

int qrgpu_mpc_setup(qrgpu_ctx *c, int type_id, float dt, int horizon, float mu, float fmax, float mass,
                    const float inertia[3], const float weights[12], float alpha)
{
    if (!c || type_id < 0 || type_id >= QRGPU_MAX_TYPES || !inertia || !weights) return QRGPU_ERR_BAD_ARG;
    if (horizon <= 0 || horizon > c->horizon_max) return QRGPU_ERR_BAD_ARG;
    // one horizon per context (the reference has one global problem size, qr_mpc_interface.cpp:35-104):
    // a different horizon re-sizes the problem and invalidates the other types' setup, as a second SetupProblem would
    if (c->mpc.horizon != horizon) for (int t = 0; t < QRGPU_MAX_TYPES; ++t) if (t != type_id) c->mpc_ready[t] = false;
    MpcType &T = c->mpc.type[type_id];
    T.dt = dt; T.mu = mu; T.fmax = fmax; T.mass = mass; T.alpha = alpha;
    for (int i = 0; i < 3; ++i) T.inertia[i] = inertia[i];
    for (int i = 0; i < 12; ++i) T.weights[i] = weights[i];
    if (!c->wbc_ready[type_id]) { T.hip_l = 0.08505f; T.upper_l = 0.2f; T.lower_l = 0.2f; }
    c->mpc.horizon = horizon;
    c->mpc_ready[type_id] = true;
    return QRGPU_OK;
}

int qrgpu_wbc_setup(qrgpu_ctx *c, int type_id, const qrgpu_model_desc *desc)
{
    if (!c || type_id < 0 || type_id >= QRGPU_MAX_TYPES || !desc) return QRGPU_ERR_BAD_ARG;
    build_wbc_const(*desc, c->wbc_host[type_id]);
    MpcType &T = c->mpc.type[type_id];
    T.hip_l = desc->hip_l; T.upper_l = desc->upper_l; T.lower_l = desc->lower_l;    // leg geometry for the MPC torque map
    c->wbc_ready[type_id] = true;
    c->wbc_dirty = true;
    return QRGPU_OK;
}

int qrgpu_mpc_solve_batch(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_mpc_state, const float *d_traj,
                          const float *d_gait, const float *d_q, float *d_force, float *d_tau_mpc, int *d_status)
{
    MpcOpts o;
    o.epilogue = c ? c->epilogue : 0;
    return launch_mpc(c, n, mpc_io(d_type_id, d_mpc_state, d_traj, d_gait, d_q, d_force, d_tau_mpc, d_status), o);
}

int qrgpu_mpc_assemble_batch(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_mpc_state, const float *d_traj,
                             const float *d_gait, float *d_H, float *d_g)
{
    if (!c || !d_H || !d_g) return QRGPU_ERR_BAD_ARG;
    // the kernel needs somewhere to put the forces: scratch of this call's own
    DeviceScratch scratch;
    HIPCHK(c, hipMalloc(&scratch.p, sizeof(float) * 12 * (size_t)n));
    MpcIO io = mpc_io(d_type_id, d_mpc_state, d_traj, d_gait, nullptr, (float *)scratch.p, nullptr, nullptr);
    io.dbgH = d_H; io.dbgG = d_g;
    const int rc = launch_mpc(c, n, io);
    hipStreamSynchronize(c->stream);
    return rc;
}

int qrgpu_wbc_run_batch(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_fb_state, const float *d_wbc_cmd,
                        float *d_prev_ori, float *d_tau, float *d_qdes, int *d_status)
{
    return launch_wbc(c, n, d_type_id, d_fb_state, d_wbc_cmd, d_prev_ori, d_tau, d_qdes, d_status);
}

int qrgpu_fb_debug_batch(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_fb_state, float *d_out)
{
    if (!d_out) return QRGPU_ERR_BAD_ARG;
    WbcOpts o;
    o.dbg = d_out;
    return launch_wbc(c, n, d_type_id, d_fb_state, nullptr, nullptr, nullptr, nullptr, nullptr, o);
}

int qrgpu_wbc_inspect_batch(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_fb_state, const float *d_wbc_cmd,
                            float *d_prev_ori, float *d_tau, float *d_qp, int *d_status)
{
    if (!d_qp) return QRGPU_ERR_BAD_ARG;
    WbcOpts o;
    o.qp = d_qp;
    return launch_wbc(c, n, d_type_id, d_fb_state, d_wbc_cmd, d_prev_ori, d_tau, nullptr, d_status, o);
}

void qrgpu_vmc_desc_default(qrgpu_vmc_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->mass = 13.f;
    d->inertia[0] = 0.24f; d->inertia[4] = 0.80f; d->inertia[8] = 1.0f;
    const float w[6] = {1.f, 1.f, 1.f, 10.f, 10.f, 1.f};
    memcpy(d->acc_weight, w, sizeof(w));
    d->reg_weight = 1e-4f; d->friction = 0.5f; d->fmin_ratio = 0.01f; d->fmax_ratio = 10.f;
    d->hip_l = 0.08505f; d->upper_l = 0.2f; d->lower_l = 0.2f;
}

int qrgpu_vmc_setup(qrgpu_ctx *c, int type_id, const qrgpu_vmc_desc *d)
{
    if (!c || !d || type_id < 0 || type_id >= QRGPU_MAX_TYPES) return QRGPU_ERR_BAD_ARG;
    if (!(d->mass > 0.f)) return QRGPU_ERR_BAD_ARG;
    c->vmc.type[type_id] = *d;
    c->vmc_ready[type_id] = true;
    return QRGPU_OK;
}

int qrgpu_vmc_force_batch(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_vmc_in, const float *d_q, float *d_force, float *d_tau,
                          int *d_status)
{
    return launch_vmc(c, n, d_type_id, d_vmc_in, nullptr, d_q, d_force, d_tau, d_status);
}

int qrgpu_vmc_force_world_batch(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_vmc_in, const float *d_ratio, const float *d_q,
                                float *d_force, float *d_tau, int *d_status)
{
    if (!d_ratio) return QRGPU_ERR_BAD_ARG;
    return launch_vmc(c, n, d_type_id, d_vmc_in, d_ratio, d_q, d_force, d_tau, d_status);
}

int qrgpu_set_torque_epilogue(qrgpu_ctx *c, int flags)
{
    if (!c || (flags & ~(QRGPU_EPILOGUE_HIP_COMP | QRGPU_EPILOGUE_CLIP))) return QRGPU_ERR_BAD_ARG;
    c->epilogue = flags;
    return QRGPU_OK;
}

// The single-robot calls stage through the context (qrgpu_ctx.h): with zero copy the host fills the pinned block in place, the one
// launch reads and writes it over PCIe, and the only stream command besides the launch is the wait.
static int stage_in(qrgpu_ctx *c, const float *src, size_t nfloat, int type_id, int **d_type)
{
    *d_type = nullptr;
    if (c->zero_copy) {
        memcpy(c->h_in1, src, nfloat * sizeof(float));
        if (type_id != 0) { c->h_st1[1] = type_id; *d_type = c->d_st1 + 1; }
        return QRGPU_OK;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_in1, src, nfloat * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (type_id != 0) {
        *d_type = c->d_st1 + 1;
        c->type_stage = type_id;         // (a context member: the copy is asynchronous)
        HIPCHK(c, hipMemcpyAsync(*d_type, &c->type_stage, sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    return QRGPU_OK;
}
static int stage_out(qrgpu_ctx *c, float *out, size_t nfloat, int *st)
{
    if (c->zero_copy) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        memcpy(out, c->h_out1, nfloat * sizeof(float));
        *st = c->h_st1[0];
        return QRGPU_OK;
    }
    HIPCHK(c, hipMemcpyAsync(out, c->d_out1, nfloat * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(st, c->d_st1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QRGPU_OK;
}

int qrgpu_mpc_solve1(qrgpu_ctx *c, int type_id, const float p[3], const float v[3], const float quat[4], const float w[3],
                     const float r[12], const float rpy[3], const float *traj, const float *gait, const float q[12],
                     double f_out[12], float tau_out[12], int *status)
{
    if (!c || !p || !v || !quat || !w || !r || !rpy || !traj || !gait || !f_out) return QRGPU_ERR_BAD_ARG;
    if (type_id < 0 || type_id >= QRGPU_MAX_TYPES || !c->mpc_ready[type_id]) return QRGPU_ERR_NOT_SETUP;
    const int h = c->mpc.horizon;
    float in[28 + 16 * QRGPU_MAX_HORIZON + 12];
    const size_t nin = 28 + 16 * (size_t)h + 12;
    memcpy(&in[0], p, 12); memcpy(&in[3], v, 12); memcpy(&in[6], quat, 16); memcpy(&in[10], w, 12);
    memcpy(&in[13], r, 48); memcpy(&in[25], rpy, 12);
    memcpy(&in[28], traj, sizeof(float) * 12 * h);
    memcpy(&in[28 + 12 * h], gait, sizeof(float) * 4 * h);
    if (q) memcpy(&in[28 + 16 * h], q, 48); else memset(&in[28 + 16 * h], 0, 48);
    HIPCHK(c, hipSetDevice(c->device));
    int *d_type = nullptr;
    int rc = stage_in(c, in, nin, type_id, &d_type);
    if (rc) return rc;
    rc = launch_mpc(c, 1, mpc_io(d_type, c->d_in1, c->d_in1 + 28, c->d_in1 + 28 + 12 * h, c->d_in1 + 28 + 16 * h, c->d_out1, (q && tau_out) ? c->d_out1 + 12 : nullptr, c->d_st1));
    if (rc) return rc;
    float out[24]; int st = 0;
    rc = stage_out(c, out, 24, &st);
    if (rc) return rc;
    for (int i = 0; i < 12; ++i) f_out[i] = out[i];
    if (q && tau_out) for (int i = 0; i < 12; ++i) tau_out[i] = out[12 + i];
    if (status) *status = st;
    return QRGPU_OK;
}

int qrgpu_wbc_run1(qrgpu_ctx *c, int type_id, const float fb_state[37], const float wbc_cmd[67], float prev_ori_vel[3],
                   float tau_out[12], float qdes_out[12], float qddes_out[12], int *status)
{
    if (!c || !fb_state || !wbc_cmd || !prev_ori_vel || !tau_out) return QRGPU_ERR_BAD_ARG;
    if (type_id < 0 || type_id >= QRGPU_MAX_TYPES || !c->wbc_ready[type_id]) return QRGPU_ERR_NOT_SETUP;
    float in[37 + 67 + 3];
    memcpy(in, fb_state, 37 * 4); memcpy(in + 37, wbc_cmd, 67 * 4); memcpy(in + 104, prev_ori_vel, 12);
    HIPCHK(c, hipSetDevice(c->device));
    int *d_type = nullptr;
    int rc = stage_in(c, in, 107, type_id, &d_type);
    if (rc) return rc;
    const bool want_q = qdes_out || qddes_out;
    rc = launch_wbc(c, 1, d_type, c->d_in1, c->d_in1 + 37, c->d_in1 + 104, c->d_out1, want_q ? c->d_out1 + 12 : nullptr, c->d_st1);
    if (rc) return rc;
    float out[36]; int st = 0;
    if (!c->zero_copy) HIPCHK(c, hipMemcpyAsync(prev_ori_vel, c->d_in1 + 104, 12, hipMemcpyDeviceToHost, c->stream));
    rc = stage_out(c, out, 36, &st);
    if (rc) return rc;
    if (c->zero_copy) memcpy(prev_ori_vel, c->h_in1 + 104, 12);
    memcpy(tau_out, out, 48);
    if (qdes_out) memcpy(qdes_out, out + 12, 48);
    if (qddes_out) memcpy(qddes_out, out + 24, 48);
    if (status) *status = st;
    return QRGPU_OK;
}

static int vmc_force1(qrgpu_ctx *c, int type_id, const float vmc_in[37], const float ratio[8], const float q[12], float force_out[12], float tau_out[12],
                      int *status)
{
    if (!c || !vmc_in || !force_out) return QRGPU_ERR_BAD_ARG;
    if (tau_out && !q) return QRGPU_ERR_BAD_ARG;
    if (type_id < 0 || type_id >= QRGPU_MAX_TYPES || !c->vmc_ready[type_id]) return QRGPU_ERR_NOT_SETUP;
    float in[37 + 12 + 8];
    memset(in, 0, sizeof(in));
    memcpy(in, vmc_in, 37 * 4);
    if (q) memcpy(in + 37, q, 48);
    if (ratio) memcpy(in + 49, ratio, 32);
    HIPCHK(c, hipSetDevice(c->device));
    int *d_type = nullptr;
    { const int rc_ = stage_in(c, in, sizeof(in) / sizeof(float), type_id, &d_type); if (rc_) return rc_; }
    VmcLaunch P = c->vmc;
    P.n = 1; P.ratio = ratio ? c->d_in1 + 49 : nullptr; P.type_ready = ready_mask(c->vmc_ready);
    hipLaunchKernelGGL(qr_vmc_kernel, dim3(8), dim3(64), 0, c->stream, P, d_type, c->d_in1, q ? c->d_in1 + 37 : nullptr, c->d_out1,
                       (q && tau_out) ? c->d_out1 + 12 : nullptr, c->d_st1);
    HIPCHK(c, hipGetLastError());
    float out[24]; int st = 0;
    { const int rc_ = stage_out(c, out, 24, &st); if (rc_) return rc_; }
    memcpy(force_out, out, 48);
    if (q && tau_out) memcpy(tau_out, out + 12, 48);
    if (status) *status = st;
    return QRGPU_OK;
}

int qrgpu_vmc_force1(qrgpu_ctx *c, int type_id, const float vmc_in[37], const float q[12], float force_out[12], float tau_out[12], int *status)
{
    return vmc_force1(c, type_id, vmc_in, nullptr, q, force_out, tau_out, status);
}

int qrgpu_vmc_force_world1(qrgpu_ctx *c, int type_id, const float vmc_in[37], const float ratio[8], const float q[12], float force_out[12],
                           float tau_out[12], int *status)
{
    if (!ratio) return QRGPU_ERR_BAD_ARG;
    return vmc_force1(c, type_id, vmc_in, ratio, q, force_out, tau_out, status);
}

int qrgpu_sync(qrgpu_ctx *c)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->lane[0].h_pre_count && c->lane[0].h_pre_count[2]) {
        // the join of a pipelined tick waited 20 ms for its WBC launch and went on without it: outputs of that tick are incomplete
        c->lane[0].h_pre_count[2] = 0;
        (void)hipStreamSynchronize(c->wbc_stream);
        c->err = "a bounded device-side wait gave up: the WBC launch of a pipelined tick did not finish within 20 ms of its join, or an all-gather did not finish "
                 "(or its tick did not) within 30 s: outputs of that call were incomplete when the stream went on";
        return QRGPU_ERR_LAUNCH;
    }
    return QRGPU_OK;
}

int qrgpu_enable_timing(qrgpu_ctx *c, int on)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (on < 0) { c->timing = false; c->timing_paused = true; return QRGPU_OK; }     // pause: what was measured so far is kept
    const bool resume = on > 0 && c->timing_paused;
    c->timing = on != 0;
    c->timing_paused = false;
    c->timing_every = on > 1 ? on : 1;
    if (!resume) {
        c->ev_calls[0] = c->ev_calls[1] = 0;
        c->ev_used[0] = c->ev_used[1] = 0;
    }
    if (on) {
        // the event pairs of the first launches are made here, not inside the caller's timed steps (TimerScope still grows the pool beyond them)
        HIPCHK(c, hipSetDevice(c->device));
        for (int k = 0; k < 2; ++k)
            while (c->ev[k].size() < 512) {
                hipEvent_t a, b;
                HIPCHK(c, hipEventCreate(&a));
                HIPCHK(c, hipEventCreate(&b));
                c->ev[k].push_back({a, b});
            }
    }
    return QRGPU_OK;
}

int qrgpu_get_timing(qrgpu_ctx *c, int kernel, double *mean_ms, int *count)
{
    if (!c || kernel < 0 || kernel > 1 || !mean_ms) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (size_t i = 0; i < c->ev_used[kernel]; ++i) {
        float ms = 0.f;
        // (a pipelined tick records the WBC launch's events on the WBC stream, an overlapped one the main pass's on a lane's stream: the tick's join on
        //  the context's stream polls counts the kernels bump BEFORE they retire, so the second event may still be pending)
        HIPCHK(c, hipEventSynchronize(c->ev[kernel][i].second));
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[kernel][i].first, c->ev[kernel][i].second));
        tot += ms;
    }
    *mean_ms = c->ev_used[kernel] ? tot / (double)c->ev_used[kernel] : 0.0;
    if (count) *count = (int)c->ev_used[kernel];
    return QRGPU_OK;
}

void *qrgpu_malloc(qrgpu_ctx *c, unsigned long long bytes)
{
    if (!c) return nullptr;
    void *p = nullptr;
    hipSetDevice(c->device);
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}
void qrgpu_free(qrgpu_ctx *c, void *p) { if (c && p) { hipSetDevice(c->device); hipFree(p); } }
int qrgpu_memcpy_h2d(qrgpu_ctx *c, void *dst, const void *src, unsigned long long bytes)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QRGPU_OK;
}
int qrgpu_memcpy_d2h(qrgpu_ctx *c, void *dst, const void *src, unsigned long long bytes)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QRGPU_OK;
}

void *qrgpu_host_alloc(qrgpu_ctx *c, unsigned long long bytes)
{
    if (!c) return nullptr;
    void *p = nullptr;
    hipSetDevice(c->device);
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void qrgpu_host_free(qrgpu_ctx *c, void *p) { if (c && p) { hipSetDevice(c->device); hipHostFree(p); } }
int qrgpu_memcpy_async(qrgpu_ctx *c, void *dst, const void *src, unsigned long long bytes, int kind)
{
    if (!c || kind < 0 || kind > 2) return QRGPU_ERR_BAD_ARG;
    static const hipMemcpyKind k[3] = {hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice};
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, k[kind], c->stream));
    return QRGPU_OK;
}
int qrgpu_memset_async(qrgpu_ctx *c, void *dst, int byte_value, unsigned long long bytes)
{
    if (!c || !dst) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipMemsetAsync(dst, byte_value, bytes, c->stream));
    return QRGPU_OK;
}
int qrgpu_mark(qrgpu_ctx *c, int index)
{
    if (!c || index < 0 || index >= 65536) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    while ((int)c->marks.size() <= index) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        c->marks.push_back(e);
    }
    HIPCHK(c, hipEventRecord(c->marks[index], c->stream));
    return QRGPU_OK;
}
int qrgpu_mark_elapsed_ms(qrgpu_ctx *c, int from, int to, double *ms)
{
    if (!c || !ms || from < 0 || to < 0 || from >= (int)c->marks.size() || to >= (int)c->marks.size()) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipEventSynchronize(c->marks[to]));
    float f = 0.f;
    HIPCHK(c, hipEventElapsedTime(&f, c->marks[from], c->marks[to]));
    *ms = f;
    return QRGPU_OK;
}

}  // extern "C"
