// ============================================================================
// libqrgpu.so host side: the C ABI of include/qrgpu.h on top of the HIP runtime.
// No torch, no CPU compute path: every solve is a kernel launch on gfx950.
// ============================================================================
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "qrgpu_ctx.h"

namespace qrgpu {
__global__ void qr_selftest_kernel(double *out);
__global__ void qr_gait_kernel(int n, GaitDesc D, float currentTime, int stop, int fresh, const float *g_contact, float *st, float *g_out, float *g_fe);
__global__ void qr_swing_velocity_kernel(int n, EstimatorDesc D, SwingVelDesc V, const float *g_in, float *g_out);
__global__ void qr_ground_kernel(int n, int fresh, const float *g_in, double *g_st, float *g_out, float *g_est_in);
__global__ void qr_walk_gait_kernel(int n, WalkDesc D, float currentTime, int stop, int fresh, const float *g_contact, float *st, float *g_out, float *g_ratio,
                                    float *g_vmc_in);
__global__ void qr_swing_kernel(int n, EstimatorDesc D, const float *g_in, float *g_cmd, float *g_tgt_world, float *g_qdes);
__global__ void qr_foothold_kernel(int n, FootholdDesc D, const float *g_in, const float *g_gait_state, const float *g_gait_out, float *g_swing);
__global__ void qr_swing_update_kernel(int n, SwingModeDesc M, int reset, int stop, const float *g_est_in, const float *g_est_out, const float *g_gait_out,
                                       float *g_st, float *g_swing_in, float *g_swing_vel_in, float *g_fe_in, int *g_flags);
__global__ void qr_swing_action_kernel(int n, SwingModeDesc M, EstimatorDesc D, int stop, const float *g_est_in, const float *g_est_out, const float *g_gait_out,
                                       const float *g_gait_state, float *g_st, float *g_out, int *g_flags);
__global__ void qr_stance_update_kernel(int n, StanceDesc S, float current_time, int stop, int reset, const float *g_est_in, const float *g_est_out,
                                        const float *g_ground, const float *g_rpy, const float *g_gait_out, const float *g_gait_state, const float *g_cmd,
                                        float *g_st, float *g_vmc_in, float *g_ratio, float *g_out);
__global__ void qr_stance_command_kernel(int n, StanceDesc S, int stop, const float *g_vmc_in, const float *g_stance_out, const float *g_tau,
                                         const float *g_swing_q, const float *g_swing_flag, float *g_cmd);
__global__ void qr_pose_plan_kernel(int n, PosePlanDesc D, int event, const int *g_event, int reset, const float *g_est_in, const float *g_est_out,
                                    const float *g_ground, const float *g_rpy, const float *g_walk, float *g_state, float *g_cmd, float *g_out, int *g_flags);
__global__ void qr_pack_state_kernel(int n, float c0, float c1, float c2, const float *g_in, const float *g_est, const float *g_rpy, float *g_mpc, float *g_fb);
__global__ void qr_estimator_kernel(int n, EstimatorDesc D, const float *g_in, const unsigned *g_tick, double *st, float *g_out);
__global__ void qr_vmc_kernel(VmcLaunch P, const int *type_id, const float *g_in, const float *g_q, float *g_force, float *g_tau, int *g_status);
__global__ void qr_frontend_kernel(int n, int horizon, int numHorizonL, float dt, float dtMPC, const float *fin, float *fst, float *g_traj,
                                   float *g_gait, float *g_cmd, int *g_updated);
__global__ void qr_wbc_kernel(int n, const WbcConst *types, const int *type_id, const float *g_state, const float *g_cmd,
                              float *g_prev, float *g_tau, float *g_qdes, int *g_status, float *g_dbg, int merge_tau, int status_or, long long *dbgT,
                              const float *g_fr, int type_ready, int epilogue, float *g_qp, WbcPipe pipe);
__global__ void qr_wbc_kernel_dbg(int n, const WbcConst *types, const int *type_id, const float *g_state, const float *g_cmd,
                                  float *g_prev, float *g_tau, float *g_qdes, int *g_status, float *g_dbg, int merge_tau, int status_or, long long *dbgT,
                                  const float *g_fr, int type_ready, int epilogue, float *g_qp, WbcPipe pipe);
}

// ---------------------------------------------------------------------------------------------
// BuildDynamicModel (QS/robots/qr_robot_a1_sim.cpp:176-343; the Lite3 file is a literal copy) reduced
// to rigid-body parameters.  Literals are the reference's float literals, evaluated in double.
// ---------------------------------------------------------------------------------------------
namespace {
struct RB { double m, h[3], I[6]; };     // I: xx yy zz xy xz yz about the frame origin
RB make_rb(double m, const double c[3], const double Ic[9])
{   // SpatialInertia(mass, com, inertia), QI/dynamics/spatial.hpp:390-398: Ibar = I + m [c]x[c]x^T
    RB r; r.m = m;
    for (int i = 0; i < 3; ++i) r.h[i] = m * c[i];
    const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    double Ib[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Ib[i][j] = Ic[3 * i + j] + m * ((i == j ? cc : 0.0) - c[i] * c[j]);
    r.I[0] = Ib[0][0]; r.I[1] = Ib[1][1]; r.I[2] = Ib[2][2]; r.I[3] = Ib[0][1]; r.I[4] = Ib[0][2]; r.I[5] = Ib[1][2];
    return r;
}
RB flip_y(const RB &a)
{   // flipAlongAxis(Y), spatial.hpp:505-534: mirror y
    RB r = a;
    r.h[1] = -a.h[1];
    r.I[3] = -a.I[3];
    r.I[5] = -a.I[5];
    return r;
}
RB add_rb(const RB &a, const RB &b)
{
    RB r; r.m = a.m + b.m;
    for (int i = 0; i < 3; ++i) r.h[i] = a.h[i] + b.h[i];
    for (int i = 0; i < 6; ++i) r.I[i] = a.I[i] + b.I[i];
    return r;
}
void store_rb(double *dst, const RB &r)
{
    dst[0] = r.m; dst[1] = r.h[0]; dst[2] = r.h[1]; dst[3] = r.h[2];
    for (int i = 0; i < 6; ++i) dst[4 + i] = r.I[i];
}
void build_wbc_const(const qrgpu_model_desc &d, WbcConst &K)
{
    auto F = [](double x) { return (double)(float)x; };      // the reference's literals are floats
    const double u = F(1e-6);
    const double abadI[9] = {F(469.2) * u, F(-9.4) * u, F(-0.342) * u, F(-9.4) * u, F(807.5) * u, F(-0.466) * u, F(-0.342) * u, F(-0.466) * u, F(552.9) * u};
    const double abadC[3] = {F(-0.0033), 0, 0};
    const double hipI[9] = {F(5529) * u, F(4.825) * u, F(343.9) * u, F(4.825) * u, F(5139.3) * u, F(22.4) * u, F(343.9) * u, F(22.4) * u, F(1367.8) * u};
    const double hipC[3] = {F(-0.003237), F(-0.022327), F(-0.027326)};
    const double kneeI[9] = {F(2998) * u, 0, F(-141.2) * u, 0, F(3014) * u, 0, F(-141.2) * u, 0, F(32.4) * u};
    const double kneeC[3] = {F(0.006435), 0, F(-0.107)};
    const double bodyI[9] = {F(15853) * u, 0, 0, 0, F(37799) * u, 0, 0, 0, F(45654) * u};
    const double zero3[3] = {0, 0, 0};
    const double m_abad = F(0.696), m_hip = F(1.013), m_knee = F(0.166), m_body = 6.0;
    const RB abadL = make_rb(m_abad, abadC, abadI), hipL = make_rb(m_hip, hipC, hipI), knee = make_rb(m_knee, kneeC, kneeI);
    const RB abadR = flip_y(abadL), hipR = flip_y(hipL);
    const RB base = make_rb(m_body, zero3, bodyI);
    // rotors (:193-198, :244-247): mass 1e-8, inertia (1e-2 * 1e-6) * identity  (setIdentity() overrides 33/33/63)
    const double k_rot = (double)(float)(F(1e-2) * 1e-6), m_rot = F(1e-8);
    auto rotor_at = [&](double x, double y, double z) {
        const double c[3] = {x, y, z};
        const double I[9] = {k_rot, 0, 0, 0, k_rot, 0, 0, 0, k_rot};
        return make_rb(m_rot, c, I);
    };
    RB base_eff = base;
    const double arx = F(0.14), ary = F(0.047);
    for (int leg = 0; leg < 4; ++leg) base_eff = add_rb(base_eff, rotor_at((leg < 2 ? 1 : -1) * arx, ((leg & 1) ? 1 : -1) * ary, 0.0));
    const double hry = F(0.04);
    const RB abadR_eff = add_rb(abadR, rotor_at(0, -hry, 0)), abadL_eff = add_rb(abadL, rotor_at(0, hry, 0));
    const RB hipR_eff = add_rb(hipR, rotor_at(0, 0, 0)), hipL_eff = add_rb(hipL, rotor_at(0, 0, 0));
    store_rb(K.rb[QR_RB_BASE], base);          store_rb(K.rb[QR_RB_BASE_EFF], base_eff);
    store_rb(K.rb[QR_RB_ABAD + 0], abadR);     store_rb(K.rb[QR_RB_ABAD + 1], abadL);
    store_rb(K.rb[QR_RB_ABAD_EFF + 0], abadR_eff); store_rb(K.rb[QR_RB_ABAD_EFF + 1], abadL_eff);
    store_rb(K.rb[QR_RB_HIP + 0], hipR);       store_rb(K.rb[QR_RB_HIP + 1], hipL);
    store_rb(K.rb[QR_RB_HIP_EFF + 0], hipR_eff); store_rb(K.rb[QR_RB_HIP_EFF + 1], hipL_eff);
    store_rb(K.rb[QR_RB_KNEE], knee);
    K.abad_loc[0] = F(0.1805); K.abad_loc[1] = F(0.047); K.abad_loc[2] = 0.0;
    K.hip_l = d.hip_l; K.upper_l = d.upper_l; K.lower_l = d.lower_l; K.foot_y = F(0.004);
    K.k_rot = k_rot;
    const double pi_f = (double)(float)M_PI;                   // coordinateRotation(Z, float(M_PI)) (:299)
    K.hiprot_ex = -std::sin(pi_f); K.hiprot_ey = std::cos(pi_f);
    const double total = m_body + 4.0 * (m_abad + m_hip + m_knee);                  // totalNonRotorMass()
    K.max_fz = (double)(float)total * (double)9.81f;
    K.kp_pos = d.kp_body_pos; K.kd_pos = d.kd_body_pos; K.kp_ori = d.kp_body_ori; K.kd_ori = d.kd_body_ori;
    K.kp_foot = d.kp_foot; K.kd_foot = d.kd_foot;
    K.w_fb = d.weight_fb; K.w_fr = d.weight_fr; K.mu = d.mu;
}
}  // namespace

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

// A lane's buffers, counters and (lanes 1, 2) streams.  Counters start at zero and are never cleared.
int lane_create(qrgpu_ctx *c, Lane &L, bool own_stream, bool masked)
{
    if (L.d_order) return QRGPU_OK;
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
        L.own_stream = ok; L.masked = ok && masked;
    }
    if (ok && masked) ok = hipMemset(L.d_rescue + 2, 0xff, sizeof(int) * nb) == hipSuccess;      // (an entry reads -1 until it is written: MpcLaunch::rescue_taken)
    if (ok) { L.h_pre_count[0] = L.h_pre_count[1] = L.h_pre_count[2] = L.h_pre_count[3] = 0; }       // ([2] of lane 0: a pipelined tick's join gave up waiting)
    (void)hipDeviceSynchronize();          // (the fills went to the default stream: none of the context's streams waits for that one)
    return ok ? QRGPU_OK : QRGPU_ERR_ALLOC;
}
static void lane_destroy(Lane &L)
{
    if (L.stream && L.own_stream) { (void)hipStreamSynchronize(L.stream); }
    if (L.side_stream && (!L.own_stream || L.masked)) { (void)hipStreamSynchronize(L.side_stream); hipStreamDestroy(L.side_stream); }     // (lanes 1, 2 borrow lane 0's)
    if (L.stream && L.own_stream) hipStreamDestroy(L.stream);
    if (L.d_order) hipFree(L.d_order);
    if (L.d_rescue) hipFree(L.d_rescue);
    if (L.d_pre) hipFree(L.d_pre);
    if (L.d_skip) hipFree(L.d_skip);
    if (L.h_pre_count) hipHostFree(L.h_pre_count);
    if (L.d_started) hipFree(L.d_started);
    if (L.d_done_flag) hipFree(L.d_done_flag);
    if (L.d_qhead) hipFree(L.d_qhead);
    if (L.d_planned_done) hipFree(L.d_planned_done);
    if (L.d_go) hipFree(L.d_go);
    if (L.d_lane_done) hipFree(L.d_lane_done);
    if (L.d_main_done) hipFree(L.d_main_done);
    if (L.d_rescue_taken) hipFree(L.d_rescue_taken);
    if (L.d_cmd_tick) hipFree(L.d_cmd_tick);
    if (L.ev_fork) hipEventDestroy(L.ev_fork);
    if (L.ev_join) hipEventDestroy(L.ev_join);
    L = Lane{};
}

static int upload_wbc(qrgpu_ctx *c)
{
    if (!c->wbc_dirty) return QRGPU_OK;
    HIPCHK(c, hipMemcpyAsync(c->d_wbc, c->wbc_host, sizeof(WbcConst) * QR_MAX_TYPES, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->wbc_dirty = false;
    return QRGPU_OK;
}

int launch_wbc(qrgpu_ctx *c, int n, const int *d_type, const float *d_state, const float *d_cmd, float *d_prev, float *d_tau, float *d_qdes, int *d_status,
               const WbcOpts &o)
{
    if (!c || n <= 0 || n > c->max_batch || !d_state) return QRGPU_ERR_BAD_ARG;
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
    bool ok = stage_ok && hipMalloc(&c->d_wbc, sizeof(WbcConst) * QR_MAX_TYPES) == hipSuccess;
    const size_t nb = (size_t)max_batch;
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
    if (c->h_stage) hipHostFree(c->h_stage);
    else {
        if (c->d_in1) hipFree(c->d_in1);
        if (c->d_out1) hipFree(c->d_out1);
        if (c->d_st1) hipFree(c->d_st1);
    }
    if (c->d_wbc) hipFree(c->d_wbc);
    if (c->d_cost[0]) hipFree(c->d_cost[0]);
    if (c->d_cost[1]) hipFree(c->d_cost[1]);
    if (c->d_warm) hipFree(c->d_warm);
    if (c->d_flops) hipFree(c->d_flops);
    if (c->wbc_stream) hipStreamDestroy(c->wbc_stream);
    if (c->wbc_stream_hi) { (void)hipStreamSynchronize(c->wbc_stream_hi); hipStreamDestroy(c->wbc_stream_hi); }
    for (int k = 0; k < 2; ++k) if (c->ev_call[k]) hipEventDestroy(c->ev_call[k]);
    if (c->d_main_started) hipFree(c->d_main_started);
    if (c->d_ftime) hipFree(c->d_ftime);
    if (c->d_wbc_finished) hipFree(c->d_wbc_finished);
    if (c->d_gate_abort) hipFree(c->d_gate_abort);
    if (c->d_solved) hipFree(c->d_solved);
    if (c->d_wbc_done) hipFree(c->d_wbc_done);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    if (c->d_gather_done) hipFree(c->d_gather_done);
    if (c->d_tick_done) hipFree(c->d_tick_done);
    if (c->d_timeline) hipFree(c->d_timeline);
    if (c->d_tlr) hipFree(c->d_tlr);
    if (c->d_sinv_spill) hipFree(c->d_sinv_spill);
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
    if (!c || type_id < 0 || type_id >= QR_MAX_TYPES || !inertia || !weights) return QRGPU_ERR_BAD_ARG;
    if (horizon <= 0 || horizon > c->horizon_max) return QRGPU_ERR_BAD_ARG;
    // one horizon per context (the reference has one global problem size, qr_mpc_interface.cpp:35-104):
    // a different horizon re-sizes the problem and invalidates the other types' setup, as a second SetupProblem would
    if (c->mpc.horizon != horizon) for (int t = 0; t < QR_MAX_TYPES; ++t) if (t != type_id) c->mpc_ready[t] = false;
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
    if (!c || type_id < 0 || type_id >= QR_MAX_TYPES || !desc) return QRGPU_ERR_BAD_ARG;
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
    // the kernel needs somewhere to put the forces; use the head of d_g's robot 0 row?  No: own scratch.
    float *scratch = nullptr;
    HIPCHK(c, hipMalloc(&scratch, sizeof(float) * 12 * (size_t)n));
    MpcIO io = mpc_io(d_type_id, d_mpc_state, d_traj, d_gait, nullptr, scratch, nullptr, nullptr);
    io.dbgH = d_H; io.dbgG = d_g;
    int rc = launch_mpc(c, n, io);
    hipStreamSynchronize(c->stream);
    hipFree(scratch);
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

void qrgpu_estimator_desc_default(qrgpu_estimator_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->hip_l = 0.08505f; d->upper_l = 0.2f; d->lower_l = 0.2f;
    const float ho[12] = {0.1805f, -0.047f, 0.f, 0.1805f, 0.047f, 0.f, -0.1805f, -0.047f, 0.f, -0.1805f, 0.047f, 0.f};
    memcpy(d->hip_offset, ho, sizeof(ho));
    d->time_step = 0.002f; d->accelerometer_variance = 0.1f; d->sensor_variance = 0.1f; d->window = 120; d->body_height = 0.28f;
}

int qrgpu_estimator_state_doubles(int window) { return window > 0 ? 96 + 3 * window : 0; }

int qrgpu_estimator_update_batch(qrgpu_ctx *c, int n, const qrgpu_estimator_desc *desc, const float *d_est_in, const unsigned *d_tick,
                                 double *d_est_state, float *d_est_out)
{
    if (!c || n <= 0 || n > c->max_batch || !desc || !d_est_in || !d_tick || !d_est_state || !d_est_out) return QRGPU_ERR_BAD_ARG;
    if (desc->window <= 0 || desc->window > 4096) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    EstimatorDesc D;
    D.hip_l = desc->hip_l; D.upper_l = desc->upper_l; D.lower_l = desc->lower_l;
    memcpy(D.hip_offset, desc->hip_offset, sizeof(D.hip_offset));
    D.time_step = desc->time_step; D.accelerometer_variance = desc->accelerometer_variance; D.sensor_variance = desc->sensor_variance;
    D.window = desc->window; D.body_height = desc->body_height;
    hipLaunchKernelGGL(qr_estimator_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, D, d_est_in, d_tick, d_est_state, d_est_out);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

void qrgpu_gait_desc_default(qrgpu_gait_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof(*d));
    for (int l = 0; l < 4; ++l) { d->stance_duration[l] = 0.5f; d->duty_factor[l] = 0.6f; d->initial_leg_state[l] = 1; }
    d->initial_leg_phase[0] = 0.5f; d->initial_leg_phase[3] = 0.5f;
    d->contact_detection_phase_threshold = 0.5f; d->wait_time = 1.0f; d->advanced_trot = 1;
}

int qrgpu_gait_update_batch(qrgpu_ctx *c, int n, const qrgpu_gait_desc *desc, float current_time, int robot_stop, int reset, const float *d_contact,
                            float *d_gait_state, float *d_gait_out, float *d_fe_in)
{
    if (!c || n <= 0 || n > c->max_batch || !desc || !d_contact || !d_gait_state) return QRGPU_ERR_BAD_ARG;
    for (int l = 0; l < 4; ++l) if (!(desc->duty_factor[l] > 0.001f) || !(desc->stance_duration[l] > 0.f)) return QRGPU_ERR_BAD_ARG;   // USERDEFINED_SWING legs are not built
    HIPCHK(c, hipSetDevice(c->device));
    GaitDesc D;
    memcpy(D.stance_duration, desc->stance_duration, 16); memcpy(D.duty_factor, desc->duty_factor, 16); memcpy(D.initial_leg_phase, desc->initial_leg_phase, 16);
    memcpy(D.initial_leg_state, desc->initial_leg_state, 16);
    D.contact_detection_phase_threshold = desc->contact_detection_phase_threshold; D.wait_time = desc->wait_time; D.advanced_trot = desc->advanced_trot;
    hipLaunchKernelGGL(qr_gait_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, D, current_time, robot_stop, reset, d_contact, d_gait_state, d_gait_out, d_fe_in);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

void qrgpu_walk_gait_desc_default(qrgpu_walk_gait_desc *d)
{   // config/a1_sim/openloop_gait_generator.yaml, gait "walk"
    if (!d) return;
    memset(d, 0, sizeof(*d));
    for (int l = 0; l < 4; ++l) { d->stance_duration[l] = 7.5f; d->duty_factor[l] = 0.75f; d->initial_leg_state[l] = 1; }
    d->initial_leg_phase[0] = 0.5f; d->initial_leg_phase[1] = 0.f; d->initial_leg_phase[2] = 0.75f; d->initial_leg_phase[3] = 0.25f;
    d->contact_detection_phase_threshold = 0.1f;
    d->n_states = 4;
    d->state_switch[0] = 7; d->state_switch[1] = 6; d->state_switch[2] = 8; d->state_switch[3] = 5;
    d->state_ratio[0] = 0.2f; d->state_ratio[1] = 0.3f; d->state_ratio[2] = 0.3f; d->state_ratio[3] = 0.2f;
}

int qrgpu_walk_gait_update_batch(qrgpu_ctx *c, int n, const qrgpu_walk_gait_desc *desc, float current_time, int robot_stop, int reset,
                                 const float *d_contact, float *d_walk_state, float *d_walk_out, float *d_ratio, float *d_vmc_in)
{
    if (!c || n <= 0 || n > c->max_batch || !desc || !d_contact || !d_walk_state || reset < 0 || reset > 2) return QRGPU_ERR_BAD_ARG;
    if (desc->n_states < 1 || desc->n_states > 4) return QRGPU_ERR_BAD_ARG;
    for (int l = 0; l < 4; ++l) if (!(desc->duty_factor[l] > 0.001f) || !(desc->duty_factor[l] < 1.f) || !(desc->stance_duration[l] > 0.f)) return QRGPU_ERR_BAD_ARG;
    // the constructor's bookkeeping (qr_walk_gait_generator.cpp:87-157): sub-states below a ratio of 0.01 are dropped, the stance-like ones
    // in front of true_swing add up to its start, running sums in float
    WalkDesc D;
    memset(&D, 0, sizeof(D));
    float stand = 0.f;
    for (int k = 0; k < desc->n_states; ++k) {
        if (desc->state_ratio[k] < 0.01) continue;
        const int st = desc->state_switch[k];
        if (st != 5 && st != 6 && st != 7 && st != 8) return QRGPU_ERR_BAD_ARG;
        if (st == 8) D.true_swing_start_in_swing = stand; else stand += desc->state_ratio[k];
        D.que[D.nq] = st; D.ratio[D.nq] = desc->state_ratio[k]; ++D.nq;
    }
    if (D.nq < 1) return QRGPU_ERR_BAD_ARG;
    D.accum[0] = 0.f;
    for (int k = 0; k < D.nq; ++k) D.accum[k + 1] = D.accum[k] + D.ratio[k];
    if (!(fabsf(D.accum[D.nq] - 1.0f) < 1e-4f)) return QRGPU_ERR_BAD_ARG;       // "not vaild ratio definition" (:124)
    for (int l = 0; l < 4; ++l) {
        D.duty_factor[l] = desc->duty_factor[l]; D.initial_leg_phase[l] = desc->initial_leg_phase[l]; D.initial_leg_state[l] = desc->initial_leg_state[l];
        D.full[l] = desc->stance_duration[l] / desc->duty_factor[l];
        D.state_index0[l] = 0;
        if (desc->initial_leg_state[l] == 0) {
            const float ph = (desc->initial_leg_phase[l] - desc->duty_factor[l]) / desc->duty_factor[l];
            int k = 0;
            while (k < D.nq && ph > D.accum[k]) k++;
            D.state_index0[l] = k - 1 > 0 ? k - 1 : 0;
        }
    }
    D.contact_detection_phase_threshold = desc->contact_detection_phase_threshold;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_walk_gait_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, D, current_time, robot_stop, reset, d_contact, d_walk_state, d_walk_out,
                       d_ratio, d_vmc_in);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

int qrgpu_ground_update_batch(qrgpu_ctx *c, int n, int reset, const float *d_ground_in, double *d_ground_state, float *d_ground_out, float *d_est_in)
{
    if (!c || n <= 0 || n > c->max_batch || !d_ground_in || !d_ground_state) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_ground_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, reset, d_ground_in, d_ground_state, d_ground_out, d_est_in);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

void qrgpu_foothold_desc_default(qrgpu_foothold_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof(*d));
    const float ho[12] = {0.1805f, -0.047f, 0.f, 0.1805f, 0.047f, 0.f, -0.1805f, -0.047f, 0.f, -0.1805f, 0.047f, 0.f};
    const float hp[12] = {0.185f, -0.135f, 0.f, 0.185f, 0.135f, 0.f, -0.185f, -0.135f, 0.f, -0.185f, 0.135f, 0.f};     // config/a1_sim/a1_sim.yaml:40-43
    memcpy(d->hip_offset, ho, sizeof(ho)); memcpy(d->default_hip_position, hp, sizeof(hp));
    d->hip_l = 0.08505f; d->swing_kp[0] = d->swing_kp[1] = d->swing_kp[2] = 0.16f; d->foot_clearance = 0.01f;
}

int qrgpu_footholds_batch(qrgpu_ctx *c, int n, const qrgpu_foothold_desc *desc, const float *d_fh_in, const float *d_gait_state,
                          const float *d_gait_out, float *d_swing_in)
{
    if (!c || n <= 0 || n > c->max_batch || !desc || !d_fh_in || !d_swing_in) return QRGPU_ERR_BAD_ARG;
    if ((d_gait_state == nullptr) != (d_gait_out == nullptr)) return QRGPU_ERR_BAD_ARG;      // both or neither
    HIPCHK(c, hipSetDevice(c->device));
    FootholdDesc D;
    memcpy(D.hip_offset, desc->hip_offset, sizeof(D.hip_offset)); memcpy(D.default_hip_position, desc->default_hip_position, sizeof(D.default_hip_position));
    D.hip_l = desc->hip_l; memcpy(D.swing_kp, desc->swing_kp, sizeof(D.swing_kp)); D.foot_clearance = desc->foot_clearance;
    hipLaunchKernelGGL(qr_foothold_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, D, d_fh_in, d_gait_state, d_gait_out, d_swing_in);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

int qrgpu_swing_velocity_batch(qrgpu_ctx *c, int n, const qrgpu_estimator_desc *desc, const qrgpu_swing_velocity_desc *vdesc, const float *d_swing_vel_in,
                               float *d_out)
{
    if (!c || n <= 0 || n > c->max_batch || !desc || !vdesc || !d_swing_vel_in || !d_out) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    EstimatorDesc D;
    memset(&D, 0, sizeof(D));
    D.hip_l = desc->hip_l; D.upper_l = desc->upper_l; D.lower_l = desc->lower_l;
    memcpy(D.hip_offset, desc->hip_offset, sizeof(D.hip_offset));
    SwingVelDesc V;
    memcpy(V.hip_pos_com, vdesc->hip_position_com, sizeof(V.hip_pos_com)); memcpy(V.stance_duration, vdesc->stance_duration, sizeof(V.stance_duration));
    memcpy(V.swing_kp, vdesc->swing_kp, sizeof(V.swing_kp)); V.desired_height = vdesc->desired_height;
    hipLaunchKernelGGL(qr_swing_velocity_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, D, V, d_swing_vel_in, d_out);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

int qrgpu_swing_targets_batch(qrgpu_ctx *c, int n, const qrgpu_estimator_desc *desc, const float *d_swing_in, float *d_wbc_cmd, float *d_foot_target_world,
                              float *d_qdes)
{
    if (!c || n <= 0 || n > c->max_batch || !desc || !d_swing_in || (!d_wbc_cmd && !d_foot_target_world && !d_qdes)) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    EstimatorDesc D;
    memset(&D, 0, sizeof(D));
    D.hip_l = desc->hip_l; D.upper_l = desc->upper_l; D.lower_l = desc->lower_l;
    memcpy(D.hip_offset, desc->hip_offset, sizeof(D.hip_offset));
    hipLaunchKernelGGL(qr_swing_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, D, d_swing_in, d_wbc_cmd, d_foot_target_world, d_qdes);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

void qrgpu_swing_mode_desc_default(qrgpu_swing_mode_desc *d, int mode)
{   // config/a1_sim: terrain.yaml (terrain_type 3, gaps 0.51 1.31 1.91, gap_width 0.14) after qrGroundSurfaceEstimator::Reset (:73-100)
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->mode = mode; d->is_sim = 1; d->foothold_delta = 0.10f;
    d->terrain = mode == QRGPU_MODE_POSITION ? 1 : mode == QRGPU_MODE_ADVANCED_TROT ? 2 : 3;
    d->gap_width = 0.14f;
    if (mode == QRGPU_MODE_POSITION) { d->n_gaps = 3; d->gap_distance[0] = 0.51f; d->gap_distance[1] = 1.31f; d->gap_distance[2] = 1.91f; }
}

static bool swing_mode_desc(const qrgpu_swing_mode_desc *d, SwingModeDesc &M)
{
    if (!d || d->mode < 0 || d->mode > 3 || d->n_gaps < 0 || d->n_gaps > QRGPU_SWING_MAX_GAPS) return false;
    static_assert(QRGPU_SWING_MAX_GAPS == QR_SWING_MAX_GAPS && QRGPU_SWING_MAX_PLAN == QR_SWING_MAX_PLAN, "swing state layout");
    memset(&M, 0, sizeof(M));
    M.mode = d->mode; M.terrain = d->terrain; M.is_sim = d->is_sim; M.foothold_delta = d->foothold_delta;
    M.n_gaps = d->terrain == 1 ? d->n_gaps : 0;                // the stepper copies gaps on PLUM_PILES only (qr_foot_stepper.cpp:31-38)
    memcpy(M.gap_distance, d->gap_distance, sizeof(M.gap_distance)); M.gap_width = d->gap_width;
    return true;
}

int qrgpu_swing_update_batch(qrgpu_ctx *c, int n, const qrgpu_swing_mode_desc *desc, int reset, int robot_stop, const float *d_est_in,
                             const float *d_est_out, const float *d_gait_out, const float *d_gait_state, float *d_swing_state,
                             float *d_swing_in, float *d_swing_vel_in, float *d_fe_in, int *d_swing_flags)
{
    (void)d_gait_state;
    SwingModeDesc M;
    if (!c || n <= 0 || n > c->max_batch || !swing_mode_desc(desc, M) || reset < 0 || reset > 2) return QRGPU_ERR_BAD_ARG;
    if (!d_est_in || !d_est_out || !d_gait_out || !d_swing_state || !d_swing_flags) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_swing_update_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, M, reset, robot_stop ? 1 : 0, d_est_in, d_est_out, d_gait_out,
                       d_swing_state, d_swing_in, d_swing_vel_in, d_fe_in, d_swing_flags);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

int qrgpu_swing_action_batch(qrgpu_ctx *c, int n, const qrgpu_swing_mode_desc *desc, const qrgpu_estimator_desc *geom, int robot_stop,
                             const float *d_est_in, const float *d_est_out, const float *d_gait_out, const float *d_gait_state,
                             float *d_swing_state, float *d_out, int *d_swing_flags)
{
    SwingModeDesc M;
    if (!c || n <= 0 || n > c->max_batch || !swing_mode_desc(desc, M) || !geom) return QRGPU_ERR_BAD_ARG;
    if (M.mode != QRGPU_MODE_POSITION && M.mode != QRGPU_MODE_WALK) return QRGPU_ERR_BAD_ARG;      // the other two have kernels of their own
    if (!d_est_in || !d_est_out || !d_gait_out || !d_swing_state || !d_out || !d_swing_flags) return QRGPU_ERR_BAD_ARG;
    if (M.mode == QRGPU_MODE_POSITION && !d_gait_state) return QRGPU_ERR_BAD_ARG;                   // allowSwitchLegState
    HIPCHK(c, hipSetDevice(c->device));
    EstimatorDesc D;
    memset(&D, 0, sizeof(D));
    D.hip_l = geom->hip_l; D.upper_l = geom->upper_l; D.lower_l = geom->lower_l;
    memcpy(D.hip_offset, geom->hip_offset, sizeof(D.hip_offset));
    hipLaunchKernelGGL(qr_swing_action_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, M, D, robot_stop ? 1 : 0, d_est_in, d_est_out, d_gait_out,
                       d_gait_state, d_swing_state, d_out, d_swing_flags);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

int qrgpu_pack_state_batch(qrgpu_ctx *c, int n, const float com_offset[3], const float *d_est_in, const float *d_est_out, const float *d_rpy,
                           float *d_mpc_state, float *d_fb_state)
{
    if (!c || n <= 0 || n > c->max_batch || !com_offset || !d_est_in || !d_est_out || (!d_mpc_state && !d_fb_state)) return QRGPU_ERR_BAD_ARG;
    if (d_mpc_state && !d_rpy) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_pack_state_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, com_offset[0], com_offset[1], com_offset[2], d_est_in, d_est_out,
                       d_rpy, d_mpc_state, d_fb_state);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
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
    if (!c || !d || type_id < 0 || type_id >= QR_MAX_TYPES) return QRGPU_ERR_BAD_ARG;
    if (!(d->mass > 0.f)) return QRGPU_ERR_BAD_ARG;
    VmcType &t = c->vmc.type[type_id];
    t.mass = d->mass;
    memcpy(t.inertia, d->inertia, sizeof(t.inertia));
    memcpy(t.acc_weight, d->acc_weight, sizeof(t.acc_weight));
    t.reg_weight = d->reg_weight; t.friction = d->friction; t.fmin_ratio = d->fmin_ratio; t.fmax_ratio = d->fmax_ratio;
    t.hip_l = d->hip_l; t.upper_l = d->upper_l; t.lower_l = d->lower_l;
    c->vmc_ready[type_id] = true;
    return QRGPU_OK;
}

static int launch_vmc(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_vmc_in, const float *d_ratio, const float *d_q, float *d_force,
                      float *d_tau, int *d_status)
{
    if (!c || n <= 0 || n > c->max_batch || !d_vmc_in || !d_force) return QRGPU_ERR_BAD_ARG;
    if (d_tau && !d_q) return QRGPU_ERR_BAD_ARG;
    if (!(d_type_id ? ready_mask(c->vmc_ready) != 0 : c->vmc_ready[0])) return QRGPU_ERR_NOT_SETUP;
    HIPCHK(c, hipSetDevice(c->device));
    VmcLaunch P = c->vmc;
    P.n = n; P.ratio = d_ratio; P.type_ready = ready_mask(c->vmc_ready);
    hipLaunchKernelGGL(qr_vmc_kernel, dim3(8 * ((n + 7) / 8)), dim3(64), 0, c->stream, P, d_type_id, d_vmc_in, d_q, d_force, d_tau, d_status);
    HIPCHK(c, hipGetLastError());
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

void qrgpu_stance_desc_default(qrgpu_stance_desc *d, int mode)
{   // config/a1_sim/stance_leg_controller.yaml (stance_leg_params of the mode), config/user_parameters.yaml:19-21,40, config/a1_sim/a1_sim.yaml:14,62-67
    // (qr_robot_a1_sim.cpp:104-105), terrain as qrgpu_swing_mode_desc_default
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->mode = mode;
    d->terrain = mode == QRGPU_MODE_POSITION ? 1 : mode == QRGPU_MODE_ADVANCED_TROT ? 2 : 3;
    d->force_in_world = 1;
    static const float KP[4][6] = {{100.f, 100.f, 100.f, 200.f, 200.f, 0.f}, {100.f, 200.f, 200.f, 100.f, 100.f, 200.f}, {100.f, 200.f, 100.f, 100.f, 100.f, 200.f},
                                   {100.f, 100.f, 100.f, 200.f, 200.f, 100.f}};
    static const float KD[4][6] = {{20.f, 20.f, 10.f, 20.f, 20.f, 25.f}, {40.f, 30.f, 10.f, 10.f, 10.f, 30.f}, {40.f, 30.f, 10.f, 10.f, 10.f, 30.f},
                                   {30.f, 20.f, 10.f, 20.f, 20.f, 25.f}};
    const int m = mode >= 0 && mode <= 3 ? mode : 0;
    for (int k = 0; k < 6; ++k) {
        d->kp[k] = KP[m][k]; d->kd[k] = KD[m][k];
        d->max_ddq[k] = (m == 3 || k < 3) ? 10.f : 20.f;
        d->min_ddq[k] = -d->max_ddq[k];
    }
    d->desired_height = 0.27f;
    d->body_height = 0.28f;
    for (int j = 0; j < 12; ++j) { d->motor_kp[j] = 100.f; d->motor_kd[j] = (j % 3 == 0) ? 1.f : 2.f; }
}

static bool stance_desc(const qrgpu_stance_desc *d, StanceDesc &S)
{
    if (!d || d->mode < 0 || d->mode > 3 || d->terrain < 0 || d->terrain > 4) return false;
    memset(&S, 0, sizeof(S));
    S.mode = d->mode; S.terrain = d->terrain; S.force_in_world = d->force_in_world ? 1 : 0;
    memcpy(S.kp, d->kp, sizeof(S.kp)); memcpy(S.kd, d->kd, sizeof(S.kd));
    memcpy(S.max_ddq, d->max_ddq, sizeof(S.max_ddq)); memcpy(S.min_ddq, d->min_ddq, sizeof(S.min_ddq));
    S.desired_height = d->desired_height; memcpy(S.desired_speed, d->desired_speed, sizeof(S.desired_speed));
    S.desired_twisting_speed = d->desired_twisting_speed; S.body_height = d->body_height; S.pose_reset_time = d->pose_reset_time;
    memcpy(S.motor_kp, d->motor_kp, sizeof(S.motor_kp)); memcpy(S.motor_kd, d->motor_kd, sizeof(S.motor_kd));
    return true;
}

static bool stance_world(const StanceDesc &S) { return S.mode == QRGPU_MODE_WALK || (S.mode == QRGPU_MODE_ADVANCED_TROT && S.force_in_world); }

static int stance_update_check(const qrgpu_ctx *c, int n, const qrgpu_stance_desc *desc, StanceDesc &S, const float *d_est_in, const float *d_est_out,
                               const float *d_ground_out, const float *d_rpy, const float *d_gait_out, const float *d_gait_state, const float *d_stance_cmd,
                               const float *d_stance_state)
{
    if (!c || n <= 0 || n > c->max_batch || !stance_desc(desc, S)) return QRGPU_ERR_BAD_ARG;
    if (!d_est_in || !d_est_out || !d_ground_out || !d_rpy || !d_gait_out || !d_stance_cmd || !d_stance_state) return QRGPU_ERR_BAD_ARG;
    if ((S.mode == QRGPU_MODE_POSITION || S.mode == QRGPU_MODE_ADVANCED_TROT) && !d_gait_state) return QRGPU_ERR_BAD_ARG;   // allowSwitchLegState
    return QRGPU_OK;
}

static int stance_command_check(const qrgpu_ctx *c, int n, const StanceDesc &S, const float *d_vmc_in, const float *d_stance_out, const float *d_tau,
                                const float *d_swing_q, const float *d_swing_flag, const float *d_motor_cmd)
{
    if (!c || n <= 0 || n > c->max_batch || !d_tau || !d_motor_cmd) return QRGPU_ERR_BAD_ARG;
    if (S.mode == QRGPU_MODE_WALK && (!d_vmc_in || !d_stance_out)) return QRGPU_ERR_BAD_ARG;             // contacts, N, moveBasePhase
    if ((d_swing_q == nullptr) != (d_swing_flag == nullptr)) return QRGPU_ERR_BAD_ARG;                   // both or neither
    return QRGPU_OK;
}

int qrgpu_stance_update_batch(qrgpu_ctx *c, int n, const qrgpu_stance_desc *desc, float current_time, int robot_stop, int reset, const float *d_est_in,
                              const float *d_est_out, const float *d_ground_out, const float *d_rpy, const float *d_gait_out, const float *d_gait_state,
                              const float *d_stance_cmd, float *d_stance_state, float *d_vmc_in, float *d_ratio, float *d_stance_out)
{
    StanceDesc S;
    const int e = stance_update_check(c, n, desc, S, d_est_in, d_est_out, d_ground_out, d_rpy, d_gait_out, d_gait_state, d_stance_cmd, d_stance_state);
    if (e != QRGPU_OK) return e;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_stance_update_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, S, current_time, robot_stop ? 1 : 0, reset ? 1 : 0, d_est_in,
                       d_est_out, d_ground_out, d_rpy, d_gait_out, d_gait_state, d_stance_cmd, d_stance_state, d_vmc_in, d_ratio, d_stance_out);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

int qrgpu_stance_command_batch(qrgpu_ctx *c, int n, const qrgpu_stance_desc *desc, int robot_stop, const float *d_vmc_in, const float *d_stance_out,
                               const float *d_tau, const float *d_swing_q, const float *d_swing_flag, float *d_motor_cmd)
{
    StanceDesc S;
    if (!stance_desc(desc, S)) return QRGPU_ERR_BAD_ARG;
    const int e = stance_command_check(c, n, S, d_vmc_in, d_stance_out, d_tau, d_swing_q, d_swing_flag, d_motor_cmd);
    if (e != QRGPU_OK) return e;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_stance_command_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, S, robot_stop ? 1 : 0, d_vmc_in, d_stance_out, d_tau, d_swing_q,
                       d_swing_flag, d_motor_cmd);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

int qrgpu_stance_tick_batch(qrgpu_ctx *c, int n, const qrgpu_stance_desc *desc, float current_time, int robot_stop, int reset, const int *d_type_id,
                            const float *d_est_in, const float *d_est_out, const float *d_ground_out, const float *d_rpy, const float *d_gait_out,
                            const float *d_gait_state, const float *d_stance_cmd, float *d_stance_state, float *d_vmc_in, float *d_ratio, float *d_stance_out,
                            float *d_force, float *d_tau, int *d_status, const float *d_swing_q, const float *d_swing_flag, float *d_motor_cmd)
{
    StanceDesc S;
    int e = stance_update_check(c, n, desc, S, d_est_in, d_est_out, d_ground_out, d_rpy, d_gait_out, d_gait_state, d_stance_cmd, d_stance_state);
    if (e != QRGPU_OK) return e;
    const bool world = stance_world(S);
    if (!d_vmc_in || !d_force || (world && !d_ratio)) return QRGPU_ERR_BAD_ARG;
    e = stance_command_check(c, n, S, d_vmc_in, d_stance_out, d_tau, d_swing_q, d_swing_flag, d_motor_cmd);
    if (e != QRGPU_OK) return e;
    if (!(d_type_id ? ready_mask(c->vmc_ready) != 0 : c->vmc_ready[0])) return QRGPU_ERR_NOT_SETUP;
    e = qrgpu_stance_update_batch(c, n, desc, current_time, robot_stop, reset, d_est_in, d_est_out, d_ground_out, d_rpy, d_gait_out, d_gait_state, d_stance_cmd,
                                  d_stance_state, d_vmc_in, d_ratio, d_stance_out);
    if (e != QRGPU_OK) return e;
    const float *d_q = d_est_in + (size_t)17 * n;                                                       // motor angles: rows 17-28 of est_in
    e = launch_vmc(c, n, d_type_id, d_vmc_in, world ? d_ratio : nullptr, d_q, d_force, d_tau, d_status);
    if (e != QRGPU_OK) return e;
    return qrgpu_stance_command_batch(c, n, desc, robot_stop, d_vmc_in, d_stance_out, d_tau, d_swing_q, d_swing_flag, d_motor_cmd);
}

void qrgpu_pose_plan_desc_default(qrgpu_pose_plan_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof(*d));
    for (int leg = 0; leg < 4; ++leg) { d->rBH[3 * leg] = leg < 2 ? 0.18f : -0.18f; d->rBH[3 * leg + 1] = (leg & 1) ? 0.047f : -0.047f; }
    d->l_min = 0.22f; d->l_max = 0.35f; d->omega = 0.5f; d->eps = 0.1f; d->body_height = 0.27f; d->loops = QRGPU_POSE_MAX_LOOPS;
}

int qrgpu_pose_plan_batch(qrgpu_ctx *c, int n, const qrgpu_pose_plan_desc *desc, int event, const int *d_event, int reset, const float *d_est_in,
                          const float *d_est_out, const float *d_ground_out, const float *d_rpy, const float *d_walk_out, float *d_pose_state,
                          float *d_stance_cmd, float *d_pose_out, int *d_pose_flags)
{
    if (!c || n <= 0 || n > c->max_batch || !desc || event < 0 || event > 3) return QRGPU_ERR_BAD_ARG;
    if (!d_est_in || !d_est_out || !d_ground_out || !d_rpy || !d_walk_out || !d_pose_state || !d_stance_cmd || !d_pose_flags) return QRGPU_ERR_BAD_ARG;
    if (!d_event && event == 0 && !reset) return QRGPU_OK;                                              // nothing to do: no launch
    static_assert(QRGPU_POSE_STATE_ROWS == QR_POSE_STATE_ROWS && QRGPU_POSE_OUT_ROWS == QR_POSE_OUT_ROWS && QRGPU_POSE_MAX_LOOPS == QR_POSE_MAX_LOOPS, "pose rows");
    static_assert(QRGPU_PP_FEW_CONTACTS == QR_PP_FEW_CONTACTS && QRGPU_PP_NOT_PD == QR_PP_NOT_PD && QRGPU_PP_INFEASIBLE == QR_PP_INFEASIBLE &&
                  QRGPU_PP_LAMBDA_GROWN == QR_PP_LAMBDA_GROWN && QRGPU_PP_NONCONVEX == QR_PP_NONCONVEX && QRGPU_PP_NAN == QR_PP_NAN &&
                  QRGPU_PP_MAXITER == QR_PP_MAXITER, "pose flags");
    PosePlanDesc D;
    memcpy(D.rBH, desc->rBH, sizeof(D.rBH));
    D.l_min = desc->l_min; D.l_max = desc->l_max; D.omega = desc->omega; D.eps = desc->eps; D.body_height = desc->body_height; D.loops = desc->loops;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_pose_plan_kernel, dim3(8 * ((n + 7) / 8)), dim3(64), 0, c->stream, n, D, event, d_event, reset ? 1 : 0, d_est_in, d_est_out,
                       d_ground_out, d_rpy, d_walk_out, d_pose_state, d_stance_cmd, d_pose_out, d_pose_flags);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

int qrgpu_mpc_frontend_batch(qrgpu_ctx *c, int n, int num_horizon_l, float dt_ctrl, float dt_mpc, const float *d_fe_in, float *d_fe_state,
                             float *d_traj, float *d_gait, float *d_wbc_cmd, int *d_mpc_updated)
{
    if (!c || n <= 0 || n > c->max_batch || !d_fe_in || !d_fe_state || !d_traj || !d_gait) return QRGPU_ERR_BAD_ARG;
    if (num_horizon_l <= 0 || !(dt_ctrl > 0.f) || !(dt_mpc > 0.f)) return QRGPU_ERR_BAD_ARG;
    if (!c->mpc_ready[0]) return QRGPU_ERR_NOT_SETUP;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_frontend_kernel, dim3((n + 63) / 64), dim3(64, c->mpc.horizon), 0, c->stream, n, c->mpc.horizon, num_horizon_l, dt_ctrl, dt_mpc,
                       d_fe_in, d_fe_state, d_traj, d_gait, d_wbc_cmd, d_mpc_updated);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
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
    if (type_id < 0 || type_id >= QR_MAX_TYPES || !c->mpc_ready[type_id]) return QRGPU_ERR_NOT_SETUP;
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
    if (type_id < 0 || type_id >= QR_MAX_TYPES || !c->wbc_ready[type_id]) return QRGPU_ERR_NOT_SETUP;
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
    if (type_id < 0 || type_id >= QR_MAX_TYPES || !c->vmc_ready[type_id]) return QRGPU_ERR_NOT_SETUP;
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

int qrgpu_debug_cycles(qrgpu_ctx *c, long long *host_out /* [n][8] or NULL to disable */, int n)
{   // undocumented diagnostic: phase cycle stamps of the last MPC launch (enable by calling once with NULL first; NULL with n < 0 switches them off again)
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!host_out && n < 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->d_dbg_cycles) hipFree(c->d_dbg_cycles);
        if (c->d_dbg_cycles_wbc) hipFree(c->d_dbg_cycles_wbc);
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
    HIPCHK(c, hipMemcpy(host_out, c->d_timeline + 512, sizeof(long long) * 256, hipMemcpyDeviceToHost));      // [64][2] gate up / open, then [64][2] planned launch first start / last end
    return QRGPU_OK;
}

int qrgpu_debug_timeline_solves(qrgpu_ctx *c, long long *host_out /* [2][16][1024]: per epoch & 15 and robot: (publish time << 8 | launch kind), (cross-tick wait << 8 | kind | 8 gave up) */)
{
    if (!c || !c->d_timeline || !host_out) return QRGPU_ERR_BAD_ARG;
    (void)hipDeviceSynchronize();
    HIPCHK(c, hipMemcpy(host_out, c->d_timeline + 768, sizeof(long long) * 2 * 16 * 1024, hipMemcpyDeviceToHost));
    return QRGPU_OK;
}

int qrgpu_debug_timeline_plans(qrgpu_ctx *c, long long *host_out /* [64][64] list length each planned workgroup read, then [64] the length each tick's planning left */)
{
    if (!c || !c->d_timeline || !host_out) return QRGPU_ERR_BAD_ARG;
    (void)hipDeviceSynchronize();
    HIPCHK(c, hipMemcpy(host_out, c->d_timeline + 768 + 32768, sizeof(long long) * (4096 + 64), hipMemcpyDeviceToHost));
    return QRGPU_OK;
}

int qrgpu_debug_timeline_trace(qrgpu_ctx *c, long long *host_out /* [16][1024] what happened to each robot in each epoch & 15 (QR_TRACE bits) */)
{
    if (!c || !c->d_timeline || !host_out) return QRGPU_ERR_BAD_ARG;
    (void)hipDeviceSynchronize();
    HIPCHK(c, hipMemcpy(host_out, c->d_timeline + 768 + 32768 + 4096 + 64, sizeof(long long) * 16384, hipMemcpyDeviceToHost));
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
    if (!c->d_timeline) { HIPCHK(c, hipMalloc(&c->d_timeline, sizeof(long long) * (768 + 2 * 16 * 1024 + 4096 + 64 + 16384))); HIPCHK(c, hipMemset(c->d_timeline, 0, sizeof(long long) * (768 + 2 * 16 * 1024 + 4096 + 64 + 16384))); }
    {   // (the planned launch's first start is an atomicMin)
        long long ext[128];
        for (int e = 0; e < 64; ++e) { ext[2 * e] = 0x7fffffffffffffffLL; ext[2 * e + 1] = 0; }
        HIPCHK(c, hipMemcpy(c->d_timeline + 640, ext, sizeof(ext), hipMemcpyHostToDevice));
    }
    if (!c->d_tlr) HIPCHK(c, hipMalloc(&c->d_tlr, sizeof(int) * 4 * (size_t)c->max_batch));
    if (host_out) HIPCHK(c, hipMemcpy(host_out, c->d_timeline, sizeof(long long) * 512, hipMemcpyDeviceToHost));
    long long init[512];
    for (int e = 0; e < 64; ++e) for (int k = 0; k < 8; ++k) init[e * 8 + k] = (k == 0 || k == 3 || k == 5) ? 0x7fffffffffffffffLL : 0;
    HIPCHK(c, hipMemcpy(c->d_timeline, init, sizeof(init), hipMemcpyHostToDevice));
    if (host_out) host_out[512] = (long long)c->tick_epoch;
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
    double *d = nullptr;
    HIPCHK(c, hipMalloc(&d, 256 * sizeof(double)));
    hipLaunchKernelGGL(qr_selftest_kernel, dim3(1), dim3(64), 0, c->stream, d);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(host_out256, d, 256 * sizeof(double), hipMemcpyDeviceToHost));
    hipFree(d);
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
