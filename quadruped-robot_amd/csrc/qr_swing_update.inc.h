// Included twice by qr_swing_modes_kernel.hip: with QR_STAGE_PR 0 this is the kernel text as it always was (the compiled code is instruction for instruction
// that of the single definition it replaces); with QR_STAGE_PR 1 the same text makes the per-robot form NAME_pr (qrgpu_set_stage_reset), which takes the
// binding as one more argument, SR.  Only the lines between #if QR_STAGE_PR and #endif differ.  A function template on the same switch, force-inlined
// into both kernels, did not reproduce the old kernels' code.  No include guard.

// Reset (reset != 0) and Update of the swing-leg controller and its foothold planner: the lift-off memory of every mode, the footholds
// and walk trajectories of the position and walk modes.  Optionally writes the lift-off rows the ADVANCED_TROT / VELOCITY kernels read.
__global__ void __launch_bounds__(64) QR_STAGE_K(qr_swing_update_kernel)(int n, qrgpu_swing_mode_desc M, int reset, int stop, const float *__restrict__ g_est_in,
                                                             const float *__restrict__ g_est_out, const float *__restrict__ g_gait_out, float *__restrict__ g_st,
                                                             float *__restrict__ g_swing_in, float *__restrict__ g_swing_vel_in, float *__restrict__ g_fe_in,
                                                             int *__restrict__ g_flags QR_STAGE_PARAM)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
#if QR_STAGE_PR          // the lane's own reset level: the call's scalar reset wins, then the bound level of a masked robot
    if (!reset && stage_masked(SR, i)) reset = SR.level;
#endif
#define ST(f) g_st[(size_t)(f) * N + i]
    const float q[4] = {g_est_in[6 * N + i], g_est_in[7 * N + i], g_est_in[8 * N + i], g_est_in[9 * N + i]};
    const float bp[3] = {g_est_out[36 * N + i], g_est_out[37 * N + i], g_est_out[38 * N + i]};
    float Rq[3][3];                                                           // invertRigidTransform's rotation (Eigen)
    quat_to_rot(q[0], q[1], q[2], q[3], Rq);
    // feet in the base frame and GetFootPositionsInWorldFrame (:222-230), read per leg (a runtime leg index must not select a private array)
#define LOC(l, r) g_est_out[(size_t)(12 + 3 * (l) + (r)) * N + i]
#define WLD(l, r) (dot3(Rq[r], LOC(l, 0), LOC(l, 1), LOC(l, 2)) + bp[r])
    int flags = reset ? 0 : g_flags[i];
    const bool side = M.mode == 0 || M.mode == 3;                             // the rows of the VELOCITY / ADVANCED_TROT kernels
    if (reset) {
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float lc = LOC(l, r), wd = WLD(l, r);
                ST(SS_LOCAL + 3 * l + r) = lc;
                ST(SS_GLOBAL + 3 * l + r) = wd;
                if (M.mode == 1) ST(SS_FH + 3 * l + r) = (r == 0 && (l == 0 || l == 3)) ? (float)((double)wd - 0.05) : wd;
                else if (M.mode == 2) ST(SS_FH + 3 * l + r) = wd;
                else if (reset == 2) ST(SS_FH + 3 * l + r) = 0.f;
                ST(SS_OFF + 3 * l + r) = 0.f;                                 // qrFootholdPlanner::Reset: desiredFootholdsOffset = 0
                if (side && g_swing_in) g_swing_in[(size_t)(12 + 3 * l + r) * N + i] = wd;
                if (side && g_swing_vel_in) g_swing_vel_in[(size_t)(8 + 3 * l + r) * N + i] = lc;
            }
        if (side && g_fe_in) { g_fe_in[62 * N + i] = bp[0]; g_fe_in[63 * N + i] = bp[1]; }   // firstSwingBaseState
        ST(SS_MAP) = 0.f;                                                     // swingJointAnglesVelocities.clear()
        if (reset == 2) {                                                     // a constructed controller: no trajectory, an unplanned stepper
            ST(SS_BUILT) = 0.f; ST(SS_PFLAGS) = 0.f; ST(SS_HEAD) = 0.f; ST(SS_TAIL) = 0.f;
        }
    }
    float Rb[3][3];                                                           // stateDataFlow.baseRMat
    base_rmat(q, Rb);
    int built = (int)ST(SS_BUILT);
    for (int l = 0; l < 4; ++l) {
        const int nst = (int)g_gait_out[(size_t)(8 + l) * N + i], cur = (int)g_gait_out[(size_t)(16 + l) * N + i];
        bool lift;
        if (M.mode == 1) lift = (nst == 0 || nst == 4) && cur == 1 && !stop;
        else if (M.mode == 2) lift = (nst == 8 || nst == 4) && cur == 6 && !stop;
        else lift = nst == 0 && nst != cur;
        if (!lift) continue;
        const float lc[3] = {LOC(l, 0), LOC(l, 1), LOC(l, 2)};
        float wd[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) { ST(SS_LOCAL + 3 * l + r) = lc[r]; wd[r] = WLD(l, r); }
        if (side) {
            float g[3];                                                       // Rb * local: a rotation only (:186)
#pragma unroll
            for (int r = 0; r < 3; ++r) { g[r] = dot3(Rb[r], lc[0], lc[1], lc[2]); ST(SS_GLOBAL + 3 * l + r) = g[r]; }
            if (g_swing_in)
#pragma unroll
                for (int r = 0; r < 3; ++r) g_swing_in[(size_t)(12 + 3 * l + r) * N + i] = g[r];
            if (g_swing_vel_in)
#pragma unroll
                for (int r = 0; r < 3; ++r) g_swing_vel_in[(size_t)(8 + 3 * l + r) * N + i] = lc[r];
            if (M.mode == 3 && g_fe_in) { g_fe_in[62 * N + i] = bp[0]; g_fe_in[63 * N + i] = bp[1]; }
            continue;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) ST(SS_GLOBAL + 3 * l + r) = wd[r];
        // qrFootholdPlanner::UpdateOnce: position mode at leg 0 for all legs, walk mode for this leg
        if (M.mode == 2 || l == 0) {
            float off0[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) off0[k] = M.foothold_delta;            // nextFootholdsOffset row 0 (rows 1, 2 stay zero)
            if (M.terrain == 2) {                                             // GetFootholdsInWorldFrame, STAIRS (:181-202)
                if (M.mode == 2) ST(SS_FH + 3 * l) = ST(SS_FH + 3 * l) + 0.1f;
            } else if (M.n_gaps > 0) {                                        // GetOptimalFootholdsOffset (:483-525)
                int pf = (int)fminf(fmaxf(ST(SS_PFLAGS), 0.f), 3.f);
                // head / tail address the queue: clamped, so that a state array that never saw reset = 2 cannot index outside it
                int tail = (int)fminf(fmaxf(ST(SS_TAIL), 0.f), (float)QRGPU_SWING_MAX_PLAN);
                int head = (int)fminf(fmaxf(ST(SS_HEAD), 0.f), (float)tail);
                if (!(pf & 1)) {
                    head = 0; tail = 0;
                    float cx[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) cx[k] = ST(SS_FH + 3 * k);
                    const float lastD = M.gap_distance[M.n_gaps - 1];
                    while ((double)cx[3] < (double)lastD + (double)M.gap_width / 2.0) {
                        float des[4];
                        const int f = step_generator(M, cx, des, &pf);
                        if (f == -2) { flags |= SW_PLAN_EXIT; break; }        // exit(-1) in the reference
                        if (f == -1) {
                            if (tail > head) {
                                ST(SS_PLAN + 4 * (tail - 1)) = (float)((double)ST(SS_PLAN + 4 * (tail - 1)) + (double)M.foothold_delta / 2.0);
                                ST(SS_PLAN + 4 * (tail - 1) + 3) = (float)((double)ST(SS_PLAN + 4 * (tail - 1) + 3) + (double)M.foothold_delta / 2.0);
                            } else {
                                flags |= SW_PLAN_EMPTY;                      // steps.back() on an empty queue
                            }
                            cx[0] = (float)((double)cx[0] + (double)M.foothold_delta / 2.0);
                            cx[3] = (float)((double)cx[3] + (double)M.foothold_delta / 2.0);
                        } else {
                            if (tail >= QRGPU_SWING_MAX_PLAN) { flags |= SW_PLAN_FULL; break; }
#pragma unroll
                            for (int k = 0; k < 4; ++k) { ST(SS_PLAN + 4 * tail + k) = des[k]; cx[k] = cx[k] + des[k]; }
                            ++tail;
                        }
                    }
                    pf |= 1;
                }
                if (tail > head) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) off0[k] = ST(SS_PLAN + 4 * head + k);
                    ++head;
                }
                ST(SS_PFLAGS) = (float)pf; ST(SS_HEAD) = (float)head; ST(SS_TAIL) = (float)tail;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) { ST(SS_OFF + 3 * k) = off0[k]; ST(SS_OFF + 3 * k + 1) = 0.f; ST(SS_OFF + 3 * k + 2) = 0.f; }
        }
        if (M.mode == 1) {
#pragma unroll
            for (int r = 0; r < 3; ++r) ST(SS_FH + 3 * l + r) = ST(SS_FH + 3 * l + r) + ST(SS_OFF + 3 * l + r);
        } else {                                                              // walk: SwingFootTrajectory(BSpline, source, target, 1, 0.15)
            float src[3], tgt[3];
            if (M.is_sim) {
#pragma unroll
                for (int r = 0; r < 3; ++r) { src[r] = wd[r]; tgt[r] = ST(SS_FH + 3 * l + r); }
                tgt[2] = src[2] + ST(SS_OFF + 3 * l + 2);
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) src[r] = lc[r];
                tgt[0] = l <= 1 ? 0.30f : -0.17f;
                tgt[1] = (float)(-0.145 * ((l & 1) ? -1.0 : 1.0));
                tgt[2] = -0.32f;
            }
            const float lo = 0.15f + fabsf(tgt[2] - src[2]);                 // std::min(0.2f, std::max(0.1f, maxClearance + |dz|)) (:298)
            const float mx = (0.1f < lo) ? lo : 0.1f;
            const float hh = (mx < 0.2f) ? mx : 0.2f;
#pragma unroll
            for (int r = 0; r < 3; ++r) { ST(SS_SRC + 3 * l + r) = src[r]; ST(SS_TGT + 3 * l + r) = tgt[r]; }
            ST(SS_H + l) = hh;
            built |= 1 << l;
        }
    }
    ST(SS_BUILT) = (float)built;
    g_flags[i] = flags;
#undef ST
#undef LOC
#undef WLD
}
