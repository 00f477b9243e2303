// The planner's __global__ entry, compiled by qr_pose_plan_kernel.hip with QR_STAGE_PR 0 -- the kernel text as it always was -- and once more by
// qr_pose_plan_kernel_pr.hip with QR_STAGE_PR 1, which names it qr_pose_plan_kernel_pr and gives it the binding of qrgpu_set_stage_reset as one more
// argument, SR.  Only the lines between #if QR_STAGE_PR and #endif differ.  No include guard.

// event: 0 none, 1 Update, 2 ResetBasePose, 3 Update where a leg has legState SWING and curLegState STANCE (qr_locomotion_controller.cpp:81-89);
// g_event (may be null) overrides it per robot with 0 / 1 / 2.  reset: every robot's state is first put into the constructed state (:31-69).
__global__ void __launch_bounds__(64) QR_STAGE_K(qr_pose_plan_kernel)(int n, qrgpu_pose_plan_desc D, int event, const int *__restrict__ g_event, int reset,
                                                          const float *__restrict__ g_est_in, const float *__restrict__ g_est_out,
                                                          const float *__restrict__ g_ground, const float *__restrict__ g_rpy,
                                                          const float *__restrict__ g_walk, float *__restrict__ g_state, float *__restrict__ g_cmd,
                                                          float *__restrict__ g_out, int *__restrict__ g_flags QR_STAGE_PARAM)
{
    const int lane = threadIdx.x;
    const int rid = xcd_robot_index(blockIdx.x, n);
    if (rid < 0) return;
    const size_t Ns = (size_t)n;
#if QR_STAGE_PR          // the robot's own reset, uniform over its wavefront
    if (!reset && stage_masked(SR, rid)) reset = 1;
#endif
    int ev = g_event ? g_event[rid] : event;
    if (!g_event && event == 3) {
        ev = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if ((int)g_walk[(size_t)(12 + l) * Ns + rid] == 0 && (int)g_walk[(size_t)(16 + l) * Ns + rid] == 1) ev = 1;
    }
    if (ev != 1 && ev != 2) ev = 0;
    if (reset && lane < QRGPU_POSE_STATE_ROWS) {                                 // the constructor (:31-69)
        float v = 0.f;
        if (lane < 12) v = 0.1f;
        else if (lane == 12) v = 12.f;
        else if (lane < 16) v = g_est_out[(size_t)(36 + lane - 13) * Ns + rid];
        else if (lane == 16) v = 1.f;
        else if (lane >= 20 && lane < 23) v = g_est_out[(size_t)(36 + lane - 20) * Ns + rid];
        g_state[(size_t)lane * Ns + rid] = v;
    }
    if (reset) {                                                              // those stores land before lane 0's stores to the same rows at the end
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (ev == 0) return;
    __shared__ PoseWork W;
    pose_plan_robot(W, lane, rid, n, D, ev, reset, g_est_in, g_est_out, g_ground, g_rpy, g_walk, g_state, g_cmd, g_out, g_flags);
}
