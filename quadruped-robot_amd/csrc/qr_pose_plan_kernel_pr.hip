// The walk pose planner once more in its per-robot form, qr_pose_plan_kernel_pr (qrgpu_set_stage_reset): see QR_STAGE_PR in qr_pose_plan_kernel.hip
// and qr_pose_plan_entry.inc.h.  Launched only while a binding is set.
#define QR_STAGE_PR 1
#include "qr_pose_plan_kernel.hip"
