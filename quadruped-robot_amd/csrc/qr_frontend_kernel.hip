// ============================================================================
// MPC front-end, one thread per (robot, horizon step): command filter, desired-pose integration,
// contact table and reference trajectory of
//   MPCStanceLegController::SetupCommand / Run / UpdateMPC
//   (quadruped/src/controllers/mpc/qr_mpc_stance_leg_controller.cpp:158-204, 207-334, 337-382)
// for n robots whose gait-generator / estimator outputs are device resident.  Pure streaming work:
// (64 + 2*8 + 16h + 19 + 1) floats per robot, SoA so every load and store is a coalesced 256 B row
// segment per wave; bound by HBM, no LDS, no cross-lane traffic.
//
// The float/double mix of each expression is the reference's (double literals promote, assignment narrows),
// and contraction is off, so results are bit-identical to the CPU restatement except where std::sin's last
// bit differs between libm and the device library.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_kernels.h"

namespace qrgpu {

#pragma clang fp contract(off)
__device__ __forceinline__ float fe_clip(float c, float lo, float hi) { return c < lo ? lo : (c > hi ? hi : c); }

// The stage kernels with memory, compiled twice: as they always were, and in their per-robot form (suffix _pr, qrgpu_set_stage_reset).
#define QR_STAGE_PR 0
#include "qr_frontend.inc.h"
#undef QR_STAGE_PR
#define QR_STAGE_PR 1
#include "qr_frontend.inc.h"
#undef QR_STAGE_PR

}  // namespace qrgpu
