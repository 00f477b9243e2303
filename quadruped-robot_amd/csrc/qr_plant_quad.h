// What the plant kernels (qr_plant_kernel.hip, qr_plant_body_kernel.hip) share on the device: the quad of four lanes that is one robot -- who it is,
// sums and flags across it, the forward dynamics across it -- and the lane's column of LDS.  Device only: the algebra that also runs on a CPU is
// qr_plant_math.h's.
#pragma once
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_wave_helpers.h"
#include "qr_plant_math.h"

namespace qrgpu {

using namespace plant;

#define QR_PL_QUADS 16     // robots per wavefront

__device__ __forceinline__ real quad_sum(real v)
{
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v;
}
__device__ __forceinline__ v3 quad_sum(v3 v) { return mk(quad_sum(v.x), quad_sum(v.y), quad_sum(v.z)); }
__device__ __forceinline__ int quad_or(int v)
{
    v |= __shfl_xor(v, 1);
    v |= __shfl_xor(v, 2);
    return v;
}
__device__ __forceinline__ bool finite3(v3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// Which robot, which constants: the WBC kernel's rule for a type that was never set up (computed with the first valid type, flagged).
struct Who { int robot, leg, flags; bool live; const WbcConst *K; };
__device__ __forceinline__ Who who_am_i(int n, const WbcConst *types, const int *type_id, int type_ready)
{
    Who w;
    const int robot = blockIdx.x * QR_PL_QUADS + (threadIdx.x >> 2);
    w.live = robot < n;
    w.robot = w.live ? robot : n - 1;
    w.leg = threadIdx.x & 3;
    int tyid = type_id ? type_id[w.robot] : 0;
    const bool bad_type = resolve_type(tyid, type_ready);
    w.flags = bad_type ? QRGPU_PL_BAD_TYPE : 0;
    w.K = types + (tyid & (QRGPU_MAX_TYPES - 1));
    return w;
}

// The quaternion normalised in fp64; a zero or non-finite one is flagged and replaced by the identity.
__device__ __forceinline__ void unit_quat(real &w, real &x, real &y, real &z, int &flags)
{
    const real nn = w * w + x * x + y * y + z * z;
    if (!(nn > 0.0) || !isfinite(nn)) { flags |= QRGPU_PL_QUAT_ZERO; w = 1.0; x = y = z = 0.0; return; }
    const real inv = 1.0 / sqrt(nn);
    w *= inv; x *= inv; y *= inv; z *= inv;
}

// Forward dynamics of one robot across its quad, after leg_start: this lane's leg in, the base's and this leg's accelerations out.
// WRENCH: an external wrench on the base (moment about its origin; force), base frame, enters the base's bias force.
template <bool WRENCH = false>
__device__ __forceinline__ void forward_dynamics(const WbcConst &K, int leg, const Stash &st, const frame3 &R, sv6 v0, real qd0, real qd1, real qd2, real tau0,
                                                 real tau1, real tau2, v3 f_b, sv6 &afb, real &qdd0, real &qdd1, real &qdd2, sv6 wrench_b = sv6())
{
    abi IA;
    sv6 pA;
    leg_inward(K, leg, st, qd0, qd1, qd2, tau0, tau1, tau2, f_b, IA, pA);
#pragma unroll
    for (int i = 0; i < 6; ++i) { IA.I[i] = quad_sum(IA.I[i]); IA.M[i] = quad_sum(IA.M[i]); }
    IA.h0 = quad_sum(IA.h0); IA.h1 = quad_sum(IA.h1); IA.h2 = quad_sum(IA.h2);
    pA.a = quad_sum(pA.a); pA.l = quad_sum(pA.l);
    abi IA0; sv6 pA0;
    base_start(K, v0, IA0, pA0);
    if (WRENCH) pA0 = pA0 + (-1.0) * wrench_b;
    sv6 a0;
    base_solve(IA0 + IA, pA0 + pA, R, afb, a0);
    leg_outward(K, leg, st, a0, qdd0, qdd1, qdd2);
}

// A lane's column of the workgroup's LDS: what a leg keeps between its joints (qr_plant_math.h).  Lane-private: no barrier stands anywhere.
#define QR_PL_STASH() __shared__ real stash_lds[QR_PL_ST_SLOTS * 64]; Stash st; st.p = stash_lds + threadIdx.x; st.stride = 64

#define ROW(p, f) (p)[(size_t)(f) * N + i]

__device__ __forceinline__ real clip(real x, real lim) { return fmin(fmax(x, -lim), lim); }

}  // namespace qrgpu
