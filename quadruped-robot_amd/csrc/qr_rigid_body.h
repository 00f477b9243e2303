// 3-vector, spatial-vector and rigid-body-inertia algebra shared by the WBC kernel's rigid-body chains (qr_wbc_rigid_body.h) and the plant
// (qr_plant_math.h).  fp64 throughout.  Every function is __host__ __device__: the same text runs in the kernels and in the CPU checks
// (tests/stubs/wbc_rigid_body_host.hip).
//   motion vector (a; l): angular velocity; velocity of the body-fixed point that passes the frame's origin
//   force vector  (a; l): moment about the frame's origin; force
// The two users keep a 3 x 3 type each (xform3 in qr_wbc_rigid_body.h, frame3 in qr_plant_math.h): they store and sum differently.
#pragma once
#include <hip/hip_runtime.h>

#define QR_HD __host__ __device__ __forceinline__

namespace qrgpu {

typedef double real;

struct v3 { real x, y, z; };
QR_HD v3 mk(real x, real y, real z) { v3 r = {x, y, z}; return r; }
QR_HD v3 operator+(v3 a, v3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
QR_HD v3 operator-(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
QR_HD v3 operator*(real s, v3 a) { return mk(s * a.x, s * a.y, s * a.z); }
QR_HD v3 cross(v3 a, v3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
QR_HD real dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// Spatial vector (angular; linear) and the two cross products.
struct sv6 { v3 a, l; };
QR_HD sv6 operator+(sv6 u, sv6 v) { sv6 o; o.a = u.a + v.a; o.l = u.l + v.l; return o; }
QR_HD sv6 operator*(real s, sv6 v) { sv6 o; o.a = s * v.a; o.l = s * v.l; return o; }
QR_HD real dot(sv6 u, sv6 v) { return dot(u.a, v.a) + dot(u.l, v.l); }
QR_HD sv6 crm(sv6 v, sv6 u) { sv6 o; o.a = cross(v.a, u.a); o.l = cross(v.a, u.l) + cross(v.l, u.a); return o; }   // v x u   (motion)
QR_HD sv6 crf(sv6 v, sv6 f) { sv6 o; o.a = cross(v.a, f.a) + cross(v.l, f.l); o.l = cross(v.a, f.l); return o; }   // v x* f  (force)

// Rigid-body spatial inertia [[Ibar, [h]x], [[h]x^T, m 1]] as (m, h = m c, Ibar about the origin, symmetric: xx yy zz xy xz yz).
struct rbi { real m; v3 h; real I[6]; };
QR_HD v3 sym_mul(const real I[6], v3 w)
{
    return mk(I[0] * w.x + I[3] * w.y + I[4] * w.z, I[3] * w.x + I[1] * w.y + I[5] * w.z, I[4] * w.x + I[5] * w.y + I[2] * w.z);
}
QR_HD rbi rbi_load(const real *p)
{
    rbi r; r.m = p[0]; r.h = mk(p[1], p[2], p[3]);
#pragma unroll
    for (int i = 0; i < 6; ++i) r.I[i] = p[4 + i];
    return r;
}
QR_HD rbi rbi_add(const rbi &a, const rbi &b)
{
    rbi r; r.m = a.m + b.m; r.h = a.h + b.h;
#pragma unroll
    for (int i = 0; i < 6; ++i) r.I[i] = a.I[i] + b.I[i];
    return r;
}
QR_HD sv6 rbi_mul(const rbi &I, sv6 v) { sv6 o; o.a = sym_mul(I.I, v.a) + cross(I.h, v.l); o.l = I.m * v.l - cross(I.h, v.a); return o; }

}  // namespace qrgpu
