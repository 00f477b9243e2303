// The ground as a height field, and the contact law on it: what qr_plant_step_terrain_kernel (qr_plant_kernel.hip) has beyond the flat plant.
// fp64 on the fp32 heights.  Every function is __host__ __device__: the same text compiles for a CPU check against tests/terrain_ref.py
// (tests/stubs/terrain_host.hip).  include/qrgpu.h states the sampler and the law (qrgpu_plant_step_terrain_batch).
//
// A field is ny x nx heights, x fastest; node (i, j) lies at (x0 + i cell, y0 + j cell).  The surface is the separable Catmull-Rom (cubic
// convolution, a = -1/2) interpolant of the nodes, evaluated at the query point clipped to the grid, with node indices clamped to the grid: it is
// C1 everywhere, so choosing the cell on either side of a grid line gives the same height and normal to rounding, and outside the grid it is the
// height and normal of the nearest border point.
#pragma once
#include "qr_device_types.h"
#include "qr_rigid_body.h"

namespace qrgpu {
namespace terrain {

// One axis of the sampler: the cell, the four clamped node indices and the weights of the value and of the derivative (per unit of u).
struct Axis { int i0, i1, i2, i3; real w0, w1, w2, w3, d0, d1, d2, d3; bool off; };
QR_HD Axis axis_of(real x, real x0, real cell, int nx)
{
    Axis a;
    const real top = (real)(nx - 1);
    const real ur = (x - x0) / cell;
    a.off = !(ur >= 0.0 && ur <= top);
    const real u = fmin(fmax(ur, 0.0), top);          // a NaN becomes 0: the indices below never leave the grid
    int i = (int)floor(u);
    i = i > nx - 2 ? nx - 2 : i;
    const real t = u - (real)i, t2 = t * t, t3 = t2 * t;
    a.w0 = 0.5 * (-t3 + 2.0 * t2 - t); a.w1 = 0.5 * (3.0 * t3 - 5.0 * t2 + 2.0); a.w2 = 0.5 * (-3.0 * t3 + 4.0 * t2 + t); a.w3 = 0.5 * (t3 - t2);
    a.d0 = 0.5 * (-3.0 * t2 + 4.0 * t - 1.0); a.d1 = 0.5 * (9.0 * t2 - 10.0 * t); a.d2 = 0.5 * (-9.0 * t2 + 8.0 * t + 1.0); a.d3 = 0.5 * (3.0 * t2 - 2.0 * t);
    a.i0 = i > 0 ? i - 1 : 0; a.i1 = i; a.i2 = i + 1; a.i3 = i + 2 < nx ? i + 2 : nx - 1;
    return a;
}

// Height, slopes dz/dx and dz/dy of one field at (x, y); off = the point lies outside the grid (the border was extended).
struct Sample { real z, zx, zy; bool off; };
QR_HD Sample sample(const float *h, int nx, int ny, real x0, real y0, real cell, real x, real y)
{
    const Axis ax = axis_of(x, x0, cell, nx), ay = axis_of(y, y0, cell, ny);
    const int jj[4] = {ay.i0, ay.i1, ay.i2, ay.i3};
    const real wy[4] = {ay.w0, ay.w1, ay.w2, ay.w3}, dy[4] = {ay.d0, ay.d1, ay.d2, ay.d3};
    real z = 0, zx = 0, zy = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float *row = h + (size_t)jj[k] * (size_t)nx;
        const real h0 = (real)row[ax.i0], h1 = (real)row[ax.i1], h2 = (real)row[ax.i2], h3 = (real)row[ax.i3];
        const real r = (ax.w0 * h0 + ax.w1 * h1) + (ax.w2 * h2 + ax.w3 * h3);
        const real rx = (ax.d0 * h0 + ax.d1 * h1) + (ax.d2 * h2 + ax.d3 * h3);
        z += wy[k] * r; zx += wy[k] * rx; zy += dy[k] * r;
    }
    Sample s;
    s.z = z; s.zx = zx / cell; s.zy = zy / cell; s.off = ax.off || ay.off;
    return s;
}

// unit normal of the surface with slopes zx, zy
QR_HD v3 normal_of(real zx, real zy)
{
    const real inv = 1.0 / sqrt((zx * zx + zy * zy) + 1.0);
    return mk(-zx * inv, -zy * inv, inv);
}

// The contact law on a surface of height z_g and unit normal n under the foot: depth along the normal, a spring-damper normal force that never
// pulls, friction in the tangent plane regularised at v_eps.  On a level surface it is the flat plant's law.  p, v: the foot point's world
// position and velocity.
QR_HD v3 contact_force(real z_g, v3 n, real k, real a, real mu, real v_eps, v3 p, v3 v, real &fn)
{
    const real depth = (z_g - p.z) * n.z;
    const real vn = dot(v, n);
    const v3 vt = v - vn * n;
    fn = 0.0;
    if (depth > 0.0) fn = fmax(0.0, k * depth * (1.0 - a * vn));
    const real s = -mu * fn / sqrt(dot(vt, vt) + v_eps * v_eps);
    return fn * n + s * vt;
}

}  // namespace terrain
}  // namespace qrgpu
