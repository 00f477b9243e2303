// The terrain plant's sampler and contact law (qr_terrain.h) compiled for the host, driven over files:
//   in:  int nx, ny, n_fields, npts; float x0, y0, cell; float k, a, mu, v_eps, ground_z; float height[n_fields][ny][nx];
//        per point: int field; double x, y, pz, vx, vy, vz; double z_g, zx, zy (a surface given to the law on its own)
//   out: double [npts][18]: z (sampled), dz/dx, dz/dy, outside (0 / 1); the law on the surface sampled: normal [3], force [3], f_n; the law on
//        the surface given: normal [3], force [3], f_n -- unrounded
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#include "qr_terrain.h"
using namespace qrgpu;

struct Pt { int field; int pad; double x, y, pz, vx, vy, vz, zg, zx, zy; };

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[4];
    float g[3], p[5];
    bool ok = fread(hd, 4, 4, f) == 4 && fread(g, 4, 3, f) == 3 && fread(p, 4, 5, f) == 5;
    const int nx = hd[0], ny = hd[1], nf = hd[2], npts = hd[3];
    ok = ok && nx >= 2 && ny >= 2 && nx <= 4096 && ny <= 4096 && nf >= 1 && nf <= 64 && npts >= 1 && npts <= (1 << 20);
    if (!ok) return 2;
    std::vector<float> height((size_t)nf * ny * nx);
    std::vector<Pt> pts(npts);
    ok = fread(height.data(), 4, height.size(), f) == height.size() && fread(pts.data(), sizeof(Pt), npts, f) == (size_t)npts;
    fclose(f);
    if (!ok) return 2;
    std::vector<double> out((size_t)npts * 18);
    for (int i = 0; i < npts; ++i) {
        const Pt &q = pts[i];
        if (q.field < 0 || q.field >= nf) return 2;
        const terrain::Sample s = terrain::sample(height.data() + (size_t)q.field * ny * nx, nx, ny, (real)g[0], (real)g[1], (real)g[2], q.x, q.y);
        const v3 n = terrain::normal_of(s.zx, s.zy);
        real fn;
        const v3 fc = terrain::contact_force(s.z + (real)p[4], n, (real)p[0], (real)p[1], (real)p[2], (real)p[3], mk(q.x, q.y, q.pz), mk(q.vx, q.vy, q.vz), fn);
        double *o = out.data() + (size_t)i * 18;
        o[0] = s.z; o[1] = s.zx; o[2] = s.zy; o[3] = s.off ? 1.0 : 0.0;
        o[4] = n.x; o[5] = n.y; o[6] = n.z; o[7] = fc.x; o[8] = fc.y; o[9] = fc.z; o[10] = fn;
        const v3 n2 = terrain::normal_of(q.zx, q.zy);
        real fn2;
        const v3 f2 = terrain::contact_force(q.zg, n2, (real)p[0], (real)p[1], (real)p[2], (real)p[3], mk(q.x, q.y, q.pz), mk(q.vx, q.vy, q.vz), fn2);
        o[11] = n2.x; o[12] = n2.y; o[13] = n2.z; o[14] = f2.x; o[15] = f2.y; o[16] = f2.z; o[17] = fn2;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    ok = fwrite(out.data(), 8, out.size(), f) == out.size();
    fclose(f);
    return ok ? 0 : 2;
}
