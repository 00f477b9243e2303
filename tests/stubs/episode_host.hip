// The episode step (qr_episode.h) compiled for the host, driven over files, one robot after the other as qr_episode_kernel runs a lane:
//   in:  int n, n_spawn, nx, ny, n_fields, has_terrain, reset_all, sizeof(qrgpu_episode_desc); float x0, y0, cell, ground_z; qrgpu_episode_desc;
//        float height[n_fields][ny][nx]; float table[4][n_spawn];
//        per robot: int field, plant_status, tick_status, force_reset, ep_state[6]; float fb_state[37], ep_stats[9]
//   out: int [n][28]: done (reason | flags), reset (0 / 1), ep_state[6] after the call, the twenty words of blocks 0..4 at the episode index after
//        the call;  double [n][49]: fb_state[37] after the call (a spawn: unrounded), ep_stats[9] after the call (unrounded), R_zz, clearance, margin
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "qr_episode.h"
using namespace qrgpu;

struct Rec { int field, pstatus, tstatus, force, st[6]; float fb[37], stats[9]; };

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[8];
    float g[4];
    qrgpu_episode_desc D;
    bool ok = fread(hd, 4, 8, f) == 8 && fread(g, 4, 4, f) == 4 && hd[7] == (int)sizeof(D) && fread(&D, sizeof(D), 1, f) == 1;
    const int n = hd[0], n_spawn = hd[1], nx = hd[2], ny = hd[3], nf = hd[4], has = hd[5], reset_all = hd[6];
    ok = ok && n >= 1 && n <= (1 << 20) && n_spawn >= 1 && n_spawn <= 4096 && nx >= 2 && ny >= 2 && nx <= 4096 && ny <= 4096 && nf >= 1 && nf <= 64;
    if (!ok) return 2;
    std::vector<float> height((size_t)nf * ny * nx), table((size_t)4 * n_spawn);
    std::vector<Rec> rec(n);
    ok = fread(height.data(), 4, height.size(), f) == height.size() && fread(table.data(), 4, table.size(), f) == table.size() &&
         fread(rec.data(), sizeof(Rec), n, f) == (size_t)n;
    fclose(f);
    if (!ok) return 2;
    qrgpu_terrain_desc T;
    T.nx = nx; T.ny = ny; T.n_fields = nf; T.x0 = g[0]; T.y0 = g[1]; T.cell = g[2];
    const real cos_tilt = episode::cos_tilt_of(D.tilt_max);
    std::vector<int> oi((size_t)n * 28);
    std::vector<double> od((size_t)n * 49);
    for (int r = 0; r < n; ++r) {
        const Rec &q = rec[r];
        int flags = 0, fid = 0;
        if (has) { fid = q.field; if (fid < 0 || fid >= nf) { fid = 0; flags = QRGPU_EP_BAD_FIELD; } }
        const episode::Ground G = episode::ground_of(has != 0, T, height.data(), fid, g[3]);
        episode::Book b;
        memset(&b, 0, sizeof(b));
        int reason = QRGPU_EP_FORCED;
        bool finite = true;
        episode::Verdict v;
        v.reason = 0; v.rzz = v.clearance = v.margin = 0.0;
        double *d = od.data() + (size_t)r * 49;
        int *o = oi.data() + (size_t)r * 28;
        for (int k = 0; k < 37; ++k) d[k] = (double)q.fb[k];
        if (!reset_all) {
            b.ticks = q.st[0]; b.epi = q.st[1]; b.deb = q.st[2]; b.last = q.st[3]; b.n_fail = q.st[4]; b.n_time = q.st[5];
            b.sx = q.stats[0]; b.sy = q.stats[1]; b.sz = q.stats[2]; b.syaw = q.stats[3]; b.len = q.stats[4]; b.dx = q.stats[5]; b.dy = q.stats[6];
            b.last_min = q.stats[7]; b.run_min = q.stats[8];
            finite = episode::state_finite(q.fb, 1);
            v = episode::decide(D, cos_tilt, G, q.pstatus, q.tstatus, q.force, finite, q.fb[0], q.fb[1], q.fb[2], q.fb[3], q.fb[4], q.fb[5], q.fb[6], b.deb, b.ticks);
            reason = v.reason;
            episode::note_clearance(b, finite, v.clearance);
        }
        const bool reset = reason != 0;
        if (reset) {
            if (!reset_all) episode::close_episode(b, reason, finite, q.fb[4], q.fb[5]);
            const episode::Spawn s = episode::spawn(D, G, table.data(), n_spawn, (unsigned)r, (unsigned)b.epi);
            episode::open_episode(b, s, (real)D.spawn_height);
            for (int k = 0; k < 37; ++k) d[k] = 0.0;
            d[0] = s.qw; d[1] = s.qx; d[2] = s.qy; d[3] = s.qz; d[4] = s.x; d[5] = s.y; d[6] = s.z; d[10] = s.vx; d[11] = s.vy;
            for (int k = 0; k < 12; ++k) d[13 + k] = s.q[k];
        }
        d[37] = b.sx; d[38] = b.sy; d[39] = b.sz; d[40] = b.syaw; d[41] = b.len; d[42] = b.dx; d[43] = b.dy; d[44] = b.last_min; d[45] = b.run_min;
        d[46] = v.rzz; d[47] = v.clearance; d[48] = v.margin;
        o[0] = reason | flags; o[1] = reset ? 1 : 0;
        o[2] = b.ticks; o[3] = b.epi; o[4] = b.deb; o[5] = b.last; o[6] = b.n_fail; o[7] = b.n_time;
        for (int k = 0; k < 5; ++k) {
            const episode::Words w = episode::block(D.seed, (unsigned)r, (unsigned)b.epi, (unsigned)k);
            o[8 + 4 * k] = (int)w.w0; o[9 + 4 * k] = (int)w.w1; o[10 + 4 * k] = (int)w.w2; o[11 + 4 * k] = (int)w.w3;
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    ok = fwrite(oi.data(), 4, oi.size(), f) == oi.size() && fwrite(od.data(), 8, od.size(), f) == od.size();
    fclose(f);
    return ok ? 0 : 2;
}
