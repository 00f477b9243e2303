// The body plant's sub-step (qr_plant_body.h on qr_plant_math.h and qr_terrain.h) compiled for the host, with a loop over the four legs where the
// kernel has the quad, driven over files:
//   in:  int n, ntypes, nx, ny, n_fields, pad; float x0, y0, cell; float k, a, mu, v_eps, ground_z, tau_max; qrgpu_model_desc[ntypes];
//        qrgpu_plant_body_desc[ntypes]; float height[n_fields][ny][nx]; per robot: int type, field; float push[6], state[37], cmd[60]
//   out: double [n][78]: nu_dot [18]; force (world) of the sixteen points [48] -- feet 0-3, knees 4-7, corners at 8 + 2 leg + top; tau_lim [12]
//        -- of one sub-step from the state given, unrounded
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#include "qr_plant_body.h"
#include "qr_terrain.h"
#include "qr_wbc_model.h"
using namespace qrgpu;
using namespace qrgpu::plant;

struct Robot { int type, field; float push[6], state[37], cmd[60]; };

static real clip(real x, real lim) { return fmin(fmax(x, -lim), lim); }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[6];
    float g[3], p[6];
    bool ok = fread(hd, 4, 6, f) == 6 && fread(g, 4, 3, f) == 3 && fread(p, 4, 6, f) == 6;
    const int n = hd[0], ntypes = hd[1], nx = hd[2], ny = hd[3], nf = hd[4];
    ok = ok && n > 0 && n <= 4096 && ntypes > 0 && ntypes <= QRGPU_MAX_TYPES && nx >= 2 && ny >= 2 && nx <= 4096 && ny <= 4096 && nf >= 1 && nf <= 64;
    if (!ok) return 2;
    std::vector<qrgpu_model_desc> desc(ntypes);
    std::vector<qrgpu_plant_body_desc> body(ntypes);
    std::vector<float> height((size_t)nf * ny * nx);
    std::vector<Robot> robots(n);
    ok = fread(desc.data(), sizeof(qrgpu_model_desc), ntypes, f) == (size_t)ntypes && fread(body.data(), sizeof(qrgpu_plant_body_desc), ntypes, f) == (size_t)ntypes &&
         fread(height.data(), 4, height.size(), f) == height.size() && fread(robots.data(), sizeof(Robot), n, f) == (size_t)n;
    fclose(f);
    if (!ok) return 2;
    std::vector<WbcConst> types(ntypes);
    for (int t = 0; t < ntypes; ++t) build_wbc_const(desc[t], types[t]);
    const real ck = p[0], ca = p[1], mu = p[2], v_eps = p[3], ground_z = p[4], tau_max = p[5];

    std::vector<double> out((size_t)n * 78);
    for (int r = 0; r < n; ++r) {
        const Robot &rb = robots[r];
        if (rb.type < 0 || rb.type >= ntypes || rb.field < 0 || rb.field >= nf) return 2;
        const WbcConst &K = types[rb.type];
        const qrgpu_plant_body_desc &B = body[rb.type];
        const float *field = height.data() + (size_t)rb.field * ny * nx;
        double *o = out.data() + (size_t)r * 78;
        real qw = rb.state[0], qx = rb.state[1], qy = rb.state[2], qz = rb.state[3];
        const real inv = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
        qw *= inv; qx *= inv; qy *= inv; qz *= inv;
        const frame3 R = quat_to_rot(qw, qx, qy, qz);
        const v3 pos = mk(rb.state[4], rb.state[5], rb.state[6]);
        sv6 v0; v0.a = mk(rb.state[7], rb.state[8], rb.state[9]); v0.l = mk(rb.state[10], rb.state[11], rb.state[12]);
        real store[4][QR_PL_ST_SLOTS];
        abi IA; sv6 pA;
        base_start(K, v0, IA, pA);
        sv6 wrench; wrench.a = mulT(R, mk(rb.push[3], rb.push[4], rb.push[5])); wrench.l = mulT(R, mk(rb.push[0], rb.push[1], rb.push[2]));
        real qd[12];
        for (int leg = 0; leg < 4; ++leg) {
            const int j = 3 * leg;
            Stash st; st.p = store[leg]; st.stride = 1;
            real tau[3];
            for (int k = 0; k < 3; ++k) {
                const real q = rb.state[13 + j + k];
                qd[j + k] = rb.state[25 + j + k];
                const real tl = limit_torque(q, qd[j + k], B.q_lo[k], B.q_hi[k], B.limit_k, B.limit_a);
                tau[k] = clip((real)rb.cmd[12 + j + k] * ((real)rb.cmd[j + k] - q) + (real)rb.cmd[36 + j + k] * ((real)rb.cmd[24 + j + k] - qd[j + k]) + (real)rb.cmd[48 + j + k], tau_max) + tl;
                o[66 + j + k] = tl;
            }
            v3 foot, foot_vel, knee, knee_vel;
            leg_start_body(K, leg, st, rb.state[13 + j], rb.state[14 + j], rb.state[15 + j], qd[j], qd[j + 1], qd[j + 2], v0, foot, foot_vel, knee, knee_vel);
            v3 f_b = mk(0, 0, 0), fk_b = mk(0, 0, 0);
            for (int k = 0; k < QR_PB_POINTS; ++k) {
                v3 p_b, v_b;
                lane_point(B, leg, k, v0, foot, foot_vel, knee, knee_vel, p_b, v_b);
                const v3 p_w = pos + mul(R, p_b), v_w = mul(R, v_b);
                const terrain::Sample s = terrain::sample(field, nx, ny, (real)g[0], (real)g[1], (real)g[2], p_w.x, p_w.y);
                real fn;
                const v3 fw = terrain::contact_force(s.z + ground_z, terrain::normal_of(s.zx, s.zy), ck, ca, mu, v_eps, p_w, v_w, fn);
                const v3 fb = mulT(R, fw);
                const int at = k == QR_PB_FOOT ? leg : k == QR_PB_KNEE ? 4 + leg : 8 + 2 * leg + (k == QR_PB_TOP ? 1 : 0);
                o[18 + 3 * at] = fw.x; o[19 + 3 * at] = fw.y; o[20 + 3 * at] = fw.z;
                if (k == QR_PB_FOOT) f_b = fb; else if (k == QR_PB_KNEE) fk_b = fb; else wrench = wrench + corner_wrench(p_b, fb);
            }
            abi IAl; sv6 pAl;
            leg_inward_body(K, leg, st, qd[j], qd[j + 1], qd[j + 2], tau[0], tau[1], tau[2], f_b, fk_b, IAl, pAl);
            IA = IA + IAl; pA = pA + pAl;
        }
        pA = pA + (-1.0) * wrench;
        sv6 afb, a0;
        base_solve(IA, pA, R, afb, a0);
        o[0] = afb.a.x; o[1] = afb.a.y; o[2] = afb.a.z; o[3] = afb.l.x; o[4] = afb.l.y; o[5] = afb.l.z;
        for (int leg = 0; leg < 4; ++leg) {
            Stash st; st.p = store[leg]; st.stride = 1;
            real qdd0, qdd1, qdd2;
            leg_outward(K, leg, st, a0, qdd0, qdd1, qdd2);
            o[6 + 3 * leg] = qdd0; o[7 + 3 * leg] = qdd1; o[8 + 3 * leg] = qdd2;
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    ok = fwrite(out.data(), 8, out.size(), f) == out.size();
    fclose(f);
    return ok ? 0 : 2;
}
