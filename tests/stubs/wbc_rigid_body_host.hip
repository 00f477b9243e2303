// The WBC kernel's rigid-body chains (qr_wbc_rigid_body.h) and the library's model constants (qr_wbc_model.h) compiled for the host, with
// plain loops where the kernel has lanes, driven over files:
//   in:  int n, ntypes; qrgpu_model_desc[ntypes]; int type_id[n]; float fb_state[n][37]
//   out: double [n][612] in qrgpu_fb_debug_batch's layout: H 324, G 18, C 18, Jc 4 x 3 x 18, Jcdqd 12, pGC 12, vGC 12 -- unrounded
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#include "qr_wbc_rigid_body.h"
#include "qr_wbc_model.h"
using namespace qrgpu;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n = 0, ntypes = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && fread(&ntypes, 4, 1, f) == 1 && n > 0 && n <= 4096 && ntypes > 0 && ntypes <= QRGPU_MAX_TYPES;
    if (!ok) return 2;
    std::vector<qrgpu_model_desc> desc(ntypes);
    std::vector<int> tid(n);
    std::vector<float> state((size_t)n * 37);
    ok = fread(desc.data(), sizeof(qrgpu_model_desc), ntypes, f) == (size_t)ntypes && fread(tid.data(), 4, n, f) == (size_t)n &&
         fread(state.data(), 4, state.size(), f) == state.size();
    fclose(f);
    if (!ok) return 2;
    std::vector<WbcConst> types(ntypes);
    for (int t = 0; t < ntypes; ++t) build_wbc_const(desc[t], types[t]);

    std::vector<double> out((size_t)n * 612);
    for (int r = 0; r < n; ++r) {
        if (tid[r] < 0 || tid[r] >= ntypes) return 2;
        const WbcConst &K = types[tid[r]];
        // the kernel's load: the state widened, A and the foot Jacobians zeroed
        real st[37], A[324] = {0}, JcA[216] = {0}, Gv[18], Cv[18], Jcd[12], pGC[12], vGC[12], legB[64], sS[12], sC[12];
        for (int i = 0; i < 37; ++i) st[i] = (real)state[(size_t)r * 37 + i];
        const real *quat = st, *pos = st + 4, *bv = st + 7, *qj = st + 13, *qdj = st + 25;
        const xform3 Rwb = quat_to_rot_wb(quat);
        for (int i = 0; i < 12; ++i) { sS[i] = std::sin(qj[i]); sC[i] = std::cos(qj[i]); }
        // wave 0
        for (int leg = 0; leg < 4; ++leg) wbc_leg_inertia_chain(K, Rwb, sS, sC, leg, A, JcA, Gv, legB);
        wbc_base_block(K, Rwb, legB, A, Gv);
        // wave 1
        for (int leg = 0; leg < 4; ++leg) wbc_leg_velocity_chain(K, Rwb, pos, bv, qdj, sS, sC, leg, pGC, vGC, Jcd, Cv, legB);
        wbc_base_coriolis(K, bv, legB, Cv);
        double *o = out.data() + (size_t)r * 612;
        for (int e = 0; e < 324; ++e) o[e] = A[e];
        for (int e = 0; e < 18; ++e) { o[324 + e] = Gv[e]; o[342 + e] = Cv[e]; }
        for (int e = 0; e < 216; ++e) o[360 + e] = JcA[e];
        for (int e = 0; e < 12; ++e) { o[576 + e] = Jcd[e]; o[588 + e] = pGC[e]; o[600 + e] = vGC[e]; }
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    ok = fwrite(out.data(), 8, out.size(), f) == out.size();
    fclose(f);
    return ok ? 0 : 2;
}
