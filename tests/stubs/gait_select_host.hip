// The gait generator and the stage clock (qr_gait.h) compiled for the host, driven over files, the robots one after the other as the kernels of
// qr_gait_kernel.hip run their lanes: arrays [row][n], a robot's column at stride n.  The header's n_gaits word picks the kernel.
// n_gaits >= 1, qr_gait_select_kernel and qr_stage_clock_kernel.  Per tick: the clock from the tick's mask and the robots' tick counts, then the gait
// on that clock (one float32 product, as the binding's) with the reset level the tick's level word names.
//   in:  int n, T, n_gaits, sizeof(qrgpu_gait_desc); float tick_dt; the table [n_gaits]; float sel[T][n]; int level[T][n]; int ticks[T][n]; int stop[T];
//        float contact[T][4][n]
// n_gaits = 0, qr_gait_kernel: no table but one gait, every robot at the tick's level and time; n_gaits = -1 the same with gait_out and fe_in null.
//   in:  the header; the desc; int level[T]; float time[T]; int stop[T]; float contact[T][4][n]
// Both write the same record; what a kernel does not write keeps its start value.
//   out: per tick: float state[52][n], out[24][n], fe_in[64][n], swing_in[24][n]; int flags[n], origin[n], local[n].  The mask word of a robot with a
//        level is 0x40 (under bits 0xff), every other robot carries a word outside the bits.  The outputs start every tick at the poison value; the state
//        and the clock's origin are carried and start at poison.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "qr_gait.h"
using namespace qrgpu;

template <typename T> static bool rd(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static float clock_time(int ticks, float dt)
{
#pragma clang fp contract(off)
    return (float)ticks * dt;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[4];
    float dt;
    bool ok = fread(hd, 4, 4, f) == 4 && hd[3] == (int)sizeof(qrgpu_gait_desc) && fread(&dt, 4, 1, f) == 1;
    const int n = hd[0], T = hd[1], ng = hd[2];
    const bool fixed = ng <= 0;
    ok = ok && n >= 1 && n <= 4096 && T >= 1 && T <= 8192 && ng >= -1 && ng <= QRGPU_MAX_GAITS;
    if (!ok) return 2;
    const size_t N = (size_t)n, TN = (size_t)T * N;
    std::vector<qrgpu_gait_desc> table(fixed ? 1 : ng);
    std::vector<float> sel(fixed ? 0 : TN), time(fixed ? T : 0), contact(4 * TN);
    std::vector<int> level(fixed ? T : TN), ticks(fixed ? 0 : TN), stop(T);
    ok = rd(f, table) && rd(f, sel) && rd(f, level) && rd(f, ticks) && rd(f, time) && rd(f, stop) && rd(f, contact);
    fclose(f);
    if (!ok) return 2;
    const float poison = -12345.5f;
    std::vector<float> st(QRGPU_GAIT_STATE_FLOATS * N, poison), out(24 * N), fe(64 * N), sw(24 * N);
    std::vector<int> flags(N), origin(N, 0x7fffffff), local(N), mask(N);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    for (int t = 0; t < T && ok; ++t) {
        for (auto *a : {&out, &fe, &sw}) std::fill(a->begin(), a->end(), poison);
        std::fill(flags.begin(), flags.end(), 0x7fffffff);
        std::fill(local.begin(), local.end(), 0x7fffffff);
        if (fixed) {
            for (int r = 0; r < n; ++r)
                gait::fixed_update(table[0], level[t], time[t], stop[t], N, contact.data() + (size_t)t * 4 * N + r, st.data() + r,
                                   ng == 0 ? out.data() + r : nullptr, ng == 0 ? fe.data() + r : nullptr);
        } else {
            for (int r = 0; r < n; ++r) mask[r] = level[(size_t)t * N + r] ? 0x40 : 0x01000000;
            for (int r = 0; r < n; ++r) {
                gait::stage_clock(mask[r], 0xffu, ticks[(size_t)t * N + r], origin.data() + r, local.data() + r);
                gait::select_update(table.data(), ng, sel[(size_t)t * N + r], level[(size_t)t * N + r], clock_time(local[r], dt), stop[t], N,
                                    contact.data() + (size_t)t * 4 * N + r, st.data() + r, out.data() + r, fe.data() + r, sw.data() + r, flags.data() + r);
            }
        }
        ok = ok && wr(f, st) && wr(f, out) && wr(f, fe) && wr(f, sw) && wr(f, flags) && wr(f, origin) && wr(f, local);
    }
    fclose(f);
    return ok ? 0 : 2;
}
