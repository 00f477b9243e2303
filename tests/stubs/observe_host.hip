// The sensor stage's per-robot step (qr_observe.h) compiled for the host, driven over files, the robots one after the other as qr_observe_kernel runs
// its lanes: arrays [row][n], a robot's column at stride n, est_in aliasing the raw rows.
//   in:  int n, T, has_prev, sizeof(qrgpu_observe_desc); qrgpu_observe_desc; unsigned steps[T]; int resets[T][n]; float raw[T][41][n];
//        float prev[T][3][n] (rows 36-38 of the previous est_out; has_prev only)
//   out: per tick: float est_in[54][n] (rows 41-53 hold the poison they were given), rpy[3][n], ground_in[23][n]; unsigned tick[n];
//        float state[rows][n]; unsigned words[n][8][4] (the noise blocks of that tick's step)
#include <hip/hip_runtime.h>
// the rotation helpers of qr_wave_helpers.h are __device__ functions: on the host build they are host functions too
#define __device__ __attribute__((host)) __attribute__((device))
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "qr_observe.h"
using namespace qrgpu;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[4];
    qrgpu_observe_desc D;
    bool ok = fread(hd, 4, 4, f) == 4 && hd[3] == (int)sizeof(D) && fread(&D, sizeof(D), 1, f) == 1;
    const int n = hd[0], T = hd[1], has_prev = hd[2];
    ok = ok && n >= 1 && n <= 4096 && T >= 1 && T <= 4096;
    if (!ok) return 2;
    const size_t N = (size_t)n;
    std::vector<unsigned> steps(T);
    std::vector<int> resets((size_t)T * N);
    std::vector<float> raw((size_t)T * 41 * N), prev3(has_prev ? (size_t)T * 3 * N : 0);
    ok = fread(steps.data(), 4, steps.size(), f) == steps.size() && fread(resets.data(), 4, resets.size(), f) == resets.size() &&
         fread(raw.data(), 4, raw.size(), f) == raw.size() && (!has_prev || fread(prev3.data(), 4, prev3.size(), f) == prev3.size());
    fclose(f);
    if (!ok) return 2;
    const int rows = D.filter_motor_velocity ? observe::ROWS_MV : observe::ROWS;
    std::vector<float> est(54 * N, -12345.5f), rpy(3 * N), gin(23 * N), st((size_t)rows * N, -12345.5f), prev(42 * N, 0.f);
    std::vector<unsigned> tick(N), words(N * 32);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    for (int t = 0; t < T && ok; ++t) {
        memcpy(est.data(), raw.data() + (size_t)t * 41 * N, 41 * N * sizeof(float));
        if (has_prev) memcpy(prev.data() + 36 * N, prev3.data() + (size_t)t * 3 * N, 3 * N * sizeof(float));
        for (int r = 0; r < n; ++r) {
            observe::step(D, resets[(size_t)t * N + r] != 0, (unsigned)r, steps[t], N, est.data() + r, has_prev ? prev.data() + r : nullptr, st.data() + r,
                          est.data() + r, rpy.data() + r, gin.data() + r, tick.data() + r);
            for (unsigned k = 0; k < 8; ++k) {
                const episode::Words w = observe::noise_block(D.seed, (unsigned)r, steps[t], k);
                unsigned *o = words.data() + (size_t)r * 32 + 4 * k;
                o[0] = w.w0; o[1] = w.w1; o[2] = w.w2; o[3] = w.w3;
            }
        }
        ok = fwrite(est.data(), 4, est.size(), f) == est.size() && fwrite(rpy.data(), 4, rpy.size(), f) == rpy.size() &&
             fwrite(gin.data(), 4, gin.size(), f) == gin.size() && fwrite(tick.data(), 4, tick.size(), f) == tick.size() &&
             fwrite(st.data(), 4, st.size(), f) == st.size() && fwrite(words.data(), 4, words.size(), f) == words.size();
    }
    fclose(f);
    return ok ? 0 : 2;
}
