// The data-flow stage of the force-balance trot (qr_velocity_flow.h) compiled for the host, driven over files, the robots one after the other as the
// kernel of qr_velocity_flow_kernel.hip runs its lanes: arrays [row][n], a robot's column at stride n, est_in written in place.
//   in:  int n, T, terrain; int reset[T][n]; float est_in[T][54][n], est_out[T][42][n], ground_out[T][32][n], gait_out[T][24][n], gait_state[T][52][n],
//        state_des[T][12][n]
//   out: per tick: float swing_vel_in[53][n], est_in[54][n]; int mem[n]; float swing_flag[4][n].  swing_vel_in and swing_flag start every tick at the
//        poison value; mem is carried from tick to tick and starts at 0x7fffffff.  On terrain < 2 the stage gets no ground_out at all.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "qr_velocity_flow.h"
using namespace qrgpu;

template <typename T> static bool rd(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[3];
    bool ok = fread(hd, 4, 3, f) == 3;
    const int n = hd[0], T = hd[1], terrain = hd[2];
    ok = ok && n >= 1 && n <= 4096 && T >= 1 && T <= 4096 && terrain >= 0 && terrain <= 4;
    if (!ok) { fclose(f); return 2; }
    const size_t N = (size_t)n, TN = (size_t)T * N;
    std::vector<int> reset(TN);
    std::vector<float> est_in(54 * TN), est_out(42 * TN), ground(32 * TN), gait_out(24 * TN), gait_state(52 * TN), des(12 * TN);
    ok = rd(f, reset) && rd(f, est_in) && rd(f, est_out) && rd(f, ground) && rd(f, gait_out) && rd(f, gait_state) && rd(f, des);
    fclose(f);
    if (!ok) return 2;
    const float poison = -12345.5f;
    std::vector<float> sv(53 * N), ei(54 * N), flag(4 * N);
    std::vector<int> mem(N, 0x7fffffff);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    for (int t = 0; t < T && ok; ++t) {
        std::fill(sv.begin(), sv.end(), poison);
        std::fill(flag.begin(), flag.end(), poison);
        memcpy(ei.data(), est_in.data() + (size_t)t * 54 * N, 54 * N * sizeof(float));
        for (int r = 0; r < n; ++r)
            velocity_flow::velocity_inputs(terrain, reset[(size_t)t * N + r] != 0, N, ei.data() + r, est_out.data() + (size_t)t * 42 * N + r,
                                           terrain < 2 ? nullptr : ground.data() + (size_t)t * 32 * N + r, gait_out.data() + (size_t)t * 24 * N + r,
                                           gait_state.data() + (size_t)t * 52 * N + r, des.data() + (size_t)t * 12 * N + r, sv.data() + r, ei.data() + r,
                                           mem.data() + r, flag.data() + r);
        ok = wr(f, sv) && wr(f, ei) && wr(f, mem) && wr(f, flag);
    }
    fclose(f);
    return ok ? 0 : 2;
}
