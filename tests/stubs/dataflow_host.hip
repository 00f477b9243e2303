// The trot's command, data-flow and motor-command stages (qr_dataflow.h) compiled for the host, driven over files, the robots one after the other as
// the kernels of qr_dataflow_kernel.hip run their lanes: arrays [row][n], a robot's column at stride n, est_in written in place.
//   in:  int n, T, sizeof(qrgpu_command_desc), sizeof(qrgpu_mpc_command_desc); the two descs; int cmd_reset[T][n], mem_reset[T][n];
//        float joy[T][8][n], est_in[T][54][n], est_out[T][42][n], rpy[T][3][n], gait_out[T][24][n], gait_state[T][52][n], tau[T][12][n], qdes[T][24][n],
//        swing_flag[T][4][n]
//   out: per tick: float cmd_state[6][n], state_des[12][n], fe_in[64][n], fh_in[46][n], swing_vel_in[53][n], stance_cmd[28][n], swing_in[58][n],
//        est_in[54][n]; int mem[n]; float motor_cmd[60][n].  The five arrays the stages scatter into start every tick at the poison value
//        (swing_in rows 0-3: the tick's flags); cmd_state and mem are carried from tick to tick and start at poison.
#include <hip/hip_runtime.h>
// the rotation helpers of qr_wave_helpers.h are __device__ functions: on the host build they are host functions too
#define __device__ __attribute__((host)) __attribute__((device))
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "qr_dataflow.h"
using namespace qrgpu;

template <typename T> static bool rd(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[4];
    qrgpu_command_desc C;
    qrgpu_mpc_command_desc M;
    bool ok = fread(hd, 4, 4, f) == 4 && hd[2] == (int)sizeof(C) && hd[3] == (int)sizeof(M) && fread(&C, sizeof(C), 1, f) == 1 && fread(&M, sizeof(M), 1, f) == 1;
    const int n = hd[0], T = hd[1];
    ok = ok && n >= 1 && n <= 4096 && T >= 1 && T <= 4096;
    if (!ok) return 2;
    const size_t N = (size_t)n, TN = (size_t)T * N;
    std::vector<int> cmd_reset(TN), mem_reset(TN);
    std::vector<float> joy(8 * TN), est_in(54 * TN), est_out(42 * TN), rpy(3 * TN), gait_out(24 * TN), gait_state(52 * TN), tau(12 * TN), qdes(24 * TN), flag(4 * TN);
    ok = rd(f, cmd_reset) && rd(f, mem_reset) && rd(f, joy) && rd(f, est_in) && rd(f, est_out) && rd(f, rpy) && rd(f, gait_out) && rd(f, gait_state) && rd(f, tau) &&
         rd(f, qdes) && rd(f, flag);
    fclose(f);
    if (!ok) return 2;
    const float poison = -12345.5f;
    std::vector<float> st(6 * N, poison), des(12 * N), fe(64 * N), fh(46 * N), sv(53 * N), sc(28 * N), sw(58 * N), ei(54 * N), cmd(60 * N);
    std::vector<int> mem(N, 0x7fffffff);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    for (int t = 0; t < T && ok; ++t) {
        for (auto *a : {&des, &fe, &fh, &sv, &sc, &sw, &cmd}) std::fill(a->begin(), a->end(), poison);
        memcpy(sw.data(), flag.data() + (size_t)t * 4 * N, 4 * N * sizeof(float));
        memcpy(ei.data(), est_in.data() + (size_t)t * 54 * N, 54 * N * sizeof(float));
        for (int r = 0; r < n; ++r) {
            dataflow::command_update(C, cmd_reset[(size_t)t * N + r] != 0, N, joy.data() + (size_t)t * 8 * N + r, st.data() + r, des.data() + r, fe.data() + r,
                                     fh.data() + r, sv.data() + r, sc.data() + r);
            dataflow::trot_inputs(N, ei.data() + r, est_out.data() + (size_t)t * 42 * N + r, rpy.data() + (size_t)t * 3 * N + r, gait_out.data() + (size_t)t * 24 * N + r,
                                  gait_state.data() + (size_t)t * 52 * N + r, fe.data() + r, fh.data() + r, sw.data() + r, ei.data() + r);
            dataflow::mpc_command(M, mem_reset[(size_t)t * N + r] != 0, N, tau.data() + (size_t)t * 12 * N + r, qdes.data() + (size_t)t * 24 * N + r, sw.data() + r,
                                  gait_out.data() + (size_t)t * 24 * N + r, gait_state.data() + (size_t)t * 52 * N + r, mem.data() + r, cmd.data() + r);
        }
        ok = wr(f, st) && wr(f, des) && wr(f, fe) && wr(f, fh) && wr(f, sv) && wr(f, sc) && wr(f, sw) && wr(f, ei) && wr(f, mem) && wr(f, cmd);
    }
    fclose(f);
    return ok ? 0 : 2;
}
