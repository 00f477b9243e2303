// The control state machine (qr_fsm.h) compiled for the host, driven over files, the robots one after the other as the kernels of qr_fsm_kernel.hip run
// their lanes: arrays [row][n], a robot's column at stride n.  Per tick: update, zero command, command.
//   in:  int n, T, n_script, sizeof(qrgpu_fsm_desc); the desc; int reset[T][n]; float joy_msg[T][10][n]; int ticks[T][n]; float script[5][n_script];
//        float est_in[T][54][n], loco[T][60][n]
//   out: per tick: float state[106][n], joy[8][n]; int plan[n], mask[n]; float state_des[12][n], fe_in[64][n], fh_in[46][n], swing_vel_in[53][n],
//        stance_cmd[28][n], motor_cmd[60][n], fsm_out[11][n].  The resets go through done words (0x40 under bits 0xff; every other robot carries a word
//        outside the bits).  Every output but the state starts every tick at the poison value; the state is carried and starts at poison.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "qr_fsm.h"
using namespace qrgpu;

template <typename T> static bool rd(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[4];
    qrgpu_fsm_desc D;
    bool ok = fread(hd, 4, 4, f) == 4 && hd[3] == (int)sizeof(D) && fread(&D, sizeof(D), 1, f) == 1;
    const int n = hd[0], T = hd[1], ns = hd[2];
    ok = ok && n >= 1 && n <= 4096 && T >= 1 && T <= 8192 && ns >= 0 && ns <= QRGPU_FSM_SCRIPT_MAX;
    if (!ok) return 2;
    const size_t N = (size_t)n, TN = (size_t)T * N;
    std::vector<int> reset(TN), ticks(TN);
    std::vector<float> msg(QRGPU_JOY_MSG_ROWS * TN), script((size_t)QRGPU_FSM_SCRIPT_ROWS * ns), est_in(54 * TN), loco(QRGPU_MOTOR_CMD_ROWS * TN);
    ok = rd(f, reset) && rd(f, msg) && rd(f, ticks) && rd(f, script) && rd(f, est_in) && rd(f, loco);
    fclose(f);
    if (!ok) return 2;
    const float poison = -12345.5f;
    std::vector<float> st(QRGPU_FSM_STATE_ROWS * N, poison), joy(QRGPU_JOY_ROWS * N), des(12 * N), fe(64 * N), fh(46 * N), sv(53 * N), sc(28 * N),
        cmd(QRGPU_MOTOR_CMD_ROWS * N), out(QRGPU_FSM_OUT_ROWS * N);
    std::vector<int> plan(N), mask(N), done(N);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    for (int t = 0; t < T && ok; ++t) {
        for (auto *a : {&joy, &des, &fe, &fh, &sv, &sc, &cmd, &out}) std::fill(a->begin(), a->end(), poison);
        std::fill(plan.begin(), plan.end(), 0x7fffffff);
        std::fill(mask.begin(), mask.end(), 0x7fffffff);
        for (int r = 0; r < n; ++r) done[r] = reset[(size_t)t * N + r] ? 0x40 : 0x01000000;
        for (int r = 0; r < n; ++r) {
            fsm::update(D, 0, N, msg.data() + (size_t)t * QRGPU_JOY_MSG_ROWS * N + r, ns ? script.data() : nullptr, ns, ns ? ticks.data() + (size_t)t * N + r : nullptr,
                        done.data() + r, 0xffu, st.data() + r, joy.data() + r, plan.data() + r, mask.data() + r);
            fsm::zero_command(N, plan[r], des.data() + r, fe.data() + r, fh.data() + r, sv.data() + r, sc.data() + r);
            fsm::command(D, N, plan[r], est_in.data() + (size_t)t * 54 * N + r, loco.data() + (size_t)t * QRGPU_MOTOR_CMD_ROWS * N + r, st.data() + r, cmd.data() + r,
                         out.data() + r);
        }
        ok = wr(f, st) && wr(f, joy) && wr(f, plan) && wr(f, mask) && wr(f, des) && wr(f, fe) && wr(f, fh) && wr(f, sv) && wr(f, sc) && wr(f, cmd) && wr(f, out);
    }
    fclose(f);
    return ok ? 0 : 2;
}
