// The walk pose planner's kernel source compiled for the host (QR_POSE_PLAN_HOST: the lanes of a wavefront as a loop), driven over files:
//   in:  int n, reset; qrgpu_pose_plan_desc; [rows][n] float arrays est_in 29, est_out 40, ground 31, rpy 3, walk 41, state 26, cmd 28; int event[n]
//   out: state, cmd, pose_out [QRGPU_POSE_OUT_ROWS][n], int flags[n]
// The helpers of qr_wave_helpers.h are device functions; for this build they are host functions as well.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#define QR_POSE_PLAN_HOST
#include "qr_pose_plan_kernel.hip"
#include <cstdio>
#include <vector>
using namespace qrgpu;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n = 0, reset = 0;
    qrgpu_pose_plan_desc D;
    bool ok = fread(&n, 4, 1, f) == 1 && fread(&reset, 4, 1, f) == 1 && fread(&D, sizeof(D), 1, f) == 1 && n > 0 && n <= 4096;
    auto rd = [&](int rows) { std::vector<float> v((size_t)rows * n); ok = ok && fread(v.data(), 4, v.size(), f) == v.size(); return v; };
    if (!ok) return 2;
    auto est_in = rd(29), est_out = rd(40), ground = rd(31), rpy = rd(3), walk = rd(41), state = rd(QRGPU_POSE_STATE_ROWS), cmd = rd(28);
    std::vector<int> ev(n);
    ok = ok && fread(ev.data(), 4, n, f) == (size_t)n;
    fclose(f);
    if (!ok) return 2;
    std::vector<float> out((size_t)QRGPU_POSE_OUT_ROWS * n, -777.f);
    std::vector<int> flags(n, -12345);
    static PoseWork W;
    for (int r = 0; r < n; ++r)
        if (ev[r] == 1 || ev[r] == 2)
            pose_plan_robot(W, 0, r, n, D, ev[r], reset, est_in.data(), est_out.data(), ground.data(), rpy.data(), walk.data(), state.data(), cmd.data(),
                            out.data(), flags.data());
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(state.data(), 4, state.size(), f); fwrite(cmd.data(), 4, cmd.size(), f); fwrite(out.data(), 4, out.size(), f); fwrite(flags.data(), 4, n, f);
    fclose(f);
    return 0;
}
