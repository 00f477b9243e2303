// The two maps of the cadenced tick (qr_cadence.h) compiled for the host, driven over files, the robots one after the other as qr_cadence_kernel runs
// its lanes: arrays [row][n], a robot's column at stride n.
//   in:  int n; float hip_l, upper_l, lower_l; float quat[4][n] (w, x, y, z), force[12][n], q[12][n]
//   out: float hold[12][n] = -R^T f, tau[12][n] = J(q)^T hold.  Both start at the poison value.
#include <hip/hip_runtime.h>
// the helpers of qr_wave_helpers.h are __device__ functions: on the host build they are host functions too
#define __device__ __attribute__((host)) __attribute__((device))
#include <cmath>
#include <cstdio>
#include <vector>
#include "qr_cadence.h"
using namespace qrgpu;

template <typename T> static bool rd(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n = 0;
    float legs[3];
    bool ok = fread(&n, 4, 1, f) == 1 && fread(legs, 4, 3, f) == 3 && n >= 1 && n <= 65536;
    if (!ok) return 2;
    const size_t N = (size_t)n;
    std::vector<float> quat(4 * N), force(12 * N), q(12 * N);
    ok = rd(f, quat) && rd(f, force) && rd(f, q);
    fclose(f);
    if (!ok) return 2;
    const float poison = -12345.5f;
    std::vector<float> hold(12 * N, poison), tau(12 * N, poison);
    for (int r = 0; r < n; ++r) {
        cadence::hold_from_force(N, quat.data() + r, force.data() + r, hold.data() + r);
        cadence::held_torque(legs[0], legs[1], legs[2], N, q.data() + r, hold.data() + r, tau.data() + r);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    ok = wr(f, hold) && wr(f, tau);
    fclose(f);
    return ok ? 0 : 2;
}
