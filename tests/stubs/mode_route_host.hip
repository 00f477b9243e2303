// The mode route, the masks of the cadenced tick and the merge (qr_mode_route.h) compiled for the host, driven over files, the robots one after the other
// as the kernels of qr_mode_route_kernel.hip run their lanes: arrays [row][n], a robot's column at stride n.
//   in:  int n, has_plan, sizeof(qrgpu_mode_route_desc), with_status; the desc; float sel[n]; int plan[n], updated[n]; float cmd_mpc[60][n], cmd_fb[60][n];
//        int st_mpc[n], st_fb[n]
//   out: int chain[n], flags[n], count[3], due[n], skip[n]; float out[60][n]; int st[n]; then the merge once more into each input: float out_in_mpc[60][n],
//        out_in_fb[60][n].  The merge runs on the routed chains.  count is the plain sum (the kernel's ballots are the device's business).  Without
//        with_status the merge gets no status inputs.  Every output starts at a poison value.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include "qr_mode_route.h"
using namespace qrgpu;

template <typename T> static bool rd(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[4];
    qrgpu_mode_route_desc D;
    bool ok = fread(hd, 4, 4, f) == 4 && hd[2] == (int)sizeof(D) && fread(&D, sizeof(D), 1, f) == 1;
    const int n = hd[0];
    ok = ok && n >= 1 && n <= (1 << 20);
    if (!ok) return 2;
    const size_t N = (size_t)n;
    std::vector<float> sel(N), a(QRGPU_MOTOR_CMD_ROWS * N), b(QRGPU_MOTOR_CMD_ROWS * N);
    std::vector<int> plan(N), updated(N), sa(N), sb(N);
    ok = rd(f, sel) && rd(f, plan) && rd(f, updated) && rd(f, a) && rd(f, b) && rd(f, sa) && rd(f, sb);
    fclose(f);
    if (!ok) return 2;
    const float poison = -12345.5f;
    std::vector<int> chain(N, 0x7fffffff), flags(N, 0x7fffffff), count(3, 0), due(N, 0x7fffffff), skip(N, 0x7fffffff), st(N, 0x7fffffff);
    std::vector<float> out(QRGPU_MOTOR_CMD_ROWS * N, poison), in_a(a), in_b(b);
    for (int r = 0; r < n; ++r) {
        chain[r] = mode_route::route(D, sel[r], hd[1] != 0, plan[r], flags[r]);
        if (chain[r] >= 0 && chain[r] < 3) ++count[chain[r]];
        mode_route::masks(updated[r], chain[r], due[r], skip[r]);
        const int *pa = hd[3] ? sa.data() + r : nullptr, *pb = hd[3] ? sb.data() + r : nullptr;
        mode_route::command(N, chain[r], a.data() + r, b.data() + r, pa, pb, out.data() + r, st.data() + r);
        mode_route::command(N, chain[r], in_a.data() + r, b.data() + r, pa, pb, in_a.data() + r, nullptr);
        mode_route::command(N, chain[r], a.data() + r, in_b.data() + r, pa, pb, in_b.data() + r, nullptr);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    ok = wr(f, chain) && wr(f, flags) && wr(f, count) && wr(f, due) && wr(f, skip) && wr(f, out) && wr(f, st) && wr(f, in_a) && wr(f, in_b);
    fclose(f);
    return ok ? 0 : 2;
}
