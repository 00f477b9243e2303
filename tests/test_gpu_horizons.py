"""-m gpu: every MPC horizon the C ABI accepts (1..16) and the batch sizes at which the dispatch changes its form, against the CPU oracle.

The kernels branch on the horizon (h <= 11: register-resident blocks, the rescue / planned list launches; h = 11 alone takes a whole CU for its
main pass; h > 11: two workgroups per CU from 7 num_cu / 2 robots on) and on the batch size (below 64 robots: one whole-CU launch; from 64: the
longest-first order and the list launches; from 4096: the chunked WBC launch of the laboratory).  Each of those forms is held here at its edges.
Tolerances are the suite's: assembly bit-exact on stance x stance entries, forces 1e-5 max(1, |f|max) per robot, torques G.tau_tol."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_helpers as G
from test_gpu_frontend import frontend_parity
from test_gpu_mpc import bf16x3_vs_oracle
from test_gpu_overlap import _compare, _run_sequence

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HORIZONS = list(range(1, 17))
QR_QH = 96                      # working-set positions of the whole-CU kernels (qr_device_types.h)


@pytest.fixture
def ctx(gpu_ctx, pkg):
    """The session context, handed back at h = 10 with the motor tail off (what the other modules assume)."""
    yield gpu_ctx
    gpu_ctx.set_torque_epilogue(False, False)
    G.setup_a1(gpu_ctx, pkg, 10)


def _gait_mix(b):
    """Robots 0..3: all stance, three legs, flight, flight now / stance later (at h = 1: flight); the rest keep their drawn tables."""
    n, h = b["n"], b["horizon"]
    g = b["gait"].reshape(n, h, 4).copy()
    g[0] = 1.0
    g[1] = 1.0; g[1, :, 2] = 0.0
    g[2] = 0.0
    g[3] = 0.0; g[3, (h + 1) // 2:, :] = 1.0
    b["gait"] = g.reshape(n, 4 * h)
    return b


def _oracle_mpc(oracle, pkg, b, robot="a1"):
    cfg, geom = pkg.mpc_cfg(robot), pkg.model_desc(robot)[:3]
    n, h = b["n"], b["horizon"]
    f = np.zeros((n, 12)); tau = np.zeros((n, 12), np.float32); n_act = np.zeros(n, int)
    for i in range(n):
        u, st, rc = oracle.mpc_solve(cfg, h, b["mpc_state"][i], b["traj"][i], b["gait"][i])
        assert rc == 0, (h, i, rc)
        f[i] = u[:12]; n_act[i] = st["n_active"]
        tau[i] = oracle.mpc_force_to_torque(geom, b["fb_state"][i, 0:4], b["fb_state"][i, 13:25], u[:12])
    return f, tau, n_act


def _force_err(got, ref):
    """per robot: max |df| / max(1, |f|max)"""
    return np.abs(got - ref).max(1) / np.maximum(1.0, np.abs(ref).max(1))


def _check_mpc(out, f, tau, what, rows=None):
    rows = np.arange(len(f)) if rows is None else rows
    fl = G.flags(out["status"][rows])
    assert np.all(fl == 0), (what, np.unique(fl), rows[fl != 0][:8])
    ef = _force_err(out["force"][rows], f)
    assert ef.max() <= 1e-5, (what, int(rows[ef.argmax()]), ef.max())
    assert np.all(np.abs(out["tau"][rows] - tau) <= G.tau_tol(tau)), (what, np.abs(out["tau"][rows] - tau).max())


def _check_tick(oracle, pkg, b, out, what, rows=None, epilogue=0, robot="a1"):
    """The full tick's forces and torques (and the orientation task's memory, bit for bit) against the threaded oracle on `rows`."""
    rows = np.arange(b["n"]) if rows is None else np.asarray(rows)
    md = pkg.model_desc(robot)
    f, tau, st, _, prev = oracle.tick_batch(1, pkg.mpc_cfg(robot), b["horizon"], md[:3], md, b["mpc_state"][rows], b["traj"][rows], b["gait"][rows],
                                            b["fb_state"][rows], b["wbc_cmd"][rows], b["prev_ori_vel"][rows].copy(), nthreads=16, epilogue=epilogue)
    assert np.all(st == 0), what
    fl = G.flags(out["status"][rows])
    assert np.all(fl == 0), (what, np.unique(fl), rows[fl != 0][:8])
    ef = _force_err(out["force"][rows], f)
    assert ef.max() <= 1e-5, (what, int(rows[ef.argmax()]), ef.max())
    assert np.all(np.abs(out["tau"][rows] - tau) <= G.tau_tol(tau)), (what, np.abs(out["tau"][rows] - tau).max())
    assert np.array_equal(out["prev"][rows], prev), what


def _sample(out, n, k=256, seed=0):
    """every robot up to 1024; beyond, k random ones -- always with the 32 robots of the most iterations"""
    if n <= 1024:
        return np.arange(n)
    top = np.argsort(-G.iterations(out["status"]), kind="stable")[:32]
    return np.union1d(np.random.default_rng(seed).choice(n, k, replace=False), top)


# ---------------------------------------------------------------------------------------------------- B: the horizon sweep

@pytest.mark.parametrize("h", HORIZONS)
def test_assembly_bit_exact_every_horizon(ctx, pkg, oracle, h):
    """K1-K4 (qrgpu_mpc_assemble_batch, no status output): every stance x stance entry finite and bit-identical to the oracle's dense GEMM, every
    swing entry untouched -- a robot the kernel skipped shows as NaN where the oracle has numbers.  Tile edges: 12 h is a multiple of 16 only
    at h = 0 mod 4, and h = 1..3 give one to three tiles."""
    G.setup_a1(ctx, pkg, h)
    cfg = pkg.mpc_cfg("a1")
    b = _gait_mix(pkg.make_batch(16, h, "a1", seed=0x600 + h, frac_all_stance=0.2, frac_three_leg=0.2))
    Hg, gg = G.run_assemble(ctx, pkg, b)
    for i in range(b["n"]):
        Ho, go, ub = oracle.mpc_assemble(cfg, h, b["mpc_state"][i], b["traj"][i], b["gait"][i])
        free = np.repeat(ub[4::5] > 0, 3)
        m2 = np.outer(free, free)
        assert np.all(np.isfinite(Hg[i][m2])) and np.all(np.isfinite(gg[i][free])), (h, i)
        assert np.array_equal(Hg[i][m2].view(np.uint32), Ho[m2].view(np.uint32)), "H differs bitwise (h %d, robot %d)" % (h, i)
        assert np.array_equal(gg[i][free].view(np.uint32), go[free].view(np.uint32)), "g differs bitwise (h %d, robot %d)" % (h, i)
        assert np.all(np.isnan(Hg[i][~m2])) and np.all(np.isnan(gg[i][~free])), (h, i)      # swing entries are never touched
    assert np.all(np.isnan(Hg[2])) and np.all(np.isfinite(Hg[0]))


@pytest.mark.parametrize("h", HORIZONS)
def test_mpc_parity_every_horizon(ctx, pkg, oracle, h):
    """128 robots (past the 64 of the longest-first order: main pass, rescue and planned list launches) with all-stance and three-leg robots at
    1.5 x the ranges, and 7 robots with the edge gaits (the whole-CU launch of batches below 64 at h <= 11; the one-workgroup-per-CU variant
    above): no flags, every robot's forces and J^T f torques against the oracle."""
    G.setup_a1(ctx, pkg, h)
    b = pkg.make_batch(128, h, "a1", seed=0x700 + h, frac_all_stance=0.15, frac_three_leg=0.1, excite=1.5)
    out = G.run_mpc(ctx, pkg, b)
    f, tau, _ = _oracle_mpc(oracle, pkg, b)
    _check_mpc(out, f, tau, "h %d n 128" % h)
    small = _gait_mix(pkg.make_batch(7, h, "a1", seed=0x780 + h, excite=1.5))
    out = G.run_mpc(ctx, pkg, small)
    f, tau, _ = _oracle_mpc(oracle, pkg, small)
    _check_mpc(out, f, tau, "h %d n 7" % h)
    assert np.all(out["force"][2] == 0) and np.all(out["tau"][2] == 0) and np.all(out["force"][3] == 0)


@pytest.mark.parametrize("h,first_step_flight,excite", [(15, False, 1.5), (16, True, 2.0)])
def test_h_above_11_working_sets_beyond_the_lds_held_rows(ctx, pkg, oracle, h, first_step_flight, excite):
    """Below 7 num_cu / 2 robots h > 11 runs one workgroup per CU and no list launch.  Behind the inverse Hessian of 60 stance leg-steps that CU's
    LDS holds 66-68 rows of S^-1; S^-1 used to go to the global scratch only when fewer than 64 rows fitted there, so a working set of 69..96 rows
    (h = 15 all stance, h = 16 with the first step in flight) was flagged QRGPU_ST_MPC_OVERFLOW and never solved.  Every robot but those whose
    oracle active set exceeds the 96 positions against the oracle, and there are robots between."""
    G.setup_a1(ctx, pkg, h)
    b = pkg.make_batch(64, h, "a1", seed={15: 0xF15, 16: 0xF16}[h], frac_all_stance=1.0, frac_three_leg=0.0, excite=excite)
    if first_step_flight:
        g = b["gait"].reshape(64, h, 4); g[:, 0, :] = 0.0; b["gait"] = g.reshape(64, 4 * h)
    out = G.run_mpc(ctx, pkg, b)
    f, tau, n_act = _oracle_mpc(oracle, pkg, b)
    ok = n_act <= QR_QH
    assert ((n_act > 68) & ok).sum() >= 4, n_act
    assert np.all((G.flags(out["status"][~ok]) & 0x4) != 0)
    _check_mpc(out, f[ok], tau[ok], "h %d" % h, rows=np.nonzero(ok)[0])


@pytest.mark.parametrize("h", HORIZONS)
def test_full_tick_every_horizon(ctx, pkg, oracle, h):
    """The pipelined tick (MPC -> WBC) at 256 robots with the K14 motor tail on, every robot against the oracle's tick (epilogue 3)."""
    G.setup_a1(ctx, pkg, h)
    b = pkg.make_batch(256, h, "a1", seed=0x800 + h)
    ctx.set_torque_epilogue(hip_comp=True, clip=True)
    out = G.run_tick(ctx, pkg, b)
    _check_tick(oracle, pkg, b, out, "h %d" % h, epilogue=3)
    assert np.abs(out["tau"]).max() <= 23.0


@pytest.mark.parametrize("h", HORIZONS)
@pytest.mark.parametrize("L", [2, 3])
def test_frontend_parity_every_horizon(ctx, pkg, oracle, h, L):
    """qrgpu_mpc_frontend_batch launches dim3(64, h): one row of threads per horizon step (a 1024-thread block at h = 16).  1000 robots (ragged)."""
    frontend_parity(ctx, pkg, oracle, h, L, n=1000, seed=0x900 + 16 * L + h)


@pytest.mark.parametrize("h,n,mixed", [(1, 64, False), (4, 64, True), (11, 128, False), (15, 128, True)])
def test_bf16x3_at_more_horizons(ctx, pkg, oracle, h, n, mixed):
    """The bf16-limb Hessian mode at a single step, at one tile edge (h = 4: 48 = 3 tiles exactly), at the last small horizon and at h = 15,
    with test_bf16x3_solve_vs_oracle_on_its_own_hessian's comparator (the oracle solving the (H, g) this mode assembled)."""
    bf16x3_vs_oracle(ctx, pkg, oracle, h, n, mixed)


# ---------------------------------------------------------------------------------------------------- C: the class boundaries h = 11 and 12

def test_h11_all_stance_through_the_list_launches(ctx, pkg, oracle):
    """h = 11 is the last horizon of the register-resident class and the only one whose main pass takes a whole CU (tri(44) = 990 blocks; 83 KB
    of LDS).  512 all-stance robots at twice the ranges: working sets beyond the main pass's rows go to the list launches.  With the rescue
    pass on nobody is flagged but a robot whose oracle active set exceeds the 96 positions of the whole-CU kernels; two cold calls agree bit
    for bit; every robot against the oracle."""
    h, n = 11, 512
    G.setup_a1(ctx, pkg, h)
    b = pkg.make_batch(n, h, "a1", seed=0xB11, excite=2.0, frac_all_stance=1.0, frac_three_leg=0.0)
    ctx.set_rescue_pass(False)
    try:
        flagged = (G.run_mpc(ctx, pkg, b)["status"] & 0x4) != 0
    finally:
        ctx.set_rescue_pass(True)
    with G.cold_start(ctx):
        out = G.run_mpc(ctx, pkg, b)
        out2 = G.run_mpc(ctx, pkg, b)
    assert flagged.sum() > 0, "the batch must exercise the list launches"
    assert np.array_equal(out["force"], out2["force"]) and np.array_equal(out["status"], out2["status"])
    f, tau, n_act = _oracle_mpc(oracle, pkg, b)
    over = n_act > QR_QH
    fl = G.flags(out["status"])
    assert np.all(fl[~over] == 0), (np.unique(fl[~over]), np.nonzero((fl != 0) & ~over)[0][:8], n_act[(fl != 0) & ~over][:8])
    assert np.all((fl[over] & 0x4) != 0)
    ok = ~over
    ef = _force_err(out["force"][ok], f[ok])
    assert ef.max() <= 1e-5, (int(np.nonzero(ok)[0][ef.argmax()]), ef.max())
    assert np.all(np.abs(out["tau"][ok] - tau[ok]) <= G.tau_tol(tau[ok]))


def test_h11_overlapped_ticks_match_the_plain_tick(pkg, oracle):
    """Overlapped ticks at h = 11 (its main pass on whole CUs, its list launches in the overlapped form) against the serial tick over a sequence
    with 30 % all-stance robots within SURVEY.md 8d's ranges (where a trotting robot never needs a list launch): chained, no robot flagged or
    unsolved that the serial tick solves, trotting robots bit for bit, the rest to the solver's tolerance (_compare), the last tick against the
    oracle."""
    h, n = 11, 512
    seq = pkg.make_batch_sequence(n, h, "a1", seed=0x0B11, steps=6, frac_all_stance=0.3, excite=1.0)
    ser, prevs, prev_s, _ = _run_sequence(pkg, seq, h, n, "serial", True)
    ovl, _, prev_o, stats = _run_sequence(pkg, seq, h, n, "overlap", False)
    assert stats[0] >= 1 and stats[0] + stats[1] <= 6, stats          # (once a lane has a plan the context goes back to the plain pipelined tick)
    for k, (x, y) in enumerate(zip(ser, ovl)):
        assert np.all(np.isfinite(y["tau"])) and np.all(np.isfinite(y["force"])), k
        lost = (G.flags(y["status"]) != 0) & (G.flags(x["status"]) == 0)
        assert not lost.any(), (k, np.nonzero(lost)[0][:8], [hex(int(v)) for v in G.flags(y["status"][lost][:8])])
    _compare(pkg, seq, ser, ovl, h, "h = 11 overlap vs serial")
    last, b = ovl[-1], seq[-1]
    md = pkg.model_desc("a1")
    f, tau, st, sec, prev = oracle.tick_batch(1, pkg.mpc_cfg("a1"), h, md[:3], md, b["mpc_state"], b["traj"], b["gait"], b["fb_state"], b["wbc_cmd"],
                                              prevs[-2].copy(), nthreads=16, epilogue=3)
    ok = (G.flags(last["status"]) == 0) & (st == 0)
    assert ok.mean() > 0.97, ok.mean()
    assert np.all(np.abs(last["tau"][ok] - tau[ok]) <= G.tau_tol(tau[ok])), np.abs(last["tau"][ok] - tau[ok]).max()
    assert _force_err(last["force"][ok], f[ok]).max() <= 1e-5


@pytest.mark.parametrize("edge", [-1, 0])
def test_h12_across_the_two_per_cu_threshold(ctx, pkg, oracle, edge):
    """h > 11 runs its main pass two workgroups to a CU from 7 num_cu / 2 robots on (one below: one per CU).  A1 and Lite3 interleaved, two full
    ticks (the first without a plan, the second with one), every robot of both types against the oracle."""
    h = 12
    n = 7 * ctx.device_info()["cus"] // 2 + edge
    G.setup_a1(ctx, pkg, h)
    ctx.mpc_setup_packed(1, pkg.mpc_cfg("lite3"), h); ctx.wbc_setup_packed(1, pkg.model_desc("lite3"))
    na = (n + 1) // 2
    ba = pkg.make_batch(na, h, "a1", seed=0xC12 + edge); bl = pkg.make_batch(n - na, h, "lite3", seed=0xD12 + edge)
    b = dict(ba); b["n"] = n
    for k in ("mpc_state", "traj", "gait", "fb_state", "wbc_cmd", "prev_ori_vel"):
        b[k] = np.empty((n,) + ba[k].shape[1:], ba[k].dtype); b[k][0::2] = ba[k]; b[k][1::2] = bl[k]
    tid = (np.arange(n) % 2).astype(np.int32)
    for tick in range(2):
        out = G.run_tick(ctx, pkg, b, type_id=tid)
        for t, robot, part in ((0, "a1", ba), (1, "lite3", bl)):
            sel = np.nonzero(tid == t)[0]
            sub = {k: out[k][sel] for k in ("force", "tau", "status", "prev")}
            _check_tick(oracle, pkg, part, sub, "n %d tick %d %s" % (n, tick, robot), robot=robot)


# ---------------------------------------------------------------------------------------------------- D: batch-size edges

@pytest.mark.parametrize("h", [10, 16])
@pytest.mark.parametrize("n", [1, 7, 9, 63, 64, 65, 1023, 1025, 4096])
def test_full_tick_at_batch_size_edges(ctx, pkg, oracle, h, n):
    """One robot, the WBC's workgroups of 8 robots (7, 9), the 64 of the whole-CU small-batch launch and of the longest-first order, 1024 and
    the session context's largest batch; beyond 1024 robots 256 sampled ones and the 32 of the most iterations against the oracle."""
    G.setup_a1(ctx, pkg, h)
    b = pkg.make_batch(n, h, "a1", seed=0xE00 + n + h)
    out = G.run_tick(ctx, pkg, b)
    assert np.all(G.flags(out["status"]) == 0), np.unique(G.flags(out["status"]))
    assert np.all(np.isfinite(out["tau"])) and np.all(np.isfinite(out["force"]))
    _check_tick(oracle, pkg, b, out, "h %d n %d" % (h, n), rows=_sample(out, n))


_BIG = r"""
import os, sys
import numpy as np
root, dst = sys.argv[1], sys.argv[2]
sys.path.insert(0, os.path.join(root, "tests"))
import conftest, gpu_helpers as G
pkg = conftest.load_pkg()
h, n = 10, 8192
ctx = pkg.Context(0, n, 16)
try:
    G.setup_a1(ctx, pkg, h)
    ctx.set_tick_pipeline(True)
    ctx.set_torque_epilogue(hip_comp=True, clip=True)
    seq = pkg.make_batch_sequence(n, h, "a1", seed=0x8192, steps=3)
    outs = [G.run_tick(ctx, pkg, b, want_qdes=True) for b in seq]
finally:
    ctx.close()
np.savez(dst, **{"%s_%d" % (k, t): o[k] for t, o in enumerate(outs) for k in ("force", "tau", "status", "prev", "qdes")})
print("BIG_OK")
"""


def test_8192_robots_in_one_call_and_the_chunked_wbc_launch(pkg, oracle, tmp_path):
    """8192 robots per call (a context of max_batch 8192), h = 10, three pipelined ticks with K12 and the K14 tail, overlap off,
    in two fresh processes -- the default one-launch WBC and the laboratory's chunked one (QRGPU_LAB=1 QRGPU_WBC_CHUNKS=1: launches of 1024
    workgroups behind gates of their own, LAB_NOTES A.7) -- which must agree bit for bit.  Every robot of every tick: no flag, the friction pyramid,
    zero force on swing feet, the +-23 N m clip; 256 sampled robots and the 32 of the most iterations of the last tick against the oracle."""
    h, n = 10, 8192
    res = []
    for lab in (False, True):
        env = {k: v for k, v in os.environ.items() if k not in ("QRGPU_LAB", "QRGPU_WBC_CHUNKS")}
        if lab:
            env.update(QRGPU_LAB="1", QRGPU_WBC_CHUNKS="1")
        dst = str(tmp_path / ("big_%d.npz" % lab))
        r = subprocess.run([sys.executable, "-c", _BIG, ROOT, dst], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "BIG_OK" in r.stdout
        res.append(dict(np.load(dst)))
    plain, chunked = res
    for k in plain:
        assert np.array_equal(plain[k].view(np.uint8), chunked[k].view(np.uint8)), k
    seq = pkg.make_batch_sequence(n, h, "a1", seed=0x8192, steps=3)
    mu, fmax = np.float32(0.45), np.float32(13 * 9.81)
    for t, b in enumerate(seq):
        o = {k: plain["%s_%d" % (k, t)] for k in ("force", "tau", "status", "prev", "qdes")}
        assert np.all(G.flags(o["status"]) == 0), (t, np.unique(G.flags(o["status"])))
        f = o["force"].reshape(n, 4, 3)
        assert np.all(f[:, :, 2] >= -1e-6) and np.all(f[:, :, 2] <= fmax * (1 + 1e-6)), t
        assert np.all(np.abs(f[:, :, 0]) <= mu * f[:, :, 2] + 1e-5) and np.all(np.abs(f[:, :, 1]) <= mu * f[:, :, 2] + 1e-5), t
        assert np.all(f[b["gait"][:, :4] == 0] == 0), t
        assert np.all(np.isfinite(o["tau"])) and np.abs(o["tau"]).max() <= 23.0, t
    _check_tick(oracle, pkg, seq[-1], o, "8192 robots, last tick", rows=_sample(o, n, seed=1), epilogue=3)


def test_argument_edges_return_bad_arg_and_touch_nothing(ctx, pkg, oracle):
    """n = max_batch + 1 (and 0) on every batched MPC entry: QRGPU_ERR_BAD_ARG, the poisoned outputs as they were.  Horizons 0 and 17, and one above
    the context's horizon_max, are refused by qrgpu_mpc_setup and leave the setup as it was; horizon_max 17 is refused by qrgpu_create."""
    h = 10
    G.setup_a1(ctx, pkg, h)
    mb = ctx.max_batch
    S = pkg.to_soa
    for n in (mb + 1, 0):
        m = max(n, 1)
        b = pkg.make_batch(m, h, "a1", seed=0xBAD)
        d = dict(state=ctx.alloc((28, m)).upload(S(b["mpc_state"])), traj=ctx.alloc((12 * h, m)).upload(S(b["traj"])), gait=ctx.alloc((4 * h, m)).upload(S(b["gait"])),
                 fb=ctx.alloc((37, m)).upload(S(b["fb_state"])), cmd=ctx.alloc((67, m)).upload(S(b["wbc_cmd"])), prev=ctx.alloc((3, m)).upload(S(b["prev_ori_vel"])),
                 q=ctx.alloc((12, m)).upload(S(b["fb_state"][:, 13:25])),
                 force=ctx.alloc((12, m)).upload(np.full((12, m), np.nan, np.float32)), tau=ctx.alloc((12, m)).upload(np.full((12, m), np.nan, np.float32)),
                 qdes=ctx.alloc((24, m)).upload(np.full((24, m), np.nan, np.float32)), status=ctx.alloc((m,), np.int32).upload(np.full((m,), 0x7f0000ff, np.int32)))
        calls = (lambda: ctx.tick_batch(n, d["state"], d["traj"], d["gait"], d["fb"], d["cmd"], d["prev"], d["force"], d["tau"], d["status"], qdes=d["qdes"]),
                 lambda: ctx.mpc_solve_batch(n, d["state"], d["traj"], d["gait"], d["q"], d["force"], d["tau"], d["status"]),
                 lambda: ctx.wbc_run_batch(n, d["fb"], d["cmd"], d["prev"], d["tau"], d["qdes"], d["status"]))
        for call in calls:
            with pytest.raises(pkg.QrgpuError, match="BAD_ARG"):
                call()
        ctx.sync()
        assert np.all(np.isnan(d["force"].download())) and np.all(np.isnan(d["tau"].download())) and np.all(np.isnan(d["qdes"].download())), n
        assert np.all(d["status"].download() == 0x7f0000ff), n
        assert np.array_equal(d["prev"].download(), S(b["prev_ori_vel"])), n
        for v in d.values():
            v.free()
    for bad in (0, 17, -1):
        with pytest.raises(pkg.QrgpuError, match="BAD_ARG"):
            ctx.mpc_setup_packed(0, pkg.mpc_cfg("a1"), bad)
    # the refused calls left the setup at h = 10: a batch solves as before
    b = _gait_mix(pkg.make_batch(8, h, "a1", seed=0xBAE))
    out = G.run_mpc(ctx, pkg, b)
    f, tau, _ = _oracle_mpc(oracle, pkg, b)
    _check_mpc(out, f, tau, "after refused setups")
    # a context whose horizon_max is 12 (a separate context: the session's allows 16)
    small = pkg.Context(0, 64, 12)
    try:
        for bad in (13, 16):
            with pytest.raises(pkg.QrgpuError, match="BAD_ARG"):
                small.mpc_setup_packed(0, pkg.mpc_cfg("a1"), bad)
        with pytest.raises(pkg.QrgpuError, match="NOT_SETUP"):         # nothing was set up by the refused calls
            G.run_mpc(small, pkg, pkg.make_batch(8, 12, "a1", seed=1))
        G.setup_a1(small, pkg, 12)
        b = _gait_mix(pkg.make_batch(8, 12, "a1", seed=0xBAF))
        out = G.run_mpc(small, pkg, b)
        f, tau, _ = _oracle_mpc(oracle, pkg, b)
        _check_mpc(out, f, tau, "horizon_max 12")
    finally:
        small.close()
    with pytest.raises(pkg.QrgpuError, match="BAD_ARG"):
        pkg.Context(0, 64, 17)
