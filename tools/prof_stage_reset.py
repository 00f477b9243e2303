"""Workload for the per-launch times of the eight stage kernels with memory, bound and unbound: ground, estimator, gait,
walk gait, swing update (position mode), stance update (ADVANCED_TROT), pose plan and MPC front-end at 1024 robots, every tick all eight, the
ticks alternating between an unbound call (even ticks) and a bound one (odd ticks; qrgpu_set_stage_reset: mask and tick arrays on the device),
meant to run under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o zero   -- python tools/prof_stage_reset.py
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o masked -- python tools/prof_stage_reset.py --all-masked

Default: an all-zero mask and tick counts that follow the scalar clock, so the bound and the unbound ticks compute the same thing and the trace
compares one kernel with and without the two row loads of a binding.  --all-masked: every robot is reset at every bound tick (the estimator's zeroing pass).  The inputs change
every third tick, so each input set, and each change of inputs (a ground fit fires on newly made contacts), meets both forms equally often.

    python tools/prof_stage_reset.py --summarise OUT/zero_kernel_trace.csv [OUT/masked_kernel_trace.csv]

prints, per kernel and trace, calls, median, min and max of the launch durations as CSV (profiles/stage_one_text_kernel_stats.csv), the unbound
and the bound ticks apart.  Both run the same kernel: every tick launches each kernel once, so in start order the k-th launch of a kernel belongs to
tick k, and the odd ticks are the bound ones."""
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = ("qr_ground_kernel", "qr_estimator_kernel", "qr_gait_kernel", "qr_walk_gait_kernel", "qr_swing_update_kernel", "qr_stance_update_kernel",
          "qr_pose_plan_kernel", "qr_frontend_kernel")


def main(all_masked, n=1024, ticks=600):
    from conftest import load_pkg
    import gpu_helpers as G
    import pose_plan_ref as P
    import stage_ref as SR
    import stance_ref as R
    pkg = load_pkg()
    pkg._build.build()
    W = pkg.workload
    S = pkg.to_soa
    ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    G.setup_a1(ctx, pkg, 10)
    rng = np.random.default_rng(23)
    up = lambda a: ctx.alloc(a.shape, a.dtype).upload(a)
    gin = G.ground_sequences(n, 2, seed=24)
    x, _ = SR.wide_sensor_streams(n, 2, 25)
    d_gin = [up(S(gin[j])) for j in range(2)]; d_x = [up(S(x[j])) for j in range(2)]
    d_stamp = ctx.alloc((n,), np.uint32)
    window = 120
    d_gst = ctx.alloc((13, n), np.float64); d_gout = ctx.alloc((32, n))
    d_est = up(np.zeros((96 + 3 * window, n), np.float64)); d_eo = ctx.alloc((42, n))
    d_ct = up(np.ones((4, n), np.float32))
    d_gs, d_go, d_fe = ctx.alloc((52, n)), ctx.alloc((24, n)), ctx.alloc((64, n))
    d_ws, d_wo = ctx.alloc((33, n)), ctx.alloc((41, n))
    est_in = np.zeros((54, n), np.float32); est_in[6] = 1.0
    est_out = np.zeros((42, n), np.float32)
    est_out[12:24] = np.array([0.18, -0.13, -0.28, 0.18, 0.13, -0.28, -0.18, -0.13, -0.28, -0.18, 0.13, -0.28], np.float32)[:, None]
    est_out[36] = rng.uniform(-0.3, 0.3, n); est_out[38] = 0.28
    d_sei, d_seo = up(est_in), up(est_out)
    d_sst = ctx.alloc((pkg.qrgpu.SWING_STATE_FLOATS, n)); d_sfl = ctx.alloc((n,), np.int32)
    sti = [R.make_inputs(n, 3, seed=26 + j) for j in range(2)]
    d_sti = [{k: up(S(v)) for k, v in s.items()} for s in sti]
    d_st, d_vmc, d_ratio, d_sout = ctx.alloc((1, n)), ctx.alloc((37, n)), ctx.alloc((8, n)), ctx.alloc((33, n))
    cases = [P.pack_inputs([P.make_case(rng, swing_leg=(r % 5 if r % 5 < 4 else None), offset=rng.uniform(-0.02, 0.02, 3)) for r in range(n)]) for _ in range(2)]
    d_pp = [{k: up(S(v)) for k, v in c.items()} for c in cases]
    d_pst, d_pcmd, d_pfl = ctx.alloc((P.STATE_ROWS, n)), ctx.alloc((28, n)), ctx.alloc((n,), np.int32)
    fe, fst = W.make_frontend_batch(n, seed=28)
    d_fin, d_fst = up(S(fe)), up(S(fst))
    d_traj, d_gait, d_cmd, d_upd = ctx.alloc((120, n)), ctx.alloc((40, n)), ctx.alloc((67, n)), ctx.alloc((n,), np.int32)
    gcfg, wcfg, ecfg = W.gait_cfg(), W.walk_cfg(stance_duration=0.75), W.estimator_cfg("a1", window=window)
    sdesc, tdesc, pdesc = pkg.swing_mode_desc(1), pkg.stance_desc(3), pkg.pose_plan_desc()
    d_mask = up(np.full(n, 0x80 if all_masked else 0, np.int32)); d_ticks = ctx.alloc((n,), np.int32)
    for k in range(ticks):
        j = (k // 3) % 2
        first = k == 0
        t = float(np.float32(np.float32(k) * np.float32(0.002)))
        d_stamp.upload(np.full(n, 1 + 2 * k, np.uint32))
        if k % 2 == 1:
            d_ticks.upload(np.full(n, 0 if all_masked else k, np.int32))
            ctx.set_stage_reset(mask=d_mask, level=pkg.qrgpu.STAGE_RESET_CONSTRUCT, ticks=d_ticks, tick_dt=0.002)
        else:
            ctx.clear_stage_reset()
        ctx.ground_update_batch(n, d_gin[j], d_gst, d_gout, reset=first)
        ctx.estimator_update_batch(n, ecfg, d_x[j], d_stamp, d_est, d_eo)
        ctx.gait_update_batch(n, gcfg, t, d_ct, d_gs, d_go, d_fe, reset=first)
        ctx.walk_gait_update_batch(n, wcfg, t, d_ct, d_ws, d_wo, reset=2 if first else 0)
        ctx.swing_update_batch(n, sdesc, d_sei, d_seo, d_go, d_sst, d_sfl, gait_state=d_gs, reset=2 if first else 0)
        s = d_sti[j]
        ctx.stance_update_batch(n, tdesc, s["est_in"], s["est_out"], s["ground"], s["rpy"], s["gait_out"], s["cmd"], d_st, gait_state=s["gait_state"], vmc_in=d_vmc,
                                ratio=d_ratio, stance_out=d_sout, current_time=t, reset=first)
        p = d_pp[j]
        ctx.pose_plan_batch(n, pdesc, p["est_in"], p["est_out"], p["ground"], p["rpy"], p["walk"], d_pst, d_pcmd, d_pfl, event=1, reset=first)
        ctx.mpc_frontend_batch(n, d_fin, d_fst, d_traj, d_gait, d_cmd, d_upd)
    ctx.sync()
    ctx.clear_stage_reset()
    print("%d robots, %d ticks, bound ticks %s; finite front-end state %s, pose flags set on %d robots" % (
        n, ticks, "reset every robot" if all_masked else "reset nobody", bool(np.isfinite(d_fst.download()).all()), int((d_pfl.download() != 0).sum())))
    ctx.close()


def summarise(paths):
    """rocprofv3's kernel trace(s) -> CSV on stdout: per trace and stage kernel one row for its unbound ticks and one for its bound ticks"""
    print('"Trace","Kernel","Ticks","Calls","MedianNs","MinNs","MaxNs"')
    for path in paths:
        launches = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                m = [s for s in STAGES if ("qrgpu::" + s + "(") in row["Kernel_Name"]]
                if m:
                    launches.setdefault(m[0], []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
        tag = os.path.basename(path).replace("_kernel_trace.csv", "")
        for s in STAGES:
            in_order = [d for _, d in sorted(launches.get(s, []))]
            for ticks, d in (("unbound", in_order[0::2]), ("bound", in_order[1::2])):
                a = np.array(d or [0])
                print('"%s","%s","%s",%d,%d,%d,%d' % (tag, s, ticks, len(d), int(np.median(a)), int(a.min()), int(a.max())))


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        summarise(sys.argv[sys.argv.index("--summarise") + 1:])
    else:
        main("--all-masked" in sys.argv)
