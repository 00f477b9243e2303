"""Workload for the per-launch times of qr_swing_update_kernel / qr_swing_action_kernel: 2 000 control ticks of one mode
at 1024 robots, gait generator -> swing update -> swing action, meant to run under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o walk     -- python tools/prof_swing_modes.py walk
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o position -- python tools/prof_swing_modes.py position

--bound (after the mode) alternates the ticks between unbound calls and calls under qrgpu_set_stage_reset with an all-zero mask, so that one trace
holds the gait and swing update kernels' unbound and bound launches: each runs once a tick, so in start order its k-th launch belongs to tick k.

The walk runs the shortened cycle (0.75 s stance); the position mode uses a1_sim's gaps, whose plan is made at the first leg-0 lift-off
(the slowest update launch of the run)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg  # noqa: E402


def main(mode, n=1024, ticks=2000, bound=False):
    pkg = load_pkg()
    pkg._build.build()
    W = pkg.workload
    ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    rng = np.random.default_rng(17)
    est_in = np.zeros((54, n), np.float32); est_in[6] = 1.0
    est_in[17:29] = np.tile(np.array([0.0, 0.9, -1.8], np.float32), 4)[:, None]
    est_out = np.zeros((42, n), np.float32)
    est_out[12:24] = np.array([0.18, -0.13, -0.28, 0.18, 0.13, -0.28, -0.18, -0.13, -0.28, -0.18, 0.13, -0.28], np.float32)[:, None]
    est_out[36] = rng.uniform(-0.3, 0.3, n); est_out[38] = 0.28
    d_ei = ctx.alloc((54, n)).upload(est_in); d_eo = ctx.alloc((42, n)).upload(est_out)
    d_fl = ctx.alloc((n,), np.int32); d_out = ctx.alloc((52, n)); d_st = ctx.alloc((pkg.qrgpu.SWING_STATE_FLOATS, n))
    d_ct = ctx.alloc((4, n)).upload(np.ones((4, n), np.float32))
    ecfg = W.estimator_cfg("a1")
    if mode == "walk":
        d_gs, d_go = ctx.alloc((33, n)), ctx.alloc((41, n))
        gcfg, desc = W.walk_cfg(stance_duration=0.75), pkg.swing_mode_desc(2)
    else:
        d_gs, d_go = ctx.alloc((52, n)).upload(np.zeros((52, n), np.float32)), ctx.alloc((24, n))
        gcfg, desc = W.gait_cfg(), pkg.swing_mode_desc(1)
    if bound:
        d_mask = ctx.alloc((n,), np.int32).upload(np.zeros(n, np.int32)); d_ticks = ctx.alloc((n,), np.int32)
    for k in range(ticks):
        if bound:                                  # odd ticks: the kernels bound to an all-zero mask and the robots' own (equal) clocks
            d_ticks.upload(np.full(n, k, np.int32))    # (every tick, so that both kinds of tick start behind the same blocking copy)
            if k % 2:
                ctx.set_stage_reset(mask=d_mask, ticks=d_ticks, tick_dt=0.002)
            else:
                ctx.clear_stage_reset()
        if mode == "walk":
            ctx.walk_gait_update_batch(n, gcfg, k * 0.002, d_ct, d_gs, d_go, reset=2 if k == 0 else 0)
        else:
            ctx.gait_update_batch(n, gcfg, k * 0.002, d_ct, d_gs, d_go, reset=(k == 0))
        ctx.swing_update_batch(n, desc, d_ei, d_eo, d_go, d_st, d_fl, gait_state=d_gs, reset=2 if k == 0 else 0)
        ctx.swing_action_batch(n, desc, ecfg, d_ei, d_eo, d_go, d_st, d_out, d_fl, gait_state=d_gs)
    ctx.sync()
    st = d_st.download()
    print("%s: %d robots, %d ticks; robots with a gap plan: %d" % (mode, n, ticks, int((st[102].astype(int) & 1).sum())))
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "walk", bound="--bound" in sys.argv[2:])
