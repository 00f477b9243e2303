"""Workload for the per-launch times of qr_stance_update_kernel / qr_stance_command_kernel: 2 000 force-balance control
ticks of one mode at 1024 robots -- gait generator -> swing update -> stance tick (front-end, force-balance QP, motor commands) -> swing
action for the walk and position modes -- meant to run under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o walk -- python tools/prof_stance.py walk

once per mode (velocity, position, walk, advanced_trot), each in a run of its own.  --bound (after the mode) alternates the ticks between unbound
calls and calls under qrgpu_set_stage_reset with an all-zero mask: one trace then holds the unbound and the bound launches of the gait, swing update and
stance update kernels: each runs once a tick, so in start order its k-th launch belongs to tick k."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg  # noqa: E402
import stance_ref as R  # noqa: E402

MODES = {"velocity": 0, "position": 1, "walk": 2, "advanced_trot": 3}


def main(name, n=1024, ticks=2000, bound=False):
    mode = MODES[name]
    pkg = load_pkg()
    pkg._build.build()
    W = pkg.workload
    ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    S = lambda a: np.ascontiguousarray(a.T)
    inp = R.make_inputs(n, mode, seed=17)                  # attitudes, control frames and commands of the parity tests
    d = {k: ctx.alloc(S(v).shape).upload(S(v)) for k, v in inp.items() if k not in ("gait_out", "gait_state")}
    d_ct = ctx.alloc((4, n)).upload(np.ones((4, n), np.float32))
    ecfg = W.estimator_cfg("a1")
    ctx.vmc_setup_packed(0, W.vmc_cfg("a1", friction=0.6 if mode == 2 else 0.5), pkg.model_desc("a1")[:3])
    if mode == 2:
        d_gs, d_go, gcfg = ctx.alloc((33, n)), ctx.alloc((41, n)), W.walk_cfg(stance_duration=0.75)
    else:
        d_gs, d_go, gcfg = ctx.alloc((52, n)).upload(np.zeros((52, n), np.float32)), ctx.alloc((24, n)), W.gait_cfg()
    sdesc, desc = pkg.swing_mode_desc(mode), pkg.stance_desc(mode)
    d_sst = ctx.alloc((pkg.qrgpu.SWING_STATE_FLOATS, n)); d_sfl = ctx.alloc((n,), np.int32)
    d_sout = ctx.alloc((52, n)).upload(np.zeros((52, n), np.float32))
    d_st, d_vmc, d_ratio, d_out = ctx.alloc((1, n)), ctx.alloc((37, n)), ctx.alloc((8, n)), ctx.alloc((33, n))
    d_f, d_t, d_s, d_mc = ctx.alloc((12, n)), ctx.alloc((12, n)), ctx.alloc((n,), np.int32), ctx.alloc((60, n))
    acts = mode in (1, 2)
    if bound:
        d_mask = ctx.alloc((n,), np.int32).upload(np.zeros(n, np.int32)); d_ticks = ctx.alloc((n,), np.int32)
    for k in range(ticks):
        if bound:                                  # odd ticks: the kernels bound to an all-zero mask and the robots' own (equal) clocks
            d_ticks.upload(np.full(n, k, np.int32))    # (every tick, so that both kinds of tick start behind the same blocking copy)
            if k % 2:
                ctx.set_stage_reset(mask=d_mask, ticks=d_ticks, tick_dt=0.002)
            else:
                ctx.clear_stage_reset()
        if mode == 2:
            ctx.walk_gait_update_batch(n, gcfg, k * 0.002, d_ct, d_gs, d_go, reset=2 if k == 0 else 0)
        else:
            ctx.gait_update_batch(n, gcfg, k * 0.002, d_ct, d_gs, d_go, reset=(k == 0))
        ctx.swing_update_batch(n, sdesc, d["est_in"], d["est_out"], d_go, d_sst, d_sfl, gait_state=d_gs, reset=2 if k == 0 else 0)
        ctx.stance_tick_batch(n, desc, d["est_in"], d["est_out"], d["ground"], d["rpy"], d_go, d["cmd"], d_st, d_vmc, d_f, d_t, d_mc,
                              gait_state=None if mode == 2 else d_gs, ratio=d_ratio, stance_out=d_out, status=d_s,
                              swing_q=d_sout.ptr + 24 * n * 4 if acts else None, swing_flag=d_sout.ptr + 48 * n * 4 if acts else None,
                              current_time=k * 0.002, reset=(k == 0))
        if acts:
            ctx.swing_action_batch(n, sdesc, ecfg, d["est_in"], d["est_out"], d_go, d_sst, d_sout, d_sfl, gait_state=d_gs)
    ctx.sync()
    out, mc = d_out.download(), d_mc.download()
    print("%s: %d robots, %d ticks; mean N %.2f, finite commands %s" % (name, n, ticks, float(out[30].mean()), bool(np.isfinite(mc[48:]).all())))
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "walk", bound="--bound" in sys.argv[2:])
