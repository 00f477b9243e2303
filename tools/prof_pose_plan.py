"""Workload for the per-launch time of qr_pose_plan_kernel beside the unchanged kernels of a WALK tick: 200 control ticks
at 1024 robots -- walk gait -> pose plan -> swing update -> stance tick (front-end, force-balance QP, motor commands) -> swing action --
meant to run under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o all -- python tools/prof_pose_plan.py all

once per mode, each in a run of its own, with no counters:
  all   every robot replans on every tick (event 1; three stance feet, the full 20-iteration SQP)
  none  the switchToSwing rule (event 3) finds no robot: every wavefront leaves after reading its event
  host  no GPU: the float64 restatement's QuadProg++ (tests/pose_plan_ref.py) timed on this CPU, the n x 20 solves a leg switch costs
        on the host path this kernel replaces (the two copies, n x 23 floats down and n x 18 up, are not in that figure)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg  # noqa: E402
import pose_plan_ref as P  # noqa: E402
import stance_ref as R  # noqa: E402


def walk_like(n, switch):
    rng = np.random.default_rng(5)
    cases = []
    for r in range(n):
        c = P.make_case(rng, swing_leg=r % 4, offset=(rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05)))
        if not switch:
            c["cur_leg_state"] = list(c["leg_state"])
        cases.append(c)
    return cases


def host(n=1024):
    cases = walk_like(16, True)
    t, k = 0.0, 0
    for c in cases:
        r = P.update(np.float64, P.Desc(), c, P.new_state(np.float64, c["base_pos"]), record_qp=True)
        for qp in r["qps"]:
            t0 = time.perf_counter()
            P.solve_quadprog(qp["G"], qp["g0"], qp["CI"], qp["ci0"])
            t += time.perf_counter() - t0
            k += 1
    print("host: %d solves, %.1f us each; %d robots x 20 = %.1f ms per leg switch" % (k, 1e6 * t / k, n, 1e3 * n * 20 * t / k))


def main(name, n=1024, ticks=200):
    if name == "host":
        return host(n)
    pkg = load_pkg()
    pkg._build.build()
    W = pkg.workload
    ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    S = lambda a: np.ascontiguousarray(a.T)
    inp = R.make_inputs(n, R.WALK, seed=17)
    mine = P.pack_inputs(walk_like(n, name == "all"))
    inp["est_in"][:, 6:10] = mine["est_in"][:, 6:10]
    inp["est_out"][:, 12:24] = mine["est_out"][:, 12:24]; inp["est_out"][:, 36:39] = mine["est_out"][:, 36:39]
    inp["ground"][:, 6:9] = mine["ground"][:, 6:9]
    inp["rpy"][:] = mine["rpy"]
    d = {k: ctx.alloc(S(v).shape).upload(S(v)) for k, v in inp.items() if k not in ("gait_out", "gait_state")}
    d_walk = ctx.alloc((41, n)).upload(S(mine["walk"]))    # the legs the planner sees: one swinging, three in stance
    d_ct = ctx.alloc((4, n)).upload(np.ones((4, n), np.float32))
    ecfg = W.estimator_cfg("a1")
    ctx.vmc_setup_packed(0, W.vmc_cfg("a1", friction=0.6), pkg.model_desc("a1")[:3])
    d_gs, d_go, gcfg = ctx.alloc((33, n)), ctx.alloc((41, n)), W.walk_cfg(stance_duration=0.75)
    sdesc, desc, pdesc = pkg.swing_mode_desc(2), pkg.stance_desc(2), pkg.pose_plan_desc()
    d_sst = ctx.alloc((pkg.qrgpu.SWING_STATE_FLOATS, n)); d_sfl = ctx.alloc((n,), np.int32)
    d_sout = ctx.alloc((52, n)).upload(np.zeros((52, n), np.float32))
    d_st, d_vmc, d_ratio, d_out = ctx.alloc((1, n)), ctx.alloc((37, n)), ctx.alloc((8, n)), ctx.alloc((33, n))
    d_f, d_t, d_s, d_mc = ctx.alloc((12, n)), ctx.alloc((12, n)), ctx.alloc((n,), np.int32), ctx.alloc((60, n))
    d_ps = ctx.alloc((pkg.qrgpu.POSE_STATE_ROWS, n)); d_pf = ctx.alloc((n,), np.int32).upload(np.full(n, -1, np.int32))
    for k in range(ticks):
        ctx.walk_gait_update_batch(n, gcfg, k * 0.002, d_ct, d_gs, d_go, reset=2 if k == 0 else 0)
        ctx.pose_plan_batch(n, pdesc, d["est_in"], d["est_out"], d["ground"], d["rpy"], d_walk, d_ps, d["cmd"], d_pf,
                            event=1 if name == "all" else 3, reset=(k == 0))
        ctx.swing_update_batch(n, sdesc, d["est_in"], d["est_out"], d_go, d_sst, d_sfl, gait_state=d_gs, reset=2 if k == 0 else 0)
        ctx.stance_tick_batch(n, desc, d["est_in"], d["est_out"], d["ground"], d["rpy"], d_go, d["cmd"], d_st, d_vmc, d_f, d_t, d_mc,
                              ratio=d_ratio, stance_out=d_out, status=d_s, swing_q=d_sout.ptr + 24 * n * 4, swing_flag=d_sout.ptr + 48 * n * 4,
                              current_time=k * 0.002, reset=(k == 0))
        ctx.swing_action_batch(n, sdesc, ecfg, d["est_in"], d["est_out"], d_go, d_sst, d_sout, d_sfl, gait_state=d_gs)
    ctx.sync()
    fl, mc = d_pf.download(), d_mc.download()
    print("%s: %d robots, %d ticks; robots that planned %d, flag words %s, finite commands %s"
          % (name, n, ticks, int((fl != -1).sum()), sorted(set(int(v) for v in fl)), bool(np.isfinite(mc[48:]).all())))
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "all")
