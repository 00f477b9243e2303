"""The MPC trot closed on the device, the whole queue of tools/closed_loop.py --trot: plant, observe, ground, estimator, pack, command, gait, trot inputs,
swing update, footholds, swing targets, MPC front-end, tick, MPC command -- 64 A1 robots, horizon 10, 60 ticks from the settled state, command 0.15 m/s.
Leg 0 (and its diagonal partner, leg 3) lifts off at tick 42 with the default gait, so the run crosses a lift-off, a foothold plan and several re-plans.

  * teacher-forced: after each of ticks 0, 1, 41, 42, 43 and 59 the inputs and outputs of the three new stages are downloaded, and tests/dataflow_ref.py
    applied to the device's own inputs of that tick must reproduce the outputs -- bit for bit, rows 14-25 of fe_in under 8 x the restatement's
    float32-to-float64 gap on those inputs, never under 2e-6.  Nothing is compared across ticks, so nothing diverges through the MPC.
  * structure, whatever the trot does: at tick 42 legs 0 and 3 carry {q, kp, qd, kd, 0} with the desc's gains and legs 1 and 2 {0, 0, 0, 3.0, tau} with the
    tick's d_tau; before tick 42 no motor carries a swing command; rows 41-44 of est_in are rows 8-11 of gait_out of the same tick.
No assertion on standing, speed or falls: that is the tool's report.

Measured on an MI355X (test_teacher_forced prints them): the restatement's float32-to-float64 gap on the device's inputs 1.2e-8 .. 2.7e-8 (the robots stand
near the origin) -> bar 2.0e-6; worst distance 0 at all six ticks."""
import numpy as np
import pytest

import dataflow_ref as R

pytestmark = pytest.mark.gpu

f32, f64, i32 = np.float32, np.float64, np.int32
N, H, TICKS, LIFT_OFF = 64, 10, 60, 42
CHECKED = (0, 1, 41, 42, 43, 59)
STAND_POSE = np.tile(np.array([0.0, 0.8, -1.6], f32), 4)


@pytest.fixture(scope="module")
def run(pkg):
    """The 60 ticks, once: per tick the motor command, tau, gait_out, est_in rows 41-44, the command state and memory; at the checked ticks everything the
    three stages read and wrote."""
    pkg._build.build()
    q, W, n = pkg.qrgpu, pkg.workload, N
    ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    try:
        ctx.mpc_setup_packed(0, pkg.mpc_cfg("a1"), H)
        ctx.wbc_setup_packed(0, pkg.model_desc("a1"))
        ctx.plant_body_setup(0, pkg.plant_body_desc("a1"))
        grid, field = pkg.terrain.make("flat", None)
        tdesc = pkg.terrain_desc(n_fields=1, **grid.desc())
        fb0 = np.zeros((37, n), f32); fb0[0] = 1.0; fb0[6] = 0.30; fb0[13:25] = STAND_POSE[:, None]
        cmd0 = np.zeros((60, n), f32); cmd0[0:12] = STAND_POSE[:, None]; cmd0[12:24] = 100.0; cmd0[36:48] = 2.0
        wcmd = np.zeros((67, n), f32); wcmd[2] = 0.27; wcmd[63:67] = 1.0
        odesc, ecfg, gcfg, fcfg = pkg.observe_desc("sim"), W.estimator_cfg("a1"), W.gait_cfg(), W.foothold_cfg("a1")
        cdesc, mdesc, sdesc = pkg.command_desc(), pkg.mpc_command_desc(), pkg.swing_mode_desc(q.MODE_ADVANCED_TROT, terrain=0)
        com = np.asarray(W.ROBOTS["a1"]["com_offset"], f32)
        est0 = np.zeros((54, n), f32); est0[41:45] = 1.0
        joy = np.zeros((q.JOY_ROWS, n), f32); joy[0] = 0.15; joy[6] = cdesc.body_height; joy[7] = q.RC_JOY_ADVANCED_TROT
        swing_in = np.zeros((58, n), f32); swing_in[8:12] = f32(gcfg[0]) / f32(gcfg[4]) - f32(gcfg[0])
        al = ctx.alloc
        d = dict(fb=al((37, n)).upload(fb0), cmd=al((60, n)).upload(cmd0), mpc=al((28, n)), height=al((1, grid.ny, grid.nx)).upload(pkg.terrain.stack([field])),
                 push=al((6, n)).zero(), status=al((n,), i32), traj=al((12 * H, n)).zero(), gait=al((4 * H, n)).upload(np.ones((4 * H, n), f32)),
                 wcmd=al((67, n)).upload(wcmd), prev=al((3, n)).zero(), force=al((12, n)), tick_status=al((n,), i32),
                 est_in=al((54, n)).upload(est0), obs=al((ctx.observe_state_rows(odesc), n)), rpy=al((3, n)), gin=al((23, n)), stamp=al((n,), np.uint32),
                 gst=al((13, n), f64), est_state=al((ctx.estimator_state_doubles(int(ecfg[6])), n), f64).zero(), est_out=al((42, n)).zero(),
                 mpc_est=al((28, n)), fb_est=al((37, n)), joy=al((q.JOY_ROWS, n)).upload(joy), cmd_state=al((q.CMD_STATE_ROWS, n)), state_des=al((12, n)),
                 fe_in=al((64, n)).zero(), fe_state=al((8, n)), fh_in=al((46, n)).zero(), swing_in=al((58, n)).upload(swing_in), gait_state=al((52, n)),
                 gait_out=al((24, n)), swing_state=al((q.SWING_STATE_FLOATS, n)), swing_flags=al((n,), i32), qdes=al((24, n)).zero(), tau=al((12, n)),
                 cmd_mem=al((1, n), i32), updated=al((n,), i32))

        def plant(par, **out):
            ctx.plant_step_body_batch(n, par, tdesc, d["height"], d["fb"], d["cmd"], base_push=d["push"], **out)

        settle = pkg.plant_params(dt=0.001, substeps=1)
        for _ in range(400):
            plant(settle, mpc_state=d["mpc"])
        ctx.sync()
        fb = d["fb"].download()
        fst = np.zeros((8, n), f32); fst[4:7] = fb[4:7]
        d["fe_state"].upload(fst); d["cmd"].zero()
        ctx.set_warm_start(True)
        params = pkg.plant_params(dt=0.002, substeps=2)
        log = {k: [] for k in ("motor_cmd", "tau", "gait_out", "leg_state_rows", "cmd_state", "mem")}
        full = {}
        for k in range(TICKS):
            first = k == 0
            plant(params, mpc_state=d["mpc"], status=d["status"], est_in=d["est_in"])
            ctx.observe_batch(n, odesc, d["est_in"], d["obs"], d["est_in"], d["rpy"], ground_in=d["gin"], tick=d["stamp"], est_out_prev=d["est_out"], reset=first, step=k)
            ctx.ground_update_batch(n, d["gin"], d["gst"], None, d["est_in"], reset=first)
            ctx.estimator_update_batch(n, ecfg, d["est_in"], d["stamp"], d["est_state"], d["est_out"])
            ctx.pack_state_batch(n, com, d["est_in"], d["est_out"], d["rpy"], d["mpc_est"], d["fb_est"])
            ctx.command_update(n, cdesc, d["joy"], d["cmd_state"], state_des=d["state_des"], fe_in=d["fe_in"], fh_in=d["fh_in"], reset=int(first))
            ctx.gait_update_batch(n, gcfg, float(f32(k) * f32(0.002)), d["est_in"].row(13), d["gait_state"], d["gait_out"], d["fe_in"], reset=first)
            ctx.trot_inputs(n, d["est_in"], d["est_out"], d["rpy"], d["gait_out"], gait_state=d["gait_state"], fe_in=d["fe_in"], fh_in=d["fh_in"],
                            swing_in=d["swing_in"], est_in_next=d["est_in"])
            ctx.swing_update_batch(n, sdesc, d["est_in"], d["est_out"], d["gait_out"], d["swing_state"], d["swing_flags"], gait_state=d["gait_state"],
                                   swing_in=d["swing_in"], fe_in=d["fe_in"], reset=2 if first else 0)
            ctx.footholds_batch(n, fcfg, d["fh_in"], d["swing_in"], gait_state=d["gait_state"], gait_out=d["gait_out"])
            ctx.swing_targets_batch(n, ecfg, d["swing_in"], wbc_cmd=d["wcmd"], foot_target_world=d["fe_in"].row(26), qdes=d["qdes"])
            ctx.mpc_frontend_batch(n, d["fe_in"], d["fe_state"], d["traj"], d["gait"], d["wcmd"], d["updated"])
            ctx.tick_batch(n, d["mpc_est"], d["traj"], d["gait"], d["fb_est"], d["wcmd"], d["prev"], d["force"], d["tau"], d["tick_status"])
            ctx.mpc_command(n, mdesc, d["tau"], d["qdes"], d["swing_in"], d["gait_out"], d["gait_state"], d["cmd_mem"], d["cmd"], reset=int(first))
            log["motor_cmd"].append(d["cmd"].download()); log["tau"].append(d["tau"].download()); log["gait_out"].append(d["gait_out"].download())
            log["leg_state_rows"].append(d["est_in"].download()[41:45]); log["cmd_state"].append(d["cmd_state"].download()); log["mem"].append(d["cmd_mem"].download()[0])
            if k in CHECKED:
                full[k] = {key: d[key].download() for key in ("joy", "state_des", "fe_in", "fh_in", "swing_in", "est_in", "est_out", "rpy", "gait_state", "qdes")}
        return dict(log={k: np.stack(v) for k, v in log.items()}, full=full, cdesc=dict(R.COMMAND_DESC), mdesc=dict(R.MPC_COMMAND_DESC))
    finally:
        ctx.close()


@pytest.mark.parametrize("k", CHECKED)
def test_teacher_forced(run, k):
    """The restatement on the device's own inputs of tick k reproduces the three stages' outputs of tick k."""
    log, x, n = run["log"], run["full"][k], N
    first = k == 0
    # the command stage: state before the call = the state after tick k - 1
    before = np.zeros((6, n), f32) if first else log["cmd_state"][k - 1]
    s, filt = R.command_update(run["cdesc"], x["joy"], before, reset=np.full(n, first))
    rows = R.command_rows(s)
    got = dict(cmd_state=log["cmd_state"][k], state_des=x["state_des"], fe=x["fe_in"][0:6], fh=x["fh_in"][16:21])
    want = dict(cmd_state=filt, state_des=s, fe=np.stack([rows["fe"][r] for r in range(6)]), fh=np.stack([rows["fh"][r] for r in range(16, 21)]))
    for key in got:
        assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(want[key]).tobytes(), ("command", key)
    # the data-flow stage: it does not write a row it reads, so the arrays after the tick hold its inputs
    go, gs = log["gait_out"][k], x["gait_state"]
    ti = R.trot_inputs(x["est_in"], x["est_out"], x["rpy"], go, gs)
    ti64 = R.trot_inputs(x["est_in"], x["est_out"], x["rpy"], go, gs, T=f64)
    gap = max(float(np.abs(ti["fe"][r].astype(f64) - ti64["fe"][r]).max()) for r in range(14, 26))
    bar = max(8.0 * gap, 2e-6)
    worst = 0.0
    for name, arr in (("fe", x["fe_in"]), ("fh", x["fh_in"]), ("sw", x["swing_in"]), ("ei", x["est_in"])):
        for r, v in ti[name].items():
            if name == "fe" and 14 <= r < 26:
                dist = float(np.abs(arr[r].astype(f64) - v.astype(f64)).max())
                worst = max(worst, dist)
                assert dist <= bar, (name, r, dist, bar)
            else:
                assert arr[r].tobytes() == np.ascontiguousarray(v, f32).tobytes(), ("trot inputs", name, r)
    print("tick %d: foot positions in the world frame: gap %.2e, bar %.2e, worst %.2e" % (k, gap, bar, worst))
    # the motor command: the memory before the call = the memory after tick k - 1
    mem = np.zeros(n, i32) if first else log["mem"][k - 1]
    cmd, mem_after = R.mpc_command(run["mdesc"], log["tau"][k], x["qdes"], x["swing_in"], go, gs, mem, reset=np.full(n, first))
    assert log["motor_cmd"][k].tobytes() == cmd.tobytes() and np.array_equal(log["mem"][k], mem_after)


def test_structure_of_the_lift_off(run, pkg):
    log, md = run["log"], run["mdesc"]
    cmd = log["motor_cmd"].reshape(TICKS, 5, 12, N)                       # p, Kp, d, Kd, tua
    kp, kd = np.asarray(md["kp"], f32)[:, None], np.asarray(md["kd"], f32)[:, None]
    # before the lift-off every motor carries the stance command
    early = cmd[:LIFT_OFF]
    assert np.all(early[:, 0] == 0) and np.all(early[:, 2] == 0) and np.all(early[:, 3] == f32(3.0))
    assert early[:, 4].tobytes() == log["tau"][:LIFT_OFF].tobytes() and np.all(log["mem"][:LIFT_OFF] == 0)
    # at the lift-off legs 0 and 3 swing, legs 1 and 2 stand
    at = cmd[LIFT_OFF]
    x = run["full"][LIFT_OFF]
    for leg in (0, 3):
        m = slice(3 * leg, 3 * leg + 3)
        assert at[0, m].tobytes() == x["qdes"][m].tobytes() and at[2, m].tobytes() == x["qdes"][12 + 3 * leg:15 + 3 * leg].tobytes()
        assert np.all(at[1, m] == kp[m]) and np.all(at[3, m] == kd[m]) and np.all(at[4, m] == 0)
        assert np.isfinite(at[:, m]).all()
    for leg in (1, 2):
        m = slice(3 * leg, 3 * leg + 3)
        assert np.all(at[0, m] == 0) and np.all(at[1, m] == 0) and np.all(at[2, m] == 0) and np.all(at[3, m] == f32(3.0))
        assert at[4, m].tobytes() == log["tau"][LIFT_OFF][m].tobytes()
    assert np.all(log["mem"][LIFT_OFF] == 0b1001)
    # the estimator's desiredLegState rows are this tick's gait's
    assert log["leg_state_rows"].tobytes() == np.ascontiguousarray(log["gait_out"][:, 8:12]).tobytes()
