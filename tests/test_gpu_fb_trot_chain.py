"""The force-balance trot closed on the device, the whole queue of tools/closed_loop.py --fb-trot: plant, observe, ground, estimator, command (JOY_TROT), gait
(the `trot` entry of the default gait table), velocity inputs, swing update (VELOCITY), swing velocity, stance tick (VELOCITY) -- 64 A1 robots on flat
terrain, 40 ticks from the settled state, command 0.15 m/s.  With the trot entry (stance 0.3 s, duty factor 0.6, leg phases 0.5, 0, 0, 0.5) leg 0 and its
diagonal partner, leg 3, lift off at tick 25: tests/gait_ref.py on the same clock says so, and test_lift_off_tick checks it.

  * teacher-forced: after each of ticks 0, 1, 24, 25, 26 and 39 the inputs and outputs of qrgpu_velocity_inputs_batch are downloaded, and
    tests/velocity_flow_ref.py applied to the device's own inputs of that tick (and the entries the tick before left) must reproduce the outputs bit for bit.
    Nothing is compared across ticks, so nothing diverges through the QP.
  * structure, whatever the trot does: before tick 25 no motor carries a swing command; at tick 25 legs 0 and 3 carry {q, kp, qd, kd, 0} with q and qd from
    rows 24-35 and 36-47 of the swing-velocity output and the desc's motor gains, legs 1 and 2 {0, 0, 0, 0, tau} with the tick's torque; rows 41-44 of
    est_in are rows 8-11 of gait_out of the same tick.
No assertion on standing, speed or falls: that is the tool's report."""
import numpy as np
import pytest

import gait_ref
import velocity_flow_ref as R

pytestmark = pytest.mark.gpu

f32, f64, i32 = np.float32, np.float64, np.int32
N, TICKS, LIFT_OFF, TERRAIN = 64, 40, 25, R.PLANE
CHECKED = (0, 1, 24, 25, 26, 39)
STAND_POSE = np.tile(np.array([0.0, 0.8, -1.6], f32), 4)
CLOCK = [float(f32(k) * f32(0.002)) for k in range(TICKS)]


@pytest.fixture(scope="module")
def run(pkg):
    """The 40 ticks, once: per tick the motor command, tau, gait_out, est_in rows 41-44, the entries and the swing flags; at the checked ticks everything the
    new stage read and wrote, and the swing-velocity output."""
    pkg._build.build()
    q, W, n = pkg.qrgpu, pkg.workload, N
    ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    try:
        ctx.mpc_setup_packed(0, pkg.mpc_cfg("a1"), 10)
        ctx.wbc_setup_packed(0, pkg.model_desc("a1"))
        ctx.plant_body_setup(0, pkg.plant_body_desc("a1"))
        ctx.vmc_setup_packed(0, W.vmc_cfg("a1"), pkg.model_desc("a1")[:3])
        grid, field = pkg.terrain.make("flat", None)
        tdesc = pkg.terrain_desc(n_fields=1, **grid.desc())
        fb0 = np.zeros((37, n), f32); fb0[0] = 1.0; fb0[6] = 0.30; fb0[13:25] = STAND_POSE[:, None]
        cmd0 = np.zeros((60, n), f32); cmd0[0:12] = STAND_POSE[:, None]; cmd0[12:24] = 100.0; cmd0[36:48] = 2.0
        odesc, ecfg = pkg.observe_desc("sim"), W.estimator_cfg("a1")
        cdesc, sdesc, stdesc = pkg.command_desc(), pkg.swing_mode_desc(q.MODE_VELOCITY, terrain=TERRAIN), pkg.stance_desc(q.MODE_VELOCITY, terrain=TERRAIN)
        gcfg = pkg.gait_table_default()[q.FSM_GAIT_TROT]
        svcfg = W.swing_velocity_cfg("a1", stance_duration=float(gcfg[0]))
        est0 = np.zeros((54, n), f32); est0[41:45] = 1.0
        joy = np.zeros((q.JOY_ROWS, n), f32); joy[0] = 0.15; joy[6] = cdesc.body_height; joy[7] = q.RC_JOY_TROT
        scmd = np.zeros((28, n), f32); scmd[9] = 0.27; scmd[15] = 0.27
        al = ctx.alloc
        d = dict(fb=al((37, n)).upload(fb0), cmd=al((60, n)).upload(cmd0), mpc=al((28, n)), height=al((1, grid.ny, grid.nx)).upload(pkg.terrain.stack([field])),
                 push=al((6, n)).zero(), status=al((n,), i32), est_in=al((54, n)).upload(est0), obs=al((ctx.observe_state_rows(odesc), n)), rpy=al((3, n)),
                 gin=al((23, n)), stamp=al((n,), np.uint32), gst=al((13, n), f64), gout=al((32, n)),
                 est_state=al((ctx.estimator_state_doubles(int(ecfg[6])), n), f64).zero(), est_out=al((42, n)).zero(), joy=al((q.JOY_ROWS, n)).upload(joy),
                 cmd_state=al((q.CMD_STATE_ROWS, n)), state_des=al((12, n)), stance_cmd=al((28, n)).upload(scmd), gait_state=al((52, n)), gait_out=al((24, n)),
                 swing_state=al((q.SWING_STATE_FLOATS, n)), swing_flags=al((n,), i32), sv=al((53, n)).zero(), sv_out=al((48, n)).zero(),
                 cmd_mem=al((1, n), i32).upload(np.full((1, n), R.MEM_POISON, i32)), swing_flag=al((4, n)).zero(), stance_state=al((q.STANCE_STATE_FLOATS, n)),
                 vmc_in=al((37, n)), ratio=al((8, n)), stance_out=al((33, n)), force=al((12, n)), tau=al((12, n)), vmc_status=al((n,), i32))

        def plant(par, **out):
            ctx.plant_step_body_batch(n, par, tdesc, d["height"], d["fb"], d["cmd"], base_push=d["push"], **out)

        settle = pkg.plant_params(dt=0.001, substeps=1)
        for _ in range(400):
            plant(settle, mpc_state=d["mpc"])
        ctx.sync()
        d["cmd"].zero()
        params = pkg.plant_params(dt=0.002, substeps=2)
        log = {k: [] for k in ("motor_cmd", "tau", "gait_out", "leg_state_rows", "mem", "flag")}
        full = {}
        for k in range(TICKS):
            first = k == 0
            plant(params, mpc_state=d["mpc"], status=d["status"], est_in=d["est_in"])
            ctx.observe_batch(n, odesc, d["est_in"], d["obs"], d["est_in"], d["rpy"], ground_in=d["gin"], tick=d["stamp"], est_out_prev=d["est_out"], reset=first, step=k)
            ctx.ground_update_batch(n, d["gin"], d["gst"], d["gout"], d["est_in"], reset=first)
            ctx.estimator_update_batch(n, ecfg, d["est_in"], d["stamp"], d["est_state"], d["est_out"])
            ctx.command_update(n, cdesc, d["joy"], d["cmd_state"], state_des=d["state_des"], stance_cmd=d["stance_cmd"], reset=int(first))
            ctx.gait_update_batch(n, gcfg, CLOCK[k], d["est_in"].row(13), d["gait_state"], d["gait_out"], reset=first)
            ctx.velocity_inputs(n, d["est_in"], d["est_out"], d["gait_out"], d["gait_state"], d["state_des"], ground_out=d["gout"], swing_vel_in=d["sv"],
                                est_in_next=d["est_in"], cmd_mem=d["cmd_mem"], swing_flag=d["swing_flag"], terrain=TERRAIN, reset=int(first))
            ctx.swing_update_batch(n, sdesc, d["est_in"], d["est_out"], d["gait_out"], d["swing_state"], d["swing_flags"], swing_vel_in=d["sv"], reset=2 if first else 0)
            ctx.swing_velocity_batch(n, ecfg, svcfg, d["sv"], d["sv_out"])
            ctx.stance_tick_batch(n, stdesc, d["est_in"], d["est_out"], d["gout"], d["rpy"], d["gait_out"], d["stance_cmd"], d["stance_state"], d["vmc_in"],
                                  d["force"], d["tau"], d["cmd"], gait_state=d["gait_state"], ratio=d["ratio"], stance_out=d["stance_out"], status=d["vmc_status"],
                                  swing_q=d["sv_out"].row(24), swing_flag=d["swing_flag"], current_time=CLOCK[k], reset=first)
            log["motor_cmd"].append(d["cmd"].download()); log["tau"].append(d["tau"].download()); log["gait_out"].append(d["gait_out"].download())
            log["leg_state_rows"].append(d["est_in"].download()[41:45]); log["mem"].append(d["cmd_mem"].download()[0]); log["flag"].append(d["swing_flag"].download())
            if k in CHECKED:
                full[k] = {key: d[key].download() for key in ("est_in", "est_out", "gout", "gait_state", "state_des", "sv", "sv_out")}
        return dict(log={k: np.stack(v) for k, v in log.items()}, full=full, kp=np.array(stdesc.motor_kp[:], f32), kd=np.array(stdesc.motor_kd[:], f32),
                    gcfg=np.array(gcfg, f32))
    finally:
        ctx.close()


def test_lift_off_tick(run):
    """The first lift-off of the trot entry on the chain's clock, from the gait restatement on the CPU: legs 0 and 3 at tick 25, inside the run."""
    out = gait_ref.run(run["gcfg"], CLOCK, np.ones((TICKS, 4)))
    swings = [k for k in range(TICKS) if (out[k, 8:12] == gait_ref.SWING).any()]
    assert swings[0] == LIFT_OFF < TICKS - 1 and out[LIFT_OFF, 8:12].tolist() == [0, 1, 1, 0]
    assert LIFT_OFF - 1 in CHECKED and LIFT_OFF in CHECKED and LIFT_OFF + 1 in CHECKED and TICKS - 1 in CHECKED and TICKS <= 80
    # the device's gait agrees on the schedule
    assert np.all(run["log"]["gait_out"][:LIFT_OFF, 8:12] == 1) and np.all(run["log"]["gait_out"][LIFT_OFF, 8:12] == np.array([0, 1, 1, 0], f32)[:, None])


@pytest.mark.parametrize("k", CHECKED)
def test_teacher_forced(run, k):
    """The restatement on the device's own inputs of tick k reproduces the new stage's outputs of tick k.  The stage does not write a row it reads, so the
    arrays after the tick hold its inputs."""
    log, x, n = run["log"], run["full"][k], N
    first = k == 0
    mem = np.full(n, R.MEM_POISON, i32) if first else log["mem"][k - 1]
    want = R.velocity_inputs(TERRAIN, x["est_in"], x["est_out"], x["gout"], log["gait_out"][k], x["gait_state"], x["state_des"], mem, np.full(n, first))
    for r, v in want["sv"].items():
        R.same_bits(x["sv"][r], np.ascontiguousarray(v, f32), tag="swing_vel_in row %d" % r)
    for r, v in want["ei"].items():
        R.same_bits(x["est_in"][r], np.ascontiguousarray(v, f32), tag="est_in row %d" % r)
    R.same_bits(log["mem"][k], want["mem"], tag="entries")
    R.same_bits(log["flag"][k], want["flag"], tag="swing flags")


def test_structure_of_the_lift_off(run):
    log = run["log"]
    cmd = log["motor_cmd"].reshape(TICKS, 5, 12, N)                       # p, Kp, d, Kd, tua
    kp, kd = run["kp"][:, None], run["kd"][:, None]
    # before the lift-off no motor carries a swing command
    early = cmd[:LIFT_OFF]
    assert np.all(early[:, 0:4] == 0) and early[:, 4].tobytes() == log["tau"][:LIFT_OFF].tobytes()
    assert np.all(log["mem"][:LIFT_OFF] == 0) and np.all(log["flag"][:LIFT_OFF] == 0)
    # at the lift-off legs 0 and 3 swing, legs 1 and 2 stand
    at, x = cmd[LIFT_OFF], run["full"][LIFT_OFF]
    for leg in (0, 3):
        m = slice(3 * leg, 3 * leg + 3)
        assert at[0, m].tobytes() == x["sv_out"][24:36][m].tobytes() and at[2, m].tobytes() == x["sv_out"][36:48][m].tobytes()
        assert np.all(at[1, m] == kp[m]) and np.all(at[3, m] == kd[m]) and np.all(at[4, m] == 0)
        assert np.isfinite(at[:, m]).all()
    for leg in (1, 2):
        m = slice(3 * leg, 3 * leg + 3)
        assert np.all(at[0:4, m] == 0) and at[4, m].tobytes() == log["tau"][LIFT_OFF][m].tobytes()
    assert np.all(log["mem"][LIFT_OFF] == 0b1001) and np.all(log["flag"][LIFT_OFF] == np.array([1, 0, 0, 1], f32)[:, None])
    # the estimator's desiredLegState rows are this tick's gait's
    assert log["leg_state_rows"].tobytes() == np.ascontiguousarray(log["gait_out"][:, 8:12]).tobytes()
