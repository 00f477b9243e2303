"""-m gpu: a robot does not depend on its neighbours' modes.  The full two-chain tick of tools/closed_loop.py --fsm-mode without the state machine --
stage clock and binding, qrgpu_mode_route_batch, qrgpu_set_mode_route, observe, ground, estimator, pack, command update (the rows of both chains), gait
select, the MPC chain up to qrgpu_mpc_command_batch, the force-balance chain up to qrgpu_stance_tick_batch, qrgpu_mode_command_batch -- on 70 A1 robots,
horizon 10, 50 ticks, which cross the first lift-off of the `trot` entry (tick 25) and of `advanced_trot` (tick 42).

Teacher-forced: one closed run (plant in the loop, everybody on the MPC chain) records the sensor rows the plant writes per tick; every compared run
reads those rows instead of a plant's, so no run's commands feed back and the only thing that differs between the runs is who is on which chain.
Every robot runs the gait of its own mode (`trot` where the mode is VELOCITY) in every run; the front-end's counter starts at 50 + r % 12, so robots
on the MPC chain are solved on some ticks and held (the cadence kernel and the WBC) on the others; every solve starts cold (gpu_helpers.cold_start).

  * the mixed batch: modes -1, ADVANCED_TROT, VELOCITY by r % 3.  For every robot and every tick the merged motor command and status word equal,
    bit for bit, those of the same robot in the batch of the same n where EVERY robot is on that robot's chain; a robot on no chain gets zeros.
  * a robot whose mode changes at tick 20, with its QRGPU_FSM_ENTERED bit in the stage mask of that tick (one from the MPC chain to the force-balance
    chain, one the other way): before tick 20 it equals its robot of the uniform batch of the old chain, from tick 20 on its robot of the uniform batch
    of the new chain given the same reset at tick 20.  MPC-side memory that no stage reset touches (d_hold, d_prev_ori) does not show here: the
    front-end's reset makes the 50 ticks that follow due ones, so d_hold is rewritten before it is read and the WBC, which alone reads d_prev_ori, first
    runs again 50 ticks later -- on what the robot's last WBC pass left, as in the reference, whose wbcController is made once and never reset
    (include/qrgpu.h)."""
import numpy as np
import pytest

import mode_route_ref as R

pytestmark = pytest.mark.gpu

f32, f64, i32 = np.float32, np.float64, np.int32
N, H, TICKS, SWITCH, PERIOD = 70, 10, 50, 20, 12
TO_FB, TO_MPC = 4, 8                        # 4 % 3 == 1: on the MPC chain until the switch; 8 % 3 == 2: on the force-balance chain until the switch
STAND_POSE = np.tile(np.array([0.0, 0.8, -1.6], f32), 4)
CLOCK = [float(f32(k) * f32(0.002)) for k in range(TICKS)]


def modes_of(kind, t):
    """mode_sel [n] float32 of a run at tick t."""
    r = np.arange(N)
    if kind == "mpc":
        return np.full(N, 3, f32)
    if kind == "fb":
        return np.full(N, 0, f32)
    m = np.where(r % 3 == 0, -1, np.where(r % 3 == 1, 3, 0)).astype(f32)
    if t >= SWITCH:
        m[TO_FB], m[TO_MPC] = 0, 3
    return m


@pytest.fixture(scope="module")
def runs(pkg):
    pkg._build.build()
    q, W, n = pkg.qrgpu, pkg.workload, N
    ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    try:
        ctx.mpc_setup_packed(0, pkg.mpc_cfg("a1"), H)
        ctx.wbc_setup_packed(0, pkg.model_desc("a1"))
        ctx.plant_body_setup(0, pkg.plant_body_desc("a1"))
        ctx.vmc_setup_packed(0, W.vmc_cfg("a1"), pkg.model_desc("a1")[:3])
        ctx.set_warm_start(False); ctx.set_planned_list(False)
        ctx.set_torque_epilogue(hip_comp=True, clip=True)
        grid, field = pkg.terrain.make("flat", None)
        tdesc = pkg.terrain_desc(n_fields=1, **grid.desc())
        odesc, ecfg, fcfg = pkg.observe_desc("sim"), W.estimator_cfg("a1"), W.foothold_cfg("a1")
        com = np.asarray(W.ROBOTS["a1"]["com_offset"], f32)
        cdesc, mdesc, rdesc = pkg.command_desc(), pkg.mpc_command_desc(), pkg.mode_route_desc()
        sdesc, fb_sdesc, stdesc = pkg.swing_mode_desc(q.MODE_ADVANCED_TROT, terrain=0), pkg.swing_mode_desc(q.MODE_VELOCITY, terrain=0), pkg.stance_desc(q.MODE_VELOCITY, terrain=0)
        gtable = W.gait_table()
        svcfg = W.swing_velocity_cfg("a1", stance_duration=float(pkg.gait_table_default()[q.FSM_GAIT_TROT][0]))
        al = ctx.alloc
        rawlog = al((TICKS, 41, n))
        height = al((1, grid.ny, grid.nx)).upload(pkg.terrain.stack([field]))
        fb0 = np.zeros((37, n), f32); fb0[0] = 1.0; fb0[6] = 0.30; fb0[13:25] = STAND_POSE[:, None]
        cmd0 = np.zeros((60, n), f32); cmd0[0:12] = STAND_POSE[:, None]; cmd0[12:24] = 100.0; cmd0[36:48] = 2.0
        d_fb, d_pcmd, d_push, d_mpc = al((37, n)).upload(fb0), al((60, n)).upload(cmd0), al((6, n)).zero(), al((28, n))
        settle = pkg.plant_params(dt=0.001, substeps=1)
        for _ in range(400):
            ctx.plant_step_body_batch(n, settle, tdesc, height, d_fb, d_pcmd, base_push=d_push, mpc_state=d_mpc)
        ctx.sync()
        fb_settled = d_fb.download()
        params = pkg.plant_params(dt=0.002, substeps=2)

        def run(kind, closed=False):
            """One run from the settled state; kind: "mpc", "fb" (uniform) or "mixed".  -> motor_cmd [T][60][n], status [T][n], chain [T][n], due [T][n]."""
            wcmd = np.zeros((67, n), f32); wcmd[2] = 0.27; wcmd[63:67] = 1.0
            est0 = np.zeros((54, n), f32); est0[41:45] = 1.0
            joy = np.zeros((q.JOY_ROWS, n), f32); joy[0] = 0.15; joy[6] = cdesc.body_height
            scmd = np.zeros((28, n), f32); scmd[9] = 0.27; scmd[15] = 0.27
            fst = np.zeros((8, n), f32); fst[4:7] = fb_settled[4:7]; fst[7] = 50 + np.arange(n) % PERIOD
            d = dict(traj=al((12 * H, n)).zero(), gait=al((4 * H, n)).upload(np.ones((4 * H, n), f32)), wcmd=al((67, n)).upload(wcmd), prev=al((3, n)).zero(),
                     force=al((12, n)).zero(), hold=al((12, n)).zero(), tau=al((12, n)).zero(), mpc_status=al((n,), i32).zero(), qdes=al((24, n)).zero(),
                     est_in=al((54, n)).upload(est0), obs=al((ctx.observe_state_rows(odesc), n)), rpy=al((3, n)), gin=al((23, n)), stamp=al((n,), np.uint32),
                     gst=al((13, n), f64), gout=al((32, n)), est_state=al((ctx.estimator_state_doubles(int(ecfg[6])), n), f64).zero(), est_out=al((42, n)).zero(),
                     mpc_est=al((28, n)), fb_est=al((37, n)), joy=al((q.JOY_ROWS, n)), cmd_state=al((q.CMD_STATE_ROWS, n)), state_des=al((12, n)),
                     fe_in=al((64, n)).zero(), fe_state=al((8, n)).upload(fst), fh_in=al((46, n)).zero(), swing_in=al((58, n)).zero(), gait_state=al((52, n)),
                     gait_out=al((24, n)), gait_sel=al((n,)), gait_flags=al((n,), i32), swing_state=al((q.SWING_STATE_FLOATS, n)), swing_flags=al((n,), i32),
                     cmd_mem=al((1, n), i32).zero(), updated=al((n,), i32), cmd_mpc=al((60, n)).zero(),
                     stance_cmd=al((28, n)).upload(scmd), fb_swing_state=al((q.SWING_STATE_FLOATS, n)), fb_swing_flags=al((n,), i32), sv=al((53, n)).zero(),
                     sv_out=al((48, n)).zero(), fb_cmd_mem=al((1, n), i32).zero(), swing_flag=al((4, n)).zero(), stance_state=al((q.STANCE_STATE_FLOATS, n)),
                     vmc_in=al((37, n)), ratio=al((8, n)), stance_out=al((33, n)), fb_force=al((12, n)).zero(), fb_tau=al((12, n)).zero(), fb_status=al((n,), i32).zero(),
                     cmd_fb=al((60, n)).zero(), mode_sel=al((n,)), chain=al((n,), i32), route_flags=al((n,), i32), count=al((3,), i32), mask=al((n,), i32),
                     ticks=al((n,), i32), origin=al((n,), i32).zero(), local=al((n,), i32), cmd=al((60, n)), status=al((n,), i32))
            if closed:
                d_fb.upload(fb_settled); d_pcmd.zero()
            log = {k: [] for k in ("cmd", "status", "chain", "due", "count", "flags")}
            try:
                for k in range(TICKS):
                    first = k == 0
                    modes = modes_of(kind, k)
                    # what the state machine would hand the tick: the mode and the gait OnEnter latched, the joystick rows, QRGPU_FSM_ENTERED at the switch
                    mask = np.zeros(n, i32)
                    if k == SWITCH:
                        mask[[TO_FB, TO_MPC]] = q.FSM_ENTERED
                    trot = modes == q.MODE_VELOCITY
                    joy[7] = np.where(trot, q.RC_JOY_TROT, q.RC_JOY_ADVANCED_TROT)
                    d["mode_sel"].upload(modes); d["gait_sel"].upload(np.where(trot, q.FSM_GAIT_TROT, q.FSM_GAIT_ADVANCED_TROT).astype(f32))
                    d["mask"].upload(mask); d["ticks"].upload(np.full(n, k, i32)); d["joy"].upload(joy)
                    ctx.stage_clock(n, d["mask"], q.FSM_ENTERED, d["ticks"], d["origin"], d["local"])
                    ctx.set_stage_reset(mask=d["mask"], bits=q.FSM_ENTERED, ticks=d["local"])
                    ctx.mode_route(n, rdesc, d["mode_sel"], d["chain"], route_flags=d["route_flags"], chain_count=d["count"])
                    ctx.set_mode_route(d["chain"])
                    if closed:
                        ctx.plant_step_body_batch(n, params, tdesc, height, d_fb, d_pcmd, base_push=d_push, mpc_state=d_mpc, est_in=d["est_in"])
                        ctx.copy_rows(rawlog.row(k), d["est_in"], 41 * n)
                    ctx.observe_batch(n, odesc, rawlog.row(k), d["obs"], d["est_in"], d["rpy"], ground_in=d["gin"], tick=d["stamp"], est_out_prev=d["est_out"],
                                      reset=first, step=k)
                    ctx.ground_update_batch(n, d["gin"], d["gst"], d["gout"], d["est_in"], reset=first)
                    ctx.estimator_update_batch(n, ecfg, d["est_in"], d["stamp"], d["est_state"], d["est_out"])
                    ctx.pack_state_batch(n, com, d["est_in"], d["est_out"], d["rpy"], d["mpc_est"], d["fb_est"])
                    ctx.command_update(n, cdesc, d["joy"], d["cmd_state"], state_des=d["state_des"], fe_in=d["fe_in"], fh_in=d["fh_in"], stance_cmd=d["stance_cmd"],
                                       reset=int(first))
                    ctx.gait_select_update_batch(n, gtable, d["gait_sel"], CLOCK[k], d["est_in"].row(13), d["gait_state"], d["gait_out"], d["fe_in"],
                                                 swing_in=d["swing_in"], flags=d["gait_flags"], reset=int(first))
                    # the MPC chain, into its own arrays
                    ctx.trot_inputs(n, d["est_in"], d["est_out"], d["rpy"], d["gait_out"], gait_state=d["gait_state"], fe_in=d["fe_in"], fh_in=d["fh_in"],
                                    swing_in=d["swing_in"], est_in_next=d["est_in"])
                    ctx.swing_update_batch(n, sdesc, d["est_in"], d["est_out"], d["gait_out"], d["swing_state"], d["swing_flags"], gait_state=d["gait_state"],
                                           swing_in=d["swing_in"], fe_in=d["fe_in"], reset=2 if first else 0)
                    ctx.footholds_batch(n, fcfg, d["fh_in"], d["swing_in"], gait_state=d["gait_state"], gait_out=d["gait_out"])
                    ctx.swing_targets_batch(n, ecfg, d["swing_in"], wbc_cmd=d["wcmd"], foot_target_world=d["fe_in"].row(26), qdes=d["qdes"])
                    ctx.mpc_frontend_batch(n, d["fe_in"], d["fe_state"], d["traj"], d["gait"], d["wcmd"], d["updated"])
                    ctx.tick_cadence_batch(n, d["updated"], d["mpc_est"], d["traj"], d["gait"], d["fb_est"], d["wcmd"], d["prev"], d["force"], d["hold"], d["tau"],
                                           d["mpc_status"])
                    ctx.mpc_command(n, mdesc, d["tau"], d["qdes"], d["swing_in"], d["gait_out"], d["gait_state"], d["cmd_mem"], d["cmd_mpc"], reset=int(first))
                    # the force-balance chain, into its own arrays
                    ctx.velocity_inputs(n, d["est_in"], d["est_out"], d["gait_out"], d["gait_state"], d["state_des"], ground_out=d["gout"], swing_vel_in=d["sv"],
                                        est_in_next=d["est_in"], cmd_mem=d["fb_cmd_mem"], swing_flag=d["swing_flag"], terrain=0, reset=int(first))
                    ctx.swing_update_batch(n, fb_sdesc, d["est_in"], d["est_out"], d["gait_out"], d["fb_swing_state"], d["fb_swing_flags"], swing_vel_in=d["sv"],
                                           reset=2 if first else 0)
                    ctx.swing_velocity_batch(n, ecfg, svcfg, d["sv"], d["sv_out"])
                    ctx.stance_tick_batch(n, stdesc, d["est_in"], d["est_out"], d["gout"], d["rpy"], d["gait_out"], d["stance_cmd"], d["stance_state"], d["vmc_in"],
                                          d["fb_force"], d["fb_tau"], d["cmd_fb"], gait_state=d["gait_state"], ratio=d["ratio"], stance_out=d["stance_out"],
                                          status=d["fb_status"], swing_q=d["sv_out"].row(24), swing_flag=d["swing_flag"], current_time=CLOCK[k], reset=first)
                    ctx.mode_command(n, d["chain"], d["cmd_mpc"], d["cmd_fb"], d["cmd"], status_mpc=d["mpc_status"], status_fb=d["fb_status"], status=d["status"])
                    if closed:
                        ctx.copy_rows(d_pcmd, d["cmd"], 60 * n)
                    ctx.sync()
                    for key, src in (("cmd", "cmd"), ("status", "status"), ("chain", "chain"), ("due", "updated"), ("count", "count"), ("flags", "route_flags")):
                        log[key].append(d[src].download())
            finally:
                ctx.clear_mode_route(); ctx.clear_stage_reset()
                for v in d.values():
                    v.free()
            return {k: np.stack(v) for k, v in log.items()}

        run("mpc", closed=True)                                    # the recording: its own results are not compared
        return {kind: run(kind) for kind in ("mixed", "mpc", "fb")}
    finally:
        ctx.close()


def words(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_route_of_every_run(runs):
    for kind in ("mixed", "mpc", "fb"):
        for k in range(TICKS):
            chain, flags, count = R.route(modes_of(kind, k))
            assert np.array_equal(runs[kind]["chain"][k], chain) and np.array_equal(runs[kind]["flags"][k], flags) and np.array_equal(runs[kind]["count"][k], count), (kind, k)
    assert set(np.unique(runs["mixed"]["chain"])) == {0, 1, 2}


def test_every_robot_equals_its_robot_of_the_uniform_batch(runs):
    mixed = runs["mixed"]
    for k in range(TICKS):
        chain = mixed["chain"][k]
        for c, kind in ((R.CHAIN_MPC, "mpc"), (R.CHAIN_FORCE_BALANCE, "fb")):
            on = chain == c
            bad = np.nonzero((words(mixed["cmd"][k][:, on]) != words(runs[kind]["cmd"][k][:, on])).any(0))[0]
            assert bad.size == 0, ("tick", k, kind, "robots", np.nonzero(on)[0][bad].tolist())
            assert np.array_equal(mixed["status"][k][on], runs[kind]["status"][k][on]), (k, kind)
        idle = chain == R.CHAIN_NONE
        assert idle.any() and not words(mixed["cmd"][k][:, idle]).any() and not mixed["status"][k][idle].any(), k


def test_a_robot_that_changes_chains(runs):
    mixed = runs["mixed"]
    for robot, old, new in ((TO_FB, "mpc", "fb"), (TO_MPC, "fb", "mpc")):
        assert np.all(mixed["chain"][:SWITCH, robot] == (1 if old == "mpc" else 2)) and np.all(mixed["chain"][SWITCH:, robot] == (1 if new == "mpc" else 2))
        for k in range(TICKS):
            ref = runs[old if k < SWITCH else new]
            assert np.array_equal(words(mixed["cmd"][k][:, robot]), words(ref["cmd"][k][:, robot])), (robot, k)
            assert mixed["status"][k][robot] == ref["status"][k][robot], (robot, k)
    # the front-end's reset at the switch: every tick that follows in the run is a due one for the robot that entered the MPC chain
    assert np.all(mixed["due"][SWITCH:, TO_MPC] != 0) and np.all(runs["mpc"]["due"][SWITCH:, TO_MPC] != 0)


def test_the_runs_are_not_vacuous(runs):
    """Both chains cross a lift-off; robots on the MPC chain are solved on some ticks and held on others; the two chains command different things."""
    mixed = runs["mixed"]
    cmd = mixed["cmd"].reshape(TICKS, 5, 12, N)                                # p, Kp, d, Kd, tua
    on_mpc, on_fb = mixed["chain"] == R.CHAIN_MPC, mixed["chain"] == R.CHAIN_FORCE_BALANCE
    swing = (cmd[:, 1] != 0).any(1)                                            # [tick][robot]: some motor carries a position gain
    assert (swing & on_fb).any() and (swing & on_mpc).any() and not (swing & on_fb)[:20].any()
    due = mixed["due"] != 0
    plain = np.ones(N, bool); plain[[TO_FB, TO_MPC]] = False
    m = on_mpc & plain[None, :]
    assert (due & m).any() and (~due & m).any()
    r_mpc, r_fb = 1, 2
    assert not np.array_equal(words(runs["mpc"]["cmd"][:, :, r_fb]), words(runs["fb"]["cmd"][:, :, r_fb]))
    assert not np.array_equal(words(runs["mpc"]["cmd"][:, :, r_mpc]), words(runs["fb"]["cmd"][:, :, r_mpc]))
