"""A robot's life cycle on the device with no host decision: episode step, body plant, qrgpu_fsm_update_batch, qrgpu_fsm_command_batch, 16 robots, 150
ticks, short durations (time_step 0.1: a stand-up of 30 ticks; transition_ticks 8).  The robots spawn sitting; a device script keyed on each robot's
episode tick presses X (to JOY_STAND) and X again with a velocity on the axes (to JOY_ADVANCED_TROT).  No locomotion chain runs: the command array is
its own locomotion column, so a robot in locomotion keeps the command it has.

  * every tick the device's est_in (the plant's contacts and joint angles), the episode words and the command column are read back and fed to
    tests/fsm_ref.py: the device's plan, command, state column, joy rows and stage mask are the restatement's, bit for bit.
  * a robot forced to respawn in mid-run starts its stand-up again from its spawn angles, and its bit is in d_stage_mask.
Base heights at the end are printed, not asserted."""
import numpy as np
import pytest

import fsm_ref as R

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
N, T, FORCED, FORCED_AT = 16, 150, 3, 70
SCRIPT = np.array([[36, R.BTN_X, 0.0, 0.0, 0.0], [52, R.BTN_X, 0.0, 0.0, 1.0]], f32).T.copy()
D = dict(R.A1, time_step=0.1, transition_ticks=8)


def test_life_cycle_against_fsm_ref(gpu_ctx, pkg):
    ctx, q, n = gpu_ctx, pkg.qrgpu, N
    ctx.wbc_setup_packed(0, pkg.model_desc("a1"))
    ctx.plant_body_setup(0, pkg.plant_body_desc("a1"))
    grid, field = pkg.terrain.make("flat", None)
    tdesc = pkg.terrain_desc(n_fields=1, **grid.desc())
    fdesc = pkg.fsm_desc(**D)
    sit = np.asarray(D["sit_down_angles"], f32)
    # an episode ends by the forced reset alone: a sitting robot rests on its trunk
    edesc = pkg.episode_desc(status_mask=0, tilt_max=4.0, min_clearance=0.0, spawn_height=0.14, q_spawn=list(sit), seed=3, q_jitter=0.02)
    params = pkg.plant_params(dt=0.002, substeps=2)
    cx, cy = grid.x0 + 0.5 * (grid.nx - 1) * grid.cell, grid.y0 + 0.5 * (grid.ny - 1) * grid.cell
    table = np.zeros((4, 1), f32); table[0] = cx; table[1] = cy
    d = dict(fb=ctx.alloc((37, n)).zero(), cmd=ctx.alloc((60, n)).zero(), est_in=ctx.alloc((54, n)).zero(), height=ctx.alloc((1, grid.ny, grid.nx)).upload(pkg.terrain.stack([field])),
             table=ctx.alloc((4, 1)).upload(table), ep_state=ctx.alloc((q.EPISODE_STATE_ROWS, n), i32).zero(), ep_stats=ctx.alloc((q.EPISODE_STATS_ROWS, n)).zero(),
             done=ctx.alloc((n,), i32), force=ctx.alloc((n,), i32).zero(), prev=ctx.alloc((3, n)).zero(), status=ctx.alloc((n,), i32),
             state=ctx.alloc((q.FSM_STATE_ROWS, n)).upload(np.full((q.FSM_STATE_ROWS, n), R.POISON, f32)), joy=ctx.alloc((q.JOY_ROWS, n)), plan=ctx.alloc((n,), i32),
             mask=ctx.alloc((n,), i32), out=ctx.alloc((q.FSM_OUT_ROWS, n)), script=ctx.alloc(SCRIPT.shape).upload(SCRIPT))
    robots = [None] * n
    seen = set()
    try:
        for t in range(T):
            force = np.zeros(n, i32); force[FORCED] = int(t == FORCED_AT)
            d["force"].upload(force)
            ctx.episode_step_batch(n, edesc, d["fb"], d["table"], 1, d["ep_state"], d["ep_stats"], d["done"], reset_all=(t == 0), params=params, terrain=tdesc,
                                   height=d["height"], force_reset=d["force"], prev_ori=d["prev"], motor_cmd=d["cmd"])
            ctx.plant_step_body_batch(n, params, tdesc, d["height"], d["fb"], d["cmd"], est_in=d["est_in"], status=d["status"])
            loco = d["cmd"].download()
            ctx.fsm_update(n, fdesc, d["state"], d["joy"], d["plan"], stage_mask=d["mask"], script=d["script"], n_script=SCRIPT.shape[1], ticks=d["ep_state"],
                           done=d["done"], bits=q.EP_REASONS)
            ctx.fsm_command(n, fdesc, d["plan"], d["est_in"], d["cmd"], d["state"], d["cmd"], fsm_out=d["out"])
            est, done, ticks = d["est_in"].download(), d["done"].download(), d["ep_state"].download()[0]
            got = dict(plan=d["plan"].download(), cmd=d["cmd"].download(), state=d["state"].download(), joy=d["joy"].download(), mask=d["mask"].download(),
                       out=d["out"].download())
            assert (done[FORCED] & q.EP_REASONS != 0) == (t in (0, FORCED_AT)) and np.isfinite(est[13:29]).all()
            for r in range(n):
                rst = (done[r] & q.EP_REASONS) != 0
                if rst:
                    robots[r] = R.Robot(D)
                o = robots[r].tick(R.script_message(SCRIPT, ticks[r]), False, est[13:17, r], est[17:29, r], loco[:, r])
                want_mask = (done[r] & q.EP_REASONS) | (R.ENTERED if o["entered"] else 0)
                assert got["plan"][r] == o["plan"] and got["mask"][r] == want_mask, (t, r, got["plan"][r], o["plan"], got["mask"][r], want_mask)
                for k, want in (("cmd", o["cmd"]), ("state", robots[r].state_rows()), ("joy", o["joy"]), ("out", o["out"])):
                    assert np.array_equal(got[k][:, r].view(np.uint32), want.view(np.uint32)), (t, r, k)
                seen.add(o["plan"] & 0x7f)
            if t == FORCED_AT:      # the respawned robot starts its stand-up again, from the angles the plant reports of its spawn pose
                r = FORCED
                assert got["plan"][r] == (R.ACTION | R.ACTION_FIRST) and got["mask"][r] & q.EP_FORCED and got["out"][0, r] == R.STAND_UP
                assert np.array_equal(got["state"][31:43, r], est[17:29, r]) and np.abs(est[17:29, r] - sit).max() < 0.2
                assert got["out"][0, 0] == R.LOCOMOTION and got["plan"][0] & (R.RUN | R.PHASE1 | R.PHASE2 | R.REPEAT)      # the others are where the script took them
        assert seen >= {R.ACTION, R.HOLD, R.REPEAT, R.PHASE1, R.PHASE2, R.RUN}, seen
        fb = d["fb"].download()
        print("base heights at the end: min %.3f mean %.3f max %.3f; the respawned robot %.3f" % (fb[6].min(), fb[6].mean(), fb[6].max(), fb[6, FORCED]))
    finally:
        for v in d.values():
            v.free()
