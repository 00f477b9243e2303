#!/usr/bin/env python3
"""n simulated A1 robots in closed loop on one GPU: plant -> truth mpc_state -> qrgpu_tick_batch -> plant, tick after tick, with no host copy
inside the loop.

  python tools/closed_loop.py [--robots 1024] [--ticks 500] [--substeps 2]            prints ONE JSON line
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/closed_loop.py --profile    the same loop as the workload of a kernel trace
  python tools/closed_loop.py --terrain plane:0.2 [--push 30]                         the same loop on a height field, with a push on the base
  python tools/closed_loop.py --body [--terrain stairs:0.04] [--push 30]              the same loop with knee and trunk contact and joint limits
  python tools/closed_loop.py --episodes [--max-ticks 400] [--terrain plane:0.2]      episode step -> plant -> tick: robots that fall start again
  python tools/closed_loop.py --estimator [--sensor-noise 0.02]                       the tick reads the estimator chain's state, not the plant's truth
  python tools/closed_loop.py --trot [--cmd-vx 0.15] [--cmd-yaw 0.1] [--episodes] [--terrain ...]   the MPC trot, every stage on the device
  python tools/closed_loop.py --trot --cadence [...]                                  the same with the tick on the reference's cadence: MPC or WBC per robot
  python tools/closed_loop.py --fsm [--ticks 3000] [--cmd-vx 0.15] [--fsm-speed 1]    a robot's whole life cycle: sit, stand up, MPC standing, trot, fall, again
  python tools/closed_loop.py --fsm --fsm-gait [...]                                  the same with every robot on the gait its state machine chose
  python tools/closed_loop.py --fsm-mode [--fsm-trot-every 3] [...]                   the same with every robot's solve in the chain its state machine chose
  python tools/closed_loop.py --fb-trot [--cmd-vx 0.15] [--cmd-yaw 0.1] [--episodes] [--terrain ...]   the force-balance trot, every stage on the device

The robots are dropped from z = 0.30 onto joint PD at the stand pose (400 ticks of 1 ms), shoved by up to 0.3 m/s in x and y, and handed to
MPC + WBC: qrgpu_plant_step_batch (include/qrgpu.h) writes the ground-truth mpc_state and fb_state the tick reads, and the tick -- the plain
one: pipelined, consecutive ticks not overlapped -- writes its torque straight into rows 48-59 of the motor command the plant reads.  All-stance
gait, a trajectory and a WBC command that hold the origin at height 0.27, warm start on.

--terrain KIND[:ARG] (flat, plane:SLOPE_X, stairs:HEIGHT, gap:WIDTH, rough:AMPLITUDE; quadruped-robot_amd/terrain.py) runs the settle phase and
the loop through qrgpu_plant_step_terrain_batch on that field; on a plane the robots start aligned with the slope (a level robot dropped onto
a slope of 0.2 tips over backwards).  --push N holds a world-frame force of N newtons along +x on every base during the timed loop.  The
controller's trajectory and command stay the level ones: what it makes of a pitched ground is reported, not judged.  Without either option
the run is the flat one.  --body runs the settle phase and the loop through qrgpu_plant_step_body_batch (on the flat field unless --terrain names
another): a robot that loses its footing comes to rest on knees and trunk instead of sinking through the ground, and is counted.

--episodes (implies --body) puts qrgpu_episode_step_batch in front of every plant step of the loop, warm-up included: a robot whose trunk touches
the ground, that tilts beyond 1 rad, sinks under 0.10 m of clearance, leaves the field (margin 0.2 m) or -- with --max-ticks N -- has run N ticks is
spawned again on the device at spawn height 0.30 on a 3 x 3 grid of points around the field's centre (--spawn-spread, default 0.05 m between
points: the controller's command holds the origin, so a wide grid would measure the WBC's position task, not the episode layer), aligned with the
slope on a plane, with the run's shove as its spawn velocity, on the joint PD hold the call writes (the tick's torque is added to it, as the motor law
adds them).  Episode 0 is the settled, shoved state of the other runs: nothing is spawned before the first fall.  Without the option the tool runs
exactly what it ran.

--estimator closes the loop from the sensors: [episode step,] plant (which writes its sensor rows 0-40 into est_in), qrgpu_observe_batch (the
robot class's filters, in place), qrgpu_ground_update_batch, qrgpu_estimator_update_batch, qrgpu_pack_state_batch into arrays of their own, and the tick
on those; the plant's true fb_state is read by the plant alone.  All-stance gait: rows 41-44 of est_in are STANCE, uploaded once.  With --episodes the
stage-reset binding (mask = the step's done words, ticks = ep_state) restarts the observe, ground and estimator memory of a respawned robot.
--sensor-noise A adds the stage's noise (accelerometer 10 A m/s^2, gyro A rad/s, q 0.1 A rad, qd A rad/s).  How the standing batch fares on the
estimate, and how far the estimate lies from the truth, is reported, not judged; the trot in this loop and stability under noise are not claimed.

--trot (implies --estimator and --body) runs the reference's MPC trot (LocomotionMode::ADVANCED_TROT with MPC + WBC) closed on the device.  After the
settle phase each tick queues, in the order of qrLocomotionController::Update / GetAction / qrFSMStateLocomotion::Run: [episode step,] plant, observe,
ground, estimator, pack, qrgpu_command_update_batch (the operator's command --cmd-vx / --cmd-yaw in mode JOY_ADVANCED_TROT, uploaded once), gait (its
contacts are rows 13-16 of est_in, no copy), qrgpu_trot_inputs_batch, swing update, footholds, swing targets, MPC front-end, tick,
qrgpu_mpc_command_batch, whose output is the motor command the plant reads.  With --episodes the stage-reset binding restarts the command filter and the
swing-command memory of a respawned robot with the other stages' memory, and the gait runs on the robot's own clock.  The reference runs either the MPC
or the WBC on a tick (wbcData.allowAfterMPC); the plain --trot tick runs both every tick, and the front-end re-plans the trajectory on its own cadence.
--cadence (needs --trot) runs the reference's tick instead: qrgpu_tick_cadence_batch with the `updated` array the front-end fills -- a robot that
re-plans is solved and commands J^T f_ff, every other robot commands its held f_ff through the current Jacobian and runs the WBC on the held Fr_des.
The mask never leaves the device; its mean over the timed ticks is logged there and read once, after the loop (mpc_due_share).  The
run logs on the device, per tick, the tick's status words and the Kd rows of the motor command (one device-to-device copy of 12 rows), and the true state
100 ticks before the end; they are read once, after the loop.  Whether the batch trots, drifts or falls is reported, not judged.

--fsm (implies --trot --episodes) puts the control state machine in charge of every robot: qrgpu_fsm_update_batch after the episode step (its joy rows
feed qrgpu_command_update_batch, its stage mask -- the episode's reasons or QRGPU_FSM_ENTERED -- is the stage-reset binding's), qrgpu_fsm_zero_command_batch
after the command update, qrgpu_fsm_command_batch after the MPC command, whose column it passes on, replaces or repeats.  The robots spawn at the
sit-down angles, 0.14 above the ground; an episode ends by tilt, by a clearance under 0.05 m or by a non-finite state (a sitting robot rests on its
trunk: trunk contact is no reason here).  A device script keyed on each robot's episode tick presses X once the stand-up is over (to JOY_STAND) and X
again with --cmd-vx / --cmd-yaw on the axes (to JOY_ADVANCED_TROT): a respawned robot goes through the same sequence again.  time_step is the
tick's 0.002 x --fsm-speed and transition_ticks 500 / --fsm-speed: at speed 1 the stand-up takes 1500 ticks and the script presses at ticks 1600 and 2400.
--fsm-gait (implies --fsm) lets the gait follow the machine: the gait call becomes qrgpu_gait_select_update_batch on row 44 of fsm_state over the default
gait table, with swing_in given (rows 8-11: the swingDuration of each robot's gait), and the binding's clock comes from qrgpu_stage_clock_batch, so it
counts from the robot's last OnEnter or spawn.  Without the flag the launches and the output are what they were.
--fsm-mode (implies --fsm --fsm-gait --cadence) lets the MODE follow the machine too.  One tick: episode step, fsm update, stage clock and binding,
qrgpu_mode_route_batch on row 45 of fsm_state and the plan, qrgpu_set_mode_route, plant, observe, ground (its output kept), estimator, pack, command update
(the rows of both chains: fe_in, fh_in, stance_cmd), zero command, gait select, the MPC chain up to qrgpu_mpc_command_batch and the force-balance chain up to
qrgpu_stance_tick_batch, each into arrays of its own, qrgpu_mode_command_batch, fsm command.  Under the binding the cadenced tick solves only the robots on the
MPC chain and the force-balance QP only those on its own; a robot that sits, stands up or holds is solved by neither.  Every --fsm-trot-every-th robot (default:
every third) presses X a third time four ticks after the second, inside the gait transition, so that OnEnter finds it in JOY_TROT: mode VELOCITY, the `trot`
gait, the force-balance chain.  The script is one for the batch; the robots that do not press on read it on a clock shifted past its third entry
(qrgpu_stage_clock_batch with a mask nobody raises subtracts a per-robot origin).  Without the flag the launches and the output are what they were.

--fb-trot (implies --estimator and --body; not with --trot, --cadence or --fsm) runs the reference's force-balance trot -- JOY_TROT:
LocomotionMode::VELOCITY_LOCOMOTION with TorqueStanceLegController and the velocity case of the swing controller -- closed on the device.  Per tick, with
no host copy: [episode step,] plant, observe, ground (its output kept: the stance stage reads it), estimator, qrgpu_command_update_batch (--cmd-vx /
--cmd-yaw in mode JOY_TROT, uploaded once; it writes stateDes and rows 0-6 of stance_cmd, swing_vel_in / fe_in / fh_in not given), gait (the `trot` entry
of qrgpu_gait_table_default), qrgpu_velocity_inputs_batch, swing update (mode VELOCITY: the lift-off rows of swing_vel_in), qrgpu_swing_velocity_batch (the
entry's stance duration), qrgpu_stance_tick_batch (mode VELOCITY; swing_q = row 24 of the swing-velocity output, swing_flag from the inputs stage), whose
motor command the plant reads.  Rows 7-27 of stance_cmd (the walk pose plan's and the position mode's, which VELOCITY does not read) hold the stand pose
and zeros, uploaded once.  --terrain picks the TerrainType the stages get: flat and gap PLANE, stairs STAIRS, plane SLOPE, rough ROUGH.  With --episodes
the stage-reset binding also clears the swing-command entries of a respawned robot.  Whether the batch trots, drifts or falls is reported, not judged.

  fb_trot, cmd_vx, cmd_yaw, speed_along_command_mean / speed_robots (as --trot), swing_legs_commanded (legs x ticks x robots whose swing flag was set,
                warm-up included; _per_robot_tick), vmc_flagged_share (share of ticks x robots whose force-balance QP status word carries a flag)
  fsm, fsm_state_share (share of robots x timed ticks in PASSIVE, STAND_UP, LOCOMOTION), stood_up (robots that completed a stand-up), entered_locomotion,
                fell_before_locomotion (robots whose first episode ended before they had entered locomotion): warm-up included, reported, not judged
  fsm_gait, gait_share (--fsm-gait; share of robots x timed ticks on each entry of the gait table: none_yet, trot, advanced_trot, walk, stand, from
                row 48 of gait_state), standing_robot_ticks (robots x ticks in LOCOMOTION under JOY_STAND, the "MPC standing" phase, warm-up included),
                standing_swing_legs_commanded (legs that carried a swing command in them) beside standing_swing_legs_nominal_without (the legs the one
                advanced_trot desc of --fsm schedules to swing in the same robot-ticks, on its clock from the spawn, holds ignored): reported, not judged
  fsm_mode, chain_share (--fsm-mode; share of robots x timed ticks on no chain, the MPC chain, the force-balance chain, from the counters the route writes
                per tick), route_flagged (share whose route word carries a flag), solved_share (share that was due AND on the MPC chain: the solves that
                ran), tick_flagged_share_mpc / vmc_flagged_share_force_balance and swing_legs_commanded_mpc / _force_balance (the trot's figures over the
                robot-ticks of each chain, warm-up included): reported, not judged
  ticks_per_s   closed-loop control ticks per second: every robot advances one tick per (plant step + controller tick)
  trot, cmd_vx, cmd_yaw, speed_along_command_mean (world x over the last 100 ticks, m/s, robots not respawned in them: speed_robots), yaw_rate_mean,
                tick_flagged_share (share of ticks x robots whose tick status word carries a flag), swing_legs_commanded (legs x ticks x robots that
                carried a swing command, warm-up included; _per_robot_tick: their mean number per robot and tick), swing_flags_seen (OR of QRGPU_SW_*)
  cadence, mpc_due_share   (--cadence) true; the share of robots x timed ticks that were solved (1 / the front-end's period once the first 50 ticks are over)
  in_band       share of the robots that end inside the stand band: |z - 0.27| <= 0.01, |x|, |y| <= 0.03, |roll|, |pitch| <= 0.03
  fallen        (--body) robots that raised PL_TRUNK_CONTACT or PL_KNEE_CONTACT at any tick of the loop, warm-up included
  nonfinite     robots whose state left the finite numbers
  episodes_finished, by_reason, mean_episode_ticks   (--episodes) episodes ended in the loop, warm-up included; how often each EP_* bit was among the
                reasons; their mean length in ticks
  alive_at_end  (--episodes) share of the robots that are finite, within 0.5 rad of level and off their knees and trunk at the last tick
  est_err_velocity / height / roll_pitch _mean, _max   (--estimator) |estimated - true| of the base velocity (world, m/s), the height (m) and roll and
                pitch (rad) over the robots whose estimate and truth are finite (estimate_finite) at the last tick; sensor_noise: A
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAND_POSE = np.tile(np.array([0.0, 0.8, -1.6], np.float32), 4)
HEIGHT, HORIZON = 0.27, 10


def _load_pkg():
    d = os.path.join(ROOT, "quadruped-robot_amd")
    spec = importlib.util.spec_from_file_location("quadruped_robot_amd", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["quadruped_robot_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def _rpy(q):
    q0, q1, q2, q3 = (q[:, k].astype(np.float64) for k in range(4))
    return np.stack([np.arctan2(2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3), np.arcsin(np.clip(-2 * (q1 * q3 - q0 * q2), -1, 1))], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=500, help="closed-loop ticks of 2 ms, timed")
    ap.add_argument("--substeps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--terrain", default=None, metavar="KIND[:ARG]", help="run on a height field: flat, plane:0.2, stairs:0.04, gap:0.1, rough:0.01")
    ap.add_argument("--push", type=float, default=0.0, metavar="N", help="world-frame force along +x on every base during the timed loop, newtons")
    ap.add_argument("--body", action="store_true", help="knee and trunk contact and joint limits: qrgpu_plant_step_body_batch")
    ap.add_argument("--episodes", action="store_true", help="per-robot termination and respawn on the device: qrgpu_episode_step_batch (implies --body)")
    ap.add_argument("--max-ticks", type=int, default=0, metavar="N", help="(--episodes) truncate an episode after N ticks; 0 = never")
    ap.add_argument("--spawn-spread", type=float, default=0.05, metavar="M", help="(--episodes) spacing of the 3 x 3 grid of spawn points, metres")
    ap.add_argument("--estimator", action="store_true", help="the tick reads the estimator chain's state (plant sensor rows -> observe -> ground -> estimator -> pack), not the plant's truth")
    ap.add_argument("--sensor-noise", type=float, default=0.0, metavar="A", help="(--estimator) sensor noise: acc 10 A m/s^2, gyro A rad/s, q 0.1 A rad, qd A rad/s")
    ap.add_argument("--trot", action="store_true", help="the MPC trot closed on the device: command, gait, data flow, swing, front-end, tick, MPC command (implies --estimator --body)")
    ap.add_argument("--cmd-vx", type=float, default=0.0, metavar="V", help="(--trot) joyCmdVx, m/s")
    ap.add_argument("--cmd-yaw", type=float, default=0.0, metavar="W", help="(--trot) joyCmdYawRate, rad/s")
    ap.add_argument("--cadence", action="store_true", help="(--trot) the tick on the reference's cadence: per robot the MPC or the WBC, from the front-end's mask (qrgpu_tick_cadence_batch)")
    ap.add_argument("--fsm", action="store_true", help="the control state machine decides what every robot runs: sit, stand up, stand, trot (implies --trot --episodes)")
    ap.add_argument("--fsm-speed", type=float, default=1.0, metavar="S", help="(--fsm) run the stand-up and the transitions S times faster")
    ap.add_argument("--fsm-gait", action="store_true", help="(implies --fsm) every robot on the gait its state machine chose, the stages' clock counted from its last OnEnter or spawn")
    ap.add_argument("--fsm-mode", action="store_true", help="(implies --fsm --fsm-gait --cadence) every robot's solve in the chain its state machine chose: JOY_TROT robots on the force-balance chain, the others on the MPC chain")
    ap.add_argument("--fsm-trot-every", type=int, default=3, metavar="K", help="(--fsm-mode) every K-th robot presses on to JOY_TROT; 0 = nobody")
    ap.add_argument("--fb-trot", action="store_true", help="the force-balance trot (JOY_TROT, mode VELOCITY) closed on the device: command, gait, velocity inputs, swing, stance tick (implies --estimator --body)")
    ap.add_argument("--profile", action="store_true", help="the run a profiler traces: fewer ticks, nothing else changed")
    a = ap.parse_args()
    a.fsm_gait = a.fsm_gait or a.fsm_mode
    a.cadence = a.cadence or a.fsm_mode
    a.fsm = a.fsm or a.fsm_gait
    if a.fsm_trot_every < 0:
        ap.error("--fsm-trot-every is a count")
    if a.fb_trot and (a.trot or a.cadence or a.fsm):
        ap.error("--fb-trot excludes --trot, --cadence and --fsm")
    a.trot = a.trot or a.fsm
    a.episodes = a.episodes or a.fsm
    if (a.cmd_vx != 0.0 or a.cmd_yaw != 0.0) and not (a.trot or a.fb_trot):
        ap.error("--cmd-vx / --cmd-yaw need --trot or --fb-trot")
    if a.cadence and not a.trot:
        ap.error("--cadence needs --trot")
    a.estimator = a.estimator or a.trot or a.fb_trot
    a.body = a.body or a.episodes or a.trot or a.fb_trot
    if a.sensor_noise != 0.0 and not a.estimator:
        ap.error("--sensor-noise needs --estimator")
    pkg = _load_pkg()
    pkg._build.build()
    n, h = a.robots, HORIZON
    ticks = min(a.ticks, 100) if a.profile else a.ticks
    ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    ctx.mpc_setup_packed(0, pkg.mpc_cfg("a1"), h)
    ctx.wbc_setup_packed(0, pkg.model_desc("a1"))
    fb0 = np.zeros((37, n), np.float32); fb0[0] = 1.0; fb0[6] = 0.30; fb0[13:25] = STAND_POSE[:, None]
    cmd0 = np.zeros((60, n), np.float32); cmd0[0:12] = STAND_POSE[:, None]; cmd0[12:24] = 100.0; cmd0[36:48] = 2.0
    if a.fsm:           # the robots start sitting
        fdesc = pkg.fsm_desc(time_step=0.002 * a.fsm_speed, transition_ticks=max(1, int(round(500 / a.fsm_speed))))
        fb0[6] = 0.14; fb0[13:25] = np.array(fdesc.sit_down_angles[:], np.float32)[:, None]; cmd0[0:12] = fb0[13:25]
    traj = np.zeros((h, 12, n), np.float32); traj[:, 5] = HEIGHT
    wcmd = np.zeros((67, n), np.float32); wcmd[2] = HEIGHT; wcmd[63:67] = 1.0
    d = dict(fb=ctx.alloc((37, n)).upload(fb0), cmd=ctx.alloc((60, n)).upload(cmd0), mpc=ctx.alloc((28, n)), out=ctx.alloc((pkg.qrgpu.PLANT_OUT_ROWS, n)),
             traj=ctx.alloc((12 * h, n)).upload(traj.reshape(12 * h, n)), gait=ctx.alloc((4 * h, n)).upload(np.ones((4 * h, n), np.float32)),
             wcmd=ctx.alloc((67, n)).upload(wcmd), prev=ctx.alloc((3, n)).zero(), force=ctx.alloc((12, n)),
             tick_status=ctx.alloc((n,), np.int32), plant_status=ctx.alloc((n,), np.int32), flags=ctx.alloc((2, n), np.int32))
    on_field = a.terrain is not None or a.push != 0.0 or a.body
    if on_field:
        kind, _, arg = (a.terrain or "flat").partition(":")
        grid, field = pkg.terrain.make(kind, arg or None)
        if kind == "plane":                                           # aligned with the slope: z axis along the normal, 0.30 above the origin
            th = np.arctan(float(arg) if arg else 0.2)
            fb0[0] = np.cos(-0.5 * th); fb0[2] = np.sin(-0.5 * th); fb0[4] = -0.30 * np.sin(th); fb0[6] = 0.30 * np.cos(th)
            d["fb"].upload(fb0)
        tdesc = pkg.terrain_desc(n_fields=1, **grid.desc())
        d["height"] = ctx.alloc((1, grid.ny, grid.nx)).upload(pkg.terrain.stack([field]))
        d["push"] = ctx.alloc((6, n)).zero()
        d["tout"] = ctx.alloc((pkg.qrgpu.TERRAIN_OUT_ROWS, n))
    if a.body:
        ctx.plant_body_setup(0, pkg.plant_body_desc("a1"))
        d["bout"] = ctx.alloc((pkg.qrgpu.BODY_OUT_ROWS, n))
        d["status_log"] = ctx.alloc((ticks + 20, n), np.int32).zero()        # every tick's plant status: read once, after the loop

    if a.episodes:
        q = pkg.qrgpu
        cx, cy = grid.x0 + 0.5 * (grid.nx - 1) * grid.cell, grid.y0 + 0.5 * (grid.ny - 1) * grid.cell
        gx, gy = np.meshgrid(cx + a.spawn_spread * np.arange(-1, 2), cy + a.spawn_spread * np.arange(-1, 2))
        table = np.zeros((4, 9), np.float32); table[0] = gx.ravel(); table[1] = gy.ravel()
        sitting = dict(q_spawn=fdesc.sit_down_angles[:], spawn_height=0.14, status_mask=q.PL_NONFINITE | q.PL_QUAT_ZERO, min_clearance=0.05) if a.fsm else {}
        edesc = pkg.episode_desc(max_ticks=a.max_ticks, seed=a.seed, align_to_slope=int(kind == "plane"), field_margin=0.2, v_jitter=0.3, **sitting)
        d.update(table=ctx.alloc((4, 9)).upload(table), ep_state=ctx.alloc((q.EPISODE_STATE_ROWS, n), np.int32).zero(), ep_stats=ctx.alloc((q.EPISODE_STATS_ROWS, n)),
                 done_log=ctx.alloc((ticks + 20, n), np.int32).zero(), done_list=ctx.alloc((n,), np.int32), done_count=ctx.alloc((1,), np.int32))

    if a.estimator:     # the sensor-driven chain's arrays: the plant's rows are filtered in place (est_in = raw); rows 41-44 of est_in are STANCE, uploaded once
        A = a.sensor_noise
        odesc = pkg.observe_desc("sim", seed=a.seed, acc_noise=10.0 * A, gyro_noise=A, q_noise=0.1 * A, qd_noise=A)
        ecfg = pkg.workload.estimator_cfg("a1")
        com = np.asarray(pkg.workload.ROBOTS["a1"]["com_offset"], np.float32)
        est0 = np.zeros((54, n), np.float32); est0[41:45] = 1.0
        nd = ctx.estimator_state_doubles(int(ecfg[6]))                    # (the window)
        d.update(est_in=ctx.alloc((54, n)).upload(est0), obs=ctx.alloc((ctx.observe_state_rows(odesc), n)), rpy=ctx.alloc((3, n)), gin=ctx.alloc((23, n)),
                 stamp=ctx.alloc((n,), np.uint32), gst=ctx.alloc((13, n), np.float64), est_state=ctx.alloc((nd, n), np.float64).zero(),
                 est_out=ctx.alloc((42, n)).zero(), mpc_est=ctx.alloc((28, n)), fb_est=ctx.alloc((37, n)))

    if a.trot:          # the trot's stages: their memory, the arrays they hand one another, the operator's command (uploaded once)
        q, W = pkg.qrgpu, pkg.workload
        cdesc, mdesc, sdesc = pkg.command_desc(), pkg.mpc_command_desc(), pkg.swing_mode_desc(q.MODE_ADVANCED_TROT, terrain=0)
        gcfg, fcfg = W.gait_cfg(), W.foothold_cfg("a1")
        joy = np.zeros((q.JOY_ROWS, n), np.float32); joy[0] = a.cmd_vx; joy[5] = a.cmd_yaw; joy[6] = cdesc.body_height; joy[7] = q.RC_JOY_ADVANCED_TROT
        swing_in = np.zeros((58, n), np.float32)
        swing_in[8:12] = np.float32(gcfg[0]) / np.float32(gcfg[4]) - np.float32(gcfg[0])       # swingDuration = stanceDuration / dutyFactor - stanceDuration
        d.update(joy=ctx.alloc((q.JOY_ROWS, n)).upload(joy), cmd_state=ctx.alloc((q.CMD_STATE_ROWS, n)), state_des=ctx.alloc((12, n)),
                 fe_in=ctx.alloc((64, n)).zero(), fe_state=ctx.alloc((8, n)), fh_in=ctx.alloc((46, n)).zero(), swing_in=ctx.alloc((58, n)).upload(swing_in),
                 gait_state=ctx.alloc((52, n)), gait_out=ctx.alloc((24, n)), swing_state=ctx.alloc((q.SWING_STATE_FLOATS, n)),
                 swing_flags=ctx.alloc((n,), np.int32), qdes=ctx.alloc((24, n)).zero(), tau=ctx.alloc((12, n)), cmd_mem=ctx.alloc((1, n), np.int32),
                 updated=ctx.alloc((n,), np.int32), tick_log=ctx.alloc((ticks + 20, n), np.int32).zero(), kd_log=ctx.alloc((ticks + 20, 12, n)),
                 fb_then=ctx.alloc_pinned((37, n)))
        if a.cadence:   # the kept base-frame force (the force array is the other half of the memory), and every tick's mask
            d.update(hold=ctx.alloc((12, n)).zero(), due_log=ctx.alloc((ticks + 20, n), np.int32).zero())
            d["force"].zero()

    if a.fb_trot:       # the force-balance trot's stages: their memory, the arrays they hand one another, the operator's command (uploaded once)
        q, W = pkg.qrgpu, pkg.workload
        ttype = dict(flat=0, gap=0, stairs=2, plane=3, rough=4)[kind]                   # TerrainType: PLANE, STAIRS, SLOPE, ROUGH
        cdesc, sdesc, stdesc = pkg.command_desc(), pkg.swing_mode_desc(q.MODE_VELOCITY, terrain=ttype), pkg.stance_desc(q.MODE_VELOCITY, terrain=ttype)
        gcfg = pkg.gait_table_default()[q.FSM_GAIT_TROT]                              # advanced_trot 0
        svcfg = W.swing_velocity_cfg("a1", stance_duration=float(gcfg[0]))
        ctx.vmc_setup_packed(0, W.vmc_cfg("a1"), pkg.model_desc("a1")[:3])
        joy = np.zeros((q.JOY_ROWS, n), np.float32); joy[0] = a.cmd_vx; joy[5] = a.cmd_yaw; joy[6] = cdesc.body_height; joy[7] = q.RC_JOY_TROT
        scmd = np.zeros((28, n), np.float32); scmd[9] = HEIGHT; scmd[15] = HEIGHT          # rows 7-27: not read in VELOCITY
        d.update(joy=ctx.alloc((q.JOY_ROWS, n)).upload(joy), cmd_state=ctx.alloc((q.CMD_STATE_ROWS, n)), state_des=ctx.alloc((12, n)),
                 stance_cmd=ctx.alloc((28, n)).upload(scmd), gout=ctx.alloc((32, n)), gait_state=ctx.alloc((52, n)), gait_out=ctx.alloc((24, n)),
                 swing_state=ctx.alloc((q.SWING_STATE_FLOATS, n)), swing_flags=ctx.alloc((n,), np.int32), sv=ctx.alloc((53, n)).zero(),
                 sv_out=ctx.alloc((48, n)).zero(), cmd_mem=ctx.alloc((1, n), np.int32).zero(), swing_flag=ctx.alloc((4, n)).zero(),
                 stance_state=ctx.alloc((q.STANCE_STATE_FLOATS, n)), vmc_in=ctx.alloc((37, n)), ratio=ctx.alloc((8, n)), stance_out=ctx.alloc((33, n)),
                 tau=ctx.alloc((12, n)), vmc_log=ctx.alloc((ticks + 20, n), np.int32).zero(), flag_log=ctx.alloc((ticks + 20, 4, n)).zero(),
                 fb_then=ctx.alloc_pinned((37, n)))

    if a.fsm:           # the machine's memory, what it hands the stages, its per-tick report, the script (X after the stand-up, X with the command)
        q = pkg.qrgpu
        up = int(np.ceil(fdesc.stand_up_total / fdesc.time_step))
        first_press = up + max(4, int(100 / a.fsm_speed))
        press = np.array([[first_press, q.JOY_BTN_X, 0.0, 0.0, 0.0],
                          [first_press + max(20, int(800 / a.fsm_speed)), q.JOY_BTN_X, a.cmd_yaw / fdesc.max_yawrate, 0.0, a.cmd_vx / fdesc.max_velx]], np.float32).T.copy()
        if a.fsm_mode:  # a third X four ticks later, inside the gait transition: JOY_ADVANCED_TROT -> JOY_TROT before OnEnter reads it.  The script is one for
                        # the batch, keyed on a tick count per robot: the robots that do not press on read the first two entries SCRIPT_SHIFT ticks later, on a
                        # clock shifted by as much (script_ticks below), and never meet the third
            SCRIPT_SHIFT = 1 << 20
            third = press[:, 1].copy(); third[0] += 4
            late = press.copy(); late[0] += SCRIPT_SHIFT
            press = np.concatenate([press, third[:, None], late], axis=1).copy()
        d.update(fsm_state=ctx.alloc((q.FSM_STATE_ROWS, n)), plan=ctx.alloc((n,), np.int32), stage_mask=ctx.alloc((n,), np.int32), script=ctx.alloc(press.shape).upload(press),
                 fsm_log=ctx.alloc((ticks + 20, q.FSM_OUT_ROWS, n)).zero(), plan_log=ctx.alloc((ticks + 20, n), np.int32).zero())
    if a.fsm_gait:      # the gait table, the clock's memory and its output, the flags, every tick's index in force (row 48 of gait_state)
        gtable = pkg.workload.gait_table()
        d.update(clock_origin=ctx.alloc((n,), np.int32).zero(), clock_local=ctx.alloc((n,), np.int32).zero(), gait_flags=ctx.alloc((n,), np.int32),
                 gait_log=ctx.alloc((ticks + 20, n)).zero())
    if a.fsm_mode:      # the route, the force-balance chain's stages and the arrays the two chains do not share: swing memory and flags, swing-command entries,
                        # force, torque, status, motor command.  The command, gait, ground, estimator and observe arrays are shared
        q, W = pkg.qrgpu, pkg.workload
        ttype = dict(flat=0, gap=0, stairs=2, plane=3, rough=4)[kind]
        rdesc = pkg.mode_route_desc()
        fb_sdesc, stdesc = pkg.swing_mode_desc(q.MODE_VELOCITY, terrain=ttype), pkg.stance_desc(q.MODE_VELOCITY, terrain=ttype)
        svcfg = W.swing_velocity_cfg("a1", stance_duration=float(pkg.gait_table_default()[q.FSM_GAIT_TROT][0]))
        ctx.vmc_setup_packed(0, W.vmc_cfg("a1"), pkg.model_desc("a1")[:3])
        scmd = np.zeros((28, n), np.float32); scmd[9] = HEIGHT; scmd[15] = HEIGHT
        presses_on = (np.arange(n) % a.fsm_trot_every == a.fsm_trot_every - 1) if a.fsm_trot_every else np.zeros(n, bool)
        d.update(chain_log=ctx.alloc((ticks + 20, n), np.int32).zero(), count_log=ctx.alloc((ticks + 20, 3), np.int32).zero(),
                 route_log=ctx.alloc((ticks + 20, n), np.int32).zero(), script_origin=ctx.alloc((n,), np.int32).upload(np.where(presses_on, 0, -SCRIPT_SHIFT).astype(np.int32)),
                 script_ticks=ctx.alloc((n,), np.int32).zero(), nobody=ctx.alloc((n,), np.int32).zero(),
                 cmd_mpc=ctx.alloc((60, n)).zero(), cmd_fb=ctx.alloc((60, n)).zero(), stance_cmd=ctx.alloc((28, n)).upload(scmd), gout=ctx.alloc((32, n)),
                 fb_swing_state=ctx.alloc((q.SWING_STATE_FLOATS, n)), fb_swing_flags=ctx.alloc((n,), np.int32), sv=ctx.alloc((53, n)).zero(),
                 sv_out=ctx.alloc((48, n)).zero(), fb_cmd_mem=ctx.alloc((1, n), np.int32).zero(), swing_flag=ctx.alloc((4, n)).zero(),
                 stance_state=ctx.alloc((q.STANCE_STATE_FLOATS, n)), vmc_in=ctx.alloc((37, n)), ratio=ctx.alloc((8, n)), stance_out=ctx.alloc((33, n)),
                 fb_force=ctx.alloc((12, n)).zero(), fb_tau=ctx.alloc((12, n)).zero(), mpc_status=ctx.alloc((n,), np.int32).zero(),
                 fb_status=ctx.alloc((n,), np.int32).zero())
        d["tau"].zero()

    def plant(par, **out):
        if a.body:
            ctx.plant_step_body_batch(n, par, tdesc, d["height"], d["fb"], d["cmd"], base_push=d["push"], terrain_out=d["tout"], body_out=d["bout"], **out)
        elif on_field:
            ctx.plant_step_terrain_batch(n, par, tdesc, d["height"], d["fb"], d["cmd"], base_push=d["push"], terrain_out=d["tout"], **out)
        else:
            ctx.plant_step_batch(n, par, d["fb"], d["cmd"], **out)

    settle = pkg.plant_params(dt=0.001, substeps=1)
    for _ in range(400):
        plant(settle, mpc_state=d["mpc"])
    ctx.sync()
    fb = d["fb"].download()
    rng = np.random.default_rng(a.seed)
    fb[10:12] += rng.uniform(-0.3, 0.3, (2, n)).astype(np.float32)
    d["fb"].upload(fb); d["cmd"].zero()
    if a.push != 0.0:
        push = np.zeros((6, n), np.float32); push[0] = a.push
        d["push"].upload(push)
    ctx.set_warm_start(True)
    params = pkg.plant_params(dt=0.002, substeps=a.substeps)
    tau = d["cmd"].row(48)
    if a.trot:          # MPCStanceLegController::Reset on the settled robot: yawDesTrue, posDesiredinWorld from the pose at hand, the counter at 0
        fst = np.zeros((8, n), np.float32)
        fst[3] = np.arctan2(2 * (fb[0] * fb[3] + fb[1] * fb[2]), 1 - 2 * (fb[2] ** 2 + fb[3] ** 2)); fst[4:7] = fb[4:7]
        d["fe_state"].upload(fst)

    done, total = [0], [20 + ticks]
    if a.episodes:      # episode 0 is the state at hand: its spawn rows written here, not drawn
        stats = np.zeros((pkg.qrgpu.EPISODE_STATS_ROWS, n), np.float32); stats[0:3] = fb[4:7]; stats[8] = 0.30
        d["ep_stats"].upload(stats)

    def loop(k):
        for _ in range(k):
            if a.episodes:
                ctx.episode_step_batch(n, edesc, d["fb"], d["table"], 9, d["ep_state"], d["ep_stats"], d["done_log"].row(done[0]), params=params, terrain=tdesc,
                                       height=d["height"], plant_status=d["status_log"].row(done[0] - 1) if done[0] else None, tick_status=None,
                                       prev_ori=d["prev"], motor_cmd=d["cmd"], done_list=d["done_list"], done_count=d["done_count"])
            if a.fsm:                         # JoyCallback, the change request, RunFSM up to the decision: the joy rows, the plan, the stages' reset mask
                if a.fsm_mode:                # the script's clock per robot: the episode's tick count, shifted for the robots that do not press on
                    ctx.stage_clock(n, d["nobody"], 1, d["ep_state"], d["script_origin"], d["script_ticks"])
                ctx.fsm_update(n, fdesc, d["fsm_state"], d["joy"], d["plan"], stage_mask=d["stage_mask"], script=d["script"], n_script=press.shape[1],
                               ticks=d["script_ticks"] if a.fsm_mode else d["ep_state"], done=d["done_log"].row(done[0]), bits=pkg.qrgpu.EP_REASONS,
                               reset=int(done[0] == 0))
                if a.fsm_gait:                # the stages' clock counts from the robot's last OnEnter or spawn, not from the spawn alone
                    ctx.stage_clock(n, d["stage_mask"], pkg.qrgpu.EP_REASONS | pkg.qrgpu.FSM_ENTERED, d["ep_state"], d["clock_origin"], d["clock_local"])
                    ctx.set_stage_reset(mask=d["stage_mask"], bits=pkg.qrgpu.EP_REASONS | pkg.qrgpu.FSM_ENTERED, ticks=d["clock_local"])
                else:
                    ctx.set_stage_reset(mask=d["stage_mask"], bits=pkg.qrgpu.EP_REASONS | pkg.qrgpu.FSM_ENTERED, ticks=d["ep_state"])
                if a.fsm_mode:                # the chain each robot is on this tick, from the mode OnEnter latched (row 45 of fsm_state) and this tick's plan
                    ctx.mode_route(n, rdesc, d["fsm_state"].row(45), d["chain_log"].row(done[0]), plan=d["plan"], route_flags=d["route_log"].row(done[0]),
                                   chain_count=d["count_log"].row(done[0]))
                    ctx.set_mode_route(d["chain_log"].row(done[0]))
            elif a.estimator and a.episodes:  # the observe, ground and estimator stages restart a robot this episode step respawned
                ctx.set_stage_reset(mask=d["done_log"].row(done[0]), ticks=d["ep_state"])
            plant(params, plant_out=d["out"], mpc_state=d["mpc"], status=d["status_log"].row(done[0]) if a.body else d["plant_status"],
                  **(dict(est_in=d["est_in"]) if a.estimator else {}))
            if a.estimator:                   # the plant's true fb_state is read by the plant alone: the tick gets mpc_est, fb_est
                first = done[0] == 0
                ctx.observe_batch(n, odesc, d["est_in"], d["obs"], d["est_in"], d["rpy"], ground_in=d["gin"], tick=d["stamp"], est_out_prev=d["est_out"],
                                  reset=first, step=done[0])
                ctx.ground_update_batch(n, d["gin"], d["gst"], d["gout"] if a.fb_trot or a.fsm_mode else None, d["est_in"], reset=first)
                ctx.estimator_update_batch(n, ecfg, d["est_in"], d["stamp"], d["est_state"], d["est_out"])
                if not a.fb_trot:             # (the force-balance chain reads est_in / est_out themselves: packed once after the loop, for the report)
                    ctx.pack_state_batch(n, com, d["est_in"], d["est_out"], d["rpy"], d["mpc_est"], d["fb_est"])
            done[0] += 1
            if a.fb_trot:                     # qrLocomotionController::Update / GetAction of the velocity mode, in the reference's order
                k = done[0] - 1
                t = float(np.float32(k) * np.float32(0.002))                   # (under --episodes the gait and the stance stage run on the binding's clock)
                ctx.command_update(n, cdesc, d["joy"], d["cmd_state"], state_des=d["state_des"], stance_cmd=d["stance_cmd"], reset=int(first))
                ctx.gait_update_batch(n, gcfg, t, d["est_in"].row(13), d["gait_state"], d["gait_out"], reset=first)
                ctx.velocity_inputs(n, d["est_in"], d["est_out"], d["gait_out"], d["gait_state"], d["state_des"], ground_out=d["gout"], swing_vel_in=d["sv"],
                                    est_in_next=d["est_in"], cmd_mem=d["cmd_mem"], swing_flag=d["swing_flag"], terrain=ttype, reset=int(first))
                ctx.swing_update_batch(n, sdesc, d["est_in"], d["est_out"], d["gait_out"], d["swing_state"], d["swing_flags"], swing_vel_in=d["sv"],
                                       reset=2 if first else 0)
                ctx.swing_velocity_batch(n, ecfg, svcfg, d["sv"], d["sv_out"])
                ctx.stance_tick_batch(n, stdesc, d["est_in"], d["est_out"], d["gout"], d["rpy"], d["gait_out"], d["stance_cmd"], d["stance_state"], d["vmc_in"],
                                      d["force"], d["tau"], d["cmd"], gait_state=d["gait_state"], ratio=d["ratio"], stance_out=d["stance_out"],
                                      status=d["vmc_log"].row(k), swing_q=d["sv_out"].row(24), swing_flag=d["swing_flag"], current_time=t, reset=first)
                ctx.copy_rows(d["flag_log"].row(k), d["swing_flag"], 4 * n)    # the report's log: the legs that carried a swing command this tick
                if k == total[0] - 101:
                    d["fb"].copy_to_pinned(d["fb_then"])                       # the truth 100 ticks before the end, for the mean speed
                continue
            if a.trot:                        # qrLocomotionController::Update / GetAction, qrFSMStateLocomotion::Run, in the reference's order
                k = done[0] - 1
                t = float(np.float32(k) * np.float32(0.002))                   # (under --episodes the gait runs on the binding's per-robot clock)
                fb_rows = dict(stance_cmd=d["stance_cmd"]) if a.fsm_mode else {}  # (the force-balance chain's copy of the command: rows 0-6 of stance_cmd)
                ctx.command_update(n, cdesc, d["joy"], d["cmd_state"], state_des=d["state_des"], fe_in=d["fe_in"], fh_in=d["fh_in"], reset=int(first), **fb_rows)
                if a.fsm:                     # SwitchMode / StandLoop: the robots in phase 1 run the chain on a zeroed command
                    ctx.fsm_zero_command(n, d["plan"], state_des=d["state_des"], fe_in=d["fe_in"], fh_in=d["fh_in"], **fb_rows)
                if a.fsm_gait:                # the gait OnEnter chose (row 44 of fsm_state), latched at the robot's reset; its swingDuration into swing_in
                    ctx.gait_select_update_batch(n, gtable, d["fsm_state"].row(44), t, d["est_in"].row(13), d["gait_state"], d["gait_out"], d["fe_in"],
                                                 swing_in=d["swing_in"], flags=d["gait_flags"], reset=int(first))
                    ctx.copy_rows(d["gait_log"].row(k), d["gait_state"].row(48), n)
                else:
                    ctx.gait_update_batch(n, gcfg, t, d["est_in"].row(13), d["gait_state"], d["gait_out"], d["fe_in"], reset=first)
                ctx.trot_inputs(n, d["est_in"], d["est_out"], d["rpy"], d["gait_out"], gait_state=d["gait_state"], fe_in=d["fe_in"], fh_in=d["fh_in"],
                                swing_in=d["swing_in"], est_in_next=d["est_in"])
                ctx.swing_update_batch(n, sdesc, d["est_in"], d["est_out"], d["gait_out"], d["swing_state"], d["swing_flags"], gait_state=d["gait_state"],
                                       swing_in=d["swing_in"], fe_in=d["fe_in"], reset=2 if first else 0)
                ctx.footholds_batch(n, fcfg, d["fh_in"], d["swing_in"], gait_state=d["gait_state"], gait_out=d["gait_out"])
                ctx.swing_targets_batch(n, ecfg, d["swing_in"], wbc_cmd=d["wcmd"], foot_target_world=d["fe_in"].row(26), qdes=d["qdes"])
                ctx.mpc_frontend_batch(n, d["fe_in"], d["fe_state"], d["traj"], d["gait"], d["wcmd"], d["updated"])
                if a.cadence:                 # (--fsm-mode: the status words of the robots on the chain land in an array that is not cleared in between)
                    ctx.tick_cadence_batch(n, d["updated"], d["mpc_est"], d["traj"], d["gait"], d["fb_est"], d["wcmd"], d["prev"], d["force"], d["hold"], d["tau"],
                                           d["mpc_status"] if a.fsm_mode else d["tick_log"].row(k))
                    ctx.copy_rows(d["due_log"].row(k), d["updated"], n)        # the report's log: who was solved this tick
                else:
                    ctx.tick_batch(n, d["mpc_est"], d["traj"], d["gait"], d["fb_est"], d["wcmd"], d["prev"], d["force"], d["tau"], d["tick_log"].row(k))
                ctx.mpc_command(n, mdesc, d["tau"], d["qdes"], d["swing_in"], d["gait_out"], d["gait_state"], d["cmd_mem"], d["cmd_mpc" if a.fsm_mode else "cmd"],
                                reset=int(first))
                if a.fsm_mode:                # the force-balance chain into its own arrays, then every robot's column and status word from its own chain
                    ctx.velocity_inputs(n, d["est_in"], d["est_out"], d["gait_out"], d["gait_state"], d["state_des"], ground_out=d["gout"], swing_vel_in=d["sv"],
                                        est_in_next=d["est_in"], cmd_mem=d["fb_cmd_mem"], swing_flag=d["swing_flag"], terrain=ttype, reset=int(first))
                    ctx.swing_update_batch(n, fb_sdesc, d["est_in"], d["est_out"], d["gait_out"], d["fb_swing_state"], d["fb_swing_flags"], swing_vel_in=d["sv"],
                                           reset=2 if first else 0)
                    ctx.swing_velocity_batch(n, ecfg, svcfg, d["sv"], d["sv_out"])
                    ctx.stance_tick_batch(n, stdesc, d["est_in"], d["est_out"], d["gout"], d["rpy"], d["gait_out"], d["stance_cmd"], d["stance_state"], d["vmc_in"],
                                          d["fb_force"], d["fb_tau"], d["cmd_fb"], gait_state=d["gait_state"], ratio=d["ratio"], stance_out=d["stance_out"],
                                          status=d["fb_status"], swing_q=d["sv_out"].row(24), swing_flag=d["swing_flag"], current_time=t, reset=first)
                    ctx.mode_command(n, d["chain_log"].row(k), d["cmd_mpc"], d["cmd_fb"], d["cmd"], status_mpc=d["mpc_status"], status_fb=d["fb_status"],
                                     status=d["tick_log"].row(k))
                if a.fsm:                     # the rest of RunFSM: the chain's column passed on, replaced by a stand-up, blend or hold, or repeated
                    ctx.fsm_command(n, fdesc, d["plan"], d["est_in"], d["cmd"], d["fsm_state"], d["cmd"], fsm_out=d["fsm_log"].row(k))
                    ctx.copy_rows(d["plan_log"].row(k), d["plan"], n, np.int32)
                ctx.copy_rows(d["kd_log"].row(k), d["cmd"].row(36), 12 * n)    # the report's log: Kd of this tick's command (a swing command carries the motor's)
                if k == total[0] - 101:
                    d["fb"].copy_to_pinned(d["fb_then"])                       # the truth 100 ticks before the end, for the mean speed
            elif a.estimator:
                ctx.tick_batch(n, d["mpc_est"], d["traj"], d["gait"], d["fb_est"], d["wcmd"], d["prev"], d["force"], tau, d["tick_status"])
            else:
                ctx.tick_batch(n, d["mpc"], d["traj"], d["gait"], d["fb"], d["wcmd"], d["prev"], d["force"], tau, d["tick_status"])

    loop(20)                                                          # warm-up: the first launches, the scheduler's history
    ctx.sync()
    t0 = time.perf_counter()
    loop(ticks)
    ctx.sync()
    sec = time.perf_counter() - t0
    if a.fb_trot:     # the estimate in the tick's layout, for the report below
        ctx.pack_state_batch(n, com, d["est_in"], d["est_out"], d["rpy"], d["mpc_est"], d["fb_est"])
        ctx.sync()
    fb = d["fb"].download()
    rp = _rpy(fb[0:4].T)
    ok = (np.abs(fb[6] - HEIGHT) <= 0.01) & (np.abs(fb[4:6]).max(0) <= 0.03) & (np.abs(rp).max(1) <= 0.03)
    tick_log = d["tick_log"].download() if a.trot else None
    vmc_log = d["vmc_log"].download() if a.fb_trot else None
    tick_flags = pkg.status_flags(tick_log[-1] if a.trot else vmc_log[-1] if a.fb_trot else d["tick_status"].download())
    log = d["status_log"].download() if a.body else None
    plant_flags = log[-1] if a.body else d["plant_status"].download()
    res = dict(metric="closed_loop_ticks_per_s", value=ticks / sec, robot_ticks_per_s=n * ticks / sec, ms_per_tick=1e3 * sec / ticks, robots=n, ticks=ticks,
               substeps=a.substeps, in_band=float(ok.mean()), last_tick_flagged=int(((tick_flags != 0) | (plant_flags != 0)).sum()), profile=bool(a.profile))
    if a.estimator:   # how far the estimate the tick read lies from the plant's truth at the last tick: reported, not judged
        est, tru = d["mpc_est"].download().astype(np.float64), d["mpc"].download().astype(np.float64)
        fin = np.isfinite(est).all(0) & np.isfinite(tru).all(0)
        err = dict(velocity=np.abs(est[3:6] - tru[3:6]).max(0), height=np.abs(est[2] - tru[2]), roll_pitch=np.abs(est[25:27] - tru[25:27]).max(0))
        res.update(estimator=True, sensor_noise=a.sensor_noise, estimate_finite=int(fin.sum()))
        for k, e in err.items():
            res["est_err_%s_mean" % k] = float(e[fin].mean()) if fin.any() else None
            res["est_err_%s_max" % k] = float(e[fin].max()) if fin.any() else None
    if on_field:      # what the controllers made of it: reported, not judged
        out = d["out"].download()
        fin = np.isfinite(fb).all(0)                                    # a robot whose state left the finite numbers is counted, not averaged
        m = lambda x: float(x[fin].mean()) if fin.any() else None
        res.update(terrain=a.terrain or "flat", push=a.push, nonfinite=int((~fin).sum()), pitch_mean=m(rp[:, 1]), z_mean=m(fb[6]), x_mean=m(fb[4]),
                   feet_in_contact=m(out[24:28].mean(0)), upright=float((fin & (np.nan_to_num(np.abs(rp).max(1), nan=9.0) < 0.5)).mean()),
                   plant_flags=int(np.bitwise_or.reduce(plant_flags)))
    if a.body:
        q = pkg.qrgpu
        seen = np.bitwise_or.reduce(log, axis=0)
        res.update(body=True, fallen=int(((seen & (q.PL_TRUNK_CONTACT | q.PL_KNEE_CONTACT)) != 0).sum()), at_a_stop=int(((seen & q.PL_JOINT_LIMIT) != 0).sum()),
                   fallen_at_end=int(((plant_flags & (q.PL_TRUNK_CONTACT | q.PL_KNEE_CONTACT)) != 0).sum()))
    if a.episodes:
        q = pkg.qrgpu
        dl = d["done_log"].download() & q.EP_REASONS
        st = d["ep_state"].download()
        names = ("status", "tick_status", "nonfinite", "tilt", "height", "off_field", "timeout", "forced")
        lengths = []
        for r in range(n):                                              # episode lengths from the log of reason words: ticks between a robot's ends
            t = np.nonzero(dl[:, r])[0]
            lengths.extend(np.diff(np.concatenate([[-1], t])).tolist())
        fell = (plant_flags & (q.PL_TRUNK_CONTACT | q.PL_KNEE_CONTACT)) != 0
        alive = np.isfinite(fb).all(0) & (np.nan_to_num(np.abs(rp).max(1), nan=9.0) < 0.5) & ~fell
        res.update(episodes=True, max_ticks=a.max_ticks, episodes_finished=int(st[4].sum() + st[5].sum()), episodes_failed=int(st[4].sum()),
                   episodes_timed_out=int(st[5].sum()), by_reason={nm: int(((dl >> k) & 1).sum()) for k, nm in enumerate(names)},
                   mean_episode_ticks=float(np.mean(lengths)) if lengths else None, alive_at_end=float(alive.mean()))
    if a.trot:        # what the trot did: reported, not judged
        kd = d["kd_log"].download()[:, 0::3]                              # [tick][leg][robot]: the abad's Kd, the motor's own on a swing command
        swing = kd != np.float32(mdesc.stance_kd)
        res.update(trot=True, cmd_vx=a.cmd_vx, cmd_yaw=a.cmd_yaw, tick_flagged_share=float((pkg.status_flags(tick_log) != 0).mean()),
                   swing_legs_commanded=int(swing.sum()), swing_legs_commanded_per_robot_tick=float(swing.sum(1).mean()),
                   swing_flags_seen=int(np.bitwise_or.reduce(d["swing_flags"].download())))
        if a.cadence:
            res.update(cadence=True, mpc_due_share=float((d["due_log"].download()[20:20 + ticks] != 0).mean()))
    if a.fb_trot:     # what the force-balance trot did: reported, not judged
        swing = d["flag_log"].download() != 0                             # [tick][leg][robot]
        res.update(fb_trot=True, cmd_vx=a.cmd_vx, cmd_yaw=a.cmd_yaw, vmc_flagged_share=float((pkg.status_flags(vmc_log) != 0).mean()),
                   swing_legs_commanded=int(swing.sum()), swing_legs_commanded_per_robot_tick=float(swing.sum(1).mean()),
                   swing_flags_seen=int(np.bitwise_or.reduce(d["swing_flags"].download())))
    if a.trot or a.fb_trot:
        if ticks >= 81:   # mean base speed along the command over the last 100 ticks, from the plant's truth; robots respawned in that window left out
            then = d["fb_then"].array
            calm = np.isfinite(fb).all(0) & np.isfinite(then).all(0)
            if a.episodes:
                calm &= (d["done_log"].download()[total[0] - 100:total[0]] & pkg.qrgpu.EP_REASONS).max(0) == 0
            c = np.array([a.cmd_vx, 0.0]) if a.cmd_vx != 0.0 else np.array([1.0, 0.0])
            v = ((fb[4:6] - then[4:6]) / (100 * 0.002) * (c / np.linalg.norm(c))[:, None]).sum(0)
            res.update(speed_along_command_mean=float(v[calm].mean()) if calm.any() else None, speed_robots=int(calm.sum()),
                       yaw_rate_mean=float(((np.arctan2(2 * (fb[0] * fb[3] + fb[1] * fb[2]), 1 - 2 * (fb[2] ** 2 + fb[3] ** 2)) -
                                             np.arctan2(2 * (then[0] * then[3] + then[1] * then[2]), 1 - 2 * (then[2] ** 2 + then[3] ** 2)))[calm] / 0.2).mean())
                       if calm.any() else None)
    if a.fsm:         # where the machine took the robots: reported, not judged
        q = pkg.qrgpu
        state = d["fsm_log"].download()[:, 0]                             # [tick][robot]
        plans, ends = d["plan_log"].download(), (d["done_log"].download() & q.EP_REASONS) != 0
        ends[0] = False                                                   # (the first call's reset_all is no fall)
        loco = state == q.FSM_LOCOMOTION
        first_loco = np.where(loco.any(0), loco.argmax(0), state.shape[0])
        first_end = np.where(ends.any(0), ends.argmax(0), state.shape[0])
        timed = state[20:20 + ticks]
        res.update(fsm=True, fsm_speed=a.fsm_speed, script_ticks=[int(x) for x in press[0]],
                   fsm_state_share={nm: float((timed == v).mean()) for nm, v in (("passive", q.FSM_PASSIVE), ("stand_up", q.FSM_STAND_UP), ("locomotion", q.FSM_LOCOMOTION))},
                   stood_up=int(((plans & q.FSM_PLAN_ACTION_END) != 0).any(0).sum()), entered_locomotion=int(loco.any(0).sum()),
                   fell_before_locomotion=int((first_end < first_loco).sum()))
    if a.fsm_gait:    # which gait the robots ran, and what the stand gait does to the "MPC standing" phase: reported, not judged
        names = ("none_yet", "trot", "advanced_trot", "walk", "stand")
        index = d["gait_log"].download()[20:20 + ticks]                    # [tick][robot]: row 48 of gait_state
        log = d["fsm_log"].download()
        standing = (log[:, 0] == q.FSM_LOCOMOTION) & (log[:, 3] == q.RC_JOY_STAND)      # [tick][robot], warm-up included as swing_legs_commanded is
        # the same robot-ticks under the one batch-wide desc of --fsm: the legs advanced_trot's nominal schedule swings on the clock from the spawn
        dl = (d["done_log"].download() & q.EP_REASONS) != 0
        at = np.arange(dl.shape[0])[:, None]
        tsr = ((at - np.maximum.accumulate(np.where(dl, at, 0), axis=0)).astype(np.float32) * np.float32(0.002)).astype(np.float64)
        full = float(gcfg[0]) / float(gcfg[4])
        nominal = np.stack([np.fmod(float(gcfg[8 + l]) * full + tsr, full) / full >= float(gcfg[4]) for l in range(4)], axis=1)
        res.update(fsm_gait=True, gait_share={nm: float((index == e).mean()) for e, nm in enumerate(names)}, standing_robot_ticks=int(standing.sum()),
                   standing_swing_legs_commanded=int((swing & standing[:, None, :]).sum()),
                   standing_swing_legs_nominal_without=int((nominal & standing[:, None, :]).sum()), gait_flags_seen=int(np.bitwise_or.reduce(d["gait_flags"].download())))
    if a.fsm_mode:    # who ran on which chain, who was solved, and the trot's figures per chain: reported, not judged
        q = pkg.qrgpu
        chain = d["chain_log"].download()                                  # [tick][robot]
        counts = d["count_log"].download()[20:20 + ticks].astype(np.float64)
        on_mpc, on_fb = chain == q.CHAIN_MPC, chain == q.CHAIN_FORCE_BALANCE
        due = d["due_log"].download() != 0
        flagged = pkg.status_flags(tick_log) != 0                           # (the merged status words: each robot's own chain's)
        kd_abad = d["kd_log"].download()[:, 0::3]
        swing_fb = (kd_abad != 0) & on_fb[:, None, :]                       # (a force-balance stance leg carries no gains)
        swing_mpc = swing & on_mpc[:, None, :]
        share = lambda x, m: float(x[m].mean()) if m.any() else None
        res.update(fsm_mode=True, fsm_trot_every=a.fsm_trot_every, script_ticks=[int(x) for x in press[0, :3]],
                   chain_share={nm: float(counts[:, c].sum() / (n * ticks)) for c, nm in enumerate(("none", "mpc", "force_balance"))},
                   route_flagged=float((d["route_log"].download()[20:20 + ticks] != 0).mean()),
                   solved_share=float((due & on_mpc)[20:20 + ticks].mean()),
                   tick_flagged_share_mpc=share(flagged, on_mpc), vmc_flagged_share_force_balance=share(flagged, on_fb),
                   swing_legs_commanded_mpc=int(swing_mpc.sum()), swing_legs_commanded_force_balance=int(swing_fb.sum()),
                   swing_legs_commanded_per_robot_tick_mpc=float(swing_mpc.sum() / max(1, on_mpc.sum())),
                   swing_legs_commanded_per_robot_tick_force_balance=float(swing_fb.sum() / max(1, on_fb.sum())),
                   fb_swing_flags_seen=int(np.bitwise_or.reduce(d["fb_swing_flags"].download())))
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
