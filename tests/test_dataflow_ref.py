"""CPU: tests/dataflow_ref.py against facts of the reference that need no kernel."""
import numpy as np

import dataflow_ref as R

F, D = np.float32, np.float64


def _joy(n, mode, vx=0.0, vy=0.0, yaw=0.0, pitch=0.0, height=0.28):
    j = np.zeros((8, n), F)
    j[0], j[1], j[4], j[5], j[6], j[7] = vx, vy, pitch, yaw, height, mode
    return j


def test_filter_converges_geometrically_to_the_clipped_command():
    """filtered_k = c (1 - (1 - f)^k) from zero (:223-230), so stateDes(6) rises geometrically and then sits on the clip; inside the clip it follows the
    filter.  f = 0.02; float32 rounding of 400 steps stays under 1e-5 relative."""
    d = R.COMMAND_DESC
    cmds = np.array([0.1, 0.3, -0.1, -0.4], F)                              # inside, beyond MAX_VELX 0.2, inside, beyond MIN_VELX -0.15
    joy = _joy(4, R.JOY_ADVANCED_TROT)
    joy[0] = cmds; joy[5] = cmds
    filt = np.zeros((6, 4), F)
    a = 1.0 - float(F(d["filter_factor"]))
    for k in range(1, 401):
        s, filt = R.command_update(d, joy, filt)
        want = cmds.astype(D) * (1.0 - a ** k)
        assert np.allclose(filt[0], want, rtol=1e-5, atol=1e-7), k
        assert np.array_equal(s[6], R.clip(filt[0], F(d["min_velx"]), F(d["max_velx"])))
        assert np.array_equal(s[11], R.clip(filt[5], F(d["min_yawrate"]), F(d["max_yawrate"])))
        assert np.all(s[[0, 1, 3, 5, 8, 9, 10]] == 0)                       # dt times entries of the zeroed vector, and the constants
    assert abs(float(filt[0, 0]) - 0.1) < 0.1 * a ** 400 + 1e-6
    assert s[6, 1] == F(0.2) and s[6, 3] == F(-0.15) and s[11, 1] == F(0.2) and s[11, 3] == F(-0.2)
    # the remaining distance shrinks by (1 - f) per tick
    f0 = np.zeros((6, 1), F)
    _, f1 = R.command_update(d, _joy(1, R.JOY_TROT, vx=0.1), f0)
    _, f2 = R.command_update(d, _joy(1, R.JOY_TROT, vx=0.1), f1)
    assert np.isclose((0.1 - float(f2[0, 0])) / (0.1 - float(f1[0, 0])), a, rtol=1e-5)


def test_stand_and_the_other_modes_zero_state_and_output():
    d = R.COMMAND_DESC
    filt = np.full((6, 5), 0.1, F)
    joy = _joy(5, 0, vx=0.1, vy=0.05, yaw=0.1, pitch=3.0)
    joy[7] = [R.JOY_STAND, R.BODY_UP, R.BODY_DOWN, R.EXIT, R.HARD_CODE]
    s, f = R.command_update(d, joy, filt)
    assert np.all(f[:, :4] == 0) and np.all(s[[4, 6, 7, 11], :4] == 0) and np.all(s[2, :4] == F(0.28))
    # HARD_CODE takes the rows unfiltered: vDesInBodyFrame, wDesInBodyFrame
    assert np.array_equal(f[:, 4], joy[0:6, 4]) and s[6, 4] == F(0.1) and s[7, 4] == F(0.05) and s[11, 4] == F(0.1) and s[4, 4] == F(3.0) * F(0.002)
    # a reset is the constructed state: zeros
    s, f = R.command_update(d, _joy(5, R.JOY_WALK), filt, reset=np.array([1, 0, 1, 0, 0], bool))
    assert np.all(f[:, [0, 2]] == 0) and np.all(f[:, [1, 3, 4]] == F(0.1) * F(D(1.0) - D(F(0.02))))


def test_height_is_lowered_when_walking_back():
    """stateDes(2) = joycmdBodyHeight * 0.85 (a double product) where stateDes(6) < -0.01, else joycmdBodyHeight (:247, :262-263)"""
    d = R.COMMAND_DESC
    vx = np.array([-0.15, -0.0101, -0.01, -0.0099, 0.0, 0.2], F)
    joy = _joy(6, R.HARD_CODE, height=0.3)
    joy[0] = vx
    s, _ = R.command_update(d, joy, np.zeros((6, 6), F))
    low = F(D(F(0.3)) * D(0.85))
    assert np.array_equal(s[2], np.array([low, low, F(0.3), F(0.3), F(0.3), F(0.3)], F))  # float32(-0.01) = -0.0099999998 is not below the double -0.01
    assert np.array_equal(s[6], vx)


def test_level_robot_at_the_origin():
    """A level robot: the world-frame foot positions are the base-frame ones plus the base position, exactly; at the origin they are equal."""
    rng = np.random.default_rng(3)
    fp = rng.uniform(-0.3, 0.3, (12, 7)).astype(F)
    bp = rng.uniform(-1, 1, (3, 7)).astype(F); bp[:, 0] = 0
    quat = np.zeros((4, 7), F); quat[0] = 1
    fw = R.foot_world(F, bp, quat, fp)
    assert np.array_equal(fw, fp + np.tile(bp, (4, 1)))
    assert np.array_equal(fw[:, 0], fp[:, 0])
    # a quarter turn about z: x -> y, y -> -x
    quat[0] = quat[3] = np.sqrt(0.5)
    fw = R.foot_world(D, np.zeros((3, 7)), quat.astype(D), fp.astype(D))
    assert np.allclose(fw[0::3], -fp[1::3], atol=1e-7) and np.allclose(fw[1::3], fp[0::3], atol=1e-7) and np.allclose(fw[2::3], fp[2::3], atol=1e-7)
    # the robot of streams() that is level at the origin, through the stage's rows
    S, ref = R.streams(), R.reference()
    assert np.array_equal(ref["fe"][0, 14:26, 0], S["est_out"][0, 12:24, 0])


def test_contacts_follow_update_f_ratio():
    des = np.array([R.STANCE, R.STANCE, R.SWING, R.SWING, R.STANCE])
    allow = np.array([1, 0, 1, 1, 0], F)
    leg = np.array([R.STANCE, R.STANCE, R.SWING, R.EARLY_CONTACT, R.EARLY_CONTACT])
    assert R.contacts(des, allow, leg).tolist() == [True, False, False, True, True]


def test_motor_command_merge_on_a_hand_built_case():
    """Leg 0 EARLY_CONTACT, leg 1 swinging (computed this tick), leg 2 with an entry from an earlier swing but a false flag, leg 3 in stance."""
    d = dict(R.MPC_COMMAND_DESC)
    tau = np.arange(1, 13).astype(F)
    qdes = np.concatenate([0.1 * np.arange(1, 13), -0.1 * np.arange(1, 13)]).astype(F)
    computed = [0, 1, 0, 0]
    desired = [R.STANCE, R.SWING, R.STANCE, R.STANCE]
    leg = [R.EARLY_CONTACT, R.SWING, R.STANCE, R.STANCE]
    cur = [R.SWING, R.SWING, R.STANCE, R.STANCE]
    allow = [True, True, True, True]
    out, entries = R.mpc_command_robot(d, tau, qdes, computed, desired, leg, cur, allow, entries={2})
    assert entries == {1, 2}
    cmd = out.reshape(5, 12)                                                 # p, Kp, d, Kd, tua
    assert np.array_equal(cmd[:, 0], [0, 100, 0, 3, 1]) and np.array_equal(cmd[:, 1], [0, 0, 0, 3, 2]) and np.array_equal(cmd[:, 2], [0, 0, 0, 3, 3])
    for j, kd in zip((3, 4, 5), (1, 2, 2)):
        assert np.array_equal(cmd[:, j], np.array([qdes[j], 100, qdes[12 + j], kd, 0], F))
    for j in range(6, 12):
        assert np.array_equal(cmd[:, j], np.array([0, 0, 0, 3, tau[j]], F))
    # the held schedule: curLegState SWING while allowSwitchLegState is false makes leg 2's entry a command again -- it re-emits its last targets
    cur2, allow2 = [R.SWING, R.SWING, R.SWING, R.STANCE], [True, True, False, True]
    out, _ = R.mpc_command_robot(d, tau, qdes, computed, desired, leg, cur2, allow2, entries={2})
    assert np.array_equal(out.reshape(5, 12)[:, 6], np.array([qdes[6], 100, qdes[18], 1, 0], F))
    # no entry, no swing command, whatever the leg state says
    out, entries = R.mpc_command_robot(d, tau, qdes, [0, 0, 0, 0], desired, leg, cur, allow, entries=set())
    assert entries == set() and np.array_equal(out.reshape(5, 12)[:, 3], np.array([0, 0, 0, 3, 4], F))
    # the epilogue on a swing command: -+0.9 on the abad (legs 0, 2 minus, legs 1, 3 plus), nothing on the other motors; tau is taken as it comes
    out, _ = R.mpc_command_robot(dict(d, epilogue=3), tau, qdes, computed, desired, leg, cur, allow, entries={2})
    assert np.array_equal(out.reshape(5, 12)[4], np.array([1, 2, 3, 0.9, 0, 0, 7, 8, 9, 10, 11, 12], F))
    # a swing-command leg that is in contact_state keeps the WBC's torque (leg 1: legState SWING, desired STANCE)
    out, _ = R.mpc_command_robot(dict(d, epilogue=3), tau, qdes, computed, [R.STANCE] * 4, leg, cur, allow, entries=set())
    assert np.array_equal(out.reshape(5, 12)[:, 3], np.array([qdes[3], 100, qdes[15], 1, tau[3]], F))


def test_hip_compensation_signs():
    """pow(-1, (leg + 1) % 2): FR, RR -0.9; FL, RL +0.9 (qr_fsm_state_locomotion.cpp:146)"""
    assert [float(F(R.hip_compensation(m))) for m in (0, 3, 6, 9)] == [float(F(-0.9)), float(F(0.9)), float(F(-0.9)), float(F(0.9))]
    assert all(R.hip_compensation(m) == 0 for m in (1, 2, 4, 5, 7, 8, 10, 11))
