"""CPU: the numpy restatement of the stance front-end and motor commands (tests/stance_ref.py), which the GPU kernels are held to, against
independent statements: scipy's rotations, closed forms written out by hand, workload.make_vmc_batch's pitched control frame, and the
force-balance oracle, which must accept what it builds."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import stance_ref as R

f32, f64 = np.float32, np.float64
N = 257


# ---- rotation helpers against scipy, float64 ---------------------------------------------------------------------------------------------
def _quats(n, seed):
    q = np.random.default_rng(seed).normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def test_rotation_helpers_against_scipy():
    rng = np.random.default_rng(1)
    for q in _quats(50, 2):
        S = Rotation.from_quat([q[1], q[2], q[3], q[0]])
        M = S.as_matrix()
        p, t = rng.normal(size=3), rng.normal(size=3)
        assert np.allclose(R.quat_to_rot(f64, *q), M, atol=1e-14)
        assert np.allclose(R.base_rmat(f64, q), M, atol=1e-14)
        assert np.allclose(R.invert_rigid_transform(f64, q, t, p), M @ p + t, atol=1e-14)
        assert np.allclose(R.rigid_transform(f64, q, t, p), M.T @ (p - t), atol=1e-14)
        assert np.allclose(R.transform_vec_by_quat(f64, q, p), M @ p, atol=1e-14)
        assert np.allclose(R.transform_vec_by_quat(f64, R.quat_inverse(f64, q), p), M.T @ p, atol=1e-14)
    for _ in range(50):
        rpy = np.array([rng.uniform(-3, 3), rng.uniform(-1.4, 1.4), rng.uniform(-3, 3)])
        active = Rotation.from_euler("ZYX", rpy[::-1]).as_matrix()                 # Rz(yaw) Ry(pitch) Rx(roll)
        Mc = np.array(R.rpy_to_rotmat(f64, rpy))                                   # the coordinate-transform product Rx Ry Rz: its transpose
        assert np.allclose(Mc, active.T, atol=1e-14)
        back = R.rotmat_t_to_rpy(f64, Mc.T)                                        # rotationMatrixToRPY(rpyToRotMat(rpy))
        assert np.allclose(back, rpy, atol=1e-9), (rpy, back)
        assert np.allclose(back, Rotation.from_matrix(active).as_euler("ZYX")[::-1], atol=1e-9)


def test_rotation_to_rpy_every_branch():
    """rotationMatrixToQuaternion's four branches (trace > 0 and each dominant diagonal) give the same rotation back."""
    for rpy in ([0.1, 0.2, 0.3], [3.0, 0.1, 0.2], [0.1, 0.2, 3.0], [3.0, 0.2, 3.0], [0.2, 1.3, 3.1]):
        Mc = np.array(R.rpy_to_rotmat(f64, rpy))
        back = R.rotmat_t_to_rpy(f64, Mc.T)
        assert np.allclose(R.rpy_to_rotmat(f64, back), Mc, atol=1e-9), rpy


# ---- CoM adjuster ------------------------------------------------------------------------------------------------------------------------
def test_com_adjuster_closed_form():
    rng = np.random.default_rng(3)
    s2 = math.sqrt(2.0)
    for _ in range(40):
        ls = rng.integers(0, 4, 4); ph = rng.uniform(0, 1, 4); feet = rng.normal(size=(4, 3))
        w = []
        for l in range(4):
            if ls[l] in (1, 3):
                w.append(0.5 * (math.erf(ph[l] / s2) + math.erf((1 - ph[l]) / s2)))
            else:
                w.append(0.5 * (2 + math.erf(-ph[l] / s2) + math.erf((ph[l] - 1) / s2)))
        assert np.allclose(R.com_weights(f64, ls, ph), w, atol=1e-15)
        verts = []
        for l, (cw, ccw) in enumerate(R.ADJ):
            vcw = w[l] * feet[l] + (1 - w[l]) * feet[cw]
            vccw = w[l] * feet[l] + (1 - w[l]) * feet[ccw]
            verts.append((w[l] * feet[l] + w[ccw] * vccw + w[cw] * vcw) / (w[l] + w[ccw] + w[cw]))
        want = np.mean(verts, axis=0)
        assert np.allclose(R.com_adjust(f64, ls, ph, feet), want, atol=1e-14)
        assert np.allclose(R.com_adjust(f32, ls, ph, feet.astype(f32)), want, atol=2e-6)


def test_com_adjuster_equal_phase_is_mean_of_feet():
    rng = np.random.default_rng(4)
    for ph in (0.0, 0.3, 0.5, 1.0):
        feet = rng.normal(size=(4, 3))
        got = R.com_adjust(f64, [1, 1, 1, 1], [ph] * 4, feet)
        assert np.allclose(got, feet.mean(0), atol=1e-14), ph
    assert R.ADJ == ((2, 1), (0, 3), (3, 0), (1, 2))


# ---- hand-derived cases: identity attitude on PLANE --------------------------------------------------------------------------------------
def level_robot(mode, seed):
    """One robot with identity attitude on level ground: est_in, est_out, ground, rpy, gait_out, gait_state, cmd"""
    rng = np.random.default_rng(seed)
    ei, eo, gr = np.zeros(54, f32), np.zeros(42, f32), np.zeros(32, f32)
    ei[6] = 1.0
    ei[10:13] = rng.uniform(-0.3, 0.3, 3)
    eo[6:9] = rng.uniform(-0.3, 0.3, 3)
    eo[12:24] = [0.18, -0.13, -0.28, 0.18, 0.13, -0.28, -0.18, -0.13, -0.28, -0.18, 0.13, -0.28]
    eo[36:39] = [0.4, -0.2, 0.26]
    eo[39] = 0.265
    gr[9] = 1.0
    gr[13:22] = np.eye(3).reshape(-1); gr[22:31] = np.eye(3).reshape(-1)
    if mode == R.WALK:
        go = np.zeros(41, f32)
        go[8:12] = 1; go[20:24] = 1; go[28] = 0.4; go[29:33] = 1; go[33:37] = 0.001; go[37:41] = 10.0
    else:
        go = np.zeros(24, f32)
        go[4:8] = 0.4; go[8:12] = 1; go[12:16] = 1
    gs = np.zeros(52, f32); gs[20:24] = 1
    cmd = np.zeros(28, f32)
    cmd[0] = 0.29; cmd[1:4] = [0.3, -0.1, 0.0]; cmd[4:7] = [0.05, -0.02, 0.2]
    cmd[7:13] = [0.38, -0.21, 0.25, 0, 0, 0]; cmd[13:19] = [0.45, -0.18, 0.28, 0, 0, 0]; cmd[19:25] = [0.1, 0.0, 0.02, 0.01, -0.02, 0.03]
    cmd[25:28] = [0.01, -0.02, 0.03]
    return ei, eo, gr, np.zeros(3, f32), go, gs, cmd


def pd(d, des, cur):
    a = [d.kp[k] * (float(des[k]) - float(cur[k])) + d.kd[k] * (float(des[6 + k]) - float(cur[6 + k])) for k in range(6)]
    return np.clip(a, d.min_ddq, d.max_ddq)


def run_one(T, d, args, st=None, **kw):
    st = np.zeros(1, f32) if st is None else st
    return R.stance_update(T, d, kw.get("current_time", 0.0), kw.get("stop", False), kw.get("reset", True), *args, st)


def check_hand(d, args, cur, des, contacts=(1, 1, 1, 1), world=0.0):
    want = pd(d, des, cur)
    for T, tol in ((f64, 1e-12), (f32, 2e-5)):
        vin, ratio, out = run_one(T, d, args)
        assert np.allclose(out[0:12], cur, atol=tol), (T, out[0:12], cur)
        assert np.allclose(out[12:24], des, atol=tol), (T, out[12:24], des)
        assert np.allclose(out[24:30], want, atol=tol * 400), (T, out[24:30], want)
        assert np.array_equal(vin[12:18], out[24:30]) and np.array_equal(vin[0:12], T(1) * args[1][12:24].astype(T))
        assert list(vin[18:22]) == list(contacts) and out[30] == sum(contacts) and out[32] == world
    return vin, ratio, out


def test_hand_velocity_level():
    d = R.Desc(R.VELOCITY, terrain=0)
    a = level_robot(R.VELOCITY, 11)
    ei, eo, cmd = a[0], a[1], a[6]
    cur = [0, 0, eo[38], 0, 0, 0, *eo[6:9], *ei[10:13]]
    des = [0, 0, 0.27, 0, 0, 0, *cmd[1:4], *cmd[4:7]]
    vin, ratio, out = check_hand(d, a, cur, des)
    assert list(vin[22:37]) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, f64(f32(9.8)), 0, 0, 1]
    assert list(ratio) == [f64(f32(0.01))] * 4 + [10.0] * 4
    a[4][8:12] = [1, 0, 0, 1]                                                  # VELOCITY: contact = desiredLegState is STANCE, whatever allow says
    a[5][20:24] = 0
    check_hand(d, a, cur, des, contacts=(1, 0, 0, 1))


def test_hand_advanced_trot_level_both_frames():
    a = level_robot(R.ADVANCED_TROT, 12)
    ei, eo, cmd = a[0], a[1], a[6]
    d = R.Desc(R.ADVANCED_TROT, terrain=0, force_in_world=0, desired_speed=[0.2, 0.1, 0.0], desired_twisting_speed=0.3)
    cur = [0, 0, eo[38], 0, 0, 0, *eo[6:9], *ei[10:13]]
    des = [0, 0, float(eo[38]) * 0.7 + float(f32(0.27)) * 0.3, 0, 0, 0, f32(0.2), f32(0.1), 0, 0, 0, f32(0.3)]
    check_hand(d, a, cur, des)
    d = R.Desc(R.ADVANCED_TROT, terrain=0, force_in_world=1)
    des = [eo[36], eo[37], cmd[0], 0, 0, 0, *cmd[1:4], *cmd[4:7]]
    vin, _, _ = check_hand(d, a, cur, des, world=1.0)
    assert list(vin[22:37]) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, f64(f32(9.8)), 0, 0, 1]
    # contacts: (desired STANCE and allowSwitchLegState) or legState EARLY_CONTACT
    a[5][20:24] = [1, 0, 1, 0]; a[4][8:12] = [1, 1, 0, 0]; a[4][12:16] = [1, 1, 2, 0]
    check_hand(d, a, cur, des, contacts=(1, 0, 1, 0), world=1.0)
    # front feet close to the body slow the command down: scale = max(0.1, footX / 0.1)
    a[1][12] = 0.05
    des[6:9] = [float(f32(0.05)) / float(f32(0.1)) * float(v) for v in cmd[1:4]]
    check_hand(d, a, cur, des, contacts=(1, 0, 1, 0), world=1.0)


def test_hand_advanced_trot_pitch_clip_and_height_compensation():
    d = R.Desc(R.ADVANCED_TROT, terrain=0, force_in_world=1)
    for pitch, want, bump in ((0.05, 0.0, True), (0.3, 0.3, False), (0.7, 0.5, False), (-0.3, -0.3, True), (-0.7, -0.5, True)):
        a = level_robot(R.ADVANCED_TROT, 13)
        a[2][7] = pitch
        a[6][3] = 0.04                                                        # v_z command above 0.01
        _, _, out = run_one(f64, d, a)
        assert out[16] == f64(f32(want)), pitch
        comp = f64(f32(0.04)) * abs(f64(f32(want)) / 0.5) if bump else 0.0
        assert abs(out[14] - (f64(a[6][0]) + comp)) < 1e-15, (pitch, out[14])


def test_hand_position_level():
    d = R.Desc(R.POSITION, terrain=1, desired_speed=[0.15, -0.05, 0.0])
    a = level_robot(R.POSITION, 14)
    ei, eo, cmd = a[0], a[1], a[6]
    feet = eo[12:24].reshape(4, 3).astype(f64)
    cur = [0, 0, eo[38], 0, 0, 0, *eo[6:9], *ei[10:13]]
    des = [feet[:, 0].mean(), feet[:, 1].mean(), f32(0.27), *cmd[25:28], f32(0.15), f32(-0.05), 0, 0, 0, 0]
    check_hand(d, a, cur, des)


def test_hand_walk_level():
    d = R.Desc(R.WALK, terrain=0)
    a = level_robot(R.WALK, 15)
    ei, eo, go, cmd = a[0], a[1], a[4], a[6]
    go[8] = 6; go[20] = 0                                                      # leg 0 unloads: the generator's moveBasePhase applies
    ph = float(go[28])
    pose = [ph * float(cmd[13 + k]) + (1.0 - ph) * float(cmd[7 + k]) for k in range(6)]
    cur = [*eo[36:39], 0, 0, 0, *eo[6:9], *ei[10:13]]
    des = [*pose, *cmd[19:25]]
    vin, ratio, out = check_hand(d, a, cur, des, world=1.0)
    assert out[31] == go[28]
    go[8] = 1; go[20] = 1                                                      # every leg in stance: moveBasePhase stays 1, the pose is poseDest
    des = [*cmd[13:19], *cmd[19:25]]
    _, _, out = check_hand(d, a, cur, des, world=1.0)
    assert out[31] == 1.0


def test_walk_rotation_error_branch():
    """dq.tail(3) = robotR rpy(dR), ddq.tail(3) = robotR ((R_des w_des)^ - (robotR^T w_cur)^)v (:456-468) against scipy."""
    d = R.Desc(R.WALK, terrain=0)
    a = level_robot(R.WALK, 16)
    a[3][:] = [0.2, -0.3, 0.8]
    a[6][10:13] = [0.05, 0.1, 0.6]; a[6][16:19] = [0.05, 0.1, 0.6]
    q = Rotation.from_euler("ZYX", a[3][::-1].astype(f64)).as_quat()
    a[0][6:10] = [q[3], q[0], q[1], q[2]]
    _, _, out = run_one(f64, d, a)
    cr, dr = a[3].astype(f64), a[6][10:13].astype(f64)
    robotR = Rotation.from_euler("ZYX", cr[::-1]).as_matrix()                  # rpyToRotMat(rpy)^T
    desRT = Rotation.from_euler("ZYX", dr[::-1]).as_matrix().T
    e = Rotation.from_matrix((desRT @ robotR).T).as_euler("ZYX")[::-1]
    dq = robotR @ e
    wcur = out[9:12]
    dw = robotR @ (desRT @ a[6][22:25].astype(f64) - robotR.T @ wcur)
    want = np.clip(np.array(d.kp[3:]) * dq + np.array(d.kd[3:]) * dw, d.min_ddq[3:], d.max_ddq[3:])
    assert np.allclose(out[27:30], want, atol=1e-9), (out[27:30], want)
    assert np.allclose(wcur, Rotation.from_quat(q).as_matrix() @ a[0][10:13].astype(f64), atol=1e-7)


# ---- stop, height memory -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_stop_branch(mode):
    d = R.Desc(mode, pose_reset_time=1.0)
    a = level_robot(mode, 20 + mode)
    if mode == R.WALK:
        a[4][8:12] = [8, 6, 5, 1]; a[4][20:24] = [0, 0, 0, 1]; a[4][29:33] = [0, 1, 1, 1]; a[4][37:41] = [0.002, 3.0, 4.0, 10.0]
    else:
        a[4][8:12] = [0, 1, 0, 1]
    for T in (f32, f64):
        vin, ratio, out = run_one(T, d, a, stop=True, current_time=3.0)
        assert list(vin[18:22]) == [1, 1, 1, 1] and out[30] == 4 and out[31] == 1
        assert list(ratio) == [T(f32(0.01))] * 4 + [T(10)] * 4
    if mode == R.WALK:                                                         # the pose runs on wall time: (3 - 1) / 5 of the way, then capped at 1
        _, _, out = run_one(f64, d, a, stop=True, current_time=3.0)
        ph = f64(f32(2.0) / f32(5.0))
        assert np.allclose(out[12:15], ph * a[6][13:16].astype(f64) + f64(f32(1.0 - ph)) * a[6][7:10].astype(f64), atol=1e-7)
        _, _, out = run_one(f64, d, a, stop=True, current_time=9.0)
        assert np.array_equal(out[12:15], a[6][13:16].astype(f64))
        cmd = R.stance_command(d, True, vin, out, np.arange(12, dtype=f32))
        assert np.array_equal(cmd[48:60], np.arange(12, dtype=f32)) and np.all(cmd[36:48] == f32(0.5) * np.array(d.motor_kd, f32))


def test_height_memory():
    """ADVANCED_TROT in the control frame on a slope reads heightInControlFrame; a NaN (no stance foot) keeps the previous value, a reset
    starts from bodyHeight."""
    d = R.Desc(R.ADVANCED_TROT, terrain=3, force_in_world=0)
    a = level_robot(R.ADVANCED_TROT, 30)
    st = np.zeros(1, f32)
    a[1][39] = np.nan
    _, _, out = run_one(f32, d, a, st=st, reset=True)
    assert st[0] == f32(0.28) and out[2] == f32(0.28)
    a[1][39] = 0.251
    _, _, out = run_one(f32, d, a, st=st, reset=False)
    assert st[0] == f32(0.251) and out[2] == f32(0.251)
    a[1][39] = np.nan
    for _ in range(2):
        _, _, out = run_one(f32, d, a, st=st, reset=False)
        assert st[0] == f32(0.251) and out[2] == f32(0.251) and np.isfinite(out).all()
    _, _, out = run_one(f32, d, a, st=st, reset=True)
    assert st[0] == f32(0.28)


# ---- the motor command ---------------------------------------------------------------------------------------------------------------------
def test_motor_command_cases():
    tau = np.arange(1, 13, dtype=f32)
    z12 = np.zeros(12, f32)
    for mode in (0, 1, 3):
        cmd = R.stance_command(R.Desc(mode), False, None, None, tau)
        assert np.array_equal(cmd[:48], np.zeros(48, f32)) and np.array_equal(cmd[48:], tau)
    d = R.Desc(R.WALK)
    vin, so = np.zeros(37, f32), np.zeros(33, f32)
    vin[18:22] = [1, 0, 0, 0]; so[30] = 3; so[31] = 0.5                         # leg 0 in contact; the others: N < 4 and the base still moving
    cmd = R.stance_command(d, False, vin, so, tau)
    assert np.array_equal(cmd[0:36], np.zeros(36, f32)) and np.array_equal(cmd[48:], tau)
    assert list(cmd[36:48]) == [0.5, 1.0, 1.0] + [0.0] * 9
    so[31] = 0.8                                                               # moveBasePhase past 0.7: the swing legs get nothing
    cmd = R.stance_command(d, False, vin, so, tau)
    assert np.array_equal(cmd[48:], np.concatenate([tau[:3], np.zeros(9, f32)]))
    cmd = R.stance_command(d, True, vin, so, tau)                              # ... unless the robot is stopped
    assert np.array_equal(cmd[48:], tau)
    sq = np.arange(100, 124, dtype=f32)
    cmd = R.stance_command(d, False, vin, so, tau, sq, np.array([0, 1, 0, 0], f32))
    assert list(cmd[3:6]) == [103, 104, 105] and list(cmd[15:18]) == [100, 100, 100] and list(cmd[27:30]) == [115, 116, 117]
    assert list(cmd[39:42]) == [1, 2, 2] and list(cmd[51:54]) == [0, 0, 0] and np.array_equal(cmd[48:51], tau[:3])
    assert np.array_equal(z12, R.stance_command(d, False, vin, so, tau, sq, np.ones(4, f32))[48:])


# ---- vmc_in against the workload's pitched control frame and the oracle -----------------------------------------------------------------------
def test_pitched_vmc_in_matches_workload(pkg):
    n = 32
    want, _ = pkg.workload.make_vmc_batch(n, seed=41, sloped=1.0)
    d = R.Desc(R.VELOCITY, terrain=3)
    for i in range(n):
        pitch = math.atan2(-f64(want[i, 34]), f64(want[i, 36]))
        a = level_robot(R.VELOCITY, 40)
        Rc = np.array(R.rpy_to_rotmat(f64, [0.0, pitch, 0.0])).T
        a[2][7] = pitch
        a[2][9:13] = R._quat_of_r(Rc)
        a[2][13:22] = Rc.reshape(-1); a[2][22:31] = Rc.T.reshape(-1)
        vin, _, _ = run_one(f32, d, a)
        # both sides round cos / sin of the same pitch to float32 once or twice: an ulp of 1 on the rotation, of 9.8 on gravity
        assert np.abs(vin[22:31] - want[i, 22:31]).max() <= 2 * 2.0 ** -24, i
        assert np.abs(vin[31:34] - want[i, 31:34]).max() <= 2 * 2.0 ** -21, i
        assert np.abs(vin[34:37] - want[i, 34:37]).max() <= 2 * 2.0 ** -24, i


@pytest.mark.parametrize("mode,fiw", [(0, 1), (1, 1), (2, 1), (3, 1), (3, 0)])
def test_oracle_accepts_vmc_in(pkg, oracle, mode, fiw):
    """All-stance robots on level ground: the oracle's QP takes the restatement's vmc_in (and ratio, for the world-frame overload) and
    returns finite forces that carry the robot."""
    W = pkg.workload
    vcfg, geom = W.vmc_cfg("a1"), pkg.model_desc("a1")[:3]
    d = R.Desc(mode, terrain=0 if mode != 1 else 1, force_in_world=fiw)
    for seed in range(4):
        a = level_robot(mode, 50 + seed)
        vin, ratio, out = run_one(f32, d, a)
        assert list(vin[18:22]) == [1, 1, 1, 1]
        q = np.tile(np.array([0.0, 0.9, -1.8], f32), 4)
        f, t, x, st, rc = oracle.vmc_solve(vcfg, geom, vin, q, ratio if out[32] == 1 else None)
        assert rc == 0 and np.isfinite(f).all() and np.isfinite(t).all()
        assert 0.3 * 13 * 9.8 < -f.reshape(4, 3)[:, 2].sum() < 3 * 13 * 9.8


# ---- the seeded batches of the GPU test ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_input_generator_stays_under_exclusion_cap(case):
    mode, terrain, fiw, seed = R.CASES[case]
    d = R.Desc(mode, terrain=terrain, force_in_world=fiw)
    inp = R.make_inputs(N, mode, seed)
    ex = R.excluded(d, inp)
    assert ex.sum() <= R.EXCLUDE_CAP * N, (case, int(ex.sum()))
    assert np.isnan(inp["est_out"][:, 39]).sum() > N // 10
    assert np.abs(inp["rpy"][:, :2]).max() <= 0.5 and np.abs(inp["ground"][:, 7]).max() <= 0.6
    go = inp["gait_out"]
    if mode == R.WALK:
        assert set(np.unique(go[:, 8:12])) == {1, 5, 6, 7, 8} and set(np.unique(go[:, 20:24])) == {0, 1, 2, 3}
    else:
        assert set(np.unique(go[:, 8:12])) == {0, 1} and set(np.unique(go[:, 12:16])) == {0, 1, 2, 3}
    # the float64 reading alone: finite, and the float32 one stays close to it on the robots that are compared
    st = np.zeros((N, 1), f32)
    v64, r64, o64 = R.run_batch(f64, d, inp, st, reset=True)
    v32, r32, o32 = R.run_batch(f32, d, inp, st.copy(), reset=True)
    assert np.isfinite(o64).all() and np.isfinite(v64).all()
    assert np.abs(o32 - o64)[~ex].max() < 1e-3


def test_desc_defaults_match_library(pkg):
    pkg._build.build()
    for mode in range(4):
        lib, ref = pkg.stance_desc(mode), R.Desc(mode)
        for name in ("mode", "terrain", "force_in_world", "desired_height", "desired_twisting_speed", "body_height", "pose_reset_time"):
            assert getattr(lib, name) == f32(getattr(ref, name)), (mode, name)
        for name in ("kp", "kd", "max_ddq", "min_ddq", "desired_speed", "motor_kp", "motor_kd"):
            assert list(getattr(lib, name)) == [f32(v) for v in getattr(ref, name)], (mode, name)
    assert C.sizeof(pkg.qrgpu.stance_desc_struct) == 4 * (3 + 24 + 7 + 24)
