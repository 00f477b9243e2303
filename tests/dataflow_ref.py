"""TEST INFRASTRUCTURE -- the trot's command, data-flow and motor-command stages as the reference states them, in numpy, written from the reference's
source (it shares no text with csrc/qr_dataflow.h):
  qrDesiredStateCommand::Update            quadruped/src/controllers/qr_desired_state_command.cpp:164-265 (members and constants: the .hpp)
  the getters the trot's controllers call  qrRobot::GetFootPositionsInWorldFrame qr_robot.cpp:222-230 with invertRigidTransform qr_se3.h:442-449;
                                           TorqueStanceLegController::UpdateFRatio qr_torque_stance_leg_controller.cpp:103-124 (the `contacts`
                                           MPCStanceLegController::Run reads, qr_mpc_stance_leg_controller.cpp:161, :212)
  MPCStanceLegController::GetAction        qr_mpc_stance_leg_controller.cpp:129-156
  qrRaibertSwingLegController::GetAction   qr_swing_leg_controller.cpp:419 (the map), :426-459 (the command loop)
  qrLocomotionController::GetAction        qr_locomotion_controller.cpp:128-147 (the merge)
  the torque tail                          qr_fsm_state_locomotion.cpp:140-157, qr_wbc_locomotion_controller.cpp:205-217, qr_safety_checker.cpp:48-66

Number formats.  Members and locals are float32 unless the reference's expression promotes: F() and D() mark every such step.  The command stage
and the copies are float32 throughout (the one double step: joycmdBodyHeight * 0.85, and the comparison with -0.01).  The foot positions in the
world frame go through Eigen's Quaternion::toRotationMatrix and a 3 x 3 product: foot_world(T, ...) runs them in T = float32 as the reference does,
or T = float64 for the gap that sets the tests' bar.  baseRMat-style products are ((r0 x + r1 y) + r2 z), the project's standing order.

The streams (streams()) are what the host and the GPU tests run over: N_REF robots, T_REF ticks, modes drawn over every RC_MODE, resets in the
middle of the run.  reference() is computed once and shared; callers leave it unchanged.
"""
import functools

import numpy as np

F = np.float32
D = np.float64
N_REF, T_REF = 130, 48
POISON = F(-12345.5)
HARD_CODE, JOY_TROT, JOY_ADVANCED_TROT, JOY_WALK, JOY_STAND, BODY_UP, BODY_DOWN, EXIT = range(8)       # RC_MODE, config/qr_enum_types.h:101-113
SWING, STANCE, EARLY_CONTACT, LOSE_CONTACT, USERDEFINED_SWING = range(5)                              # LegState, :62-68
FE_ROWS, FH_ROWS, SW_ROWS, SV_ROWS, SC_ROWS, MOTOR_CMD_ROWS = 64, 46, 58, 53, 28, 60
EPILOGUE_HIP_COMP, EPILOGUE_CLIP = 1, 2

# qr_desired_state_command.hpp:155, :266, :302-337; robot_params.body_height of config/a1_sim
COMMAND_DESC = dict(dt=0.002, filter_factor=0.02, body_height=0.28, min_velx=-0.15, max_velx=0.2, min_vely=-0.1, max_vely=0.1, min_yawrate=-0.2,
                    max_yawrate=0.2, min_pitch=-0.5, max_pitch=0.5)
# robot->GetMotorKps / GetMotorKdp of config/a1_sim; qr_mpc_stance_leg_controller.cpp:145, :149
MPC_COMMAND_DESC = dict(kp=[100.0] * 12, kd=[1.0, 2.0, 2.0] * 4, stance_kd=3.0, early_contact_abad_kp=100.0, epilogue=0)


def clip(command, minVal, maxVal):
    """utils/qr_algebra.h:57-65 clip<float>, elementwise: a NaN passes"""
    return np.where(command < minVal, minVal, np.where(command > maxVal, maxVal, command)).astype(F)


# ------------------------------------------------------------------------------------------------------------------ qrDesiredStateCommand::Update
def command_update(d, joy, filtered, reset=None):
    """joy [8][n] (joyCmdVx, Vy, Vz, RollRate, PitchRate, YawRate, joycmdBodyHeight, joyCtrlState), filtered [6][n] (filteredVel, filteredOmega),
    reset [n] bool (as constructed: zeros, .cpp:36-37) -> stateDes [12][n], the new filtered [6][n]"""
    joy = np.asarray(joy, F)
    n = joy.shape[1]
    filt = np.array(filtered, F)
    if reset is not None:
        filt[:, np.asarray(reset, bool)] = F(0)
    dt, ff = F(d["dt"]), F(d["filter_factor"])
    mode = joy[7]
    cmd = joy[0:6]                                            # (joyCmdVx, Vy, Vz), (joyCmdRollRate, PitchRate, YawRate)
    a = F(D(1.0) - D(ff))                                      # (1.0 - filterFactor): a double, narrowed to the vector's scalar by Eigen
    lowpass = filt * a + cmd * ff                              # :223-230
    is_filter = (mode == JOY_TROT) | (mode == JOY_ADVANCED_TROT) | (mode == JOY_WALK)
    is_hard = mode == HARD_CODE                                # vDesInBodyFrame, wDesInBodyFrame, unfiltered (:232-233)
    filt = np.where(is_filter, lowpass, np.where(is_hard, cmd, F(0))).astype(F)        # JOY_STAND and the else branch zero the state (:220-221, :241-242)
    s = np.zeros((12, n), F)                                   # stateDes.setZero() (:171)
    s[0] = dt * s[6]; s[1] = dt * s[7]                         # (:245-246: the entries are still zero)
    s[2] = joy[6]
    s[3] = F(0)
    s[4] = clip(filt[4] * dt, F(d["min_pitch"]), F(d["max_pitch"]))
    s[5] = dt * s[11]
    s[6] = clip(filt[0], F(d["min_velx"]), F(d["max_velx"]))
    s[7] = clip(filt[1], F(d["min_vely"]), F(d["max_vely"]))
    s[11] = clip(filt[5], F(d["min_yawrate"]), F(d["max_yawrate"]))
    back = s[6].astype(D) < D(-0.01)                           # :262
    s[2] = np.where(back, (joy[6].astype(D) * D(0.85)).astype(F), s[2])
    return s, filt


def command_rows(s):
    """array -> {row: value}: where the stateDes entries go (include/qrgpu.h)"""
    return dict(fe={0: s[2], 1: s[3], 2: s[4], 3: s[6], 4: s[7], 5: s[11]}, fh={16: s[6], 17: s[7], 18: s[8], 19: s[11], 20: s[2]},
                sv={23: s[6], 24: s[7], 25: s[8], 26: s[11]}, sc={0: s[2], 1: s[6], 2: s[7], 3: s[8], 4: s[9], 5: s[10], 6: s[11]})


# ------------------------------------------------------------------------------------------------------------------ the getters
def quat_to_rot(T, q):
    """Eigen::Quaternion<T>::toRotationMatrix of (w, x, y, z), elementwise over robots"""
    w, x, y, z = (np.asarray(v, T) for v in q)
    two, one = T(2), T(1)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]


def foot_world(T, basePosition, baseOrientation, footPositionsInBaseFrame):
    """invertRigidTransform(basePosition, baseOrientation, footPositionsInBaseFrame): translate(t) then rotate(q) -> R p + t.  [12][n] in, [12][n] out"""
    R = quat_to_rot(T, baseOrientation)
    t = [np.asarray(v, T) for v in basePosition]
    out = []
    for leg in range(4):
        p = [np.asarray(footPositionsInBaseFrame[3 * leg + a], T) for a in range(3)]
        for r in range(3):
            out.append(((R[r][0] * p[0] + R[r][1] * p[1]) + R[r][2] * p[2]) + t[r])
    return np.stack(out)


def contacts(desiredLegState, allowSwitchLegState, legState):
    """UpdateFRatio outside the walk mode, robot not stopped (:109-123)"""
    return ((desiredLegState == STANCE) & (allowSwitchLegState != 0)) | (legState == EARLY_CONTACT)


def trot_inputs(est_in, est_out, rpy, gait_out, gait_state, T=F):
    """-> array -> {row: value} of what the stage writes (include/qrgpu.h); T: the format of the rotation behind fe rows 14-25"""
    quat, rate, angles = est_in[6:10], est_in[10:13], est_in[17:29]
    vWorld, vBase, feetBase, basePosition = est_out[3:6], est_out[6:9], est_out[12:24], est_out[36:39]
    desired, leg, allow = gait_out[8:12], gait_out[12:16], gait_state[20:24]
    fe = {6 + a: basePosition[a] for a in range(3)}
    fe[9] = rpy[2]
    fe.update({10 + a: quat[a] for a in range(4)})
    fw = foot_world(T, basePosition, quat, feetBase)
    fe.update({14 + k: fw[k] for k in range(12)})
    ct = contacts(desired.astype(np.int64), allow, leg.astype(np.int64))
    fe.update({38 + a: ct[a].astype(F) for a in range(4)})
    fh = {21 + k: feetBase[k] for k in range(12)}
    fh.update({33 + a: quat[a] for a in range(4)})
    fh.update({37 + a: rpy[a] for a in range(3)}); fh.update({40 + a: vBase[a] for a in range(3)}); fh.update({43 + a: rate[a] for a in range(3)})
    sw = {36 + a: basePosition[a] for a in range(3)}
    sw.update({39 + a: quat[a] for a in range(4)}); sw.update({43 + a: vWorld[a] for a in range(3)}); sw.update({46 + k: angles[k] for k in range(12)})
    return dict(fe=fe, fh=fh, sw=sw, ei={41 + a: desired[a] for a in range(4)})


# ------------------------------------------------------------------------------------------------------------------ the motor command of the MPC mode
def hip_compensation(motorId):
    """tua_ * pow(-1, (motorId / 3 + 1) % 2) on the abad motors, 0 elsewhere (qr_fsm_state_locomotion.cpp:143-149); tua_ is the float 0.9"""
    return D(F(0.9)) * D((-1.0) ** ((motorId // 3 + 1) % 2)) if motorId % 3 == 0 else D(0)


def mpc_command_robot(d, tau, qdes, computed, desiredLegState, legState, curLegState, allowSwitchLegState, entries):
    """One robot.  tau [12] (the tick's torque: MPC J^T f on the legs outside contact_state, the WBC's on the legs inside, the context's epilogue
    applied), qdes [24] (the swing targets, kept from earlier ticks for legs not recomputed), computed [4] (the legs GetAction's loop ran for this
    tick), entries: the set of legs that already have keys in swingJointAnglesVelocities.  -> motor command [60] = p, Kp, d, Kd, tua; the new set."""
    entries = set(entries)
    for legId in range(4):                                                           # :419: keys 3 legId .. 3 legId + 2
        if computed[legId] != 0:
            entries.add(legId)
    swingJointAnglesVelocities = {3 * legId + i: (qdes[3 * legId + i], qdes[12 + 3 * legId + i], legId) for legId in sorted(entries) for i in range(3)}
    swingAction = {}
    for jointId, (angle, velocity, singleLegId) in swingJointAnglesVelocities.items():      # :431-459, the default branch
        flag = (legState[singleLegId] == SWING or legState[singleLegId] == USERDEFINED_SWING) or \
               (curLegState[singleLegId] == SWING and not allowSwitchLegState[singleLegId])
        if flag:
            swingAction[jointId] = [angle, F(d["kp"][jointId]), velocity, F(d["kd"][jointId]), F(0)]
    stanceAction = {}
    for legId in range(4):                                                           # qr_mpc_stance_leg_controller.cpp:139-153
        for j in range(3):
            motorId = 3 * legId + j
            kp = F(d["early_contact_abad_kp"]) if legState[legId] == EARLY_CONTACT and motorId % 3 == 0 else F(0)
            stanceAction[motorId] = [F(0), kp, F(0), F(d["stance_kd"]), tau[motorId]]
    contact_state = [(desiredLegState[l] == STANCE and bool(allowSwitchLegState[l])) or legState[l] == EARLY_CONTACT for l in range(4)]
    out = np.zeros(60, F)
    for jointId in range(12):                                                        # qr_locomotion_controller.cpp:138-145
        if jointId in swingAction:
            p, Kp, dd, Kd, tua = swingAction[jointId]
            # the tail on a swing command: += compensation (every motor), the WBC's overwrite on a contact_state leg (= tau), the clip; on a stance
            # command all of it is in tau already
            if contact_state[jointId // 3]:
                tua = tau[jointId]
            else:
                t = D(tua)
                if d["epilogue"] & EPILOGUE_HIP_COMP:
                    t = t + hip_compensation(jointId)
                if d["epilogue"] & EPILOGUE_CLIP:
                    t = D(23) if t > 23 else D(-23) if t < -23 else t
                tua = F(t)
        else:
            p, Kp, dd, Kd, tua = stanceAction[jointId]
        out[jointId], out[12 + jointId], out[24 + jointId], out[36 + jointId], out[48 + jointId] = p, Kp, dd, Kd, tua
    return out, entries


def mpc_command(d, tau, qdes, swing_in, gait_out, gait_state, mem, reset=None):
    """[row][n] arrays; mem [n] int (bit per leg), reset [n] bool (Reset() clears the map, qr_swing_leg_controller.cpp:100) -> motor_cmd [60][n], mem [n]"""
    n = tau.shape[1]
    out, mem_out = np.zeros((60, n), F), np.zeros(n, np.int32)
    gi = gait_out.astype(np.int64)
    for r in range(n):
        had = 0 if (reset is not None and reset[r]) else int(mem[r]) & 0xf
        entries = {l for l in range(4) if (had >> l) & 1}
        out[:, r], entries = mpc_command_robot(d, tau[:, r], qdes[:, r], swing_in[0:4, r], gi[8:12, r], gi[12:16, r], gi[16:20, r], gait_state[20:24, r] != 0, entries)
        mem_out[r] = sum(1 << l for l in entries)
    return out, mem_out


# ------------------------------------------------------------------------------------------------------------------ the streams and their reference
def _rpy_to_quat(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])


@functools.lru_cache(maxsize=None)
def streams(n=N_REF, T=T_REF, seed=2024):
    """The three stages' inputs over T ticks of n robots, [T][row][n] float32 unless said: commands beyond every clip, modes over every RC_MODE held
    for a few ticks, attitudes up to 1 rad and all yaws, base positions up to 2 m, every leg state, held schedules, swing legs and leftovers of
    earlier swings; resets of the command state and of the command memory in the middle of the run (tick 0 resets everyone)."""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi, *shape: rng.uniform(lo, hi, shape).astype(F)
    joy = np.zeros((T, 8, n), F)
    joy[:, 0:3] = u(-0.5, 0.5, T, 3, n); joy[:, 3:6] = u(-0.5, 0.5, T, 3, n)
    joy[:, 4] = u(-400, 400, T, n)                                # pitch rate * dt reaches beyond +-0.5
    joy[:, 6] = u(0.24, 0.32, T, n)
    mode = np.zeros((T, n), np.int64)
    mode[0] = rng.integers(0, 8, n)
    for t in range(1, T):
        change = rng.uniform(0, 1, n) < 0.15
        mode[t] = np.where(change, rng.integers(0, 8, n), mode[t - 1])
    mode[:, 0] = JOY_ADVANCED_TROT                                # robot 0 filters from start to end, robot 1 stands
    mode[:, 1] = JOY_STAND
    joy[:, 7] = mode.astype(F)
    hold = rng.uniform(0, 1, (T, 1, n)) < 0.7                     # most commands are held for several ticks, so the filter converges somewhere
    for t in range(1, T):
        joy[t, 0:7] = np.where(hold[t], joy[t - 1, 0:7], joy[t, 0:7])
    cmd_reset = rng.uniform(0, 1, (T, n)) < 0.04; cmd_reset[0] = True; cmd_reset[:, 0] = False; cmd_reset[0, 0] = True
    mem_reset = rng.uniform(0, 1, (T, n)) < 0.04; mem_reset[0] = True
    est_in = u(-2, 2, T, 54, n)
    est_in[:, 6:10] = _rpy_to_quat(rng.uniform(-1, 1, (T, n)), rng.uniform(-1, 1, (T, n)), rng.uniform(-np.pi, np.pi, (T, n))).transpose(1, 0, 2).astype(F)
    est_in[:, 41:45] = POISON
    est_out = u(-2, 2, T, 42, n)
    hip = np.array([0.18, -0.13, -0.27, 0.18, 0.13, -0.27, -0.18, -0.13, -0.27, -0.18, 0.13, -0.27], F)
    est_out[:, 12:24] = hip[None, :, None] + u(-0.1, 0.1, T, 12, n)
    est_out[:, 36:39] = u(-2, 2, T, 3, n); est_out[:, 38] = u(0.1, 0.4, T, n)
    est_out[0, 36:39, 0] = 0; est_in[0, 6:10, 0] = [1, 0, 0, 0]   # one level robot at the origin
    rpy = u(-3.1, 3.1, T, 3, n)
    gait_out = u(0, 1, T, 24, n)
    gait_out[:, 8:12] = rng.choice([SWING, STANCE], (T, 4, n), p=[0.4, 0.6])
    gait_out[:, 12:16] = rng.choice([SWING, STANCE, EARLY_CONTACT, LOSE_CONTACT], (T, 4, n), p=[0.35, 0.4, 0.15, 0.1])
    gait_out[:, 16:20] = rng.choice([SWING, STANCE], (T, 4, n), p=[0.4, 0.6])
    gait_state = u(-1, 1, T, 52, n)
    gait_state[:, 20:24] = (rng.uniform(0, 1, (T, 4, n)) < 0.8).astype(F)
    tau = u(-30, 30, T, 12, n)
    qdes = u(-3, 3, T, 24, n)
    swing_flag = ((gait_out[:, 12:16] == SWING) & (rng.uniform(0, 1, (T, 4, n)) < 0.8)) | (rng.uniform(0, 1, (T, 4, n)) < 0.05)
    out = dict(joy=joy, cmd_reset=cmd_reset, mem_reset=mem_reset, est_in=est_in, est_out=est_out, rpy=rpy, gait_out=gait_out, gait_state=gait_state, tau=tau,
               qdes=qdes, swing_flag=swing_flag.astype(F))
    for v in out.values():
        v.setflags(write=False)
    return out


def fill(rows, n, written):
    """A poisoned [rows][n] array with the rows of `written` ({row: value}) set"""
    a = np.full((rows, n), POISON, F)
    for r, v in written.items():
        a[r] = v
    return a


@functools.lru_cache(maxsize=None)
def reference(epilogue=0, n=N_REF, T=T_REF):
    """The three stages over streams(n, T), tick by tick.  -> dict of [T]... arrays: cmd_state, state_des, fe / fh / sv / sc / sw as the stages leave
    poisoned arrays (sw rows 0-3: the tick's swing flags), est_in after the stage, mem, motor_cmd; fe64: rows 14-25 in float64."""
    S = streams(n, T)
    cd, md = COMMAND_DESC, dict(MPC_COMMAND_DESC, epilogue=epilogue)
    filt, mem = np.full((6, n), POISON, F), np.full(n, 0x7fffffff, np.int32)
    keys = ("cmd_state", "state_des", "fe", "fh", "sv", "sc", "sw", "est_in", "mem", "motor_cmd", "fe64")
    out = {k: [] for k in keys}
    for t in range(T):
        s, filt = command_update(cd, S["joy"][t], filt, S["cmd_reset"][t])
        cr = command_rows(s)
        ti = trot_inputs(S["est_in"][t], S["est_out"][t], S["rpy"][t], S["gait_out"][t], S["gait_state"][t])
        ti64 = trot_inputs(S["est_in"][t], S["est_out"][t], S["rpy"][t], S["gait_out"][t], S["gait_state"][t], T=D)
        sw = fill(SW_ROWS, n, ti["sw"]); sw[0:4] = S["swing_flag"][t]
        cmd, mem = mpc_command(md, S["tau"][t], S["qdes"][t], sw, S["gait_out"][t], S["gait_state"][t], mem, S["mem_reset"][t])
        ei = np.array(S["est_in"][t]); ei[41:45] = np.stack([ti["ei"][41 + a] for a in range(4)])
        vals = (filt, s, fill(FE_ROWS, n, {**cr["fe"], **ti["fe"]}), fill(FH_ROWS, n, {**cr["fh"], **ti["fh"]}), fill(SV_ROWS, n, cr["sv"]),
                fill(SC_ROWS, n, cr["sc"]), sw, ei, mem, cmd, np.stack([ti64["fe"][14 + k] for k in range(12)]))
        for k, v in zip(keys, vals):
            out[k].append(np.array(v))
    out = {k: np.stack(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def foot_world_bar(ref):
    """The bar of fe rows 14-25: 8 x the restatement's own float32-to-float64 gap on the streams, never tighter than 2e-6 (tests/test_observe_host.py)
    -> (gap, bar)"""
    gap = float(np.abs(ref["fe"][:, 14:26].astype(D) - ref["fe64"]).max())
    return gap, max(8.0 * gap, 2e-6)


BARRED = {"fe": slice(14, 26)}


def compare(got, ref, keys, bar, tag=""):
    """got / ref: dicts of [..., row, n] arrays (mem: [..., n]), one shape and type per key.  Bit for bit -- as 32-bit patterns, so a NaN or a -0
    counts -- everywhere but the barred rows, which go under `bar`.  -> the worst distance seen on the barred rows"""
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    worst = 0.0
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, k, g.shape, w.shape, g.dtype, w.dtype)
        if k in BARRED:
            d = np.abs(g[..., BARRED[k], :].astype(D) - w[..., BARRED[k], :].astype(D))
            assert np.isfinite(d).all() and d.max() <= bar, (tag, k, float(d.max()), bar)
            worst = max(worst, float(d.max()))
            g, w = np.delete(g, np.r_[BARRED[k]], axis=-2), np.delete(w, np.r_[BARRED[k]], axis=-2)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, (tag, k, len(bad), bad[:5].tolist())
    return worst
