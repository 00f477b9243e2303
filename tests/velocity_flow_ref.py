"""TEST INFRASTRUCTURE -- the data-flow stage of the force-balance trot (LocomotionMode::VELOCITY_LOCOMOTION) as the reference states it, in numpy,
written from the reference's source (it shares no text with csrc/qr_velocity_flow.h):
  qrRaibertSwingLegController::Reset       quadruped/src/controllers/qr_swing_leg_controller.cpp:100 (swingJointAnglesVelocities.clear())
  qrRaibertSwingLegController::Update      :218-229 (the default branch: which legs go into swingFootIds)
  qrRaibertSwingLegController::GetAction   :256-258 (GetMotorAngles, GetBaseRollPitchYawRate()(2), GetEstimatedVelocity), :271-276 (dR and robotBaseR: the
                                           identity where terrainType < 2, else baseRInControlFrame and baseRMat), :294 (stateDes.segment(6, 3), stateDes(11)),
                                           :306 (normalizedPhase), :408-424 (every leg of swingFootIds gets its three keys in the map), :431-459 with the
                                           VELOCITY case :446-448 (an entry is commanded while desiredLegState == SWING)
  qrRobotVelocityEstimator::Update         quadruped/src/estimators/qr_robot_velocity_estimator.cpp:126-131: estimatedVelocity ends in the base frame and is
                                           what robot->baseVelocityInBaseFrame receives -- rows 6-8 of est_out (include/qrgpu.h)

Everything here is a copy, a comparison or a set operation: the stage has no arithmetic, so every written row is compared bit for bit.  The map is kept
per robot as a Python set of leg ids, one robot after the other, as the reference keeps one map per controller.

The streams (streams()) are what the host and the GPU tests run over: N_REF robots, T_REF ticks, leg states over every LegState value, allowSwitchLegState
both ways, a scalar reset and masked resets in the middle of the run.  reference(terrain) is computed once per terrain and shared; callers leave it unchanged.
"""
import functools

import numpy as np

F = np.float32
N_REF, T_REF = 130, 48
POISON = F(-12345.5)
MEM_POISON = np.int32(0x7fffffff)
SWING, STANCE, EARLY_CONTACT, LOSE_CONTACT, USERDEFINED_SWING = range(5)                              # LegState, config/qr_enum_types.h:62-68
PLANE, PLUM_PILES, STAIRS, SLOPE, ROUGH = range(5)                                                    # TerrainType, :86-92
SV_ROWS, EST_IN_ROWS = 53, 54
SCALAR_RESETS = (0, 17)                                                                               # ticks at which the call's scalar reset is 1


def swing_foot_ids(legState, allowSwitchLegState):
    """:218-229 for one robot: legState [4], allowSwitchLegState [4] -> the list swingFootIds"""
    ids = []
    for legId in range(4):
        tempState = legState[legId]
        if (tempState == STANCE and allowSwitchLegState[legId]) or tempState == EARLY_CONTACT:
            continue
        ids.append(legId)
    return ids


def robot_tick(swingFootIds, desiredLegState, entries, reset):
    """One robot, one tick of the map's keys: Reset() if asked, GetAction's loop over swingFootIds, the command loop's VELOCITY flag.
    entries: the set of legs with keys before the tick -> (the set after, the legs whose entry is commanded)"""
    entries = set() if reset else set(entries)
    for legId in swingFootIds:                                         # :419
        entries.add(legId)
    commanded = [singleLegId for singleLegId in sorted(entries) if desiredLegState[singleLegId] == SWING]        # :446-448, :456
    return entries, commanded


def velocity_inputs(terrain, est_in, est_out, ground_out, gait_out, gait_state, state_des, mem, reset):
    """[row][n] arrays of one tick; mem [n] int (bit per leg), reset [n] bool -> dict: sv {row: value} (swing_vel_in), ei {row: value} (est_in rows
    41-44), mem [n] int32, flag [4][n]"""
    n = est_in.shape[1]
    normalizedPhase, desiredLegState, legState = gait_out[4:8], gait_out[8:12], gait_out[12:16]
    allowSwitchLegState = gait_state[20:24] != 0
    in_ids, flag, mem_out = np.zeros((4, n), F), np.zeros((4, n), F), np.zeros(n, np.int32)
    for r in range(n):
        ids = swing_foot_ids(legState[:, r], allowSwitchLegState[:, r])
        had = {l for l in range(4) if (int(mem[r]) >> l) & 1}
        entries, commanded = robot_tick(ids, desiredLegState[:, r], had, bool(reset[r]))
        in_ids[ids, r] = 1
        flag[commanded, r] = 1
        mem_out[r] = sum(1 << l for l in entries)
    sv = {legId: in_ids[legId] for legId in range(4)}
    sv.update({4 + legId: normalizedPhase[legId] for legId in range(4)})
    sv.update({20 + a: est_out[6 + a] for a in range(3)})              # baseVelocity = stateEstimator->GetEstimatedVelocity(), base frame
    sv[23] = est_in[12]                                                # yawDot = GetBaseRollPitchYawRate()(2)
    sv.update({24: state_des[6], 25: state_des[7], 26: state_des[8], 27: state_des[11]})
    if terrain < 2:                                                    # horizontal terrain: dR.setIdentity(), robotBaseR.setIdentity()
        eye = np.eye(3, dtype=F).reshape(9)
        sv.update({28 + k: np.full(n, eye[k], F) for k in range(9)})
        sv.update({37 + a: np.full(n, F(1 if a == 0 else 0), F) for a in range(4)})
    else:                                                              # dR = baseRInControlFrame, robotBaseR = baseRMat (of the base quaternion)
        sv.update({28 + k: ground_out[22 + k] for k in range(9)})
        sv.update({37 + a: est_in[6 + a] for a in range(4)})
    sv.update({41 + k: est_in[17 + k] for k in range(12)})             # currentJointAngles = GetMotorAngles()
    return dict(sv=sv, ei={41 + a: desiredLegState[a] for a in range(4)}, mem=mem_out, flag=flag)


@functools.lru_cache(maxsize=None)
def streams(n=N_REF, T=T_REF, seed=4711):
    """The stage's inputs over T ticks of n robots, [T][row][n] float32 unless said.  scalar_reset [T] bool (the call's scalar), mask_reset [T][n] bool
    (the binding's mask, on the other ticks)."""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi, *shape: rng.uniform(lo, hi, shape).astype(F)
    est_in = u(-2, 2, T, EST_IN_ROWS, n)
    est_in[:, 41:45] = POISON
    est_out = u(-2, 2, T, 42, n)
    ground_out = u(-1, 1, T, 32, n)
    gait_out = u(0, 1, T, 24, n)
    gait_out[:, 8:12] = rng.choice([SWING, STANCE], (T, 4, n), p=[0.4, 0.6])
    gait_out[:, 12:16] = rng.choice([SWING, STANCE, EARLY_CONTACT, LOSE_CONTACT, USERDEFINED_SWING], (T, 4, n), p=[0.2, 0.5, 0.15, 0.1, 0.05])
    gait_state = u(-1, 1, T, 52, n)
    gait_state[:, 20:24] = (rng.uniform(0, 1, (T, 4, n)) < 0.75).astype(F)
    state_des = u(-0.5, 0.5, T, 12, n)
    scalar_reset = np.zeros(T, bool); scalar_reset[list(SCALAR_RESETS)] = True
    mask_reset = rng.uniform(0, 1, (T, n)) < 0.05
    mask_reset[scalar_reset] = False
    out = dict(est_in=est_in, est_out=est_out, ground_out=ground_out, gait_out=gait_out, gait_state=gait_state, state_des=state_des, scalar_reset=scalar_reset,
               mask_reset=mask_reset)
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
def reference(terrain, n=N_REF, T=T_REF):
    """The stage over streams(n, T), tick by tick, the memory starting at MEM_POISON.  -> dict of [T]... arrays: sv (as the stage leaves a poisoned
    swing_vel_in), est_in (after the stage, written in place), mem, flag"""
    S = streams(n, T)
    mem = np.full(n, MEM_POISON, np.int32)
    out = dict(sv=[], est_in=[], mem=[], flag=[])
    for t in range(T):
        reset = S["mask_reset"][t] | S["scalar_reset"][t]
        o = velocity_inputs(terrain, S["est_in"][t], S["est_out"][t], S["ground_out"][t], S["gait_out"][t], S["gait_state"][t], S["state_des"][t], mem, reset)
        mem = o["mem"]
        ei = np.array(S["est_in"][t]); ei[41:45] = np.stack([o["ei"][41 + a] for a in range(4)])
        for k, v in (("sv", fill(SV_ROWS, n, o["sv"])), ("est_in", ei), ("mem", mem), ("flag", o["flag"])):
            out[k].append(np.array(v))
    out = {k: np.stack(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def same_bits(got, want, tag=""):
    """Bit for bit, as 32-bit patterns: a NaN or a -0 counts"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (tag, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
    assert bad.size == 0, (tag, len(bad), bad[:5].tolist())
