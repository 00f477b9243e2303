"""TEST INFRASTRUCTURE -- the open-loop gait generator as an explicit state machine in numpy float32, one robot at a time, written from the
reference line by line (quadruped/src/gait/qr_openloop_gait_generator.cpp:126-249 Update / Schedule, :77-123 Reset,
quadruped/include/quadruped/gait/qr_gait.h:76-87 qrGaitGenerator::Reset, :263-294 the members' initialisers), for legs with a non-zero duty
factor.  Every arithmetic step is one float32 operation in the reference's order and fmod is exact, so qr_gait_kernel and
oracle/qr_oracle_gait.cpp are expected to agree with it bit for bit.

What the members are when, in the reference:
  * construction: gaitCycle = 0, cumDt = 0, firstSwing = firstStance = false, swingTimeRemaining = 0 (member initialisers); phaseInFullCycle
    and allowSwitchLegState have none and are written before they are read (taken as 0 / true here); then Reset(0).
  * Reset(t): resetTime = lastTime = t, normalizedPhase = 0, cur / last / leg / desired state = initialLegState, contactStartPhase = 0.
    NOTHING else: gaitCycle, cumDt, firstSwing, firstStance, swingTimeRemaining and phaseInFullCycle survive a Reset in mid-run.
  * initStateRadioInCycle is dutyFactor for either initial state (:107-116 of the configuration-file Reset, the one the controllers use).
"""
import numpy as np

_f = np.float32
SWING, STANCE, EARLY_CONTACT = 0, 1, 2


class GaitGenerator:
    """cfg19 = workload.gait_cfg(): stance_duration[4], duty_factor[4], initial_leg_phase[4], initial_leg_state[4],
    contact_detection_phase_threshold, wait_time, advanced_trot."""

    def __init__(self, cfg19):
        c = np.asarray(cfg19, _f)
        self.stanceDuration, self.dutyFactor, self.initialLegPhase = c[0:4].copy(), c[4:8].copy(), c[8:12].copy()
        self.initialLegState = [int(v) for v in c[12:16]]
        self.contactDetectionPhaseThreshold, self.waitTime, self.advancedTrot = c[16], c[17], bool(c[18] != 0)
        # member initialisers (qr_gait.h:263-294, qr_openloop_gait_generator.h:100)
        self.gaitCycle = 0
        self.cumDt = _f(0)
        self.firstSwing = [False] * 4
        self.firstStance = [False] * 4
        self.swingTimeRemaining = np.zeros(4, _f)
        self.phaseInFullCycle = np.zeros(4, _f)
        self.allowSwitchLegState = [True] * 4
        self.Reset(0.0)

    def Reset(self, currentTime):
        # qrOpenLoopGaitGenerator::Reset (:92-118), duty factor != 0
        self.fullCyclePeriod = np.zeros(4, _f); self.swingDuration = np.zeros(4, _f); self.initStateRadioInCycle = np.zeros(4, _f)
        for legId in range(4):
            self.fullCyclePeriod[legId] = self.stanceDuration[legId] / self.dutyFactor[legId]
            self.swingDuration[legId] = self.fullCyclePeriod[legId] - self.stanceDuration[legId]
            self.initStateRadioInCycle[legId] = self.dutyFactor[legId]
        # qrGaitGenerator::Reset (qr_gait.h:76-87)
        self.resetTime = _f(currentTime)
        self.lastTime = _f(currentTime)
        self.normalizedPhase = np.zeros(4, _f)
        self.curLegState = list(self.initialLegState)
        self.lastLegState = list(self.curLegState)
        self.legState = list(self.curLegState)
        self.desiredLegState = list(self.curLegState)
        self.contactStartPhase = np.zeros(4, _f)

    def Schedule(self, currentTime, contactState):
        if self.resetTime + self.fullCyclePeriod[0] < self.timeSinceReset:
            self.resetTime = self.timeSinceReset
            self.gaitCycle += 1
        self.timeSinceReset = self.timeSinceReset - self.resetTime
        self.allowSwitchLegState = [True] * 4
        if self.advancedTrot:
            for legId in range(4):
                if self.curLegState[legId] == SWING and self.desiredLegState[legId] == STANCE and not contactState[legId]:
                    self.allowSwitchLegState[legId] = False
            if sum(self.allowSwitchLegState) < 4:
                dt_ = currentTime - self.lastTime
                self.cumDt = self.cumDt + dt_
                if self.cumDt > self.waitTime:
                    self.allowSwitchLegState = [True] * 4
                    return
                self.resetTime = self.resetTime + dt_
            else:
                self.cumDt = _f(0)

    def Update(self, currentTime, contact, stop=False):
        """One control tick: contact [4] = robot->GetFootContact(), stop = robot->stop.  -> out [24] float32 as the oracle's gait_run:
        phaseInFullCycle, normalizedPhase, desiredLegState, legState, curLegState, swingTimeRemaining."""
        currentTime = _f(currentTime)
        contactState = [bool(v != 0) for v in contact]
        self.timeSinceReset = currentTime
        self.Schedule(currentTime, contactState)
        one = _f(1)
        for legId in range(4):
            if sum(self.allowSwitchLegState) == 4:
                if not stop or (stop and self.lastLegState[legId] == SWING):
                    self.lastLegState[legId] = self.curLegState[legId]
                    self.curLegState[legId] = self.desiredLegState[legId]
                augmentedTime = self.initialLegPhase[legId] * self.fullCyclePeriod[legId] + self.timeSinceReset
                self.phaseInFullCycle[legId] = np.fmod(augmentedTime, self.fullCyclePeriod[legId]) / self.fullCyclePeriod[legId]
                ratio = self.initStateRadioInCycle[legId]
                if self.phaseInFullCycle[legId] < ratio:
                    self.desiredLegState[legId] = STANCE
                    self.normalizedPhase[legId] = self.phaseInFullCycle[legId] / ratio
                else:
                    self.desiredLegState[legId] = SWING
                    self.normalizedPhase[legId] = (self.phaseInFullCycle[legId] - ratio) / (one - ratio)
                    if self.curLegState[legId] == STANCE:
                        self.firstSwing[legId] = True
                        self.contactStartPhase[legId] = 0
                        self.firstStance[legId] = False
                        self.swingTimeRemaining[legId] = self.swingDuration[legId]
                    else:
                        self.firstSwing[legId] = False
                        self.swingTimeRemaining[legId] = self.swingDuration[legId] * (one - self.normalizedPhase[legId])
                if self.legState[legId] == EARLY_CONTACT and self.desiredLegState[legId] == SWING:
                    continue
                else:
                    self.legState[legId] = self.desiredLegState[legId]
                if self.normalizedPhase[legId] < self.contactDetectionPhaseThreshold:
                    continue
                if self.legState[legId] == SWING and contactState[legId]:
                    self.legState[legId] = EARLY_CONTACT
                    self.contactStartPhase[legId] = self.phaseInFullCycle[legId] - one
                if self.curLegState[legId] == SWING and (self.legState[legId] == EARLY_CONTACT or self.legState[legId] == STANCE):
                    self.firstStance[legId] = True
                    self.firstSwing[legId] = False
        self.lastTime = currentTime
        return self.out()

    def out(self):
        return np.concatenate([self.phaseInFullCycle, self.normalizedPhase, np.asarray(self.desiredLegState, _f), np.asarray(self.legState, _f),
                               np.asarray(self.curLegState, _f), self.swingTimeRemaining]).astype(_f)

    def state48(self):
        """Rows 0-47 of the kernel's gait_state (include/qrgpu.h; rows 48-51 are spare): resetTime, lastTime, cumDt, gaitCycle, then per leg
        cur, last, desired, legState, allow, firstSwing, firstStance, phaseInFullCycle, normalizedPhase, contactStartPhase, swingTimeRemaining."""
        i = lambda v: np.asarray(v, _f)
        return np.concatenate([i([self.resetTime, self.lastTime, self.cumDt, self.gaitCycle]), i(self.curLegState), i(self.lastLegState),
                               i(self.desiredLegState), i(self.legState), i(self.allowSwitchLegState), i(self.firstSwing), i(self.firstStance),
                               self.phaseInFullCycle, self.normalizedPhase, self.contactStartPhase, self.swingTimeRemaining]).astype(_f)


def run(cfg19, time, contact, stop=None, reset=None, want_state=False):
    """One robot from construction: time [T], contact [T][4], stop [T] (robot->stop), reset [T] (non-zero: Reset(0) on the running generator
    before that tick's Update).  -> out [T][24] (, state [T][48])."""
    g = GaitGenerator(cfg19)
    T = len(time)
    out = np.zeros((T, 24), _f); st = np.zeros((T, 48), _f)
    for k in range(T):
        if reset is not None and reset[k]:
            g.Reset(0.0)
        out[k] = g.Update(time[k], contact[k], bool(stop[k]) if stop is not None else False)
        if want_state:
            st[k] = g.state48()
    return (out, st) if want_state else out


# ----------------------------------------------------------------------------- configurations (tests/test_gait_ref.py, tests/test_gpu_gait.py)
N_ROBOTS = 65
TICKS = 700
DT = 0.002
RESET_TICKS = (400, 600)      # Reset(0) in mid-run: before the first clock restart (tick 417) and after it
STOP_TICK = 300
CONFIGS = ("default", "plain_trot", "robot_stop", "swing_start", "reset", "irregular_clock")


def contacts(n, ticks, cfg19, time, seed):
    """Per-robot contact streams [ticks][n][4] (float32 0/1) around the nominal schedule of cfg19 at the given clock: late touch-downs (no contact
    for the first 3-12 % of a stance phase: the hold of Schedule), early touch-downs (contact in the last 5-30 % of a swing: EARLY_CONTACT),
    a little of both on most robots; robot 0 follows the nominal schedule exactly."""
    rng = np.random.default_rng(seed)
    c = np.asarray(cfg19, np.float64)
    full = c[0] / c[4]
    late = rng.uniform(0.03, 0.12, (n, 4)) * (rng.uniform(0, 1, (n, 4)) < 0.4)
    early = 1.0 - rng.uniform(0.05, 0.30, (n, 4)) * (rng.uniform(0, 1, (n, 4)) < 0.4)
    late[0] = 0; early[0] = 1.0
    out = np.zeros((ticks, n, 4), _f)
    for k in range(ticks):
        for l in range(4):
            ph = np.fmod(c[8 + l] * full + float(time[k]), full) / full
            out[k, :, l] = (ph >= late[:, l]) if ph < c[4] else (ph > early[:, l])
    return out


def configuration(pkg, name, n=N_ROBOTS, ticks=TICKS):
    """-> dict(cfg, time [T] float32, contact [T][n][4], stop [T] int32, reset [T] int32) of one of CONFIGS."""
    W = pkg.workload
    cfg = W.gait_cfg(wait_time=0.06)
    time = (np.arange(ticks) * DT).astype(_f)
    stop = np.zeros(ticks, np.int32); reset = np.zeros(ticks, np.int32)
    seed = 0x6A00 + CONFIGS.index(name)
    if name == "plain_trot":
        cfg = W.gait_cfg(wait_time=0.06, advanced_trot=False)
    elif name == "robot_stop":
        stop[STOP_TICK:] = 1
    elif name == "swing_start":
        cfg = W.gait_cfg(stance_duration=0.3, duty_factor=0.5, initial_leg_state=(0, 1, 1, 0), wait_time=0.06)
    elif name == "reset":
        reset[list(RESET_TICKS)] = 1
    elif name == "irregular_clock":
        step = np.full(ticks, DT)
        step[np.random.default_rng(seed).uniform(0, 1, ticks) < 0.1] = 0.004      # occasional 4 ms steps
        step[350] = 0.100                                                        # one step longer than wait_time
        time = np.concatenate([[0.0], np.cumsum(step[1:])]).astype(_f)
    elif name != "default":
        raise KeyError(name)
    return dict(cfg=cfg, time=time, contact=contacts(n, ticks, cfg, time, seed), stop=stop, reset=reset)
