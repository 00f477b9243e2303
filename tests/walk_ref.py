"""TEST INFRASTRUCTURE -- the walk gait generator as an explicit state machine in numpy float32 with Python ints for the states, one robot at
a time, written from the reference line by line: qrWalkGaitGenerator's configuration-file constructor (quadruped/src/gait/
qr_walk_gait_generator.cpp:65-193), its Update (:202-288), qrGaitGenerator::Reset (quadruped/include/quadruped/gait/qr_gait.h:76-87) and the walk
branch of TorqueStanceLegController::UpdateFRatio (quadruped/src/controllers/balance_controller/qr_torque_stance_leg_controller.cpp:125-168).
Every arithmetic step is one operation in the reference's format (the file is `using namespace std`, so fmod and abs are the float overloads;
`(phase - ratio) / (1.0 - ratio)` is evaluated in double and narrowed; `stateRatio < 0.01` is a double compare) and fmod is exact, so
qr_walk_gait_kernel and oracle/qr_oracle_walk.cpp are expected to agree with it bit for bit.

What the members are when, in the reference:
  * the constructor drops queue entries with a ratio below 0.01, sums the kept ratios into accumStateRatioQue, takes trueSwingStartPhaseInSwingCycle
    as the sum in front of true_swing, and starts a leg whose initial state is SWING at the sub-state its initial phase falls in -- with
    (initialLegPhase - dutyFactor) / dutyFactor, the reference's division, not by 1 - dutyFactor.  Then Reset(0).
  * Reset(t): normalizedPhase = 0, cur / last / leg / desired state = initialLegState.  NOTHING else: stateIndexOfLegs, detectedLegState,
    detectedEventTickPhase, moveBasePhase and phaseInFullCycle survive a Reset in mid-run.
  * moveBasePhase, detectedLegState, detectedEventTickPhase, phaseInFullCycle (and trueSwingStartPhaseInSwingCycle without a true_swing entry)
    have no initialiser and are read before some paths write them; they are taken as 0 here, the project's reading (include/qrgpu.h).

ONE FORK.  When a tick is longer than a sub-state, "go into next state process" (:253-258) can step past the end of stateSwitchQue, where the
reference reads whatever lies behind its vector.  The project clamps the index to the last entry (qr_oracle_walk.cpp, qr_walk_gait_kernel);
the model takes the project's reading, in next_state_index() and nowhere else, and counts how often it did (self.clamped).
"""
import numpy as np

_f = np.float32
_d = np.float64
SWING, STANCE, EARLY_CONTACT, LOSE_CONTACT = 0, 1, 2, 3
LOAD_FORCE, UNLOAD_FORCE, FULL_STANCE, TRUE_SWING = 5, 6, 7, 8


class WalkGaitGenerator:
    """cfg26 = workload.walk_cfg(): stance_duration[4], duty_factor[4], initial_leg_phase[4], initial_leg_state[4],
    contact_detection_phase_threshold, n_states, state_switch[4], state_ratio[4]."""

    def __init__(self, cfg26):
        c = np.asarray(cfg26, _f)
        self.stanceDuration, self.dutyFactor, self.initialLegPhase = c[0:4].copy(), c[4:8].copy(), c[8:12].copy()
        self.initialLegState = [int(v) for v in c[12:16]]
        self.contactDetectionPhaseThreshold = c[16]
        stateSwitchStrQue = [int(v) for v in c[18:18 + int(c[17])]]
        stateRatioQue_ = c[22:22 + int(c[17])]
        self.stateSwitchQue, self.stateRatioQue = [], []
        standRatioInSwing = _f(0)
        self.trueSwingStartPhaseInSwingCycle = _f(0)
        for id_, item in enumerate(stateSwitchStrQue):
            if _d(stateRatioQue_[id_]) < _d(0.01):
                continue
            if item in (FULL_STANCE, LOAD_FORCE, UNLOAD_FORCE):
                standRatioInSwing = standRatioInSwing + stateRatioQue_[id_]
            elif item == TRUE_SWING:
                self.trueSwingStartPhaseInSwingCycle = standRatioInSwing
            else:
                raise ValueError("received invalid value!")
            self.stateSwitchQue.append(item)
            self.stateRatioQue.append(stateRatioQue_[id_])
        self.accumStateRatioQue = [_f(0)]
        for r in self.stateRatioQue:
            self.accumStateRatioQue.append(self.accumStateRatioQue[-1] + r)
        if not abs(self.accumStateRatioQue[-1] - _f(1)) < _f(1e-4):
            raise ValueError("not vaild ratio definition")
        self.fullCyclePeriod = np.zeros(4, _f); self.swingDuration = np.zeros(4, _f)
        self.stateIndexOfLegs = [0] * 4
        for legId in range(4):
            self.fullCyclePeriod[legId] = self.stanceDuration[legId] / self.dutyFactor[legId]
            self.swingDuration[legId] = self.fullCyclePeriod[legId] - self.stanceDuration[legId]
            if self.initialLegState[legId] == SWING:
                pahseInSwingCycle = (self.initialLegPhase[legId] - self.dutyFactor[legId]) / self.dutyFactor[legId]
                i = 0
                while i < len(self.stateRatioQue) and pahseInSwingCycle > self.accumStateRatioQue[i]:
                    i += 1
                self.stateIndexOfLegs[legId] = max(i - 1, 0)
        # members without an initialiser: the project's zeros
        self.phaseInFullCycle = np.zeros(4, _f)
        self.detectedLegState = [0] * 4
        self.detectedEventTickPhase = np.zeros(4, _f)
        self.moveBasePhase = _f(0)
        self.clamped = 0
        self.Reset(0.0)

    def Reset(self, currentTime):
        # qrGaitGenerator::Reset (qr_gait.h:76-87); qrWalkGaitGenerator::Reset adds nothing
        self.resetTime = _f(currentTime)
        self.lastTime = _f(currentTime)
        self.normalizedPhase = np.zeros(4, _f)
        self.curLegState = list(self.initialLegState)
        self.lastLegState = list(self.curLegState)
        self.legState = list(self.curLegState)
        self.desiredLegState = list(self.curLegState)

    def next_state_index(self, stateIdx):
        """stateIdx += 1 of :254 -- THE FORK: past the queue's end the reference is undefined, the project stays on the last entry."""
        stateIdx += 1
        if stateIdx > len(self.stateSwitchQue) - 1:
            stateIdx = len(self.stateSwitchQue) - 1
            self.clamped += 1
        return stateIdx

    def Update(self, currentTime, contact, stop=False):
        """One control tick: contact [4] = robot->GetFootContact(), stop = robot->stop.  -> out [41] float32 in the kernel's row order."""
        currentTime = _f(currentTime)
        self.lastLegState = list(self.curLegState)
        contactState = [bool(v != 0) for v in contact]
        one = _d(1.0)
        for legId in range(4):
            if not stop or (stop and self.curLegState[legId] == SWING):
                self.curLegState[legId] = self.desiredLegState[legId]
            augmentedTime = self.initialLegPhase[legId] * self.fullCyclePeriod[legId] + currentTime
            self.phaseInFullCycle[legId] = np.fmod(augmentedTime, self.fullCyclePeriod[legId]) / self.fullCyclePeriod[legId]
            phase = self.phaseInFullCycle[legId]
            ratio = self.dutyFactor[legId]
            if phase <= self.dutyFactor[legId]:
                if self.curLegState[legId] != STANCE:
                    self.stateIndexOfLegs[legId] = 0
                self.desiredLegState[legId] = STANCE
                self.legState[legId] = self.desiredLegState[legId]
                self.normalizedPhase[legId] = phase / ratio
            else:
                self.desiredLegState[legId] = SWING
                self.legState[legId] = self.desiredLegState[legId]
                self.normalizedPhase[legId] = _f(_d(phase - ratio) / (one - _d(ratio)))
            if self.desiredLegState[legId] == SWING:
                stateIdx = self.stateIndexOfLegs[legId]
                startRatioPoint = self.accumStateRatioQue[stateIdx]
                endRatioPoint = self.accumStateRatioQue[stateIdx + 1]
                phaseInSwingCycle = _f(_d(phase - self.dutyFactor[legId]) / (one - _d(self.dutyFactor[legId])))
                if phaseInSwingCycle <= endRatioPoint and phaseInSwingCycle >= startRatioPoint:
                    self.desiredLegState[legId] = self.stateSwitchQue[stateIdx]
                    self.normalizedPhase[legId] = (phaseInSwingCycle - startRatioPoint) / (endRatioPoint - startRatioPoint)
                else:
                    stateIdx = self.next_state_index(stateIdx)
                    self.desiredLegState[legId] = self.stateSwitchQue[stateIdx]
                    self.stateIndexOfLegs[legId] = stateIdx
                    self.normalizedPhase[legId] = (phaseInSwingCycle - self.accumStateRatioQue[stateIdx]) / self.stateRatioQue[stateIdx]
                if phaseInSwingCycle < self.trueSwingStartPhaseInSwingCycle:
                    self.moveBasePhase = phaseInSwingCycle / self.trueSwingStartPhaseInSwingCycle
                else:
                    self.moveBasePhase = _f(1.0)
            if self.desiredLegState[legId] != STANCE:
                self.detectedLegState[legId] = SWING
            else:
                self.detectedLegState[legId] = STANCE
            if self.normalizedPhase[legId] < self.contactDetectionPhaseThreshold:
                continue
            if self.desiredLegState[legId] == TRUE_SWING and contactState[legId]:
                self.detectedLegState[legId] = EARLY_CONTACT
                self.detectedEventTickPhase[legId] = phase
            elif self.desiredLegState[legId] == STANCE and not contactState[legId]:
                self.detectedLegState[legId] = LOSE_CONTACT
                self.detectedEventTickPhase[legId] = phase
        return self.out()

    def UpdateFRatio(self):
        """The walk branch (robot->stop not set): -> contacts [4], fMinRatio [4], fMaxRatio [4]"""
        contacts, fMinRatio, fMaxRatio = np.zeros(4, _f), np.zeros(4, _f), np.zeros(4, _f)
        for legId in range(4):
            desiredLegState, detectedLegState = self.desiredLegState[legId], self.detectedLegState[legId]
            phase = self.normalizedPhase[legId]
            fMinRatio[legId] = _f(0.001)
            if detectedLegState == STANCE or detectedLegState == LOSE_CONTACT:
                contacts[legId] = 1
                fMaxRatio[legId] = _f(10.0)
            elif detectedLegState == EARLY_CONTACT:
                contacts[legId] = 1
                tempRatio = abs(phase - _f(0.8))
                fMaxRatio[legId] = _f(10.0) * min(_f(0.01), tempRatio)
            elif desiredLegState == LOAD_FORCE:
                contacts[legId] = 1
                fMaxRatio[legId] = _f(10.0) * max(_f(0.001), phase)
            elif desiredLegState == UNLOAD_FORCE:
                contacts[legId] = 1
                phase = phase / (_f(3.0) / _f(4.0))
                fMaxRatio[legId] = _f(10.0) * max(_f(0.001), _f(1.0) - phase)
            elif desiredLegState == TRUE_SWING:
                contacts[legId] = 0
                fMaxRatio[legId] = _f(0.002)
            elif desiredLegState == FULL_STANCE:
                contacts[legId] = 1
                fMaxRatio[legId] = _f(10.0)
            else:
                raise ValueError("[stance leg controller] This leg state does not exist.")
        return contacts, fMinRatio, fMaxRatio

    def out(self):
        i = lambda v: np.asarray(v, _f)
        contacts, fMinRatio, fMaxRatio = self.UpdateFRatio()
        return np.concatenate([self.phaseInFullCycle, self.normalizedPhase, i(self.desiredLegState), i(self.legState), i(self.curLegState),
                               i(self.detectedLegState), self.detectedEventTickPhase, i([self.moveBasePhase]), contacts, fMinRatio, fMaxRatio]).astype(_f)

    def state33(self):
        """The kernel's walk_state rows (include/qrgpu.h): cur, desired, leg, detected, stateIndexOfLegs, phase, normalizedPhase,
        detectedEventTickPhase [4 each], moveBasePhase."""
        i = lambda v: np.asarray(v, _f)
        return np.concatenate([i(self.curLegState), i(self.desiredLegState), i(self.legState), i(self.detectedLegState), i(self.stateIndexOfLegs),
                               self.phaseInFullCycle, self.normalizedPhase, self.detectedEventTickPhase, i([self.moveBasePhase])]).astype(_f)


def run(cfg26, time, contact, stop=None, reset=None, want_state=False):
    """One robot from construction: time [T], contact [T][4], stop [T] (robot->stop), reset [T] (non-zero: Reset() on the running generator before
    that tick's Update).  -> out [T][41] (, state [T][33], times the fork's clamp was taken)"""
    g = WalkGaitGenerator(cfg26)
    T = len(time)
    out = np.zeros((T, 41), _f); st = np.zeros((T, 33), _f)
    for k in range(T):
        if reset is not None and reset[k]:
            g.Reset(time[k])
        out[k] = g.Update(time[k], contact[k], bool(stop[k]) if stop is not None else False)
        if want_state:
            st[k] = g.state33()
    return (out, st, g.clamped) if want_state else out


# ----------------------------------------------------------------------------- families (tests/test_walk_ref.py, tests/test_gpu_walk.py)
N_ROBOTS = 65
FAMILIES = ("yaml", "swing_start", "robot_stop", "reset", "long_step", "late_clock", "threshold_0", "threshold_1")
SUB_STATES = (FULL_STANCE, UNLOAD_FORCE, TRUE_SWING, LOAD_FORCE)
STOP_LENGTH = 70                          # 0.56 s at 8 ms: longer than the two 0.5 s sub-states of the YAML gait


def contacts(n, ticks, seed):
    """Per-robot contact streams [ticks][n][4] (float32 0/1): contact, with six gaps of 5 .. 80 ticks per leg at random places (some fall into
    stance: LOSE_CONTACT; the feet that stay down through true swing: EARLY_CONTACT); robot 0 lifts no foot at all."""
    rng = np.random.default_rng(seed)
    c = np.ones((ticks, n, 4), _f)
    for _ in range(6):
        k0 = rng.integers(0, max(ticks - 80, 1), (n, 4)); ln = rng.integers(5, 80, (n, 4))
        for r in range(1, n):
            for l in range(4):
                c[k0[r, l]:k0[r, l] + ln[r, l], r, l] = 0
    return c


def _first(mask, start=0):
    k = np.nonzero(mask[start:])[0]
    assert k.size
    return start + int(k[0])


def family(pkg, name, n=N_ROBOTS):
    """-> dict(cfg, time [T] float32, contact [T][n][4], stop [T] int32, reset [T] int32, marks) of one of FAMILIES; marks are the ticks the
    family was built around (tests/test_walk_ref.py asserts what happens there)."""
    W = pkg.workload
    cfg, T, dt, t0 = W.walk_cfg(), 1500, 0.008, 3.0                     # 12 s of the YAML gait's 10 s cycle; Update takes absolute time
    swing_start = dict(stance_duration=1.5, duty_factor=0.75, initial_leg_phase=(0.9, 0.1, 0.6, 0.35), initial_leg_state=(0, 1, 1, 1),
                       state_switch=(7, 5, 8, 6), state_ratio=(0.005, 0.2, 0.4, 0.4))      # a leg inside its swing quarter, a dropped sub-state, another order
    step = None
    marks = {}
    if name == "swing_start":
        cfg, T, dt, t0 = W.walk_cfg(**swing_start), 1100, 0.002, 0.0        # (a 2 s cycle)
    elif name == "long_step":
        # a 0.123 s cycle whose sub-states last 6, 9, 9, 6 ms, on a 4 ms clock: one 100 ms step out of a load_force sub-state lands in the next
        # cycle's swing quarter with the index still on the last entry -- the fork
        cfg, T, dt, t0 = W.walk_cfg(stance_duration=0.0925), 600, 0.004, 0.0
    elif name == "late_clock":
        T, dt, t0 = 900, 0.004, 1000.0                                   # float32 time in steps of 6e-5 s
        step = np.full(T, dt); step[450] = 0.100
    elif name.startswith("threshold"):
        cfg, T = W.walk_cfg(contact_detection_phase_threshold=float(name[-1])), 600
    elif name in ("robot_stop", "reset"):
        T = 700
    elif name != "yaml":
        raise KeyError(name)
    step = np.full(T, dt) if step is None else step
    stop = np.zeros(T, np.int32); reset = np.zeros(T, np.int32)
    ones = np.ones((T, 4), _f)
    clock = lambda s: (t0 + np.concatenate([[0.0], np.cumsum(s[1:])])).astype(_f)
    if name == "long_step":
        nominal = run(cfg, clock(step), ones)
        k = _first((nominal[:, 8] == LOAD_FORCE) & (nominal[:, 4] > 0.3), 100)
        step[k + 1] = 0.100
        marks["long_step"] = k + 1
    time = clock(step)
    if name == "robot_stop":
        # four windows of robot->stop, each opening while some leg is in another sub-state of its swing quarter
        nominal = run(cfg, time, ones)
        k = 0
        for s in SUB_STATES:
            k = _first((nominal[:, 8:12] == s).any(axis=1), k) + 3
            stop[k:k + STOP_LENGTH] = 1
            marks[s] = k
            k += STOP_LENGTH + 10
    if name == "reset":
        nominal = run(cfg, time, ones)
        # (the YAML gait always has one leg in its swing quarter: the two resets meet it in different sub-states)
        marks["in_true_swing"] = _first((nominal[:, 8:12] == TRUE_SWING).any(axis=1), 50) + 20
        marks["in_load_force"] = _first((nominal[:, 8:12] == LOAD_FORCE).any(axis=1), marks["in_true_swing"] + 400) + 5
        reset[[marks["in_true_swing"], marks["in_load_force"]]] = 1
    return dict(name=name, cfg=cfg, time=time, contact=contacts(n, T, 0x3A00 + FAMILIES.index(name)), stop=stop, reset=reset, marks=marks)


_cache = {}


def expected(pkg, name):
    """-> (family, out [n][T][41], state [n][T][33], clamped [n]) computed once per session and shared by the tests; nobody writes into it."""
    if name not in _cache:
        f = family(pkg, name)
        runs = [run(f["cfg"], f["time"], f["contact"][:, r], f["stop"], f["reset"], want_state=True) for r in range(f["contact"].shape[1])]
        _cache[name] = (f, np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]), np.array([r[2] for r in runs]))
    return _cache[name]
