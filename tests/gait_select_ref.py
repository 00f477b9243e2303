"""TEST INFRASTRUCTURE -- the open-loop gait generator with the gait chosen at Reset, and the stage clock that restarts where a mask says, in numpy:
what qrgpu_gait_select_update_batch and qrgpu_stage_clock_batch (csrc/qr_gait.h) are expected to reproduce bit for bit.

  * SelectGenerator: gait_ref.GaitGenerator whose Reset takes a config row and re-reads the parameters first, as qrOpenLoopGaitGenerator::Reset does
    from the block of `gait` (quadruped/src/gait/qr_openloop_gait_generator.cpp:77-123): stanceDuration, dutyFactor, initialLegState, initialLegPhase,
    contactDetectionPhaseThreshold, waitTime (and, here, the advanced-trot hold, which the reference tests on the `gait` string itself); then
    fullCyclePeriod, swingDuration, initStateRadioInCycle; then qrGaitGenerator::Reset.  Everything else survives.
  * run: one robot over per-tick selection, reset level and clock.  The selection counts only at a reset.
  * stage_clock: the three-line clock.
  * schedule: the mixed schedules of tests/test_gait_select_host.py and tests/test_gpu_gait_select.py.
"""
import numpy as np

import gait_ref as G

_f = np.float32
CONSTRUCT, LIVE = 1, 2
BAD_SEL = 0x1


class SelectGenerator(G.GaitGenerator):
    def _read(self, cfg19):
        c = np.asarray(cfg19, _f)
        self.stanceDuration, self.dutyFactor, self.initialLegPhase = c[0:4].copy(), c[4:8].copy(), c[8:12].copy()
        self.initialLegState = [int(v) for v in c[12:16]]
        self.contactDetectionPhaseThreshold, self.waitTime, self.advancedTrot = c[16], c[17], bool(c[18] != 0)

    def Reset(self, currentTime, cfg19=None):
        if cfg19 is not None:                           # :81-90 "update params"
            self._read(cfg19)
        super().Reset(currentTime)                      # :92-120


def index_of(v, n_gaits):
    """The integer a float32 selection holds if it is one of 0 .. n_gaits - 1, else -1."""
    v = _f(v)
    if not np.isfinite(v) or v != np.floor(v) or v < 0 or v >= n_gaits:
        return -1
    return int(v)


class Robot:
    """One robot's generator and the index in force, a tick at a time."""

    def __init__(self, table):
        self.table, self.g, self.idx = table, None, 0

    def tick(self, time, contact, sel, level, stop=False):
        """-> dict(out [24], state [49] (row 48: the index in force), fe [20] (fe_in rows 42-61), swing [4] (swing_in rows 8-11), flags)."""
        flags = 0
        if level:
            idx = index_of(sel, len(self.table))
            flags = BAD_SEL if idx < 0 else 0
            self.idx = max(idx, 0)
            if level == CONSTRUCT:
                self.g = SelectGenerator(self.table[self.idx])
            else:
                self.g.Reset(0.0, self.table[self.idx])
        g = self.g
        o = g.Update(time, contact, bool(stop))
        return dict(out=o, state=np.concatenate([g.state48(), [_f(self.idx)]]).astype(_f),
                    fe=np.concatenate([o[0:4], g.dutyFactor, o[4:8], o[8:12], o[12:16]]).astype(_f), swing=g.swingDuration.copy(), flags=flags)


def run(table, time, contact, sel, level, stop=None):
    """One robot.  table [n_gaits][19]; time [T] float32 (the robot's own clock); contact [T][4]; sel [T] float32; level [T] (0, CONSTRUCT, LIVE; the
    first must be CONSTRUCT); stop [T].  -> dict(out [T][24], state [T][49], fe [T][20], swing [T][4], flags [T]) of Robot.tick."""
    T = len(time)
    assert level[0] == CONSTRUCT
    res = dict(out=np.zeros((T, 24), _f), state=np.zeros((T, 49), _f), fe=np.zeros((T, 20), _f), swing=np.zeros((T, 4), _f), flags=np.zeros(T, np.int32))
    robot = Robot(table)
    for k in range(T):
        one = robot.tick(time[k], contact[k], sel[k], level[k], stop[k] if stop is not None else False)
        for key in res:
            res[key][k] = one[key]
    return res


def stage_clock(mask, bits, ticks, origin):
    """-> (origin, local) after one call, int32."""
    origin = np.where((np.asarray(mask).astype(np.uint32) & np.uint32(bits)) != 0, ticks, origin).astype(np.int32)
    return origin, (np.asarray(ticks, np.int32) - origin).astype(np.int32)


def clock_time(ticks, dt):
    """The binding's clock: one float32 product."""
    return (np.asarray(ticks).astype(_f) * _f(dt)).astype(_f)


# ----------------------------------------------------------------------------- the mixed schedule
N_ROBOTS, TICKS, DT = G.N_ROBOTS, G.TICKS, G.DT
RUNS = 3


def schedule(table, run_id, n=N_ROBOTS, ticks=TICKS, level=None):
    """Schedule `run_id` (0 .. RUNS - 1) for the table [5][19]: every robot has its own sequence of three selections drawn from 0 .. 4 (at tick 0 and at
    two reset ticks of its own), a level per reset drawn from CONSTRUCT and LIVE (`level`: that one level for every reset after tick 0 instead), late
    and early touch-downs from gait_ref.contacts around the gait in force on the robot's restarted clock, and robot_stop from tick 300 on in the run
    with run_id % 3 == 2.  Between resets the selection array holds a valid index OTHER than the one in force.
    -> dict(sel [T][n] float32, level [T][n] int32 (tick 0: CONSTRUCT), local [T][n] int32 (ticks since the robot's last reset), contact [T][n][4],
    stop [T] int32)."""
    rng = np.random.default_rng(0x5E1EC7 + run_id)
    n_gaits = len(table)
    picks = rng.integers(0, n_gaits, (n, 3))
    at = np.sort(rng.choice(np.arange(40, ticks - 40), (n, 2)), axis=1)
    at[:, 1] = np.where(at[:, 1] == at[:, 0], at[:, 1] + 7, at[:, 1])
    lv = rng.integers(CONSTRUCT, LIVE + 1, (n, 2)) if level is None else np.full((n, 2), level)
    time = (np.arange(ticks) * DT).astype(_f)
    streams = [G.contacts(n, ticks, table[e], time, 0x6B00 + 8 * run_id + e) for e in range(n_gaits)]
    sel = np.zeros((ticks, n), _f); level_ = np.zeros((ticks, n), np.int32); local = np.zeros((ticks, n), np.int32)
    contact = np.zeros((ticks, n, 4), _f)
    for r in range(n):
        starts = [0, int(at[r, 0]), int(at[r, 1]), ticks]
        for s in range(3):
            k0, k1, e = starts[s], starts[s + 1], int(picks[r, s])
            sel[k0, r] = e
            level_[k0, r] = CONSTRUCT if s == 0 else lv[r, s - 1]
            ks = np.arange(k0 + 1, k1)
            sel[ks, r] = (e + 1 + ks % (n_gaits - 1)) % n_gaits
            local[k0:k1, r] = np.arange(k1 - k0)
            contact[k0:k1, r] = streams[e][:k1 - k0, r]
    stop = np.zeros(ticks, np.int32)
    if run_id % 3 == 2:
        stop[G.STOP_TICK:] = 1
    return dict(sel=sel, level=level_, local=local, contact=contact, stop=stop)


def reference(table, S, robots=None):
    """run() for every robot of a schedule (or of `robots`) -> dict of [T][rows][n] arrays (flags [T][n])."""
    T, n = S["level"].shape
    robots = range(n) if robots is None else robots
    res = dict(out=np.zeros((T, 24, n), _f), state=np.zeros((T, 49, n), _f), fe=np.zeros((T, 20, n), _f), swing=np.zeros((T, 4, n), _f),
               flags=np.zeros((T, n), np.int32))
    for r in robots:
        one = run(table, clock_time(S["local"][:, r], DT), S["contact"][:, r], S["sel"][:, r], S["level"][:, r], S["stop"])
        for k in ("out", "state", "fe", "swing"):
            res[k][:, :, r] = one[k]
        res["flags"][:, r] = one["flags"]
    return res


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, _f).view(np.uint32), np.ascontiguousarray(b, _f).view(np.uint32))
