"""TEST INFRASTRUCTURE -- the MPC front-end as the reference states it, one robot at a time in numpy scalars, written from the reference
statement by statement (quadruped/src/controllers/mpc/qr_mpc_stance_leg_controller.cpp:158-204 SetupCommand, :207-334 Run without the solve,
:337-382 UpdateMPC; members and their types from qr_mpc_stance_leg_controller.h).  It shares no text with oracle/qr_oracle_frontend.cpp or
qr_frontend_kernel.hip: it is a class with the reference's member names, keeps trajAll and mpcTable as members, and counts ticks in a Python int.

Number formats.  Members and locals are float32 unless the reference's expression promotes: a double literal or M_PI / M_2PI makes the whole
expression double, and the assignment narrows it.  F() and D() below mark every such step; no Python float enters an operation.  std::sin
is math.sin of a double; the two rows it reaches (body height, pitch compensation) and the trajectory columns copied from them are the only
outputs not expected to agree bit for bit with the kernel (1 float32 ulp, tests/test_gpu_frontend.py).

What is the project's and not the reference's, said here once:
  * baseRMat * v is written out as ((r0 * x + r1 * y) + r2 * z), products rounded one by one.  The order inside the reference's Eigen product
    is the compiler's; this is the order the project takes (DESIGN section 2 lists it as open).
  * round(dtMPC / dt) < 2 makes the reference's cadence take a remainder by zero.  The model refuses it (ValueError), as
    qrgpu_mpc_frontend_batch does with QRGPU_ERR_BAD_ARG; so it does beyond 2^24.
  * iterationCounter is an integer here, as in the reference.  The kernel keeps it in a float row and folds it at 2^24 (include/qrgpu.h):
    counter_row_ok() says when a float row stands for the same counter.
"""
import math

import numpy as np

F = np.float32
D = np.float64
SWING, STANCE, EARLY_CONTACT, LOSE_CONTACT = 0, 1, 2, 3
M_PI = D(3.14159265358979323846)
M_PI_2 = D(1.57079632679489661923)
M_2PI = D(6.28318530718)                      # utils/qr_ctypes.h: the reference's own eleven-digit constant
N_ROBOTS = 65
SIN_CMD_ROWS = (2, 10)
SIN_TRAJ_COLS = (1, 5)


def clip(command, minVal, maxVal):
    """utils/qr_algebra.h clip<T>"""
    if command < minVal:
        return minVal
    if command > maxVal:
        return maxVal
    return command


def iterations_in_a_mpc(dt, dtMPC):
    """iterationsInaMPC = round(dtMPC / dt) of two floats (constructor, :51): half away from zero.  ValueError outside 2 .. 2^24."""
    q = D(F(dtMPC) / F(dt))
    r = math.floor(q + 0.5) if np.isfinite(q) else -1
    if not 2 <= r <= 1 << 24:
        raise ValueError("round(dtMPC / dt) = %r: the re-plan period would be zero, or beyond a float counter" % (r,))
    return int(r)


class MPCStanceLegController:
    def __init__(self, horizonLength, numHorizonL, st8, dt=0.002, dtMPC=0.06):
        """st8 = one robot's fe_state rows (include/qrgpu.h): the controller memory the caller starts from."""
        self.horizonLength, self.numHorizonL = int(horizonLength), int(numHorizonL)
        self.dt, self.dtMPC = F(dt), F(dtMPC)
        self.iterationsInaMPC = iterations_in_a_mpc(dt, dtMPC)
        s = np.asarray(st8, F)
        self.xVelDes, self.yVelDes, self.yawTurnRate, self.yawDesTrue = s[0], s[1], s[2], s[3]
        self.posDesiredinWorld = s[4:7].copy()
        self.iterationCounter = int(s[7])
        self.rpyComp = np.zeros(3, F)
        self.trajAll = np.full(12 * self.horizonLength, np.nan, F)          # untouched until the first re-plan
        self.mpcTable = np.ones((self.horizonLength, 4), F)
        self.mpcUpdated = False
        self.wbcData = {}
        self.seen = set()                                                   # which branches ran: the families assert their coverage with it

    # ------------------------------------------------------------------ :158-204
    def SetupCommand(self, fe):
        self.bodyHeight = fe[0]
        x_vel_cmd, y_vel_cmd, yaw_vel_cmd = fe[3], fe[4], fe[5]
        x_filter, y_filter, yaw_filter = F(0.01), F(0.005), F(0.03)
        one = F(1)
        self.xVelDes = self.xVelDes * (one - x_filter) + x_vel_cmd * x_filter
        self.yVelDes = self.yVelDes * (one - y_filter) + y_vel_cmd * y_filter
        self.yawTurnRate = self.yawTurnRate * (one - yaw_filter) + yaw_vel_cmd * yaw_filter
        self.xVelDes = clip(self.xVelDes, F(-1.0), F(2.0))
        self.yVelDes = clip(self.yVelDes, F(-0.6), F(0.6))
        yawCurrent = fe[9]
        self.yawDesTrue = self.yawDesTrue + self.dt * self.yawTurnRate
        if D(self.yawDesTrue) >= M_PI:
            self.yawDesTrue = F(D(self.yawDesTrue) - M_2PI); self.seen.add("wrap_down")
        elif D(self.yawDesTrue) <= -M_PI:
            self.yawDesTrue = F(D(self.yawDesTrue) + M_2PI); self.seen.add("wrap_up")
        if D(yawCurrent) > M_PI_2 and self.yawDesTrue < F(0):
            self.yawDesTrue = F(D(self.yawDesTrue) + M_2PI); self.seen.add("unwrap_up")
        elif D(yawCurrent) < -M_PI_2 and self.yawDesTrue > F(0):
            self.yawDesTrue = F(D(self.yawDesTrue) - M_2PI); self.seen.add("unwrap_down")
        self.rollDes, self.pitchDes = fe[1], fe[2]

    # ------------------------------------------------------------------ :207-334
    def Run(self, fe64):
        """One control tick on one robot's fe_in rows.  -> dict(traj, gait, wbc15, contact, state, updated), the oracle's layout."""
        fe = np.asarray(fe64, F)
        self.SetupCommand(fe)
        contactState = [bool(fe[38 + i] != 0) for i in range(4)]
        basePosition = fe[6:9]
        e0, e1, e2, e3 = fe[10], fe[11], fe[12], fe[13]
        one, two, zero = F(1), F(2), F(0)
        baseRMat = [[one - two * (e2 * e2 + e3 * e3), two * (e1 * e2 - e0 * e3), two * (e1 * e3 + e0 * e2)],
                    [two * (e1 * e2 + e0 * e3), one - two * (e1 * e1 + e3 * e3), two * (e2 * e3 - e0 * e1)]]      # (the third row is never read)
        rot = lambda v: [(r[0] * v[0] + r[1] * v[1]) + r[2] * v[2] for r in baseRMat]
        vDesWorld = rot([self.xVelDes, self.yVelDes, zero])
        pFoot = fe[14:26].reshape(4, 3)
        self.posDesiredinWorld[0] = self.posDesiredinWorld[0] + self.dt * vDesWorld[0]
        self.posDesiredinWorld[1] = self.posDesiredinWorld[1] + self.dt * vDesWorld[1]
        self.posDesiredinWorld[2] = self.posDesiredinWorld[2] + self.dt * zero
        self.posDesiredinWorld[2] = F(D(0.99) * D(self.bodyHeight + (self.bodyHeight - basePosition[2])) + D(0.01) * D(self.posDesiredinWorld[2]))
        self.rpyComp[1] = self.pitchDes
        desiredLegState = [int(fe[54 + i]) for i in range(4)]
        legState = [int(fe[58 + i]) for i in range(4)]
        normalizedPhase, phaseInFullCycle, dutyFactor = fe[50:54], fe[42:46], fe[46:50]
        for legId in range(4):
            if desiredLegState[legId] == SWING:
                s = D(math.sin(float(D(normalizedPhase[legId]) * M_PI)))
                self.bodyHeight = F(D(self.bodyHeight) + D(0.02) * s)
                if D(fe[3]) < D(-0.01):
                    self.rpyComp[1] = F(D(self.rpyComp[1]) - D(0.1) * s); self.seen.add("pitch_comp")
                self.seen.add("height_comp")
                break
        desiredFootholdsInWorldFrame = fe[26:38].reshape(4, 3)
        comDestination = np.zeros(3, F)
        for i in range(4):
            comDestination = comDestination + (pFoot[i] if contactState[i] else desiredFootholdsInWorldFrame[i])
        comDestination = comDestination / F(4)
        dutyF = dutyFactor[0]
        if desiredLegState[0] == SWING:
            t = phaseInFullCycle[0] - dutyF; self.seen.add("t_leg0")
        elif desiredLegState[1] == SWING:
            t = phaseInFullCycle[1] - dutyF; self.seen.add("t_leg1")
        elif phaseInFullCycle[0] < phaseInFullCycle[1]:
            t = phaseInFullCycle[0] + (one - dutyF); self.seen.add("t_after0")
        else:
            t = phaseInFullCycle[1] + (one - dutyF); self.seen.add("t_after1")
        t = t * two
        baseStartState = fe[62:64]                                           # footholdPlanner->firstSwingBaseState x, y
        for axis in range(2):
            self.posDesiredinWorld[axis] = (one - t) * baseStartState[axis] + t * comDestination[axis]
        dPhase = F(D(1.0) / D(self.numHorizonL * self.horizonLength))
        for i in range(self.horizonLength):
            for j in range(4):
                ithMPCPhase = phaseInFullCycle[j] + F(i) * dPhase
                while D(ithMPCPhase) > D(1.0):
                    ithMPCPhase = F(D(ithMPCPhase) - D(1.0)); self.seen.add("phase_wrap")
                self.mpcTable[i, j] = 1 if (ithMPCPhase < dutyFactor[j] or legState[j] == EARLY_CONTACT) else 0
                if i > 0 and ithMPCPhase == dutyFactor[j] and legState[j] != EARLY_CONTACT:
                    self.seen.add("table_tie")                                # a row that sits on the duty factor: "<" leaves it out
        for legId in range(4):
            self.mpcTable[0, legId] = F(contactState[legId])
        self.UpdateMPC(basePosition, vDesWorld)
        offsetP = rot([F(0.018), zero, zero])
        w = np.zeros(15, F)
        w[0] = self.posDesiredinWorld[0] + offsetP[0]; w[1] = self.posDesiredinWorld[1] + offsetP[1]; w[2] = self.bodyHeight
        w[3] = vDesWorld[0]; w[4] = vDesWorld[1]
        w[9] = self.rpyComp[0]; w[10] = self.rpyComp[1]; w[11] = self.yawDesTrue
        w[14] = self.yawTurnRate
        self.wbcData = dict(allowAfterMPC=not self.mpcUpdated)
        self.iterationCounter += 1
        return dict(traj=self.trajAll.copy(), gait=self.mpcTable.reshape(-1).copy(), wbc15=w, contact=np.asarray(contactState, F), state=self.state8(),
                    updated=int(self.mpcUpdated))

    # ------------------------------------------------------------------ :337-382
    def UpdateMPC(self, p, vDesWorld):
        if self.iterationCounter % (self.iterationsInaMPC // 2) == 0 or self.iterationCounter < 50:
            max_pos_error = F(0.1)
            xStart = clip(self.posDesiredinWorld[0], p[0] - max_pos_error, p[0] + max_pos_error)
            yStart = clip(self.posDesiredinWorld[1], p[1] - max_pos_error, p[1] + max_pos_error)
            self.posDesiredinWorld[0] = xStart; self.posDesiredinWorld[1] = yStart
            trajInitial = [self.rpyComp[0], self.rpyComp[1], self.yawDesTrue, xStart, yStart, self.bodyHeight, F(0), F(0), self.yawTurnRate, vDesWorld[0],
                           vDesWorld[1], F(0)]
            tr = self.trajAll
            for i in range(self.horizonLength):
                tr[12 * i:12 * i + 12] = trajInitial
                if i > 0:
                    tr[12 * i + 2] = tr[12 * (i - 1) + 2] + self.dtMPC * self.yawTurnRate
                    tr[12 * i + 3] = tr[12 * (i - 1) + 3] + self.dtMPC * vDesWorld[0]
                    tr[12 * i + 4] = tr[12 * (i - 1) + 4] + self.dtMPC * vDesWorld[1]
            self.mpcUpdated = True
        else:
            self.mpcUpdated = False

    def state8(self):
        """The fe_state rows; row 7 is the integer counter as a float64 so that it is exact beyond 2^24 (compare it with counter_row_ok)."""
        return np.array([self.xVelDes, self.yVelDes, self.yawTurnRate, self.yawDesTrue, self.posDesiredinWorld[0], self.posDesiredinWorld[1],
                         self.posDesiredinWorld[2], self.iterationCounter], D)


def folded(counter, period):
    """include/qrgpu.h: the smallest value >= 50 of counter's residue class modulo the period."""
    r = counter % period
    return r if r >= 50 else r + period * -(-(50 - r) // period)


def counter_row_ok(row7, counter, period):
    """Does the float counter row stand for the integer `counter`?  Below 2^24 it is the integer.  The tick that would store 2^24 stores
    folded(2^24, period) instead (include/qrgpu.h) and the row counts on from there, one a tick."""
    if counter < 1 << 24:
        return row7 == counter
    return row7 == folded(1 << 24, period) + (counter - (1 << 24))


def run(family, robot):
    """One robot of a family from its first tick.  -> list of the per-tick dicts of MPCStanceLegController.Run, and the branches seen."""
    m = MPCStanceLegController(family["h"], family["L"], family["st"][robot], family["dt"], family["dt_mpc"])
    fe = family["fe"]
    outs = [m.Run(fe[min(k, fe.shape[0] - 1), robot]) for k in range(family["ticks"])]
    return outs, m.seen


# ----------------------------------------------------------------------------- families (tests/test_frontend_ref.py, tests/test_gpu_frontend.py)
def _family(name, pkg, seed, h=10, L=2, dt=0.002, dt_mpc=0.06, ticks=40, n=N_ROBOTS):
    fe, st = pkg.workload.make_frontend_batch(n, seed=seed)
    return dict(name=name, h=h, L=L, dt=dt, dt_mpc=dt_mpc, ticks=ticks, fe=fe[None].copy(), st=st)


def _phase_meeting(duty, i, h, L):
    """A float32 phase p with p + i * dPhase == duty in the front-end's own float32 arithmetic."""
    step = F(i) * F(D(1.0) / D(L * h))
    p = F(duty) - step
    for cand in (p, np.nextafter(p, F(0)), np.nextafter(p, F(1))):
        if cand + step == F(duty):
            return cand
    raise ValueError("no float32 phase meets the duty factor at row %d" % i)


def _wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def family(pkg, name):
    """-> dict(name, h, L, dt, dt_mpc, ticks, fe [T or 1][n][64], st [n][8]); a family with one fe row set holds its inputs over the ticks."""
    n = N_ROBOTS
    rng = np.random.default_rng(0xFE00 + NAMES.index(name))
    if name == "yaw_seam":
        # five groups of 13: the plan crosses +pi upwards / -pi downwards with the robot's own yaw trailing it across the seam (wrap, then the
        # unwrap branches as long as robot and plan sit on opposite sides); the same two with the robot far from the seam (wrap alone); a robot
        # within 1e-3 of +-pi/2 with a plan of the other sign (both unwrap branches, on both sides of their thresholds and on them)
        f = _family(name, pkg, 0x51)
        T = f["ticks"]
        fe = np.repeat(f["fe"], T, axis=0); st = f["st"]
        g = np.arange(n) % 5
        rate = rng.uniform(0.8, 2.0, n) * np.where((g == 0) | (g == 2), 1, -1)
        start = np.where(rate > 0, np.pi - rng.uniform(0.005, 0.06, n), -np.pi + rng.uniform(0.005, 0.06, n))
        st[:, 2] = rate; fe[:, :, 5] = rate; st[:, 3] = start
        for k in range(T):
            fe[k, :, 9] = np.where(g < 2, _wrap(start + 0.9 * 0.002 * rate * k), np.where(rate > 0, 0.3, -0.3))
        q = g == 4
        side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        off = np.array([-1e-3, -1e-7, 0.0, 1e-7, 1e-3])[(np.arange(n) // 10) % 5]
        fe[:, q, 9] = (side * (np.pi / 2 + off))[q]
        st[q, 3] = (-side * rng.uniform(0.01, 0.05, n))[q]; st[q, 2] = 0; fe[:, q, 5] = 0
        f["fe"] = fe
        return f
    if name == "backwards":
        f = _family(name, pkg, 0x52)
        b = np.float32(-0.01)
        vals = np.array([b, np.nextafter(b, np.float32(-1)), np.nextafter(b, np.float32(0)), -0.0101, -0.0099, -0.5, 0.3, -1.5], np.float32)
        f["fe"][0, :, 3] = vals[np.arange(n) % 8]
        return f
    if name == "swing_order":
        # desiredLegState[0], [1] SWING or not, phase[0] < phase[1] or not: eight combinations, robot i takes i % 8
        f = _family(name, pkg, 0x53, L=3)
        fe = f["fe"][0]
        c = np.arange(n) % 8
        fe[:, 54] = np.where(c & 1, SWING, STANCE); fe[:, 55] = np.where(c & 2, SWING, STANCE)
        lo, hi = rng.uniform(0.05, 0.45, n), rng.uniform(0.5, 0.95, n)
        fe[:, 42] = np.where(c & 4, lo, hi); fe[:, 43] = np.where(c & 4, hi, lo)
        fe[::16, 43] = fe[::16, 42]                                          # a tie: the reference's "<" sends it to leg 1
        return f
    if name == "early_contact":
        f = _family(name, pkg, 0x54, h=16, ticks=8)
        fe = f["fe"][0]
        for leg in range(4):
            pick = rng.uniform(0, 1, n)
            fe[:, 58 + leg] = np.where(pick < 0.4, EARLY_CONTACT, np.where(pick < 0.5, LOSE_CONTACT, fe[:, 58 + leg]))
        return f
    if name.startswith("phase_edges"):
        h, L = [int(v) for v in name.split("_")[2:4]]
        f = _family(name, pkg, 0x55 + 16 * L + h, h=h, L=L, ticks=3)
        fe = f["fe"][0]
        top = np.float32(1) - np.float32(2.0 ** -24)
        for leg in range(4):
            duty = fe[0, 46 + leg]
            edges = [0.0, duty, top, 1.0, np.nextafter(duty, np.float32(0))]
            # phases whose row 1 / row h - 1 lands exactly on the duty factor (row 0 is overwritten by the measured contacts)
            edges += [_phase_meeting(duty, i, h, L) for i in sorted({1, h - 1}) if i >= 1]
            edges = np.array(edges, np.float32)
            pick = rng.integers(0, len(edges), n)
            keep = rng.uniform(0, 1, n) < 0.2
            fe[:, 42 + leg] = np.where(keep, fe[:, 42 + leg], edges[pick])
        return f
    if name.startswith("cadence") or name.startswith("counter_2p24"):
        ratio = int(name.rsplit("_", 1)[1])
        f = _family(name, pkg, 0x56 + ratio, dt_mpc=0.002 * ratio)
        assert iterations_in_a_mpc(f["dt"], f["dt_mpc"]) == ratio
        # counters that cross 49 -> 50 and multiples of the period within the 40 ticks, or every robot at 2^24 - 3
        f["st"][:, 7] = (1 << 24) - 3 if name.startswith("counter") else 20 + np.arange(n) % 60
        return f
    raise KeyError(name)


NAMES = ("yaw_seam", "backwards", "swing_order", "early_contact", "phase_edges_1_2", "phase_edges_1_3", "phase_edges_10_2", "phase_edges_10_3",
         "phase_edges_16_2", "phase_edges_16_3", "cadence_30", "cadence_25", "cadence_3", "counter_2p24_30", "counter_2p24_25", "counter_2p24_3")
# the branches a family is there for: tests/test_frontend_ref.py asserts that the model ran them
COVERS = {"yaw_seam": {"wrap_down", "wrap_up", "unwrap_up", "unwrap_down"}, "backwards": {"pitch_comp", "height_comp"},
          "swing_order": {"t_leg0", "t_leg1", "t_after0", "t_after1"}, "phase_edges_10_2": {"phase_wrap", "table_tie"}, "phase_edges_10_3": {"table_tie"}, "phase_edges_16_2": {"table_tie"},
          "phase_edges_16_3": {"phase_wrap", "table_tie"}}

_cache = {}


def expected(pkg, name):
    """-> (family, outs[robot][tick] of run(), seen) computed once per session and shared by the tests; nobody writes into it."""
    if name not in _cache:
        f = family(pkg, name)
        runs = [run(f, r) for r in range(f["st"].shape[0])]
        _cache[name] = (f, [o for o, _ in runs], set().union(*[s for _, s in runs]))
    return _cache[name]


def compare(out, want, counter_period, where, sin_ulps=1):
    """One robot-tick of the oracle or the kernel (dict in the oracle's layout; traj may hold stale rows when not updated) against the model's."""
    assert out["updated"] == want["updated"], where
    assert np.array_equal(out["gait"], want["gait"]), where
    assert np.array_equal(out["contact"], want["contact"]), where
    assert np.array_equal(out["state"][:7], want["state"][:7].astype(F)), (where, out["state"], want["state"])
    assert counter_row_ok(out["state"][7], int(want["state"][7]), counter_period), (where, out["state"][7], want["state"][7])
    exact = [r for r in range(15) if r not in SIN_CMD_ROWS]
    assert np.array_equal(out["wbc15"][exact], want["wbc15"][exact]), where
    assert ulp_close(out["wbc15"][list(SIN_CMD_ROWS)], want["wbc15"][list(SIN_CMD_ROWS)], sin_ulps), where
    to, tw = out["traj"].reshape(-1, 12), want["traj"].reshape(-1, 12)
    cols = [c for c in range(12) if c not in SIN_TRAJ_COLS]
    assert np.array_equal(to[:, cols], tw[:, cols], equal_nan=True), where
    assert ulp_close(to[:, SIN_TRAJ_COLS], tw[:, SIN_TRAJ_COLS], sin_ulps), where


def ulp_close(a, b, ulps=1):
    a = np.asarray(a, F); b = np.asarray(b, F)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        return bool(np.all(both_nan | (np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b))))))
