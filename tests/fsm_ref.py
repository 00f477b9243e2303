"""numpy restatement of the reference's control state machine, written from the reference, one RunFSM per tick and robot; it shares no code with
csrc/qr_fsm.h.  float32 scalars where the reference computes in float.  QS = quadruped/src of the reference.

  Command             qrDesiredStateCommand: the constructor QS/controllers/qr_desired_state_command.cpp:46-58, JoyCallback :66-161, the head of Update
                      :166-243 (gaitSwitch, the change-request block, the zeros of the joyCmd members)
  Passive, StandUp, Locomotion   QS/fsm/qr_fsm_state_passive.cpp, qr_fsm_state_standup.cpp, qr_fsm_state_locomotion.cpp (OnEnter :78-126, CheckTransition
                      :162-222, Transition :226-268, SwitchMode :272-310, StandLoop :314-340, OnExit :351-355)
  Fsm                 qrControlFSM: Initialize QS/fsm/qr_control_fsm.cpp:57-64, RunFSM :68-152, SafetyPostCheck :164-177,
                      qrSafetyChecker::CheckForceFeedForward QS/fsm/qr_safety_checker.cpp:48-66
  the actions         Action::StandUp, SitDown QS/action/qr_action.cpp:31-96, one loop pass per tick (include/qrgpu.h: unrolling)

A command is a [60] float32 vector p[12], Kp[12], d[12], Kd[12], tua[12], or None for an empty std::vector (written as zeros).  Every tick notes what
ran (the plan bits of include/qrgpu.h) and which branches it took (Robot.cov, for the coverage test)."""
import numpy as np

f32 = np.float32
HARD_CODE, JOY_TROT, JOY_ADVANCED_TROT, JOY_WALK, JOY_STAND, BODY_UP, BODY_DOWN, EXIT = range(8)            # config/qr_enum_types.h:101-113
RC_MODE_ITEMS = EXIT
K_STAND_DOWN, K_PASSIVE, K_STAND_UP, GAIT_TRANSITION, K_LOCOMOTION, LOCOMOTION_STAND = -1, 0, 1, 3, 4, 7   # fsm/qr_fsm_state.hpp:38-48
PASSIVE, STAND_UP, LOCOMOTION = 1, 4, 7                                                                     # FSM_StateName
NORMAL, TRANSITIONING = 0, 1
VELOCITY_LOCOMOTION, WALK_LOCOMOTION, ADVANCED_TROT = 0, 2, 3                                               # LocomotionMode
RUN, PHASE1, PHASE2, ACTION, HOLD, PLAN_PASSIVE, REPEAT, DONE, ACTION_FIRST, ACTION_END = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x100, 0x200, 0x400
BTN_A, BTN_B, BTN_X, BTN_Y, BTN_RB, GAIT_SWITCH = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
ENTERED = 0x00010000
STATE_ROWS, OUT_ROWS, MSG_ROWS, SCRIPT_ROWS, CMD_ROWS = 106, 11, 10, 5, 60
POISON = f32(-12345.5)

_HIP = np.arccos(f32(0.28) / f32(2.0) / f32(0.2), dtype=f32)          # qr_robot_a1_sim.cpp:116: std::acos(float)
A1 = dict(stand_up_angles=[0.0, float(_HIP), float(f32(-2.0) * _HIP)] * 4, sit_down_angles=[-0.167136, 0.934969, -2.54468] * 4, kp=[100.0] * 12,
          kd=[1.0, 2.0, 2.0] * 4, stand_up_time=2.0, stand_up_total=3.0, sit_down_time=1.5, time_step=0.001, transition_ticks=1000,
          gait_transition_duration=2.0, stand_transition_duration=1.0, tau_clip=23.0, body_height=0.28, initial_ctrl_state=BODY_UP,
          hard_code_v=[0.0] * 3, hard_code_w=[0.0] * 3, max_velx=0.2, max_vely=0.1, max_yawrate=0.2)
SHORT = dict(A1, transition_ticks=16, time_step=0.05)                    # the streams': 60 stand-up ticks, 30 sit-down ticks, transitions of 32 and 16


def desc(**kw):
    return dict(A1, **kw)


def pd_command(D, p):
    """{p, Kp, 0, Kd, 0} per motor"""
    c = np.zeros(CMD_ROWS, f32)
    c[0:12] = p; c[12:24] = np.asarray(D["kp"], f32); c[36:48] = np.asarray(D["kd"], f32)
    return c


class Robot:
    cov = set()                       # branches taken, over every robot

    def __init__(self, D):
        self.D = D
        self.stand = np.asarray(D["stand_up_angles"], f32); self.sit = np.asarray(D["sit_down_angles"], f32)
        # qrDesiredStateCommand's constructor
        self.joyCtrlState = int(D["initial_ctrl_state"]); self.prevJoyCtrlState = JOY_STAND
        self.joyCmd = np.zeros(6, f32)                    # Vx, Vy, Vz, RollRate, PitchRate, YawRate
        self.request = False; self.joyCtrlOnRequest = True; self.joyCmdExit = False; self.bodyUp = 0; self.movementMode = 0; self.gaitSwitch = False
        # the three states as constructed
        self.fsmMode = None
        self.l = dict(next=LOCOMOTION, dur=f32(0), iter=0, checks=True, done=False, legCommand=None)       # TurnOnAllSafetyChecks, checkPDesFoot = false
        self.su = dict(next=STAND_UP, standUp=0, isUp=True, done=False, legCommand=None, motorAngles=None)
        self.p = dict(next=PASSIVE, done=False, legCommand=None)
        self.legCmd = None
        self.gait, self.mode, self.entered = 0, -1, False
        self.action = 0; self.t = f32(0); self.before = np.zeros(12, f32)
        # qrControlFSM::Initialize
        self.state = STAND_UP
        self.on_enter()
        self.nextState = self.state
        self.op = NORMAL

    # ---- qrDesiredStateCommand
    def joy_callback(self, btn, axes):
        c = Robot.cov
        self.joyCmd[2] = 0
        if btn & BTN_A:
            c.add("A on" if not self.joyCtrlOnRequest else "A off")
            self.joyCtrlOnRequest = not self.joyCtrlOnRequest
        if btn & BTN_X:
            c.add("X first" if self.movementMode == 0 else "X again")
            if self.movementMode == 0:
                self.movementMode = 1
            self.request = True
        if self.joyCtrlOnRequest:
            c.add("axes")
            self.joyCmd[0] = f32(axes[2]) * f32(self.D["max_velx"])
            self.joyCmd[1] = f32(axes[1]) * f32(self.D["max_vely"])
            self.joyCmd[5] = f32(axes[0]) * f32(self.D["max_yawrate"])
            self.joyCmd[3] = 0; self.joyCmd[4] = 0
        else:
            c.add("axes off")
        if btn & BTN_B:
            if self.movementMode == 1:
                c.add("B stop"); self.movementMode = 0; self.request = True
            elif self.movementMode == 0:
                if self.bodyUp >= 0:
                    c.add("B stand"); self.bodyUp = 0; self.request = True
                else:
                    c.add("B down")
        if btn & BTN_Y:
            if self.movementMode == 0 and self.bodyUp <= 0:
                c.add("Y exit"); self.joyCmdExit = True; self.request = True; self.joyCtrlOnRequest = False
            else:
                c.add("Y ignored")
        if btn & BTN_RB:
            if self.movementMode == 0:
                c.add("RB first" if self.bodyUp == 0 else "RB flip")
                self.bodyUp = 1 if self.bodyUp == 0 else -self.bodyUp
                self.request = True
            else:
                c.add("RB moving")

    def command_update(self):
        c = Robot.cov
        if self.gaitSwitch:
            c.add("gaitSwitch"); self.request = True; self.gaitSwitch = False
        if self.request:
            s = self.joyCtrlState
            if self.movementMode > 0:
                if s == HARD_CODE or s == BODY_UP:
                    c.add("to stand"); s = JOY_STAND
                elif s == JOY_STAND:
                    c.add("to advanced trot"); s = JOY_ADVANCED_TROT
                else:
                    s = (s + 1) % (RC_MODE_ITEMS + 1)
                    if s == HARD_CODE:
                        c.add("cycle past hard code"); s = s + 1
                    elif s > JOY_ADVANCED_TROT:
                        c.add("cycle to trot"); s = JOY_TROT
                    else:
                        c.add("cycle next")
            else:
                if s <= 3:
                    c.add("prev kept"); self.prevJoyCtrlState = s
                if self.joyCmdExit:
                    c.add("exit"); s = EXIT
                elif self.bodyUp == -1:
                    c.add("body down"); s = BODY_DOWN
                elif self.bodyUp == 1:
                    c.add("body up"); s = BODY_UP
                else:
                    c.add("stand"); s = JOY_STAND
            self.joyCtrlState = s
        if self.joyCtrlState not in (JOY_TROT, JOY_ADVANCED_TROT, JOY_WALK, HARD_CODE):
            self.joyCmd[:] = 0                               # the JOY_STAND branch and the else branch

    # ---- the states
    def on_enter(self):
        if self.state == PASSIVE:
            self.p.update(next=PASSIVE, done=False, legCommand=None)
        elif self.state == STAND_UP:
            self.su.update(next=STAND_UP, done=False, legCommand=None, standUp=1)
            self.fsmMode = K_STAND_UP
        else:
            self.l.update(next=LOCOMOTION, done=False, legCommand=None)
            s = self.joyCtrlState
            if s != HARD_CODE:
                if s == JOY_TROT:
                    self.mode, self.gait = VELOCITY_LOCOMOTION, 1
                elif s == JOY_ADVANCED_TROT:
                    self.mode, self.gait = ADVANCED_TROT, 2
                elif s == JOY_WALK:
                    self.mode, self.gait = WALK_LOCOMOTION, 3
                else:
                    self.gait = 4
                self.entered = True                           # quadruped->Reset(), locomotionController->Reset(), stateEstimators->Reset()

    def check_transition(self):
        m = self.fsmMode
        if self.state == STAND_UP:
            su = self.su
            su["next"] = STAND_UP
            if m == K_STAND_UP:
                if not su["isUp"]:
                    su["standUp"] = 1
            elif m == K_STAND_DOWN:
                if su["isUp"]:
                    su["standUp"] = -1
            elif m in (K_LOCOMOTION, LOCOMOTION_STAND, GAIT_TRANSITION):
                su["next"] = LOCOMOTION
            elif m == K_PASSIVE:
                su["next"] = PASSIVE
            return su["next"], f32(0)
        if self.state == PASSIVE:
            self.p["next"] = PASSIVE
            if m == K_STAND_UP:
                self.p["next"] = STAND_UP
            return self.p["next"], f32(0)
        l = self.l
        l["iter"] += 1
        if m == GAIT_TRANSITION:
            l["dur"] = f32(self.D["gait_transition_duration"]); l["iter"] = 0
        elif m == LOCOMOTION_STAND:
            l["dur"] = f32(self.D["stand_transition_duration"]); l["iter"] = 0
        elif m == K_PASSIVE:
            l["next"] = PASSIVE; l["dur"] = f32(0)
        elif m in (K_STAND_UP, K_STAND_DOWN):
            l["next"] = STAND_UP; l["dur"] = f32(0)
        return l["next"], l["dur"]

    def run(self, angles, loco):
        if self.state == LOCOMOTION:
            self.legCmd = loco.copy(); self.ran = RUN
        elif self.state == PASSIVE:
            self.legCmd = np.zeros(CMD_ROWS, f32); self.ran = PLAN_PASSIVE
        else:
            su = self.su
            if su["standUp"] != 0:                            # the action begins: its first pass
                self.action = su["standUp"]; self.t = f32(0); self.before = angles.copy()
                self.action_pass(); self.ran |= ACTION_FIRST
                return
            self.after_action()

    def action_pass(self):
        D = self.D
        if self.action == 1:                                  # Action::StandUp: t < totalTime
            blend = self.t / f32(D["stand_up_time"])
            p = blend * self.stand + (f32(1) - blend) * self.before if blend < f32(1.0) else self.stand.copy()
        else:                                                 # Action::SitDown: t < endTime
            blend = self.t / f32(D["sit_down_time"])
            p = blend * self.sit + (f32(1) - blend) * self.before
        self.legCmd = pd_command(D, p.astype(f32))            # POSITION_MODE
        self.t = f32(self.t + f32(D["time_step"]))
        self.ran = ACTION

    def after_action(self):                                   # qrFSMStateStandUp::Run after the action (:63-81)
        su = self.su
        if self.action == 1:
            su["motorAngles"], su["isUp"] = self.stand, True
        elif self.action == -1:
            su["motorAngles"], su["isUp"] = self.sit, False
        self.ran = HOLD | (ACTION_END if self.action else 0)
        self.action = 0
        su["standUp"] = 0
        self.legCmd = pd_command(self.D, su["motorAngles"])

    def transition(self, contacts, angles, loco):
        if self.state == STAND_UP:
            su = self.su
            su["done"] = True
            if su["next"] == LOCOMOTION:
                su["legCommand"] = None if self.legCmd is None else self.legCmd.copy()
            self.ran = REPEAT if su["next"] == LOCOMOTION else PLAN_PASSIVE
            return su
        if self.state == PASSIVE:
            self.p["done"] = True
            self.ran = PLAN_PASSIVE
            return self.p
        l = self.l
        if l["next"] == LOCOMOTION:
            (self.switch_mode if self.fsmMode == GAIT_TRANSITION else self.stand_loop)(contacts, angles, loco)
            l["iter"] += 1
        elif l["next"] == PASSIVE:
            l["checks"] = False; l["done"] = True              # TurnOffAllSafetyChecks
            self.ran = PLAN_PASSIVE
        else:
            l["done"] = True
            l["legCommand"] = None if self.legCmd is None else self.legCmd.copy()
            self.ran = REPEAT
        return l

    def switch_mode(self, contacts, angles, loco):
        l, T = self.l, int(self.D["transition_ticks"])
        if f32(l["iter"]) >= l["dur"] * f32(T):
            self.fsmMode = K_LOCOMOTION; l["iter"] = 0; l["done"] = True; l["dur"] = f32(0)
            Robot.cov.add("switch mode done"); self.ran = REPEAT
            return
        N = int(np.count_nonzero(contacts))
        if l["iter"] < T:
            l["legCommand"] = loco.copy(); self.zeroed = True; self.ran = PHASE1
            if N == 4:
                Robot.cov.add("switch mode: four contacts"); l["iter"] = T
            else:
                Robot.cov.add("switch mode: phase 1 goes on")
        else:
            ratio = max(f32(0.45), f32(l["iter"] - T) / f32(T))
            l["legCommand"] = pd_command(self.D, (self.stand * ratio + (f32(1) - ratio) * angles).astype(f32))
            Robot.cov.add("switch mode: floor" if ratio == f32(0.45) else "switch mode: ramp")
            self.ran = PHASE2

    def stand_loop(self, contacts, angles, loco):
        l, T = self.l, int(self.D["transition_ticks"])
        if l["iter"] >= T:
            self.fsmMode = K_LOCOMOTION; l["iter"] = 0; l["done"] = True; l["dur"] = f32(0)
            Robot.cov.add("stand loop done"); self.ran = REPEAT
            return
        N = int(np.count_nonzero(contacts))
        self.ran = REPEAT
        if f32(l["iter"]) < l["dur"] * f32(T):
            l["legCommand"] = loco.copy(); self.zeroed = True; self.ran = PHASE1
            if N == 4:
                Robot.cov.add("stand loop: four contacts"); l["iter"] = T
            else:
                Robot.cov.add("stand loop: phase 1 goes on")

    # ---- qrRobotRunner::Update without the estimators, and qrControlFSM::RunFSM
    def tick(self, msg, gait_switch, contacts, angles, loco):
        """msg: (button mask, axes[3]) or None -> dict(joy [8], plan, entered (of the previous tick), cmd [60], zeroed, out [11])"""
        D = self.D
        if gait_switch:
            self.gaitSwitch = True
        if msg is not None:
            self.joy_callback(msg[0], msg[1])
        entered, self.entered = self.entered, False
        self.zeroed, self.ran = False, 0
        start = self.state
        if self.action:                                       # inside Action::StandUp / SitDown: the runner is blocked
            Robot.cov.add("message during an action" if msg is not None else "action")
            total = f32(D["stand_up_total"] if self.action == 1 else D["sit_down_time"])
            if self.t < total:
                self.action_pass()
            else:
                self.after_action()
            trace = (start, NORMAL)
        else:
            self.command_update()
            if self.request:                                  # RunFSM :72-94
                s = self.joyCtrlState
                self.fsmMode = (GAIT_TRANSITION if s in (JOY_TROT, JOY_ADVANCED_TROT, JOY_WALK, HARD_CODE) else K_STAND_DOWN if s == BODY_DOWN
                                else K_STAND_UP if s == BODY_UP else LOCOMOTION_STAND if s == JOY_STAND else K_PASSIVE)
                self.request = False
            if self.op == NORMAL:
                name, dur = self.check_transition()
                if name != self.state:
                    self.op = TRANSITIONING; self.nextState = name
                elif np.float64(dur) > 0.1:
                    self.op = TRANSITIONING
                else:
                    self.run(angles, loco)
            trace = (start, self.op)
            if self.op == TRANSITIONING:
                td = self.transition(contacts, angles, loco)
                self.legCmd = None if td["legCommand"] is None else td["legCommand"].copy()
                self.safety_post_check()
                if td["done"]:
                    self.ran |= DONE
                    if self.state == LOCOMOTION:
                        self.l["iter"] = 0                    # OnExit
                    self.state = self.nextState
                    self.on_enter()
                    self.op = NORMAL
            else:
                self.safety_post_check()
        Robot.cov.add(trace)
        hard = self.joyCtrlState == HARD_CODE
        joy = np.concatenate([np.asarray(D["hard_code_v"], f32) if hard else self.joyCmd[0:3], np.asarray(D["hard_code_w"], f32) if hard else self.joyCmd[3:6],
                              [f32(D["body_height"]), f32(self.joyCtrlState)]]).astype(f32)
        cmd = np.zeros(CMD_ROWS, f32) if self.legCmd is None else self.legCmd.copy()
        on = self.state == LOCOMOTION and self.l["checks"]
        out = np.array([self.state, self.op, self.fsmMode, self.joyCtrlState, self.l["iter"], on, 0, on, self.gait, self.mode, self.action], f32)
        return dict(joy=joy, plan=self.ran, entered=entered, cmd=cmd, zeroed=self.zeroed, out=out)

    def safety_post_check(self):
        if self.state == LOCOMOTION and self.l["checks"] and self.legCmd is not None:      # checkForceFeedForward
            lim = f32(self.D["tau_clip"])
            t = self.legCmd[48:60]
            self.legCmd[48:60] = np.where(t > lim, lim, np.where(t < -lim, -lim, t))

    def state_rows(self):
        """the column of d_fsm_state after the tick (csrc/qr_fsm.h lists the rows)"""
        s = np.zeros(STATE_ROWS, f32)
        s[0:8] = [self.joyCtrlState, self.prevJoyCtrlState, self.movementMode, self.bodyUp, self.joyCtrlOnRequest, self.request, self.joyCmdExit, self.gaitSwitch]
        s[8:14] = self.joyCmd
        s[14:18] = [self.fsmMode, self.state, self.op, self.nextState]
        l, su, p = self.l, self.su, self.p
        s[18:23] = [l["next"], l["dur"], l["iter"], l["checks"], l["done"]]
        s[23:27] = [su["next"], su["standUp"], su["isUp"], su["done"]]
        s[27:29] = [p["next"], p["done"]]
        s[29] = self.action; s[30] = self.t; s[31:43] = self.before
        s[43:46] = [self.entered, self.gait, self.mode]
        if self.legCmd is not None:
            s[46:106] = self.legCmd
        return s


# ---- the streams of the host and device tests -----------------------------------------------------------------------------------------------------------
N_REF, T_REF = 130, 264
SCRIPT = np.array([[62, BTN_X, 0.0, 0.0, 0.0], [66, BTN_X, 0.5, -1.0, 1.0], [110, BTN_B, 0.0, 0.0, 0.0], [130, BTN_RB | GAIT_SWITCH, 0.0, 0.0, 0.0],
                   [62, BTN_Y, 0.0, 0.0, 0.0], [200, BTN_RB, 0.25, 0.25, 0.25]], f32).T.copy()       # [5][6]; the second entry of tick 62 is never taken
_STREAMS = None
# robots with a written-out life (button masks by tick, through d_joy_msg); their script clock never matches
SCENARIOS = {
    0: {},
    1: {65: BTN_X, 90: BTN_X, 140: BTN_B, 170: BTN_RB},
    2: {65: BTN_RB, 70: BTN_RB, 80: BTN_A, 105: BTN_Y, 120: BTN_RB, 125: BTN_A, 130: BTN_X},
    3: {65: BTN_RB, 70: BTN_RB, 110: BTN_RB},
    4: {65: BTN_X, 80: BTN_Y, 85: BTN_B, 110: BTN_Y},
    5: {10: BTN_X, 90: BTN_X},                       # reset during the stand-up (tick 30), then again during a gait transition (tick 100)
    6: {65: BTN_X, 70: BTN_X, 120: BTN_X, 160: BTN_X | BTN_B, 200: BTN_B, 205: BTN_B},
}
SCENARIO_RESETS = {5: (30, 100)}
SCENARIO_CONTACTS = {1: 0.0, 4: 1.0, 5: 0.0, 6: 0.0}


def streams():
    """130 robots, 264 ticks at SHORT: reset [T][n], joy_msg [T][10][n], ticks [T][n] (the script's clock), est_in [T][54][n] (contacts, motor angles),
    loco [T][60][n] (the locomotion chain's command, torques beyond the clip among them)"""
    global _STREAMS
    if _STREAMS is not None:
        return _STREAMS
    rng = np.random.default_rng(20240611)
    n, T = N_REF, T_REF
    reset = rng.uniform(size=(T, n)) < 0.002
    reset[0] = True
    msg = np.zeros((T, MSG_ROWS, n), f32)
    arrived = rng.uniform(size=(T, n)) < 0.08
    press = rng.uniform(size=(T, 5, n)) < np.array([0.06, 0.2, 0.4, 0.08, 0.25])[None, :, None]
    msg[:, 1:6] = press
    msg[:, 6:9] = rng.uniform(-1, 1, (T, 3, n)).astype(f32)
    msg[:, 0] = arrived
    msg[:, 9] = rng.uniform(size=(T, n)) < 0.004
    p4 = rng.choice([0.0, 0.05, 0.3, 1.0], n)
    for r, life in SCENARIOS.items():
        reset[1:, r] = False
        for t in SCENARIO_RESETS.get(r, ()):
            reset[t, r] = True
        msg[:, :, r] = 0
        msg[:, 6:9, r] = rng.uniform(-1, 1, (T, 3)).astype(f32)
        for t, b in life.items():
            msg[t, 0, r] = 1
            msg[t, 1:6, r] = [(b >> k) & 1 for k in range(5)]
        if r in SCENARIO_CONTACTS:
            p4[r] = SCENARIO_CONTACTS[r]
    # the script's clock: ticks since the robot's reset; every other robot's clock is far from the script
    ticks = np.zeros((T, n), np.int32)
    count = np.zeros(n, np.int64)
    for t in range(T):
        count = np.where(reset[t], 0, count + 1)
        ticks[t] = count
    off = np.where(np.arange(n) % 2 == 1, 0, 100000).astype(np.int32)
    off[list(SCENARIOS)] = 100000
    ticks += off[None, :]
    # robots 7 and 9 follow the script alone (9: four contacts); robot 11 gets a message of its own on a script tick as well
    for r in (7, 9, 11):
        reset[1:, r] = False
        ticks[:, r] = np.arange(T)
        msg[:, :, r] = 0
    p4[7], p4[9] = 0.0, 1.0
    msg[66, 0, 11] = 1; msg[66, 5, 11] = 1; msg[66, 6:9, 11] = [0.5, 0.5, 0.5]
    est_in = rng.uniform(-1, 1, (T, 54, n)).astype(f32)
    four = rng.uniform(size=(T, n)) < p4[None, :]
    c = (rng.uniform(size=(T, 4, n)) < 0.6)
    c[:, 0] &= ~(c[:, 1] & c[:, 2] & c[:, 3])                 # never four by chance
    est_in[:, 13:17] = np.where(four[:, None, :], 1.0, c).astype(f32)
    est_in[:, 17:29] = rng.uniform(-2.6, 1.2, (T, 12, n)).astype(f32)
    loco = rng.uniform(-3, 3, (T, CMD_ROWS, n)).astype(f32)
    loco[:, 48:60] = rng.uniform(-40, 40, (T, 12, n)).astype(f32)
    _STREAMS = dict(reset=reset, joy_msg=msg, ticks=ticks, est_in=est_in, loco=loco)
    return _STREAMS


def script_message(script, tick):
    """the first entry of script [5][k] whose tick equals `tick` -> (mask, axes) or None"""
    for e in range(script.shape[1]):
        if script[0, e] == f32(tick):
            return int(script[1, e]), script[2:5, e].copy()
    return None


def message(S, script, t, r):
    """what robot r receives at tick t -> ((button mask, axes) or None, gaitSwitch, which paths applied)"""
    m = S["joy_msg"][t, :, r]
    own = None
    if m[0] != 0:
        own = (sum(1 << k for k in range(5) if m[1 + k] == 1), m[6:9].copy())
    sc = None if script is None else script_message(script, S["ticks"][t, r])
    gs = bool(m[9] != 0) or (sc is not None and bool(sc[0] & GAIT_SWITCH))
    return (own if own is not None else sc), gs, (own is not None, sc is not None)


_REFERENCE = {}


def reference(n=N_REF, first=0, last=T_REF, fresh_at=None, D=None, script=SCRIPT):
    """The restatement over ticks first..last-1 of the streams for robots 0..n-1 (fresh_at: everyone is reset at that tick too) -> stacked [T'] arrays:
    joy [8][n], plan [n], mask [n] (bit 0: reset, ENTERED), cmd [60][n], out [11][n], state [106][n], zeroed [n]; and paths [T'][n][2]."""
    key = (n, first, last, fresh_at, script is None)
    if D is None and key in _REFERENCE:
        return _REFERENCE[key]
    DD = SHORT if D is None else D
    S = streams()
    robots = [None] * n
    keys = ("joy", "plan", "mask", "cmd", "out", "state", "zeroed")
    rows = dict(joy=8, cmd=CMD_ROWS, out=OUT_ROWS, state=STATE_ROWS)
    res = {k: np.zeros((last - first, rows[k], n), f32) if k in rows else np.zeros((last - first, n), np.int32) for k in keys}
    res["paths"] = np.zeros((last - first, n, 2), bool)
    for t in range(first, last):
        for r in range(n):
            rst = bool(S["reset"][t, r]) or t == fresh_at or robots[r] is None
            if rst:
                if robots[r] is not None:
                    Robot.cov.add("reset during an action" if robots[r].action else "reset during a transition" if robots[r].op == TRANSITIONING else "reset")
                robots[r] = Robot(DD)
            m, gs, paths = message(S, script, t, r)
            o = robots[r].tick(m, gs, S["est_in"][t, 13:17, r], S["est_in"][t, 17:29, r], S["loco"][t, :, r])
            k = t - first
            res["joy"][k, :, r] = o["joy"]; res["plan"][k, r] = o["plan"]; res["mask"][k, r] = (1 if rst else 0) | (ENTERED if o["entered"] else 0)
            res["cmd"][k, :, r] = o["cmd"]; res["out"][k, :, r] = o["out"]; res["state"][k, :, r] = robots[r].state_rows(); res["zeroed"][k, r] = o["zeroed"]
            res["paths"][k, r] = paths
    if D is None:
        _REFERENCE[key] = res
    return res


def zero_rows():
    """the rows qrgpu_fsm_zero_command_batch writes, per array"""
    return dict(state_des=list(range(6, 12)), fe=[3, 4, 5], fh=[16, 17, 18, 19], sv=[23, 24, 25, 26], sc=list(range(1, 7)))


ZERO_ARRAY_ROWS = dict(state_des=12, fe=64, fh=46, sv=53, sc=28)


def expected_zero_arrays(zeroed):
    """what the five arrays of the zeroing stage hold after a tick that found them at POISON: +0 in the listed rows of the robots in phase 1"""
    out = {}
    for k, rows in zero_rows().items():
        a = np.full((ZERO_ARRAY_ROWS[k], zeroed.shape[0]), POISON, f32)
        a[np.ix_(rows, np.nonzero(zeroed)[0])] = 0
        out[k] = a
    return out


def compare(got, ref, t, n, tag="", done_word=0x40):
    """one tick of a device or host run against the restatement, bit for bit: got[k] [rows][n] (plan, mask: [n]); the resets went through done words
    `done_word` (0: through the scalar)"""
    for k in ("state", "joy", "cmd", "out"):
        a, b = np.ascontiguousarray(got[k], f32).view(np.uint32), np.ascontiguousarray(ref[k][t][:, :n]).view(np.uint32)
        if not np.array_equal(a, b):
            row, r = np.argwhere(a != b)[0]
            raise AssertionError("%s tick %d: %s row %d robot %d: %r != %r" % (tag, t, k, row, r, got[k][row, r], ref[k][t][row, r]))
    assert np.array_equal(got["plan"], ref["plan"][t][:n]), (tag, t, "plan", np.nonzero(got["plan"] != ref["plan"][t][:n])[0][:5])
    want = np.where(ref["mask"][t][:n] & 1, done_word, 0) | (ref["mask"][t][:n] & ENTERED)
    assert np.array_equal(got["mask"], want), (tag, t, "mask")
    for k, a in expected_zero_arrays(ref["zeroed"][t][:n]).items():
        if k in got:
            assert np.array_equal(np.ascontiguousarray(got[k], f32).view(np.uint32), a.view(np.uint32)), (tag, t, k)
