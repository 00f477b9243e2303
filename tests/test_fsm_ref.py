"""CPU: tests/fsm_ref.py, the numpy restatement of the reference's control state machine, against scenario tables written out by hand from the
reference's sources (not by running the restatement), a coverage check of the streams the host and device tests run, and one run at the reference's
own durations for the tick counts.

The tables use time_step 0.25 and transition_ticks 4: the stand-up's t runs 0, 0.25 ... 2.75 (twelve passes below stand_up_total 3, all exact in
float32; the blend t / 2 reaches 1 at the ninth), the sit-down's 0 ... 1.25 (six passes below 1.5); a gait transition lasts 2 x 4 ticks, a stand
transition 1 x 4."""
import numpy as np

import fsm_ref as R

f32 = np.float32
D4 = R.desc(time_step=0.25, transition_ticks=4)
LOCO = np.concatenate([np.arange(48, dtype=f32) / 8, [40, -40, 23, -23, 22.5, -22.5, 0, 1, 2, 3, 4, 5]]).astype(f32)        # tua beyond the clip
ANGLES = np.linspace(-1.0, 0.5, 12).astype(f32)
KINDS = {R.RUN: "run", R.PHASE1: "p1", R.PHASE2: "p2", R.ACTION: "act", R.HOLD: "hold", R.PLAN_PASSIVE: "passive", R.REPEAT: "repeat"}


def drive(D, buttons, T, four=False, robot=None):
    """one robot over T ticks: buttons {tick: mask}, axes (0.5, -1, 1) with every message -> the robot and a list of per-tick dicts"""
    rb = R.Robot(D) if robot is None else robot
    log = []
    for t in range(T):
        msg = (buttons[t], np.array([0.5, -1.0, 1.0], f32)) if t in buttons else None
        contacts = np.ones(4, f32) if (four(t) if callable(four) else four) else np.array([1, 0, 0, 1], f32)
        o = rb.tick(msg, False, contacts, ANGLES, LOCO)
        o["kind"] = KINDS[o["plan"] & 0x7f]; o["flags"] = o["plan"] & ~0x7f
        log.append(o)
    return rb, log


def kinds(log, a, b):
    return [o["kind"] for o in log[a:b]]


def pd(D, p):
    return R.pd_command(D, np.asarray(p, f32))


def test_a_fresh_robot_stands_up_for_exactly_k_ticks_and_then_holds():
    rb, log = drive(D4, {}, 16)
    assert kinds(log, 0, 16) == ["act"] * 12 + ["hold"] * 4
    assert log[0]["flags"] == R.ACTION_FIRST and all(o["flags"] == 0 for o in log[1:12]) and log[12]["flags"] == R.ACTION_END and log[13]["flags"] == 0
    stand = np.asarray(D4["stand_up_angles"], f32)
    for k in range(12):
        blend = f32(k * 0.25 / 2.0)
        want = blend * stand + (f32(1) - blend) * ANGLES if k < 8 else stand          # qr_action.cpp:46-70
        assert np.array_equal(log[k]["cmd"], pd(D4, want)), k
        assert log[k]["out"][0] == R.STAND_UP and log[k]["out"][10] == 1
    for o in log[12:]:
        assert np.array_equal(o["cmd"], pd(D4, stand)) and o["out"][10] == 0
        assert list(o["joy"]) == [0, 0, 0, 0, 0, 0, f32(0.28), R.BODY_UP]
    assert all(o["entered"] is False for o in log)


def test_x_leads_to_stand_then_locomotion_by_way_of_the_stand_loop():
    stand = pd(D4, D4["stand_up_angles"])
    clipped = LOCO.copy(); clipped[48:50] = [23, -23]
    # four contacts: the loop ends at once
    rb, log = drive(D4, {13: R.BTN_X}, 18, four=True)
    assert kinds(log, 12, 18) == ["hold", "repeat", "p1", "repeat", "run", "run"]
    assert [o["flags"] for o in log[13:17]] == [R.DONE, 0, R.DONE, 0]
    assert np.array_equal(log[13]["cmd"], stand)                       # Transition: legCommand = legCmd, the hold (qr_fsm_state_standup.cpp:138-141)
    assert np.array_equal(log[14]["cmd"], clipped) and log[14]["zeroed"] and np.array_equal(log[15]["cmd"], clipped)     # the done tick sends the last command again
    assert [o["entered"] for o in log[13:18]] == [False, True, False, True, False]          # OnEnter ran twice
    assert [o["out"][0] for o in log[12:15]] == [R.STAND_UP, R.LOCOMOTION, R.LOCOMOTION] and [o["out"][1] for o in log[13:17]] == [0, 1, 0, 0]
    assert [o["out"][2] for o in log[13:17]] == [R.LOCOMOTION_STAND, R.LOCOMOTION_STAND, R.K_LOCOMOTION, R.K_LOCOMOTION]
    assert [o["out"][4] for o in log[13:17]] == [0, 5, 0, 1]           # iter: T, then ++; OnExit; CheckTransition's ++ in the run tick
    assert log[16]["out"][3] == R.JOY_STAND and log[16]["out"][8] == 4 and log[16]["out"][9] == -1 and list(log[16]["out"][5:8]) == [1, 0, 1]
    assert not log[16]["zeroed"] and np.array_equal(log[16]["cmd"], clipped)
    # no contacts: phase 1 for T ticks
    rb, log = drive(D4, {13: R.BTN_X}, 21, four=False)
    assert kinds(log, 13, 21) == ["repeat"] + ["p1"] * 4 + ["repeat", "run", "run"]
    assert [o["out"][4] for o in log[14:19]] == [1, 2, 3, 4, 0] and log[18]["flags"] == R.DONE
    assert [o["entered"] for o in log[18:21]] == [False, True, False]


def test_x_again_is_a_gait_transition():
    stand = np.asarray(D4["stand_up_angles"], f32)
    rb, log = drive(D4, {13: R.BTN_X, 18: R.BTN_X}, 30, four=lambda t: t < 18)
    assert kinds(log, 16, 30) == ["run", "run"] + ["p1"] * 4 + ["p2"] * 4 + ["repeat"] + ["run"] * 3
    assert log[26]["flags"] == R.DONE and [o["entered"] for o in log[26:29]] == [False, True, False]
    assert [o["out"][2] for o in log[17:28]] == [R.K_LOCOMOTION] + [R.GAIT_TRANSITION] * 8 + [R.K_LOCOMOTION] * 2
    for k, ratio in zip(range(22, 26), (0.45, 0.45, 0.5, 0.75)):       # max(0.45f, (iter - T) / T), iter 4, 5, 6, 7
        assert np.array_equal(log[k]["cmd"], pd(D4, stand * f32(ratio) + (f32(1) - f32(ratio)) * ANGLES)), k
    assert np.array_equal(log[26]["cmd"], log[25]["cmd"])
    assert log[27]["out"][3] == R.JOY_ADVANCED_TROT and log[27]["out"][8] == 2 and log[27]["out"][9] == R.ADVANCED_TROT
    assert list(log[27]["joy"][:6]) == [f32(1.0) * f32(0.2), f32(-1.0) * f32(0.1), 0, 0, 0, f32(0.5) * f32(0.2)]    # the axes of the last message, kept while trotting
    assert list(log[17]["joy"][:6]) == [0] * 6                            # zeroed in JOY_STAND
    # four contacts at the first phase-1 tick: iter jumps to T, the blend starts at iter 5
    rb, log = drive(D4, {13: R.BTN_X, 18: R.BTN_X}, 26, four=True)
    assert kinds(log, 18, 26) == ["p1"] + ["p2"] * 3 + ["repeat"] + ["run"] * 3
    # X once more: the gaits cycle JOY_ADVANCED_TROT -> JOY_TROT (the modulus, then "> JOY_ADVANCED_TROT")
    rb, log = drive(D4, {0: R.BTN_X}, 12, four=True, robot=rb)
    assert log[11]["out"][3] == R.JOY_TROT and log[11]["out"][8] == 1 and log[11]["out"][9] == R.VELOCITY_LOCOMOTION


def test_rb_sits_down_and_rb_again_stands_up():
    stand, sit = np.asarray(D4["stand_up_angles"], f32), np.asarray(D4["sit_down_angles"], f32)
    rb, log = drive(D4, {13: R.BTN_RB, 14: R.BTN_RB, 21: R.BTN_RB}, 36)
    assert kinds(log, 12, 36) == ["hold"] * 2 + ["act"] * 6 + ["hold"] + ["act"] * 12 + ["hold"] * 3
    assert log[13]["out"][3] == R.BODY_UP and log[14]["out"][3] == R.BODY_DOWN and log[14]["out"][2] == R.K_STAND_DOWN and log[14]["out"][10] == -1
    assert log[14]["flags"] == R.ACTION_FIRST and log[20]["flags"] == R.ACTION_END and log[21]["flags"] == R.ACTION_FIRST and log[33]["flags"] == R.ACTION_END
    for k in range(6):
        blend = f32(k * 0.25) / f32(1.5)
        assert np.array_equal(log[14 + k]["cmd"], pd(D4, blend * sit + (f32(1) - blend) * ANGLES)), k
    assert np.array_equal(log[20]["cmd"], pd(D4, sit)) and np.array_equal(log[33]["cmd"], pd(D4, stand)) and np.array_equal(log[35]["cmd"], pd(D4, stand))
    assert log[21]["out"][3] == R.BODY_UP and log[21]["out"][2] == R.K_STAND_UP
    # a press during the action waits for its end: RB at tick 3 of the stand-up is acted on at tick 13, the first tick after the hold that ends it
    rb, log = drive(D4, {3: R.BTN_RB, 5: R.BTN_RB}, 16)
    assert kinds(log, 0, 16) == ["act"] * 12 + ["hold"] + ["act"] * 3 and log[12]["out"][3] == R.BODY_UP and log[13]["out"][3] == R.BODY_DOWN


def test_y_while_sitting_goes_passive():
    rb, log = drive(D4, {13: R.BTN_RB, 14: R.BTN_RB, 21: R.BTN_Y, 25: R.BTN_RB, 27: R.BTN_X}, 32)
    assert kinds(log, 20, 32) == ["hold"] + ["passive"] * 11
    assert log[21]["flags"] == R.DONE and all(o["flags"] == 0 for o in log[22:])
    assert all(not o["cmd"].any() for o in log[21:]) and [o["out"][0] for o in log[20:23]] == [R.STAND_UP, R.PASSIVE, R.PASSIVE]
    # joyCmdExit is never cleared: RB leaves EXIT in place, X cycles EXIT -> (HARD_CODE, skipped) -> JOY_TROT, which Passive does not answer
    assert log[25]["out"][3] == R.EXIT and log[27]["out"][3] == R.JOY_TROT and log[31]["out"][0] == R.PASSIVE and log[31]["out"][2] == R.GAIT_TRANSITION
    # Y while standing up (bodyUp 0, not moving) exits as well; Y while moving is ignored
    rb, log = drive(D4, {13: R.BTN_Y}, 15)
    assert kinds(log, 13, 15) == ["passive"] * 2
    rb, log = drive(D4, {13: R.BTN_X, 16: R.BTN_Y}, 18, four=True)
    assert kinds(log, 16, 18) == ["run"] * 2


def test_after_passive_the_locomotion_clip_is_off():
    rb, log = drive(D4, {13: R.BTN_X, 17: R.BTN_B, 21: R.BTN_Y}, 24, four=True)
    assert kinds(log, 16, 24) == ["run", "p1", "repeat", "run", "run", "passive", "passive", "passive"]
    assert log[20]["cmd"][48] == 23 and log[20]["cmd"][49] == -23 and rb.state_rows()[21] == 0 and log[21]["flags"] == R.DONE
    assert list(log[20]["out"][5:8]) == [1, 0, 1] and list(log[21]["out"][5:8]) == [0, 0, 0]
    # Transition() turned the locomotion state's checks off for good (qr_fsm_state_locomotion.cpp:250): put back into locomotion, the state does not clip
    rb.state, rb.nextState, rb.fsmMode, rb.l["next"] = R.LOCOMOTION, R.LOCOMOTION, R.K_LOCOMOTION, R.LOCOMOTION
    rb, log = drive(D4, {}, 1, robot=rb)
    assert kinds(log, 0, 1) == ["run"] and log[0]["cmd"][48] == 40 and log[0]["cmd"][49] == -40 and list(log[0]["out"][5:8]) == [0, 0, 0]


def test_leaving_locomotion_for_the_stand_up_state():
    """RB in MPC standing: BODY_UP -> K_STAND_UP -> STAND_UP by a one-tick transition that sends the last run's command; OnEnter asks for a stand-up."""
    rb, log = drive(D4, {13: R.BTN_X, 17: R.BTN_B, 20: R.BTN_RB}, 36, four=True)
    assert kinds(log, 19, 36) == ["run", "repeat"] + ["act"] * 12 + ["hold"] * 3
    assert log[20]["flags"] == R.DONE and np.array_equal(log[20]["cmd"], log[19]["cmd"]) and log[21]["flags"] == R.ACTION_FIRST


def test_the_streams_reach_every_branch():
    R.Robot.cov.clear()
    ref = R.reference(D=dict(R.SHORT))
    cov = R.Robot.cov
    # every state x operating mode a joystick can reach: PASSIVE is never left (joyCmdExit is never cleared, so K_STAND_UP cannot be asked for there)
    assert {(R.STAND_UP, 0), (R.STAND_UP, 1), (R.LOCOMOTION, 0), (R.LOCOMOTION, 1), (R.PASSIVE, 0)} <= cov and (R.PASSIVE, 1) not in cov
    joy = {"A on", "A off", "X first", "X again", "axes", "axes off", "B stop", "B stand", "B down", "Y exit", "Y ignored", "RB first", "RB flip", "RB moving"}
    block = {"gaitSwitch", "to stand", "to advanced trot", "cycle next", "cycle past hard code", "cycle to trot", "prev kept", "exit", "body down", "body up", "stand"}
    loops = {"switch mode done", "switch mode: four contacts", "switch mode: phase 1 goes on", "switch mode: floor", "switch mode: ramp", "stand loop done",
             "stand loop: four contacts", "stand loop: phase 1 goes on"}
    assert joy | block | loops <= cov, (joy | block | loops) - cov
    assert {"message during an action", "reset during an action", "reset during a transition", "reset"} <= cov
    paths = ref["paths"]
    assert (paths[..., 0] & ~paths[..., 1]).sum() > 1000 and (paths[..., 1] & ~paths[..., 0]).sum() > 100 and (paths[..., 0] & paths[..., 1]).sum() >= 1
    kind = ref["plan"] & 0x7f
    for k in KINDS:
        assert (kind == k).sum() > 500, KINDS[k]
    for flag in (R.DONE, R.ACTION_FIRST, R.ACTION_END):
        assert (ref["plan"] & flag != 0).sum() > 100, flag
    assert (ref["mask"] & R.ENTERED != 0).sum() > 100
    tua = ref["cmd"][:, 48:60]
    assert (np.abs(tua) == 23).sum() > 1000 and not (np.abs(tua) > 23).any()             # the chain's torques reach +-40: clipped wherever they are passed on
    assert (ref["state"][:, 21] == 0).sum() > 1000                                           # robots whose locomotion checks Transition() has turned off
    assert set(np.unique(ref["out"][:, 3])) == {float(x) for x in (R.JOY_TROT, R.JOY_ADVANCED_TROT, R.JOY_STAND, R.BODY_UP, R.BODY_DOWN, R.EXIT)}


def test_tick_counts_at_the_reference_s_durations():
    """One robot at the defaults (time_step 0.001, transition_ticks 1000), no contacts: K stand-up ticks, 1000 ticks of the stand loop, 1000 + 1000 of the
    gait transition."""
    K, t = 0, f32(0)
    while t < f32(3.0):
        t = f32(t + f32(0.001)); K += 1
    assert 2990 <= K <= 3010
    rb, log = drive(R.A1, {K + 1: R.BTN_X, K + 1010: R.BTN_X}, K + 3020)
    k = [o["kind"] for o in log]
    assert k[:K] == ["act"] * K and k[K] == "hold" and log[K]["flags"] == R.ACTION_END
    assert k[K + 1] == "repeat" and k[K + 2:K + 1002] == ["p1"] * 1000 and k[K + 1002] == "repeat" and k[K + 1003:K + 1010] == ["run"] * 7
    assert k[K + 1010:K + 2010] == ["p1"] * 1000 and k[K + 2010:K + 3010] == ["p2"] * 1000 and k[K + 3010] == "repeat" and k[K + 3011:] == ["run"] * 9
    first_ramp = next(i for i in range(K + 2010, K + 3010) if not np.array_equal(log[i]["cmd"][:12], log[K + 2010]["cmd"][:12]))
    assert first_ramp == K + 2010 + 451                                     # (iter - 1000) / 1000.0f exceeds 0.45f first at iter 1451


def passive_robot_asked_to_stand_up(D):
    """A robot gone passive -- RB, RB and Y pressed during its first stand-up, acted on when that ends -- then fsmMode written to K_STAND_UP: the one
    request the joystick cannot make there (above)."""
    rb, log = drive(D, {0: R.BTN_RB, 1: R.BTN_RB, 2: R.BTN_Y}, 3)
    for _ in range(5000):
        rb, log = drive(D, {}, 1, robot=rb)
        if log[0]["out"][0] == R.PASSIVE:
            break
    rb, log = drive(D, {}, 2, robot=rb)
    assert log[1]["kind"] == "passive" and log[1]["flags"] == 0 and log[1]["out"][3] == R.EXIT
    rb.fsmMode = R.K_STAND_UP
    return rb


def test_passive_answers_k_stand_up():
    """qrFSMStatePassive::CheckTransition -> STAND_UP (qr_fsm_state_passive.cpp:73-75): a one-tick transition with an empty command, then OnEnter's stand-up"""
    R.Robot.cov.clear()
    rb, log = drive(D4, {}, 15, robot=passive_robot_asked_to_stand_up(D4))
    assert (R.PASSIVE, 1) in R.Robot.cov
    assert kinds(log, 0, 15) == ["passive"] + ["act"] * 12 + ["hold"] * 2 and log[0]["flags"] == R.DONE and log[1]["flags"] == R.ACTION_FIRST
    assert not log[0]["cmd"].any() and log[0]["out"][0] == R.STAND_UP and log[13]["flags"] == R.ACTION_END
    assert np.array_equal(log[14]["cmd"], pd(D4, D4["stand_up_angles"]))
