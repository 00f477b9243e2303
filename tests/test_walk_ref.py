"""CPU: tests/walk_ref.py (the walk gait generator written from the reference line by line) against the closed form of its schedule and the
reference's Reset semantics, and oracle/qr_oracle_walk.cpp against walk_ref, bit for bit on all 41 output rows and the 33 state rows, on every
tick of every robot of every family of walk_ref.FAMILIES."""
import numpy as np
import pytest

import walk_ref as R

STANCE, LOAD, UNLOAD, FULL, TRUE_SWING = R.STANCE, R.LOAD_FORCE, R.UNLOAD_FORCE, R.FULL_STANCE, R.TRUE_SWING


@pytest.mark.parametrize("name", R.FAMILIES)
def test_oracle_is_the_model_on_every_tick(pkg, oracle, name):
    f, want, wst, clamped = R.expected(pkg, name)
    for r in range(R.N_ROBOTS):
        got, gst = oracle.walk_run(f["cfg"], f["time"], f["contact"][:, r], f["stop"], f["reset"], want_state=True)
        bad = np.nonzero((want[r] != got).any(axis=1))[0]
        assert bad.size == 0, (name, r, bad[:3], want[r][bad[0]], got[bad[0]])
        bad = np.nonzero((wst[r] != gst).any(axis=1))[0]
        assert bad.size == 0, (name, r, bad[:3], wst[r][bad[0]], gst[bad[0]])
    # every sub-state of the family's queue and every detected state occur (the feet of threshold 1 are never asked in true swing:
    # its normalizedPhase stays below 1 there)
    des = set(np.unique(want[:, :, 8:12]).astype(int)); det = set(np.unique(want[:, :, 20:24]).astype(int))
    assert des >= {1, 5, 6, 8} | ({7} if name != "swing_start" else set()), (name, des)
    assert det >= ({0, 1, 3} if name == "threshold_1" else {0, 1, 2, 3}), (name, det)
    # the fork (index past the queue) is met by the family built for it and by no other
    assert (clamped.min() > 0) if name == "long_step" else (clamped.max() == 0), (name, clamped)


def test_schedule_closed_form(pkg):
    """The closed form tests/test_oracle_walk.py holds the oracle to, on the model: phase = fmod(initial_phase * T + t, T) / T, the sub-state from
    the phase in the swing quarter (away from the boundaries: the index advances one tick late), never two legs out of STANCE."""
    cfg = pkg.workload.walk_cfg()
    T, dt = 2600, 0.005                                    # 13 s: more than one 10 s cycle
    t = (np.arange(T) * dt).astype(np.float32)
    o = R.run(cfg, t, np.ones((T, 4), np.float32))
    c = np.ones((T, 4), np.float32); c[o[:, 8:12] == TRUE_SWING] = 0
    o = R.run(cfg, t, c)
    full = 7.5 / 0.75
    init = cfg[8:12].astype(np.float64)
    for l in range(4):
        ph = np.fmod(init[l] * full + t.astype(np.float64), full) / full
        assert np.abs(o[:, l] - ph).max() < 2e-6
        psc = (ph - 0.75) / 0.25
        want = np.where(ph <= 0.75, STANCE, np.where(psc < 0.2, FULL, np.where(psc < 0.5, UNLOAD, np.where(psc < 0.8, TRUE_SWING, LOAD))))
        edge = np.zeros(T, bool)
        for b in (0.75, 0.75 + 0.25 * 0.2, 0.75 + 0.25 * 0.5, 0.75 + 0.25 * 0.8, 1.0, 0.0):
            edge |= np.abs(ph - b) < 2 * dt / full + 1e-6
        assert np.array_equal(o[~edge, 8 + l], want[~edge].astype(np.float32)), l
        # normalizedPhase is the position inside the sub-state (inside the stance phase for STANCE)
        lo = np.select([want == FULL, want == UNLOAD, want == TRUE_SWING, want == LOAD], [0.0, 0.2, 0.5, 0.8], 0.0)
        wid = np.select([want == FULL, want == UNLOAD, want == TRUE_SWING, want == LOAD], [0.2, 0.3, 0.3, 0.2], 1.0)
        nph = np.where(want == STANCE, ph / 0.75, (psc - lo) / wid)
        assert np.abs(o[~edge, 4 + l] - nph[~edge]).max() < 1e-4
        assert set(np.unique(o[:, 12 + l])) <= {0.0, 1.0}                       # legState is only ever SWING / STANCE
        assert np.array_equal(o[1:, 16 + l], o[:-1, 8 + l])                     # curLegState trails desiredLegState by one tick
    assert ((o[:, 8:12] != STANCE).sum(1) <= 1).all()                           # the legs take turns: never two legs out of STANCE
    des, nph = o[:, 8:12], o[:, 4:8]
    cont, fmin, fmax = o[:, 29:33], o[:, 33:37], o[:, 37:41]
    assert np.all(fmin == np.float32(0.001))
    assert np.all(cont[des == TRUE_SWING] == 0) and np.all(fmax[des == TRUE_SWING] == np.float32(0.002)) and np.all(cont[des != TRUE_SWING] == 1)
    assert np.all(fmax[(des == STANCE) | (des == FULL)] == 10.0)
    assert np.array_equal(fmax[des == LOAD], np.float32(10) * np.maximum(np.float32(0.001), nph[des == LOAD]))
    m = des == UNLOAD
    assert np.allclose(fmax[m], 10 * np.maximum(0.001, 1 - nph[m] / 0.75), rtol=1e-5, atol=1e-6)
    # moveBasePhase ramps over the stance-like head of the swing quarter (0.5 of it), then holds 1
    ph = np.fmod(init[1] * full + t.astype(np.float64), full) / full
    k = np.nonzero((ph > 0.76) & (ph < 0.87))[0]
    assert np.allclose(o[k, 28], ((ph[k] - 0.75) / 0.25) / 0.5, atol=1e-4)
    k = np.nonzero((ph > 0.88) & (ph < 0.99))[0]
    assert np.all(o[k, 28] == 1.0)


def test_never_two_legs_out_of_stance_in_any_regular_family(pkg):
    for name in ("yaml", "robot_stop", "reset", "late_clock", "threshold_0", "threshold_1"):
        _, out, _, _ = R.expected(pkg, name)
        assert ((out[:, :, 8:12] != STANCE).sum(axis=2) <= 1).all(), name


def test_constructor_bookkeeping(pkg):
    W = pkg.workload
    g = R.WalkGaitGenerator(W.walk_cfg())
    assert g.stateSwitchQue == [FULL, UNLOAD, TRUE_SWING, LOAD] and g.stateIndexOfLegs == [0, 0, 0, 0]
    assert np.array_equal(g.accumStateRatioQue, np.cumsum(np.float32([0, 0.2, 0.3, 0.3, 0.2]), dtype=np.float32))
    assert g.trueSwingStartPhaseInSwingCycle == np.float32(0.2) + np.float32(0.3)
    # a ratio below 0.01 drops its entry; the sum in front of true_swing is taken over what is kept, in queue order
    g = R.WalkGaitGenerator(W.walk_cfg(state_switch=(7, 5, 8, 6), state_ratio=(0.005, 0.2, 0.4, 0.4)))
    assert g.stateSwitchQue == [LOAD, TRUE_SWING, UNLOAD] and g.trueSwingStartPhaseInSwingCycle == np.float32(0.2)
    assert np.float64(np.float32(0.01)) < 0.01                                 # 0.01f itself is below the double 0.01: dropped as well
    assert R.WalkGaitGenerator(W.walk_cfg(state_ratio=(0.01, 0.3, 0.3, 0.4))).stateSwitchQue == [UNLOAD, TRUE_SWING, LOAD]
    # a leg that starts in SWING: its index comes from (initial phase - duty) / duty -- the reference's division -- against the running sums
    for ph0, idx in ((0.76, 0), (0.9, 0), (0.91, 1), (0.99, 1)):
        g = R.WalkGaitGenerator(W.walk_cfg(initial_leg_phase=(ph0, 0.1, 0.6, 0.35), initial_leg_state=(0, 1, 1, 1)))
        assert g.stateIndexOfLegs == [idx, 0, 0, 0], (ph0, g.stateIndexOfLegs)   # (0.9 - 0.75) / 0.75 = 0.2: not beyond accum[1]; 0.91 is
    with pytest.raises(ValueError):
        R.WalkGaitGenerator(W.walk_cfg(state_ratio=(0.2, 0.3, 0.3, 0.3)))


def test_reset_in_mid_run_keeps_what_the_reference_keeps(pkg):
    """Reset rewrites cur / leg / desired state and normalizedPhase (then the tick's Update runs); stateIndexOfLegs, detectedLegState,
    detectedEventTickPhase, moveBasePhase and phaseInFullCycle are left as they were."""
    f, _, _, _ = R.expected(pkg, "reset")
    for r in (0, 7, 64):
        g = R.WalkGaitGenerator(f["cfg"])
        for k in range(f["time"].size):
            if f["reset"][k]:
                before = g.state33()
                g.Reset(f["time"][k])
                after = g.state33()
                init = f["cfg"][12:16]
                assert np.array_equal(after[0:4], init) and np.array_equal(after[4:8], init) and np.array_equal(after[8:12], init)
                assert np.all(after[24:28] == 0)
                assert np.array_equal(after[12:24], before[12:24]) and np.array_equal(after[28:33], before[28:33])
                assert (before[16:20] != 0).any() and (before[20:24] != 0).all() and before[32] != 0          # ... and there was something to keep
                swing_leg = int(np.argmax(before[16:20]))
            g.Update(f["time"][k], f["contact"][k, r], bool(f["stop"][k]))
            if f["reset"][k]:
                # the leg in its swing quarter goes on in the sub-state it was in: the index survived, so it does not start over at full_stance
                assert g.state33()[4 + swing_leg] == before[4 + swing_leg] and g.state33()[16 + swing_leg] == before[16 + swing_leg]
                assert g.state33()[swing_leg] == STANCE                          # curLegState: the initial state, for this one tick
    assert set(f["marks"]) == {"in_true_swing", "in_load_force"}


def test_robot_stop_windows_open_in_every_sub_state(pkg):
    f, out, st, _ = R.expected(pkg, "robot_stop")
    assert sorted(f["marks"]) == sorted(R.SUB_STATES)
    for s, k in f["marks"].items():
        assert f["stop"][k] == 1 and f["stop"][k - 1] == 0 and (out[0, k, 8:12] == s).any()
        # curLegState only follows desiredLegState for legs in SWING (:218): curLegState never holds SWING here, so all four freeze
        assert np.all(st[:, k:k + R.STOP_LENGTH, 0:4] == st[:, k - 1:k, 0:4])
    ends = [k + R.STOP_LENGTH - 1 for k in f["marks"].values()]
    assert any((out[0, k, 8:12] != st[0, k, 0:4]).any() for k in ends)          # ... while the plan moved on under at least one window
    free = R.run(f["cfg"], f["time"], f["contact"][:, 3])
    assert np.array_equal(out[3, :, 0:4], free[:, 0:4]) and np.array_equal(out[3, :, 8:12], free[:, 8:12])      # the plan follows the clock


def test_long_step_takes_the_fork_once_and_recovers(pkg):
    f, out, st, clamped = R.expected(pkg, "long_step")
    k = f["marks"]["long_step"]
    assert np.isclose(f["time"][k] - f["time"][k - 1], 0.1, atol=1e-6)
    o = out[0]
    assert o[k - 1, 8] == LOAD and o[k, 8] == LOAD and o[k, 0] > 0.75 and o[k, 4] < 0                 # still "load_force", before its start
    assert st[0, k, 16] == 3
    later = np.nonzero(o[k:, 8] == STANCE)[0][0] + k
    assert st[0, later, 16] == 0 and set(o[later:, 8]) == {1.0, 5.0, 6.0, 7.0, 8.0}


def test_contact_detection_threshold(pkg):
    _, o0, _, _ = R.expected(pkg, "threshold_0")
    _, o1, _, _ = R.expected(pkg, "threshold_1")
    f = R.family(pkg, "threshold_0")
    # threshold 0: every foot down in true swing is EARLY_CONTACT, every foot up in STANCE is LOSE_CONTACT, from the first tick of the sub-state
    c = f["contact"].transpose(1, 0, 2)
    ts, sta = o0[:, :, 8:12] == TRUE_SWING, o0[:, :, 8:12] == STANCE
    assert np.all(o0[:, :, 20:24][ts & (c != 0)] == 2) and np.all(o0[:, :, 20:24][sta & (c == 0)] == 3)
    assert np.all(o0[:, :, 20:24][ts & (c == 0)] == 0) and np.all(o0[:, :, 20:24][sta & (c != 0)] == 1)
    # threshold 1: only a normalizedPhase of 1 or more is asked: nothing in true swing, and in STANCE only the tick that sits on the duty factor
    asked = o1[:, :, 4:8] >= 1
    assert np.all(o1[:, :, 20:24][~asked] <= 1) and not (o1[:, :, 20:24] == 2).any()
