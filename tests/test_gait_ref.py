"""CPU: tests/gait_ref.py (the open-loop gait generator written from the reference line by line) against the properties of the reference's
state machine, and oracle/qr_oracle_gait.cpp against gait_ref, bit for bit, on the six configurations of gait_ref.CONFIGS."""
import numpy as np

import gait_ref as G


def test_oracle_gait_is_bit_exact_on_every_configuration(pkg, oracle):
    for name in G.CONFIGS:
        c = G.configuration(pkg, name)
        seen = set()
        for r in range(G.N_ROBOTS):
            want, wst = G.run(c["cfg"], c["time"], c["contact"][:, r], c["stop"], c["reset"], want_state=True)
            got, gst = oracle.gait_run(c["cfg"], c["time"], c["contact"][:, r], c["stop"], c["reset"], want_state=True)
            bad = np.nonzero((want != got).any(axis=1))[0]
            assert bad.size == 0, (name, r, bad[:3], want[bad[0]], got[bad[0]])
            bad = np.nonzero((wst != gst).any(axis=1))[0]
            assert bad.size == 0, (name, r, bad[:3], wst[bad[0]], gst[bad[0]])
            seen |= set(np.unique(want[:, 12:16]).tolist())
            if (np.diff(wst[:, 2]) > 0).any():
                seen.add("hold")
        # every configuration meets EARLY_CONTACT, and the hold unless the plain trot switches it off
        assert 2.0 in seen, name
        assert ("hold" in seen) == (name != "plain_trot"), name


def test_phases_are_the_closed_form_with_every_foot_in_contact(pkg):
    """With every foot in contact the generator never holds: phase = fmod(initial_phase * T + t, T) / T up to one tick of slip per cycle (the
    clock restart of Schedule fires on the first tick strictly after a full period), as tests/test_oracle_gait.py has it for the oracle."""
    cfg = pkg.workload.gait_cfg()
    T, dt = 1500, 0.002
    full = 0.5 / 0.6
    t = (np.arange(T) * dt).astype(np.float32)
    ph = np.stack([np.fmod(cfg[8 + l] * full + t.astype(np.float64), full) / full for l in range(4)], 1)
    o, st = G.run(cfg, t, np.ones((T, 4), np.float32), want_state=True)
    err = np.abs(o[:, 0:4] - ph); err = np.minimum(err, 1 - err)
    assert err.max() < 4 * dt / full + 1e-4
    assert np.array_equal(o[:, 8:12] == 1, o[:, 0:4] < np.float32(0.6))
    assert np.all(st[:, 2] == 0) and np.all(st[:, 20:24] == 1)                      # cumDt stays 0, every leg may switch
    # gaitCycle counts the clock restarts: resetTime jumps to the current time exactly when the counter goes up
    restarts = np.nonzero(np.diff(st[:, 0]) != 0)[0] + 1
    assert restarts.size == 3 and np.array_equal(np.nonzero(np.diff(st[:, 3]) != 0)[0] + 1, restarts)
    assert np.array_equal(st[restarts, 0], t[restarts]) and st[-1, 3] == 3
    # firstSwing is raised on the tick a stance leg's desired state turns to swing, firstStance when a swinging leg is planned or found down
    for l in range(4):
        lift = (o[1:, 8 + l] == 0) & (o[:-1, 8 + l] == 1)
        assert np.array_equal(st[1:, 24 + l][lift], np.ones(lift.sum())) and np.all(o[1:, 20 + l][lift] == np.float32(full) - np.float32(0.5))
    sw = o[:, 8] == 0
    assert np.all(np.diff(o[sw, 20][:100]) <= 0) and o[sw, 20].min() >= 0                 # swingTimeRemaining runs down


def _late_contact_stream(cfg, t):
    nominal = G.run(cfg, t, np.ones((t.size, 4), np.float32))
    k0 = int(np.argmax((nominal[1:, 8] == 1) & (nominal[:-1, 8] == 0))) + 1           # leg 0's first planned touch-down
    c = np.ones((t.size, 4), np.float32); c[k0 - 2:k0 + 200, 0] = 0                    # ... which does not come
    return nominal, k0, c


def test_hold_ends_on_the_first_tick_past_wait_time(pkg):
    cfg = pkg.workload.gait_cfg(wait_time=0.05)
    t = (np.arange(1200) * 0.002).astype(np.float32)
    _, k0, c = _late_contact_stream(cfg, t)
    o, st = G.run(cfg, t, c, want_state=True)
    held = np.nonzero(st[:, 20] == 0)[0]                                               # ticks on which leg 0 may not switch
    assert held.size and held[0] == k0 + 1 and np.array_equal(held, np.arange(held[0], held[0] + held.size))
    assert np.all(o[held, 0:4] == o[held[0] - 1, 0:4])                                 # the phases stand still
    cum = st[:, 2]
    rel = held[-1] + 1                                                                 # the release tick: cumDt > wait_time for the first time
    assert cum[rel] > np.float32(0.05) and np.all(cum[held] <= np.float32(0.05)) and np.all(st[rel, 20:24] == 1)
    assert np.all(np.diff(cum[held[0] - 1:rel + 1]) > 0)
    assert held.size == 25                                                             # 0.05 s of 2 ms ticks: the 26th exceeds it
    # the release lets the leg's planned state switch to STANCE; cumDt is left standing on that tick and cleared by the next, which finds no late leg
    assert st[rel, 4] == 1 and cum[rel + 1] == 0 and not np.array_equal(o[rel + 5, 0:4], o[rel, 0:4])


def test_release_does_not_clear_cum_dt(pkg):
    """robot->stop raised one tick after leg 0 lifts off pins it at cur = SWING, last = STANCE.  When its touch-down then does not come, the hold
    is released after wait_time -- and on every tick after that as well, because cumDt is cleared only by a tick without a late leg: it keeps
    growing and the clock runs.  (A generator that cleared cumDt on release would hold again for wait_time, over and over.)"""
    cfg = pkg.workload.gait_cfg(wait_time=0.05)
    T = 900
    t = (np.arange(T) * 0.002).astype(np.float32)
    _, st0 = G.run(cfg, t, np.ones((T, 4), np.float32), want_state=True)
    lift = int(np.argmax((st0[:, 4] == 0) & (st0[:, 8] == 1)))                        # cur = SWING, last = STANCE on this tick
    stop = np.zeros(T, np.int32); stop[lift + 1:] = 1
    c = np.ones((T, 4), np.float32); c[lift:, 0] = 0
    o, st = G.run(cfg, t, c, stop, want_state=True)
    assert np.all(st[lift:, 4] == 0) and np.all(st[lift:, 8] == 1)
    hold0 = int(np.argmax(st[:, 20] == 0))
    assert hold0 > lift
    rel = hold0 + int(np.argmax(st[hold0:, 2] > np.float32(0.05)))
    assert rel - hold0 == 25
    end = hold0 + 200                                                                # (the plan for leg 0 says STANCE for 0.5 s = 250 ticks)
    assert np.all(np.diff(st[hold0 - 1:end, 2]) > 0) and st[end - 1, 2] > 0.39          # never cleared, never restarted
    assert np.all(st[rel:end, 20:24] == 1)                                           # released on every tick from there on
    ph = o[rel:rel + 100, 1]
    assert np.unique(ph).size > 90                                                   # the clock runs


def test_plain_trot_never_stops_the_clock(pkg):
    t = (np.arange(1200) * 0.002).astype(np.float32)
    adv = pkg.workload.gait_cfg(wait_time=0.05)
    plain = pkg.workload.gait_cfg(wait_time=0.05, advanced_trot=False)
    nominal, k0, c = _late_contact_stream(adv, t)
    o, st = G.run(plain, t, c, want_state=True)
    assert np.all(st[:, 20:24] == 1) and np.all(st[:, 2] == 0)
    assert np.array_equal(o[:, 0:12], nominal[:, 0:12]) and np.array_equal(st[:, 0], G.run(plain, t, np.ones((t.size, 4), np.float32), want_state=True)[1][:, 0])


def test_robot_stop_freezes_the_planned_state_of_stance_legs(pkg):
    """robot->stop: curLegState / lastLegState move on only for legs whose lastLegState is SWING; the phases and the desired state run on."""
    cfg = pkg.workload.gait_cfg()
    t = (np.arange(900) * 0.002).astype(np.float32)
    stop = np.zeros(900, np.int32); stop[300:] = 1
    o, st = G.run(cfg, t, np.ones((900, 4), np.float32), stop, want_state=True)
    free = G.run(cfg, t, np.ones((900, 4), np.float32))
    assert np.array_equal(o[:, 0:12], free[:, 0:12])
    for l in range(4):
        cur, last = st[:, 4 + l], st[:, 8 + l]
        for k in range(301, 900):
            if last[k - 1] == 0:
                assert last[k] == cur[k - 1] and cur[k] == o[k - 1, 8 + l]
            else:
                assert last[k] == last[k - 1] and cur[k] == cur[k - 1]
        assert np.all(cur[-200:] == cur[-1])                                           # every leg ends up frozen


def test_reset_in_mid_run_keeps_what_the_reference_keeps(pkg):
    c = G.configuration(pkg, "reset")
    assert np.array_equal(np.nonzero(c["reset"])[0], G.RESET_TICKS)
    for r, k in ((0, G.RESET_TICKS[0]), (7, G.RESET_TICKS[0]), (0, G.RESET_TICKS[1]), (7, G.RESET_TICKS[1])):
        o, st = G.run(c["cfg"], c["time"], c["contact"][:, r], c["stop"], c["reset"], want_state=True)
        assert st[k, 1] == c["time"][k]
        if k == G.RESET_TICKS[0]:            # t = 0.8 s, less than a period: resetTime = 0 although the time runs on; no restart yet
            assert st[k, 0] == 0 and st[k, 3] == st[k - 1, 3] == 0
        else:                                # t = 1.2 s, more than a period after the new resetTime: the clock restarts at once, and gaitCycle
            assert st[k, 0] == c["time"][k] and st[k, 3] == st[k - 1, 3] + 1 >= 2      # goes on counting from where it was
        init = c["cfg"][12:16]
        assert np.array_equal(st[k, 4:8], init) and np.array_equal(st[k, 8:12], init)  # cur := desired(=initial), last := cur(=initial)
        stance = o[k, 8:12] == 1
        assert stance.any() and np.array_equal(o[k, 20:24][stance], o[k - 1, 20:24][stance])      # swingTimeRemaining survives until the next swing
    assert (o[k - 1, 20:24] != 0).any()


def test_swing_start_and_early_contact(pkg):
    """Legs that start in SWING; a foot that touches down in the second half of its swing becomes EARLY_CONTACT with contactStartPhase =
    phase - 1, stays so while the plan says SWING, and counts as firstStance."""
    cfg = pkg.workload.gait_cfg(stance_duration=0.3, duty_factor=0.5, initial_leg_state=(0, 1, 1, 0), wait_time=0.06)
    t = (np.arange(600) * 0.002).astype(np.float32)
    c = np.ones((600, 4), np.float32)
    o, st = G.run(cfg, t, c, want_state=True)
    assert np.array_equal(st[0, 4:8], [0, 1, 1, 0])
    early = np.nonzero(o[:, 12] == 2)[0]
    assert early.size and np.all(o[early, 4] >= np.float32(0.5)) and np.all(o[early, 8] == 0)
    k = early[0]
    assert st[k, 40] == o[k, 0] - np.float32(1) and st[k, 28] == 1 and st[k, 24] == 0
    sw_first_half = (o[:, 8] == 0) & (o[:, 4] < np.float32(0.5)) & (np.arange(600) > 0)
    prev_early = np.concatenate([[False], o[:-1, 12] == 2])
    assert np.all(o[sw_first_half & ~prev_early, 12] == 0)                               # below the detection threshold contact is ignored
