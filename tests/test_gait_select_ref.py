"""CPU: tests/gait_select_ref.py -- the open-loop generator whose Reset re-reads the gait's parameters -- against tests/gait_ref.py where the gait is
held constant, against a fresh generator at a CONSTRUCT reset, and on a LIVE switch advanced_trot -> stand -> trot; and the default gait table of the
library and of workload.gait_table() against the numbers of config/a1_sim/openloop_gait_generator.yaml written out here."""
import ctypes as C

import numpy as np
import pytest

import gait_ref as G
import gait_select_ref as R

_f = np.float32
# config/a1_sim/openloop_gait_generator.yaml: stance_duration, duty_factor, init_phase_full_cycle, contact_detection_phase_threshold, advanced_trot hold
YAML = {"trot": (0.3, 0.6, (0.5, 0.0, 0.0, 0.5), 0.5, 0), "advanced_trot": (0.5, 0.6, (0.5, 0.0, 0.0, 0.5), 0.5, 1),
        "walk": (7.5, 0.75, (0.5, 0.0, 0.75, 0.25), 0.1, 0), "stand": (0.3, 1.0, (0.0, 0.0, 0.0, 0.0), 0.1, 0)}
ORDER = ("advanced_trot", "trot", "advanced_trot", "walk", "stand")          # 0 none yet, then QRGPU_FSM_GAIT_*


@pytest.mark.parametrize("name", ["default", "reset", "irregular_clock"])
@pytest.mark.parametrize("entry", range(5))
def test_a_constant_selection_is_gait_ref(pkg, entry, name):
    """Entry `entry` selected at every tick, Reset(0) where the configuration has one: bit for bit gait_ref.run with that entry's row, 65 robots, 700 ticks."""
    table = pkg.workload.gait_table()
    c = G.configuration(pkg, name)
    level = np.where(c["reset"] != 0, R.LIVE, 0); level[0] = R.CONSTRUCT
    sel = np.full(G.TICKS, entry, _f)
    for r in range(G.N_ROBOTS):
        want, wst = G.run(table[entry], c["time"], c["contact"][:, r], c["stop"], c["reset"], want_state=True)
        got = R.run(table, c["time"], c["contact"][:, r], sel, level, c["stop"])
        assert R.same_bits(got["out"], want) and R.same_bits(got["state"][:, :48], wst), (entry, name, r)
        assert np.all(got["state"][:, 48] == entry) and not got["flags"].any()
        assert R.same_bits(got["fe"][:, 4:8], np.broadcast_to(table[entry][4:8], (G.TICKS, 4)))
        assert R.same_bits(got["swing"], np.broadcast_to(table[entry][0:4] / table[entry][4:8] - table[entry][0:4], (G.TICKS, 4)))


@pytest.mark.parametrize("first,second,k", [(2, 4, 233), (1, 3, 100), (4, 1, 377), (3, 0, 550)])
def test_a_construct_reset_is_a_fresh_generator(pkg, first, second, k):
    table = pkg.workload.gait_table()
    T, n = G.TICKS, 6
    time = (np.arange(T) * G.DT).astype(_f)
    contact = G.contacts(n, T, table[second], time, 0x77)
    sel = np.full(T, first, _f); sel[k] = second                       # between resets the array names the OTHER gait: it is not read there
    sel[k + 1:] = first
    level = np.zeros(T, np.int32); level[0] = level[k] = R.CONSTRUCT
    local = np.concatenate([time[:k], time[:T - k]])
    for r in range(n):
        got = R.run(table, local, contact[:, r], sel, level)
        fresh = R.run(table, time[:T - k], contact[k:, r], np.full(T - k, second, _f), level[k:])
        for key in ("out", "state", "fe", "swing"):
            assert R.same_bits(got[key][k:], fresh[key]), (key, r)
        assert np.all(got["state"][:k, 48] == first) and np.all(got["state"][k:, 48] == second)


def test_a_live_switch_keeps_what_reset_does_not_write(pkg):
    """advanced_trot -> stand at tick 233 -> trot at tick 450, LIVE, the clock restarted at each: gaitCycle, cumDt and swingTimeRemaining cross the
    switch; legs 0 and 3 keep the 0.00066668 s of their last swing tick (tick 208) for the whole stand; the stand commands no swing; all finite."""
    table = pkg.workload.gait_table()
    T, n, a, b = G.TICKS, 8, 233, 450
    time = (np.arange(T) * G.DT).astype(_f)
    contact = G.contacts(n, T, table[2], time, 0x78)                      # robot 0 follows advanced_trot's nominal schedule
    sel = np.full(T, 2, _f); sel[a] = 4; sel[b] = 1
    level = np.zeros(T, np.int32); level[0] = R.CONSTRUCT; level[a] = level[b] = R.LIVE
    local = np.concatenate([time[:a], time[:b - a], time[:T - b]])
    for r in range(n):
        got = R.run(table, local, contact[:, r], sel, level)
        st, out = got["state"], got["out"]
        for key in got:
            assert np.isfinite(got[key]).all(), (key, r)
        assert np.all(st[:a, 48] == 2) and np.all(st[a:b, 48] == 4) and np.all(st[b:, 48] == 1)
        # cumDt (row 2) and swingTimeRemaining (rows 44-47) of tick a - 1 are those of the whole stand: nothing in it writes them; gaitCycle (row 3)
        # crosses both switches and counts on from there, once per full cycle of the gait in force
        for row in (2, 44, 45, 46, 47):
            assert R.same_bits(st[a:b, row], np.full(b - a, st[a - 1, row], _f)), (r, row)
        assert st[a, 3] == st[a - 1, 3] and st[b, 3] == st[b - 1, 3] and np.all(np.diff(st[:, 3]) >= 0) and st[b - 1, 3] > st[a, 3]
        assert np.all(out[a:b, 8:12] == G.STANCE) and np.all(out[a:b, 12:16] == G.STANCE)
        assert (out[:a, 8:12] == G.SWING).any() and (out[b:, 8:12] == G.SWING).any()
        # Reset's own: the leg states at the entry's initial state, phases from a clock at zero
        assert st[a, 0] == 0 and st[a, 1] == 0 and np.all(st[a, 4:12] == G.STANCE)
        assert R.same_bits(got["swing"][a:b], np.zeros((b - a, 4), _f)) and R.same_bits(got["fe"][a:b, 4:8], np.ones((b - a, 4), _f))
        if r == 0:
            assert np.all(np.abs(st[a:b, [44, 47]].astype(np.float64) - 0.00066668) < 5e-9), st[a, 44:48]
            assert np.all(st[a:b, [45, 46]] != st[a, 44])
    # a CONSTRUCT switch is told apart by exactly that: swingTimeRemaining starts at 0
    level[a] = R.CONSTRUCT
    got = R.run(table, local, contact[:, 0], sel, level)
    assert np.all(got["state"][a:b, 44:48] == 0)


def _rows_of(descs):
    return np.array([[*e.stance_duration, *e.duty_factor, *e.initial_leg_phase, *e.initial_leg_state, e.contact_detection_phase_threshold, e.wait_time,
                      e.advanced_trot] for e in descs], _f)


def test_default_table_is_the_yaml(pkg):
    lib = pkg.load_library()
    q = pkg.qrgpu
    d = (q.gait_desc_struct * 5)()
    C.memset(d, 0xA5, C.sizeof(d))
    lib.qrgpu_gait_table_default(d)
    one = q.gait_desc_struct()
    lib.qrgpu_gait_desc_default(C.byref(one))
    assert C.sizeof(one) == 76 and bytes(d[0]) == bytes(one) and bytes(d[2]) == bytes(one)
    for rows in (_rows_of(d), pkg.gait_table_default(), pkg.workload.gait_table()):
        assert rows.shape == (5, 19) and rows.dtype == _f
        for e, name in enumerate(ORDER):
            stance, duty, phase, threshold, hold = YAML[name]
            want = np.array([*[stance] * 4, *[duty] * 4, *phase, 1, 1, 1, 1, threshold, one.wait_time, hold], _f)
            assert R.same_bits(rows[e], want), (e, name, rows[e], want)
    assert (q.FSM_GAIT_TROT, q.FSM_GAIT_ADVANCED_TROT, q.FSM_GAIT_WALK, q.FSM_GAIT_STAND) == (1, 2, 3, 4) and q.MAX_GAITS == 8 and q.GAIT_BAD_SEL == 1
    lib.qrgpu_gait_table_default(None)                                  # a null table is ignored


def test_selection_words():
    for v, want in ((0.0, 0), (4.0, 4), (-0.0, 0), (5.0, -1), (-1.0, -1), (2.5, -1), (np.nan, -1), (np.inf, -1), (1e9, -1), (7.0, -1)):
        assert R.index_of(v, 5) == want, v
    assert R.index_of(7.0, 8) == 7


def test_clock_restarts_where_the_mask_says():
    ticks = np.array([5, 9, 0, 12], np.int32)
    origin, local = R.stage_clock(np.array([0, 0x40, 0x10000, 0x01000000]), 0x100ff, ticks, np.array([2, 3, 7, 4], np.int32))
    assert origin.tolist() == [2, 9, 0, 4] and local.tolist() == [3, 0, 0, 8]
    assert R.clock_time(np.array([3]), 0.002)[0] == _f(3) * _f(0.002)
