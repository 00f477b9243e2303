"""CPU: the numpy restatement of the mode route and the merge (tests/mode_route_ref.py) pinned by tables written by hand from include/qrgpu.h: every
mode against the default table, the selections that are no mode, each plan kind, a custom table, the counts, the masks of the cadenced tick, and the
merge with a NaN in the column that is not selected."""
import numpy as np

import mode_route_ref as R

NONE, MPC, FB = 0, 1, 2


def test_every_mode_against_the_default_table():
    chain, flags, count = R.route(np.array([-1, 0, 1, 2, 3], np.float32))
    assert chain.tolist() == [NONE, FB, MPC, MPC, MPC]
    assert flags.tolist() == [0, 0, R.ROUTE_NO_CHAIN, R.ROUTE_NO_CHAIN, 0]
    assert count.tolist() == [1, 3, 1] and chain.dtype == np.int32 and flags.dtype == np.int32 and count.dtype == np.int32


def test_selections_that_are_no_mode_fall_back_and_are_flagged():
    chain, flags, count = R.route(np.array([np.nan, 1.5, 4, -2], np.float32))
    assert chain.tolist() == [MPC] * 4 and flags.tolist() == [R.ROUTE_BAD_MODE] * 4 and count.tolist() == [0, 4, 0]
    chain, flags, _ = R.route(np.array([np.nan, 1.5, 4, -2, np.inf, -np.inf, -0.5, 3.0000002], np.float32), table=(MPC, MPC, MPC, MPC), fallback=FB)
    assert chain.tolist() == [FB] * 8 and flags.tolist() == [R.ROUTE_BAD_MODE] * 8
    # a fallback of "no chain" is allowed: the robot is idle and flagged
    chain, flags, _ = R.route(np.array([7, 1], np.float32), fallback=NONE)
    assert chain.tolist() == [NONE, NONE] and flags.tolist() == [R.ROUTE_BAD_MODE, R.ROUTE_NO_CHAIN]


def test_each_plan_kind():
    kinds = [R.PLAN_RUN, R.PLAN_PHASE1, R.PLAN_PHASE2, R.PLAN_ACTION, R.PLAN_HOLD, R.PLAN_PASSIVE, R.PLAN_REPEAT]
    plan = np.array(kinds, np.int32)
    for mode, on in ((3, MPC), (0, FB)):
        chain, flags, _ = R.route(np.full(7, mode, np.float32), plan)
        assert chain.tolist() == [on, on, NONE, NONE, NONE, NONE, NONE] and not flags.any()
    # the flag bits of a plan do not count, and a plan that runs nothing comes before a bad mode: no flag
    chain, flags, _ = R.route(np.array([3, 3, np.nan, 2], np.float32),
                              np.array([R.PLAN_RUN | R.PLAN_DONE, R.PLAN_HOLD | R.PLAN_ACTION_END, R.PLAN_ACTION | R.PLAN_ACTION_FIRST, R.PLAN_PASSIVE], np.int32))
    assert chain.tolist() == [MPC, NONE, NONE, NONE] and flags.tolist() == [0, 0, 0, 0]
    # without a plan every robot is routed by its mode alone
    chain, _, _ = R.route(np.array([3, 0, -1], np.float32), None)
    assert chain.tolist() == [MPC, FB, NONE]


def test_a_custom_table():
    chain, flags, count = R.route(np.array([0, 1, 2, 3, -1, 9], np.float32), table=(MPC, FB, FB, NONE), fallback=FB)
    assert chain.tolist() == [MPC, FB, FB, FB, NONE, FB]
    assert flags.tolist() == [0, 0, 0, R.ROUTE_NO_CHAIN, 0, R.ROUTE_BAD_MODE]
    assert count.tolist() == [1, 1, 4]


def test_counts_add_up_over_a_large_column():
    sel, plan = R.random_columns(4097, 5)
    chain, flags, count = R.route(sel, plan)
    assert int(count.sum()) == 4097 and all(int(count[c]) == int((chain == c).sum()) for c in range(3)) and count.min() > 0
    assert set(np.unique(flags)) == {0, R.ROUTE_BAD_MODE, R.ROUTE_NO_CHAIN}
    assert not flags[(plan & 3) == 0].any() and not chain[(plan & 3) == 0].any()


def test_masks_of_the_cadenced_tick():
    due, skip = R.masks(np.array([1, 0, 1, 0, 7, 0], np.int32), np.array([MPC, MPC, FB, FB, NONE, NONE], np.int32))
    assert due.tolist() == [1, 0, 0, 0, 0, 0] and skip.tolist() == [1, 0, 1, 1, 1, 1]


def test_patterns():
    assert R.pattern("mod3", 7).tolist() == [0, 1, 2, 0, 1, 2, 0]
    w = R.pattern("wave_idle", 130)
    assert not w[64:128].any() and w[:64].all() and w[128:].all() and set(w[:64]) == {MPC, FB}
    assert not (R.pattern("no_mpc", 130) == MPC).any() and (R.pattern("no_mpc", 130) == FB).any()
    assert not (R.pattern("no_fb", 130) == FB).any() and (R.pattern("no_fb", 130) == MPC).any()
    assert (R.pattern("all_mpc", 9) == MPC).all() and (R.pattern("all_fb", 9) == FB).all()


def test_merge_selects_and_never_blends():
    n = 5
    a = np.arange(60 * n, dtype=np.float32).reshape(60, n) + 1
    b = -a
    a[:, 2] = np.nan                                   # robot 2 is on the force-balance chain: the NaN of the other column must not reach it
    b[:, 1] = np.nan
    a[3, 0] = np.nan; b[3, 0] = np.nan                 # robot 0 is on no chain
    chain = np.array([NONE, MPC, FB, 3, -1], np.int32)
    out, st = R.command(chain, a, b, np.array([10, 11, 12, 13, 14], np.int32), np.array([20, 21, 22, 23, 24], np.int32))
    assert out.dtype == np.float32 and out.shape == (60, n)
    assert np.array_equal(out[:, 1], a[:, 1]) and np.array_equal(out[:, 2], b[:, 2])
    assert not out[:, [0, 3, 4]].any() and not np.signbit(out[:, [0, 3, 4]]).any()
    assert st.tolist() == [0, 11, 22, 0, 0]
    # a NaN that IS selected is passed through with its payload
    a[5, 1] = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
    out, st = R.command(chain, a, b)
    assert out.view(np.uint32)[5, 1] == 0x7fc01234 and st.tolist() == [0] * n
