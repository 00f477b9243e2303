"""-m gpu: qrgpu_episode_step_batch -- per-robot termination, reset and spawn on the device -- against the float64 restatement of
tests/episode_ref.py on the host test's generator (130 robots over five consecutive calls), at the batch edges, across histories, with each optional
array left out, in closed loop with the plant (falls are recycled) and with the controller (the first tick after a reset), and its error returns.

Bars: integers exact; floats the plant's 1e-6 * max(1, |ref|) per component (tests/test_gpu_plant.py); whatever a call does not write, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import body_contact_ref as BR
import episode_ref as ER
import gpu_helpers as G
import plant_ref as PR

pytestmark = pytest.mark.gpu

BAR = 1e-6
N = 130                                   # two full wavefronts and two lanes of a third
CALLS = 4                                 # after the reset_all call
INT_KEYS, FLOAT_KEYS = ("done", "st"), ("fb", "stats", "prev", "cmd")


def _i32(a):
    return np.ascontiguousarray(np.asarray(a).T, np.int32)


def _tdesc(pkg, D):
    return pkg.terrain_desc(D["nx"], D["ny"], D["n_fields"], D["x0"], D["y0"], D["cell"])


def _cdesc(pkg, d):
    return pkg.episode_desc(**{k: (list(v) if k == "q_spawn" else v) for k, v in d.items()})


class Ep:
    """Device arrays of one batch for the episode call; outputs poisoned."""

    def __init__(self, ctx, pkg, n, ground=None, table=ER.TABLE):
        self.ctx, self.pkg, self.n, self.ground = ctx, pkg, n, ground
        A = ctx.alloc
        self.fb, self.prev, self.cmd = A((37, n)), A((3, n)), A((60, n))
        self.st, self.stats = A((ER.STATE_ROWS, n), np.int32), A((ER.STATS_ROWS, n))
        self.done, self.list, self.count = A((n,), np.int32), A((n,), np.int32), A((1,), np.int32)
        self.ps, self.ts, self.fr = A((n,), np.int32), A((n,), np.int32), A((n,), np.int32)
        self.table = A(table.shape).upload(table)
        self.n_spawn = table.shape[1]
        self.height = self.fid = self.tdesc = None
        if ground is not None:
            self.height = A(ground["height"].shape).upload(ground["height"])
            self.fid = A((n,), np.int32).upload(np.asarray(ground["fid"][:n], np.int32))
            self.tdesc = _tdesc(pkg, ground["D"])
        self.params = pkg.plant_params(ground_z=ER.GROUND_Z)
        for v in (self.st, self.ps, self.ts, self.fr):
            v.zero()
        self.stats.zero()

    def put(self, c=None, fb=None, st=None, stats=None, prev=None, cmd=None):
        """Upload robot-major inputs (the first n robots of a case c and / or single arrays)."""
        n, S = self.n, self.pkg.to_soa
        if c is not None:
            self.fb.upload(S(c["fb"][:n])); self.ps.upload(c["pstatus"][:n]); self.ts.upload(c["tstatus"][:n]); self.fr.upload(c["force"][:n])
        for dev, host, conv in ((self.fb, fb, S), (self.st, st, _i32), (self.stats, stats, S), (self.prev, prev, S), (self.cmd, cmd, S)):
            if host is not None:
                dev.upload(conv(host[:n]))

    def step(self, desc, reset_all=False, omit=()):
        n = self.n
        self.done.upload(np.full(n, -1, np.int32)); self.list.upload(np.full(n, -1, np.int32)); self.count.upload(np.full(1, -1, np.int32))
        g = lambda name, v: None if name in omit else v
        ter = "terrain" not in omit and self.ground is not None
        self.ctx.episode_step_batch(n, desc, self.fb, self.table, self.n_spawn, self.st, self.stats, self.done, reset_all=reset_all, params=self.params,
                                    terrain=self.tdesc if ter else None, height=self.height if ter else None, field_id=self.fid if ter else None,
                                    plant_status=self.ps, tick_status=g("tick_status", self.ts), force_reset=g("force_reset", self.fr),
                                    prev_ori=g("prev_ori", self.prev), motor_cmd=g("motor_cmd", self.cmd), done_list=g("done_list", self.list),
                                    done_count=g("done_count", self.count))
        self.ctx.sync()
        return dict(fb=self.fb.download().T.copy(), st=self.st.download().T.copy(), stats=self.stats.download().T.copy(), prev=self.prev.download().T.copy(),
                    cmd=self.cmd.download().T.copy(), done=self.done.download(), list=self.list.download(), count=int(self.count.download()[0]))

    def free(self):
        for v in (self.fb, self.prev, self.cmd, self.st, self.stats, self.done, self.list, self.count, self.ps, self.ts, self.fr, self.table, self.height, self.fid):
            if v is not None:
                v.free()


def _inputs(pkg):
    """The chain's inputs: the desc, the ground, CALLS cases of the host test's generator (robot i of the same kind in each), and what prev_ori and
    motor_cmd hold before each call."""
    d = ER.desc(**ER.CASE_DESC)
    ground = ER.case_ground(pkg)(N)
    calls = [ER.cases(d, ground, N, 30100 + k) for k in range(CALLS)]
    rng = np.random.default_rng(30200)
    side = [(rng.uniform(-1, 1, (N, 3)).astype(np.float32), rng.uniform(-5, 5, (N, 60)).astype(np.float32)) for _ in range(CALLS + 1)]
    return d, ground, calls, side


def _gpu_chain(ctx, pkg, n, inp):
    """reset_all, then the designed counters of calls[0] and CALLS consecutive calls.  -> (inputs, outputs) per call"""
    d, ground, calls, side = inp
    cd = _cdesc(pkg, d)
    g = dict(ground, fid=ground["fid"][:n])
    e = Ep(ctx, pkg, n, g)
    out = []
    e.put(c=calls[0], prev=side[0][0], cmd=side[0][1])
    out.append(e.step(cd, reset_all=True))
    for k, c in enumerate(calls):
        if k == 0:
            e.put(st=c["st"], stats=c["stats"])
        e.put(c=c, prev=side[k + 1][0], cmd=side[k + 1][1])
        out.append(e.step(cd))
    e.free()
    return out


def _ref_chain(inp, n=N, ground="given"):
    d, g0, calls, side = inp
    g = g0 if ground == "given" else ground
    r = ER.step(d, g, ER.GROUND_Z, ER.TABLE, calls[0]["fb"][:n], np.zeros((n, 6)), np.zeros((n, 9)), reset_all=True, prev_ori=side[0][0][:n], motor_cmd=side[0][1][:n])
    out = [r]
    for k, c in enumerate(calls):
        st, stats = (c["st"][:n], c["stats"][:n]) if k == 0 else (r["ep_state"], r["ep_stats"])
        r = ER.step(d, g, ER.GROUND_Z, ER.TABLE, c["fb"][:n], st, stats, c["pstatus"][:n], c["tstatus"][:n], c["force"][:n], prev_ori=side[k + 1][0][:n],
                    motor_cmd=side[k + 1][1][:n])
        out.append(r)
    return out


@pytest.fixture(scope="module")
def chain(gpu_ctx, pkg):
    inp = _inputs(pkg)
    return dict(inp=inp, gpu=_gpu_chain(gpu_ctx, pkg, N, inp), ref=_ref_chain(inp))


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_parity_over_consecutive_calls(chain):
    """130 robots, about a third of them ending their episode at every call, five calls: integers exact, the state of reset robots and the statistics
    within 1e-6 * max(1, |ref|), whatever belongs to a robot not reset bit for bit what went in, the list of reset robots as a set."""
    d, ground, calls, side = chain["inp"]
    worst = 0.0
    for k, (g, r) in enumerate(zip(chain["gpu"], chain["ref"])):
        reset = r["reset"]
        assert np.array_equal(g["done"], r["done"]), k
        assert np.array_equal(g["st"], r["ep_state"]), k
        if k:
            assert (0.3 if k == 1 else 0.15) < reset.mean() < 0.45, (k, reset.mean())      # (from the second call on the counters are the chain's, not designed)
        else:
            assert reset.all() and np.all(g["done"] == ER.EP_FORCED)
        for key, ref in (("fb", r["fb"]), ("stats", r["ep_stats"]), ("prev", r["prev_ori"]), ("cmd", r["motor_cmd"])):
            sel = slice(None) if key == "stats" else reset
            e = np.abs(g[key][sel] - ref[sel]) / np.maximum(1.0, np.abs(ref[sel]))
            worst = max(worst, float(e.max()))
            assert np.all(e <= BAR), (k, key, float(e.max()))
        # a robot not reset: state, prev_ori, motor command and the statistics rows of episodes past are the bits that went in
        c = calls[max(k - 1, 0)]
        keep = ~reset
        stats_in = c["stats"] if k == 1 else chain["gpu"][k - 1]["stats"]
        assert np.array_equal(_u32(g["fb"][keep]), _u32(c["fb"][keep])), k
        assert np.array_equal(_u32(g["prev"][keep]), _u32(side[k][0][keep])) and np.array_equal(_u32(g["cmd"][keep]), _u32(side[k][1][keep])), k
        assert np.array_equal(_u32(g["stats"][keep][:, 0:8]), _u32(stats_in[keep][:, 0:8])), k
        # the compacted list
        idx = np.nonzero(g["done"] & ER.EP_REASONS)[0]
        assert g["count"] == len(idx) and set(g["list"][:g["count"]]) == set(idx) and len(set(g["list"][:g["count"]])) == g["count"], k
        assert np.all(g["list"][g["count"]:] == -1), k
        q = g["fb"][reset, 0:4].astype(np.float64)
        assert np.abs((q * q).sum(1) - 1).max() < 1e-6 and np.all(q[:, 0] >= 0)
    print("worst |gpu - ref| / max(1, |ref|) over the five calls: %.3e" % worst)
    epi = chain["gpu"][-1]["st"][:, 1]
    assert epi.max() >= 4 and len(np.unique(epi)) >= 4                       # the episode indices advanced, differently per robot
    deb = np.stack([g["st"][:, 2] for g in chain["gpu"]])
    assert deb.max() >= 2                                                    # the debounce counters advanced across calls


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_edges(gpu_ctx, pkg, chain, n):
    """The first n robots alone: bit for bit the first n robots of the 130-robot calls (the random numbers are keyed by the robot index)."""
    got = _gpu_chain(gpu_ctx, pkg, n, chain["inp"])
    for k, (a, b) in enumerate(zip(got, chain["gpu"])):
        for key in INT_KEYS + FLOAT_KEYS:
            assert np.array_equal(_u32(a[key]), _u32(b[key][:n])), (k, key)
        idx = set(np.nonzero(a["done"] & ER.EP_REASONS)[0])
        assert a["count"] == len(idx) and set(a["list"][:a["count"]]) == idx, k
        if n <= 64:
            assert list(a["list"][:a["count"]]) == sorted(idx), k             # one wavefront: ascending


def test_history_independence(gpu_ctx, pkg):
    """A robot's spawn at episode index k: bit for bit the same after k resets in one context and with the state row set to k - 1 and one reset in
    a fresh context."""
    n = 70
    d = ER.desc(**dict(ER.CASE_DESC, max_ticks=0))
    cd = _cdesc(pkg, d)
    ground = ER.case_ground(pkg)(n)
    e = Ep(gpu_ctx, pkg, n, ground)
    e.put(fb=PR.stand_state(n))
    e.step(cd, reset_all=True)
    for rnd in range(5):
        e.fr.upload(((np.arange(n) + rnd) % 3 != 0).astype(np.int32))
        e.put(fb=PR.stand_state(n))                                          # (healthy: only the forced ones end)
        a = e.step(cd)
    e.free()
    epi = a["st"][:, 1]
    assert epi.min() >= 3 and epi.max() == 4
    fresh = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    try:
        f = Ep(fresh, pkg, n, ground)
        f.put(fb=PR.stand_state(n))
        f.step(cd, reset_all=True)
        last = ((np.arange(n) + 4) % 3 != 0)                                 # those reset in the last round; the others spawned a round earlier
        st = np.zeros((n, 6), np.int32); st[:, 1] = epi - 1
        f.put(st=st, fb=PR.stand_state(n))
        f.fr.upload(np.ones(n, np.int32))
        b = f.step(cd)
        f.free()
    finally:
        fresh.close()
    assert np.array_equal(b["st"][:, 1], epi)
    assert np.array_equal(_u32(b["fb"][last]), _u32(a["fb"][last]))
    assert np.array_equal(_u32(b["stats"][:, 0:4]), _u32(a["stats"][:, 0:4]))          # the spawn of the running episode, every robot
    ref = ER.spawn(d, ground, ER.GROUND_Z, ER.TABLE, np.arange(n), epi)
    assert np.all(np.abs(b["fb"] - ref["fb"]) <= BAR * np.maximum(1.0, np.abs(ref["fb"])))


def test_optional_arrays(gpu_ctx, pkg, chain):
    """Each optional array NULL in turn: the other outputs are the full call's bits wherever they do not depend on the array left out."""
    d, ground, calls, side = chain["inp"]
    cd = _cdesc(pkg, d)
    c = calls[0]

    def run(omit):
        e = Ep(gpu_ctx, pkg, N, ground)
        e.put(c=c, prev=side[0][0], cmd=side[0][1]); e.step(cd, reset_all=True)
        e.put(c=c, st=c["st"], stats=c["stats"], prev=side[1][0], cmd=side[1][1])
        out = e.step(cd, omit=omit)
        e.free()
        return out
    full = run(())
    assert np.array_equal(full["done"], chain["gpu"][1]["done"])
    same = lambda a, keys, sel=slice(None): all(np.array_equal(_u32(a[k][sel]), _u32(full[k][sel])) for k in keys)
    a = run(("prev_ori",))
    assert same(a, ("done", "st", "fb", "stats", "cmd")) and a["count"] == full["count"] and np.array_equal(_u32(a["prev"]), _u32(side[1][0]))
    a = run(("motor_cmd",))
    assert same(a, ("done", "st", "fb", "stats", "prev")) and a["count"] == full["count"] and np.array_equal(_u32(a["cmd"]), _u32(side[1][1]))
    a = run(("done_list",))
    assert same(a, INT_KEYS + FLOAT_KEYS) and a["count"] == full["count"] and np.all(a["list"] == -1)
    a = run(("done_list", "done_count"))
    assert same(a, INT_KEYS + FLOAT_KEYS) and a["count"] == -1 and np.all(a["list"] == -1)
    for omit, arr, bit in (("tick_status", c["tstatus"] & d["tick_mask"], ER.EP_TICK_STATUS), ("force_reset", c["force"], ER.EP_FORCED)):
        a = run((omit,))
        free = arr == 0                                                      # robots whose result does not depend on the array
        assert free.sum() >= 100 and same(a, INT_KEYS + FLOAT_KEYS, free), omit
        assert np.array_equal(a["done"][~free], full["done"][~free] & ~bit), omit
        assert a["count"] == int(((a["done"] & ER.EP_REASONS) != 0).sum())
    # no terrain: flat at ground_z -- another ground, so against the reference; what does not depend on the ground (the words drawn: row, joints,
    # velocities of the robots reset in both) are the full call's bits
    a = run(("terrain",))
    r = ER.step(d, None, ER.GROUND_Z, ER.TABLE, c["fb"], c["st"], c["stats"], c["pstatus"], c["tstatus"], c["force"])
    assert np.array_equal(a["done"], r["done"]) and np.array_equal(a["st"], r["ep_state"]) and not (a["done"] & ER.EP_OFF_FIELD).any()
    assert np.all(np.abs(a["fb"] - r["fb"]) <= BAR * np.maximum(1.0, np.abs(r["fb"])))
    both = r["reset"] & ((full["done"] & ER.EP_REASONS) != 0)
    assert both.sum() >= 30 and np.array_equal(_u32(a["fb"][both][:, 10:37]), _u32(full["fb"][both][:, 10:37]))
    assert np.all(a["fb"][r["reset"], 1:3] == 0)                             # level


def test_bad_field_id_is_flagged_and_field_0_used(gpu_ctx, pkg):
    n = 8
    d = ER.desc(**ER.CASE_DESC)
    ground = ER.case_ground(pkg)(n)
    fid = np.array([0, 1, 2, -1, 1, 0, 99, 1], np.int32)
    e = Ep(gpu_ctx, pkg, n, dict(ground, fid=fid))
    e.put(fb=PR.stand_state(n))
    a = e.step(_cdesc(pkg, d), reset_all=True)
    e.free()
    r = ER.step(d, dict(ground, fid=fid), ER.GROUND_Z, ER.TABLE, PR.stand_state(n), np.zeros((n, 6)), np.zeros((n, 9)), reset_all=True)
    bad = (fid < 0) | (fid > 1)
    assert np.array_equal(a["done"], np.where(bad, ER.EP_FORCED | ER.EP_BAD_FIELD, ER.EP_FORCED)) and np.array_equal(a["done"], r["done"])
    assert np.all(np.abs(a["fb"] - r["fb"]) <= BAR * np.maximum(1.0, np.abs(r["fb"]))) and a["count"] == n


def test_a_nonfinite_value_in_any_row_ends_the_episode(gpu_ctx, pkg):
    """The kernel's scan of the 37 state rows: 130 healthy robots, robot i < 111 with a NaN, +Inf or -Inf (i % 3) in row i // 3 -- every row with every
    value -- the other 19 untouched.  Exactly the 111 end with EP_NONFINITE alone, the geometric bits off (rows 0-6 would otherwise trip them), and
    all is the reference's; a robot with a bad quaternion or position is respawned finite."""
    n = 130
    d = ER.desc(**dict(ER.CASE_DESC, max_ticks=0))
    ground = ER.case_ground(pkg)(n)
    fb = PR.stand_state(n)
    rng = np.random.default_rng(30300)
    fb[:, 7:13] = rng.uniform(-1, 1, (n, 6)); fb[:, 25:37] = rng.uniform(-3, 3, (n, 12))
    bad = np.arange(n) < 111
    for i in range(111):
        fb[i, i // 3] = (np.nan, np.inf, -np.inf)[i % 3]
    assert np.all((~np.isfinite(fb)).sum(1) == bad) and np.all((~np.isfinite(fb)).sum(0) == 3)          # every row, every value, one per robot
    e = Ep(gpu_ctx, pkg, n, ground)
    e.put(fb=PR.stand_state(n))
    first = e.step(_cdesc(pkg, d), reset_all=True)
    e.put(fb=fb)
    a = e.step(_cdesc(pkg, d))
    e.free()
    r = ER.step(d, ground, ER.GROUND_Z, ER.TABLE, fb, first["st"], first["stats"])
    assert np.array_equal(a["done"], np.where(bad, ER.EP_NONFINITE, 0)) and np.array_equal(a["done"], r["done"])
    assert np.array_equal(a["st"], r["ep_state"]) and a["count"] == 111 and set(a["list"][:111]) == set(range(111))
    assert np.isfinite(a["fb"][bad]).all() and np.all(np.abs(a["fb"][bad] - r["fb"][bad]) <= BAR * np.maximum(1.0, np.abs(r["fb"][bad])))
    assert np.array_equal(_u32(a["fb"][~bad]), _u32(fb[~bad])) and np.all(a["stats"][bad, 5:7] == 0)


def _rzz(fb):
    q = fb[:, 0:4].astype(np.float64)
    return 1.0 - 2.0 * (q[:, 1] ** 2 + q[:, 2] ** 2) / (q * q).sum(1)


def test_falls_are_recycled(gpu_ctx, pkg):
    """32 A1 robots on the flat field through qrgpu_plant_step_body_batch, the episode step before every plant step for 1.5 s: the odd ones are
    dropped limp on their backs (test_falls_are_physical's set-up), the even ones stand on the PD hold.  Every dropped robot raises EP_STATUS
    exactly once, is at episode 1 at the end and upright (R_zz > 0.95, base z within 0.03 of episode_ref.STAND_SETTLE_Z, where the float64 chain
    of body_contact_ref settles the PD stand: test_episode_ref.py); no standing robot ever ends an episode, and its state is bit for bit that of a
    run without the episode call; every robot is finite on every tick."""
    G.setup_a1(gpu_ctx, pkg, 10)
    for t, robot in enumerate(PR.ROBOTS):
        gpu_ctx.plant_body_setup(t, pkg.plant_body_desc(robot))
    n, ticks = 32, 1500
    D, height, s, c, scen = BR.fall_case(pkg, n)
    s[0::2] = PR.stand_state(n // 2); c[0::2] = PR.stand_cmd(n // 2)
    down = scen == 1
    params = pkg.plant_params(**BR.FALL_PARAMS)
    tdesc = _tdesc(pkg, D)
    # the fall is to be named by the plant's status alone: a robot dropped upside down is beyond any tilt bound from the first call, and a trunk that
    # lies on the ground is under any clearance bound, so this desc judges neither (cos(pi) = -1 and 0 m are never undercut above the ground)
    cd = pkg.episode_desc(tilt_max=np.pi, min_clearance=0.0)
    table = np.zeros((4, 1), np.float32)
    end = {}
    for with_episodes in (True, False):
        e = Ep(gpu_ctx, pkg, n, dict(D=D, height=height, fid=np.zeros(n, np.int32)), table=table)
        e.params = pkg.plant_params(**BR.FALL_PARAMS)
        e.put(fb=s, cmd=c)
        # episode 0 is the state uploaded, not a spawn: the rows of a fresh start written by hand (spawn x, y = 0, running minimum = the drop height)
        stats = np.zeros((n, 9), np.float32); stats[:, 2] = 0.30; stats[:, 8] = 0.30
        e.put(stats=stats)
        log = gpu_ctx.alloc((ticks, n), np.int32).upload(np.full((ticks, n), -1, np.int32))
        plog = gpu_ctx.alloc((ticks, n), np.int32).upload(np.full((ticks, n), -1, np.int32))
        for k in range(ticks):
            if with_episodes:
                gpu_ctx.episode_step_batch(n, cd, e.fb, e.table, 1, e.st, e.stats, log.row(k), params=e.params, terrain=tdesc, height=e.height,
                                           plant_status=plog.row(k - 1) if k else e.ps, prev_ori=e.prev, motor_cmd=e.cmd, done_list=e.list, done_count=e.count)
            gpu_ctx.plant_step_body_batch(n, params, tdesc, e.height, e.fb, e.cmd, status=plog.row(k))
        gpu_ctx.sync()
        end[with_episodes] = dict(fb=e.fb.download().T.copy(), st=e.st.download().T.copy(), stats=e.stats.download().T.copy(), done=log.download(),
                                  pstatus=plog.download(), cmd=e.cmd.download().T.copy())
        e.free(); log.free(); plog.free()
    a, b = end[True], end[False]
    ends = (a["done"] & ER.EP_REASONS) != 0
    assert not (a["done"] & ER.EP_NONFINITE).any() and not (a["pstatus"] & pkg.qrgpu.PL_NONFINITE).any() and not (b["pstatus"] & pkg.qrgpu.PL_NONFINITE).any()
    assert np.isfinite(a["fb"]).all()
    assert np.all(ends[:, down].sum(0) == 1) and np.all(a["done"][:, down].max(0) == ER.EP_STATUS), a["done"][:, down].max(0)
    assert not ends[:, ~down].any()
    assert np.all(a["st"][down, 1] == 1) and np.all(a["st"][~down, 1] == 0) and np.all(a["st"][down, 4] == 1) and np.all(a["st"][:, 5] == 0)
    when = ends[:, down].argmax(0)
    print("the dropped robots end their episode at ticks %d .. %d; at the end z %.4f .. %.4f (PD stand settles at %.4f), R_zz >= %.4f"
          % (when.min(), when.max(), a["fb"][down, 6].min(), a["fb"][down, 6].max(), ER.STAND_SETTLE_Z, _rzz(a["fb"][down]).min()))
    assert np.all(_rzz(a["fb"][down]) > 0.95) and np.all(np.abs(a["fb"][down, 6] - ER.STAND_SETTLE_Z) <= 0.03)
    assert np.array_equal(_u32(a["fb"][~down]), _u32(b["fb"][~down]))
    assert np.array_equal(a["stats"][down, 4], (when + 1).astype(np.float32))  # the length of the episode that ended: the calls it saw (no spawn call began it)
    assert np.array_equal(_u32(a["cmd"][down]), _u32(PR.stand_cmd(int(down.sum()))))
    assert np.all(_rzz(b["fb"][down]) < 0.0)                                  # without the episode call they are still on their backs


def test_controller_after_a_reset(gpu_ctx, pkg):
    """16 A1 robots settled on PD with one tick run; half of them are force-reset, then plant step, then tick.  The reset robots' forces and torques
    are those of a FRESH context's tick on the same state (their stale warm-start set costs speed only); the other half's are bit for bit those of
    a run without the reset.  Three contexts, so that no history but the one under test is shared.  The bar is the warm start's own, 1e-9 relative
    (include/qrgpu.h, qrgpu_set_warm_start).  Measured on an MI355X: forces and torques bit for bit the fresh context's, the same iteration counts."""
    n, h = 16, PR.HORIZON
    S = pkg.to_soa
    traj, gait, wcmd, prev0 = PR.stand_tick_inputs(n)
    d = ER.desc(xy_jitter=0.02, yaw_jitter=0.2, q_jitter=0.03, v_jitter=0.1, seed=77)
    cd = _cdesc(pkg, d)
    forced = (np.arange(n) % 2 == 0)
    params = pkg.plant_params(dt=0.002, substeps=2)

    def make():
        ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
        G.setup_a1(ctx, pkg, h)
        ctx.set_planned_list(False)          # (which launch solves a robot changes the last bits: gpu_helpers.cold_start)
        A = ctx.alloc
        v = dict(fb=A((37, n)), cmd=A((60, n)), mpc=A((28, n)), traj=A((12 * h, n)).upload(S(traj)), gait=A((4 * h, n)).upload(S(gait)),
                 wcmd=A((67, n)).upload(S(wcmd)), prev=A((3, n)).upload(S(prev0)), force=A((12, n)), status=A((n,), np.int32), pstatus=A((n,), np.int32))
        return ctx, v

    def tick(ctx, v):
        ctx.tick_batch(n, v["mpc"], v["traj"], v["gait"], v["fb"], v["wcmd"], v["prev"], v["force"], v["cmd"].row(48), v["status"])

    def history(reset):
        ctx, v = make()
        try:
            v["fb"].upload(S(PR.stand_state(n))); v["cmd"].upload(S(PR.stand_cmd(n)))
            pd = pkg.plant_params(dt=0.001, substeps=1)
            for _ in range(400):
                ctx.plant_step_batch(n, pd, v["fb"], v["cmd"], mpc_state=v["mpc"])
            v["cmd"].zero()
            tick(ctx, v)
            if reset:
                e = Ep(ctx, pkg, n, None, table=np.zeros((4, 1), np.float32))
                e.params = pkg.plant_params()
                e.fr.upload(forced.astype(np.int32))
                stats = np.zeros((n, 9), np.float32); stats[:, 8] = 0.3
                e.put(stats=stats)
                ctx.episode_step_batch(n, cd, v["fb"], e.table, 1, e.st, e.stats, e.done, params=e.params, force_reset=e.fr, prev_ori=v["prev"], motor_cmd=v["cmd"])
                ctx.sync()
                done = e.done.download()
                e.free()
                assert np.array_equal(done, np.where(forced, ER.EP_FORCED, 0))
            ctx.plant_step_batch(n, params, v["fb"], v["cmd"], mpc_state=v["mpc"], status=v["pstatus"])
            ctx.sync()
            state = dict(fb=v["fb"].download(), mpc=v["mpc"].download(), prev=v["prev"].download())
            tick(ctx, v)
            ctx.sync()
            out = dict(force=v["force"].download().T.copy(), tau=v["cmd"].download()[48:60].T.copy(), status=v["status"].download(), pstatus=v["pstatus"].download())
            return state, out
        finally:
            ctx.close()

    state, with_reset = history(True)
    _, without = history(False)
    ctx, v = make()
    try:
        v["fb"].upload(state["fb"]); v["mpc"].upload(state["mpc"]); v["prev"].upload(state["prev"]); v["cmd"].zero()
        tick(ctx, v)
        ctx.sync()
        fresh = dict(force=v["force"].download().T.copy(), tau=v["cmd"].download()[48:60].T.copy(), status=v["status"].download())
    finally:
        ctx.close()
    assert np.all(G.flags(with_reset["status"]) == 0) and np.all(G.flags(fresh["status"]) == 0) and np.all(with_reset["pstatus"] == 0)
    k = forced
    scale = np.maximum(1.0, np.abs(fresh["force"][k]).max(1))
    ef = (np.abs(with_reset["force"][k] - fresh["force"][k]).max(1) / scale).max()
    et = (np.abs(with_reset["tau"][k] - fresh["tau"][k]) / np.maximum(1.0, np.abs(fresh["tau"][k]))).max()
    print("after a reset against a fresh context: forces %.3e of the force scale, torques %.3e * max(1, |tau|); iterations %s against %s"
          % (ef, et, G.iterations(with_reset["status"])[k], G.iterations(fresh["status"])[k]))
    assert ef <= 1e-9, ef
    assert et <= 1e-9, et
    assert np.array_equal(_u32(with_reset["force"][~k]), _u32(without["force"][~k])) and np.array_equal(_u32(with_reset["tau"][~k]), _u32(without["tau"][~k]))
    assert not np.array_equal(with_reset["force"][k], without["force"][k])   # (the reset did change what the controller saw)


def test_error_returns(gpu_ctx, pkg):
    """QRGPU_ERR_BAD_ARG for every case the header lists, nothing launched (the poisoned d_done is untouched) and qrgpu_last_error naming the argument."""
    n = 6
    d = ER.desc(**ER.CASE_DESC)
    ground = ER.case_ground(pkg)(n)
    e = Ep(gpu_ctx, pkg, n, ground)
    e.put(fb=PR.stand_state(n))
    e.done.upload(np.full(n, -1, np.int32))
    lib, h = gpu_ctx._lib, gpu_ctx._h
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    nan, inf = float("nan"), float("inf")

    def call(n_=n, desc="default", terrain="default", height="default", spawn="default", n_spawn=7, fb="default", st="default", stats="default", done="default",
             lst=None, count=None, **fields):
        pick = lambda v, dflt: dflt if isinstance(v, str) else v
        cd = pick(desc, _cdesc(pkg, dict(d, **fields)))
        t = pick(terrain, e.tdesc)
        return lib.qrgpu_episode_step_batch(h, n_, None if cd is None else C.byref(cd), 0, C.byref(e.params), None if t is None else C.byref(t),
                                            vp(pick(height, e.height)), vp(e.fid), vp(pick(spawn, e.table)), n_spawn, vp(e.ps), None, None, vp(pick(fb, e.fb)), None,
                                            None, vp(pick(st, e.st)), vp(pick(stats, e.stats)), vp(pick(done, e.done)), vp(lst), vp(count))

    T = lambda **kw: pkg.terrain_desc(**dict(dict(nx=24, ny=20, n_fields=2, x0=-1.2, y0=-0.9, cell=0.11), **kw))
    cases = [("n", dict(n_=0)), ("n", dict(n_=gpu_ctx.max_batch + 1)), ("desc", dict(desc=None)), ("d_fb_state", dict(fb=None)), ("d_ep_state", dict(st=None)),
             ("d_ep_stats", dict(stats=None)), ("d_done", dict(done=None)), ("d_spawn", dict(spawn=None)), ("n_spawn", dict(n_spawn=0)),
             ("terrain", dict(terrain=T(nx=1))), ("terrain", dict(terrain=T(n_fields=0))), ("terrain", dict(terrain=T(cell=0.0))), ("terrain", dict(terrain=T(x0=nan))),
             ("d_height", dict(height=None)), ("d_done_count", dict(lst=e.list)), ("status_ticks", dict(status_ticks=0)), ("max_ticks", dict(max_ticks=-1)),
             ("tilt_max", dict(tilt_max=nan)), ("tilt_max", dict(tilt_max=-0.1)), ("min_clearance", dict(min_clearance=inf)), ("field_margin", dict(field_margin=-1.0)),
             ("spawn_height", dict(spawn_height=nan)), ("xy_jitter", dict(xy_jitter=-0.1)), ("yaw_jitter", dict(yaw_jitter=inf)), ("q_jitter", dict(q_jitter=nan)),
             ("v_jitter", dict(v_jitter=-1.0)), ("kp", dict(kp=nan)), ("kd", dict(kd=-1.0)), ("q_spawn", dict(q_spawn=[nan] + [0.0] * 11))]
    for name, kw in cases:
        assert call(**kw) == 2, (name, kw)
        assert name in gpu_ctx.last_error() and "qrgpu_episode_step_batch" in gpu_ctx.last_error(), (name, gpu_ctx.last_error())
    gpu_ctx.sync()
    assert np.all(e.done.download() == -1)                                   # nothing was launched
    assert lib.qrgpu_episode_step_batch(None, n, None, 0, None, None, None, None, None, 1, None, None, None, None, None, None, None, None, None, None, None) == 2
    assert call() == 0                                                       # ... and the good call goes through
    gpu_ctx.sync()
    assert np.all(e.done.download() != -1)
    e.free()
