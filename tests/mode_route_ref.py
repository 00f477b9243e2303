"""A numpy restatement of the mode route and the merge (include/qrgpu.h, "the mode per robot"), written from the header's rules alone: the chain each
robot's mode selects with its flag word and the counts per chain, the two masks of the cadenced tick under the binding, and the motor command of the
robot's own chain.  Integers and copies: every comparison against it is bit for bit."""
import numpy as np

CHAIN_NONE, CHAIN_MPC, CHAIN_FORCE_BALANCE = 0, 1, 2
ROUTE_BAD_MODE, ROUTE_NO_CHAIN = 0x1, 0x2
PLAN_RUN, PLAN_PHASE1, PLAN_PHASE2, PLAN_ACTION, PLAN_HOLD, PLAN_PASSIVE, PLAN_REPEAT = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
PLAN_DONE, PLAN_ACTION_FIRST, PLAN_ACTION_END = 0x100, 0x200, 0x400
DEFAULT_TABLE, DEFAULT_FALLBACK = (CHAIN_FORCE_BALANCE, CHAIN_NONE, CHAIN_NONE, CHAIN_MPC), CHAIN_MPC
CMD_ROWS = 60


def route(mode_sel, plan=None, table=DEFAULT_TABLE, fallback=DEFAULT_FALLBACK):
    """mode_sel [n] float32, plan [n] int32 or None -> chain [n] int32, flags [n] int32, count [3] int32."""
    sel = np.asarray(mode_sel, np.float32)
    n = sel.shape[0]
    chain, flags = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for r in range(n):
        v = float(sel[r])
        if plan is not None and (int(plan[r]) & (PLAN_RUN | PLAN_PHASE1)) == 0:
            continue                                   # no locomotion controller runs on such a tick
        if v == -1.0:
            continue                                   # none yet
        if v != v or v != np.floor(v) or v < -1.0 or v > 3.0:
            chain[r], flags[r] = fallback, ROUTE_BAD_MODE
        elif table[int(v)] == CHAIN_NONE:
            chain[r], flags[r] = fallback, ROUTE_NO_CHAIN
        else:
            chain[r] = table[int(v)]
    count = np.array([(chain == c).sum() for c in range(3)], np.int32)
    return chain, flags, count


def masks(updated, chain):
    """The cadenced tick under the binding: due' = updated && on the MPC chain, skip' = updated || not on it."""
    up, on = np.asarray(updated) != 0, np.asarray(chain) == CHAIN_MPC
    return (up & on).astype(np.int32), (up | ~on).astype(np.int32)


def command(chain, cmd_mpc, cmd_fb, status_mpc=None, status_fb=None):
    """cmd_* [60][n] float32, status_* [n] int32 or None -> motor_cmd [60][n], status [n]; the words are copied, never computed with."""
    chain = np.asarray(chain)
    a, b = np.ascontiguousarray(cmd_mpc, np.float32).view(np.uint32), np.ascontiguousarray(cmd_fb, np.float32).view(np.uint32)
    n = chain.shape[0]
    out = np.where(chain[None, :] == CHAIN_MPC, a, np.where(chain[None, :] == CHAIN_FORCE_BALANCE, b, np.uint32(0)))
    sa = np.zeros(n, np.int32) if status_mpc is None else np.asarray(status_mpc, np.int32)
    sb = np.zeros(n, np.int32) if status_fb is None else np.asarray(status_fb, np.int32)
    st = np.where(chain == CHAIN_MPC, sa, np.where(chain == CHAIN_FORCE_BALANCE, sb, 0)).astype(np.int32)
    return np.ascontiguousarray(out, np.uint32).view(np.float32), st


# ------------------------------------------------------------------------------------------------------------------ the patterns the GPU tests share
PATTERNS = ("mod3", "wave_idle", "no_mpc", "no_fb", "all_mpc", "all_fb")


def pattern(name, n):
    """chain [n] int32: r % 3; one whole wavefront (robots 64-127, as far as there are any) idle in an alternating batch; nobody on the MPC chain;
    nobody on the force-balance chain; everybody on one chain."""
    r = np.arange(n)
    if name == "mod3":
        c = r % 3
    elif name == "wave_idle":
        c = 1 + (r & 1)
        c[64:128] = CHAIN_NONE
        if n <= 64:
            c[:] = CHAIN_NONE
    elif name == "no_mpc":
        c = np.where(r % 2 == 0, CHAIN_FORCE_BALANCE, CHAIN_NONE)
    elif name == "no_fb":
        c = np.where(r % 2 == 0, CHAIN_MPC, CHAIN_NONE)
    elif name == "all_mpc":
        c = np.full(n, CHAIN_MPC)
    elif name == "all_fb":
        c = np.full(n, CHAIN_FORCE_BALANCE)
    else:
        raise KeyError(name)
    return c.astype(np.int32)


def random_columns(n, seed):
    """mode_sel [n] float32 and plan [n] int32 for the host and GPU comparisons: every mode, the bad ones of the hand tables and a few more, every
    plan kind with and without its flag bits."""
    rng = np.random.default_rng(seed)
    pool = np.array([-1, 0, 1, 2, 3, 0, 3, 3, np.nan, 1.5, 4, -2, -0.5, 2.9999998, 1e9, -1e9, np.inf, -np.inf, 3.0000002, -1.0000001], np.float32)
    sel = pool[rng.integers(0, len(pool), n)]
    kinds = np.array([PLAN_RUN, PLAN_PHASE1, PLAN_PHASE2, PLAN_ACTION, PLAN_HOLD, PLAN_PASSIVE, PLAN_REPEAT], np.int32)
    plan = kinds[rng.integers(0, len(kinds), n)] | np.where(rng.random(n) < 0.25, PLAN_DONE, 0) | np.where(rng.random(n) < 0.1, PLAN_ACTION_FIRST, 0)
    plan[rng.random(n) < 0.4] = PLAN_RUN
    return sel.astype(np.float32), plan.astype(np.int32)
