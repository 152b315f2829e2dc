"""Plain references for cp2_fills_finish_many: the layer sizes of a session's compact (layer-major) buffer, the per-level tables
k_finish_layer_many reads and the lane -> (session, slot, node, rows) turn through them, the verdict offsets and their inverse, the
refusals with their index, and the order of saves, objects and hand-overs.

It restates csrc/fill_finish_plan.hpp and what csrc/kernels.hpp says of launch_finish_layers_many; none of it shares code with the
product.  tests/test_fill_finish_many_cpu.py holds it against brute force and compares the product's plan with it;
tests/test_gpu_fill_finish_many_unit.py feeds these tables to the launcher.  A session here is (n_blocks, n_local)."""
import collections
import random

import numpy as np

BLOCKS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 33, 64, 128, 257)
LOCALS = (1, 2, 3, 5, 64, 65)
TOTALS = (1, 63, 64, 65, 255, 256, 257, 4097)      # lanes of level 0
WAVE = 64


def layer_sizes(n):
    """rows of every layer of one slot's tree over n >= 1 block roots, bottom first: one round of compression even for a single block"""
    sizes, m = [n], n
    while True:
        m = (m + 1) // 2
        sizes.append(m)
        if m == 1:
            return sizes


def depth(n):
    return len(layer_sizes(n)) - 1


def rows(n, n_local):
    return n_local * sum(layer_sizes(n))


def layer_off(n, n_local, level):
    """first row of layer `level` in the layer-major buffer of n_local slots"""
    return n_local * sum(layer_sizes(n)[:level])


def row_of(n, n_local, level, slot, node):
    return layer_off(n, n_local, level) + slot * layer_sizes(n)[level] + node


Plan = collections.namedtuple("Plan", "sessions voff prefix sess_of level_off level_cnt level_work rows_built launches")
Lane = collections.namedtuple("Lane", "session slot node src dst pair last")


def plan(sessions):
    voff = [0]
    for n, nl in sessions:
        voff.append(voff[-1] + nl)
    prefix, sess_of, off, cnt, work = [], [], [], [], []
    for level in range(max([depth(n) for n, _ in sessions], default=0)):
        off.append(len(prefix))
        s = 0
        for k, (n, nl) in enumerate(sessions):
            if depth(n) > level:
                s += nl * layer_sizes(n)[level + 1]
                prefix.append(s)
                sess_of.append(k)
        cnt.append(len(prefix) - off[-1])
        work.append(s)
    return Plan(list(sessions), voff, prefix, sess_of, off, cnt, work, sum(work), sum(1 for w in work if w))


def trips(cnt):
    s = 0
    while (1 << s) < cnt:
        s += 1
    return s


def find(prefix, t):
    """the kernel's search: the entry of lane t, in trips(len(prefix)) steps whatever t is"""
    lo, cnt = 0, len(prefix)
    for s in reversed(range(trips(cnt))):
        mid = lo + (1 << s)
        if mid < cnt and prefix[mid - 1] <= t:
            lo = mid
    return lo


def lane(p, level, t):
    pre = p.prefix[p.level_off[level]:p.level_off[level] + p.level_cnt[level]]
    e = find(pre, t)
    k = p.sess_of[p.level_off[level] + e]
    n, nl = p.sessions[k]
    j = t - (pre[e - 1] if e else 0)
    m_in, m_out = layer_sizes(n)[level], layer_sizes(n)[level + 1]
    slot, node = divmod(j, m_out)
    return Lane(k, slot, node, row_of(n, nl, level, slot, 2 * node), row_of(n, nl, level + 1, slot, node), 2 * node + 1 < m_in,
                level + 1 == depth(n))


def where(p, v):
    """verdict index -> (index into fills, local slot)"""
    k = max(i for i in range(len(p.sessions)) if p.voff[i] <= v)
    return k, v - p.voff[k]


def tables(p, addrs, roots):
    """the plan as the arrays the launcher takes: the descriptor table (7 uint64 per session: tree, n_rows, slot_roots, n_local, layer_tab
    = 0, n_blocks, depth in the low word of the last), voff, prefix, sess_of and the three host tables"""
    tab = np.zeros((len(p.sessions), 7), dtype=np.uint64)
    for k, (n, nl) in enumerate(p.sessions):
        tab[k] = (addrs[k], rows(n, nl), roots[k], nl, 0, n, depth(n))
    return (tab.reshape(-1), np.asarray(p.voff[:-1], dtype=np.uint64), np.asarray(p.prefix, dtype=np.uint64), np.asarray(p.sess_of, dtype=np.uint32),
            np.asarray(p.level_off, dtype=np.uint64), np.asarray(p.level_cnt, dtype=np.uint64), np.asarray(p.level_work, dtype=np.uint64))


# ---- the shapes of the launcher test -----------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "no sessions")


def lanes0(s):
    return s[1] * layer_sizes(s[0])[1]


def compose(total, rnd):
    """sessions whose level 0 has `total` lanes: a one-block, one-slot session first and last, drawn shapes between"""
    if total == 1:
        return [(1, 1)]
    out, left = [(1, 1)], total - 2
    shapes = [(n, nl) for n in BLOCKS for nl in LOCALS]
    while left:
        s = rnd.choice([s for s in shapes if lanes0(s) <= left])
        out.append(s)
        left -= lanes0(s)
    return out + [(1, 1)]


def cases():
    out = [Case(i, compose(t, random.Random(0xF1 + t))) for i, t in enumerate(TOTALS)]
    # one wave at level 0 with eight kinds of session in it: paired and odd-tail nodes, inner lanes and comparing lanes side by side
    out.append(Case(len(out), [(1, 1), (3, 2), (5, 1), (2, 3), (7, 1), (9, 1), (4, 2), (16, 1), (1, 1)]))
    out.append(Case(len(out), [(1, 1), (2, 5), (3, 3), (1, 2), (5, 2), (33, 1), (2, 1), (9, 2), (1, 1)]))
    out.append(Case(len(out), [(1, 1), (1, 3), (7, 2), (2, 2), (3, 1), (8, 3), (1, 5), (5, 3), (64, 1), (1, 1)]))
    # every block count, the slot counts cycling, 64 and 65 slots beside one
    out.append(Case(len(out), [(1, 1)] + [(n, LOCALS[i % len(LOCALS)]) for i, n in enumerate(BLOCKS)] + [(2, 64), (3, 65), (1, 1)]))
    return out


def mixed_wave(p, level, w):
    """does wave w of level `level` hold lanes of four or more sessions, paired nodes and odd tails, inner lanes and comparing lanes?"""
    ls = [lane(p, level, t) for t in range(w * WAVE, min((w + 1) * WAVE, p.level_work[level]))]
    return len({x.session for x in ls}) >= 4 and len({x.pair for x in ls}) == 2 and len({x.last for x in ls}) == 2


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
# a session's state for the checks: "ok", "finished", "other" (another context) or ("missing", [absent local * n_blocks + block, ...])
def missing_text(n, first_slot, absent):
    g = min(absent)
    return "fill: %d block(s) are missing, the first is (slot %d, block %d)" % (len(absent), first_slot + g // n, g % n)


FINISHED = "fill: the session is finished: it accepts only cp2_fill_free"


def refusal(fills, world):
    """fills: indices into world (None: a NULL entry); world[i] = (n_blocks, n_local, first_slot, state).  (index, text) or None"""
    for k, i in enumerate(fills):
        if i is None:
            return k, "fills: fills[%d] is NULL" % k
        if world[i][3] == "other":
            return k, "fills: fills[%d] belongs to another context" % k
        if world[i][3] == "finished":
            return k, "fills: fills[%d]: %s" % (k, FINISHED)
    seen = set()
    for k, i in enumerate(fills):
        if i in seen:
            return k, "fills: fills[%d] is listed twice: one session is finished once" % k
        seen.add(i)
    for k, i in enumerate(fills):
        if isinstance(world[i][3], tuple):
            return k, "fills: fills[%d]: %s" % (k, missing_text(world[i][0], world[i][2], world[i][3][1]))
    return None


def mismatch_text(fills, world, p, bad):
    """what a set of non-zero verdict indices is reported as: the first in order"""
    k, local = where(p, min(bad))
    return k, "fills: fills[%d]: fill: the tree over the kept block roots of slot %d does not end in the stated slot root" % (k, world[fills[k]][2] + local)


def commit_events(n, has_path, fail_at, alloc_fail_at=None):
    """(status, events, saved): saves serially in order where there is a path, the first failing one ends the call with -5 and nothing
    else; then n objects (a failing one ends it with -3); only then n hand-overs"""
    ev, saved = [], 0
    for k in range(n):
        if has_path[k]:
            ev.append("save %d" % k)
            if k == fail_at:
                return -5, ev, saved
            saved += 1
    for k in range(n):
        ev.append("make %d" % k)
        if k == alloc_fail_at:
            return -3, ev, saved
    return 0, ev + ["hand %d" % k for k in range(n)], saved


# ---- scenarios for tests/host_check/fill_finish_many_check.cpp ----------------------------------------------------------------------------
def scenario(seed):
    """(world, calls): calls = [(fills, has_path, bad verdicts)]"""
    rnd = random.Random(0xF1F1 + seed)
    world = []
    for _ in range(rnd.randint(3, 24)):
        n, nl = rnd.choice(BLOCKS), rnd.choice(LOCALS[:4] if rnd.random() < 0.8 else LOCALS)
        world.append([n, nl, rnd.randrange(0, 9), "ok"])
    good = list(range(len(world)))
    for state in ("finished", "other", "missing", "missing"):
        n, nl = rnd.choice(BLOCKS), rnd.choice(LOCALS[:4])
        if state == "missing":
            state = ("missing", sorted(rnd.sample(range(n * nl), rnd.randint(1, min(3, n * nl)))))
        world.append([n, nl, rnd.randrange(0, 9), state])
    bad_ones = list(range(len(good), len(world)))
    calls = []
    for kind in ("all", "sub", "null", "twice", "bad", "bad", "bad", "bad", "twice and missing", "one"):
        fills = list(good)
        rnd.shuffle(fills)
        if kind == "sub":
            fills = fills[:max(1, len(fills) // 2)]
        if kind == "one":
            fills = fills[:1]
        if kind == "null":
            fills.insert(rnd.randrange(len(fills) + 1), None)
        if kind.startswith("twice"):
            fills.insert(rnd.randrange(len(fills) + 1), rnd.choice(fills))
        if kind == "bad":
            fills.insert(rnd.randrange(len(fills) + 1), bad_ones[len([c for c in calls if c[3] == "bad"])])
        if kind == "twice and missing":
            fills.insert(0, bad_ones[2])
        has_path = [rnd.random() < 0.5 for _ in fills]
        nv = sum(world[i][1] for i in fills if i is not None)
        bad = sorted(rnd.sample(range(nv), min(nv, rnd.randint(1, 3))))
        calls.append((fills, has_path, bad, kind))
    return world, [c[:3] for c in calls]


def scenario_text(world, calls):
    out = ["world %d" % len(world)]
    for n, nl, first, state in world:
        out.append("session %d %d %d %s" % (n, nl, first, state if isinstance(state, str) else "missing " + " ".join(str(g) for g in state[1])))
    for fills, has_path, bad in calls:
        out.append("call %d %s" % (len(fills), " ".join("-1" if i is None else str(i) for i in fills)))
        out.append("paths %s" % " ".join("1" if h else "0" for h in has_path))
        out.append("bad %d %s" % (len(bad), " ".join(str(v) for v in bad)))
    return "\n".join(out) + "\n"


def cases_text(cs):
    """the launcher test's shapes as a scenario: every case one call over complete sessions"""
    world, calls = [], []
    for c in cs:
        first = len(world)
        world += [[n, nl, 0, "ok"] for n, nl in c.sessions]
        calls.append((list(range(first, len(world))), [False] * len(c.sessions), [0]))
    return world, calls


def lane_sum(p):
    """what the check prints of a level's lanes instead of listing them: count and a position-weighted sum of every field"""
    out = []
    for level in range(len(p.level_off)):
        acc = 0
        for t in range(p.level_work[level]):
            x = lane(p, level, t)
            acc = (acc * 1000003 + x.session * 7 + x.slot * 11 + x.node * 13 + x.src * 17 + x.dst * 19 + int(x.pair) * 23 + int(x.last) * 29) % (1 << 61)
        out.append("lanes %d count %d sum %d" % (level, p.level_work[level], acc))
    return out


def expected_lines(world, calls):
    out = []
    for fills, has_path, bad in calls:
        why = refusal(fills, world)
        if why is not None:
            out.append("refused %d %s" % why)
            continue
        p = plan([(world[i][0], world[i][1]) for i in fills])
        out.append("voff " + " ".join(str(v) for v in p.voff))
        for level in range(len(p.level_off)):
            a, b = p.level_off[level], p.level_off[level] + p.level_cnt[level]
            out.append("level %d off %d cnt %d work %d trips %d entries %s" % (
                level, a, p.level_cnt[level], p.level_work[level], trips(p.level_cnt[level]), " ".join("%d:%d" % e for e in zip(p.sess_of[a:b], p.prefix[a:b]))))
        out.append("rows_built %d launches %d" % (p.rows_built, p.launches))
        out += lane_sum(p)
        out.append("where " + " ".join("%d:%d" % where(p, v) for v in range(p.voff[-1])))
        out.append("mismatch %d %s" % mismatch_text(fills, world, p, bad))
        out.append("clean none")
        for fail_at in list(range(len(fills))) + [None]:
            st, ev, saved = commit_events(len(fills), has_path, fail_at)
            out.append("commit fail %s status %d saved %d: %s" % ("none" if fail_at is None else fail_at, st, saved, ", ".join(ev)))
        st, ev, saved = commit_events(len(fills), has_path, None, alloc_fail_at=len(fills) // 2)
        out.append("commit alloc %d status %d saved %d: %s" % (len(fills) // 2, st, saved, ", ".join(ev)))
    return out
