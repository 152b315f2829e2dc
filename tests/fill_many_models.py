"""A plain model of cp2_fills_add_many (include/codex_p2.h): one SessionModel (tests/fill_session_model.py) per session, and a many-add that
is the model's add or anchored add on each session's subsequence of the requests -- the call is defined by the calls that exist.  Also the
seeded generator of the scenarios tests/host_check/fill_many_check.cpp runs csrc/fill_many_plan.hpp over, and the lines that program must
print for them.  It imports nothing from the product.

A scenario is a list of sessions [nb, first, n_local, keep, files] and a list of steps:

  ["call", fills, reqs, levels, have_paths, fail]   fills: indices into the scenario's sessions, in the order of the call's `fills`;
                                                    reqs: [[index into fills, slot, block, kind], ...], kind "ok" / "data" / "sib";
                                                    levels: None (whole paths) or one per request; have_paths: is `paths` not NULL;
                                                    fail: {index into fills: the slot whose file cannot be written}
  ["keep", session]   ["finish", session]           between calls, per session, as they exist today"""
import random

import fill_anchor_models as A
import fill_nodes_models as M
import fill_session_model as F

OK, ERR_INVALID, ERR_IO = F.OK, F.ERR_INVALID, F.ERR_IO
BLOCKS = (1, 2, 8, 16, 64)
SEEDS = tuple(range(1, 13))
WAVE = 64


class ManyModel:
    def __init__(self, sessions):
        self.shapes = [tuple(s) for s in sessions]
        self.sessions = [F.SessionModel((nb, first, n_local), files=bool(files)) for nb, first, n_local, _, files in sessions]
        for m, s in zip(self.sessions, sessions):
            if s[3]:
                m.apply(["keep"])

    def refusal(self, fills, reqs, levels, have_paths):
        """None, or ("fills" / "request", index): the first rule broken, in the order the call checks them"""
        seen = set()
        for k, j in enumerate(fills):                             # the same session twice
            if j in seen:
                return ("fills", k)
            seen.add(j)
        for i, r in enumerate(reqs):                              # a session index >= n_fills
            if r[0] >= len(fills):
                return ("request", i)
        for k, j in enumerate(fills):                             # each session's own rules over its subsequence, in `fills` order
            m = self.sessions[j]
            if m.finished:
                return ("fills", k)
            for i, (kk, s, b, _) in enumerate(reqs):
                if kk != k:
                    continue
                if not m.first <= s < m.first + m.n_local or b >= m.nb:
                    return ("request", i)
                if levels is None:
                    continue
                if levels[i] > m.depth:
                    return ("request", i)
                if m.keeping and not m.node.accepts(m.local(s), b, levels[i]):
                    return ("request", i)                         # an anchor that is not known when the call starts
                if not m.keeping and levels[i] < m.depth:
                    return ("request", i)                         # a short path into a session that keeps no nodes
        if not have_paths:
            for i, (k, _, _, _) in enumerate(reqs):
                if (self.sessions[fills[k]].depth if levels is None else levels[i]) > 0:
                    return ("request", i)
        return None

    def add_many(self, fills, reqs, levels=None, have_paths=True, fail=None):
        """{"err", "refused"} or {"err", "status": one per request, "n_new": one per entry of fills}"""
        fail = fail or {}
        why = self.refusal(fills, reqs, levels, have_paths)
        if why:
            return {"err": ERR_INVALID, "refused": why}
        status, n_new, err = [None] * len(reqs), [], OK
        for k, j in enumerate(fills):
            m = self.sessions[j]
            idx = [i for i, r in enumerate(reqs) if r[0] == k]
            if not idx:
                n_new.append(0)
                continue
            if levels is None or not m.keeping:
                res = m.apply(["add", [[reqs[i][1], reqs[i][2], reqs[i][3]] for i in idx], fail.get(k)])
            else:
                res = m.apply(["anchored", [[reqs[i][1], reqs[i][2], levels[i], reqs[i][3]] for i in idx], fail.get(k)])
            assert res["err"] in (OK, ERR_IO), (res, k)
            if res["err"] == ERR_IO and err == OK:
                err = ERR_IO
            for i, st in zip(idx, res["status"]):
                status[i] = st
            n_new.append(res["n_new"])
        return {"err": err, "status": status, "n_new": n_new}

    # ---- what fill_many_check.cpp prints ---------------------------------------------------------------------------------------------------
    def state_lines(self):
        out = []
        for j, m in enumerate(self.sessions):
            bits = "".join("1" if (s, b) in m.present else "0" for s in range(m.n_local) for b in range(m.nb))
            out.append("state %d: keeps %d finished %d present %s known %s" % (j, m.keeping, m.finished, bits, " ".join(map(str, sorted(m.known))) or "-"))
        return out

    def table_lines(self, fills, reqs, levels):
        """the grouping, the session table, the request arrays and the per-chunk maxima of an accepted call, before anything changes"""
        out = []
        for k, j in enumerate(fills):
            out.append("group %d: %s" % (k, " ".join(str(i) for i, r in enumerate(reqs) if r[0] == k) or "-"))
        for k, j in enumerate(fills):
            m = self.sessions[j]
            out.append("session %d: rows %d local %d keeps %d blocks %d depth %d" % (k, m.rows, m.n_local, m.keeping, m.nb, m.depth))
        at, lv = 0, []
        for i, (k, s, b, _) in enumerate(reqs):
            m = self.sessions[fills[k]]
            a = m.depth if levels is None else levels[i]
            row = A.anchor_row(m.nb, m.n_local, m.local(s), b, a)
            out.append("req %d: session %d local %d block %d level %d off %d dest %d anchor %s" % (
                i, k, m.local(s), b, a, at, M.node_row(m.nb, m.n_local, 0, m.local(s), b), "root" if row is None else row))
            at += a
            lv.append(a)
        out.append("paths %d" % at)
        for chunk in sorted({1, 3, WAVE, max(1, len(reqs))}):
            most = max([1] + [sum(lv[c0:c0 + chunk]) for c0 in range(0, len(reqs), chunk)])
            out.append("chunk %d: most %d" % (chunk, most))
        return out

    def step_lines(self, step):
        """apply one step of a scenario; returns the lines the check program prints for it"""
        if step[0] == "keep":
            self.sessions[step[1]].apply(["keep"])
            return ["keep %d" % step[1]] + self.state_lines()
        if step[0] == "finish":
            self.sessions[step[1]].finished = True
            return ["finish %d" % step[1]] + self.state_lines()
        _, fills, reqs, levels, have_paths, fail = step
        out = ["call: %d session(s), %d request(s), %s" % (len(fills), len(reqs), "whole paths" if levels is None else "levels")]
        why = self.refusal(fills, reqs, levels, have_paths)
        if why:
            return out + ["refused %s %d" % why] + self.state_lines()
        out += self.table_lines(fills, reqs, levels)
        res = self.add_many(fills, reqs, levels, have_paths, fail)
        for k in range(len(fills)):
            out.append("status %d: %s" % (k, " ".join(str(res["status"][i]) for i, r in enumerate(reqs) if r[0] == k) or "-"))
        out.append("result %d: status %s n_new %s" % (res["err"], " ".join(map(str, res["status"])) or "-", " ".join(map(str, res["n_new"])) or "-"))
        return out + self.state_lines()


# ---- the generator --------------------------------------------------------------------------------------------------------------------------
def _one_call(rng, model, fills, n, levels_given):
    """n requests interleaved at random over the sessions of `fills`, with repeats, some that will not prove, valid levels"""
    reqs, levels = [], []
    for _ in range(n):
        k = rng.randrange(len(fills))
        m = model.sessions[fills[k]]
        if reqs and rng.random() < 0.15:
            k, s, b = rng.choice(reqs)[:3]
            m = model.sessions[fills[k]]
        else:
            s, b = rng.choice(m.pairs)
        a = m.node.anchor(m.local(s), b)
        lvl = m.depth if not m.keeping else a if rng.random() < 0.6 else rng.randint(a, m.depth)
        y = rng.random()
        kind = "ok" if y < 0.8 else "data" if y < 0.92 or lvl == 0 else "sib"
        reqs.append([k, s, b, kind])
        levels.append(lvl)
    return reqs, (levels if levels_given else None)


def _refusals(rng, model, fills, reqs, levels):
    """the accepted call (fills, reqs, levels) broken one rule at a time; every one of them must change nothing"""
    out = []
    put = lambda f=fills, r=reqs, lv=levels, p=True: out.append(["call", list(f), [list(x) for x in r], None if lv is None else list(lv), p, {}])   # noqa: E731
    i = rng.randrange(len(reqs))
    k = reqs[i][0]
    m = model.sessions[fills[k]]

    def changed(col, v, seq=reqs):
        x = [list(r) for r in seq]
        x[i][col] = v
        return x

    def level(v):
        x = list(levels)
        x[i] = v
        return x
    if len(fills) > 1:
        put(f=list(fills[:-1]) + [fills[0]])                                          # the same session twice
    put(r=changed(0, len(fills)))                                                    # a session index >= n_fills
    put(r=changed(1, m.first + m.n_local))                                           # a slot outside ITS session's range
    put(r=changed(1, m.first - 1) if m.first else changed(2, m.nb + 3))
    put(r=changed(2, m.nb))                                                          # a block >= ITS session's nBlocks
    if levels is not None:
        put(lv=level(m.depth + 1))                                                   # a level above ITS session's depth
        if m.keeping:
            low = [j for j, r in enumerate(reqs) if model.sessions[fills[r[0]]].keeping and
                   model.sessions[fills[r[0]]].node.anchor(model.sessions[fills[r[0]]].local(r[1]), r[2]) > 0]
            if low:
                j = rng.choice(low)
                mm = model.sessions[fills[reqs[j][0]]]
                x = list(levels)
                x[j] = rng.randrange(mm.node.anchor(mm.local(reqs[j][1]), reqs[j][2]))
                put(lv=x)                                                            # an anchor not known when the call starts
        plain = [j for j, r in enumerate(reqs) if not model.sessions[fills[r[0]]].keeping]
        if plain:
            j = rng.choice(plain)
            x = list(levels)
            x[j] = rng.randrange(model.sessions[fills[reqs[j][0]]].depth)
            put(lv=x)                                                                # a short level into a session that keeps no nodes
    put(p=False)                                                                     # NULL paths while a level is not 0
    return out


def scenario(seed):
    """(sessions, steps) of one committed seed: 1 to 9 sessions of 1, 2, 8, 16 and 64 blocks a slot and 1 to 3 local slots, keeping nodes or
    not; calls of whole paths and of levels, small and wave-sized; refusals after the second call; a keep and a finish on the way"""
    rng = random.Random("fill many %d" % seed)
    n_sessions = 1 + (seed * 5) % 9
    sessions = []
    for j in range(n_sessions):
        nb = BLOCKS[(seed + j) % len(BLOCKS)] if j < 5 else rng.choice(BLOCKS)
        n_local = rng.randint(1, 3)
        sessions.append([nb, rng.randint(0, 4 - n_local), n_local, int(rng.random() < 0.6), int(rng.random() < 0.5)])
    model = ManyModel(sessions)
    steps = []

    def run(step):
        steps.append(step)
        model.step_lines(step)

    everyone = list(range(n_sessions))
    for c in range(8):
        fills = everyone[:]
        rng.shuffle(fills)
        fills = [j for j in fills if not model.sessions[j].finished]
        if c % 3 == 2 and len(fills) > 1:
            fills = fills[:rng.randint(1, len(fills))]
        n = WAVE + rng.randint(0, 40) if c in (1, 5) else rng.randint(0 if c == 4 else 1, 24)
        reqs, levels = _one_call(rng, model, fills, n, levels_given=c % 2 == 1)
        fail = {}
        if c in (3, 6):                                        # slot files that cannot be written, in up to two sessions
            for k in rng.sample(range(len(fills)), min(2, len(fills))):
                m = model.sessions[fills[k]]
                fresh = sorted({r[1] for r in reqs if r[0] == k and r[3] == "ok" and (m.local(r[1]), r[2]) not in m.present})
                if m.files and fresh:
                    fail[k] = rng.choice(fresh)
        if c == 2 and reqs:
            for step in _refusals(rng, model, fills, *_one_call(rng, model, fills, 12, True)):
                run(step)
            for step in _refusals(rng, model, fills, *_one_call(rng, model, fills, 6, False)):
                run(step)
        run(["call", fills, reqs, levels, True, fail])
        if c == 3:
            plain = [j for j in everyone if not model.sessions[j].keeping and not model.sessions[j].finished]
            if plain:
                run(["keep", rng.choice(plain)])
        if c == 5 and n_sessions > 1:
            j = rng.choice(everyone)
            run(["finish", j])
            left = [x for x in everyone if x != j and not model.sessions[x].finished]
            if left:                                           # a finished session among the fills: refused, by its `fills` index
                run(["call", left[:1] + [j], [[0, model.sessions[left[0]].pairs[0][0], 0, "ok"]], None, True, {}])
    return sessions, steps


def scenario_text(sessions, steps):
    """the scenario as the check program reads it: whitespace-separated integers, one record a line"""
    kinds = {"ok": 0, "data": 1, "sib": 1}
    out = ["%d %d" % (len(sessions), len(steps))] + [" ".join(map(str, s)) for s in sessions]
    for step in steps:
        if step[0] == "keep":
            out.append("1 %d" % step[1])
        elif step[0] == "finish":
            out.append("2 %d" % step[1])
        else:
            _, fills, reqs, levels, have_paths, fail = step
            out.append("0 %d %d %d %d" % (len(fills), len(reqs), levels is not None, have_paths))
            out.append(" ".join("%d %d" % (j, fail.get(k, -1)) for k, j in enumerate(fills)))
            for i, (k, s, b, kind) in enumerate(reqs):
                out.append("%d %d %d %d %d" % (k, s, b, levels[i] if levels is not None else 0, kinds[kind]))
    return "\n".join(out) + "\n"


def expected_lines(sessions, steps):
    model = ManyModel(sessions)
    out = model.state_lines()
    for step in steps:
        out += model.step_lines(step)
    return out
