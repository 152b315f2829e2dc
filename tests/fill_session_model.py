"""One plain model of a whole fill session (include/codex_p2.h: cp2_fill_*), composed from the models of its single features --
tests/fill_nodes_models.py (presence, known rows, proof statuses), fill_anchor_models.py (anchors, anchored adds), fill_adopt_models.py (the
judgement of an adopt) and fill_resume_models.py (what a checkpoint holds) -- and a seeded generator of operation sequences that cross the
features in orders nobody scripted.  It imports nothing from the product.

The session covers local slots [first, first + n_local) of n_blocks blocks.  Its state: which (local, block) pairs are present, which rows
of the compact layout are known, whether nodes are kept, which candidate block roots an adopt remembers (each 'T': the true root, or 'D':
the root of damaged bytes), what the last checkpoint holds, and per slot file how many whole blocks it covers and whether each holds the
true bytes ('T') or anything else ('D': a flipped byte, the zeros of a hole).  Every operation is plain data (lists of ints and strings), so
a sequence can be printed, pasted back and replayed:

  ["add", [[slot, block, kind], ...], fail_slot]         kind: "ok", "data" (one data byte flipped) or "sib" (one sibling flipped);
                                                         fail_slot: None, or the slot whose file cannot be written during this call
  ["anchored", [[slot, block, level, kind], ...], fail_slot]
  ["keep"]   ["save"]   ["resume", trust_files]          (resume frees the session and opens the last checkpoint)
  ["anchors", [[slot, block], ...]]   ["proofs", [[slot, block], ...]]   ["missing", cap]
  ["damage", slot, "flip", block] / [.., "truncate", n_bytes_in_blocks_x2] / [.., "remove", 0]    (truncate: to arg / 2 blocks, halves allowed)
  ["place", slot, [block, ...]]                          true bytes of absent blocks written into the file, as a crashed writer leaves them
  ["adopt", first_slot, n_slots, no_read]                n_slots 0: every local slot
  ["finish"]

apply(op) returns what the product must report: {"err": 0 or a negative status, ...results}."""
import random
from collections import Counter

import fill_adopt_models as D
import fill_anchor_models as A
import fill_nodes_models as M
import fill_resume_models as R

OK, ERR_INVALID, ERR_IO = 0, -1, -5
FILL_NEW, FILL_MISMATCH, FILL_DUPLICATE, FILL_UNWRITTEN = 0, 1, 2, 3
PROOF_OK, PROOF_ABSENT, PROOF_PARTIAL = M.PROOF_OK, M.PROOF_ABSENT, M.PROOF_PARTIAL

# name: (blocks per slot, first local slot, local slots) of a dataset of four slots; cells of 64 bytes, blocks of 256
SHAPES = {"b1": (1, 1, 3), "b2": (2, 0, 2), "b8": (8, 0, 4), "b16": (16, 2, 2), "b64": (64, 0, 4)}
FAKE_SHAPES = ("b8", "b16")
# three seeds per shape and source, chosen so that tests/test_fill_session_model_cpu.py's coverage conditions hold with these step counts
SEEDS = {"b1": (1, 10, 18), "b2": (1, 2, 14), "b8": (1, 2, 24), "b16": (1, 2, 37), "b64": (1, 2, 12)}
FAKE_SEEDS = {"b8": (1, 2, 3), "b16": (1, 2, 3)}
STEPS = {"b1": 16, "b2": 16, "b8": 40, "b16": 40, "b64": 40}
OP_KINDS = ("add", "anchored", "keep", "save", "resume", "anchors", "proofs", "missing", "damage", "place", "adopt", "finish")
FAKE_OP_KINDS = tuple(k for k in OP_KINDS if k not in ("damage", "place", "adopt"))
CONDITIONS = ("anchored_inner_level", "anchor_proved_by_adopt", "adopt_strict_subset", "no_read_adopt_after_add", "resume_drops",
              "resume_drops_none", "keep_after_add", "keep_after_resume", "partial_then_ok", "unwritten_then_present",
              "new_duplicate_mismatch_in_one_call", "finish_refused_then_finished")


class SessionModel:
    def __init__(self, shape, files=True):
        self.nb, self.first, self.n_local = shape
        self.files = files
        self.depth = A.depth_of(self.nb)
        self.sizes, self.offs, self.rows = M.layout(self.nb, self.n_local)
        self.pairs = [(self.first + s, b) for s in range(self.n_local) for b in range(self.nb)]
        # the true node of every row as a name, compress as a tuple builder (injective by construction), as in fill_adopt_models.Slot
        self.truth = [None] * self.rows
        for s in range(self.n_local):
            for b in range(self.nb):
                self.truth[self.row(0, s, b)] = ("leaf", s, b)
            for lvl in range(self.depth):
                for j in range(self.sizes[lvl + 1]):
                    pair = 2 * j + 1 < self.sizes[lvl]
                    right = self.truth[self.row(lvl, s, 2 * j + 1)] if pair else 0
                    self.truth[self.row(lvl + 1, s, j)] = (self.truth[self.row(lvl, s, 2 * j)], right, (1 if lvl == 0 else 0) + (0 if pair else 2))
        self.node = A.Session(self.nb, self.n_local)      # present, known, keeping
        self.finished = False
        self.resumed = False                              # this session came from a checkpoint
        self.ckpt = None                                  # the presence the last checkpoint holds
        self.disk = {s: None for s in range(self.n_local)}   # per local slot: None (no file) or the labels of the whole blocks it covers
        self.remember = {}                                # (local, block) -> 'T' / 'D': the candidates an adopt remembers
        self.stale = set()                                # local slots whose file the sequence changed since an adopt last read it
        # what the coverage conditions need
        self.cov = Counter()
        self.proved_by = {}                               # row -> "add" / "adopt" / "keep": what first made it known in this session
        self.known_grew = False                           # an add or anchored add made a row known since the last adopt
        self.partial_seen = set()
        self.unwritten = set()
        self.finish_refused = False

    # ---- layout ------------------------------------------------------------------------------------------------------------------------
    def row(self, lvl, s, k):
        return self.offs[lvl] + s * self.sizes[lvl] + k

    def local(self, slot):
        return slot - self.first

    @property
    def present(self):
        return self.node.present

    @property
    def known(self):
        return self.node.known

    @property
    def keeping(self):
        return self.node.keeping

    def _learn(self, rows, how):
        for r in rows:
            if r not in self.node.known:
                self.proved_by[r] = how
                if how == "add":
                    self.known_grew = True
        self.node.known.update(rows)

    # ---- what a caller can observe --------------------------------------------------------------------------------------------------------
    def missing(self):
        return [p for p in self.pairs if (self.local(p[0]), p[1]) not in self.present]

    def anchor_levels(self):
        return [self.node.anchor(self.local(s), b) for s, b in self.pairs]

    def proof_statuses(self):
        return [self.node.status(self.local(s), b) for s, b in self.pairs]

    def checkpoint_bits(self):
        """the presence bits of a checkpoint saved now, in fill_resume_models.parse_checkpoint's order (local-major)"""
        return [1 if (s, b) in self.present else 0 for s in range(self.n_local) for b in range(self.nb)]

    def pending(self):
        """the remembered candidates no adopt has proved yet, in slots whose files the sequence has not touched since they were read"""
        return sorted(p for p in self.remember if p not in self.present and p[0] not in self.stale)

    def file_exists(self, s):
        return self.disk[s] is not None

    def covered(self, s, b):
        return self.disk[s] is not None and b < len(self.disk[s])

    # ---- the slot files --------------------------------------------------------------------------------------------------------------------
    def _write(self, s, b):
        """pwrite of the true block at its offset: a missing file is created, a hole before it reads as zeros"""
        d = self.disk[s] if self.disk[s] is not None else []
        d.extend("D" * (b + 1 - len(d)))
        d[b] = "T"
        self.disk[s] = d

    # ---- operations ------------------------------------------------------------------------------------------------------------------------
    def apply(self, op):
        res = getattr(self, "op_" + op[0])(*op[1:])
        self.cov["op:" + op[0]] += 1
        if self.keeping and not self.finished:
            for p, st in zip(self.pairs, self.proof_statuses()):
                if st == PROOF_PARTIAL:
                    self.partial_seen.add(p)
                elif st == PROOF_OK and p in self.partial_seen:
                    self.partial_seen.discard(p)
                    self.cov["partial_then_ok"] += 1
        return res

    def _settle(self, pairs, proved, fail_slot):
        """NEW / DUPLICATE, the writer and its roll-back, presence: what cp2_fill_add and cp2_fill_add_anchored share"""
        status, seen = [], set()
        for p, ok in zip(pairs, proved):
            if not ok:
                status.append(FILL_MISMATCH)
            else:
                status.append(FILL_DUPLICATE if p in self.present or p in seen else FILL_NEW)
                seen.add(p)
        err = OK
        if self.files:
            failing = fail_slot is not None and any(st == FILL_NEW and p[0] == self.local(fail_slot) for p, st in zip(pairs, status))
            lost = {p for p, st in zip(pairs, status) if failing and st == FILL_NEW and p[0] >= self.local(fail_slot)}
            if lost:
                err = ERR_IO
                status = [FILL_UNWRITTEN if p in lost and st in (FILL_NEW, FILL_DUPLICATE) else st for p, st in zip(pairs, status)]
                if self.keeping:
                    self.unwritten.update(lost)
            for p, st in sorted(zip(pairs, status)):
                if st == FILL_NEW:
                    self._write(*p)
        n_new = 0
        for p, st in zip(pairs, status):
            if st == FILL_NEW:
                n_new += 1
                self.present.add(p)
                if p in self.unwritten:
                    self.unwritten.discard(p)
                    self.cov["unwritten_then_present"] += 1
        if {FILL_NEW, FILL_DUPLICATE, FILL_MISMATCH} <= set(status):
            self.cov["new_duplicate_mismatch_in_one_call"] += 1
        return {"err": err, "status": status, "n_new": n_new}

    def op_add(self, reqs, fail_slot=None):
        if self.finished:
            return {"err": ERR_INVALID}
        pairs = [(self.local(s), b) for s, b, _ in reqs]
        proved = [kind == "ok" for _, _, kind in reqs]
        if self.keeping:
            for (s, b), ok in zip(pairs, proved):
                if ok:
                    self._learn(M.stored_rows(self.nb, self.n_local, s, b), "add")
        return self._settle(pairs, proved, fail_slot)

    def op_anchored(self, reqs, fail_slot=None):
        if self.finished or not self.keeping:
            return {"err": ERR_INVALID}
        pairs = [(self.local(s), b) for s, b, _, _ in reqs]
        if not all(lvl <= self.depth and self.node.accepts(s, b, lvl) for (s, b), (_, _, lvl, _) in zip(pairs, reqs)):
            return {"err": ERR_INVALID}                   # a level whose node was not known when the call started
        proved = [kind == "ok" for _, _, _, kind in reqs]
        anchors = [A.anchor_row(self.nb, self.n_local, s, b, lvl) for (s, b), (_, _, lvl, _) in zip(pairs, reqs)]
        from_adopt = [r is not None and self.proved_by.get(r) == "adopt" for r in anchors]
        for (s, b), (_, _, lvl, _), ok in zip(pairs, reqs, proved):
            if ok:
                self._learn(A.stored_rows(self.nb, self.n_local, s, b, lvl), "add")
        res = self._settle(pairs, proved, fail_slot)
        for (_, _, lvl, _), st, fa in zip(reqs, res["status"], from_adopt):
            if st == FILL_NEW and 0 < lvl < self.depth:
                self.cov["anchored_inner_level"] += 1
            if st != FILL_MISMATCH and fa:                # the walk ended in a row k_adopt_resolve wrote, and matched it
                self.cov["anchor_proved_by_adopt"] += 1
        return res

    def op_keep(self):
        if self.finished:
            return {"err": ERR_INVALID}
        if not self.keeping:
            if self.resumed:
                self.cov["keep_after_resume"] += 1
            elif self.present:
                self.cov["keep_after_add"] += 1
            self.node.keep_nodes()                        # what presence gives: fill_nodes_models.Session.keep_nodes
            self.proved_by = {r: "keep" for r in self.node.known}
        return {"err": OK}

    def op_anchors(self, pairs):
        if self.finished:
            return {"err": ERR_INVALID}
        return {"err": OK, "levels": [self.node.anchor(self.local(s), b) for s, b in pairs]}

    def op_proofs(self, pairs):
        if self.finished or not self.keeping:
            return {"err": ERR_INVALID}
        return {"err": OK, "status": [self.node.status(self.local(s), b) for s, b in pairs]}

    def op_missing(self, cap):
        m = self.missing()
        return {"err": OK, "missing": [list(p) for p in m[:cap]], "n_missing": len(m)}

    def op_save(self):
        if self.finished:
            return {"err": ERR_INVALID}
        self.ckpt = frozenset(self.present)               # layer 0 and the presence bitmap, nothing of the known rows
        return {"err": OK}

    def op_resume(self, trust):
        """cp2_fill_free, then cp2_fill_resume of the last checkpoint: a session begun fresh that has received exactly the surviving blocks; it
        keeps no nodes until it is told to, and remembers no candidates"""
        assert self.ckpt is not None and not self.finished
        dropped = set()
        if not trust and self.files:                      # the fake source regenerates its blocks: always clean
            dropped = {(s, b) for s, b in self.ckpt if not self.covered(s, b) or self.disk[s][b] != "T"}
        self.node = A.Session(self.nb, self.n_local)
        self.node.present = set(self.ckpt) - dropped
        self.resumed, self.remember, self.stale, self.proved_by = True, {}, set(), {}
        self.partial_seen, self.unwritten, self.known_grew = set(), set(), False
        if not trust:
            self.cov["resume_drops" if dropped else "resume_drops_none"] += 1
        return {"err": OK, "n_dropped": len(dropped)}

    def op_damage(self, slot, how, arg):
        s = self.local(slot)
        assert self.files and self.disk[s] is not None
        if how == "flip":
            assert arg < len(self.disk[s])
            self.disk[s][arg] = "D"
        elif how == "truncate":
            self.disk[s] = self.disk[s][:arg // 2]
        else:
            self.disk[s] = None
        self.stale.add(s)
        return {"err": OK}

    def op_place(self, slot, blocks):
        s = self.local(slot)
        assert self.files and all((s, b) not in self.present for b in blocks)
        for b in blocks:
            self._write(s, b)
        self.stale.add(s)
        return {"err": OK}

    def op_adopt(self, first_slot, n_slots, no_read):
        if self.finished or not self.keeping or not self.files:
            return {"err": ERR_INVALID}
        s0, ns = (0, self.n_local) if n_slots == 0 else (self.local(first_slot), n_slots)
        slots = list(range(s0, s0 + ns))
        n_read = 0
        if not no_read:                                   # a read refreshes what is remembered of the slots it covers
            self.remember = {p: v for p, v in self.remember.items() if p[0] not in slots}
            for s in slots:
                for b in range(self.nb):
                    if (s, b) not in self.present and self.covered(s, b):
                        self.remember[(s, b)] = self.disk[s][b]
                        n_read += 1
                self.stale.discard(s)
        self.remember = {p: v for p, v in self.remember.items() if p not in self.present}   # present in the meantime: no candidate any more
        flags = [D.KNOWN if r in self.known else 0 for r in range(self.rows)]
        for s in range(self.n_local):
            flags[self.row(self.depth, s, 0)] |= D.KNOWN  # the stated slot root always counts
        cand = [None] * self.rows
        for (s, b), label in self.remember.items():
            if s in slots:
                flags[self.row(0, s, b)] |= D.CAND
                cand[self.row(0, s, b)] = self.truth[self.row(0, s, b)] if label == "T" else ("damaged", s, b)
        roots = [self.truth[self.row(self.depth, s, 0)] for s in range(self.n_local)]
        cand, flags = D.layers(self.nb, self.n_local, slots, self.truth, cand, flags, roots, lambda x, y, key: (x, y, key), 0)
        out, _ = D.resolve(self.nb, self.n_local, slots, self.truth, cand, flags)
        self._learn([r for r in range(self.rows) if out[r] & D.PROVED and r not in self.known], "adopt")
        got = [(s, b) for s in slots for b in range(self.nb) if out[self.row(0, s, b)] & D.ADOPTED and (s, b) not in self.present]
        self.present.update(got)
        if not no_read and 0 < len(got) < n_read:
            self.cov["adopt_strict_subset"] += 1
        if no_read and got and self.known_grew:
            self.cov["no_read_adopt_after_add"] += 1
        self.known_grew = False
        return {"err": OK, "n_read": n_read, "n_adopted": len(got)}

    def op_finish(self):
        if self.finished or self.missing():
            if not self.finished:
                self.finish_refused = True
            return {"err": ERR_INVALID}
        self.finished = True
        if self.finish_refused:
            self.cov["finish_refused_then_finished"] += 1
        return {"err": OK}


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def _weights(m, files):
    """how likely each operation is in the model's state; 0 where it would mean nothing"""
    absent = len(m.missing())
    w = {"add": 6 if absent else 1, "anchors": 1, "proofs": 1, "missing": 1, "save": 2, "finish": 1 if absent else 0}
    w["keep"] = 1 if m.keeping else 3 if m.present or m.resumed else 1
    w["anchored"] = (5 if absent else 1) if m.keeping else 0.3   # on a session that keeps no nodes: refused, as the header says
    w["resume"] = 0 if m.ckpt is None else 2
    if files:
        w["damage"] = 2 if any(m.disk[s] for s in range(m.n_local)) else 0
        w["place"] = 2 if absent else 0
        w["adopt"] = (8 if m.pending() and m.known_grew else 4) if m.keeping else 0.3
    return w


def _requests(rng, m, files):
    """a batch for add: mostly absent blocks, some present ones, some pairs twice, some that will not prove"""
    absent, present = m.missing(), [p for p in m.pairs if p not in set(m.missing())]
    # blocks whose path would vouch for candidates an adopt has read and could not prove: absent neighbours in the same slot
    beside = [p for p in absent if (m.local(p[0]), p[1]) not in m.remember and any(s == m.local(p[0]) for s, _ in m.pending())]
    reqs = []
    for _ in range(rng.randint(1, 7)):
        x = rng.random()
        if beside and x < 0.3:
            s, b = rng.choice(beside)
        elif reqs and x < 0.45:
            s, b = rng.choice(reqs)[:2]
        elif present and (x < 0.6 or not absent):
            s, b = rng.choice(present)
        elif absent:
            s, b = rng.choice(absent)
        else:
            s, b = rng.choice(m.pairs)
        y = rng.random()
        reqs.append([s, b, "ok" if y < 0.78 else "data" if y < 0.9 else "sib"])
    return reqs


def _fail_slot(rng, m, reqs, files):
    """sometimes the file of a slot that would take a new block cannot be written.  Whichever way the caller brings that about, a file that
    does not exist yet must not be asked for before the failing one: such requests leave the batch."""
    if not files or rng.random() > 0.15:
        return reqs, None
    fresh = sorted({r[0] for r in reqs if r[-1] == "ok" and (m.local(r[0]), r[1]) not in m.present})
    if not fresh:
        return reqs, None
    fail = rng.choice(fresh)
    reqs = [r for r in reqs if r[0] >= fail or m.file_exists(m.local(r[0]))]
    return reqs, fail


def _propose(rng, m, files):
    w = _weights(m, files)
    kind = rng.choices(list(w), weights=list(w.values()))[0]
    if kind == "add":
        reqs, fail = _fail_slot(rng, m, _requests(rng, m, files), files)
        return ["add", reqs, fail]
    if kind == "anchored":
        reqs = []
        for s, b, how in _requests(rng, m, files):
            a = m.node.anchor(m.local(s), b)
            lvl = a if rng.random() < 0.65 else rng.randint(a, m.depth)
            if how == "sib" and lvl == 0:
                how = "data"                              # no sibling to flip
            reqs.append([s, b, lvl, how])
        if m.keeping and rng.random() < 0.1:              # one level below its anchor: the whole call is refused
            low = [r for r in reqs if m.node.anchor(m.local(r[0]), r[1]) > 0]
            if low:
                r = rng.choice(low)
                r[2] = rng.randrange(m.node.anchor(m.local(r[0]), r[1]))
                return ["anchored", reqs, None]
        if not m.keeping:
            return ["anchored", reqs, None]
        reqs, fail = _fail_slot(rng, m, reqs, files)
        return ["anchored", reqs, fail]
    if kind in ("anchors", "proofs"):
        return [kind, [list(rng.choice(m.pairs)) for _ in range(rng.randint(1, 6))]]
    if kind == "missing":
        return ["missing", rng.choice((0, 1, 3, 1 << 20))]
    if kind == "resume":
        return ["resume", rng.random() < 0.3]
    if kind == "damage":
        s = rng.choice([s for s in range(m.n_local) if m.disk[s]])
        x = rng.random()
        if x < 0.7:
            return ["damage", m.first + s, "flip", rng.randrange(len(m.disk[s]))]
        if x < 0.9:
            return ["damage", m.first + s, "truncate", rng.randrange(2 * len(m.disk[s]))]
        return ["damage", m.first + s, "remove", 0]
    if kind == "place":
        s = rng.choice(sorted({m.local(p[0]) for p in m.missing()}))
        blocks = [b for b in range(m.nb) if (s, b) not in m.present]
        if rng.random() < 0.5:
            k = rng.randrange(len(blocks))
            blocks = blocks[k:k + rng.randint(1, max(1, m.nb // 2))]
        return ["place", m.first + s, blocks]
    if kind == "adopt":
        if rng.random() < 0.4:
            s0, ns, first, n = 0, m.n_local, m.first, 0
        else:
            s0 = rng.randrange(m.n_local)
            ns = rng.randint(1, m.n_local - s0)
            first, n = m.first + s0, ns
        # CP2_ADOPT_NO_READ trusts the files unchanged since they were read: only where the sequence has not touched them since
        no_read = rng.random() < (0.8 if m.pending() and m.known_grew else 0.3) and not any(s in m.stale for s in range(s0, s0 + ns))
        return ["adopt", first, n, no_read]
    return [kind]


def _tail(m):
    """whatever is missing arrives, the session finishes, and a finished session refuses a second finish and an add"""
    ops = []

    def push(op):
        m.apply(op)
        ops.append(op)

    if m.files and any(not m.covered(s, b) or m.disk[s][b] != "T" for s, b in m.present):
        # present blocks the disk no longer backs (a trusting resume, damage after the last re-check): the finished dataset reads its slot
        # files, so a re-checking resume takes them back first and they arrive again
        push(["save"])
        push(["resume", False])
    while m.missing():
        batch = m.missing()[:16]
        if m.keeping:
            push(["anchored", [[s, b, m.node.anchor(m.local(s), b), "ok"] for s, b in batch], None])
        else:
            push(["add", [[s, b, "ok"] for s, b in batch], None])
    last = list(m.pairs[-1])
    for op in (["finish"], ["finish"], ["add", [last + ["ok"]], None]):
        push(op)
    return ops


def sequence(seed, shape, n_steps, files=True):
    """n_steps operations chosen by state-dependent weights, then the tail that completes and finishes the session; the same arguments give
    the same list"""
    rng = random.Random("fill session %d %r %d %d" % (seed, tuple(shape), n_steps, files))
    m = SessionModel(shape, files)
    ops = []
    for _ in range(n_steps):
        op = _propose(rng, m, files)
        m.apply(op)
        ops.append(op)
    return ops + _tail(m)


def replay(shape, ops, files=True):
    """the model after a literal list of operations, and what each returned"""
    m = SessionModel(shape, files)
    return m, [m.apply(op) for op in ops]


def describe(seed, shape, files, ops):
    """what a failing run prints: everything needed to run it again"""
    return "seed %r, shape %r, %s; replay with these operations:\n[%s]" % (seed, tuple(shape), "slot files" if files else "fake source",
                                                                          ",\n ".join(repr(op) for op in ops))
