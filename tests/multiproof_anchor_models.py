"""The model of multiproofs against what a fill session knows (csrc/multiproof_anchor_plan.hpp, k_multiproof_tops, k_multiproof_fold): the
want list of a group against a known set, an independent restatement beside it, the work table, kept inputs, jobs, tops and commit list of
a call, a verifier over any keyed compression (the tests pass the C oracle's), a model fill, and the cases of the launcher test.  Plain
Python, no device and no library: tests/test_multiproof_anchor_cpu.py holds it against the issue's literals, against the restatement,
against tests/multiproof_models.py where only the root is known, and against the product's plan;
tests/test_gpu_multiproof_anchor_unit.py takes its tables and cases to the launcher."""
import numpy as np

import multiproof_models as M

depth, layer_sizes, ZERO, canonical = M.depth, M.layer_sizes, M.ZERO, M.canonical
PAIR, KEPT, SENT, NONE = 0, 1, 2, 3


def is_known(n_blocks, known, l, i):
    """the stated slot root always counts as known"""
    return l == depth(n_blocks) or (l, i) in known


def walk(n_blocks, B, known):
    """The format, level by level: (sent [(l, i)], kept [(l, i)], tops [(l, i)], steps) with steps[l] = [(i, kind, parent index)] for every
    unknown node of A_l that is not the right half of a pair.  B distinct, known a set of (level, index)."""
    A, m, sent, kept, tops, steps = sorted(B), n_blocks, [], [], [], []
    for l in range(depth(n_blocks) + 1):
        here, nxt, unknown = [], [], {i for i in A if not is_known(n_blocks, known, l, i)}
        for i in A:
            if i not in unknown:
                tops.append((l, i))
                continue
            if i & 1 and i ^ 1 in unknown:
                continue                                 # taken by its left sibling
            s = i ^ 1
            if s >= m:
                kind = NONE
            elif is_known(n_blocks, known, l, s):
                kind = KEPT
                kept.append((l, s))
            elif s in unknown:
                kind = PAIR
            else:
                kind = SENT
                sent.append((l, s))
            here.append((i, kind))
            nxt.append(i >> 1)
        steps.append(here)
        A, m = nxt, (m + 1) >> 1
    return sent, kept, tops, steps


def want(n_blocks, B, known):
    return walk(n_blocks, B, known)[0]


def restated(n_blocks, B, known):
    """the issue's independent restatement: per block the lowest known level a_b on its way up; sent = siblings - chains - known"""
    sizes, chains, sibs = layer_sizes(n_blocks), set(), set()
    for b in B:
        a = next(l for l in range(depth(n_blocks) + 1) if is_known(n_blocks, known, l, b >> l))
        for l in range(a):
            chains.add((l, b >> l))
            if (b >> l) ^ 1 < sizes[l]:
                sibs.add((l, (b >> l) ^ 1))
    return sorted(x for x in sibs - chains if not is_known(n_blocks, known, *x))


def anchor_level(n_blocks, known, b):
    return next(l for l in range(depth(n_blocks) + 1) if is_known(n_blocks, known, l, b >> l))


def anchored_leaves(n_blocks, B, known):
    """what ONE cp2_fill_add_anchored of B at the lowest anchors makes known (FillPlan::mark_proved_anchored): per block its root unless
    that is the anchor, its in-range siblings below the anchor and the ancestors strictly between"""
    sizes, out = layer_sizes(n_blocks), set()
    for b in B:
        a = anchor_level(n_blocks, known, b)
        if a > 0:
            out.add((0, b))
        for l in range(a):
            if (b >> l) ^ 1 < sizes[l]:
                out.add((l, (b >> l) ^ 1))
            if l + 1 < a:
                out.add((l + 1, b >> (l + 1)))
    return out


class Plan:
    """groups = [(n_blocks, B sorted, known set)].  Work rows: the n leaves in request order, the sent rows packed in group order, the kept
    inputs group after group in walk order, then the computed rows level after level, group-major inside a level.  jobs[l] = [(left, right,
    key, group)]: no job has `last`.  node[row] = (group, level, index); tops = [(row, group, level, index)] group-major; commit = the rows
    a proved group leaves."""

    def __init__(self, groups):
        self.groups = [(n, sorted(B), set(k)) for n, B, k in groups]
        self.n = sum(len(B) for _, B, _ in self.groups)
        walks = [walk(n, B, k) for n, B, k in self.groups]
        self.node, at, row = {}, 0, self.n
        cur = []
        for g, (n, B, _) in enumerate(self.groups):
            cur.append({b: at + j for j, b in enumerate(B)})
            for j, b in enumerate(B):
                self.node[at + j] = (g, 0, b)
            at += len(B)
        sent_row, kept_row = [], []
        for g, w in enumerate(walks):
            sent_row.append({})
            for l, i in w[0]:
                sent_row[g][(l, i)] = row
                self.node[row] = (g, l, i)
                row += 1
        self.n_rows = row - self.n
        self.kept_base = row
        for g, w in enumerate(walks):
            kept_row.append([])
            for l, i in w[1]:
                kept_row[g].append(row)
                self.node[row] = (g, l, i)
                row += 1
        self.n_kept = row - self.kept_base
        self.level_base, self.jobs, tops = [], [], [[] for _ in self.groups]
        levels = max(depth(n) for n, _, _ in self.groups)
        for l in range(levels + 1):
            jobs = []
            if l < levels:
                self.level_base.append(row)
            for g, (n, B, k) in enumerate(self.groups):
                if depth(n) < l:
                    continue
                steps, nxt = walks[g][3][l], {}
                for i in sorted(cur[g]):
                    if is_known(n, k, l, i):
                        tops[g].append((cur[g][i], g, l, i))
                for i, kind in steps:
                    other = cur[g][i ^ 1] if kind == PAIR else kept_row[g].pop(0) if kind == KEPT else sent_row[g][(l, i ^ 1)] if kind == SENT else ZERO
                    left, right = (other, cur[g][i]) if i & 1 else (cur[g][i], other)
                    jobs.append((left, right, int(l == 0) + (2 if kind == NONE else 0), g))
                    self.node[row] = (g, l + 1, i >> 1)
                    nxt[i >> 1] = row
                    row += 1
                cur[g] = nxt
            if l < levels:
                self.jobs.append(jobs)
            else:
                assert not jobs
        self.n_work = row
        self.level_off = [0]
        for jobs in self.jobs:
            self.level_off.append(self.level_off[-1] + len(jobs))
        self.tops, self.top_off = [], [0]
        for t in tops:
            self.tops += t
            self.top_off.append(len(self.tops))
        top_rows = {t[0] for t in self.tops}
        self.commit = [r for r in range(self.n_work) if r not in top_rows and not self.kept_base <= r < self.kept_base + self.n_kept]

    def computed(self):
        return self.level_off[-1]

    def tables(self):
        flat = [j for jobs in self.jobs for j in jobs]
        return (np.array(flat, dtype=np.uint32).reshape(-1, 4), np.array(self.level_off, dtype=np.uint64), np.array(self.level_base, dtype=np.uint64))

    def left_known(self, g):
        """the places group g makes known when it proves"""
        return {self.node[r][1:] for r in self.commit if self.node[r][0] == g}


def verify(compress, n_blocks, B, known, leaves, rows, kept_row, root):
    """(holds, {(level, index): bytes of every computed node}); leaves in the order of sorted B, rows in want order, kept_row(l, i) the
    32 bytes the session keeps at a known place"""
    p = Plan([(n_blocks, B, known)])
    if len(rows) != p.n_rows or len(leaves) != p.n:
        return False, {}
    work = [canonical(x) for x in leaves] + [canonical(x) for x in rows] + [canonical(kept_row(*p.node[p.kept_base + k][1:])) for k in range(p.n_kept)]
    nodes = {}
    for jobs in p.jobs:
        for left, right, key, _ in jobs:
            work.append(np.array(compress(work[left], work[right] if right != ZERO else np.zeros(32, dtype=np.uint8), key), dtype=np.uint8))
            nodes[p.node[len(work) - 1][1:]] = work[-1]
    ok = bool(p.tops)
    for r, _, l, i in p.tops:
        ok = ok and bool(np.array_equal(work[r], canonical(root if l == depth(n_blocks) else kept_row(l, i))))
    return ok, nodes


def derive(n_blocks, present):
    """FillPlan::derive_from_presence: what a session knows from presence alone"""
    sizes, known = layer_sizes(n_blocks), {(0, b) for b in present}
    for l in range(depth(n_blocks)):
        for k in range(sizes[l + 1]):
            if (l, 2 * k) in known and (2 * k + 1 >= sizes[l] or (l, 2 * k + 1) in known):
                known.add((l + 1, k))
    return known


def random_known(rng, n_blocks, share):
    """a seeded known set below the root: each place with probability `share`"""
    sizes = layer_sizes(n_blocks)
    return {(l, i) for l in range(depth(n_blocks)) for i in range(sizes[l]) if rng.random() < share}


# ---- the scenario files of tests/host_check/multiproof_anchor_check.cpp and the lines it must print --------------------------------------------
def known_words(n_blocks, known):
    return " ".join("%d %d" % x for x in sorted(known))


def want_cmd(n_blocks, B, known):
    return "want %d %d %s %d %s" % (n_blocks, len(B), " ".join(map(str, B)), len(known), known_words(n_blocks, known))


def want_line(n_blocks, B, known):
    return " ".join(["want"] + ["%d:%d" % x for x in want(n_blocks, B, known)])


def plan_cmd(groups):
    return "plan %d %s" % (len(groups), " ".join("%d %d %s %d %s" % (n, len(B), " ".join(map(str, B)), len(k), known_words(n, k)) for n, B, k in groups))


def plan_lines(groups):
    p = Plan(groups)
    out = ["plan n %d n_rows %d n_kept %d n_work %d levels %d computed %d tops %d" % (p.n, p.n_rows, p.n_kept, p.n_work, len(p.jobs), p.computed(), len(p.tops))]
    for l, jobs in enumerate(p.jobs):
        out.append("level %d base %d jobs %d" % (l, p.level_base[l], len(jobs)))
        out += ["job %d %d %d %d" % j for j in jobs]
    out += ["row %d %d %d %d" % ((r,) + p.node[r]) for r in range(p.n_work)]
    out += ["top %d %d %d %d" % t for t in p.tops]
    out.append(" ".join(["top_off"] + [str(x) for x in p.top_off]))
    out.append(" ".join(["commit"] + [str(x) for x in p.commit]))
    return out


def fill_cmd(n_blocks, first, n_local, steps):
    """steps = [[(slot, verdict, B)]]: calls one after the other on one session that keeps nodes"""
    return "fill %d %d %d %d %s" % (n_blocks, first, n_local, len(steps), " ".join(
        "%d %s" % (len(call), " ".join("%d %d %d %s" % (s, v, len(B), " ".join(map(str, B))) for s, v, B in call)) for call in steps))


def fill_lines(n_blocks, first, n_local, steps):
    """per call the rows its groups want against the session as it stands, and the known bitmap after it by the ANCHORED rule: per proved
    group what one add_anchored of its blocks at their lowest anchors leaves"""
    known = [set() for _ in range(n_local)]
    sizes, out = layer_sizes(n_blocks), []
    rows = n_local * sum(sizes)
    for call in steps:
        before = [set(k) for k in known]
        out.append(" ".join(["rows"] + [str(len(want(n_blocks, B, before[s - first]))) for s, _, B in call]))
        for s, v, B in call:
            if v == 0:
                known[s - first] |= anchored_leaves(n_blocks, B, before[s - first])
        words = [0] * ((rows + 63) // 64)
        for s in range(n_local):
            for l, i in known[s]:
                r = M.node_row(n_blocks, n_local, l, s, i)
                words[r >> 6] |= 1 << (r & 63)
        out.append(" ".join(["known"] + ["%x" % w for w in words]))
    return out


def stale_text(call, n_rows, wanted):
    return "%s: n_rows = %d, the groups' want lists against the session as it stands hold %d rows" % (call, n_rows, wanted)


# ---- the launcher test's cases ------------------------------------------------------------------------------------------------------------------
N_TOPS = (1, 63, 64, 65, 257, 4097)
WRONG_KINDS = ("low byte", "top limb", "swapped")


class TopsCase:
    """n_tops tops dealt out to groups: top_off (n_groups + 1), level[t] (where the kept row of top t sits: the test only needs variety),
    wrong = {top: kind}.  The expected top_verdict and verdict follow from `wrong` alone."""

    def __init__(self, no, sizes, levels, wrong):
        self.no, self.sizes, self.levels, self.wrong = no, sizes, levels, wrong
        self.top_off = [0]
        for s in sizes:
            self.top_off.append(self.top_off[-1] + s)
        self.n_tops, self.n_groups = self.top_off[-1], len(sizes)

    def group_of(self, t):
        return next(g for g in range(self.n_groups) if self.top_off[g] <= t < self.top_off[g + 1])

    def expected(self):
        tv = [int(t in self.wrong) for t in range(self.n_tops)]
        return tv, [int(any(tv[self.top_off[g]:self.top_off[g + 1]])) for g in range(self.n_groups)]


def tops_cases():
    """Case 0: one group, one top, right; case 1: one group, one top, wrong.  Then one case per n_tops of N_TOPS above 1: group sizes drawn
    from 1 .. 9 with a few long groups (70 and 300 tops: ranges that straddle wave and workgroup boundaries), tops of one group at level 0
    throughout, others at three or more levels.  Wrong tops: the groups are dealt out so that between 15 % and 40 % hold a wrong top, at
    least one group is all right, and at least one failing group has exactly one wrong top among several."""
    rng = np.random.default_rng(0x7A11)
    out = [TopsCase(0, [1], [0], {}), TopsCase(1, [1], [3], {0: "low byte"})]
    for n_tops in N_TOPS[1:]:
        sizes, have = [], 0
        long = [70, 300] if n_tops >= 4097 else [70] if n_tops >= 257 else []
        while have < n_tops:
            s = long.pop() if long and rng.random() < 0.2 else int(rng.integers(1, 6 if n_tops < 100 else 10))
            s = min(s, n_tops - have)
            sizes.append(s)
            have += s
        levels = []
        for g, s in enumerate(sizes):
            levels += [0] * s if g % 3 == 0 else [int(x) for x in rng.integers(0, 8, size=s)] if s < 3 else [0, 3, 6] + [int(x) for x in rng.integers(0, 8, size=s - 3)]
        case = TopsCase(len(out), sizes, levels, {})
        n_wrong = max(3, round(0.27 * len(sizes)))
        several = [g for g, s in enumerate(sizes) if s >= 3]
        pairs = [g for g, s in enumerate(sizes) if s >= 2 and g != several[0]]
        groups = [several[0], pairs[0]] + [int(g) for g in rng.permutation(len(sizes)) if g not in (several[0], pairs[0])][:n_wrong - 2]
        for j, g in enumerate(groups):
            t0, t1 = case.top_off[g], case.top_off[g + 1]
            if j == 0:                                     # exactly one wrong top among several
                case.wrong[t0 + 1] = "low byte"
            elif j == 1:                                   # a swap makes two tops wrong, both inside the group
                case.wrong[t0] = case.wrong[t0 + 1] = "swapped"
            else:
                for t in rng.choice(np.arange(t0, t1), size=int(rng.integers(1, min(3, t1 - t0) + 1)), replace=False):
                    case.wrong[int(t)] = ("top limb", "low byte")[len(case.wrong) % 2]
        out.append(case)
    return out


def tops_condition(case):
    """the issue's condition on every case of more than one group"""
    _, v = case.expected()
    failing = [g for g in range(case.n_groups) if v[g]]
    one_among_several = [g for g in failing if case.sizes[g] > 1 and sum(t in case.wrong for t in range(case.top_off[g], case.top_off[g + 1])) == 1]
    return 0.15 <= len(failing) / case.n_groups <= 0.40 and len(failing) < case.n_groups and bool(one_among_several)
