"""The model of block multiproofs (csrc/multiproof_plan.hpp, k_multiproof_layer): the layout of a group's rows, brute force beside it, the
refusals in their order, the work table and the per-level job tables of a call, and a verifier over any keyed compression (the tests pass
the C oracle's).  Plain Python, no device and no library: tests/test_multiproof_cpu.py holds it against the issue's literals, against brute
force and against the product's plan; tests/test_gpu_multiproof_unit.py takes its tables and cases to the launcher."""
import numpy as np

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ZERO = 0xFFFFFFFF                 # MULTIPROOF_ZERO: the `right` of an odd layer's last node
ROW_LIMIT = 0xFFFFFFFF            # a call whose rows would reach it is refused
WAVE = 64


def depth(n_blocks):
    """cp2_block_proof_depth: ceil(log2(n)), and 1 for a single block"""
    if n_blocks == 0:
        return 0
    d, m = 1, (n_blocks + 1) >> 1
    while m > 1:
        d, m = d + 1, (m + 1) >> 1
    return d


def layer_sizes(n_blocks):
    s = [n_blocks]
    for _ in range(depth(n_blocks)):
        s.append((s[-1] + 1) >> 1)
    return s


def layout(n_blocks, B):
    """the issue's restatement: [(level, index)] of the rows, in order"""
    K, m, out = sorted(B), n_blocks, []
    for l in range(depth(n_blocks)):
        S = set(K)
        out += [(l, i ^ 1) for i in K if (i ^ 1) not in S and (i ^ 1) < m]
        K, m = sorted({i >> 1 for i in K}), (m + 1) >> 1
    return out


def brute(n_blocks, B):
    """the union over B of each block's in-range single-path siblings, minus every node on some block's own way up; as a sorted list"""
    sizes, sib, own = layer_sizes(n_blocks), set(), set()
    for b in B:
        for l in range(depth(n_blocks)):
            own.add((l, b >> l))
            if (b >> l) ^ 1 < sizes[l]:
                sib.add((l, (b >> l) ^ 1))
    return sorted(sib - own), len(sib)


# ---- validation, in the header's order ------------------------------------------------------------------------------------------------------
def refusal(call, what, groups, blocks, first, n_local, n_blocks, n_rows=None):
    """None, or the text cp2_last_error holds; groups = [(slot or root index, count)], blocks flat.  n_rows None: not checked (serving)."""
    head = call + ": group "
    for g, (_, c) in enumerate(groups):
        if c == 0:
            return head + "%d holds no block" % g
    for g, (s, _) in enumerate(groups):
        if not first <= s < first + n_local:
            return head + "%d: %s %d is not inside the range %d + %d" % (g, what, s, first, n_local)
    spans, at = [], 0
    for g, (_, c) in enumerate(groups):
        spans.append((g, at, c))
        at += c
    for g, a, c in spans:
        for i in range(a, a + c):
            if blocks[i] >= n_blocks:
                return head + "%d, request %d: block %d is not below nBlocks = %d" % (g, i, blocks[i], n_blocks)
    for g, a, c in spans:
        for i in range(a + 1, a + c):
            if blocks[i] <= blocks[i - 1]:
                return head + "%d, request %d: block %d does not ascend from %d" % (g, i, blocks[i], blocks[i - 1])
    rows = sum(len(layout(n_blocks, blocks[a:a + c])) for _, a, c in spans)
    if n_rows is not None and rows != n_rows:
        return "%s: n_rows = %d, the groups' layouts hold %d rows" % (call, n_rows, rows)
    return None


# ---- the work table and the jobs ------------------------------------------------------------------------------------------------------------
class Plan:
    """groups = [(n_blocks, B sorted)].  Work rows: the n leaves in request order, the n_rows sent rows packed, then the computed rows level
    after level, group-major inside a level.  jobs[l] = [(left, right, key | last << 8, group)]; job k of level l writes row
    level_base[l] + k.  node[row] = (group, level, index) of every row; top[g] = the row of group g's root."""

    def __init__(self, groups):
        self.groups = [(n, sorted(B)) for n, B in groups]
        self.n = sum(len(B) for _, B in self.groups)
        self.node, cur, sent, at = {}, [], [], 0
        for g, (n, B) in enumerate(self.groups):
            cur.append([(b, at + j) for j, b in enumerate(B)])
            for j, b in enumerate(B):
                self.node[at + j] = (g, 0, b)
            at += len(B)
        row = self.n
        for g, (n, B) in enumerate(self.groups):
            sent.append(row)
            for l, i in layout(n, B):
                self.node[row] = (g, l, i)
                row += 1
        self.n_rows = row - self.n
        self.level_base, self.jobs, self.top = [], [], {}
        m = [n for n, _ in self.groups]
        for l in range(max(depth(n) for n, _ in self.groups)):
            self.level_base.append(row)
            jobs = []
            for g, (n, _) in enumerate(self.groups):
                if depth(n) <= l:
                    continue
                last, c, nxt, t = int(l + 1 == depth(n)), cur[g], [], 0
                while t < len(c):
                    i, r = c[t]
                    tail = 0
                    if i & 1:
                        left, right = sent[g], r
                        sent[g] += 1
                    elif t + 1 < len(c) and c[t + 1][0] == i + 1:
                        left, right, t = r, c[t + 1][1], t + 1
                    elif i + 1 < m[g]:
                        left, right = r, sent[g]
                        sent[g] += 1
                    else:
                        left, right, tail = r, ZERO, 2
                    jobs.append((left, right, (int(l == 0) + tail) | last << 8, g))
                    self.node[row] = (g, l + 1, i >> 1)
                    nxt.append((i >> 1, row))
                    if last:
                        self.top[g] = row
                    row += 1
                    t += 1
                cur[g], m[g] = nxt, (m[g] + 1) >> 1
            self.jobs.append(jobs)
        self.n_work = row
        self.level_off = [0]
        for jobs in self.jobs:
            self.level_off.append(self.level_off[-1] + len(jobs))

    def computed(self):
        return self.level_off[-1]

    def tables(self):
        """(jobs: uint32[computed, 4], level_off: uint64[levels + 1], level_base: uint64[levels]) as the launcher takes them"""
        flat = [j for jobs in self.jobs for j in jobs]
        return (np.array(flat, dtype=np.uint32).reshape(-1, 4), np.array(self.level_off, dtype=np.uint64), np.array(self.level_base, dtype=np.uint64))


def rows_fit(rows, more):
    return rows < ROW_LIMIT and more < ROW_LIMIT - rows


# ---- a verifier over a keyed compression ------------------------------------------------------------------------------------------------------
def canonical(row):
    """a 32-byte row as the canonical bytes of its value mod r"""
    v = int.from_bytes(bytes(bytearray(row)), "little") % R_MOD
    return np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)


def verify(compress, n_blocks, B, leaves, rows, root):
    """(holds, {(level, index): 32 bytes of every computed node}); leaves in the order of sorted B, rows in layout order"""
    p = Plan([(n_blocks, B)])
    if len(rows) != p.n_rows or len(leaves) != p.n:
        return False, {}
    work = [canonical(x) for x in leaves] + [canonical(x) for x in rows]
    nodes = {}
    for l, jobs in enumerate(p.jobs):
        for left, right, kl, _ in jobs:
            work.append(np.array(compress(work[left], work[right] if right != ZERO else np.zeros(32, dtype=np.uint8), kl & 3), dtype=np.uint8))
            _, lv, i = p.node[len(work) - 1]
            nodes[(lv, i)] = work[-1]
    return bool(np.array_equal(work[p.top[0]], canonical(root))), nodes


# ---- the launcher test's cases ----------------------------------------------------------------------------------------------------------------
BLOCKS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 33, 64, 257)
KINDS = ("one", "last", "all", "second", "half")
TOTALS = (1, 63, 64, 65, 255, 256, 257, 4097)       # level-0 job counts


def pick(n_blocks, kind, rng):
    """the set B of one group: one block, the last block (of an odd layer where n is odd), all, every second, a seeded random half"""
    if kind == "one":
        return [int(rng.integers(0, n_blocks))]
    if kind == "last":
        return [n_blocks - 1]
    if kind == "all":
        return list(range(n_blocks))
    if kind == "second":
        return list(range(0, n_blocks, 2))
    return sorted(int(x) for x in rng.choice(n_blocks, size=max(1, n_blocks // 2), replace=False))


class Case:
    def __init__(self, no, groups):
        self.no, self.groups = no, groups


def level0_jobs(n_blocks, B):
    return len({b >> 1 for b in B})


ONE_JOB = ((1, [0]), (2, [0]), (3, [2]), (5, [4]), (2, [1]), (4, [1]), (7, [6]), (9, [8]), (16, [3]), (33, [32]))   # ten groups, one level-0 job each


def cases():
    """Case 0: one job in the whole call.  Case 1: every n of BLOCKS with every kind of B.  One case per level-0 job count of TOTALS above 1:
    the ten one-job groups of ONE_JOB (seven depths), then seeded groups of mixed depths, filled up one job at a time.  Three cases of 40
    small groups of at least three depths, so that one wave holds the jobs of four or more groups.  Every case but the first has at least
    ten groups (the share of wrong stated roots is kept per case)."""
    rng = np.random.default_rng(0x3B1F)
    out = [Case(0, [(1, [0])]),
           Case(1, [(n, pick(n, k, rng)) for n in BLOCKS for k in KINDS])]
    for total in TOTALS[1:]:
        groups, have = list(ONE_JOB), len(ONE_JOB)
        while have < total:
            n = int(rng.choice(BLOCKS))
            B = pick(n, str(rng.choice(KINDS)), rng)
            j = level0_jobs(n, B)
            if have + j > total:
                n, B, j = 2, [0], 1
            groups.append((n, B))
            have += j
        out.append(Case(len(out), groups))
    small = (1, 2, 3, 4, 5, 7, 8, 9)
    for _ in range(3):
        out.append(Case(len(out), [(int(n), pick(int(n), str(rng.choice(KINDS)), rng)) for n in rng.choice(small, size=40)]))
    return out


def wrong_roots(n_groups, rng):
    """{group: how its stated root is wrong} for a case of at least ten groups: max(4, n_groups // 4) groups or one more, the kinds in turn
    (a swap with the next group's makes two wrong), at seeded places"""
    wrong, kinds, k = {}, ("swapped", "low byte", "top limb"), 0
    for g in (int(x) for x in rng.permutation(n_groups)):
        if len(wrong) >= max(4, n_groups // 4):
            break
        if g in wrong:
            continue
        if kinds[k % 3] == "swapped":
            if g + 1 >= n_groups or g + 1 in wrong:
                continue
            wrong[g + 1] = "swapped"
        wrong[g] = kinds[k % 3]
        k += 1
    return wrong


def mixed_wave(p, level, w):
    """wave w of the level's launch holds jobs of >= 4 groups of >= 3 depths, with an odd-tail job, an inner job and a last job among them"""
    jobs = p.jobs[level][w * WAVE:(w + 1) * WAVE]
    gs = {g for _, _, _, g in jobs}
    return (len(gs) >= 4 and len({depth(p.groups[g][0]) for g in gs}) >= 3 and any(r == ZERO for _, r, _, _ in jobs) and
            any(not kl >> 8 for _, _, kl, _ in jobs) and any(kl >> 8 for _, _, kl, _ in jobs))


# ---- the scenario files of tests/host_check/multiproof_plan_check.cpp and the lines it must print ------------------------------------------
def layout_cmd(n_blocks, B):
    return "layout %d %d %s" % (n_blocks, len(B), " ".join(map(str, B)))


def layout_line(n_blocks, B):
    return " ".join(["layout"] + ["%d:%d" % x for x in layout(n_blocks, B)])


def validate_cmd(call, what, groups, blocks, first, n_local, n_blocks, n_rows):
    return "validate %s %s %d %d %d %d %d %s %d %s" % (call, what, first, n_local, n_blocks, -1 if n_rows is None else n_rows, len(groups),
                                                       " ".join("%d %d" % g for g in groups), len(blocks), " ".join(map(str, blocks)))


def validate_line(call, what, groups, blocks, first, n_local, n_blocks, n_rows):
    why = refusal(call, what, groups, blocks, first, n_local, n_blocks, n_rows)
    if why is not None:
        return "refused " + why
    at, rows = 0, 0
    for _, c in groups:
        rows += len(layout(n_blocks, blocks[at:at + c]))
        at += c
    return "ok rows %d" % rows


def plan_cmd(groups):
    return "plan %d %s" % (len(groups), " ".join("%d %d %s" % (n, len(B), " ".join(map(str, B))) for n, B in groups))


def plan_lines(groups):
    p = Plan(groups)
    out = ["plan n %d n_rows %d n_work %d levels %d computed %d" % (p.n, p.n_rows, p.n_work, len(p.jobs), p.computed())]
    for l, jobs in enumerate(p.jobs):
        out.append("level %d base %d jobs %d" % (l, p.level_base[l], len(jobs)))
        out += ["job %d %d %d %d" % j for j in jobs]
    out += ["row %d %d %d %d" % ((r,) + p.node[r]) for r in range(p.n_work)]
    return out


LIMIT_TEXT = "refused multiproof: the rows of this call reach 2^32 - 1"


# ---- what a fill session keeps ----------------------------------------------------------------------------------------------------------------
def node_row(n_blocks, n_local, level, local, index):
    """FillPlan::node_row: the compact layout is layer-major over the local slots"""
    sizes = layer_sizes(n_blocks)
    return n_local * sum(sizes[:level]) + local * sizes[level] + index


def mark_cmd(n_blocks, first, n_local, groups):
    """groups = [(slot, verdict, B)]"""
    return "mark %d %d %d %d %s" % (n_blocks, first, n_local, len(groups), " ".join("%d %d %d %s" % (s, v, len(B), " ".join(map(str, B))) for s, v, B in groups))


def mark_lines(n_blocks, first, n_local, groups):
    """the commit list (every row of the work table, where the compact layout has it) and the known bitmap by the WHOLE-PATH rule: per
    proved block its root, its in-range siblings and its ancestors"""
    p = Plan([(n_blocks, B) for _, _, B in groups])
    out = ["commit %d %d %d" % (r, node_row(n_blocks, n_local, p.node[r][1], groups[p.node[r][0]][0] - first, p.node[r][2]), p.node[r][0]) for r in range(p.n_work)]
    sizes, known = layer_sizes(n_blocks), set()
    for s, v, B in groups:
        if v != 0:
            continue
        for b in B:
            known.add(node_row(n_blocks, n_local, 0, s - first, b))
            for l in range(depth(n_blocks)):
                if (b >> l) ^ 1 < sizes[l]:
                    known.add(node_row(n_blocks, n_local, l, s - first, (b >> l) ^ 1))
                known.add(node_row(n_blocks, n_local, l + 1, s - first, b >> (l + 1)))
    rows = n_local * sum(sizes)
    words = [0] * ((rows + 63) // 64)
    for r in known:
        words[r >> 6] |= 1 << (r & 63)
    return out + [" ".join(["known"] + ["%x" % w for w in words])]
