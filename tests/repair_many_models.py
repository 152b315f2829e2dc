"""A Python model of the host plan behind cp2_datasets_repair_blocks_many (csrc/repair_many_plan.hpp): which calls are refused and with
which words (arguments, then datasets, then the lowest offending request), the chunking (repair_check_with's expression), the descriptor
of every request (want address, block, nBlocks, path row inside its chunk's staged paths, path length), the matched requests grouped by
slot file NAME, which worker of the threaded writer takes which file, and what the call makes of the writer's outcomes.  Seeded random
calls in the text form tests/host_check/repair_many_check.cpp reads, with the lines it must print; validate_brute restates the refusal
rule request by request without any sorting."""
import random

CHECK_ONLY = 1
MATCH, MISMATCH, UNWRITTEN = 0, 1, 2


def depth_of(n_blocks):
    if n_blocks == 0:
        return 0
    d, m = 1, (n_blocks + 1) >> 1
    while m > 1:
        m = (m + 1) >> 1
        d += 1
    return d


class DS:
    """one listed dataset as the plan sees it (ReadDataset)"""

    def __init__(self, kind="ok", cell=128, block=4096, n_cells=256, first_slot=0, n_local=1, mode=2, whole=True, from_file=True, base="/d/a",
                 nodes=0x100000, roots=0x900000, root_off=0, root_size=None, n_layers=None, same_as=0):
        self.kind, self.cell, self.block, self.n_cells, self.first_slot, self.n_local = kind, cell, block, n_cells, first_slot, n_local
        self.mode, self.whole, self.from_file, self.base, self.nodes, self.roots, self.root_off, self.same_as = mode, whole, from_file, base, nodes, roots, root_off, same_as
        self.root_size = (1 if mode == 1 else self.n_blocks) if root_size is None else root_size
        self.n_layers = (self.depth + 1 if mode else 0) if n_layers is None else n_layers

    @property
    def n_blocks(self):
        return self.n_cells // (self.block // self.cell) if self.cell and self.block >= self.cell else 0

    @property
    def depth(self):
        return depth_of(self.n_blocks)

    def line(self):
        return "ds %s %d %d %d %d %d %d %d %d %s %d %d %d %d %d %d" % (
            self.kind, self.cell, self.block, self.n_cells, self.first_slot, self.n_local, self.mode, int(self.whole), int(self.from_file), self.base,
            self.nodes, self.roots, self.root_off, self.root_size, self.n_layers, self.same_as)


class Call:
    def __init__(self, ds, req, path_off=None, flags=0, has=None, n_ds=None, n=None, chunk=4):
        self.ds, self.req, self.path_off, self.flags, self.chunk = ds, [tuple(r) for r in req], path_off, flags, chunk
        self.has = dict(ds=True, req=True, data=True, paths=path_off is not None, path_off=path_off is not None, status=True)
        self.has.update(has or {})
        self.n_ds = len(ds) if n_ds is None else n_ds
        self.n = len(self.req) if n is None else n

    def lines(self):
        h = self.has
        out = ["reset"] + [d.line() for d in self.ds]
        po = self.path_off if self.path_off is not None else []
        out.append("call %d %d %d %d %d %d %d %d %d %d %d %s" % (
            self.flags, h["ds"], h["req"], h["data"], h["paths"], h["path_off"], h["status"], self.n_ds, self.n, self.chunk, len(po),
            " ".join(str(x) for r in self.req for x in r) + (" " if self.req else "") + " ".join(str(x) for x in po)))
        return out


def file_of(ds):
    f = []
    for k, d in enumerate(ds):
        f.append(d.same_as)
        if d.from_file:
            for j in range(k):
                if ds[j].from_file and ds[j].base == d.base:
                    f[k] = j
                    break
    return f


def _args_and_datasets(c):
    h, ds = c.has, c.ds
    if c.flags & ~CHECK_ONLY:
        return "repair many: unknown flag bits 0x%x" % (c.flags & ~CHECK_ONLY)
    if h["paths"] != h["path_off"]:
        return "repair many: paths without path_off" if h["paths"] else "repair many: path_off without paths"
    if c.n == 0:
        return ""
    if not (h["ds"] and h["req"] and h["data"] and h["status"]):
        return "repair many: ds, req, data and status must not be NULL when n > 0"
    if h["path_off"] and c.path_off[0] != 0:
        return "repair many: path_off[0] is %d, not 0" % c.path_off[0]
    for k, d in enumerate(ds):
        who = "repair many: dataset %d: " % k
        if d.kind == "null":
            return who + "NULL dataset"
        if d.kind == "foreign":
            return who + "it belongs to another context"
        if (d.cell, d.block) != (ds[0].cell, ds[0].block):
            return who + "cell_size %d, block_size %d differ from dataset 0's %d, %d" % (d.cell, d.block, ds[0].cell, ds[0].block)
    return None


def _own_rule(c, i):
    """the rule request i breaks on its own, or None"""
    k, s, b = c.req[i]
    who = "repair many: request %d: " % i
    if k >= c.n_ds:
        return who + "dataset index %d is not below n_ds = %d" % (k, c.n_ds)
    d = c.ds[k]
    po = c.path_off if c.has["path_off"] else None
    ln = po[i + 1] - po[i] if po else 0
    if ln < 0:
        return who + "path_off decreases from %d to %d" % (po[i], po[i + 1])
    if ln and ln != d.depth:
        return who + "a path of %d row(s) is neither empty nor the depth %d of dataset %d" % (ln, d.depth, k)
    if not ln and d.mode == 0:
        return who + "an empty path for dataset %d, which keeps only its slot roots, no block roots to check a block against: give the path" % k
    if not ln and (not d.whole or d.n_layers != d.depth + 1):
        return who + "an empty path for dataset %d, whose kept layers are not those of whole slot trees: give the path" % k
    if s < d.first_slot or s - d.first_slot >= d.n_local:
        return who + "slot %d is not inside the local range %d + %d of dataset %d" % (s, d.first_slot, d.n_local, k)
    if b >= d.n_blocks:
        return who + "block %d of slot %d is not below nBlocks = %d of dataset %d" % (b, s, d.n_blocks, k)
    if not d.from_file and not c.flags & CHECK_ONLY:
        return who + "dataset %d has the fake source and no slot files to write: only CP2_REPAIR_CHECK_ONLY is accepted" % k
    return None


def _again(c, i, first):
    k, s, b = c.req[i]
    return "repair many: request %d: (slot %d, block %d) of dataset %d is the block of request %d again" % (i, s, b, k, first)


def validate(c):
    """None: accepted; else the refusal's text.  The plan's own way: the lowest own-rule failure, then the pairs below it by sorting."""
    early = _args_and_datasets(c)
    if early is not None:
        return early or None
    bad, text = c.n, None
    for i in range(c.n):
        text = _own_rule(c, i)
        if text:
            bad = i
            break
    f = file_of(c.ds)
    key = lambda i: (f[c.req[i][0]], c.req[i][1], c.req[i][2])
    order = sorted(range(bad), key=lambda i: (key(i), i))
    twice = bad
    for a, b in zip(order, order[1:]):
        if key(a) == key(b) and b < twice:
            twice = b
    if twice < bad:
        return _again(c, twice, next(i for i in range(twice) if key(i) == key(twice)))
    return text


def validate_brute(c):
    """the same rule request by request: the first request that breaks a rule of its own or names the block of an earlier one"""
    early = _args_and_datasets(c)
    if early is not None:
        return early or None
    for i in range(c.n):
        text = _own_rule(c, i)
        if text:
            return text
        for j in range(i):
            a, b = c.ds[c.req[i][0]], c.ds[c.req[j][0]]
            same_file = (a.from_file and b.from_file and a.base == b.base) or (not a.from_file and not b.from_file and a.same_as == b.same_as)
            if same_file and c.req[i][1:] == c.req[j][1:]:
                return _again(c, i, j)
    return None


def chunk_of(stage_bytes, block, n):
    return max(1, min(n, (stage_bytes // 2) // block))


def kept_addr(d, s, b):
    local = s - d.first_slot
    row = d.root_off + (local * d.n_blocks + b) * d.root_size if d.mode == 1 else d.root_off + local * d.root_size + b
    return d.nodes + row * 32


def table(c):
    """per request (want, blk, n_blocks, path_at, len)"""
    po, chunk, t = (c.path_off if c.has["path_off"] else None), max(1, c.chunk), []
    for i, (k, s, b) in enumerate(c.req):
        d = c.ds[k]
        ln = po[i + 1] - po[i] if po else 0
        want = d.roots + (s - d.first_slot) * 32 if ln else kept_addr(d, s, b)
        t.append((want, b, d.n_blocks, po[i] - po[i // chunk * chunk] if po else 0, ln))
    return t


def most_path_rows(c):
    po, chunk = (c.path_off if c.has["path_off"] else None), max(1, c.chunk)
    return max([po[min(c.n, c0 + chunk)] - po[c0] for c0 in range(0, c.n, chunk)] or [0]) if po else 0


def verdict_pattern(n):
    return [MISMATCH if i % 3 == 1 else MATCH for i in range(n)]


def write_groups(c, status):
    """[(dataset that names the file, slot, name, [requests ascending block])] in (dataset, slot) order"""
    f = file_of(c.ds)
    idx = [i for i in range(c.n) if status[i] == MATCH and c.ds[c.req[i][0]].from_file]
    idx.sort(key=lambda i: (f[c.req[i][0]], c.req[i][1], c.req[i][2]))
    g = []
    for i in idx:
        k, s, _ = c.req[i]
        if not g or (g[-1][0], g[-1][1]) != (f[k], s):
            g.append((f[k], s, "%s%d.dat" % (c.ds[f[k]].base, s), []))
        g[-1][3].append(i)
    return g


def worker_of(threads, count):
    """on_threads' contiguous shares: which worker takes file j"""
    threads = max(1, min(max(threads, 1), count))
    w = [0] * count
    for t in range(threads):
        for j in range(count * t // threads, count * (t + 1) // threads):
            w[j] = t
    return w


def settle(c, groups, failed, status):
    """what the call makes of the writer's outcomes: (first failing group or len(groups), n_written, per dataset the slots whose stamps
    it is offered); status is updated in place"""
    first_bad, n_written, written = len(groups), 0, [[] for _ in c.ds]
    for j, (f, slot, _, reqs) in enumerate(groups):
        if j in failed:
            first_bad = min(first_bad, j)
            for i in reqs:
                status[i] = UNWRITTEN
            continue
        n_written += len(reqs)
        handles = sorted({c.ds[c.req[i][0]].same_as for i in reqs})
        for h in handles:
            for k, d in enumerate(c.ds):
                if d.same_as == h:
                    written[k].append(slot)
    return first_bad, n_written, written


def expected_lines(c):
    """what `plan` prints for one call"""
    why = validate(c)
    if why is not None:
        return ["refused: " + why]
    out = ["accepted n %d most %d" % (c.n, most_path_rows(c))]
    out += ["desc %d %d %d %d %d %d" % ((i,) + t) for i, t in enumerate(table(c))]
    status = verdict_pattern(c.n)
    groups = write_groups(c, status)
    for f, slot, name, reqs in groups:
        out.append("file %d/%d %s: %s" % (f, slot, name, ",".join(map(str, reqs))))
    failed = {j for j in range(len(groups)) if j % 4 == 1}
    first_bad, n_written, written = settle(c, groups, failed, status)
    out.append("settled bad %d written %d status %s" % (first_bad, n_written, " ".join(map(str, status))))
    out += ["stamps %d: %s" % (k, " ".join(map(str, w))) for k, w in enumerate(written)]
    return out


# ---- seeded random calls ------------------------------------------------------------------------------------------------------------------------
GEOMS = (256, 64, 32)   # n_cells at cell 128 / block 4096: 8, 2 and 1 block(s) a slot


def random_datasets(rng):
    """4 to 7 entries: every residency, a fake source, a handle listed twice, two handles over one base name"""
    ds, bases = [], ["/d/a", "/d/b", "/d/c"]
    for k in range(rng.randint(4, 7)):
        mode = rng.choice((0, 1, 2, 2))
        n_local = rng.randint(1, 3)
        d = DS(n_cells=rng.choice(GEOMS), first_slot=rng.randint(0, 2), n_local=n_local, mode=mode, from_file=rng.random() < 0.8,
               base=rng.choice(bases), nodes=0x100000 * (k + 1), roots=0x9000000 + 0x1000 * k, root_off=rng.choice((0, 16, 1000)), same_as=k)
        if k and rng.random() < 0.25:      # the handle of an earlier entry again
            j = rng.randrange(k)
            e = ds[ds[j].same_as]
            d = DS(n_cells=e.n_cells, first_slot=e.first_slot, n_local=e.n_local, mode=e.mode, from_file=e.from_file, base=e.base, nodes=e.nodes,
                   roots=e.roots, root_off=e.root_off, same_as=e.same_as)
        ds.append(d)
    return ds


def random_call(rng, spoil):
    """one call; spoil names what is wrong with it (None: nothing on purpose)"""
    ds = random_datasets(rng)
    flags = CHECK_ONLY if any(not d.from_file for d in ds) and rng.random() < 0.8 else 0
    n = rng.randint(1, 14)
    req, seen, f = [], set(), file_of(ds)
    for _ in range(n):
        for _try in range(50):
            k = rng.randrange(len(ds))
            d = ds[k]
            r = (k, d.first_slot + rng.randrange(d.n_local), rng.randrange(d.n_blocks))
            if (f[k], r[1], r[2]) not in seen and (d.from_file or flags):
                break
        else:
            continue
        seen.add((f[r[0]], r[1], r[2]))
        req.append(r)
    n = len(req)
    with_paths = rng.random() < 0.8
    po = None
    if with_paths:
        po = [0]
        for k, _, _ in req:
            d = ds[k]
            po.append(po[-1] + (d.depth if d.mode == 0 or rng.random() < 0.5 else 0))
    else:
        req = [r for r in req if ds[r[0]].mode != 0]
        n = len(req)
    c = Call(ds, req, po, flags, chunk=rng.choice((1, 3, 4, 100)))
    if not n:
        return c
    i = rng.randrange(n)
    k, s, b = c.req[i]
    if spoil == "flag":
        c.flags |= rng.choice((2, 4, 6))
    elif spoil == "pairing":
        c.has["paths" if rng.random() < 0.5 else "path_off"] ^= True
        if c.path_off is None:
            c.path_off = [0] * (n + 1)
    elif spoil == "null":
        c.has[rng.choice(("ds", "req", "data", "status"))] = False
    elif spoil == "off0" and po:
        c.path_off = [x + 1 for x in po]
    elif spoil == "dataset":
        j = rng.randrange(len(ds))
        what = rng.choice(("null", "foreign", "size"))
        if what == "size" and j:
            ds[j].block = 8192
        else:
            ds[j].kind = "null" if what == "size" else what
    elif spoil == "index":
        c.req[i] = (len(ds) + rng.randint(0, 2), s, b)
    elif spoil == "decrease" and po and po[i] > 0:
        c.path_off = po[:i + 1] + [po[i] - 1] * (n - i)
    elif spoil == "length" and po:
        c.path_off = po[:i + 1] + [x + 1 for x in po[i + 1:]]
    elif spoil == "slot":
        c.req[i] = (k, ds[k].first_slot + ds[k].n_local + rng.randint(0, 1), b)
    elif spoil == "block":
        c.req[i] = (k, s, ds[k].n_blocks + rng.randint(0, 3))
    elif spoil == "layers":
        ds[k].n_layers += 1
    elif spoil == "fake":
        c.flags = 0
    elif spoil == "twice" and n > 1:
        j = rng.randrange(n)
        if j != i:
            twins = [m for m, e in enumerate(ds) if f[m] == f[k] and e.first_slot <= s < e.first_slot + e.n_local and b < e.n_blocks]
            c.req[j] = (rng.choice(twins), s, b)
    return c


SPOILS = (None, None, "flag", "pairing", "null", "off0", "dataset", "index", "decrease", "length", "slot", "block", "layers", "fake", "twice", "twice")


def calls(seed=20251, count=160):
    rng = random.Random(seed)
    return [random_call(rng, SPOILS[i % len(SPOILS)]) for i in range(count)] + fixed_calls()


def fixed_calls():
    """the cases a seeded draw may miss, stated"""
    a = DS(base="/d/a", same_as=0, n_local=2)
    a2 = DS(base="/d/a", same_as=0, n_local=2)                                   # the handle of entry 0 again
    b = DS(base="/d/a", same_as=2, n_local=2, nodes=0x300000, roots=0x9002000)   # another handle over the same base name
    r = DS(base="/d/r", same_as=3, mode=0, n_cells=64, nodes=0, roots=0x9003000)
    fk = DS(base="/d/f", same_as=4, from_file=False, nodes=0x500000, roots=0x9004000)
    fk2 = DS(base="/d/f", same_as=5, from_file=False, nodes=0x600000, roots=0x9005000)
    ds = [a, a2, b, r, fk, fk2]
    out = [
        Call(ds, [], None, 0),                                                                  # n == 0
        Call(ds, [(0, 0, 1), (1, 0, 1)], None, 0),                                              # one handle listed twice
        Call(ds, [(0, 1, 7), (3, 0, 0), (2, 1, 7)], [0, 0, 1, 1], 0),                           # two handles over one base name
        Call(ds, [(4, 0, 3), (5, 0, 3), (4, 0, 3)], None, CHECK_ONLY),                          # fake: the key is the handle
        Call(ds, [(3, 0, 1)], None, 0),                                                         # roots only, no path
        Call(ds, [(3, 0, 1), (0, 0, 0), (2, 1, 3), (1, 1, 0), (3, 0, 0)], [0, 1, 1, 4, 7, 8], 0, chunk=2),   # paths across chunk boundaries
        Call(ds, [(0, 0, 0), (0, 0, 9), (0, 0, 0)], None, 0),                                   # a bad block below a repeat: the block wins
        Call(ds, [(0, 0, 0), (0, 0, 0), (0, 0, 9)], None, 0),                                   # a repeat below a bad block: the repeat wins
        Call(ds, [(0, 0, 0)], None, 0, n_ds=0),
    ]
    return out


# ---- the writer against real files --------------------------------------------------------------------------------------------------------------
EISDIR = 21


def write_case():
    """one call over base names `a` and `b` (the checker puts them under its directory): a handle listed twice, a second handle over `a`,
    files shared between handles, blocks out of order; with the verdict pattern 11 of 16 requests are written"""
    ds = [DS(base="a", n_local=4, same_as=0), DS(base="b", n_local=3, same_as=1, nodes=0x200000), DS(base="a", n_local=4, same_as=2, nodes=0x300000),
          DS(base="a", n_local=4, same_as=0)]
    req = [(0, 0, 5), (1, 1, 0), (2, 0, 2), (0, 1, 7), (1, 0, 3), (3, 2, 1), (2, 3, 0), (1, 2, 6), (0, 2, 0), (3, 0, 0), (1, 1, 4), (2, 1, 1), (0, 3, 7),
           (1, 0, 0), (2, 2, 5), (1, 2, 1)]
    return Call(ds, req, None, 0)


WRITE_DIRS = ("a1.dat", "b1.dat")          # directories where slot files belong: they fail alone
WRITE_PRESENT = {"a0.dat": 8, "a2.dat": 2, "b0.dat": 8, "b2.dat": 8}   # files there before the call, in blocks of 0xEE; a3.dat is missing


def row_byte(i, j):
    return (i * 37 + j * 11 + (j >> 8)) & 0xFF


def expected_write_lines(threads):
    c = write_case()
    status = verdict_pattern(c.n)
    groups = write_groups(c, status)
    failed = {j for j, g in enumerate(groups) if g[2] in WRITE_DIRS}
    out = ["files %d syncs %d" % (len(groups), len(groups) - len(failed)), "workers " + " ".join(map(str, worker_of(threads, len(groups))))]
    out += ["file %s: %d" % (g[2], EISDIR if j in failed else 0) for j, g in enumerate(groups)]
    first_bad, n_written, written = settle(c, groups, failed, status)
    out.append("settled bad %d written %d status %s" % (first_bad, n_written, " ".join(map(str, status))))
    out += ["stamps %d: %s" % (k, " ".join(map(str, w))) for k, w in enumerate(written)]
    return out + ["repair many ok"]


def expected_write_files(block):
    """name -> bytes after the call, for every file that is no directory"""
    c = write_case()
    status = verdict_pattern(c.n)
    files = {name: bytearray(b"\xEE" * (blocks * block)) for name, blocks in WRITE_PRESENT.items()}
    for _, _, name, reqs in write_groups(c, status):
        if name in WRITE_DIRS:
            continue
        img = files.setdefault(name, bytearray())
        for i in reqs:
            off = c.req[i][2] * block
            if len(img) < off + block:
                img.extend(b"\0" * (off + block - len(img)))
            img[off:off + block] = bytes(row_byte(i, j) for j in range(block))
    return files


def scenario(cs):
    return "\n".join(ln for c in cs for ln in c.lines()) + "\n"


def expected_plan_lines(cs):
    return [ln for c in cs for ln in expected_lines(c)]
