"""A model of the host side of cp2_fills_resume_many (csrc/fills_resume_plan.hpp), restated in plain Python: the order and words of the
argument checks, the short-file drop, the request list over N sessions -- every present block once, in (entry, global index) order --,
the owners the reader looks at, the address table, the seeds and first cells of fake-source requests, the groups of every chunk, the
verdict index turned back into (entry, block), the per-entry drop lists and the cuts of the staged uploads.  The scenario texts feed
tests/host_check/fills_resume_many_check.cpp, whose output tests/test_fills_resume_many_cpu.py compares line by line with
expected_*_lines."""
import errno
import os
from collections import namedtuple

MASK = (1 << 64) - 1
INVALID, IO = -1, -5
TRUST_FILES = 1

Session = namedtuple("Session", "n_blocks first_slot n_local from_file base seed layer0 bits whole")
# bits: the presence bitmap as one int (bit local * n_blocks + block); whole: None, or per local slot the whole blocks its file holds


def seed_stub(seed, slot):
    """what the check program puts in cp2_slot_seed's place"""
    return (seed * 1000003 + slot) & MASK


def words(bits, total):
    return [(bits >> (64 * w)) & MASK for w in range((total + 63) // 64)]


def drop_short(s):
    """fill_ckpt_drop_short: (bits after the drop, the dropped global indices ascending)"""
    if s.whole is None:
        return s.bits, []
    bits, dropped = s.bits, []
    for local, w in enumerate(s.whole):
        for b in range(w, s.n_blocks):
            g = local * s.n_blocks + b
            if bits >> g & 1:
                bits &= ~(1 << g)
                dropped.append(g)
    return bits, dropped


Plan = namedtuple("Plan", "req first g addr same_as fake seeds firsts n_file")


def plan(sessions, cell, block, seed_of=seed_stub):
    cpb = block // cell
    req, first, gs, addr, same_as, fake, seeds, firsts, n_file = [], [0], [], [], [], [], [], [], 0
    for k, s in enumerate(sessions):
        bits, _ = drop_short(s)
        same = k
        if s.from_file:
            for j in range(k):
                if sessions[j].from_file and sessions[j].base == s.base:
                    same = j
                    break
        same_as.append(same)
        for g in range(s.n_local * s.n_blocks):
            if not bits >> g & 1:
                continue
            slot, b = s.first_slot + g // s.n_blocks, g % s.n_blocks
            req.append((k, slot, b))
            gs.append(g)
            addr.append(s.layer0 + g * 32)
            fake.append(0 if s.from_file else 1)
            seeds.append(0 if s.from_file else seed_of(s.seed, slot))
            firsts.append(0 if s.from_file else b * cpb)
            n_file += s.from_file
        first.append(len(gs))
    if not any(fake):
        fake, seeds, firsts = [], [], []
    return Plan(req, first, gs, addr, same_as, fake, seeds, firsts, n_file)


def read_plan(p, sessions, chunk):
    """per chunk: (begin, end, [(owner, slot, [request indices in read order])]) -- read_blocks_plan over the owners"""
    n, chunk = len(p.g), max(1, chunk)
    out = []
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        idx = [i for i in range(c0, c1) if sessions[p.req[i][0]].from_file]
        idx.sort(key=lambda i: (p.same_as[p.req[i][0]], p.req[i][1], p.req[i][2], i))
        groups = []
        for i in idx:
            key = (p.same_as[p.req[i][0]], p.req[i][1])
            if not groups or groups[-1][:2] != key:
                groups.append((key[0], key[1], []))
            groups[-1][2].append(i)
        out.append((c0, c1, groups))
    return out


def where(p, i):
    """(entry, global index) of request i"""
    k = next(j for j in range(len(p.first) - 1) if p.first[j] <= i < p.first[j + 1])
    return k, p.g[i]


def drops(p, verdict):
    return [[p.g[i] for i in range(p.first[k], p.first[k + 1]) if verdict[i]] for k in range(len(p.first) - 1)]


def cuts(sizes, piece):
    out, at = [], 0
    piece = max(piece, 1)
    for s, size in enumerate(sizes):
        off = 0
        while off < size:
            ln = min(size - off, piece - at)
            out.append([s, off, ln, at, False])
            off += ln
            at += ln
            if at == piece:
                out[-1][4] = True
                at = 0
    if out:
        out[-1][4] = True
    return out


# ---- scenario text and what the check program must print -------------------------------------------------------------------------------------
def entry_text(s):
    total = s.n_local * s.n_blocks
    w = words(s.bits, total)
    whole = [] if s.whole is None else list(s.whole)
    return "entry %d %d %d %s %s %d %d %d %s %d %s" % (s.n_blocks, s.first_slot, s.n_local, "file" if s.from_file else "fake", s.base or "-", s.seed,
                                                       s.layer0, len(w), " ".join(map(str, w)), len(whole), " ".join(map(str, whole)))


def plan_scenario(cases):
    """cases: [(sessions, cell, block, [chunk sizes])]"""
    lines = []
    for sessions, cell, block, chunks in cases:
        lines.append("reset")
        lines += [entry_text(s) for s in sessions]
        lines += ["plan %d %d %d" % (cell, block, c) for c in chunks]
    return "\n".join(lines) + "\n"


def verdict_pattern(n):
    return [(1 + i % 2) if i % 3 == 1 else 0 for i in range(n)]


def _list(name, v):
    return (name + " " + " ".join(map(str, v))).rstrip() if v else name


def expected_plan_lines(cases):
    out = []
    for sessions, cell, block, chunks in cases:
        for k, s in enumerate(sessions):
            out.append(("dropped %d: " % k + " ".join(map(str, drop_short(s)[1]))).rstrip())
        p = plan(sessions, cell, block)
        for chunk in chunks:
            out.append("n %d file %d" % (len(p.g), p.n_file))
            out.append(_list("req", [x for r in p.req for x in r]))
            out.append(_list("first", p.first))
            out.append(_list("g", p.g))
            out.append(_list("addr", p.addr))
            out.append(_list("same_as", p.same_as))
            if not p.fake:
                out.append("fake none")
            else:
                out += [_list("fake", p.fake), _list("seeds", p.seeds), _list("firsts", p.firsts)]
            for c, (c0, c1, groups) in enumerate(read_plan(p, sessions, chunk)):
                out.append(("chunk %d [%d,%d): " % (c, c0, c1) + " ".join("%d/%d=%s" % (d, s, ",".join(map(str, idx))) for d, s, idx in groups)).rstrip())
            out.append(_list("where", ["%d:%d" % where(p, i) for i in range(len(p.g))]))
            for k, d in enumerate(drops(p, verdict_pattern(len(p.g)))):
                out.append(("drops %d: " % k + " ".join(map(str, d))).rstrip())
    return out


# ---- the argument checks ------------------------------------------------------------------------------------------------------------------------
Call = namedtuple("Call", "flags cfgs ranges slot_roots paths out entries")      # entries: [(cfg, roots, path, cell, block, begin refuses)]


def entry_prefix(k):
    return "fills: entry %d: " % k


def check_args(c):
    """None, or (index, status, text, how many entries cp2_fill_begin's checks were asked about)"""
    n = len(c.entries)
    if c.flags & ~TRUST_FILES:
        return n, INVALID, "fills: unknown resume flag bits 0x%x" % (c.flags & ~TRUST_FILES), 0
    if n == 0:
        return None
    if not (c.cfgs and c.ranges and c.slot_roots and c.paths and c.out):
        return n, INVALID, "fills: cfgs, ranges, slot_roots, paths and out must not be NULL when n_fills > 0", 0
    asked = 0
    for k, (cfg, roots, path, cell, block, begin) in enumerate(c.entries):
        for there, name in ((cfg, "cfgs"), (roots, "slot_roots"), (path, "paths")):
            if not there:
                return k, INVALID, entry_prefix(k) + "%s[%d] is NULL" % (name, k), asked
        asked += 1
        if begin:
            return k, INVALID, entry_prefix(k) + "fill: stub refusal of %d" % k, asked
        c0, b0 = c.entries[0][3], c.entries[0][4]
        if (cell, block) != (c0, b0):
            return k, INVALID, entry_prefix(k) + ("cell_size %d, block_size %d differ from entry 0's %d, %d: the sessions of one call share the data "
                                                  "path's shape" % (cell, block, c0, b0)), asked
    return None


def call_text(c):
    head = "call %d %d %d %d %d %d %d" % (c.flags, c.cfgs, c.ranges, c.slot_roots, c.paths, c.out, len(c.entries))
    return head + "".join(" %d %d %d %d %d %d" % tuple(int(x) for x in e) for e in c.entries)


def expected_call_line(c):
    r = check_args(c)
    if r is None:
        return "accepted asked %d" % len(c.entries)
    return "refused %d status %d asked %d: %s" % (r[0], r[1], r[3], r[2])


def expected_found_line(statuses):
    for k, st in enumerate(statuses):
        if st:
            return "failed %d status %d: %sfinding of %d" % (k, st, entry_prefix(k), k)
    return "failed none"


DESCRIBES = {
    "none": "describes none: 0 ",
    "n_cells": "describes n_cells: -1 fill: checkpoint /ck/p describes another session: n_cells differs (checkpoint 128, session 64)",
    "first_slot": "describes first_slot: -1 fill: checkpoint /ck/p describes another session: first_slot differs (checkpoint 0, session 1)",
    "source": "describes source: -1 fill: checkpoint /ck/p describes another session: source differs (checkpoint fake, session slot files)",
    "base": "describes base: -1 fill: checkpoint /ck/p describes another session: file base name differs (checkpoint /y/s, session /x/s)",
    "root": "describes root: -1 fill: checkpoint /ck/p describes another session: stated root of slot 2 differs",
}


def expected_read_lines():
    """the read mode's world is fixed in the check program: 28 requests, 26 of them from files, three chunks of 10, 10 and 8"""
    isdir = os.strerror(errno.EISDIR)
    return ["reader ok: 28 rows, 3 chunks, 26 from files", "chunk 0 fails: cannot read a3.dat: " + isdir, "chunk 1 fails: cannot read a3.dat: " + isdir,
            "chunk 2 fails: cannot open a4.dat", "fills resume many ok"]


# ---- the cases the issue names -------------------------------------------------------------------------------------------------------------------
def cases():
    """[(sessions, cell, block, chunk sizes)]: bitmaps empty, full and of one block; 1, 2 and 8 blocks a slot; ranges off slot 0; files too
    short for their present blocks and files that are gone; fake and file entries in turn; two entries over one base; chunks of 1, 3 and
    more than the whole list"""
    full = lambda n: (1 << n) - 1   # noqa: E731
    A, B = "/w/a", "/w/b"
    mixed = [
        Session(8, 3, 2, True, A, 0, 0x100000, 0b1011001110001101, [8, 5]),        # slot 4's file holds 5 of 8 blocks: 13 and 15 go
        Session(2, 0, 3, False, "", 11, 0x200000, 0b110101, None),                  # fake, between two file entries
        Session(8, 4, 1, True, A, 0, 0x300000, full(8), [8]),                       # the same files as entry 0's second slot
        Session(1, 7, 2, True, B, 0, 0x400000, 0b11, [1, 0]),                       # one block a slot; slot 8's file is gone
        Session(2, 5, 1, False, "", 12, 0x500000, 0, None),                         # empty
        Session(8, 0, 3, True, B, 0, 0x600000, 1 << 17, [8, 8, 8]),                 # one block only, in its last slot
    ]
    alone = [Session(2, 9, 1, True, A, 0, 0x700000, 0b10, [2])]
    fakes = [Session(1, 2, 3, False, "", 5, 0x800000, full(3), None), Session(8, 1, 1, False, "", 6, 0x900000, 0b10010001, None)]
    nothing = [Session(8, 0, 1, True, A, 0, 0xA00000, 0, [8]), Session(2, 1, 1, True, A, 0, 0xB00000, full(2), [0])]   # all dropped
    wide = [Session(8, 2, 9, True, B, 0, 0xC00000, full(72) & ~(1 << 64), [8] * 9)]                                    # a second bitmap word
    return [(mixed, 128, 4096, [1, 3, 1000]), (alone, 128, 4096, [1, 3]), (fakes, 64, 512, [3, 100]), (nothing, 128, 4096, [3]),
            (wide, 128, 4096, [1, 3, 71, 72])]


def calls():
    good = (1, 1, 1, 128, 4096, 0)
    return [
        Call(0, 1, 1, 1, 1, 1, [good] * 3),
        Call(1, 1, 1, 1, 1, 1, [good]),
        Call(0, 0, 0, 0, 0, 0, []),
        Call(2, 0, 0, 0, 0, 0, []),                                                  # flag bits before anything else
        Call(6, 1, 1, 1, 1, 1, [good, (0, 1, 1, 0, 0, 0)]),
        Call(0, 0, 1, 1, 1, 1, [good]), Call(0, 1, 0, 1, 1, 1, [good]), Call(0, 1, 1, 0, 1, 1, [good]), Call(0, 1, 1, 1, 0, 1, [good]),
        Call(0, 1, 1, 1, 1, 0, [good]),
        Call(0, 1, 1, 1, 1, 1, [good, (0, 1, 1, 0, 0, 0), (1, 0, 1, 128, 4096, 0)]),  # the lowest index wins
        Call(0, 1, 1, 1, 1, 1, [good, (1, 0, 1, 128, 4096, 0), good]),
        Call(0, 1, 1, 1, 1, 1, [good, good, (1, 1, 0, 128, 4096, 0)]),
        Call(0, 1, 1, 1, 1, 1, [good, (1, 1, 1, 128, 4096, 1), (1, 1, 1, 64, 4096, 0)]),   # begin's refusal of 1 before the shape of 2
        Call(0, 1, 1, 1, 1, 1, [good, (1, 1, 1, 128, 8192, 0), (1, 1, 1, 128, 4096, 1)]),  # the shape of 1 before begin's refusal of 2
        Call(0, 1, 1, 1, 1, 1, [good, (1, 1, 1, 256, 4096, 1)]),                            # on one entry: begin's checks, then the shape
        Call(0, 1, 1, 1, 1, 1, [(1, 1, 1, 64, 512, 0), (1, 1, 1, 64, 512, 0), (1, 1, 1, 128, 512, 0)]),
    ]


FOUND = [[0, 0, 0], [0, IO, INVALID], [0, INVALID, IO], [IO], [0, 0, 0, 0, IO], []]


def args_scenario():
    lines = [call_text(c) for c in calls()] + ["found %d %s" % (len(f), " ".join(map(str, f))) for f in FOUND]
    lines += ["describes " + k for k in DESCRIBES]
    return "\n".join(lines) + "\n"


def expected_args_lines():
    return [expected_call_line(c) for c in calls()] + [expected_found_line(f) for f in FOUND] + [DESCRIBES[k].rstrip() if k != "none" else DESCRIBES[k]
                                                                                                 for k in DESCRIBES]
