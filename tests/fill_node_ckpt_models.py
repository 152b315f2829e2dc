"""Plain models of a fill checkpoint with nodes (csrc/node_ckpt_plan.hpp; cp2_fill_save_nodes / cp2_fill_resume_nodes; k_nodes_restore_layer):
the documented layout of a CP2FILL2 file read and written without the library (the checksum is fill_resume_models.checksum64), a plain
top-down restore over opaque values, and the session model of tests/fill_session_model.py extended with the two operations and a seeded
generator that proposes them among the others.  Nothing here shares code with the product."""
import random
import struct

import numpy as np

import fill_anchor_models as A
import fill_nodes_models as M
import fill_resume_models as R
import fill_session_model as S

MAGIC2 = b"CP2FILL2"
KNOWN, CAND, RESTORED, REJECTED = 1, 2, 4, 8


# ---- the file ---------------------------------------------------------------------------------------------------------------------------
def parse_checkpoint2(raw):
    """The fields of a CP2FILL2 file as a dict: fill_resume_models.parse_checkpoint's fields (layer0 as the file states it), `known` (0 / 1 per
    row of the compact layout) and `mid` ({row: uint8[32]} of the known rows between layer 0 and the top).  Asserts magic, sizes, padding,
    the packed count and the checksum."""
    assert raw[:8] == MAGIC2
    c = dict(zip(R.WORDS, struct.unpack_from("<10Q", raw, 8)))
    total = c["n_local"] * c["n_blocks"]
    assert c["n_blocks"] == c["n_cells"] // (c["block_size"] // c["cell_size"])
    sizes, offs, rows = M.layout(c["n_blocks"], c["n_local"])
    at = 88
    c["file_base"] = raw[at:at + c["file_base_len"]]
    pad = (c["file_base_len"] + 7) // 8 * 8
    assert raw[at + c["file_base_len"]:at + pad] == bytes(pad - c["file_base_len"])
    at += pad
    c["roots"] = np.frombuffer(raw, dtype=np.uint8, count=c["n_local"] * 32, offset=at).reshape(-1, 32).copy()
    at += c["n_local"] * 32
    words = (total + 63) // 64
    bitmap = struct.unpack_from("<%dQ" % words, raw, at)
    at += words * 8
    c["bits"] = [(bitmap[g >> 6] >> (g & 63)) & 1 for g in range(total)]
    assert all(bitmap[g >> 6] >> (g & 63) & 1 == 0 for g in range(total, words * 64))
    kwords = (rows + 63) // 64
    kmap = struct.unpack_from("<%dQ" % kwords, raw, at)
    at += kwords * 8
    c["known"] = [(kmap[r >> 6] >> (r & 63)) & 1 for r in range(rows)]
    assert all(kmap[r >> 6] >> (r & 63) & 1 == 0 for r in range(rows, kwords * 64))
    c["layer0"] = np.frombuffer(raw, dtype=np.uint8, count=total * 32, offset=at).reshape(-1, 32).copy()
    at += total * 32
    for g in range(total):
        assert c["bits"][g] or c["known"][g] or not c["layer0"][g].any(), ("a row that is neither present nor known is not zero", g)
    c["mid"] = {}
    for r in range(total, offs[-1]):
        if c["known"][r]:
            c["mid"][r] = np.frombuffer(raw, dtype=np.uint8, count=32, offset=at).copy()
            at += 32
    assert len(raw) == at + 8 and struct.unpack_from("<Q", raw, at)[0] == R.checksum64(raw[:at])
    return c


def write_checkpoint2(c, known_pad=0, extra_rows=0):
    """The bytes of a CP2FILL2 file with the fields of `c` (as parse_checkpoint2 returns them), by the documented layout, checksum valid.
    known_pad: bits set past the last row; extra_rows: packed rows the bitmap does not state (negative: rows left out) -- corrupt files
    with a valid checksum."""
    total = c["n_local"] * c["n_blocks"]
    sizes, offs, rows = M.layout(c["n_blocks"], c["n_local"])
    base = bytes(c["file_base"])
    out = bytearray(MAGIC2)
    out += struct.pack("<10Q", *[len(base) if w == "file_base_len" else c[w] for w in R.WORDS])
    out += base + bytes((len(base) + 7) // 8 * 8 - len(base))
    out += np.ascontiguousarray(c["roots"], dtype=np.uint8).tobytes()

    def bitmap(bits, n, pad=0):
        words = [0] * ((n + 63) // 64)
        for g, b in enumerate(bits):
            if b:
                words[g >> 6] |= 1 << (g & 63)
        for g in range(n, min(n + pad, len(words) * 64)):
            words[g >> 6] |= 1 << (g & 63)
        return struct.pack("<%dQ" % len(words), *words)

    out += bitmap(c["bits"], total)
    out += bitmap(c["known"], rows, known_pad)
    out += np.ascontiguousarray(c["layer0"], dtype=np.uint8).tobytes()
    packed = [np.asarray(c["mid"][r], dtype=np.uint8).tobytes() for r in range(total, offs[-1]) if c["known"][r]]
    packed = packed[:len(packed) + extra_rows] if extra_rows < 0 else packed + [bytes(32)] * extra_rows
    out += b"".join(packed)
    out += struct.pack("<Q", R.checksum64(bytes(out)))
    return bytes(out)


# ---- k_nodes_restore_layer -----------------------------------------------------------------------------------------------------------------
def same(a, b):
    return bytes(a) == bytes(b) if hasattr(a, "tobytes") else a == b


def restore_layer(tree, cand, flags, roots, off_in, m_in, off_out, n_local, bottom, top, n_rows, compress, zero):
    """one launch: per parent of every slot; tree / cand / flags are per-row lists changed in place"""
    m_out = (m_in + 1) // 2
    for s in range(n_local):
        for j in range(m_out):
            rl, rp = off_in + s * m_in + 2 * j, off_out + s * m_out + j
            pair = 2 * j + 1 < m_in
            rr = rl + (1 if pair else 0)
            if rr >= n_rows or rp >= n_rows:
                continue
            if not flags[rp] & (KNOWN | RESTORED):
                continue
            fl, fr = flags[rl], flags[rr] if pair else KNOWN
            if not fl & (KNOWN | CAND) or not fr & (KNOWN | CAND) or not (fl | fr) & CAND:
                continue
            left = tree[rl] if fl & KNOWN else cand[rl]
            right = zero if not pair else tree[rr] if fr & KNOWN else cand[rr]
            v = compress(left, right, (1 if bottom else 0) + (0 if pair else 2))
            ok = same(v, roots[s] if top else tree[rp])
            for r, f in ((rl, fl), (rr, fr if pair else 0)):
                if f & CAND:
                    if ok:
                        tree[r] = cand[r]
                    flags[r] = RESTORED if ok else REJECTED


def restore(n_blocks, n_local, tree, cand, flags, roots, compress, zero, n_rows=None):
    """every layer, top first; returns (tree, flags), the inputs are not changed"""
    sizes, offs, rows = M.layout(n_blocks, n_local)
    tree, flags = list(tree), list(flags)
    depth = len(sizes) - 1
    for lvl in range(depth - 1, -1, -1):
        restore_layer(tree, cand, flags, roots, offs[lvl], sizes[lvl], offs[lvl + 1], n_local, lvl == 0, lvl + 1 == depth,
                      rows if n_rows is None else n_rows, compress, zero)
    return tree, flags


def restore_known(n_blocks, n_local, derived, saved, value_of, truth, roots):
    """What a resume makes of the saved rows: (known', restored, rejected, unproved) as sets of rows.  derived: D; saved: the file's known
    rows; value_of(r): the value the file states for row r; truth: the true node per row (names); the compression builds tuples."""
    sizes, offs, rows = M.layout(n_blocks, n_local)
    top = offs[-1]
    flags = [KNOWN if (r in derived or r >= top) else CAND if r in saved else 0 for r in range(rows)]
    cand = [value_of(r) if flags[r] == CAND else None for r in range(rows)]
    _, down = restore(n_blocks, n_local, truth, cand, flags, roots, lambda x, y, key: (x, y, key), 0)
    pick = lambda st: {r for r in range(top) if flags[r] == CAND and down[r] == st}    # noqa: E731
    restored, rejected, unproved = pick(RESTORED), pick(REJECTED), pick(CAND)
    return set(derived) | restored | {r for r in saved if r >= top}, restored, rejected, unproved


# ---- the session ----------------------------------------------------------------------------------------------------------------------------
class NodeSessionModel(S.SessionModel):
    """fill_session_model.SessionModel with two more operations:
      ["save_nodes"]                       cp2_fill_save_nodes to a file of its own, beside the one ["save"] writes
      ["resume_nodes", trust, which]       cp2_fill_free, then cp2_fill_resume_nodes of that file (which = "nodes") or of the CP2FILL1 file
                                           (which = "plain"): the result of the latter is ["resume", trust] followed by ["keep"]"""

    def __init__(self, shape, files=True):
        super().__init__(shape, files)
        self.nckpt = None                                 # (present, known) of the last save_nodes
        self.anchored_rows = set()                        # rows an anchored add made known in this session

    def op_anchored(self, reqs, fail_slot=None):
        before = set(self.known)
        res = super().op_anchored(reqs, fail_slot)
        self.anchored_rows |= set(self.known) - before
        return res

    def kinds_of_known_rows(self):
        """which kinds of known rows a save taken now would hold"""
        top = self.offs[-1]
        kinds = set()
        for s, b in [(self.local(p[0]), p[1]) for p in self.missing()]:
            for lvl in range(self.depth):
                sib = (b >> lvl) ^ 1
                if sib < self.sizes[lvl] and self.row(lvl, s, sib) in self.known:
                    kinds.add("sibling_of_absent")
        if self.anchored_rows & self.known:
            kinds.add("anchored")
        if any(self.proved_by.get(r) == "adopt" for r in self.known):
            kinds.add("adopt")
        for lvl in range(1, self.depth):
            for s in range(self.n_local):
                for k in range(self.sizes[lvl]):
                    r = self.row(lvl, s, k)
                    if r in self.known and self.proved_by.get(r) == "keep" and r < top and self.row(lvl + 1, s, k >> 1) not in self.known:
                        kinds.add("frontier")
        return kinds

    def op_save_nodes(self):
        if self.finished or not self.keeping:
            return {"err": S.ERR_INVALID}
        self.nckpt = (frozenset(self.present), frozenset(self.known))
        return {"err": S.OK}

    def checkpoint_known(self):
        return [1 if r in self.known else 0 for r in range(self.rows)]

    def op_resume_nodes(self, trust, which):
        if which == "plain":
            res = self.op_resume(trust)
            self.op_keep()
            self.anchored_rows = set()
            return dict(res, n_restored=0, n_unproved=0, n_rejected=0)
        assert self.nckpt is not None and not self.finished
        saved_present, saved_known = self.nckpt
        dropped = set()
        if not trust and self.files:
            dropped = {(s, b) for s, b in saved_present if not self.covered(s, b) or self.disk[s][b] != "T"}
        self.node = A.Session(self.nb, self.n_local)
        self.node.present = set(saved_present) - dropped
        self.resumed, self.remember, self.stale = True, {}, set()
        self.partial_seen, self.unwritten, self.known_grew, self.anchored_rows = set(), set(), False, set()
        self.node.keep_nodes()
        derived = set(self.node.known)
        roots = [self.truth[self.row(self.depth, s, 0)] for s in range(self.n_local)]
        known, restored, rejected, unproved = restore_known(self.nb, self.n_local, derived, saved_known, lambda r: self.truth[r], self.truth, roots)
        self.node.known = known
        self.proved_by = {r: "keep" for r in derived}
        self.proved_by.update({r: "restore" for r in known - derived})
        if not trust:
            self.cov["resume_drops" if dropped else "resume_drops_none"] += 1
        self.cov["nodes_restored"] += len(restored)
        self.cov["nodes_unproved"] += len(unproved)
        return {"err": S.OK, "n_dropped": len(dropped), "n_restored": len(restored), "n_unproved": len(unproved), "n_rejected": len(rejected)}


OP_KINDS = S.OP_KINDS + ("save_nodes", "resume_nodes")


def _propose(rng, m, files):
    w = S._weights(m, files)
    mine = {"save_nodes": 3 if m.keeping else 0.3, "resume_nodes": 3 if m.nckpt is not None else 1 if m.ckpt is not None else 0}
    x = rng.random() * (sum(w.values()) + sum(mine.values()))
    if x < mine["save_nodes"]:
        return ["save_nodes"]
    if x < mine["save_nodes"] + mine["resume_nodes"]:
        which = "nodes" if m.nckpt is not None and (m.ckpt is None or rng.random() < 0.8) else "plain"
        return ["resume_nodes", rng.random() < 0.3, which]
    return S._propose(rng, m, files)


def sequence(seed, shape, n_steps, files=True):
    """fill_session_model.sequence with the two operations among the others; the same arguments give the same list"""
    rng = random.Random("fill node checkpoints %d %r %d %d" % (seed, tuple(shape), n_steps, files))
    m = NodeSessionModel(shape, files)
    ops = []
    for _ in range(n_steps):
        op = _propose(rng, m, files)
        m.apply(op)
        ops.append(op)
    return ops + S._tail(m)
