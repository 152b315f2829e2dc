"""Plain models of cp2_fill_adopt's judgement (csrc/adopt_plan.hpp; k_adopt_layer, k_adopt_resolve): the tree over candidate block roots
with the session's known nodes wherever it has them, and which rows that proves.  They share no code with the product.  Values are opaque:
the GPU unit test hands in 32-byte rows and the oracle's compression, the ABI test hands in names and a compression that builds tuples
(injective by construction), which is all the rule needs to say WHICH blocks are adopted.  The layout comes from tests/fill_nodes_models.py."""
import fill_anchor_models as A
import fill_nodes_models as M
import kernel_models as K

KNOWN, CAND, MATCH, PROVED, ADOPTED = 1, 2, 4, 8, 16

# the kernels' shapes: the one-block slot, powers of two, and 5 (odd layers at two heights)
ADOPT_N_BLOCKS = (1, 2, 5, 8, 64)


def depth_of(n_blocks):
    return len(K.layer_sizes(n_blocks)) - 1


def same(a, b):
    """opaque values compare by their bytes where they have any"""
    return bytes(a) == bytes(b) if hasattr(a, "tobytes") else a == b


def layers(n_blocks, n_local, slots, tree, cand, flags, roots, compress, zero):
    """k_adopt_layer over every layer for the local slots in `slots`: tree / cand are per-row lists, flags a per-row list of ints, roots one
    value per local slot.  Returns (cand, flags) after the last layer; the inputs are not changed."""
    sizes, offs, _ = M.layout(n_blocks, n_local)
    cand, flags = list(cand), list(flags)
    for lvl in range(len(sizes) - 1):
        for s in slots:
            for j in range(sizes[lvl + 1]):
                rl, rp = offs[lvl] + s * sizes[lvl] + 2 * j, offs[lvl + 1] + s * sizes[lvl + 1] + j
                pair = 2 * j + 1 < sizes[lvl]
                fl, fr = flags[rl], flags[rl + 1] if pair else KNOWN
                known = flags[rp] & KNOWN
                flags[rp] = known
                if not (fl & (KNOWN | CAND)) or not (fr & (KNOWN | CAND)):
                    continue
                left = tree[rl] if fl & KNOWN else cand[rl]
                right = zero if not pair else tree[rl + 1] if fr & KNOWN else cand[rl + 1]
                v = compress(left, right, (1 if lvl == 0 else 0) + (0 if pair else 2))
                cand[rp] = v
                flags[rp] = known | CAND
                if known and same(v, roots[s] if lvl + 1 == len(sizes) - 1 else tree[rp]):
                    flags[rp] |= MATCH
    return cand, flags


def resolve(n_blocks, n_local, slots, tree, cand, flags):
    """k_adopt_resolve: (out bytes per row -- 0 outside the selected slots and on the top rows --, the tree after the proved rows were copied)"""
    sizes, offs, rows = M.layout(n_blocks, n_local)
    depth = len(sizes) - 1
    out, tree = [0] * rows, list(tree)
    for lvl in range(depth):
        for s in slots:
            for k in range(sizes[lvl]):
                r = offs[lvl] + s * sizes[lvl] + k
                f = flags[r] & (KNOWN | CAND | MATCH)
                if not f & CAND:
                    out[r] = f
                    continue
                if f & KNOWN:
                    if lvl == 0:
                        f = (f & ~MATCH) | ((MATCH | ADOPTED) if same(cand[r], tree[r]) else 0)
                    out[r] = f
                    continue
                proved, idx = False, k
                for up in range(lvl + 1, depth + 1):
                    idx >>= 1
                    fa = flags[offs[up] + s * sizes[up] + idx]
                    if not fa & CAND:
                        break
                    if fa & KNOWN:
                        proved = bool(fa & MATCH)
                        break
                if proved:
                    tree[r] = cand[r]
                    f |= PROVED | (ADOPTED if lvl == 0 else 0)
                out[r] = f
    return out, tree


class Slot:
    """One slot of a keeping session by names: which rows are known, which blocks present, and what an adopt over candidate blocks does.
    `damaged` blocks hold bytes that hash to another root."""

    def __init__(self, n_blocks):
        self.n_blocks = n_blocks
        self.sizes, self.offs, self.rows = M.layout(n_blocks, 1)
        self.depth = len(self.sizes) - 1
        self.truth = [None] * self.rows
        for b in range(n_blocks):
            self.truth[b] = ("leaf", b)
        for lvl in range(self.depth):
            for j in range(self.sizes[lvl + 1]):
                pair = 2 * j + 1 < self.sizes[lvl]
                kids = self.truth[self.offs[lvl] + 2 * j], self.truth[self.offs[lvl] + 2 * j + 1] if pair else 0
                self.truth[self.offs[lvl + 1] + j] = (kids[0], kids[1], (1 if lvl == 0 else 0) + (0 if pair else 2))
        self.known, self.present = set(), set()

    def add_path(self, block, level=None):
        """a proved add of `block` at `level` (default: its whole path); returns the siblings it brought"""
        level = self.depth if level is None else level
        self.known.update(M.stored_rows(self.n_blocks, 1, 0, block) if level == self.depth else A.stored_rows(self.n_blocks, 1, 0, block, level))
        self.present.add(block)
        return level

    def anchor(self, block):
        for lvl in range(self.depth):
            if self.offs[lvl] + (block >> lvl) in self.known:
                return lvl
        return self.depth

    def adopt(self, candidates, damaged=()):
        """the blocks an adopt over `candidates` (absent ones only) makes present; known and present are updated"""
        flags = [KNOWN if r in self.known else 0 for r in range(self.rows)]
        flags[self.rows - 1] |= KNOWN
        cand = [None] * self.rows
        for b in candidates:
            if b not in self.present:
                flags[b] |= CAND
                cand[b] = ("damaged", b) if b in damaged else self.truth[b]
        cand, flags = layers(self.n_blocks, 1, [0], self.truth, cand, flags, [self.truth[-1]], lambda x, y, key: (x, y, key), 0)
        out, _ = resolve(self.n_blocks, 1, [0], self.truth, cand, flags)
        self.known.update(r for r in range(self.rows) if out[r] & PROVED)
        got = [b for b in range(self.n_blocks) if out[b] & ADOPTED]
        self.present.update(got)
        return got
