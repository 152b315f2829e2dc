"""Plain models of what a serving fill session keeps (csrc/fill_plan.hpp: node_row, mark_proved, derive_from_presence, servable) and of what
k_block_path_commit_nodes stores for a request it proved.  None of them shares code with the product; the layer sizes and the case plans
come from tests/kernel_models.py."""
import kernel_models as K

PROOF_OK, PROOF_ABSENT, PROOF_PARTIAL = 0, 1, 2

# the kernel's shapes: tests/kernel_models.py's walk sizes up to 17 -- every size 1 ... 9 (odd layers at every level, the singleton), 16
# and 17 (a full tree, and one more: an out-of-range sibling at the top levels) -- over three local slots, so that the slot stride is in
# every row
NODE_N_BLOCKS = tuple(n for n in K.WALK_N_BLOCKS if n <= 9 or n in (16, 17))
NODE_N_LOCAL = 3


def layout(n_blocks, n_local):
    """(sizes, offsets, rows) of the compact layout: layer l of local slot s starts at row offsets[l] + s * sizes[l]."""
    sizes = K.layer_sizes(n_blocks)
    offs, rows = [], 0
    for m in sizes:
        offs.append(rows)
        rows += n_local * m
    return sizes, offs, rows


def node_row(n_blocks, n_local, level, local, index):
    sizes, offs, _ = layout(n_blocks, n_local)
    assert index < sizes[level] and local < n_local
    return offs[level] + local * sizes[level] + index


def stored_nodes(n_blocks, block):
    """[(level, index, what)] of the rows a proved request for `block` stores: what = ('root',), ('sibling', l) or ('ancestor', l); a sibling
    whose index lies past its layer has no row."""
    sizes = K.layer_sizes(n_blocks)
    out = [(0, block, ("root",))]
    for lvl in range(len(sizes) - 1):
        sib = (block >> lvl) ^ 1
        if sib < sizes[lvl]:
            out.append((lvl, sib, ("sibling", lvl)))
        out.append((lvl + 1, block >> (lvl + 1), ("ancestor", lvl)))
    return out


def stored_rows(n_blocks, n_local, local, block):
    return sorted(node_row(n_blocks, n_local, lvl, local, idx) for lvl, idx, _ in stored_nodes(n_blocks, block))


def sibling_rows(n_blocks, n_local, local, block):
    """The rows a proof of (local, block) is gathered from, bottom first; None where the path holds zero."""
    sizes = K.layer_sizes(n_blocks)
    return [node_row(n_blocks, n_local, lvl, local, (block >> lvl) ^ 1) if ((block >> lvl) ^ 1) < sizes[lvl] else None
            for lvl in range(len(sizes) - 1)]


class Session:
    """present: set of (local, block); known: set of rows.  add() is what a keeping session does with proved requests."""

    def __init__(self, n_blocks, n_local):
        self.n_blocks, self.n_local = n_blocks, n_local
        self.present, self.known, self.keeping = set(), set(), False

    def add(self, local, block, written=True):
        if self.keeping:
            self.known.update(stored_rows(self.n_blocks, self.n_local, local, block))
        if written:
            self.present.add((local, block))

    def keep_nodes(self):
        if self.keeping:
            return
        self.keeping = True
        sizes = K.layer_sizes(self.n_blocks)
        self.known = {node_row(self.n_blocks, self.n_local, 0, s, b) for s, b in self.present}
        for lvl in range(len(sizes) - 1):
            for s in range(self.n_local):
                for k in range(sizes[lvl + 1]):
                    kids = [c for c in (2 * k, 2 * k + 1) if c < sizes[lvl]]
                    if all(node_row(self.n_blocks, self.n_local, lvl, s, c) in self.known for c in kids):
                        self.known.add(node_row(self.n_blocks, self.n_local, lvl + 1, s, k))

    def servable(self, local, block):
        return (local, block) in self.present and all(r is None or r in self.known for r in sibling_rows(self.n_blocks, self.n_local, local, block))

    def status(self, local, block):
        return PROOF_ABSENT if (local, block) not in self.present else PROOF_OK if self.servable(local, block) else PROOF_PARTIAL
