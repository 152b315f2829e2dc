"""Plain models of an add whose path stops at a node the session already holds (csrc/fill_plan.hpp: anchor_level, validate_anchored,
mark_proved_anchored; k_block_path_commit_anchored): the lowest known level above a block, the rows a proved anchored request stores, and
the anchored walk.  None of them shares code with the product; the layout comes from tests/fill_nodes_models.py, the walk from
tests/kernel_models.py with the oracle's compression."""
import fill_nodes_models as M
import kernel_models as K

# the kernel's shapes: the one-block slot, powers of two, odd layers at several heights -- over three local slots
ANCHOR_N_BLOCKS = (1, 2, 3, 5, 6, 8, 13)
ANCHOR_N_LOCAL = M.NODE_N_LOCAL


def depth_of(n_blocks):
    return len(K.layer_sizes(n_blocks)) - 1


def anchor_level(n_blocks, n_local, known, local, block, keeping=True):
    """The lowest level in [0, depth] whose node above `block` has its row in `known`; the stated slot root (level depth) always counts."""
    depth = depth_of(n_blocks)
    if not keeping:
        return depth
    for lvl in range(depth):
        if M.node_row(n_blocks, n_local, lvl, local, block >> lvl) in known:
            return lvl
    return depth


def anchor_row(n_blocks, n_local, local, block, level):
    """The row an anchored walk of `level` levels must arrive at; None for the stated slot root."""
    return None if level >= depth_of(n_blocks) else M.node_row(n_blocks, n_local, level, local, block >> level)


def stored_nodes(n_blocks, block, level):
    """[(level, index, what)] of the rows a proved request anchored at `level` stores: the block root, the in-range siblings below the
    level, the ancestors strictly between; nothing at level 0 (the block root is the anchor), never the anchor or anything above it."""
    sizes = K.layer_sizes(n_blocks)
    assert 0 <= level <= len(sizes) - 1
    if level == 0:
        return []
    out = [(0, block, ("root",))]
    for lvl in range(level):
        sib = (block >> lvl) ^ 1
        if sib < sizes[lvl]:
            out.append((lvl, sib, ("sibling", lvl)))
        if lvl + 1 < level:
            out.append((lvl + 1, block >> (lvl + 1), ("ancestor", lvl)))
    return out


def stored_rows(n_blocks, n_local, local, block, level):
    return sorted(M.node_row(n_blocks, n_local, lvl, local, idx) for lvl, idx, _ in stored_nodes(n_blocks, block, level))


def walk(block_root, block, n_blocks, path, compress):
    """The node `block_root` at leaf `block` reaches over the len(path) lowest levels: K.walk_model cut short (its schedule carries the
    index and the layer size from level 0, so a prefix of the path is a prefix of the walk)."""
    return K.walk_model(block_root, block, n_blocks, list(path), compress)


class Session(M.Session):
    """M.Session with anchored adds: add_anchored() is what a keeping session does with a proved anchored request."""

    def anchor(self, local, block):
        return anchor_level(self.n_blocks, self.n_local, self.known, local, block, self.keeping)

    def accepts(self, local, block, level):
        row = anchor_row(self.n_blocks, self.n_local, local, block, level)
        return self.keeping and level <= depth_of(self.n_blocks) and (row is None or row in self.known)

    def add_anchored(self, local, block, level, written=True):
        assert self.accepts(local, block, level)
        self.known.update(stored_rows(self.n_blocks, self.n_local, local, block, level))
        if written:
            self.present.add((local, block))


def fill_with_lowest_anchors(n_blocks, order):
    """Siblings a one-slot session receives when every block of `order` arrives at its lowest anchor."""
    s = Session(n_blocks, 1)
    s.keep_nodes()
    total = 0
    for b in order:
        a = s.anchor(0, b)
        total += a
        s.add_anchored(0, b, a)
    return total, s
