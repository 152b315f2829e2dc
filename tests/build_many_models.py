"""Plain references for cp2_datasets_build_many: the scatter kernel behind an address table, the grouping of requests into classes,
items and batches, and where every kept layer lies in a batch and in a request's own buffer.

scatter_model restates what csrc/kernels.hpp documents for k_scatter_rows_addr: row g < rows * n_items is row g % rows of item g / rows
and is copied from source row item * sstride + g % rows to the 32 bytes of "memory" at addr[item] + (g % rows) * 32; address 0 is an item
that keeps nothing.  "Memory" is one flat byte array and an address is an offset into it (never 0 for a real destination), so a case may
put its items anywhere, in any order, with anything between them.  The rest restates csrc/build_many_plan.hpp and what
include/codex_p2.h says of the call; none of it shares code with the product.  tests/test_build_many_cpu.py holds the model against a
plain row loop and the plan against brute force over explicit layouts, and compares the product's plan with this one."""
import collections

import numpy as np


def scatter_model(src, sstride, mem, addr, rows, n_items):
    """`mem` (a flat uint8 array, changed in place and returned) after the scatter; src: uint8[*, 32]"""
    src = np.asarray(src, dtype=np.uint8).reshape(-1, 32)
    addr = np.asarray(addr, dtype=np.int64).reshape(-1)
    total = rows * n_items
    if total == 0:
        return mem
    item, r = np.divmod(np.arange(total, dtype=np.int64), rows)
    live = addr[item] != 0
    item, r = item[live], r[live]
    at = addr[item] + r * 32
    mem[at[:, None] + np.arange(32, dtype=np.int64)[None, :]] = src[item * sstride + r]
    return mem


def scatter_loop(src, sstride, mem, addr, rows, n_items):
    """the same, one row at a time"""
    src = np.asarray(src, dtype=np.uint8).reshape(-1, 32)
    for item in range(n_items):
        if int(addr[item]) == 0:
            continue
        for r in range(rows):
            a = int(addr[item]) + r * 32
            mem[a:a + 32] = src[item * sstride + r]
    return mem


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
Request = collections.namedtuple("Request", "cell_size block_size n_cells first_slot n_local from_file")
Class = collections.namedtuple("Class", "key items batch")    # items: (request index, local slot) in request order
Layer = collections.namedtuple("Layer", "rows src_prefix dst_prefix")


def layer_sizes(n):
    """n, ceil(n / 2), ... 1: the bottom layer is always compressed once (merkle/bn254.nim:29-58)"""
    out, bottom = [], True
    while True:
        out.append(n)
        if n == 1 and not bottom:
            return out
        n, bottom = (n + 1) // 2, False


def kept_layers(cell_size, block_size, n_cells, mode):
    """(layers kept under `mode`, rows of every layer of one item, rows one local slot keeps).  A batch of n items holds layer k at
    row n * src_prefix, item j at + j * rows; a request of n_local slots keeps it at row n_local * dst_prefix, slot s at + s * rows."""
    cpb = block_size // cell_size
    nblocks = n_cells // cpb
    b, t = layer_sizes(cpb), layer_sizes(nblocks)
    layers, src = [], 0
    for k in range(len(b) - 1):
        if mode == 1:
            layers.append(Layer(nblocks * b[k], src, src))
        src += nblocks * b[k]
    dst = src if mode == 1 else 0
    for k in range(len(t)):
        if mode != 0 or k == len(t) - 1:
            layers.append(Layer(t[k], src, 0 if mode == 0 else dst))
        src += t[k]
        dst += t[k]
    return layers, src, sum(x.rows for x in layers)


def batch_items(stage_bytes, item_rows, n_items):
    """half a staging chunk of nodes, at least one item, no more than there are"""
    return max(1, min(n_items, (stage_bytes // 2) // max(1, item_rows * 32)))


def plan(requests, stage_bytes):
    """(file classes in order of first appearance, indices of the fake-source requests)"""
    classes, fake = collections.OrderedDict(), []
    for i, q in enumerate(requests):
        if not q.from_file:
            fake.append(i)
            continue
        classes.setdefault((q.cell_size, q.block_size, q.n_cells), []).extend((i, s) for s in range(q.n_local))
    out = []
    for key, items in classes.items():
        out.append(Class(key, items, batch_items(stage_bytes, kept_layers(key[0], key[1], key[2], 1)[1], len(items))))
    return out, fake


def addr_table(cls, layers, requests, base, i0, n):
    """entry layer * n + j: the address of row 0 of what item i0 + j's request keeps of that layer (base[request] 0: keeps nothing)"""
    out = []
    for lay in layers:
        for j in range(n):
            r, s = cls.items[i0 + j]
            out.append(0 if base[r] == 0 else base[r] + (requests[r].n_local * lay.dst_prefix + s * lay.rows) * 32)
    return out


# ---- explicit layouts (brute force): every row of a buffer as a label --------------------------------------------------------------
def full_layout(cell_size, block_size, n_cells, n_slots):
    """trees_layout's layer-major order as a list of labels: ("b", k, slot, row) for block-tree layer k below the block roots (row counts
    through the slot's blocks), ("t", k, slot, row) for the big tree's layer k"""
    cpb = block_size // cell_size
    nblocks = n_cells // cpb
    b, t = layer_sizes(cpb), layer_sizes(nblocks)
    out = []
    for k in range(len(b) - 1):
        out += [("b", k, s, r) for s in range(n_slots) for r in range(nblocks * b[k])]
    for k in range(len(t)):
        out += [("t", k, s, r) for s in range(n_slots) for r in range(t[k])]
    return out


def kept_layout(cell_size, block_size, n_cells, n_slots, mode):
    """what a dataset of n_slots local slots keeps, as labels in the order of its buffer: every node (trees_layout), the compact layers
    (layer k of slot s at coff[k] + s * csizes[k]) or the roots"""
    full = full_layout(cell_size, block_size, n_cells, n_slots)
    if mode == 1:
        return full
    top = len(layer_sizes(n_cells // (block_size // cell_size))) - 1
    return [x for x in full if x[0] == "t" and (mode == 2 or x[1] == top)]


# ---- the text the stand-alone check reads and prints (tests/host_check/build_many_plan_check.cpp) -----------------------------------
def describe(requests, base, stage_bytes, mode):
    lines = ["stage %d" % stage_bytes, "mode %d" % mode]
    for q, b in zip(requests, base):
        lines.append("R %d %d %d %d %d %d %d" % (q.cell_size, q.block_size, q.n_cells, q.first_slot, q.n_local, int(q.from_file), b))
    return "\n".join(lines) + "\n"


def expected(requests, base, stage_bytes, mode):
    classes, fake = plan(requests, stage_bytes)
    out = ["fake" + "".join(" %d" % i for i in fake)]
    for c, cls in enumerate(classes):
        layers, item_rows, kept_rows = kept_layers(cls.key[0], cls.key[1], cls.key[2], mode)
        out.append("class %d %d %d %d batch %d item_rows %d kept_rows %d" % ((c,) + cls.key + (cls.batch, item_rows, kept_rows)))
        out.append("items" + "".join(" %d:%d" % it for it in cls.items))
        out.append("layers" + "".join(" %d/%d/%d" % lay for lay in layers))
        for k, i0 in enumerate(range(0, len(cls.items), cls.batch)):
            n = min(cls.batch, len(cls.items) - i0)
            out.append("batch %d %d %d src" % (k, i0, n) + "".join(" %d" % (n * lay.src_prefix) for lay in layers))
            out.append("table" + "".join(" %d" % a for a in addr_table(cls, layers, requests, base, i0, n)))
    return "\n".join(out) + "\n"
