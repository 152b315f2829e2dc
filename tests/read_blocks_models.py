"""A Python model of the host plan behind cp2_datasets_read_blocks (csrc/read_blocks_plan.hpp): which calls are refused and with which
index, the order a chunk's blocks are read in, the chunks, the packed path offsets and the two device address tables (kept block roots,
path rows) for the every-node and the compact layouts.  Pure arithmetic, restated from the header's and the issue's words, not
translated from the C++: tests/test_read_blocks_cpu.py holds the C++ against it."""
from dataclasses import dataclass, field

CHECK_ONLY = 1


def layer_sizes(n):
    """element counts of all layers of a tree over n leaves, bottom first: the bottom layer is always compressed once"""
    s, m, bottom = [], n, True
    while True:
        s.append(m)
        if m == 1 and not bottom:
            return s
        m, bottom = (m + 1) // 2, False


def proof_depth(n_blocks):
    return len(layer_sizes(n_blocks)) - 1 if n_blocks else 0


@dataclass
class Dataset:
    cell_size: int = 128
    block_size: int = 4096
    n_cells: int = 256
    first_slot: int = 0
    n_local: int = 1
    mode: int = 2                 # 1 every node kept, 2 compact, 0 roots only
    whole: bool = True
    from_file: bool = True
    base: str = "-"
    seed: int = 0
    nodes: int = 0                # device address of the kept node buffer
    null: bool = False
    foreign: bool = False
    same_as: int = 0
    root_off: int = 0
    root_size: int = 0
    offs: list = field(default_factory=list)
    sizes: list = field(default_factory=list)

    @property
    def n_blocks(self):
        return self.n_cells // (self.block_size // self.cell_size)

    @property
    def depth(self):
        return proof_depth(self.n_blocks)

    def layout(self):
        """the kept layers as the builders lay them out, layer-major over the local slots"""
        nb, cpb = self.n_blocks, self.block_size // self.cell_size
        tsizes = layer_sizes(nb)
        if self.mode == 2:                      # compact: the big tree's layers from row 0
            off, offs = 0, []
            for m in tsizes:
                offs.append(off)
                off += self.n_local * m
            self.offs, self.sizes, self.root_off, self.root_size = offs, tsizes, offs[0], tsizes[0]
        elif self.mode == 1:                    # every node: the block trees' layers, whose last layer is layer 0 of the big trees
            bsizes = layer_sizes(cpb)
            off, boff = 0, []
            for m in bsizes:
                boff.append(off)
                off += self.n_local * nb * m
            offs = [boff[-1]]
            for m in tsizes[1:]:
                offs.append(off)
                off += self.n_local * m
            self.offs, self.sizes, self.root_off, self.root_size = offs, tsizes, boff[-1], bsizes[-1]
        return self


def refusal(ds, req, flags=0, have=("ds", "req", "data", "status")):
    """None, or (kind, index) of the first rule a call breaks: arguments, then datasets in order, then requests in order"""
    have, n = set(have), len(req)
    if flags & ~CHECK_ONLY:
        return ("flag", None)
    if ("paths" in have) != ("path_off" in have):
        return ("paths", None)
    if n == 0:
        return None
    if not {"ds", "req", "status"} <= have:
        return ("null", None)
    if "data" not in have and not flags & CHECK_ONLY:
        return ("data", None)
    for k, d in enumerate(ds):
        if d.null:
            return ("dataset null", k)
        if d.foreign:
            return ("dataset foreign", k)
        if (d.cell_size, d.block_size) != (ds[0].cell_size, ds[0].block_size):
            return ("dataset sizes", k)
        if d.mode == 0:
            return ("dataset roots-only", k)
        if not d.whole or len(d.offs) != d.depth + 1 or len(d.sizes) != d.depth + 1:
            return ("dataset layers", k)
    for i, (k, s, b) in enumerate(req):
        if k >= len(ds):
            return ("request dataset", i)
        d = ds[k]
        if not d.first_slot <= s < d.first_slot + d.n_local:
            return ("request slot", i)
        if b >= d.n_blocks:
            return ("request block", i)
    return None


REFUSAL_WORDS = {"flag": "unknown flag", "paths": "path_off", "null": "must not be NULL", "data": "data is NULL", "dataset null": "NULL dataset",
                 "dataset foreign": "another context", "dataset sizes": "differ from dataset 0", "dataset roots-only": "keeps only its slot roots",
                 "dataset layers": "not those of whole slot trees", "request dataset": "is not below n_ds", "request slot": "local range",
                 "request block": "is not below nBlocks"}


def chunk_size(stage_bytes, block_size, n):
    return max(1, min(n, (stage_bytes // 2) // block_size))


def read_plan(ds, req, chunk):
    """per chunk, the list of (file dataset, slot, [request indices in reading order]): files ascending, offsets ascending inside a file, a
    repeat after the request it repeats; fake-source requests are read by nobody"""
    out = []
    for c0 in range(0, len(req), chunk):
        idx = [i for i in range(c0, min(len(req), c0 + chunk)) if ds[req[i][0]].from_file]
        idx.sort(key=lambda i: (ds[req[i][0]].same_as, req[i][1], req[i][2], i))
        groups = []
        for i in idx:
            key = (ds[req[i][0]].same_as, req[i][1])
            if not groups or groups[-1][:2] != key:
                groups.append(key + ([],))
            groups[-1][2].append(i)
        out.append(groups)
    return out


def path_off(ds, req):
    off = [0]
    for k, _, _ in req:
        off.append(off[-1] + ds[k].depth)
    return off


def addr_table(ds, req):
    """one kept-root address per request, then one per path row (0: the ZERO sibling)"""
    kept, rows = [], []
    for k, s, b in req:
        d = ds[k]
        local = s - d.first_slot
        if d.mode == 1:
            kept.append(d.nodes + 32 * (d.root_off + (local * d.n_blocks + b) * d.root_size))
        else:
            kept.append(d.nodes + 32 * (d.root_off + local * d.root_size + b))
        for l in range(d.depth):
            sib = (b >> l) ^ 1
            rows.append(d.nodes + 32 * (d.offs[l] + local * d.sizes[l] + sib) if sib < d.sizes[l] else 0)
    return kept + rows


def describe(ds, req, chunk, flags=0, have=("ds", "req", "data", "status")):
    """the text tests/host_check/read_blocks_check.cpp reads"""
    have = set(have)
    lines = ["args %d %d %d %d %d %d %d %d" % tuple([int(x in have) for x in ("ds", "req", "data", "paths", "path_off", "status")] + [len(ds), flags])]
    for d in ds:
        lines.append("D %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s %d %s" % (
            d.null, d.foreign, d.same_as, d.cell_size, d.block_size, d.n_cells, d.first_slot, d.n_local, d.mode, d.whole, d.from_file, d.seed, d.nodes,
            d.root_off, d.root_size, d.base, len(d.offs), " ".join(str(x) for x in list(d.offs) + list(d.sizes))))
    lines.append("chunk %d" % chunk)
    lines.extend("R %d %d %d" % tuple(r) for r in req)
    return "\n".join(lines) + "\n"
