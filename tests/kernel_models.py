"""Plain references, and the case plans, for the kernels that tests/test_gpu_kernel_units.py runs one launcher at a time.

The models restate in Python and numpy what csrc/kernels.hpp documents for k_scrub_compare, k_sample_paths, k_sample_many and the two
block-path kernels; none of them shares code with the product.  tests/test_kernel_models_cpu.py holds them against
oracle/poseidon2_ref.py on small trees and checks that every edge the GPU module claims is really in its plan; the plans are plain
functions, so that check needs no GPU."""
import collections

import numpy as np

SCRUB_TILE = 4096          # asserted against the library (ku_scrub_tile) by the GPU module
MAX_LAYERS = 40
PAD_ROW = (1 << 64) - 1
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617


# ---- scrub -----------------------------------------------------------------------------------------------------------------------
def scrub_groups(total):
    return (total + SCRUB_TILE - 1) // SCRUB_TILE


def scrub_model(fresh, kept, rows, fstride, kstride, n_items):
    """(bits, counts): bit g % 64 of bits[g / 64] is set where row g % rows of item g / rows differs between the two sides; the words
    run to the end of the last tile; counts[w] = set bits of tile w."""
    fresh = np.asarray(fresh, dtype=np.uint8).reshape(-1, 32)
    kept = np.asarray(kept, dtype=np.uint8).reshape(-1, 32)
    total = rows * n_items
    item, r = np.divmod(np.arange(total, dtype=np.int64), rows)
    flags = np.zeros(scrub_groups(total) * SCRUB_TILE, dtype=bool)
    flags[:total] = (fresh[item * fstride + r] != kept[item * kstride + r]).any(axis=1)
    bits = np.packbits(flags.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)
    counts = flags.reshape(-1, SCRUB_TILE).sum(axis=1).astype(np.uint32)
    return bits, counts


# ---- tree layout and sampled paths -------------------------------------------------------------------------------------------------
Geom = collections.namedtuple("Geom", "nb nt cpb nblocks n_cells n_slots boff bsz toff tsz total_rows")


def layer_sizes(n):
    """Sizes of the layers of a tree over n leaves, leaves first; one leaf still gets one compression (two layers)."""
    out = [n]
    while len(out) < 2 or out[-1] > 1:
        out.append((out[-1] + 1) // 2)
    return out


def tree_geom(cpb, nblocks, n_cells, n_slots):
    """The layer-major layout documented at TreeGeom: every block-tree layer below the block roots in turn (layer k of block b of slot
    s at boff[k] + (s * nblocks + b) * bsz[k]), then every layer of the slots' big trees (layer k of slot s at toff[k] + s * tsz[k]);
    the block roots are layer 0 of the big trees, the slot roots the last."""
    bsz, tsz = layer_sizes(cpb), layer_sizes(nblocks)
    assert len(bsz) <= MAX_LAYERS and len(tsz) <= MAX_LAYERS
    off, boff, toff = 0, [], []
    for k, m in enumerate(bsz):
        boff.append(off)
        if k + 1 < len(bsz):
            off += n_slots * nblocks * m
    for m in tsz:
        toff.append(off)
        off += n_slots * m
    return Geom(len(bsz), len(tsz), cpb, nblocks, n_cells, n_slots, boff, bsz, toff, tsz, off)


def path_depth(geom):
    return geom.nb - 1 + geom.nt - 1


def path_rows_model(geom, slot, cell, md):
    """Row of each sibling on the merged path of `cell` of `slot`, bottom first, cut or padded with ~0 to md entries; ~0 also where
    the sibling lies past the end of its layer."""
    block, j = divmod(cell, geom.cpb)
    rows = []
    for k in range(geom.nb - 1):
        sib = j ^ 1
        rows.append(geom.boff[k] + (slot * geom.nblocks + block) * geom.bsz[k] + sib if sib < geom.bsz[k] else PAD_ROW)
        j //= 2
    j = block
    for k in range(geom.nt - 1):
        sib = j ^ 1
        rows.append(geom.toff[k] + slot * geom.tsz[k] + sib if sib < geom.tsz[k] else PAD_ROW)
        j //= 2
    return (rows + [PAD_ROW] * md)[:md]


def path_addr_model(geom, base, slot, cell, md):
    """(addresses, leaf address) of k_sample_many: base + row * 32, 0 where the path is padded."""
    rows = path_rows_model(geom, slot, cell, md)
    return [0 if r == PAD_ROW else base + r * 32 for r in rows], base + (slot * geom.n_cells + cell) * 32


def root_row(geom, slot):
    return geom.toff[geom.nt - 1] + slot


# ---- block path walk ----------------------------------------------------------------------------------------------------------------
def walk_model(block_root, block, n_blocks, path, compress):
    """The root that `block_root` at leaf `block` of n_blocks reaches over `path`; compress(x, y, key) is the oracle's."""
    h, j, m = block_root, block, n_blocks
    for lvl, sib in enumerate(path):
        bottom = 1 if lvl == 0 else 0
        if j % 2 == 1:
            h = compress(sib, h, bottom)
        else:
            h = compress(h, sib, bottom + (2 if j == m - 1 else 0))
        j //= 2
        m = (m + 1) // 2
    return h


# ---- case plans ---------------------------------------------------------------------------------------------------------------------
SCRUB_TOTALS = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 12289)
SCRUB_FACTORED = ((7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (65, 63), (64, 64), (17, 241), (128, 64))     # dense, many items
SCRUB_STRIDED = {(1, 1, 2): SCRUB_TOTALS,                                  # (rows, fstride, kstride): n_items
                 (3, 5, 7): (1, 21, 22, 85, 86, 1365, 1366, 2731, 4097),
                 (4097, 4100, 4097): (1, 2, 3),
                 (64, 64, 65): (1, 4, 64, 65, 128, 193)}
SCRUB_PLANTED = ("none", "all", "row0", "last", "63/64", "4095/4096", "1%")
ScrubCase = collections.namedtuple("ScrubCase", "no rows fstride kstride n_items planted serial")   # serial: planted rows of the cases before


def scrub_planted_rows(case):
    total = case.rows * case.n_items
    if case.planted == "1%":
        rng = np.random.default_rng([0x5C2B, case.no])
        return np.sort(rng.choice(total, size=max(1, total // 100), replace=False)).astype(np.int64)
    pick = {"none": [], "all": range(total), "row0": [0], "last": [total - 1], "63/64": [63, 64], "4095/4096": [4095, 4096]}[case.planted]
    return np.array([g for g in pick if g < total], dtype=np.int64)


def scrub_planted_bits(case):
    """The one bit (0..255) in which the k-th planted row of the case differs, and the side that carries the flip (0 fresh, 1 kept)."""
    k = np.arange(scrub_planted_rows(case).size, dtype=np.int64)
    return (case.serial + k) % 256, (case.no + k) % 2


def scrub_plan():
    layouts = [(t, t, t, 1) for t in SCRUB_TOTALS] + [(r, r, r, n) for r, n in SCRUB_FACTORED]
    layouts += [(r, fs, ks, n) for (r, fs, ks), items in SCRUB_STRIDED.items() for n in items]
    cases, serial = [], 0
    for (rows, fs, ks, n) in layouts:
        for planted in SCRUB_PLANTED:
            c = ScrubCase(len(cases), rows, fs, ks, n, planted, serial)
            if planted == "none" or scrub_planted_rows(c).size:
                cases.append(c)
                serial += min(2, scrub_planted_rows(c).size)      # the one- and two-row sets alone walk through all 256 bits
    return cases


REPAIR_NS = (1, 63, 64, 65, 257, 1000)
RepairCase = collections.namedtuple("RepairCase", "no n kind tail")


def repair_plan():
    """kind: rows[] a permutation or with repeats; tail: rows[n - 1] as drawn, = kept_rows - 1, or = kept_rows (a backed row)."""
    return [RepairCase(i, n, kind, tail) for i, (n, kind, tail) in
            enumerate((n, kind, tail) for n in REPAIR_NS for kind in ("permutation", "repeats") for tail in ("plain", "last", "bound"))]


def repair_flips(case):
    """(i, bit) of the requests whose fresh row differs from its kept row, in one bit."""
    return [(i, (i * 37 + case.no * 11) % 256) for i in range(case.n)
            if i % 3 == case.no % 3 and not (case.tail == "bound" and i == case.n - 1)]


SAMPLE_GEOMS = tuple((cpb, nblocks) for cpb in (1, 2, 4, 32) for nblocks in (1, 2, 64, 1 << 15))
SAMPLE_LANES = ((1, 1), (1, 255), (1, 256), (1, 257), (5, 51), (5, 52), (100, 1), (100, 3))       # (ns, n_items)
SAMPLE_MD = (-1, 0, 3)                                                                            # md - depth
# Layers of odd size: with n_cells a power of two and nblocks = n_cells / cpb every big-tree layer is even, and (m + 1) >> 1 could be
# m >> 1 unnoticed.  The kernels take n_cells apart from cpb * nblocks, so these trees have more blocks than the sampled cells reach.
SAMPLE_ODD_GEOMS = ((4, 5, 16), (1, 3, 2), (2, 7, 8), (3, 6, 16))                                  # (cpb, nblocks, n_cells)
SampleCase = collections.namedtuple("SampleCase", "no cpb nblocks n_cells n_slots ns n_items md form slot0")


def sample_plan():
    """Three slots, and explicit slots[] lists wherever there are more items than slots.  The range form (slot0 + item) runs with up to
    three items on every geometry, and with 255 / 256 / 257 items on the geometries small enough to back one slot root per item."""
    cases = []
    geoms = [(cpb, nblocks, cpb * nblocks) for cpb, nblocks in SAMPLE_GEOMS] + list(SAMPLE_ODD_GEOMS)
    for gi, (cpb, nblocks, n_cells) in enumerate(geoms):
        depth = path_depth(tree_geom(cpb, nblocks, n_cells, 3))
        for li, (ns, n_items) in enumerate(SAMPLE_LANES):
            form = "range" if n_items <= 3 and (gi + li) % 2 == 0 else "list"
            cases.append(SampleCase(len(cases), cpb, nblocks, n_cells, 3, ns, n_items, depth + SAMPLE_MD[(gi + li) % 3], form, 3 - n_items if form == "range" else 0))
        if nblocks <= 64:
            n_items = (255, 256, 257)[gi % 3]
            cases.append(SampleCase(len(cases), cpb, nblocks, n_cells, n_items + 2, 1, n_items, depth + SAMPLE_MD[(gi // 3) % 3], "range", 2))
    return cases


COMPACT_N_CELLS = (1 << 31, 1 << 32, 1 << 33, 1 << 40, 1 << 63)
COMPACT_CPB = (1, 32, 3, 1000003)
COMPACT_NS, COMPACT_REQS = 5, 3


def compact_plan():
    return [(n_cells, cpb) for n_cells in COMPACT_N_CELLS for cpb in COMPACT_CPB]


def reaches_high(index, n_cells):
    """What at least one sampled index of a compact case must do: have a bit above bit 31 set where the mask allows one, else
    (n_cells <= 2^32 leaves none) the top bit of the mask."""
    return index >> 32 != 0 if n_cells > (1 << 32) else (index >> (n_cells.bit_length() - 2)) & 1 == 1


GRID_WORDS = 4096 * 256              # work above this goes round the grid-stride loop
GATHER_ROWS_WIDTHS = (4, 32, 36, 2048)
GATHER_ADDR_WIDTHS = (1, 3, 31, 32, 33, 100, 2048, 2050)
GATHER_ADDR_OFFSETS = (0, 1, 2)
GATHER_SMALL_ROWS = (1, 63, 64, 65, 257, 1000)


def over_the_grid_rows(row_bytes, word):
    return GRID_WORDS // (row_bytes // word) + 1


def gather_rows_plan():
    """(row_bytes, nrows)"""
    return [(w, n) for w in GATHER_ROWS_WIDTHS for n in GATHER_SMALL_ROWS + (over_the_grid_rows(w, 4),)]


def gather_addr_plan():
    """(row_bytes, out offset, nrows); word-wise when both row_bytes and the offset are multiples of four"""
    cases = [(w, a, n) for w in GATHER_ADDR_WIDTHS for a in GATHER_ADDR_OFFSETS for n in GATHER_SMALL_ROWS]
    cases += [(32, 0, over_the_grid_rows(32, 4)), (33, 0, over_the_grid_rows(33, 1)), (32, 1, over_the_grid_rows(32, 1)), (1, 0, over_the_grid_rows(1, 1)),
              (2048, 0, over_the_grid_rows(2048, 4))]
    return cases


def gather_addr_wordwise(row_bytes, offset):
    return row_bytes % 4 == 0 and offset % 4 == 0


LAYER_M_IN = (1, 2, 3, 4, 5, 255, 256, 257, 511, 513)
LAYER_NSEG = (1, 3, 257)
LAYER_EXTRA = ((0, 0), (1, 1), (5, 5), (1, 5))         # rows of gap after a segment: (input, output)


def layer_plan():
    """(m_in, nseg, bottom, in stride, out stride)"""
    return [(m, nseg, bottom, m + gi, (m + 1) // 2 + go) for m in LAYER_M_IN for nseg in LAYER_NSEG for bottom in (0, 1) for gi, go in LAYER_EXTRA]


FAKE_PER = (1, 3, 100)
FAKE_ROWS = (1, 63, 64, 65, 257, 301)
FAKE_SIZES = (1, 127, 128, 2048, 2049)
FAKE_OFFSETS = (0, 4, 1)
FAKE_GROUP_FIRSTS = (0, (1 << 32) - 2, 1 << 21, (1 << 32) - 99, 7)
FAKE_GROUP_SEEDS = (12417, 0, (1 << 64) - 5, 1 << 40, 99991)


def fake_group(g):
    """(seed, first) of group g: distinct per group, `first` near 2^32 in some so that first + i % per crosses it"""
    return (FAKE_GROUP_SEEDS[g % 5] + 1001 * (g // 5)) % (1 << 64), FAKE_GROUP_FIRSTS[g % 5] + 1000 * (g // 5)


def fake_many_plan():
    return [(per, n, cs, a) for per in FAKE_PER for n in FAKE_ROWS for cs in FAKE_SIZES for a in FAKE_OFFSETS]


WALK_N_BLOCKS = tuple(range(1, 18)) + (31, 32, 33)
WalkReq = collections.namedtuple("WalkReq", "n_blocks block kind level index root")    # index: the block index handed to the kernel


def walk_plan(n_blocks):
    """Per block: the true request (slot root as it is, and as root + r), one flipped bit in the sibling of each level, one in the fresh
    root, and the true path under each neighbouring block index.  root: index into slot_roots (0 the root, 1 root + r, 2 another)."""
    depth = len(layer_sizes(n_blocks)) - 1
    reqs = []
    for b in range(n_blocks):
        reqs.append(WalkReq(n_blocks, b, "true", -1, b, 0))
        reqs.append(WalkReq(n_blocks, b, "true", -1, b, 1))
        reqs.append(WalkReq(n_blocks, b, "other root", -1, b, 2))
        reqs += [WalkReq(n_blocks, b, "sibling", lvl, b, (b + lvl) % 2) for lvl in range(depth)]
        reqs.append(WalkReq(n_blocks, b, "fresh", -1, b, b % 2))
        reqs += [WalkReq(n_blocks, b, "neighbour", -1, nb, b % 2) for nb in (b - 1, b + 1) if 0 <= nb < n_blocks]
    return reqs
