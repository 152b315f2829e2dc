"""Plain references, and the case plans, for the kernels that tests/test_gpu_kernel_units.py runs one launcher at a time.

The models restate in Python and numpy what csrc/kernels.hpp documents for k_scrub_compare, k_sample_paths, k_sample_many, the two
block-path kernels and the index mapping of k_gen_fake_cells; none of them shares code with the product.  tests/test_kernel_models_cpu.py holds them against
oracle/poseidon2_ref.py on small trees and checks that every edge the GPU module claims is really in its plan; the plans are plain
functions, so that check needs no GPU.

k_verify_samples has no model of its own here: what it must answer is tests/circuit_verdict.py, the circuit restated signal for signal.
This module adds the builder of inputs that the circuit accepts (trees from the producer-side oracle), the packer into the launcher's
four arrays, and the plan of launches (verify_plan).  Out of scope of that plan: blockTreeDepth == 0 (the host refuses it and the
circuit cannot be instantiated), nSamples >= 2^29 (the counter's second limb would need about 2^29 lanes) and a grid beyond
fits_one_grid."""
import collections
import contextlib
import functools
import itertools
import random

import numpy as np

import circuit_verdict as V
from oracle import circom_ref
from oracle import poseidon2_ref as P

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


def fake_cell_of(g, cells_per_slot, units_per_slot, first_unit):
    """(slot, idx) of global cell g as launch_gen_fake_cells documents it: the cell is cell idx of the slot seeded seed0 + 1001 * slot.
    cells_per_slot == 0: one slot, or with units the batch's unit 0 alone.  units_per_slot > 1: g / cells_per_slot counts units of cells_per_slot cells from first_unit on,
    units_per_slot of them to a slot; with units_per_slot <= 1 first_unit is not read."""
    slot, idx = divmod(g, cells_per_slot) if cells_per_slot else (0, g)
    if units_per_slot > 1:
        slot, unit_in_slot = divmod(first_unit + slot, units_per_slot)
        idx += unit_in_slot * cells_per_slot
    return slot, idx


FAKE_SINGLE_ROWS = (1, 63, 64, 65, 257)
FAKE_SINGLE_OFFSETS = (0, 4)
FAKE_SINGLE_CPS = (0, 1, 3, 64)
FAKE_SINGLE_FIRSTS = (0, 7, (1 << 32) - 2)
FAKE_SINGLE_UNITS = tuple((ups, fu) for ups in (1, 2, 4) for fu in (0, 5))
FakeSingleCase = collections.namedtuple("FakeSingleCase", "no n cell_size offset cells_per_slot first units_per_slot first_unit listed seed0")


def fake_is_wide(cell_size, offset):
    """the write-out through LDS: whole 128-byte lines into a 16-byte-aligned pointer (offset: the pointer's, mod 16)"""
    return cell_size % 128 == 0 and offset % 16 == 0


def fake_single_plan():
    """Every index mapping -- cells_per_slot x first x (units_per_slot, first_unit), as a range and as a list -- twice: once through
    the wide write-out and once byte by byte.  Not the full product: the shapes (rows, cell_size, offset) and the seeds are taken in
    rotation, so every shape and every mapping runs, and a given mapping meets one wide and one narrow shape."""
    shapes = [(n, cs, a) for cs in FAKE_SIZES for a in FAKE_SINGLE_OFFSETS for n in FAKE_SINGLE_ROWS]
    wide = [s for s in shapes if fake_is_wide(s[1], s[2])]
    narrow = [s for s in shapes if not fake_is_wide(s[1], s[2])]
    mappings = [(cps, first, ups, fu, listed) for cps in FAKE_SINGLE_CPS for first in FAKE_SINGLE_FIRSTS for ups, fu in FAKE_SINGLE_UNITS
                for listed in (False, True)]
    cases = []
    for i, m in enumerate(mappings):
        for shape in (wide[i % len(wide)], narrow[i % len(narrow)]):
            cases.append(FakeSingleCase(len(cases), *shape, *m, FAKE_GROUP_SEEDS[(i + i // 5) % 5]))
    return cases


def fake_single_cells(case):
    """The global cell of each lane: first + t, or a list that is not monotone, repeats an entry and jumps between slots and units."""
    if not case.listed:
        return [case.first + t for t in range(case.n)]
    rng = np.random.default_rng([0xFA4E, case.no])
    cells = [case.first + int(x) for x in rng.integers(0, 6 * max(case.cells_per_slot, 1) + 5, size=case.n)]
    if case.n >= 3:
        cells[0] = cells[2] = case.first + 5 * max(case.cells_per_slot, 1) + 1
        cells[1] = case.first
    return cells


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


# ---- k_verify_samples: inputs the circuit accepts, the launcher's arrays, the plan -----------------------------------------------------
VERIFY_GEOMS = ((3, 1, 0, 1), (2, 2, 1, 2), (5, 2, 3, 3), (6, 3, 5, 4), (8, 2, 4, 67))     # (maxDepth, blockTreeDepth, maxLog2NSlots, felts per cell)
VERIFY_NS = (5, 4, 3, 2, 2)                                                                 # nSamples of each geometry's launch
VERIFY_CELL_SIZE = {1: 16, 2: 32, 3: 64, 4: 96, 67: 2048}                                   # a cellSize with that many felts
VERIFY_FELTS_2048 = (0, 1, 32, 65, 66)                                                      # the cell felts mutated where nf = 67
VERIFY_SLOT_PAIRS = {0: ((1, 0),), 1: ((1, 0), (2, 1), (2, 0)), 3: ((1, 0), (8, 7), (5, 4), (3, 1), (8, 2)),
                     4: ((1, 0), (16, 15), (11, 10), (6, 3), (16, 8), (13, 12), (9, 4), (2, 1)),
                     5: ((1, 0), (32, 31), (11, 10), (21, 6), (32, 13), (7, 5))}           # (nSlots, slotIndex) by maxLog2NSlots
VERIFY_EDGES = (0, 1, R_MOD - 1, 1 << 253, (1 << 29) - 1, 1 << 29, 1 << 58, 1 << 232)
VERIFY_UNWRITTEN = (1 << 256) - 1                                                           # 32 bytes of 0xFF: what a refused input carries
VERIFY_TOP_M = (0, 1, 3, 5)
# (n inputs, nSamples): 1, 255, 256, 257 and 513 lanes; n * ns = 0, 1 and 63 mod 64, and 256
VERIFY_LAYOUTS = ((1, 0), (51, 4), (64, 3), (1, 256), (171, 2), (13, 5), (21, 3))
VerifyItem = collections.namedtuple("VerifyItem", "tag d expect kind")     # expect: the ns + 1 bytes the plan states, or None (the model's)
VerifyLaunch = collections.namedtuple("VerifyLaunch", "name geom ns items")
_PERMUTED, _EXPECTED = {}, {}


@contextlib.contextmanager
def memoised_hashing():
    """The oracle's two permutations (circuit side, producer side) each behind a table while the block runs: a mutant of an input
    shares all but a few of its compressions with its base, and the model computes every level of a path whatever the mask selects."""
    c_perm, p_perm = circom_ref.Permutation, P.permutation

    def c_cached(inp):
        key = ("c",) + tuple(v % R_MOD for v in inp)
        if key not in _PERMUTED:
            _PERMUTED[key] = tuple(c_perm(list(key[1:])))
        return list(_PERMUTED[key])

    def p_cached(st):
        key = ("p",) + tuple(v % R_MOD for v in st)
        if key not in _PERMUTED:
            _PERMUTED[key] = tuple(p_perm(key[1:]))
        return _PERMUTED[key]

    circom_ref.Permutation, P.permutation = c_cached, p_cached
    try:
        yield
    finally:
        circom_ref.Permutation, P.permutation = c_perm, p_perm


def _memoised(f):
    @functools.wraps(f)
    def g(*a, **kw):
        with memoised_hashing():
            return f(*a, **kw)
    return g


def verify_cfg(geom):
    """The configuration keys circuit_verdict reads, for (md, bd, m, nf)."""
    md, bd, m, nf = geom
    cs = VERIFY_CELL_SIZE[nf]
    assert (cs + 30) // 31 == nf and 1 <= bd <= md
    return {"maxDepth": md, "maxLog2NSlots": m, "cellSize": cs, "blockSize": cs << bd}


def verify_values(*seed):
    """A source of arbitrary field elements: each call returns the next one."""
    rng = random.Random(repr(seed))
    return lambda: rng.randrange(R_MOD)


def verify_values_2048(*seed):
    """As verify_values, but of every 67 draws the first 62 repeat: the 2048-byte cells of one slot share 62 felts (each position its
    own value) and differ in their last five, so that the memoised oracle hashes a cell in 3 permutations, not in 34."""
    rng = random.Random(repr(seed))
    prefix, count = [rng.randrange(R_MOD) for _ in range(62)], itertools.count()

    def draw():
        j = next(count) % 67
        return prefix[j] if j < 62 else rng.randrange(R_MOD)
    return draw


def verify_edge_values(seed):
    rng = random.Random(repr(("edges", seed)))
    return lambda: rng.choice(VERIFY_EDGES)


class VerifySlot:
    """One slot: its cell rows, its root, and path(i), the maxDepth siblings the circuit reads for cell i."""

    def __init__(self, rows, root, path):
        self.rows, self.root, self.path = rows, root, path


def verify_slot(md, bd, nf, n_cells, values):
    """n_cells = 2^k cells of nf arbitrary felts under the trees of the producer: block trees of 2^bd cells and the tree over their
    roots (k == bd: that tree is one compression with key 3, its sibling 0).  Where the producer has no counterpart the entries lie
    where the circuit reads them: for k < bd the one tree over the 2^k cells is what the bottom walk reconstructs, and the middle
    walk's one compression takes its sibling from path index bd; for md == bd there is no middle walk and the slot root is 0."""
    k = n_cells.bit_length() - 1
    assert n_cells == 1 << k and 1 <= k <= md and 1 <= bd <= md
    rows = [[values() for _ in range(nf)] for _ in range(n_cells)]
    leaves = [P.sponge2(r) for r in rows]
    cpb = 1 << bd
    if k >= bd and md > bd:
        mini = [P.merkle_tree(leaves[b * cpb:(b + 1) * cpb]) for b in range(n_cells // cpb)]
        big = P.merkle_tree([t[-1][0] for t in mini])

        def path(i):
            merged = P.merge_merkle_proofs(P.merkle_proof(mini[i // cpb], i % cpb), P.merkle_proof(big, i // cpb))
            assert merged["leafIndex"] == i
            return P.pad_merkle_proof(merged, md)["merklePath"]
        return VerifySlot(rows, big[-1][0], path)
    tree = P.merkle_tree(leaves)
    sib = values() if md > bd else None
    root = P.compress(tree[-1][0], sib, 3) if md > bd else 0

    def path(i):
        p = P.pad_merkle_proof(P.merkle_proof(tree, i), md)["merklePath"]
        if sib is not None:
            p[bd] = sib
        return p
    return VerifySlot(rows, root, path)


def verify_input(slot, geom, ns, n_slots, slot_index, entropy, values, roots=None):
    """The felt dict of `slot` as slot slot_index of a dataset of n_slots (the other slot roots from `roots`, else drawn from `values`),
    sampled ns times under `entropy`.  maxLog2NSlots == 0: no dataset tree, the dataset root is 0."""
    md, bd, m, nf = geom
    assert 1 <= n_slots <= 1 << m and 0 <= slot_index < n_slots
    if m == 0:
        dataset_root, proof = 0, []
    else:
        roots = list(roots) if roots is not None else [values() for _ in range(n_slots)]
        assert len(roots) == n_slots
        roots[slot_index] = slot.root
        dset = P.merkle_tree(roots)
        dataset_root, proof = dset[-1][0], P.pad_merkle_proof(P.merkle_proof(dset, slot_index), m)["merklePath"]
    n_cells = len(slot.rows) if slot.rows else 2
    d = {"dataSetRoot": dataset_root, "entropy": entropy, "nCellsPerSlot": n_cells, "nSlotsPerDataSet": n_slots, "slotIndex": slot_index,
         "slotRoot": slot.root, "slotProof": proof, "cellData": [], "merklePaths": []}
    for cnt in range(ns):
        i = V.sample_index(d, None, cnt)
        d["cellData"].append(list(slot.rows[i]))
        d["merklePaths"].append(slot.path(i))
    return d


@_memoised
def verify_build(md, bd, m, nf, ns, n_cells, n_slots, slot_index, entropy, values):
    """A felt dict (circuit_verdict's format) that the circuit accepts; `values` is called for every felt that is free."""
    return verify_input(verify_slot(md, bd, nf, n_cells, values), (md, bd, m, nf), ns, n_slots, slot_index, entropy, values)


def verify_past(d, geom, slot_index, accepted):
    """d with slotIndex moved to one the shape allows although it is >= nSlotsPerDataSet; accepted: with the dataset root that the
    circuit's top walk then reaches."""
    assert d["nSlotsPerDataSet"] <= slot_index < 1 << geom[2]
    e = V.copy(d)
    e["slotIndex"] = slot_index
    if accepted:
        e["dataSetRoot"] = V.top_root(e, verify_cfg(geom))
    return e


def verify_find_entropy(slot_root, n_cells, ns, want, *seed):
    """The first entropy of a seeded sequence under which some sample's index satisfies want(index)."""
    rng = random.Random(repr(("entropy",) + seed))
    stub = {"slotRoot": slot_root, "nCellsPerSlot": n_cells}
    for _ in range(64 * n_cells):
        stub["entropy"] = rng.randrange(R_MOD)
        if any(want(V.sample_index(stub, None, c)) for c in range(ns)):
            return stub["entropy"]
    raise AssertionError("no entropy found")


@_memoised
def verify_expected(d, geom):
    """The ns + 1 bytes the kernel owes input d: one per sample, then the dataset-root byte.  From circuit_verdict.verdict alone."""
    if id(d) not in _EXPECTED:
        status, ok = V.verdict(d, verify_cfg(geom))
        assert (status & V.SHAPE == 0) or not any(ok)
        _EXPECTED[id(d)] = (d, tuple(ok) + ((0 if status & (V.SHAPE | V.DATASET_ROOT) else 1),))
    return _EXPECTED[id(d)][1]


def verify_levels_read(geom, n_cells):
    """Indices of merklePaths that the slot-root comparison depends on: the bottom walk's min(k, bd) levels, then max(1, k - bd) of the
    middle walk from index bd on (maskBitsCorrected[0] = 1).  None where maxDepth == blockTreeDepth: RootFromMerklePath(0) is the
    empty sum, the sample compares 0 with slotRoot, and what the bottom walk reconstructed goes nowhere."""
    md, bd, m, nf = geom
    k = n_cells.bit_length() - 1
    return set(range(min(k, bd))) | set(range(bd, bd + max(1, k - bd))) if md > bd else set()


def verify_top_levels_read(geom, n_slots):
    """Indices of slotProof below CeilingLog2(nSlots), at least one (none where maxLog2NSlots == 0)."""
    return set(range(max(1, (n_slots - 1).bit_length()))) if geom[2] else set()


def _felt_rows(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def verify_pack(dicts, geom):
    """(prm, heads, cells, paths) as the comment above VerifyGeom lays them out: prm n x 4 words (nCellsPerSlot, nSlotsPerDataSet,
    slotIndex, shape ok), heads n x (3 + m) felts (dataSetRoot, entropy, slotRoot, slotProof), cells n x ns x nf felts, paths
    n x ns x md felts; a felt is 32 bytes, little endian."""
    md, bd, m, nf = geom
    cfg, n = verify_cfg(geom), len(dicts)
    ns = len(dicts[0]["cellData"]) if n else 0
    for d in dicts:
        assert len(d["slotProof"]) == m and len(d["cellData"]) == len(d["merklePaths"]) == ns
        assert all(len(r) == nf for r in d["cellData"]) and all(len(r) == md for r in d["merklePaths"])
    prm = np.array([[d["nCellsPerSlot"], d["nSlotsPerDataSet"], d["slotIndex"], 1 if V.shape_ok(d, cfg) else 0] for d in dicts], dtype=np.uint64).reshape(n, 4)
    heads = _felt_rows(v for d in dicts for v in [d["dataSetRoot"], d["entropy"], d["slotRoot"]] + d["slotProof"])
    cells = _felt_rows(v for d in dicts for r in d["cellData"] for v in r)
    paths = _felt_rows(v for d in dicts for r in d["merklePaths"] for v in r)
    u8 = lambda b, *shape: np.frombuffer(b, dtype=np.uint8).reshape(*shape, 32).copy()       # noqa: E731
    return prm, u8(heads, n, 3 + m), u8(cells, n, ns, nf), u8(paths, n, ns, md)


def verify_unpack(prm, heads, cells, paths):
    """The felt dicts that verify_pack's arrays hold, and their shape-ok words."""
    felts = lambda a: [int.from_bytes(a[i].tobytes(), "little") for i in range(a.shape[0])]      # noqa: E731
    out = []
    for i in range(prm.shape[0]):
        h = felts(heads[i])
        out.append({"dataSetRoot": h[0], "entropy": h[1], "nCellsPerSlot": int(prm[i, 0]), "nSlotsPerDataSet": int(prm[i, 1]),
                    "slotIndex": int(prm[i, 2]), "slotRoot": h[2], "slotProof": h[3:], "cellData": [felts(r) for r in cells[i]],
                    "merklePaths": [felts(r) for r in paths[i]]})
    return out, [int(x) for x in prm[:, 3]]


def _bump(v):
    return (v + 1) % R_MOD


def _ones(ns, zero=None):
    return tuple(0 if i == zero else 1 for i in range(ns + 1))


def verify_mutants(tag, base, geom, felts=None):
    """One copy of the accepted `base` per position, that felt + 1 mod r: every cellData felt (of `felts`), every merklePaths level,
    every slotProof level, dataSetRoot, slotRoot, entropy.  A position the circuit reads clears exactly its own byte (a sample's, or
    the dataset-root byte); one above the selected layer or above CeilingLog2 changes nothing, and where maxDepth == blockTreeDepth no
    cell felt and no path level does (verify_levels_read); slotRoot and entropy: the model's."""
    md, bd, m, nf = geom
    ns = len(base["cellData"])
    read, top_read = verify_levels_read(geom, base["nCellsPerSlot"]), verify_top_levels_read(geom, base["nSlotsPerDataSet"])
    compared, out = md > bd, []

    def add(what, change, expect, kind):
        d = V.copy(base)
        change(d)
        out.append(VerifyItem("%s; %s + 1" % (tag, what), d, expect, kind))

    for s in range(ns):
        for j in (range(nf) if felts is None else felts):
            add("cellData[%d][%d]" % (s, j), lambda d, s=s, j=j: d["cellData"][s].__setitem__(j, _bump(d["cellData"][s][j])), _ones(ns, s if compared else None),
                "cell" if compared else "cell, not compared")
        for lvl in range(md):
            add("merklePaths[%d][%d] (%s)" % (s, lvl, "read" if lvl in read else "above the selected layer" if compared else "not compared"),
                lambda d, s=s, lvl=lvl: d["merklePaths"][s].__setitem__(lvl, _bump(d["merklePaths"][s][lvl])),
                _ones(ns, s if lvl in read else None), "path read" if lvl in read else "path above")
    for lvl in range(m):
        add("slotProof[%d] (%s)" % (lvl, "read" if lvl in top_read else "above CeilingLog2"),
            lambda d, lvl=lvl: d["slotProof"].__setitem__(lvl, _bump(d["slotProof"][lvl])),
            _ones(ns, ns if lvl in top_read else None), "proof read" if lvl in top_read else "proof above")
    add("dataSetRoot", lambda d: d.__setitem__("dataSetRoot", _bump(d["dataSetRoot"])), _ones(ns, ns), "dataSetRoot")
    add("slotRoot", lambda d: d.__setitem__("slotRoot", _bump(d["slotRoot"])), None, "slotRoot")
    add("entropy", lambda d: d.__setitem__("entropy", _bump(d["entropy"])), None, "entropy")
    return out


def _interleaved(lists):
    return [x for group in itertools.zip_longest(*lists) for x in group if x is not None]


@functools.lru_cache(maxsize=None)
@_memoised
def verify_geometry_launch(gi):
    """One launch of geometry gi: accepted inputs of every k = 1..maxDepth in turn (neighbouring inputs differ in nCellsPerSlot), over
    the (nSlots, slotIndex) pairs of VERIFY_SLOT_PAIRS; three more at k = maxDepth whose entropy was searched for a sample at index 0,
    at index nCells - 1, and at the last cell of a block that is not the last; then every base's mutants, base after base in turn."""
    geom, ns = VERIFY_GEOMS[gi], VERIFY_NS[gi]
    md, bd, m, nf = geom
    pairs = VERIFY_SLOT_PAIRS[m]
    source = verify_values_2048 if nf == 67 else verify_values
    bases = []
    for j in range(max(md, len(pairs))):
        k, (n_slots, si) = j % md + 1, pairs[j % len(pairs)]
        d = verify_build(md, bd, m, nf, ns, 1 << k, n_slots, si, verify_values("entropy", gi, j)(), source("geometry", gi, j))
        bases.append(("k=%d nSlots=%d slotIndex=%d" % (k, n_slots, si), d))
    n_cells, cpb = 1 << md, 1 << bd
    extremes = [("index 0", lambda i: i == 0), ("index nCells - 1", lambda i: i == n_cells - 1)]
    if md > bd:
        extremes.append(("low bd bits ones", lambda i: i & (cpb - 1) == cpb - 1 and i >> bd != (n_cells >> bd) - 1))
    for e, (name, want) in enumerate(extremes):
        n_slots, si = pairs[(e + 1) % len(pairs)]
        slot = verify_slot(md, bd, nf, n_cells, source("extreme", gi, e))
        entropy = verify_find_entropy(slot.root, n_cells, ns, want, gi, e)
        d = verify_input(slot, geom, ns, n_slots, si, entropy, verify_values("extreme roots", gi, e))
        bases.append(("k=%d nSlots=%d slotIndex=%d, %s" % (md, n_slots, si, name), d))
    items = [VerifyItem(tag, d, _ones(ns), "base") for tag, d in bases]
    items += _interleaved([verify_mutants(tag, d, geom, VERIFY_FELTS_2048 if nf == 67 else None) for tag, d in bases])
    return VerifyLaunch("geometry %s ns=%d" % (geom, ns), geom, ns, items)


def _geom_of_m(m):
    return [g for g in VERIFY_GEOMS if g[2] == m][0]


@functools.lru_cache(maxsize=None)
@_memoised
def verify_top_launch(m, ns):
    """Every nSlots in 1..2^m with every slotIndex < 2^m.  slotIndex < nSlots: accepted by construction.  Past nSlots (which the
    shape allows): once as it is, the model's verdict, and once with the dataset root the circuit reaches, accepted.  ns == 0: top lanes
    only, the slot roots arbitrary felts; ns > 0: one sampled slot stands at slotIndex (at slotIndex % nSlots where that is past)."""
    geom = _geom_of_m(m)
    md, bd, _, nf = geom
    values = verify_values("top", m, ns)
    slot = verify_slot(md, bd, nf, 1 << min(md, 3), values) if ns else None
    entropy, items = values(), []
    for n_slots in range(1, (1 << m) + 1):
        roots = [values() for _ in range(n_slots)]
        for si in range(1 << m):
            at = si % n_slots
            d = verify_input(slot or VerifySlot(None, roots[at], None), geom, ns, n_slots, at, entropy, None, roots)
            tag = "top m=%d nSlots=%d slotIndex=%d" % (m, n_slots, si)
            if si < n_slots:
                items.append(VerifyItem(tag, d, _ones(ns), "top"))
            else:
                items.append(VerifyItem(tag + ", past nSlots, the dataset root of slotIndex %d" % at, verify_past(d, geom, si, False), None, "top past"))
                items.append(VerifyItem(tag + ", past nSlots, the dataset root the circuit reaches", verify_past(d, geom, si, True), _ones(ns), "top past accepted"))
    return VerifyLaunch("top walk m=%d ns=%d" % (m, ns), geom, ns, items)


VERIFY_EDGE_GEOM, VERIFY_EDGE_NS = VERIFY_GEOMS[2], 5
VERIFY_EDGE_SHAPES = ((1, 2, 1), (2, 5, 4), (4, 2, 0))        # (k, nSlots, slotIndex): k < bd, k == bd, k > bd
VERIFY_EDGE_SIBLINGS = 8                                      # further inputs of k < bd and two slots: two free siblings each


def verify_root_mutations(v):
    return (("+ 1", v + 1), ("- 1", v - 1), ("bit 253", v ^ (1 << 253)))


def verify_free_siblings(d, geom):
    """The siblings of an accepted input that are no hash: the middle walk's where k < bd, the other slot root where nSlots == 2."""
    md, bd, m, nf = geom
    out = [p[bd] for p in d["merklePaths"]] if d["nCellsPerSlot"] < 1 << bd < 1 << md else []
    return out + (d["slotProof"][:1] if d["nSlotsPerDataSet"] == 2 else [])


@functools.lru_cache(maxsize=None)
@_memoised
def verify_edge_launch():
    """Accepted inputs whose cell felts, middle sibling (k < bd) and other slot roots are all drawn from VERIFY_EDGES; the first
    three also with the dataset root, then the slot root, mutated by + 1, by - 1 and in bit 253: rejected.  The draw is the first
    seeded one after which every mutated root is still below r (what the launcher's contract asks), every edge value is in some
    sampled cell, and every edge value is some sibling."""
    geom, ns = VERIFY_EDGE_GEOM, VERIFY_EDGE_NS
    md, bd, m, nf = geom
    shapes = VERIFY_EDGE_SHAPES + tuple((1, 2, j % 2) for j in range(VERIFY_EDGE_SIBLINGS))
    for seed in range(4096):
        values = verify_edge_values(seed)
        bases = [("edges %d: k=%d nSlots=%d slotIndex=%d" % (j, k, n_slots, si), verify_build(md, bd, m, nf, ns, 1 << k, n_slots, si, values(), values))
                 for j, (k, n_slots, si) in enumerate(shapes)]
        roots = [d[key] for _, d in bases[:len(VERIFY_EDGE_SHAPES)] for key in ("dataSetRoot", "slotRoot")]
        sampled = {v for _, d in bases for r in d["cellData"] for v in r}
        siblings = {v for _, d in bases for v in verify_free_siblings(d, geom)}
        if all(0 <= w < R_MOD for v in roots for _, w in verify_root_mutations(v)) and sampled == set(VERIFY_EDGES) == siblings:
            break
    else:
        raise AssertionError("no draw of edge values found")
    items = []
    for j, (tag, d) in enumerate(bases):
        items.append(VerifyItem(tag, d, _ones(ns), "edge base"))
        for key, expect in (("dataSetRoot", _ones(ns, ns)), ("slotRoot", (0,) * (ns + 1))) if j < len(VERIFY_EDGE_SHAPES) else ():
            for how, w in verify_root_mutations(d[key]):
                e = V.copy(d)
                e[key] = w
                items.append(VerifyItem("%s; %s %s" % (tag, key, how), e, expect, "edge " + key))
    return VerifyLaunch("field edges", geom, ns, items)


def verify_refused(d, n_cells):
    """d with an nCellsPerSlot that witness generation refuses; everything the kernel must not read of it is 32 bytes of 0xFF a felt."""
    e = V.copy(d)
    e["nCellsPerSlot"] = n_cells
    e["slotProof"] = [VERIFY_UNWRITTEN] * len(e["slotProof"])
    e["cellData"] = [[VERIFY_UNWRITTEN] * len(r) for r in e["cellData"]]
    e["merklePaths"] = [[VERIFY_UNWRITTEN] * len(r) for r in e["merklePaths"]]
    return e


def _layout_pool(geom, ns, name):
    """Three accepted inputs of different nCellsPerSlot and nSlotsPerDataSet with ns samples, and of each a copy with the dataset
    root mutated, one with the last sample's first cell felt mutated and one with the first sample's."""
    md, bd, m, nf = geom
    pairs = VERIFY_SLOT_PAIRS[m]
    pool = []
    for j, k in enumerate((md, 1, bd + 1)):
        n_slots, si = pairs[(j + 2) % len(pairs)]
        d = verify_build(md, bd, m, nf, ns, 1 << k, n_slots, si, verify_values(name, "entropy", j)(), verify_values(name, j))
        tag = "k=%d nSlots=%d slotIndex=%d" % (k, n_slots, si)
        top, last, first = V.copy(d), V.copy(d), V.copy(d)
        top["dataSetRoot"] = _bump(d["dataSetRoot"])
        group = [VerifyItem(tag, d, _ones(ns), "base"), VerifyItem(tag + "; dataSetRoot + 1", top, _ones(ns, ns), "dataSetRoot")]
        if ns:
            last["cellData"][ns - 1][0] = _bump(d["cellData"][ns - 1][0])
            first["cellData"][0][0] = _bump(d["cellData"][0][0])
            group += [VerifyItem("%s; cellData[%d][0] + 1" % (tag, ns - 1), last, _ones(ns, ns - 1), "cell"),
                      VerifyItem(tag + "; cellData[0][0] + 1", first, _ones(ns, 0), "cell")]
        pool.append(group)
    return pool


@functools.lru_cache(maxsize=None)
@_memoised
def verify_layout_launches():
    """The launches of VERIFY_LAYOUTS on the (5, 2, 3, 3) geometry.  Input 0, whose dataset-root lane is the first after the sample
    lanes, has its dataset root mutated; the last input has its last sample mutated (the lane before that boundary) where there are
    samples; the inputs between go round the pool."""
    geom = VERIFY_GEOMS[2]
    launches = []
    for n, ns in VERIFY_LAYOUTS:
        pool = _layout_pool(geom, ns, "layout ns=%d" % ns)
        ring = _interleaved(pool)
        items = [ring[i % len(ring)] for i in range(n)]
        if n > 1:
            items[0] = pool[0][1]
            items[-1] = pool[1][2] if ns else pool[1][0]
        elif ns:
            items[0] = pool[0][2]
        launches.append(VerifyLaunch("layout n=%d ns=%d" % (n, ns), geom, ns, items))
    return launches


@functools.lru_cache(maxsize=None)
@_memoised
def verify_refused_launch():
    """Refused inputs (nCellsPerSlot 0 and 3, their slot proof, cells and paths all 0xFF bytes) between accepted ones and mutants."""
    geom, ns = VERIFY_GEOMS[2], 3
    pool = _layout_pool(geom, ns, "refused")
    items = []
    for i, it in enumerate(_interleaved(pool) * 2):
        items.append(it)
        bad = (0, 3)[i % 2]
        items.append(VerifyItem("%s; refused: nCellsPerSlot = %d, the rest 0xFF bytes" % (it.tag, bad), verify_refused(it.d, bad), (0,) * (ns + 1), "refused"))
    return VerifyLaunch("refused shapes", geom, ns, items)


def verify_plan():
    """Every launch of the k_verify_samples test; the sections are cached, a caller may take them one by one."""
    launches = [verify_geometry_launch(gi) for gi in range(len(VERIFY_GEOMS))]
    launches += [verify_top_launch(m, 0) for m in VERIFY_TOP_M] + [verify_top_launch(3, 2)]
    return launches + [verify_edge_launch()] + verify_layout_launches() + [verify_refused_launch()]


def verify_plan_cases(launches=None):
    """Inputs of the plan (each owes ns + 1 bytes)."""
    return sum(len(x.items) for x in (verify_plan() if launches is None else launches))
