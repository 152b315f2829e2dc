"""GPU suite: the compare, sampling, gather, layer, fake-cell, path-walk and proof-input verify kernels one launcher at a time.

The feature tests (scrub, repair, proof_many, block proofs, fill) reach these kernels only behind hosts that validate every request, so
the kernels there see nothing but well-formed hashes.  Here each cp2k::launch_* is called directly, through the forwarders of
tests/device_check/libkernel_unit.so.  That library is LINKED against libcodex_p2.so (nm -D shows cp2k::launch_* exported there), so the
code objects that run are the product's own; tests/test_kernel_models_cpu.py checks the linkage.  Expected values come from
tests/kernel_models.py and the C oracle, every comparison is bit exact, every output lies between guard bytes and is pre-filled with
a non-zero pattern, and every row or address handed to a kernel is backed by memory of the test: where a bound is tested (rows[i] ==
kept_rows, dest == n_rows) a real matching row lies behind it, so a kernel that ignored the bound would answer wrongly, not fault.

The plans (which totals, layouts, lane counts, widths, offsets run) are functions of tests/kernel_models.py, checked without a GPU.

Compact sampling at n_cells <= 2^32 cannot produce an index with a bit above bit 31 (the mask removes them); those cases assert the top
bit of the mask instead, the cases from 2^33 up a bit above 31 (kernel_models.reaches_high).

Sampling also runs on four trees with layers of odd size (kernel_models.SAMPLE_ODD_GEOMS): with n_cells a power of two and
nblocks = n_cells / cpb no big-tree layer is odd, and the (m + 1) >> 1 of the path loops could be m >> 1 unnoticed.

k_verify_samples runs the launches of kernel_models.verify_plan: every nCellsPerSlot side by side in one launch, each felt of each
accepted input mutated in turn, the top walk over every (nSlots, slotIndex), field edges, lane layouts, refused inputs whose unread
regions are 0xFF bytes.  What it owes, byte for byte, is tests/circuit_verdict.py; the plan's own expectations are held against that
model by the CPU suite.  Each ok buffer lies between guards, and the four input arrays are read back after every launch.

Counts and times, printed by each test ("[kernel units] ...") and by test_summary.  On an MI355X the module ran in 6.1 s, 1.5 s of
it loading the libraries: scrub compare 320 cases 0.4 s, repair compare 36 cases 0.01 s, sample paths / sample many 176 cases (37 776
lanes through each kernel) 0.4 s, compact sampling 20 cases 0.01 s, gather rows 28 cases 0.2 s, gather addr 149 cases 0.3 s, compress
layer 240 cases 0.3 s, fake cells with many seeds 270 cases 0.1 s, the fake cells' index mapping 288 cases 0.1 s, block path roots 2547
requests 0.02 s (0.16 s before it for the oracle's trees and the model's verdicts), block path commit 2816 requests 0.01 s.  Those are
6890 cases.  The k_verify_samples plan adds
3241 inputs (7990 lanes in 19 launches: five geometries 144 / 105 / 248 / 261 / 374 inputs, top walks 1 / 5 / 92 / 1520 / 92, edges,
layouts and refused shapes 399); building it and taking the model's verdicts costs about 8 s of pure Python on the host, most of it in
the 2048-byte geometry (2.6 s) and in the model's first pass.  The summary line: "10131 cases, 0 skipped"."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import kernel_models as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libkernel_unit.so")
FRONT = 256                                   # guard bytes before a body (keeps the allocation's alignment), and at least as many after
ORACLE_THREADS = 16
HIP_INVALID = 1                               # hipErrorInvalidValue
PATTERN = ((np.arange(4099, dtype=np.int64) * 7 + 0xC3) % 255 + 1).astype(np.uint8)     # never zero
TALLY = {}


class TreeGeom(ctypes.Structure):
    _fields_ = [("nb", ctypes.c_uint32), ("nt", ctypes.c_uint32), ("cpb", ctypes.c_uint64), ("nblocks", ctypes.c_uint64),
                ("n_cells", ctypes.c_uint64), ("boff", ctypes.c_uint64 * K.MAX_LAYERS), ("bsz", ctypes.c_uint64 * K.MAX_LAYERS),
                ("toff", ctypes.c_uint64 * K.MAX_LAYERS), ("tsz", ctypes.c_uint64 * K.MAX_LAYERS)]


class VerifyGeom(ctypes.Structure):
    _fields_ = [("n", ctypes.c_size_t), ("ns", ctypes.c_uint32), ("nf", ctypes.c_uint32), ("md", ctypes.c_uint32), ("m", ctypes.c_uint32),
                ("bd", ctypes.c_uint32)]


class ManyReq(ctypes.Structure):
    _fields_ = [("entropy", ctypes.c_uint8 * 32), ("slot_root", ctypes.c_uint8 * 32), ("n_cells", ctypes.c_uint64), ("cpb", ctypes.c_uint64),
                ("nodes", ctypes.c_uint64), ("slot", ctypes.c_uint64), ("geom", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("tail", ctypes.c_uint64)]        # alignas(16): 104 bytes of members, 112 a request


def geom_struct(g):
    s = TreeGeom()
    s.nb, s.nt, s.cpb, s.nblocks, s.n_cells = g.nb, g.nt, g.cpb, g.nblocks, g.n_cells
    for k in range(g.nb):
        s.boff[k], s.bsz[k] = g.boff[k], g.bsz[k]
    for k in range(g.nt):
        s.toff[k], s.tsz[k] = g.toff[k], g.tsz[k]
    return s


@pytest.fixture(scope="module")
def ku(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libkernel_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp, sz, u64, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    sigs = {"ku_scrub_compare": [vp, sz, vp, sz, sz, sz, vp, vp],
            "ku_repair_compare": [vp, vp, sz, vp, sz, vp],
            "ku_sample_paths": [ctypes.POINTER(TreeGeom), vp, vp, vp, u64, sz, u32, u32, vp, vp, vp],
            "ku_sample_many": [vp, vp, sz, u32, u32, vp, vp, vp],
            "ku_gather_rows": [vp, vp, sz, sz, vp],
            "ku_gather_addr": [vp, sz, sz, vp],
            "ku_gen_fake_cells": [u64, u64, u64, vp, sz, sz, vp, u64, u64],
            "ku_gen_fake_cells_many": [vp, vp, u64, sz, sz, vp],
            "ku_compress_layer": [vp, vp, sz, sz, i32, sz, sz],
            "ku_block_path_roots": [vp, vp, vp, vp, u64, u32, sz, vp, vp],
            "ku_block_path_commit": [vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64],
            "ku_verify_samples": [ctypes.POINTER(VerifyGeom), vp, vp, vp, vp, vp]}
    for name, args in sigs.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = i32, args
    for name in ("ku_sizeof_tree_geom", "ku_sizeof_many_req", "ku_sizeof_verify_geom", "ku_scrub_tile"):
        getattr(lib, name).restype = sz
    assert lib.ku_sizeof_tree_geom() == ctypes.sizeof(TreeGeom) == 1312
    assert lib.ku_sizeof_many_req() == ctypes.sizeof(ManyReq) == 112
    assert lib.ku_sizeof_verify_geom() == ctypes.sizeof(VerifyGeom) == 32
    assert lib.ku_scrub_tile() == K.SCRUB_TILE
    return lib


@pytest.fixture(scope="module")
def torch_(ku):
    import torch
    yield torch
    torch.cuda.synchronize()


# ---- buffers -----------------------------------------------------------------------------------------------------------------------
def up(torch, arr):
    """A host array's bytes on the device."""
    a = np.array(arr, copy=True, order="C")
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


class Out:
    """nbytes of output at `offset` bytes past an aligned address, pre-filled with PATTERN like the FRONT guard bytes before it and the
    `back` bytes after it.  check() compares the whole buffer -- guards included -- with the pattern overwritten by `want`."""

    def __init__(self, torch, nbytes, offset=0, back=FRONT):
        self.torch, self.lo, self.n = torch, FRONT + offset, nbytes
        self.pre = np.resize(PATTERN, self.lo + nbytes + back)
        self.t = torch.from_numpy(self.pre.copy()).cuda()
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + self.lo

    def fetch(self):
        self.torch.cuda.synchronize()
        self.got = self.t.cpu().numpy()
        return self.got[self.lo:self.lo + self.n]

    def guards_ok(self):
        return np.array_equal(self.got[:self.lo], self.pre[:self.lo]) and np.array_equal(self.got[self.lo + self.n:], self.pre[self.lo + self.n:])

    def prefill(self):
        return self.pre[self.lo:self.lo + self.n]

    def check(self, want, what, bad, row_bytes=0, name=None):
        """Appends to `bad` what differs: the first differing row (row_bytes > 0) or byte, and disturbed guards."""
        body = self.fetch()
        want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert want.size == self.n
        if not self.guards_ok():
            bad.append("%s: bytes around the output changed" % what)
        if not np.array_equal(body, want):
            i = int(np.nonzero(body != want)[0][0])
            where = "byte %d" % i if not row_bytes else "row %d byte %d" % (i // row_bytes, i % row_bytes)
            bad.append("%s: %d bytes differ, first at %s: device %#04x, expected %#04x%s" % (
                what, int((body != want).sum()), where, int(body[i]), int(want[i]), name(i // row_bytes) if name and row_bytes else ""))
        return body


def canonical_rows(rng, n):
    """n random field elements below 2^253 < r, as canonical 32-byte rows."""
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x1F
    return a


def flip(rows, i, bit):
    rows[i, bit // 8] ^= np.uint8(1 << (bit % 8))


def as_int(row):
    return int.from_bytes(np.asarray(row, dtype=np.uint8).tobytes(), "little")


def report(capsys, name, cases, bad, t0):
    TALLY[name] = cases
    with capsys.disabled():
        print("\n[kernel units] %s: %d cases, 0 skipped, %d failed, %.1f s" % (name, cases, len(bad), time.time() - t0))
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:200]))


# ---- k_scrub_compare -----------------------------------------------------------------------------------------------------------------
def test_scrub_compare_bitmap_and_counts(ku, torch_, capsys):
    """Rows equal on both sides except at the planted ones, which differ in one bit; gap rows of the strided layouts differ everywhere.
    Every bitmap word to the end of the last tile, every count, and the words after them."""
    torch, t0, bad, plan = torch_, time.time(), [], K.scrub_plan()
    for c in plan:
        what = "scrub rows=%d fstride=%d kstride=%d n_items=%d planted=%s" % (c.rows, c.fstride, c.kstride, c.n_items, c.planted)
        rng = np.random.default_rng([0x5C2B, c.no])
        total = c.rows * c.n_items
        fresh = rng.integers(0, 256, size=(c.n_items * c.fstride, 32), dtype=np.uint8)
        kept = rng.integers(0, 256, size=(c.n_items * c.kstride, 32), dtype=np.uint8)
        item, r = np.divmod(np.arange(total, dtype=np.int64), c.rows)
        fo, ko = item * c.fstride + r, item * c.kstride + r
        kept[ko] = fresh[fo]
        rows = K.scrub_planted_rows(c)
        bit, side = K.scrub_planted_bits(c)
        mask = (1 << (bit % 8)).astype(np.uint8)
        f, k = side == 0, side == 1
        fresh[fo[rows[f]], bit[f] // 8] ^= mask[f]
        kept[ko[rows[k]], bit[k] // 8] ^= mask[k]
        want_bits, want_counts = K.scrub_model(fresh, kept, c.rows, c.fstride, c.kstride, c.n_items)
        groups = K.scrub_groups(total)
        assert int(want_counts.sum()) == rows.size and want_bits.size == groups * K.SCRUB_TILE // 64 and want_counts.size == groups
        d_fresh, d_kept = up(torch, fresh), up(torch, kept)
        bits, counts = Out(torch, want_bits.size * 8), Out(torch, groups * 4)
        status = ku.ku_scrub_compare(d_fresh.data_ptr(), c.fstride, d_kept.data_ptr(), c.kstride, c.rows, c.n_items, bits.ptr, counts.ptr)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        bits.check(want_bits, what + " bits", bad, 8, lambda w: " (rows %d..%d)" % (64 * w, 64 * w + 63))
        counts.check(want_counts, what + " counts", bad, 4)
    report(capsys, "scrub compare", len(plan), bad, t0)


def test_scrub_compare_refusals_and_no_work(ku, torch_):
    torch = torch_
    rows = up(torch, np.zeros((8, 32), dtype=np.uint8))
    bits, counts = Out(torch, K.SCRUB_TILE // 8), Out(torch, 4)
    p = rows.data_ptr()
    assert ku.ku_scrub_compare(p, 4, p, 4, 4, 0, bits.ptr, counts.ptr) == 0 and ku.ku_scrub_compare(p, 4, p, 4, 0, 2, bits.ptr, counts.ptr) == 0
    assert ku.ku_scrub_compare(p, 3, p, 4, 4, 2, bits.ptr, counts.ptr) == HIP_INVALID and ku.ku_scrub_compare(p, 4, p, 3, 4, 2, bits.ptr, counts.ptr) == HIP_INVALID
    assert ku.ku_scrub_compare(None, 4, p, 4, 4, 2, bits.ptr, counts.ptr) == HIP_INVALID and ku.ku_scrub_compare(p, 4, p, 4, 4, 2, None, counts.ptr) == HIP_INVALID
    bad = []
    bits.check(bits.prefill(), "bits", bad)
    counts.check(counts.prefill(), "counts", bad)
    assert not bad, bad


# ---- k_repair_compare ------------------------------------------------------------------------------------------------------------------
def test_repair_compare_verdicts(ku, torch_, capsys):
    torch, t0, bad, plan = torch_, time.time(), [], K.repair_plan()
    for c in plan:
        what = "repair n=%d rows[]=%s tail=%s" % (c.n, c.kind, c.tail)
        rng = np.random.default_rng([0x4E9A, c.no])
        kept_rows = c.n + 5
        kept = rng.integers(0, 256, size=(kept_rows + 1, 32), dtype=np.uint8)      # row kept_rows: backed, outside what the kernel may read
        rows = rng.permutation(kept_rows)[:c.n] if c.kind == "permutation" else rng.integers(0, c.n // 4 + 1, size=c.n)
        rows = rows.astype(np.uint64)
        if c.tail != "plain":
            rows[c.n - 1] = kept_rows - 1 if c.tail == "last" else kept_rows
        fresh = kept[rows.astype(np.int64)].copy()
        for i, bit in K.repair_flips(c):
            flip(fresh, i, bit)
        want = ((rows >= kept_rows) | (fresh != kept[rows.astype(np.int64)]).any(axis=1)).astype(np.uint32)
        assert int(want.sum()) == len(K.repair_flips(c)) + (c.tail == "bound")
        d_fresh, d_kept, d_rows = up(torch, fresh), up(torch, kept), up(torch, rows)
        verdict = Out(torch, c.n * 4)
        status = ku.ku_repair_compare(d_fresh.data_ptr(), d_kept.data_ptr(), kept_rows, d_rows.data_ptr(), c.n, verdict.ptr)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        verdict.check(want, what, bad, 4, lambda i: " (request %d, row %d of %d)" % (i, int(rows[i]), kept_rows))
    report(capsys, "repair compare", len(plan), bad, t0)


# ---- k_sample_paths, k_sample_many -----------------------------------------------------------------------------------------------------
SAMPLE_ROOTS = canonical_rows(np.random.default_rng(0x5A3F), 260)
SAMPLE_ENTROPY = canonical_rows(np.random.default_rng(0xE271), 1)[0]
DECOY_GEOM = K.tree_geom(3, 5, 15, 7)


@pytest.fixture(scope="module")
def node_arena(torch_):
    """Room for the largest node buffer of the plan (under 256 MiB).  The sampling kernels read only the slot roots of it; the rest stays
    as allocated: whatever a wrong kernel read there would be inside this buffer."""
    return torch_.empty(256 << 20, dtype=torch_.uint8, device="cuda")


def test_sample_paths_and_sample_many_agree_with_the_models(ku, torch_, oracle, node_arena, capsys):
    """indices from the oracle's cell_index, gcell / rows / addresses from the models, and k_sample_many's addresses = base + 32 * the
    rows k_sample_paths wrote for the same requests."""
    torch, t0, bad, plan = torch_, time.time(), [], K.sample_plan()
    C, _ = oracle
    index_of, lanes_run = {}, 0
    d_entropy = up(torch, SAMPLE_ENTROPY)
    base = node_arena.data_ptr()
    for c in plan:
        what = "sample cpb=%d nblocks=%d n_cells=%d n_slots=%d ns=%d n_items=%d md=%d %s" % (c.cpb, c.nblocks, c.n_cells, c.n_slots, c.ns, c.n_items, c.md, c.form)
        g = K.tree_geom(c.cpb, c.nblocks, c.n_cells, c.n_slots)
        assert g.total_rows * 32 <= node_arena.numel()
        r0 = K.root_row(g, 0) * 32
        node_arena[r0:r0 + 32 * c.n_slots] = up(torch, SAMPLE_ROOTS[:c.n_slots])
        rng = np.random.default_rng([0x5A3F, c.no])
        slots = rng.integers(0, 3, size=c.n_items).astype(np.uint64) if c.form == "list" else (c.slot0 + np.arange(c.n_items)).astype(np.uint64)
        assert int(slots.max()) < c.n_slots
        d_slots = up(torch, slots) if c.form == "list" else None
        lanes = c.ns * c.n_items
        lanes_run += lanes
        want_idx, want_g, want_rows = np.empty(lanes, np.uint64), np.empty(lanes, np.uint64), np.empty((lanes, c.md), np.uint64)
        want_addr, want_leaf = np.empty((lanes, c.md), np.uint64), np.empty(lanes, np.uint64)
        rows_of = {}
        for t in range(lanes):
            slot, counter = int(slots[t // c.ns]), t % c.ns + 1
            key = (slot, g.n_cells, counter)
            if key not in index_of:
                index_of[key] = C.cell_index(SAMPLE_ENTROPY, SAMPLE_ROOTS[slot], g.n_cells, counter)
            cell = index_of[key]
            if (slot, cell) not in rows_of:
                addrs, leaf = K.path_addr_model(g, base, slot, cell, c.md)
                rows_of[(slot, cell)] = (np.array(K.path_rows_model(g, slot, cell, c.md), dtype=np.uint64), np.array(addrs, dtype=np.uint64), leaf)
            want_idx[t], want_g[t] = cell, slot * g.n_cells + cell
            want_rows[t], want_addr[t], want_leaf[t] = rows_of[(slot, cell)]
        gs = geom_struct(g)
        idx, gcell, rows = Out(torch, lanes * 8), Out(torch, lanes * 8), Out(torch, lanes * c.md * 8)
        status = ku.ku_sample_paths(ctypes.byref(gs), base, d_entropy.data_ptr(), d_slots.data_ptr() if d_slots is not None else None, c.slot0,
                                    c.n_items, c.ns, c.md, idx.ptr, gcell.ptr, rows.ptr)
        if status != 0:
            bad.append("%s: ku_sample_paths status %d" % (what, status))
            continue
        lane = lambda t: " (item %d counter %d slot %d)" % (t // c.ns, t % c.ns + 1, int(slots[t // c.ns]))      # noqa: E731
        idx.check(want_idx, what + " indices", bad, 8, lane)
        gcell.check(want_g, what + " gcell", bad, 8, lane)
        got_rows = rows.check(want_rows, what + " rows", bad, 8 * c.md, lane).view(np.uint64)
        # the same requests through k_sample_many: a three-entry geometry table whose entry 0 is another geometry
        reqs = (ManyReq * c.n_items)()
        for i in range(c.n_items):
            q = reqs[i]
            q.entropy[:] = SAMPLE_ENTROPY.tolist()
            q.slot_root[:] = SAMPLE_ROOTS[int(slots[i])].tolist()
            q.n_cells, q.cpb, q.nodes, q.slot, q.geom, q.pad, q.tail = g.n_cells, g.cpb, base, int(slots[i]), 1 + i % 2, 0xFFFFFFFF, PATTERN_WORD
        table = (TreeGeom * 3)(geom_struct(DECOY_GEOM), gs, gs)
        d_reqs, d_table = up(torch, np.frombuffer(bytes(reqs), dtype=np.uint8)), up(torch, np.frombuffer(bytes(table), dtype=np.uint8))
        idx2, blocks, addr = Out(torch, lanes * 8), Out(torch, lanes * 8), Out(torch, (lanes * c.md + lanes) * 8)
        status = ku.ku_sample_many(d_reqs.data_ptr(), d_table.data_ptr(), c.n_items, c.ns, c.md, idx2.ptr, blocks.ptr, addr.ptr)
        if status != 0:
            bad.append("%s: ku_sample_many status %d" % (what, status))
            continue
        idx2.check(want_idx, what + " many: indices", bad, 8, lane)
        blocks.check(blocks.prefill(), what + " many: blocks[] of resident requests", bad, 8, lane)
        got_addr = addr.check(np.concatenate([want_addr.reshape(-1), want_leaf]), what + " many: addresses", bad, 8).view(np.uint64)
        twin = np.where(got_rows == K.PAD_ROW, np.uint64(0), np.uint64(base) + got_rows * np.uint64(32))
        if not np.array_equal(got_addr[:lanes * c.md], twin):
            bad.append("%s: k_sample_many's addresses are not base + 32 * k_sample_paths' rows" % what)
    with capsys.disabled():
        print("\n[kernel units] sampling: %d lanes through each kernel" % lanes_run)
    report(capsys, "sample paths / sample many", len(plan), bad, t0)


PATTERN_WORD = 0xA5C3A5C3A5C3A5C3


def test_sample_many_compact_requests_above_32_bits(ku, torch_, oracle, capsys):
    """nodes == 0: indices and blocks[] against the oracle at n_cells from 2^31 to 2^63, the address region untouched."""
    torch, t0, bad, plan = torch_, time.time(), [], K.compact_plan()
    C, _ = oracle
    ns, n_req, md = K.COMPACT_NS, K.COMPACT_REQS, 8
    table = (TreeGeom * 1)(geom_struct(DECOY_GEOM))
    d_table = up(torch, np.frombuffer(bytes(table), dtype=np.uint8))
    for no, (n_cells, cpb) in enumerate(plan):
        what = "compact n_cells=2^%d cpb=%d" % (n_cells.bit_length() - 1, cpb)
        for attempt in range(16):                                  # the first seeded entropies whose samples reach the high bits
            rng = np.random.default_rng([0xC0A7, no, attempt])
            entropy, roots = canonical_rows(rng, n_req), canonical_rows(rng, n_req)
            want_idx = np.array([C.cell_index(entropy[i], roots[i], n_cells, k + 1) for i in range(n_req) for k in range(ns)], dtype=np.uint64)
            if any(K.reaches_high(int(x), n_cells) for x in want_idx):
                break
        assert any(K.reaches_high(int(x), n_cells) for x in want_idx), what
        assert all(int(x) < n_cells for x in want_idx)
        reqs = (ManyReq * n_req)()
        for i in range(n_req):
            q = reqs[i]
            q.entropy[:] = entropy[i].tolist()
            q.slot_root[:] = roots[i].tolist()
            q.n_cells, q.cpb, q.nodes, q.slot, q.geom, q.pad, q.tail = n_cells, cpb, 0, 0, 0, 0, 0
        d_reqs = up(torch, np.frombuffer(bytes(reqs), dtype=np.uint8))
        lanes = ns * n_req
        idx, blocks, addr = Out(torch, lanes * 8), Out(torch, lanes * 8), Out(torch, (lanes * md + lanes) * 8)
        status = ku.ku_sample_many(d_reqs.data_ptr(), d_table.data_ptr(), n_req, ns, md, idx.ptr, blocks.ptr, addr.ptr)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        idx.check(want_idx, what + " indices", bad, 8)
        blocks.check(np.array([int(x) // cpb for x in want_idx], dtype=np.uint64), what + " blocks", bad, 8)
        addr.check(addr.prefill(), what + " address region", bad, 8)
    report(capsys, "sample many, compact", len(plan), bad, t0)


# ---- k_gather_rows, k_gather_addr ------------------------------------------------------------------------------------------------------
def source_rows(n, row_bytes):
    """Row i carries i: in its first four bytes where it has them, and mixed into every byte."""
    i, c = np.arange(n, dtype=np.int64)[:, None], np.arange(row_bytes, dtype=np.int64)[None, :]
    src = ((i * 131 + c * 29 + (i >> 8) * 7 + 17) & 0xFF).astype(np.uint8)
    if row_bytes >= 4:
        src[:, :4] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)
    return src


def index_list(rng, nrows, nsrc):
    """Repeats (fewer sources than rows, or drawn with replacement), ~0 at every seventh place, the first and the last source row."""
    idx = rng.integers(0, nsrc, size=nrows).astype(np.uint64)
    idx[3::7] = K.PAD_ROW
    idx[0] = nsrc - 1
    if nrows > 2:
        idx[1], idx[2] = 0, nsrc - 1
    return idx


def gathered(src, idx):
    pad = idx == K.PAD_ROW
    out = src[np.where(pad, 0, idx).astype(np.int64)]
    out[pad] = 0
    return out


def named(idx, body, row_bytes):
    def name(r):
        got = body[r * row_bytes:r * row_bytes + 4]
        return " (index[%d] = %#x%s)" % (r, int(idx[r]), ", the device's row begins like source row %d" % int(got.view("<u4")[0]) if row_bytes >= 4 else "")
    return name


def test_gather_rows(ku, torch_, capsys):
    torch, t0, bad, plan = torch_, time.time(), [], K.gather_rows_plan()
    for no, (w, n) in enumerate(plan):
        what = "gather_rows row_bytes=%d nrows=%d" % (w, n)
        rng = np.random.default_rng([0x6A7E, no])
        nsrc = 997 if n > 2 else 3
        src, idx = source_rows(nsrc, w), index_list(rng, n, nsrc)
        d_src, d_idx = up(torch, src), up(torch, idx)
        out = Out(torch, n * w)
        status = ku.ku_gather_rows(d_src.data_ptr(), d_idx.data_ptr(), n, w, out.ptr)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        out.fetch()
        out.check(gathered(src, idx), what, bad, w, named(idx, out.got[out.lo:], w))
    report(capsys, "gather rows", len(plan), bad, t0)


def test_gather_rows_refuses_what_it_would_truncate(ku, torch_):
    """A row length or a pointer that is no multiple of four: hipErrorInvalidValue and nothing written."""
    torch = torch_
    d_src = up(torch, source_rows(16, 40))
    d_idx = up(torch, np.arange(8, dtype=np.uint64))
    out = Out(torch, 8 * 40)
    src, idx = d_src.data_ptr(), d_idx.data_ptr()
    for w in (1, 2, 3, 5, 6, 7, 33, 34, 35):
        assert ku.ku_gather_rows(src, idx, 8, w, out.ptr) == HIP_INVALID, w
    for a in (1, 2, 3):
        assert ku.ku_gather_rows(src + a, idx, 8, 32, out.ptr) == HIP_INVALID and ku.ku_gather_rows(src, idx, 8, 32, out.ptr + a) == HIP_INVALID, a
    assert ku.ku_gather_rows(src + 1, idx, 0, 33, out.ptr + 1) == 0               # no rows: nothing to refuse
    bad = []
    out.check(out.prefill(), "refused gathers", bad)
    assert not bad, bad
    assert ku.ku_gather_rows(src + 4, idx, 8, 36, out.ptr + 4) == 0               # 4-byte alignment is enough
    want = out.prefill().copy()
    flat = source_rows(16, 40).reshape(-1)
    for r in range(8):
        want[4 + 36 * r:4 + 36 * (r + 1)] = flat[4 + 36 * r:4 + 36 * (r + 1)]
    out.check(want, "gather at 4-byte alignment", bad)
    assert not bad, bad


def test_gather_addr(ku, torch_, capsys):
    torch, t0, bad, plan = torch_, time.time(), [], K.gather_addr_plan()
    for no, (w, a, n) in enumerate(plan):
        what = "gather_addr row_bytes=%d out offset=%d nrows=%d (%s)" % (w, a, n, "words" if K.gather_addr_wordwise(w, a) else "bytes")
        rng = np.random.default_rng([0xADD2, no])
        nsrc = 997 if n > 2 else 3
        src, idx = source_rows(nsrc, w), index_list(rng, n, nsrc)
        d_src = up(torch, src)
        addr = np.where(idx == K.PAD_ROW, np.uint64(0), np.uint64(d_src.data_ptr()) + idx * np.uint64(w))
        live = addr[addr != 0]
        assert live.min() >= d_src.data_ptr() and live.max() + w <= d_src.data_ptr() + src.size and (addr == 0).any() == (n > 3)
        d_addr = up(torch, addr)
        out = Out(torch, n * w, offset=a)
        assert out.ptr % 4 == a
        status = ku.ku_gather_addr(d_addr.data_ptr(), n, w, out.ptr)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        out.fetch()
        out.check(gathered(src, idx), what, bad, w, named(idx, out.got[out.lo:], w))
    report(capsys, "gather addr", len(plan), bad, t0)


# ---- k_compress_layer ------------------------------------------------------------------------------------------------------------------
def test_compress_layer_with_gaps_between_segments(ku, torch_, oracle, capsys):
    """Expected rows from the C oracle's compress, taken many states at a time (tests/test_kernel_models_cpu.py holds the batched call
    against compress itself).  Gap rows of the input hold bytes no field element has (all ones); gap rows of the output must stay."""
    torch, t0, bad, plan = torch_, time.time(), [], K.layer_plan()
    C, _ = oracle
    expected = {}
    for no, (m, nseg, bottom, istride, ostride) in enumerate(plan):
        what = "compress_layer m_in=%d nseg=%d bottom=%d strides=%d/%d" % (m, nseg, bottom, istride, ostride)
        m_out = (m + 1) // 2
        if (m, nseg, bottom) not in expected:
            rng = np.random.default_rng([0xC1A7, m, nseg, bottom])
            rows = canonical_rows(rng, nseg * m).reshape(nseg, m, 32)
            states = np.zeros((nseg, m_out, 3, 32), dtype=np.uint8)
            states[:, :, 0] = rows[:, 0::2]
            states[:, :m // 2, 1] = rows[:, 1::2]
            states[:, :, 2, 0] = bottom
            if m % 2:
                states[:, m_out - 1, 2, 0] = bottom + 2
            expected = {(m, nseg, bottom): (rows, C.permute_batch(states.reshape(-1, 96), threads=ORACLE_THREADS)[:, :32].reshape(nseg, m_out, 32))}
            for seg, j in ((0, 0), (nseg - 1, m_out - 1)):                   # and two of them one at a time
                x, y = rows[seg, 2 * j], rows[seg, 2 * j + 1] if 2 * j + 1 < m else np.zeros(32, np.uint8)
                assert np.array_equal(expected[(m, nseg, bottom)][1][seg, j], C.compress(x, y, bottom + (0 if 2 * j + 1 < m else 2)))
        rows, want_rows = expected[(m, nseg, bottom)]
        src = np.full((nseg, istride, 32), 0xFF, dtype=np.uint8)
        src[:, :m] = rows
        d_src = up(torch, src)
        out = Out(torch, nseg * ostride * 32)
        want = out.prefill().copy().reshape(nseg, ostride, 32)
        want[:, :m_out] = want_rows
        status = ku.ku_compress_layer(d_src.data_ptr(), out.ptr, m, nseg, bottom, istride, ostride)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        out.check(want, what, bad, 32, lambda r: " (segment %d node %d of %d)" % (r // ostride, r % ostride, m_out))
    report(capsys, "compress layer", len(plan), bad, t0)


# ---- k_gen_fake_cells_many ---------------------------------------------------------------------------------------------------------------
def test_gen_fake_cells_many_every_write_out_path(ku, torch_, oracle, capsys):
    """64 guard bytes before the output and a whole workgroup's cells of room after it, so that a store by a lane without a row lands in
    compared memory.  cell_size % 128 == 0 into a 16-byte-aligned pointer goes through LDS, everything else byte by byte."""
    torch, t0, bad, plan = torch_, time.time(), [], K.fake_many_plan()
    C, _ = oracle
    nmax = max(K.FAKE_ROWS)
    groups = [K.fake_group(g) for g in range(nmax)]
    d_seeds, d_firsts = up(torch, np.array([s for s, _ in groups], dtype=np.uint64)), up(torch, np.array([f for _, f in groups], dtype=np.uint64))
    want_all = {}
    for (per, n, cs, a) in plan:
        what = "gen_fake_cells_many per=%d n_rows=%d cell_size=%d out offset=%d" % (per, n, cs, a)
        if (per, cs) not in want_all:
            want_all[(per, cs)] = np.concatenate([C.gen_fake_cells(groups[g][0], groups[g][1], min(per, nmax - g * per), cs)
                                                  for g in range((nmax + per - 1) // per)])
        buf = Out(torch, n * cs, offset=a - (FRONT - 64), back=256 * cs + 256)
        assert buf.lo == 64 + a and buf.ptr % 16 == a
        status = ku.ku_gen_fake_cells_many(d_seeds.data_ptr(), d_firsts.data_ptr(), per, n, cs, buf.ptr)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        buf.check(want_all[(per, cs)][:n], what, bad, cs, lambda r: " (group %d, cell %d of it)" % (r // per, r % per))
    report(capsys, "fake cells, many seeds", len(plan), bad, t0)


# ---- k_gen_fake_cells ----------------------------------------------------------------------------------------------------------------------
def test_gen_fake_cells_index_mapping_and_write_out(ku, torch_, oracle, capsys):
    """Lane t makes global cell list[t] or first + t; kernel_models.fake_cell_of says which cell of which slot that is, the C oracle what
    that cell holds under the seed seed0 + 1001 * slot (mod 2^64).  The output lies as in the test above: 64 guard bytes before it, a
    whole workgroup's cells of room after it.  n_cells == 0 and cell_size == 0 are no work: success, nothing touched."""
    torch, t0, bad, plan = torch_, time.time(), [], K.fake_single_plan()
    C, _ = oracle
    cell_of = {}
    for c in plan:
        what = "gen_fake_cells n=%d cell_size=%d out offset=%d cells_per_slot=%d first=%d units=%d/%d %s seed0=%d" % (
            c.n, c.cell_size, c.offset, c.cells_per_slot, c.first, c.units_per_slot, c.first_unit, "list" if c.listed else "range", c.seed0)
        cells = K.fake_single_cells(c)
        want = np.empty((c.n, c.cell_size), dtype=np.uint8)
        for t, g in enumerate(cells):
            slot, idx = K.fake_cell_of(g, c.cells_per_slot, c.units_per_slot, c.first_unit)
            key = ((c.seed0 + 1001 * slot) % (1 << 64), idx, c.cell_size)
            if key not in cell_of:
                cell_of[key] = C.gen_fake_cells(key[0], idx, 1, c.cell_size)[0]
            want[t] = cell_of[key]
        d_list = up(torch, np.array(cells, dtype=np.uint64)) if c.listed else None
        buf = Out(torch, c.n * c.cell_size, offset=c.offset - (FRONT - 64), back=256 * c.cell_size + 256)
        assert buf.lo == 64 + c.offset and buf.ptr % 16 == c.offset
        status = ku.ku_gen_fake_cells(c.seed0, c.cells_per_slot, c.first, d_list.data_ptr() if c.listed else None, c.n, c.cell_size, buf.ptr,
                                      c.units_per_slot, c.first_unit)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        buf.check(want, what, bad, c.cell_size, lambda t: " (global cell %d = cell %d of slot %d)" % ((cells[t],) + K.fake_cell_of(
            cells[t], c.cells_per_slot, c.units_per_slot, c.first_unit)[::-1]))
    buf = Out(torch, 4 * 128, offset=-(FRONT - 64), back=256 * 128 + 256)
    for n, cs in ((0, 128), (4, 0), (0, 0)):
        status = ku.ku_gen_fake_cells(12417, 3, 7, None, n, cs, buf.ptr, 2, 5)
        if status != 0:
            bad.append("gen_fake_cells n=%d cell_size=%d: status %d" % (n, cs, status))
    buf.check(buf.prefill(), "gen_fake_cells without work", bad)
    report(capsys, "fake cells, index mapping", len(plan), bad, t0)


# ---- k_block_path_roots, k_block_path_commit ---------------------------------------------------------------------------------------------
def walk_requests(C, n_blocks):
    """The requests of K.walk_plan(n_blocks) over one random tree: (plan, fresh, paths, pairs, slot_roots, depth, expected verdicts)."""
    rng = np.random.default_rng([0xB10C, n_blocks])
    layers = C.merkle_tree(canonical_rows(rng, n_blocks))
    depth = len(layers) - 1
    assert [len(x) for x in layers] == K.layer_sizes(n_blocks)
    root = layers[-1][0]
    plus_r = np.frombuffer((as_int(root) + K.R_MOD).to_bytes(32, "little"), dtype=np.uint8)            # below 2^256
    slot_roots = np.stack([root, plus_r, canonical_rows(rng, 1)[0]])
    canon_roots = [root, root, slot_roots[2]]
    plan = K.walk_plan(n_blocks)
    fresh, paths = np.empty((len(plan), 32), np.uint8), np.zeros((len(plan), depth, 32), np.uint8)
    pairs, want = np.empty((len(plan), 2), np.uint64), np.empty(len(plan), np.uint32)
    for i, q in enumerate(plan):
        j = q.block
        fresh[i] = layers[0][j]
        for lvl in range(depth):
            if (j ^ 1) < len(layers[lvl]):
                paths[i, lvl] = layers[lvl][j ^ 1]
            j >>= 1
        if q.kind == "sibling":
            flip(paths[i], q.level, (q.block * 7 + q.level * 13) % 248)
        elif q.kind == "fresh":
            flip(fresh, i, (q.block * 11 + 5) % 248)
        assert as_int(fresh[i]) < K.R_MOD and all(as_int(p) < K.R_MOD for p in paths[i])
        pairs[i] = (q.root, q.index)
        reached = K.walk_model(fresh[i], q.index, n_blocks, list(paths[i]), C.compress)
        want[i] = 0 if np.array_equal(reached, canon_roots[q.root]) else 1
        assert want[i] == (0 if q.kind == "true" else 1), q           # the plan's own claim, confirmed by the model
    return plan, fresh, paths, pairs, slot_roots, depth, want


@pytest.fixture(scope="module")
def walks(oracle):
    C, _ = oracle
    return {n: walk_requests(C, n) for n in K.WALK_N_BLOCKS}


def test_block_path_roots_at_every_position(ku, torch_, walks, capsys):
    torch, t0, bad, cases = torch_, time.time(), [], 0
    for n_blocks, (plan, fresh, paths, pairs, slot_roots, depth, want) in walks.items():
        what = "block_path_roots n_blocks=%d" % n_blocks
        n = len(plan)
        cases += n
        d = [up(torch, x) for x in (fresh, paths, pairs, slot_roots)]
        name = lambda i: " (%s)" % (plan[i],)      # noqa: E731
        for with_roots in (True, False):
            verdict, roots_out = Out(torch, n * 4), Out(torch, n * 32)
            status = ku.ku_block_path_roots(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n_blocks, depth, n, verdict.ptr,
                                            roots_out.ptr if with_roots else None)
            if status != 0:
                bad.append("%s: status %d" % (what, status))
                break
            verdict.check(want, what + " verdicts", bad, 4, name)
            roots_out.check(fresh if with_roots else roots_out.prefill(), what + " roots_out", bad, 32, name)
    report(capsys, "block path roots", cases, bad, t0)


def test_block_path_commit_stores_what_it_proved_and_nothing_else(ku, torch_, walks, capsys):
    """dest a permutation of the rows; every second matching request once more with the same dest; one matching request with
    dest == n_rows, a backed row.  layer0 row for row: the fresh row where a matching request names it, the pre-fill everywhere else."""
    torch, t0, bad, cases = torch_, time.time(), [], 0
    for n_blocks, (plan, fresh, paths, pairs, slot_roots, depth, want) in walks.items():
        what = "block_path_commit n_blocks=%d" % n_blocks
        rng = np.random.default_rng([0xC0FF, n_blocks])
        n_rows = len(plan)
        dest = rng.permutation(n_rows).astype(np.uint64)
        match = np.nonzero(want == 0)[0]
        again = np.concatenate([match[::2], match[:1]])                # duplicates, then the request aimed at row n_rows
        fresh2, paths2, pairs2 = (np.concatenate([x, x[again]]) for x in (fresh, paths, pairs))
        dest2 = np.concatenate([dest, dest[again]])
        dest2[-1] = n_rows
        want2 = np.concatenate([want, want[again]])
        want2[-1] = 1
        n = len(dest2)
        cases += n
        d = [up(torch, x) for x in (fresh2, paths2, pairs2, slot_roots, dest2)]
        verdict, layer0 = Out(torch, n * 4), Out(torch, (n_rows + 1) * 32)
        want_rows = layer0.prefill().copy().reshape(n_rows + 1, 32)
        want_rows[dest[match].astype(np.int64)] = fresh[match]
        status = ku.ku_block_path_commit(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), n_blocks, depth, n,
                                         verdict.ptr, layer0.ptr, n_rows)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        verdict.check(want2, what + " verdicts", bad, 4, lambda i: " (%s, dest %d of %d)" % (plan[i] if i < n_rows else "repeat", int(dest2[i]), n_rows))
        layer0.check(want_rows, what + " layer0", bad, 32)
    report(capsys, "block path commit", cases, bad, t0)


# ---- k_verify_samples ------------------------------------------------------------------------------------------------------------------
def run_verify_launch(ku, torch, launch, bad):
    """One launch of the plan: the inputs packed as VerifyGeom documents, every byte of ok against tests/circuit_verdict.py (and against
    what the plan itself states for that input), the guards around ok, and the four input arrays read back unchanged."""
    md, bd, m, nf = launch.geom
    n, ns = len(launch.items), launch.ns
    what = "verify_samples %s (n=%d)" % (launch.name, n)
    arrays = K.verify_pack([it.d for it in launch.items], launch.geom)
    want = np.empty(n * ns + n, dtype=np.uint8)
    for i, it in enumerate(launch.items):
        e = K.verify_expected(it.d, launch.geom)
        assert it.expect is None or it.expect == e, (launch.name, it.tag)
        want[i * ns:(i + 1) * ns], want[n * ns + i] = e[:ns], e[ns]
    dev = [up(torch, a) for a in arrays]
    ptrs = [t.data_ptr() if t.numel() else None for t in dev]
    assert ptrs[0] and ptrs[1] and (ns == 0) == (ptrs[2] is None) == (ptrs[3] is None)
    ok = Out(torch, n * ns + n)
    g = VerifyGeom(n, ns, nf, md, m, bd)
    status = ku.ku_verify_samples(ctypes.byref(g), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ok.ptr)
    if status != 0:
        bad.append("%s: status %d" % (what, status))
        return 0
    body = ok.fetch()
    if not ok.guards_ok():
        bad.append("%s: bytes around ok changed" % what)
    wrong = np.nonzero(body != want)[0]
    for t in wrong[:8].tolist():
        i, lane = (t - n * ns, "dataset root") if t >= n * ns else (t // ns, "sample %d" % (t % ns))
        bad.append("%s: lane %d = input %d [%s], %s: device %#04x, the circuit %#04x (%d lanes differ)" % (
            what, t, i, launch.items[i].tag, lane, int(body[t]), int(want[t]), wrong.size))
    for name, a, t in zip(("prm", "heads", "cells", "paths"), arrays, dev):
        if not np.array_equal(t.cpu().numpy(), a.view(np.uint8).reshape(-1)):
            bad.append("%s: the kernel changed %s" % (what, name))
    return n * ns + n


def run_verify_launches(ku, torch_, capsys, name, launches):
    t0, bad = time.time(), []
    lanes = sum(run_verify_launch(ku, torch_, x, bad) for x in launches)
    with capsys.disabled():
        print("\n[kernel units] %s: %d launches, %d lanes" % (name, len(launches), lanes))
    report(capsys, name, K.verify_plan_cases(launches), bad, t0)


def verify_name(gi):
    return "verify samples, geometry %d" % gi


@pytest.mark.parametrize("gi", range(len(K.VERIFY_GEOMS)), ids=["-".join(map(str, g)) for g in K.VERIFY_GEOMS])
def test_verify_samples_every_depth_in_one_launch_and_every_felt(ku, torch_, capsys, gi):
    """Accepted inputs of every nCellsPerSlot = 2^1..2^maxDepth side by side in one launch, over several (nSlots, slotIndex), with the
    sampled index at 0, at nCells - 1 and at a block's last cell; and of each one copy per cell felt, path level, slot-proof level and
    head felt, that felt + 1: a felt the circuit reads clears its own byte, one it does not read clears none."""
    run_verify_launches(ku, torch_, capsys, verify_name(gi), [K.verify_geometry_launch(gi)])


VERIFY_TOP_RUNS = tuple((m, 0) for m in K.VERIFY_TOP_M) + ((3, 2),)


@pytest.mark.parametrize("m,ns", VERIFY_TOP_RUNS, ids=["m%d-ns%d" % r for r in VERIFY_TOP_RUNS])
def test_verify_samples_top_walk_over_every_slot_count_and_index(ku, torch_, capsys, m, ns):
    """Every nSlots <= 2^m with every slotIndex < 2^m, past nSlots too (rejected with the true root, accepted with the one the circuit
    reaches); ns == 0: a launch of top lanes only, cells and paths NULL."""
    run_verify_launches(ku, torch_, capsys, "verify samples, top walk m=%d ns=%d" % (m, ns), [K.verify_top_launch(m, ns)])


def test_verify_samples_field_edges_lane_layouts_and_refused_shapes(ku, torch_, capsys):
    """Cells and siblings at the field's edges with the compared root off by one and in bit 253; launches of 1, 255, 256, 257 and 513
    lanes whose first top lane falls on, after and before a wave's first lane and on a workgroup's; refused inputs full of 0xFF bytes."""
    run_verify_launches(ku, torch_, capsys, "verify samples, edges, layouts, refused", [K.verify_edge_launch()] + K.verify_layout_launches() + [K.verify_refused_launch()])


def test_verify_samples_no_inputs_no_work(ku, torch_):
    launch = K.verify_geometry_launch(2)
    arrays = K.verify_pack([it.d for it in launch.items[:2]], launch.geom)
    dev = [up(torch_, a) for a in arrays]
    ok = Out(torch_, 2 * launch.ns + 2)
    md, bd, m, nf = launch.geom
    g = VerifyGeom(0, launch.ns, nf, md, m, bd)
    assert ku.ku_verify_samples(ctypes.byref(g), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), ok.ptr) == 0
    bad = []
    ok.check(ok.prefill(), "ok", bad)
    assert not bad, bad


def test_summary():
    """Runs last in this module: every plan ran whole."""
    walk = sum(len(K.walk_plan(n)) for n in K.WALK_N_BLOCKS)
    want = {"scrub compare": len(K.scrub_plan()), "repair compare": len(K.repair_plan()), "sample paths / sample many": len(K.sample_plan()),
            "sample many, compact": len(K.compact_plan()), "gather rows": len(K.gather_rows_plan()), "gather addr": len(K.gather_addr_plan()),
            "compress layer": len(K.layer_plan()), "fake cells, many seeds": len(K.fake_many_plan()), "fake cells, index mapping": len(K.fake_single_plan()),
            "block path roots": walk}
    want.update({verify_name(gi): len(K.verify_geometry_launch(gi).items) for gi in range(len(K.VERIFY_GEOMS))})
    want.update({"verify samples, top walk m=%d ns=%d" % (m, ns): len(K.verify_top_launch(m, ns).items) for m, ns in VERIFY_TOP_RUNS})
    want["verify samples, edges, layouts, refused"] = K.verify_plan_cases([K.verify_edge_launch()] + K.verify_layout_launches() + [K.verify_refused_launch()])
    assert sum(n for name, n in want.items() if name.startswith("verify samples")) == K.verify_plan_cases()
    for name, n in want.items():
        assert TALLY.get(name) == n, name
    assert TALLY.get("block path commit", 0) > walk
    print("kernel units on the device: %d cases, 0 skipped" % sum(TALLY.values()))
