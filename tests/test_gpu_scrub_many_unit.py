"""GPU suite: launch_scrub_compare_many on its own (csrc/kernels.hpp), through the forwarders of tests/device_check/scrub_many_unit.hip.

cp2_datasets_scrub_many reaches k_scrub_compare_many only behind a host that builds every address from a dataset's layout; here the
launcher gets its inputs directly.  Each case first runs the same fresh and kept rows through launch_scrub_compare and -- with the
contiguous address table kept + i * kstride * 32 -- through launch_scrub_compare_many: bits and counts must be identical, and equal to
kernel_models.scrub_model.  Then the items are scattered over separate allocations in shuffled order, at addresses that are multiples
of 16 but not of 32, and the result is held against scrub_many_models.scrub_many_model.  Outputs sit between guard bytes: every word to
the end of the last tile is checked (zeros past the last row) and nothing around them may change.

Shapes: rows in {1, 3, 16, 64}, fstride >= rows, item counts that give 1, 63, 64, 65, 4095, 4096, 4097 and 2 * 4096 + 1 rows (where
rows does not divide a total, the item counts on either side of it); a single mismatch at the first and the last row of the first item,
on each side of the tile boundary, at the last row of the last item, one that differs in the last 4 bytes of a row only, and a clean
case."""
import collections
import ctypes
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import kernel_models as K
import scrub_many_models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libscrub_many_unit.so")
FRONT = 256
HIP_INVALID = 1                               # hipErrorInvalidValue
PATTERN = ((np.arange(4099, dtype=np.int64) * 7 + 0xC3) % 255 + 1).astype(np.uint8)     # never zero
TOTALS = (1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1)
LAYOUTS = ((1, 1, 2), (1, 2, 1), (3, 3, 3), (3, 5, 4), (16, 16, 16), (16, 17, 16), (64, 64, 64), (64, 64, 70))   # rows, fstride, kstride
PLANTED = ("none", "first row of item 0", "last row of item 0", "row 4095", "row 4096", "last row", "last 4 bytes")
Case = collections.namedtuple("Case", "no rows fstride kstride n_items planted")


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def planted_row(c):
    """the one row of the case that differs (None: clean, or the row does not exist in this shape)"""
    total = c.rows * c.n_items
    g = {"none": None, "first row of item 0": 0, "last row of item 0": c.rows - 1, "row 4095": 4095, "row 4096": 4096, "last row": total - 1,
         "last 4 bytes": total // 2}[c.planted]
    return g if g is not None and g < total else None


def plan():
    cases = []
    for rows, fs, ks in LAYOUTS:
        counts = sorted({n for t in TOTALS for n in (t // rows, -(-t // rows)) if n})
        for n in counts:
            for planted in PLANTED:
                c = Case(len(cases), rows, fs, ks, n, planted)
                if planted == "none" or planted_row(c) is not None:
                    cases.append(c)
    return cases


def test_the_plan_holds_the_edges_it_claims():
    cases = plan()
    totals = {c.rows * c.n_items for c in cases}
    assert set(TOTALS) <= totals and {c.rows for c in cases} == {1, 3, 16, 64}
    assert all(c.fstride >= c.rows and c.kstride >= c.rows for c in cases) and any(c.fstride > c.rows for c in cases)
    for planted in PLANTED:
        assert sum(1 for c in cases if c.planted == planted) >= 20, planted
    assert any(c.planted == "row 4096" and c.rows == 64 and c.n_items == 65 for c in cases)     # the seam between items 63 and 64


@pytest.fixture(scope="module")
def smu(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libscrub_many_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.smu_scrub_compare.restype, lib.smu_scrub_compare.argtypes = i32, [vp, sz, vp, sz, sz, sz, vp, vp]
    lib.smu_scrub_compare_many.restype, lib.smu_scrub_compare_many.argtypes = i32, [vp, sz, vp, sz, sz, vp, vp]
    lib.smu_scrub_tile.restype = sz
    assert lib.smu_scrub_tile() == K.SCRUB_TILE
    return lib


@pytest.fixture(scope="module")
def torch_(smu):
    import torch
    yield torch
    torch.cuda.synchronize()


def up(torch, arr):
    a = np.array(arr, copy=True, order="C")
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


class Out:
    """nbytes of output between FRONT guard bytes, all pre-filled with PATTERN; check() compares the whole buffer, guards included"""

    def __init__(self, torch, nbytes):
        self.torch, self.n = torch, nbytes
        self.pre = np.resize(PATTERN, FRONT + nbytes + FRONT)
        self.t = torch.from_numpy(self.pre.copy()).cuda()
        self.ptr = self.t.data_ptr() + FRONT

    def check(self, want, what, bad):
        self.torch.cuda.synchronize()
        got = self.t.cpu().numpy()
        expect = self.pre.copy()
        expect[FRONT:FRONT + self.n] = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        if not np.array_equal(got, expect):
            i = int(np.nonzero(got != expect)[0][0]) - FRONT
            bad.append("%s: %d bytes differ, first at byte %d of the output (negative: the guard before it)" % (what, int((got != expect).sum()), i))
        return got[FRONT:FRONT + self.n]


def case_arrays(c):
    """fresh and kept rows equal at every compared row and different everywhere else, then the case's one planted difference"""
    rng = np.random.default_rng([0x5CA7, c.no])
    total = c.rows * c.n_items
    fresh = rng.integers(0, 256, size=(c.n_items * c.fstride, 32), dtype=np.uint8)
    kept = rng.integers(0, 256, size=(c.n_items * c.kstride, 32), dtype=np.uint8)
    item, r = np.divmod(np.arange(total, dtype=np.int64), c.rows)
    kept[item * c.kstride + r] = fresh[item * c.fstride + r]
    g = planted_row(c)
    if g is not None:
        row = (g // c.rows) * c.kstride + g % c.rows
        byte = 28 + c.no % 4 if c.planted == "last 4 bytes" else (c.no * 5) % 32
        kept[row, byte] ^= np.uint8(1 << (c.no % 8))
    return fresh, kept


def test_equals_launch_scrub_compare_then_scattered_items_against_the_model(smu, torch_, capsys):
    torch, bad, cases = torch_, [], plan()
    for c in cases:
        what = "rows=%d fstride=%d kstride=%d n_items=%d planted=%s" % (c.rows, c.fstride, c.kstride, c.n_items, c.planted)
        total, g = c.rows * c.n_items, planted_row(c)
        groups = K.scrub_groups(total)
        fresh, kept = case_arrays(c)
        want_bits, want_counts = K.scrub_model(fresh, kept, c.rows, c.fstride, c.kstride, c.n_items)
        assert int(want_counts.sum()) == (0 if g is None else 1) and want_bits.size == groups * K.SCRUB_TILE // 64
        assert M.decode(want_bits, c.rows, c.n_items) == ([] if g is None else [(g // c.rows, g % c.rows)])
        d_fresh, d_kept = up(torch, fresh), up(torch, kept)
        # 1. the strided launcher and the address-table launcher over the same memory
        b1, c1, b2, c2 = Out(torch, want_bits.size * 8), Out(torch, groups * 4), Out(torch, want_bits.size * 8), Out(torch, groups * 4)
        st = smu.smu_scrub_compare(d_fresh.data_ptr(), c.fstride, d_kept.data_ptr(), c.kstride, c.rows, c.n_items, b1.ptr, c1.ptr)
        addr = np.uint64(d_kept.data_ptr()) + np.arange(c.n_items, dtype=np.uint64) * np.uint64(c.kstride * 32)
        d_addr = up(torch, addr)
        st2 = smu.smu_scrub_compare_many(d_fresh.data_ptr(), c.fstride, d_addr.data_ptr(), c.rows, c.n_items, b2.ptr, c2.ptr)
        if st != 0 or st2 != 0:
            bad.append("%s: status %d / %d" % (what, st, st2))
            continue
        got1 = b1.check(want_bits, what + ": launch_scrub_compare bits", bad)
        got2 = b2.check(want_bits, what + ": launch_scrub_compare_many bits", bad)
        cnt1 = c1.check(want_counts, what + ": launch_scrub_compare counts", bad)
        cnt2 = c2.check(want_counts, what + ": launch_scrub_compare_many counts", bad)
        if not (np.array_equal(got1, got2) and np.array_equal(cnt1, cnt2)):
            bad.append("%s: the two launchers differ" % what)
        # 2. the items scattered over up to five allocations, shuffled, 16 bytes past a 32-byte boundary, 48 bytes between them
        rng = np.random.default_rng([0x5CA8, c.no])
        n_alloc = min(5, c.n_items)
        owner = rng.integers(0, n_alloc, size=c.n_items)
        owner[rng.permutation(c.n_items)[:n_alloc]] = np.arange(n_alloc)
        images, dev, model_addr, dev_addr, base = [], [], np.zeros(c.n_items, np.int64), np.zeros(c.n_items, np.uint64), 0
        for a in range(n_alloc):
            mine = rng.permutation(np.nonzero(owner == a)[0])
            span = c.rows * 32 + 48
            img = rng.integers(0, 256, size=16 + mine.size * span, dtype=np.uint8)
            for place, item in enumerate(mine):
                at = 16 + place * span
                img[at:at + c.rows * 32] = kept[item * c.kstride:item * c.kstride + c.rows].reshape(-1)
                model_addr[item] = base + at
            t = up(torch, img)
            assert t.data_ptr() % 32 == 0
            for place, item in enumerate(mine):
                dev_addr[item] = t.data_ptr() + 16 + place * span
            images.append(img)
            dev.append(t)
            base += img.size
        m_bits, m_counts = M.scrub_many_model(fresh, c.fstride, np.concatenate(images), model_addr, c.rows, c.n_items)
        assert np.array_equal(m_bits, want_bits) and np.array_equal(m_counts, want_counts)     # (scattering changes nothing)
        b3, c3 = Out(torch, m_bits.size * 8), Out(torch, groups * 4)
        d_addr = up(torch, dev_addr)
        st3 = smu.smu_scrub_compare_many(d_fresh.data_ptr(), c.fstride, d_addr.data_ptr(), c.rows, c.n_items, b3.ptr, c3.ptr)
        if st3 != 0:
            bad.append("%s scattered: status %d" % (what, st3))
            continue
        b3.check(m_bits, what + " scattered: bits", bad)
        c3.check(m_counts, what + " scattered: counts", bad)
    with capsys.disabled():
        print("\n[scrub many unit] %d cases, 0 skipped, %d failed" % (len(cases), len(bad)))
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:100]))


def test_refusals_and_no_work(smu, torch_):
    torch = torch_
    rows = up(torch, np.zeros((8, 32), dtype=np.uint8))
    p = rows.data_ptr()
    table = up(torch, np.array([p, p + 4 * 32], dtype=np.uint64))
    a = table.data_ptr()
    bits, counts = Out(torch, K.SCRUB_TILE // 8), Out(torch, 4)
    f = smu.smu_scrub_compare_many
    assert f(p, 4, a, 4, 0, bits.ptr, counts.ptr) == 0 and f(p, 4, a, 0, 2, bits.ptr, counts.ptr) == 0          # no items, no rows: no work
    assert f(p, 3, a, 4, 2, bits.ptr, counts.ptr) == HIP_INVALID                                                  # fstride < rows
    assert f(None, 4, a, 4, 2, bits.ptr, counts.ptr) == HIP_INVALID and f(p, 4, None, 4, 2, bits.ptr, counts.ptr) == HIP_INVALID
    assert f(p, 4, a, 4, 2, None, counts.ptr) == HIP_INVALID and f(p, 4, a, 4, 2, bits.ptr, None) == HIP_INVALID
    bad = []
    bits.check(bits.pre[FRONT:FRONT + bits.n], "bits", bad)
    counts.check(counts.pre[FRONT:FRONT + counts.n], "counts", bad)
    assert not bad, bad
    assert f(p, 4, a, 4, 2, bits.ptr, counts.ptr) == 0                                                            # and the same arguments, valid
    bits.check(np.zeros(K.SCRUB_TILE // 64, dtype=np.uint64), "bits", bad)
    counts.check(np.zeros(1, dtype=np.uint32), "counts", bad)
    assert not bad, bad
