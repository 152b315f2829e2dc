"""GPU suite: launch_scatter_rows_addr on its own (csrc/kernels.hpp), through the forwarder of tests/device_check/build_many_unit.hip.

cp2_datasets_build_many reaches k_scatter_rows_addr only behind a host that builds every address from a dataset's layout; here the
launcher gets its inputs directly.  The items of a case are scattered over up to five allocations in shuffled order, the first of an
allocation 16 bytes past a 32-byte boundary and 48 bytes between one item and the next, as tests/test_gpu_scrub_many_unit.py places them
(multiples of 16 throughout; every other item of an allocation is no multiple of 32, which the 48 bytes make of the ones between);
every allocation is compared WHOLE with build_many_models.scatter_model,
so the bytes between two items, the guard bytes in front and what follows an item's last row must keep their pattern, and the source must
be unchanged.  Every case runs again with every third item's address 0 (those destinations stay untouched) and in slices of 1, 100 and
rows * n_items - 1 rows (the same result as the unsliced launch).

Shapes: rows in {1, 3, 16, 64}, sstride in {rows, rows + 1, rows + 6}, item counts that give 1, 63, 64, 65, 4095, 4096, 4097 and 8193
rows (where rows does not divide a total, the item counts on either side of it)."""
import collections
import ctypes
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import build_many_models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libbuild_many_unit.so")
HIP_INVALID = 1                               # hipErrorInvalidValue
TOTALS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
ROWS = (1, 3, 16, 64)
EXTRA = (0, 1, 6)                             # sstride - rows
Case = collections.namedtuple("Case", "no rows sstride n_items")


@pytest.fixture(autouse=True)
def time_limit():
    """every test under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def plan():
    cases = []
    for rows in ROWS:
        counts = sorted({n for t in TOTALS for n in (t // rows, -(-t // rows)) if n})
        for n in counts:
            for extra in EXTRA:
                cases.append(Case(len(cases), rows, rows + extra, n))
    return cases


def test_the_plan_holds_the_shapes_it_claims():
    cases = plan()
    assert set(TOTALS) <= {c.rows * c.n_items for c in cases} and {c.rows for c in cases} == set(ROWS)
    for rows in ROWS:
        assert {c.sstride - c.rows for c in cases if c.rows == rows} == set(EXTRA)
        for t in TOTALS:
            assert {t // rows, -(-t // rows)} - {0} <= {c.n_items for c in cases if c.rows == rows}
    assert any(c.rows == 64 and c.n_items == 65 for c in cases)              # 4160 rows: more than one workgroup's worth many times over


@pytest.fixture(scope="module")
def bmu(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libbuild_many_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.bmu_scatter_rows_addr.restype, lib.bmu_scatter_rows_addr.argtypes = ctypes.c_int, [vp, sz, vp, sz, sz, sz]
    return lib


@pytest.fixture(scope="module")
def torch_(bmu):
    import torch
    yield torch
    torch.cuda.synchronize()


def up(torch, arr):
    a = np.array(arr, copy=True, order="C")
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


class Scattered:
    """The destinations of one case: its items over up to five allocations, shuffled, each 16 bytes past a 32-byte boundary with 48 bytes
    to the next; `images` are the allocations' initial bytes (a pattern, never what the source holds), one flat model memory beside them."""

    def __init__(self, c):
        rng = np.random.default_rng([0xB11E, c.no])
        self.c = c
        self.src = rng.integers(0, 256, size=(c.n_items * c.sstride, 32), dtype=np.uint8)
        n_alloc = min(5, c.n_items)
        owner = rng.integers(0, n_alloc, size=c.n_items)
        owner[rng.permutation(c.n_items)[:n_alloc]] = np.arange(n_alloc)
        self.span = c.rows * 32 + 48
        self.images, self.at, self.owner = [], np.zeros(c.n_items, np.int64), owner
        for a in range(n_alloc):
            mine = rng.permutation(np.nonzero(owner == a)[0])
            self.images.append(rng.integers(0, 256, size=16 + mine.size * self.span + 16, dtype=np.uint8))
            self.at[mine] = 16 + np.arange(mine.size, dtype=np.int64) * self.span
        self.start = np.concatenate([[0], np.cumsum([img.size for img in self.images])])[:-1] + 4096     # (model addresses: never 0)

    def model(self, zero_every_third):
        """the allocations after the scatter, by the model"""
        c = self.c
        mem = np.concatenate([np.zeros(4096, np.uint8)] + self.images)
        addr = self.start[self.owner] + self.at
        if zero_every_third:
            addr[::3] = 0
        M.scatter_model(self.src, c.sstride, mem, addr, c.rows, c.n_items)
        assert not mem[:4096].any()
        return [mem[s:s + img.size] for s, img in zip(self.start, self.images)]

    def run(self, torch, lib, zero_every_third, slice_rows, bad, what):
        c = self.c
        dev = [up(torch, img) for img in self.images]
        assert all(t.data_ptr() % 32 == 0 for t in dev)
        addr = np.array([dev[o].data_ptr() for o in self.owner], dtype=np.uint64) + self.at.astype(np.uint64)
        assert (addr % 16 == 0).all() and (addr[self.at == 16] % 32 == 16).all() and (c.n_items < 6 or (addr % 32 == 0).any())
        if zero_every_third:
            addr[::3] = 0
        d_src, d_addr = up(torch, self.src), up(torch, addr)
        st = lib.bmu_scatter_rows_addr(d_src.data_ptr(), c.sstride, d_addr.data_ptr(), c.rows, c.n_items, slice_rows)
        torch.cuda.synchronize()
        if st != 0:
            bad.append("%s: status %d" % (what, st))
            return
        for a, (t, want) in enumerate(zip(dev, self.model(zero_every_third))):
            got = t.cpu().numpy()
            if not np.array_equal(got, want):
                i = int(np.nonzero(got != want)[0][0])
                bad.append("%s: allocation %d: %d bytes differ, first at byte %d of %d" % (what, a, int((got != want).sum()), i, got.size))
        if not np.array_equal(d_src.cpu().numpy().reshape(-1, 32), self.src):
            bad.append("%s: the source changed" % what)


def test_scattered_items_against_the_model_with_zero_addresses_and_slices(bmu, torch_, capsys):
    torch, bad, cases, runs = torch_, [], plan(), 0
    for c in cases:
        s = Scattered(c)
        total = c.rows * c.n_items
        for zero, sl in [(False, 0), (True, 0)] + [(False, x) for x in sorted({1, 100, total - 1}) if x > 0]:
            what = "rows=%d sstride=%d n_items=%d zero=%s slice=%d" % (c.rows, c.sstride, c.n_items, zero, sl)
            s.run(torch, bmu, zero, sl, bad, what)
            runs += 1
    with capsys.disabled():
        print("\n[build many unit] %d cases, %d launches checked, 0 skipped, %d failed" % (len(cases), runs, len(bad)))
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:100]))


def test_refusals_and_no_work(bmu, torch_):
    torch = torch_
    src = np.arange(8 * 32, dtype=np.uint8).reshape(8, 32)
    d_src = up(torch, src)
    pre = np.full(16 + 2 * (4 * 32 + 48), 0xA7, dtype=np.uint8)
    dst = up(torch, pre)
    p, q = d_src.data_ptr(), dst.data_ptr()
    table = up(torch, np.array([q + 16, q + 16 + 4 * 32 + 48], dtype=np.uint64))
    a = table.data_ptr()
    f = bmu.bmu_scatter_rows_addr
    assert f(p, 4, a, 4, 0, 0) == 0 and f(p, 4, a, 0, 2, 0) == 0 and f(None, 4, None, 0, 0, 0) == 0       # no items, no rows: no work
    assert f(p, 3, a, 4, 2, 0) == HIP_INVALID                                                                  # sstride < rows
    assert f(None, 4, a, 4, 2, 0) == HIP_INVALID and f(p, 4, None, 4, 2, 0) == HIP_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), pre) and np.array_equal(d_src.cpu().numpy().reshape(8, 32), src)  # outputs untouched
    assert f(p, 4, a, 4, 2, 0) == 0                                                                            # and the same arguments, valid
    torch.cuda.synchronize()
    want = pre.copy()
    want[16:16 + 128] = src[:4].reshape(-1)
    want[16 + 176:16 + 176 + 128] = src[4:].reshape(-1)
    assert np.array_equal(dst.cpu().numpy(), want)
