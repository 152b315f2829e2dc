"""GPU suite: launch_repair_compare_addr on its own (csrc/kernels.hpp), through the forwarders of tests/device_check/read_blocks_unit.hip.

cp2_datasets_read_blocks reaches k_repair_compare_addr only behind a host that builds every address from a dataset's layout; here the
launcher gets its inputs directly.  Each case runs the same fresh and kept rows through launch_repair_compare (the kept rows in one
buffer, a shuffled row index per request) and through launch_repair_compare_addr with the kept rows scattered over separate allocations
at addresses that are multiples of 16 and not of 32: the verdicts must be identical and equal to a numpy model.  The verdicts sit between
guard bytes that must not change.

Sizes: n in {1, 63, 64, 65, 255, 256, 257}, and 600 requests launched in slices of 256 (two whole slices and a part).  Planted: nothing,
request 0, the last request, a row that differs in its first 4 bytes only, one that differs in its last 4 bytes only; and a zero
address, which is a mismatch that is not read."""
import ctypes
import faulthandler
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libread_blocks_unit.so")
GUARD = 256
SIZES = ((1, 0), (63, 0), (64, 0), (65, 0), (255, 0), (256, 0), (257, 0), (600, 256))          # (n, slice)
PLANTED = ("none", "request 0", "last request", "first 4 bytes", "last 4 bytes")
N_ALLOC = 5


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def rbu(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libread_blocks_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.rbu_repair_compare.restype, lib.rbu_repair_compare.argtypes = i32, [vp, vp, sz, vp, sz, vp]
    lib.rbu_repair_compare_addr.restype, lib.rbu_repair_compare_addr.argtypes = i32, [vp, vp, sz, vp, sz]
    return lib


def up(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def planted_at(n, planted):
    return {"none": None, "request 0": 0, "last request": n - 1, "first 4 bytes": n // 2, "last 4 bytes": n // 3}[planted]


@pytest.mark.parametrize("planted", PLANTED)
@pytest.mark.parametrize("n,slice_", SIZES)
def test_addr_form_beside_index_form(rbu, n, slice_, planted):
    import torch
    rng = np.random.default_rng(n * 7 + PLANTED.index(planted))
    fresh = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kept = fresh.copy()
    at = planted_at(n, planted)
    if at is not None:
        if planted == "first 4 bytes":
            kept[at, 1] ^= 0x10
        elif planted == "last 4 bytes":
            kept[at, 30] ^= 0x01
        else:
            kept[at, int(rng.integers(0, 32))] ^= 0x80
    want = (fresh != kept).any(axis=1).astype(np.uint32)
    assert int(want.sum()) == (0 if at is None else 1)
    # index form: the kept rows shuffled inside one buffer among rows nobody asks for
    where = rng.permutation(2 * n + 3)[:n].astype(np.uint64)
    one = rng.integers(0, 256, (2 * n + 3, 32), dtype=np.uint8)
    one[where] = kept
    d_fresh, d_one, d_where = up(torch, fresh), up(torch, one), up(torch, where)
    # address form: the kept rows dealt over N_ALLOC allocations, row j of an allocation at its base + 16 + 64 * j
    owner = rng.integers(0, N_ALLOC, n)
    hosts = [rng.integers(0, 256, 16 + 64 * (int((owner == a).sum()) + 1), dtype=np.uint8) for a in range(N_ALLOC)]
    offs, seen = np.zeros(n, dtype=np.int64), [0] * N_ALLOC
    for i in range(n):
        offs[i] = 16 + 64 * seen[owner[i]]
        seen[owner[i]] += 1
        hosts[owner[i]][offs[i]:offs[i] + 32] = kept[i]
    devs = [up(torch, h) for h in hosts]
    addr = np.array([devs[owner[i]].data_ptr() + int(offs[i]) for i in range(n)], dtype=np.uint64)
    assert all(int(a) % 16 == 0 and int(a) % 32 == 16 for a in addr)
    d_addr = up(torch, addr)
    pre = np.full(GUARD + 4 * n + GUARD, 0xA5, dtype=np.uint8)
    outs = [up(torch, pre), up(torch, pre)]
    assert rbu.rbu_repair_compare(d_fresh.data_ptr(), d_one.data_ptr(), one.shape[0], d_where.data_ptr(), n, outs[0].data_ptr() + GUARD) == 0
    assert rbu.rbu_repair_compare_addr(d_fresh.data_ptr(), d_addr.data_ptr(), n, outs[1].data_ptr() + GUARD, slice_) == 0
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    for g in got:
        assert np.array_equal(g[:GUARD], pre[:GUARD]) and np.array_equal(g[GUARD + 4 * n:], pre[GUARD + 4 * n:])
        assert np.array_equal(g[GUARD:GUARD + 4 * n].view(np.uint32), want)
    assert np.array_equal(got[0], got[1])


def test_a_zero_address_is_a_mismatch_and_nothing_to_launch_is_fine(rbu):
    import torch
    fresh = np.zeros((3, 32), dtype=np.uint8)                          # equal to what a read of address 0 could never be asked for
    kept = up(torch, np.zeros(64, dtype=np.uint8))
    addr = np.array([kept.data_ptr(), 0, kept.data_ptr() + 16], dtype=np.uint64)
    out = up(torch, np.full(12, 0xA5, dtype=np.uint8))
    d_fresh, d_addr = up(torch, fresh), up(torch, addr)
    assert rbu.rbu_repair_compare_addr(d_fresh.data_ptr(), d_addr.data_ptr(), 3, out.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint32).tolist() == [0, 1, 0]
    assert rbu.rbu_repair_compare_addr(d_fresh.data_ptr(), d_addr.data_ptr(), 0, out.data_ptr(), 0) == 0
    assert rbu.rbu_repair_compare_addr(None, d_addr.data_ptr(), 3, out.data_ptr(), 0) == 1          # hipErrorInvalidValue, nothing launched
