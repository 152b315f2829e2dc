"""GPU suite: launch_block_root_recheck_addr on its own, through tests/device_check/libfills_resume_many_unit.so, against a numpy model.
The kept rows of several "sessions" lie in ONE torch allocation with guard rows in front, between and behind; the verdict words have guards
too and are pre-filled.  The addresses come in a shuffled order, so that neighbouring lanes point into different sessions.  The whole
buffer is compared after every launch: differing rows are zeros, equal rows, guards and `fresh` are as they were, every verdict exact.
Nothing here provokes a fault: address 0 and a misaligned address are ordinary verdicts by the kernel's own rule."""
import ctypes
import faulthandler
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libfills_resume_many_unit.so")
GUARD_ROWS = 8                                     # 256 bytes between two sessions
FILL = 0xA5A5A5A5
SIZES = [1, 63, 64, 65, 255, 256, 257, 4097]


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def frmu(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libfills_resume_many_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.frmu_block_root_recheck_addr.restype = ctypes.c_int
    lib.frmu_block_root_recheck_addr.argtypes = [vp, vp, ctypes.c_size_t, vp]
    return lib


def model(fresh, rows_of, kept):
    """(verdict, kept after): lane i compares fresh[i] with kept[rows_of[i]]; 1 and the row zeroed where they differ; rows_of[i] < 0 (an
    address the kernel refuses): 1, nothing touched"""
    out = kept.copy()
    verdict = np.ones(len(rows_of), dtype=np.uint32)
    for i, r in enumerate(rows_of):
        if r < 0:
            continue
        if np.array_equal(fresh[i], kept[r]):
            verdict[i] = 0
        else:
            out[r] = 0
    return verdict, out


def world(rng, n, sessions=3):
    """one buffer of 32-byte rows: guard, session 0, guard, session 1, ..., guard.  Returns (the buffer, the buffer row of every kept row in
    a shuffled order: lane i judges row order[i])"""
    cut = sorted(int(x) for x in rng.integers(0, n + 1, sessions - 1))
    sizes = [b - a for a, b in zip([0] + cut, cut + [n])]
    rows, at = [], GUARD_ROWS
    for m in sizes:
        rows += list(range(at, at + m))
        at += m + GUARD_ROWS
    buf = rng.integers(1, 256, size=(at, 32), dtype=np.uint8)                          # never zero: a zeroed row shows
    order = [rows[i] for i in rng.permutation(n)]
    return buf, order


def damage(rng, fresh, which):
    """`which` lanes differ, each in one of three ways; returns the lanes that differ in the end"""
    lanes = set()
    n = len(fresh)
    for j, i in enumerate(which):
        kind = j % 3
        if kind == 0:
            fresh[i, 0] ^= 0x01                                                          # the lowest byte only
        elif kind == 1:
            fresh[i, 24 + int(rng.integers(0, 8))] ^= 0x80                               # the top limb only
        elif n > 1:
            o = i + 1 if i + 1 < n else i - 1                                            # swapped with a neighbour's fresh row
            fresh[[i, o]] = fresh[[o, i]]
            lanes.add(o)
        else:
            fresh[i, 17] ^= 0x10
        lanes.add(i)
    return lanes


def run(torch, lib, fresh, addr, buf, n):
    d_fresh = torch.from_numpy(fresh.reshape(-1).copy()).cuda()
    d_addr = torch.from_numpy(addr.view(np.uint8).copy()).cuda()
    vsent = np.full(n + 2 * GUARD_ROWS, FILL, dtype=np.uint32)
    d_verdict = torch.from_numpy(vsent.view(np.uint8).copy()).cuda()
    st = lib.frmu_block_root_recheck_addr(d_fresh.data_ptr(), d_addr.data_ptr(), n, d_verdict.data_ptr() + 4 * GUARD_ROWS)
    torch.cuda.synchronize()
    return st, d_fresh.cpu().numpy().reshape(-1, 32), d_verdict.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_the_launcher_alone(frmu, n):
    import torch
    rng = np.random.default_rng([0xADD4, n])
    for case in ("a quarter", "every row", "none"):
        buf, order = world(rng, n)
        fresh = buf[order].copy()
        which = {"a quarter": sorted(int(i) for i in rng.permutation(n)[:max(1, n // 4)]), "every row": list(range(n)), "none": []}[case]
        damage(rng, fresh, which)
        want_verdict, want_buf = model(fresh, order, buf)
        if case == "none":
            assert not want_verdict.any()
        if case == "every row":
            assert want_verdict.all()
        if case == "a quarter":
            assert 0 < int(want_verdict.sum()) <= 2 * max(1, n // 4)
        d_buf = torch.from_numpy(buf.reshape(-1).copy()).cuda()
        assert d_buf.data_ptr() % 16 == 0
        addr = np.array([d_buf.data_ptr() + 32 * r for r in order], dtype=np.uint64)
        assert len(set(addr.tolist())) == n
        st, got_fresh, got_verdict = run(torch, frmu, fresh, addr, buf, n)
        assert st == 0, case
        got_buf = d_buf.cpu().numpy().reshape(-1, 32)
        assert np.array_equal(got_buf, want_buf), (case, np.nonzero((got_buf != want_buf).any(axis=1))[0][:8])
        assert np.array_equal(got_fresh, fresh), case
        assert (got_verdict[:GUARD_ROWS] == FILL).all() and (got_verdict[GUARD_ROWS + n:] == FILL).all(), case
        assert np.array_equal(got_verdict[GUARD_ROWS:GUARD_ROWS + n], want_verdict), (case, np.nonzero(got_verdict[GUARD_ROWS:GUARD_ROWS + n] != want_verdict)[0][:8])


def test_address_zero_and_a_misaligned_address_are_mismatches_that_touch_nothing(frmu):
    import torch
    n = 65
    rng = np.random.default_rng(0xADD5)
    buf, order = world(rng, n)
    fresh = buf[order].copy()                                                            # every row equal: only the addresses decide
    d_buf = torch.from_numpy(buf.reshape(-1).copy()).cuda()
    addr = np.array([d_buf.data_ptr() + 32 * r for r in order], dtype=np.uint64)
    rows = list(order)
    for i in (0, 31, 64):
        addr[i], rows[i] = 0, -1
    for i in (1, 32, 63):
        addr[i] += 8                                                                     # inside the buffer, 8-byte aligned only
        rows[i] = -1
    want_verdict, want_buf = model(fresh, rows, buf)
    assert int(want_verdict.sum()) == 6 and np.array_equal(want_buf, buf)
    st, got_fresh, got_verdict = run(torch, frmu, fresh, addr, buf, n)
    assert st == 0
    assert np.array_equal(d_buf.cpu().numpy().reshape(-1, 32), buf) and np.array_equal(got_fresh, fresh)
    assert np.array_equal(got_verdict[GUARD_ROWS:GUARD_ROWS + n], want_verdict)
    assert (got_verdict[:GUARD_ROWS] == FILL).all() and (got_verdict[GUARD_ROWS + n:] == FILL).all()


def test_nothing_to_do_launches_nothing_and_null_tables_are_refused(frmu):
    import torch
    buf = np.full((4, 32), 7, dtype=np.uint8)
    d_buf = torch.from_numpy(buf.reshape(-1).copy()).cuda()
    d_addr = torch.from_numpy(np.array([d_buf.data_ptr()], dtype=np.uint64).view(np.uint8).copy()).cuda()
    d_verdict = torch.from_numpy(np.full(4, FILL, dtype=np.uint32).view(np.uint8).copy()).cuda()
    d_fresh = torch.from_numpy(np.zeros(32, dtype=np.uint8)).cuda()
    assert frmu.frmu_block_root_recheck_addr(d_fresh.data_ptr(), d_addr.data_ptr(), 0, d_verdict.data_ptr()) == 0
    assert frmu.frmu_block_root_recheck_addr(None, None, 0, None) == 0
    assert frmu.frmu_block_root_recheck_addr(None, d_addr.data_ptr(), 1, d_verdict.data_ptr()) == 1          # hipErrorInvalidValue
    assert frmu.frmu_block_root_recheck_addr(d_fresh.data_ptr(), None, 1, d_verdict.data_ptr()) == 1
    assert frmu.frmu_block_root_recheck_addr(d_fresh.data_ptr(), d_addr.data_ptr(), 1, None) == 1
    torch.cuda.synchronize()
    assert np.array_equal(d_buf.cpu().numpy().reshape(-1, 32), buf) and (d_verdict.cpu().numpy().view(np.uint32) == FILL).all()
