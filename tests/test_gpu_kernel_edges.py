"""GPU suite: the byte staging of k_hash_cells and the write-out of k_gen_fake_cells at every state they can take.

The arithmetic of the hash kernel is pinned elsewhere (reference KAT, 2^24 states against the C oracle, the host build of the
field headers).  This module sweeps what lies between global memory and the first to_mont: the three load branches, the 47-word
LDS ring at every base, the terminator and the sponge pad in every dword position, the parity of the consumed offset, the cells a
lane's 32 loads may touch -- through cp2_hash_cells_dev, at every cell size from 0 to 6200 and around 16384 and 65536 (there, at a = 0, with the smaller counts only: SMALL_COUNTS), at unaligned base pointers, with guard
rows around the output and two different fillings of the bytes around the input.  Every expected value comes from the C oracle
(tests/test_oracle_hash_edges.py holds that oracle against the Python big-int one at the same framing edges).

The plan of the sweep (which sizes, offsets and counts run) is made by plain functions and checked without a GPU by
test_sweep_plan; tests/hash_block_child.py imports the same functions for the 64-lane workgroup shape."""
import ctypes
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# ---- the plan --------------------------------------------------------------------------------------------------------------------
MAX_SIZE = 6200          # 47 lines of 128 B = 6016 B: the final line has had every ring base; + 184 B: every residue mod 124 meets the last bases
WINDOWS = (16384, 65536)
WINDOW_HALF = 70
BIG_CELL = (1 << 20) + 5
COUNTS = (1, 2, 63, 64, 65, 67, 127, 128, 129, 255, 256, 257, 511, 513)
# The 65536 window at a = 0 takes only the counts of the cycle up to 67 (waves 0 and 1 of one workgroup): what is NOT seen after ~520
# ring revolutions is an empty trailing wave and a second workgroup; the 16384 window (~130 revolutions) keeps the whole cycle.
# Cells per size at a != 0 are already at the 3..5 minimum, so this is the one place left where cells could be cut.
SMALL_COUNTS = COUNTS[:6]
OFFSETS = (0, 1, 2, 3)
WINDOW_OFFSETS = (0, 1, 2, 3, 4, 8, 13)
FILLS = (0xFF, 0x00, 0x01)
GUARD_EVERY = 16
CHILD_EVERY = 7
CHILD_COUNTS = (1, 65, 129)
CHILD_OFFSETS = (0, 1)

FRONT, TAIL, ALIGN = 64, 192, 256    # slack before the base pointer (plus the misalignment), after the last cell, region alignment
GUARD_ROWS = 4
GUARD_ROW = np.arange(32, dtype=np.uint8) * 7 + 0xC3
SLACK = np.random.default_rng(0x51AC).integers(0, 256, size=1024, dtype=np.uint8)
ORACLE_THREADS = 16
LAUNCH_STREAMS = 4


def count_for(size):
    """The cycle, shifted by one every 14 sizes: every count meets every residue of the size mod 4."""
    return COUNTS[(size + size // len(COUNTS)) % len(COUNTS)]


def small_count_for(size):
    return SMALL_COUNTS[(size + size // len(SMALL_COUNTS)) % len(SMALL_COUNTS)]


def misaligned_count(size, a):
    return 3 + (size + a) % 3        # three to five cells


def window_sizes(centre):
    return list(range(centre - WINDOW_HALF, centre + WINDOW_HALF + 1))


def fill_sizes():
    """For each (size mod 31 in {0, 29, 30}) x (size mod 4 in 0..3): the first such size above 124."""
    out = []
    for r31 in (0, 29, 30):
        for r4 in range(4):
            out.append(next(s for s in range(125, 125 + 124) if s % 31 == r31 and s % 4 == r4))
    return sorted(out)


def contiguous_cases():
    """(cell_size, a, n_cells, fill, complemented slack) of the contiguous sweep; fill None = seeded random bytes."""
    cases = []
    for s in range(MAX_SIZE + 1):
        for a in OFFSETS:
            n = count_for(s) if a == 0 else misaligned_count(s, a)
            cases.append((s, a, n, None, False))
            if s % GUARD_EVERY == 0:
                cases.append((s, a, n, None, True))
    for s in fill_sizes():
        for fill in FILLS:
            for a in OFFSETS:
                cases.append((s, a, 67 if a == 0 else misaligned_count(s, a), fill, False))
    return cases


def window_cases(centre):
    cases = []
    for s in window_sizes(centre):
        for a in WINDOW_OFFSETS:
            n = (count_for(s) if centre == WINDOWS[0] else small_count_for(s)) if a == 0 else misaligned_count(s, a)
            cases += [(s, a, n, None, False), (s, a, n, None, True)]
    return cases


def child_cases():
    sizes = list(range(0, MAX_SIZE + 1, CHILD_EVERY)) + window_sizes(WINDOWS[0])
    return [(s, a, n, None, False) for s in sizes for a in CHILD_OFFSETS for n in CHILD_COUNTS]


def distinct(cases):
    return len({(s, a, n) for (s, a, n, _, _) in cases})


def test_sweep_plan():
    """No GPU: the sweep covers what it says (sizes, offsets, counts against size mod 4, guard runs, fills)."""
    cc = contiguous_cases()
    rnd = [c for c in cc if c[3] is None and not c[4]]
    assert {(s, a) for (s, a, _, _, _) in rnd} == {(s, a) for s in range(MAX_SIZE + 1) for a in OFFSETS}
    assert {(n, s % 4) for (s, a, n, _, _) in rnd if a == 0} == {(n, r) for n in COUNTS for r in range(4)}
    assert {n for (s, a, n, _, _) in rnd if a} == {3, 4, 5}
    assert {s for (s, a, n, f, comp) in cc if comp} == set(range(0, MAX_SIZE + 1, GUARD_EVERY))
    fs = fill_sizes()
    assert len(fs) == 12 and min(fs) > 124 and {(s % 31, s % 4) for s in fs} == {(r, q) for r in (0, 29, 30) for q in range(4)}
    assert {(s, a, f) for (s, a, n, f, _) in cc if f is not None} == {(s, a, f) for s in fs for a in OFFSETS for f in FILLS}
    for centre in WINDOWS:
        wc = window_cases(centre)
        assert {(s, a, comp) for (s, a, _, _, comp) in wc} == {(s, a, c) for s in window_sizes(centre) for a in WINDOW_OFFSETS for c in (False, True)}
        assert {n for (s, a, n, _, _) in wc if a} == {3, 4, 5}
    assert {n for (s, a, n, _, _) in window_cases(WINDOWS[0]) if a == 0} == set(COUNTS)
    assert {(n, s % 4) for (s, a, n, _, _) in window_cases(WINDOWS[1]) if a == 0} == {(n, r) for n in SMALL_COUNTS for r in range(4)}
    # the ring base of the final line takes all 47 values inside the contiguous range
    bases = set()
    for s in range(MAX_SIZE + 1):
        nfelts = (s + 31) // 31
        stream = 31 * ((nfelts + 2) & ~1)
        bases.add((((stream + 127) // 128 - 1) * 32) % 47)
    assert bases == set(range(47))
    ch = child_cases()
    assert distinct(ch) == len(ch) == (len(range(0, MAX_SIZE + 1, CHILD_EVERY)) + 2 * WINDOW_HALF + 1) * len(CHILD_OFFSETS) * len(CHILD_COUNTS)


# ---- data and expected values ----------------------------------------------------------------------------------------------------
def cells_for(size, n, fill=None):
    """n cells of `size` bytes, flat.  Seeded by the size alone: the same bytes at every base offset and in the child process."""
    if fill is not None:
        return np.full(n * size, fill, dtype=np.uint8)
    return np.random.default_rng([0xED6E, size]).integers(0, 256, size=n * size, dtype=np.uint8)


def oracle_hashes(C, cells, size, n, fill=None):
    if size == 0:
        return np.tile(C.hash_bytes(b""), (n, 1))
    if fill is not None:                                          # equal cells: one digest
        return np.tile(C.hash_cells(cells[:size], size), (n, 1))
    return C.hash_cells(cells[:n * size], size, threads=1)


def make_size(C, size, n, fill=None):
    cells = cells_for(size, n, fill)
    return cells, oracle_hashes(C, cells, size, n, fill)


def cells_needed(cases):
    need = {}
    for (s, a, n, fill, _) in cases:
        need[(s, fill)] = max(need.get((s, fill), 0), n)
    return need


def chunks_of(need, limit=160 << 20):
    """Keys of `need` in order, cut so that a chunk's cell bytes stay below `limit`."""
    out, cur, used = [], [], 0
    for key in sorted(need, key=lambda k: (k[0], -1 if k[1] is None else k[1])):
        b = need[key] * key[0]
        if cur and used + b > limit:
            out.append(cur)
            cur, used = [], 0
        cur.append(key)
        used += b
    if cur:
        out.append(cur)
    return out


# ---- one batch on the device -----------------------------------------------------------------------------------------------------
def _up(x):
    return (x + ALIGN - 1) // ALIGN * ALIGN


def run_hash_batch(torch, ctx, items):
    """items: (cell_size, a, n_cells, fill, comp, cells, want).  One input buffer, one output buffer, every launch enqueued, one
    synchronise.  Around each case's cells lie FRONT + a bytes before the base pointer and at least TAIL after the last cell, taken
    from SLACK (comp: its complement); around its n_cells output rows lie GUARD_ROWS guard rows on each side.
    Returns the failures as strings."""
    lay, off, row = [], 0, 0
    for (s, a, n, fill, comp, cells, want) in items:
        lay.append((off, off + FRONT + a, _up(off + FRONT + a + n * s + TAIL), row + GUARD_ROWS))
        off, row = lay[-1][2], row + n + 2 * GUARD_ROWS
    host = np.empty(off, dtype=np.uint8)
    pre = np.tile(GUARD_ROW, (row, 1))
    exp = pre.copy()
    for (s, a, n, fill, comp, cells, want), (r0, p, r1, r) in zip(items, lay):
        pat = ~SLACK if comp else SLACK
        host[r0:p] = pat[:p - r0]
        host[p:p + n * s] = cells[:n * s]
        host[p + n * s:r1] = pat[512:512 + r1 - p - n * s]
        exp[r:r + n] = want[:n]
    d_in = torch.from_numpy(host).cuda()
    d_out = torch.from_numpy(pre).cuda()
    assert d_in.data_ptr() % ALIGN == 0 and d_out.data_ptr() % 16 == 0
    # A launch here is one to three workgroups whose time is the length of one cell's sponge: the launches go round LAUNCH_STREAMS
    # streams so that several run side by side (their output rows are disjoint), all of them after the two uploads: on one stream
    # the module takes about three times as long.  The tensors outlive the device-wide synchronise below, so no record_stream.
    main = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(LAUNCH_STREAMS)]
    try:
        for i, ((s, a, n, *_), (r0, p, r1, r)) in enumerate(zip(items, lay)):
            assert (d_in.data_ptr() + p) % 16 == a % 16 and p + n * s + TAIL <= r1 <= host.size     # the case is what it says, inside the buffer
            st = streams[i % LAUNCH_STREAMS]
            if i < LAUNCH_STREAMS:
                st.wait_stream(main)
            ctx.set_stream(st.cuda_stream)
            ctx.hash_cells_dev(d_in.data_ptr() + p, s, n, d_out.data_ptr() + 32 * r)
    finally:
        ctx.set_stream(main.cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    if np.array_equal(got, exp):
        return []
    bad = []
    for (s, a, n, fill, comp, cells, want), (r0, p, r1, r) in zip(items, lay):
        what = "cell_size=%d a=%d n_cells=%d%s%s" % (s, a, n, "" if fill is None else " fill=0x%02X" % fill, " (complemented slack)" if comp else "")
        rows = np.nonzero((got[r:r + n] != exp[r:r + n]).any(axis=1))[0]
        if rows.size:
            bad.append("%s: %d of %d digests differ, first at cell %d" % (what, rows.size, n, rows[0]))
        lo, hi = got[r - GUARD_ROWS:r], got[r + n:r + n + GUARD_ROWS]
        if not (np.array_equal(lo, pre[:GUARD_ROWS]) and np.array_equal(hi, pre[:GUARD_ROWS])):
            bad.append("%s: guard rows around the output changed" % what)
    return bad


def sweep(torch, ctx, C, cases):
    """Runs `cases` chunk by chunk; the oracle works on the next chunk's sizes while the device hashes this one's."""
    need = cells_needed(cases)
    by_key = {}
    for c in cases:
        by_key.setdefault((c[0], c[3]), []).append(c)
    bad = []
    with ThreadPoolExecutor(ORACLE_THREADS) as pool:
        def submit(keys):
            return {k: pool.submit(make_size, C, k[0], need[k], k[1]) for k in keys}
        chunks = chunks_of(need)
        ahead = submit(chunks[0])
        for i in range(len(chunks)):
            cur, ahead = ahead, (submit(chunks[i + 1]) if i + 1 < len(chunks) else None)
            items = []
            for k in chunks[i]:
                cells, want = cur[k].result()
                items += [c + (cells, want) for c in by_key[k]]
            bad += run_hash_batch(torch, ctx, items)
    return bad


def report(capsys, name, cases, bad, t0):
    with capsys.disabled():
        print("\n[kernel edges] %s: %d runs, %d distinct (cell_size, a, n_cells) cases, none skipped, %d failed, %.1f s"
              % (name, len(cases), distinct(cases), len(bad), time.time() - t0))
    assert not bad, "%d failing runs:\n%s" % (len(bad), "\n".join(bad[:400]))


@pytest.fixture
def dev(ctx):
    """torch, with the context's launches on torch's current stream for the length of one test."""
    import torch
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    yield torch
    torch.cuda.synchronize()
    ctx.reset_stream()


# ---- 1. k_hash_cells through cp2_hash_cells_dev ----------------------------------------------------------------------------------
@gpu
def test_hash_cells_every_size_every_base_offset(ctx, oracle, dev, capsys):
    C, _ = oracle
    t0, cases = time.time(), contiguous_cases()
    report(capsys, "sizes 0..%d x a in %s" % (MAX_SIZE, list(OFFSETS)), cases, sweep(dev, ctx, C, cases), t0)


@gpu
@pytest.mark.parametrize("centre", WINDOWS)
def test_hash_cells_windows_after_many_ring_revolutions(ctx, oracle, dev, capsys, centre):
    C, _ = oracle
    t0, cases = time.time(), window_cases(centre)
    report(capsys, "sizes %d..%d x a in %s" % (centre - WINDOW_HALF, centre + WINDOW_HALF, list(WINDOW_OFFSETS)), cases, sweep(dev, ctx, C, cases), t0)


@gpu
def test_hash_cells_one_cell_of_a_mebibyte_and_five_bytes(ctx, oracle, dev, capsys):
    C, _ = oracle
    t0, cases = time.time(), [(BIG_CELL, a, 1, None, False) for a in OFFSETS]
    report(capsys, "one cell of 2^20 + 5 bytes", cases, sweep(dev, ctx, C, cases), t0)


@gpu
def test_hash_cells_of_no_cells_touches_nothing(ctx, dev):
    torch = dev
    pre = np.tile(GUARD_ROW, (2 * GUARD_ROWS, 1))
    d_in = torch.from_numpy(SLACK.copy()).cuda()
    d_out = torch.from_numpy(pre).cuda()
    for size in (0, 1, 31, 2048):
        assert ctx.L.cp2_hash_cells_dev(ctx.h, ctypes.c_void_p(d_in.data_ptr() + 1), size, 0, ctypes.c_void_p(d_out.data_ptr() + 32 * GUARD_ROWS)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), pre)


# ---- 2. k_hash_cells<64> -----------------------------------------------------------------------------------------------------------
CHILD = os.path.join(HERE, "hash_block_child.py")


def save_child_job(path, cases, want):
    need = cells_needed(cases)
    keys = sorted(k[0] for k in need)
    np.savez(path, sizes=np.array(keys, dtype=np.int64), rows=np.array([need[(s, None)] for s in keys], dtype=np.int64),
             want=np.concatenate([want[(s, None)][:need[(s, None)]] for s in keys]), cases=np.array([c[:3] for c in cases], dtype=np.int64))
    return path


def run_child(argv, env, cases):
    p = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "child exit status %d\n%s\n%s" % (p.returncode, p.stdout[-6000:], p.stderr[-3000:])
    res = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith('{"block"')]
    assert res == [{"block": env.get("CP2_HASH_BLOCK"), "runs": len(cases), "distinct": distinct(cases), "failed": 0}], p.stdout[-3000:]


@gpu
def test_hash_cells_workgroups_of_64_lanes(oracle, tmp_path, capsys):
    """CP2_HASH_BLOCK is read once per process: a fresh child hashes, the expected digests come from here.
    What this does NOT observe is the shape the library launched: the child only echoes the variable it was given, and the digests
    are the same from either shape.  It rests on hash_block_override() in csrc/kernels.hip reading that variable; if that stopped,
    these cases would run on the 256-lane kernel and still pass.  The boundary has no getter for the shape in use."""
    C, _ = oracle
    t0, cases = time.time(), child_cases()
    need = cells_needed(cases)
    with ThreadPoolExecutor(ORACLE_THREADS) as pool:
        futs = {k: pool.submit(make_size, C, k[0], need[k], k[1]) for k in need}
        want = {k: f.result()[1] for k, f in futs.items()}
    env = dict(os.environ, CP2_HASH_BLOCK="64")
    run_child([sys.executable, CHILD, save_child_job(str(tmp_path / "want.npz"), cases, want)], env, cases)
    report(capsys, "64-lane workgroups (child process)", cases, [], t0)


# ---- 3. k_gen_fake_cells through cp2_gen_fake_cells_dev ----------------------------------------------------------------------------
GEN_SIZES = (0, 1, 17, 127, 128, 129, 256, 2048, 2049, 16384)
GEN_COUNTS = (1, 63, 64, 65, 255, 256, 257)
GEN_FIRSTS = (0, 1 << 21, (1 << 32) - 3)
GEN_SEEDS = (12417, 0, (1 << 64) - 5)
GEN_OFFSETS = (0, 1, 4, 8, 15, 16)


@gpu
def test_gen_fake_cells_every_write_out_path(ctx, oracle, dev, capsys):
    """Both paths (whole 128-byte lines through LDS for cell_size % 128 == 0 into a 16-byte-aligned pointer, bytes otherwise)
    against the oracle, with 64 guard bytes before and at least 192 after each output.  The buffer ends in room for a whole
    workgroup's cells, so that a store by a lane without a cell would land in compared memory."""
    torch = dev
    C, _ = oracle
    t0, bad, cases = time.time(), [], []
    nmax = max(GEN_COUNTS)
    for cs in GEN_SIZES:
        for seed in GEN_SEEDS:
            want = {first: C.gen_fake_cells(seed, first, nmax, cs) for first in GEN_FIRSTS}
            lay, off = [], 0
            for first in GEN_FIRSTS:
                for n in GEN_COUNTS:
                    for a in GEN_OFFSETS:
                        lay.append((first, n, a, off + FRONT + a))
                        off = _up(off + FRONT + a + n * cs + TAIL)
            total = off + 256 * cs + 4096
            exp = np.resize(SLACK, total)
            d = torch.from_numpy(exp).cuda()
            exp = exp.copy()
            for (first, n, a, p) in lay:
                assert (d.data_ptr() + p) % 16 == a % 16
                ctx.gen_fake_cells_dev(seed, first, n, cs, d.data_ptr() + p)
                exp[p:p + n * cs] = want[first][:n].reshape(-1)
                cases.append((cs, a, n, None, False))
            torch.cuda.synchronize()
            got = d.cpu().numpy()
            if np.array_equal(got, exp):
                continue
            for i, (first, n, a, p) in enumerate(lay):
                what = "cell_size=%d n=%d first=%d seed=%d a=%d" % (cs, n, first, seed, a)
                g, e = got[p:p + n * cs], exp[p:p + n * cs]
                if not np.array_equal(g, e):
                    bad.append("%s: cells differ, first at cell %d" % (what, np.nonzero(g != e)[0][0] // max(cs, 1)))
                end = lay[i + 1][3] - FRONT - lay[i + 1][2] if i + 1 < len(lay) else total
                if not (np.array_equal(got[p - FRONT - a:p], exp[p - FRONT - a:p]) and np.array_equal(got[p + n * cs:end], exp[p + n * cs:end])):
                    bad.append("%s: bytes around the output changed" % what)
    with capsys.disabled():
        print("\n[kernel edges] fake cells: %d runs (%d sizes x %d counts x %d firsts x %d seeds x %d offsets), none skipped, %d failed, %.1f s"
              % (len(cases), len(GEN_SIZES), len(GEN_COUNTS), len(GEN_FIRSTS), len(GEN_SEEDS), len(GEN_OFFSETS), len(bad), time.time() - t0))
    assert len(cases) == len(GEN_SIZES) * len(GEN_COUNTS) * len(GEN_FIRSTS) * len(GEN_SEEDS) * len(GEN_OFFSETS)
    assert not bad, "%d failing runs:\n%s" % (len(bad), "\n".join(bad[:400]))


# ---- 4. refusals that launch nothing -------------------------------------------------------------------------------------------------
CP2_ERR_INVALID, CP2_ERR_ALIGN = -1, -6


@gpu
def test_hash_cells_dev_refusals(pkg, ctx, dev, golden):
    torch = dev
    vp = ctypes.c_void_p
    n = 70
    pre = np.tile(GUARD_ROW, (n + 2 * GUARD_ROWS, 1))
    d_in = torch.from_numpy(np.resize(SLACK, n * 64)).cuda()
    d_out = torch.from_numpy(pre).cuda()
    rows = d_out.data_ptr() + 32 * GUARD_ROWS
    assert ctx.L.cp2_hash_cells_dev(ctx.h, vp(d_in.data_ptr()), 64, n, vp(rows + 8)) == CP2_ERR_ALIGN
    assert ctx.L.cp2_hash_cells_dev(ctx.h, vp(d_in.data_ptr()), 64, n, None) == CP2_ERR_INVALID
    assert ctx.L.cp2_hash_cells_dev(ctx.h, None, 64, n, vp(rows)) == CP2_ERR_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), pre)
    assert ctx.L.cp2_hash_cells_dev(ctx.h, None, 0, n, vp(rows)) == 0
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    empty = pkg.felt_bytes(int(golden("hash_bytes.json")["hash"][0]))
    assert np.array_equal(got[GUARD_ROWS:GUARD_ROWS + n], np.tile(empty, (n, 1)))
    assert np.array_equal(got[:GUARD_ROWS], pre[:GUARD_ROWS]) and np.array_equal(got[GUARD_ROWS + n:], pre[:GUARD_ROWS])


@gpu
def test_sponge2_felts_batch_dev_refusals(pkg, ctx, dev, oracle, golden):
    torch = dev
    C, P = oracle
    vp = ctypes.c_void_p
    n, nf = 70, 3
    pre = np.tile(GUARD_ROW, (n + 2 * GUARD_ROWS, 1))
    felts = C.felts_to_array([(i * 0x9E3779B97F4A7C15 + 1) % P.R_MOD for i in range(n * nf)])
    d_in = torch.from_numpy(np.concatenate([felts, np.zeros((1, 32), dtype=np.uint8)])).cuda()
    d_out = torch.from_numpy(pre).cuda()
    rows = d_out.data_ptr() + 32 * GUARD_ROWS
    f = ctx.L.cp2_sponge2_felts_batch_dev
    assert f(ctx.h, vp(d_in.data_ptr()), nf, n, vp(rows + 8)) == CP2_ERR_ALIGN
    assert f(ctx.h, vp(d_in.data_ptr() + 8), nf, n, vp(rows)) == CP2_ERR_ALIGN
    assert f(ctx.h, vp(d_in.data_ptr()), nf, n, None) == CP2_ERR_INVALID
    assert f(ctx.h, None, nf, n, vp(rows)) == CP2_ERR_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), pre)
    assert f(ctx.h, None, 0, n, vp(rows)) == 0                      # no elements: the sponge of the empty list
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert str(P.sponge2([])) == golden("sponge_felts.json")["rate2"][0]
    assert np.array_equal(got[GUARD_ROWS:GUARD_ROWS + n], np.tile(pkg.felt_bytes(P.sponge2([])), (n, 1)))
    assert np.array_equal(got[:GUARD_ROWS], pre[:GUARD_ROWS]) and np.array_equal(got[GUARD_ROWS + n:], pre[:GUARD_ROWS])
    ctx.sponge2_felts_batch_dev(d_in.data_ptr(), nf, n, rows)       # and the call that is not refused, against the oracle
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy()[GUARD_ROWS:GUARD_ROWS + n], np.stack([C.sponge2_felts(felts[i * nf:(i + 1) * nf]) for i in range(n)]))
