"""GPU suite: cp2_dataset_repair_blocks / cp2_multi_dataset_repair_blocks -- candidate blocks checked on the device against the block roots
the dataset keeps, only the matching ones written back into the slot files, each file synced once, and the cache's stamps of those files
kept valid: after a matching repair the scrub is clean, the proof inputs and input.json files are those from before the damage, and the
next cached build loads the cache instead of rebuilding.  Wrong candidates are never written; refused calls touch nothing."""
import ctypes
import faulthandler
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIRCUIT = dict(maxDepth=10, maxLog2NSlots=4, cellSize=64, blockSize=256, nSamples=5)
CS, CPB, BS = 64, 4, 256                # cell size, cells per network block, block size
N_CELLS, N_SLOTS = 64, 6                # 16 blocks per slot
N_BLOCKS = N_CELLS // CPB
CP2_ERR_INVALID, CP2_ERR_IO = -1, -5
EXTRA = 100                             # slot 4's file holds this many bytes past nCells * cellSize
ENTROPY = 123457
OLD_NS = 1_600_000_000 * 10**9          # the files' mtime after writing: far from "now", so a write always moves it


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def sctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def config(pkg, base=None, n_slots=N_SLOTS, seed=5):
    return pkg.make_config(nCells=N_CELLS, nSlots=n_slots, seed=seed, file=base, **CIRCUIT)


def write_files(base, n_slots=N_SLOTS, seed=1):
    rng = np.random.default_rng(seed)
    data = {}
    for k in range(n_slots):
        b = rng.integers(1, 256, N_CELLS * CS + (EXTRA if k == 4 else 0), dtype=np.uint8).tobytes()   # no zero byte: a hole always differs
        path = "%s%d.dat" % (base, k)
        with open(path, "wb") as f:
            f.write(b)
        os.utime(path, ns=(OLD_NS, OLD_NS + k))
        data[k] = b
    return data


def flip(base, slot, offset):
    with open("%s%d.dat" % (base, slot), "r+b") as f:
        f.seek(offset)
        v = f.read(1)
        f.seek(offset)
        f.write(bytes([v[0] ^ 0x5A]))


def flip_keep_mtime(base, slot, offset):
    """bit rot: the bytes change, size and mtime do not"""
    path = "%s%d.dat" % (base, slot)
    st = os.stat(path)
    flip(base, slot, offset)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))


def build(ctx, cfg, mode, **kw):
    ctx.set_keep_trees(mode)
    try:
        ds = ctx.dataset(cfg, **kw)
    finally:
        ctx.set_keep_trees(-1)
    assert ds.tree_mode == mode
    return ds


def block(data, slot, b):
    return data[slot][b * BS:(b + 1) * BS]


def candidates(data, reqs):
    return np.frombuffer(b"".join(block(data, s, b) for s, b in reqs), dtype=np.uint8)


def files(base, n_slots=N_SLOTS):
    """(bytes, mtime_ns) of every slot file; None for a missing one"""
    out = {}
    for k in range(n_slots):
        p = "%s%d.dat" % (base, k)
        out[k] = (open(p, "rb").read(), os.stat(p).st_mtime_ns) if os.path.isfile(p) else None
    return out


def blocks_of(granularity, bad):
    """the scrub's report as sorted unique (slot, block) pairs (cells of the slot -> their blocks)"""
    return sorted({(int(s), int(i) // CPB if granularity == 2 else int(i)) for s, i in bad})


def raw_repair(fn, h, sb, data, n, flags=0, cache=None):
    """the C call itself with sentinel outputs: (status, statuses, n_written)"""
    status = np.full(max(n, 1), 7, dtype=np.uint32)
    w = ctypes.c_size_t(99)
    st = fn(h, None if sb is None else np.ascontiguousarray(sb, dtype=np.uint64).ctypes.data, None if data is None else data.ctypes.data, n, flags,
            cache, status.ctypes.data, ctypes.byref(w))
    return st, status[:n], w.value


@pytest.mark.parametrize("mode", [1, 2])
def test_damaged_blocks_repaired_with_the_original_bytes(pkg, sctx, tmp_path, mode):
    base = str(tmp_path / "slot")
    data = write_files(base)
    ds = build(sctx, config(pkg, base), mode)
    before = {s: ds.proof_input(s, ENTROPY).json() for s in range(N_SLOTS)}
    flip(base, 0, 3 * BS + 17)                                    # one byte in block 3 of slot 0
    flip(base, 2, N_CELLS * CS - 1)                               # the last byte of slot 2
    flip(base, 3, 6 * BS)
    flip(base, 3, 7 * BS + BS - 1)                                # two neighbouring blocks of slot 3
    with open("%s1.dat" % base, "r+b") as f:                      # slot 1 cut in the middle of block 13
        f.truncate(13 * BS + 100)
    g, bad, n = ds.scrub()
    reqs = blocks_of(g, bad)
    assert reqs == [(0, 3), (1, 13), (1, 14), (1, 15), (2, 15), (3, 6), (3, 7)]
    os.remove("%s5.dat" % base)                                   # slot 5 lost (a scrub cannot read it): every block restored
    reqs += [(5, b) for b in range(N_BLOCKS)]
    status, n_written = ds.repair_blocks(reqs, candidates(data, reqs))
    assert (status == pkg.REPAIR_MATCH).all() and n_written == len(reqs)
    for s in range(N_SLOTS):
        assert open("%s%d.dat" % (base, s), "rb").read()[:N_CELLS * CS] == data[s][:N_CELLS * CS]
    assert open("%s4.dat" % base, "rb").read() == data[4]        # (an untouched file keeps its tail)
    assert ds.scrub()[2] == 0
    assert {s: ds.proof_input(s, ENTROPY).json() for s in range(N_SLOTS)} == before
    ds.free()


@pytest.mark.parametrize("mode", [1, 2])
def test_wrong_candidates_are_never_written(pkg, sctx, tmp_path, mode):
    base = str(tmp_path / "slot")
    data = write_files(base)
    ds = build(sctx, config(pkg, base), mode)
    last_cell_bit = bytearray(block(data, 1, 4))
    last_cell_bit[BS - CS + 5] ^= 0x01
    reqs = [(0, 1), (1, 4), (2, 0), (3, 5), (4, 7), (5, 15)]
    cand = np.frombuffer(block(data, 0, 2) + bytes(last_cell_bit) + bytes(BS) + block(data, 3, 6) + block(data, 4, 7) + block(data, 5, 15),
                         dtype=np.uint8)
    was = files(base)
    status, n_written = ds.repair_blocks(reqs, cand)
    M, X = pkg.REPAIR_MATCH, pkg.REPAIR_MISMATCH
    assert list(status) == [X, X, X, X, M, M] and n_written == 2
    now = files(base)
    for s in range(N_SLOTS):
        assert now[s][0] == was[s][0]                             # every byte as it was (the matches wrote what was there)
    for s in range(4):
        assert now[s][1] == was[s][1]                             # the files of wrong candidates were not even opened for writing
    assert ds.scrub()[2] == 0
    ds.free()


def test_check_only_fake_source_and_refusals(pkg, sctx, tmp_path):
    base = str(tmp_path / "slot")
    data = write_files(base)
    cfg = config(pkg, base)
    ds = build(sctx, cfg, 2)
    flip(base, 0, 3 * BS + 1)
    was = files(base)
    reqs = [(0, 3), (1, 2)]
    status, n_written = ds.repair_blocks(reqs, candidates(data, reqs), check_only=True)
    assert list(status) == [pkg.REPAIR_MATCH] * 2 and n_written == 0
    assert files(base) == was                                     # bytes and mtimes: nothing written
    # the fake source: verdicts, and a write request refused
    fake = build(sctx, config(pkg), 1)
    seed = sctx.slot_seed(cfg.seed, 2)
    good = sctx.gen_fake_cells(seed, 5 * CPB, CPB, CS).tobytes()
    other = sctx.gen_fake_cells(seed, 6 * CPB, CPB, CS).tobytes()
    status, n_written = fake.repair_blocks([(2, 5), (2, 9)], np.frombuffer(good + other, dtype=np.uint8), check_only=True)
    assert list(status) == [pkg.REPAIR_MATCH, pkg.REPAIR_MISMATCH] and n_written == 0
    L = sctx.L
    fn = L.cp2_dataset_repair_blocks
    one = np.frombuffer(good, dtype=np.uint8)
    st, out, w = raw_repair(fn, fake.h, np.array([[2, 5]]), one, 1)
    assert (st, list(out), w) == (CP2_ERR_INVALID, [7], 99) and "fake source" in L.cp2_last_error(sctx.h).decode()
    # refusals on the file dataset: nothing written, outputs untouched, the request named
    roots_only = build(sctx, cfg, 0)
    two = candidates(data, [(0, 3), (0, 3)])
    for h, sb, d, n, flags, words in ((roots_only.h, np.array([[0, 3]]), two[:BS], 1, 0, "slot roots"),
                                      (ds.h, np.array([[0, 3], [1, 1], [0, 3]]), np.concatenate([two, two[:BS]]), 3, 0, "request 2"),
                                      (ds.h, np.array([[0, 3], [N_SLOTS, 0]]), two, 2, 0, "request 1"),
                                      (ds.h, np.array([[0, N_BLOCKS]]), two[:BS], 1, 0, "request 0"),
                                      (ds.h, None, two[:BS], 1, 0, "NULL"),
                                      (ds.h, np.array([[0, 3]]), None, 1, 0, "NULL"),
                                      (ds.h, np.array([[0, 3]]), two[:BS], 1, 4, "flag")):
        st, out, w = raw_repair(fn, h, sb, d, n, flags)
        assert (st, list(out), w) == (CP2_ERR_INVALID, [7] * n, 99), words
        assert words in L.cp2_last_error(sctx.h).decode(), (words, L.cp2_last_error(sctx.h))
    st = fn(ds.h, np.array([[0, 3]], dtype=np.uint64).ctypes.data, two.ctypes.data, 1, 0, None, None, None)
    assert st == CP2_ERR_INVALID
    assert files(base) == was
    st, out, w = raw_repair(fn, ds.h, None, None, 0)              # nothing to do
    assert (st, w) == (0, 0)
    for d in (roots_only, fake, ds):
        d.free()


def test_cached_compact_dataset_repair_keeps_the_cache_valid(pkg, sctx, tmp_path):
    """Bit rot under a compact cached dataset: a proof touching the block fails; the repair with cache_path writes the block and
    restamps the file in the cache, so the proof input is the one from before and the next cached build loads instead of rebuilding.
    Without cache_path, or when the damage moved the mtime (the cache was stale already), the next build rebuilds."""
    slot, cell = 3, 41
    blk = cell // CPB

    def setup(name):
        base = str(tmp_path / name)
        data = write_files(base)
        cfg = config(pkg, base)
        cache = str(tmp_path / (name + ".cache"))
        ds = build(sctx, cfg, 2, cache=cache)
        return base, data, cfg, cache, ds

    base, data, cfg, cache, ds = setup("a")
    roots = ds.local_roots()
    hit = next(e for e in range(1, 5000)
               if blk in set(int(i) // CPB for i in sctx.cell_indices(pkg.felt_bytes(e), roots[slot], N_CELLS, CIRCUIT["nSamples"])))
    before = {e: ds.proof_input(slot, e).json() for e in (ENTROPY, hit)}
    ds.free()
    flip_keep_mtime(base, slot, cell * CS + 9)
    ds2 = build(sctx, cfg, 2, cache=cache)
    assert np.array_equal(ds2.local_roots(), roots)              # loaded from the cache: the damage is not seen
    with pytest.raises(pkg.CodexP2Error) as ei:
        ds2.proof_input(slot, hit)
    assert ei.value.status == CP2_ERR_IO
    status, n_written = ds2.repair_blocks([(slot, blk)], candidates(data, [(slot, blk)]), cache_path=cache)
    assert list(status) == [pkg.REPAIR_MATCH] and n_written == 1
    assert {e: ds2.proof_input(slot, e).json() for e in (ENTROPY, hit)} == before
    ds2.free()
    st = os.stat(cache)
    ds3 = build(sctx, cfg, 2, cache=cache)                        # the cache is loaded: a rebuild would rename a new file into place
    st3 = os.stat(cache)
    assert (st3.st_ino, st3.st_mtime_ns) == (st.st_ino, st.st_mtime_ns)
    assert np.array_equal(ds3.local_roots(), roots) and ds3.scrub()[2] == 0
    assert ds3.proof_input(slot, hit).json() == before[hit]
    ds3.free()
    # control 1: the same damage repaired without cache_path -> the next build rebuilds
    base, data, cfg, cache, ds = setup("b")
    ds.free()
    flip_keep_mtime(base, slot, cell * CS + 9)
    ds = build(sctx, cfg, 2, cache=cache)
    st = os.stat(cache)
    assert list(ds.repair_blocks([(slot, blk)], candidates(data, [(slot, blk)]))[0]) == [pkg.REPAIR_MATCH]
    ds.free()
    ds = build(sctx, cfg, 2, cache=cache)
    assert os.stat(cache).st_ino != st.st_ino
    ds.free()
    # control 2: damage that moved the mtime -> the cache was stale and stays stale, even with cache_path
    base, data, cfg, cache, ds = setup("c")
    flip(base, slot, cell * CS + 9)
    digest = hashlib.sha256(open(cache, "rb").read()).hexdigest()
    st = os.stat(cache)
    status, n_written = ds.repair_blocks([(slot, blk)], candidates(data, [(slot, blk)]), cache_path=cache)
    assert list(status) == [pkg.REPAIR_MATCH] and n_written == 1
    assert hashlib.sha256(open(cache, "rb").read()).hexdigest() == digest
    ds.free()
    ds = build(sctx, cfg, 2, cache=cache)
    assert os.stat(cache).st_ino != st.st_ino
    ds.free()


def test_a_file_that_cannot_be_written_stops_the_writing(pkg, sctx, tmp_path):
    base = str(tmp_path / "slot")
    data = write_files(base)
    ds = build(sctx, config(pkg, base), 2)
    reqs = [(5, 0), (1, 2), (3, 4), (3, 9)]
    for s, b in reqs:
        flip(base, s, b * BS + 7)
    os.remove("%s3.dat" % base)
    os.mkdir("%s3.dat" % base)                                    # slot 3's file is now a directory
    st, status, n_written = raw_repair(sctx.L.cp2_dataset_repair_blocks, ds.h, np.array(reqs), candidates(data, reqs), len(reqs))
    U, M = pkg.REPAIR_UNWRITTEN, pkg.REPAIR_MATCH
    assert st == CP2_ERR_IO and list(status) == [U, M, U, U] and n_written == 1
    msg = sctx.L.cp2_last_error(sctx.h).decode()
    assert "cannot write" in msg and "slot3.dat" in msg, msg
    assert open("%s1.dat" % base, "rb").read() == data[1]         # the file before it: written
    assert open("%s5.dat" % base, "rb").read() != data[5]         # the file after it: not
    ds.free()


CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as g
job = json.loads(sys.argv[1])
pkg = g.load_package()
ctx = pkg.Context(0)
cfg = pkg.make_config(**job["config"])
ctx.set_keep_trees(job["mode"])
ds = ctx.dataset(cfg)
reqs = np.array(job["reqs"], dtype=np.uint64)
cand = np.fromfile(job["cand"], dtype=np.uint8)
out = {"pageable": ds.repair_blocks(reqs, cand, check_only=True)[0].tolist()}
import torch
pinned = torch.from_numpy(cand).pin_memory()
out["pinned"] = ds.repair_blocks(reqs, pinned.numpy(), check_only=True)[0].tolist()
ds.free()
ctx.close()
print(json.dumps(out), flush=True)
""" % ROOT


@pytest.mark.parametrize("stage_mb,n_cells,n_slots", [(1, 4096, 8), (80, 16384, 64)])
def test_many_chunks_pageable_and_pinned_same_verdicts(pkg, sctx, tmp_path, stage_mb, n_cells, n_slots):
    """64 KiB blocks.  1 MiB of staging: chunks of 8 requests; 80 MiB: a chunk through the pinned ring (more than 32 MiB) and a smaller
    one; caller-pinned candidates read in place.  The verdicts equal those of one chunk with the default staging."""
    bs = 65536
    base = str(tmp_path / "big")
    rng = np.random.default_rng(n_cells)
    data = {}
    for k in range(n_slots):
        data[k] = rng.integers(1, 256, n_cells * CS, dtype=np.uint8).tobytes()
        with open("%s%d.dat" % (base, k), "wb") as f:
            f.write(data[k])
    conf = dict(maxDepth=16, maxLog2NSlots=max(1, (n_slots - 1).bit_length()), cellSize=CS, blockSize=bs, nSlots=n_slots, nCells=n_cells,
                nSamples=5, seed=3, file=base)
    nb = n_cells * CS // bs
    reqs = [(s, b) for s in range(n_slots) for b in range(nb)]
    order = np.random.default_rng(1).permutation(len(reqs))
    reqs = [reqs[i] for i in order]
    parts = []
    for i, (s, b) in enumerate(reqs):
        blk = data[s][b * bs:(b + 1) * bs]
        if i % 3 == 1:
            blk = blk[:-1] + bytes([blk[-1] ^ 1])                   # the last byte of the last cell
        elif i % 7 == 2:
            s2, b2 = reqs[(i + 1) % len(reqs)]
            blk = data[s2][b2 * bs:(b2 + 1) * bs]                   # another block's bytes
        parts.append(blk)
    cand = np.frombuffer(b"".join(parts), dtype=np.uint8)
    cand_path = str(tmp_path / "cand.bin")
    cand.tofile(cand_path)
    for mode in (1, 2):
        ref = build(sctx, pkg.make_config(**conf), mode)
        want, w = ref.repair_blocks(reqs, cand, check_only=True)
        ref.free()
        assert w == 0 and want[1::3].tolist() == [pkg.REPAIR_MISMATCH] * len(want[1::3])
        assert 0 < int((want == pkg.REPAIR_MATCH).sum()) < len(reqs)
        job = {"config": conf, "mode": mode, "reqs": reqs, "cand": cand_path}
        clean = {k: v for k, v in os.environ.items() if not k.startswith("CODEX_P2_")}
        r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(job)], capture_output=True, text=True, timeout=200,
                           env=dict(clean, CODEX_P2_STAGE_MB=str(stage_mb)))
        assert r.returncode == 0, r.stderr[-3000:]
        got = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert got["pageable"] == want.tolist() and got["pinned"] == want.tolist()


def test_multi_equals_single_context(pkg, sctx, tmp_path):
    """Three contexts on one device, by whole slots (each shard compact) and cut by units (every node): the requests in mixed order and
    with one wrong candidate, the statuses and the files equal those of the single-context call, and the multi scrub is clean after."""
    base = str(tmp_path / "slot")
    data = write_files(base, n_slots=7)
    cfg = config(pkg, base, n_slots=7)
    damage = [(6, 8), (0, 0), (3, 4), (2, 15), (3, 5), (4, 10), (1, 7)]
    wrong = (5, 3)

    def damage_files():
        for s, b in damage:
            flip(base, s, b * BS + 11)

    reqs = damage + [wrong]
    cand = np.concatenate([candidates(data, damage), np.zeros(BS, dtype=np.uint8)])
    m = pkg.Multi([0, 0, 0])
    try:
        m.set_policy(pkg.GATHER_AUTO, 1)
        for split, mode in ((1, 2), (0, 1)):
            m.set_split(split)
            for i in range(3):
                m.ctx(i).set_keep_trees(mode)
            md = m.dataset(cfg)
            for i in range(3):
                m.ctx(i).set_keep_trees(-1)
            assert len(md.shards()) == 3 and (md.units_per_slot > 1) == (split == 0)
            ref = build(sctx, cfg, mode)
            damage_files()
            want, w_want = ref.repair_blocks(reqs, cand)
            after_single = {s: v[0] for s, v in files(base, 7).items()}
            ref.free()
            assert list(want) == [pkg.REPAIR_MATCH] * len(damage) + [pkg.REPAIR_MISMATCH] and w_want == len(damage)
            damage_files()                                          # (flipping again damages the repaired bytes again)
            assert md.scrub()[2] > 0
            got, w_got = md.repair_blocks(reqs, cand)
            assert list(got) == list(want) and w_got == w_want
            assert {s: v[0] for s, v in files(base, 7).items()} == after_single
            assert md.scrub()[2] == 0
            md.free()
    finally:
        m.close()


def traced(capfd, f):
    """f() with CP2_TRACE set: (its result, what the library wrote to stderr meanwhile)"""
    os.environ["CP2_TRACE"] = "1"
    capfd.readouterr()
    try:
        out = f()
    finally:
        del os.environ["CP2_TRACE"]
    return out, capfd.readouterr().err


def test_multi_repair_restamps_the_caches_the_cached_build_wrote(pkg, tmp_path, capfd):
    """cp2_multi_dataset_repair_blocks with cache_path, two contexts on one device, by whole slots and cut by units: the shard caches it
    restamps are the files cp2_multi_dataset_build_cached wrote (one function names them for both), so after bit rot and its repair the
    next cached build finds the same files and nothing else, loads them (same inode, same mtime as after the restamp) and reads no slot
    file.  By slots the shards' tree caches get a compact build's ".kept" files beside them first: both names are restamped, and both a
    compact and an every-node build load afterwards."""
    slot, blk = 4, 9
    m = pkg.Multi([0, 0])

    def multi_build(cfg, cache, mode):
        for i in range(2):
            m.ctx(i).set_keep_trees(mode)
        try:
            return traced(capfd, lambda: m.dataset(cfg, cache=cache))
        finally:
            for i in range(2):
                m.ctx(i).set_keep_trees(-1)

    try:
        m.set_policy(pkg.GATHER_AUTO, 1)
        for split in (1, 0):
            d = tmp_path / ("cut%d" % split)
            d.mkdir()
            base = str(d / "slot")
            data = write_files(base, n_slots=7)
            cfg = config(pkg, base, n_slots=7)
            cache = str(d / "c.cp2")
            caches = lambda: sorted(f for f in os.listdir(d) if f.startswith("c.cp2"))
            stats = lambda: {f: (os.stat(d / f).st_ino, os.stat(d / f).st_mtime_ns) for f in caches()}
            m.set_split(split)
            md, err = multi_build(cfg, cache, 1)
            assert "slot files:" in err, err                         # the first build read the slot files
            assert len(md.shards()) == 2
            if split == 1:
                assert md.units_per_slot == 1
                md.free()
                md, err = multi_build(cfg, cache, 2)                 # compact beside the tree caches: rebuilt once, saved as ".kept"
                assert "slot files:" in err and md.units_per_slot == 1
                names = ["c.cp2.shard0of2", "c.cp2.shard0of2.kept", "c.cp2.shard1of2", "c.cp2.shard1of2.kept"]
            else:
                assert md.units_per_slot == 2                        # 7 slots over 2 contexts: the plan cuts every slot in two
                names = ["c.cp2.units2.shard0of2", "c.cp2.units2.shard1of2"]
            assert caches() == names
            flip_keep_mtime(base, slot, blk * BS + 77)
            assert blocks_of(*md.scrub()[:2]) == [(slot, blk)]
            status, n_written = md.repair_blocks([(slot, blk)], candidates(data, [(slot, blk)]), cache_path=cache)
            assert list(status) == [pkg.REPAIR_MATCH] and n_written == 1
            md.free()
            after_repair = stats()
            for mode in ((2, 1) if split == 1 else (1,)):
                md, err = multi_build(cfg, cache, mode)
                assert caches() == names and stats() == after_repair   # the same files, none written again
                assert "slot files:" not in err, err                 # ... and loaded: no slot file was read
                assert (md.units_per_slot > 1) == (split == 0) and md.scrub()[2] == 0
                md.free()
    finally:
        m.close()
