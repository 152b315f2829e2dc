"""GPU suite: cp2_dataset_scrub / cp2_multi_dataset_scrub -- slots re-read from their source and compared with what the dataset keeps
(cell hashes, block roots or slot roots) report exactly the changed cells / blocks / slots, sorted, capped and counted; changed data is
not an error, a missing file or a bad range is, and a scrub leaves the dataset, its cache and every input.json as they were."""
import ctypes
import faulthandler
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CIRCUIT = dict(maxDepth=10, maxLog2NSlots=4, cellSize=64, blockSize=256, nSamples=5)
CS, CPB = 64, 4                        # cell size, cells per network block
N_CELLS, N_SLOTS = 64, 6               # 16 blocks per slot
CP2_ERR_INVALID, CP2_ERR_IO = -1, -5
LEVEL = {1: 2, 2: 1, 0: 0}             # keep-trees mode -> CP2_SCRUB_CELL / _BLOCK / _SLOT
EXTRA = 100                            # slot 4's file holds this many bytes past nCells * cellSize


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


def config(pkg, base=None, n_cells=N_CELLS, n_slots=N_SLOTS, seed=5):
    return pkg.make_config(nCells=n_cells, nSlots=n_slots, seed=seed, file=base, **CIRCUIT)


def write_files(base, n_slots=N_SLOTS, n_cells=N_CELLS, seed=1):
    rng = np.random.default_rng(seed)
    data = {}
    for k in range(n_slots):
        n = n_cells * CS + (EXTRA if k == 4 else 0)
        b = rng.integers(1, 256, n, dtype=np.uint8).tobytes()   # no zero byte: a truncated tail always differs
        with open("%s%d.dat" % (base, k), "wb") as f:
            f.write(b)
        data[k] = b
    return data


def restore(base, data):
    for k, b in data.items():
        with open("%s%d.dat" % (base, k), "wb") as f:
            f.write(b)


def flip(base, slot, offset):
    with open("%s%d.dat" % (base, slot), "r+b") as f:
        f.seek(offset)
        v = f.read(1)
        f.seek(offset)
        f.write(bytes([v[0] ^ 0x5A]))


def build(ctx, cfg, mode, **kw):
    ctx.set_keep_trees(mode)
    try:
        ds = ctx.dataset(cfg, **kw)
    finally:
        ctx.set_keep_trees(-1)
    assert ds.tree_mode == mode
    return ds


def slot_bytes(base, slot, n_cells=N_CELLS):
    """what the builders hash: the file's first nCells * cellSize bytes, zeros past its end (slot.nim:61-66)"""
    b = open("%s%d.dat" % (base, slot), "rb").read()[:n_cells * CS]
    return np.frombuffer(b + bytes(n_cells * CS - len(b)), dtype=np.uint8)


def changed_cells(before, base):
    out = set()
    for s, b in before.items():
        a = np.frombuffer(b[:N_CELLS * CS], dtype=np.uint8).reshape(N_CELLS, CS)
        now = slot_bytes(base, s).reshape(N_CELLS, CS)
        out |= {(s, int(c)) for c in np.nonzero((a != now).any(axis=1))[0]}
    return out


def expect(cells, mode):
    if mode == 1:
        return sorted(cells)
    if mode == 2:
        return sorted({(s, c // CPB) for s, c in cells})
    return sorted({(s, 0) for s, _ in cells})


def pairs(bad):
    return [(int(a), int(b)) for a, b in bad]


def raw_scrub(L, ds, first, n, cap):
    """the C call itself with sentinel outputs: (status, bad rows, n_bad, granularity)"""
    bad = np.full((max(cap, 1), 2), 7, dtype=np.uint64)
    nb, g = ctypes.c_size_t(99), ctypes.c_int(42)
    st = L.cp2_dataset_scrub(ds.h, first, n, bad.ctypes.data, cap, ctypes.byref(nb), ctypes.byref(g))
    return st, bad, nb.value, g.value


@pytest.mark.parametrize("mode", [1, 2, 0])
def test_clean_file_and_fake_datasets(pkg, sctx, tmp_path, mode):
    base = str(tmp_path / "slot")
    write_files(base)
    for cfg in (config(pkg, base), config(pkg)):
        ds = build(sctx, cfg, mode)
        g, bad, n = ds.scrub()
        assert (g, n, bad.shape) == (LEVEL[mode], 0, (0, 2))
        g, bad, n = ds.scrub(2, 3, cap=0)
        assert (g, n) == (LEVEL[mode], 0)
        ds.free()


@pytest.mark.parametrize("mode", [1, 2, 0])
def test_changed_bytes_report_exactly_the_changed_set(pkg, sctx, oracle, tmp_path, mode):
    C, _ = oracle
    base = str(tmp_path / "slot")
    data = write_files(base)
    ds = build(sctx, config(pkg, base), mode)
    # first and last cell of a slot, two cells of one block, one more elsewhere; and a byte past nCells * cellSize (not hashed)
    for s, c, byte in ((0, 0, 0), (2, N_CELLS - 1, CS - 1), (3, 20, 5), (3, 21, 63), (5, 7, 31)):
        flip(base, s, c * CS + byte)
    flip(base, 4, N_CELLS * CS + EXTRA // 2)
    want_cells = changed_cells(data, base)
    assert want_cells == {(0, 0), (2, N_CELLS - 1), (3, 20), (3, 21), (5, 7)}
    g, bad, n = ds.scrub()
    assert g == LEVEL[mode] and pairs(bad) == expect(want_cells, mode) and n == len(expect(want_cells, mode))
    # a truncated file: exactly its tail that was not zero
    cut = N_CELLS * CS - 2 * CPB * CS - 100                       # mid-block 13: blocks 13, 14, 15 change
    with open("%s1.dat" % base, "r+b") as f:
        f.truncate(cut)
    want_cells = changed_cells(data, base)
    assert {c for s, c in want_cells if s == 1} == set(range(cut // CS, N_CELLS))
    g, bad, n = ds.scrub()
    assert pairs(bad) == expect(want_cells, mode) and n == len(expect(want_cells, mode))
    if mode == 2:   # the C oracle: hash_cells, then merkle_root per block -- the reported blocks are those whose root changed
        roots = lambda b: [C.merkle_root(C.hash_cells(b[k * CPB * CS:(k + 1) * CPB * CS], CS)).tobytes() for k in range(N_CELLS // CPB)]
        oracle_blocks = []
        for s in range(N_SLOTS):
            was = np.frombuffer(data[s][:N_CELLS * CS], dtype=np.uint8)
            oracle_blocks += [(s, k) for k, (x, y) in enumerate(zip(roots(was), roots(slot_bytes(base, s)))) if x != y]
        assert pairs(bad) == oracle_blocks
    restore(base, data)
    assert ds.scrub()[2] == 0
    ds.free()


def test_cached_compact_dataset_names_the_block_a_proof_would_fail_on(pkg, sctx, tmp_path):
    """The motivating case: the cache trusts size and mtime; the scrub finds the block; a proof touching it fails there; the repair
    makes the scrub clean and input.json byte-identical to the one made before the damage."""
    base = str(tmp_path / "slot")
    data = write_files(base)
    cfg = config(pkg, base)
    cache = str(tmp_path / "kept.cache")
    ds = build(sctx, cfg, 2, cache=cache)
    roots = ds.local_roots()
    entropy = 123457
    before = {s: ds.proof_input(s, entropy).json() for s in (0, 3)}
    cache_digest = hashlib.sha256(open(cache, "rb").read()).hexdigest()
    assert ds.scrub()[2] == 0                                     # a clean scrub changes nothing
    assert {s: ds.proof_input(s, entropy).json() for s in (0, 3)} == before
    assert hashlib.sha256(open(cache, "rb").read()).hexdigest() == cache_digest and ds.tree_mode == 2
    ds.free()
    slot, cell = 3, 41                                            # block 10 of slot 3
    path = "%s%d.dat" % (base, slot)
    stat = os.stat(path)
    flip(base, slot, cell * CS + 9)
    os.utime(path, ns=(stat.st_atime_ns, stat.st_mtime_ns))
    ds2 = build(sctx, cfg, 2, cache=cache)
    assert np.array_equal(ds2.local_roots(), roots)              # loaded from the cache, not rehashed
    g, bad, n = ds2.scrub()
    assert (g, pairs(bad), n) == (pkg.SCRUB_BLOCK, [(slot, cell // CPB)], 1)
    # an entropy whose samples touch that block: the proof input fails with CP2_ERR_IO naming the same block
    hit = next(e for e in range(1, 5000)
               if cell // CPB in set(int(i) // CPB for i in sctx.cell_indices(pkg.felt_bytes(e), roots[slot], N_CELLS, CIRCUIT["nSamples"])))
    with pytest.raises(pkg.CodexP2Error) as ei:
        ds2.proof_input(slot, hit)
    assert ei.value.status == CP2_ERR_IO and ("block %d of slot %d" % (cell // CPB, slot)) in str(ei.value)
    # repair: the bytes back, the scrub clean, input.json as before the damage
    restore(base, data)
    assert ds2.scrub()[2] == 0
    assert {s: ds2.proof_input(s, entropy).json() for s in (0, 3)} == before
    assert hashlib.sha256(open(cache, "rb").read()).hexdigest() == cache_digest
    ds2.free()


def test_range_cap_count_and_errors(pkg, sctx, tmp_path):
    base = str(tmp_path / "slot")
    data = write_files(base)
    ds = build(sctx, config(pkg, base), 1)
    part = build(sctx, config(pkg, base), 2, first_slot=1, n_local=3)
    for s in range(N_SLOTS):
        for c in (s, 10 + 3 * s, N_CELLS - 1 - s):
            flip(base, s, c * CS)
    want = sorted(changed_cells(data, base))
    g, bad, n = ds.scrub()
    assert g == pkg.SCRUB_CELL and pairs(bad) == want and n == len(want) == 3 * N_SLOTS
    g, bad, n = ds.scrub(2, 2)                                    # a subrange reports only its slots
    assert pairs(bad) == [p for p in want if p[0] in (2, 3)] and n == 6
    g, bad, n = ds.scrub(cap=4)                                   # the lowest `cap` in order, and the full count
    assert pairs(bad) == want[:4] and n == len(want)
    g, bad, n = ds.scrub(cap=0)                                   # counting only
    assert bad.shape == (0, 2) and n == len(want)
    L = sctx.L
    st, out, nb, gr = raw_scrub(L, ds, N_SLOTS, 1, 2)             # outside the local range: refused, outputs untouched
    assert (st, nb, gr) == (CP2_ERR_INVALID, 99, 42) and (out == 7).all()
    st, out, nb, gr = raw_scrub(L, ds, 4, 3, 2)
    assert (st, nb, gr) == (CP2_ERR_INVALID, 99, 42) and (out == 7).all()
    st, out, nb, gr = raw_scrub(L, part, 0, 1, 2)
    assert (st, nb, gr) == (CP2_ERR_INVALID, 99, 42) and (out == 7).all()
    assert pairs(part.scrub()[1]) == [p for p in expect(set(want), 2) if 1 <= p[0] <= 3]
    os.rename("%s2.dat" % base, "%s2.gone" % base)                 # a missing file: CP2_ERR_IO, nothing written
    st, out, nb, gr = raw_scrub(L, ds, 0, 0, 2)
    assert (st, nb, gr) == (CP2_ERR_IO, 99, 42) and (out == 7).all()
    assert "cannot open" in L.cp2_last_error(sctx.h).decode()
    os.rename("%s2.gone" % base, "%s2.dat" % base)
    assert ds.scrub()[2] == len(want)
    part.free()
    ds.free()


@pytest.mark.parametrize("direct", [0, 1])
def test_many_turns_and_batches_same_report(pkg, tmp_path, direct):
    """1 MiB of staging (transient batches of two large slots), ring turns smaller than a slot and turns holding several small slots,
    with O_DIRECT on and off: the report is the same as with the defaults."""
    os.environ["CODEX_P2_STAGE_MB"] = "1"
    try:
        small = pkg.Context(0)
    finally:
        del os.environ["CODEX_P2_STAGE_MB"]
    ref = pkg.Context(0)
    try:
        for n_cells, n_slots, chunk in ((4096, 7, 96 << 10), (N_CELLS, 9, 10 << 10)):
            base = str(tmp_path / ("s%d_" % n_cells))
            rng = np.random.default_rng(n_cells)
            for k in range(n_slots):
                with open("%s%d.dat" % (base, k), "wb") as f:
                    f.write(rng.integers(1, 256, n_cells * CS, dtype=np.uint8).tobytes())
            cfg = config(pkg, base, n_cells=n_cells, n_slots=n_slots)
            for mode in (1, 2):
                want_ds = build(ref, cfg, mode)
                ds = build(small, cfg, mode)
                for s, c in ((0, 0), (1, n_cells - 1), (3, n_cells // 2), (3, n_cells // 2 + 1), (n_slots - 1, 5)):
                    flip(base, s, c * CS + 3)
                small.set_ingest(0, 0, chunk)
                small.set_ingest_direct(direct)
                got = ds.scrub()
                small.set_ingest(0, 0, 0)
                small.set_ingest_direct(-1)
                want = want_ds.scrub()
                assert got[0] == want[0] == LEVEL[mode] and got[2] == want[2] > 0
                assert np.array_equal(got[1], want[1])
                for s, c in ((0, 0), (1, n_cells - 1), (3, n_cells // 2), (3, n_cells // 2 + 1), (n_slots - 1, 5)):
                    flip(base, s, c * CS + 3)                      # (flipping again restores the byte)
                assert ds.scrub()[2] == 0
                ds.free()
                want_ds.free()
    finally:
        small.close()
        ref.close()


@pytest.mark.parametrize("mode", [2, 0])
def test_fake_source_through_four_batches_the_last_one_short(pkg, oracle, mode):
    """The fake source through the batch loop (csrc/batch_loop.hpp) with both node buffers handed on and a short last batch: 1 MiB of
    staging cuts 7 slots of 2^12 cells into batches of 2, 2, 2 and 1 -- for the compact / roots-only build, whose roots are the
    oracle's, and for the scrub after it, which finds nothing."""
    C, _ = oracle
    os.environ["CODEX_P2_STAGE_MB"] = "1"
    try:
        small = pkg.Context(0)
    finally:
        del os.environ["CODEX_P2_STAGE_MB"]
    try:
        ds = build(small, config(pkg, n_cells=4096, n_slots=7, seed=77), mode)
        want = np.stack([C.fake_slot_root(C.slot_seed(77, s), CS, CS * CPB, 4096, 4) for s in range(7)])
        assert np.array_equal(ds.local_roots(), want)
        g, bad, n = ds.scrub()
        assert (g, n, bad.shape) == (LEVEL[mode], 0, (0, 2))
        ds.free()
    finally:
        small.close()


def test_multi_merged_report_equals_single_context(pkg, sctx, tmp_path):
    """Three contexts on one device, by whole slots (each shard compact) and cut by units (cells of the slot, not of the unit)."""
    base = str(tmp_path / "slot")
    data = write_files(base, n_slots=7)
    cfg = config(pkg, base, n_slots=7)
    changes = ((0, 0), (2, 63), (3, 17), (3, 18), (4, 40), (6, 33))
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
            assert md.scrub()[2] == 0
            ref = build(sctx, cfg, mode)                           # the single-context report to match
            for s, c in changes:
                flip(base, s, c * CS + 1)
            want = ref.scrub()
            got = md.scrub()
            assert got[0] == want[0] == LEVEL[mode]
            assert pairs(got[1]) == pairs(want[1]) == expect(set(changes), mode) and got[2] == want[2]
            got = md.scrub(2, 3, cap=2)                             # a range across shard borders, capped
            sub = [p for p in pairs(want[1]) if 2 <= p[0] <= 4]
            assert pairs(got[1]) == sub[:2] and got[2] == len(sub)
            assert md.scrub(cap=0)[2] == want[2]
            restore(base, data)
            assert md.scrub()[2] == 0
            ref.free()
            md.free()
    finally:
        m.close()
