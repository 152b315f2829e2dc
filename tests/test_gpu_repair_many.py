"""GPU suite: cp2_datasets_repair_blocks_many -- replacement blocks of many datasets judged in one pass and written back -- set beside
twin datasets repaired one at a time with cp2_dataset_repair_blocks and cp2_dataset_repair_blocks_proved.  Expected verdicts follow from
how each candidate is made (the right bytes, a flipped byte, the right bytes under another block's path, another dataset's bytes), expected
block roots, trees and paths come from the oracles (c_oracle.hash_cells / merkle_tree, poseidon2_ref.merkle_proof), never from the call
under test; the round trip alone feeds cp2_datasets_read_blocks' own output back in.  Every comparison is bit-exact.  Geometries: cell 128 /
block 4096 with 256, 64 and 32 cells a slot (8, 2 and 1 blocks), and one case of 2048 / 65536 with 4096 cells (128 blocks)."""
import ctypes
import faulthandler
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CP2_OK, CP2_ERR_INVALID, CP2_ERR_IO = 0, -1, -5
ENTROPY = 123457
OLD_NS = 1_600_000_000 * 10**9
GEOMS = {"b128": (2048, 65536, 4096), "b8": (128, 4096, 256), "b2": (128, 4096, 64), "b1": (128, 4096, 32)}
N_SLOTS = 2
# the six file-sourced datasets of a world: (geometry, residency, built with a cache); the call lists dataset 1 a second time at index 6
SPEC = (("b8", 1, True), ("b8", 2, True), ("b2", 0, False), ("b1", 2, False), ("b2", 1, False), ("b8", 0, True))
LISTED = (0, 1, 2, 3, 4, 5, 1)


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


def build(ctx, cfg, mode, **kw):
    ctx.set_keep_trees(mode)
    try:
        ds = ctx.dataset(cfg, **kw)
    finally:
        ctx.set_keep_trees(-1)
    assert ds.tree_mode == mode
    return ds


def config(pkg, geom, base=None, n_slots=N_SLOTS, seed=5):
    cs, bs, nc = geom
    return pkg.make_config(maxDepth=16, maxLog2NSlots=max(1, (n_slots - 1).bit_length()), cellSize=cs, blockSize=bs, nSlots=n_slots, nCells=nc,
                           nSamples=5, seed=seed, file=base)


def slot_bytes(geom, seed, n_slots=N_SLOTS):
    cs, _, nc = geom
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 256, nc * cs, dtype=np.uint8) for _ in range(n_slots)]          # no zero byte: a hole always differs


def write_files(base, data):
    for k, d in enumerate(data):
        path = "%s%d.dat" % (base, k)
        d.tofile(path)
        os.utime(path, ns=(OLD_NS, OLD_NS + k))


def flip(base, slot, offset, keep_mtime=False):
    path = "%s%d.dat" % (base, slot)
    st = os.stat(path)
    with open(path, "r+b") as f:
        f.seek(offset)
        v = f.read(1)
        f.seek(offset)
        f.write(bytes([v[0] ^ 0x5A]))
    if keep_mtime:
        os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))


def sha_files(base, n_slots=N_SLOTS):
    return [hashlib.sha256(open("%s%d.dat" % (base, k), "rb").read()).hexdigest() for k in range(n_slots)]


# ---- the oracle's side: computed once per (geometry, seed), shared, never changed ---------------------------------------------------------------
_slots = {}


def oracle_slots(oracle, name, seed, n_slots=N_SLOTS):
    """(per-slot bytes, per-slot big-tree layers as integers) of the slots slot_bytes(GEOMS[name], seed) makes"""
    key = (name, seed, n_slots)
    if key not in _slots:
        C, _ = oracle
        cs, bs, _ = GEOMS[name]
        cpb = bs // cs
        data, layers = slot_bytes(GEOMS[name], seed, n_slots), []
        for cells in data:
            leaves = C.hash_cells(cells, cs, threads=16)
            roots = np.stack([C.merkle_tree(leaves[b * cpb:(b + 1) * cpb])[-1][0] for b in range(leaves.shape[0] // cpb)])
            layers.append([C.array_to_felts(layer) for layer in C.merkle_tree(roots)])
        _slots[key] = (data, layers)
    return _slots[key]


def oracle_path(oracle, layers, b):
    C, P = oracle
    prf = P.merkle_proof(layers, b)
    assert P.reconstruct_root(prf) == layers[-1][0]
    return C.felts_to_array(prf["merklePath"])


def block(data, s, b, bs):
    return data[s][b * bs:(b + 1) * bs]


def pack(paths):
    """per-request lists of 32-byte rows -> (packed rows, path_off)"""
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.uint64)
    rows = np.concatenate([np.asarray(p, dtype=np.uint8).reshape(-1, 32) for p in paths] + [np.zeros((0, 32), np.uint8)])
    return rows, off


def raw_many(ctx, sets, reqs, data, paths=None, off=None, flags=0, caches=None, n=None, n_ds=None, no=()):
    """the C call itself with sentinel outputs: (return value, statuses, n_written, last error)"""
    rq = np.ascontiguousarray(np.asarray(reqs, dtype=np.uint64).reshape(-1, 3))
    n = rq.shape[0] if n is None else n
    hs = (ctypes.c_void_p * max(len(sets), 1))(*[None if d is None else d.h for d in sets])
    status = np.full(max(n, 1), 7, dtype=np.uint32)
    w = ctypes.c_size_t(99)
    cps = None if caches is None else (ctypes.c_char_p * len(sets))(*[c.encode() if c else None for c in caches])
    d = np.ascontiguousarray(data)
    arg = lambda name, a: None if name in no or a is None else a.ctypes.data
    r = ctx.L.cp2_datasets_repair_blocks_many(ctx.h, None if "ds" in no else hs, len(sets) if n_ds is None else n_ds, arg("req", rq), arg("data", d),
                                              arg("paths", paths), arg("path_off", off), n, flags, cps, arg("status", status), ctypes.byref(w))
    return r, status[:n], w.value, ctx.L.cp2_last_error(ctx.h).decode()


class World:
    """the six datasets of SPEC under one directory, their files, caches and oracle trees"""

    def __init__(self, pkg, oracle, ctx, root):
        self.pkg, self.ctx, self.bases, self.caches, self.sets, self.data, self.layers = pkg, ctx, [], [], [], [], []
        for k, (name, mode, cached) in enumerate(SPEC):
            base = os.path.join(str(root), "d%d_" % k)
            data, layers = oracle_slots(oracle, name, 100 + k)
            write_files(base, data)
            cache = os.path.join(str(root), "d%d.cache" % k) if cached else None
            ds = build(ctx, config(pkg, GEOMS[name], base), mode, **({"cache": cache} if cached else {}))
            assert np.array_equal(ds.local_roots(), np.stack([oracle[0].felt_bytes(l[-1][0]) for l in layers]))
            self.bases.append(base); self.caches.append(cache); self.sets.append(ds); self.data.append(data); self.layers.append(layers)
        self.before = [[ds.proof_input(s, ENTROPY).json() for s in range(N_SLOTS)] for ds in self.sets]

    def listed(self):
        return [self.sets[k] for k in LISTED]

    def cache_loads(self, k):
        """free dataset k and build it again from its cache: True when the cache was loaded, False when it was rebuilt"""
        name, mode, _ = SPEC[k]
        st = os.stat(self.caches[k])
        self.sets[k].free()
        self.sets[k] = build(self.ctx, config(self.pkg, GEOMS[name], self.bases[k]), mode, cache=self.caches[k])
        return os.stat(self.caches[k]).st_ino == st.st_ino

    def free(self):
        for ds in self.sets:
            ds.free()


# the damage: (dataset, slot, block, the mtime moves); dataset 0's second file is damaged with its mtime moved, so its cache is stale before
# the repair and stays stale; every other cached dataset suffers bit rot only
DAMAGE = ((0, 0, 2, False), (0, 0, 7, False), (0, 1, 5, True), (1, 0, 0, False), (1, 1, 3, False), (1, 1, 6, False), (2, 0, 1, False), (2, 1, 0, False),
          (3, 1, 0, False), (4, 0, 0, False), (4, 1, 1, False), (5, 0, 4, False), (5, 1, 7, False))


def many_requests(oracle, world):
    """(req, candidates, per-request path rows, expected statuses): the damaged blocks with the right bytes, and among them wrong blocks, right
    blocks under another block's path and another dataset's blocks, for intact places; dataset 1 is named through index 1 and index 6"""
    M, X = world.pkg.REPAIR_MATCH, world.pkg.REPAIR_MISMATCH
    bs = 4096
    rows = []
    for j, (k, s, b, _) in enumerate(DAMAGE):
        whole = SPEC[k][1] == 0 or j % 2 == 0
        rows.append((6 if k == 1 and j % 2 else k, k, s, b, block(world.data[k], s, b, bs), oracle_path(oracle, world.layers[k][s], b) if whole else [], M))
    def intact(k, s, b, cand, path, want, idx=None):
        rows.append((k if idx is None else idx, k, s, b, cand, path, want))
    wrong = block(world.data[0], 1, 1, bs).copy()
    wrong[-1] ^= 1                                                                            # the last byte of the last cell
    intact(0, 1, 1, wrong, [], X)
    wrong = block(world.data[5], 0, 0, bs).copy()
    wrong[0] ^= 0x80
    intact(5, 0, 0, wrong, oracle_path(oracle, world.layers[5][0], 0), X)
    intact(1, 0, 5, block(world.data[1], 0, 5, bs), oracle_path(oracle, world.layers[1][0], 4), X, idx=6)   # the right block, block 4's path
    intact(2, 1, 1, block(world.data[2], 1, 1, bs), oracle_path(oracle, world.layers[2][0], 1), X)          # the right block, the other slot's path
    intact(1, 0, 2, block(world.data[0], 0, 2, bs), [], X)                                                  # dataset 0's block of the same place
    intact(5, 1, 2, block(world.data[0], 1, 2, bs), oracle_path(oracle, world.layers[5][1], 2), X)
    intact(3, 0, 0, block(world.data[3], 0, 0, bs), [], M)                                                  # right blocks for intact places: written again
    intact(4, 1, 0, block(world.data[4], 1, 0, bs), oracle_path(oracle, world.layers[4][1], 0), M)
    order = np.random.default_rng(5).permutation(len(rows))
    rows = [rows[int(i)] for i in order]
    req = [(idx, s, b) for idx, _, s, b, _, _, _ in rows]
    return req, np.stack([r[4] for r in rows]), [r[5] for r in rows], [r[6] for r in rows]


def do_damage(world):
    for k, s, b, moves in DAMAGE:
        flip(world.bases[k], s, b * 4096 + 11 + b, keep_mtime=not moves)


# ---- 1: the call beside the per-dataset loop -------------------------------------------------------------------------------------------------
def test_six_datasets_in_one_call_equal_twins_repaired_one_by_one(pkg, oracle, sctx, tmp_path):
    worlds = []
    for tag in ("many", "loop"):
        (tmp_path / tag).mkdir()
        worlds.append(World(pkg, oracle, sctx, tmp_path / tag))
    many, loop = worlds
    clean = [sha_files(b) for b in many.bases]
    assert clean == [sha_files(b) for b in loop.bases]
    for w in worlds:
        do_damage(w)
        assert [sha_files(b) for b in w.bases] != clean
    req, cand, paths, want = many_requests(oracle, many)
    rows, off = pack(paths)
    assert any(len(p) for p in paths) and any(not len(p) for p in paths) and {len(p) for p in paths} >= {0, 1, 3}
    # check only first: the verdicts, nothing written
    damaged = [sha_files(b) for b in many.bases]
    st, n_written = sctx.repair_blocks_many(many.listed(), req, cand, rows, off, check_only=True)
    assert st.tolist() == want and n_written == 0 and [sha_files(b) for b in many.bases] == damaged
    # the call
    st, n_written = sctx.repair_blocks_many(many.listed(), req, cand, rows, off, cache_paths=[many.caches[k] for k in LISTED])
    print("statuses", st.tolist(), "written", n_written)
    assert st.tolist() == want and n_written == want.count(pkg.REPAIR_MATCH)
    # the loop: per dataset (both listings of dataset 1 together), the path-less requests through cp2_dataset_repair_blocks and the proved
    # ones through cp2_dataset_repair_blocks_proved, each in request order
    got, total = [None] * len(req), 0
    for k, ds in enumerate(loop.sets):
        mine = [i for i, r in enumerate(req) if LISTED[r[0]] == k]
        flat = [i for i in mine if not len(paths[i])]
        proved = [i for i in mine if len(paths[i])]
        if flat:
            s1, w1 = ds.repair_blocks([req[i][1:] for i in flat], cand[flat], cache_path=loop.caches[k])
            total += w1
            for i, v in zip(flat, s1.tolist()):
                got[i] = v
        if proved:
            s2, w2 = ds.repair_blocks_proved([req[i][1:] for i in proved], cand[proved], np.stack([paths[i] for i in proved]), cache_path=loop.caches[k])
            total += w2
            for i, v in zip(proved, s2.tolist()):
                got[i] = v
    assert got == st.tolist() and total == n_written
    for w in worlds:
        assert [sha_files(b) for b in w.bases] == clean
        for k, ds in enumerate(w.sets):
            assert ds.scrub()[2] == 0, k
            assert [ds.proof_input(s, ENTROPY).json() for s in range(N_SLOTS)] == w.before[k], k
    # the stamps: bit rot repaired with the cache named -> the next build loads it; a cache that was stale before stays stale
    loads = [[w.cache_loads(k) for k in (0, 1, 5)] for w in worlds]
    print("cache loaded (datasets 0, 1, 5): many", loads[0], "loop", loads[1])
    assert loads[0] == loads[1] == [False, True, True]
    for w in worlds:
        w.free()


# ---- 2: the round trip ---------------------------------------------------------------------------------------------------------------------------
def test_paths_of_a_verified_read_back_go_straight_back_in(pkg, oracle, sctx, tmp_path):
    bs = 4096
    specs = (("b8", 2, 201), ("b2", 1, 202), ("b8", 1, 203))
    bases, data, sets = [], [], []
    for k, (name, mode, seed) in enumerate(specs):
        base = str(tmp_path / ("r%d_" % k))
        d, _ = oracle_slots(oracle, name, seed)
        write_files(base, d)
        bases.append(base); data.append(d); sets.append(build(sctx, config(pkg, GEOMS[name], base), mode))
    clean = [sha_files(b) for b in bases]
    reqs = [(0, 0, 3), (1, 1, 1), (2, 1, 7), (0, 1, 0), (2, 0, 2), (1, 0, 0), (0, 0, 4)]
    for k, s, b in reqs[:5]:
        flip(bases[k], s, b * bs + 100)
    _, roots, paths, off, status, n_ok = sctx.read_blocks(sets, reqs, check_only=True, want_data=False)
    assert status.tolist() == [pkg.READ_DAMAGED] * 5 + [pkg.READ_OK] * 2 and n_ok == 2
    bad = [i for i in range(len(reqs)) if status[i] == pkg.READ_DAMAGED]
    cand = np.stack([block(data[k], s, b, bs) for k, s, b in reqs])
    # the whole answer, as it came: packed paths and offsets of all seven requests
    st, w = sctx.repair_blocks_many(sets, reqs, cand, paths, off)
    assert st.tolist() == [pkg.REPAIR_MATCH] * len(reqs) and w == len(reqs)
    assert [sha_files(b) for b in bases] == clean and all(ds.scrub()[2] == 0 for ds in sets)
    # the kept block roots it returned are the oracle's
    for i in bad:
        k, s, b = reqs[i]
        _, layers = oracle_slots(oracle, specs[k][0], specs[k][2])
        assert roots[i].tobytes() == oracle[0].felt_bytes(layers[s][0][b]).tobytes()
    for ds in sets:
        ds.free()


# ---- 3: chunks, pageable and pinned ----------------------------------------------------------------------------------------------------------------
def test_three_chunks_with_packed_paths_across_them_pageable_and_pinned(pkg, oracle, monkeypatch, capfd, tmp_path):
    """64 KiB blocks under 1 MiB of staging: chunks of 8 requests, 20 requests, so three chunks; the requests alternate between the path-less
    and the proved kind and between a compact and a roots-only dataset, so every chunk stages its own range of the packed paths."""
    import torch
    monkeypatch.setenv("CODEX_P2_STAGE_MB", "1")
    monkeypatch.setenv("CP2_TRACE", "1")
    ctx = pkg.Context(0)
    cs, bs, nc = GEOMS["b128"]
    M, X = pkg.REPAIR_MATCH, pkg.REPAIR_MISMATCH
    bases, data, layers, sets = [], [], [], []
    for k, mode in enumerate((2, 0)):
        base = str(tmp_path / ("c%d_" % k))
        d, l = oracle_slots(oracle, "b128", 300 + k, n_slots=1)
        write_files(base, d)
        bases.append(base); data.append(d); layers.append(l); sets.append(build(ctx, config(pkg, GEOMS["b128"], base, n_slots=1), mode))
    rng = np.random.default_rng(9)
    blocks = [int(b) for b in rng.permutation(128)[:20]]
    reqs, cand, paths, want = [], [], [], []
    for i, b in enumerate(blocks):
        k = i % 2
        whole = k == 1 or i % 4 == 0
        c = block(data[k], 0, b, bs).copy()
        path = oracle_path(oracle, layers[k][0], b) if whole else []
        kind = i % 5
        if kind == 1:
            c[int(rng.integers(0, bs))] ^= 0x04
        elif kind == 3 and whole:
            path = oracle_path(oracle, layers[k][0], b ^ 1)
        reqs.append((k, 0, b)); cand.append(c); paths.append(path); want.append(X if kind == 1 or (kind == 3 and whole) else M)
    rows, off = pack(paths)
    cand = np.stack(cand)
    assert X in want and M in want and int(off[8]) not in (0, int(off[-1])) and int(off[16]) != int(off[8])
    capfd.readouterr()
    st, w = ctx.repair_blocks_many(sets, reqs, cand, rows, off, check_only=True)
    err = capfd.readouterr().err
    print("pageable", st.tolist())
    assert st.tolist() == want and w == 0
    line = [l for l in err.splitlines() if "repair many:" in l]
    assert len(line) == 1 and "2 dataset(s), 20 request(s), 3 chunk(s)" in line[0] and "%d with paths" % sum(1 for p in paths if len(p)) in line[0], err[-2000:]
    pinned = torch.from_numpy(cand.copy()).pin_memory()
    st, w = ctx.repair_blocks_many(sets, reqs, pinned.numpy(), rows, off, check_only=True)
    print("pinned  ", st.tolist())
    assert st.tolist() == want and w == 0
    for ds in sets:
        ds.free()
    ctx.close()


# ---- 4: the fake source ------------------------------------------------------------------------------------------------------------------------------
def test_check_only_on_fake_source_datasets(pkg, oracle, sctx, tmp_path):
    cs, bs, nc = GEOMS["b8"]
    cpb = bs // cs
    fake = build(sctx, config(pkg, GEOMS["b8"], None, seed=9), 2)
    fake0 = build(sctx, config(pkg, GEOMS["b2"], None, seed=4), 0)
    base = str(tmp_path / "f_")
    d, _ = oracle_slots(oracle, "b8", 400)
    write_files(base, d)
    filed = build(sctx, config(pkg, GEOMS["b8"], base), 1)
    C = oracle[0]
    cells = lambda seed, s, b, n_cells: C.gen_fake_cells(C.slot_seed(seed, s), b * cpb, cpb, cs).reshape(-1)
    # the roots-only fake dataset needs the oracle's path: its two block roots, then the tree over them
    leaves = C.hash_cells(C.gen_fake_cells(C.slot_seed(4, 1), 0, 64, cs).reshape(-1), cs, threads=4)
    roots0 = np.stack([C.merkle_tree(leaves[b * cpb:(b + 1) * cpb])[-1][0] for b in range(2)])
    layers0 = [C.array_to_felts(layer) for layer in C.merkle_tree(roots0)]
    spoiled = cells(9, 0, 6, nc).copy()
    spoiled[5] ^= 1
    reqs = [(0, 1, 3), (2, 0, 1), (0, 0, 6), (1, 1, 1), (0, 0, 0)]
    cand = np.stack([cells(9, 1, 3, nc), block(d, 0, 1, bs), spoiled, cells(4, 1, 1, 64), cells(9, 0, 0, nc)])
    rows, off = pack([[], [], [], oracle_path(oracle, layers0, 1), []])
    M, X = pkg.REPAIR_MATCH, pkg.REPAIR_MISMATCH
    before = sha_files(base)
    st, w = sctx.repair_blocks_many([fake, fake0, filed], reqs, cand, rows, off, check_only=True)
    assert st.tolist() == [M, M, X, M, M] and w == 0 and sha_files(base) == before
    r, status, written, msg = raw_many(sctx, [fake, fake0, filed], reqs, cand, rows, off)
    assert r == CP2_ERR_INVALID and "request 0" in msg and "fake source" in msg and status.tolist() == [7] * 5 and written == 99 and sha_files(base) == before
    for ds in (fake, fake0, filed):
        ds.free()


# ---- 5: a file that cannot be written fails alone ----------------------------------------------------------------------------------------------------
def test_an_unwritable_file_fails_alone_and_the_first_one_is_named(pkg, oracle, sctx, tmp_path):
    bs = 4096
    bases, data, sets, caches = [], [], [], []
    for k, mode in enumerate((2, 1, 2)):
        base = str(tmp_path / ("u%d_" % k))
        d, _ = oracle_slots(oracle, "b8", 500 + k)
        write_files(base, d)
        cache = str(tmp_path / ("u%d.cache" % k))
        bases.append(base); data.append(d); caches.append(cache); sets.append(build(sctx, config(pkg, GEOMS["b8"], base), mode, cache=cache))
    clean = [sha_files(b) for b in bases]
    reqs = [(2, 1, 4), (0, 0, 1), (1, 1, 6), (1, 0, 2), (2, 0, 0), (0, 1, 3), (1, 1, 0), (2, 1, 7)]
    for k, s, b in reqs:
        flip(bases[k], s, b * bs + 9, keep_mtime=True)
    for name in ("%s1.dat" % bases[1], "%s1.dat" % bases[2]):         # two slot files are now directories: (1, 1) comes first
        os.remove(name)
        os.mkdir(name)
    cand = np.stack([block(data[k], s, b, bs) for k, s, b in reqs])
    r, status, written, msg = raw_many(sctx, sets, reqs, cand, caches=caches)
    U, M = pkg.REPAIR_UNWRITTEN, pkg.REPAIR_MATCH
    print("statuses", status.tolist(), "written", written, "error", msg)
    assert r == CP2_ERR_IO and status.tolist() == [U, M, U, M, M, M, U, U] and written == 4
    assert "cannot write" in msg and msg.count(".dat") == 1 and ("%s1.dat" % bases[1]) in msg, msg
    assert sha_files(bases[0]) == clean[0] and sha_files(bases[1], 1) == clean[1][:1] and sha_files(bases[2], 1) == clean[2][:1]
    assert not os.listdir("%s1.dat" % bases[1]) and not os.listdir("%s1.dat" % bases[2])
    # dataset 0 was written whole and restamped: its cache still loads
    st0 = os.stat(caches[0])
    sets[0].free()
    sets[0] = build(sctx, config(pkg, GEOMS["b8"], bases[0]), 2, cache=caches[0])
    assert os.stat(caches[0]).st_ino == st0.st_ino and sets[0].scrub()[2] == 0
    for ds in sets:
        ds.free()


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_index_and_touch_nothing(pkg, oracle, sctx, tmp_path):
    bs = 4096
    other = pkg.Context(0)
    base = str(tmp_path / "x_")
    d, layers = oracle_slots(oracle, "b8", 600)
    write_files(base, d)
    cache = str(tmp_path / "x.cache")
    a = build(sctx, config(pkg, GEOMS["b8"], base), 2, cache=cache)
    same = build(sctx, config(pkg, GEOMS["b8"], base), 1)                                  # another handle over the same base name
    base2 = str(tmp_path / "y_")
    d2, layers2 = oracle_slots(oracle, "b2", 601)
    write_files(base2, d2)
    bare = build(sctx, config(pkg, GEOMS["b2"], base2), 0)
    big = build(sctx, config(pkg, GEOMS["b128"], None, n_slots=1), 2)                      # another cell and block size
    alien = build(other, config(pkg, GEOMS["b8"], None), 2)
    fake = build(sctx, config(pkg, GEOMS["b8"], None, seed=3), 2)
    flip(base, 0, 5 * bs, keep_mtime=True)
    files, cached = sha_files(base) + sha_files(base2), open(cache, "rb").read()
    sets = [a, bare, a, same]
    good = [(0, 0, 5), (1, 1, 1), (2, 1, 2), (3, 0, 0)]
    cand = np.stack([block(d, 0, 5, bs), block(d2, 1, 1, bs), block(d, 1, 2, bs), block(d, 0, 0, bs)])
    p_bare = oracle_path(oracle, layers2[1], 1)
    rows, off = pack([[], p_bare, [], []])
    r, status, _, _ = raw_many(sctx, sets, good, cand, rows, off, flags=1)
    assert r == CP2_OK and status.tolist() == [pkg.REPAIR_MATCH] * 4                      # the call these refusals are variations of
    p3 = oracle_path(oracle, layers[0], 0)
    cases = [
        (dict(flags=2), "unknown flag bits 0x2"),
        (dict(no=("path_off",)), "paths without path_off"),
        (dict(no=("paths",)), "path_off without paths"),
        (dict(no=("ds",)), "must not be NULL"),
        (dict(no=("req",)), "must not be NULL"),
        (dict(no=("data",)), "must not be NULL"),
        (dict(no=("status",)), "must not be NULL"),
        (dict(off=off + 1), "path_off[0] is 1"),
        (dict(sets=[a, None, a, same]), "dataset 1: NULL dataset"),
        (dict(sets=[a, bare, alien, same]), "dataset 2: it belongs to another context"),
        (dict(sets=[a, bare, a, big]), "dataset 3: cell_size 2048"),
        (dict(reqs=[(0, 0, 5), (4, 1, 1), (2, 1, 2), (3, 0, 0)]), "request 1: dataset index 4"),
        (dict(off=np.array([0, 0, 1, 0, 0], dtype=np.uint64)), "request 2: path_off decreases from 1 to 0"),
        (dict(rows=np.concatenate([p3, p3]), off=np.array([0, 0, 1, 1, 3], dtype=np.uint64)), "request 3: a path of 2 row(s)"),
        (dict(rows=None, off=None), "request 1: an empty path for dataset 1, which keeps only its slot roots"),
        (dict(reqs=[(0, 0, 5), (1, 1, 1), (2, 2, 2), (3, 0, 0)]), "request 2: slot 2 is not inside the local range"),
        (dict(reqs=[(0, 0, 8), (1, 1, 1), (2, 1, 2), (3, 0, 0)]), "request 0: block 8 of slot 0 is not below nBlocks = 8"),
        (dict(reqs=[(0, 0, 5), (1, 1, 1), (2, 1, 2), (2, 0, 5)]), "request 3: (slot 0, block 5) of dataset 2 is the block of request 0 again"),     # one handle listed twice
        (dict(reqs=[(0, 0, 5), (1, 1, 1), (3, 0, 5), (3, 0, 0)]), "request 2: (slot 0, block 5) of dataset 3 is the block of request 0 again"),     # two handles, one base name
        (dict(sets=[a, bare, fake, same], flags=0), "request 2: dataset 2 has the fake source"),
        (dict(sets=[a, bare, fake, fake], reqs=[(0, 0, 5), (1, 1, 1), (2, 1, 2), (3, 1, 2)]), "request 3: (slot 1, block 2) of dataset 3 is the block of request 2 again"),
        # arguments before datasets before requests, and the lowest request wins
        (dict(flags=4, sets=[None, bare, a, same]), "unknown flag bits 0x4"),
        (dict(sets=[a, None, a, same], reqs=[(0, 0, 9), (1, 1, 1), (2, 1, 2), (3, 0, 0)]), "dataset 1: NULL dataset"),
        (dict(reqs=[(0, 0, 5), (1, 1, 2), (2, 1, 2), (0, 0, 5)]), "request 1: block 2 of slot 1 is not below nBlocks = 2"),
    ]
    for kw, words in cases:
        kw = dict(kw)
        flags = kw.pop("flags", 1 if "fake" not in words else 0)
        r, status, written, msg = raw_many(sctx, kw.pop("sets", sets), kw.pop("reqs", good), cand, kw.pop("rows", rows), kw.pop("off", off), flags=flags,
                                           caches=[cache, None, None, None], **kw)
        assert r == CP2_ERR_INVALID and words in msg, (words, r, msg)
        assert status.tolist() == [7] * 4 and written == 99, words
        assert sha_files(base) + sha_files(base2) == files and open(cache, "rb").read() == cached, words
    # nothing to do is fine, whatever else is NULL
    w = ctypes.c_size_t(99)
    assert sctx.L.cp2_datasets_repair_blocks_many(sctx.h, None, 0, None, None, None, None, 0, 0, None, None, ctypes.byref(w)) == CP2_OK and w.value == 0
    assert sctx.repair_blocks_many(sets, [], np.zeros(0, np.uint8))[1] == 0
    for ds in (a, same, bare, big, alien, fake):
        ds.free()
    other.close()
