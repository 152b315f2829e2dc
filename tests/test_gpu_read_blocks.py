"""GPU suite: the verified read-back -- cp2_datasets_read_blocks and cp2_dataset_read_blocks read listed blocks from the slot files, check
them on the device against the block roots the datasets keep and return bytes, roots and paths together.  Expected bytes are the files'
(or cp2_gen_fake_cells'), expected roots and paths are cp2_dataset_block_proofs', expected verdicts are what cp2_dataset_scrub names.
Every comparison is bit-exact.  One refusal of the header's list cannot be reached through the boundary -- a cp2_dataset whose kept layers
are those of unit builds exists only inside a cp2_multi_dataset -- and is held by tests/test_read_blocks_cpu.py alone."""
import ctypes
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CP2_OK, CP2_ERR_INVALID, CP2_ERR_IO = 0, -1, -5
ENTROPY = 123457
GEOMS = {"b128": (2048, 65536, 4096), "b8": (128, 4096, 256), "b2": (128, 4096, 64), "b1": (128, 4096, 32)}
DEPTH = {"b128": 7, "b8": 3, "b2": 1, "b1": 1}
N_SLOTS = 3


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


def conf(geom, base=None, n_slots=N_SLOTS, seed=5):
    cs, bs, nc = geom
    return dict(maxDepth=16, maxLog2NSlots=max(1, (n_slots - 1).bit_length()), cellSize=cs, blockSize=bs, nSlots=n_slots, nCells=nc, nSamples=5,
                seed=seed, file=base)


def write_files(base, geom, n_slots=N_SLOTS, seed=1):
    cs, _, nc = geom
    rng = np.random.default_rng(seed)
    data = {}
    for k in range(n_slots):
        data[k] = rng.integers(1, 256, nc * cs, dtype=np.uint8)          # no zero byte: a hole always differs
        data[k].tofile("%s%d.dat" % (base, k))
    return data


def flip(base, slot, offset):
    with open("%s%d.dat" % (base, slot), "r+b") as f:
        f.seek(offset)
        v = f.read(1)
        f.seek(offset)
        f.write(bytes([v[0] ^ 0x5A]))


def rows_of(data, reqs, bs):
    return np.stack([data[s][b * bs:(b + 1) * bs] for s, b in reqs])


def shuffled_requests(nb, seed, n_slots=N_SLOTS):
    """every block of every slot in shuffled order, some of them twice"""
    reqs = [(s, b) for s in range(n_slots) for b in range(nb)]
    rng = np.random.default_rng(seed)
    reqs += [reqs[int(i)] for i in rng.integers(0, len(reqs), max(2, len(reqs) // 8))]
    return [reqs[int(i)] for i in rng.permutation(len(reqs))]


def last_error(ctx):
    return ctx.L.cp2_last_error(ctx.h).decode()


# ---- 1: clean ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("source", ["file", "fake"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_clean_blocks_come_back_with_their_proofs(pkg, sctx, tmp_path, name, source, mode):
    cs, bs, nc = GEOMS[name]
    nb = nc // (bs // cs)
    base = str(tmp_path / "slot") if source == "file" else None
    if source == "file":
        data = write_files(base, GEOMS[name])
    else:
        data = {s: sctx.gen_fake_cells(sctx.slot_seed(5, s), 0, nc, cs).reshape(-1) for s in range(N_SLOTS)}
    ds = build(sctx, pkg.make_config(**conf(GEOMS[name], base)), mode)
    assert ds.block_proof_depth == DEPTH[name]
    reqs = shuffled_requests(nb, nb)
    want_roots, want_paths = ds.block_proofs(reqs)
    got, roots, paths, status, n_ok = ds.read_blocks(reqs)
    assert (status == pkg.READ_OK).all() and n_ok == len(reqs)
    assert got.tobytes() == rows_of(data, reqs, bs).tobytes()
    assert roots.tobytes() == want_roots.tobytes() and paths.tobytes() == want_paths.tobytes()
    # the many-dataset form over the same dataset: packed paths of one depth are the same bytes
    got2, roots2, paths2, off, status2, n_ok2 = sctx.read_blocks([ds], [(0, s, b) for s, b in reqs])
    assert got2.tobytes() == got.tobytes() and roots2.tobytes() == roots.tobytes() and paths2.tobytes() == paths.tobytes()
    assert off.tolist() == [DEPTH[name] * i for i in range(len(reqs) + 1)] and status2.tolist() == status.tolist() and n_ok2 == n_ok
    assert ds.read_blocks([])[3].size == 0 and ds.read_blocks([])[4] == 0
    ds.free()


# ---- 2: damage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["b8", "b128"])
def test_damage_is_found_where_a_scrub_finds_it_and_repair_heals_it(pkg, sctx, tmp_path, name, mode):
    cs, bs, nc = GEOMS[name]
    nb, cpb = nc // (bs // cs), bs // cs
    base = str(tmp_path / "slot")
    data = write_files(base, GEOMS[name], n_slots=4)
    ds = build(sctx, pkg.make_config(**conf(GEOMS[name], base, n_slots=4)), mode)
    flip(base, 0, 2 * bs)                                              # the first byte of a block
    flip(base, 0, 5 * bs + bs - 1)                                     # the last byte of a block
    flip(base, 3, nb * bs - 7)                                         # the last block of the last slot
    with open("%s1.dat" % base, "r+b") as f:                           # cut in the middle of block 4
        f.truncate(4 * bs + 100)
    with open("%s2.dat" % base, "r+b") as f:                           # cut at a block boundary
        f.truncate((nb - 2) * bs)
    g, bad, _ = ds.scrub()
    named = sorted({(int(s), int(i) // cpb if g == pkg.SCRUB_CELL else int(i)) for s, i in bad})
    assert named == sorted([(0, 2), (0, 5), (3, nb - 1)] + [(1, b) for b in range(4, nb)] + [(2, nb - 2), (2, nb - 1)])
    assert g == (pkg.SCRUB_CELL if mode == 1 else pkg.SCRUB_BLOCK)
    reqs = shuffled_requests(nb, 3, n_slots=4)
    want_roots, want_paths = ds.block_proofs(reqs)
    got, roots, paths, status, n_ok = ds.read_blocks(reqs)
    want_status = np.array([pkg.READ_DAMAGED if r in named else pkg.READ_OK for r in reqs], dtype=np.uint32)
    assert status.tolist() == want_status.tolist() and n_ok == int((want_status == pkg.READ_OK).sum())
    want = rows_of(data, reqs, bs)
    want[want_status == pkg.READ_DAMAGED] = 0
    assert got.tobytes() == want.tobytes()
    assert roots.tobytes() == want_roots.tobytes() and paths.tobytes() == want_paths.tobytes()      # the kept nodes, damaged or not
    # the originals put back through repair: the same requests come back OK
    st, n_written = ds.repair_blocks(named, rows_of(data, named, bs))
    assert (st == pkg.REPAIR_MATCH).all() and n_written == len(named)
    got, roots, paths, status, n_ok = ds.read_blocks(reqs)
    assert (status == pkg.READ_OK).all() and n_ok == len(reqs) and got.tobytes() == rows_of(data, reqs, bs).tobytes()
    ds.free()


# ---- 3: many datasets ----------------------------------------------------------------------------------------------------------------
def test_many_datasets_in_one_pass_equal_the_single_calls(pkg, sctx, tmp_path):
    bs = 4096
    bases = [str(tmp_path / ("d%d_" % k)) for k in range(3)]
    data = [write_files(bases[0], GEOMS["b8"], seed=10), write_files(bases[1], GEOMS["b8"], seed=11), write_files(bases[2], GEOMS["b2"], seed=12)]
    a = build(sctx, pkg.make_config(**conf(GEOMS["b8"], bases[0])), 2)
    b = build(sctx, pkg.make_config(**conf(GEOMS["b8"], bases[1])), 1)
    # b2 compact, through a fill session: every block proved out of a built twin, then cp2_fill_finish
    twin = build(sctx, pkg.make_config(**conf(GEOMS["b2"], bases[2])), 2)
    every = [(s, blk) for s in range(N_SLOTS) for blk in range(2)]
    _, proof = twin.block_proofs(every)
    session = sctx.fill(pkg.make_config(**conf(GEOMS["b2"], bases[2])), twin.local_roots())
    st, n_new = session.add(every, rows_of(data[2], every, bs), proof)
    assert n_new == len(every)
    c = session.finish()
    twin.free()
    d = build(sctx, pkg.make_config(**conf(GEOMS["b1"], None, seed=9)), 2)
    sets = [a, b, c, d, a]
    nbs = [8, 8, 2, 1, 8]
    rng = np.random.default_rng(77)
    reqs = []
    for _ in range(60):
        k = int(rng.integers(0, 5))
        reqs.append((k, int(rng.integers(0, N_SLOTS)), int(rng.integers(0, nbs[k]))))
    reqs += [(0, 1, 6), (4, 1, 6), (1, 2, 0), (2, 0, 1)]               # the planted ones are asked for, the first under both listings
    reqs = [reqs[int(i)] for i in rng.permutation(len(reqs))]
    flip(bases[0], 1, 6 * bs + 9)
    flip(bases[1], 2, 77)
    got, roots, paths, off, status, n_ok = sctx.read_blocks(sets, reqs)
    depth = [3, 3, 1, 1, 3]
    assert off.tolist() == np.concatenate([[0], np.cumsum([depth[k] for k, _, _ in reqs])]).tolist()
    assert paths.shape[0] == off[-1]
    seen_damage = 0
    for k, ds in enumerate(sets):
        mine = [i for i, r in enumerate(reqs) if r[0] == k]
        g1, r1, p1, s1, ok1 = ds.read_blocks([reqs[i][1:] for i in mine])
        assert got[mine].tobytes() == g1.tobytes() and roots[mine].tobytes() == r1.tobytes() and status[mine].tolist() == s1.tolist()
        for j, i in enumerate(mine):
            assert paths[int(off[i]):int(off[i + 1])].tobytes() == p1[j].tobytes()
            want_damaged = (reqs[i][0] in (0, 4) and reqs[i][1:] == (1, 6)) or reqs[i] == (1, 2, 0)
            assert status[i] == (pkg.READ_DAMAGED if want_damaged else pkg.READ_OK)
            seen_damage += want_damaged
            if not want_damaged and k != 3:
                s, blk = reqs[i][1:]
                assert got[i].tobytes() == data[(0, 1, 2, None, 0)[k]][s][blk * bs:(blk + 1) * bs].tobytes()
    assert seen_damage >= 3 and n_ok == len(reqs) - seen_damage
    fake = [i for i, r in enumerate(reqs) if r[0] == 3]
    for i in fake:
        assert got[i].tobytes() == sctx.gen_fake_cells(sctx.slot_seed(9, reqs[i][1]), 0, 32, 128).tobytes()
    # check only, no data: the same statuses, roots and paths
    none, roots2, paths2, off2, status2, n_ok2 = sctx.read_blocks(sets, reqs, check_only=True, want_data=False)
    assert none is None and roots2.tobytes() == roots.tobytes() and paths2.tobytes() == paths.tobytes() and off2.tolist() == off.tolist()
    assert status2.tolist() == status.tolist() and n_ok2 == n_ok
    # neither roots nor paths wanted
    st = np.full(len(reqs), 9, dtype=np.uint32)
    rq = np.array(reqs, dtype=np.uint64)
    hs = (ctypes.c_void_p * 5)(*[x.h for x in sets])
    assert sctx.L.cp2_datasets_read_blocks(sctx.h, hs, 5, rq.ctypes.data, len(reqs), 1, None, None, None, None, st.ctypes.data, None) == CP2_OK
    assert st.tolist() == status.tolist()
    for x in (a, b, c, d):
        x.free()
    session.free()


# ---- 4: chunk edges -------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as g
job = json.loads(sys.argv[1])
pkg = g.load_package()
ctx = pkg.Context(0)
ctx.set_keep_trees(2)
ds = ctx.dataset(pkg.make_config(**job["config"]))
reqs = job["reqs"]
for name, offset in job["flips"]:                  # the damage comes after the build, as in the parent
    with open(name, "r+b") as f:
        f.seek(offset)
        v = f.read(1)
        f.seek(offset)
        f.write(bytes([v[0] ^ 0x5A]))
import hashlib
def digest(r):
    data, roots, paths, status, n_ok = r
    return {"status": status.tolist(), "n_ok": n_ok, "roots": hashlib.sha256(roots.tobytes()).hexdigest(), "paths": hashlib.sha256(paths.tobytes()).hexdigest(),
            "data": None if data is None else hashlib.sha256(np.asarray(data).tobytes()).hexdigest()}
out = {"pageable": digest(ds.read_blocks(reqs))}
import torch
pinned = torch.empty(len(reqs) * 65536, dtype=torch.uint8).pin_memory()
out["pinned"] = digest(ds.read_blocks(reqs, data=pinned.numpy().reshape(len(reqs), 65536)))
out["null"] = digest(ds.read_blocks(reqs, check_only=True, want_data=False))
ds.free()
ctx.close()
print(json.dumps(out), flush=True)
""" % ROOT


def test_chunk_edges_pageable_pinned_and_null(pkg, sctx, tmp_path):
    """1 MiB of staging and 64 KiB blocks: 17 requests in chunks of 8, 8 and 1, damage at the last of a chunk, the first of the next and the
    lone last one; the verdicts and every output equal those of one chunk under the default staging"""
    import hashlib
    cs, bs, nc = GEOMS["b128"]
    base = str(tmp_path / "slot")
    write_files(base, GEOMS["b128"])
    rng = np.random.default_rng(17)
    reqs = [(int(rng.integers(0, N_SLOTS)), int(b)) for b in rng.permutation(128)[:17]]
    c = conf(GEOMS["b128"], base)
    ds = build(sctx, pkg.make_config(**c), 2)
    for i in (7, 8, 16):
        flip(base, reqs[i][0], reqs[i][1] * bs + 1000 + i)
    data, roots, paths, status, n_ok = ds.read_blocks(reqs)
    ds.free()
    assert [i for i in range(17) if status[i] == pkg.READ_DAMAGED] == [7, 8, 16] and n_ok == 14
    want = {"status": status.tolist(), "n_ok": 14, "roots": hashlib.sha256(roots.tobytes()).hexdigest(), "paths": hashlib.sha256(paths.tobytes()).hexdigest(),
            "data": hashlib.sha256(data.tobytes()).hexdigest()}
    flips = []
    for i in (7, 8, 16):                                               # the bytes back: the child builds from whole files and damages them itself
        flip(base, reqs[i][0], reqs[i][1] * bs + 1000 + i)
        flips.append(("%s%d.dat" % (base, reqs[i][0]), reqs[i][1] * bs + 1000 + i))
    clean = {k: v for k, v in os.environ.items() if not k.startswith("CODEX_P2_")}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps({"config": c, "reqs": reqs, "flips": flips})], capture_output=True, text=True, timeout=200,
                       env=dict(clean, CODEX_P2_STAGE_MB="1", CP2_TRACE="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert got["pageable"] == want and got["pinned"] == want and got["null"] == dict(want, data=None)
    lines = [l for l in r.stderr.splitlines() if "read blocks:" in l]
    assert len(lines) == 3 and all("1 dataset(s), 17 request(s), 3 chunk(s)" in l and "3 damaged" in l for l in lines), r.stderr[-2000:]


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched(pkg, sctx, tmp_path):
    bs = 4096
    base = str(tmp_path / "slot")
    write_files(base, GEOMS["b8"])
    good = build(sctx, pkg.make_config(**conf(GEOMS["b8"], base)), 2)
    rootsonly = build(sctx, pkg.make_config(**conf(GEOMS["b8"], base)), 0)
    small_cell = build(sctx, pkg.make_config(**conf((64, 4096, 256), None)), 2)
    big_block = build(sctx, pkg.make_config(**conf((128, 8192, 256), None)), 2)
    other = pkg.Context(0)
    foreign = build(other, pkg.make_config(**conf(GEOMS["b8"], base)), 2)
    L = sctx.L
    n = 3
    rq = np.array([(0, 0, 1), (0, 2, 7), (0, 1, 0)], dtype=np.uint64)

    def call(ctx=sctx.h, sets=(good,), req=rq, n=n, flags=0, data=True, roots=True, paths=True, off=True, status=True, n_ds=None, word=None):
        hs = None if sets is None else (ctypes.c_void_p * max(len(sets), 1))(*[None if x is None else x.h for x in sets])
        bufs = {"data": np.full(3 * bs, 0xA5, dtype=np.uint8), "roots": np.full(96, 0xA5, dtype=np.uint8), "paths": np.full(9 * 32, 0xA5, dtype=np.uint8),
                "off": np.full(4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), "status": np.full(3, 0xA5A5A5A5, dtype=np.uint32)}
        ok = ctypes.c_size_t(4242)
        p = lambda name, on: bufs[name].ctypes.data if on else None
        r = L.cp2_datasets_read_blocks(ctx, hs, (len(sets) if sets is not None else 1) if n_ds is None else n_ds, None if req is None else req.ctypes.data, n, flags,
                                       p("data", data), p("roots", roots), p("paths", paths), p("off", off), p("status", status), ctypes.byref(ok))
        assert r == CP2_ERR_INVALID, (r, word)
        assert ok.value == 4242 and all((v.view(np.uint8) == 0xA5).all() for v in bufs.values()), word
        if word is not None:
            assert word in last_error(sctx), (word, last_error(sctx))

    call(ctx=None)
    call(sets=None, word="must not be NULL")
    call(status=False, word="must not be NULL")
    call(req=None, word="must not be NULL")
    call(data=False, word="data is NULL without CP2_READ_CHECK_ONLY")
    call(off=False, word="paths without path_off")
    call(paths=False, word="path_off without paths")
    call(flags=2, word="unknown flag bits 0x2")
    call(flags=3, word="unknown flag bits 0x2")
    call(sets=(good, None), word="dataset 1: NULL dataset")
    call(sets=(good, good, foreign), word="dataset 2: it belongs to another context")
    call(sets=(good, small_cell), word="dataset 1: cell_size 64")
    call(sets=(good, big_block), word="dataset 1: cell_size 128, block_size 8192")
    call(sets=(good, rootsonly), word="dataset 1: block proofs: this dataset keeps only its slot roots")
    call(req=np.array([(0, 0, 1), (1, 2, 7), (0, 1, 0)], dtype=np.uint64), word="request 1: dataset index 1 is not below n_ds = 1")
    call(req=np.array([(0, 0, 1), (0, 2, 7), (0, 3, 0)], dtype=np.uint64), word="request 2: slot 3 is not inside the local range 0 + 3")
    call(req=np.array([(0, 0, 8), (0, 2, 7), (0, 1, 0)], dtype=np.uint64), word="request 0: block 8 of slot 0 is not below nBlocks = 8")
    # the single form: its own NULL rules, block proofs' words for a roots-only dataset
    st = np.full(3, 0xA5A5, dtype=np.uint32)
    sb = np.array([(0, 1), (2, 7), (1, 0)], dtype=np.uint64)
    assert L.cp2_dataset_read_blocks(good.h, sb.ctypes.data, 3, 0, None, None, None, st.ctypes.data, None) == CP2_ERR_INVALID
    assert "data is NULL" in last_error(sctx)
    assert L.cp2_dataset_read_blocks(rootsonly.h, sb.ctypes.data, 3, 1, None, None, None, st.ctypes.data, None) == CP2_ERR_INVALID
    assert "keeps only its slot roots" in last_error(sctx) and (st == 0xA5A5).all()
    # n == 0 is fine with nothing at all
    ok = ctypes.c_size_t(4242)
    assert L.cp2_datasets_read_blocks(sctx.h, None, 0, None, 0, 0, None, None, None, None, None, ctypes.byref(ok)) == CP2_OK and ok.value == 0
    for x in (good, rootsonly, small_cell, big_block, foreign):
        x.free()
    other.close()


# ---- 6: an I/O error ----------------------------------------------------------------------------------------------------------------------
def test_a_lost_slot_file_is_an_io_error_and_no_file_byte_stays(pkg, sctx, tmp_path):
    bs = 4096
    base = str(tmp_path / "slot")
    data = write_files(base, GEOMS["b8"])
    ds = build(sctx, pkg.make_config(**conf(GEOMS["b8"], base)), 2)
    os.remove(base + "2.dat")
    reqs = np.array(shuffled_requests(8, 4), dtype=np.uint64)
    n = reqs.shape[0]
    out = np.full((n, bs), 0, dtype=np.uint8)                          # (the files hold no zero byte: any byte of theirs would show)
    roots, paths, st = np.full(n * 32, 0xA5, dtype=np.uint8), np.full(n * 96, 0xA5, dtype=np.uint8), np.full(n, 0xA5A5, dtype=np.uint32)
    ok = ctypes.c_size_t(4242)
    r = sctx.L.cp2_dataset_read_blocks(ds.h, reqs.ctypes.data, n, 0, out.ctypes.data, roots.ctypes.data, paths.ctypes.data, st.ctypes.data, ctypes.byref(ok))
    assert r == CP2_ERR_IO and last_error(sctx) == "cannot open " + base + "2.dat"
    assert ok.value == 4242 and (roots == 0xA5).all() and (paths == 0xA5).all() and (st == 0xA5A5).all()
    assert not out.any()
    # the context goes on working
    keep = [(s, b) for s, b in reqs.tolist() if s != 2]
    got, _, _, status, n_ok = ds.read_blocks(keep)
    assert n_ok == len(keep) and got.tobytes() == rows_of(data, keep, bs).tobytes()
    ds.free()


# ---- 7: read-only ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_a_read_with_damage_present_changes_nothing(pkg, sctx, tmp_path, mode):
    bs = 4096
    base = str(tmp_path / "slot")
    write_files(base, GEOMS["b8"])
    ds = build(sctx, pkg.make_config(**conf(GEOMS["b8"], base)), mode)
    before = {s: ds.proof_input(s, ENTROPY).json() for s in range(N_SLOTS)} if mode == 1 else None
    roots_before, proofs_before = ds.local_roots().tobytes(), ds.block_proofs([(s, b) for s in range(N_SLOTS) for b in range(8)])
    if mode == 2:
        before = {s: ds.proof_input(s, ENTROPY).json() for s in range(N_SLOTS)}
    flip(base, 1, 3 * bs + 5)
    stamp = {s: (os.stat("%s%d.dat" % (base, s)).st_mtime_ns, open("%s%d.dat" % (base, s), "rb").read()) for s in range(N_SLOTS)}
    _, _, _, status, n_ok = ds.read_blocks([(s, b) for s in range(N_SLOTS) for b in range(8)])
    assert n_ok == 23 and status[8 + 3] == pkg.READ_DAMAGED
    assert ds.tree_mode == mode and ds.local_roots().tobytes() == roots_before
    after = ds.block_proofs([(s, b) for s in range(N_SLOTS) for b in range(8)])
    assert after[0].tobytes() == proofs_before[0].tobytes() and after[1].tobytes() == proofs_before[1].tobytes()
    assert stamp == {s: (os.stat("%s%d.dat" % (base, s)).st_mtime_ns, open("%s%d.dat" % (base, s), "rb").read()) for s in range(N_SLOTS)}
    flip(base, 1, 3 * bs + 5)                                          # the byte back: the proof inputs are those from before, byte for byte
    assert {s: ds.proof_input(s, ENTROPY).json() for s in range(N_SLOTS)} == before
    ds.free()
