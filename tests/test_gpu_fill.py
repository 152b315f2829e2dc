"""GPU suite: fill sessions -- cp2_fill_begin / _add / _missing / _finish / _free.  A session is fed the proved network blocks of its slots
in a shuffled order over several calls and must end in a compact dataset that is indistinguishable from the one cp2_dataset_build makes
from the same data: roots, dataset root, every block proof, input.json byte for byte.  Slot roots and one full set of compact layers are
also checked against oracle/poseidon2_ref.py, so the comparison does not rest on the library alone.  Every comparison is bit-exact."""
import faulthandler
import hashlib
import json
import os
import re
import stat
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CP2_ERR_INVALID, CP2_ERR_IO = -1, -5
ENTROPIES = (1234567, 99)
# name: (config, first_slot, n_local).  The reference default (16 blocks per slot), a slot of one block, slots of 2^10 blocks in a range
# that starts past slot 0, and 16 small blocks (cheap enough for the pure-Python oracle to build every tree).
GEOMS = {
    "default": (dict(maxDepth=32, maxLog2NSlots=8, cellSize=2048, blockSize=65536, nSlots=11, nCells=512, nSamples=5, seed=12345), 0, 11),
    "one_block": (dict(maxDepth=8, maxLog2NSlots=3, cellSize=128, blockSize=4096, nSlots=4, nCells=32, nSamples=3, seed=7), 0, 4),
    "b1024": (dict(maxDepth=16, maxLog2NSlots=3, cellSize=64, blockSize=256, nSlots=5, nCells=4096, nSamples=4, seed=31), 2, 3),
    "tiny16": (dict(maxDepth=8, maxLog2NSlots=2, cellSize=64, blockSize=256, nSlots=3, nCells=64, nSamples=3, seed=42), 0, 3),
}


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


def build_compact(ctx, cfg, first_slot=0, n_local=None, cache=None):
    ctx.set_keep_trees(2)
    try:
        ds = ctx.dataset(cfg, first_slot, n_local, cache=cache)
    finally:
        ctx.set_keep_trees(-1)
    assert ds.tree_mode == 2
    return ds


def n_blocks_of(cfg):
    return cfg.n_cells // (cfg.block_size // cfg.cell_size)


def fake_blocks(ctx, cfg, slot):
    """the bytes of one fake slot as (nBlocks, blockSize), from cp2_gen_fake_cells"""
    cells = ctx.gen_fake_cells(ctx.slot_seed(cfg.seed, slot), 0, cfg.n_cells, cfg.cell_size)
    return np.ascontiguousarray(cells).reshape(n_blocks_of(cfg), cfg.block_size)


class Source:
    """every block of local slots [first, first + n) with its path, from a built dataset: what the peers would send"""

    def __init__(self, ctx, cfg, ds, first, n, blocks_of=None):
        self.cfg, self.nb = cfg, n_blocks_of(cfg)
        self.pairs = [(s, b) for s in range(first, first + n) for b in range(self.nb)]
        self.roots, self.paths = ds.block_proofs(self.pairs)
        self.blocks = {s: (blocks_of(s) if blocks_of else fake_blocks(ctx, cfg, s)) for s in range(first, first + n)}
        self.index = {p: i for i, p in enumerate(self.pairs)}

    def data(self, pairs):
        return np.stack([self.blocks[s][b] for s, b in pairs]) if pairs else np.empty((0, self.cfg.block_size), dtype=np.uint8)

    def path(self, pairs):
        return np.stack([self.paths[self.index[p]] for p in pairs]) if pairs else np.empty((0, self.paths.shape[1], 32), dtype=np.uint8)


def add(f, src, pairs, data=None, paths=None):
    return f.add(pairs, src.data(pairs) if data is None else data, src.path(pairs) if paths is None else paths)


def uneven_calls(pairs, seed):
    """the pairs in a seeded shuffled order, cut into several calls of uneven size"""
    rng = np.random.default_rng(seed)
    order = [pairs[i] for i in rng.permutation(len(pairs))]
    cuts = sorted({0, len(order)} | {int(c) for c in rng.integers(0, len(order) + 1, 4)} | {min(1, len(order)), len(order) // 3})
    return [order[a:b] for a, b in zip(cuts, cuts[1:])]


def flip(a, index, mask=0x5A):
    out = a.copy()
    out.reshape(-1)[index] ^= mask
    return out


# ---- 1: a filled dataset equals the built one --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMS))
def test_filled_dataset_equals_the_built_one(pkg, oracle, golden, sctx, name):
    C, P = oracle
    cfgd, first, n_local = GEOMS[name]
    cfg = pkg.make_config(**cfgd)
    nb = n_blocks_of(cfg)
    built = build_compact(sctx, cfg, first, n_local)
    whole = built if n_local == cfg.n_slots else build_compact(sctx, cfg)
    all_roots = whole.local_roots()
    roots = built.local_roots()
    assert roots.tobytes() == all_roots[first:first + n_local].tobytes()
    src = Source(sctx, cfg, built, first, n_local)
    assert src.paths.shape[1] == built.block_proof_depth == max(1, (nb - 1).bit_length())

    f = sctx.fill(cfg, roots, first, n_local)
    calls = uneven_calls(src.pairs, seed=nb + n_local)
    assert len(calls) >= 3 or len(src.pairs) < 3
    left = len(src.pairs)
    for pairs in calls:
        status, n_new = add(f, src, pairs)
        assert (status == pkg.FILL_NEW).all() and n_new == len(pairs)
        left -= len(pairs)
        assert f.missing(0)[1] == left
    filled = f.finish()
    assert filled.tree_mode == 2

    assert filled.local_roots().tobytes() == roots.tobytes()
    for ds in (built, filled):
        ds.set_roots(all_roots if n_local != cfg.n_slots else None)
    assert filled.root().tobytes() == built.root().tobytes()
    got_roots, got_paths = filled.block_proofs(src.pairs)
    assert got_roots.tobytes() == src.roots.tobytes() and got_paths.tobytes() == src.paths.tobytes()
    for slot in range(first, first + n_local):
        for e in ENTROPIES:
            assert filled.proof_input(slot, e).json() == built.proof_input(slot, e).json(), (slot, e)
    if name == "default":
        assert filled.proof_input(3, 1234567).json() == golden("input_params_default.json")

    # the oracles' word: every slot root, and every compact layer of the filled dataset, rebuilt from the served proofs
    for k in range(n_local):
        slot = first + k
        if name == "tiny16":
            big = P.build_slot_tree_full(dict(cfgd), slot)[1]                      # poseidon2_ref alone: cells, block trees, big tree
        elif name == "default":
            block_roots = C.fake_slot_block_roots(C.slot_seed(cfg.seed, slot), cfg.cell_size, cfg.block_size, cfg.n_cells, 8)
            big = P.merkle_tree(C.array_to_felts(block_roots))
        else:
            assert roots[k].tobytes() == C.fake_slot_root(C.slot_seed(cfg.seed, slot), cfg.cell_size, cfg.block_size, cfg.n_cells, 8).tobytes()
            continue
        assert len(big) == built.block_proof_depth + 1
        assert pkg.array_to_felts(roots[k]) == [big[-1][0]]
        layer0 = got_roots[k * nb:(k + 1) * nb]
        assert pkg.array_to_felts(layer0) == big[0]
        for lvl in range(1, len(big) - 1):                                          # node j of layer lvl is the sibling of node j ^ 1
            kept = [got_paths[k * nb + ((j ^ 1) << lvl)][lvl] for j in range(len(big[lvl]))]
            assert pkg.array_to_felts(np.stack(kept)) == big[lvl], (slot, lvl)
        for j in range(nb):                                                         # and layer 0 once more, as the siblings of its nodes
            assert got_paths[k * nb + (j ^ 1)][0].tobytes() == layer0[j].tobytes()
    f.free()
    filled.free()
    if whole is not built:
        whole.free()
    built.free()


# ---- 2: verdicts, counts, the missing list, refusals ------------------------------------------------------------------------------------------
def test_verdicts_counts_and_refusals(pkg, sctx):
    cfgd, first, n_local = GEOMS["default"]
    cfg = pkg.make_config(**cfgd)
    nb = n_blocks_of(cfg)
    built = build_compact(sctx, cfg)
    roots = built.local_roots()
    src = Source(sctx, cfg, built, 0, 4)
    f = sctx.fill(cfg, roots)
    total = cfg.n_slots * nb
    everything = [(s, b) for s in range(cfg.n_slots) for b in range(nb)]
    miss, n = f.missing()
    assert n == total and [tuple(int(x) for x in r) for r in miss] == everything
    present = set()

    def check_missing():
        want = [p for p in everything if p not in present]
        assert f.missing(0)[1] == len(want)                                         # the counting form
        some, n_ = f.missing(5)                                                     # a cap below the count
        assert n_ == len(want) and [tuple(int(x) for x in r) for r in some] == want[:5]
        full, n_ = f.missing(total + 7)
        assert n_ == len(want) and [tuple(int(x) for x in r) for r in full] == want

    N, X, D = pkg.FILL_NEW, pkg.FILL_MISMATCH, pkg.FILL_DUPLICATE
    status, n_new = add(f, src, [(1, 4), (0, 0)])                                   # an earlier call
    assert status.tolist() == [N, N] and n_new == 2
    present |= {(1, 4), (0, 0)}
    check_missing()
    # one call: a flipped data byte, a flipped path byte, a right block under the wrong slot, a right block twice, a block already present
    pairs = [(0, 1), (0, 2), (2, 3), (0, 5), (3, 15), (0, 5), (1, 4), (3, 0)]
    data, paths = src.data(pairs), src.path(pairs)
    data[0] = flip(data[0], 70)
    paths[1] = flip(paths[1], 2 * 32 + 9, 0x01)
    data[2], paths[2] = src.blocks[1][3], src.path([(1, 3)])[0]                      # slot 1's block 3 and its path, stated as slot 2's
    status, n_new = f.add(pairs, data, paths)
    assert status.tolist() == [X, X, X, N, N, D, D, N] and n_new == 3
    present |= {(0, 5), (3, 15), (3, 0)}
    check_missing()
    status, n_new = add(f, src, [(0, 5), (0, 5), (0, 1)])                           # across calls, and a block that failed before
    assert status.tolist() == [D, D, N] and n_new == 1
    present.add((0, 1))
    check_missing()
    assert add(f, src, []) [1] == 0                                                 # n == 0

    # refusals: CP2_ERR_INVALID, the status array untouched, the index named
    L = sctx.L
    good = [(0, 7), (1, 7), (2, 7)]
    for bad, text in (((11, 0), r"request 1: slot 11"), ((1 << 40, 0), r"request 1: slot"), ((1, nb), r"request 1: block %d" % nb)):
        req = [good[0], bad, good[2]]
        status = np.full(3, 77, dtype=np.uint32)
        with pytest.raises(pkg.CodexP2Error) as e:
            f.add(req, src.data(good), src.path(good), status=status)
        assert e.value.status == CP2_ERR_INVALID and re.search(text, str(e.value)), str(e.value)
        assert status.tolist() == [77, 77, 77]
    d, p = src.data(good), src.path(good)
    sb = np.ascontiguousarray(np.asarray(good, dtype=np.uint64))
    status = np.full(3, 77, dtype=np.uint32)
    ptr = lambda a: pkg._p(a)                                                       # noqa: E731
    for args in ((None, ptr(d), ptr(p), 3, ptr(status)), (ptr(sb), None, ptr(p), 3, ptr(status)), (ptr(sb), ptr(d), None, 3, ptr(status)),
                 (ptr(sb), ptr(d), ptr(p), 3, None)):
        assert L.cp2_fill_add(f.h, *args, None) == CP2_ERR_INVALID
        assert "NULL" in L.cp2_last_error(sctx.h).decode()
    assert L.cp2_fill_add(None, ptr(sb), ptr(d), ptr(p), 3, ptr(status), None) == CP2_ERR_INVALID
    assert status.tolist() == [77, 77, 77]
    check_missing()                                                                 # nothing of the refused calls was kept
    f.free()
    built.free()


def test_begin_refuses_what_the_builder_refuses(pkg, sctx):
    cfgd = GEOMS["default"][0]
    roots = np.zeros((11, 32), dtype=np.uint8)
    for change, first, n_local in ((dict(nCells=96), 0, 11), (dict(nCells=500), 0, 11), (dict(blockSize=65000), 0, 11), ({}, 0, 0), ({}, 5, 7),
                                   ({}, 12, 1), (dict(maxDepth=-1), 0, 11)):
        cfg = pkg.make_config(**dict(cfgd, **change))
        with pytest.raises(pkg.CodexP2Error) as e:
            pkg.FillSession(sctx, cfg, roots[:n_local], first, n_local)
        assert e.value.status == CP2_ERR_INVALID, (change, first, n_local)
        if change.get("nCells") != 96:                                                # (the builder leaves the power of two to the proof input)
            with pytest.raises(pkg.CodexP2Error):
                sctx.dataset(cfg, first, n_local)


# ---- 3: finish too early ------------------------------------------------------------------------------------------------------------------------
def test_finish_too_early_then_complete_then_closed(pkg, sctx):
    cfgd, first, n_local = GEOMS["tiny16"]
    cfg = pkg.make_config(**cfgd)
    built = build_compact(sctx, cfg)
    src = Source(sctx, cfg, built, 0, 3)
    f = sctx.fill(cfg, built.local_roots())
    held_back = [(1, 6), (1, 9), (2, 15)]
    rest = [p for p in src.pairs if p not in held_back]
    assert add(f, src, rest)[1] == len(rest)
    with pytest.raises(pkg.CodexP2Error) as e:
        f.finish()
    assert e.value.status == CP2_ERR_INVALID and "3 block(s)" in str(e.value) and "(slot 1, block 6)" in str(e.value), str(e.value)
    assert [tuple(int(x) for x in r) for r in f.missing()[0]] == held_back       # the session stays usable
    status, n_new = add(f, src, held_back[::-1])
    assert (status == pkg.FILL_NEW).all() and n_new == 3
    filled = f.finish()
    assert filled.local_roots().tobytes() == built.local_roots().tobytes()
    status = np.full(1, 77, dtype=np.uint32)
    with pytest.raises(pkg.CodexP2Error) as e:
        f.add([(0, 0)], src.data([(0, 0)]), src.path([(0, 0)]), status=status)
    assert e.value.status == CP2_ERR_INVALID and "finished" in str(e.value) and status.tolist() == [77]
    with pytest.raises(pkg.CodexP2Error) as e:
        f.finish()
    assert e.value.status == CP2_ERR_INVALID
    f.free()
    for ds in (built, filled):                                                      # the dataset outlives its session
        ds.set_roots()
    assert filled.proof_input(2, 99).json() == built.proof_input(2, 99).json()
    filled.free()
    built.free()


# ---- 4, 5: slot files, a file that cannot be written, the cache ---------------------------------------------------------------------------------
FILE_GEOM = dict(maxDepth=16, maxLog2NSlots=2, cellSize=128, blockSize=4096, nSlots=3, nCells=256, nSamples=5, seed=1)


def file_source(pkg, ctx, directory):
    """three slot files of random bytes in `directory`/src, a compact dataset built from them, and what the peers would send"""
    os.makedirs(os.path.join(directory, "src"))
    base = os.path.join(directory, "src", "slot")
    rng = np.random.default_rng(4)
    nb = FILE_GEOM["nCells"] * FILE_GEOM["cellSize"] // FILE_GEOM["blockSize"]
    data = {s: rng.integers(0, 256, (nb, FILE_GEOM["blockSize"]), dtype=np.uint8) for s in range(3)}
    for s in range(3):
        data[s].tofile("%s%d.dat" % (base, s))
    cfg = pkg.make_config(file=base, **FILE_GEOM)
    built = build_compact(ctx, cfg)
    return cfg, built, Source(ctx, cfg, built, 0, 3, blocks_of=lambda s: data[s]), data


def test_files_are_written_and_an_unwritable_file_leaves_its_blocks_missing(pkg, sctx, tmp_path):
    cfg_src, built, src, data = file_source(pkg, sctx, str(tmp_path))
    out = tmp_path / "out"
    out.mkdir()
    base = str(out / "slot")
    cfg = pkg.make_config(file=base, **FILE_GEOM)
    nb = src.nb
    f = sctx.fill(cfg, built.local_roots())
    N, U = pkg.FILL_NEW, pkg.FILL_UNWRITTEN
    first_call = [(0, 3), (0, 0)]
    assert add(f, src, first_call)[0].tolist() == [N, N]
    assert os.path.exists(base + "0.dat") and not os.path.exists(base + "1.dat")    # created by the session

    # the file of slot 1 cannot be created: a read-only directory (for a user whom modes do not bind, a directory in the file's place)
    def block():
        if os.geteuid() == 0:
            os.mkdir(base + "1.dat")
        else:
            os.chmod(str(out), stat.S_IRUSR | stat.S_IXUSR)

    def unblock():
        if os.geteuid() == 0:
            os.rmdir(base + "1.dat")
        else:
            os.chmod(str(out), stat.S_IRWXU)

    pairs = [(2, 1), (1, 5), (0, 7), (1, 0), (2, 2), (1, 5), (0, 7)]                # the last two: repeats of a failing and of a written block
    block()
    try:
        with pytest.raises(pkg.CodexP2Error) as e:
            add(f, src, pairs)
    finally:
        unblock()
    assert e.value.status == CP2_ERR_IO and "slot1.dat" in str(e.value), str(e.value)
    # slot 0's file was there; slot 1 failed, slot 2 came after; the repeat of a block that stays missing is UNWRITTEN, not DUPLICATE
    assert e.value.fill_status.tolist() == [U, U, N, U, U, U, pkg.FILL_DUPLICATE] and e.value.n_new == 1
    still = [tuple(int(x) for x in r) for r in f.missing()[0]]
    assert all(p in still for p in pairs if p != (0, 7)) and (0, 7) not in still
    assert len(still) == 3 * nb - 3
    status, n_new = add(f, src, pairs)                                             # accepted once the directory is writable again
    assert status.tolist() == [N, N, pkg.FILL_DUPLICATE, N, N, pkg.FILL_DUPLICATE, pkg.FILL_DUPLICATE] and n_new == 4
    for pairs in uneven_calls([tuple(p) for p in f.missing()[0].tolist()], seed=5):
        assert (add(f, src, pairs)[0] == N).all()
    filled = f.finish()
    for s in range(3):
        assert open("%s%d.dat" % (base, s), "rb").read() == data[s].tobytes()
    assert filled.scrub()[2] == 0
    rebuilt = build_compact(sctx, cfg)
    for ds in (filled, rebuilt):
        ds.set_roots()
    assert filled.local_roots().tobytes() == rebuilt.local_roots().tobytes() == built.local_roots().tobytes()
    assert filled.proof_input(1, 1234567).json() == rebuilt.proof_input(1, 1234567).json()
    for h in (f, filled, rebuilt, built):
        h.free()


def test_finish_writes_the_cache_a_cached_build_loads(pkg, sctx, tmp_path):
    cfg_src, built, src, data = file_source(pkg, sctx, str(tmp_path))
    out = tmp_path / "out"
    out.mkdir()
    base, cache = str(out / "slot"), str(tmp_path / "kept.cache")
    cfg = pkg.make_config(file=base, **FILE_GEOM)
    f = sctx.fill(cfg, built.local_roots())
    for pairs in uneven_calls(src.pairs, seed=9):
        add(f, src, pairs)
    filled = f.finish(cache)
    roots = filled.local_roots()
    assert os.path.exists(cache) and roots.tobytes() == built.local_roots().tobytes()
    f.free()
    filled.free()
    # one byte of slot 2's block 5 changes behind the cache's back: same size, same mtime
    name = base + "2.dat"
    st = os.stat(name)
    with open(name, "r+b") as fh:
        fh.seek(5 * cfg.block_size + 17)
        fh.write(bytes([data[2][5][17] ^ 0xFF]))
    os.utime(name, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert os.stat(name).st_mtime_ns == st.st_mtime_ns and os.stat(name).st_size == st.st_size
    loaded = build_compact(sctx, cfg, cache=cache)
    assert loaded.local_roots().tobytes() == roots.tobytes()                        # the kept form was loaded: a rebuild sees the changed byte
    _, bad, n_bad = loaded.scrub()
    assert n_bad == 1 and bad.tolist() == [[2, 5]]
    fresh = build_compact(sctx, cfg)
    assert fresh.local_roots()[2].tobytes() != roots[2].tobytes() and fresh.local_roots()[:2].tobytes() == roots[:2].tobytes()
    for h in (loaded, fresh, built):
        h.free()


# ---- 6: a stated root that is not the slot's ------------------------------------------------------------------------------------------------------
def test_an_altered_slot_root_rejects_every_block_of_that_slot(pkg, sctx):
    cfgd, first, n_local = GEOMS["tiny16"]
    cfg = pkg.make_config(**cfgd)
    built = build_compact(sctx, cfg)
    src = Source(sctx, cfg, built, 0, 3)
    roots = built.local_roots().copy()
    roots[1] = flip(roots[1], 3, 0x01)
    f = sctx.fill(cfg, roots)
    status, n_new = add(f, src, src.pairs)
    want = [pkg.FILL_MISMATCH if s == 1 else pkg.FILL_NEW for s, _ in src.pairs]
    assert status.tolist() == want and n_new == 2 * src.nb
    assert [tuple(int(x) for x in r) for r in f.missing()[0]] == [(1, b) for b in range(src.nb)]
    with pytest.raises(pkg.CodexP2Error) as e:
        f.finish()
    assert e.value.status == CP2_ERR_INVALID and "%d block(s)" % src.nb in str(e.value) and "(slot 1, block 0)" in str(e.value)
    f.free()
    built.free()


def test_roots_of_at_least_r_are_reduced(pkg, sctx):
    """a stated root given as value + r names the same field element: its blocks prove"""
    R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    cfgd, first, n_local = GEOMS["one_block"]
    cfg = pkg.make_config(**cfgd)
    built = build_compact(sctx, cfg)
    src = Source(sctx, cfg, built, 0, 4)
    roots = built.local_roots().copy()
    v = pkg.array_to_felts(roots[2])[0] + R
    assert v < 1 << 256
    roots[2] = pkg.felt_bytes(v)
    f = sctx.fill(cfg, roots)
    assert (add(f, src, src.pairs)[0] == pkg.FILL_NEW).all()
    filled = f.finish()
    assert filled.local_roots().tobytes() == built.local_roots().tobytes()
    for h in (f, filled, built):
        h.free()


# ---- many chunks: the per-chunk offsets of requests, destination rows and paths, pageable and pinned ------------------------------------------
CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
import __graft_entry__ as g
pkg = g.load_package()
job = json.loads(sys.argv[1])
ctx = pkg.Context(0)
cand, paths, roots, reqs, bad_cand, bad_paths = (np.load(job[k]) for k in ("cand", "paths", "roots", "reqs", "bad_cand", "bad_paths"))
cfg = pkg.make_config(**job["config"])
import torch
out = {}
for kind in ("pageable", "pinned"):
    view = (lambda a: torch.from_numpy(a).pin_memory().numpy()) if kind == "pinned" else (lambda a: a)
    f = ctx.fill(cfg, roots)
    st1, new1 = f.add(reqs, view(bad_cand), bad_paths)              # some requests damaged: they stay missing
    missing = f.missing()[0]
    st2, new2 = f.add(reqs, view(cand), paths)                      # everything once more, right this time
    ds = f.finish()
    proofs = ds.block_proofs(reqs)
    out[kind] = {"st1": st1.tolist(), "new1": new1, "missing": missing.tolist(), "st2": st2.tolist(), "new2": new2,
                 "roots": hashlib.sha256(ds.local_roots().tobytes()).hexdigest(),
                 "proofs": hashlib.sha256(proofs[0].tobytes() + proofs[1].tobytes()).hexdigest()}
    ds.free()
    f.free()
ctx.close()
print(json.dumps(out), flush=True)
""" % ROOT


@pytest.mark.parametrize("stage_mb,n_cells,n_slots", [(1, 4096, 8), (80, 16384, 64)])
def test_many_chunks_pageable_and_pinned(pkg, oracle, sctx, tmp_path, stage_mb, n_cells, n_slots):
    """64 KiB blocks of 64-byte cells, fake source.  1 MiB of staging: chunks of 8 requests; 80 MiB: a chunk through the pinned ring (more
    than 32 MiB) and a smaller one; caller-pinned blocks read in place.  The requests come shuffled, so a chunk's destination rows lie all
    over layer 0.  Damaged requests are planted by index (i % 3 == 1: the last byte of the block, i % 7 == 2: one byte of one path level) on
    both sides of every chunk edge: exactly those are MISMATCH and stay missing; sent again right they are NEW and the rest DUPLICATE.  The
    finished dataset's roots are the C oracle's, and its roots and block proofs are the built dataset's."""
    C, _ = oracle
    cfgd = dict(maxDepth=32, maxLog2NSlots=max(1, (n_slots - 1).bit_length()), cellSize=64, blockSize=65536, nSlots=n_slots, nCells=n_cells,
                nSamples=3, seed=77)
    cfg = pkg.make_config(**cfgd)
    built = build_compact(sctx, cfg)
    src = Source(sctx, cfg, built, 0, n_slots)
    reqs = [src.pairs[i] for i in np.random.default_rng(1).permutation(len(src.pairs))]
    cand, paths = src.data(reqs), src.path(reqs)
    bad_cand, bad_paths = cand.copy(), paths.copy()
    depth = paths.shape[1]
    bad = [i % 3 == 1 or i % 7 == 2 for i in range(len(reqs))]
    for i in range(len(reqs)):
        if i % 3 == 1:
            bad_cand[i, -1] ^= 1
        elif i % 7 == 2:
            bad_paths[i, i % depth, (i * 11) % 31] ^= 0x10
    roots = built.local_roots()
    for s in range(n_slots):
        assert roots[s].tobytes() == C.fake_slot_root(C.slot_seed(77, s), 64, 65536, n_cells, 8).tobytes()
    want_proofs = built.block_proofs(reqs)
    names = {}
    for k, a in (("cand", cand.reshape(-1)), ("paths", paths), ("roots", roots), ("reqs", np.array(reqs, dtype=np.uint64)),
                 ("bad_cand", bad_cand.reshape(-1)), ("bad_paths", bad_paths)):
        names[k] = str(tmp_path / (k + ".npy"))
        np.save(names[k], a)
    built.free()
    clean = {k: v for k, v in os.environ.items() if not k.startswith("CODEX_P2_")}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(dict(names, config=cfgd))], capture_output=True, text=True, timeout=200,
                       env=dict(clean, CODEX_P2_STAGE_MB=str(stage_mb)))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    N, X, D = pkg.FILL_NEW, pkg.FILL_MISMATCH, pkg.FILL_DUPLICATE
    for kind in ("pageable", "pinned"):
        o = got[kind]
        assert o["st1"] == [X if b else N for b in bad] and o["new1"] == bad.count(False), kind
        assert o["missing"] == sorted(list(p) for p, b in zip(reqs, bad) if b), kind
        assert o["st2"] == [N if b else D for b in bad] and o["new2"] == bad.count(True), kind
        assert o["roots"] == hashlib.sha256(roots.tobytes()).hexdigest(), kind
        assert o["proofs"] == hashlib.sha256(want_proofs[0].tobytes() + want_proofs[1].tobytes()).hexdigest(), kind
