"""GPU suite: block proofs -- cp2_dataset_block_proofs serves (block root, Merkle path to the slot root) from what a dataset keeps,
cp2_blocks_verify checks candidate blocks and their paths against bare slot roots, cp2_dataset_repair_blocks_proved repairs with proved
blocks in every residency mode, the roots-only one included.  Expected values come from the oracles (c_oracle for hashes and trees,
poseidon2_ref.merkle_proof for the proofs), never from another call of the library except in the round trip.  Every comparison is
bit-exact."""
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
CP2_ERR_INVALID = -1
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ENTROPY = 123457
OLD_NS = 1_600_000_000 * 10**9
# (cell size, block size, cells per slot): 128 blocks (depth 7), the testMain.hs geometry (8 blocks), 2 blocks, the singleton
GEOMS = {"b128": (2048, 65536, 4096), "b8": (128, 4096, 256), "b2": (128, 4096, 64), "b1": (128, 4096, 32)}
N_SLOTS = 4


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


def config(pkg, geom, n_slots=N_SLOTS, base=None, seed=5):
    cs, bs, nc = geom
    return pkg.make_config(maxDepth=16, maxLog2NSlots=max(1, (n_slots - 1).bit_length()), cellSize=cs, blockSize=bs, nSlots=n_slots, nCells=nc,
                           nSamples=5, seed=seed, file=base)


# ---- the oracle's side ------------------------------------------------------------------------------------------------------------
def oracle_block_roots(C, cells, cs, bs):
    """the root of every network block of one slot's bytes (blocks/bn254.nim:60-67): (nBlocks, 32) uint8"""
    cpb = bs // cs
    leaves = C.hash_cells(cells, cs, threads=16)
    return np.stack([C.merkle_tree(leaves[b * cpb:(b + 1) * cpb])[-1][0] for b in range(leaves.shape[0] // cpb)])


class OracleSlot:
    """the big tree of one slot over its block roots and merkleProof(bigTree, b) of any block, from the oracles alone"""

    def __init__(self, C, P, block_roots, python_tree=False):
        self.C, self.P = C, P
        self.block_roots = block_roots
        if python_tree:
            self.layers = P.merkle_tree(C.array_to_felts(block_roots))
        else:
            self.layers = [C.array_to_felts(l) for l in C.merkle_tree(block_roots)]
        self.root = C.felt_bytes(self.layers[-1][0])
        self.depth = len(self.layers) - 1

    def path(self, b):
        prf = self.P.merkle_proof(self.layers, b)
        assert self.P.reconstruct_root(prf) == self.layers[-1][0]
        return self.C.felts_to_array(prf["merklePath"])


_cache = {}


def oracle_dataset(C, P, name, source, tmp_root):
    """N_SLOTS slots of geometry `name`, fake source (seed 5) or slot files of random bytes: (config kwargs, per-slot bytes, OracleSlots)"""
    key = (name, source)
    if key in _cache:
        return _cache[key]
    cs, bs, nc = GEOMS[name]
    base = None
    data, slots = [], []
    if source == "file":
        base = os.path.join(str(tmp_root), "%s_slot" % name)
        rng = np.random.default_rng(nc)
    for s in range(N_SLOTS):
        if source == "file":
            cells = rng.integers(1, 256, nc * cs, dtype=np.uint8)
            cells.tofile("%s%d.dat" % (base, s))
        else:
            cells = C.gen_fake_cells(C.slot_seed(5, s), 0, nc, cs).reshape(-1)
        data.append(cells)
        slots.append(OracleSlot(C, P, oracle_block_roots(C, cells, cs, bs)))
    _cache[key] = (base, data, slots)
    return _cache[key]


@pytest.fixture(scope="module")
def files_root(tmp_path_factory):
    return tmp_path_factory.mktemp("block_proofs")


# ---- 1: served proofs equal the oracle's ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("source", ["file", "fake"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_served_proofs_equal_the_oracles(pkg, oracle, sctx, files_root, name, source, mode):
    C, P = oracle
    cs, bs, nc = GEOMS[name]
    base, _, slots = oracle_dataset(C, P, name, source, files_root)
    nb = nc // (bs // cs)
    ds = build(sctx, config(pkg, GEOMS[name], base=base), mode)
    assert ds.block_proof_depth == slots[0].depth == (7, 3, 1, 1)[list(GEOMS).index(name)]
    assert np.array_equal(ds.local_roots(), np.stack([s.root for s in slots]))
    rng = np.random.default_rng(nb)
    reqs = [(s, b) for s in (0, 3) for b in range(nb)]                # every block of two slots
    reqs += [(int(rng.integers(1, 3)), int(rng.integers(0, nb))) for _ in range(min(nb, 40))]   # a sample (with repeats) over the rest
    want_roots = np.stack([slots[s].block_roots[b] for s, b in reqs])
    want_paths = np.stack([slots[s].path(b) for s, b in reqs])
    roots, paths = ds.block_proofs(reqs)
    assert roots.tobytes() == want_roots.tobytes()
    assert paths.tobytes() == want_paths.tobytes()
    if name == "b1":
        assert not paths.any()                                        # the singleton's path: one zero entry
    roots2, paths2 = ds.block_proofs(reqs)                            # serving is read-only: the same bytes again
    assert roots2.tobytes() == roots.tobytes() and paths2.tobytes() == paths.tobytes()
    ds.free()


# ---- 2: verify accepts exactly the right ones -------------------------------------------------------------------------------------------
def flip_byte(a, index, mask=0x5A):
    out = a.copy()
    out.reshape(-1)[index] ^= mask
    return out


def test_verify_accepts_exactly_the_right_ones(pkg, oracle, sctx, files_root):
    C, P = oracle
    cs, bs, nc = GEOMS["b128"]
    _, data, slots = oracle_dataset(C, P, "b128", "fake", files_root)
    nb, depth = nc // (bs // cs), 7
    roots = np.stack([slots[0].root, slots[1].root])
    blocks = lambda s: data[s].reshape(nb, bs)                       # noqa: E731
    # all correct: every block of slot 0 and slot 1
    rb = [(s, b) for s in (0, 1) for b in range(nb)]
    cand = np.concatenate([blocks(0), blocks(1)])
    paths = np.stack([slots[s].path(b) for s, b in rb])
    status, got_roots = sctx.blocks_verify(cs, bs, nc, roots, rb, cand, paths)
    assert (status == pkg.BLOCK_MATCH).all()
    assert got_roots.tobytes() == np.concatenate([slots[0].block_roots, slots[1].block_roots]).tobytes()
    # one damaged request at position K of a batch of otherwise correct ones
    batch = [(0, 5), (1, 77), (0, 127), (0, 0), (1, 126), (0, 64), (1, 1), (0, 33)]
    K = 5
    s, b = batch[K]
    good_d = np.stack([blocks(s_)[b_] for s_, b_ in batch])
    good_p = np.stack([slots[s_].path(b_) for s_, b_ in batch])
    X, M = pkg.BLOCK_MISMATCH, pkg.BLOCK_MATCH

    def run(rb_=None, d=None, p=None):
        st, _ = sctx.blocks_verify(cs, bs, nc, roots, batch if rb_ is None else rb_, good_d if d is None else d, good_p if p is None else p)
        return st.tolist()

    def replaced(a, row):
        out = a.copy()
        out[K] = row
        return out

    assert run() == [M] * len(batch)
    only_k = [M] * K + [X] + [M] * (len(batch) - K - 1)
    assert run(d=replaced(good_d, flip_byte(good_d[K], 3))) == only_k                       # a byte of the first cell
    assert run(d=replaced(good_d, flip_byte(good_d[K], bs - 1, 0x01))) == only_k            # the last byte of the last cell
    for lvl in range(depth):                                                                # one byte of each path level
        assert run(p=replaced(good_p, flip_byte(good_p[K], lvl * 32 + (lvl * 5) % 31, 0x01))) == only_k, lvl
    assert run(p=replaced(good_p, slots[s].path(b ^ 1))) == only_k                          # the right block with its neighbour's path
    assert run(p=replaced(good_p, slots[s].path(b + 2))) == only_k
    for wrong in ((s, b ^ 1), (s, b ^ 2), (s, b + 1), (s ^ 1, b)):                          # the wrong block index, the wrong root index
        rb_ = list(batch)
        rb_[K] = wrong
        assert run(rb_=rb_) == only_k, wrong
    # a sibling given as value + r is taken mod r: still a match
    lifted = good_p[K].copy()
    for lvl in (0, 3, 6):
        v = int.from_bytes(lifted[lvl].tobytes(), "little") + R_MOD
        assert v < 1 << 256
        lifted[lvl] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
    assert not np.array_equal(lifted, good_p[K])
    assert run(p=replaced(good_p, lifted)) == [M] * len(batch)
    # the same (root, block) twice is allowed: each gets its own verdict
    st, _ = sctx.blocks_verify(cs, bs, nc, roots, [batch[0], batch[0], batch[0]], np.stack([good_d[0], flip_byte(good_d[0], 100), good_d[0]]),
                               np.stack([good_p[0]] * 3))
    assert st.tolist() == [M, X, M]


def test_verify_the_singleton(pkg, oracle, sctx, files_root):
    C, P = oracle
    cs, bs, nc = GEOMS["b1"]
    _, data, slots = oracle_dataset(C, P, "b1", "fake", files_root)
    roots = np.stack([s.root for s in slots])
    rb = [(s, 0) for s in range(N_SLOTS)]
    cand = np.stack(data)
    paths = np.zeros((N_SLOTS, 1, 32), dtype=np.uint8)
    assert np.array_equal(np.stack([s.path(0) for s in slots]), paths)
    st, got = sctx.blocks_verify(cs, bs, nc, roots, rb, cand, paths)
    assert st.tolist() == [pkg.BLOCK_MATCH] * N_SLOTS and got.tobytes() == np.concatenate([s.block_roots for s in slots]).tobytes()
    paths[2, 0, 0] = 1                                                                      # a non-zero entry where the path holds zero
    st, _ = sctx.blocks_verify(cs, bs, nc, roots, rb, cand, paths)
    assert st.tolist() == [pkg.BLOCK_MATCH, pkg.BLOCK_MATCH, pkg.BLOCK_MISMATCH, pkg.BLOCK_MATCH]


@pytest.mark.parametrize("n_blocks", [3, 5, 6, 7])
def test_verify_without_a_dataset_over_odd_block_counts(pkg, oracle, sctx, n_blocks):
    """Slots no cp2_dataset can hold (nBlocks not a power of two): cells from gen_fake_cell, the big tree and the proofs from the Python
    oracle.  The only place where the odd keys 2 / 3 are reached above a singleton."""
    C, P = oracle
    cs, bs = 128, 4096
    cpb = bs // cs
    nc = n_blocks * cpb
    cells = np.frombuffer(b"".join(P.gen_fake_cell(P.slot_seed(77, n_blocks), i, cs) for i in range(nc)), dtype=np.uint8)
    slot = OracleSlot(C, P, oracle_block_roots(C, cells, cs, bs), python_tree=True)
    assert [len(l) for l in slot.layers] == {3: [3, 2, 1], 5: [5, 3, 2, 1], 6: [6, 3, 2, 1], 7: [7, 4, 2, 1]}[n_blocks]
    assert pkg.block_proof_depth(cs, bs, nc) == slot.depth
    rb = [(0, b) for b in range(n_blocks)]
    paths = np.stack([slot.path(b) for b in range(n_blocks)])
    st, got = sctx.blocks_verify(cs, bs, nc, slot.root.reshape(1, 32), rb, cells, paths)
    assert st.tolist() == [pkg.BLOCK_MATCH] * n_blocks
    assert got.tobytes() == slot.block_roots.tobytes()
    # the last block: a non-zero value wherever its path holds zero
    last = paths[n_blocks - 1]
    zero_levels = [l for l in range(slot.depth) if not last[l].any()]
    assert zero_levels == {3: [0], 5: [0, 1], 6: [1], 7: [0]}[n_blocks]
    for lvl in zero_levels:
        bad = paths.copy()
        bad[n_blocks - 1, lvl, 0] = 1
        st, _ = sctx.blocks_verify(cs, bs, nc, slot.root.reshape(1, 32), rb, cells, bad)
        assert st.tolist() == [pkg.BLOCK_MATCH] * (n_blocks - 1) + [pkg.BLOCK_MISMATCH], lvl


# ---- 3: round trip without a tree -------------------------------------------------------------------------------------------------------
def test_round_trip_served_by_a_compact_dataset_checked_on_a_fresh_context(pkg, oracle, sctx, files_root):
    C, P = oracle
    cs, bs, nc = GEOMS["b8"]
    _, data, _ = oracle_dataset(C, P, "b8", "fake", files_root)
    ds = build(sctx, config(pkg, GEOMS["b8"]), 2)
    nb = nc // (bs // cs)
    reqs = [(s, b) for s in range(N_SLOTS) for b in range(nb)]
    _, paths = ds.block_proofs(reqs)
    roots = ds.local_roots()
    ds.free()
    cand = np.concatenate(data)
    fresh = pkg.Context(0)                                           # nothing but the roots
    try:
        st, _ = fresh.blocks_verify(cs, bs, nc, roots, reqs, cand, paths)
        assert (st == pkg.BLOCK_MATCH).all()
        shifted = np.roll(paths, 1, axis=0)                          # every block with another block's path
        st, _ = fresh.blocks_verify(cs, bs, nc, roots, reqs, cand, shifted)
        assert (st == pkg.BLOCK_MISMATCH).all()
    finally:
        fresh.close()


# ---- 4: repair of a roots-only dataset --------------------------------------------------------------------------------------------------
CS, CPB, BS = 64, 4, 256
N_CELLS, R_SLOTS = 64, 6
N_BLOCKS = N_CELLS // CPB
REPAIR_GEOM = (CS, BS, N_CELLS)


def write_files(base, n_slots=R_SLOTS, seed=1):
    rng = np.random.default_rng(seed)
    data = {}
    for k in range(n_slots):
        b = rng.integers(1, 256, N_CELLS * CS, dtype=np.uint8).tobytes()
        path = "%s%d.dat" % (base, k)
        with open(path, "wb") as f:
            f.write(b)
        os.utime(path, ns=(OLD_NS, OLD_NS + k))
        data[k] = b
    return data


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


def sha_files(base, n_slots=R_SLOTS):
    return [hashlib.sha256(open("%s%d.dat" % (base, k), "rb").read()).hexdigest() for k in range(n_slots)]


def repair_config(pkg, base):
    return pkg.make_config(maxDepth=10, maxLog2NSlots=4, cellSize=CS, blockSize=BS, nSlots=R_SLOTS, nCells=N_CELLS, nSamples=5, seed=5, file=base)


def repair_oracle(C, P, data):
    return {s: OracleSlot(C, P, oracle_block_roots(C, np.frombuffer(data[s], dtype=np.uint8), CS, BS)) for s in data}


def block(data, s, b):
    return np.frombuffer(data[s][b * BS:(b + 1) * BS], dtype=np.uint8)


def test_roots_only_dataset_repaired_with_proved_blocks(pkg, oracle, sctx, tmp_path):
    C, P = oracle
    base = str(tmp_path / "slot")
    data = write_files(base)
    slots = repair_oracle(C, P, data)
    original = sha_files(base)
    ds = build(sctx, repair_config(pkg, base), 0)
    assert np.array_equal(ds.local_roots(), np.stack([slots[s].root for s in range(R_SLOTS)]))
    before = {s: ds.proof_input(s, ENTROPY).json() for s in range(R_SLOTS)}
    damaged = [(0, 3), (2, 15), (2, 0), (5, 7)]
    for s, b in damaged:
        flip(base, s, b * BS + 17)
    g, bad, n_bad = ds.scrub()
    assert g == pkg.SCRUB_SLOT and n_bad == 3 and [(int(s), int(i)) for s, i in bad] == [(0, 0), (2, 0), (5, 0)]
    good = np.concatenate([block(data, s, b) for s, b in damaged])
    with pytest.raises(pkg.CodexP2Error) as ei:                                             # unchanged: no block roots to compare with
        ds.repair_blocks(damaged, good)
    assert ei.value.status == CP2_ERR_INVALID and "slot roots" in str(ei.value)
    assert sha_files(base) != original
    # the original bytes with the oracle's paths, and among them wrong candidates for blocks that are intact
    reqs = damaged + [(1, 4), (3, 9), (4, 1), (0, 8)]
    cand = np.concatenate([good, block(data, 1, 5), flip_byte(block(data, 3, 9), BS - 1, 0x01), block(data, 4, 1), block(data, 0, 8)])
    paths = np.stack([slots[s].path(b) for s, b in reqs])
    paths[6] = slots[4].path(2)                                                             # the right block (4, 1) with a wrong path
    M, X = pkg.REPAIR_MATCH, pkg.REPAIR_MISMATCH
    st, w = ds.repair_blocks_proved(reqs, cand, paths, check_only=True)
    assert st.tolist() == [M, M, M, M, X, X, X, M] and w == 0 and sha_files(base) != original
    st, w = ds.repair_blocks_proved(reqs, cand, paths)
    assert st.tolist() == [M, M, M, M, X, X, X, M] and w == 5
    assert sha_files(base) == original
    for s in (1, 3, 4):
        assert os.stat("%s%d.dat" % (base, s)).st_mtime_ns == OLD_NS + s                    # files of wrong candidates: not opened for writing
    assert ds.scrub()[2] == 0
    assert {s: ds.proof_input(s, ENTROPY).json() for s in range(R_SLOTS)} == before
    ds.free()


def test_roots_only_cached_dataset_repair_keeps_the_cache_valid(pkg, oracle, sctx, tmp_path):
    C, P = oracle
    base = str(tmp_path / "slot")
    data = write_files(base)
    slots = repair_oracle(C, P, data)
    cfg = repair_config(pkg, base)
    cache = str(tmp_path / "roots.cache")
    ds = build(sctx, cfg, 0, cache=cache)
    roots = ds.local_roots()
    ds.free()
    flip(base, 3, 10 * BS + 9, keep_mtime=True)                                             # bit rot: size and mtime as before
    ds = build(sctx, cfg, 0, cache=cache)
    assert np.array_equal(ds.local_roots(), roots)                                          # loaded from the cache: the damage is not seen
    assert [int(s) for s, _ in ds.scrub()[1]] == [3]
    st, w = ds.repair_blocks_proved([(3, 10)], block(data, 3, 10), slots[3].path(10).reshape(1, -1, 32), cache_path=cache)
    assert st.tolist() == [pkg.REPAIR_MATCH] and w == 1
    assert ds.scrub()[2] == 0
    ds.free()
    st0 = os.stat(cache)
    ds = build(sctx, cfg, 0, cache=cache)                                                   # loaded: a rebuild would rename a new file into place
    st1 = os.stat(cache)
    assert (st1.st_ino, st1.st_mtime_ns) == (st0.st_ino, st0.st_mtime_ns)
    assert np.array_equal(ds.local_roots(), roots) and ds.scrub()[2] == 0
    ds.free()
    # control: the same repair without cache_path leaves the cache stale, and the next build rebuilds
    flip(base, 3, 10 * BS + 9, keep_mtime=True)
    ds = build(sctx, cfg, 0, cache=cache)
    st0 = os.stat(cache)
    assert ds.repair_blocks_proved([(3, 10)], block(data, 3, 10), slots[3].path(10).reshape(1, -1, 32))[0].tolist() == [pkg.REPAIR_MATCH]
    ds.free()
    ds = build(sctx, cfg, 0, cache=cache)
    assert os.stat(cache).st_ino != st0.st_ino
    ds.free()


@pytest.mark.parametrize("mode", [1, 2])
def test_proved_repair_gives_repairs_verdicts_where_block_roots_are_kept(pkg, oracle, sctx, tmp_path, mode):
    C, P = oracle
    base = str(tmp_path / "slot")
    data = write_files(base)
    slots = repair_oracle(C, P, data)
    ds = build(sctx, repair_config(pkg, base), mode)
    reqs = [(0, 1), (1, 4), (2, 0), (3, 5), (4, 7), (5, 15)]
    cand = np.concatenate([block(data, 0, 2), flip_byte(block(data, 1, 4), BS - CS + 5, 0x01), np.zeros(BS, dtype=np.uint8), block(data, 3, 6),
                           block(data, 4, 7), block(data, 5, 15)])
    paths = np.stack([slots[s].path(b) for s, b in reqs])
    M, X = pkg.REPAIR_MATCH, pkg.REPAIR_MISMATCH
    want, _ = ds.repair_blocks(reqs, cand, check_only=True)
    got, w = ds.repair_blocks_proved(reqs, cand, paths, check_only=True)
    assert want.tolist() == got.tolist() == [X, X, X, X, M, M] and w == 0
    was = sha_files(base)
    got, w = ds.repair_blocks_proved(reqs, cand, paths)
    assert got.tolist() == [X, X, X, X, M, M] and w == 2 and sha_files(base) == was
    ds.free()


# ---- 5: chunks and memory kinds ---------------------------------------------------------------------------------------------------------
CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as g
job = json.loads(sys.argv[1])
pkg = g.load_package()
ctx = pkg.Context(0)
cand, paths, roots, rb = (np.load(job[k]) for k in ("cand", "paths", "roots", "rb"))
geom = job["geom"]
out = {"pageable": ctx.blocks_verify(*geom, roots, rb, cand, paths)[0].tolist()}
import torch
pinned = torch.from_numpy(cand).pin_memory()
st, got = ctx.blocks_verify(*geom, roots, rb, pinned.numpy(), paths)
out["pinned"] = st.tolist()
out["roots_sha"] = __import__("hashlib").sha256(got.tobytes()).hexdigest()
ctx.close()
print(json.dumps(out), flush=True)
""" % ROOT


@pytest.mark.parametrize("stage_mb,n_cells,n_slots", [(1, 4096, 8), (80, 16384, 64)])
def test_many_chunks_pageable_and_pinned_planted_verdicts(pkg, oracle, tmp_path, stage_mb, n_cells, n_slots):
    """64 KiB blocks of 64-byte cells.  1 MiB of staging: chunks of 8 requests; 80 MiB: a chunk through the pinned ring (more than 32 MiB)
    and a smaller one; caller-pinned candidates read in place.  Bad requests are planted by index (i % 3 == 1: the last byte of the block,
    i % 7 == 2: one byte of one path level), so they fall on both sides of every chunk edge; the verdicts equal the planted pattern."""
    C, P = oracle
    cs, bs = 64, 65536
    nb = n_cells * cs // bs
    rng = np.random.default_rng(n_cells)
    slots, data = [], []
    for k in range(n_slots):
        cells = rng.integers(1, 256, n_cells * cs, dtype=np.uint8)
        data.append(cells.reshape(nb, bs))
        slots.append(OracleSlot(C, P, oracle_block_roots(C, cells, cs, bs)))
    reqs = [(s, b) for s in range(n_slots) for b in range(nb)]
    reqs = [reqs[i] for i in np.random.default_rng(1).permutation(len(reqs))]
    cand = np.stack([data[s][b] for s, b in reqs])
    paths = np.stack([slots[s].path(b) for s, b in reqs])
    depth = paths.shape[1]
    want = []
    for i in range(len(reqs)):
        if i % 3 == 1:
            cand[i, bs - 1] ^= 1
        elif i % 7 == 2:
            paths[i, i % depth, (i * 11) % 31] ^= 0x10
        want.append(pkg.BLOCK_MISMATCH if (i % 3 == 1 or i % 7 == 2) else pkg.BLOCK_MATCH)
    want_roots = np.stack([slots[s].block_roots[b] for s, b in reqs])
    names = {}
    for k, a in (("cand", cand.reshape(-1)), ("paths", paths), ("roots", np.stack([s.root for s in slots])), ("rb", np.array(reqs, dtype=np.uint64))):
        names[k] = str(tmp_path / (k + ".npy"))
        np.save(names[k], a)
    job = dict(names, geom=[cs, bs, n_cells])
    clean = {k: v for k, v in os.environ.items() if not k.startswith("CODEX_P2_")}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(job)], capture_output=True, text=True, timeout=200,
                       env=dict(clean, CODEX_P2_STAGE_MB=str(stage_mb)))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert got["pageable"] == want and got["pinned"] == want
    # what each candidate hashed to: the oracle's block root wherever the data was left alone
    untouched = np.array([i % 3 != 1 for i in range(len(reqs))])
    sctx = pkg.Context(0)
    try:
        st, roots_out = sctx.blocks_verify(cs, bs, n_cells, np.stack([s.root for s in slots]), reqs, cand.reshape(-1), paths)
    finally:
        sctx.close()
    assert st.tolist() == want
    assert roots_out[untouched].tobytes() == want_roots[untouched].tobytes()
    assert not (roots_out[~untouched] == want_roots[~untouched]).all(axis=1).any()
    assert got["roots_sha"] == hashlib.sha256(roots_out.tobytes()).hexdigest()


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_request_and_touch_nothing(pkg, oracle, sctx, tmp_path):
    C, P = oracle
    L = sctx.L
    base = str(tmp_path / "slot")
    data = write_files(base)
    slots = repair_oracle(C, P, data)
    cfg = repair_config(pkg, base)
    depth = 4
    last_error = lambda: L.cp2_last_error(sctx.h).decode()          # noqa: E731
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)        # noqa: E731
    ptr = lambda a: None if a is None else a.ctypes.data            # noqa: E731
    two_d = np.concatenate([block(data, 0, 3), block(data, 1, 1)])
    two_p = np.stack([slots[0].path(3), slots[1].path(1)])
    was = sha_files(base)
    full, compact, roots_only = (build(sctx, cfg, m) for m in (1, 2, 0))

    # -- cp2_dataset_block_proofs
    def raw_proofs(ds, sb, n, want_paths=True):
        roots = np.full((max(n, 1), 32), 9, dtype=np.uint8)
        paths = np.full((max(n, 1), depth, 32), 9, dtype=np.uint8)
        st = L.cp2_dataset_block_proofs(ds.h, ptr(sb), n, roots.ctypes.data, paths.ctypes.data if want_paths else None)
        return st, bool((roots == 9).all() and (paths == 9).all())

    for ds, sb, n, wp, words in ((roots_only, u64([[0, 3]]), 1, True, "slot roots"),
                                 (compact, u64([[0, 3], [R_SLOTS, 0]]), 2, True, "request 1"),
                                 (full, u64([[0, 3], [1, 1], [2, N_BLOCKS]]), 3, True, "request 2"),
                                 (compact, None, 1, True, "NULL"),
                                 (full, u64([[0, 3]]), 1, False, "NULL")):
        st, untouched = raw_proofs(ds, sb, n, wp)
        assert st == CP2_ERR_INVALID and untouched, words
        assert words in last_error(), (words, last_error())
    assert raw_proofs(compact, None, 0) == (0, True)
    roots, paths = full.block_proofs([(0, 3), (0, 3)])                                       # a repeat is served
    assert roots[0].tobytes() == roots[1].tobytes() == slots[0].block_roots[3].tobytes() and paths[0].tobytes() == paths[1].tobytes()
    st = L.cp2_dataset_block_proofs(compact.h, u64([[1, 1]]).ctypes.data, 1, None, paths.ctypes.data)   # block_roots may be NULL
    assert st == 0 and paths[0].tobytes() == slots[1].path(1).tobytes()

    # -- cp2_blocks_verify
    sroots = np.stack([slots[0].root, slots[1].root])

    def raw_verify(geom, r, n_roots, rb, d, p, n):
        status = np.full(max(n, 1), 7, dtype=np.uint32)
        out = np.full((max(n, 1), 32), 9, dtype=np.uint8)
        st = L.cp2_blocks_verify(sctx.h, *geom, ptr(r), n_roots, ptr(rb), ptr(d), ptr(p), n, status.ctypes.data, out.ctypes.data)
        return st, bool((status == 7).all() and (out == 9).all())

    ok_rb = u64([[0, 3], [1, 1]])
    for geom, r, n_roots, rb, d, p, n, words in (((0, BS, N_CELLS), sroots, 2, ok_rb, two_d, two_p, 2, "geometry"),
                                                 ((CS, BS + 1, N_CELLS), sroots, 2, ok_rb, two_d, two_p, 2, "geometry"),
                                                 ((CS, BS, N_CELLS + 1), sroots, 2, ok_rb, two_d, two_p, 2, "geometry"),
                                                 (REPAIR_GEOM, sroots, 2, u64([[0, 3], [2, 1]]), two_d, two_p, 2, "request 1"),
                                                 (REPAIR_GEOM, sroots, 2, u64([[0, N_BLOCKS], [2, 1]]), two_d, two_p, 2, "request 0"),
                                                 (REPAIR_GEOM, None, 2, ok_rb, two_d, two_p, 2, "NULL"),
                                                 (REPAIR_GEOM, sroots, 2, None, two_d, two_p, 2, "NULL"),
                                                 (REPAIR_GEOM, sroots, 2, ok_rb, None, two_p, 2, "NULL"),
                                                 (REPAIR_GEOM, sroots, 2, ok_rb, two_d, None, 2, "NULL")):
        st, untouched = raw_verify(geom, r, n_roots, rb, d, p, n)
        assert st == CP2_ERR_INVALID and untouched, words
        assert words in last_error(), (words, last_error())
    assert L.cp2_blocks_verify(sctx.h, *REPAIR_GEOM, sroots.ctypes.data, 2, ok_rb.ctypes.data, two_d.ctypes.data, two_p.ctypes.data, 2, None, None) == CP2_ERR_INVALID
    assert raw_verify(REPAIR_GEOM, None, 0, None, None, None, 0) == (0, True)
    st, _ = sctx.blocks_verify(*REPAIR_GEOM, sroots, ok_rb, two_d, two_p, want_roots=False)  # block_roots may be NULL
    assert st.tolist() == [pkg.BLOCK_MATCH] * 2

    # -- cp2_dataset_repair_blocks_proved
    def raw_repair(ds, sb, d, p, n, flags=0):
        status = np.full(max(n, 1), 7, dtype=np.uint32)
        w = ctypes.c_size_t(99)
        st = L.cp2_dataset_repair_blocks_proved(ds.h, ptr(sb), ptr(d), ptr(p), n, flags, None, status.ctypes.data, ctypes.byref(w))
        return st, bool((status == 7).all()) and w.value == 99

    fake = build(sctx, pkg.make_config(maxDepth=10, maxLog2NSlots=4, cellSize=CS, blockSize=BS, nSlots=R_SLOTS, nCells=N_CELLS, nSamples=5, seed=5), 0)
    three_d, three_p = np.concatenate([two_d, two_d[:BS]]), np.concatenate([two_p, two_p[:1]])
    for ds, sb, d, p, n, flags, words in ((roots_only, u64([[0, 3], [1, 1], [0, 3]]), three_d, three_p, 3, 0, "request 2"),
                                          (roots_only, u64([[0, 3], [R_SLOTS, 0]]), two_d, two_p, 2, 0, "request 1"),
                                          (compact, u64([[0, N_BLOCKS]]), two_d, two_p, 1, 0, "request 0"),
                                          (roots_only, None, two_d, two_p, 1, 0, "NULL"),
                                          (roots_only, ok_rb, None, two_p, 2, 0, "NULL"),
                                          (roots_only, ok_rb, two_d, None, 2, 0, "paths"),
                                          (full, ok_rb, two_d, two_p, 2, 4, "flag"),
                                          (fake, ok_rb, two_d, two_p, 2, 0, "fake source")):
        st, untouched = raw_repair(ds, sb, d, p, n, flags)
        assert st == CP2_ERR_INVALID and untouched, words
        assert words in last_error(), (words, last_error())
    assert L.cp2_dataset_repair_blocks_proved(roots_only.h, ok_rb.ctypes.data, two_d.ctypes.data, two_p.ctypes.data, 2, 0, None, None, None) == CP2_ERR_INVALID
    w = ctypes.c_size_t(99)
    assert L.cp2_dataset_repair_blocks_proved(roots_only.h, None, None, None, 0, 0, None, None, ctypes.byref(w)) == 0 and w.value == 0
    # the fake source takes check-only calls: its own cells match, another block's do not
    seed = sctx.slot_seed(cfg.seed, 2)
    cells = C.gen_fake_cells(C.slot_seed(5, 2), 0, N_CELLS, CS)
    assert C.slot_seed(5, 2) == seed
    fslot = OracleSlot(C, P, oracle_block_roots(C, cells.reshape(-1), CS, BS))
    fb = cells.reshape(N_BLOCKS, BS)
    st, w = fake.repair_blocks_proved([(2, 5), (2, 9)], np.concatenate([fb[5], fb[6]]), np.stack([fslot.path(5), fslot.path(9)]), check_only=True)
    assert st.tolist() == [pkg.REPAIR_MATCH, pkg.REPAIR_MISMATCH] and w == 0
    assert sha_files(base) == was
    for d in (fake, roots_only, compact, full):
        d.free()
