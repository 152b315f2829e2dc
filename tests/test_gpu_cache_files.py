"""GPU suite: the library's cache files (csrc/cache_file.hpp, cache_file.cpp) -- the tree cache and the kept form through one head
and one pinned payload ring.  Byte identity with files written before that module existed, the ring's edges (2, 3, 4 and 5 chunks
around a ring of depth 3), and a kept payload of more than one chunk."""
import hashlib
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "cache_files")
FILES = {"tree_3slots.cp2": 1, "kept_mode2.cp2": 2, "kept_mode0.cp2": 0}     # file -> the kept mode that writes and loads it
CHUNK = 64 << 20                                                              # the ring's chunk (cache_file.cpp)


def _maker():
    spec = importlib.util.spec_from_file_location("make_cache_files_golden", os.path.join(ROOT, "tests", "golden", "make_cache_files_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _flip(path, at):
    """one bit of the byte at `at`; returns the byte as it was"""
    with open(path, "r+b") as f:
        f.seek(at)
        b = f.read(1)
        f.seek(at)
        f.write(bytes([b[0] ^ 1]))
    return b


def _stamp(path):
    st = os.stat(path)
    return st.st_ino, st.st_mtime_ns, st.st_size


def test_saves_are_byte_identical_to_the_golden_files(pkg, ctx, tmp_path):
    """The three saves of tests/golden/make_cache_files_golden.py give the files the parent of the cache-file module wrote."""
    roots = _maker().write(ctx, pkg, str(tmp_path))
    want = json.load(open(os.path.join(GOLDEN_DIR, "config.json")))
    assert roots == want["slot_roots"]
    for name in FILES:
        assert _read(str(tmp_path / name)) == _read(os.path.join(GOLDEN_DIR, name)), name
    assert sorted(os.listdir(tmp_path)) == sorted(FILES), "a tmp file stayed behind"


@pytest.mark.parametrize("name", sorted(FILES))
def test_golden_files_load(pkg, ctx, tmp_path, name):
    """Each golden file loads (nothing is rebuilt: the file keeps its inode), and gives the golden roots and the proof input of an
    uncached dataset."""
    want = json.load(open(os.path.join(GOLDEN_DIR, "config.json")))
    c = want["config"]
    cfg = pkg.make_config(**c)
    roots = np.frombuffer(bytes.fromhex(want["slot_roots"][name]), dtype=np.uint8).reshape(-1, 32)
    plain = ctx.dataset(cfg)
    texts = [plain.proof_input(s, 4242).json() for s in range(c["nSlots"])]
    plain.free()
    path = str(tmp_path / name)                     # a copy: a build that did not load would write here
    shutil.copyfile(os.path.join(GOLDEN_DIR, name), path)
    before = _stamp(path)
    if FILES[name] == 1:
        t = ctx.slot_trees_load(path)
        assert np.array_equal(t.roots(), roots)
        t.free()
    ctx.set_keep_trees(FILES[name])
    try:
        ds = ctx.dataset(cfg, cache=path)
        assert ds.tree_mode == FILES[name] and _stamp(path) == before and os.listdir(tmp_path) == [name]
        assert np.array_equal(ds.local_roots(), roots)
        assert [ds.proof_input(s, 4242).json() for s in range(c["nSlots"])] == texts
        ds.free()
    finally:
        ctx.set_keep_trees(-1)


@pytest.mark.parametrize("n_slots,n_chunks", [(512, 2), (768, 3), (1024, 4), (1100, 5)])
def test_tree_cache_ring_edges(pkg, ctx, tmp_path, n_slots, n_chunks):
    """Node buffers of exactly 2, 3, 4 and 5 chunks of 64 MiB through the ring of depth 3 (fewer chunks than buffers, as many, one more,
    the last one short; the 2-chunk buffer is just short of two full chunks, where the file I/O runs on the calling thread, the others
    go through the worker): save, load, the same roots and paths; one flipped byte in the LAST chunk is refused by the checksum, a file
    32 bytes short as truncated."""
    trees = ctx.slot_trees_fake(12345, 0, n_slots, 2048, 65536, 1 << 12)
    roots = trees.roots()
    cells = np.array([0, 1, 4095, 2048, 77], dtype=np.uint64)
    want_paths, want_leaves = trees.paths(n_slots - 1, cells, 32)
    path = str(tmp_path / "t.cp2")
    trees.save(path)
    trees.free()
    size = os.path.getsize(path)
    payload = size - 104                              # fake source: no base name, no stamps
    assert (payload + CHUNK - 1) // CHUNK == n_chunks and (payload < 2 * CHUNK) == (n_chunks == 2), (payload, payload / CHUNK)
    back = ctx.slot_trees_load(path)
    assert np.array_equal(back.roots(), roots)
    got_paths, got_leaves = back.paths(n_slots - 1, cells, 32)
    assert np.array_equal(got_paths, want_paths) and np.array_equal(got_leaves, want_leaves)
    back.free()
    at = 104 + (n_chunks - 1) * CHUNK + (payload - (n_chunks - 1) * CHUNK) // 2
    _flip(path, at)
    with pytest.raises(pkg.CodexP2Error) as e:
        ctx.slot_trees_load(path)
    assert "checksum" in str(e.value)
    _flip(path, at)
    os.truncate(path, size - 32)
    with pytest.raises(pkg.CodexP2Error) as e:
        ctx.slot_trees_load(path)
    assert "truncated" in str(e.value)
    assert os.listdir(tmp_path) == ["t.cp2"]


def test_kept_payload_of_two_chunks_goes_through_the_ring(pkg, ctx, tmp_path):
    """A compact dataset whose kept layers exceed one 64 MiB chunk (513 slots of 2^12 cells of 32 bytes, two cells per block: 4095 kept
    rows per slot): the cached build writes them, the second run loads them (the file keeps its inode), a flipped payload byte in the
    second chunk means a rebuild that writes the same bytes again -- and the proof input is the uncached dataset's every time."""
    c = dict(maxDepth=16, maxLog2NSlots=10, cellSize=32, blockSize=64, nSlots=513, nCells=1 << 12, nSamples=5, seed=11)
    cfg = pkg.make_config(**c)
    path = str(tmp_path / "kept.cp2")
    ctx.set_keep_trees(2)
    try:
        plain = ctx.dataset(cfg)
        want = [plain.proof_input(s, 777).json() for s in (0, 256, 512)]
        plain.free()
        a = ctx.dataset(cfg, cache=path)
        assert a.tree_mode == 2
        size = os.path.getsize(path)
        assert size == 104 + 513 * 4095 * 32 and CHUNK < size - 104 <= 2 * CHUNK
        assert [a.proof_input(s, 777).json() for s in (0, 256, 512)] == want
        a.free()
        written = hashlib.sha256(_read(path)).hexdigest()
        before = _stamp(path)
        b = ctx.dataset(cfg, cache=path)                   # loaded
        assert _stamp(path) == before and b.tree_mode == 2
        assert [b.proof_input(s, 777).json() for s in (0, 256, 512)] == want
        b.free()
        _flip(path, 104 + CHUNK + 4321)                    # the second chunk
        d = ctx.dataset(cfg, cache=path)                   # refused -> rebuilt and written again
        assert _stamp(path)[0] != before[0] and hashlib.sha256(_read(path)).hexdigest() == written
        assert [d.proof_input(s, 777).json() for s in (0, 256, 512)] == want
        d.free()
        assert os.listdir(tmp_path) == ["kept.cp2"]
    finally:
        ctx.set_keep_trees(-1)
