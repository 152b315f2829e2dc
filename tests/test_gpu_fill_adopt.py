"""GPU suite: adopting blocks from disk -- cp2_fill_adopt.  A session that keeps nodes must take over the blocks its slot files already hold
wherever the tree above them reaches a node it knows, the stated slot root included, and nothing else; it must end as exactly the dataset
cp2_dataset_build makes from the same data.  The small geometry of tests/test_gpu_fill_serve.py (cells of 64 bytes, blocks of 256, 4 slots),
1, 8 and 64 blocks a slot, slot files in tmp_path.  Which blocks an adopt takes is computed by tests/fill_adopt_models.py.  Every
comparison is bit-exact."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest

import fill_adopt_models as D
from test_gpu_fill import Source, add, build_compact
from test_gpu_fill_anchored import N_SLOTS, World, last_error

pytestmark = pytest.mark.gpu

CP2_OK, CP2_ERR_INVALID = 0, -1


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


def name_of(w, s):
    return "%s%d.dat" % (w.out_base, s)


def place(w, s, blocks=None, nbytes=None):
    """slot s's file as the session will find it: the true bytes, other blocks, or a prefix"""
    raw = (w.data[s] if blocks is None else blocks).tobytes()
    with open(name_of(w, s), "wb") as fh:
        fh.write(raw if nbytes is None else raw[:nbytes])


def missing_of(f):
    return [tuple(p) for p in f.missing()[0].tolist()]


# ---- 1: intact files under nothing but the stated roots ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 8, 64])
def test_intact_files_are_adopted_whole_and_finish_as_the_built_dataset(pkg, sctx, tmp_path, nb):
    w = World(pkg, sctx, nb, str(tmp_path))
    for s in range(N_SLOTS):
        place(w, s)
    f = w.session(sctx)
    assert f.missing(0)[1] == N_SLOTS * nb
    assert f.adopt(no_read=True) == (0, 0)                                               # nothing is remembered yet
    assert f.adopt() == (N_SLOTS * nb, N_SLOTS * nb)
    assert f.missing(0)[1] == 0 and (f.anchors(w.pairs) == 0).all()
    assert f.adopt() == (0, 0)                                                           # present blocks are never read
    w.check_finished(pkg, f)
    for s in range(N_SLOTS):
        assert open(name_of(w, s), "rb").read() == w.data[s].tobytes()
    f.free()
    w.free()


# ---- 2: one flipped byte in one block of a 64-block slot ----------------------------------------------------------------------------------------
def test_one_damaged_block_costs_its_own_siblings_and_one_path(pkg, sctx, tmp_path):
    nb, slot, bad, q = 64, 1, 37, 5
    w = World(pkg, sctx, nb, str(tmp_path))
    for s in range(N_SLOTS):
        place(w, s)
    blocks = w.data[slot].copy()
    blocks[bad, 100] ^= 0x20
    place(w, slot, blocks)
    f = w.session(sctx)
    model = D.Slot(nb)
    assert model.adopt(range(nb), damaged=[bad]) == []
    assert f.adopt() == (N_SLOTS * nb, (N_SLOTS - 1) * nb)                               # nothing vouches for less than the whole of that slot
    assert missing_of(f) == [(slot, b) for b in range(nb)]
    # one other block with its whole path: its siblings vouch for every subtree but the one that holds the damage
    siblings = model.add_path(q)
    assert add(f, w.src, [(slot, q)])[0].tolist() == [pkg.FILL_NEW]
    want = model.adopt(range(nb), damaged=[bad])
    assert want == [b for b in range(nb) if b != q and not 32 <= b < 64] and len(want) == 31
    assert f.adopt(no_read=True) == (0, len(want))
    assert missing_of(f) == [(slot, b) for b in range(nb) if b not in model.present]
    # the damaged block with the levels cp2_fill_anchors names, then what lay beside it under that node
    levels = f.anchors([(slot, bad)])
    assert levels.tolist() == [model.anchor(bad)] == [5]
    status, n_new, _ = w.add_anchored(f, [(slot, bad)], levels=levels)
    assert status.tolist() == [pkg.FILL_NEW] and n_new == 1
    siblings += model.add_path(bad, int(levels[0]))
    rest = [b for b in range(nb) if b not in model.present]
    assert model.adopt(rest) == rest and len(rest) == 31
    assert f.adopt(no_read=True) == (0, len(rest))
    assert f.missing(0)[1] == 0
    assert siblings == w.depth + 5 == 11                                                  # against 64 x 6 for the slot fetched again
    w.check_finished(pkg, f)
    assert open(name_of(w, slot), "rb").read() == w.data[slot].tobytes()                 # the add wrote the damaged block over
    f.free()
    w.free()


# ---- 3: crash recovery ------------------------------------------------------------------------------------------------------------------------
def test_blocks_added_after_the_last_save_are_recovered_from_the_files(pkg, sctx, tmp_path):
    nb = 8
    w = World(pkg, sctx, nb, str(tmp_path))
    f = w.session(sctx, keep=False)
    saved = [(s, b) for s in (0, 1) for b in range(4)]
    assert (add(f, w.src, saved)[0] == pkg.FILL_NEW).all()
    ckpt = str(tmp_path / "session.ckpt")
    f.save(ckpt)
    later = [(0, b) for b in range(4, 8)] + [(1, 4), (1, 5)]                              # slot 0's file is complete, slot 1's ends after block 5
    assert (add(f, w.src, later)[0] == pkg.FILL_NEW).all()
    f.free()                                                                              # the crash: nothing saved since
    f = sctx.fill_resume(w.cfg, w.roots, ckpt, 0, N_SLOTS)
    assert f.n_dropped == 0 and f.missing(0)[1] == N_SLOTS * nb - len(saved)
    f.keep_nodes()
    assert f.adopt() == (6, 4)                                                            # slot 1: blocks 6 and 7 are not there, nothing vouches for 4 and 5
    assert missing_of(f) == [(1, b) for b in range(4, 8)] + [(s, b) for s in (2, 3) for b in range(nb)]
    assert add(f, w.src, [(1, 6)])[0].tolist() == [pkg.FILL_NEW]                          # its path brings the node above blocks 4 and 5
    assert f.adopt(1, 1, no_read=True) == (0, 2)
    assert missing_of(f) == [(1, 7)] + [(s, b) for s in (2, 3) for b in range(nb)]
    status, roots, paths = f.block_proofs([(1, 4), (1, 5)])
    assert status.tolist() == [pkg.FILL_PROOF_OK] * 2
    for i, p in enumerate([(1, 4), (1, 5)]):
        assert roots[i].tobytes() == w.src.roots[w.src.index[p]].tobytes() and paths[i].tobytes() == w.src.paths[w.src.index[p]].tobytes()
    f.free()
    w.free()


# ---- 4: absence is a state ------------------------------------------------------------------------------------------------------------------------
def test_a_short_file_and_a_missing_file_yield_no_candidates_and_no_error(pkg, sctx, tmp_path):
    nb = 8
    w = World(pkg, sctx, nb, str(tmp_path))
    place(w, 0, nbytes=3 * 256 + 128)                                                     # three whole blocks and half of the fourth
    for s in (2, 3):
        place(w, s)
    f = w.session(sctx)
    assert f.adopt() == (3 + 2 * nb, 2 * nb)                                              # slot 1 has no file; slot 0's three blocks prove nothing
    assert missing_of(f) == [(s, b) for s in (0, 1) for b in range(nb)]
    assert f.adopt(1, 1) == (0, 0) and f.adopt(0, 1) == (3, 0)
    assert not os.path.exists(name_of(w, 1)) and os.path.getsize(name_of(w, 0)) == 3 * 256 + 128
    f.free()
    w.free()


# ---- 5: served from the moment it is adopted --------------------------------------------------------------------------------------------------------
def test_an_adopted_block_is_served_at_once(pkg, sctx, tmp_path):
    nb = 8
    w = World(pkg, sctx, nb, str(tmp_path))
    place(w, 2)
    f = w.session(sctx)
    pairs = [(2, b) for b in range(nb)]
    assert f.block_proofs(pairs, statuses_only=True).tolist() == [pkg.FILL_PROOF_ABSENT] * nb
    assert f.adopt(2, 1) == (nb, nb)
    status, roots, paths = f.block_proofs(pairs)
    assert status.tolist() == [pkg.FILL_PROOF_OK] * nb
    for i, p in enumerate(pairs):
        assert roots[i].tobytes() == w.src.roots[w.src.index[p]].tobytes() and paths[i].tobytes() == w.src.paths[w.src.index[p]].tobytes(), p
    f.free()
    w.free()


# ---- 6: a checkpoint after an adopt ---------------------------------------------------------------------------------------------------------------
def test_a_checkpoint_saved_after_an_adopt_resumes_and_drops_nothing(pkg, sctx, tmp_path):
    nb = 8
    w = World(pkg, sctx, nb, str(tmp_path))
    for s in (0, 1):
        place(w, s)
    f = w.session(sctx)
    assert f.adopt() == (2 * nb, 2 * nb)
    ckpt = str(tmp_path / "after.ckpt")
    f.save(ckpt)
    f.free()
    f = sctx.fill_resume(w.cfg, w.roots, ckpt, 0, N_SLOTS)                                # with the re-check: every adopted block is read and compared
    assert f.n_dropped == 0 and missing_of(f) == [(s, b) for s in (2, 3) for b in range(nb)]
    f.keep_nodes()
    assert (f.anchors([(s, b) for s in (0, 1) for b in range(nb)]) == 0).all()
    for s in (2, 3):
        place(w, s)
    assert f.adopt() == (2 * nb, 2 * nb)
    w.check_finished(pkg, f)
    f.free()
    w.free()


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(pkg, sctx, tmp_path):
    nb = 8
    w = World(pkg, sctx, nb, str(tmp_path))
    for s in range(N_SLOTS):
        place(w, s)
    L = pkg.load_library()
    read, adopted = ctypes.c_uint64(5), ctypes.c_uint64(6)

    def call(f, first=0, n=0, flags=0):
        return L.cp2_fill_adopt(f.h if f is not None else None, first, n, flags, ctypes.byref(read), ctypes.byref(adopted))

    def untouched():
        return read.value == 5 and adopted.value == 6

    assert call(None) == CP2_ERR_INVALID and untouched()
    plain = w.session(sctx, keep=False)                                                  # a session that does not keep nodes: the anchored add's words
    assert call(plain) == CP2_ERR_INVALID and "cp2_fill_keep_nodes" in last_error(sctx) and untouched()
    assert last_error(sctx) == "fill: this session does not keep the nodes of the paths it proves: call cp2_fill_keep_nodes first"
    plain.free()
    fake = sctx.fill(pkg.make_config(maxDepth=8, maxLog2NSlots=2, cellSize=64, blockSize=256, nSlots=4, nCells=4 * nb, nSamples=3, seed=40 + nb),
                     w.roots, 0, N_SLOTS)                                                # a session of the fake source has no files
    fake.keep_nodes()
    assert call(fake) == CP2_ERR_INVALID and "fake source" in last_error(sctx) and untouched()
    fake.free()
    f = w.session(sctx)
    assert call(f, flags=2) == CP2_ERR_INVALID and "flag" in last_error(sctx) and untouched()
    assert call(f, flags=-1) == CP2_ERR_INVALID and untouched()
    for first, n in ((N_SLOTS, 1), (0, N_SLOTS + 1), (1, N_SLOTS), (2, 3)):
        assert call(f, first, n) == CP2_ERR_INVALID and "local range" in last_error(sctx) and untouched(), (first, n)
    assert f.missing(0)[1] == N_SLOTS * nb                                               # nothing changed
    assert call(f) == CP2_OK and (read.value, adopted.value) == (N_SLOTS * nb, N_SLOTS * nb)
    read.value, adopted.value = 5, 6
    filled = f.finish()
    assert call(f) == CP2_ERR_INVALID and "finished" in last_error(sctx) and untouched()
    filled.free()
    f.free()
    w.free()


# ---- 8: many chunks -----------------------------------------------------------------------------------------------------------------------------------
def test_many_chunks_damage_on_both_sides_of_a_chunk_edge(pkg, monkeypatch, tmp_path):
    """test_gpu_fill_resume.py's test_many_chunks_fake_and_files for adopt.  1 MiB of staging and 64 KiB blocks: chunks of 8 blocks, 5 slots of
    4 blocks, so the 20 absent blocks are read in two full chunks and a last one of 4.  One flipped byte in entries 7 and 8 of the read plan,
    (slot 1, block 3) and (slot 2, block 0), the two sides of the first chunk edge: nothing below a slot root is known, so exactly those two
    slots yield nothing."""
    monkeypatch.setenv("CODEX_P2_STAGE_MB", "1")
    ctx = pkg.Context(0)
    cfgd = dict(maxDepth=16, maxLog2NSlots=3, cellSize=64, blockSize=65536, nSlots=5, nCells=4096, nSamples=3, seed=77)
    cfg = pkg.make_config(**cfgd)
    built = build_compact(ctx, cfg)
    roots = built.local_roots()
    src = Source(ctx, cfg, built, 0, 5)
    nb = src.nb
    assert nb == 4 and len(src.pairs) == 20
    base = str(tmp_path / "slot")
    fcfg = pkg.make_config(file=base, **cfgd)                                            # the same bytes in slot files: the same roots
    f = ctx.fill(fcfg, roots)
    status, n_new = add(f, src, src.pairs)
    assert (status == pkg.FILL_NEW).all() and n_new == 20
    f.free()                                                                             # unsaved: the files hold the true bytes, nothing else is left
    victims = [src.pairs[7], src.pairs[8]]                                               # the plan's order: ascending (slot, block)
    assert victims == [(1, 3), (2, 0)]
    for s, b in victims:
        with open("%s%d.dat" % (base, s), "r+b") as fh:
            fh.seek(b * cfg.block_size + 65535 - 100 * s)
            byte = fh.read(1)
            fh.seek(-1, os.SEEK_CUR)
            fh.write(bytes([byte[0] ^ 0x80]))

    g = ctx.fill(fcfg, roots)
    g.keep_nodes()
    damaged = {1: [3], 2: [0]}
    want = {s: D.Slot(nb).adopt(range(nb), damaged=damaged.get(s, ())) for s in range(5)}
    assert want[1] == [] and want[2] == [] and all(want[s] == list(range(nb)) for s in (0, 3, 4))
    assert g.adopt() == (20, 12) and sum(len(v) for v in want.values()) == 12
    missing = missing_of(g)
    assert missing == [(s, b) for s in (1, 2) for b in range(nb)] == [(s, b) for s in range(5) for b in range(nb) if b not in want[s]]
    assert g.adopt() == (8, 0)                                                           # read again, and still nothing vouches for them

    status, n_new = add(g, src, missing)                                                 # from the source, with their proofs: NEW, and written over
    assert (status == pkg.FILL_NEW).all() and n_new == 8
    filled = g.finish()
    assert filled.local_roots().tobytes() == roots.tobytes() and filled.scrub()[2] == 0
    for h in (filled, g, built):
        h.free()
    ctx.close()
