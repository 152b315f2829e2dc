"""GPU suite: fill checkpoints -- cp2_fill_save / cp2_fill_resume.  A half-filled session is saved, freed and resumed; the resumed session must
be indistinguishable from one that was begun fresh and received exactly the blocks the source still backs: the same missing list, dropped
blocks accepted again as NEW, and a finished dataset whose roots are the C oracle's and whose proof inputs are cp2_dataset_build's, byte for
byte.  Damage on disk (a flipped byte, a truncated file, a deleted file) and a checkpoint whose layer 0 is wrong on purpose are ordinary
verdicts: nothing here faults.  The checkpoint is read and written by tests/fill_resume_models.py from the documented layout alone, and
k_block_root_recheck is also driven on its own through tests/device_check/libfill_resume_unit.so against a numpy model."""
import ctypes
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import fill_resume_models as M
from test_gpu_fill import Source, add, build_compact, uneven_calls

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libfill_resume_unit.so")
CP2_ERR_INVALID, CP2_ERR_IO = -1, -5
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
# name: (config, first_slot, n_local).  The testMain.hs shape (8 blocks per slot: three tree levels above the blocks) over a range that
# starts past slot 0, and slots of one block.
GEOMS = {
    "main": (dict(maxDepth=16, maxLog2NSlots=3, cellSize=128, blockSize=4096, nSlots=5, nCells=256, nSamples=5, seed=1), 2, 3),
    "one_block": (dict(maxDepth=8, maxLog2NSlots=3, cellSize=128, blockSize=4096, nSlots=4, nCells=32, nSamples=3, seed=7), 1, 3),
}


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def sctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def tuples(a):
    return [tuple(int(x) for x in r) for r in a]


def uneven_half(pairs, seed):
    """a seeded shuffle's first half and a bit: some slots nearly full, others nearly empty"""
    order = [pairs[i] for i in np.random.default_rng(seed).permutation(len(pairs))]
    return order[:len(order) // 2 + 1]


@pytest.fixture(scope="module")
def fake(pkg, sctx):
    """per geometry, once: (cfg, first, n_local, built dataset with the whole dataset's roots set, the roots of every slot, what peers send)"""
    made = {}

    def get(name):
        if name not in made:
            cfgd, first, n_local = GEOMS[name]
            cfg = pkg.make_config(**cfgd)
            whole = build_compact(sctx, cfg)
            all_roots = whole.local_roots().copy()
            whole.free()
            built = build_compact(sctx, cfg, first, n_local)
            built.set_roots(all_roots)
            made[name] = (cfg, first, n_local, built, all_roots, Source(sctx, cfg, built, first, n_local))
        return made[name]

    yield get
    for v in made.values():
        v[3].free()


def finish_and_compare(pkg, oracle, f, cfg, first, n_local, built, all_roots):
    """the finished dataset: roots from the C oracle, a proof input byte for byte cp2_dataset_build's"""
    C, _ = oracle
    filled = f.finish()
    roots = filled.local_roots()
    for k in range(n_local):
        assert roots[k].tobytes() == C.fake_slot_root(C.slot_seed(cfg.seed, first + k), cfg.cell_size, cfg.block_size, cfg.n_cells, 4).tobytes()
    filled.set_roots(all_roots)
    for slot in (first, first + n_local - 1):
        assert filled.proof_input(slot, 1234567).json() == built.proof_input(slot, 1234567).json(), slot
    filled.free()


# ---- 1: the fake source, with the re-check and without --------------------------------------------------------------------------------------
@pytest.mark.parametrize("trust", [False, True])
@pytest.mark.parametrize("name", list(GEOMS))
def test_saved_freed_resumed_then_completed(pkg, oracle, sctx, fake, tmp_path, name, trust):
    cfg, first, n_local, built, all_roots, src = fake(name)
    roots = all_roots[first:first + n_local]
    path = str(tmp_path / "session.ckpt")
    f = sctx.fill(cfg, roots, first, n_local)
    half = uneven_half(src.pairs, seed=3)
    assert add(f, src, half)[1] == len(half)
    before, n_before = f.missing()
    f.save(path)
    first_save = open(path, "rb").read()
    f.save(path)                                                                       # over the older one, through a temporary name
    assert open(path, "rb").read() == first_save and os.listdir(str(tmp_path)) == ["session.ckpt"]
    assert f.missing()[1] == n_before                                                  # nothing of the session changed
    f.free()

    g = sctx.fill_resume(cfg, roots, path, first, n_local, trust_files=trust)
    assert g.n_dropped == 0
    again, n_again = g.missing()
    assert n_again == n_before == len(src.pairs) - len(half) and again.tolist() == before.tolist()
    status, n_new = add(g, src, half[:2])                                              # what was present stays present
    assert (status == pkg.FILL_DUPLICATE).all() and n_new == 0
    rest = tuples(again)
    for pairs in uneven_calls(rest, seed=11):
        status, n_new = add(g, src, pairs)
        assert (status == pkg.FILL_NEW).all() and n_new == len(pairs)
    finish_and_compare(pkg, oracle, g, cfg, first, n_local, built, all_roots)
    with pytest.raises(pkg.CodexP2Error) as e:                                         # a finished session's durable form is the kept cache
        g.save(path)
    assert e.value.status == CP2_ERR_INVALID and "finished" in str(e.value)
    assert open(path, "rb").read() == first_save
    g.free()


# ---- 2: determinism: absent rows are zeros whatever the buffer held ----------------------------------------------------------------------------
def test_absent_rows_are_zeros_and_the_layout_is_the_documented_one(pkg, sctx, fake, tmp_path):
    cfg, first, n_local, built, all_roots, src = fake("main")
    roots = all_roots[first:first + n_local]
    nb = src.nb
    full = sctx.fill(cfg, roots, first, n_local)                                      # a buffer of the same size, every row written, freed
    assert add(full, src, src.pairs)[1] == len(src.pairs)
    full.free()
    f = sctx.fill(cfg, roots, first, n_local)                                         # ... and the session's buffer allocated after it
    some = [(first, 1), (first + 2, nb - 1), (first + 1, 0)]
    add(f, src, some)
    a, b = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    f.save(a)
    f.save(b)
    f.free()
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    c = M.parse_checkpoint(raw)                                                        # magic, sizes, padding, checksum
    assert [c[k] for k in ("cell_size", "block_size", "n_cells", "n_slots", "first_slot", "n_local", "source", "seed", "n_blocks")] == \
        [cfg.cell_size, cfg.block_size, cfg.n_cells, cfg.n_slots, first, n_local, M.SRC_FAKE, cfg.seed, nb]
    assert c["file_base"] == b"" and c["roots"].tobytes() == roots.tobytes()
    present = {(s - first) * nb + blk for s, blk in some}
    assert [g for g, bit in enumerate(c["bits"]) if bit] == sorted(present)
    for g in range(n_local * nb):
        want = src.roots[g] if g in present else np.zeros(32, dtype=np.uint8)          # Source lists its pairs in this order
        assert c["layer0"][g].tobytes() == want.tobytes(), g
    assert M.write_checkpoint(c) == raw                                                # the model's writer is the documented layout


# ---- 3: slot files: a flipped byte, a truncated file, a deleted file ----------------------------------------------------------------------------
FILE_GEOM = dict(maxDepth=16, maxLog2NSlots=3, cellSize=128, blockSize=4096, nSlots=5, nCells=256, nSamples=5, seed=1)
FILE_FIRST, FILE_LOCAL = 2, 3


@pytest.fixture(scope="module")
def filed(pkg, sctx, tmp_path_factory):
    """slot files of random bytes for slots 2 .. 4, the compact dataset built from them and what the peers would send"""
    d = tmp_path_factory.mktemp("resume_src")
    base = str(d / "slot")
    rng = np.random.default_rng(8)
    nb = FILE_GEOM["nCells"] * FILE_GEOM["cellSize"] // FILE_GEOM["blockSize"]
    data = {s: rng.integers(0, 256, (nb, FILE_GEOM["blockSize"]), dtype=np.uint8) for s in range(FILE_FIRST, FILE_FIRST + FILE_LOCAL)}
    for s, a in data.items():
        a.tofile("%s%d.dat" % (base, s))
    built = build_compact(sctx, pkg.make_config(file=base, **FILE_GEOM), FILE_FIRST, FILE_LOCAL)
    yield built, Source(sctx, pkg.make_config(file=base, **FILE_GEOM), built, FILE_FIRST, FILE_LOCAL, blocks_of=lambda s: data[s]), data
    built.free()


def damaged_session(pkg, sctx, filed, out):
    """a session over `out`/slot*.dat with two blocks still missing, saved and freed; then one byte of slot 2's block 3 flipped, slot 3's file
    cut in the middle of block 4 (below its present blocks 5 and 7) and slot 4's file deleted.  Returns what a re-check must drop."""
    built, src, data = filed
    base, path = str(out / "slot"), str(out / "session.ckpt")
    cfg = pkg.make_config(file=base, **FILE_GEOM)
    roots = built.local_roots()
    f = sctx.fill(cfg, roots, FILE_FIRST, FILE_LOCAL)
    held_back = [(3, 6), (4, 1)]
    for pairs in uneven_calls([p for p in src.pairs if p not in held_back], seed=2):
        assert (add(f, src, pairs)[0] == pkg.FILL_NEW).all()
    assert tuples(f.missing()[0]) == held_back
    f.save(path)
    f.free()
    bs = cfg.block_size
    with open(base + "2.dat", "r+b") as fh:
        fh.seek(3 * bs + 1000)
        fh.write(bytes([data[2][3][1000] ^ 0x04]))
    os.truncate(base + "3.dat", 4 * bs + bs // 2)
    os.remove(base + "4.dat")
    damage = [(2, 3), (3, 4), (3, 5), (3, 7)] + [(4, b) for b in range(src.nb) if b != 1]
    return cfg, roots, base, path, held_back, damage


def test_resume_drops_exactly_what_the_disk_no_longer_backs(pkg, sctx, filed, tmp_path):
    built, src, data = filed
    cfg, roots, base, path, held_back, damage = damaged_session(pkg, sctx, filed, tmp_path)
    g = sctx.fill_resume(cfg, roots, path, FILE_FIRST, FILE_LOCAL)
    assert g.n_dropped == len(damage) == 11
    missing = tuples(g.missing()[0])
    assert missing == sorted(held_back + damage)                                       # in (slot, block) order
    assert not os.path.exists(base + "4.dat")                                          # absence is a state: nothing was created or read
    status, n_new = add(g, src, missing)                                               # sent again with their proofs: NEW, and written
    assert (status == pkg.FILL_NEW).all() and n_new == len(missing)
    for s in data:
        assert open("%s%d.dat" % (base, s), "rb").read() == data[s].tobytes()
    filled = g.finish()
    assert filled.local_roots().tobytes() == roots.tobytes()
    assert filled.scrub()[2] == 0
    all_roots = np.zeros((cfg.n_slots, 32), dtype=np.uint8)
    all_roots[FILE_FIRST:FILE_FIRST + FILE_LOCAL] = roots
    for ds in (filled, built):
        ds.set_roots(all_roots)
    assert filled.proof_input(3, 99).json() == built.proof_input(3, 99).json()
    filled.free()
    g.free()


def test_trusting_the_files_drops_nothing_and_the_scrub_finds_the_damage(pkg, sctx, filed, tmp_path):
    built, src, data = filed
    cfg, roots, base, path, held_back, damage = damaged_session(pkg, sctx, filed, tmp_path)
    g = sctx.fill_resume(cfg, roots, path, FILE_FIRST, FILE_LOCAL, trust_files=True)
    assert g.n_dropped == 0 and tuples(g.missing()[0]) == held_back
    assert not os.path.exists(base + "4.dat")
    assert (add(g, src, held_back)[0] == pkg.FILL_NEW).all()
    filled = g.finish()                                                                # the kept roots are right: the top layer matches
    assert filled.local_roots().tobytes() == roots.tobytes()
    _, bad, n_bad = filled.scrub()
    assert n_bad == len(damage) and tuples(bad) == sorted(damage)                      # what a re-check would have dropped
    filled.free()
    g.free()


# ---- 4: a checkpoint whose layer 0 is wrong on purpose -----------------------------------------------------------------------------------------
def test_a_wrong_kept_root_is_dropped_or_caught_by_finish(pkg, oracle, sctx, fake, tmp_path):
    cfg, first, n_local, built, all_roots, src = fake("main")
    roots = all_roots[first:first + n_local]
    nb = src.nb
    path, wrong = str(tmp_path / "good.ckpt"), str(tmp_path / "wrong.ckpt")
    f = sctx.fill(cfg, roots, first, n_local)
    half = uneven_half(src.pairs, seed=5)
    add(f, src, half)
    before = tuples(f.missing()[0])
    f.save(path)
    f.free()
    c = M.parse_checkpoint(open(path, "rb").read())
    victim = sorted(half)[len(half) // 2]
    g_victim = (victim[0] - first) * nb + victim[1]
    assert c["bits"][g_victim] == 1
    c["layer0"][g_victim, 9] ^= 0x20
    open(wrong, "wb").write(M.write_checkpoint(c))                                    # a valid checksum over a wrong root

    g = sctx.fill_resume(cfg, roots, wrong, first, n_local)
    assert g.n_dropped == 1 and tuples(g.missing()[0]) == sorted(before + [victim])
    rest = tuples(g.missing()[0])
    assert (add(g, src, rest)[0] == pkg.FILL_NEW).all()
    finish_and_compare(pkg, oracle, g, cfg, first, n_local, built, all_roots)
    g.free()

    t = sctx.fill_resume(cfg, roots, wrong, first, n_local, trust_files=True)
    assert t.n_dropped == 0 and tuples(t.missing()[0]) == before
    assert (add(t, src, before)[0] == pkg.FILL_NEW).all()
    with pytest.raises(pkg.CodexP2Error) as e:
        t.finish()
    assert e.value.status == CP2_ERR_IO and "slot %d" % victim[0] in str(e.value), str(e.value)
    t.free()


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_create_no_session_and_say_why(pkg, sctx, fake, tmp_path):
    cfg, first, n_local, built, all_roots, src = fake("main")
    cfgd = GEOMS["main"][0]
    roots = all_roots[first:first + n_local]
    path = str(tmp_path / "session.ckpt")
    f = sctx.fill(cfg, roots, first, n_local)
    add(f, src, uneven_half(src.pairs, seed=6))
    before = f.missing()[0].tolist()
    f.save(path)
    f.free()
    raw = open(path, "rb").read()
    cut, gone = str(tmp_path / "cut.ckpt"), str(tmp_path / "gone.ckpt")
    open(cut, "wb").write(raw[:len(raw) - 40])
    other_root = roots.copy()
    other_root[1, 0] ^= 1
    L = sctx.L

    def refused(cfg_, first_, roots_, path_, status, text):
        out, dropped = ctypes.c_void_p(1234), ctypes.c_uint64(42)
        r = np.ascontiguousarray(roots_)
        st = L.cp2_fill_resume(sctx.h, ctypes.byref(cfg_), first_, n_local, pkg._p(r), path_.encode(), 0, ctypes.byref(out), ctypes.byref(dropped))
        msg = L.cp2_last_error(sctx.h).decode()
        assert st == status and out.value is None and dropped.value == 42, (st, msg)
        for word in text:
            assert word in msg, msg

    refused(pkg.make_config(**dict(cfgd, seed=2)), first, roots, path, CP2_ERR_INVALID, [path, "describes another session", "seed differs"])
    refused(pkg.make_config(**dict(cfgd, nCells=512)), first, roots, path, CP2_ERR_INVALID, [path, "n_cells differs (checkpoint 256, session 512)"])
    refused(cfg, first - 1, roots, path, CP2_ERR_INVALID, [path, "first_slot differs (checkpoint 2, session 1)"])
    refused(cfg, first, other_root, path, CP2_ERR_INVALID, [path, "stated root of slot %d differs" % (first + 1)])
    refused(cfg, first, roots, cut, CP2_ERR_IO, [cut, "truncated"])
    refused(cfg, first, roots, gone, CP2_ERR_IO, [gone, "cannot open"])
    refused(pkg.make_config(**dict(cfgd, nCells=96)), first, roots, path, CP2_ERR_INVALID, ["power of two"])       # cp2_fill_begin's checks first

    # a stated root of at least r names the same field element as the reduced value the checkpoint holds
    big = roots.copy()
    v = pkg.array_to_felts(roots[2])[0] + R
    assert v < 1 << 256
    big[2] = pkg.felt_bytes(v)
    g = sctx.fill_resume(cfg, big, path, first, n_local)
    assert g.n_dropped == 0 and g.missing()[0].tolist() == before
    g.free()


# ---- 6: many chunks ---------------------------------------------------------------------------------------------------------------------------------
def test_many_chunks_fake_and_files(pkg, oracle, monkeypatch, tmp_path):
    """1 MiB of staging and 64 KiB blocks: chunks of 8 blocks.  19 present blocks: two full chunks and a last one of 3.  Damage at the first
    and last entry of the plan and on both sides of a chunk edge (entries 0, 7, 8, 18): exactly those are dropped.  Fake source: a wrong kept
    root (the regenerated blocks cannot be damaged); slot files: a flipped byte on disk."""
    C, _ = oracle
    monkeypatch.setenv("CODEX_P2_STAGE_MB", "1")
    ctx = pkg.Context(0)
    cfgd = dict(maxDepth=16, maxLog2NSlots=3, cellSize=64, blockSize=65536, nSlots=5, nCells=4096, nSamples=3, seed=77)
    cfg = pkg.make_config(**cfgd)
    built = build_compact(ctx, cfg)
    roots = built.local_roots()
    for s in range(5):
        assert roots[s].tobytes() == C.fake_slot_root(C.slot_seed(77, s), 64, 65536, 4096, 4).tobytes()
    src = Source(ctx, cfg, built, 0, 5)
    nb = src.nb
    assert nb == 4
    held_back = (2, 1)
    present = [p for p in src.pairs if p != held_back]                                 # the plan's order: ascending (slot, block)
    victims = [present[i] for i in (0, 7, 8, 18)]
    assert len(present) == 19

    path, wrong = str(tmp_path / "fake.ckpt"), str(tmp_path / "wrong.ckpt")
    f = ctx.fill(cfg, roots)
    add(f, src, [present[i] for i in np.random.default_rng(4).permutation(19)])
    f.save(path)
    f.free()
    clean = ctx.fill_resume(cfg, roots, path)                                          # 19 regenerated blocks in three chunks, nothing to drop
    assert clean.n_dropped == 0 and tuples(clean.missing()[0]) == [held_back]
    clean.free()
    c = M.parse_checkpoint(open(path, "rb").read())
    for s, b in victims:
        c["layer0"][s * nb + b, 31 - b] ^= 0x01
    open(wrong, "wb").write(M.write_checkpoint(c))
    g = ctx.fill_resume(cfg, roots, wrong)
    assert g.n_dropped == 4 and tuples(g.missing()[0]) == sorted(victims + [held_back])
    g.free()

    base, fpath = str(tmp_path / "slot"), str(tmp_path / "files.ckpt")
    fcfg = pkg.make_config(file=base, **cfgd)                                          # the same bytes in slot files: the same roots
    f = ctx.fill(fcfg, roots)
    add(f, src, present)
    f.save(fpath)
    f.free()
    for s, b in victims:
        with open("%s%d.dat" % (base, s), "r+b") as fh:
            fh.seek(b * cfg.block_size + 65535 - 100 * s)
            byte = fh.read(1)
            fh.seek(-1, os.SEEK_CUR)
            fh.write(bytes([byte[0] ^ 0x80]))
    g = ctx.fill_resume(fcfg, roots, fpath)
    assert g.n_dropped == 4 and tuples(g.missing()[0]) == sorted(victims + [held_back])
    again = tuples(g.missing()[0])
    assert (add(g, src, again)[0] == pkg.FILL_NEW).all()
    filled = g.finish()
    assert filled.local_roots().tobytes() == roots.tobytes() and filled.scrub()[2] == 0
    for h in (filled, g, built):
        h.free()
    ctx.close()


# ---- 7: the launcher alone --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fru(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libfill_resume_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.fru_block_root_recheck.restype = ctypes.c_int
    lib.fru_block_root_recheck.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_uint64]
    return lib


GUARD = 256
PATTERN = ((np.arange(4099, dtype=np.int64) * 7 + 0xC3) % 255 + 1).astype(np.uint8)     # never zero


def guarded(torch, body):
    """the bytes of `body` on the device between GUARD bytes of a non-zero pattern; (tensor, pointer to the body, the whole buffer as sent)"""
    raw = np.ascontiguousarray(body).view(np.uint8).reshape(-1)
    whole = np.concatenate([np.resize(PATTERN, GUARD), raw, np.resize(PATTERN[::-1], GUARD)])
    t = torch.from_numpy(whole.copy()).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + GUARD, whole


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_the_launcher_alone(fru, n):
    """Distinct destination rows all over a layer 0 of n + 5 rows.  Three launches per n: every root equal; the first and the last lane differ in
    one bit; and the same with one lane's row AT n_rows, behind which a real, matching row lies -- a kernel that ignored the bound would
    answer 0 there, not fault.  The whole layer-0 buffer (rows past n_rows and guards included) and the verdicts with their guards are
    compared with the numpy model: nothing is stored out of range."""
    import torch
    rng = np.random.default_rng([0x7E5, n])
    n_rows = n + 5
    for case in ("equal", "first and last differ", "one row at n_rows"):
        layer0 = rng.integers(0, 256, size=(n_rows + 1, 32), dtype=np.uint8)            # row n_rows: backed, outside what the kernel may touch
        dest = rng.permutation(n_rows)[:n].astype(np.uint64)
        if case == "one row at n_rows":
            dest[n // 2] = n_rows
        fresh = layer0[dest.astype(np.int64)].copy()
        flips = [] if case == "equal" else sorted({0, n - 1} - ({n // 2} if case == "one row at n_rows" else set()))
        for i in flips:
            fresh[i, (7 * i) % 32] ^= np.uint8(1 << (i % 8))
        want_verdict, want_layer0 = M.recheck_model(fresh, dest, layer0, n_rows)
        assert int(want_verdict.sum()) == len(flips) + (case == "one row at n_rows")
        d_fresh = torch.from_numpy(fresh.reshape(-1).copy()).cuda()
        d_dest = torch.from_numpy(dest.view(np.uint8).copy()).cuda()
        t_layer0, p_layer0, sent = guarded(torch, layer0)
        t_verdict, p_verdict, vsent = guarded(torch, np.full(n, 0x77777777, dtype=np.uint32))
        assert fru.fru_block_root_recheck(d_fresh.data_ptr(), d_dest.data_ptr(), n, p_verdict, p_layer0, n_rows) == 0, case
        torch.cuda.synchronize()
        got_layer0, got_verdict = t_layer0.cpu().numpy(), t_verdict.cpu().numpy()
        want_all = sent.copy()
        want_all[GUARD:GUARD + want_layer0.size] = want_layer0.reshape(-1)
        assert np.array_equal(got_layer0, want_all), (case, np.nonzero(got_layer0 != want_all)[0][:8])
        vwant = vsent.copy()
        vwant[GUARD:GUARD + 4 * n] = want_verdict.view(np.uint8)
        assert np.array_equal(got_verdict, vwant), (case, np.nonzero(got_verdict != vwant)[0][:8])
    # nothing to do, and arguments the launcher refuses: nothing is launched
    assert fru.fru_block_root_recheck(d_fresh.data_ptr(), d_dest.data_ptr(), 0, p_verdict, p_layer0, n_rows) == 0
    assert fru.fru_block_root_recheck(None, d_dest.data_ptr(), n, p_verdict, p_layer0, n_rows) == 1                # hipErrorInvalidValue
    assert fru.fru_block_root_recheck(d_fresh.data_ptr(), d_dest.data_ptr(), n, p_verdict, None, n_rows) == 1
    torch.cuda.synchronize()
    assert np.array_equal(t_layer0.cpu().numpy(), want_all) and np.array_equal(t_verdict.cpu().numpy(), vwant)
