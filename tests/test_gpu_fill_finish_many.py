"""GPU suite: cp2_fills_finish_many -- many fill sessions finished in one pass.  The call is defined by the call that exists, so the test is
twin worlds, as in tests/test_gpu_fill_many.py and on its small geometry (cells of 64 bytes, blocks of 256): seven sessions on one context
in each -- (nBlocks, n_local) = (1, 1), (2, 3), (8, 2), (16, 1), (64, 5), (8, 2) and, with cells of 128 and blocks of 512 bytes, (4, 2);
slot files and the fake source; keeping nodes and not; one completed by anchored adds, one resumed from a checkpoint, one completed by
cp2_fill_adopt, the rest by cp2_fills_add_many.  World A ends in ONE cp2_fills_finish_many, world B in the loop of cp2_fill_finish, and per
dataset the local roots, the range, cp2_dataset_keeps_trees == 2, cp2_dataset_block_proofs of every block (which touches every kept row)
and, after cp2_datasets_set_roots_many, one input.json must be equal bit for bit; the roots equal cp2_dataset_build's on the same data;
the kept files load in a fresh context and, for the fake source, are byte-equal to world B's.  Every refusal changes nothing, and a kept
file that cannot be written leaves every session usable.

The CP2_ERR_IO verdict path has no route through the API: proved layer-0 rows cannot disagree with the stated root, and the single call
has no such test either.  It is covered by the launcher test (tests/test_gpu_fill_finish_many_unit.py: the verdicts of wrong stated
roots) and by the CPU plan check (tests/test_fill_finish_many_cpu.py: which session and slot are named, and that nothing is handed
over).  Nothing here corrupts device memory to reach it."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest

import fill_finish_many_models as M
from test_gpu_fill import Source, build_compact

pytestmark = pytest.mark.gpu

CP2_OK, CP2_ERR_INVALID, CP2_ERR_IO = 0, -1, -5
N_SLOTS = 8
# blocks a slot, slot files, keeps nodes, first local slot, local slots, how it is completed, (cellSize, blockSize)
SHAPES = [(1, False, False, 0, 1, "many", (64, 256)), (2, True, True, 1, 3, "anchored", (64, 256)), (8, False, True, 0, 2, "many", (64, 256)),
          (16, True, False, 2, 1, "resumed", (64, 256)), (64, False, True, 3, 5, "many", (64, 256)), (8, True, True, 6, 2, "adopted", (64, 256)),
          (4, False, False, 4, 2, "many", (128, 512))]
INCOMPLETE = 2
SENTINEL = 0x5E5E
ENTROPY = 4242


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


def last_error(ctx):
    return ctx.L.cp2_last_error(ctx.h).decode()


class Spec:
    """one dataset: its data, the compact dataset cp2_dataset_build makes of it and what the peers would send; shared by both worlds"""

    def __init__(self, pkg, ctx, k, directory):
        self.k = k
        self.nb, self.files, self.keep, self.first, self.n_local, self.how, (cell, block) = SHAPES[k]
        self.block = block
        self.kw = dict(maxDepth=8, maxLog2NSlots=3, cellSize=cell, blockSize=block, nSlots=N_SLOTS, nCells=(block // cell) * self.nb, nSamples=3,
                       seed=700 + k)
        self.pkg, self.data = pkg, None
        if self.files:
            os.makedirs(os.path.join(directory, "src%d" % k))
            base = os.path.join(directory, "src%d" % k, "slot")
            rng = np.random.default_rng([0xF1, k])
            self.data = {s: rng.integers(0, 256, (self.nb, block), dtype=np.uint8) for s in range(N_SLOTS)}
            for s in range(N_SLOTS):
                self.data[s].tofile("%s%d.dat" % (base, s))
            self.src_cfg = pkg.make_config(file=base, **self.kw)
        else:
            self.src_cfg = pkg.make_config(**self.kw)
        self.built = build_compact(ctx, self.src_cfg, self.first, self.n_local)
        self.roots = self.built.local_roots()
        self.src = Source(ctx, self.src_cfg, self.built, self.first, self.n_local, blocks_of=(lambda s: self.data[s]) if self.files else None)
        self.pairs = self.src.pairs
        self.depth = self.src.paths.shape[1]
        rng = np.random.default_rng([0xF2, k])                 # the manifest: random field elements, the built roots in the local rows
        self.manifest = np.zeros((N_SLOTS, 32), dtype=np.uint8)
        self.manifest[:, :31] = rng.integers(0, 256, size=(N_SLOTS, 31), dtype=np.uint8)
        self.manifest[self.first:self.first + self.n_local] = self.roots

    def cfg_for(self, out_base):
        return self.pkg.make_config(file=out_base, **self.kw) if self.files else self.src_cfg


@pytest.fixture(scope="module")
def specs(pkg, sctx, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fill_finish_many_src"))
    made = [Spec(pkg, sctx, k, d) for k in range(len(SHAPES))]
    assert [(sp.nb, sp.n_local) for sp in made[:5]] == [(1, 1), (2, 3), (8, 2), (16, 1), (64, 5)]
    yield made
    for sp in made:
        sp.built.free()


class World:
    """the sessions of one world, every one complete unless `leave_out` names (session, slot, block) pairs to hold back"""

    def __init__(self, pkg, ctx, specs, directory, leave_out=()):
        self.ctx, self.specs = ctx, specs
        self.sessions, self.cfgs, self.out_dirs = [], [], []
        many = []
        for sp in specs:
            out_dir = os.path.join(directory, "out%d" % sp.k)
            os.makedirs(out_dir)
            cfg = sp.cfg_for(os.path.join(out_dir, "slot"))
            f = ctx.fill(cfg, sp.roots, sp.first, sp.n_local)
            held = [(s, b) for k, s, b in leave_out if k == sp.k]
            pairs = [p for p in sp.pairs if p not in held]
            if sp.how == "resumed":                       # half by plain adds, a checkpoint, a resume, the rest by plain adds
                half = pairs[:len(pairs) // 2]
                assert (f.add(half, sp.src.data(half), sp.src.path(half))[0] == 0).all()
                path = os.path.join(directory, "session%d.ckpt" % sp.k)
                f.save(path)
                f.free()
                f = ctx.fill_resume(cfg, sp.roots, path, sp.first, sp.n_local)
                assert f.n_dropped == 0
                rest = pairs[len(pairs) // 2:]
                assert (f.add(rest, sp.src.data(rest), sp.src.path(rest))[0] == 0).all()
            if sp.keep:
                f.keep_nodes()
            if sp.how == "anchored":                      # one whole path per slot, then every other block at its lowest anchor
                whole = [p for p in pairs if p[1] == 0]
                assert (f.add(whole, sp.src.data(whole), sp.src.path(whole))[0] == 0).all()
                rest = [p for p in pairs if p[1] != 0]
                lv = f.anchors(rest)
                assert (lv < sp.depth).any()
                packed = np.concatenate([sp.src.paths[sp.src.index[p]][:int(a)] for p, a in zip(rest, lv)] + [np.zeros((0, 32), np.uint8)])
                assert (f.add_anchored(rest, sp.src.data(rest), lv, packed if packed.size else None)[0] == 0).all()
            if sp.how == "adopted":                       # the bytes are on disk already; the stated roots vouch for whole slots
                for s in range(sp.first, sp.first + sp.n_local):
                    sp.data[s].tofile(os.path.join(out_dir, "slot%d.dat" % s))
                assert f.adopt() == (len(sp.pairs), len(sp.pairs))
            if sp.how == "many":
                many += [(len(self.sessions), s, b) for s, b in pairs]
            self.sessions.append(f)
            self.cfgs.append(cfg)
            self.out_dirs.append(out_dir)
        # the sessions of the small geometry in one cp2_fills_add_many; the other cell and block size in a call of its own
        for block in sorted({sp.block for sp in specs}):
            reqs = [r for r in many if specs[r[0]].block == block]
            ks = sorted({r[0] for r in reqs})
            req = np.array([(ks.index(k), s, b) for k, s, b in reqs], dtype=np.uint64).reshape(-1, 3)
            data = np.concatenate([specs[k].src.data([(s, b)]) for k, s, b in reqs])
            paths = np.concatenate([specs[k].src.paths[specs[k].src.index[(s, b)]] for k, s, b in reqs])
            st, _ = pkg.fills_add_many(ctx, [self.sessions[k] for k in ks], req, data, paths)
            assert (st == 0).all()
        for sp, f in zip(specs, self.sessions):
            assert f.missing(0)[1] == len([r for r in leave_out if r[0] == sp.k])

    def free(self):
        for f in self.sessions:
            f.free()


def observables(sp, ds):
    """what a finished dataset shows: range, kept mode, local roots, the proofs of every block"""
    roots, paths = ds.block_proofs(sp.pairs)
    return (ds.first_slot, ds.n_local, ds.tree_mode, ds.local_roots().tobytes(), roots.tobytes(), paths.tobytes())


def refuses_everything_but_free(pkg, sp, f):
    one = sp.pairs[:1]
    for call in (lambda: f.add(one, sp.src.data(one), sp.src.path(one)), lambda: f.save(os.devnull), lambda: f.finish()):
        with pytest.raises(pkg.CodexP2Error) as e:
            call()
        assert e.value.status == CP2_ERR_INVALID and "finished" in str(e.value)
    assert f.missing(0)[1] == 0


# ---- 1: one call leaves what the loop leaves -----------------------------------------------------------------------------------------------
def test_one_call_leaves_what_the_loop_of_finishes_leaves(pkg, sctx, specs, tmp_path, capfd):
    a, b = World(pkg, sctx, specs, str(tmp_path / "A")), World(pkg, sctx, specs, str(tmp_path / "B"))
    caches = {w: [None if sp.k == 2 else os.path.join(str(tmp_path), "%s_kept%d.cache" % (name, sp.k)) for sp in specs] for w, name in ((a, "A"), (b, "B"))}
    os.environ["CP2_TRACE"] = "1"
    try:
        capfd.readouterr()
        got = pkg.fills_finish_many(sctx, a.sessions, caches[a])
        lines = [ln for ln in capfd.readouterr().err.splitlines() if "fills finish many:" in ln]
    finally:
        del os.environ["CP2_TRACE"]
    want = [f.finish(c) for f, c in zip(b.sessions, caches[b])]
    # one trace line: sessions, slots, rows built, launches (one per level of the deepest session), kept forms saved
    assert len(lines) == 1 and "%d session(s), %d slot(s)" % (len(specs), sum(sp.n_local for sp in specs)) in lines[0], lines
    rows_built = sum(sp.n_local * sum(M.layer_sizes(sp.nb)[1:]) for sp in specs)
    assert "%d row(s) built, %d launch(es), %d kept form(s) saved" % (rows_built, max(sp.depth for sp in specs), len(specs) - 1) in lines[0], lines
    assert all(f.finished for f in a.sessions)
    for sp, g, w in zip(specs, got, want):
        assert observables(sp, g) == observables(sp, w), sp.k
        assert g.tree_mode == 2 and (g.first_slot, g.n_local) == (sp.first, sp.n_local)
        assert g.local_roots().tobytes() == sp.roots.tobytes()                  # cp2_dataset_build's, on the same data
        assert g.block_proofs(sp.pairs)[0].tobytes() == sp.src.roots.tobytes() and g.block_proofs(sp.pairs)[1].tobytes() == sp.src.paths.tobytes()
    # the dataset trees in one pass, then one input.json per dataset against the loop's
    sctx.set_roots_many(got, [sp.manifest for sp in specs])
    for sp, w in zip(specs, want):
        w.set_roots(sp.manifest)
    for sp, g, w in zip(specs, got, want):
        slot = sp.first + sp.n_local - 1
        assert g.root().tobytes() == w.root().tobytes()
        assert g.proof_input(slot, ENTROPY + sp.k).json() == w.proof_input(slot, ENTROPY + sp.k).json() == \
            sp_built_json(sp, slot)
    # every session of both worlds refuses add, save and finish, and has nothing missing
    for w in (a, b):
        for sp, f in zip(specs, w.sessions):
            refuses_everything_but_free(pkg, sp, f)
    # the kept files: byte-equal for the fake source, and a fresh context's cached build loads each to the same roots
    fresh = pkg.Context(0)
    for sp in specs:
        pa, pb = caches[a][sp.k], caches[b][sp.k]
        if pa is None:
            assert not [n for n in os.listdir(str(tmp_path)) if n.endswith("kept%d.cache" % sp.k)]
            continue
        assert os.path.exists(pa) and os.path.exists(pb)
        if not sp.files:
            assert open(pa, "rb").read() == open(pb, "rb").read(), sp.k
        loaded = build_compact(fresh, a.cfgs[sp.k], sp.first, sp.n_local, cache=pa)
        assert loaded.local_roots().tobytes() == sp.roots.tobytes()
        assert loaded.block_proofs(sp.pairs)[1].tobytes() == sp.src.paths.tobytes()
        loaded.free()
    fresh.close()
    for d in got + want:
        d.free()
    a.free()
    b.free()


def sp_built_json(sp, slot):
    """the same input.json from the dataset cp2_dataset_build made of the same data"""
    sp.built.set_roots(sp.manifest)
    return sp.built.proof_input(slot, ENTROPY + sp.k).json()


# ---- 2: refusals: all or nothing ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_changes_nothing(pkg, sctx, specs, tmp_path):
    held = (INCOMPLETE, specs[INCOMPLETE].first + 1, 5)
    a = World(pkg, sctx, specs, str(tmp_path / "A"), leave_out=[held])
    L = pkg.load_library()
    n = len(a.sessions)
    complete = [k for k in range(n) if k != INCOMPLETE]
    kept_dir = tmp_path / "kept"
    kept_dir.mkdir()
    out = (ctypes.c_void_p * n)(*([SENTINEL] * n))
    paths = (ctypes.c_char_p * n)(*[os.fsencode(str(kept_dir / ("k%d" % k))) for k in range(n)])

    def handles(ks, **swap):
        x = (ctypes.c_void_p * n)(*[a.sessions[k].h for k in ks] + [None] * (n - len(ks)))
        for i, h in swap.items():
            x[int(i[1:])] = h
        return x

    def refused(where, hs, nf, ctx_=sctx.h, out_=out):
        assert L.cp2_fills_finish_many(ctx_, hs, nf, paths, out_) == CP2_ERR_INVALID, where
        if where:
            assert where in last_error(sctx), (where, last_error(sctx))
        assert list(out) == [SENTINEL] * n and os.listdir(str(kept_dir)) == []
        assert [f.missing(0)[1] for f in a.sessions] == [int(k == INCOMPLETE) for k in range(n)]

    m = len(complete)
    refused(None, handles(complete), m, ctx_=None)
    refused("fills and out must not be NULL", None, m)
    refused("fills and out must not be NULL", handles(complete), m, out_=None)
    other = pkg.Context(0)
    stranger = other.fill(specs[0].src_cfg, specs[0].roots, specs[0].first, specs[0].n_local)
    done = sctx.fill(specs[0].src_cfg, specs[0].roots, specs[0].first, specs[0].n_local)
    assert (done.add(specs[0].pairs, specs[0].src.data(specs[0].pairs), specs[0].src.path(specs[0].pairs))[0] == 0).all()
    filled = done.finish()
    refused("fills[3] is NULL", handles(complete, k3=None), m)
    refused("fills[3] belongs to another context", handles(complete, k3=stranger.h), m)
    refused("fills[3]: fill: the session is finished", handles(complete, k3=done.h), m)
    refused("fills[4] is listed twice", handles(complete, k4=a.sessions[complete[1]].h), m)
    refused("fills[2]: fill: 1 block(s) are missing, the first is (slot %d, block %d)" % held[1:], handles(list(range(n))), n)
    refused("fills[0]: fill: 1 block(s) are missing", handles([INCOMPLETE] + complete), n)
    # n_fills == 0 is nothing to do, whatever else is passed
    assert L.cp2_fills_finish_many(sctx.h, None, 0, None, None) == CP2_OK and L.cp2_fills_finish_many(sctx.h, handles(complete), 0, paths, out) == CP2_OK
    assert list(out) == [SENTINEL] * n and os.listdir(str(kept_dir)) == []
    # afterwards the complete sessions still finish one by one, and the incomplete one takes its block and then finishes
    sp = specs[INCOMPLETE]
    one = [held[1:]]
    assert a.sessions[INCOMPLETE].add(one, sp.src.data(one), sp.src.path(one))[0].tolist() == [pkg.FILL_NEW]
    for sp, f in zip(specs, a.sessions):
        ds = f.finish()
        assert ds.local_roots().tobytes() == sp.roots.tobytes() and ds.block_proofs(sp.pairs)[1].tobytes() == sp.src.paths.tobytes()
        ds.free()
    for h in (filled, done, stranger):
        h.free()
    other.close()
    a.free()


# ---- 3: a kept file that cannot be written ---------------------------------------------------------------------------------------------------------
def test_an_unwritable_cache_path_makes_no_dataset_and_leaves_every_session_usable(pkg, sctx, specs, tmp_path):
    a = World(pkg, sctx, specs, str(tmp_path / "A"))
    L = pkg.load_library()
    n = len(a.sessions)
    good = [str(tmp_path / ("kept%d" % k)) for k in range(n)]
    bad = list(good)
    bad[3] = str(tmp_path / "no_such_directory" / "kept3")
    out = (ctypes.c_void_p * n)(*([SENTINEL] * n))
    hs = (ctypes.c_void_p * n)(*[f.h for f in a.sessions])
    st = L.cp2_fills_finish_many(sctx.h, hs, n, (ctypes.c_char_p * n)(*[os.fsencode(p) for p in bad]), out)
    assert st == CP2_ERR_IO and "fills[3]" in last_error(sctx) and "no_such_directory" in last_error(sctx), (st, last_error(sctx))
    assert list(out) == [SENTINEL] * n
    # the kept files of the earlier sessions stay (valid caches of complete sessions); none of a later one was begun
    assert [os.path.exists(p) for p in good] == [k < 3 for k in range(n)]
    for sp, f in zip(specs, a.sessions):                       # every session is complete and not finished: it still serves and saves
        assert f.missing(0)[1] == 0
        f.save(str(tmp_path / ("again%d.ckpt" % sp.k)))
        if sp.keep:
            assert f.block_proofs(sp.pairs)[2].tobytes() == sp.src.paths.tobytes()
    got = pkg.fills_finish_many(sctx, a.sessions, good)        # a second call with good paths succeeds
    fresh = pkg.Context(0)
    for sp, g in zip(specs, got):
        assert g.local_roots().tobytes() == sp.roots.tobytes() and g.block_proofs(sp.pairs)[1].tobytes() == sp.src.paths.tobytes()
        loaded = build_compact(fresh, a.cfgs[sp.k], sp.first, sp.n_local, cache=good[sp.k])
        assert loaded.local_roots().tobytes() == sp.roots.tobytes()
        loaded.free()
        g.free()
    fresh.close()
    a.free()
