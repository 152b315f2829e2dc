"""GPU suite: fill sessions that serve -- cp2_fill_keep_nodes / cp2_fill_block_proofs.  A session that keeps the nodes of the paths it
proves must serve, while it is still filling, exactly the proofs cp2_dataset_block_proofs serves from a compact dataset built from the same
data; which blocks it can serve is checked against tests/fill_nodes_models.py.  The smallest cells and blocks of tests/test_gpu_fill.py,
1, 2, 4 and 16 blocks a slot, two or three local slots, fake source and slot files.  Every comparison is bit-exact."""
import faulthandler
import os
import stat

import numpy as np
import pytest

import fill_nodes_models as M
from test_gpu_fill import Source, add, build_compact, flip

pytestmark = pytest.mark.gpu

CP2_OK, CP2_ERR_INVALID, CP2_ERR_IO = 0, -1, -5
# name: (blocks per slot, first local slot, local slots) of a dataset of four slots
SHAPES = {"one_block": (1, 1, 3), "two_blocks": (2, 0, 2), "four_blocks": (4, 1, 3), "sixteen_blocks": (16, 2, 2)}


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


def config(pkg, nb, file=None):
    kw = dict(maxDepth=8, maxLog2NSlots=2, cellSize=64, blockSize=256, nSlots=4, nCells=4 * nb, nSamples=3, seed=40 + nb)
    return pkg.make_config(file=file, **kw) if file else pkg.make_config(**kw)


class World:
    """a compact dataset of the local range built from the data, and what the peers would send: the reference every proof is held against"""

    def __init__(self, pkg, ctx, name, directory=None):
        self.nb, self.first, self.n_local = SHAPES[name]
        self.data = None
        if directory:                                # slot files of random bytes; the session under test writes to another directory
            os.makedirs(os.path.join(directory, "src"))
            base = os.path.join(directory, "src", "slot")
            rng = np.random.default_rng(self.nb)
            self.data = {s: rng.integers(0, 256, (self.nb, 256), dtype=np.uint8) for s in range(4)}
            for s in range(4):
                self.data[s].tofile("%s%d.dat" % (base, s))
            os.makedirs(os.path.join(directory, "out"))
            self.out_dir = os.path.join(directory, "out")
            self.out_base = os.path.join(self.out_dir, "slot")
            self.cfg = config(pkg, self.nb, file=self.out_base)
            src_cfg = config(pkg, self.nb, file=base)
        else:
            self.cfg = src_cfg = config(pkg, self.nb)
        self.built = build_compact(ctx, src_cfg, self.first, self.n_local)
        self.roots = self.built.local_roots()
        self.src = Source(ctx, src_cfg, self.built, self.first, self.n_local, blocks_of=(lambda s: self.data[s]) if directory else None)
        self.pairs = self.src.pairs
        self.depth = self.src.paths.shape[1]

    def shuffled(self, seed):
        rng = np.random.default_rng([seed, self.nb])
        return [self.pairs[i] for i in rng.permutation(len(self.pairs))]

    def local(self, pair):
        return pair[0] - self.first, pair[1]

    def check(self, pkg, f, model, what=""):
        """every block of the range asked at once: the statuses are the model's, an OK proof is the dataset's, every other row is zeros; the
        statuses-only form answers the same"""
        status, roots, paths = f.block_proofs(self.pairs)
        want = [model.status(*self.local(p)) for p in self.pairs]
        assert status.tolist() == want, (what, status.tolist(), want)
        assert f.block_proofs(self.pairs, statuses_only=True).tolist() == want
        for i, p in enumerate(self.pairs):
            if want[i] == M.PROOF_OK:
                assert roots[i].tobytes() == self.src.roots[i].tobytes() and paths[i].tobytes() == self.src.paths[i].tobytes(), (what, p)
            else:
                assert not roots[i].any() and not paths[i].any(), (what, p)
        return status

    def free(self):
        self.built.free()


@pytest.fixture(scope="module")
def worlds(pkg, sctx):
    made = {name: World(pkg, sctx, name) for name in SHAPES}
    yield made
    for w in made.values():
        w.free()


def last_error(ctx):
    return ctx.L.cp2_last_error(ctx.h).decode()


def calls_of(order, size):
    return [order[i:i + size] for i in range(0, len(order), size)]


# ---- 1: a keeping session serves what the built dataset serves, from the first block on -----------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_serves_the_built_datasets_proofs_while_filling(pkg, sctx, worlds, name):
    w = worlds[name]
    f = sctx.fill(w.cfg, w.roots, w.first, w.n_local)
    f.keep_nodes()
    model = M.Session(w.nb, w.n_local)
    model.keep_nodes()
    w.check(pkg, f, model, "empty")
    for pairs in calls_of(w.shuffled(1), 5):
        status, n_new = add(f, w.src, pairs)
        assert (status == pkg.FILL_NEW).all() and n_new == len(pairs)
        for p in pairs:
            model.add(*w.local(p))
        got = w.check(pkg, f, model, "after %s" % (pairs,))
        assert all(got[w.src.index[p]] == pkg.FILL_PROOF_OK for p in pairs)                 # served from the moment it is present
    assert (w.check(pkg, f, model, "full") == pkg.FILL_PROOF_OK).all()
    filled = f.finish()
    got_roots, got_paths = filled.block_proofs(w.pairs)
    assert got_roots.tobytes() == w.src.roots.tobytes() and got_paths.tobytes() == w.src.paths.tobytes()
    assert filled.local_roots().tobytes() == w.roots.tobytes()
    f.free()
    filled.free()


# ---- 2: a peer fills from a peer that is still filling ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["four_blocks", "sixteen_blocks"])
def test_a_peer_fills_from_a_filling_peer(pkg, sctx, worlds, name):
    w = worlds[name]
    a = sctx.fill(w.cfg, w.roots, w.first, w.n_local)
    a.keep_nodes()
    order = w.shuffled(2)
    half = order[:len(order) // 2]
    for pairs in calls_of(half, 3):
        assert (add(a, w.src, pairs)[0] == pkg.FILL_NEW).all()
    b = sctx.fill(w.cfg, w.roots, w.first, w.n_local)
    status, roots, paths = a.block_proofs(half)
    assert (status == pkg.FILL_PROOF_OK).all()
    data = w.src.data(half)
    st, n_new = b.add(half, data, paths)                                                  # only what A serves, never the dataset's paths
    assert (st == pkg.FILL_NEW).all() and n_new == len(half)
    verdict, hashed = sctx.blocks_verify(w.cfg.cell_size, w.cfg.block_size, w.cfg.n_cells, w.roots, [(s - w.first, blk) for s, blk in half], data, paths)
    assert (verdict == pkg.BLOCK_MATCH).all() and hashed.tobytes() == roots.tobytes()
    assert b.missing(0)[1] == len(order) - len(half)
    a.free()
    b.free()


# ---- 3: a request that does not prove leaves nothing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["four_blocks", "sixteen_blocks"])
def test_unproved_data_leaves_nothing(pkg, sctx, worlds, name):
    w = worlds[name]
    f = sctx.fill(w.cfg, w.roots, w.first, w.n_local)
    f.keep_nodes()
    model = M.Session(w.nb, w.n_local)
    model.keep_nodes()
    s0 = w.first
    here = [(s0, b) for b in range(0, w.nb, 2)] + [(s0 + 1, 1)]                            # every even block of one slot: their siblings are absent
    assert (add(f, w.src, here)[0] == pkg.FILL_NEW).all()
    for p in here:
        model.add(*w.local(p))
    before = f.block_proofs(w.pairs)
    # absent blocks whose paths name rows the session holds (the roots of present blocks as their level-0 siblings, kept ancestors above):
    # the true block with one path bit flipped at every level in turn, and a wrong block under the true path
    bad = [(s0, 1)] * w.depth + [(s0, 3)]
    data, paths = w.src.data(bad), w.src.path(bad)
    for lvl in range(w.depth):
        paths[lvl] = flip(paths[lvl], lvl * 32 + 5)
    data[w.depth] = flip(data[w.depth], 17)
    status, n_new = f.add(bad, data, paths)
    assert (status == pkg.FILL_MISMATCH).all() and n_new == 0
    after = f.block_proofs(w.pairs)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    w.check(pkg, f, model, "after the mismatches")
    rest = [p for p in w.shuffled(3) if p not in here]
    for pairs in calls_of(rest, 4):
        assert (add(f, w.src, pairs)[0] == pkg.FILL_NEW).all()
        for p in pairs:
            model.add(*w.local(p))
        w.check(pkg, f, model)
    filled = f.finish()
    assert filled.block_proofs(w.pairs)[1].tobytes() == w.src.paths.tobytes()
    f.free()
    filled.free()


# ---- 4: turned on late, and after a resume ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["late", "resumed", "resumed_trusting"])
@pytest.mark.parametrize("name", ["two_blocks", "four_blocks", "sixteen_blocks"])
def test_turned_on_late_and_after_resume(pkg, sctx, worlds, tmp_path, name, how):
    w = worlds[name]
    order = w.shuffled(4)
    half, rest = order[:len(order) // 2], order[len(order) // 2:]
    f = sctx.fill(w.cfg, w.roots, w.first, w.n_local)
    model = M.Session(w.nb, w.n_local)
    for pairs in calls_of(half, 3):
        assert (add(f, w.src, pairs)[0] == pkg.FILL_NEW).all()
        for p in pairs:
            model.add(*w.local(p))
    with pytest.raises(pkg.CodexP2Error) as e:                                           # a plain session serves nothing
        f.block_proofs(half)
    assert e.value.status == CP2_ERR_INVALID and "cp2_fill_keep_nodes" in str(e.value)
    if how != "late":
        path = str(tmp_path / "session.ckpt")
        f.save(path)
        f.free()
        f = sctx.fill_resume(w.cfg, w.roots, path, w.first, w.n_local, trust_files=(how == "resumed_trusting"))
        assert f.n_dropped == 0
        with pytest.raises(pkg.CodexP2Error):                                              # a resumed session keeps no nodes until it is told to
            f.block_proofs(half)
    f.keep_nodes()
    model.keep_nodes()
    status = w.check(pkg, f, model, "just turned on")
    assert (status != pkg.FILL_PROOF_ABSENT).sum() == len(half)
    for p in rest:                                                                         # one block a call: PARTIAL turns OK exactly when the model says
        assert add(f, w.src, [p])[0].tolist() == [pkg.FILL_NEW]
        model.add(*w.local(p))
        w.check(pkg, f, model, "after %s" % (p,))
    assert (w.check(pkg, f, model, "full") == pkg.FILL_PROOF_OK).all()
    filled = f.finish()
    assert filled.block_proofs(w.pairs)[1].tobytes() == w.src.paths.tobytes()
    f.free()
    filled.free()


def test_a_half_full_session_has_partial_blocks_until_their_neighbours_arrive(pkg, sctx, worlds):
    """the case the parametrised walk may or may not meet, pinned: blocks 0 and 5 of 16 arrive, keeping is turned on, then 4, then 1"""
    w = worlds["sixteen_blocks"]
    s = w.first
    f = sctx.fill(w.cfg, w.roots, w.first, w.n_local)
    model = M.Session(w.nb, w.n_local)
    for p in [(s, 0), (s, 5)]:
        add(f, w.src, [p])
        model.add(*w.local(p))
    f.keep_nodes()
    model.keep_nodes()
    P, O, A = pkg.FILL_PROOF_PARTIAL, pkg.FILL_PROOF_OK, pkg.FILL_PROOF_ABSENT
    assert f.block_proofs([(s, 0), (s, 5), (s, 4)], statuses_only=True).tolist() == [P, P, A]
    add(f, w.src, [(s, 4)])                                                              # its path carries leaf 5's sibling row and every ancestor of 4 and 5
    model.add(*w.local((s, 4)))
    assert f.block_proofs([(s, 0), (s, 5), (s, 4)], statuses_only=True).tolist() == [P, O, O]
    add(f, w.src, [(s, 1)])
    model.add(*w.local((s, 1)))
    assert f.block_proofs([(s, 0), (s, 1), (s, 5), (s, 4), (s, 4)], statuses_only=True).tolist() == [O, O, O, O, O]
    w.check(pkg, f, model)
    f.free()


def test_a_keeping_sessions_checkpoint_is_a_plain_sessions(pkg, sctx, worlds, tmp_path):
    w = worlds["sixteen_blocks"]
    order = w.shuffled(5)
    half = order[:len(order) // 2]
    saved = []
    for keeping in (False, True):
        f = sctx.fill(w.cfg, w.roots, w.first, w.n_local)
        if keeping:
            add(f, w.src, half[:3])
            f.keep_nodes()
            add(f, w.src, half[3:])
        else:
            add(f, w.src, half)
        path = str(tmp_path / ("keeping.ckpt" if keeping else "plain.ckpt"))
        f.save(path)
        saved.append(open(path, "rb").read())
        f.free()
    assert saved[0] == saved[1] and saved[0][:8] == b"CP2FILL1"


# ---- 5: a block that proves but cannot be written ---------------------------------------------------------------------------------------------
def test_an_unwritten_block_stays_absent_and_its_neighbours_are_served(pkg, sctx, tmp_path):
    w = World(pkg, sctx, "four_blocks", str(tmp_path))
    s = w.first
    f = sctx.fill(w.cfg, w.roots, w.first, w.n_local)
    f.keep_nodes()
    model = M.Session(w.nb, w.n_local)
    model.keep_nodes()
    first_call = [(s, 0), (s + 1, 0), (s + 1, 2)]
    assert (add(f, w.src, first_call)[0] == pkg.FILL_NEW).all()
    for p in first_call:
        model.add(*w.local(p))
    w.check(pkg, f, model, "before the failure")
    name = "%s%d.dat" % (w.out_base, s + 1)

    # slot s + 1's file can no longer be written: for a user whom modes do not bind, a directory in the file's place
    kept = name + ".kept_aside"
    os.rename(name, kept)
    if os.geteuid() == 0:
        os.mkdir(name)
    else:
        os.chmod(w.out_dir, stat.S_IRUSR | stat.S_IXUSR)
    pairs = [(s, 1), (s + 1, 1), (s + 1, 3)]
    try:
        with pytest.raises(pkg.CodexP2Error) as e:
            add(f, w.src, pairs)
    finally:
        if os.geteuid() == 0:
            os.rmdir(name)
        else:
            os.chmod(w.out_dir, stat.S_IRWXU)
        os.rename(kept, name)
    assert e.value.status == CP2_ERR_IO
    assert e.value.fill_status.tolist() == [pkg.FILL_NEW, pkg.FILL_UNWRITTEN, pkg.FILL_UNWRITTEN]
    model.add(*w.local((s, 1)))
    model.add(*w.local((s + 1, 1)), written=False)
    model.add(*w.local((s + 1, 3)), written=False)
    status = w.check(pkg, f, model, "after the failure")
    A, O = pkg.FILL_PROOF_ABSENT, pkg.FILL_PROOF_OK
    assert [int(status[w.src.index[p]]) for p in [(s + 1, 1), (s + 1, 3), (s + 1, 0), (s + 1, 2), (s, 0), (s, 1)]] == [A, A, O, O, O, O]
    assert (add(f, w.src, pairs[1:])[0] == pkg.FILL_NEW).all()                             # sent again, now written
    for p in pairs[1:]:
        model.add(*w.local(p))
    w.check(pkg, f, model, "after the retry")
    f.free()
    w.free()


# ---- 6: refusals and no-ops ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(pkg, sctx, worlds):
    w = worlds["four_blocks"]
    L = pkg.load_library()
    s = w.first
    f = sctx.fill(w.cfg, w.roots, w.first, w.n_local)
    sb = np.array([(s, 0), (s, 1)], dtype=np.uint64)
    status = np.full(2, 7, dtype=np.uint32)
    roots = np.full((2, 32), 9, dtype=np.uint8)
    paths = np.full((2, w.depth, 32), 9, dtype=np.uint8)

    def call(sb_, n, status_=status, roots_=roots, paths_=paths):
        P = pkg._p
        return L.cp2_fill_block_proofs(f.h, P(sb_) if sb_ is not None else None, n, P(status_) if status_ is not None else None,
                                       P(roots_) if roots_ is not None else None, P(paths_) if paths_ is not None else None)

    def untouched():
        return (status == 7).all() and (roots == 9).all() and (paths == 9).all()

    assert call(sb, 2) == CP2_ERR_INVALID and "cp2_fill_keep_nodes" in last_error(sctx) and untouched()      # a plain session
    assert call(sb, 0) == CP2_ERR_INVALID
    add(f, w.src, [(s, 0)])
    f.keep_nodes()
    assert f.block_proofs(sb, statuses_only=True).tolist() == [pkg.FILL_PROOF_PARTIAL, pkg.FILL_PROOF_ABSENT]
    f.keep_nodes()                                                                       # the second call: CP2_OK, nothing changes
    assert L.cp2_fill_keep_nodes(f.h) == CP2_OK
    assert f.block_proofs(sb, statuses_only=True).tolist() == [pkg.FILL_PROOF_PARTIAL, pkg.FILL_PROOF_ABSENT]
    assert call(None, 2) == CP2_ERR_INVALID and untouched()
    assert call(sb, 2, status_=None) == CP2_ERR_INVALID and untouched()
    assert call(None, 0, None, None, None) == CP2_OK and call(sb, 0) == CP2_OK and untouched()             # n == 0
    for wrong, text in ((np.array([(s, 0), (s + w.n_local, 0)], dtype=np.uint64), "request 1"), (np.array([(s, w.nb), (s, 0)], dtype=np.uint64), "request 0"),
                        (np.array([(s, 0), (s - 1, 0)], dtype=np.uint64), "request 1")):
        assert call(wrong, 2) == CP2_ERR_INVALID and text in last_error(sctx) and untouched(), text
    assert call(sb, 2, roots_=None, paths_=None) == CP2_OK and status.tolist() == [pkg.FILL_PROOF_PARTIAL, pkg.FILL_PROOF_ABSENT]
    assert (roots == 9).all() and (paths == 9).all()
    # the same pair may repeat; block_roots alone, paths alone
    add(f, w.src, [(s, 1)])
    rep = np.array([(s, 1), (s, 1)], dtype=np.uint64)
    assert call(rep, 2, paths_=None) == CP2_OK and status.tolist() == [0, 0] and (paths == 9).all()
    assert roots[0].tobytes() == roots[1].tobytes() == w.src.roots[w.src.index[(s, 1)]].tobytes()
    assert call(rep, 2, roots_=None) == CP2_OK and paths[0].tobytes() == paths[1].tobytes() == w.src.paths[w.src.index[(s, 1)]].tobytes()
    # a finished session: its proofs come from the dataset
    rest = [p for p in w.pairs if p not in [(s, 0), (s, 1)]]
    add(f, w.src, rest)
    filled = f.finish()
    status[:] = 7
    roots[:] = 9
    paths[:] = 9
    assert call(sb, 2) == CP2_ERR_INVALID and "finished" in last_error(sctx) and untouched()
    assert L.cp2_fill_keep_nodes(f.h) == CP2_ERR_INVALID and "finished" in last_error(sctx)
    g = sctx.fill(w.cfg, w.roots, w.first, w.n_local)                                     # ... also for one that never kept nodes
    add(g, w.src, w.pairs)
    done = g.finish()
    assert L.cp2_fill_keep_nodes(g.h) == CP2_ERR_INVALID
    for h in (f, filled, g, done):
        h.free()
