"""GPU suite: anchored fill adds -- cp2_fill_anchors / cp2_fill_add_anchored.  A session that keeps nodes must accept a block on the
strength of the lowest node it already holds above it, with only the siblings below that node, and end as exactly the dataset
cp2_dataset_build makes from the same data.  The small geometry of tests/test_gpu_fill_serve.py (cells of 64 bytes, blocks of 256), 4, 8
and 64 blocks a slot, fake source and slot files.  Every comparison is bit-exact."""
import faulthandler
import os
import stat

import numpy as np
import pytest

import fill_anchor_models as A
from test_gpu_fill import Source, add, build_compact, flip
from test_gpu_fill_serve import config

pytestmark = pytest.mark.gpu

CP2_OK, CP2_ERR_INVALID, CP2_ERR_IO = 0, -1, -5
N_SLOTS = 4                                          # every slot of the dataset is local: the filled dataset needs no roots from elsewhere


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


class World:
    """a compact dataset of all four slots built from the data, and what the peers would send: the reference everything is held against"""

    def __init__(self, pkg, ctx, nb, directory=None):
        self.nb, self.first, self.n_local = nb, 0, N_SLOTS
        self.data = None
        if directory:                                # slot files of random bytes; the session under test writes to another directory
            os.makedirs(os.path.join(directory, "src"))
            self.src_base = os.path.join(directory, "src", "slot")
            rng = np.random.default_rng(nb)
            self.data = {s: rng.integers(0, 256, (nb, 256), dtype=np.uint8) for s in range(N_SLOTS)}
            for s in range(N_SLOTS):
                self.data[s].tofile("%s%d.dat" % (self.src_base, s))
            self.out_dir = os.path.join(directory, "out")
            os.makedirs(self.out_dir)
            self.out_base = os.path.join(self.out_dir, "slot")
            self.cfg = config(pkg, nb, file=self.out_base)
            src_cfg = config(pkg, nb, file=self.src_base)
        else:
            self.cfg = src_cfg = config(pkg, nb)
        self.built = build_compact(ctx, src_cfg, 0, N_SLOTS)
        self.roots = self.built.local_roots()
        self.src = Source(ctx, src_cfg, self.built, 0, N_SLOTS, blocks_of=(lambda s: self.data[s]) if directory else None)
        self.pairs = self.src.pairs
        self.depth = self.src.paths.shape[1]
        assert self.depth == A.depth_of(nb)

    def shuffled(self, seed):
        rng = np.random.default_rng([seed, self.nb])
        return [self.pairs[i] for i in rng.permutation(len(self.pairs))]

    def session(self, ctx, keep=True):
        f = ctx.fill(self.cfg, self.roots, 0, N_SLOTS)
        if keep:
            f.keep_nodes()
        return f

    def packed(self, pairs, levels):
        rows = [self.src.paths[self.src.index[p]][:int(a)] for p, a in zip(pairs, levels)]
        return np.concatenate(rows + [np.zeros((0, 32), np.uint8)])

    def add_anchored(self, f, pairs, levels=None, data=None, paths=None):
        """the blocks of `pairs` with the lowest siblings the levels ask for (default: what cp2_fill_anchors names right now)"""
        levels = f.anchors(pairs) if levels is None else np.asarray(levels, dtype=np.uint32)
        status, n_new = f.add_anchored(pairs, self.src.data(pairs) if data is None else data, levels, self.packed(pairs, levels) if paths is None else paths)
        return status, n_new, levels

    def check_finished(self, pkg, f, entropy=1234567):
        """cp2_fill_finish yields the dataset cp2_dataset_build makes: slot roots, every block proof, one proof-input JSON byte for byte"""
        filled = f.finish()
        assert filled.tree_mode == 2 and filled.local_roots().tobytes() == self.roots.tobytes()
        got_roots, got_paths = filled.block_proofs(self.pairs)
        assert got_roots.tobytes() == self.src.roots.tobytes() and got_paths.tobytes() == self.src.paths.tobytes()
        for ds in (self.built, filled):
            ds.set_roots(None)
        assert filled.root().tobytes() == self.built.root().tobytes()
        assert filled.proof_input(2, entropy).json() == self.built.proof_input(2, entropy).json()
        filled.free()

    def free(self):
        self.built.free()


@pytest.fixture(scope="module")
def worlds(pkg, sctx):
    made = {nb: World(pkg, sctx, nb) for nb in (4, 8, 64)}
    yield made
    for w in made.values():
        w.free()


def last_error(ctx):
    return ctx.L.cp2_last_error(ctx.h).decode()


# ---- 1: a whole slot at the lowest anchors, one block a call -----------------------------------------------------------------------------------
@pytest.mark.parametrize("files", [False, True], ids=["fake", "files"])
@pytest.mark.parametrize("nb", [8, 64])
def test_lowest_anchors_one_block_a_call_take_n_blocks_minus_one_siblings(pkg, sctx, worlds, tmp_path, nb, files):
    w = World(pkg, sctx, nb, str(tmp_path)) if files else worlds[nb]
    f = w.session(sctx)
    assert (f.anchors(w.pairs) == w.depth).all()                                         # an empty session holds the stated roots only
    siblings, bare = 0, 0
    for p in w.shuffled(11):
        status, n_new, levels = w.add_anchored(f, [p])
        assert status.tolist() == [pkg.FILL_NEW] and n_new == 1, (p, status, levels)
        assert f.anchors([p]).tolist() == [0]
        siblings += int(levels[0])
        bare += int(levels[0] == 0)
    assert siblings == N_SLOTS * (nb - 1) and bare == N_SLOTS * nb // 2                  # against depth x nBlocks a slot with whole paths
    assert f.missing(0)[1] == 0 and (f.anchors(w.pairs) == 0).all()
    w.check_finished(pkg, f)
    if files:
        for s in range(N_SLOTS):
            assert open("%s%d.dat" % (w.out_base, s), "rb").read() == w.data[s].tobytes()
        w.free()
    f.free()


# ---- 2: batches of mixed levels, anchors asked once a batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [8, 64])
def test_batches_of_mixed_levels(pkg, sctx, worlds, nb):
    w = worlds[nb]
    f = w.session(sctx)
    order = w.shuffled(12)
    seen, siblings = set(), 0
    for k in range(0, len(order), 7):
        pairs = order[k:k + 7]
        status, n_new, levels = w.add_anchored(f, pairs)
        assert (status == pkg.FILL_NEW).all() and n_new == len(pairs), (pairs, status, levels)
        seen.add(tuple(sorted(set(levels.tolist()))))
        siblings += int(levels.sum())
    assert any(len(s) > 1 for s in seen)                                                 # lengths really were mixed inside a call
    assert N_SLOTS * (nb - 1) <= siblings < N_SLOTS * nb * w.depth                       # the anchors of a batch are those of its start
    w.check_finished(pkg, f)
    f.free()


def test_a_node_that_only_the_same_call_would_prove_does_not_count(pkg, sctx, tmp_path):
    w = World(pkg, sctx, 8, str(tmp_path))
    f = w.session(sctx)
    s = 1
    assert (w.add_anchored(f, [(0, 5)])[0] == pkg.FILL_NEW).all()
    before = [open("%s%d.dat" % (w.out_base, 0), "rb").read(), sorted(os.listdir(w.out_dir))]
    anchors_before, proofs_before = f.anchors(w.pairs), f.block_proofs(w.pairs)
    pairs = [(s, 2), (s, 3), (s, 0)]                                                     # block 2's whole path would prove leaf 3
    levels = np.array([w.depth, 0, w.depth], dtype=np.uint32)
    status = np.full(3, 7, dtype=np.uint32)
    with pytest.raises(pkg.CodexP2Error) as e:
        f.add_anchored(pairs, w.src.data(pairs), levels, w.packed(pairs, levels), status=status)
    assert e.value.status == CP2_ERR_INVALID and "request 1:" in str(e.value) and "not known" in str(e.value)
    assert (status == 7).all() and e.value.n_new == 0
    assert [open("%s%d.dat" % (w.out_base, 0), "rb").read(), sorted(os.listdir(w.out_dir))] == before
    assert f.anchors(w.pairs).tolist() == anchors_before.tolist() and f.missing(0)[1] == len(w.pairs) - 1
    for x, y in zip(proofs_before, f.block_proofs(w.pairs)):
        assert x.tobytes() == y.tobytes()
    assert w.add_anchored(f, pairs[:1])[0].tolist() == [pkg.FILL_NEW]                    # in two calls it is accepted
    assert w.add_anchored(f, pairs[1:2], levels=[0])[0].tolist() == [pkg.FILL_NEW]
    f.free()
    w.free()


# ---- 3: what does not prove leaves nothing ----------------------------------------------------------------------------------------------------------
def test_a_wrong_block_and_a_wrong_sibling_leave_nothing(pkg, sctx, worlds):
    w = worlds[8]
    f = w.session(sctx)
    assert (w.add_anchored(f, [(0, 0), (0, 7), (1, 4)])[0] == pkg.FILL_NEW).all()
    # leaf 1 is known as block 0's sibling; above block 5 node (1, 2) is known as a sibling of block 7's path and node (2, 1) as its
    # ancestor: any known level may be stated, and the wrong sibling goes in under level 2
    assert f.anchors([(0, 1), (0, 5)]).tolist() == [0, 1]
    anchors_before, proofs_before, missing_before = f.anchors(w.pairs), f.block_proofs(w.pairs), f.missing()[0]
    bad = [(0, 1), (0, 5)]
    data = w.src.data(bad)
    data[0] = flip(data[0], 17)
    paths = w.packed(bad, [0, 2]).copy()
    paths[1] = flip(paths[1], 9)
    status, n_new, _ = w.add_anchored(f, bad, levels=[0, 2], data=data, paths=paths)
    assert status.tolist() == [pkg.FILL_MISMATCH, pkg.FILL_MISMATCH] and n_new == 0
    assert f.anchors(w.pairs).tolist() == anchors_before.tolist() and f.missing()[0].tolist() == missing_before.tolist()
    for x, y in zip(proofs_before, f.block_proofs(w.pairs)):
        assert x.tobytes() == y.tobytes()
    status, n_new, _ = w.add_anchored(f, bad, levels=[0, 2])                             # the true ones go in
    assert status.tolist() == [pkg.FILL_NEW, pkg.FILL_NEW] and n_new == 2
    f.free()


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, sctx, worlds):
    w = worlds[4]
    L, P = pkg.load_library(), pkg._p
    pairs = [(0, 0), (0, 1)]
    sb = np.array(pairs, dtype=np.uint64)
    data, levels = w.src.data(pairs), np.array([w.depth, w.depth], dtype=np.uint32)
    paths = w.packed(pairs, levels)
    status = np.full(2, 7, dtype=np.uint32)
    n_new = __import__("ctypes").c_size_t(5)

    def call(f, sb_=sb, data_=data, levels_=levels, paths_=paths, n=2, status_=status):
        opt = lambda a: P(a) if a is not None else None      # noqa: E731
        return L.cp2_fill_add_anchored(f.h, opt(sb_), opt(data_), opt(levels_), opt(paths_), n, opt(status_), __import__("ctypes").byref(n_new))

    def untouched():
        return (status == 7).all() and n_new.value == 5

    plain = w.session(sctx, keep=False)                                                  # a session that does not keep nodes
    assert call(plain) == CP2_ERR_INVALID and "cp2_fill_keep_nodes" in last_error(sctx) and untouched()
    assert plain.anchors(w.pairs).tolist() == [w.depth] * len(w.pairs)                   # ... is answered all the same: depth throughout
    assert plain.missing(0)[1] == len(w.pairs)
    plain.free()

    f = w.session(sctx)
    assert call(f, levels_=np.array([w.depth, w.depth + 1], dtype=np.uint32)) == CP2_ERR_INVALID and "request 1:" in last_error(sctx) and untouched()
    assert call(f, levels_=None) == CP2_ERR_INVALID and untouched()
    assert call(f, paths_=None) == CP2_ERR_INVALID and untouched()                        # NULL paths with a level that is not 0
    assert call(f, sb_=None) == CP2_ERR_INVALID and call(f, data_=None) == CP2_ERR_INVALID and call(f, status_=None) == CP2_ERR_INVALID and untouched()
    assert call(f, sb_=np.array([(0, 0), (N_SLOTS, 0)], dtype=np.uint64)) == CP2_ERR_INVALID and "request 1" in last_error(sctx) and untouched()
    assert call(f, sb_=np.array([(0, w.nb), (0, 0)], dtype=np.uint64)) == CP2_ERR_INVALID and "request 0" in last_error(sctx) and untouched()
    assert call(f, levels_=np.array([0, w.depth], dtype=np.uint32)) == CP2_ERR_INVALID and "request 0:" in last_error(sctx) and untouched()
    assert f.missing(0)[1] == len(w.pairs)
    assert call(f, None, None, None, None, 0, None) == CP2_OK and n_new.value == 0        # n == 0
    n_new.value = 5
    out = np.full(2, 9, dtype=np.uint32)
    assert L.cp2_fill_anchors(f.h, None, 2, P(out)) == CP2_ERR_INVALID and L.cp2_fill_anchors(f.h, P(sb), 2, None) == CP2_ERR_INVALID
    assert L.cp2_fill_anchors(f.h, P(np.array([(0, 0), (0, w.nb)], dtype=np.uint64)), 2, P(out)) == CP2_ERR_INVALID and "request 1" in last_error(sctx)
    assert L.cp2_fill_anchors(f.h, P(np.array([(N_SLOTS, 0), (0, 0)], dtype=np.uint64)), 2, P(out)) == CP2_ERR_INVALID and "request 0" in last_error(sctx)
    assert (out == 9).all() and L.cp2_fill_anchors(f.h, None, 0, None) == CP2_OK
    # NULL paths are fine when every level is 0
    assert (w.add_anchored(f, [(0, 0)])[0] == pkg.FILL_NEW).all()
    one = np.array([(0, 1)], dtype=np.uint64)
    assert call(f, sb_=one, data_=w.src.data([(0, 1)]), levels_=np.array([0], dtype=np.uint32), paths_=None, n=1) == CP2_OK
    assert status.tolist() == [pkg.FILL_NEW, 7] and n_new.value == 1
    status[:] = 7
    n_new.value = 5
    # a finished session
    rest = [p for p in w.pairs if p not in [(0, 0), (0, 1)]]
    assert (w.add_anchored(f, rest)[0] == pkg.FILL_NEW).all()
    filled = f.finish()
    assert call(f) == CP2_ERR_INVALID and "finished" in last_error(sctx) and untouched()
    assert L.cp2_fill_anchors(f.h, P(sb), 2, P(out)) == CP2_ERR_INVALID and "finished" in last_error(sctx) and (out == 9).all()
    filled.free()
    f.free()


# ---- 5: twice in one call, and once more ------------------------------------------------------------------------------------------------------------
def test_duplicates(pkg, sctx, worlds):
    w = worlds[8]
    f = w.session(sctx)
    status, n_new, _ = w.add_anchored(f, [(1, 3), (1, 3)])
    assert status.tolist() == [pkg.FILL_NEW, pkg.FILL_DUPLICATE] and n_new == 1
    status, n_new, levels = w.add_anchored(f, [(1, 3), (1, 2)])                          # a present block at level 0: its own kept root
    assert levels.tolist() == [0, 0] and status.tolist() == [pkg.FILL_DUPLICATE, pkg.FILL_NEW] and n_new == 1
    status, n_new, _ = w.add_anchored(f, [(1, 3)], levels=[w.depth])                     # ... and with its whole path
    assert status.tolist() == [pkg.FILL_DUPLICATE] and n_new == 0
    assert f.missing(0)[1] == len(w.pairs) - 2
    f.free()


# ---- 6: a block that proves but cannot be written -----------------------------------------------------------------------------------------------------
def test_an_unwritten_block_stays_missing_and_its_nodes_are_known(pkg, sctx, tmp_path):
    w = World(pkg, sctx, 4, str(tmp_path))
    f = w.session(sctx)
    assert (w.add_anchored(f, [(0, 0), (1, 0)])[0] == pkg.FILL_NEW).all()
    name = "%s%d.dat" % (w.out_base, 1)
    kept = name + ".kept_aside"                                                          # slot 1's file can no longer be written
    os.rename(name, kept)
    if os.geteuid() == 0:
        os.mkdir(name)
    else:
        os.chmod(w.out_dir, stat.S_IRUSR | stat.S_IXUSR)
    pairs = [(0, 1), (1, 2)]
    assert f.anchors([(1, 2), (1, 3)]).tolist() == [1, 1]
    try:
        with pytest.raises(pkg.CodexP2Error) as e:
            w.add_anchored(f, pairs)
    finally:
        if os.geteuid() == 0:
            os.rmdir(name)
        else:
            os.chmod(w.out_dir, stat.S_IRWXU)
        os.rename(kept, name)
    assert e.value.status == CP2_ERR_IO
    assert e.value.fill_status.tolist() == [pkg.FILL_NEW, pkg.FILL_UNWRITTEN] and e.value.n_new == 1
    assert (1, 2) in [tuple(p) for p in f.missing()[0].tolist()]
    assert f.block_proofs([(1, 2)], statuses_only=True).tolist() == [pkg.FILL_PROOF_ABSENT]
    assert f.anchors([(1, 2), (1, 3)]).tolist() == [0, 0]                                 # its nodes are authentic: the neighbour needs no sibling
    status, n_new, levels = w.add_anchored(f, [(1, 2), (1, 3)])                          # sent again, as bare bytes, now written
    assert levels.tolist() == [0, 0] and status.tolist() == [pkg.FILL_NEW, pkg.FILL_NEW] and n_new == 2
    rest = [tuple(p) for p in f.missing()[0].tolist()]
    for p in rest:
        assert w.add_anchored(f, [p])[0].tolist() == [pkg.FILL_NEW]
    w.check_finished(pkg, f)
    for s in range(N_SLOTS):
        assert open("%s%d.dat" % (w.out_base, s), "rb").read() == w.data[s].tobytes()
    f.free()
    w.free()


# ---- 7: served from the moment it is present ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [8, 64])
def test_a_block_added_anchored_is_served_at_once(pkg, sctx, worlds, nb):
    w = worlds[nb]
    f = w.session(sctx)
    for p in w.shuffled(13)[:3 * nb]:
        assert w.add_anchored(f, [p])[0].tolist() == [pkg.FILL_NEW]
        status, roots, paths = f.block_proofs([p])
        i = w.src.index[p]
        assert status.tolist() == [pkg.FILL_PROOF_OK] and roots[0].tobytes() == w.src.roots[i].tobytes() and paths[0].tobytes() == w.src.paths[i].tobytes(), p
    f.free()


# ---- 8: plain adds, a checkpoint, a resume, then anchored ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [8, 64])
def test_resumed_then_completed_with_anchored_adds(pkg, sctx, worlds, tmp_path, nb):
    w = worlds[nb]
    order = w.shuffled(14)
    half, rest = order[:len(order) // 2], order[len(order) // 2:]
    f = w.session(sctx, keep=False)
    for k in range(0, len(half), 9):
        assert (add(f, w.src, half[k:k + 9])[0] == pkg.FILL_NEW).all()
    path = str(tmp_path / "session.ckpt")
    f.save(path)
    f.free()
    f = sctx.fill_resume(w.cfg, w.roots, path, 0, N_SLOTS)
    assert f.n_dropped == 0 and (f.anchors(w.pairs) == w.depth).all()                    # resumed: no nodes kept yet
    f.keep_nodes()
    assert (f.anchors(half) == 0).all()                                                  # what presence gives
    model = A.Session(nb, N_SLOTS)
    for p in half:
        model.add(*p)
    model.keep_nodes()
    assert f.anchors(w.pairs).tolist() == [model.anchor(*p) for p in w.pairs]
    siblings = 0
    for k in range(0, len(rest), 5):
        pairs = rest[k:k + 5]
        status, n_new, levels = w.add_anchored(f, pairs)
        assert (status == pkg.FILL_NEW).all() and n_new == len(pairs)
        siblings += int(levels.sum())
    assert siblings < len(rest) * w.depth
    w.check_finished(pkg, f)
    f.free()


# ---- 9: every level equal to depth is cp2_fill_add ------------------------------------------------------------------------------------------------------
def test_whole_paths_are_cp2_fill_add(pkg, sctx, worlds):
    w = worlds[8]
    order = w.shuffled(15)[:20]
    pairs = order + order[:3] + [(2, 6)]                                                 # repeats, and one that will not prove
    data, paths = w.src.data(pairs), w.src.path(pairs)
    paths[-1] = flip(paths[-1], 40)
    a, b = w.session(sctx), w.session(sctx)
    st_a, new_a = a.add(pairs, data, paths)
    st_b, new_b = b.add_anchored(pairs, data, np.full(len(pairs), w.depth, dtype=np.uint32), paths.reshape(-1, 32))
    assert st_a.tolist() == st_b.tolist() and new_a == new_b == 20
    assert st_a.tolist() == [pkg.FILL_NEW] * 20 + [pkg.FILL_DUPLICATE] * 3 + [pkg.FILL_MISMATCH]
    for x, y in zip(a.block_proofs(w.pairs), b.block_proofs(w.pairs)):
        assert x.tobytes() == y.tobytes()
    assert a.anchors(w.pairs).tolist() == b.anchors(w.pairs).tolist()
    assert a.missing()[0].tolist() == b.missing()[0].tolist()
    a.free()
    b.free()
