"""GPU suite: cp2_fills_add_many -- proved blocks added to many fill sessions in one pass.  The call is defined by the calls that exist, so
the test is twin worlds: six sessions on one context in each (1, 2, 8, 16, 64 and 64 blocks a slot; slot files and the fake source; some
keeping nodes; different local ranges; the last one resumed from a checkpoint before the calls).  World A receives every batch through
cp2_fills_add_many, world B the subsequences through cp2_fill_add / cp2_fill_add_anchored, and after every batch statuses, n_new,
cp2_fill_missing, cp2_fill_anchors of every block, cp2_fill_block_proofs (statuses and bytes) and the slot files must be equal.  The
context has the smallest staging it accepts (1 MiB: chunks of 2048 blocks of 256 bytes), so the large batch spans three chunks.  The small
geometry of the fill tests (cells of 64 bytes, blocks of 256).  Every comparison is bit exact."""
import ctypes
import faulthandler
import os
import stat

import numpy as np
import pytest

from test_gpu_fill import Source, build_compact, flip

pytestmark = pytest.mark.gpu

CP2_OK, CP2_ERR_INVALID, CP2_ERR_IO = 0, -1, -5
N_SLOTS = 4
# blocks a slot, slot files, keeps nodes, first local slot, local slots
SHAPES = [(1, False, False, 0, 4), (2, True, True, 1, 3), (8, False, True, 0, 4), (16, True, False, 2, 2), (64, False, True, 3, 1), (64, True, True, 0, 2)]
RESUMED = 5
CHUNK = 2048                                         # requests a chunk at 1 MiB of staging: (1 MiB / 2) / 256


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def sctx(pkg):
    old = os.environ.get("CODEX_P2_STAGE_MB")
    os.environ["CODEX_P2_STAGE_MB"] = "1"            # read once, when the context is made
    try:
        c = pkg.Context(0)
    finally:
        if old is None:
            del os.environ["CODEX_P2_STAGE_MB"]
        else:
            os.environ["CODEX_P2_STAGE_MB"] = old
    yield c
    c.close()


def last_error(ctx):
    return ctx.L.cp2_last_error(ctx.h).decode()


class Spec:
    """one dataset: its data, the compact dataset built from it and what the peers would send; shared by both worlds"""

    def __init__(self, pkg, ctx, k, directory):
        self.k = k
        self.nb, self.files, self.keep, self.first, self.n_local = SHAPES[k]
        self.kw = dict(maxDepth=8, maxLog2NSlots=2, cellSize=64, blockSize=256, nSlots=N_SLOTS, nCells=4 * self.nb, nSamples=3, seed=900 + k)
        self.pkg, self.data = pkg, None
        if self.files:
            os.makedirs(os.path.join(directory, "src%d" % k))
            base = os.path.join(directory, "src%d" % k, "slot")
            rng = np.random.default_rng([77, k])
            self.data = {s: rng.integers(0, 256, (self.nb, 256), dtype=np.uint8) for s in range(N_SLOTS)}
            for s in range(N_SLOTS):
                self.data[s].tofile("%s%d.dat" % (base, s))
            src_cfg = pkg.make_config(file=base, **self.kw)
        else:
            src_cfg = pkg.make_config(**self.kw)
        self.src_cfg = src_cfg
        self.built = build_compact(ctx, src_cfg, self.first, self.n_local)
        self.roots = self.built.local_roots()
        self.src = Source(ctx, src_cfg, self.built, self.first, self.n_local, blocks_of=(lambda s: self.data[s]) if self.files else None)
        self.pairs = self.src.pairs
        self.depth = self.src.paths.shape[1]
        assert self.depth == max(1, (self.nb - 1).bit_length())

    def cfg_for(self, out_base):
        return self.pkg.make_config(file=out_base, **self.kw) if self.files else self.src_cfg


class World:
    def __init__(self, ctx, specs, directory):
        self.ctx, self.specs, self.dir = ctx, specs, directory
        self.sessions, self.cfgs, self.out_dirs = [], [], []
        for sp in specs:
            out_dir = os.path.join(directory, "out%d" % sp.k)
            os.makedirs(out_dir)
            cfg = sp.cfg_for(os.path.join(out_dir, "slot"))
            f = ctx.fill(cfg, sp.roots, sp.first, sp.n_local)
            if sp.k == RESUMED:                      # a few plain adds, a checkpoint, a resume: before any batch
                some = sp.pairs[3:40:3]
                assert (f.add(some, sp.src.data(some), sp.src.path(some))[0] == 0).all()
                path = os.path.join(directory, "session%d.ckpt" % sp.k)
                f.save(path)
                f.free()
                f = ctx.fill_resume(cfg, sp.roots, path, sp.first, sp.n_local)
                assert f.n_dropped == 0
            if sp.keep:
                f.keep_nodes()
            self.sessions.append(f)
            self.cfgs.append(cfg)
            self.out_dirs.append(out_dir)

    def state(self):
        out = []
        for sp, f, d in zip(self.specs, self.sessions, self.out_dirs):
            miss, n_miss = f.missing()
            one = [miss.tobytes(), n_miss, f.anchors(sp.pairs).tobytes()]
            if sp.keep:
                one += [x.tobytes() for x in f.block_proofs(sp.pairs)]
            if sp.files:
                one.append(sorted((name, open(os.path.join(d, name), "rb").read()) for name in os.listdir(d) if os.path.isfile(os.path.join(d, name))))
            out.append(one)
        return out


@pytest.fixture(scope="module")
def specs(pkg, sctx, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fill_many_src"))
    made = [Spec(pkg, sctx, k, d) for k in range(len(SHAPES))]
    yield made
    for sp in made:
        sp.built.free()


def twins(sctx, specs, tmp_path):
    a, b = World(sctx, specs, str(tmp_path / "A")), World(sctx, specs, str(tmp_path / "B"))
    assert a.state() == b.state()
    return a, b


def free(*worlds):
    for w in worlds:
        for f in w.sessions:
            f.free()


def tables(specs, reqs, levels):
    """req, data, packed paths of a list of (session, slot, block) with the levels given (None: whole paths)"""
    req = np.array(reqs, dtype=np.uint64).reshape(-1, 3)
    data = np.concatenate([specs[k].src.data([(s, b)]) for k, s, b in reqs] + [np.zeros((0, 256), np.uint8)])
    lv = [specs[k].depth for k, _, _ in reqs] if levels is None else levels
    rows = [specs[k].src.paths[specs[k].src.index[(s, b)]][:int(a)] for (k, s, b), a in zip(reqs, lv)]
    return req, data, np.concatenate(rows + [np.zeros((0, 32), np.uint8)])


def lowest(world, reqs):
    return np.array([int(world.sessions[k].anchors([(s, b)])[0]) for k, s, b in reqs], dtype=np.uint32)


def loop(pkg, world, req, data, paths, levels):
    """world B: per session, in `fills` order, the subsequence through the calls that exist; an I/O failure does not stop the loop"""
    n = req.shape[0]
    status, n_new, failed = np.full(n, 77, dtype=np.uint32), [], []
    lv = np.array([world.specs[int(k)].depth for k in req[:, 0]], dtype=np.uint32) if levels is None else np.asarray(levels, dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(lv, dtype=np.int64)])
    for k, (sp, f) in enumerate(zip(world.specs, world.sessions)):
        idx = [i for i in range(n) if int(req[i, 0]) == k]
        if not idx:
            n_new.append(0)
            continue
        sb = req[idx][:, 1:] if idx else np.zeros((0, 2), np.uint64)
        d = data[idx] if idx else np.zeros((0, 256), np.uint8)
        p = np.concatenate([paths[off[i]:off[i + 1]] for i in idx] + [np.zeros((0, 32), np.uint8)])
        try:
            if levels is None or not sp.keep:
                st, new = f.add(sb, d, p.reshape(len(idx), sp.depth, 32))
            else:
                st, new = f.add_anchored(sb, d, lv[idx], p)
        except pkg.CodexP2Error as e:
            assert e.status == CP2_ERR_IO
            st, new = e.fill_status, e.n_new
            failed.append((k, str(e)))
        status[idx] = st
        n_new.append(new)
    return status, n_new, failed


def send(pkg, a, b, reqs, levels=None, damage=None):
    """one batch through both worlds; returns A's (status, n_new).  damage(data, paths): in place, before either world sees them"""
    req, data, paths = tables(a.specs, reqs, levels)
    if damage:
        damage(data, paths)
    st_a, new_a = pkg.fills_add_many(a.ctx, a.sessions, req, data, paths if paths.size or levels is None else None, levels)
    st_b, new_b, failed = loop(pkg, b, req, data, paths, levels)
    assert not failed
    assert st_a.tolist() == st_b.tolist(), (st_a.tolist(), st_b.tolist())
    assert new_a == new_b
    assert a.state() == b.state()
    return st_a, new_a


def everything(specs):
    return [(sp.k, s, b) for sp in specs for s, b in sp.pairs]


def shuffled(specs, seed):
    al = everything(specs)
    return [al[i] for i in np.random.default_rng(seed).permutation(len(al))]


def oracle_slot_root(C, blocks):
    leaves = C.hash_cells(blocks.reshape(-1), 64)
    return C.merkle_root(np.stack([C.merkle_root(leaves[4 * b:4 * b + 4]) for b in range(blocks.shape[0])]))


# ---- 1: a whole life: whole paths, lowest anchors, NEW / DUPLICATE / MISMATCH, n == 0, the finished datasets ------------------------------------
def test_batches_leave_both_worlds_equal_and_finish_as_the_built_datasets(pkg, oracle, sctx, specs, tmp_path):
    C, _ = oracle
    N, X, D = pkg.FILL_NEW, pkg.FILL_MISMATCH, pkg.FILL_DUPLICATE
    a, b = twins(sctx, specs, tmp_path)
    order = shuffled(specs, 1)
    third = len(order) // 3
    # whole paths only, levels == NULL: every session takes them, keeping nodes or not
    st, new = send(pkg, a, b, order[:third])
    present = {(5, s, bb) for s, bb in specs[RESUMED].pairs[3:40:3]}
    assert st.tolist() == [D if r in present else N for r in order[:third]] and sum(new) == st.tolist().count(N)
    assert len({k for k, _, _ in order[:third]}) == len(SHAPES)
    # n == 0
    st, new = pkg.fills_add_many(sctx, a.sessions, np.zeros((0, 3), np.uint64), np.zeros(0, np.uint8), None)
    assert st.size == 0 and new == [0] * len(SHAPES) and a.state() == b.state()
    # NEW, DUPLICATE and MISMATCH of one block with other sessions' requests between them; the MISMATCH comes first and decides nothing
    fresh = [r for r in order[third:] if r[0] == 2][:1] + [r for r in order[third:] if r[0] == 4][:2] + [r for r in order[third:] if r[0] == 0][:1]
    one = fresh[0]
    batch = [one, fresh[1], one, fresh[2], fresh[3], one]

    def first_wrong(data, paths):
        data[0] = flip(data[0], 5)
    st, new = send(pkg, a, b, batch, damage=first_wrong)
    assert st.tolist() == [X, N, N, N, N, D] and new == [1, 0, 1, 0, 2, 0]
    # lowest anchors, in a shuffled order: sessions that keep no nodes answer their depth and take whole paths
    rest = [r for r in order[third:] if r not in fresh]
    half = len(rest) // 2
    lv = lowest(a, rest[:half])
    assert lv.tolist() == lowest(b, rest[:half]).tolist() and len(set(lv.tolist())) >= 3
    st, new = send(pkg, a, b, rest[:half], levels=lv)
    assert st.tolist() == [D if r in present else N for r in rest[:half]]
    # a wrong sibling and a wrong block among the last ones leave nothing; sent again right they are NEW
    last = rest[half:]
    lv = lowest(a, last)
    hit = [i for i, x in enumerate(lv) if x > 0][:2]
    off = np.concatenate([[0], np.cumsum(lv, dtype=np.int64)])

    def two_wrong(data, paths):
        paths[off[hit[0]]] = flip(paths[off[hit[0]]], 9)
        data[hit[1]] = flip(data[hit[1]], 200)
    st, new = send(pkg, a, b, last, levels=lv, damage=two_wrong)
    assert st.tolist() == [X if i in hit else D if r in present else N for i, r in enumerate(last)]
    again = [last[i] for i in hit]
    st, new = send(pkg, a, b, again, levels=lowest(a, again))
    assert (st == N).all()
    # every session is complete: finished, each dataset's roots are the built dataset's and the oracle's
    for w in (a, b):
        for sp, f in zip(specs, w.sessions):
            assert f.missing(0)[1] == 0
            filled = f.finish()
            assert filled.local_roots().tobytes() == sp.roots.tobytes()
            got_roots, got_paths = filled.block_proofs(sp.pairs)
            assert got_roots.tobytes() == sp.src.roots.tobytes() and got_paths.tobytes() == sp.src.paths.tobytes()
            filled.free()
    for sp in specs:
        for i in range(sp.n_local):
            slot = sp.first + i
            want = (oracle_slot_root(C, sp.data[slot]) if sp.files else
                    C.fake_slot_root(C.slot_seed(sp.kw["seed"], slot), 64, 256, 4 * sp.nb, 8))
            assert sp.roots[i].tobytes() == want.tobytes(), (sp.k, slot)
        if sp.files:
            for w in (a, b):
                for slot in range(sp.first, sp.first + sp.n_local):
                    assert open(os.path.join(w.out_dirs[sp.k], "slot%d.dat" % slot), "rb").read() == sp.data[slot].tobytes()
    free(a, b)


# ---- 2: three chunks of the data path ---------------------------------------------------------------------------------------------------------
def test_a_batch_of_three_chunks_with_a_session_and_a_path_range_across_the_edges(pkg, sctx, specs, tmp_path):
    N, X, D = pkg.FILL_NEW, pkg.FILL_MISMATCH, pkg.FILL_DUPLICATE
    a, b = twins(sctx, specs, tmp_path)
    order = shuffled(specs, 2)
    send(pkg, a, b, order[:200], levels=lowest(a, order[:200]))       # something is known, so the anchors differ
    rng = np.random.default_rng(3)
    reqs = [order[i] for i in rng.integers(0, len(order), 2 * CHUNK + 300)]
    deep = [r for r in order if r[0] == 4]                            # one session's requests on both sides of both chunk edges
    for edge in (CHUNK, 2 * CHUNK):
        reqs[edge - 2:edge + 2] = [deep[edge % 7], deep[edge % 11 + 1], deep[edge % 5 + 2], deep[edge % 3 + 3]]
    low = lowest(a, reqs)
    depth = np.array([specs[k].depth for k, _, _ in reqs], dtype=np.uint32)
    lv = np.where((rng.random(len(reqs)) < 0.5) | (low == depth), depth, low).astype(np.uint32)   # any known level may be stated
    for edge in (CHUNK, 2 * CHUNK):
        lv[edge - 2:edge + 2] = depth[edge - 2:edge + 2]
    off = np.concatenate([[0], np.cumsum(lv, dtype=np.int64)])
    assert len(reqs) > 2 * CHUNK and all(reqs[e - 1][0] == reqs[e][0] == 4 for e in (CHUNK, 2 * CHUNK))
    assert all(0 < off[e] - off[e - 1] and 0 < off[e + 1] - off[e] for e in (CHUNK, 2 * CHUNK)) and len(set(lv.tolist())) >= 4
    wrong = [CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK + 1, 17]

    def damage(data, paths):
        for i in wrong[:2]:
            data[i] = flip(data[i], 100)
        for i in wrong[2:4]:
            paths[off[i]] = flip(paths[off[i]], 3)
        data[wrong[4]] = flip(data[wrong[4]], 0)
    st, new = send(pkg, a, b, reqs, levels=lv, damage=damage)
    assert all(st[i] == X for i in wrong) and set(st.tolist()) == {N, X, D}
    assert sum(new) == st.tolist().count(N)
    # the same again with whole paths throughout: levels == NULL over three chunks
    st, new = send(pkg, a, b, reqs)
    assert sum(new) == st.tolist().count(N) and X not in st.tolist()
    free(a, b)


# ---- 3: a slot file that cannot be written ---------------------------------------------------------------------------------------------------------
def test_a_session_whose_file_cannot_be_written_leaves_the_others_alone(pkg, sctx, specs, tmp_path):
    N, U = pkg.FILL_NEW, pkg.FILL_UNWRITTEN
    a, b = twins(sctx, specs, tmp_path)
    stuck = (1, 3)                                                    # two file sessions fail; the first in `fills` order is named
    reqs = [(0, 0, 0), (1, 1, 0), (5, 0, 7), (3, 2, 5), (1, 2, 1), (2, 1, 3), (3, 3, 0), (5, 1, 9), (4, 3, 60), (1, 1, 1)]
    undo = []
    for w in (a, b):
        for k in stuck:
            d = w.out_dirs[k]
            if os.geteuid() == 0:                                     # (nothing is written there yet: the names are taken by directories)
                for s in range(N_SLOTS):
                    os.mkdir(os.path.join(d, "slot%d.dat" % s))
                    undo.append(lambda p=os.path.join(d, "slot%d.dat" % s): os.rmdir(p))
            else:
                os.chmod(d, stat.S_IRUSR | stat.S_IXUSR)
                undo.append(lambda p=d: os.chmod(p, stat.S_IRWXU))
    req, data, paths = tables(specs, reqs, None)
    try:
        with pytest.raises(pkg.CodexP2Error) as e:
            pkg.fills_add_many(sctx, a.sessions, req, data, paths)
        st_b, new_b, failed = loop(pkg, b, req, data, paths, None)
    finally:
        for u in undo:
            u()
    assert e.value.status == CP2_ERR_IO
    want = [U if k in stuck else N for k, _, _ in reqs]
    assert e.value.fill_status.tolist() == want == st_b.tolist()
    assert e.value.n_new == new_b == [1, 0, 1, 0, 1, 2]
    assert [k for k, _ in failed] == list(stuck)
    assert os.path.join(a.out_dirs[1], "slot1.dat") in str(e.value) and "out3" not in str(e.value)
    assert a.state() == b.state()
    for k, s, bb in reqs:                                             # the others' blocks are present, the stuck sessions' still missing
        assert ([s, bb] in a.sessions[k].missing()[0].tolist()) == (k in stuck)
    assert a.sessions[1].anchors([(1, 0), (1, 1)]).tolist() == [0, 0]  # proved all the same: its nodes are known
    st, new = send(pkg, a, b, [r for r in reqs if r[0] in stuck])      # sent again, now written
    assert (st == N).all()
    free(a, b)


# ---- 4: refusals: all or nothing ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_changes_nothing(pkg, sctx, specs, tmp_path):
    a, b = twins(sctx, specs, tmp_path)
    L, P = pkg.load_library(), pkg._p
    order = shuffled(specs, 4)
    send(pkg, a, b, order[:150], levels=lowest(a, order[:150]))
    before = a.state()
    k8, k16 = 2, 3                                                    # a session that keeps nodes, one that keeps none
    pick = lambda k: [r for r in order[150:] if r[0] == k and (not specs[k].keep or lowest(a, [r])[0] > 0)][0]   # noqa: E731
    reqs = [pick(0), pick(k8), pick(k16), pick(4)]                   # absent blocks of sessions 0, 2, 3 and 4
    lv = np.array([specs[r[0]].depth for r in reqs], dtype=np.uint32)
    req, data, paths = tables(specs, reqs, lv)
    hs = (ctypes.c_void_p * len(a.sessions))(*[f.h for f in a.sessions])
    status = np.full(len(reqs), 7, dtype=np.uint32)
    n_new = (ctypes.c_size_t * len(a.sessions))(*([5] * len(a.sessions)))

    def call(ctx_=sctx.h, hs_=hs, nf=len(a.sessions), req_=req, data_=data, lv_=lv, paths_=paths, n=len(reqs), status_=status):
        opt = lambda x: P(x) if x is not None else None      # noqa: E731
        return L.cp2_fills_add_many(ctx_, hs_, nf, opt(req_), opt(data_), opt(lv_), opt(paths_), n, opt(status_), n_new)

    def refused(where=None, **kw):
        assert call(**kw) == CP2_ERR_INVALID, kw
        if where:
            assert where in last_error(sctx), (where, last_error(sctx))
        assert (status == 7).all() and list(n_new) == [5] * len(a.sessions)
        assert a.state() == before

    def with_req(i, col, v):
        r = req.copy()
        r[i, col] = v
        return r

    def with_lv(i, v):
        x = lv.copy()
        x[i] = v
        return x

    assert call(ctx_=None) == CP2_ERR_INVALID and (status == 7).all()
    refused(hs_=None)
    refused(req_=None)
    refused(data_=None)
    refused(status_=None)
    other = pkg.Context(0)
    stranger = other.fill(specs[0].src_cfg, specs[0].roots, 0, 4)
    bigger = sctx.fill(pkg.make_config(**dict(specs[0].kw, cellSize=128, blockSize=512, nCells=8)), specs[0].roots, 0, 4)
    wider = sctx.fill(pkg.make_config(**dict(specs[0].kw, blockSize=512, nCells=8)), specs[0].roots, 0, 4)
    done = sctx.fill(specs[0].src_cfg, specs[0].roots, 0, 4)
    assert (done.add(specs[0].pairs, specs[0].src.data(specs[0].pairs), specs[0].src.path(specs[0].pairs))[0] == 0).all()
    filled = done.finish()
    for h, what in ((None, "fills[5] is NULL"), (stranger.h, "fills[5] belongs to another context"), (bigger.h, "fills[5] has another cell_size"),
                    (wider.h, "fills[5] has another block_size"), (done.h, "fills[5]"), (a.sessions[1].h, "fills[5] is listed twice")):
        x = (ctypes.c_void_p * len(a.sessions))(*[f.h for f in a.sessions])
        x[5] = h
        refused(what, hs_=x)
        assert h != done.h or "finished" in last_error(sctx)
    refused("request 2", req_=with_req(2, 0, len(a.sessions)))         # a session index >= n_fills
    refused("request 0", nf=0)
    refused("request 3", req_=with_req(3, 1, 2))                       # a slot outside ITS session's local range (another's holds it)
    refused("request 0", req_=with_req(0, 2, 1))                       # a block >= ITS session's nBlocks
    refused("request 1", lv_=with_lv(1, specs[k8].depth + 1))          # a level above ITS session's depth (another's is deeper)
    refused("request 1", lv_=with_lv(1, 0))                            # an anchor that is not known when the call starts
    refused("request 2", lv_=with_lv(2, specs[k16].depth - 1))         # a short path into a session that keeps no nodes
    assert "cp2_fill_keep_nodes" in last_error(sctx)
    refused("request 0", paths_=None)                                  # NULL paths while a level is not 0
    refused("request 0", lv_=None, paths_=None)
    # NULL paths are fine when every level is 0, n == 0 zeroes n_new, and the call as it stands is accepted
    known = [r for r in order[:150] if r[0] in (1, 2, 4, 5)][:3]
    r0, d0, _ = tables(specs, known, [0, 0, 0])
    st0 = np.full(3, 7, dtype=np.uint32)
    assert call(req_=r0, data_=d0, lv_=np.zeros(3, np.uint32), paths_=None, n=3, status_=st0) == CP2_OK
    assert st0.tolist() == [pkg.FILL_DUPLICATE] * 3 and list(n_new) == [0] * len(a.sessions) and a.state() == before
    n_new[2] = 5
    assert call(hs_=hs, req_=None, data_=None, lv_=None, paths_=None, n=0, status_=None) == CP2_OK and list(n_new) == [0] * len(a.sessions)
    assert call() == CP2_OK and status.tolist() == [pkg.FILL_NEW] * 4 and list(n_new) == [1, 0, 1, 1, 1, 0]
    for h in (filled, done, wider, bigger, stranger):
        h.free()
    other.close()
    free(a, b)
