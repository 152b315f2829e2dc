"""GPU suite: k_block_path_commit_many through its launcher alone (tests/device_check/libfill_many_unit.so, a forwarder linked against the
product).  Five session buffers stand in ONE allocation with guard rows before, between and behind, pre-filled with a non-zero pattern;
the trees are the C oracle's, and authentic nodes stand exactly in the rows the case calls known.  Two plans cover n_blocks 1, 2, 3, 5, 8
and 64 (odd sizes too: the launcher takes them, so the odd-last key rule is walked per lane); in each, two sessions keep no nodes and two
are built over the SAME trees with different known rows, one root stated as root + r.

ONE launch holds every (session, slot, block, level) the host would admit -- level = depth, or a level whose anchor row is known -- in a
seeded shuffled order, so every wave mixes sessions, depths, levels and keeping with non-keeping; each as a true request, with a bit flipped
in the fresh root, and with a bit flipped in one sibling below the level; every fourth true request hands a sibling in as value + r.  The
second twin also gets the requests whose anchor is known in the first twin only (pairs whose anchor a matching request of the launch stores
are left out: the host never lets them in): they must MISMATCH.  A second launch holds the defensive cases.  Compared: the WHOLE
allocation, every verdict word, the scratch guards; and the same inputs cut by session through launch_block_path_commit_anchored and, for
whole paths with keep_top, launch_block_path_commit_nodes give the same verdicts and rows.  Every comparison is bit exact."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import fill_anchor_models as A
import fill_nodes_models as M
import kernel_models as K
from test_gpu_kernel_units import Out, as_int, canonical_rows, flip, up

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "device_check")
LIBS = [os.path.join(DIR, n) for n in ("libfill_many_unit.so", "libfill_anchor_unit.so", "libfill_nodes_unit.so")]
NO_ROW = (1 << 64) - 1
GUARD = 8                                            # rows between two session buffers
N_LOCAL = 2
# (n_blocks, keeps nodes, twin): twin 'a' knows every row below the top, twin 'b' a seeded part and states slot 0's root as root + r
PLANS = {"8-8-64-5-1": [(8, True, "a"), (8, True, "b"), (64, True, None), (5, False, None), (1, False, None)],
         "3-3-2-1-64": [(3, True, "a"), (3, True, "b"), (2, False, None), (1, True, None), (64, False, None)]}


@pytest.fixture(scope="module")
def libs(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    for path in LIBS:                                # a missing check library is built, never worked around
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/" + os.path.basename(path)],
                                  stdout=subprocess.DEVNULL)
    vp, sz, u64, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    fmu, fau, fnu = (ctypes.CDLL(p) for p in LIBS)
    fmu.fmu_block_path_commit_many.restype = i32
    fmu.fmu_block_path_commit_many.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, i32, sz, vp, vp]
    fau.fau_block_path_commit_anchored.restype = i32
    fau.fau_block_path_commit_anchored.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64, vp]
    fnu.fnu_block_path_commit_nodes.restype, fnu.fnu_block_path_commit_nodes.argtypes = i32, [vp, vp, vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64, vp]
    return fmu, fau, fnu


def reduced(row):
    return np.frombuffer((as_int(row) % K.R_MOD).to_bytes(32, "little"), dtype=np.uint8)


def plus_r(row):
    return np.frombuffer((as_int(row) + K.R_MOD).to_bytes(32, "little"), dtype=np.uint8)          # below 2^256: the value is below r


class Sess:
    def __init__(self, k, nb, keeps, trees, known, roots):
        self.k, self.nb, self.keeps, self.trees, self.known, self.roots = k, nb, keeps, trees, known, roots
        self.sizes, self.offs, self.n_rows = M.layout(nb, N_LOCAL)
        self.depth = len(self.sizes) - 1

    def row(self, lvl, s, idx):
        return M.node_row(self.nb, N_LOCAL, lvl, s, idx)

    def node_of(self, r):
        for s in range(N_LOCAL):
            for lvl in range(self.depth + 1):
                base = self.offs[lvl] + s * self.sizes[lvl]
                if base <= r < base + self.sizes[lvl]:
                    return self.trees[s][lvl][r - base]
        raise AssertionError(r)

    def true_path(self, s, b, level):
        p = np.zeros((level, 32), np.uint8)
        for lvl in range(level):
            if ((b >> lvl) ^ 1) < len(self.trees[s][lvl]):
                p[lvl] = self.trees[s][lvl][(b >> lvl) ^ 1]
        return p


class Req:
    def __init__(self, sess, slot, block, level, fresh, path, label):
        self.k, self.slot, self.block, self.level, self.fresh, self.path, self.label = sess.k, slot, block, level, fresh, path, label


class Plan:
    def __init__(self, C, name):
        rng = np.random.default_rng([0xF1A, sorted(PLANS).index(name)])
        self.C, self.sessions, twin_trees = C, [], None
        for k, (nb, keeps, twin) in enumerate(PLANS[name]):
            if twin == "b":
                trees = twin_trees
            else:
                trees = [C.merkle_tree(canonical_rows(rng, nb)) for _ in range(N_LOCAL)]
            if twin == "a":
                twin_trees = trees
            sizes, _, _ = M.layout(nb, N_LOCAL)
            depth = len(sizes) - 1
            assert [len(x) for x in trees[0]] == sizes and depth == A.depth_of(nb)
            below = [M.node_row(nb, N_LOCAL, lvl, s, i) for s in range(N_LOCAL) for lvl in range(depth) for i in range(sizes[lvl])]
            known = set() if not keeps else set(below) if twin == "a" else {r for r in below if rng.random() < 0.4}
            roots = np.stack([t[-1][0] for t in trees])
            if twin == "b":
                roots[0] = plus_r(roots[0])
                known.discard(M.node_row(nb, N_LOCAL, depth - 1, 1, 0))               # for certain unknown here and known in twin 'a'
            self.sessions.append(Sess(k, nb, keeps, trees, known, roots))
        self.reqs, self.lifted, self.borrowed, self.left_out = [], 0, 0, 0
        count = 0
        for q in self.sessions:
            triples = [(s, b, lvl) for s in range(N_LOCAL) for b in range(q.nb) for lvl in range(q.depth + 1)
                       if lvl == q.depth or (q.keeps and q.row(lvl, s, b >> lvl) in q.known)]
            if q.k == 1:                                                             # the second twin's slot 1 gets no whole path: a whole path stores
                triples = [t for t in triples if not (t[0] == 1 and t[2] == q.depth)]   # every row, and no anchor there would stay unknown
            for s, b, lvl in triples:
                leaf = q.trees[s][0][b]
                true = Req(q, s, b, lvl, leaf.copy(), q.true_path(s, b, lvl), "session %d slot %d block %d level %d true" % (q.k, s, b, lvl))
                in_range = [low for low in range(lvl) if ((b >> low) ^ 1) < q.sizes[low]]
                if count % 4 == 0 and in_range:                                       # the same value, handed in as value + r
                    low = in_range[count % len(in_range)]
                    true.path[low] = plus_r(true.path[low])
                    true.label += ", sibling %d + r" % low
                    self.lifted += 1
                count += 1
                self.reqs.append(true)
                fresh = leaf.copy().reshape(1, 32)
                flip(fresh, 0, (b * 11 + lvl * 3 + 5) % 248)
                self.reqs.append(Req(q, s, b, lvl, fresh[0], q.true_path(s, b, lvl), "session %d slot %d block %d level %d fresh flipped" % (q.k, s, b, lvl)))
                if lvl:
                    path = q.true_path(s, b, lvl)
                    low = (b + lvl) % lvl
                    flip(path, low, (b * 7 + lvl * 13) % 248)
                    self.reqs.append(Req(q, s, b, lvl, leaf.copy(), path, "session %d slot %d block %d level %d sibling %d flipped" % (q.k, s, b, lvl, low)))
        # the second twin: true paths to anchors only the first twin knows
        ta, tb = self.sessions[0], self.sessions[1]
        stored = set()
        for r in self.reqs:
            if r.k == tb.k and "true" in r.label:
                stored |= set(A.stored_rows(tb.nb, N_LOCAL, r.slot, r.block, r.level))
        for s in range(N_LOCAL):
            for b in range(tb.nb):
                for lvl in range(tb.depth):
                    anchor = tb.row(lvl, s, b >> lvl)
                    if anchor in tb.known:
                        continue
                    if anchor in stored:
                        self.left_out += 1
                        continue
                    assert anchor in ta.known
                    self.borrowed += 1
                    self.reqs.append(Req(tb, s, b, lvl, tb.trees[s][0][b].copy(), tb.true_path(s, b, lvl),
                                         "session %d slot %d block %d level %d true, anchor known in the twin only" % (tb.k, s, b, lvl)))
        order = rng.permutation(len(self.reqs))
        self.reqs = [self.reqs[i] for i in order]
        self.want = np.array([self.verdict(r) for r in self.reqs], dtype=np.uint32)
        # the layout of the one allocation: guard rows, session 0, guard rows, session 1, ... guard rows
        self.base, at = [], GUARD
        for q in self.sessions:
            self.base.append(at)
            at += q.n_rows + GUARD
        self.pool_rows = at

    def verdict(self, r):
        q = self.sessions[r.k]
        reached = reduced(A.walk(r.fresh, r.block, q.nb, list(r.path), self.C.compress))
        if r.level == q.depth:
            return 0 if np.array_equal(reached, q.trees[r.slot][-1][0]) else 1
        anchor = q.row(r.level, r.slot, r.block >> r.level)
        return 0 if q.keeps and anchor in q.known and np.array_equal(reached, q.trees[r.slot][r.level][r.block >> r.level]) else 1

    def start_rows(self, pattern_rows):
        rows = pattern_rows.copy()
        for q, base in zip(self.sessions, self.base):
            for r in q.known:
                rows[base + r] = q.node_of(r)
        return rows

    def stored(self, r, keep_top=False):
        """the rows of its session's buffer a matching request stores, with their values"""
        q = self.sessions[r.k]
        if r.level == 0:
            return []
        if not q.keeps:
            return [(q.row(0, r.slot, r.block), q.trees[r.slot][0][r.block])]
        nodes = M.stored_nodes(q.nb, r.block) if keep_top and r.level == q.depth else A.stored_nodes(q.nb, r.block, r.level)
        return [(q.row(lvl, r.slot, idx), q.trees[r.slot][lvl][idx]) for lvl, idx, _ in nodes]


@pytest.fixture(scope="module")
def plans(oracle):
    C, _ = oracle
    return {name: Plan(C, name) for name in PLANS}


def device_tables(torch, p, reqs, pool_ptr, base_off):
    """what the launcher reads: (kept-alive tensors, argument pointers, total path rows, path offsets)"""
    keep = []

    def dev(a):
        t = up(torch, a)
        keep.append(t)
        return t.data_ptr()
    table = np.zeros((len(p.sessions), 7), dtype=np.uint64)
    for q, base in zip(p.sessions, p.base):
        tab = dev(np.array(list(q.offs) + list(q.sizes), dtype=np.uint64)) if q.keeps else 0
        table[q.k] = [pool_ptr + 32 * base, q.n_rows, dev(q.roots), N_LOCAL, tab, q.nb, q.depth]
    levels = np.array([r.level for r in reqs], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(levels, dtype=np.uint64)]).astype(np.uint64)
    total = int(off[-1])
    paths = np.concatenate([r.path for r in reqs] + [np.zeros((1, 32), np.uint8)])
    args = dict(fresh=dev(np.stack([r.fresh for r in reqs])), paths=dev(paths), table=dev(table),
                sess=dev(np.array([r.k for r in reqs], dtype=np.uint64)), levels=dev(levels), off=dev((off[:-1] + np.uint64(base_off)).astype(np.uint64)),
                pairs=dev(np.array([(r.slot, r.block) for r in reqs], dtype=np.uint64)),
                dest=dev(np.array([p.sessions[r.k].row(0, r.slot, r.block) for r in reqs], dtype=np.uint64)),
                anchor=dev(np.array([NO_ROW if r.level == p.sessions[r.k].depth else p.sessions[r.k].row(r.level, r.slot, r.block >> r.level)
                                     for r in reqs], dtype=np.uint64)))
    return keep, args, total, off


def launch(fmu, p, a, base_off, keep_top, n, verdict, scratch):
    return fmu.fmu_block_path_commit_many(a["fresh"], a["paths"], a["table"], len(p.sessions), a["sess"], a["levels"], a["off"], base_off, a["pairs"],
                                          a["dest"], a["anchor"], keep_top, n, verdict.ptr, scratch.ptr)


@pytest.mark.parametrize("name", list(PLANS))
def test_one_launch_over_five_sessions_stores_exactly_what_each_session_proves(libs, plans, capsys, name):
    import torch
    fmu, fau, _ = libs
    t0, bad, p = time.time(), [], plans[name]
    reqs, want, n = p.reqs, p.want, len(p.reqs)
    assert n > 256 and p.lifted > 0 and p.borrowed > 0 and (want == 0).sum() > 0 and (want == 1).sum() > 0
    first_wave = reqs[:64]
    assert len({r.k for r in first_wave}) >= 3 and len({r.level for r in first_wave}) >= 3 and len({p.sessions[r.k].keeps for r in first_wave}) == 2
    assert len({p.sessions[r.k].depth for r in first_wave}) >= 2
    pool = Out(torch, p.pool_rows * 32)
    pattern = pool.prefill().copy().reshape(p.pool_rows, 32)
    start = p.start_rows(pattern)
    pool.t[pool.lo:pool.lo + pool.n] = torch.from_numpy(start.reshape(-1).copy()).cuda()
    base_off = 5 * n                                                                  # path_off as a later chunk of a call would see it
    keep, a, total, off = device_tables(torch, p, reqs, pool.ptr, base_off)
    verdict, scratch = Out(torch, n * 4), Out(torch, total * 64)
    want_rows = start.copy()
    for r, v in zip(reqs, want):
        if v == 0:
            for row, value in p.stored(r):
                want_rows[p.base[r.k] + row] = value
    status = launch(fmu, p, a, base_off, 0, n, verdict, scratch)
    assert status == 0, status
    verdict.check(want, name + " verdicts", bad, 4, lambda i: " (%s)" % reqs[i].label)
    got = pool.check(want_rows, name + " buffers", bad, 32, lambda r: " (row %d of the allocation; bases %s)" % (r, p.base)).reshape(p.pool_rows, 32).copy()
    scratch.fetch()
    if not scratch.guards_ok():
        bad.append("%s: bytes around the scratch changed" % name)
    # a request that is authentic for the first twin and unknown in the second matches only in the former
    ta, tb = p.sessions[0], p.sessions[1]
    for i, r in enumerate(reqs):
        if "in the twin only" in r.label:
            assert want[i] == 1 and ta.row(r.level, r.slot, r.block >> r.level) in ta.known
    # the same inputs, cut by session, through the launcher of cp2_fill_add_anchored: the same verdicts and rows
    for q in p.sessions:
        if not q.keeps:
            continue
        idx = [i for i, r in enumerate(reqs) if r.k == q.k]
        sub = [reqs[i] for i in idx]
        lv = np.array([r.level for r in sub], dtype=np.uint32)
        o = np.concatenate([[0], np.cumsum(lv, dtype=np.uint64)]).astype(np.uint64)
        d = [up(torch, x) for x in (np.stack([r.fresh for r in sub]), np.concatenate([r.path for r in sub] + [np.zeros((1, 32), np.uint8)]), lv, o[:-1].copy(),
                                    np.array([(r.slot, r.block) for r in sub], dtype=np.uint64), q.roots,
                                    np.array([q.row(0, r.slot, r.block) for r in sub], dtype=np.uint64),
                                    np.array([NO_ROW if r.level == q.depth else q.row(r.level, r.slot, r.block >> r.level) for r in sub], dtype=np.uint64),
                                    np.array(q.offs, dtype=np.uint64), np.array(q.sizes, dtype=np.uint64))]
        v1, tree1, s1 = Out(torch, len(sub) * 4), Out(torch, q.n_rows * 32), Out(torch, int(o[-1]) * 64)
        tree1.t[tree1.lo:tree1.lo + tree1.n] = torch.from_numpy(start[p.base[q.k]:p.base[q.k] + q.n_rows].reshape(-1).copy()).cuda()
        st = fau.fau_block_path_commit_anchored(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 0, d[4].data_ptr(), d[5].data_ptr(),
                                                d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), d[9].data_ptr(), q.nb, q.depth, len(sub), v1.ptr,
                                                tree1.ptr, q.n_rows, s1.ptr)
        assert st == 0
        v1.check(want[idx], "%s session %d verdicts of the anchored launcher" % (name, q.k), bad, 4)
        tree1.check(got[p.base[q.k]:p.base[q.k] + q.n_rows], "%s session %d rows of the anchored launcher" % (name, q.k), bad, 32)
    with capsys.disabled():
        print("\n[fill many unit] %s: %d requests in one launch over %d sessions (%d match), %d siblings handed in as value + r, %d anchored on a row "
              "known in the twin only, %d racy pairs left out, %d failed, %.1f s" % (name, n, len(p.sessions), int((want == 0).sum()), p.lifted,
                                                                                      p.borrowed, p.left_out, len(bad), time.time() - t0))
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:100]))


@pytest.mark.parametrize("name", list(PLANS))
def test_whole_paths_with_keep_top_leave_what_commit_nodes_leaves(libs, plans, name):
    """every block's whole path, true and with the fresh root flipped, from all-pattern buffers, keep_top set: a keeping session gets all
    2 x depth + 1 nodes, the slot root's row among them, exactly as k_block_path_commit_nodes stores them; a plain one its block roots"""
    import torch
    fmu, _, fnu = libs
    bad, p = [], plans[name]
    reqs = [r for r in p.reqs if r.level == p.sessions[r.k].depth and ("fresh flipped" in r.label or " true" in r.label)]
    n = len(reqs)
    want = np.array([p.verdict(r) for r in reqs], dtype=np.uint32)
    assert n > 64 and (want == 0).sum() * 2 == n
    pool = Out(torch, p.pool_rows * 32)
    pattern = pool.prefill().copy().reshape(p.pool_rows, 32)
    keep, a, total, off = device_tables(torch, p, reqs, pool.ptr, 0)
    verdict, scratch = Out(torch, n * 4), Out(torch, total * 64)
    want_rows = pattern.copy()
    for r, v in zip(reqs, want):
        if v == 0:
            for row, value in p.stored(r, keep_top=True):
                want_rows[p.base[r.k] + row] = value
    assert launch(fmu, p, a, 0, 1, n, verdict, scratch) == 0
    verdict.check(want, name + " verdicts", bad, 4, lambda i: " (%s)" % reqs[i].label)
    got = pool.check(want_rows, name + " buffers", bad, 32).reshape(p.pool_rows, 32).copy()
    for q in p.sessions:
        t = p.base[q.k] + q.row(q.depth, 0, 0)                            # slot 0's root row: stored where nodes are kept, else untouched
        assert np.array_equal(got[t], q.trees[0][-1][0] if q.keeps else pattern[t]), q.k
        if not q.keeps:
            continue
        sub = [r for r in reqs if r.k == q.k]
        d = [up(torch, x) for x in (np.stack([r.fresh for r in sub]), np.concatenate([r.path for r in sub]),
                                    np.array([(r.slot, r.block) for r in sub], dtype=np.uint64), q.roots,
                                    np.array([q.row(0, r.slot, r.block) for r in sub], dtype=np.uint64), np.array(q.offs, dtype=np.uint64),
                                    np.array(q.sizes, dtype=np.uint64))]
        v1, tree1, s1 = Out(torch, len(sub) * 4), Out(torch, q.n_rows * 32), Out(torch, len(sub) * q.depth * 64)
        assert fnu.fnu_block_path_commit_nodes(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                                               d[6].data_ptr(), q.nb, q.depth, len(sub), v1.ptr, tree1.ptr, q.n_rows, s1.ptr) == 0
        v1.check(want[[i for i, r in enumerate(reqs) if r.k == q.k]], "%s session %d verdicts of k_block_path_commit_nodes" % (name, q.k), bad, 4)
        mine, theirs = got[p.base[q.k]:p.base[q.k] + q.n_rows], tree1.prefill().copy().reshape(q.n_rows, 32)
        written = (mine != pattern[p.base[q.k]:p.base[q.k] + q.n_rows]).any(axis=1)      # (the pattern differs from place to place)
        theirs[written] = mine[written]
        tree1.check(theirs, "%s session %d rows of k_block_path_commit_nodes" % (name, q.k), bad, 32)
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:100]))


def test_defensive_mismatches_write_their_verdict_word_and_nothing_else(libs, plans):
    """a session index at the table's length, a level above the session's depth, a level below it in a session that keeps no nodes, a slot at
    n_local, a dest row at n_rows, an anchor row at n_rows: each true otherwise; between them one good request, which is the only one to store"""
    import torch
    fmu, _, _ = libs
    bad, p = [], plans["8-8-64-5-1"]
    keeping, plain = p.sessions[2], p.sessions[3]
    good = [r for r, v in zip(p.reqs, p.want) if v == 0 and r.k == keeping.k and r.level == keeping.depth and "+ r" not in r.label][:7]
    plain_true = [r for r, v in zip(p.reqs, p.want) if v == 0 and r.k == plain.k][0]
    reqs = good[:3] + [plain_true] + good[3:]
    n = len(reqs)
    pool = Out(torch, p.pool_rows * 32)
    pattern = pool.prefill().copy().reshape(p.pool_rows, 32)
    keep, a, total, off = device_tables(torch, p, reqs, pool.ptr, 0)

    def poke(name, i, dtype, value, col=None):
        arr = keep[[k for k, t in enumerate(keep) if t.data_ptr() == a[name]][0]]
        host = arr.cpu().numpy().view(dtype).copy()
        if col is None:
            host[i] = value
        else:
            host.reshape(-1, 2)[i, col] = value
        arr.copy_(torch.from_numpy(host.view(np.uint8)))
    poke("sess", 0, np.uint64, len(p.sessions))                      # 0: a session index at the table's length
    poke("levels", 1, np.uint32, keeping.depth + 1)                  # 1: a level above the session's depth
    poke("levels", 3, np.uint32, plain.depth - 1)                    # 3: a level below depth in a session that keeps no nodes
    poke("pairs", 4, np.uint64, N_LOCAL, col=0)                      # 4: a slot at n_local
    poke("dest", 5, np.uint64, keeping.n_rows)                       # 5: a dest row at n_rows
    poke("anchor", 6, np.uint64, keeping.n_rows)                     # 6: an anchor row at n_rows
    want = np.array([1, 1, 0, 1, 1, 1, 1, 0], dtype=np.uint32)
    assert n == 8
    want_rows = pattern.copy()
    for i in (2, 7):
        for row, value in p.stored(reqs[i]):
            want_rows[p.base[reqs[i].k] + row] = value
    verdict, scratch = Out(torch, n * 4), Out(torch, total * 64)
    assert launch(fmu, p, a, 0, 0, n, verdict, scratch) == 0
    verdict.check(want, "defensive verdicts", bad, 4, lambda i: " (lane %d)" % i)
    pool.check(want_rows, "defensive buffers", bad, 32)
    sc = scratch.fetch().reshape(total, 64)
    pre = scratch.prefill().reshape(total, 64)
    for i in range(n):                                               # a refused lane leaves its staging rows alone too
        rows = slice(int(off[i]), int(off[i + 1]))
        if want[i] == 1 and not np.array_equal(sc[rows], pre[rows]):
            bad.append("lane %d wrote its scratch rows" % i)
    if not scratch.guards_ok():
        bad.append("bytes around the scratch changed")
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad))


def test_launcher_refusals_and_no_work(libs):
    import torch
    fmu, _, _ = libs
    z = up(torch, np.zeros(64, np.uint64))
    ptr = z.data_ptr()
    out = Out(torch, 256)
    f = fmu.fmu_block_path_commit_many
    ins = lambda: [ptr, ptr, ptr, 1, ptr, ptr, ptr, 0, ptr, ptr, ptr, 0]      # noqa: E731
    assert f(*ins(), 0, out.ptr, out.ptr) == 0                                # n == 0: nothing launched
    for hole in (0, 1, 2, 4, 5, 6, 8, 9, 10):
        args = ins()
        args[hole] = None
        assert f(*args, 1, out.ptr, out.ptr) == 1                             # hipErrorInvalidValue
    args = ins()
    args[3] = 0
    assert f(*args, 1, out.ptr, out.ptr) == 1                                 # an empty session table
    assert f(*ins(), 1, None, out.ptr) == 1 and f(*ins(), 1, out.ptr, None) == 1
    out.fetch()
    assert out.guards_ok() and np.array_equal(out.got[out.lo:out.lo + out.n], out.prefill())
