"""GPU suite: k_block_path_commit_anchored through its launcher alone (tests/device_check/libfill_anchor_unit.so, a forwarder linked against
the product).  Three local slots as in tests/test_gpu_fill_nodes_unit.py -- slots 0 and 1 hold the same tree, its root stated as it is
and as root + r, slot 2 another tree -- and the session's buffer between guard bytes, pre-filled with a non-zero pattern; the oracle's
authentic nodes stand in exactly the rows the case calls known.  Every (block, level) pair with 0 <= level <= depth goes into ONE launch,
so lengths are mixed inside a wave and the offsets into the path buffer are really packed.  What each slot is for:

  slot 0   every row below the top is known: each pair as a true request, with a flipped bit in the fresh root, with a flipped bit in one
           sibling below the level; every fourth true one hands a sibling in as value + r.  Nothing it stores may change a byte, and the
           top row (never an anchor, never written) keeps the pattern.
  slot 1   a seeded part of the rows is known.  A pair whose anchor row is known (or that walks to the stated root + r) must match and
           store its nodes into rows that held the pattern; a pair whose anchor row holds the pattern must MISMATCH although the same row of
           slot 0's stride is authentic.  Pairs whose anchor a matching request of the same launch stores are left out: the host never lets
           such a pair in (FillPlan::validate_anchored), and its verdict would depend on the order of the lanes.
  slot 2   nothing is known: every true path that stops below the top -- the full-length-minus-one paths among them -- must MISMATCH and
           store nothing.

A second launch holds the whole paths (level = depth) of all three slots, and k_block_path_commit_nodes runs on the same inputs over a
second buffer: the same verdicts, the same rows but the slot roots' own.  Every comparison is bit exact."""
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
LIB = os.path.join(ROOT, "tests", "device_check", "libfill_anchor_unit.so")
NODES_LIB = os.path.join(ROOT, "tests", "device_check", "libfill_nodes_unit.so")
NO_ROW = (1 << 64) - 1


@pytest.fixture(scope="module")
def libs(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    for path in (LIB, NODES_LIB):    # a missing check library is built, never worked around
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/" + os.path.basename(path)],
                                  stdout=subprocess.DEVNULL)
    vp, sz, u64, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    fau, fnu = ctypes.CDLL(LIB), ctypes.CDLL(NODES_LIB)
    fau.fau_block_path_commit_anchored.restype = i32
    fau.fau_block_path_commit_anchored.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64, vp]
    fnu.fnu_block_path_commit_nodes.restype, fnu.fnu_block_path_commit_nodes.argtypes = i32, [vp, vp, vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64, vp]
    return fau, fnu


def reduced(row):
    return np.frombuffer((as_int(row) % K.R_MOD).to_bytes(32, "little"), dtype=np.uint8)


def plus_r(row):
    return np.frombuffer((as_int(row) + K.R_MOD).to_bytes(32, "little"), dtype=np.uint8)          # below 2^256: the value is below r


class Req:
    def __init__(self, slot, block, level, fresh, path, label):
        self.slot, self.block, self.level, self.fresh, self.path, self.label = slot, block, level, fresh, path, label


class Plan:
    """The trees, the known rows and the requests of one tree size, with the verdicts the model gives them."""

    def __init__(self, C, n_blocks):
        rng = np.random.default_rng([0xA2C4, n_blocks])
        self.n_blocks, self.n_local = n_blocks, A.ANCHOR_N_LOCAL
        tree_a, tree_b = C.merkle_tree(canonical_rows(rng, n_blocks)), C.merkle_tree(canonical_rows(rng, n_blocks))
        self.trees = [tree_a, tree_a, tree_b]
        self.depth = depth = len(tree_a) - 1
        assert [len(x) for x in tree_a] == K.layer_sizes(n_blocks) and depth == A.depth_of(n_blocks)
        self.slot_roots = np.stack([tree_a[-1][0], plus_r(tree_a[-1][0]), tree_b[-1][0]])
        self.sizes, self.offs, self.n_rows = M.layout(n_blocks, self.n_local)
        self.C = C
        row = lambda lvl, s, k: M.node_row(n_blocks, self.n_local, lvl, s, k)      # noqa: E731
        below_top = [(lvl, k) for lvl in range(depth) for k in range(self.sizes[lvl])]
        self.known = {row(lvl, 0, k) for lvl, k in below_top}                        # slot 0: all below the top; slot 2: nothing
        known_1 = {row(lvl, 1, k) for lvl, k in below_top if rng.random() < 0.4}
        self.known |= known_1
        pairs = [(b, lvl) for b in range(n_blocks) for lvl in range(depth + 1)]
        self.reqs, self.lifted, self.borrowed, self.minus_one, self.left_out = [], 0, 0, 0, 0

        # slot 0
        for k, (b, lvl) in enumerate(pairs):
            self.reqs.append(Req(0, b, lvl, tree_a[0][b].copy(), self.true_path(0, b, lvl), "slot 0 block %d level %d true" % (b, lvl)))
            in_range = [low for low in range(lvl) if ((b >> low) ^ 1) < self.sizes[low]]
            if k % 4 == 0 and in_range:                                              # the same value, handed in as value + r
                low = in_range[k % len(in_range)]
                self.reqs[-1].path[low] = plus_r(self.reqs[-1].path[low])
                self.reqs[-1].label += " sibling %d + r" % low
                self.lifted += 1
            fresh = tree_a[0][b].copy().reshape(1, 32)
            flip(fresh, 0, (b * 11 + lvl * 3 + 5) % 248)
            self.reqs.append(Req(0, b, lvl, fresh[0], self.true_path(0, b, lvl), "slot 0 block %d level %d fresh flipped" % (b, lvl)))
            if lvl:
                path = self.true_path(0, b, lvl)
                low = (b + lvl) % lvl
                flip(path, low, (b * 7 + lvl * 13) % 248)
                self.reqs.append(Req(0, b, lvl, tree_a[0][b].copy(), path, "slot 0 block %d level %d sibling %d flipped" % (b, lvl, low)))
        # slot 1: what matches, what that stores, and the pairs whose anchor holds the pattern for certain
        matches = [(b, lvl) for b, lvl in pairs if (lvl == depth and b == 0) or (lvl < depth and row(lvl, 1, b >> lvl) in known_1)]
        stored = set()
        for b, lvl in matches:
            stored |= set(A.stored_rows(n_blocks, self.n_local, 1, b, lvl))
            self.reqs.append(Req(1, b, lvl, tree_a[0][b].copy(), self.true_path(1, b, lvl), "slot 1 block %d level %d true, anchor known" % (b, lvl)))
        self.fresh_rows = len(stored - known_1)
        for b, lvl in pairs:
            if lvl == depth or (b, lvl) in matches:
                continue
            if row(lvl, 1, b >> lvl) in stored:
                self.left_out += 1
                continue
            assert row(lvl, 0, b >> lvl) in self.known
            self.borrowed += 1
            self.reqs.append(Req(1, b, lvl, tree_a[0][b].copy(), self.true_path(1, b, lvl), "slot 1 block %d level %d true, anchor known in slot 0 only" % (b, lvl)))
        # slot 2: true paths to rows that hold the pattern
        for b, lvl in pairs:
            if lvl < depth:
                self.minus_one += lvl == depth - 1
                self.reqs.append(Req(2, b, lvl, tree_b[0][b].copy(), self.true_path(2, b, lvl), "slot 2 block %d level %d true, nothing known" % (b, lvl)))
        self.want = np.array([self.verdict(q) for q in self.reqs], dtype=np.uint32)
        good = [i for i in range(len(self.reqs)) if self.want[i] == 0]
        k = 0
        while len(self.reqs) <= 256:                                                  # more than one workgroup: matching requests once more
            self.reqs.append(self.reqs[good[k % len(good)]])
            k += 1
        self.want = np.array([self.verdict(q) for q in self.reqs], dtype=np.uint32)

    def true_path(self, slot, b, level):
        tree = self.trees[slot]
        p = np.zeros((level, 32), np.uint8)
        for lvl in range(level):
            if ((b >> lvl) ^ 1) < len(tree[lvl]):
                p[lvl] = tree[lvl][(b >> lvl) ^ 1]
        return p

    def verdict(self, q):
        reached = reduced(A.walk(q.fresh, q.block, self.n_blocks, list(q.path), self.C.compress))
        if q.level == self.depth:
            return 0 if np.array_equal(reached, self.trees[q.slot][-1][0]) else 1
        anchor = M.node_row(self.n_blocks, self.n_local, q.level, q.slot, q.block >> q.level)
        return 0 if anchor in self.known and np.array_equal(reached, self.trees[q.slot][q.level][q.block >> q.level]) else 1

    def node_of(self, r):
        for slot in range(self.n_local):
            for lvl in range(self.depth + 1):
                base = self.offs[lvl] + slot * self.sizes[lvl]
                if base <= r < base + self.sizes[lvl]:
                    return self.trees[slot][lvl][r - base]
        raise AssertionError(r)


@pytest.fixture(scope="module")
def plans(oracle):
    C, _ = oracle
    return {n: Plan(C, n) for n in A.ANCHOR_N_BLOCKS}


def tables(p, reqs, base):
    levels = np.array([q.level for q in reqs], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(levels, dtype=np.uint64)]).astype(np.uint64)
    total = int(off[-1])
    paths = np.concatenate([q.path for q in reqs] + [np.zeros((0, 32), np.uint8)]).reshape(total, 32)
    pairs = np.array([(q.slot, q.block) for q in reqs], dtype=np.uint64)
    fresh = np.stack([q.fresh for q in reqs])
    dest = np.array([M.node_row(p.n_blocks, p.n_local, 0, q.slot, q.block) for q in reqs], dtype=np.uint64)
    anchor = np.array([NO_ROW if q.level == p.depth else M.node_row(p.n_blocks, p.n_local, q.level, q.slot, q.block >> q.level) for q in reqs], dtype=np.uint64)
    return levels, off, total, paths, pairs, fresh, dest, anchor, (off[:-1] + np.uint64(base)).astype(np.uint64)


def test_anchored_commit_compares_with_the_kept_row_and_stores_only_below_it(libs, plans, capsys):
    import torch
    fau, _ = libs
    t0, bad, cases = time.time(), [], 0
    lifted = borrowed = minus_one = fresh_rows = left_out = zero_level = 0
    for n_blocks, p in plans.items():
        what = "anchored n_blocks=%d" % n_blocks
        reqs, want, n = p.reqs, p.want, len(p.reqs)
        assert n > 256
        cases += n
        lifted, borrowed, minus_one = lifted + p.lifted, borrowed + p.borrowed, minus_one + p.minus_one
        fresh_rows, left_out = fresh_rows + p.fresh_rows, left_out + p.left_out
        base = 7 * n_blocks                                                           # path_off as a later chunk of a call would see it
        levels, off, total, paths, pairs, fresh, dest, anchor, off_dev = tables(p, reqs, base)
        assert total > 0
        d = [up(torch, x) for x in (fresh, paths, levels, off_dev, pairs, p.slot_roots, dest, anchor, np.array(p.offs, dtype=np.uint64),
                                    np.array(p.sizes, dtype=np.uint64))]
        verdict, tree, scratch = Out(torch, n * 4), Out(torch, p.n_rows * 32), Out(torch, total * 64)
        start = tree.prefill().copy().reshape(p.n_rows, 32)
        for r in p.known:
            start[r] = p.node_of(r)
        tree.t[tree.lo:tree.lo + tree.n] = torch.from_numpy(start.reshape(-1).copy()).cuda()
        want_rows, named = start.copy(), set()
        for i, q in enumerate(reqs):
            zero_level += q.level == 0 and want[i] == 0
            if want[i] == 0:
                for lvl, idx, _ in A.stored_nodes(n_blocks, q.block, q.level):
                    r = M.node_row(n_blocks, p.n_local, lvl, q.slot, idx)
                    named.add(r)
                    want_rows[r] = p.trees[q.slot][lvl][idx]
        status = fau.fau_block_path_commit_anchored(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), base, d[4].data_ptr(),
                                                    d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), d[9].data_ptr(), n_blocks,
                                                    p.depth, n, verdict.ptr, tree.ptr, p.n_rows, scratch.ptr)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        verdict.check(want, what + " verdicts", bad, 4, lambda i: " (%s)" % reqs[i].label)
        tree.check(want_rows, what + " tree", bad, 32, lambda r: " (row %d of %d, named by a match: %s, known before: %s)" % (r, p.n_rows, r in named, r in p.known))
        # the top rows were never anchors and are never written; slot 2 proved nothing
        got_rows = tree.fetch().reshape(p.n_rows, 32)
        for slot in range(p.n_local):
            top = M.node_row(n_blocks, p.n_local, p.depth, slot, 0)
            if not np.array_equal(got_rows[top], tree.prefill().reshape(p.n_rows, 32)[top]):
                bad.append("%s: the top row of slot %d changed" % (what, slot))
        # scratch: exactly 2 x sum(levels) rows, sibling l canonical at row 2 l of the request's rows, the ancestors of a match the tree's
        got = scratch.fetch().reshape(total, 2, 32)
        if not scratch.guards_ok():
            bad.append("%s: bytes around the scratch changed" % what)
        for i, q in enumerate(reqs):
            for lvl in range(q.level):
                at = int(off[i]) + lvl
                if not np.array_equal(got[at, 0], reduced(q.path[lvl])):
                    bad.append("%s: scratch sibling %d of request %d (%s) is not the canonical sibling" % (what, lvl, i, q.label))
                if want[i] == 0 and not np.array_equal(got[at, 1], p.trees[q.slot][lvl + 1][q.block >> (lvl + 1)]):
                    bad.append("%s: scratch ancestor %d of request %d (%s) is not the tree's" % (what, lvl, i, q.label))
    with capsys.disabled():
        print("\n[fill anchor unit] %d requests over %d tree sizes, %d at level 0 proved, %d siblings handed in as value + r, %d rows of slot 1 stored "
              "over the pattern, %d requests anchored on a row known in slot 0 only, %d full-length-minus-one paths to a pattern row, %d racy pairs "
              "left out, %d failed, %.1f s" % (cases, len(plans), zero_level, lifted, fresh_rows, borrowed, minus_one, left_out, len(bad), time.time() - t0))
    assert zero_level > 0 and lifted > 0 and fresh_rows > 0 and borrowed > 0 and minus_one > 0        # the plan really holds the edges it claims
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:100]))


def test_whole_paths_behave_as_commit_nodes(libs, plans, capsys):
    """level = depth for every block of all three slots -- true, fresh root flipped, one sibling flipped -- from an all-pattern buffer:
    k_block_path_commit_nodes on the same inputs gives the same verdicts and the same rows, but for the slot roots' own."""
    import torch
    fau, fnu = libs
    t0, bad, cases = time.time(), [], 0
    for n_blocks, p in plans.items():
        what = "whole paths n_blocks=%d" % n_blocks
        reqs = []
        for slot in range(p.n_local):
            for b in range(n_blocks):
                leaf = p.trees[slot][0][b]
                reqs.append(Req(slot, b, p.depth, leaf.copy(), p.true_path(slot, b, p.depth), "slot %d block %d true" % (slot, b)))
                fresh = leaf.copy().reshape(1, 32)
                flip(fresh, 0, (b * 11 + 5) % 248)
                reqs.append(Req(slot, b, p.depth, fresh[0], p.true_path(slot, b, p.depth), "slot %d block %d fresh flipped" % (slot, b)))
                path = p.true_path(slot, b, p.depth)
                flip(path, b % p.depth, (b * 7 + 3) % 248)
                reqs.append(Req(slot, b, p.depth, leaf.copy(), path, "slot %d block %d sibling flipped" % (slot, b)))
        n = len(reqs)
        cases += n
        want = np.array([p.verdict(q) for q in reqs], dtype=np.uint32)
        assert (want[0::3] == 0).all() and (want[1::3] == 1).all() and (want[2::3] == 1).all()
        levels, off, total, paths, pairs, fresh, dest, anchor, off_dev = tables(p, reqs, 0)
        assert total == n * p.depth and (anchor == NO_ROW).all()
        d = [up(torch, x) for x in (fresh, paths, levels, off_dev, pairs, p.slot_roots, dest, anchor, np.array(p.offs, dtype=np.uint64),
                                    np.array(p.sizes, dtype=np.uint64))]
        verdict, tree, scratch = Out(torch, n * 4), Out(torch, p.n_rows * 32), Out(torch, total * 64)
        verdict_n, tree_n, scratch_n = Out(torch, n * 4), Out(torch, p.n_rows * 32), Out(torch, total * 64)
        status = fau.fau_block_path_commit_anchored(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 0, d[4].data_ptr(),
                                                    d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), d[9].data_ptr(), n_blocks,
                                                    p.depth, n, verdict.ptr, tree.ptr, p.n_rows, scratch.ptr)
        status_n = fnu.fnu_block_path_commit_nodes(d[0].data_ptr(), d[1].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[8].data_ptr(),
                                                   d[9].data_ptr(), n_blocks, p.depth, n, verdict_n.ptr, tree_n.ptr, p.n_rows, scratch_n.ptr)
        if status != 0 or status_n != 0:
            bad.append("%s: status %d, k_block_path_commit_nodes %d" % (what, status, status_n))
            continue
        verdict.check(want, what + " verdicts", bad, 4, lambda i: " (%s)" % reqs[i].label)
        verdict_n.check(want, what + " verdicts of k_block_path_commit_nodes", bad, 4, lambda i: " (%s)" % reqs[i].label)
        rows, rows_n = tree.fetch().reshape(p.n_rows, 32).copy(), tree_n.fetch().reshape(p.n_rows, 32)
        pattern = tree.prefill().reshape(p.n_rows, 32)
        for slot in range(p.n_local):
            top = M.node_row(n_blocks, p.n_local, p.depth, slot, 0)
            if not np.array_equal(rows[top], pattern[top]):
                bad.append("%s: the top row of slot %d was written" % (what, slot))
            if not np.array_equal(rows_n[top], p.trees[slot][-1][0]):
                bad.append("%s: k_block_path_commit_nodes did not store the top row of slot %d" % (what, slot))
            rows[top] = rows_n[top]
        if not np.array_equal(rows, rows_n) or not tree.guards_ok() or not tree_n.guards_ok():
            bad.append("%s: the rows differ from what k_block_path_commit_nodes stores" % what)
        if not np.array_equal(scratch.fetch(), scratch_n.fetch()) or not scratch.guards_ok():
            bad.append("%s: the scratch differs from k_block_path_commit_nodes'" % what)
    with capsys.disabled():
        print("\n[fill anchor unit] %d whole paths over %d tree sizes against k_block_path_commit_nodes, %d failed, %.1f s" % (cases, len(plans), len(bad),
                                                                                                                             time.time() - t0))
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:100]))


def test_anchored_commit_refusals_and_no_work(libs):
    import torch
    fau, _ = libs
    a = up(torch, np.zeros(64, np.uint64))
    p = a.data_ptr()
    out = Out(torch, 256)
    f = fau.fau_block_path_commit_anchored
    ins = lambda: [p, p, p, p, 0, p, p, p, p, p, p]      # noqa: E731
    assert f(*ins(), 4, 2, 0, out.ptr, out.ptr, 4, out.ptr) == 0                          # n == 0: nothing launched
    for hole in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10):
        args = ins()
        args[hole] = None
        assert f(*args, 4, 2, 1, out.ptr, out.ptr, 4, out.ptr) == 1                       # hipErrorInvalidValue
    assert f(*ins(), 4, 0, 1, out.ptr, out.ptr, 4, out.ptr) == 1
    assert f(*ins(), 0, 2, 1, out.ptr, out.ptr, 4, out.ptr) == 1
    assert f(*ins(), 4, 2, 1, None, out.ptr, 4, out.ptr) == 1
    assert f(*ins(), 4, 2, 1, out.ptr, None, 4, out.ptr) == 1
    assert f(*ins(), 4, 2, 1, out.ptr, out.ptr, 4, None) == 1
    out.fetch()
    assert out.guards_ok() and np.array_equal(out.got[out.lo:out.lo + out.n], out.prefill())
