"""GPU suite: k_block_path_commit_nodes through its launcher alone (tests/device_check/libfill_nodes_unit.so, a forwarder linked against the
product).  Three local slots -- slots 0 and 1 hold the same tree, its root stated as it is and as root + r, slot 2 another tree -- so the
requests of tests/kernel_models.py's walk_plan name their slot directly and the slot stride is in every row.  The session's buffer lies
between guard bytes and is pre-filled with a non-zero pattern; afterwards it must hold, row for row, the oracle's tree node wherever a
MATCHING request's stored set (tests/fill_nodes_models.py) names the row and the pre-fill everywhere else.  Every comparison is bit exact."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import fill_nodes_models as M
import kernel_models as K
from test_gpu_kernel_units import Out, as_int, canonical_rows, flip, up

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libfill_nodes_unit.so")
KU_LIB = os.path.join(ROOT, "tests", "device_check", "libkernel_unit.so")


@pytest.fixture(scope="module")
def libs(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    for path in (LIB, KU_LIB):       # a missing check library is built, never worked around
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/" + os.path.basename(path)],
                                  stdout=subprocess.DEVNULL)
    vp, sz, u64, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    fnu, ku = ctypes.CDLL(LIB), ctypes.CDLL(KU_LIB)
    fnu.fnu_block_path_commit_nodes.restype, fnu.fnu_block_path_commit_nodes.argtypes = i32, [vp, vp, vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64, vp]
    ku.ku_block_path_commit.restype, ku.ku_block_path_commit.argtypes = i32, [vp, vp, vp, vp, vp, u64, u32, sz, vp, vp, u64]
    return fnu, ku


def reduced(row):
    return np.frombuffer((as_int(row) % K.R_MOD).to_bytes(32, "little"), dtype=np.uint8)


def plus_r(row):
    return np.frombuffer((as_int(row) + K.R_MOD).to_bytes(32, "little"), dtype=np.uint8)          # below 2^256: the value is below r


def node_requests(C, n_blocks):
    """walk_plan(n_blocks) with the slot_roots index as the local slot, then slot 2's own blocks: every third one true, the others with one
    flipped sibling bit; every fourth true request hands one sibling in as value + r; every second matching request once more."""
    rng = np.random.default_rng([0xF111, n_blocks])
    tree_a, tree_b = C.merkle_tree(canonical_rows(rng, n_blocks)), C.merkle_tree(canonical_rows(rng, n_blocks))
    trees = [tree_a, tree_a, tree_b]
    depth = len(tree_a) - 1
    assert [len(x) for x in tree_a] == K.layer_sizes(n_blocks)
    slot_roots = np.stack([tree_a[-1][0], plus_r(tree_a[-1][0]), tree_b[-1][0]])

    def true_path(tree, b):
        p = np.zeros((depth, 32), np.uint8)
        for lvl in range(depth):
            if ((b >> lvl) ^ 1) < len(tree[lvl]):
                p[lvl] = tree[lvl][(b >> lvl) ^ 1]
        return p

    reqs = []                                          # (slot, index, fresh, path, label)
    for q in K.walk_plan(n_blocks):
        fresh, path = tree_a[0][q.block].copy(), true_path(tree_a, q.block)
        if q.kind == "sibling":
            flip(path, q.level, (q.block * 7 + q.level * 13) % 248)
        elif q.kind == "fresh":
            fresh = fresh.copy()
            flip(fresh.reshape(1, 32), 0, (q.block * 11 + 5) % 248)
        reqs.append((q.root, q.index, fresh, path, str(q)))
    for b in range(n_blocks):
        path = true_path(tree_b, b)
        if b % 3:
            flip(path, b % depth, (b * 5 + 3) % 248)
        reqs.append((2, b, tree_b[0][b].copy(), path, "slot 2 block %d %s" % (b, "flipped" if b % 3 else "true")))
    want = np.empty(len(reqs), np.uint32)
    for i, (slot, index, fresh, path, _) in enumerate(reqs):
        reached = K.walk_model(fresh, index, n_blocks, list(path), C.compress)
        want[i] = 0 if np.array_equal(reached, trees[slot][-1][0]) else 1
    lifted = 0
    for i in np.nonzero(want == 0)[0][::4]:            # the same value, handed in as value + r, at a level that has a sibling
        slot, index, fresh, path, label = reqs[i]
        levels = [lvl for lvl in range(depth) if ((index >> lvl) ^ 1) < len(trees[slot][lvl])]
        if levels:
            lvl = levels[i % len(levels)]
            path = path.copy()
            path[lvl] = plus_r(path[lvl])
            reqs[i] = (slot, index, fresh, path, label + " sibling %d + r" % lvl)
            lifted += 1
    again = np.nonzero(want == 0)[0][::2]
    reqs += [reqs[i] for i in again]
    want = np.concatenate([want, want[again]])
    return trees, depth, slot_roots, reqs, want, lifted


@pytest.fixture(scope="module")
def plans(oracle):
    C, _ = oracle
    return {n: node_requests(C, n) for n in M.NODE_N_BLOCKS}


def test_commit_nodes_stores_the_proved_paths_and_nothing_else(libs, plans, capsys):
    import torch
    fnu, ku = libs
    t0, bad, cases, only_mismatching, lifted_all, out_of_range = time.time(), [], 0, 0, 0, 0
    n_local = M.NODE_N_LOCAL
    for n_blocks, (trees, depth, slot_roots, reqs, want, lifted) in plans.items():
        what = "commit_nodes n_blocks=%d" % n_blocks
        sizes, offs, n_rows = M.layout(n_blocks, n_local)
        n = len(reqs)
        cases += n
        lifted_all += lifted
        pairs = np.array([(slot, index) for slot, index, _, _, _ in reqs], dtype=np.uint64)
        fresh = np.stack([r[2] for r in reqs])
        paths = np.stack([r[3] for r in reqs])
        dest = np.array([M.node_row(n_blocks, n_local, 0, slot, index) for slot, index, _, _, _ in reqs], dtype=np.uint64)
        d = [up(torch, x) for x in (fresh, paths, pairs, slot_roots, dest, np.array(offs, dtype=np.uint64), np.array(sizes, dtype=np.uint64))]
        verdict, tree, scratch = Out(torch, n * 4), Out(torch, n_rows * 32), Out(torch, n * depth * 64)
        verdict_plain, layer0_plain = Out(torch, n * 4), Out(torch, n_rows * 32)
        # expected rows: the oracle's node wherever a matching request's stored set names the row
        want_rows = tree.prefill().copy().reshape(n_rows, 32)
        named_by_match, named_by_any = set(), set()
        for i, (slot, index, _, _, _) in enumerate(reqs):
            for lvl, idx, _ in M.stored_nodes(n_blocks, index):
                row = M.node_row(n_blocks, n_local, lvl, slot, idx)
                named_by_any.add(row)
                if want[i] == 0:
                    named_by_match.add(row)
                    want_rows[row] = trees[slot][lvl][idx]
            out_of_range += sum(1 for lvl in range(depth) if ((index >> lvl) ^ 1) >= sizes[lvl] and want[i] == 0)
        only_mismatching += len(named_by_any - named_by_match)
        status = fnu.fnu_block_path_commit_nodes(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                                                 d[6].data_ptr(), n_blocks, depth, n, verdict.ptr, tree.ptr, n_rows, scratch.ptr)
        if status != 0:
            bad.append("%s: status %d" % (what, status))
            continue
        name = lambda i: " (%s)" % reqs[i][4]      # noqa: E731
        verdict.check(want, what + " verdicts", bad, 4, name)
        tree.check(want_rows, what + " tree", bad, 32, lambda r: " (row %d of %d, named by a match: %s)" % (r, n_rows, r in named_by_match))
        # the scratch stays inside its n x depth x 64 bytes; sibling l of request i lands canonical at row 2 l, the ancestors of a matching
        # request are the tree's
        got = scratch.fetch().reshape(n, depth, 2, 32)
        if not scratch.guards_ok():
            bad.append("%s: bytes around the scratch changed" % what)
        for i, (slot, index, _, path, label) in enumerate(reqs):
            for lvl in range(depth):
                if not np.array_equal(got[i, lvl, 0], reduced(path[lvl])):
                    bad.append("%s: scratch sibling %d of request %d (%s) is not the canonical sibling" % (what, lvl, i, label))
                if want[i] == 0 and not np.array_equal(got[i, lvl, 1], trees[slot][lvl + 1][index >> (lvl + 1)]):
                    bad.append("%s: scratch ancestor %d of request %d (%s) is not the tree's" % (what, lvl, i, label))
        # k_block_path_commit on the same requests: the same verdicts, and layer 0 of its buffer equals layer 0 of this one
        status = ku.ku_block_path_commit(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), n_blocks, depth, n,
                                         verdict_plain.ptr, layer0_plain.ptr, n_rows)
        if status != 0:
            bad.append("%s: k_block_path_commit status %d" % (what, status))
            continue
        if not np.array_equal(verdict_plain.fetch(), verdict.fetch()):
            bad.append("%s: the verdicts differ from k_block_path_commit's" % what)
        plain_rows = layer0_plain.fetch().reshape(n_rows, 32)
        stored_plain = {int(dest[i]) for i in range(n) if want[i] == 0}
        for r in stored_plain:
            if not np.array_equal(plain_rows[r], want_rows[r]):
                bad.append("%s: row %d differs from what k_block_path_commit stores" % (what, r))
    with capsys.disabled():
        print("\n[fill nodes unit] %d requests over %d tree sizes, %d siblings handed in as value + r, %d out-of-range siblings skipped, %d rows named "
              "by mismatching requests only, %d failed, %.1f s" % (cases, len(plans), lifted_all, out_of_range, only_mismatching, len(bad), time.time() - t0))
    assert lifted_all > 0 and out_of_range > 0 and only_mismatching > 0          # the plan really holds the edges it claims
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:100]))


def test_commit_nodes_refusals_and_no_work(libs):
    import torch
    fnu, _ = libs
    a = up(torch, np.zeros(64, np.uint64))
    p = a.data_ptr()
    out = Out(torch, 256)
    assert fnu.fnu_block_path_commit_nodes(p, p, p, p, p, p, p, 4, 2, 0, out.ptr, out.ptr, 4, out.ptr) == 0       # n == 0: nothing launched
    for hole in range(7):
        args = [p] * 7
        args[hole] = None
        assert fnu.fnu_block_path_commit_nodes(*args, 4, 2, 1, out.ptr, out.ptr, 4, out.ptr) == 1                  # hipErrorInvalidValue
    assert fnu.fnu_block_path_commit_nodes(p, p, p, p, p, p, p, 4, 0, 1, out.ptr, out.ptr, 4, out.ptr) == 1
    assert fnu.fnu_block_path_commit_nodes(p, p, p, p, p, p, p, 0, 2, 1, out.ptr, out.ptr, 4, out.ptr) == 1
    assert fnu.fnu_block_path_commit_nodes(p, p, p, p, p, p, p, 4, 2, 1, None, out.ptr, 4, out.ptr) == 1
    assert fnu.fnu_block_path_commit_nodes(p, p, p, p, p, p, p, 4, 2, 1, out.ptr, None, 4, out.ptr) == 1
    assert fnu.fnu_block_path_commit_nodes(p, p, p, p, p, p, p, 4, 2, 1, out.ptr, out.ptr, 4, None) == 1
    out.fetch()
    assert out.guards_ok() and np.array_equal(out.got[out.lo:out.lo + out.n], out.prefill())
