"""GPU suite: launch_compress_layers_ragged on its own (csrc/kernels.hpp), through the forwarder of tests/device_check/set_roots_many_unit.hip.

cp2_datasets_set_roots_many reaches k_compress_layer_ragged only behind a host that lays its trees out back to back; here the launcher gets
its tables directly (tests/set_roots_many_models.py makes them), and the trees of a case lie in one buffer with guard rows in front,
between and behind.  The WHOLE buffer is compared: every node above the leaves must be the C oracle's Merkle tree of that tree's leaves,
the leaves must be unchanged and the guard rows must keep their pattern.

Shapes: leaf counts from {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257}; per case the trees are drawn so that
level 0 has 1, 63, 64, 65, 255, 256, 257 or 4097 nodes, the first and the last tree are singletons, trees of several depths share a case
(they leave at different levels) and small odd trees put paired and odd-tail nodes of several trees into one wave."""
import collections
import ctypes
import faulthandler
import os
import random
import subprocess

import numpy as np
import pytest

import set_roots_many_models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device_check", "libset_roots_many_unit.so")
HIP_INVALID = 1                               # hipErrorInvalidValue
LEAVES = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257)
TOTALS = (1, 63, 64, 65, 255, 256, 257, 4097)
GUARD = 3                                     # rows in front of the first and behind the last tree
Case = collections.namedtuple("Case", "no trees")


@pytest.fixture(autouse=True)
def time_limit():
    """every test under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def compose(total, rnd):
    """leaf counts whose level 0 has `total` nodes: a singleton first and last, drawn sizes between"""
    if total == 1:
        return [1]
    trees, left = [1], total - 2
    while left:
        n = rnd.choice([n for n in LEAVES if (n + 1) // 2 <= left])
        trees.append(n)
        left -= (n + 1) // 2
    return trees + [1]


def plan():
    cases = []
    for t in TOTALS:
        cases.append(Case(len(cases), compose(t, random.Random(t))))
    cases.append(Case(len(cases), [1, 3, 5, 7, 9, 3, 2, 1, 5, 4, 7, 3, 9, 1, 33, 1]))     # one wave at level 0, nine kinds of tree in it
    cases.append(Case(len(cases), list(LEAVES) + [1]))
    return cases


def test_the_plan_holds_the_shapes_it_claims():
    cases = plan()
    works = {w for c in cases for w in M.plan(c.trees).level_work}
    assert set(TOTALS) <= works
    assert {n for c in cases for n in c.trees} == set(LEAVES)
    for c in cases:
        assert c.trees[0] == 1 and c.trees[-1] == 1
    many = [c for c in cases if len(c.trees) > 3]
    assert all(len({M.levels(n) for n in c.trees}) >= 3 for c in many)       # trees leave at different levels
    mixed = 0
    for c in cases:                                                            # a wave with lanes of several trees, paired and odd-tail nodes mixed
        p = M.plan(c.trees)
        lanes = [M.lane(p, 0, t) for t in range(min(64, p.level_work[0]))]
        odd = [2 * j + 1 >= c.trees[r] for r, j in lanes]
        mixed += int(len({r for r, _ in lanes}) >= 4 and any(odd) and not all(odd))
    assert mixed >= 3
    assert any(sum(M.total(n) for n in c.trees) > 8192 for c in cases)         # many workgroups


@pytest.fixture(scope="module")
def srm(pkg):
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg.load_library()
    if not os.path.exists(LIB):      # a missing check library is built, never worked around
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "codex-storage-proofs-circuits_amd"), "../tests/device_check/libset_roots_many_unit.so"],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(LIB)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.srm_compress_layers_ragged.restype, lib.srm_compress_layers_ragged.argtypes = ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, sz]
    return lib


@pytest.fixture(scope="module")
def torch_(srm):
    import torch
    yield torch
    torch.cuda.synchronize()


def up(torch, arr):
    a = np.array(arr, copy=True, order="C")
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def hp(a):
    return a.ctypes.data if a.size else None


class Layout:
    """The buffer of one case: GUARD rows, then every tree with 1 or 2 guard rows after it, GUARD more at the end; `image` is what the
    device starts from (a pattern everywhere, random field elements in the leaves), `want` what it must hold afterwards."""

    def __init__(self, c, oracle):
        rng = np.random.default_rng([0x5E70, c.no])
        self.plan = M.plan(c.trees)
        first, at = [], GUARD
        for r, n in enumerate(c.trees):
            first.append(at)
            at += M.total(n) + 1 + r % 2
        self.rows = at + GUARD
        self.tab = np.asarray([(f, n) for f, n in zip(first, c.trees)], dtype=np.uint64).reshape(-1)
        self.image = rng.integers(0, 256, size=(self.rows, 32), dtype=np.uint8)
        self.want = self.image.copy()
        for f, n in zip(first, c.trees):
            leaves = np.zeros((n, 32), dtype=np.uint8)
            leaves[:, :31] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
            self.image[f:f + n] = leaves
            tree = np.concatenate(oracle.merkle_tree(leaves))
            assert len(tree) == M.total(n)
            self.want[f:f + len(tree)] = tree


def launch(torch, lib, lay, rows_ptr=None, tables=True):
    _, prefix, tree_of, off, cnt, work = M.ragged_tables(lay.plan)
    d_rows, d_tab, d_prefix, d_tree = up(torch, lay.image), up(torch, lay.tab), up(torch, prefix), up(torch, tree_of)
    st = lib.srm_compress_layers_ragged(d_rows.data_ptr() if rows_ptr is None else rows_ptr(d_rows), d_tab.data_ptr() if tables else None,
                                        d_prefix.data_ptr(), d_tree.data_ptr(), hp(off), hp(cnt), hp(work), len(off))
    torch.cuda.synchronize()
    return st, d_rows.cpu().numpy().reshape(-1, 32)


def test_ragged_trees_against_the_oracle_with_guard_rows(srm, torch_, oracle, capsys):
    c_oracle, _ = oracle
    bad, cases = [], plan()
    for c in cases:
        lay = Layout(c, c_oracle)
        st, got = launch(torch_, srm, lay)
        what = "case %d (%d trees, %d rows)" % (c.no, len(c.trees), lay.rows)
        if st != 0:
            bad.append("%s: status %d" % (what, st))
        elif not np.array_equal(got, lay.want):
            rows = np.nonzero((got != lay.want).any(axis=1))[0]
            bad.append("%s: %d rows differ, first row %d" % (what, rows.size, int(rows[0])))
    with capsys.disabled():
        print("\n[set roots many unit] %d cases checked, 0 skipped, %d failed" % (len(cases), len(bad)))
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad))


def test_refusals_and_no_work(srm, torch_, oracle):
    c_oracle, _ = oracle
    lay = Layout(Case(99, [1, 5, 2, 1]), c_oracle)
    st, got = launch(torch_, srm, lay, tables=False)                           # a NULL table with work to do
    assert st == HIP_INVALID and np.array_equal(got, lay.image)
    st, got = launch(torch_, srm, lay, rows_ptr=lambda t: None)
    assert st == HIP_INVALID
    st, got = launch(torch_, srm, lay, rows_ptr=lambda t: t.data_ptr() + 8)   # rows not 16-byte aligned
    assert st == HIP_INVALID and np.array_equal(got, lay.image)
    f = srm.srm_compress_layers_ragged
    zero = np.zeros(3, dtype=np.uint64)
    assert f(None, None, None, None, None, None, None, 0) == 0                 # no levels: no work
    assert f(None, None, None, None, hp(zero), hp(zero), hp(zero), 3) == 0     # levels without lanes: no work
    st, got = launch(torch_, srm, lay)                                         # and the same arguments, valid
    assert st == 0 and np.array_equal(got, lay.want)
