"""CPU checks of cp2_datasets_set_roots_many: the name is exported and carries the same signature in the header, the ctypes binding and the
Nim binding; the model's layer sizes and tree-major offsets (tests/set_roots_many_models.py) equal the oracle's Merkle layers; the model of
the plan is held against brute force at every level -- every (tree, node) covered exactly once, the lane search inverting the prefix
table, no two trees' rows overlapping, chunks within their byte bound and an oversized request alone --; and the product's plan
(csrc/set_roots_plan.hpp), compiled stand-alone under AddressSanitizer + UBSan, agrees with the model on seeded random calls."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import nim_api as N
import set_roots_many_models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
NAME = "cp2_datasets_set_roots_many"
SIGNATURE = ("i32", ["handle:ctx", "ptr(handle:dataset)", "ptr(ptr(u8))", "usize", "ptr(u8)"])


def test_the_name_is_exported_and_bound(pkg):
    protos, procs = N.header_prototypes(HEADER), N.nim_importc(NIM)
    L = pkg.load_library()
    assert NAME in set(pkg.exported_symbols())
    assert protos[NAME] == procs[NAME] == SIGNATURE, (protos[NAME], procs[NAME])
    assert getattr(L, NAME).restype is ctypes.c_int and len(L._cp2_signatures[NAME][1]) == 5
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    assert NAME in history and re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER)
    assert callable(pkg.Context.set_roots_many)


def test_null_ctx_is_refused(pkg):
    L = pkg.load_library()
    hs = (ctypes.c_void_p * 2)(5, 7)
    own = (ctypes.c_uint8 * 2)(9, 9)
    assert L.cp2_datasets_set_roots_many(None, hs, None, 2, own) == -1
    assert L.cp2_datasets_set_roots_many(None, None, None, 0, None) == -1
    assert list(own) == [9, 9]


# ---- the sizes and offsets against the oracle's tree -------------------------------------------------------------------------------------
def test_layer_sizes_and_offsets_equal_the_oracle(oracle):
    c, _ = oracle
    rng = np.random.default_rng(0x5E7)
    for n in range(1, 41):
        leaves = np.zeros((n, 32), dtype=np.uint8)
        leaves[:, :31] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
        layers = c.merkle_tree(leaves)
        assert [len(x) for x in layers] == M.layer_sizes(n)
        assert M.levels(n) == len(layers) - 1 and M.total(n) == sum(len(x) for x in layers)
        flat = np.concatenate(layers)                                         # tree-major: the layers of one tree, bottom first
        for k, layer in enumerate(layers):
            assert np.array_equal(flat[M.layer_off(n, k):M.layer_off(n, k) + len(layer)], layer)


# ---- the plan against brute force ---------------------------------------------------------------------------------------------------------
def random_call(rnd):
    kind = rnd.randrange(4)
    if kind == 0:                                                             # all singletons
        return [1] * rnd.randint(1, 300)
    if kind == 1:                                                             # one giant beside many small
        ns = [rnd.randint(1, 9) for _ in range(rnd.randint(20, 299))]
        ns.insert(rnd.randrange(len(ns) + 1), rnd.randint(3000, 5000))
        return ns
    if kind == 2:
        return [rnd.choice((1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257)) for _ in range(rnd.randint(1, 300))]
    return [rnd.randint(1, 5000) for _ in range(rnd.randint(1, 40))]


def random_bound(rnd, ns):
    big = max(M.total(n) for n in ns) * 32
    return rnd.choice((big - 32, big, 3 * big + 64, 64, 1 << 20, sum(M.total(n) for n in ns) * 32))


@pytest.mark.parametrize("seed", range(12))
def test_plan_covers_every_node_exactly_once(seed):
    rnd = random.Random(seed)
    ns = random_call(rnd) if seed else [1, 3, 1, 64, 2, 100, 1]
    p = M.plan(ns)
    assert p.rows == sum(M.total(n) for n in ns)
    owner = np.full(p.rows, -1, dtype=np.int64)                               # no two trees' rows overlap, none left over
    for r, (first, n) in enumerate(p.tree_tab):
        assert n == ns[r] and (owner[first:first + M.total(n)] == -1).all()
        owner[first:first + M.total(n)] = r
    assert (owner >= 0).all()
    assert len(p.level_off) == max(M.levels(n) for n in ns)
    written = np.zeros(p.rows, dtype=np.int32)
    for k in range(len(p.level_off)):
        active = [r for r, n in enumerate(ns) if M.levels(n) > k]
        a = p.level_off[k]
        assert p.tree_of[a:a + p.level_cnt[k]] == active
        assert p.level_work[k] == sum(M.layer_sizes(ns[r])[k + 1] for r in active)
        want = [(r, j) for r in active for j in range(M.layer_sizes(ns[r])[k + 1])]          # brute force: the lanes in order
        got = [M.lane(p, k, t) for t in range(p.level_work[k])]
        assert got == want                                                    # the search inverts the prefix table
        for r, j in got:
            first, n = p.tree_tab[r]
            src, dst = first + M.layer_off(n, k) + 2 * j, first + M.layer_off(n, k + 1) + j
            assert src < first + M.layer_off(n, k + 1) and owner[dst] == r
            written[dst] += 1
    leaves = np.zeros(p.rows, dtype=bool)
    for first, n in p.tree_tab:
        leaves[first:first + n] = True
    assert (written[leaves] == 0).all() and (written[~leaves] == 1).all()     # every node above the leaves exactly once


@pytest.mark.parametrize("seed", range(12))
def test_chunks_respect_the_bound_and_an_oversized_request_is_alone(seed):
    rnd = random.Random(100 + seed)
    ns = random_call(rnd)
    bound = random_bound(rnd, ns)
    cs = M.chunks(ns, bound)
    assert [c.first for c in cs] == [sum(x.count for x in cs[:i]) for i in range(len(cs))] and sum(c.count for c in cs) == len(ns)
    for i, c in enumerate(cs):
        assert c.count >= 1 and c.rows == sum(M.total(n) for n in ns[c.first:c.first + c.count])
        assert c.rows * 32 <= bound or c.count == 1
        if i + 1 < len(cs):                                                   # greedy: the next request would not have fitted
            assert (c.rows + M.total(ns[cs[i + 1].first])) * 32 > bound
    for i, n in enumerate(ns):
        if M.total(n) * 32 > bound:
            assert [c for c in cs if c.first <= i < c.first + c.count][0].count == 1


# ---- the product's plan, stand-alone under the sanitizers, against the model ----------------------------------------------------------------
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("srm") / "set_roots_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "set_roots_plan_check.cpp")])
    return exe


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return r.stdout


CALLS = [([1] * 300, 64), ([1] * 7, 1 << 20), ([5000], 1 << 20), ([1, 5000, 1], 1 << 20), ([3] * 20 + [4096] + [2] * 279, 4096),
         ([1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1], 1 << 30)]


@pytest.mark.parametrize("seed", range(len(CALLS) + 10))
def test_product_plan_equals_the_model(check, tmp_path, seed):
    if seed < len(CALLS):
        ns, bound = CALLS[seed]
    else:
        rnd = random.Random(2000 + seed)
        ns = random_call(rnd)
        bound = random_bound(rnd, ns)
    f = tmp_path / "call.txt"
    f.write_text(M.describe(ns, bound))
    assert run(check, f) == M.expected(ns, bound)


def test_the_calls_cover_what_they_claim():
    calls = [c[0] for c in CALLS] + [random_call(random.Random(2000 + s)) for s in range(len(CALLS), len(CALLS) + 10)]
    assert min(min(c) for c in calls) == 1 and max(max(c) for c in calls) == 5000
    assert min(len(c) for c in calls) == 1 and max(len(c) for c in calls) == 300
    assert any(set(c) == {1} and len(c) > 1 for c in calls) and any(len(c) > 20 and max(c) >= 3000 and sorted(c)[-2] <= 9 for c in calls)
