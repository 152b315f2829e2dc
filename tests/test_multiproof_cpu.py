"""CPU checks of block multiproofs: the layout (the model of tests/multiproof_models.py and the library's cp2_block_multiproof_rows /
cp2_block_multiproof_layout) against the issue's literals and against brute force; the model's verifier over C-oracle trees -- it
reproduces the root and every inner node, and fails for any flipped leaf, flipped row or swap of two differing rows --; the names in the
header, the Nim binding and the ctypes table; NULL arguments refused with outputs untouched; and the product's host side
(csrc/multiproof_plan.hpp), compiled with its own main under AddressSanitizer + UBSan and run as a process, against the model line by
line: layouts, every refusal in its order with its index, the work table, the job tables, every row's (group, level, index), the commit
list of a fill, FillPlan::mark_proved_multi bit for bit against mark_proved, and the 2^32 - 1 row limit through synthetic counts."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import multiproof_models as M
import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_OK, CP2_ERR_INVALID = 0, -1
NAMES = ("cp2_block_multiproof_rows", "cp2_block_multiproof_layout", "cp2_dataset_block_multiproofs", "cp2_blocks_verify_multi", "cp2_fill_add_multi")
SECTION = "---- block multiproofs: many blocks of a slot served, checked and filled with shared Merkle nodes"
LITERALS = [(1, [0], []), (2, [0], [(0, 1)]), (5, [4], [(2, 0)]), (5, [0, 4], [(0, 1), (1, 1)]), (5, [1, 2], [(0, 0), (0, 3), (2, 1)]),
            (7, [6], [(1, 2), (2, 0)]), (9, [0, 8], [(0, 1), (1, 1), (2, 1)]), (128, [0, 1, 2, 3], [(l, 1) for l in range(2, 7)]),
            (8, list(range(8)), [])]
RANDOM_BLOCKS = list(range(11, 34)) + [64, 65, 127, 128, 129, 257]
CELL, BLOCK = 128, 4096                               # 32 cells per block: n_cells = 32 x nBlocks


def subsets(rng, n, count):
    for _ in range(count):
        k = int(rng.integers(1, n + 1))
        yield sorted(int(x) for x in rng.choice(n, size=k, replace=False))


# ---- the layout -----------------------------------------------------------------------------------------------------------------------------
def test_the_models_layout_holds_the_literals():
    for n, B, want in LITERALS:
        assert M.layout(n, B) == want, (n, B)


def test_the_librarys_layout_holds_the_literals(pkg):
    for n, B, want in LITERALS:
        assert pkg.block_multiproof_rows(CELL, BLOCK, 32 * n, B) == len(want), (n, B)
        assert pkg.block_multiproof_layout(CELL, BLOCK, 32 * n, B) == want, (n, B)


def test_the_library_refuses_lists_and_geometries(pkg):
    L = pkg.load_library()
    none = ctypes.c_size_t(-1).value

    def rows(n_cells, B, cell=CELL):
        b = np.array(B, dtype=np.uint64)
        return L.cp2_block_multiproof_rows(cell, BLOCK, n_cells, b.ctypes.data if b.size else None, len(B))

    assert rows(32 * 5, [0, 4]) == 2
    assert rows(32 * 5, []) == none and rows(32 * 5, [5]) == none and rows(32 * 5, [1, 1]) == none and rows(32 * 5, [2, 1]) == none
    assert rows(32 * 5 + 1, [0]) == none and rows(32 * 5, [0], cell=0) == none
    li = np.full((4, 2), 0x5E, dtype=np.uint64)
    b = np.array([2, 1], dtype=np.uint64)
    assert L.cp2_block_multiproof_layout(CELL, BLOCK, 32 * 5, b.ctypes.data, 2, li.ctypes.data) == CP2_ERR_INVALID and (li == 0x5E).all()
    with pytest.raises(ValueError):
        pkg.block_multiproof_layout(CELL, BLOCK, 32 * 5, [1, 1])


def test_the_layout_against_brute_force():
    rng = np.random.default_rng(0x3B)
    for n in range(1, 11):
        for k in range(1, n + 1):
            for B in itertools.combinations(range(n), k):
                rows, union = M.brute(n, B)
                got = M.layout(n, list(B))
                assert got == rows and len(got) <= union, (n, B)
        assert M.layout(n, list(range(n))) == []
    for n in RANDOM_BLOCKS:
        for B in subsets(rng, n, 200):
            rows, union = M.brute(n, B)
            got = M.layout(n, B)
            assert got == rows and len(got) <= union, (n, B)
        assert M.layout(n, list(range(n))) == []


def test_the_librarys_layout_against_the_model(pkg):
    rng = np.random.default_rng(0x3C)
    for n in list(range(1, 11)) + RANDOM_BLOCKS:
        for B in subsets(rng, n, 12):
            assert pkg.block_multiproof_layout(CELL, BLOCK, 32 * n, B) == M.layout(n, B), (n, B)


# ---- the verifier over the oracle's trees ---------------------------------------------------------------------------------------------------
def tree_of(c_oracle, rng, n):
    leaves = np.zeros((n, 32), dtype=np.uint8)
    leaves[:, :31] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
    return c_oracle.merkle_tree(leaves)


def test_the_verifier_reproduces_the_oracles_trees(oracle):
    c_oracle, _ = oracle
    rng = np.random.default_rng(0x3D)
    sizes = [1, 2, 3, 4, 5, 7, 8, 9, 16, 33, 64, 65]
    for t in range(100):
        n = sizes[t % len(sizes)]
        layers = tree_of(c_oracle, rng, n)
        assert [len(x) for x in layers] == M.layer_sizes(n)
        B = next(subsets(rng, n, 1))
        rows = [layers[l][i] for l, i in M.layout(n, B)]
        ok, nodes = M.verify(c_oracle.compress, n, B, [layers[0][b] for b in B], rows, layers[-1][0])
        assert ok, (n, B)
        want = {(l, b >> l) for b in B for l in range(1, M.depth(n) + 1)}
        assert set(nodes) == want
        for (l, i), v in nodes.items():
            assert np.array_equal(v, layers[l][i]), (n, B, l, i)


def test_the_verifier_fails_for_every_single_corruption(oracle):
    c_oracle, _ = oracle
    rng = np.random.default_rng(0x3E)
    for n in (1, 2, 5, 7, 9, 16, 33):
        layers = tree_of(c_oracle, rng, n)
        for B in subsets(rng, n, 3):
            leaves, rows, root = [layers[0][b].copy() for b in B], [layers[l][i].copy() for l, i in M.layout(n, B)], layers[-1][0]
            assert M.verify(c_oracle.compress, n, B, leaves, rows, root)[0]
            for j in range(len(leaves)):
                bad = [x.copy() for x in leaves]
                bad[j][int(rng.integers(0, 31))] ^= 1 << int(rng.integers(0, 8))
                assert not M.verify(c_oracle.compress, n, B, bad, rows, root)[0], (n, B, "leaf", j)
            for j in range(len(rows)):
                bad = [x.copy() for x in rows]
                bad[j][int(rng.integers(0, 31))] ^= 1 << int(rng.integers(0, 8))
                assert not M.verify(c_oracle.compress, n, B, leaves, bad, root)[0], (n, B, "row", j)
            for j, k in itertools.combinations(range(len(rows)), 2):
                if not np.array_equal(rows[j], rows[k]):
                    bad = list(rows)
                    bad[j], bad[k] = rows[k], rows[j]
                    assert not M.verify(c_oracle.compress, n, B, leaves, bad, root)[0], (n, B, "swap", j, k)
            assert not M.verify(c_oracle.compress, n, B, leaves, rows[:-1], root)[0] or not rows


def test_a_row_plus_r_verifies_like_the_row(oracle):
    c_oracle, _ = oracle
    rng = np.random.default_rng(0x3F)
    seen = 0
    for n in (5, 9, 33):
        layers = tree_of(c_oracle, rng, n)
        for B in subsets(rng, n, 4):
            rows = [layers[l][i].copy() for l, i in M.layout(n, B)]
            for j, row in enumerate(rows):
                v = int.from_bytes(row.tobytes(), "little") + M.R_MOD
                if v < 1 << 256:
                    rows[j] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
                    seen += 1
            assert M.verify(c_oracle.compress, n, B, [layers[0][b] for b in B], rows, layers[-1][0])[0]
    assert seen > 20


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
def test_the_names_are_exported_and_match_in_header_nim_and_ctypes(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    protos, procs = N.header_prototypes(HEADER), N.nim_importc(NIM)
    L = pkg.load_library()
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    for name in NAMES:
        assert name in exported and name in history, name
        assert protos[name] == procs[name], (name, protos[name], procs[name])
        assert name in L._cp2_signatures and callable(getattr(L, name))
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER) and pkg.ABI_VERSION_MINOR == 2
    at = HEADER.index(SECTION)
    section = HEADER[at:HEADER.index(";", HEADER.index("int cp2_fill_add_multi("))]
    assert "#define" not in section
    for word in ("belongs to the GROUP", "cannot say which one", "NOT sent", "STRICTLY ASCENDING", "always the full count", "Read-only", "CP2_TRACE",
                 "all or nothing", "2^32 - 1", "n_groups == 0", "CP2_ERR_HIP", "Out of scope", "cp2_multi", "k_multiproof_layer", "k_multiproof_commit", "by the calls that exist",
                 "a finished session", "leaves nothing in the buffer"):
        assert word in section, word


def test_null_arguments_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    status = np.full(2, 0x5E5E5E5E, dtype=np.uint32)
    groups = np.array([[0, 1], [0, 1]], dtype=np.uint64)
    n_rows = ctypes.c_size_t(0x5E)
    assert L.cp2_blocks_verify_multi(None, CELL, BLOCK, 64, None, 0, groups.ctypes.data, 2, None, None, None, 0, status.ctypes.data, None) == CP2_ERR_INVALID
    assert L.cp2_dataset_block_multiproofs(None, groups.ctypes.data, 2, None, None, None, 0, ctypes.byref(n_rows)) == CP2_ERR_INVALID
    n_new = ctypes.c_size_t(0x5E)
    assert L.cp2_fill_add_multi(None, groups.ctypes.data, 2, None, None, None, 0, status.ctypes.data, ctypes.byref(n_new)) == CP2_ERR_INVALID
    assert (status == 0x5E5E5E5E).all() and n_rows.value == 0x5E and n_new.value == 0x5E


# ---- the product's plan, stand-alone under the sanitizers, against the model ---------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("multiproof_plan_check") / "multiproof_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "multiproof_plan_check.cpp")])
    return exe


def held(checker, path, cmds, want, what):
    open(path, "w").write("\n".join(cmds) + "\n")
    r = subprocess.run([checker, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, "%s:\n%s" % (what, (r.stdout + r.stderr)[-4000:])
    got, want = r.stdout.splitlines(), want + ["multiproof plan ok"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s, line %d:\n  the plan:  %s\n  the model: %s" % (what, i, g[:600], w[:600])
    assert len(got) == len(want), "%s: %d lines, the model has %d" % (what, len(got), len(want))


def test_the_plans_layouts_agree_with_the_model(checker, tmp_path):
    rng = np.random.default_rng(0x40)
    pairs = [(n, B) for n, B, _ in LITERALS] + [(n, B) for n in list(range(1, 11)) + RANDOM_BLOCKS for B in subsets(rng, n, 20)]
    held(checker, str(tmp_path / "layouts.txt"), [M.layout_cmd(n, B) for n, B in pairs], [M.layout_line(n, B) for n, B in pairs], "layouts")
    held(checker, str(tmp_path / "bad.txt"), [M.layout_cmd(5, [1, 1]), M.layout_cmd(5, [5]), M.layout_cmd(5, [])], ["layout refused"] * 3, "refused lists")


def test_the_plans_tables_agree_with_the_model(checker, tmp_path):
    rng = np.random.default_rng(0x41)
    calls = [c.groups for c in M.cases() if sum(len(B) for _, B in c.groups) < 3000]
    for _ in range(20):
        calls.append([(int(n), next(subsets(rng, int(n), 1))) for n in rng.choice(RANDOM_BLOCKS + [1, 2, 3, 5], size=int(rng.integers(1, 9)))])
    cmds, want = [], []
    for groups in calls:
        cmds.append(M.plan_cmd(groups))
        want += M.plan_lines(groups)
    held(checker, str(tmp_path / "plans.txt"), cmds, want, "plans")


def test_every_refusal_in_its_order_with_its_index(checker, tmp_path):
    n_blocks, good = 9, ([(3, 2), (4, 1), (3, 3)], [0, 8, 5, 1, 2, 7])
    rows = sum(len(M.layout(n_blocks, b)) for b in ([0, 8], [5], [1, 2, 7]))
    sets = [  # (groups, blocks, n_rows, the word the refusal must hold); every later rule is broken too, in a LOWER group: the order decides
        (good[0], good[1], rows, None),
        ([(3, 2), (4, 0), (9, 3)], [0, 9, 1, 1, 7], rows, "group 1 holds no block"),
        ([(9, 2), (2, 1), (3, 3)], [9, 8, 5, 1, 1, 7], rows, "group 0: root_index 9"),
        ([(3, 2), (4, 1), (1, 3)], [0, 8, 5, 1, 1, 7], rows, "group 2: root_index 1 is not inside the range 3 + 3"),
        ([(3, 2), (4, 1), (3, 3)], [8, 8, 5, 1, 9, 7], rows, "group 2, request 4: block 9"),
        ([(3, 2), (4, 1), (3, 3)], [0, 8, 5, 2, 2, 7], rows + 1, "group 2, request 4: block 2 does not ascend from 2"),
        ([(3, 2), (4, 1), (3, 3)], [0, 8, 5, 7, 2, 1], rows, "group 2, request 4: block 2 does not ascend from 7"),
        (good[0], good[1], rows + 1, "n_rows = %d, the groups' layouts hold %d rows" % (rows + 1, rows)),
        (good[0], good[1], None, None),
    ]
    cmds = [M.validate_cmd("verify", "root_index", g, b, 3, 3, n_blocks, r) for g, b, r, _ in sets]
    want = [M.validate_line("verify", "root_index", g, b, 3, 3, n_blocks, r) for g, b, r, _ in sets]
    for (g, b, r, word), line in zip(sets, want):
        assert (line.startswith("ok rows %d" % rows)) if word is None else (line.startswith("refused verify: ") and word in line), line
    held(checker, str(tmp_path / "refusals.txt"), cmds, want, "refusals")


def test_the_row_limit_through_synthetic_counts(checker, tmp_path):
    lim = M.ROW_LIMIT
    fits = [(0, 0), (0, lim - 1), (0, lim), (lim - 1, 0), (lim - 1, 1), (lim, 0), (lim - 2, 1), (1 << 40, 1), (5, (1 << 64) - 1), (lim - 10, 9), (lim - 10, 10)]
    cmds = ["fit %d %d" % f for f in fits] + ["counts 1 %d" % lim, "counts 2 %d %d" % (lim - 2, 2), "counts 3 1 %d 7" % ((1 << 64) - 1)]
    want = ["fit %d" % int(M.rows_fit(*f)) for f in fits] + [M.LIMIT_TEXT] * 3
    assert [int(M.rows_fit(*f)) for f in fits] == [1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0]     # rows + more stays below 2^32 - 1
    held(checker, str(tmp_path / "limit.txt"), cmds, want, "the row limit")


def test_mark_proved_multi_sets_the_bits_of_whole_paths_and_the_commit_list_is_the_models(checker, tmp_path):
    rng = np.random.default_rng(0x42)
    cmds, want = [], []
    for n_blocks in (1, 2, 3, 5, 8, 9, 33, 64, 65):
        for _ in range(6):
            first, n_local = int(rng.integers(0, 5)), int(rng.integers(1, 5))
            groups = [(first + int(rng.integers(0, n_local)), int(rng.integers(0, 3) == 0), next(subsets(rng, n_blocks, 1))) for _ in range(int(rng.integers(1, 7)))]
            cmds.append(M.mark_cmd(n_blocks, first, n_local, groups))
            want += M.mark_lines(n_blocks, first, n_local, groups)
    held(checker, str(tmp_path / "marks.txt"), cmds, want, "mark_proved_multi and the commit list")
