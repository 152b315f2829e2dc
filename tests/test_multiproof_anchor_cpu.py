"""CPU checks of multiproofs against what a fill session knows: the want list (the model of tests/multiproof_anchor_models.py) against the
issue's literals and against its independent restatement, exhaustively up to 6 blocks and seeded above; with only the root known the
plan of tests/multiproof_models.py (its `last` bits and its root rows apart: the verdicts come from the tops, and a top is never
committed); with everything known no rows and no jobs; a model fill whose state after every group is that of add_anchored at the lowest
anchors and which receives at most nBlocks - 1 rows; the model's verifier over C-oracle trees -- it reproduces every computed node, and the
group fails for any flipped leaf, sent row, kept input or kept top and any swap of two differing sent rows --; the condition on the
launcher test's cases; the names in the header, the Nim binding and the ctypes table; NULL arguments refused with outputs untouched; and
the product's host side (csrc/multiproof_anchor_plan.hpp), compiled with its own main under AddressSanitizer + UBSan and run as a
process, against the model line by line."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import multiproof_anchor_models as A
import multiproof_models as M
import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_ERR_INVALID = -1
NAMES = ("cp2_fill_multiproof_want", "cp2_dataset_block_tree_rows", "cp2_fill_block_tree_rows", "cp2_fill_add_multi_anchored")
SECTION = "---- multiproofs against what a fill session knows; tree rows served by place"
SEEDED = (7, 8, 9, 16, 33, 64, 257)
# (n_blocks, B, known below the root, want list, tops)
LITERALS = [
    (8, [0], {(0, 1)}, [(1, 1), (2, 1)], [(3, 0)]),
    (8, [0], {(1, 0)}, [(0, 1)], [(1, 0)]),
    (8, [0], {(0, 0)}, [], [(0, 0)]),
    (8, [0, 1, 2, 3], set(), [(2, 1)], [(3, 0)]),
    # odd layers: the last node of a layer of odd size has no sibling, neither sent nor kept
    (5, [4], set(), [(2, 0)], [(3, 0)]),
    (5, [4], {(2, 0)}, [], [(3, 0)]),
    (5, [3, 4], {(1, 2)}, [(0, 2), (1, 0), (2, 1)], [(1, 2), (3, 0)]),
    (7, [6], {(1, 2)}, [(2, 0)], [(3, 0)]),
    (7, [5, 6], {(2, 0)}, [(0, 4)], [(3, 0)]),
    (9, [8], {(3, 0)}, [], [(4, 0)]),
    (9, [0, 8], {(3, 0)}, [(0, 1), (1, 1), (2, 1)], [(3, 0), (4, 0)]),
    (9, [8], {(1, 4)}, [], [(1, 4)]),
]


def subsets(rng, n, count):
    for _ in range(count):
        k = int(rng.integers(1, n + 1))
        yield sorted(int(x) for x in rng.choice(n, size=k, replace=False))


def places(n):
    return [(l, i) for l, m in enumerate(M.layer_sizes(n)[:-1]) for i in range(m)]


# ---- the want list --------------------------------------------------------------------------------------------------------------------------
def test_the_models_want_list_holds_the_literals():
    for n, B, known, rows, tops in LITERALS:
        sent, _, got_tops, _ = A.walk(n, B, known)
        assert sent == rows and got_tops == tops, (n, B, known, sent, got_tops)


def test_the_want_list_against_the_restatement_exhaustively_up_to_six_blocks():
    for n in range(1, 7):
        pl = places(n)
        for mask in range(1 << len(pl)):
            known = {p for j, p in enumerate(pl) if mask >> j & 1}
            for k in range(1, n + 1):
                for B in itertools.combinations(range(n), k):
                    assert A.want(n, list(B), known) == A.restated(n, B, known), (n, B, known)


def test_the_want_list_against_the_restatement_seeded():
    rng = np.random.default_rng(0x51)
    for n in SEEDED:
        for t in range(120):
            known = A.random_known(rng, n, (0.05, 0.3, 0.7)[t % 3]) if t % 4 else A.derive(n, next(subsets(rng, n, 1)))
            B = next(subsets(rng, n, 1))
            got = A.want(n, B, known)
            assert got == A.restated(n, B, known) and got == sorted(got), (n, B)
            assert not set(got) & known


def test_with_only_the_root_known_it_is_the_multiproof_plan():
    rng = np.random.default_rng(0x52)
    calls = [c.groups for c in M.cases() if sum(len(B) for _, B in c.groups) < 3000]
    for _ in range(20):
        calls.append([(int(n), next(subsets(rng, int(n), 1))) for n in rng.choice(list(SEEDED) + [1, 2, 3, 5], size=int(rng.integers(1, 9)))])
    for groups in calls:
        m, a = M.Plan(groups), A.Plan([(n, B, set()) for n, B in groups])
        for g, (n, B) in enumerate(groups):
            assert A.want(n, B, set()) == M.layout(n, B)
        assert (a.n, a.n_rows, a.n_kept, a.n_work, a.level_base, a.level_off, a.node) == (m.n, m.n_rows, 0, m.n_work, m.level_base, m.level_off, m.node)
        # no job compares: the verdicts come from the tops, one per group, the row multiproof_plan's `last` job writes
        assert a.jobs == [[(left, right, kl & 0xFF, g) for left, right, kl, g in jobs] for jobs in m.jobs]
        assert [(r, g) for r, g, _, _ in a.tops] == [(m.top[g], g) for g in range(len(groups))] and a.top_off == list(range(len(groups) + 1))
        assert all((l, i) == (M.depth(groups[g][0]), 0) for _, g, l, i in a.tops)
        # ... and a top is never committed: multiproof_plan's commit list (every row) without the roots
        assert a.commit == [r for r in range(m.n_work) if r not in m.top.values()]


def test_with_everything_known_there_is_nothing_to_send_or_hash():
    rng = np.random.default_rng(0x53)
    for n in (1, 2, 5, 8, 9, 33):
        for B in subsets(rng, n, 5):
            p = A.Plan([(n, B, set(places(n)))])
            assert p.n_rows == 0 and p.n_kept == 0 and p.computed() == 0 and p.commit == []
            assert [(l, i) for _, _, l, i in p.tops] == [(0, b) for b in B] and [r for r, _, _, _ in p.tops] == list(range(len(B)))


def test_a_model_fill_takes_at_most_n_minus_one_rows_and_equals_anchored_adds():
    rng = np.random.default_rng(0x54)
    for n in (8, 64, 33):
        for _ in range(6):
            order, known, rows, at = [int(x) for x in rng.permutation(n)], set(), 0, 0
            while at < n:
                k = int(rng.integers(1, max(2, n // 3)))
                B = sorted(order[at:at + k])
                at += k
                p = A.Plan([(n, B, known)])
                rows += p.n_rows
                left = p.left_known(0)
                assert not left & known                        # a row that was known is never written
                assert known | left == known | A.anchored_leaves(n, B, known), (n, B)
                known |= left
            assert rows <= n - 1, (n, rows)
            assert all((0, b) in known for b in range(n))
        assert A.Plan([(n, list(range(n)), set())]).n_rows == 0


# ---- the verifier over the oracle's trees ---------------------------------------------------------------------------------------------------
def tree_of(c_oracle, rng, n):
    leaves = np.zeros((n, 32), dtype=np.uint8)
    leaves[:, :31] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
    return c_oracle.merkle_tree(leaves)


def flipped(rng, row):
    bad = row.copy()
    bad[int(rng.integers(0, 31))] ^= 1 << int(rng.integers(0, 8))
    return bad


def test_the_verifier_reproduces_the_oracles_nodes_and_fails_for_every_corruption(oracle):
    c_oracle, _ = oracle
    rng = np.random.default_rng(0x55)
    seen = {"leaf": 0, "sent": 0, "kept": 0, "top": 0, "swap": 0}
    for n in (1, 2, 3, 5, 7, 8, 9, 16, 33):
        layers = tree_of(c_oracle, rng, n)
        root = layers[-1][0]
        for t in range(8):
            known = A.random_known(rng, n, (0.1, 0.3, 0.6)[t % 3]) if t % 2 else A.derive(n, next(subsets(rng, n, 1)))
            B = next(subsets(rng, n, 1))
            p = A.Plan([(n, B, known)])
            leaves, rows = [layers[0][b].copy() for b in B], [layers[l][i].copy() for l, i in A.want(n, B, known)]

            def run(leaves=leaves, rows=rows, patch=None, root=root):
                kept = lambda l, i: patch[1] if patch and patch[0] == (l, i) else layers[l][i]
                return A.verify(c_oracle.compress, n, B, known, leaves, rows, kept, root)

            ok, nodes = run()
            assert ok, (n, B, known)
            assert len(nodes) == p.computed()
            for (l, i), v in nodes.items():
                assert np.array_equal(v, layers[l][i]), (n, B, l, i)
            for j in range(len(leaves)):
                assert not run(leaves=leaves[:j] + [flipped(rng, leaves[j])] + leaves[j + 1:])[0], (n, B, "leaf", j)
                seen["leaf"] += 1
            for j in range(len(rows)):
                assert not run(rows=rows[:j] + [flipped(rng, rows[j])] + rows[j + 1:])[0], (n, B, "sent", j)
                seen["sent"] += 1
            for k in range(p.n_kept):
                l, i = p.node[p.kept_base + k][1:]
                assert not run(patch=((l, i), flipped(rng, layers[l][i])))[0], (n, B, "kept input", l, i)
                seen["kept"] += 1
            for _, _, l, i in p.tops:
                if l == M.depth(n):
                    assert not run(root=flipped(rng, root))[0]
                elif (l, i) not in {p.node[p.kept_base + k][1:] for k in range(p.n_kept)}:
                    assert not run(patch=((l, i), flipped(rng, layers[l][i])))[0], (n, B, "kept top", l, i)
                seen["top"] += 1
            for j, k in itertools.combinations(range(len(rows)), 2):
                if not np.array_equal(rows[j], rows[k]):
                    bad = list(rows)
                    bad[j], bad[k] = rows[k], rows[j]
                    assert not run(rows=bad)[0], (n, B, "swap", j, k)
                    seen["swap"] += 1
    assert all(v > 20 for v in seen.values()), seen


# ---- the launcher test's cases hold the issue's condition -----------------------------------------------------------------------------------
def test_the_launcher_cases_hold_the_condition_on_wrong_tops():
    cases = A.tops_cases()
    assert sorted({c.n_tops for c in cases}) == sorted(A.N_TOPS)
    for c in cases:
        assert len(c.levels) == c.n_tops and all(s > 0 for c_ in [c] for s in c_.sizes)
        if c.n_groups > 1:
            assert A.tops_condition(c), c.no
            assert any(s == 1 for s in c.sizes)
            level_sets = [set(c.levels[c.top_off[g]:c.top_off[g + 1]]) for g in range(c.n_groups)]
            assert any(s == {0} for g, s in enumerate(level_sets) if c.sizes[g] > 1) and any(len(s) >= 3 for s in level_sets)
            assert {k for k in c.wrong.values()} == set(A.WRONG_KINDS)
        if c.n_tops > 256:                               # a range that straddles a wave boundary and one that straddles a workgroup's
            spans = [(c.top_off[g], c.top_off[g + 1]) for g in range(c.n_groups)]
            assert any(a // 64 != (b - 1) // 64 for a, b in spans) and any(a // 256 != (b - 1) // 256 for a, b in spans)


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
    assert at > HEADER.index("int cp2_fill_add_multi(")
    section = HEADER[at:HEADER.index(";", HEADER.index("int cp2_fill_add_multi_anchored("))]
    got = {k: int(v) for k, v in re.findall(r"CP2_FILL_ROW_(\w+) = \((\d+)\)", section)}     # parenthesised, in an enum: no new #define
    assert "#define" not in section
    assert got == {"KNOWN": 0, "UNKNOWN": 1} and (pkg.FILL_ROW_KNOWN, pkg.FILL_ROW_UNKNOWN) == (0, 1)
    assert re.search(r"CP2_FILL_ROW_KNOWN\* = 0'u32", NIM) and re.search(r"CP2_FILL_ROW_UNKNOWN\* = 1'u32", NIM)
    for word in ("belongs to the GROUP", "KEPT INPUT", "never sent", "TOP", "always the full count", "Read-only", "CP2_TRACE", "all or nothing",
                 "AS IT STANDS NOW", "stale", "Out of scope", "cp2_multi", "k_multiproof_tops", "k_multiproof_fold", "k_multiproof_commit",
                 "nBlocks - 1", "a finished session", "never written", "zeros", "no device work"):
        assert word in section, word
    old = HEADER[HEADER.index("---- block multiproofs:"):at]
    assert "stop at anchors" not in old and "serving multiproofs from a fill session" not in old


def test_null_arguments_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    status = np.full(2, 0x5E5E5E5E, dtype=np.uint32)
    rows = np.full((2, 32), 0x5E, dtype=np.uint8)
    li = np.full((4, 2), 0x5E, dtype=np.uint64)
    groups = np.array([[0, 1], [0, 1]], dtype=np.uint64)
    pl = np.array([[0, 0, 0], [0, 1, 0]], dtype=np.uint64)
    n_rows, n_new = ctypes.c_size_t(0x5E), ctypes.c_size_t(0x5E)
    assert L.cp2_fill_multiproof_want(None, groups.ctypes.data, 2, None, li.ctypes.data, 4, ctypes.byref(n_rows), None) == CP2_ERR_INVALID
    assert L.cp2_dataset_block_tree_rows(None, pl.ctypes.data, 2, rows.ctypes.data) == CP2_ERR_INVALID
    assert L.cp2_fill_block_tree_rows(None, pl.ctypes.data, 2, status.ctypes.data, rows.ctypes.data) == CP2_ERR_INVALID
    assert L.cp2_fill_add_multi_anchored(None, groups.ctypes.data, 2, None, None, None, 0, status.ctypes.data, ctypes.byref(n_new)) == CP2_ERR_INVALID
    assert (status == 0x5E5E5E5E).all() and (rows == 0x5E).all() and (li == 0x5E).all() and n_rows.value == 0x5E and n_new.value == 0x5E


# ---- the product's plan, stand-alone under the sanitizers, against the model ---------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("multiproof_anchor_check") / "multiproof_anchor_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "multiproof_anchor_check.cpp")])
    return exe


def held(checker, path, cmds, want, what):
    open(path, "w").write("\n".join(cmds) + "\n")
    r = subprocess.run([checker, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, "%s:\n%s" % (what, (r.stdout + r.stderr)[-4000:])
    got, want = r.stdout.splitlines(), want + ["multiproof anchor plan ok"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s, line %d:\n  the plan:  %s\n  the model: %s" % (what, i, g[:600], w[:600])
    assert len(got) == len(want), "%s: %d lines, the model has %d" % (what, len(got), len(want))


def seeded_triples(rng, sizes, count):
    for n in sizes:
        for t in range(count):
            known = A.random_known(rng, n, (0.0, 0.1, 0.3, 0.7, 1.0)[t % 5]) if t % 3 else A.derive(n, next(subsets(rng, n, 1)))
            yield n, next(subsets(rng, n, 1)), known


def test_the_plans_want_lists_agree_with_the_model(checker, tmp_path):
    rng = np.random.default_rng(0x56)
    triples = [(n, B, k) for n, B, k, _, _ in LITERALS] + list(seeded_triples(rng, list(range(1, 11)) + list(SEEDED), 15))
    held(checker, str(tmp_path / "wants.txt"), [A.want_cmd(*t) for t in triples], [A.want_line(*t) for t in triples], "want lists")


def test_the_plans_tables_agree_with_the_model(checker, tmp_path):
    rng = np.random.default_rng(0x57)
    pool = list(seeded_triples(rng, [1, 2, 3, 5, 8, 9, 16, 33, 64, 257], 12))
    calls = [[t] for t in pool[:30]] + [[(n, B, k) for n, B, k, _, _ in LITERALS]]
    for _ in range(25):
        calls.append([pool[int(j)] for j in rng.integers(0, len(pool), size=int(rng.integers(2, 9)))])
    calls.append([(n, B, set()) for n, B in M.cases()[1].groups])
    cmds, want = [], []
    for groups in calls:
        cmds.append(A.plan_cmd(groups))
        want += A.plan_lines(groups)
    held(checker, str(tmp_path / "plans.txt"), cmds, want, "plans")


def validate_cmd(groups, blocks, first, n_local, n_blocks, n_rows, knowns):
    return "validate %d %d %d %d %d %s %d %s %s" % (first, n_local, n_blocks, -1 if n_rows is None else n_rows, len(groups),
                                                    " ".join("%d %d" % g for g in groups), len(blocks), " ".join(map(str, blocks)),
                                                    " ".join("%d %s" % (len(k), A.known_words(n_blocks, k)) for k in knowns))


def validate_line(groups, blocks, first, n_local, n_blocks, n_rows, knowns):
    call = "fill multi anchored"
    why = M.refusal(call, "slot", groups, blocks, first, n_local, n_blocks, None)
    if why is not None:
        return "refused " + why
    at, rows = 0, 0
    for (_, c), k in zip(groups, knowns):
        rows += len(A.want(n_blocks, blocks[at:at + c], k))
        at += c
    return "refused " + A.stale_text(call, n_rows, rows) if n_rows is not None and rows != n_rows else "ok rows %d" % rows


def test_every_refusal_in_its_order_with_its_index_and_the_stale_list(checker, tmp_path):
    n_blocks, good = 9, ([(3, 2), (4, 1), (3, 3)], [0, 8, 5, 1, 2, 7])
    knowns = [{(1, 0)}, set(), {(0, 3), (2, 1)}]
    rows = sum(len(A.want(n_blocks, b, k)) for b, k in zip(([0, 8], [5], [1, 2, 7]), knowns))
    before = sum(len(M.layout(n_blocks, b)) for b in ([0, 8], [5], [1, 2, 7]))
    assert rows < before                               # what a list made against an empty session would hold
    sets = [  # every later rule is broken too, in a LOWER group: the order decides
        (good[0], good[1], rows, None),
        ([(3, 2), (4, 0), (9, 3)], [0, 9, 1, 1, 7], rows, "group 1 holds no block"),
        ([(9, 2), (2, 1), (3, 3)], [9, 8, 5, 1, 1, 7], rows, "group 0: slot 9"),
        ([(3, 2), (4, 1), (1, 3)], [0, 8, 5, 1, 1, 7], rows, "group 2: slot 1 is not inside the range 3 + 3"),
        ([(3, 2), (4, 1), (3, 3)], [8, 8, 5, 1, 9, 7], rows, "group 2, request 4: block 9"),
        ([(3, 2), (4, 1), (3, 3)], [0, 8, 5, 2, 2, 7], rows + 1, "group 2, request 4: block 2 does not ascend from 2"),
        (good[0], good[1], before, "n_rows = %d, the groups' want lists against the session as it stands hold %d rows" % (before, rows)),
        (good[0], good[1], None, None),
    ]
    cmds = [validate_cmd(g, b, 3, 3, n_blocks, r, knowns) for g, b, r, _ in sets]
    want = [validate_line(g, b, 3, 3, n_blocks, r, knowns) for g, b, r, _ in sets]
    for (g, b, r, word), line in zip(sets, want):
        assert (line == "ok rows %d" % rows) if word is None else (line.startswith("refused fill multi anchored: ") and word in line), line
    held(checker, str(tmp_path / "refusals.txt"), cmds, want, "refusals")
    pl = [("3 3 9 2 3 0 0 5 4 0", "ok"), ("3 3 9 2 3 0 0 6 0 0", "refused tree rows: request 1: slot 6 is not inside the local range 3 + 3"),
          ("3 3 9 2 2 0 0 3 5 0", "refused tree rows: request 0: slot 2 is not inside the local range 3 + 3"),
          ("3 3 9 1 3 5 0", "refused tree rows: request 0: level 5 is above the depth 4"),
          ("3 3 9 2 3 1 4 3 1 5", "refused tree rows: request 1: index 5 is not below the 5 node(s) of level 1")]
    held(checker, str(tmp_path / "places.txt"), ["places " + c for c, _ in pl], [w for _, w in pl], "places")


def test_the_row_limit_through_synthetic_counts(checker, tmp_path):
    lim = M.ROW_LIMIT
    cmds = ["counts 1 %d" % lim, "counts 2 %d %d" % (lim - 2, 2), "counts 3 1 %d 7" % ((1 << 64) - 1)]
    held(checker, str(tmp_path / "limit.txt"), cmds, [M.LIMIT_TEXT] * 3, "the row limit")


def test_mark_proved_multi_over_the_commit_list_sets_the_bits_of_anchored_adds(checker, tmp_path):
    rng = np.random.default_rng(0x58)
    cmds, want = [], []
    for n_blocks in (1, 2, 3, 5, 8, 9, 33, 64):
        for _ in range(4):
            first, n_local = int(rng.integers(0, 5)), int(rng.integers(1, 4))
            steps = [[(first + int(rng.integers(0, n_local)), int(rng.integers(0, 4) == 0), next(subsets(rng, n_blocks, 1))[:max(1, n_blocks // 3)])
                      for _ in range(int(rng.integers(1, 4)))] for _ in range(int(rng.integers(2, 7)))]
            cmds.append(A.fill_cmd(n_blocks, first, n_local, steps))
            want += A.fill_lines(n_blocks, first, n_local, steps)
    held(checker, str(tmp_path / "fills.txt"), cmds, want, "mark_proved_multi against mark_proved_anchored")
