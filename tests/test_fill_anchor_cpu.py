"""CPU checks of anchored fill adds: cp2_fill_anchors and cp2_fill_add_anchored are exported and carry the same signature in the header,
the ctypes binding and the Nim binding, both stand in the header's `next:` list, MINOR is still 2, the section stands where the issue puts
it and defines no new CP2_FILL_* constant, NULL handles are refused without touching a device or the outputs, the Python models
(tests/fill_anchor_models.py) hold on small trees, and the host logic (csrc/fill_plan.hpp) holds under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np

import fill_anchor_models as A
import fill_nodes_models as M
import kernel_models as K
import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_OK, CP2_ERR_INVALID = 0, -1
WANT = {
    "cp2_fill_anchors": ("i32", ["ptr(void)", "ptr(u64)", "usize", "ptr(u32)"]),
    "cp2_fill_add_anchored": ("i32", ["ptr(void)", "ptr(u64)", "ptr(u8)", "ptr(u32)", "ptr(u8)", "usize", "ptr(u32)", "ptr(usize)"]),
}


def test_the_library_exports_both_names(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert set(WANT) <= exported, set(WANT) - exported
    assert set(pkg.exported_symbols()) == {n for n in exported if n.startswith("cp2_")} == set(pkg.load_library()._cp2_signatures)


def test_the_two_names_match_in_header_nim_and_ctypes(pkg):
    protos = N.header_prototypes(HEADER)
    procs = N.nim_importc(NIM)
    L = pkg.load_library()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    width = {"ptr(void)": vp, "ptr(u64)": vp, "ptr(u32)": vp, "ptr(u8)": vp, "usize": sz, "ptr(usize)": ctypes.POINTER(sz)}
    for name, (ret, args) in WANT.items():
        assert protos[name] == (ret, args), name
        assert procs[name] == (ret, args), name
        f = getattr(L, name)
        assert f.restype is ctypes.c_int, name
        assert list(f.argtypes) == [width[a] for a in args], name
        assert L._cp2_signatures[name] == (ctypes.c_int, [width[a] for a in args]), name
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    for name in WANT:
        assert name in history, name
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER) and pkg.ABI_VERSION_MINOR == 2


def test_the_section_stands_where_it_belongs_and_defines_no_status():
    assert (HEADER.index("int cp2_fill_block_proofs(") < HEADER.index("anchored fill adds:") < HEADER.index("int cp2_fill_anchors(") <
            HEADER.index("int cp2_fill_add_anchored(") < HEADER.index("cp2_write_circom_main("))
    section = HEADER[HEADER.index("anchored fill adds:"):HEADER.index("cp2_write_circom_main(")]
    assert "#define" not in section
    # the statuses stay the four bare numbers of cp2_fill_add and the three parenthesised ones of cp2_fill_block_proofs
    assert sorted(re.findall(r"#define (CP2_FILL_\w+)", HEADER)) == sorted(
        ["CP2_FILL_NEW", "CP2_FILL_MISMATCH", "CP2_FILL_DUPLICATE", "CP2_FILL_UNWRITTEN", "CP2_FILL_PROOF_OK", "CP2_FILL_PROOF_ABSENT", "CP2_FILL_PROOF_PARTIAL"])
    for word in ("cp2_multi", "k_block_path_commit_anchored", "UNWRITTEN", "WHEN THE CALL STARTED", "adopting blocks from disk", "what is served",
                 "checkpointing the known siblings"):
        assert word in section, word


def test_null_handles_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    sb = (ctypes.c_uint64 * 2)(0, 0)
    levels = (ctypes.c_uint32 * 2)(7, 7)
    status = (ctypes.c_uint32 * 2)(7, 7)
    data = (ctypes.c_uint8 * 64)(*([9] * 64))
    paths = (ctypes.c_uint8 * 64)(*([9] * 64))
    n_new = ctypes.c_size_t(5)
    assert L.cp2_fill_anchors(None, sb, 1, levels) == CP2_ERR_INVALID
    assert L.cp2_fill_anchors(None, None, 0, None) == CP2_ERR_INVALID
    assert L.cp2_fill_add_anchored(None, sb, data, levels, paths, 1, status, ctypes.byref(n_new)) == CP2_ERR_INVALID
    assert L.cp2_fill_add_anchored(None, None, None, None, None, 0, None, None) == CP2_ERR_INVALID
    assert list(levels) == [7, 7] and list(status) == [7, 7] and n_new.value == 5 and list(paths) == [9] * 64 and list(data) == [9] * 64


def test_models_on_small_trees():
    """anchor_level over a known-set, the stored set of an anchored request and the sibling count of a whole slot, against the tree's shape
    and against the models of whole paths (tests/fill_nodes_models.py)."""
    assert A.ANCHOR_N_BLOCKS == (1, 2, 3, 5, 6, 8, 13)
    rng = np.random.default_rng(0xA2C)
    for n_blocks in range(1, 34):
        depth = A.depth_of(n_blocks)
        sizes = K.layer_sizes(n_blocks)
        for n_local in (1, 3):
            s = n_local - 1
            for b in range(n_blocks):
                # level depth: a whole path less the slot root's own row; level 0: nothing; each set inside the next
                whole = set(M.stored_rows(n_blocks, n_local, s, b))
                top = M.node_row(n_blocks, n_local, depth, s, 0)
                assert set(A.stored_rows(n_blocks, n_local, s, b, depth)) == whole - {top}
                assert A.stored_rows(n_blocks, n_local, s, b, 0) == []
                for lvl in range(depth + 1):
                    rows = set(A.stored_rows(n_blocks, n_local, s, b, lvl))
                    chain = {M.node_row(n_blocks, n_local, up, s, b >> up) for up in range(lvl, depth + 1)}
                    assert not rows & chain                                                  # never the anchor, never a row above it
                    assert lvl == depth or rows <= set(A.stored_rows(n_blocks, n_local, s, b, lvl + 1))
                    in_range = sum(1 for low in range(lvl) if ((b >> low) ^ 1) < sizes[low])
                    assert len(rows) == (0 if lvl == 0 else 1 + in_range + lvl - 1)
                assert A.anchor_row(n_blocks, n_local, s, b, depth) is None
        # an empty keeping session anchors everything at the slot root; a plain one too, whatever it holds
        empty = A.Session(n_blocks, 2)
        assert all(empty.anchor(1, b) == depth for b in range(n_blocks))
        empty.keep_nodes()
        assert all(empty.anchor(1, b) == depth for b in range(n_blocks))
        assert not empty.accepts(0, 0, depth + 1) and empty.accepts(0, 0, depth) and (depth == 0 or not empty.accepts(0, 0, 0))
        # a whole slot at lowest anchors in a shuffled order
        total, full = A.fill_with_lowest_anchors(n_blocks, [int(b) for b in rng.permutation(n_blocks)])
        if n_blocks == 1:
            assert total == 1                            # the one round of the one-block slot, against a zero that has no row
        elif n_blocks & (n_blocks - 1) == 0:
            assert total == n_blocks - 1
        else:
            assert n_blocks - 1 <= total <= n_blocks - 1 + depth
        assert all(full.servable(0, b) and full.anchor(0, b) == 0 for b in range(n_blocks))
    # pinned: four blocks; block 2's whole path makes leaf 3 and node (1, 0) known, so 3 needs nothing and 0 needs one sibling
    four = A.Session(4, 1)
    four.keep_nodes()
    assert [four.anchor(0, b) for b in range(4)] == [2, 2, 2, 2]
    four.add_anchored(0, 2, 2)
    assert [four.anchor(0, b) for b in range(4)] == [1, 1, 0, 0]
    assert not four.accepts(0, 0, 0) and four.accepts(0, 0, 1) and four.accepts(0, 0, 2)
    four.add_anchored(0, 3, 0)
    four.add_anchored(0, 0, 1)
    assert [four.anchor(0, b) for b in range(4)] == [0, 0, 0, 0] and four.status(0, 1) == M.PROOF_ABSENT
    four.add_anchored(0, 1, 0, written=False)
    assert four.status(0, 1) == M.PROOF_ABSENT and all(four.status(0, b) == M.PROOF_OK for b in (0, 2, 3))


def test_the_anchored_walk_is_a_prefix_of_the_whole_walk(oracle):
    """On the oracle's trees: the walk over the lowest `level` siblings reaches the tree's node at that level, for every block and level."""
    C, _ = oracle
    rng = np.random.default_rng(0xA2D)
    for n_blocks in A.ANCHOR_N_BLOCKS:
        leaves = rng.integers(0, 256, size=(n_blocks, 32), dtype=np.uint8)
        leaves[:, 31] &= 0x1F
        tree = C.merkle_tree(leaves)
        depth = len(tree) - 1
        assert depth == A.depth_of(n_blocks)
        for b in range(n_blocks):
            path = [tree[lvl][(b >> lvl) ^ 1] if ((b >> lvl) ^ 1) < len(tree[lvl]) else np.zeros(32, np.uint8) for lvl in range(depth)]
            for level in range(depth + 1):
                assert np.array_equal(A.walk(tree[0][b], b, n_blocks, path[:level], C.compress), tree[level][b >> level]), (n_blocks, b, level)


def test_fill_anchor_with_sanitizers(tmp_path):
    """csrc/fill_plan.hpp over 1000 random sessions: anchor_level, validate_anchored, the device tables and mark_proved_anchored against
    brute force, with the invariants tests/host_check/fill_anchor_check.cpp names."""
    exe = str(tmp_path / "fill_anchor_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "fill_anchor_check.cpp")])
    r = subprocess.run([exe, "1000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fill anchor ok" in r.stdout and ", 0 failures" in r.stdout, r.stdout
