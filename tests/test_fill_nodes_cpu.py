"""CPU checks of the fill sessions that serve: cp2_fill_keep_nodes and cp2_fill_block_proofs are exported and carry the same signature in
the header, the ctypes binding and the Nim binding, both stand in the header's `next:` list, the CP2_FILL_PROOF_* constants agree between
header and binding, NULL handles are refused without touching a device or the outputs, the Python models (tests/fill_nodes_models.py)
hold on small trees, and the host logic (csrc/fill_plan.hpp) holds under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

import fill_nodes_models as M
import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_OK, CP2_ERR_INVALID = 0, -1
WANT = {
    "cp2_fill_keep_nodes": ("i32", ["ptr(void)"]),
    "cp2_fill_block_proofs": ("i32", ["ptr(void)", "ptr(u64)", "usize", "ptr(u32)", "ptr(u8)", "ptr(u8)"]),
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
    width = {"ptr(void)": vp, "ptr(u64)": vp, "ptr(u32)": vp, "ptr(u8)": vp, "usize": sz}
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
    # the new section stands after the checkpoint section, which stands after the fill section
    assert (HEADER.index("void cp2_fill_free(") < HEADER.index("int cp2_fill_resume(") < HEADER.index("fill sessions that serve:") <
            HEADER.index("int cp2_fill_keep_nodes(") < HEADER.index("int cp2_fill_block_proofs(") < HEADER.index("cp2_write_circom_main("))


def test_proof_constants_match_the_header(pkg):
    got = {k: int(v) for k, v in re.findall(r"#define CP2_FILL_PROOF_(\w+)\s+\((\d+)\)", HEADER)}
    assert got == {"OK": pkg.FILL_PROOF_OK, "ABSENT": pkg.FILL_PROOF_ABSENT, "PARTIAL": pkg.FILL_PROOF_PARTIAL}
    assert got == {"OK": 0, "ABSENT": 1, "PARTIAL": 2} == {"OK": M.PROOF_OK, "ABSENT": M.PROOF_ABSENT, "PARTIAL": M.PROOF_PARTIAL}
    section = HEADER[HEADER.index("fill sessions that serve:"):HEADER.index("int cp2_fill_keep_nodes(")]
    assert all(HEADER.index("#define CP2_FILL_PROOF_" + k) > HEADER.index("fill sessions that serve:") for k in got)
    for word in ("cp2_multi", "k_block_path_commit_nodes", "UNWRITTEN", "Read-only", "Checkpoints stay"):
        assert word in section, word


def test_null_handles_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    sb = (ctypes.c_uint64 * 2)(0, 0)
    status = (ctypes.c_uint32 * 2)(7, 7)
    roots = (ctypes.c_uint8 * 32)(*([9] * 32))
    paths = (ctypes.c_uint8 * 64)(*([9] * 64))
    assert L.cp2_fill_keep_nodes(None) == CP2_ERR_INVALID
    assert L.cp2_fill_block_proofs(None, sb, 1, status, roots, paths) == CP2_ERR_INVALID
    assert L.cp2_fill_block_proofs(None, None, 0, None, None, None) == CP2_ERR_INVALID
    assert L.cp2_fill_block_proofs(None, sb, 1, status, None, None) == CP2_ERR_INVALID
    assert list(status) == [7, 7] and list(roots) == [9] * 32 and list(paths) == [9] * 64


def test_models_on_small_trees():
    """The models against each other and against the tree's shape: node_row is a bijection onto the rows, a proved request stores 2 depth +
    1 rows less the out-of-range siblings, the stored set holds every sibling row of the block's own proof, and the derivation of a complete
    session knows every row."""
    assert M.NODE_N_BLOCKS == tuple(range(1, 10)) + (16, 17)
    for n_blocks in range(1, 34):
        for n_local in (1, 3):
            sizes, offs, rows = M.layout(n_blocks, n_local)
            depth = len(sizes) - 1
            assert rows == n_local * sum(sizes) and sizes[0] == n_blocks and sizes[-1] == 1 and len(sizes) >= 2
            every = sorted(M.node_row(n_blocks, n_local, lvl, s, k) for lvl in range(depth + 1) for s in range(n_local) for k in range(sizes[lvl]))
            assert every == list(range(rows))
            s = n_local - 1
            for b in range(n_blocks):
                nodes = M.stored_nodes(n_blocks, b)
                out_of_range = sum(1 for lvl in range(depth) if ((b >> lvl) ^ 1) >= sizes[lvl])
                assert len(nodes) == 2 * depth + 1 - out_of_range == len(set(M.stored_rows(n_blocks, n_local, s, b)))
                assert (depth, 0) in [(lvl, idx) for lvl, idx, _ in nodes]                       # the slot root's own row
                assert {r for r in M.sibling_rows(n_blocks, n_local, s, b) if r is not None} <= set(M.stored_rows(n_blocks, n_local, s, b))
            full = M.Session(n_blocks, n_local)
            for s in range(n_local):
                for b in range(n_blocks):
                    full.add(s, b)
            assert not full.known
            full.keep_nodes()
            assert full.known == set(range(rows)) and all(full.servable(s, b) for s in range(n_local) for b in range(n_blocks))
    # turned on half way: what came before is PARTIAL until its neighbourhood arrives, what comes after is served at once
    half = M.Session(4, 1)
    half.add(0, 0)
    half.keep_nodes()
    assert half.status(0, 0) == M.PROOF_PARTIAL and half.status(0, 1) == M.PROOF_ABSENT
    half.add(0, 2)
    assert half.status(0, 2) == M.PROOF_OK and half.status(0, 0) == M.PROOF_PARTIAL      # block 2's path names node (1, 0) but not leaf 1
    half.add(0, 1)
    assert half.status(0, 0) == M.PROOF_OK and half.status(0, 1) == M.PROOF_OK
    half.add(0, 3, written=False)
    assert half.status(0, 3) == M.PROOF_ABSENT and half.status(0, 2) == M.PROOF_OK
    single = M.Session(1, 2)
    single.add(1, 0)
    single.keep_nodes()
    assert single.status(1, 0) == M.PROOF_OK and single.status(0, 0) == M.PROOF_ABSENT and M.sibling_rows(1, 2, 1, 0) == [None]


def test_fill_nodes_with_sanitizers(tmp_path):
    """csrc/fill_plan.hpp over 1000 random sessions: node_row against a brute-force layout, the known bits against a set of nodes, after
    every add servable(b) <=> present and every in-range sibling row of block_proof_rows known; a block added after keeping is servable at
    once, and a complete session serves every block after one derivation."""
    exe = str(tmp_path / "fill_nodes_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "fill_nodes_check.cpp")])
    r = subprocess.run([exe, "1000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fill nodes ok" in r.stdout and ", 0 failures" in r.stdout, r.stdout
