"""CPU checks of the block proofs: cp2_block_proof_depth, cp2_dataset_block_proofs, cp2_blocks_verify and cp2_dataset_repair_blocks_proved
are exported, carry Python signatures and a Nim binding each, the CP2_BLOCK_* constants agree between header and binding, the proof depth
equals the length of the Python oracle's merkleProof, NULL handles are refused without touching a device or the outputs, and the host
logic (csrc/block_proof_plan.hpp) holds under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
ARITY = {"cp2_block_proof_depth": 3, "cp2_dataset_block_proofs": 5, "cp2_blocks_verify": 12, "cp2_dataset_repair_blocks_proved": 9}
CP2_ERR_INVALID = -1


def test_block_proof_symbols_are_exported_with_python_signatures_and_nim_lines(pkg):
    L = pkg.load_library()
    nim = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
    for name, arity in ARITY.items():
        assert name in pkg.exported_symbols()
        assert name in L._cp2_signatures
        f = getattr(L, name)
        assert f.restype is (ctypes.c_size_t if name == "cp2_block_proof_depth" else ctypes.c_int) and len(f.argtypes) == arity
        assert re.search(r"proc %s\(" % name, nim), name


def test_block_constants_match_the_header_and_the_abi_minor_stays(pkg):
    header = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define CP2_BLOCK_(\w+)\s+(\d+)", header)}
    assert got == {"MATCH": pkg.BLOCK_MATCH, "MISMATCH": pkg.BLOCK_MISMATCH} == {"MATCH": 0, "MISMATCH": 1}
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", header) and pkg.ABI_VERSION_MINOR == 2
    history = header[header.index("next:"):header.index("#define CP2_ABI_VERSION_MAJOR")]
    for name in ARITY:
        assert name in history, name


@pytest.mark.parametrize("n_blocks", [1, 2, 3, 5, 8, 128])
def test_depth_is_the_length_of_the_oracles_proof(pkg, oracle, n_blocks):
    """merkle_tree / merkle_proof of the Python oracle over n_blocks leaves: every leaf's path has cp2_block_proof_depth entries, the proof
    reconstructs the root and a changed leaf does not."""
    _, P = oracle
    cs, bs = 128, 4096
    layers = P.merkle_tree([1000 + 7 * i for i in range(n_blocks)])
    depth = pkg.block_proof_depth(cs, bs, n_blocks * (bs // cs))
    assert depth == len(layers) - 1 == pkg.load_library().cp2_merkle_num_layers(n_blocks) - 1
    for b in sorted({0, n_blocks // 2, n_blocks - 1}):
        prf = P.merkle_proof(layers, b)
        assert len(prf["merklePath"]) == depth
        assert P.reconstruct_root(prf) == layers[-1][0]
        assert P.reconstruct_root(dict(prf, leafValue=prf["leafValue"] + 1)) != layers[-1][0]
    if n_blocks == 1:
        assert P.merkle_proof(layers, 0)["merklePath"] == [0]
    if n_blocks == 5:                                             # layers 5-3-2-1: the last leaf's path is zero, zero, non-zero
        p = P.merkle_proof(layers, 4)["merklePath"]
        assert p[0] == 0 and p[1] == 0 and p[2] != 0


def test_depth_is_zero_for_refused_geometries(pkg):
    d = pkg.block_proof_depth
    assert d(2048, 65536, 4096) == 7 and d(2048, 65536, 1 << 22) == 17 and d(128, 4096, 32) == 1 and d(64, 64, 3) == 2
    for cs, bs, nc in ((0, 4096, 256), (128, 0, 256), (128, 4096, 0), (128, 4000, 256), (128, 4096, 250), (128, 4096, 33),
                       ((1 << 30) + 1, (1 << 30) + 1, 1), (128, 4096, (1 << 40) + 32)):
        assert d(cs, bs, nc) == 0, (cs, bs, nc)


def test_null_handles_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    sb = (ctypes.c_uint64 * 2)(0, 0)
    data = (ctypes.c_uint8 * 256)()
    roots = (ctypes.c_uint8 * 32)(*([9] * 32))
    paths = (ctypes.c_uint8 * 64)(*([9] * 64))
    status = (ctypes.c_uint32 * 2)(7, 7)
    written = ctypes.c_size_t(99)
    assert L.cp2_dataset_block_proofs(None, sb, 1, roots, paths) == CP2_ERR_INVALID
    assert L.cp2_dataset_block_proofs(None, None, 0, None, None) == CP2_ERR_INVALID
    assert L.cp2_blocks_verify(None, 64, 256, 64, roots, 1, sb, data, paths, 1, status, roots) == CP2_ERR_INVALID
    assert L.cp2_blocks_verify(None, 64, 256, 64, None, 0, None, None, None, 0, None, None) == CP2_ERR_INVALID
    fn = L.cp2_dataset_repair_blocks_proved
    assert fn(None, sb, data, paths, 1, 0, None, status, ctypes.byref(written)) == CP2_ERR_INVALID
    assert fn(None, sb, data, paths, 1, 1, b"/nonexistent/cache", status, ctypes.byref(written)) == CP2_ERR_INVALID
    assert fn(None, None, None, None, 0, 0, None, None, None) == CP2_ERR_INVALID
    assert list(status) == [7, 7] and written.value == 99 and list(roots) == [9] * 32 and list(paths) == [9] * 64


def test_block_proof_plan_with_sanitizers(tmp_path):
    """csrc/block_proof_plan.hpp over 20000 random geometries: depths, sibling rows of both kept layouts against a brute-force layout,
    absent rows exactly past a layer's end, the (right, key) schedule against a transcription of reconstructRoot, refusals naming the
    lowest offending request."""
    exe = str(tmp_path / "block_proof_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "block_proof_plan_check.cpp")])
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "block proof plan ok" in r.stdout and ", 0 failures" in r.stdout, r.stdout
