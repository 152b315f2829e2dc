"""CPU checks of the block repair: cp2_dataset_repair_blocks and cp2_multi_dataset_repair_blocks are exported, carry Python signatures
and a Nim binding, the CP2_REPAIR_* constants agree between header and binding, NULL handles are refused without touching a device or
the outputs, and the host logic (csrc/repair_plan.hpp) holds under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
NAMES = ("cp2_dataset_repair_blocks", "cp2_multi_dataset_repair_blocks")
CP2_ERR_INVALID = -1


def test_repair_symbols_are_exported_with_python_signatures_and_nim_lines(pkg):
    L = pkg.load_library()
    nim = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
    for name in NAMES:
        assert name in pkg.exported_symbols()
        assert name in L._cp2_signatures
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == 8
        assert re.search(r"proc %s\(" % name, nim), name


def test_repair_constants_match_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define CP2_REPAIR_(\w+)\s+(\d+)", header)}
    assert got == {"CHECK_ONLY": pkg.REPAIR_CHECK_ONLY, "MATCH": pkg.REPAIR_MATCH, "MISMATCH": pkg.REPAIR_MISMATCH,
                   "UNWRITTEN": pkg.REPAIR_UNWRITTEN} == {"CHECK_ONLY": 1, "MATCH": 0, "MISMATCH": 1, "UNWRITTEN": 2}


def test_null_handles_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    sb = (ctypes.c_uint64 * 2)(0, 0)
    data = (ctypes.c_uint8 * 256)()
    status = (ctypes.c_uint32 * 2)(7, 7)
    written = ctypes.c_size_t(99)
    for name in NAMES:
        fn = getattr(L, name)
        assert fn(None, sb, data, 1, 0, None, status, ctypes.byref(written)) == CP2_ERR_INVALID
        assert fn(None, sb, data, 1, 1, b"/nonexistent/cache", status, ctypes.byref(written)) == CP2_ERR_INVALID
        assert fn(None, None, None, 0, 0, None, None, None) == CP2_ERR_INVALID
        assert list(status) == [7, 7] and written.value == 99


def test_repair_plan_with_sanitizers(tmp_path):
    """csrc/repair_plan.hpp, the header repair.cpp and multi_gpu.cpp use, over 20000 random request sets: duplicates and ranges caught
    with the right index named, kept rows equal to the layouts restated, every matched block in exactly one write group in ascending
    order, unit routing covering every block once, and only stamps that were valid before the call restamped."""
    exe = str(tmp_path / "repair_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "repair_plan_check.cpp")])
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "repair plan ok" in r.stdout and ", 0 failures" in r.stdout, r.stdout
