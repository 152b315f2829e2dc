"""CPU checks of the scrub boundary: cp2_dataset_scrub and cp2_multi_dataset_scrub are exported, carry Python signatures and a Nim
binding, the CP2_SCRUB_* constants agree between header and binding, and NULL handles are refused without touching a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
NAMES = ("cp2_dataset_scrub", "cp2_multi_dataset_scrub")
CP2_ERR_INVALID = -1


def test_scrub_symbols_are_exported_with_python_signatures_and_nim_lines(pkg):
    L = pkg.load_library()
    nim = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
    for name in NAMES:
        assert name in pkg.exported_symbols()
        assert name in L._cp2_signatures
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == 7
        assert re.search(r"proc %s\(" % name, nim), name


def test_scrub_constants_match_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define CP2_SCRUB_(\w+)\s+(\d+)", header)}
    assert got == {"SLOT": pkg.SCRUB_SLOT, "BLOCK": pkg.SCRUB_BLOCK, "CELL": pkg.SCRUB_CELL} == {"SLOT": 0, "BLOCK": 1, "CELL": 2}


def test_null_handles_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    bad = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    n, g = ctypes.c_size_t(99), ctypes.c_int(42)
    for name in NAMES:
        fn = getattr(L, name)
        assert fn(None, 0, 0, bad, 2, ctypes.byref(n), ctypes.byref(g)) == CP2_ERR_INVALID
        assert fn(None, 0, 0, None, 0, ctypes.byref(n), ctypes.byref(g)) == CP2_ERR_INVALID
        assert fn(None, 0, 0, None, 0, None, None) == CP2_ERR_INVALID
        assert list(bad) == [7, 7, 7, 7] and n.value == 99 and g.value == 42
