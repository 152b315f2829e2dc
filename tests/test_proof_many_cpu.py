"""CPU checks of the proof-inputs-across-datasets boundary (ABI 1.2): the two entry points are exported, carry Python signatures and a
Nim binding, and refuse what they must without touching a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
NAMES = ("cp2_proof_inputs_generate_many", "cp2_proof_inputs_export_many")
CP2_ERR_INVALID = -1


def test_new_symbols_are_exported_with_python_signatures(pkg):
    L = pkg.load_library()
    for name in NAMES:
        assert name in pkg.exported_symbols()
        assert name in L._cp2_signatures
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == {"cp2_proof_inputs_generate_many": 6, "cp2_proof_inputs_export_many": 9}[name]
    nim = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
    for name in NAMES:
        assert re.search(r"proc %s\(" % name, nim), name


def test_abi_version_is_1_2_everywhere(pkg):
    header = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
    assert "#define CP2_ABI_VERSION_MINOR 2" in header
    assert pkg.load_library().cp2_abi_version() == (1 << 16) | 2
    assert (pkg.ABI_VERSION_MAJOR, pkg.ABI_VERSION_MINOR) == (1, 2)
    nim = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
    assert re.search(r"abiVersionMinor\* = 2\b", nim)


def test_calls_without_a_context_are_refused(pkg):
    """No device here (or none used): a NULL context is CP2_ERR_INVALID, for n == 0 and with NULL arrays alike, and nothing crashes."""
    L = pkg.load_library()
    out = (ctypes.c_void_p * 2)(1, 1)
    slots = (ctypes.c_uint64 * 2)(0, 1)
    ent = (ctypes.c_uint8 * 64)()
    hs = (ctypes.c_void_p * 2)(None, None)
    assert L.cp2_proof_inputs_generate_many(None, None, None, None, 0, None) == CP2_ERR_INVALID
    assert L.cp2_proof_inputs_generate_many(None, hs, slots, ent, 2, out) == CP2_ERR_INVALID
    assert L.cp2_proof_inputs_generate_many(None, None, None, None, 2, None) == CP2_ERR_INVALID
    total = ctypes.c_uint64(5)
    assert L.cp2_proof_inputs_export_many(None, None, None, None, 0, None, 1, 0, ctypes.byref(total)) == CP2_ERR_INVALID
    assert L.cp2_proof_inputs_export_many(None, hs, slots, ent, 2, None, 4, 1, None) == CP2_ERR_INVALID
