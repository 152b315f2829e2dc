"""CPU checks of the fill sessions: cp2_fill_begin, cp2_fill_add, cp2_fill_missing, cp2_fill_finish and cp2_fill_free are exported and carry
the same signature in the header, the ctypes binding and the Nim binding, the library's exports still equal what the header declares, the
CP2_FILL_* constants agree between header and binding, NULL handles are refused without touching a device or the outputs, and the host
logic (csrc/fill_plan.hpp) holds under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
CP2_ERR_INVALID = -1
# what the header must say, in the classes of tests/nim_api.py: the session handle is an untyped pointer (cp2_fill is void)
WANT = {
    "cp2_fill_begin": ("i32", ["handle:ctx", "ptr(config)", "u64", "u64", "ptr(u8)", "ptr(ptr(void))"]),
    "cp2_fill_add": ("i32", ["ptr(void)", "ptr(u64)", "ptr(u8)", "ptr(u8)", "usize", "ptr(u32)", "ptr(usize)"]),
    "cp2_fill_missing": ("i32", ["ptr(void)", "ptr(u64)", "usize", "ptr(u64)"]),
    "cp2_fill_finish": ("i32", ["ptr(void)", "cstr", "ptr(handle:dataset)"]),
    "cp2_fill_free": ("void", ["ptr(void)"]),
}


def test_the_five_names_match_in_header_nim_and_ctypes(pkg):
    protos = N.header_prototypes(HEADER)
    procs = N.nim_importc(open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read())
    L = pkg.load_library()
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    pvp = ctypes.POINTER(vp)
    # every pointer to bytes, words or a handle travels as a void pointer in the ctypes binding; out-parameters of one scalar are typed
    width = {"handle:ctx": vp, "ptr(void)": vp, "ptr(u8)": vp, "ptr(u64)": vp, "ptr(u32)": vp, "usize": sz, "u64": u64, "cstr": ctypes.c_char_p,
             "ptr(config)": ctypes.POINTER(pkg.Config), "ptr(ptr(void))": pvp, "ptr(handle:dataset)": pvp, "ptr(usize)": ctypes.POINTER(sz)}
    for name, (ret, args) in WANT.items():
        assert protos[name] == (ret, args), name
        assert procs[name] == (ret, args), name
        f = getattr(L, name)
        assert f.restype is (ctypes.c_int if ret == "i32" else None), name
        got = list(f.argtypes)
        assert len(got) == len(args), name
        for i, (g, a) in enumerate(zip(got, args)):
            if name == "cp2_fill_missing" and i == 3:
                assert g is ctypes.POINTER(u64)                    # n_missing: one uint64 out
            else:
                assert g is width[a], (name, i, g, a)
    assert re.search(r"typedef void cp2_fill;", HEADER)


def test_exports_equal_the_header_and_the_abi_minor_stays(pkg):
    L = pkg.load_library()
    names = pkg.exported_symbols()
    assert set(WANT) <= set(names) and set(names) == set(L._cp2_signatures)
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("cp2_")}
    assert exported == set(names), exported ^ set(names)
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER) and pkg.ABI_VERSION_MINOR == 2
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    for name in WANT:
        assert name in history, name


def test_fill_constants_match_the_header(pkg):
    got = {k: int(v) for k, v in re.findall(r"#define CP2_FILL_(\w+)\s+(\d+)", HEADER)}
    assert got == {"NEW": pkg.FILL_NEW, "MISMATCH": pkg.FILL_MISMATCH, "DUPLICATE": pkg.FILL_DUPLICATE, "UNWRITTEN": pkg.FILL_UNWRITTEN}
    assert got == {"NEW": 0, "MISMATCH": 1, "DUPLICATE": 2, "UNWRITTEN": 3}
    for word in ("cp2_multi", "resum", "already on disk", "erasure"):      # the header says what a session does not do
        assert word in HEADER[HEADER.index("fill sessions:"):HEADER.index("typedef void cp2_fill;")], word


def test_null_handles_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    sb = (ctypes.c_uint64 * 2)(0, 0)
    data = (ctypes.c_uint8 * 256)()
    paths = (ctypes.c_uint8 * 64)(*([9] * 64))
    status = (ctypes.c_uint32 * 2)(7, 7)
    new = ctypes.c_size_t(99)
    missing = (ctypes.c_uint64 * 2)(5, 5)
    n_missing = ctypes.c_uint64(42)
    out = ctypes.c_void_p(1234)
    cfg = pkg.make_config()
    assert L.cp2_fill_begin(None, ctypes.byref(cfg), 0, 11, data, ctypes.byref(out)) == CP2_ERR_INVALID and out.value == 1234
    assert L.cp2_fill_add(None, sb, data, paths, 1, status, ctypes.byref(new)) == CP2_ERR_INVALID
    assert L.cp2_fill_add(None, None, None, None, 0, None, None) == CP2_ERR_INVALID
    assert L.cp2_fill_missing(None, missing, 1, ctypes.byref(n_missing)) == CP2_ERR_INVALID
    assert L.cp2_fill_finish(None, None, ctypes.byref(out)) == CP2_ERR_INVALID and out.value == 1234
    L.cp2_fill_free(None)
    assert list(status) == [7, 7] and new.value == 99 and list(missing) == [5, 5] and n_missing.value == 42


def test_fill_plan_with_sanitizers(tmp_path):
    """csrc/fill_plan.hpp over 2000 random sessions: the compact layout and the destination rows against a brute-force layout, refusals
    naming the lowest offending request, NEW / DUPLICATE against a map walked in index order, the UNWRITTEN roll-back, the bitmap and the
    ordered, capped and counting missing list against a set, the finish precondition with its count and first pair."""
    exe = str(tmp_path / "fill_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "fill_plan_check.cpp")])
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fill plan ok" in r.stdout and ", 0 failures" in r.stdout, r.stdout
