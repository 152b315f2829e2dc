"""CPU checks of the fill checkpoints: cp2_fill_save and cp2_fill_resume are exported and carry the same signature in the header, the ctypes
binding and the Nim binding, both stand in the header's `next:` list, CP2_RESUME_TRUST_FILES is 1 everywhere, NULL arguments are refused
without touching a device or the outputs, and the host logic (csrc/fill_checkpoint.hpp) holds under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_ERR_INVALID = -1
WANT = {
    "cp2_fill_save": ("i32", ["ptr(void)", "cstr"]),
    "cp2_fill_resume": ("i32", ["handle:ctx", "ptr(config)", "u64", "u64", "ptr(u8)", "cstr", "i32", "ptr(ptr(void))", "ptr(u64)"]),
}


def test_the_two_names_match_in_header_nim_and_ctypes(pkg):
    protos = N.header_prototypes(HEADER)
    procs = N.nim_importc(NIM)
    L = pkg.load_library()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    width = {"handle:ctx": vp, "ptr(void)": vp, "ptr(u8)": vp, "u64": u64, "i32": ctypes.c_int, "cstr": ctypes.c_char_p,
             "ptr(config)": ctypes.POINTER(pkg.Config), "ptr(ptr(void))": ctypes.POINTER(vp), "ptr(u64)": ctypes.POINTER(u64)}
    for name, (ret, args) in WANT.items():
        assert protos[name] == (ret, args), name
        assert procs[name] == (ret, args), name
        f = getattr(L, name)
        assert f.restype is ctypes.c_int, name
        assert [g for g in f.argtypes] == [width[a] for a in args], name
        assert L._cp2_signatures[name] == (ctypes.c_int, [width[a] for a in args]), name
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    for name in WANT:
        assert name in history, name
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER)
    # the new section stands after the fill section, and the fill section points to it
    assert HEADER.index("void cp2_fill_free(") < HEADER.index("fill checkpoints:") < HEADER.index("int cp2_fill_save(") < HEADER.index("cp2_write_circom_main(")
    assert "checkpoint section below" in HEADER[HEADER.index("fill sessions:"):HEADER.index("typedef void cp2_fill;")]


def test_the_flag_is_one_everywhere(pkg):
    assert [int(v) for v in re.findall(r"#define CP2_RESUME_TRUST_FILES\s+(\d+)", HEADER)] == [1]
    assert [int(v) for v in re.findall(r"CP2_RESUME_TRUST_FILES\*\s*=\s*(\d+)", NIM)] == [1]
    assert pkg.RESUME_TRUST_FILES == 1
    assert not re.findall(r"#define CP2_FILL_(?!NEW|MISMATCH|DUPLICATE|UNWRITTEN)\w+\s+\d+", HEADER)     # the statuses stay the four


def test_null_arguments_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    roots = (ctypes.c_uint8 * 64)()
    out = ctypes.c_void_p(1234)
    dropped = ctypes.c_uint64(42)
    cfg = pkg.make_config()
    fake_handle = ctypes.c_void_p(ctypes.addressof(roots))           # never dereferenced: the NULL beside it is refused first
    assert L.cp2_fill_save(None, b"/nonexistent/checkpoint") == CP2_ERR_INVALID
    assert L.cp2_fill_save(None, None) == CP2_ERR_INVALID
    assert not os.path.exists("/nonexistent")
    for args in ((None, ctypes.byref(cfg), 0, 2, roots, b"/nonexistent/checkpoint", 0, ctypes.byref(out), ctypes.byref(dropped)),
                 (None, ctypes.byref(cfg), 0, 2, roots, None, 0, ctypes.byref(out), ctypes.byref(dropped)),
                 (None, None, 0, 2, roots, b"/nonexistent/checkpoint", 1, ctypes.byref(out), ctypes.byref(dropped)),
                 (fake_handle, ctypes.byref(cfg), 0, 2, roots, b"/nonexistent/checkpoint", 0, None, ctypes.byref(dropped)),
                 (fake_handle, ctypes.byref(cfg), 0, 2, roots, None, 0, ctypes.byref(out), ctypes.byref(dropped)),
                 (fake_handle, None, 0, 2, roots, b"/nonexistent/checkpoint", 0, ctypes.byref(out), None)):
        assert L.cp2_fill_resume(*args) == CP2_ERR_INVALID
        assert out.value == 1234 and dropped.value == 42


def test_fill_checkpoint_with_sanitizers(tmp_path):
    """csrc/fill_checkpoint.hpp over 500 random sessions: the round trip (1 block per slot, bitmaps that are no multiple of 64 bits, empty and
    full sessions, absent rows zeroed), every truncation point and every flipped byte of a small file refused, each differing field named,
    short and missing files, the read plan (each present block once, ascending per file), FillPlan::restore and ::drop.  Then its two
    readers against real slot files in a scratch directory, 500 random geometries: the whole blocks each file holds (absent, empty, whole and
    ragged files, ENOTDIR as absence, ENAMETOOLONG as an error naming the file) and every chunk of a read plan byte for byte into a buffer
    of exactly a chunk; a file removed or replaced by a directory after the plan was made is an error naming the lowest such file and its
    errno, a file cut short reads as zeros past its end."""
    exe = str(tmp_path / "fill_checkpoint_check")
    scratch = tmp_path / "files"
    scratch.mkdir()
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "fill_checkpoint_check.cpp")])
    r = subprocess.run([exe, "500", str(scratch)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fill checkpoint ok" in r.stdout and ", 0 failures" in r.stdout, r.stdout
    assert list(scratch.iterdir()) == []
