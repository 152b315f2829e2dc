"""CPU checks of adopting blocks from disk: cp2_fill_adopt is exported and carries the same signature in the header, the ctypes binding and
the Nim binding, stands in the header's `next:` list, MINOR is still 2, the section stands after the anchored adds and says what the issue
asks it to say, a NULL session is refused without touching a device or the outputs, the Python models (tests/fill_adopt_models.py) hold on
small trees, and the host logic (csrc/adopt_plan.hpp) holds under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

import fill_adopt_models as D
import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_ERR_INVALID = -1
WANT = {"cp2_fill_adopt": ("i32", ["ptr(void)", "u64", "u64", "i32", "ptr(u64)", "ptr(u64)"])}


def test_the_library_exports_the_name(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert set(WANT) <= exported, set(WANT) - exported
    assert set(pkg.exported_symbols()) == {n for n in exported if n.startswith("cp2_")} == set(pkg.load_library()._cp2_signatures)


def test_the_name_matches_in_header_nim_and_ctypes(pkg):
    protos = N.header_prototypes(HEADER)
    procs = N.nim_importc(NIM)
    L = pkg.load_library()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    width = {"ptr(void)": vp, "u64": u64, "i32": ctypes.c_int, "ptr(u64)": ctypes.POINTER(u64)}
    for name, (ret, args) in WANT.items():
        assert protos[name] == (ret, args), (name, protos[name])
        assert procs[name] == (ret, args), (name, procs[name])
        f = getattr(L, name)
        assert f.restype is ctypes.c_int, name
        assert list(f.argtypes) == [width[a] for a in args], name
        assert L._cp2_signatures[name] == (ctypes.c_int, [width[a] for a in args]), name
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    assert "cp2_fill_adopt" in history
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER) and pkg.ABI_VERSION_MINOR == 2
    assert re.search(r"#define CP2_ADOPT_NO_READ 1\b", HEADER) and pkg.ADOPT_NO_READ == 1 and "CP2_ADOPT_NO_READ* = 1.cint" in NIM


def test_the_section_stands_after_the_anchored_adds_and_says_what_it_must():
    # (after cp2_write_circom_main, which closes the anchored adds' section: that section defines nothing, and tests/test_fill_anchor_cpu.py says so)
    assert (HEADER.index("int cp2_fill_add_anchored(") < HEADER.index("cp2_write_circom_main(") < HEADER.index("adopting blocks from disk:") <
            HEADER.index("int cp2_fill_adopt(") < HEADER.index("every GPU of the node behind one handle"))
    section = HEADER[HEADER.index("adopting blocks from disk:"):HEADER.index("every GPU of the node behind one handle")]
    assert re.findall(r"#define (\w+)", section) == ["CP2_ADOPT_NO_READ"]
    for word in ("cp2_multi", "k_adopt_layer", "k_adopt_resolve", "TRUSTS THE FILES UNCHANGED SINCE THEY WERE READ", "fdatasync", "CP2_FILL_UNWRITTEN",
                 "a known row is never", "without a match", "checkpointing known siblings or candidates", "pipelining the reads", "CP2_ERR_HIP",
                 "CP2_TRACE", "absence is a state"):
        assert word in section, word


def test_a_null_session_is_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    read, adopted = ctypes.c_uint64(5), ctypes.c_uint64(6)
    assert L.cp2_fill_adopt(None, 0, 0, 0, ctypes.byref(read), ctypes.byref(adopted)) == CP2_ERR_INVALID
    assert L.cp2_fill_adopt(None, 0, 0, 1, None, None) == CP2_ERR_INVALID
    assert read.value == 5 and adopted.value == 6


def test_models_on_small_trees():
    """an intact slot is adopted whole from the stated root; with one damaged block and one proved path exactly the blocks under the
    siblings that do not hold the damage are adopted, and lowest anchors then complete the slot with the siblings the model counts"""
    for nb in (1, 2, 3, 4, 5, 8, 13, 64):
        s = D.Slot(nb)
        assert s.adopt(range(nb)) == list(range(nb)) and s.known >= set(range(s.rows - 1))
        assert D.Slot(nb).adopt(range(nb), damaged=[0]) == []                              # nothing vouches for less than the whole slot
        if nb & (nb - 1) or nb < 2:
            continue
        for bad in (0, nb - 1, nb // 2):
            for q in (b for b in (1, nb - 2, nb // 2 - 1) if 0 <= b < nb):
                if q == bad:
                    continue
                s = D.Slot(nb)
                assert s.adopt(range(nb), damaged=[bad]) == []
                siblings = s.add_path(q)
                got = s.adopt(range(nb), damaged=[bad])
                lvl_of_bad = max(lvl for lvl in range(s.depth) if (bad >> lvl) != (q >> lvl))
                want = [b for b in range(nb) if b != q and (b >> lvl_of_bad) != (bad >> lvl_of_bad)]
                assert got == want, (nb, bad, q, got, want)
                assert s.anchor(bad) == lvl_of_bad                                          # the damaged block needs the siblings below that node
                siblings += s.add_path(bad, s.anchor(bad))
                rest = [b for b in range(nb) if b not in s.present]
                assert s.adopt(rest, damaged=[]) == rest and len(s.present) == nb            # what lay beside it under that node is intact
                assert siblings == s.depth + lvl_of_bad
    # pinned: eight blocks, block 5 damaged, block 2 proved with its whole path: siblings are leaf 3, node (1, 0), node (2, 1)
    s = D.Slot(8)
    s.add_path(2)
    assert s.adopt(range(8), damaged=[5]) == [0, 1, 3] and s.anchor(5) == 2 and s.anchor(4) == 2
    s.add_path(5, 2)
    assert s.adopt(range(8)) == [4, 6, 7]


def test_adopt_plan_with_sanitizers(tmp_path):
    """csrc/adopt_plan.hpp over 1000 random sessions: the read set, the flag bytes, the model of the two kernels against a top-down
    restatement, and what comes back, with the invariants tests/host_check/adopt_plan_check.cpp names."""
    exe = str(tmp_path / "adopt_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "adopt_plan_check.cpp")])
    r = subprocess.run([exe, "1000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "adopt plan ok" in r.stdout and ", 0 failures" in r.stdout, r.stdout
