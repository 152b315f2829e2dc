"""CPU checks of cp2_datasets_repair_blocks_many: the name is exported and carries one signature in the header, the ctypes binding and the
Nim binding, stands in the header's `next:` list with MINOR still 2, and its section sits between the verified read-back and the fill
sessions and says how its writer differs from the single call's; NULL handles are refused without touching a device or an output; the
model of the plan (tests/repair_many_models.py) agrees with a request-by-request restatement of the refusal rule and holds what its cases
claim; and the host side (csrc/repair_many_plan.hpp), compiled with its own main under AddressSanitizer + UBSan, agrees with the model line
by line -- every refusal and its index in the stated order, the descriptor tables with path rows across chunk boundaries, the write groups
and repeats through a twice-listed handle and through two handles on one base name -- and its threaded writer, against real files, also
under ThreadSanitizer, writes the right bytes at the right offsets with one sync per file, lets a directory fail alone, and names the same
first failing file on 1, 2 and 8 threads."""
import ctypes
import os
import re
import subprocess

import pytest

import nim_api as N
import repair_many_models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_OK, CP2_ERR_INVALID = 0, -1
NAME = "cp2_datasets_repair_blocks_many"
SIGNATURE = ("i32", ["handle:ctx", "ptr(handle:dataset)", "usize", "ptr(u64)", "ptr(u8)", "ptr(u8)", "ptr(u64)", "usize", "i32", "ptr(cstr)", "ptr(u32)",
                     "ptr(usize)"])
SECTION = "---- repair many: replacement blocks of many datasets"
SRC = os.path.join(ROOT, "tests", "host_check", "repair_many_check.cpp")


def test_the_name_is_exported_and_matches_in_header_nim_and_ctypes(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    protos, procs = N.header_prototypes(HEADER), N.nim_importc(NIM)
    assert protos[NAME] == procs[NAME] == SIGNATURE, (protos[NAME], procs[NAME])
    L = pkg.load_library()
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert L._cp2_signatures[NAME] == (ctypes.c_int, [vp, vp, sz, vp, vp, vp, vp, sz, i32, vp, vp, ctypes.POINTER(sz)])
    assert getattr(L, NAME).restype is ctypes.c_int and callable(pkg.Context.repair_blocks_many)
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    assert NAME in history
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER) and pkg.ABI_VERSION_MINOR == 2


def test_the_section_sits_between_the_read_back_and_the_fill_sessions():
    at, proto = HEADER.index(SECTION), HEADER.index("int " + NAME + "(")
    assert HEADER.index("int cp2_dataset_read_blocks(") < at < proto < HEADER.index("---- fill sessions: slots filled")
    section = HEADER[at:HEADER.index(";", proto)]
    assert "#define" not in section
    for word in ("Datasets", "Requests", "Meaning", "Refused", "Write", "Cache", "Trace", "Out of scope", "cp2_multi", "UNLIKE the single calls",
                 "every file is\n *              attempted on its own", "CP2_ERR_IO", "CP2_ERR_INVALID", "CP2_REPAIR_CHECK_ONLY", "cp2_block_proof_depth",
                 "roots-only", "listed twice", "same base name", "path_off[0] != 0", "n == 0", "CP2_TRACE", "ingestion"):
        assert word in section, word


def test_null_handles_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    status = (ctypes.c_uint32 * 2)(7, 7)
    written = ctypes.c_size_t(99)
    req = (ctypes.c_uint64 * 6)(0, 0, 0, 0, 0, 1)
    data = (ctypes.c_uint8 * 16)()
    assert L.cp2_datasets_repair_blocks_many(None, None, 0, req, data, None, None, 2, 0, None, status, ctypes.byref(written)) == CP2_ERR_INVALID
    assert L.cp2_datasets_repair_blocks_many(None, None, 0, None, None, None, None, 0, 0, None, None, None) == CP2_ERR_INVALID
    assert list(status) == [7, 7] and written.value == 99


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
CALLS = M.calls()


def test_the_cases_hold_what_they_claim():
    verdicts = [M.validate(c) for c in CALLS]
    said = " | ".join(v for v in verdicts if v)
    for words in ("unknown flag bits", "paths without path_off", "path_off without paths", "must not be NULL when n > 0", "path_off[0] is", "NULL dataset",
                  "belongs to another context", "differ from dataset 0's", "is not below n_ds", "path_off decreases", "is neither empty nor the depth",
                  "keeps only its slot roots", "not those of whole slot trees", "is not inside the local range", "is not below nBlocks", "has the fake source",
                  "is the block of request"):
        assert words in said, words
    accepted = [c for c, v in zip(CALLS, verdicts) if v is None and c.n]
    assert len(accepted) >= 20
    # both kinds of request in one call, paths that cross chunk boundaries, every residency, several depths
    assert any({t[4] == 0 for t in M.table(c)} == {True, False} for c in accepted)
    assert any(t[3] > 0 and i % max(1, c.chunk) for c in accepted for i, t in enumerate(M.table(c)))
    assert any(t[3] == 0 and t[4] and i and i % max(1, c.chunk) == 0 and c.path_off[i] for c in accepted for i, t in enumerate(M.table(c)))
    assert {c.ds[r[0]].mode for c in accepted for r in c.req} == {0, 1, 2}
    assert {c.ds[r[0]].depth for c in accepted for r in c.req} >= {1, 3}
    # repeats through one handle listed twice, through two handles over one base name, and through fake handles
    again = [c for c, v in zip(CALLS, verdicts) if v and "is the block of request" in v]
    def pair(c, v):
        i, j = int(re.search(r"request (\d+):", v).group(1)), int(re.search(r"of request (\d+) again", v).group(1))
        return c.ds[c.req[i][0]], c.ds[c.req[j][0]], c.req[i][0], c.req[j][0]
    pairs = [pair(c, M.validate(c)) for c in again]
    assert any(a.same_as == b.same_as and ka != kb for a, b, ka, kb in pairs)
    assert any(a.same_as != b.same_as and a.from_file and a.base == b.base for a, b, _, _ in pairs)
    assert any(not a.from_file for a, _, _, _ in pairs)
    # a file shared by two handles is one group
    assert any(len({c.ds[c.req[i][0]].same_as for i in g[3]}) > 1 for c in accepted for g in M.write_groups(c, M.verdict_pattern(c.n)))


def test_the_model_agrees_with_the_request_by_request_rule():
    for no, c in enumerate(CALLS):
        assert M.validate(c) == M.validate_brute(c), no


def test_the_groups_and_the_shares_cover_everything_once():
    for c in CALLS:
        if M.validate(c) is not None or not c.n:
            continue
        status = M.verdict_pattern(c.n)
        groups = M.write_groups(c, status)
        names = [g[2] for g in groups]
        assert len(set(names)) == len(names) and [(g[0], g[1]) for g in groups] == sorted((g[0], g[1]) for g in groups)
        assert sorted(i for g in groups for i in g[3]) == [i for i in range(c.n) if status[i] == M.MATCH and c.ds[c.req[i][0]].from_file]
        for g in groups:
            blocks = [c.req[i][2] for i in g[3]]
            assert blocks == sorted(blocks) and len(set(blocks)) == len(blocks)
        # the staged rows of a chunk hold every path of the chunk back to back
        if c.has["path_off"]:
            t, chunk = M.table(c), max(1, c.chunk)
            for c0 in range(0, c.n, chunk):
                at = 0
                for i in range(c0, min(c.n, c0 + chunk)):
                    assert t[i][3] == at
                    at += t[i][4]
                assert at <= M.most_path_rows(c)
    for threads in (1, 2, 8):
        for count in (0, 1, 7, 9):
            w = M.worker_of(threads, count)
            assert w == sorted(w) and (not w or set(w) == set(range(min(threads, count))))
    assert M.chunk_of(64 << 20, 65536, 16384) == 512 and M.chunk_of(1 << 20, 4096, 5) == 5 and M.chunk_of(0, 4096, 5) == 1


# ---- the product's plan, stand-alone under the sanitizers, against the model ---------------------------------------------------------------------
def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", *flags, "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("repair_many_check"), "repair_many_check", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def held(r, want, what):
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, "%s:\n%s" % (what, (r.stdout + r.stderr)[-4000:])
    got = r.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.rstrip() == w.rstrip(), "%s, line %d:\n  the plan:  %s\n  the model: %s" % (what, i, g[:600], w[:600])
    assert len(got) == len(want), "%s: %d lines, the model has %d" % (what, len(got), len(want))


def test_the_plan_agrees_with_the_model(checker, tmp_path):
    path = str(tmp_path / "calls.txt")
    open(path, "w").write(M.scenario(CALLS))
    r = subprocess.run([checker, "plan", path], capture_output=True, text=True, timeout=300)
    held(r, M.expected_plan_lines(CALLS) + ["repair many ok"], "the plans")


def lay_out(d, block):
    d.mkdir()
    for name in M.WRITE_DIRS:
        (d / name).mkdir()
    for name, blocks in M.WRITE_PRESENT.items():
        (d / name).write_bytes(b"\xEE" * (blocks * block))


def test_the_writer_against_real_files_asan_ubsan_and_tsan(checker, tmp_path):
    """Real slot files -- present, short, missing, and two directories in their place -- written by the threaded writer on 1, 2 and 8
    threads: the bytes at their offsets and nothing else, one fdatasync per file that opened, each directory failing alone with its
    neighbours written, and the same first failing file whatever the thread count."""
    case = M.write_case()
    block = case.ds[0].block
    path = str(tmp_path / "write.txt")
    open(path, "w").write(M.scenario([case]))
    assert M.validate(case) is None
    first = set()
    for name, exe in (("asan", checker), ("tsan", build(tmp_path, "check_tsan", ["-fsanitize=thread"]))):
        for threads in (1, 2, 8):
            d = tmp_path / ("%s%d" % (name, threads))
            lay_out(d, block)
            r = subprocess.run([exe, "write", path, str(d), str(threads)], capture_output=True, text=True, timeout=300)
            want = M.expected_write_lines(threads)
            held(r, want, "%s on %d thread(s)" % (name, threads))
            first.add(next(ln for ln in want if ln.startswith("settled")).split()[2])
            files = M.expected_write_files(block)
            assert sorted(os.listdir(d)) == sorted(set(files) | set(M.WRITE_DIRS))
            for fname, img in files.items():
                assert (d / fname).read_bytes() == bytes(img), (name, threads, fname)
            for fname in M.WRITE_DIRS:
                assert os.path.isdir(d / fname) and not os.listdir(d / fname)
    assert first == {"1"}      # a1.dat: the failing file that comes first in (dataset, slot) order
