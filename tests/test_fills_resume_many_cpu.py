"""CPU checks of cp2_fills_resume_many: the name is exported and carries one signature in the header, the ctypes binding and the Nim
binding, and stands in the header's `next:` list with MINOR still 2; its section follows cp2_fills_finish_many's, leaves that section as
it was and names what it leaves out; NULL arguments are refused without touching a device or `out`; the model of the plan
(tests/fills_resume_many_models.py) is held against brute force -- every present block exactly once, each file of a chunk opened once and
read in ascending offsets, verdict to (entry, block) and back, distinct 32-byte-strided addresses inside layer 0 --; and the host side
(csrc/fills_resume_plan.hpp), compiled with its own main under AddressSanitizer + UBSan, agrees with the model line by line: plans,
refusals with the lowest index winning and arguments before checkpoints, and the reader against real files on four threads, also under
ThreadSanitizer."""
import ctypes
import os
import re
import subprocess

import pytest

import fills_resume_many_models as M
import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_OK, CP2_ERR_INVALID = 0, -1
NAME = "cp2_fills_resume_many"
SIGNATURE = ("i32", ["handle:ctx", "ptr(ptr(void))", "ptr(u64)", "ptr(ptr(u8))", "ptr(cstr)", "usize", "i32", "ptr(ptr(void))", "ptr(u64)"])
SECTION = "---- many fill sessions resumed in one pass"
SRC = os.path.join(ROOT, "tests", "host_check", "fills_resume_many_check.cpp")


def test_the_name_is_exported_and_matches_in_header_nim_and_ctypes(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    protos, procs = N.header_prototypes(HEADER), N.nim_importc(NIM)
    assert protos[NAME] == procs[NAME] == SIGNATURE, (protos[NAME], procs[NAME])
    L = pkg.load_library()
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert L._cp2_signatures[NAME] == (ctypes.c_int, [vp, vp, vp, vp, vp, sz, i32, vp, vp])
    assert getattr(L, NAME).restype is ctypes.c_int and callable(pkg.fills_resume_many)
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    assert NAME in history
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER) and pkg.ABI_VERSION_MINOR == 2


def test_the_section_follows_the_finish_and_says_what_it_leaves_out():
    at, proto = HEADER.index(SECTION), HEADER.index("int " + NAME + "(")
    assert HEADER.index("int cp2_fills_finish_many(") < at < proto < HEADER.index("---- e: every GPU of the node")
    section = HEADER[at:HEADER.index(";", proto)]
    assert "#define" not in section
    for word in ("Sessions", "Meaning", "Refused", "Device", "Failure", "Trace", "Out of scope", "cp2_multi", "CP2FILL2", "cp2_fill_keep_nodes",
                 "cp2_fill_resume_nodes", "cp2_fill_adopt", "many-session begin", "O_DIRECT", "all or nothing", "k_block_root_recheck_addr",
                 "CP2_ERR_IO", "CP2_ERR_INVALID", "CP2_ERR_HIP", "CP2_TRACE", "n_fills == 0", "CP2_RESUME_TRUST_FILES", "CP2_FILL_NEW"):
        assert word in section, word
    # the sections before it say what they said: a many-session save or adopt is still out of their scope
    assert "begin, save or adopt" in HEADER[HEADER.index("---- many fill sessions finished in one pass"):at]


def test_null_arguments_are_refused_and_out_untouched(pkg):
    L = pkg.load_library()
    out = (ctypes.c_void_p * 2)(0x5E, 0x5E)
    dropped = (ctypes.c_uint64 * 2)(7, 7)
    assert L.cp2_fills_resume_many(None, None, None, None, None, 2, 0, out, dropped) == CP2_ERR_INVALID
    assert L.cp2_fills_resume_many(None, None, None, None, None, 0, 0, None, None) == CP2_ERR_INVALID
    assert list(out) == [0x5E, 0x5E] and list(dropped) == [7, 7]


# ---- the model against brute force -------------------------------------------------------------------------------------------------------------
CASES = M.cases()


def test_the_cases_hold_what_they_claim():
    sessions = [s for c in CASES for s in c[0]]
    totals = [s.n_local * s.n_blocks for s in sessions]
    assert {s.n_blocks for s in sessions} == {1, 2, 8}
    assert any(s.bits == 0 for s in sessions) and any(s.bits == (1 << t) - 1 for s, t in zip(sessions, totals))
    assert any(bin(s.bits).count("1") == 1 and t > 1 for s, t in zip(sessions, totals))
    assert any(s.first_slot > 0 for s in sessions) and any(s.whole and 0 in s.whole for s in sessions)
    assert any(s.whole and any(0 < w < s.n_blocks for w in s.whole) for s in sessions)
    mixed = CASES[0][0]
    assert [s.from_file for s in mixed[:3]] == [True, False, True] and mixed[0].base == mixed[2].base
    assert {1, 3} <= {c for case in CASES for c in case[3]}
    assert any(c > len(M.plan(case[0], case[1], case[2]).g) for case in CASES for c in case[3])


@pytest.mark.parametrize("no", range(len(CASES)))
def test_the_model_names_every_present_block_once(no):
    sessions, cell, block, chunks = CASES[no]
    p = M.plan(sessions, cell, block)
    # brute force: walk every (entry, local slot, block) and ask the bitmap and the files
    want = []
    for k, s in enumerate(sessions):
        for local in range(s.n_local):
            for b in range(s.n_blocks):
                g = local * s.n_blocks + b
                backed = s.whole is None or b < s.whole[local]
                if s.bits >> g & 1 and backed:
                    want.append((k, s.first_slot + local, b, g))
    assert [(r[0], r[1], r[2], g) for r, g in zip(p.req, p.g)] == want and len(set(want)) == len(want)
    assert p.n_file == sum(sessions[k].from_file for k, _, _, _ in want)
    # the short-file drop took exactly the present blocks the files do not back, ascending
    for s in sessions:
        bits, dropped = M.drop_short(s)
        assert dropped == sorted(dropped) and all(s.bits >> g & 1 and not bits >> g & 1 for g in dropped)
        assert bits | sum(1 << g for g in dropped) == s.bits
    # verdict index to (entry, block) and back; the drop lists of a pattern
    assert [M.where(p, i) for i in range(len(p.g))] == [(k, g) for k, _, _, g in want]
    verdict = M.verdict_pattern(len(p.g))
    d = M.drops(p, verdict)
    assert sorted((k, g) for k, gs in enumerate(d) for g in gs) == sorted(M.where(p, i) for i, v in enumerate(verdict) if v)
    assert all(gs == sorted(gs) for gs in d)
    # addresses: distinct, 32-byte strided, inside layer 0 of their own session
    assert len(set(p.addr)) == len(p.addr)
    for (k, _, _, g), a in zip(want, p.addr):
        s = sessions[k]
        assert (a - s.layer0) % 32 == 0 and 0 <= (a - s.layer0) // 32 == g < s.n_local * s.n_blocks
    # fake requests: the seed of their slot and the first cell of their block; file requests none
    for i, (k, slot, b, _) in enumerate(want):
        if p.fake:
            assert p.fake[i] == (not sessions[k].from_file)
            assert (p.seeds[i], p.firsts[i]) == ((M.seed_stub(sessions[k].seed, slot), b * (block // cell)) if p.fake[i] else (0, 0))
    assert bool(p.fake) == any(not sessions[k].from_file for k, _, _, _ in want)
    # chunks: every file-sourced request of the chunk in exactly one group; a file once per chunk; ascending offsets inside it
    for chunk in chunks:
        rp = M.read_plan(p, sessions, chunk)
        assert [c0 for c0, _, _ in rp] == list(range(0, len(p.g), chunk)) and (not rp or rp[-1][1] == len(p.g))
        for c0, c1, groups in rp:
            files = [(sessions[d].base, slot) for d, slot, _ in groups]
            assert len(set(files)) == len(files) and files == sorted(files, key=lambda f: ([s.base for s in sessions].index(f[0]), f[1]))
            read = [i for _, _, idx in groups for i in idx]
            assert sorted(read) == [i for i in range(c0, c1) if sessions[p.req[i][0]].from_file]
            for d, slot, idx in groups:
                assert all(sessions[p.req[i][0]].base == sessions[d].base and p.req[i][1] == slot for i in idx)
                offs = [p.req[i][2] for i in idx]
                assert offs == sorted(offs)


def test_the_upload_cuts_cover_every_byte_once():
    for sizes, piece in (([32, 256, 64, 0, 32, 1024], 100), ([32, 32], 1 << 20), ([96], 32), ([1, 2, 3], 1), ([], 8)):
        cs = M.cuts(sizes, piece)
        seen = [0] * len(sizes)
        at = 0
        for seg, off, ln, where, flush in cs:
            assert off == seen[seg] and ln > 0 and where == at and at + ln <= piece
            seen[seg] += ln
            at = 0 if flush else at + ln
            assert flush == (where + ln == piece) or (seg, off + ln) == (cs[-1][0], seen[cs[-1][0]])
        assert seen == sizes and (not cs or cs[-1][4])
        assert [c[0] for c in cs] == sorted(c[0] for c in cs)


def test_the_refusals_take_the_lowest_index_and_arguments_first():
    got = [M.check_args(c) for c in M.calls()]
    assert [None if g is None else g[0] for g in got] == [None, None, None, 0, 2, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 2]
    assert all(g is None or g[1] == M.INVALID for g in got)
    assert "flag bits 0x2" in got[3][2] and "flag bits 0x6" in got[4][2] and "cfgs[1] is NULL" in got[10][2] and "slot_roots[1]" in got[11][2]
    assert "paths[2]" in got[12][2] and "stub refusal of 1" in got[13][2] and "block_size 8192" in got[14][2] and "stub refusal of 1" in got[15][2]
    assert got[16][2].startswith("fills: entry 2: cell_size 128, block_size 512 differ from entry 0's 64, 512")
    assert [M.expected_found_line(f) for f in M.FOUND][1:3] == ["failed 1 status -5: fills: entry 1: finding of 1", "failed 1 status -1: fills: entry 1: finding of 1"]


# ---- the product's plan, stand-alone under the sanitizers, against the model ---------------------------------------------------------------------
def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", *flags, "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("fills_resume_many_check"), "fills_resume_many_check", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def held(cmd, want, what):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, "%s:\n%s" % (what, (r.stdout + r.stderr)[-4000:])
    got = r.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.rstrip() == w.rstrip(), "%s, line %d:\n  the plan:  %s\n  the model: %s" % (what, i, g[:600], w[:600])
    assert len(got) == len(want), "%s: %d lines, the model has %d" % (what, len(got), len(want))


def test_the_plan_agrees_with_the_model(checker, tmp_path):
    path = str(tmp_path / "plans.txt")
    open(path, "w").write(M.plan_scenario(CASES) + "cuts 100 6 32 256 64 0 32 1024\ncuts 1 3 1 2 3\n")
    cut_lines = ["cuts " + " ".join("%d:%d+%d@%d%s" % (s, o, ln, at, "!" if f else "") for s, o, ln, at, f in M.cuts(sizes, piece))
                 for sizes, piece in (([32, 256, 64, 0, 32, 1024], 100), ([1, 2, 3], 1))]
    held([checker, "plan", path], M.expected_plan_lines(CASES) + cut_lines + ["fills resume many ok"], "the plans")


def test_the_refusals_agree_with_the_model(checker, tmp_path):
    path = str(tmp_path / "args.txt")
    open(path, "w").write(M.args_scenario())
    held([checker, "args", path], M.expected_args_lines() + ["fills resume many ok"], "the refusals")


def test_the_reader_against_real_files_asan_ubsan_and_tsan(checker, tmp_path):
    """Real slot files -- whole, short, shared by two entries -- read as a three-chunk plan on four threads, every row against the file's
    bytes; then a file that is a directory and a file that is gone: the first failing file in plan order is the one named."""
    for name, exe in (("asan", checker), ("tsan", build(tmp_path, "check_tsan", ["-fsanitize=thread"]))):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([exe, "read", str(d), "4"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr and "ERROR" not in r.stderr, (name, r.stdout, r.stderr[-2000:])
        assert r.stdout.splitlines() == M.expected_read_lines(), (name, r.stdout)
