"""CPU checks of cp2_fills_add_many: the name is exported and carries one signature in the header, the ctypes binding and the Nim binding,
stands in the header's `next:` list with MINOR still 2, its section stands after the anchored adds and says what is out of scope, NULL
arguments are refused without touching a device or the outputs, and the host side (csrc/fill_many_plan.hpp) agrees line by line with the
model (tests/fill_many_models.py, one tests/fill_session_model.py per session) over the committed seeds, under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

import pytest

import fill_many_models as MM
import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_OK, CP2_ERR_INVALID = 0, -1
NAME = "cp2_fills_add_many"
ARGS = ["ptr(void)", "ptr(ptr(void))", "usize", "ptr(u64)", "ptr(u8)", "ptr(u32)", "ptr(u8)", "usize", "ptr(u32)", "ptr(usize)"]


def test_the_name_is_exported_and_matches_in_header_nim_and_ctypes(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    protos, procs = N.header_prototypes(HEADER), N.nim_importc(NIM)
    assert protos[NAME][0] == procs[NAME][0] == "i32"
    assert protos[NAME][1] == procs[NAME][1], (protos[NAME], procs[NAME])
    assert len(protos[NAME][1]) == len(ARGS) and protos[NAME][1][2:] == ARGS[2:], protos[NAME]
    L = pkg.load_library()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert L._cp2_signatures[NAME] == (ctypes.c_int, [vp, vp, sz, vp, vp, vp, vp, sz, vp, vp])
    assert getattr(L, NAME).restype is ctypes.c_int and callable(pkg.fills_add_many)
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    assert NAME in history
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER) and pkg.ABI_VERSION_MINOR == 2


def test_the_section_stands_after_the_anchored_adds_and_says_what_it_leaves_out():
    assert HEADER.index("int cp2_fill_add_anchored(") < HEADER.index("---- proved blocks added to many fill sessions") < HEADER.index("int cp2_fills_add_many(") < \
        HEADER.index("cp2_write_circom_main(")
    section = HEADER[HEADER.index("---- proved blocks added to many fill sessions"):HEADER.index("cp2_write_circom_main(")]
    assert "#define" not in section
    for word in ("cp2_multi", "finish, save or adopt", "threads", "k_block_path_commit_many", "WHEN THE CALL STARTS", "listed twice", "all or nothing",
                 "first failing file", "n_new zeroed", "CP2_ERR_HIP", "CP2_TRACE"):
        assert word in section, word


def test_null_arguments_are_refused_and_outputs_untouched(pkg):
    L = pkg.load_library()
    req = (ctypes.c_uint64 * 3)(0, 0, 0)
    status = (ctypes.c_uint32 * 1)(7)
    data = (ctypes.c_uint8 * 64)(*([9] * 64))
    n_new = (ctypes.c_size_t * 1)(5)
    fills = (ctypes.c_void_p * 1)(None)
    assert L.cp2_fills_add_many(None, fills, 1, req, data, None, data, 1, status, n_new) == CP2_ERR_INVALID
    assert L.cp2_fills_add_many(None, None, 0, None, None, None, None, 0, None, None) == CP2_ERR_INVALID
    assert list(status) == [7] and list(n_new) == [5] and list(data) == [9] * 64


def test_the_model_alone_on_a_pinned_call():
    """A pin on the Python model only, not on the product (the product is held to the model in the test below and on the GPU): two sessions
    that receive the same (slot, block) numbers; NEW and DUPLICATE of one block with the other session's request between"""
    m = MM.ManyModel([[8, 0, 2, 1, 0], [2, 0, 2, 0, 1]])
    reqs = [[0, 1, 1, "ok"], [1, 1, 1, "ok"], [0, 1, 1, "ok"], [1, 0, 0, "data"], [0, 0, 5, "ok"]]
    res = m.add_many([0, 1], reqs)
    assert res == {"err": 0, "status": [0, 0, 2, 1, 0], "n_new": [2, 1]}
    assert m.add_many([1, 0], [[1, 1, 1, "ok"], [0, 1, 1, "ok"]], levels=[0, 0])["refused"] == ("request", 1)   # fills[0] keeps no nodes: level 0 < its depth
    assert m.add_many([0, 1], reqs, levels=[0, 1, 3, 1, 3]) == {"err": 0, "status": [2, 2, 2, 1, 2], "n_new": [0, 0]}
    assert m.add_many([0, 0], reqs)["refused"] == ("fills", 1) and m.add_many([0], reqs)["refused"] == ("request", 1)
    assert m.add_many([0, 1], reqs, have_paths=False)["refused"] == ("request", 0)
    assert m.add_many([0, 1], [[0, 1, 1, "ok"]], levels=[0], have_paths=False)["status"] == [2]
    res = m.add_many([1, 0], [[0, 0, 0, "ok"], [1, 1, 7, "ok"], [0, 1, 0, "ok"]], fail={0: 0})     # a file that cannot be written
    assert res == {"err": -5, "status": [3, 0, 3], "n_new": [0, 1]}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fill_many_check") / "fill_many_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "fill_many_check.cpp")])
    return exe


def test_the_plan_agrees_with_the_model_line_by_line_under_sanitizers(checker, tmp_path):
    seen = {"wave of three depths": 0, "same numbers in two sessions": 0, "new and duplicate across another session": 0, "refused and unchanged": 0,
            "twice": 0, "short into a plain session": 0, "io": 0, "levels": 0, "whole": 0}
    for seed in MM.SEEDS:
        sessions, steps = MM.scenario(seed)
        assert 1 <= len(sessions) <= 9 and all(s[0] in MM.BLOCKS and 1 <= s[2] <= 3 for s in sessions)
        path = str(tmp_path / ("scenario%d.txt" % seed))
        open(path, "w").write(MM.scenario_text(sessions, steps))
        r = subprocess.run([checker, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, "seed %d:\n%s" % (seed, (r.stdout + r.stderr)[-4000:])
        got, want = r.stdout.splitlines(), MM.expected_lines(sessions, steps) + ["fill many ok"]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "seed %d, line %d:\n  the plan:  %s\n  the model: %s" % (seed, i, g, w)
        assert len(got) == len(want), "seed %d: %d lines, the model has %d" % (seed, len(got), len(want))
        # what the committed seeds must contain
        model = MM.ManyModel(sessions)
        for step in steps:
            before = model.state_lines()
            if step[0] == "call":
                _, fills, reqs, levels, have_paths, fail = step
                why = model.refusal(fills, reqs, levels, have_paths)
                if why is None:
                    depths = {model.sessions[fills[r[0]]].depth for r in reqs}
                    seen["wave of three depths"] += len(reqs) >= MM.WAVE and len(depths) >= 3 and len({r[0] for r in reqs[:MM.WAVE]}) >= 3
                    numbers = {}
                    for r in reqs:
                        numbers.setdefault((r[1], r[2]), set()).add(r[0])
                    seen["same numbers in two sessions"] += any(len(v) > 1 for v in numbers.values())
                    seen["levels" if levels is not None else "whole"] += 1
                elif len(set(fills)) < len(fills):
                    seen["twice"] += 1
                elif levels is not None and why[0] == "request" and reqs[why[1]][0] < len(fills) and not model.sessions[fills[reqs[why[1]][0]]].keeping and \
                        levels[why[1]] < model.sessions[fills[reqs[why[1]][0]]].depth:
                    seen["short into a plain session"] += 1
            lines = model.step_lines(step)
            if step[0] == "call":
                if why is not None:
                    assert lines[-len(before):] == before
                    seen["refused and unchanged"] += 1
                else:
                    st = [int(x) for x in lines[-len(before) - 1].split("status ")[1].split(" n_new")[0].split()] if reqs else []
                    seen["io"] += lines[-len(before) - 1].startswith("result -5")
                    for i, r in enumerate(reqs):
                        for j in range(i + 2, len(reqs)):
                            if reqs[j][:3] == r[:3] and st[i] == 0 and st[j] == 2 and any(x[0] != r[0] for x in reqs[i + 1:j]):
                                seen["new and duplicate across another session"] += 1
    assert all(v > 0 for v in seen.values()), seen

