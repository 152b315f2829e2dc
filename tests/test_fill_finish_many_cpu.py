"""CPU checks of cp2_fills_finish_many: the name is exported and carries one signature in the header, the ctypes binding and the Nim
binding, and stands in the header's `next:` list with MINOR still 2; its section lies outside the span tests/test_fill_many_cpu.py pins and
names what it leaves out; NULL arguments are refused without touching a device or `out`; the model of the plan
(tests/fill_finish_many_models.py) is held against brute force on the launcher test's shapes -- every (session, slot, level, node) covered
exactly once, at the rows of the layer-major layout --; and the host side (csrc/fill_finish_plan.hpp), compiled with its own main under
AddressSanitizer + UBSan, agrees with the model line by line on those shapes and on seeded random ones: tables, lanes, the verdict index
turned back, every refusal with its index, and the order of saves and hand-overs with a failing save injected at every k."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fill_finish_many_models as M
import nim_api as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "codex-storage-proofs-circuits_amd")
HEADER = open(os.path.join(ROOT, "include", "codex_p2.h")).read()
NIM = open(os.path.join(PKG_DIR, "nim", "codex_p2.nim")).read()
CP2_OK, CP2_ERR_INVALID = 0, -1
NAME = "cp2_fills_finish_many"
SIGNATURE = ("i32", ["handle:ctx", "ptr(ptr(void))", "usize", "ptr(cstr)", "ptr(handle:dataset)"])
SECTION = "---- many fill sessions finished in one pass"
SEEDS = range(8)


def test_the_name_is_exported_and_matches_in_header_nim_and_ctypes(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    protos, procs = N.header_prototypes(HEADER), N.nim_importc(NIM)
    assert protos[NAME] == procs[NAME] == SIGNATURE, (protos[NAME], procs[NAME])
    L = pkg.load_library()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert L._cp2_signatures[NAME] == (ctypes.c_int, [vp, vp, sz, vp, vp])
    assert getattr(L, NAME).restype is ctypes.c_int and callable(pkg.fills_finish_many)
    history = HEADER[HEADER.index("next:"):HEADER.index("#define CP2_ABI_VERSION_MAJOR")]
    assert NAME in history
    assert re.search(r"#define CP2_ABI_VERSION_MINOR 2\b", HEADER) and pkg.ABI_VERSION_MINOR == 2


def test_the_section_lies_outside_the_pinned_span_and_says_what_it_leaves_out():
    a, b = HEADER.index("---- proved blocks added to many fill sessions"), HEADER.index("cp2_write_circom_main(")
    at, proto = HEADER.index(SECTION), HEADER.index("int " + NAME + "(")
    assert not a <= at <= b and not a <= proto <= b and at < proto
    assert HEADER.index("int cp2_fill_resume_nodes(") < at                       # after the checkpoints with nodes
    assert "finish, save or adopt" in HEADER[a:b] and NAME not in HEADER[a:b]     # that paragraph stands as it was
    section = HEADER[at:HEADER.index(";", proto)]
    assert "#define" not in section
    for word in ("cp2_multi", "begin, save or adopt", "threads", "k_finish_layer_many", "lifts the many-session finish", "listed twice",
                 "all or nothing", "CP2_ERR_IO", "CP2_ERR_ALLOC", "CP2_ERR_HIP", "CP2_TRACE", "n_fills == 0", "first missing"):
        assert word in section, word


def test_null_arguments_are_refused_and_out_untouched(pkg):
    L = pkg.load_library()
    fills = (ctypes.c_void_p * 2)(None, None)
    out = (ctypes.c_void_p * 2)(0x5E, 0x5E)
    paths = (ctypes.c_char_p * 2)(b"/nonexistent/a", None)
    assert L.cp2_fills_finish_many(None, fills, 2, paths, out) == CP2_ERR_INVALID
    assert L.cp2_fills_finish_many(None, None, 0, None, None) == CP2_ERR_INVALID
    assert L.cp2_fills_finish_many(None, None, 2, None, out) == CP2_ERR_INVALID
    assert list(out) == [0x5E, 0x5E]


# ---- the model against brute force, on the launcher test's shapes ---------------------------------------------------------------------------
def test_layer_sizes_are_the_oracles(oracle):
    c, _ = oracle
    rng = np.random.default_rng(0xF1)
    for n in M.BLOCKS:
        leaves = np.zeros((n, 32), dtype=np.uint8)
        leaves[:, :31] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
        assert [len(x) for x in c.merkle_tree(leaves)] == M.layer_sizes(n)
    assert M.layer_sizes(1) == [1, 1] and M.depth(1) == 1 and M.depth(2) == 1 and M.depth(3) == 2 and M.depth(257) == 9


@pytest.mark.parametrize("case", M.cases(), ids=lambda c: "case%d" % c.no)
def test_the_model_covers_every_node_exactly_once(case):
    ss = case.sessions
    p = M.plan(ss)
    assert p.voff == [sum(nl for _, nl in ss[:k]) for k in range(len(ss) + 1)]
    assert [M.where(p, v) for v in range(p.voff[-1])] == [(k, s) for k, (_, nl) in enumerate(ss) for s in range(nl)]
    assert len(p.level_off) == max(M.depth(n) for n, _ in ss)
    written = [np.zeros(M.rows(n, nl), dtype=np.int32) for n, nl in ss]
    compared = np.zeros(p.voff[-1], dtype=np.int32)
    for level in range(len(p.level_off)):
        active = [k for k, (n, _) in enumerate(ss) if M.depth(n) > level]
        a = p.level_off[level]
        assert p.sess_of[a:a + p.level_cnt[level]] == active
        # brute force: every (session, slot, node) of the level, in order
        want = [(k, s, j) for k in active for s in range(ss[k][1]) for j in range(M.layer_sizes(ss[k][0])[level + 1])]
        got = [M.lane(p, level, t) for t in range(p.level_work[level])]
        assert [(x.session, x.slot, x.node) for x in got] == want
        for x in got:
            n, nl = ss[x.session]
            sizes = M.layer_sizes(n)
            lo = nl * sum(sizes[:level])                                          # layer-major: coff[l] + s * csizes[l]
            assert x.src == lo + x.slot * sizes[level] + 2 * x.node and x.dst == lo + nl * sizes[level] + x.slot * sizes[level + 1] + x.node
            assert x.pair == (2 * x.node + 1 < sizes[level]) and x.last == (level + 1 == M.depth(n))
            assert x.src + int(x.pair) < lo + (x.slot + 1) * sizes[level] <= x.dst < M.rows(n, nl)
            written[x.session][x.dst] += 1
            if x.last:
                assert x.node == 0 and x.dst == M.rows(n, nl) - nl + x.slot
                compared[p.voff[x.session] + x.slot] += 1
    for (n, nl), w in zip(ss, written):
        assert (w[:n * nl] == 0).all() and (w[n * nl:] == 1).all()                # layer 0 is read only, every row above once
    assert (compared == 1).all()                                                  # every verdict has exactly one writer


def test_the_cases_hold_the_shapes_they_claim():
    cs = M.cases()
    assert set(M.TOTALS) <= {M.plan(c.sessions).level_work[0] for c in cs}
    assert {n for c in cs for n, _ in c.sessions} == set(M.BLOCKS) and {nl for c in cs for _, nl in c.sessions} == set(M.LOCALS)
    assert all(c.sessions[0] == (1, 1) and c.sessions[-1] == (1, 1) for c in cs)
    assert all(len({M.depth(n) for n, _ in c.sessions}) >= 3 for c in cs if len(c.sessions) > 3)
    mixed = 0
    for c in cs:
        p = M.plan(c.sessions)
        mixed += any(M.mixed_wave(p, level, w) for level in range(len(p.level_off)) for w in range((p.level_work[level] + M.WAVE - 1) // M.WAVE))
    assert mixed >= 3


# ---- the product's plan, stand-alone under the sanitizers, against the model ---------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fill_finish_many_check") / "fill_finish_many_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(PKG_DIR, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_check", "fill_finish_many_check.cpp")])
    return exe


def held(checker, path, world, calls, what):
    open(path, "w").write(M.scenario_text(world, calls))
    r = subprocess.run([checker, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, "%s:\n%s" % (what, (r.stdout + r.stderr)[-4000:])
    got, want = r.stdout.splitlines(), M.expected_lines(world, calls) + ["fill finish many ok"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s, line %d:\n  the plan:  %s\n  the model: %s" % (what, i, g[:600], w[:600])
    assert len(got) == len(want), "%s: %d lines, the model has %d" % (what, len(got), len(want))
    return want


def test_the_plan_agrees_with_the_model_on_the_launcher_shapes(checker, tmp_path):
    world, calls = M.cases_text(M.cases())
    lines = held(checker, str(tmp_path / "cases.txt"), world, calls, "the launcher test's shapes")
    assert not any(ln.startswith("refused") for ln in lines)


def test_the_plan_agrees_with_the_model_on_seeded_calls(checker, tmp_path):
    seen = {"NULL": 0, "another context": 0, "finished": 0, "listed twice": 0, "missing": 0, "accepted": 0, "failing save": 0, "one session": 0}
    for seed in SEEDS:
        world, calls = M.scenario(seed)
        lines = held(checker, str(tmp_path / ("scenario%d.txt" % seed)), world, calls, "seed %d" % seed)
        for ln in lines:
            for word in ("NULL", "another context", "finished", "listed twice", "missing"):
                seen[word] += ln.startswith("refused") and word in ln
            seen["failing save"] += ln.startswith("commit fail") and "status -5" in ln and "hand" not in ln and "make" not in ln
        seen["accepted"] += sum(M.refusal(c[0], world) is None for c in calls)
        seen["one session"] += sum(len(c[0]) == 1 and M.refusal(c[0], world) is None for c in calls)
        # all or nothing, in the model's own words: no hand-over unless every save and every object succeeded, and then all of them
        for fills, has_path, _ in calls:
            for fail_at in list(range(len(fills))) + [None]:
                st, ev, saved = M.commit_events(len(fills), has_path, fail_at)
                hands = [e for e in ev if e.startswith("hand")]
                assert (st == 0) == (len(hands) == len(fills)) and (st == 0 or not hands)
                assert [e for e in ev if e.startswith("save")] == ["save %d" % k for k in range(len(fills)) if has_path[k] and (st == 0 or k <= fail_at)]
                assert not hands or ev.index(hands[0]) > max(i for i, e in enumerate(ev) if e.startswith("make"))
    assert all(v > 0 for v in seen.values()), seen
