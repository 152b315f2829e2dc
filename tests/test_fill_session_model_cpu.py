"""CPU checks of the whole-session model and its sequence generator (tests/fill_session_model.py), for the very seeds and step counts
tests/test_gpu_fill_sequences.py runs on the device: (a) every sequence replayed on the product's own host plans by
tests/host_check/fill_session_replay.cpp (AddressSanitizer + UBSan, its own main) prints, step by step, what the model says -- results,
presence, known rows, remembered candidates, anchors, proof statuses; (b) the sequences really cross the features: the coverage conditions
hold for every shape of at least 8 blocks a slot, and every kind of operation occurs at least 3 times per shape.  No GPU."""
import os
import subprocess
from collections import Counter

import pytest

import fill_session_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codex-storage-proofs-circuits_amd", "csrc")
CASES = [(name, True, seed) for name in S.SHAPES for seed in S.SEEDS[name]] + [(name, False, seed) for name in S.FAKE_SHAPES for seed in S.FAKE_SEEDS[name]]


@pytest.fixture(scope="module")
def replay_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fill_session_replay") / "fill_session_replay")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "host_check", "fill_session_replay.cpp")])
    return exe


# ---- the operation list as the replay program reads it, and what the model expects it to print ----------------------------------------------
def disk_words(m):
    """how many whole blocks each slot file covers, and per block of the range 'T', 'D' or '-': the device's and the file system's verdicts"""
    whole = [len(m.disk[s]) if m.disk[s] is not None else 0 for s in range(m.n_local)]
    labels = "".join(m.disk[s][b] if m.covered(s, b) else "-" for s in range(m.n_local) for b in range(m.nb))
    return " ".join(map(str, whole)) + " " + labels


def line_of(m, op):
    """one line for the replay program; m is the model BEFORE the operation"""
    kind = op[0]
    if kind in ("add", "anchored"):
        words = [kind, len(op[1]), -1 if op[2] is None else op[2]]
        for r in op[1]:
            words += list(r[:-1]) + [0 if r[-1] == "ok" else 1]
        return " ".join(map(str, words))
    if kind in ("anchors", "proofs"):
        return " ".join(map(str, [kind, len(op[1])] + [x for p in op[1] for x in p]))
    if kind == "missing":
        return "missing %d" % op[1]
    if kind == "resume":
        return "resume %d %s" % (op[1], disk_words(m))
    if kind == "adopt":
        s0, ns = (0, m.n_local) if op[2] == 0 else (op[1] - m.first, op[2])
        return "adopt %d %d %d %s" % (s0, ns, op[3], disk_words(m))
    return kind if kind in ("keep", "save", "finish") else "nop"


def result_line(op, res):
    if res["err"] == S.ERR_INVALID:
        return "R -1"
    kind = op[0]
    if kind in ("add", "anchored"):
        return "R %d %s %d" % (res["err"], " ".join(map(str, res["status"])), res["n_new"])
    if kind == "resume":
        return "R 0 %d" % res["n_dropped"]
    if kind == "adopt":
        return "R 0 %d %d" % (res["n_read"], res["n_adopted"])
    if kind == "anchors":
        return "R 0 " + " ".join(map(str, res["levels"]))
    if kind == "proofs":
        return "R 0 " + " ".join(map(str, res["status"]))
    if kind == "missing":
        return " ".join(map(str, ["R 0", res["n_missing"]] + [x for p in res["missing"] for x in p]))
    return "R 0"


def state_lines(m):
    locals_ = [(s, b) for s in range(m.n_local) for b in range(m.nb)]
    return ["P " + "".join("1" if p in m.present else "0" for p in locals_),
            "K " + "".join("1" if r in m.known else "0" for r in range(m.rows)),
            "H " + "".join("1" if p in m.remember else "0" for p in locals_),
            "A " + " ".join(map(str, m.anchor_levels())),
            "S " + " ".join(map(str, m.proof_statuses())),
            "F %d %d" % (m.keeping, m.finished)]


def replay_on_the_plans(exe, tmp_path, shape, files, ops, what):
    m = S.SessionModel(shape, files)
    text, want = ["init %d %d %d %d" % (m.first, m.n_local, m.nb, files)], []
    for op in ops:
        text.append(line_of(m, op))
        res = m.apply(op)
        want.append((op, [result_line(op, res)] + state_lines(m)))
    path = tmp_path / "ops.txt"
    path.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (what, r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    got = r.stdout.splitlines()
    assert len(got) == 7 * len(ops), (what, len(got), len(ops))
    for k, (op, lines) in enumerate(want):
        for a, b in zip(got[7 * k:7 * k + 7], lines):
            assert a == b, "step %d %r: the plans print\n%s\nthe model\n%s\n%s" % (k, op, a, b, S.describe(what, shape, files, ops[:k + 1]))
    return m


# ---- (a) the model agrees with the product's host plans ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,files,seed", CASES, ids=["%s-%s-%d" % (n, "files" if f else "fake", s) for n, f, s in CASES])
def test_the_model_agrees_with_the_host_plans(replay_exe, tmp_path, name, files, seed):
    shape = S.SHAPES[name]
    ops = S.sequence(seed, shape, S.STEPS[name], files)
    assert ops == S.sequence(seed, shape, S.STEPS[name], files)                           # seeded: the same list every time
    m = replay_on_the_plans(replay_exe, tmp_path, shape, files, ops, seed)
    assert m.finished and not m.missing()


def test_more_seeds_on_the_host_plans(replay_exe, tmp_path):
    """the plans cost next to nothing to run: twenty more sequences per shape than the device sees"""
    for name, shape in S.SHAPES.items():
        for seed in range(100, 120):
            replay_on_the_plans(replay_exe, tmp_path, shape, True, S.sequence(seed, shape, S.STEPS[name], True), seed)


# ---- (b) the sequences do what they are for -------------------------------------------------------------------------------------------------------
def coverage(name, files=True):
    total = Counter()
    for seed in (S.SEEDS if files else S.FAKE_SEEDS)[name]:
        m, _ = S.replay(S.SHAPES[name], S.sequence(seed, S.SHAPES[name], S.STEPS[name], files), files)
        total.update(m.cov)
    return total


@pytest.mark.parametrize("name", [n for n, shape in S.SHAPES.items() if shape[0] >= 8])
def test_the_committed_seeds_meet_every_coverage_condition(name):
    cov = coverage(name)
    for cond in S.CONDITIONS:
        assert cov[cond] >= 1, (name, cond, dict(cov))


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_every_operation_kind_occurs_at_least_three_times_per_shape(name):
    cov = coverage(name)
    for kind in S.OP_KINDS:
        assert cov["op:" + kind] >= 3, (name, kind, dict(cov))
    if name in S.FAKE_SHAPES:
        cov = coverage(name, files=False)
        for kind in S.FAKE_OP_KINDS:
            assert cov["op:" + kind] >= 3, (name, kind, dict(cov))
        assert not any(cov["op:" + kind] for kind in ("adopt", "damage", "place"))          # what the header refuses there is never proposed


# ---- the model's own rules, pinned --------------------------------------------------------------------------------------------------------------
def test_pinned_crossings():
    """the seams the issue names, by hand: an unwritten block's nodes let an adopt take its neighbour; a keeping session's checkpoint resumes
    as a plain one; a level below the anchor refuses the whole call"""
    shape = S.SHAPES["b8"]
    ops = [["keep"],
           ["place", 1, [2, 3]],
           ["adopt", 1, 1, False],                                                         # the file covers blocks 0 ... 3 (a hole, then the two): nothing vouches
           ["add", [[1, 0, "ok"], [1, 1, "ok"]], 1],                                       # proved, not written: nodes known, blocks missing
           ["adopt", 1, 1, True],                                                          # node (1, 1) came as a sibling: blocks 2 and 3 prove
           ["anchored", [[1, 4, 1, "ok"]], None],                                          # level 1 is below block 4's anchor (2)
           ["save"], ["resume", False], ["proofs", [[1, 2]]], ["keep"], ["proofs", [[1, 2], [1, 3], [1, 0]]]]
    m, res = S.replay(shape, ops)
    assert (res[2]["n_read"], res[2]["n_adopted"]) == (4, 0)
    assert res[3] == {"err": S.ERR_IO, "status": [S.FILL_UNWRITTEN] * 2, "n_new": 0}
    assert (res[4]["n_read"], res[4]["n_adopted"]) == (0, 2)
    assert res[5] == {"err": S.ERR_INVALID} and res[8] == {"err": S.ERR_INVALID}
    assert res[7]["n_dropped"] == 0 and sorted(m.present) == [(1, 2), (1, 3)]
    assert res[10]["status"] == [S.PROOF_PARTIAL, S.PROOF_PARTIAL, S.PROOF_ABSENT]       # what presence gives: the siblings are gone
