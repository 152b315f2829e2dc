"""GPU suite: fill checkpoints with nodes -- cp2_fill_save_nodes / cp2_fill_resume_nodes.  A keeping session saved with its nodes and resumed
must know exactly what the device re-derives from the stated slot roots: with unchanged files everything it knew, after damage never more
than the file stated and never a value the stated roots do not vouch for.  The geometry of tests/test_gpu_fill_serve.py and
test_gpu_fill_adopt.py (cells of 64 bytes, blocks of 256, four slots; 1, 2, 8 and 64 blocks a slot), the Worlds imported from there.  Real
sessions run beside the model of tests/fill_node_ckpt_models.py through the driver of tests/test_gpu_fill_sequences.py, extended with the
two operations: after EVERY step the operation's result, missing, anchors, every block proof (against cp2_dataset_block_proofs of the
cp2_dataset_build of the same data), the slot files and, after a save, the file's fields are compared, bit-exactly.  A failing sequence
prints seed, shape and the operations so far."""
import copy
import ctypes
import faulthandler
import os
import struct

import numpy as np
import pytest

import fill_node_ckpt_models as N2
import fill_resume_models as R
import fill_session_model as S
import test_gpu_fill_sequences as Q
from test_gpu_fill_sequences import sctx, worlds  # noqa: F401  (fixtures: one context, one World per shape and source)

pytestmark = pytest.mark.gpu

CP2_OK, CP2_ERR_INVALID, CP2_ERR_IO = 0, -1, -5


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class Driver(Q.Driver):
    """test_gpu_fill_sequences.Driver with the two operations"""

    def __init__(self, *a):
        super().__init__(*a)
        self.nckpt = self.ckpt + ".nodes"

    def op_save_nodes(self):
        self.f.save_nodes(self.nckpt)
        return {"err": 0}

    def op_resume_nodes(self, trust, which):
        self.f.free()
        self.f = self.ctx.fill_resume_nodes(self.cfg, self.w.roots, self.nckpt if which == "nodes" else self.ckpt, self.first, self.n_local, trust_files=trust)
        self.was_present = None
        f = self.f
        return {"err": 0, "n_dropped": f.n_dropped, "n_restored": f.n_restored, "n_unproved": f.n_unproved, "n_rejected": f.n_rejected}

    def check(self, m, op, want, got):
        super().check(m, op, want, got)
        if op[0] == "save_nodes" and got["err"] == 0:                                     # what the file holds: presence, the known rows, the true nodes
            raw = open(self.nckpt, "rb").read()
            ck = N2.parse_checkpoint2(raw)
            assert ck["bits"] == m.checkpoint_bits() and ck["known"] == m.checkpoint_known(), "the bitmaps of the file"
            for g in range(len(ck["bits"])):
                assert not ck["known"][g] or ck["layer0"][g].tobytes() == self.w.src.roots[g].tobytes(), ("layer 0 of the file", g)
            self.f.save_nodes(self.nckpt + ".again")                                      # two saves of one state are byte-identical
            assert open(self.nckpt + ".again", "rb").read() == raw
            os.remove(self.nckpt + ".again")
            assert not [n for n in os.listdir(os.path.dirname(self.nckpt)) if ".tmp." in n]


def run(pkg, ctx, w, name, files, ops, directory, what, keep_open=False):
    shape = S.SHAPES[name]
    m = N2.NodeSessionModel(shape, files)
    d = Driver(pkg, ctx, w, shape, files, directory)
    assert d.pairs == m.pairs
    results = []
    try:
        for k, op in enumerate(ops):
            try:
                want = m.apply(op)
                got = d.apply(op)
                d.check(m, op, want, got)
                results.append(got)
            except Exception as e:
                raise AssertionError("step %d, %r: %s: %s\n%s" % (k, op, type(e).__name__, e, S.describe(what, shape, files, ops[:k + 1]))) from None
    except BaseException:
        d.close()
        raise
    if keep_open:
        return m, d, results
    d.close()
    return m, None, results


def half_in_shuffled_order(m, seed):
    """half of each slot's blocks, in one shuffled order, in calls of five, whole paths"""
    rng = np.random.default_rng([seed, m.nb])
    pairs = [p for p in m.pairs if rng.random() < 0.5 or m.nb == 1]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    return [["add", [[s, b, "ok"] for s, b in pairs[i:i + 5]], None] for i in range(0, len(pairs), 5)]


# ---- 1: serving after a resume ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b8", "b64"])
def test_a_resumed_session_serves_what_it_served_before(pkg, sctx, worlds, tmp_path, name):   # noqa: F811
    w = worlds(name, True)
    adds = half_in_shuffled_order(S.SessionModel(S.SHAPES[name]), 1)
    ops = [["keep"]] + adds + [["save_nodes"], ["save"]]
    m, d, _ = run(pkg, sctx, w, name, True, ops, str(tmp_path / "a"), "serving", keep_open=True)
    try:
        before = d.f.anchors(d.pairs).tolist()
        served = [p for p, st in zip(m.pairs, m.proof_statuses()) if st == S.PROOF_OK]
        assert served == [p for p in m.pairs if (m.local(p[0]), p[1]) in m.present] and served
        op = ["resume_nodes", False, "nodes"]
        want = m.apply(op)
        got = d.apply(op)
        d.check(m, op, want, got)                                                           # every proof against the built dataset's
        assert got["n_dropped"] == 0 and got["n_restored"] > 0 and got["n_unproved"] == 0 and got["n_rejected"] == 0
        status = d.f.block_proofs(served, statuses_only=True)
        assert (status == pkg.FILL_PROOF_OK).all()
        assert d.f.anchors(d.pairs).tolist() == before
    finally:
        d.close()
    # the same session through cp2_fill_save / cp2_fill_resume / cp2_fill_keep_nodes: today's behaviour, kept
    ops = [["keep"]] + adds + [["save"], ["resume", False], ["keep"]]
    m2, _, _ = run(pkg, sctx, w, name, True, ops, str(tmp_path / "b"), "serving, plain")
    partial = [p for p, st in zip(m2.pairs, m2.proof_statuses()) if st == S.PROOF_PARTIAL]
    assert partial and set(partial) <= set(served)                                           # (run() has held the session to these statuses)


# ---- 2: adopt after a crash ---------------------------------------------------------------------------------------------------------------------
def test_adopt_after_a_crash_rests_on_the_restored_nodes(pkg, sctx, worlds, tmp_path):   # noqa: F811
    name = "b8"
    w = worlds(name, True)
    first = [["keep"], ["add", [[0, 1, "ok"], [1, 6, "ok"], [2, 0, "ok"]], None], ["save_nodes"], ["save"]]
    later = [["add", [[0, 0, "ok"], [0, 2, "ok"], [0, 5, "ok"], [1, 7, "ok"], [1, 2, "ok"], [3, 3, "ok"]], None]]       # reach the files; no save: the crash
    _, _, res = run(pkg, sctx, w, name, True, first + later + [["resume_nodes", False, "nodes"], ["adopt", 0, 0, False]], str(tmp_path / "a"), "crash")
    _, _, plain = run(pkg, sctx, w, name, True, first + later + [["resume", False], ["keep"], ["adopt", 0, 0, False]], str(tmp_path / "b"), "crash, plain")
    # block 1's path vouches for (0, 0) and, through the node above 2 and 3, for nothing else of slot 0's left half; its top sibling vouches
    # for nothing of the right half while 4, 6, 7 are not there; (1, 7) lies under the sibling of 6; slot 3 has nothing but its stated root
    # (the holes the writer left before block 5 of slot 0 and block 7 of slot 1 are covered by their files and read too: zeros, adopted by nobody)
    assert res[-1] == {"err": 0, "n_read": 16, "n_adopted": 2} and res[-2]["n_restored"] > 0
    assert plain[-1] == {"err": 0, "n_read": 16, "n_adopted": 0}
    assert res[-1]["n_adopted"] > plain[-1]["n_adopted"]


# ---- 3: a dropped block keeps its proved root ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b1", "b8"])
def test_a_dropped_block_keeps_its_proved_root(pkg, sctx, worlds, tmp_path, name):   # noqa: F811
    w = worlds(name, True)
    slot = S.SHAPES[name][1]
    b = S.SHAPES[name][0] - 1
    ops = [["keep"], ["add", [[slot, 0, "ok"], [slot, b, "ok"]], None], ["save_nodes"], ["damage", slot, "flip", b], ["resume_nodes", False, "nodes"]]
    m, d, res = run(pkg, sctx, w, name, True, ops, str(tmp_path), "dropped", keep_open=True)
    try:
        assert res[-1]["n_dropped"] == 1 and res[-1]["n_rejected"] == 0
        assert [slot, b] in d.f.missing()[0].tolist() and d.f.anchors([(slot, b)]).tolist() == [0]
        op = ["anchored", [[slot, b, 0, "ok"]], None]                                       # bare bytes, no sibling
        want = m.apply(op)
        got = d.apply(op)
        d.check(m, op, want, got)
        assert got["status"] == [S.FILL_NEW] and got["n_new"] == 1
        assert d.f.block_proofs([(slot, b)], statuses_only=True).tolist() == [pkg.FILL_PROOF_OK]
    finally:
        d.close()


# ---- 4: the pre-keep frontier ---------------------------------------------------------------------------------------------------------------------
def test_nodes_derived_before_keep_survive_and_are_unproved_once_their_blocks_are_gone(pkg, sctx, worlds, tmp_path):   # noqa: F811
    name = "b8"
    w = worlds(name, True)
    ops = [["add", [[0, 0, "ok"], [0, 1, "ok"], [1, 4, "ok"]], None], ["keep"], ["save_nodes"], ["resume_nodes", False, "nodes"]]
    m, d, res = run(pkg, sctx, w, name, True, ops, str(tmp_path), "frontier", keep_open=True)
    try:
        assert res[-1] == {"err": 0, "n_dropped": 0, "n_restored": 0, "n_unproved": 0, "n_rejected": 0}      # presence gives all of it back
        assert d.f.anchors([(0, 0), (0, 1), (0, 2), (1, 4), (1, 5)]).tolist() == [0, 0, 3, 0, 3]
        assert m.row(1, 0, 0) in m.known and m.row(2, 0, 0) not in m.known                  # the node above 0 and 1 is a frontier node
        for op in (["damage", 0, "flip", 0], ["resume_nodes", False, "nodes"]):
            want = m.apply(op)
            got = d.apply(op)
            d.check(m, op, want, got)
        # block 0's root and the node above 0 and 1: nothing the resumed session knows vouches for either
        assert got == {"err": 0, "n_dropped": 1, "n_restored": 0, "n_unproved": 2, "n_rejected": 0}
        assert m.row(1, 0, 0) not in m.known and m.row(0, 0, 0) not in m.known
        assert d.f.anchors([(0, 0), (0, 1)]).tolist() == [3, 0]
    finally:
        d.close()


# ---- 5: a forged checkpoint -------------------------------------------------------------------------------------------------------------------------
def test_a_forged_node_is_rejected_with_its_sibling_and_serves_nothing(pkg, sctx, worlds, tmp_path):   # noqa: F811
    name = "b8"
    w = worlds(name, True)
    ops = [["keep"], ["add", [[0, 3, "ok"], [2, 5, "ok"]], None], ["save_nodes"]]
    m, d, _ = run(pkg, sctx, w, name, True, ops, str(tmp_path), "forged", keep_open=True)
    try:
        ck = N2.parse_checkpoint2(open(d.nckpt, "rb").read())
        forged = m.row(1, 0, 1)                                                             # the node above blocks 2 and 3 of slot 0
        assert forged in ck["mid"] and m.row(1, 0, 0) in ck["mid"]
        ck["mid"][forged] = ck["mid"][forged].copy()
        ck["mid"][forged][7] ^= 0x04
        bad_value = ck["mid"][forged].tobytes()
        with open(d.nckpt, "wb") as fh:
            fh.write(N2.write_checkpoint2(ck))                                              # the checksum is valid
        d.f.free()
        f = d.f = sctx.fill_resume_nodes(d.cfg, w.roots, d.nckpt, d.first, d.n_local)
        saved = {r for r in range(m.rows) if ck["known"][r] and r < m.offs[-1]}
        derived = {m.row(0, 0, 3), m.row(0, 2, 5)}
        # the forged node and its sibling candidate are rejected; block 2's root under it is reached by nobody; everything else comes back
        assert (f.n_dropped, f.n_rejected, f.n_unproved) == (0, 2, 1) and f.n_restored == len(saved - derived) - 3
        assert f.anchors([(0, 3), (0, 2), (0, 0), (0, 4), (2, 5), (2, 4)]).tolist() == [0, 2, 2, 2, 0, 0]
        status, roots, paths = f.block_proofs(d.pairs)
        want = [pkg.FILL_PROOF_PARTIAL if p == (0, 3) else pkg.FILL_PROOF_OK if p == (2, 5) else pkg.FILL_PROOF_ABSENT for p in d.pairs]
        assert status.tolist() == want
        assert bad_value not in roots.tobytes() and bad_value not in paths.tobytes()
        assert paths[d.pairs.index((2, 5))].tobytes() == w.src.paths[d.pairs.index((2, 5))].tobytes()
        # the resumed session saves what it knows, not what it was told: the rejected rows are gone from the file
        f.save_nodes(d.nckpt + ".2")
        again = N2.parse_checkpoint2(open(d.nckpt + ".2", "rb").read())
        assert {r for r in range(m.offs[-1]) if again["known"][r]} == saved - {forged, m.row(1, 0, 0), m.row(0, 0, 2)}
        assert bad_value not in open(d.nckpt + ".2", "rb").read()
        # it completes with the levels cp2_fill_anchors names, serving true proofs throughout, and finishes as the built dataset
        while f.missing(0)[1]:
            batch = [tuple(p) for p in f.missing(16)[0].tolist()]
            st, n_new, _ = w.add_anchored(f, batch)
            assert (st == pkg.FILL_NEW).all() and n_new == len(batch)
            status, roots, paths = f.block_proofs(d.pairs)
            for i in np.nonzero(status == pkg.FILL_PROOF_OK)[0]:
                assert roots[i].tobytes() == w.src.roots[i].tobytes() and paths[i].tobytes() == w.src.paths[i].tobytes()
        w.check_finished(pkg, f)
    finally:
        d.close()


# ---- 6: other formats and refusals ------------------------------------------------------------------------------------------------------------------
def test_a_plain_checkpoint_resumes_as_resume_and_keep(pkg, sctx, worlds, tmp_path):   # noqa: F811
    name = "b8"
    w = worlds(name, True)
    head = [["keep"]] + half_in_shuffled_order(S.SessionModel(S.SHAPES[name]), 2) + [["save"], ["damage", 1, "truncate", 9]]
    seen = []
    for tail in ([["resume_nodes", False, "plain"]], [["resume", False], ["keep"]]):
        m, d, res = run(pkg, sctx, w, name, True, head + tail, str(tmp_path / str(len(seen))), "plain format", keep_open=True)
        try:
            status, roots, paths = d.f.block_proofs(d.pairs)
            d.f.save_nodes(d.nckpt)
            seen.append((res[len(head)]["n_dropped"], d.f.missing()[0].tolist(), d.f.anchors(d.pairs).tolist(), status.tolist(), roots.tobytes(), paths.tobytes(),
                         N2.parse_checkpoint2(open(d.nckpt, "rb").read())["known"]))
        finally:
            d.close()
    assert seen[0] == seen[1] and seen[0][0] > 0
    assert res[0]["err"] == 0


def test_refusals(pkg, sctx, worlds, tmp_path):   # noqa: F811
    name = "b8"
    w = worlds(name, True)
    ops = [["keep"], ["add", [[0, 3, "ok"], [1, 1, "ok"]], None], ["save_nodes"], ["save"]]
    m, d, _ = run(pkg, sctx, w, name, True, ops, str(tmp_path), "refusals", keep_open=True)
    L = sctx.L
    try:
        good = open(d.nckpt, "rb").read()
        roots = np.ascontiguousarray(w.roots)
        out = ctypes.c_void_p(77)
        counts = [ctypes.c_uint64(90 + i) for i in range(4)]
        refs = [ctypes.byref(c) for c in counts]

        def resume(path=d.nckpt, ctx=sctx.h, cfg=d.cfg, first=0, n_local=4, r=roots, flags=0, out_=out, call=L.cp2_fill_resume_nodes, extra=None):
            args = [ctx, ctypes.byref(cfg) if cfg is not None else None, first, n_local, r.ctypes.data if r is not None else None,
                    os.fsencode(path) if path is not None else None, flags, ctypes.byref(out_) if out_ is not None else None]
            return call(*args, *(refs if extra is None else extra))

        def untouched():
            return [c.value for c in counts] == [90, 91, 92, 93]

        # NULLs
        assert resume(ctx=None) == CP2_ERR_INVALID and resume(cfg=None) == CP2_ERR_INVALID and resume(path=None) == CP2_ERR_INVALID
        assert resume(out_=None) == CP2_ERR_INVALID and out.value == 77 and untouched()
        assert resume(r=None) == CP2_ERR_INVALID and out.value is None and "slot_roots" in L.cp2_last_error(sctx.h).decode()
        assert L.cp2_fill_save_nodes(None, b"x") == CP2_ERR_INVALID and L.cp2_fill_save_nodes(d.f.h, None) == CP2_ERR_INVALID
        assert resume(flags=2) == CP2_ERR_INVALID and untouched()
        # the count outputs may be NULL
        assert resume(extra=[None] * 4) == CP2_OK
        L.cp2_fill_free(out)
        # a session without nodes, a finished session
        plain = sctx.fill(d.cfg, w.roots, 0, 4)
        with pytest.raises(pkg.CodexP2Error) as e:
            plain.save_nodes(d.nckpt + ".no")
        assert e.value.status == CP2_ERR_INVALID and "cp2_fill_keep_nodes" in str(e.value) and not os.path.exists(d.nckpt + ".no")
        plain.free()
        # another session's fields
        other = Q.config(pkg, 8, file=d.base + "x")
        assert resume(cfg=other) == CP2_ERR_INVALID and "file base name differs" in L.cp2_last_error(sctx.h).decode()
        assert resume(first=1, n_local=3, r=roots[1:].copy()) == CP2_ERR_INVALID and "first_slot differs" in L.cp2_last_error(sctx.h).decode()
        wrong = roots.copy()
        wrong[2, 0] ^= 1
        assert resume(r=wrong) == CP2_ERR_INVALID and "stated root of slot 2 differs" in L.cp2_last_error(sctx.h).decode()
        # CP2FILL2 into cp2_fill_resume: refused by its magic
        assert resume(call=L.cp2_fill_resume, extra=refs[:1]) == CP2_ERR_IO and "magic" in L.cp2_last_error(sctx.h).decode()
        # corrupt files: CP2_ERR_IO naming the path
        ck = N2.parse_checkpoint2(good)
        flipped = bytearray(good)
        flipped[len(good) // 2] ^= 1
        one_more = dict(ck, known=list(ck["known"]))
        free_row = next(r for r in range(32, m.offs[-1]) if not ck["known"][r])
        one_more["known"][free_row] = 1                                                    # a bit the packed rows do not back (the writer is told to leave it out)
        one_more["mid"] = dict(ck["mid"])
        one_more["mid"][free_row] = np.zeros(32, np.uint8)
        cases = {"trunc": (good[:-9], "no size its header allows"), "short": (good[:100], "truncated"), "sum": (bytes(flipped), "checksum"),
                 "pad": (N2.write_checkpoint2(ck, known_pad=1), "known bits past the last row"),
                 "more": (N2.write_checkpoint2(ck, extra_rows=1), "packed row"), "less": (N2.write_checkpoint2(one_more, extra_rows=-1), "packed row"),
                 "odd": (good[:-8] + bytes(8) + struct.pack("<Q", R.checksum64(good[:-8] + bytes(8))), "no size its header allows"),
                 "magic": (b"CP2FILL3" + good[8:], "magic")}
        assert m.rows % 64                                                                 # (there are bits past the last row)
        for key, (raw, word) in cases.items():
            path = str(tmp_path / ("bad_" + key))
            with open(path, "wb") as fh:
                fh.write(raw)
            assert resume(path=path) == CP2_ERR_IO, key
            err = L.cp2_last_error(sctx.h).decode()
            assert word in err and path in err and out.value is None and untouched(), (key, err)
        assert resume(path=str(tmp_path / "nothing")) == CP2_ERR_IO
        # a finished session
        for op in S._tail(copy.deepcopy(m)):
            d.check(m, op, m.apply(op), d.apply(op))
        assert m.finished
        with pytest.raises(pkg.CodexP2Error) as e:
            d.f.save_nodes(d.nckpt + ".late")
        assert e.value.status == CP2_ERR_INVALID and "finished" in str(e.value) and not os.path.exists(d.nckpt + ".late")
    finally:
        d.close()


# ---- 7: save properties, both sources, trusting the files -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("files", [True, False], ids=["files", "fake"])
def test_saves_are_identical_change_nothing_and_trusting_resumes_read_nothing(pkg, sctx, worlds, tmp_path, files):   # noqa: F811
    name = "b8"
    w = worlds(name, files)
    ops = [["keep"]] + half_in_shuffled_order(S.SessionModel(S.SHAPES[name], files), 3) + [["save_nodes"], ["proofs", [[0, 0], [1, 1]]], ["save_nodes"]]
    if files:
        ops += [["damage", 0, "remove", 0], ["resume_nodes", True, "nodes"], ["save_nodes"], ["resume_nodes", False, "nodes"]]
    else:
        ops += [["resume_nodes", True, "nodes"], ["save_nodes"], ["resume_nodes", False, "nodes"]]
    m, d, res = run(pkg, sctx, w, name, files, ops, str(tmp_path), "save properties", keep_open=True)     # (after every save: two saves identical, observables held)
    try:
        trusting, checking = [r for r in res if "n_restored" in r]
        assert trusting["n_dropped"] == 0 and trusting["n_unproved"] == 0 and trusting["n_restored"] > 0
        assert (checking["n_dropped"] > 0) == files
        if files:
            assert checking["n_unproved"] + checking["n_restored"] > 0
    finally:
        d.close()


# ---- 8: completion ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b1", "b2", "b8", "b64"])
def test_a_resumed_session_completes_into_the_built_dataset(pkg, sctx, worlds, tmp_path, name):   # noqa: F811
    w = worlds(name, True)
    head = [["keep"]] + half_in_shuffled_order(S.SessionModel(S.SHAPES[name]), 4)[:3] + [["save_nodes"], ["resume_nodes", False, "nodes"]]
    m = N2.NodeSessionModel(S.SHAPES[name], True)
    for op in head:
        m.apply(op)
    ops = head + S._tail(m)                                                                 # anchored adds at the lowest levels, finish, the refusals after it
    m, _, res = run(pkg, sctx, w, name, True, ops, str(tmp_path), "completion")
    assert m.finished and res[len(head) - 1]["n_rejected"] == 0 and res[len(head) - 1]["n_unproved"] == 0


# ---- 9: random sequences ----------------------------------------------------------------------------------------------------------------------------
CASES = [(name, True, seed) for name in ("b2", "b8", "b64") for seed in S.SEEDS[name][:2]] + [("b8", False, 1), ("b16", False, 2)]
TOTALS = {}


@pytest.mark.parametrize("name,files,seed", CASES, ids=["%s-%s-%d" % (n, "files" if f else "fake", s) for n, f, s in CASES])
def test_a_random_sequence_with_node_checkpoints_agrees_with_the_model_after_every_step(pkg, sctx, worlds, tmp_path, name, files, seed):   # noqa: F811
    ops = N2.sequence(seed, S.SHAPES[name], S.STEPS[name], files)
    m, _, _ = run(pkg, sctx, worlds(name, files), name, files, ops, str(tmp_path), seed)
    assert m.finished
    TOTALS[(name, files, seed)] = m.cov


def test_summary(capsys):
    assert TOTALS, "no sequence ran"
    total = sum(TOTALS.values(), type(next(iter(TOTALS.values())))())
    with capsys.disabled():
        print("\n[fill node ckpt sequences] %d sequences: %s" % (len(TOTALS), ", ".join("%s %d" % (k, total[k]) for k in sorted(total) if total[k])))
    if len(TOTALS) == len(CASES):
        assert total["op:save_nodes"] and total["op:resume_nodes"] and total["nodes_restored"]
