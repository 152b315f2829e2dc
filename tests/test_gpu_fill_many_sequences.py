"""GPU suite: cp2_fills_add_many under the seeded random sequences of tests/fill_session_model.py.  Three sessions of different shapes on
one context are driven in lockstep, each through its own generated sequence; at every step the sessions' `add` and `anchored` operations
are merged into ONE interleaved many-call, and every other operation (keep, save, resume, damage, place, adopt, the queries, finish) runs
per session as it does today.  After every step each session is compared with its own model exactly as tests/test_gpu_fill_sequences.py
compares (its Driver does it): the operation's result, missing, anchors, every block proof, the slot files byte for byte.

What the merge means for the model: a call with levels treats a keeping session's `add` as an anchored add at its depth.  An `anchored`
operation on a session that keeps no nodes is not merged: cp2_fill_add_anchored refuses it, the generated sequence goes on from that
refusal, and the many-call would accept its whole paths as plain adds -- so it runs per session like the other operations.  An operation
its session would refuse inside the merged call (an anchor below the known one, a finished session) refuses the WHOLE call, which must
change nothing anywhere, and the others' requests are then sent without it.  A failure prints the seed and the operations so far."""
import random

import numpy as np
import pytest

import fill_session_model as S
from test_gpu_fill import flip
from test_gpu_fill_sequences import Driver, sctx, time_limit, worlds  # noqa: F401  (the fixtures of the one-session sequences)

pytestmark = pytest.mark.gpu

# three shapes (name, slot files?) and the one seed their sequences are generated from
TRIPLES = [((("b1", True), ("b8", True), ("b64", True)), 1),
           ((("b2", True), ("b16", True), ("b64", True)), 2),
           ((("b8", False), ("b2", True), ("b16", False)), 2)]
SEEN = {"merged": 0, "levels": 0, "whole": 0, "refused": 0, "io": 0, "sessions in a call": 0}


def model_op(m, op, levels_given):
    """the operation the merged call performs on this session, in the model's words"""
    if op[0] == "add" and levels_given and m.keeping and not m.finished:
        return ["anchored", [[s, b, m.depth, kind] for s, b, kind in op[1]], op[2]]
    return op


def arrays(d, m, op):
    """one session's requests as (pairs, data, levels, path rows), damaged as tests/test_gpu_fill_sequences.py damages them"""
    reqs = [(r[0], r[1], r[2] if op[0] == "anchored" else m.depth, r[-1]) for r in op[1]]
    pairs = [(s, b) for s, b, _, _ in reqs]
    data = d.w.src.data(pairs)
    rows = [d.w.src.paths[d.w.src.index[p]][:int(lvl)].copy() for p, (_, _, lvl, _) in zip(pairs, reqs)]
    for i, (_, _, lvl, kind) in enumerate(reqs):
        if kind == "data":
            data[i] = flip(data[i], (17 + 31 * i) % 256)
        elif kind == "sib":
            rows[i] = flip(rows[i], (i % lvl) * 32 + 5)
    return pairs, data, [lvl for _, _, lvl, _ in reqs], rows


def many_call(pkg, ctx, rng, drivers, models, ops, ks, levels_given):
    """the add / anchored operations of sessions `ks` as one interleaved call; returns per session {"err", "status", "n_new"} or {"err"}"""
    fills = [k for k in range(len(drivers)) if k in ks or not models[k].finished]
    per = {k: arrays(drivers[k], models[k], ops[k]) for k in ks}
    left = {k: 0 for k in ks}
    order = []
    while any(left[k] < len(per[k][0]) for k in ks):                                 # a random merge that keeps each session's own order
        k = rng.choice([k for k in ks if left[k] < len(per[k][0])])
        order.append((k, left[k]))
        left[k] += 1
    req = np.array([(fills.index(k), per[k][0][i][0], per[k][0][i][1]) for k, i in order], dtype=np.uint64).reshape(-1, 3)
    data = np.stack([per[k][1][i] for k, i in order])
    levels = np.array([per[k][2][i] for k, i in order], dtype=np.uint32)
    paths = np.concatenate([per[k][3][i] for k, i in order] + [np.zeros((0, 32), np.uint8)])
    SEEN["sessions in a call"] = max(SEEN["sessions in a call"], len(ks))
    try:
        status, n_new = pkg.fills_add_many(ctx, [drivers[k].f for k in fills], req, data, paths if paths.size else None, levels if levels_given else None)
    except pkg.CodexP2Error as e:
        if e.status != S.ERR_IO:
            return {k: {"err": e.status} for k in ks}
        status, n_new = e.fill_status, e.n_new
    out = {}
    for k in ks:
        sub = [int(status[j]) for j, (kk, _) in enumerate(order) if kk == k]
        out[k] = {"err": S.ERR_IO if S.FILL_UNWRITTEN in sub else 0, "status": sub, "n_new": n_new[fills.index(k)]}
    return out


def lockstep(pkg, ctx, drivers, models, seqs, what):
    rng = random.Random("merge %r" % (what,))
    done = [[] for _ in seqs]
    for t in range(max(len(s) for s in seqs)):
        ops = [s[t] if t < len(s) else None for s in seqs]
        for k, op in enumerate(ops):
            if op:
                done[k].append(op)
        try:
            adds = [k for k, op in enumerate(ops) if op and (op[0] == "add" or (op[0] == "anchored" and (models[k].keeping or models[k].finished)))]
            for k, op in enumerate(ops):                                              # everything but the merged adds: per session, as today
                if op and k not in adds:
                    want = models[k].apply(op)
                    drivers[k].check(models[k], op, want, drivers[k].apply(op))
            if not adds:
                continue
            levels_given = any(ops[k][0] == "anchored" for k in adds)
            mops = {k: model_op(models[k], ops[k], levels_given) for k in adds}
            wants = {k: models[k].apply(mops[k]) for k in adds}
            refused = [k for k in adds if wants[k]["err"] == S.ERR_INVALID]
            SEEN["merged"] += len(adds) > 1
            SEEN["levels" if levels_given else "whole"] += 1
            got = {}
            if refused:                                                               # all or nothing: nobody's requests get in
                got = many_call(pkg, ctx, rng, drivers, models, ops, adds, levels_given)
                assert all(g == {"err": S.ERR_INVALID} for g in got.values()), got
                SEEN["refused"] += 1
            accepted = [k for k in adds if k not in refused]
            if accepted:
                undo = [drivers[k].unwritable(ops[k][2]) for k in accepted if ops[k][2] is not None]
                try:
                    got.update(many_call(pkg, ctx, rng, drivers, models, ops, accepted, levels_given))
                finally:
                    for u in undo:
                        u()
            for k in adds:
                d = drivers[k]
                SEEN["io"] += got[k]["err"] == S.ERR_IO
                for r, st in zip(ops[k][1], got[k].get("status", [])):
                    if st == S.FILL_NEW and d.files:
                        d.put(r[0], r[1], on_disk=False)
                d.check(models[k], ops[k], wants[k], got[k])
        except Exception as e:
            raise AssertionError("step %d, %r: %s: %s\n%s" % (t, ops, type(e).__name__, e, "\n".join(
                S.describe(what, (m.nb, m.first, m.n_local), d.files, ds) for m, d, ds in zip(models, drivers, done)))) from None


@pytest.mark.parametrize("case", range(len(TRIPLES)), ids=["-".join(n for n, _ in t) for t, _ in TRIPLES])
def test_three_sessions_in_lockstep_agree_with_their_models_after_every_step(pkg, sctx, worlds, tmp_path, case):  # noqa: F811
    triple, seed = TRIPLES[case]
    seqs = [S.sequence(seed, S.SHAPES[name], S.STEPS[name], files) for name, files in triple]
    models = [S.SessionModel(S.SHAPES[name], files) for name, files in triple]
    drivers = []
    try:
        for k, (name, files) in enumerate(triple):
            directory = tmp_path / ("session%d" % k)
            directory.mkdir()
            drivers.append(Driver(pkg, sctx, worlds(name, files), S.SHAPES[name], files, str(directory)))
        lockstep(pkg, sctx, drivers, models, seqs, seed)
    finally:
        for d in drivers:
            d.close()
    assert all(m.finished for m in models)


def test_summary(capsys):
    with capsys.disabled():
        print("\n[fill many sequences] %s" % ", ".join("%s %d" % kv for kv in SEEN.items()))
    assert SEEN["merged"] and SEEN["levels"] and SEEN["whole"] and SEEN["refused"] and SEEN["sessions in a call"] == 3, SEEN
