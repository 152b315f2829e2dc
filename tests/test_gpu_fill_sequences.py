"""GPU suite: fill sessions driven through seeded random sequences of interleaved operations -- add, keep_nodes, anchored add, anchors,
block proofs, missing, save, free + resume (re-checking and trusting), damage to the slot files, blocks placed as a crashed writer leaves
them, adopt (reading and no_read), finish -- against one model of the whole session (tests/fill_session_model.py).  The scenario files
check each feature and a few hand-picked crossings; here the features meet in orders nobody scripted, and after EVERY step everything a
caller can observe is compared, bit-exactly: the operation's own result, missing, anchors, every block proof (against the dataset built
from the true data), the slot files byte for byte, and -- using the model only for which operation ran -- that every served proof verifies
with the true block against the stated slot root (cp2_blocks_verify) and that no adopt took a block whose bytes on disk are not the true ones.
Every sequence ends complete and finishes into the dataset cp2_dataset_build makes.  The geometry is the smallest of the fill tests (cells of
64 bytes, blocks of 256, four slots); tests/test_fill_session_model_cpu.py holds the model to the product's host plans and checks, for these
very seeds and step counts, that the sequences cross what they are meant to cross.  A failing run prints the seed, the shape and the
operations up to the failing step as a list that REPLAY below takes back."""
import faulthandler
import os
import stat
import time
from collections import Counter

import numpy as np
import pytest

import fill_resume_models as R
import fill_session_model as S
from test_gpu_fill import flip
from test_gpu_fill_anchored import World as WholeWorld
from test_gpu_fill_serve import World as RangeWorld
from test_gpu_fill_serve import config

pytestmark = pytest.mark.gpu

RANGE_NAMES = {"b1": "one_block", "b2": "two_blocks", "b16": "sixteen_blocks"}       # tests/test_gpu_fill_serve.py's names for these shapes
CASES = [(name, True, seed) for name in S.SHAPES for seed in S.SEEDS[name]] + [(name, False, seed) for name in S.FAKE_SHAPES for seed in S.FAKE_SEEDS[name]]
# literal sequences: (shape name, slot files?, operations).  A failure's printed list goes here as a regression case.
REPLAY = [
    # an unwritten block's nodes let an adopt take its neighbours; the checkpoint of the keeping session resumes as a plain one
    ("b8", True, [["keep"], ["place", 1, [2, 3]], ["adopt", 1, 1, False], ["add", [[1, 0, "ok"], [1, 1, "ok"]], 1], ["adopt", 1, 1, True],
                  ["anchored", [[1, 4, 1, "ok"]], None], ["save"], ["resume", False], ["proofs", [[1, 2]]], ["keep"],
                  ["anchored", [[1, 0, 3, "ok"], [1, 1, 3, "sib"], [1, 1, 3, "ok"]], None], ["adopt", 0, 0, False]]),
]
TOTALS, SLOWEST = {}, [0.0, None]


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def sctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worlds(pkg, sctx, tmp_path_factory):
    """per shape and source the dataset built from the true data and what the peers would send, made once and never changed"""
    made = {}

    def world(name, files):
        if (name, files) not in made:
            directory = str(tmp_path_factory.mktemp("world_" + name)) if files else None
            if name in RANGE_NAMES:
                made[(name, files)] = RangeWorld(pkg, sctx, RANGE_NAMES[name], directory)
            else:
                made[(name, files)] = WholeWorld(pkg, sctx, S.SHAPES[name][0], directory)
        return made[(name, files)]

    yield world
    for w in made.values():
        w.free()


class Driver:
    """one real session beside the model: apply() runs an operation and reports it in the model's words, check() compares what can be seen"""

    def __init__(self, pkg, ctx, w, shape, files, directory):
        self.pkg, self.ctx, self.w, self.files = pkg, ctx, w, files
        self.nb, self.first, self.n_local = shape
        assert (w.nb, w.first, w.n_local) == tuple(shape)
        self.pairs = [tuple(p) for p in w.pairs]
        self.ckpt = os.path.join(directory, "session.ckpt")
        self.out_dir = os.path.join(directory, "out")
        os.makedirs(self.out_dir)
        self.base = os.path.join(self.out_dir, "slot")
        self.cfg = config(pkg, self.nb, file=self.base) if files else w.cfg
        self.f = ctx.fill(self.cfg, w.roots, self.first, self.n_local)
        self.expect = {s: None for s in range(self.first, self.first + self.n_local)}     # what each slot file must hold: bytes, or None
        self.was_present = set()

    def name(self, slot):
        return "%s%d.dat" % (self.base, slot)

    def true_block(self, slot, b):
        return self.w.src.blocks[slot][b].tobytes()

    # ---- the files, as the sequence and the product change them ---------------------------------------------------------------------------
    def put(self, slot, b, on_disk):
        cur = bytearray(self.expect[slot] or b"")
        cur.extend(bytes(max(0, (b + 1) * 256 - len(cur))))
        cur[b * 256:(b + 1) * 256] = self.true_block(slot, b)
        self.expect[slot] = bytes(cur)
        if on_disk:
            with open(self.name(slot), "wb") as fh:
                fh.write(cur)

    def unwritable(self, slot):
        """the file of `slot` cannot be written while the returned undo has not run: for a user whom modes do not bind, a directory in the
        file's place (tests/test_gpu_fill_serve.py)"""
        name, kept = self.name(slot), self.name(slot) + ".kept_aside"
        had = os.path.exists(name)
        if had:
            os.rename(name, kept)
        if os.geteuid() == 0:
            os.mkdir(name)
        else:
            os.chmod(self.out_dir, stat.S_IRUSR | stat.S_IXUSR)

        def undo():
            if os.geteuid() == 0:
                os.rmdir(name)
            else:
                os.chmod(self.out_dir, stat.S_IRWXU)
            if had:
                os.rename(kept, name)
        return undo

    # ---- one operation ---------------------------------------------------------------------------------------------------------------------
    def apply(self, op):
        try:
            return getattr(self, "op_" + op[0])(*op[1:])
        except self.pkg.CodexP2Error as e:
            if e.status == S.ERR_IO and hasattr(e, "fill_status"):
                return {"err": e.status, "status": e.fill_status.tolist(), "n_new": e.n_new}
            return {"err": e.status}

    def _added(self, call, pairs, fail_slot):
        undo = self.unwritable(fail_slot) if fail_slot is not None else None
        try:
            res = self.apply(["_call", call])
        finally:
            if undo:
                undo()
        for p, st in zip(pairs, res.get("status", [])):
            if st == S.FILL_NEW and self.files:
                self.put(p[0], p[1], on_disk=False)
        return res

    def op__call(self, call):
        status, n_new = call()
        return {"err": 0, "status": status.tolist(), "n_new": n_new}

    def op_add(self, reqs, fail_slot=None):
        pairs = [(s, b) for s, b, _ in reqs]
        data, paths = self.w.src.data(pairs), self.w.src.path(pairs)
        for i, (_, _, kind) in enumerate(reqs):
            if kind == "data":
                data[i] = flip(data[i], (17 + 31 * i) % 256)
            elif kind == "sib":
                paths[i] = flip(paths[i], (i % self.w.depth) * 32 + 5)
        return self._added(lambda: self.f.add(pairs, data, paths), pairs, fail_slot)

    def op_anchored(self, reqs, fail_slot=None):
        pairs = [(s, b) for s, b, _, _ in reqs]
        levels = np.array([lvl for _, _, lvl, _ in reqs], dtype=np.uint32)
        data = self.w.src.data(pairs)
        rows = [self.w.src.paths[self.w.src.index[p]][:int(lvl)].copy() for p, lvl in zip(pairs, levels)]
        for i, (_, _, lvl, kind) in enumerate(reqs):
            if kind == "data":
                data[i] = flip(data[i], (17 + 31 * i) % 256)
            elif kind == "sib":
                rows[i] = flip(rows[i], (i % lvl) * 32 + 5)
        packed = np.concatenate(rows + [np.zeros((0, 32), np.uint8)])
        return self._added(lambda: self.f.add_anchored(pairs, data, levels, packed), pairs, fail_slot)

    def op_keep(self):
        self.f.keep_nodes()
        return {"err": 0}

    def op_anchors(self, pairs):
        return {"err": 0, "levels": self.f.anchors(pairs).tolist()}

    def op_proofs(self, pairs):
        return {"err": 0, "status": self.f.block_proofs(pairs, statuses_only=True).tolist()}

    def op_missing(self, cap):
        lst, n = self.f.missing(cap)
        return {"err": 0, "missing": lst.tolist(), "n_missing": n}

    def op_save(self):
        self.f.save(self.ckpt)
        return {"err": 0}

    def op_resume(self, trust):
        self.f.free()
        self.f = self.ctx.fill_resume(self.cfg, self.w.roots, self.ckpt, self.first, self.n_local, trust_files=trust)
        self.was_present = None                           # a new session: what it holds is the checkpoint's, not an adopt's
        return {"err": 0, "n_dropped": self.f.n_dropped}

    def op_damage(self, slot, how, arg):
        if how == "remove":
            os.remove(self.name(slot))
            self.expect[slot] = None
            return {"err": 0}
        cur = bytearray(self.expect[slot])
        if how == "flip":
            cur[arg * 256 + 100] ^= 0x20
        else:
            del cur[arg * 128:]
        self.expect[slot] = bytes(cur)
        with open(self.name(slot), "wb") as fh:
            fh.write(cur)
        return {"err": 0}

    def op_place(self, slot, blocks):
        for b in blocks:
            self.put(slot, b, on_disk=True)
        return {"err": 0}

    def op_adopt(self, first_slot, n_slots, no_read):
        n_read, n_adopted = self.f.adopt(first_slot, n_slots, no_read=no_read)
        return {"err": 0, "n_read": n_read, "n_adopted": n_adopted}

    def op_finish(self):
        """a complete session finishes into the dataset cp2_dataset_build makes: local roots, every block proof and, where all four slots are
        local, the dataset root and one proof-input JSON byte for byte (World.check_finished)"""
        w = self.w
        if isinstance(w, WholeWorld):
            w.check_finished(self.pkg, self.f)
        else:
            filled = self.f.finish()
            try:
                assert filled.tree_mode == 2 and filled.local_roots().tobytes() == w.roots.tobytes()
                got_roots, got_paths = filled.block_proofs(w.pairs)
                assert got_roots.tobytes() == w.src.roots.tobytes() and got_paths.tobytes() == w.src.paths.tobytes()
            finally:
                filled.free()
        return {"err": 0}

    # ---- everything a caller can observe, after every step ------------------------------------------------------------------------------------
    def check(self, m, op, want, got):
        pkg, f, w = self.pkg, self.f, self.w
        assert got == want, ("the operation's result", got, want)
        lst, n = f.missing()
        gone = [list(p) for p in m.missing()]
        assert lst.tolist() == gone and n == len(gone) and f.missing(0)[1] == n, ("missing", lst.tolist(), gone)
        present = set(self.pairs) - {tuple(p) for p in lst.tolist()}
        if op[0] == "adopt" and self.was_present is not None:                             # the safety of an adopt, from the disk alone
            for s, b in sorted(present - self.was_present):
                on_disk = (self.expect[s] or b"")[b * 256:(b + 1) * 256]
                assert on_disk == self.true_block(s, b), ("adopted a block whose bytes on disk are not the true ones", s, b)
        self.was_present = present
        if self.files:                                                                    # the slot files, byte for byte
            names = sorted(os.path.basename(self.name(s)) for s in self.expect if self.expect[s] is not None)
            assert sorted(os.listdir(self.out_dir)) == names, ("files", sorted(os.listdir(self.out_dir)), names)
            for s, raw in self.expect.items():
                assert raw is None or open(self.name(s), "rb").read() == raw, ("the bytes of slot file", s)
        else:
            assert os.listdir(self.out_dir) == []
        if m.finished:
            for call in (lambda: f.anchors(self.pairs), lambda: f.block_proofs(self.pairs), lambda: f.save(self.ckpt + ".late"), f.keep_nodes):
                with pytest.raises(pkg.CodexP2Error) as e:
                    call()
                assert e.value.status == S.ERR_INVALID
            return
        assert f.anchors(self.pairs).tolist() == m.anchor_levels(), ("anchors", f.anchors(self.pairs).tolist(), m.anchor_levels())
        if not m.keeping:
            with pytest.raises(pkg.CodexP2Error) as e:                                      # a session that keeps no nodes serves nothing
                f.block_proofs(self.pairs)
            assert e.value.status == S.ERR_INVALID
            return
        status, roots, paths = f.block_proofs(self.pairs)
        assert status.tolist() == m.proof_statuses(), ("proof statuses", status.tolist(), m.proof_statuses())
        assert f.block_proofs(self.pairs, statuses_only=True).tolist() == status.tolist()
        ok = [i for i, st in enumerate(status.tolist()) if st == S.PROOF_OK]
        for i, p in enumerate(self.pairs):
            if status[i] == S.PROOF_OK:
                assert p in present and roots[i].tobytes() == w.src.roots[i].tobytes() and paths[i].tobytes() == w.src.paths[i].tobytes(), ("proof", p)
            else:
                assert not roots[i].any() and not paths[i].any(), ("rows of a proof that is not served", p)
        if ok:                                                                            # every served proof verifies with the true block
            served = [self.pairs[i] for i in ok]
            verdict, hashed = self.ctx.blocks_verify(self.cfg.cell_size, self.cfg.block_size, self.cfg.n_cells, w.roots,
                                                     [(s - self.first, b) for s, b in served], w.src.data(served), paths[ok])
            assert (verdict == pkg.BLOCK_MATCH).all() and hashed.tobytes() == roots[ok].tobytes(), ("a served proof does not verify", served)
        if op[0] == "save":                                                               # what a checkpoint keeps: presence and layer 0
            ck = R.parse_checkpoint(open(self.ckpt, "rb").read())
            assert ck["bits"] == m.checkpoint_bits()

    def close(self):
        self.f.free()


def run_sequence(pkg, ctx, w, name, files, ops, directory, what):
    shape = S.SHAPES[name]
    m = S.SessionModel(shape, files)
    d = Driver(pkg, ctx, w, shape, files, directory)
    assert d.pairs == m.pairs
    try:
        for k, op in enumerate(ops):
            try:
                want = m.apply(op)
                d.check(m, op, want, d.apply(op))
            except Exception as e:
                raise AssertionError("step %d, %r: %s: %s\n%s" % (k, op, type(e).__name__, e, S.describe(what, shape, files, ops[:k + 1]))) from None
    finally:
        d.close()
    return m


@pytest.mark.parametrize("name,files,seed", CASES, ids=["%s-%s-%d" % (n, "files" if f else "fake", s) for n, f, s in CASES])
def test_a_random_sequence_agrees_with_the_model_after_every_step(pkg, sctx, worlds, tmp_path, name, files, seed):
    t0 = time.time()
    ops = S.sequence(seed, S.SHAPES[name], S.STEPS[name], files)
    m = run_sequence(pkg, sctx, worlds(name, files), name, files, ops, str(tmp_path), seed)
    assert m.finished
    TOTALS.setdefault((name, files), Counter()).update(m.cov)
    TOTALS[(name, files)]["steps"] += len(ops)
    TOTALS[(name, files)]["cases"] += 1
    took = time.time() - t0
    if took > SLOWEST[0]:
        SLOWEST[:] = [took, "%s-%s-%d" % (name, "files" if files else "fake", seed)]


@pytest.mark.parametrize("case", range(len(REPLAY)))
def test_literal_sequences(pkg, sctx, worlds, tmp_path, case):
    name, files, ops = REPLAY[case]
    run_sequence(pkg, sctx, worlds(name, files), name, files, ops, str(tmp_path), "literal %d" % case)


def test_summary(capsys):
    """what ran on the device: per shape and source the operations by kind and how often each coverage condition was met"""
    assert TOTALS, "no sequence ran"
    with capsys.disabled():
        for (name, files), c in sorted(TOTALS.items()):
            print("\n[fill sequences] %s %s: %d steps; %s; %s" % (
                name, "slot files" if files else "fake source", c["steps"], ", ".join("%s %d" % (k, c["op:" + k]) for k in S.OP_KINDS if c["op:" + k]),
                ", ".join("%s %d" % (k, c[k]) for k in S.CONDITIONS if c[k])))
        print("[fill sequences] slowest case: %s, %.2f s" % (SLOWEST[1], SLOWEST[0]))
    for (name, files), c in TOTALS.items():                                             # where every seed of a shape ran, the device met what the CPU promised
        if files and S.SHAPES[name][0] >= 8 and c["cases"] == len(S.SEEDS[name]):
            assert all(c[k] for k in S.CONDITIONS), (name, dict(c))
