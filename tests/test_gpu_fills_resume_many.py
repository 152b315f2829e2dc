"""GPU suite: cp2_fills_resume_many -- many fill sessions resumed from their checkpoints in one pass.  The call is defined by the call that
exists, so it is held against twins: the same sessions over copies of the same files, saved and freed, are resumed once by ONE call and
once by a loop of cp2_fill_resume, and every observable must agree -- n_dropped, the missing list, dropped blocks accepted again as NEW,
and a finished dataset whose roots are the C oracle's and whose proof input is cp2_dataset_build's, byte for byte.  Sessions differ in
blocks per slot (1, 2, 8), range (1 and 3 slots, not all from slot 0), source (slot files and fake, in turn) and fill (empty, full, half).
Damage between save and resume -- a flipped byte, a file cut in the middle of a block, a deleted file, a forged layer-0 row under a
valid checksum -- is an ordinary verdict, dropped in exactly the session it belongs to: nothing here faults.  Refusals are all or nothing.
The checkpoint is read and written by tests/fill_resume_models.py from the documented layout alone."""
import ctypes
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fill_resume_models as M
from test_gpu_fill import Source, add, build_compact
from test_gpu_fill_resume import tuples, uneven_half

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CP2_OK, CP2_ERR_INVALID, CP2_ERR_IO = 0, -1, -5
# (source, nCells, nSlots, first_slot, n_local, fill): cell 128, block 4096, so 8, 2 and 1 blocks a slot
SPECS = [("file", 256, 5, 2, 3, "half"), ("fake", 64, 4, 0, 1, "full"), ("file", 32, 4, 1, 3, "full"), ("fake", 256, 5, 2, 3, "half"),
         ("file", 64, 3, 0, 1, "empty"), ("fake", 32, 4, 1, 3, "half"), ("file", 256, 5, 0, 1, "half")]


@pytest.fixture(autouse=True)
def time_limit():
    """every case under its own limit: a hang ends the process with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def sctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class Sess:
    """one session of a world: its config, range, stated roots, the built dataset it must become, what peers send, what it holds, its files"""


def make_session(pkg, ctx, d, k, spec):
    kind, n_cells, n_slots, first, n_local, fill = spec
    s = Sess()
    s.kind, s.first, s.n_local = kind, first, n_local
    s.cfgd = dict(maxDepth=16, maxLog2NSlots=3, cellSize=128, blockSize=4096, nSlots=n_slots, nCells=n_cells, nSamples=3, seed=10 + k)
    s.path = os.path.join(d, "session%d.ckpt" % k)
    if kind == "file":
        s.base = os.path.join(d, "s%d_" % k)
        nb = n_cells * 128 // 4096
        rng = np.random.default_rng([0xF11E, k])                                        # the same bytes in every world
        data = {slot: rng.integers(0, 256, (nb, 4096), dtype=np.uint8) for slot in range(first, first + n_local)}
        for slot, a in data.items():
            a.tofile("%s%d.dat" % (s.base, slot))
        s.data = data
        s.cfg = pkg.make_config(file=s.base, **s.cfgd)
        s.built = build_compact(ctx, s.cfg, first, n_local)
        s.roots = s.built.local_roots().copy()
        s.all_roots = np.zeros((n_slots, 32), dtype=np.uint8)
        s.all_roots[first:first + n_local] = s.roots
        s.src = Source(ctx, s.cfg, s.built, first, n_local, blocks_of=lambda slot: data[slot])
    else:
        s.base = None
        s.cfg = pkg.make_config(**s.cfgd)
        whole = build_compact(ctx, s.cfg)
        s.all_roots = whole.local_roots().copy()
        whole.free()
        s.built = build_compact(ctx, s.cfg, first, n_local)
        s.roots = s.all_roots[first:first + n_local].copy()
        s.src = Source(ctx, s.cfg, s.built, first, n_local)
    s.built.set_roots(s.all_roots)
    s.present = {"full": list(s.src.pairs), "empty": [], "half": uneven_half(s.src.pairs, seed=k)}[fill]
    f = ctx.fill(s.cfg, s.roots, first, n_local)
    if s.present:
        assert add(f, s.src, s.present)[1] == len(s.present)
    s.missing = tuples(f.missing()[0])
    f.save(s.path)
    f.free()
    return s


def make_world(pkg, ctx, d, specs=SPECS):
    os.makedirs(d)
    return [make_session(pkg, ctx, d, k, spec) for k, spec in enumerate(specs)]


def free_world(world):
    for s in world:
        s.built.free()


def damage(world):
    """between save and resume, the same in every world; returns per session what a re-check must drop"""
    want = {k: [] for k in range(len(world))}
    s = world[0]                                                                        # a flipped byte
    slot, b = sorted(s.present)[len(s.present) // 2]
    with open("%s%d.dat" % (s.base, slot), "r+b") as fh:
        fh.seek(b * 4096 + 1000)
        fh.write(bytes([s.data[slot][b][1000] ^ 0x04]))
    want[0] = [(slot, b)]
    s = world[6]                                                                        # a file cut in the middle of block 4
    os.truncate("%s%d.dat" % (s.base, 0), 4 * 4096 + 2048)
    want[6] = sorted(p for p in s.present if p[1] >= 4)
    s = world[2]                                                                        # a deleted file
    os.remove("%s%d.dat" % (s.base, 2))
    want[2] = [(2, 0)]
    s = world[3]                                                                        # a forged layer-0 row, resealed
    c = M.parse_checkpoint(open(s.path, "rb").read())
    slot, b = sorted(s.present)[1]
    g = (slot - s.first) * s.src.nb + b
    assert c["bits"][g] == 1
    c["layer0"][g, 9] ^= 0x20
    open(s.path, "wb").write(M.write_checkpoint(c))
    want[3] = [(slot, b)]
    assert all(want[k] for k in (0, 2, 3, 6))
    return want


def resume_many(pkg, ctx, world, trust=False):
    return pkg.fills_resume_many(ctx, [s.cfg for s in world], [s.roots for s in world], [s.path for s in world],
                                 ranges=[(s.first, s.n_local) for s in world], trust_files=trust)


def complete_and_compare(pkg, oracle, s, g):
    """what is missing sent again: NEW; the finished dataset: the stated roots (the C oracle's for the fake source), one proof input byte for
    byte cp2_dataset_build's"""
    C, _ = oracle
    missing = tuples(g.missing()[0])
    if missing:
        status, n_new = add(g, s.src, missing)
        assert (status == pkg.FILL_NEW).all() and n_new == len(missing)
    filled = g.finish()
    roots = filled.local_roots()
    assert roots.tobytes() == s.roots.tobytes()
    if s.kind == "fake":
        for k in range(s.n_local):
            assert roots[k].tobytes() == C.fake_slot_root(C.slot_seed(s.cfg.seed, s.first + k), 128, 4096, s.cfg.n_cells, 4).tobytes()
    else:
        for slot, a in s.data.items():
            assert open("%s%d.dat" % (s.base, slot), "rb").read() == a.tobytes()       # what was dropped is written again
    filled.set_roots(s.all_roots)
    assert filled.proof_input(s.first, 777).json() == s.built.proof_input(s.first, 777).json()
    filled.free()


# ---- 1 and 2: against twins, undamaged and damaged, with the re-check and without ----------------------------------------------------------
@pytest.mark.parametrize("trust,damaged", [(False, False), (True, False), (False, True), (True, True)])
def test_one_call_against_the_loop_over_twins(pkg, oracle, sctx, tmp_path, trust, damaged):
    one = make_world(pkg, sctx, str(tmp_path / "one"))
    two = make_world(pkg, sctx, str(tmp_path / "two"))
    want = {k: [] for k in range(len(one))}
    if damaged:
        want = damage(one)
        assert damage(two) == want
    many, n_dropped = resume_many(pkg, sctx, one, trust)
    loop = [sctx.fill_resume(s.cfg, s.roots, s.path, s.first, s.n_local, trust_files=trust) for s in two]
    assert n_dropped.dtype == np.uint64 and len(many) == len(one)
    for k, (a, b, s) in enumerate(zip(many, loop, one)):
        assert a.n_dropped == b.n_dropped == int(n_dropped[k]), k
        assert tuples(a.missing()[0]) == tuples(b.missing()[0]), k
        if trust:
            assert a.n_dropped == 0 and tuples(a.missing()[0]) == s.missing, k
        else:                                                                          # each damage in exactly the session it belongs to
            assert a.n_dropped == len(want[k]) and tuples(a.missing()[0]) == sorted(s.missing + want[k]), k
    if not (trust and damaged):                                                        # (trusted damage is finish's and scrub's to find)
        for world, sessions in ((one, many), (two, loop)):
            for s, g in zip(world, sessions):
                complete_and_compare(pkg, oracle, s, g)
    for g in many + loop:
        g.free()
    free_world(one)
    free_world(two)


# ---- 3: all or nothing ------------------------------------------------------------------------------------------------------------------------
def raw_call(pkg, ctx, entries, flags=0):
    """entries: (cfg, first, n_local, roots, path), any of cfg, roots and path None; returns (status, message, out handles, n_dropped)"""
    k = len(entries)
    keep = [None if e[3] is None else np.ascontiguousarray(e[3]) for e in entries]
    cs = (ctypes.c_void_p * k)(*[None if e[0] is None else ctypes.addressof(e[0]) for e in entries])
    rg = np.array([(e[1], e[2]) for e in entries], dtype=np.uint64)
    rs = (ctypes.c_void_p * k)(*[None if r is None else r.ctypes.data for r in keep])
    ps = (ctypes.c_char_p * k)(*[None if e[4] is None else os.fsencode(e[4]) for e in entries])
    out = (ctypes.c_void_p * k)(*([0x5E] * k))
    dropped = np.full(k, 42, dtype=np.uint64)
    st = ctx.L.cp2_fills_resume_many(ctx.h, cs, pkg._p(rg), rs, ps, k, flags, out, pkg._p(dropped))
    return st, ctx.L.cp2_last_error(ctx.h).decode(), list(out), dropped.tolist()


def test_refusals_are_all_or_nothing(pkg, sctx, tmp_path):
    world = make_world(pkg, sctx, str(tmp_path / "w"), SPECS[:5])
    good = [(s.cfg, s.first, s.n_local, s.roots, s.path) for s in world]
    raw = open(world[3].path, "rb").read()
    cut = str(tmp_path / "cut.ckpt")
    open(cut, "wb").write(raw[:len(raw) - 40])
    s3 = world[3]
    other = (pkg.make_config(**dict(s3.cfgd, seed=99)), s3.first, s3.n_local, s3.roots, s3.path)
    foreign = (pkg.make_config(**dict(s3.cfgd, blockSize=8192)), s3.first, s3.n_local, s3.roots, s3.path)
    later = (s3.cfg, s3.first, s3.n_local, s3.roots, str(tmp_path / "gone.ckpt"))
    cases = [
        ((s3.cfg, s3.first, s3.n_local, s3.roots, cut), 0, CP2_ERR_IO, ["fills: entry 3:", cut, "truncated"]),
        (other, 0, CP2_ERR_INVALID, ["fills: entry 3:", s3.path, "describes another session", "seed differs"]),
        (foreign, 0, CP2_ERR_INVALID, ["fills: entry 3:", "block_size 8192", "entry 0's"]),
        ((None, s3.first, s3.n_local, s3.roots, s3.path), 0, CP2_ERR_INVALID, ["fills: entry 3:", "cfgs[3] is NULL"]),
        ((s3.cfg, s3.first, s3.n_local, None, s3.path), 0, CP2_ERR_INVALID, ["fills: entry 3:", "slot_roots[3] is NULL"]),
        ((s3.cfg, s3.first, s3.n_local, s3.roots, None), 0, CP2_ERR_INVALID, ["fills: entry 3:", "paths[3] is NULL"]),
        (good[3], 6, CP2_ERR_INVALID, ["unknown resume flag bits 0x6"]),
    ]
    for bad, flags, status, words in cases:
        entries = good[:3] + [bad] + good[4:] + [good[0]]                              # one bad entry among five good ones
        st, msg, out, dropped = raw_call(pkg, sctx, entries, flags)
        assert st == status and out == [None] * 6 and dropped == [42] * 6, (st, msg)
        for w in words:
            assert w in msg, msg
    # arguments before checkpoints, the lowest index inside each: entry 4's NULL wins over entry 1's missing checkpoint
    entries = [good[0], later, good[2], good[3], (None, 0, 1, world[4].roots, world[4].path)]
    st, msg, out, _ = raw_call(pkg, sctx, entries)
    assert st == CP2_ERR_INVALID and "cfgs[4] is NULL" in msg and out == [None] * 5
    st, msg, out, _ = raw_call(pkg, sctx, [good[0], later, good[2], (s3.cfg, s3.first, s3.n_local, s3.roots, cut)])
    assert st == CP2_ERR_IO and "fills: entry 1:" in msg and "cannot open" in msg and out == [None] * 4
    # nothing leaked into the context: the same call without the bad entry succeeds on it, and again
    for _ in range(2):
        sessions, n_dropped = resume_many(pkg, sctx, world)
        assert n_dropped.tolist() == [0] * 5
        for s, g in zip(world, sessions):
            assert tuples(g.missing()[0]) == s.missing
            g.free()
    free_world(world)


# ---- 4: the edges -------------------------------------------------------------------------------------------------------------------------------
def test_no_entry_and_one_entry(pkg, oracle, sctx, tmp_path):
    sessions, n_dropped = pkg.fills_resume_many(sctx, [], [], [])
    assert sessions == [] and n_dropped.tolist() == []
    assert sctx.L.cp2_fills_resume_many(sctx.h, None, None, None, None, 0, 0, None, None) == CP2_OK
    one = make_world(pkg, sctx, str(tmp_path / "one"), [SPECS[0]])
    two = make_world(pkg, sctx, str(tmp_path / "two"), [SPECS[0]])
    want = None
    for world in (one, two):                                                            # the same flipped byte in both
        s = world[0]
        slot, b = sorted(s.present)[0]
        with open("%s%d.dat" % (s.base, slot), "r+b") as fh:
            fh.seek(b * 4096 + 4095)
            fh.write(bytes([s.data[slot][b][4095] ^ 0x80]))
        want = [(slot, b)]
    (a,), n_dropped = resume_many(pkg, sctx, one)
    s = two[0]
    b = sctx.fill_resume(s.cfg, s.roots, s.path, s.first, s.n_local)
    assert a.n_dropped == b.n_dropped == int(n_dropped[0]) == 1
    assert tuples(a.missing()[0]) == tuples(b.missing()[0]) == sorted(s.missing + want)
    complete_and_compare(pkg, oracle, one[0], a)
    complete_and_compare(pkg, oracle, two[0], b)
    for h in (a, b):
        h.free()
    free_world(one)
    free_world(two)


# ---- 5: chunk edges, in a fresh child under 1 MiB of staging --------------------------------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
import __graft_entry__ as g
pkg = g.load_package()
job = json.loads(sys.argv[1])
ctx = pkg.Context(0)
cfgs = [pkg.make_config(**c) for c in job["configs"]]
sessions, n_dropped = pkg.fills_resume_many(ctx, cfgs, [np.load(r) for r in job["roots"]], job["paths"])
out = {"n_dropped": n_dropped.tolist(), "missing": [s.missing()[0].tolist() for s in sessions]}
for s in sessions:
    s.free()
ctx.close()
print(json.dumps(out), flush=True)
""" % ROOT


def test_chunk_edges_in_a_child_under_small_staging(pkg, sctx, tmp_path):
    """64 KiB blocks and 1 MiB of staging: chunks of 8 blocks.  17 present blocks over three sessions (7 fake, 4 from a slot file, 6 fake): two
    full chunks and a lone last block.  Damage at the last block of the first chunk (request 7, a flipped byte on disk), the first of the
    next (request 8, the same file) and the lone last one (request 16, a forged row): exactly those are dropped, as in this process under
    the default staging, where all 17 are one chunk."""
    d = str(tmp_path)
    base = dict(maxDepth=16, maxLog2NSlots=3, cellSize=64, blockSize=65536, nCells=4096, nSamples=3)
    shapes = [dict(base, nSlots=2, seed=31), dict(base, nSlots=1, seed=32, file=os.path.join(d, "mid_")), dict(base, nSlots=2, seed=33)]
    held_back = [[(1, 2)], [], [(0, 0), (1, 3)]]
    cfgs, roots, paths, present = [], [], [], []
    for k, shape in enumerate(shapes):
        fake_cfg = pkg.make_config(**{key: v for key, v in shape.items() if key != "file"})
        built = build_compact(sctx, fake_cfg)
        src = Source(sctx, fake_cfg, built, 0, shape["nSlots"])
        cfg = pkg.make_config(**shape)                                                  # the same bytes in a slot file: the same roots
        r = built.local_roots().copy()
        f = sctx.fill(cfg, r)
        here = [p for p in src.pairs if p not in held_back[k]]
        assert add(f, src, here)[1] == len(here)
        path = os.path.join(d, "edge%d.ckpt" % k)
        f.save(path)
        f.free()
        built.free()
        np.save(os.path.join(d, "roots%d.npy" % k), r)
        cfgs.append(cfg); roots.append(r); paths.append(path); present.append(here)
    assert [len(p) for p in present] == [7, 4, 6]
    victims = [[], [(0, 0), (0, 1)], [present[2][-1]]]                                  # requests 7, 8 and 16 of the plan
    for slot, b in victims[1]:
        with open("%s%d.dat" % (shapes[1]["file"], slot), "r+b") as fh:
            fh.seek(b * 65536 + 65535 - b)
            byte = fh.read(1)
            fh.seek(-1, os.SEEK_CUR)
            fh.write(bytes([byte[0] ^ 0x80]))
    c = M.parse_checkpoint(open(paths[2], "rb").read())
    slot, b = victims[2][0]
    c["layer0"][slot * 4 + b, 3] ^= 0x01
    open(paths[2], "wb").write(M.write_checkpoint(c))

    sessions, n_dropped = pkg.fills_resume_many(sctx, cfgs, roots, paths)              # here: the default staging
    here = {"n_dropped": n_dropped.tolist(), "missing": [s.missing()[0].tolist() for s in sessions]}
    for s in sessions:
        s.free()
    assert here["n_dropped"] == [0, 2, 1]
    assert here["missing"] == [sorted(list(p) for p in held_back[k] + victims[k]) for k in range(3)]

    clean = {k: v for k, v in os.environ.items() if not k.startswith("CODEX_P2_")}
    job = dict(configs=shapes, roots=[os.path.join(d, "roots%d.npy" % k) for k in range(3)], paths=paths)
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(job)], capture_output=True, text=True, timeout=100,
                       env=dict(clean, CODEX_P2_STAGE_MB="1", CP2_TRACE="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]) == here
    trace = [ln for ln in r.stderr.splitlines() if "fills resume many" in ln]
    assert len(trace) == 1 and "3 session(s), 17 block(s) present in the checkpoints, 17 re-read, 3 dropped, 3 chunk(s)" in trace[0], r.stderr[-2000:]
