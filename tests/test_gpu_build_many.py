"""GPU suite: cp2_datasets_build_many -- n datasets of one context built in one pass are, request by request and in every observable, what
cp2_dataset_build returns for each request under the same kept mode: what they keep, their local roots and range, the dataset root after
cp2_dataset_set_roots, every block's proof, the input.json text, a clean scrub; requests of two geometries interleaved, multi-slot
requests with first_slot > 0, a repeat, a fake-source request, a short and a missing-tail file in one call, in modes 2, 0 and 1; batch
seams under 1 MiB of staging; refusals, a missing file, and freeing any subset in any order.  The circuit of tests/test_gpu_scrub_many.py:
64-byte cells, 4 cells per block, 64 or 128 cells per slot."""
import ctypes
import faulthandler
import os
import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CIRCUIT = dict(maxDepth=10, maxLog2NSlots=7, cellSize=64, blockSize=256, nSamples=5)
CS, CPB = 64, 4                        # cell size, cells per network block
CP2_ERR_INVALID, CP2_ERR_IO = -1, -5
ENTROPY = 123457


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


def config(pkg, base=None, n_cells=64, n_slots=8, seed=5, **kw):
    return pkg.make_config(nCells=n_cells, nSlots=n_slots, seed=seed, file=base, **dict(CIRCUIT, **kw))


def write_files(base, n_slots, n_cells, seed=1):
    rng = np.random.default_rng(seed)
    for k in range(n_slots):
        with open("%s%d.dat" % (base, k), "wb") as f:
            f.write(rng.integers(1, 256, n_cells * CS, dtype=np.uint8).tobytes())


def flip(base, slot, offset):
    with open("%s%d.dat" % (base, slot), "r+b") as f:
        f.seek(offset)
        v = f.read(1)
        f.seek(offset)
        f.write(bytes([v[0] ^ 0x5A]))


class Mode:
    """the context's kept mode named for the duration of a block"""

    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        self.ctx.set_keep_trees(self.mode)

    def __exit__(self, *exc):
        self.ctx.set_keep_trees(-1)


def loop(ctx, requests):
    """the yardstick: cp2_dataset_build of each request"""
    return [ctx.dataset(cfg, first_slot=first, n_local=n) for cfg, first, n in requests]


def slot_range(ds):
    first, n = ctypes.c_uint64(), ctypes.c_uint64()
    assert ds.ctx.L.cp2_dataset_range(ds.h, ctypes.byref(first), ctypes.byref(n)) == 0
    return first.value, n.value


def all_blocks(ds):
    nb = int(ds.cfg.n_cells) // CPB
    return [(s, b) for s in range(ds.first_slot, ds.first_slot + ds.n_local) for b in range(nb)]


def same_dataset(got, want, mode, all_roots, what):
    """every observable of `got` (from the one pass) against `want` (from cp2_dataset_build)"""
    assert got.tree_mode == want.tree_mode == mode, what
    assert np.array_equal(got.local_roots(), want.local_roots()), what
    assert slot_range(got) == slot_range(want) == (want.first_slot, want.n_local), what
    got.set_roots(all_roots)
    want.set_roots(all_roots)
    assert np.array_equal(got.root(), want.root()), what
    if mode != 0:
        (r1, p1), (r2, p2) = got.block_proofs(all_blocks(got)), want.block_proofs(all_blocks(want))
        assert np.array_equal(r1, r2) and np.array_equal(p1, p2), what
    for s in range(want.first_slot, want.first_slot + want.n_local):
        assert got.proof_input(s, ENTROPY + s).json() == want.proof_input(s, ENTROPY + s).json(), "%s slot %d" % (what, s)


def free_all(datasets):
    for d in datasets:
        d.free()


def full_roots(ctx, cfg):
    """the roots of every slot of a configuration (a roots-only build of the whole dataset): what cp2_dataset_set_roots is handed"""
    with Mode(ctx, 0):
        d = ctx.dataset(cfg)
    try:
        return d.local_roots().copy()
    finally:
        d.free()


@pytest.mark.parametrize("mode", [2, 0, 1])
def test_mixed_set_equals_the_loop(pkg, sctx, tmp_path, mode):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    write_files(a, 8, 64)
    write_files(b, 7, 128, seed=2)
    with open(a + "6.dat", "r+b") as f:
        f.truncate(37 * CS + 5)                                   # a short file: ends inside a cell, the rest reads as zeros
    with open(a + "7.dat", "r+b") as f:
        f.truncate(13 * CPB * CS)                                 # a missing tail: the last three blocks are not there
    cfg_a, cfg_b, cfg_f = config(pkg, a), config(pkg, b, n_cells=128, n_slots=7), config(pkg, n_slots=6, seed=9)
    requests = [(cfg_a, 0, 1), (cfg_b, 0, 1), (cfg_a, 1, 1), (cfg_b, 1, 1),      # one-slot requests of both sizes, interleaved
                (cfg_a, 2, 3), (cfg_b, 2, 5),                                     # a 3-slot and a 5-slot request, first_slot > 0
                (cfg_a, 1, 1),                                                    # request 2 again: an independent dataset
                (cfg_f, 1, 2),                                                    # fake source
                (cfg_a, 6, 1), (cfg_a, 7, 1)]                                     # the short and the missing-tail file
    roots = {id(c): full_roots(sctx, c) for c in (cfg_a, cfg_b, cfg_f)}
    with Mode(sctx, mode):
        want = loop(sctx, requests)
        got = sctx.build_many(requests)
    assert len(got) == len(requests) and len({d.h.value for d in got}) == len(requests)
    for i, (g, w) in enumerate(zip(got, want)):
        same_dataset(g, w, mode, roots[id(requests[i][0])], "mode %d request %d" % (mode, i))
    gran, bad, counts, n_bad = sctx.scrub_many(got)
    assert n_bad == 0 and not counts.any() and gran.tolist() == [{1: 2, 2: 1, 0: 0}[mode]] * len(requests)
    # a byte flipped in the file only request 0 reads: that request's root changes, no other
    before = [d.local_roots().copy() for d in got]
    flip(a, 0, 29 * CS + 7)
    with Mode(sctx, mode):
        again = sctx.build_many(requests)
    after = [d.local_roots() for d in again]
    assert [i for i in range(len(requests)) if not np.array_equal(before[i], after[i])] == [0]
    free_all(got + want + again)


def traced(capfd, f):
    """f() with CP2_TRACE set: (its result, (requests, fake, classes, items, batches, bytes, mode) of the call's one trace line)"""
    os.environ["CP2_TRACE"] = "1"
    try:
        capfd.readouterr()
        out = f()
    finally:
        del os.environ["CP2_TRACE"]
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "build many:" in ln and "request(s)" in ln]
    assert len(lines) == 1, lines
    m = re.search(r"\[cp2 trace\] build many: (\d+) request\(s\), (\d+) of them fake-source \(built one by one\); (\d+) class\(es\) of slot files, "
                  r"(\d+) item\(s\) in (\d+) batch\(es\), (\d+) bytes read, [0-9.]+ s \([0-9.]+ GB/s\), mode (\d)$", lines[0])
    assert m, lines[0]
    return out, tuple(int(x) for x in m.groups())


def test_batch_seams(pkg, sctx, tmp_path, capfd):
    """Under 1 MiB of staging a batch holds 129 slots of 64 cells.  127 one-slot requests, one 5-slot request (items 127 to 131, across the
    boundary at 129), 150 more one-slot requests, over 70 files listed repeatedly: 282 items in three batches.  Every result must equal
    the one-batch run of the same list on a default context; then the same with ring turns of 10 KiB and O_DIRECT on."""
    n = 70
    base = str(tmp_path / "s")
    write_files(base, n, 64)
    cfg = config(pkg, base, n_slots=n)
    requests = [(cfg, r % n, 1) for r in range(127)] + [(cfg, 10, 5)] + [(cfg, (127 + r) % n, 1) for r in range(150)]
    roots = full_roots(sctx, cfg)
    os.environ["CODEX_P2_STAGE_MB"] = "1"
    try:
        small = pkg.Context(0)
    finally:
        del os.environ["CODEX_P2_STAGE_MB"]
    try:
        for mode in (2, 1):
            with Mode(sctx, mode):
                ref, t = traced(capfd, lambda: sctx.build_many(requests))
            assert t == (len(requests), 0, 1, 282, 1, 282 * 64 * CS, mode)
            for d, (_, first, k) in zip(ref, requests):
                assert np.array_equal(d.local_roots(), roots[first:first + k])          # (and the one-batch run is the loop's: the roots of the files)
            for tuned in (False, True):
                if tuned:
                    small.set_ingest(0, 0, 10 << 10)
                    small.set_ingest_direct(1)
                try:
                    with Mode(small, mode):
                        got, t = traced(capfd, lambda: small.build_many(requests))
                finally:
                    small.set_ingest(0, 0, 0)
                    small.set_ingest_direct(-1)
                assert t[:4] == (len(requests), 0, 1, 282) and t[4] >= 3 and t[6] == mode
                for i, (g, w) in enumerate(zip(got, ref)):
                    assert g.tree_mode == w.tree_mode == mode and slot_range(g) == slot_range(w)
                    assert np.array_equal(g.local_roots(), w.local_roots()), i
                    (r1, p1), (r2, p2) = g.block_proofs(all_blocks(g)), w.block_proofs(all_blocks(w))
                    assert np.array_equal(r1, r2) and np.array_equal(p1, p2), i
                assert small.scrub_many(got)[3] == 0
                # the request across the boundary proves like the loop's dataset
                with Mode(small, mode):
                    one = small.dataset(cfg, first_slot=10, n_local=5)
                same_dataset(got[127], one, mode, roots, "the request across the batch boundary")
                free_all(got + [one])
            free_all(ref)
    finally:
        small.close()


def raw(pkg, L, ctx_h, requests, cfgs_null=False, ranges_null=False, out_null=False, n=None):
    """the C call itself with sentinel outputs: (status, out)"""
    k = len(requests)
    cfgs = (pkg.Config * max(k, 1))()
    ranges = (ctypes.c_uint64 * (2 * max(k, 1)))()
    for i, (cfg, first, n_local) in enumerate(requests):
        cfgs[i] = cfg
        ranges[2 * i], ranges[2 * i + 1] = first, n_local
    out = (ctypes.c_void_p * max(k, 1))(*([0xDEAD] * max(k, 1)))
    st = L.cp2_datasets_build_many(ctx_h, None if cfgs_null else cfgs, None if ranges_null else ranges, k if n is None else n, None if out_null else out)
    return st, [out[i] for i in range(max(k, 1))]


def test_refusals_name_the_request_and_open_no_file(pkg, sctx, tmp_path):
    base = str(tmp_path / "slot")
    write_files(base, 8, 64)
    good = config(pkg, base)
    nowhere = config(pkg, str(tmp_path / "nowhere" / "slot"))           # a later request whose files do not exist: opening one would be CP2_ERR_IO
    L = sctx.L
    err = lambda: L.cp2_last_error(sctx.h).decode()
    bad_requests = [
        ((good, 0, 0), "n_local"),                                                           # n_local == 0
        ((good, 7, 2), "slots 7 + 2"),                                                       # past the dataset's last slot
        ((good, 9, 1), "slots 9 + 1"),
        ((config(pkg, base, maxDepth=-1), 0, 1), "negative"),
        ((config(pkg, base, maxLog2NSlots=-2), 0, 1), "negative"),
        ((config(pkg, base, cellSize=32768, blockSize=65536), 0, 1), "32768"),             # slot.nim:60-61
        ((config(pkg, base, cellSize=0), 0, 1), "must not be 0"),
        ((config(pkg, base, blockSize=200), 0, 1), "no multiple of cell_size"),
        ((config(pkg, base, n_cells=66), 0, 1), "no multiple of the 4 cells"),
    ]
    for q, word in bad_requests:
        one = ctypes.c_void_p()
        assert L.cp2_dataset_build(sctx.h, ctypes.byref(q[0]), q[1], q[2], ctypes.byref(one)) == CP2_ERR_INVALID     # what cp2_dataset_build refuses
        st, out = raw(pkg, L, sctx.h, [(good, 0, 1), q, (nowhere, 0, 1)])
        assert st == CP2_ERR_INVALID and out == [None] * 3, (word, st, out)
        assert err().startswith("request 1: ") and word in err(), (word, err())
    ok = [(good, 0, 1), (good, 1, 1)]
    st, out = raw(pkg, L, None, ok)
    assert st == CP2_ERR_INVALID and out == [None, None]
    st, out = raw(pkg, L, sctx.h, ok + [(nowhere, 0, 1)], out_null=True)
    assert st == CP2_ERR_INVALID and "out" in err()
    st, out = raw(pkg, L, sctx.h, ok + [(nowhere, 0, 1)], cfgs_null=True)
    assert st == CP2_ERR_INVALID and out == [None] * 3 and "cfgs" in err()
    st, out = raw(pkg, L, sctx.h, ok + [(nowhere, 0, 1)], ranges_null=True)
    assert st == CP2_ERR_INVALID and out == [None] * 3 and "ranges" in err()
    st, out = raw(pkg, L, sctx.h, ok, n=0)                                    # no requests: CP2_OK, nothing written
    assert st == 0 and out == [0xDEAD, 0xDEAD]
    assert raw(pkg, L, sctx.h, [], cfgs_null=True, ranges_null=True)[0] == 0
    assert sctx.build_many([]) == []
    st, out = raw(pkg, L, sctx.h, ok)                                         # and two of the requests, valid
    assert st == 0 and all(out)
    for h in out:
        L.cp2_dataset_free(ctypes.c_void_p(h))


def test_missing_file_is_an_io_error_naming_it(pkg, sctx, tmp_path):
    n = 45
    base = str(tmp_path / "slot")
    write_files(base, n, 64)
    cfg = config(pkg, base, n_slots=n)
    requests = [(cfg, k, 1) for k in range(n)]
    roots = full_roots(sctx, cfg)
    os.rename("%s39.dat" % base, "%s39.gone" % base)                     # the 40th file
    L = sctx.L
    with Mode(sctx, 2):
        st, out = raw(pkg, L, sctx.h, requests)
        msg = L.cp2_last_error(sctx.h).decode()
        assert st == CP2_ERR_IO and out == [None] * n and "cannot open" in msg and ("%s39.dat" % base) in msg
        os.rename("%s39.gone" % base, "%s39.dat" % base)
        got = sctx.build_many(requests)                                  # the same call with the file restored
        want = loop(sctx, requests)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.tree_mode == w.tree_mode == 2 and np.array_equal(g.local_roots(), w.local_roots()) and np.array_equal(g.local_roots()[0], roots[k])
        assert all(np.array_equal(x, y) for x, y in zip(g.block_proofs(all_blocks(g)), w.block_proofs(all_blocks(w))))
    free_all(got + want)


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_any_subset_is_freed_in_any_order(pkg, sctx, tmp_path, mode):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    write_files(a, 8, 64)
    write_files(b, 4, 128, seed=3)
    cfg_a, cfg_b = config(pkg, a), config(pkg, b, n_cells=128, n_slots=4)
    requests = [(cfg_a, k, 1) for k in range(8)] + [(cfg_b, 1, 3), (cfg_a, 2, 4), (cfg_b, 0, 1), (cfg_a, 7, 1)]
    with Mode(sctx, mode):
        got = sctx.build_many(requests)
        want = loop(sctx, requests)
    order = list(range(0, len(got), 2))
    random.Random(7).shuffle(order)
    for i in order:
        got[i].free()
    sctx.trim()                                                            # (cached scratch goes: what was freed is really gone)
    rest = [i for i in range(len(got)) if i % 2]
    for i in rest:
        assert np.array_equal(got[i].local_roots(), want[i].local_roots())
        if mode != 0:
            assert all(np.array_equal(x, y) for x, y in zip(got[i].block_proofs(all_blocks(got[i])), want[i].block_proofs(all_blocks(want[i]))))
    assert sctx.scrub_many([got[i] for i in rest])[3] == 0
    for i in reversed(rest):
        got[i].free()
    free_all(want)
