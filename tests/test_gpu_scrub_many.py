"""GPU suite: cp2_datasets_scrub_many -- every local slot of many datasets of one context scrubbed in one pass reports, request by
request, exactly what cp2_dataset_scrub reports for each dataset: the same (slot, index) pairs with the request in front, sorted by
(request, slot, index), capped and counted, the per-request counts complete whatever the cap; datasets of different geometry, source,
residency and local range in one call, one of them twice; tile, batch and table seams; refusals, a missing file, and nothing changed
by the call.  Shapes as tests/test_gpu_scrub.py: 64-byte cells, 4 cells per block, 64 or 128 cells per slot."""
import ctypes
import faulthandler
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CIRCUIT = dict(maxDepth=10, maxLog2NSlots=7, cellSize=64, blockSize=256, nSamples=5)
CS, CPB = 64, 4                        # cell size, cells per network block
N_CELLS, N_SLOTS = 64, 6               # 16 blocks per slot
CP2_ERR_INVALID, CP2_ERR_IO = -1, -5
LEVEL = {1: 2, 2: 1, 0: 0}             # keep-trees mode -> CP2_SCRUB_CELL / _BLOCK / _SLOT


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


def config(pkg, base=None, n_cells=N_CELLS, n_slots=N_SLOTS, seed=5):
    return pkg.make_config(nCells=n_cells, nSlots=n_slots, seed=seed, file=base, **CIRCUIT)


def write_files(base, n_slots=N_SLOTS, n_cells=N_CELLS, seed=1):
    rng = np.random.default_rng(seed)
    data = {}
    for k in range(n_slots):
        b = rng.integers(1, 256, n_cells * CS, dtype=np.uint8).tobytes()   # no zero byte: a truncated tail always differs
        with open("%s%d.dat" % (base, k), "wb") as f:
            f.write(b)
        data[k] = b
    return data


def flip(base, slot, offset):
    with open("%s%d.dat" % (base, slot), "r+b") as f:
        f.seek(offset)
        v = f.read(1)
        f.seek(offset)
        f.write(bytes([v[0] ^ 0x5A]))


def build(ctx, cfg, mode, **kw):
    ctx.set_keep_trees(mode)
    try:
        ds = ctx.dataset(cfg, **kw)
    finally:
        ctx.set_keep_trees(-1)
    assert ds.tree_mode == mode
    return ds


def changed_cells(before, base, n_cells):
    """(slot, cell) of every cell whose bytes on disk differ from what was written: what the builders hash is the file's first
    nCells * cellSize bytes, zeros past its end (slot.nim:61-66)"""
    out = set()
    for s, b in before.items():
        a = np.frombuffer(b[:n_cells * CS], dtype=np.uint8).reshape(n_cells, CS)
        raw = open("%s%d.dat" % (base, s), "rb").read()[:n_cells * CS]
        now = np.frombuffer(raw + bytes(n_cells * CS - len(raw)), dtype=np.uint8).reshape(n_cells, CS)
        out |= {(s, int(c)) for c in np.nonzero((a != now).any(axis=1))[0]}
    return out


def expect(cells, mode, first, n_local):
    """the (slot, index) pairs a dataset in `mode` holding slots first .. first + n_local - 1 reports for these changed cells"""
    mine = {(s, c) for s, c in cells if first <= s < first + n_local}
    if mode == 1:
        return sorted(mine)
    if mode == 2:
        return sorted({(s, c // CPB) for s, c in mine})
    return sorted({(s, 0) for s, _ in mine})


def triples(bad):
    return [tuple(int(x) for x in row) for row in bad]


def loop_report(datasets):
    """what the loop over cp2_dataset_scrub reports: (granularity per request, triples, counts per request)"""
    gran, out, counts = [], [], []
    for i, ds in enumerate(datasets):
        g, bad, n = ds.scrub()
        assert n == bad.shape[0]
        gran.append(g)
        counts.append(n)
        out += [(i, int(s), int(x)) for s, x in bad]
    return gran, out, counts


def raw_many(L, ctx_h, handles, cap, bad_null=False, nbad_null=False, ds_null=False):
    """the C call itself with sentinel outputs: (status, bad, n_bad, counts, granularity)"""
    n = len(handles)
    hs = (ctypes.c_void_p * max(n, 1))(*handles)
    bad = np.full((max(cap, 1), 3), 7, dtype=np.uint64)
    counts = np.full(max(n, 1), 8, dtype=np.uint64)
    gran = np.full(max(n, 1), 42, dtype=np.int32)
    nb = ctypes.c_size_t(99)
    st = L.cp2_datasets_scrub_many(ctx_h, None if ds_null else hs, n, None if bad_null else bad.ctypes.data, cap,
                                   None if nbad_null else ctypes.byref(nb), counts.ctypes.data, gran.ctypes.data)
    return st, bad, nb.value, counts, gran


def untouched(out):
    st, bad, nb, counts, gran = out
    return nb == 99 and (bad == 7).all() and (counts == 8).all() and (gran == 42).all()


def test_mixed_set_equals_the_loop_and_the_changed_bytes(pkg, sctx, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    data_a, data_b = write_files(a), write_files(b, n_slots=3, n_cells=128, seed=2)
    cfg_a, cfg_b = config(pkg, a), config(pkg, b, n_cells=128, n_slots=3)
    # (dataset, base data, base, n_cells, mode, first, n_local); the one-slot mode-1 dataset of slot 1 is listed twice
    one1 = build(sctx, cfg_a, 1, first_slot=1, n_local=1)
    spec = [(one1, data_a, a, 64, 1, 1, 1),
            (build(sctx, cfg_a, 2, first_slot=3, n_local=1), data_a, a, 64, 2, 3, 1),
            (build(sctx, cfg_b, 1), data_b, b, 128, 1, 0, 3),                           # 128 cells: a class of its own
            (build(sctx, cfg_a, 0, first_slot=5, n_local=1), data_a, a, 64, 0, 5, 1),
            (build(sctx, config(pkg, seed=9), 2), None, None, 64, 2, 0, N_SLOTS),       # fake source: regenerated, always clean
            (build(sctx, cfg_a, 2), data_a, a, 64, 2, 0, N_SLOTS),                      # six slots, compact: the class of request 1
            (one1, data_a, a, 64, 1, 1, 1)]
    datasets = [s[0] for s in spec]
    gran, bad, counts, n = sctx.scrub_many(datasets)
    assert gran.tolist() == [LEVEL[s[4]] for s in spec] and (n, bad.shape, counts.tolist()) == (0, (0, 3), [0] * len(spec))
    # slot 1 is shared by requests 0, 5 and 6; slot 3 by 1 and 5; slot 5 by 3 and 5; slot 4 only request 5 holds
    for s, c, byte in ((1, 0, 0), (1, 63, 63), (1, 20, 5), (1, 21, 6), (3, 41, 9), (4, 7, 31), (5, 62, 1), (5, 2, 2)):
        flip(a, s, c * CS + byte)
    for s, c, byte in ((0, 127, 63), (2, 0, 0), (2, 64, 7)):
        flip(b, s, c * CS + byte)
    want = []
    for i, (_, before, base, n_cells, mode, first, n_local) in enumerate(spec):
        if base is not None:
            want += [(i, s, x) for s, x in expect(changed_cells(before, base, n_cells), mode, first, n_local)]
    assert want == sorted(want) and {t[0] for t in want} == {0, 1, 2, 3, 5, 6}
    loop_gran, loop_triples, loop_counts = loop_report(datasets)
    assert loop_triples == want                                                        # (the yardstick agrees with the files)
    gran, bad, counts, n = sctx.scrub_many(datasets)
    assert triples(bad) == loop_triples == want
    assert gran.tolist() == loop_gran and counts.tolist() == loop_counts and n == len(want) == sum(loop_counts)
    assert counts[4] == 0 and counts[0] == counts[6] == 4
    for d in {id(s[0]): s[0] for s in spec}.values():
        d.free()


def seam_datasets(pkg, ctx, base, n):
    cfg = config(pkg, base, n_slots=n)
    return [build(ctx, cfg, 1, first_slot=k, n_local=1) for k in range(n)]


def traced(capfd, f):
    """f() with CP2_TRACE set: (its result, batches the call's trace line reports)"""
    os.environ["CP2_TRACE"] = "1"
    try:
        capfd.readouterr()
        out = f()
    finally:
        del os.environ["CP2_TRACE"]
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "scrub many:" in ln]
    assert len(lines) == 1, lines
    m = re.search(r"(\d+) request\(s\), (\d+) of them fake-source .*; (\d+) class\(es\) of slot files, (\d+) item\(s\) in (\d+) batch\(es\), (\d+) bytes read", lines[0])
    assert m and "GB/s" in lines[0] and "mismatch(es)" in lines[0], lines[0]
    requests, fake, classes, items, batches, nbytes = (int(x) for x in m.groups())
    assert fake == 0 and nbytes == items * N_CELLS * CS
    return out, (requests, classes, items, batches)


def test_tile_batch_and_table_seams(pkg, sctx, tmp_path, capfd):
    """70 one-slot datasets of 64 cells are 4480 rows: the tile boundary at row 4096 falls between requests 63 and 64.  Then the same
    with 1 MiB of staging, ring turns of two files and O_DIRECT on.  CODEX_P2_STAGE_MB's minimum of 1 MiB holds 129 such slots in a
    batch, so 70 requests cannot make three batches: that run lists the 70 datasets four times over (a dataset may appear more than
    once) -- 280 requests, batches of 129, 129 and 22 -- and must equal the one-batch run of the same list."""
    n = 70
    base = str(tmp_path / "s")
    write_files(base, n_slots=n)
    os.environ["CODEX_P2_STAGE_MB"] = "1"
    try:
        small = pkg.Context(0)
    finally:
        del os.environ["CODEX_P2_STAGE_MB"]
    try:
        ref_ds, small_ds = seam_datasets(pkg, sctx, base, n), seam_datasets(pkg, small, base, n)
        damage = ((0, 0), (63, 63), (64, 0), (69, 63))
        for s, c in damage:
            flip(base, s, c * CS + 3)
        (gran, bad, counts, nb), (_, _, items, batches) = traced(capfd, lambda: sctx.scrub_many(ref_ds))
        assert (items, batches) == (n, 1)
        assert triples(bad) == [(s, s, c) for s, c in damage] and nb == 4 and gran.tolist() == [2] * n
        assert counts.tolist() == [1 if k in (0, 63, 64, 69) else 0 for k in range(n)]
        # four times over: requests 0..279, request r scrubs slot r % 70; damage in the first (0, 63, 64, 69), the middle (140, 203,
        # 204, 209 and the others of batch 1) and the last batch (258 .. 279 holds 273 = 3 * 70 + 63 and 274)
        want = [(r, r % n, c) for r in range(4 * n) for s, c in damage if r % n == s]
        (gran1, bad1, counts1, nb1), (_, _, items1, batches1) = traced(capfd, lambda: sctx.scrub_many(ref_ds * 4))
        assert (items1, batches1) == (4 * n, 1) and triples(bad1) == want and nb1 == 16
        small.set_ingest(0, 0, 10 << 10)
        small.set_ingest_direct(1)
        try:
            (gran2, bad2, counts2, nb2), (_, classes2, items2, batches2) = traced(capfd, lambda: small.scrub_many(small_ds * 4))
        finally:
            small.set_ingest(0, 0, 0)
            small.set_ingest_direct(-1)
        assert (classes2, items2) == (1, 4 * n) and batches2 >= 3
        assert {r for r, _, _ in want if r < 129} and {r for r, _, _ in want if 129 <= r < 258} and {r for r, _, _ in want if r >= 258}
        assert np.array_equal(bad2, bad1) and nb2 == nb1 and np.array_equal(counts2, counts1) and np.array_equal(gran2, gran1)
        got70 = small.scrub_many(small_ds)
        assert np.array_equal(got70[1], bad) and got70[3] == nb and np.array_equal(got70[2], counts)
        for s, c in damage:
            flip(base, s, c * CS + 3)                              # (flipping again restores the byte)
        assert small.scrub_many(small_ds * 4)[3] == 0 and sctx.scrub_many(ref_ds)[3] == 0
        for d in ref_ds + small_ds:
            d.free()
    finally:
        small.close()


def test_cap_count_and_sentinels(pkg, sctx, tmp_path):
    base = str(tmp_path / "slot")
    write_files(base)
    cfg = config(pkg, base)
    datasets = [build(sctx, cfg, 1, first_slot=k, n_local=1) for k in (4, 0, 2)] + [build(sctx, cfg, 2)]
    for s in range(N_SLOTS):
        for c in (s, 10 + 3 * s, N_CELLS - 1 - s):
            flip(base, s, c * CS)
    _, want, want_counts = loop_report(datasets)
    assert len(want) == 9 + 18 and want_counts == [3, 3, 3, 18]
    L, handles = sctx.L, [d.h for d in datasets]
    st, bad, nb, counts, gran = raw_many(L, sctx.h, handles, 64)
    assert st == 0 and nb == len(want) and triples(bad[:nb]) == want and (bad[nb:] == 7).all()
    assert counts.tolist() == want_counts and gran.tolist() == [2, 2, 2, 1]
    for cap in (1, 4, 10, len(want) - 1):                          # the lowest `cap` in order; the count and the counts complete
        st, bad, nb, counts, gran = raw_many(L, sctx.h, handles, cap)
        assert st == 0 and nb == len(want) and triples(bad) == want[:cap] and counts.tolist() == want_counts
    st, bad, nb, counts, gran = raw_many(L, sctx.h, handles, 0, bad_null=True)   # counting only
    assert st == 0 and nb == len(want) and counts.tolist() == want_counts and gran.tolist() == [2, 2, 2, 1]
    g, b, c, n = sctx.scrub_many(datasets, cap=0)
    assert b.shape == (0, 3) and n == len(want) and c.tolist() == want_counts
    st, bad, nb, counts, gran = raw_many(L, sctx.h, [], 4)          # no requests: CP2_OK, *n_bad = 0, nothing else written
    assert st == 0 and nb == 0 and (bad == 7).all() and (counts == 8).all() and (gran == 42).all()
    st, bad, nb, counts, gran = raw_many(L, sctx.h, [], 0, bad_null=True, ds_null=True)
    assert st == 0 and nb == 0
    hs = (ctypes.c_void_p * len(handles))(*handles)                 # counts and granularity may be NULL
    n_bad = ctypes.c_size_t(99)
    assert L.cp2_datasets_scrub_many(sctx.h, hs, len(handles), None, 0, ctypes.byref(n_bad), None, None) == 0 and n_bad.value == len(want)
    for d in datasets:
        d.free()


def test_refusals_leave_the_outputs_and_name_the_request(pkg, sctx, tmp_path):
    base = str(tmp_path / "slot")
    write_files(base)
    cfg = config(pkg, base)
    other = pkg.Context(0)
    try:
        mine = [build(sctx, cfg, 2, first_slot=k, n_local=1) for k in range(3)]
        theirs = build(other, cfg, 2, first_slot=1, n_local=1)
        flip(base, 1, 5)                                            # (there is something to report, were the call to run)
        L = sctx.L
        err = lambda: L.cp2_last_error(sctx.h).decode()
        out = raw_many(L, sctx.h, [mine[0].h, None, mine[2].h], 4)
        assert out[0] == CP2_ERR_INVALID and untouched(out) and "request 1" in err() and "NULL" in err()
        out = raw_many(L, sctx.h, [mine[0].h, mine[1].h, theirs.h], 4)
        assert out[0] == CP2_ERR_INVALID and untouched(out) and "request 2" in err() and "another context" in err()
        out = raw_many(L, sctx.h, [m.h for m in mine], 4, bad_null=True)     # cap > 0 with bad NULL
        assert out[0] == CP2_ERR_INVALID and untouched(out)
        out = raw_many(L, sctx.h, [m.h for m in mine], 4, nbad_null=True)
        assert out[0] == CP2_ERR_INVALID and untouched(out)
        out = raw_many(L, sctx.h, [m.h for m in mine], 4, ds_null=True)
        assert out[0] == CP2_ERR_INVALID and untouched(out)
        out = raw_many(L, None, [m.h for m in mine], 4)
        assert out[0] == CP2_ERR_INVALID and untouched(out)
        out = raw_many(L, sctx.h, [m.h for m in mine], 4)                     # and the same requests, valid
        assert out[0] == 0 and out[2] == 1 and triples(out[1][:1]) == [(1, 1, 0)]
        theirs.free()
        for m in mine:
            m.free()
    finally:
        other.close()


def test_missing_file_is_an_io_error_naming_it(pkg, sctx, tmp_path):
    base = str(tmp_path / "slot")
    write_files(base)
    cfg = config(pkg, base)
    datasets = [build(sctx, cfg, 2, first_slot=k, n_local=1) for k in (0, 2, 3, 5)]
    flip(base, 5, 9)
    os.rename("%s3.dat" % base, "%s3.gone" % base)
    L = sctx.L
    out = raw_many(L, sctx.h, [d.h for d in datasets], 4)
    msg = L.cp2_last_error(sctx.h).decode()
    assert out[0] == CP2_ERR_IO and untouched(out) and "cannot open" in msg and ("%s3.dat" % base) in msg
    os.rename("%s3.gone" % base, "%s3.dat" % base)
    gran, bad, counts, n = sctx.scrub_many(datasets)                # a later call on the same context works
    assert triples(bad) == [(3, 5, 0)] and n == 1 and counts.tolist() == [0, 0, 0, 1]
    for d in datasets:
        d.free()


def test_read_only(pkg, sctx, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    write_files(a)
    write_files(b, n_slots=3, n_cells=128, seed=2)
    full = build(sctx, config(pkg, a), 2)
    wide = build(sctx, config(pkg, b, n_cells=128, n_slots=3), 1)
    one = build(sctx, config(pkg, a), 0, first_slot=2, n_local=1)
    entropy = 123457
    before = (full.proof_input(3, entropy).json(), wide.proof_input(1, entropy).json(), full.local_roots().tobytes(), one.local_roots().tobytes())
    assert sctx.scrub_many([full, wide, one, full])[3] == 0
    flip(a, 2, 100)
    flip(b, 1, 7)
    assert sctx.scrub_many([full, wide, one, full])[2].tolist() == [1, 1, 1, 1]
    flip(a, 2, 100)
    flip(b, 1, 7)
    after = (full.proof_input(3, entropy).json(), wide.proof_input(1, entropy).json(), full.local_roots().tobytes(), one.local_roots().tobytes())
    assert after == before and (full.tree_mode, wide.tree_mode, one.tree_mode) == (2, 1, 0)
    for d in (full, wide, one):
        d.free()
