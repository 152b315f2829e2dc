"""GPU suite: cp2_datasets_set_roots_many -- the dataset trees of n datasets of one context set in one pass leave every dataset, in every
observable, as cp2_dataset_set_roots leaves its twin: the dataset root, slotProof, the input.json text, the export of a streamed build.
Datasets from cp2_datasets_build_many and from cp2_dataset_build in modes 2, 0 and 1 with n_slots in {1, 2, 3, 5, 8, 13, 64, 100, 128}:
one-slot requests at first_slot > 0, multi-slot requests, all-local datasets with NULL roots mixed in, a streamed build; `own`; a second
call that replaces the trees; chunk seams under 1 MiB of staging with a request larger than a chunk; every refusal, after which nothing
has changed.  The circuit of tests/test_gpu_build_many.py: 64-byte cells, 4 cells per block, maxLog2NSlots 7.

cp2_dataset_set_roots accepts any roots, so the roots handed in are random field elements with the dataset's own built roots in its own
rows: what a manifest holds as far as these calls can tell."""
import ctypes
import faulthandler
import os
import re

import numpy as np
import pytest

import set_roots_many_models as M

pytestmark = pytest.mark.gpu

CIRCUIT = dict(maxDepth=10, maxLog2NSlots=7, cellSize=64, blockSize=256, nSamples=5)
CP2_OK, CP2_ERR_INVALID = 0, -1
ENTROPY = 424247
# (n_slots, first_slot, n_local, built by build_many?, roots given?)
SPECS = [(1, 0, 1, True, False), (2, 1, 1, True, True), (3, 0, 3, False, False), (3, 2, 1, True, True), (5, 1, 3, False, True),
         (8, 0, 8, True, True), (13, 12, 1, True, True), (64, 63, 1, False, True), (100, 37, 2, True, True), (128, 127, 1, True, True),
         (128, 0, 128, False, False), (13, 0, 13, True, False)]
STREAMED = (5, 1, 2)                   # n_slots, first_slot, n_local of the streamed build (roots given)


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


def config(pkg, n_slots, seed, **kw):
    return pkg.make_config(nCells=64, nSlots=n_slots, seed=seed, **dict(CIRCUIT, **kw))


class Mode:
    """the context's kept mode named for the duration of a block"""

    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        self.ctx.set_keep_trees(self.mode)

    def __exit__(self, *exc):
        self.ctx.set_keep_trees(-1)


def manifest(ds, seed):
    """n_slots x 32 bytes: random field elements, the dataset's own built roots in its own rows"""
    rng = np.random.default_rng([0x5E71, seed])
    n = int(ds.cfg.n_slots)
    r = np.zeros((n, 32), dtype=np.uint8)
    r[:, :31] = rng.integers(0, 256, size=(n, 31), dtype=np.uint8)
    r[ds.first_slot:ds.first_slot + ds.n_local] = ds.local_roots()
    return r


def build_set(pkg, ctx, mode, specs=SPECS, seed0=100):
    """one dataset per spec (by cp2_datasets_build_many or cp2_dataset_build, as the spec says) and the roots each is given (or None)"""
    cfgs = [config(pkg, n, seed0 + i) for i, (n, _, _, _, _) in enumerate(specs)]
    with Mode(ctx, mode):
        many = ctx.build_many([(cfgs[i], f, k) for i, (_, f, k, bm, _) in enumerate(specs) if bm])
        out = []
        for i, (_, f, k, bm, _) in enumerate(specs):
            out.append(many.pop(0) if bm else ctx.dataset(cfgs[i], first_slot=f, n_local=k))
    roots = [manifest(d, seed0 + i) if specs[i][4] else None for i, d in enumerate(out)]
    return out, roots


def observables(ds):
    """(dataset root, per local slot (slotProof, input.json text))"""
    per_slot = []
    for s in range(ds.first_slot, ds.first_slot + ds.n_local):
        pi = ds.proof_input(s, ENTROPY + s)
        per_slot.append((pi.slot_proof().tobytes(), pi.json()))
    return ds.root().tobytes(), per_slot


def free_all(datasets):
    for d in datasets:
        d.free()


def traced(capfd, f):
    """f() with CP2_TRACE set: (its result, (requests, chunks, rows, levels) of the call's one trace line)"""
    os.environ["CP2_TRACE"] = "1"
    try:
        capfd.readouterr()
        out = f()
    finally:
        del os.environ["CP2_TRACE"]
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "set roots many:" in ln]
    assert len(lines) == 1, lines
    m = re.search(r"\[cp2 trace\] set roots many: (\d+) request\(s\) in (\d+) chunk\(s\), (\d+) tree rows, (\d+) level\(s\); upload [0-9.]+ s, "
                  r"levels [0-9.]+ s, download [0-9.]+ s, commit [0-9.]+ s$", lines[0])
    assert m, lines[0]
    return out, tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("mode", [2, 0, 1])
def test_the_one_pass_equals_the_loop(pkg, sctx, tmp_path, capfd, mode):
    got, roots = build_set(pkg, sctx, mode)
    want, roots_w = build_set(pkg, sctx, mode)
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(roots, roots_w))
    n, f, k = STREAMED
    scfg = config(pkg, n, 77)
    s_got, s_want = (sctx.dataset_streamed(scfg, ENTROPY, first_slot=f, n_local=k, threads=2) for _ in range(2))
    s_roots = manifest(s_got, 77)
    at = 4                                                                     # the streamed build in the middle of the requests
    own, t = traced(capfd, lambda: sctx.set_roots_many(got[:at] + [s_got] + got[at:], roots[:at] + [s_roots] + roots[at:]))
    assert own.tolist() == [1] * (len(got) + 1)
    rows = sum(int(pkg.load_library().cp2_merkle_total(int(d.cfg.n_slots))) for d in got + [s_got])
    assert t == (len(got) + 1, 1, rows, 7)
    for d, r in zip(want, roots):
        d.set_roots(r)
    s_want.set_roots(s_roots)
    for i, (g, w) in enumerate(zip(got, want)):
        assert observables(g) == observables(w), "mode %d request %d" % (mode, i)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    assert s_got.export_streamed(str(a), threads=2) == s_want.export_streamed(str(b), threads=2)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["input_%d.json" % s for s in range(f, f + k)]
    for name in os.listdir(a):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    assert [s_got.streamed_json(s) for s in range(f, f + k)] == [s_want.streamed_json(s) for s in range(f, f + k)]
    # cp2_proof_inputs_generate_many takes them as it takes the loop's
    reqs = lambda dss: [(d, d.first_slot + d.n_local - 1, ENTROPY + i) for i, d in enumerate(dss)]
    assert [p.json() for p in sctx.proof_inputs_many(reqs(got))] == [p.json() for p in sctx.proof_inputs_many(reqs(want))]
    free_all(got + want + [s_got, s_want])


def test_own_names_the_request_whose_row_differs_and_a_second_call_replaces_the_trees(pkg, sctx):
    got, roots = build_set(pkg, sctx, 2, seed0=300)
    want, _ = build_set(pkg, sctx, 2, seed0=300)
    k = 8                                                                      # (100 slots, slots 37 and 38 local)
    assert SPECS[k][:3] == (100, 37, 2)
    wrong = [None if r is None else r.copy() for r in roots]
    wrong[k][38, 3] ^= 0x40                                                    # the second of its own rows
    own = sctx.set_roots_many(got, wrong)
    assert own.tolist() == [int(i != k) for i in range(len(got))]
    want[k].set_roots(wrong[k])
    assert got[k].root().tobytes() == want[k].root().tobytes()                 # accepted as it is, like cp2_dataset_set_roots
    with pytest.raises(pkg.CodexP2Error) as e:
        sctx.proof_inputs_many([(got[0], 0, 1), (got[k], 38, 2)])
    assert "request 1: the root its dataset tree holds for slot 38 (cp2_dataset_set_roots) differs from the slot's built root" in str(e.value)
    before = [d.root().tobytes() for d in got]
    # other roots for everything that was given roots: rows that are not the dataset's own changed, and the roots dropped for request 5 (all local)
    other = [None if r is None else r.copy() for r in roots]
    for i, r in enumerate(other):
        if r is not None and r.shape[0] > got[i].n_local:
            row = (got[i].first_slot + got[i].n_local) % r.shape[0]
            r[row, 0] ^= 1
    assert SPECS[5][:3] == (8, 0, 8)
    other[5] = None
    own = sctx.set_roots_many(got, other)
    assert own.tolist() == [1] * len(got)
    for d, r in zip(want, other):
        d.set_roots(r)
    for i, (g, w) in enumerate(zip(got, want)):
        assert observables(g) == observables(w), i
    changed = [i for i, d in enumerate(got) if d.root().tobytes() != before[i]]
    assert changed == [i for i, r in enumerate(other) if r is not None and r.shape[0] > got[i].n_local]
    free_all(got + want)


def test_chunk_seams_and_a_request_larger_than_a_chunk(pkg, sctx, capfd):
    """Under 1 MiB of staging a chunk holds 16384 tree rows.  240 one-slot datasets of 128, 100 and 13 slots in turn (255, 202 and 27 rows:
    a seam after the first hundred of every 120) and in their middle one of 9000 slots, whose 18006 rows exceed a chunk: it runs alone,
    which makes five chunks."""
    os.environ["CODEX_P2_STAGE_MB"] = "1"
    try:
        small = pkg.Context(0)
    finally:
        del os.environ["CODEX_P2_STAGE_MB"]
    try:
        sizes = (128, 100, 13)
        cfgs = {n: config(pkg, n, 500 + n) for n in sizes}
        big = config(pkg, 9000, 9, maxLog2NSlots=14)
        requests = [(cfgs[sizes[r % 3]], (5 * r) % sizes[r % 3], 1) for r in range(240)]
        requests.insert(120, (big, 8999, 1))
        chunks = M.chunks([int(q[0].n_slots) for q in requests], 1 << 19)
        assert [(c.first, c.count) for c in chunks] == [(0, 100), (100, 20), (120, 1), (121, 100), (221, 20)] and chunks[2].rows == 18006
        with Mode(small, 2):
            got, want = small.build_many(requests), small.build_many(requests)
        roots = [manifest(d, 500 + i) for i, d in enumerate(got)]
        own, t = traced(capfd, lambda: small.set_roots_many(got, roots))
        assert own.tolist() == [1] * len(got)
        assert t == (len(got), 5, sum(c.rows for c in chunks), 14)
        for i, (g, w, r) in enumerate(zip(got, want, roots)):
            w.set_roots(r)
            assert g.root().tobytes() == w.root().tobytes(), i
        for i in sorted({j for c in chunks for j in (c.first, c.first + c.count - 1)}):     # either side of every seam, and the lone request
            assert observables(got[i]) == observables(want[i]), i
        free_all(got + want)
    finally:
        small.close()


def test_generate_many_sets_the_trees_of_all_local_datasets_in_one_pass(pkg, sctx, capfd):
    """all-local datasets without a tree, one of them in two requests: the texts of the per-dataset route, one pass (section 4)"""
    specs = [(n, 0, n, i % 2 == 0, False) for i, n in enumerate((1, 2, 3, 5, 8, 13, 64, 100, 128))]
    got, _ = build_set(pkg, sctx, 2, specs, seed0=700)
    want, _ = build_set(pkg, sctx, 2, specs, seed0=700)
    reqs = lambda dss: [(d, d.n_local - 1, ENTROPY + i) for i, d in enumerate(dss)] + [(dss[4], 0, 5)]
    pis, t = traced(capfd, lambda: sctx.proof_inputs_many(reqs(got)))
    assert t[:2] == (len(got), 1)
    assert [p.json() for p in pis] == [d.proof_input(s, e).json() for d, s, e in reqs(want)]
    free_all(got + want)


def raw(ctx, handles, ptrs, n=None, ctx_null=False, ds_null=False):
    """the C call itself: (status, own with a sentinel in every entry, the context's message)"""
    k = len(handles)
    hs = (ctypes.c_void_p * max(k, 1))(*handles)
    rp = None
    if ptrs is not None:
        rp = (ctypes.c_void_p * max(k, 1))(*[None if a is None else a.ctypes.data for a in ptrs])
    own = (ctypes.c_uint8 * max(k, 1))(*([7] * max(k, 1)))
    st = ctx.L.cp2_datasets_set_roots_many(None if ctx_null else ctx.h, None if ds_null else hs, rp, k if n is None else n, own)
    return st, list(own), ctx.L.cp2_last_error(ctx.h).decode()


def test_refusals_change_nothing(pkg, sctx):
    got, roots = build_set(pkg, sctx, 2, seed0=900)
    with_tree, bare = got[:6], got[6:]                                         # the first six get a tree now; the rest are all partial but the last two
    sctx.set_roots_many(with_tree, roots[:6])
    old = [d.root().tobytes() for d in with_tree]
    partial = [d for d in bare if d.n_local < d.cfg.n_slots]
    assert len(partial) >= 4
    other = pkg.Context(0)
    try:
        with Mode(other, 2):
            foreign = other.dataset(config(pkg, 3, 1), first_slot=1, n_local=1)
        f_roots = manifest(foreign, 1)
        hs = [d.h.value for d in got]

        def unchanged(what):
            assert [d.root().tobytes() for d in with_tree] == old, what
            for d in partial:                                                  # still no tree: nothing to prove from, no root to give
                with pytest.raises(pkg.CodexP2Error):
                    d.root()
            with pytest.raises(pkg.CodexP2Error) as e:
                sctx.proof_inputs_many([(partial[0], partial[0].first_slot, 1)])
            assert "no dataset tree" in str(e.value), what

        cases = [
            ("NULL dataset", hs[:7] + [None] + hs[7:], roots[:7] + [None] + roots[7:], 7),
            ("another context", hs[:9] + [foreign.h.value] + hs[9:], roots[:9] + [f_roots] + roots[9:], 9),
            ("the same dataset as request 2", hs + [hs[2]], roots + [roots[2]], len(hs)),
            ("NULL roots for a dataset whose slots are not all local", hs, roots[:8] + [None] + roots[9:], 8),
        ]
        for word, handles, ptrs, at in cases:
            st, own, msg = raw(sctx, handles, ptrs)
            assert st == CP2_ERR_INVALID and own == [7] * len(handles), (word, st, own)
            assert msg.startswith("request %d: " % at) and word in msg, (word, msg)
            unchanged(word)
        st, own, msg = raw(sctx, hs, None)                                     # no roots at all, with partial datasets among them
        assert st == CP2_ERR_INVALID and own == [7] * len(hs) and msg.startswith("request 1: ") and "not all local" in msg, msg
        unchanged("all_roots NULL")
        st, own, msg = raw(sctx, hs, roots, ds_null=True)
        assert st == CP2_ERR_INVALID and own == [7] * len(hs) and "ds is NULL" in msg
        st, own, _ = raw(sctx, hs, roots, ctx_null=True)
        assert st == CP2_ERR_INVALID and own == [7] * len(hs)
        unchanged("ds NULL, ctx NULL")
        st, own, _ = raw(sctx, hs, roots, n=0)                                 # no requests: CP2_OK, nothing written, nothing changed
        assert st == CP2_OK and own == [7] * len(hs)
        assert raw(sctx, [], None, ds_null=True)[0] == CP2_OK and sctx.set_roots_many([]).tolist() == []
        unchanged("n == 0")
        st, own, _ = raw(sctx, hs, roots)                                      # and the same requests, valid
        assert st == CP2_OK and own == [1] * len(hs)
        assert all(len(d.root().tobytes()) == 32 for d in partial)
        foreign.free()
    finally:
        other.close()
    free_all(got)
