"""GPU suite: cp2_proof_inputs_generate_many / _export_many -- proof inputs for (dataset, slot, entropy) requests across datasets of
one circuit are byte for byte what cp2_proof_input_generate makes for each triple, whatever each dataset keeps of its trees and
wherever its cells come from; every refusal of the contract; changed slot data; the pipelined export; chunked compact work."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
CIRCUIT = dict(maxDepth=10, maxLog2NSlots=4, cellSize=64, blockSize=256, nSamples=5)
CP2_ERR_INVALID, CP2_ERR_IO = -1, -5

# (name, nCells, nSlots, seed, keep-trees mode, slot files?)
DATASETS = [
    ("a", 4, 1, 11, 1, False),
    ("b", 32, 3, 12, 2, False),
    ("c", 256, 11, 13, 0, False),
    ("d", 1024, 16, 14, 1, True),
    ("e", 32, 11, 15, 2, True),
    ("f", 256, 3, 16, 1, False),
    ("g", 4, 16, 17, 0, True),
    ("h", 1024, 3, 18, 2, False),
]


def _config(pkg, n_cells, n_slots, seed, base=None, **circuit):
    c = dict(CIRCUIT, **circuit)
    return pkg.make_config(nCells=n_cells, nSlots=n_slots, seed=seed, file=base, **c)


def write_slot_files(base, n_slots, n_cells, cell_size, seed):
    rng = np.random.default_rng(seed)
    for k in range(n_slots):
        n = n_cells * cell_size - (cell_size // 2 if k == 1 else 0)   # slot 1 ends early: the tail reads as zeros (slot.nim:61-66)
        with open("%s%d.dat" % (base, k), "wb") as f:
            f.write(rng.integers(0, 256, n, dtype=np.uint8).tobytes())


def build(pkg, ctx, cfg, mode, first_slot=0, n_local=None):
    ctx.set_keep_trees(mode)
    try:
        ds = ctx.dataset(cfg, first_slot, n_local)
    finally:
        ctx.set_keep_trees(-1)
    assert ds.tree_mode == mode
    return ds


@pytest.fixture(scope="module")
def mctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def datasets(pkg, mctx, tmp_path_factory):
    out = {}
    d = tmp_path_factory.mktemp("many_slots")
    for name, nc, ns, seed, mode, files in DATASETS:
        base = None
        if files:
            base = str(d / ("%s_slot" % name))
            write_slot_files(base, ns, nc, CIRCUIT["cellSize"], seed)
        out[name] = build(pkg, mctx, _config(pkg, nc, ns, seed, base), mode)
    return out


def per_call(ds, slot, entropy):
    return ds.proof_input(slot, entropy).json()


def raw_many(pkg, ctx, handles, slots, entropies, n=None):
    """the C call itself: (status, out handles, cp2_last_error); out[] starts non-NULL so that a refusal has to clear it"""
    L = ctx.L
    n = len(handles) if n is None else n
    hs = (ctypes.c_void_p * max(n, 1))(*handles)
    sl = np.ascontiguousarray(np.asarray(slots, dtype=np.uint64).reshape(-1))
    en = np.zeros((max(n, 1), 32), dtype=np.uint8)
    for i, e in enumerate(entropies):
        en[i] = pkg.felt_bytes(e)
    out = (ctypes.c_void_p * max(n, 1))(*([1] * max(n, 1)))
    st = L.cp2_proof_inputs_generate_many(ctx.h, hs, sl.ctypes.data, en.ctypes.data, n, out)
    return st, [out[i] for i in range(n)], L.cp2_last_error(ctx.h).decode()


def mixed_requests(datasets):
    ents = [0, R_MOD - 1, R_MOD, 2**256 - 1, 12345, 2**200 + 7]
    reqs = []
    k = 0
    for name, nc, ns, seed, mode, files in DATASETS:
        ds = datasets[name]
        for slot in sorted({0, ns // 2, ns - 1}):
            reqs.append((ds, slot, ents[k % len(ents)]))
            k += 1
    reqs += [(datasets["b"], 1, e) for e in (5, R_MOD + 5, 99)]   # one (dataset, slot) under three entropies (two of them equal as field elements)
    reqs += [(datasets["e"], 2, 77), (datasets["e"], 2, 78)]
    return reqs


def test_parity_with_per_call_verify_and_oracle(pkg, mctx, datasets, entry):
    reqs = mixed_requests(datasets)
    pis = mctx.proof_inputs_many(reqs)
    assert len(pis) == len(reqs)
    for (ds, slot, e), pi in zip(reqs, pis):
        assert pi.json() == per_call(ds, slot, e), (ds.cfg.n_cells, slot, e)
        assert pi.roots()[2].tobytes() == (e % R_MOD).to_bytes(32, "little")
    status, ok = mctx.verify_proof_inputs(pis)
    assert status.tolist() == [0] * len(pis) and ok.all()
    # two of them against the oracle's input.json (fake source: the Python restatement of the reference)
    _, ref = entry.load_oracle()
    for name, slot, e in (("b", 2, 2**256 - 1), ("a", 0, 0)):
        _, nc, ns, seed, _, _ = next(d for d in DATASETS if d[0] == name)
        c = dict(CIRCUIT, nCells=nc, nSlots=ns, seed=seed)
        want = ref.export_json(ref.generate_proof_input(c, slot, e % R_MOD))
        got = [pi for (ds, s, ee), pi in zip(reqs, pis) if ds is datasets[name] and s == slot and ee == e]
        assert got and got[0].json() == want


@pytest.mark.parametrize("mode", [1, 2, 0])
def test_node_model_one_slot_datasets_with_manifest_roots(pkg, mctx, mode):
    cfg = _config(pkg, 256, 11, 321)
    full = build(pkg, mctx, cfg, 1)
    roots = full.local_roots()
    reqs, want = [], []
    for k in (0, 5, 10):
        one = build(pkg, mctx, cfg, mode, first_slot=k, n_local=1)
        one.set_roots(roots)
        for e in (3, 2**255 + k):
            reqs.append((one, k, e))
            want.append(per_call(full, k, e))
    got = [pi.json() for pi in mctx.proof_inputs_many(reqs)]
    assert got == want


def test_refusals_name_the_request_and_clear_every_output(pkg, mctx, datasets):
    good = datasets["b"]
    L = mctx.L
    # n == 0 is fine; NULL arrays with n > 0 are not
    st, _, _ = raw_many(pkg, mctx, [], [], [], n=0)
    assert st == 0
    assert L.cp2_proof_inputs_generate_many(mctx.h, None, None, None, 1, None) == CP2_ERR_INVALID
    total = ctypes.c_uint64(7)
    assert L.cp2_proof_inputs_export_many(mctx.h, None, None, None, 0, None, 1, 0, ctypes.byref(total)) == 0 and total.value == 0

    other = pkg.Context(0)                                               # a second context on device 0
    try:
        foreign = build(pkg, other, _config(pkg, 32, 3, 12), 1)
        deeper = build(pkg, mctx, _config(pkg, 32, 3, 12, maxDepth=11), 1)
        cfg = _config(pkg, 256, 11, 321)
        full = build(pkg, mctx, cfg, 1)
        roots = full.local_roots()
        no_tree = build(pkg, mctx, cfg, 1, first_slot=4, n_local=1)    # set_roots never called
        wrong = build(pkg, mctx, cfg, 2, first_slot=4, n_local=1)
        bad = roots.copy()
        bad[[4, 5]] = bad[[5, 4]]                                        # the manifest's roots of slots 4 and 5 swapped
        wrong.set_roots(bad)
        cases = [
            ("NULL dataset", [good.h, None], [0, 0]),
            ("another context", [good.h, good.h, foreign.h], [0, 1, 0]),
            ("circuit parameters", [good.h, deeper.h], [0, 0]),
            ("not local", [good.h, good.h, good.h, good.h], [0, 1, 2, 3]),
            ("no dataset tree", [good.h, no_tree.h], [0, 4]),
            ("differs from the slot's built root", [good.h, full.h, wrong.h], [0, 4, 4]),
        ]
        for what, hs, slots in cases:
            st, outs, msg = raw_many(pkg, mctx, hs, slots, [1] * len(hs))
            assert st == CP2_ERR_INVALID, what
            assert outs == [None] * len(hs), what
            assert ("request %d:" % (len(hs) - 1)) in msg and what in msg, (what, msg)
        with pytest.raises(pkg.CodexP2Error) as ei:
            mctx.export_proof_inputs_many([(good, 0, 1), (wrong, 4, 1)])
        assert ei.value.status == CP2_ERR_INVALID and "request 1:" in str(ei.value)
        # the same datasets are fine once the request is right
        assert mctx.proof_inputs_many([(good, 2, 1), (full, 4, 1)])[1].json() == per_call(full, 4, 1)
    finally:
        other.close()


@pytest.mark.parametrize("how", ["rewritten", "directory"])
def test_changed_slot_data_fails_the_whole_call(pkg, mctx, tmp_path, how):
    base = str(tmp_path / "slot")
    write_slot_files(base, 3, 32, CIRCUIT["cellSize"], 99)
    ds = build(pkg, mctx, _config(pkg, 32, 3, 0, base), 2)
    good = mctx.proof_inputs_many([(ds, 2, 1)])[0].json()
    path = base + "2.dat"
    if how == "rewritten":
        data = bytearray(open(path, "rb").read())
        for i in range(0, len(data), 64):
            data[i] ^= 0xff                                              # every cell changes, so every touched block does
        open(path, "wb").write(bytes(data))
    else:
        os.remove(path)
        os.mkdir(path)
    st, outs, msg = raw_many(pkg, mctx, [ds.h, ds.h, ds.h], [0, 2, 1], [1, 1, 1])
    assert st == CP2_ERR_IO and outs == [None] * 3
    assert "request 1:" in msg and "block " in msg and "of slot 2" in msg, msg
    if how == "directory":
        assert "cannot read" in msg, msg
        os.rmdir(path)
    else:
        os.remove(path)
    write_slot_files(base, 3, 32, CIRCUIT["cellSize"], 99)                # the original data again: the same text as before
    assert mctx.proof_inputs_many([(ds, 2, 1)])[0].json() == good


def test_export_writes_the_per_call_texts(pkg, mctx, datasets, tmp_path):
    reqs = mixed_requests(datasets)
    want = [per_call(ds, s, e) for ds, s, e in reqs]
    paths = [str(tmp_path / ("in_%d.json" % i)) if i % 4 else None for i in range(len(reqs))]
    total = mctx.export_proof_inputs_many(reqs, paths, threads=3, batch=5)
    assert total == sum(len(w) for w in want)
    for p, w in zip(paths, want):
        if p:
            assert open(p).read() == w
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in paths if p)
    assert mctx.export_proof_inputs_many(reqs, None, threads=2) == total   # serialise only
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in paths if p)
    assert mctx.export_proof_inputs_many([]) == 0


@pytest.mark.parametrize("files", [False, True], ids=["fake", "files"])
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_dataset_export_in_chunks_is_the_batch_call_and_export_many(pkg, mctx, tmp_path, mode, files):
    """Dataset.export_proof_inputs over 9 of 11 slots with batch=4 -- chunks of 4, 4 and 1, the second and third generated while the
    one before is formatted -- writes byte for byte what one cp2_proof_inputs_generate_batch call gives for the same slots, from either
    source and whatever the dataset keeps; cp2_proof_inputs_export_many over the same requests under the same entropy writes the same
    files (keep-trees modes 1 and 2), and the byte totals agree."""
    base = None
    if files:
        base = str(tmp_path / "slot")
        write_slot_files(base, 11, 64, 256, 31)
    ds = build(pkg, mctx, pkg.make_config(nSlots=11, nCells=64, cellSize=256, blockSize=2048, nSamples=5, file=base), mode)
    slots, entropy = [10, 0, 3, 1, 7, 2, 9, 5, 4], R_MOD + 987654321
    want = [p.json() for p in ds.proof_inputs(slots, entropy)]
    out = tmp_path / "out"
    out.mkdir()
    total = ds.export_proof_inputs(slots, entropy, str(out), threads=3, batch=4)
    assert total == sum(len(w) for w in want)
    assert sorted(os.listdir(out)) == sorted("input_%d.json" % s for s in slots)
    for s, w in zip(slots, want):
        assert open(out / ("input_%d.json" % s)).read() == w, s
    assert ds.export_proof_inputs(slots, entropy, None, threads=2, batch=4) == total   # serialise only
    if mode in (1, 2):
        many = tmp_path / "many"
        many.mkdir()
        paths = [str(many / ("input_%d.json" % s)) for s in slots]
        assert mctx.export_proof_inputs_many([(ds, s, entropy) for s in slots], paths, threads=3, batch=4) == total
        for s, p in zip(slots, paths):
            assert open(p, "rb").read() == open(out / ("input_%d.json" % s), "rb").read(), s
    ds.free()


CHUNK_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
import __graft_entry__ as g
pkg = g.load_package()
ctx = pkg.Context(0)
base = %(base)r
def cfg(seed, n_slots, file=None):
    return pkg.make_config(maxDepth=8, maxLog2NSlots=3, cellSize=2048, blockSize=65536, nSlots=n_slots, nCells=64, nSamples=10,
                           seed=seed, file=file)
ctx.set_keep_trees(2)
dss = [ctx.dataset(cfg(5, 4)), ctx.dataset(cfg(6, 3, base)), ctx.dataset(cfg(7, 2))]
ctx.set_keep_trees(1)
dss.append(ctx.dataset(cfg(8, 2)))
reqs = [(dss[i %% 4], (i * 7) %% (4, 3, 2, 2)[i %% 4], 1000 + i) for i in range(14)]
got = [p.json() for p in ctx.proof_inputs_many(reqs)]
want = [ds.proof_input(s, e).json() for ds, s, e in reqs]
total = ctx.export_proof_inputs_many(reqs, None, threads=2, batch=4)
# the one-dataset batch over every slot of a compact dataset, fake source and slot files: one slot per pass as well
# ... and equal to what the same configurations give slot by slot with every node kept
full = [ctx.dataset(cfg(5, 4)), ctx.dataset(cfg(6, 3, base))]
batch_same = all([p.json() for p in ds.proof_inputs(list(range(k)), 2000 + k)] == [ds.proof_input(s, 2000 + k).json() for s in range(k)] ==
                 [f.proof_input(s, 2000 + k).json() for s in range(k)] for ds, f, k in ((dss[0], full[0], 4), (dss[1], full[1], 3)))
print(json.dumps({"same": got == want, "total_ok": total == sum(len(w) for w in want), "n": len(got), "batch_same": batch_same}))
"""


def test_compact_work_in_several_chunks(pkg, tmp_path):
    """CODEX_P2_STAGE_MB=1 with 64 KiB blocks and 10 samples: one compact request per chunk, from cp2_proof_inputs_generate_many and
    from cp2_proof_inputs_generate_batch on one compact dataset."""
    base = str(tmp_path / "slot")
    write_slot_files(base, 3, 64, 2048, 5)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CODEX_P2_") and not k.startswith("CP2_")}
    env["CODEX_P2_STAGE_MB"] = "1"
    r = subprocess.run([sys.executable, "-c", CHUNK_CHILD % {"root": ROOT, "base": base}], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == {"same": True, "total_ok": True, "n": 14, "batch_same": True}


def test_scale_1024_requests_over_256_datasets(pkg, mctx):
    dss = []
    for i in range(256):
        dss.append(build(pkg, mctx, _config(pkg, 32, 4, 1000 + i), (1, 2, 1, 0)[i % 4]))
    rng = np.random.default_rng(7)
    reqs = [(dss[int(rng.integers(256))], int(rng.integers(4)), int(rng.integers(2**62)) * (i + 1)) for i in range(1024)]
    got = [p.json() for p in mctx.proof_inputs_many(reqs)]
    want = [per_call(ds, s, e) for ds, s, e in reqs]
    assert got == want
