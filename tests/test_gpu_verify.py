"""GPU suite: cp2_proof_inputs_verify (k_verify_samples) says what SampleAndProve accepts -- every producer path's output is accepted,
and every mutation gets the verdict of tests/circuit_verdict.py, sample by sample."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import circuit_verdict as V
import kernel_models as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = ("testmain_small", "odd_slots_one_block", "params_default")

# (name, config): odd top nodes and odd nf; one slot and even nf; nSlots = 2^maxLog2NSlots with a singleton slot tree (nCells = cellsPerBlock);
# cellsPerBlock = 2; maxDepth = log2 nCells (no padding) with 2048-byte cells
GEOMETRIES = [
    ("odd_slots", dict(maxDepth=8, maxLog2NSlots=4, cellSize=64, blockSize=256, nSlots=11, nCells=32, nSamples=5, seed=3)),
    ("one_slot", dict(maxDepth=6, maxLog2NSlots=2, cellSize=32, blockSize=64, nSlots=1, nCells=16, nSamples=4, seed=4)),
    ("full_singleton", dict(maxDepth=5, maxLog2NSlots=3, cellSize=128, blockSize=512, nSlots=8, nCells=4, nSamples=3, seed=5)),
    ("no_padding", dict(maxDepth=6, maxLog2NSlots=2, cellSize=2048, blockSize=8192, nSlots=3, nCells=64, nSamples=6, seed=6)),
]
ENTROPY = 424242


def _cfg(pkg, c, **kw):
    return pkg.make_config(**dict(c, **kw))


def _circuit(c):
    return {k: c[k] for k in ("maxDepth", "maxLog2NSlots", "cellSize", "blockSize")}


def _verify_texts(pkg, ctx, c, texts):
    ps = [pkg.parse_proof_input(_cfg(pkg, c, nSamples=0), t) for t in texts]
    return ctx.verify_proof_inputs(ps)


def _accepted(status, ok):
    return status.tolist() == [0] * len(status) and bool(ok.all())


def test_goldens_are_accepted(pkg, ctx, golden):
    for name in GOLDENS:
        c = golden("proof_inputs.json")["inputs"][name]["config"]
        status, ok = _verify_texts(pkg, ctx, c, [golden("input_%s.json" % name)])
        assert _accepted(status, ok), name
        assert ok.shape == (1, c["nSamples"])


@pytest.mark.parametrize("name,c", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_every_producer_path_is_accepted(pkg, ctx, name, c, tmp_path):
    """Objects and their JSON round trip, from the batch generator, a compact-tree build, slot files, the pipelined export and
    cp2_multi on this one device: all accepted, every sample."""
    cfg = _cfg(pkg, c)
    slots = list(range(c["nSlots"]))
    ds = ctx.dataset(cfg)
    objs = ds.proof_inputs(slots, ENTROPY)
    status, ok = ctx.verify_proof_inputs(objs)
    assert _accepted(status, ok) and ok.shape == (len(slots), c["nSamples"])
    status, ok = _verify_texts(pkg, ctx, c, [p.json() for p in objs])
    assert _accepted(status, ok)
    out = tmp_path / "export"
    out.mkdir()
    ds.export_proof_inputs(slots, ENTROPY, directory=str(out), threads=2)
    status, ok = _verify_texts(pkg, ctx, c, [open(out / ("input_%d.json" % s)).read() for s in slots])
    assert _accepted(status, ok)
    ds.free()
    # compact trees (block roots and up kept)
    ctx.set_keep_trees(2)
    try:
        ds = ctx.dataset(cfg)
        status, ok = ctx.verify_proof_inputs(ds.proof_inputs(slots, ENTROPY + 1))
        assert _accepted(status, ok)
        ds.free()
    finally:
        ctx.set_keep_trees(-1)
    # slot files
    base = str(tmp_path / "slot")
    rng = np.random.default_rng(c["seed"])
    for s in slots:
        rng.integers(0, 256, c["nCells"] * c["cellSize"], dtype=np.uint8).tofile("%s%d.dat" % (base, s))
    ds = ctx.dataset(_cfg(pkg, c, file=base))
    status, ok = ctx.verify_proof_inputs(ds.proof_inputs(slots, ENTROPY))
    assert _accepted(status, ok)
    ds.free()
    # cp2_multi on one device, whole slots
    m = pkg.Multi([0])
    try:
        md = m.dataset(cfg)
        objs = [md.proof_input(s, ENTROPY) for s in slots]
        status, ok = ctx.verify_proof_inputs(objs)
        assert _accepted(status, ok)
        md.free()
    finally:
        m.close()


def _base(pkg, ctx, c, slot=None):
    ds = ctx.dataset(_cfg(pkg, c))
    p = ds.proof_input(c["nSlots"] // 2 if slot is None else slot, ENTROPY)
    text = p.json()
    ds.free()
    return V.from_text(text)


def _check(pkg, ctx, c, ds_):
    """GPU verdicts of felt dicts == the helper's, per input and per sample; returns them."""
    status, ok = _verify_texts(pkg, ctx, c, [V.to_text(d) for d in ds_])
    for i, d in enumerate(ds_):
        want = V.verdict(d, _circuit(c))
        assert (int(status[i]), ok[i].tolist()) == (want[0], want[1]), (i, int(status[i]), ok[i].tolist(), want)
    return status, ok


def test_targeted_mutations(pkg, ctx):
    c = GEOMETRIES[0][1]
    d0 = _base(pkg, ctx, c)
    md, m, ns = c["maxDepth"], c["maxLog2NSlots"], c["nSamples"]
    depth_used = (c["nCells"] - 1).bit_length()                  # path entries below the selected layer
    cases = []                                                      # (dict, expected status or None, expected sample bytes or None)

    def mut(f, st, ok):
        d = V.copy(d0)
        f(d)
        cases.append((d, st, ok))

    only = lambda s: [1 if i != s else 0 for i in range(ns)]        # noqa: E731
    mut(lambda d: None, 0, [1] * ns)
    mut(lambda d: d["cellData"][2].__setitem__(1, d["cellData"][2][1] + 1), V.SAMPLE, only(2))
    mut(lambda d: d["merklePaths"][3].__setitem__(depth_used - 1, d["merklePaths"][3][depth_used - 1] ^ 1), V.SAMPLE, only(3))
    mut(lambda d: d["merklePaths"][0].__setitem__(md - 1, 1), 0, [1] * ns)                 # padding above the selected layer
    mut(lambda d: d["slotProof"].__setitem__(0, d["slotProof"][0] + 1), V.DATASET_ROOT, [1] * ns)
    mut(lambda d: d.__setitem__("dataSetRoot", d["dataSetRoot"] + 1), V.DATASET_ROOT, [1] * ns)
    mut(lambda d: d.__setitem__("entropy", d["entropy"] + 1), None, None)
    mut(lambda d: d.__setitem__("slotRoot", d["slotRoot"] + 1), V.DATASET_ROOT | V.SAMPLE, [0] * ns)
    mut(lambda d: d.__setitem__("slotIndex", (d["slotIndex"] + 1) % c["nSlots"]), V.DATASET_ROOT, [1] * ns)
    for k, v in (("nCellsPerSlot", 1), ("nCellsPerSlot", 3), ("nCellsPerSlot", 1 << (md + 1)), ("nSlotsPerDataSet", 0),
                 ("nSlotsPerDataSet", (1 << m) + 1), ("slotIndex", 1 << m)):
        mut(lambda d, k=k, v=v: d.__setitem__(k, v), V.SHAPE, [0] * ns)
    status, ok = _check(pkg, ctx, c, [d for d, _, _ in cases])
    for i, (d, st, want_ok) in enumerate(cases):
        if st is not None:
            assert int(status[i]) == st, (i, int(status[i]))
        if want_ok is not None:
            assert ok[i].tolist() == want_ok, (i, ok[i].tolist())


def test_random_mutations_match_the_helper(pkg, ctx):
    c = GEOMETRIES[0][1]
    rng = random.Random(7)
    bases = [_base(pkg, ctx, c, slot=s) for s in (0, 5, 10)]
    md, m, ns, nf = c["maxDepth"], c["maxLog2NSlots"], c["nSamples"], len(bases[0]["cellData"][0])
    out = []
    for _ in range(200):
        d = V.copy(rng.choice(bases))
        what = rng.randrange(7)
        val = rng.choice([0, 1, rng.randrange(1 << 64), rng.randrange(V.R_MOD)])
        if what == 0:
            d["cellData"][rng.randrange(ns)][rng.randrange(nf)] = val
        elif what == 1:
            d["merklePaths"][rng.randrange(ns)][rng.randrange(md)] = val
        elif what == 2:
            d["slotProof"][rng.randrange(m)] = val
        elif what == 3:
            d[rng.choice(["dataSetRoot", "entropy", "slotRoot"])] = val
        elif what == 4:
            d["slotIndex"] = rng.randrange(1 << (m + 1))
        elif what == 5:
            d["nCellsPerSlot"] = rng.choice([2, 4, 8, 16, 32, 64, 3, 1 << md, 1 << (md + 1)])
        else:
            d["nSlotsPerDataSet"] = rng.randrange((1 << m) + 2)
        out.append(d)
    _check(pkg, ctx, c, out)


def test_mixed_shapes_in_one_call(pkg, ctx):
    """Three inputs of one circuit, (maxDepth 5, blockTreeDepth 2, maxLog2NSlots 3, 3 felts a cell), that state different nCellsPerSlot
    (below, at and above a block's cells) and nSlotsPerDataSet, each followed by a mutant of itself, parsed and verified in ONE call: the
    host's per-input parameter words and array layout are the ones tests/test_gpu_kernel_units.py hands the launcher directly."""
    geom = (5, 2, 3, 3)
    md, bd, m, nf = geom
    c, ns = K.verify_cfg(geom), 4
    ds = []
    for j, (k, n_slots, si) in enumerate(((1, 1, 0), (2, 5, 4), (5, 8, 2))):
        d = K.verify_build(md, bd, m, nf, ns, 1 << k, n_slots, si, 1000 + j, K.verify_values("mixed shapes", j))
        e = V.copy(d)
        if j == 0:
            e["merklePaths"][3][bd] = (e["merklePaths"][3][bd] + 1) % V.R_MOD          # k < bd: the middle walk's sibling
        elif j == 1:
            e["slotProof"][2] = (e["slotProof"][2] + 1) % V.R_MOD                      # nSlots = 5: all three levels are read
        else:
            e["cellData"][1][nf - 1] = (e["cellData"][1][nf - 1] + 1) % V.R_MOD
        ds += [d, e]
    assert len({d["nCellsPerSlot"] for d in ds}) == 3 and len({d["nSlotsPerDataSet"] for d in ds}) == 3
    status, ok = _check(pkg, ctx, c, ds)
    assert status.tolist() == [0, V.SAMPLE, 0, V.DATASET_ROOT, 0, V.SAMPLE]
    assert ok.tolist() == [[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [1, 0, 1, 1]]


def test_rows_that_encode_no_bytes_are_checked_as_felts(pkg, ctx, oracle):
    """A proof input built entirely from felts (cell rows with values >= 2^248, which no byte string encodes), its block, slot and
    dataset trees built by the oracle's Merkle functions over the rows' hashes: accepted, and cell_data() is None."""
    _, P = oracle
    c = dict(maxDepth=5, maxLog2NSlots=1, cellSize=64, blockSize=256, nSlots=2, nCells=8, nSamples=4)
    cpb, nf = 4, 3
    rng = random.Random(11)
    rows = [[[rng.randrange(1 << 248, V.R_MOD) for _ in range(nf)] for _ in range(c["nCells"])] for _ in range(2)]
    trees = []
    for s in range(2):
        leaves = [V.Poseidon2_hash_rate2(r) for r in rows[s]]
        mini = [P.merkle_tree(leaves[b * cpb:(b + 1) * cpb]) for b in range(c["nCells"] // cpb)]
        trees.append((mini, P.merkle_tree([t[-1][0] for t in mini])))
    dset = P.merkle_tree([big[-1][0] for _, big in trees])
    slot = 1
    mini, big = trees[slot]
    d = {"dataSetRoot": dset[-1][0], "entropy": 77, "nCellsPerSlot": c["nCells"], "nSlotsPerDataSet": 2, "slotIndex": slot,
         "slotRoot": big[-1][0], "slotProof": P.pad_merkle_proof(P.merkle_proof(dset, slot), 1)["merklePath"], "cellData": [],
         "merklePaths": []}
    for cnt in range(c["nSamples"]):
        ci = V.sample_index(d, c, cnt)
        prf = P.merge_merkle_proofs(P.merkle_proof(mini[ci // cpb], ci % cpb), P.merkle_proof(big, ci // cpb))
        d["cellData"].append(rows[slot][ci])
        d["merklePaths"].append(P.pad_merkle_proof(prf, c["maxDepth"])["merklePath"])
    assert V.verdict(d, c) == (0, [1] * c["nSamples"])
    p = pkg.parse_proof_input(_cfg(pkg, c), V.to_text(d))
    assert p.cell_data() is None
    status, ok = ctx.verify_proof_inputs([p])
    assert _accepted(status, ok)
    d["cellData"][1][2] += 1
    _check(pkg, ctx, c, [d])


def test_scale_4096_inputs_with_planted_mutations(pkg, ctx):
    """configs[3]'s shape: 4096 slots of 2^12 cells, 100 samples, every slot's input verified in one call; 64 planted single-felt
    mutations are flagged at exactly their (input, sample)."""
    c = dict(maxDepth=32, maxLog2NSlots=12, cellSize=2048, blockSize=65536, nSlots=4096, nCells=4096, nSamples=100, seed=99)
    ctx.set_keep_trees(2)
    try:
        ds = ctx.dataset(_cfg(pkg, c))
        objs = ds.proof_inputs(list(range(c["nSlots"])), ENTROPY)
        ds.free()
    finally:
        ctx.set_keep_trees(-1)
    rng = random.Random(5)
    planted = sorted(rng.sample(range(c["nSlots"]), 64))
    samples = {i: rng.randrange(c["nSamples"]) for i in planted}
    for i in planted:
        p = pkg.parse_proof_input(_cfg(pkg, c), objs[i].json())
        d = json.loads(p.json())
        row = d["cellData"][samples[i]]
        row[5] = str((int(row[5]) + 1) % V.R_MOD)
        objs[i] = pkg.parse_proof_input(_cfg(pkg, c), json.dumps(d))
    status, ok = ctx.verify_proof_inputs(objs)
    want = np.ones((c["nSlots"], c["nSamples"]), dtype=np.uint8)
    for i in planted:
        want[i, samples[i]] = 0
    assert np.array_equal(ok, want)
    assert set(np.nonzero(status)[0].tolist()) == set(planted) and set(status[planted].tolist()) == {V.SAMPLE}


def test_the_verify_program(pkg, golden, tmp_path):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "verify")
    for name in GOLDENS:
        c = golden("proof_inputs.json")["inputs"][name]["config"]
        args = [exe, "--maxdepth=%d" % c["maxDepth"], "--maxslots=%d" % (1 << c["maxLog2NSlots"]), "--cellsize=%d" % c["cellSize"],
                "--blocksize=%d" % c["blockSize"]]
        path = os.path.join(ROOT, "tests", "golden", "input_%s.json" % name)
        r = subprocess.run(args + [path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout == "%s: accepted\n" % path, (r.returncode, r.stdout, r.stderr)
        if name != "testmain_small":
            continue
        d = V.from_text(golden("input_%s.json" % name))
        for s in (3, 7):
            d["cellData"][s][0] += 1
        bad = tmp_path / "bad.json"
        bad.write_text(V.to_text(d))
        r = subprocess.run(args + ["--nsamples=%d" % c["nSamples"], path, str(bad)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and r.stdout == "%s: accepted\n%s: rejected: samples 3,7\n" % (path, bad), (r.stdout, r.stderr)
        d = V.from_text(golden("input_%s.json" % name))
        d["nCellsPerSlot"] = 3
        shape = tmp_path / "shape.json"
        shape.write_text(V.to_text(d))
        r = subprocess.run(args + [str(shape)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and r.stdout == "%s: shape: nCellsPerSlot=3\n" % shape, (r.stdout, r.stderr)
        cut = tmp_path / "cut.json"
        cut.write_text(golden("input_%s.json" % name)[:500])
        r = subprocess.run(args + [str(cut)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "error" in r.stdout, (r.returncode, r.stdout, r.stderr)
