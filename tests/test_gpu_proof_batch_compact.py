"""GPU suite: cp2_proof_inputs_generate_batch on a COMPACT dataset (keep_trees 2) -- the input.json of every slot of the batch is byte
for byte what the same dataset built with every node kept (keep_trees 1) gives slot by slot, and the oracle's where there is one:
both sources, a strict sub-range of the slots, repeated and descending slot lists, entropies >= r, one block per slot, one cell per
block, no samples, a cell size that is no multiple of 4; and a rewritten slot file fails the whole call."""
import ctypes
import os

import numpy as np
import pytest

from test_gpu_proof_many import CIRCUIT, CP2_ERR_IO, R_MOD, _config, build, write_slot_files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def both(pkg, ctx, n_cells, n_slots, seed, base=None, **circuit):
    """the same dataset twice: every node kept (the reference of these tests), and compact"""
    cfg = _config(pkg, n_cells, n_slots, seed, base, **circuit)
    return build(pkg, ctx, cfg, 1), build(pkg, ctx, cfg, 2)


def slot_files(tmp_path, n_slots, n_cells, seed, cell_size=CIRCUIT["cellSize"]):
    base = str(tmp_path / "slot")
    write_slot_files(base, n_slots, n_cells, cell_size, seed)
    return base


def assert_batch_equals_per_slot(full, compact, slots, entropy):
    got = [p.json() for p in compact.proof_inputs(slots, entropy)]
    want = {s: full.proof_input(s, entropy).json() for s in set(slots)}
    assert got == [want[s] for s in slots]
    return got


@pytest.mark.parametrize("files", [False, True], ids=["fake", "files"])
def test_every_slot_of_a_compact_dataset(pkg, bctx, entry, tmp_path, files):
    n_cells, n_slots, seed = 32, 5, 4101
    base = slot_files(tmp_path, n_slots, n_cells, seed) if files else None
    full, compact = both(pkg, bctx, n_cells, n_slots, seed, base)
    got = assert_batch_equals_per_slot(full, compact, list(range(n_slots)), 12345)
    if not files:   # the oracle's input.json (fake source: the Python restatement of the reference)
        _, ref = entry.load_oracle()
        c = dict(CIRCUIT, nCells=n_cells, nSlots=n_slots, seed=seed)
        for s in (0, 3):
            assert got[s] == ref.export_json(ref.generate_proof_input(c, s, 12345))


@pytest.mark.parametrize("files", [False, True], ids=["fake", "files"])
def test_a_strict_sub_range_with_roots_from_a_full_build(pkg, bctx, tmp_path, files):
    """first_slot > 0 and n_local < nSlots: the generator is seeded per slot, the files are named by the global slot index"""
    n_cells, n_slots, seed = 32, 11, 4102
    base = slot_files(tmp_path, n_slots, n_cells, seed) if files else None
    cfg = _config(pkg, n_cells, n_slots, seed, base)
    full = build(pkg, bctx, cfg, 1)
    part = build(pkg, bctx, cfg, 2, first_slot=4, n_local=3)
    part.set_roots(full.local_roots())
    assert_batch_equals_per_slot(full, part, [4, 5, 6], 777)
    assert_batch_equals_per_slot(full, part, [6, 4], 2**200 + 1)
    with pytest.raises(pkg.CodexP2Error):
        part.proof_inputs([3, 4], 777)                                   # slot 3 is not local


def test_repeated_and_descending_slot_lists(pkg, bctx, tmp_path):
    n_cells, n_slots, seed = 32, 5, 4103
    full, compact = both(pkg, bctx, n_cells, n_slots, seed)
    assert_batch_equals_per_slot(full, compact, [3, 1, 1, 0, 3, 3], 5)
    assert_batch_equals_per_slot(full, compact, [4, 3, 2, 1, 0], 5)
    base = slot_files(tmp_path, n_slots, n_cells, seed)
    full, compact = both(pkg, bctx, n_cells, n_slots, seed, base)
    assert_batch_equals_per_slot(full, compact, [4, 4, 2, 1, 1, 0], 6)


def test_entropy_at_and_above_the_modulus_is_canonicalised(pkg, bctx):
    full, compact = both(pkg, bctx, 32, 3, 4104)
    for e in (R_MOD, R_MOD + 5, 2**256 - 1):
        got = assert_batch_equals_per_slot(full, compact, [0, 1, 2], e)
        assert got == [p.json() for p in compact.proof_inputs([0, 1, 2], e % R_MOD)]
        for p in compact.proof_inputs([2], e):
            assert p.roots()[2].tobytes() == (e % R_MOD).to_bytes(32, "little")


@pytest.mark.parametrize("files", [False, True], ids=["fake", "files"])
def test_one_block_per_slot(pkg, bctx, tmp_path, files):
    """nCells * cellSize == blockSize: nothing is stored above the block root but the slot root's own layer"""
    n_cells, n_slots, seed = 4, 6, 4105
    base = slot_files(tmp_path, n_slots, n_cells, seed) if files else None
    full, compact = both(pkg, bctx, n_cells, n_slots, seed, base)
    assert_batch_equals_per_slot(full, compact, [5, 0, 1, 2, 3, 4], 99)


def test_one_block_per_slot_against_the_committed_oracle_fixture(pkg, bctx, golden):
    fx = golden("proof_inputs.json")["inputs"]["odd_slots_one_block"]
    c = fx["config"]
    assert c["nCells"] * c["cellSize"] == c["blockSize"]
    bctx.set_keep_trees(2)
    try:
        compact = bctx.dataset(pkg.make_config(**c))
    finally:
        bctx.set_keep_trees(-1)
    assert compact.tree_mode == 2
    got = compact.proof_inputs(list(range(c["nSlots"])), fx["entropy"])
    assert got[fx["slotIndex"]].json() == golden("input_odd_slots_one_block.json")


@pytest.mark.parametrize("files", [False, True], ids=["fake", "files"])
def test_one_cell_per_block(pkg, bctx, tmp_path, files):
    """blockSize == cellSize: a block's own tree is one compression of its one cell"""
    n_cells, n_slots, seed = 32, 3, 4106
    base = slot_files(tmp_path, n_slots, n_cells, seed) if files else None
    full, compact = both(pkg, bctx, n_cells, n_slots, seed, base, blockSize=CIRCUIT["cellSize"])
    assert_batch_equals_per_slot(full, compact, [2, 0, 1], 31337)


@pytest.mark.parametrize("files", [False, True], ids=["fake", "files"])
def test_no_samples(pkg, bctx, tmp_path, files):
    n_cells, n_slots, seed = 32, 3, 4107
    base = slot_files(tmp_path, n_slots, n_cells, seed) if files else None
    full, compact = both(pkg, bctx, n_cells, n_slots, seed, base, nSamples=0)
    got = assert_batch_equals_per_slot(full, compact, [0, 1, 2], 8)
    pis = compact.proof_inputs([1, 2], 8)
    assert [p.nsamples() for p in pis] == [0, 0]
    assert [p.json() for p in pis] == got[1:]


@pytest.mark.parametrize("files", [False, True], ids=["fake", "files"])
def test_a_cell_size_that_is_no_multiple_of_four(pkg, bctx, tmp_path, files):
    n_cells, n_slots, seed, cell = 32, 3, 4108, 62
    base = slot_files(tmp_path, n_slots, n_cells, seed, cell) if files else None
    full, compact = both(pkg, bctx, n_cells, n_slots, seed, base, cellSize=cell, blockSize=4 * cell)
    assert_batch_equals_per_slot(full, compact, [2, 1, 0, 1], 4242)


def test_a_rewritten_slot_file_fails_the_whole_batch(pkg, bctx, tmp_path):
    """CP2_ERR_IO, a text that names the block and the slot and no request, and every out[i] NULL"""
    n_cells, n_slots, seed = 32, 3, 4109
    base = slot_files(tmp_path, n_slots, n_cells, seed)
    full, compact = both(pkg, bctx, n_cells, n_slots, seed, base)
    good = assert_batch_equals_per_slot(full, compact, [0, 2, 1], 1)
    path = base + "2.dat"
    data = bytearray(open(path, "rb").read())
    for i in range(0, len(data), CIRCUIT["cellSize"]):
        data[i] ^= 0xff                                                  # every cell changes, so every touched block does
    open(path, "wb").write(bytes(data))
    L = bctx.L
    slots = np.array([0, 2, 1], dtype=np.uint64)
    out = (ctypes.c_void_p * 3)(1, 1, 1)                                 # non-NULL: the refusal has to clear them
    entropy = pkg.felt_bytes(1)
    st = L.cp2_proof_inputs_generate_batch(compact.h, slots.ctypes.data, 3, entropy.ctypes.data, out)
    msg = L.cp2_last_error(bctx.h).decode()
    assert st == CP2_ERR_IO and [out[i] for i in range(3)] == [None] * 3
    assert "request" not in msg and "block " in msg and "of slot 2 does not hash to its stored root" in msg, msg
    os.remove(path)
    write_slot_files(base, n_slots, n_cells, CIRCUIT["cellSize"], seed)   # the original data again: the same texts as before
    assert [p.json() for p in compact.proof_inputs([0, 2, 1], 1)] == good
