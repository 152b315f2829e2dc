"""GPU suite: the SlotFile source at the host boundary (slot.nim:57-68, dataset.nim:34).  A slot file that OPENS but whose read fails
(here: a directory in its place, open() succeeds and pread() fails with EISDIR) is CP2_ERR_IO naming the file -- in every builder, in
every proof-input path after a build, and in the cli twin -- never a slot root or cell of zeros with CP2_OK; the end of a file still
reads as zeros, against the oracle; cells over 16384 bytes from files are refused (slot.nim:60-61)."""
import contextlib
import os
import subprocess

import pytest

from test_gpu_round6 import file_config, oracle_texts, write_slot_files

pytestmark = pytest.mark.gpu

CP2_ERR_INVALID, CP2_ERR_IO = -1, -5
# 6 slots of 16 KiB; ring turns of 3 whole files (slot 4 lies inside a turn of several files, slot 5 ends the batch)
GEOM = dict(maxDepth=10, maxLog2NSlots=3, cellSize=256, blockSize=2048, nSlots=6, nCells=64, nSamples=5, seed=90901)
CHUNK = 3 * 64 * 256
ENTROPY = 5150
KNOBS = ["ring", "direct", "mapped"]


@pytest.fixture(scope="module")
def slot_files(oracle, tmp_path_factory):
    C, P = oracle
    base = str(tmp_path_factory.mktemp("slotreads") / "s")
    write_slot_files(C, GEOM, base)
    return base, oracle_texts(C, P, GEOM, ENTROPY)


@contextlib.contextmanager
def directory_in_place(base, k):
    """slot k's file renamed away and a directory put in its place; the file is back afterwards"""
    path = "%s%d.dat" % (base, k)
    os.rename(path, path + ".away")
    os.mkdir(path)
    try:
        yield path
    finally:
        os.rmdir(path)
        os.rename(path + ".away", path)


def assert_read_error(e, path):
    msg = str(e.value)
    assert e.value.status == CP2_ERR_IO, msg
    assert "cannot read " + path in msg and os.strerror(21) in msg, msg      # EISDIR
    assert "does not hash" not in msg, msg                                   # the read is blamed, not the slot data


def knob_context(pkg, how, chunk=CHUNK):
    ctx = pkg.Context(0)
    ctx.set_ingest(3, 2, chunk)
    ctx.set_ingest_direct(1 if how == "direct" else 0)
    ctx.set_ingest_mapped(1 if how == "mapped" else 0)
    return ctx


def set_knobs(c, how):
    c.set_ingest(3, 2, CHUNK)
    c.set_ingest_direct(1 if how == "direct" else 0)
    c.set_ingest_mapped(1 if how == "mapped" else 0)


# ---- a read fails during a build ---------------------------------------------------------------------------------------------------
BUILDERS = ["classic_auto", "classic_compact", "classic_roots", "streamed_in_turn", "streamed_last", "file_units", "multi", "multi_streamed"]


def run_builder(pkg, ctx, m, builder, cfg_d, base):
    cfg = pkg.make_config(**file_config(cfg_d, base))
    if builder.startswith("classic"):
        ctx.set_keep_trees({"classic_auto": -1, "classic_compact": 2, "classic_roots": 0}[builder])
        return ctx.dataset(cfg)
    if builder.startswith("streamed"):
        return ctx.dataset_streamed(cfg, ENTROPY, threads=2)
    if builder == "file_units":     # every slot cut into two units of 32 cells
        return ctx.slot_trees_file_units(base, 2, 0, 2 * cfg_d["nSlots"], cfg_d["cellSize"], cfg_d["blockSize"], cfg_d["nCells"] // 2)
    if builder == "multi":
        return m.dataset(cfg)
    return m.dataset_streamed(cfg, ENTROPY, threads=2)


@pytest.mark.parametrize("how", KNOBS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_a_read_that_fails_during_a_build_is_an_io_error(pkg, slot_files, builder, how):
    """Slot k is a directory: every builder -- classic (automatic / compact / roots-only residency), streamed (k inside a turn of
    several files, and k the batch's last file), file units, cp2_multi whole and streamed -- through the ring, with O_DIRECT and
    with mapped ingestion raises CP2_ERR_IO naming the file.  With the file back, the same context builds and the input.json of
    slot k is the oracle's: nothing was left poisoned."""
    base, want = slot_files
    k = 5 if builder == "streamed_last" else 4
    ctx = knob_context(pkg, how)
    m = None
    try:
        if builder.startswith("multi"):
            m = pkg.Multi([0])
            set_knobs(m.ctx(0), how)
        with directory_in_place(base, k) as path:
            with pytest.raises(pkg.CodexP2Error) as e:
                run_builder(pkg, ctx, m, builder, GEOM, base)
            assert_read_error(e, path)
        got = run_builder(pkg, ctx, m, builder, GEOM, base)
        if builder == "file_units":
            assert got.count == 2 * GEOM["nSlots"]
        elif builder.startswith("streamed") or builder == "multi_streamed":
            got.export_streamed(None, threads=2)
            assert got.streamed_json(k) == want[k]
        else:
            if builder.startswith("classic"):
                got.set_roots(None)
            assert got.proof_input(k, ENTROPY).json() == want[k]
        got.free()
    finally:
        if m is not None:
            m.close()
        ctx.close()


CLI_GEOM_ARGS = ["--depth=10", "--maxslots=8", "--cellsize=256", "--blocksize=2048", "--nsamples=5", "--entropy=%d" % ENTROPY, "--nslots=6",
                 "-K:64", "--field=bn254", "--hash=poseidon2"]


@pytest.mark.parametrize("how", KNOBS)
def test_cli_twin_fails_on_a_slot_file_it_cannot_read(pkg, slot_files, tmp_path, how):
    """The cli twin with --file: slot 4 a directory is an error that names the file, exit status 1 and no input.json; with the file
    back, the committed oracle's input.json of slot 4."""
    base, want = slot_files
    env = dict(os.environ, CP2_INGEST_DIRECT="1" if how == "direct" else "0", CP2_INGEST_MAPPED="1" if how == "mapped" else "0")
    out = str(tmp_path / "input.json")
    args = [pkg.CLI_PATH] + CLI_GEOM_ARGS + ["--file=" + base, "--index=4", "--output=" + out]
    with directory_in_place(base, 4) as path:
        r = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 1 and "cannot read " + path in r.stderr, (r.returncode, r.stderr[-2000:])
        assert not os.path.exists(out)
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out).read() == want[4]


# ---- a read fails after a build ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "compact", "multi_slots", "multi_units"])
def test_a_read_that_fails_after_a_build_is_an_io_error(pkg, slot_files, tmp_path, mode):
    """Built from good files (every node kept, compact trees, cp2_multi with whole slots and with slots cut into two units); then
    slot k's file is replaced by a directory: proof_input(k), proof_inputs([j, k]) and export_proof_inputs raise CP2_ERR_IO naming
    the file (compact: the read, not a block root mismatch) and write no input.json.  With the file back, the same objects give the
    oracle's input.json byte for byte."""
    base, want = slot_files
    j, k = 1, 4
    cfg = pkg.make_config(**file_config(GEOM, base))
    ctx = m = None
    try:
        if mode.startswith("multi"):
            m = pkg.Multi([0])
            m.set_split(2 if mode == "multi_units" else 1)
            ds = m.dataset(cfg)
            assert ds.units_per_slot == (2 if mode == "multi_units" else 1)
        else:
            ctx = pkg.Context(0)
            ctx.set_keep_trees(1 if mode == "full" else 2)
            ds = ctx.dataset(cfg)
            assert ds.tree_mode == (1 if mode == "full" else 2)
            ds.set_roots(None)
        calls = [("proof_input", lambda: ds.proof_input(k, ENTROPY))]
        if ctx is not None:
            calls.append(("proof_inputs", lambda: ds.proof_inputs([j, k], ENTROPY)))
        out = tmp_path / "out"
        out.mkdir()
        calls.append(("export_proof_inputs", lambda: ds.export_proof_inputs([j, k], ENTROPY, directory=str(out), threads=2)))
        with directory_in_place(base, k) as path:
            for name, call in calls:
                with pytest.raises(pkg.CodexP2Error) as e:
                    call()
                assert_read_error(e, path)
            assert sorted(os.listdir(out)) == [], "input.json written by a failing call"
        assert ds.proof_input(k, ENTROPY).json() == want[k]
        if ctx is not None:
            assert [p.json() for p in ds.proof_inputs([j, k], ENTROPY)] == [want[j], want[k]]
        ds.export_proof_inputs([j, k], ENTROPY, directory=str(out), threads=2)
        for s in (j, k):
            assert (out / ("input_%d.json" % s)).read_text() == want[s]
        ds.free()
    finally:
        if m is not None:
            m.close()
        if ctx is not None:
            ctx.close()


# ---- the end of a file reads as zeros, against the oracle ----------------------------------------------------------------------------
EOF_GEOM = dict(GEOM, nSamples=24, seed=90902)


@pytest.mark.parametrize("how", ["full", "compact", "streamed"])
def test_end_of_file_reads_as_zeros_like_the_reference(pkg, oracle, tmp_path, how):
    """Slot 1 empty, slot 3 ending mid-cell, slot 4 ending exactly on a block boundary: the input.json of each (and of a whole slot)
    equals the oracle's, which reads the files the reference's way (P.generate_proof_input with the `file` config) -- after a
    classic build with every node or compact trees, and from the streamed export."""
    C, P = oracle
    base = str(tmp_path / "e")
    write_slot_files(C, EOF_GEOM, base)
    open(base + "1.dat", "wb").close()
    with open(base + "3.dat", "r+b") as f:
        f.truncate(256 * 21 + 100)                     # 21 cells and 100 bytes
    with open(base + "4.dat", "r+b") as f:
        f.truncate(2048 * 3)                           # 3 whole blocks
    cf = file_config(EOF_GEOM, base)
    ctx = pkg.Context(0)
    try:
        ctx.set_ingest(3, 2, CHUNK)
        if how == "streamed":
            ds = ctx.dataset_streamed(pkg.make_config(**cf), ENTROPY, threads=2, group_slots=2)
            ds.export_streamed(None, threads=2)
            got = {s: ds.streamed_json(s) for s in (0, 1, 3, 4)}
        else:
            ctx.set_keep_trees(1 if how == "full" else 2)
            ds = ctx.dataset(pkg.make_config(**cf))
            ds.set_roots(None)
            got = {s: ds.proof_input(s, ENTROPY).json() for s in (0, 1, 3, 4)}
        for s, text in got.items():
            assert text == P.export_json(P.generate_proof_input(dict(cf), s, ENTROPY)), "slot %d" % s
        ds.free()
    finally:
        ctx.close()


# ---- cells over 16384 bytes from files (slot.nim:60-61) ------------------------------------------------------------------------------
BIG_OK = dict(maxDepth=6, maxLog2NSlots=1, cellSize=16384, blockSize=65536, nSlots=2, nCells=8, nSamples=3, seed=90903)
BIG_BAD = dict(BIG_OK, cellSize=32768, nCells=8)   # (a geometry the fake source and units take: 4 blocks of 2 cells)


def test_slot_file_cells_of_16384_bytes_are_accepted(pkg, oracle, tmp_path):
    """The largest cell the reference reads from a file: the classic and streamed builds match the oracle."""
    C, P = oracle
    base = str(tmp_path / "b")
    write_slot_files(C, BIG_OK, base)
    want = oracle_texts(C, P, BIG_OK, ENTROPY)
    cfg = pkg.make_config(**file_config(BIG_OK, base))
    ctx = pkg.Context(0)
    try:
        ds = ctx.dataset(cfg)
        ds.set_roots(None)
        assert [ds.proof_input(s, ENTROPY).json() for s in range(2)] == want
        ds.free()
        ds = ctx.dataset_streamed(cfg, ENTROPY, threads=2)
        ds.export_streamed(None, threads=2)
        assert [ds.streamed_json(s) for s in range(2)] == want
        ds.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("builder", BUILDERS)
def test_slot_file_cells_over_16384_bytes_are_refused(pkg, oracle, tmp_path, builder):
    """cellSize 32768 from files: CP2_ERR_INVALID from every builder; the fake source still builds at that size."""
    C, _ = oracle
    base = str(tmp_path / "b")
    write_slot_files(C, BIG_BAD, base)
    ctx = pkg.Context(0)
    m = pkg.Multi([0]) if builder.startswith("multi") else None
    try:
        with pytest.raises(pkg.CodexP2Error) as e:
            run_builder(pkg, ctx, m, builder, BIG_BAD, base)
        assert e.value.status == CP2_ERR_INVALID, str(e.value)
    finally:
        if m is not None:
            m.close()
        ctx.close()


def test_fake_cells_over_16384_bytes_still_build_and_the_cli_twin_refuses_them_from_files(pkg, oracle, tmp_path):
    C, _ = oracle
    ctx = pkg.Context(0)
    try:
        ds = ctx.dataset(pkg.make_config(**BIG_BAD))
        roots = ds.local_roots()
        for s in range(2):
            assert bytes(roots[s]) == bytes(C.fake_slot_root(C.slot_seed(BIG_BAD["seed"], s), 32768, 65536, 8))
        ds.free()
    finally:
        ctx.close()
    base = str(tmp_path / "b")
    write_slot_files(C, BIG_BAD, base)
    out = str(tmp_path / "x.json")
    r = subprocess.run([pkg.CLI_PATH, "--depth=6", "--maxslots=2", "--cellsize=32768", "--blocksize=65536", "--nsamples=3", "--nslots=2", "-K:8",
                        "--entropy=%d" % ENTROPY, "--index=1", "--field=bn254", "--hash=poseidon2", "--file=" + base, "--output=" + out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "[AssertionDefect]" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not os.path.exists(out)
