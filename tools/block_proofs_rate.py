"""Rate of cp2_blocks_verify against cp2_dataset_repair_blocks (check only) over the same candidate bytes, and of cp2_dataset_block_proofs.

The two checks share their data path (upload, cell hashing, block trees) and differ in the last step: repair compares each block root
with a kept row, verify walks it up its Merkle path to the slot root (k_block_path_roots: `depth` dependent permutations).
  files   --slots 128 slot files of --slot-mib 8 MiB (2^12 cells x 2048 B, 64 KiB blocks: 128 blocks, depth 7), every block a candidate:
          16 384 blocks, 1 GiB, against a compact dataset's kept block roots (repair) and against its 128 slot roots (verify)
  deep    the same number of candidate blocks against ONE fake-source compact slot of 2^--deep-log2 cells (2^22: 131 072 blocks, depth 17),
          where the walk is longest
  serve   cp2_dataset_block_proofs for the 16 384 requests of `files`, every node kept and compact
In one process, after a warm-up of each leg, --repeats rounds of the legs alternated; pageable candidates and a pinned copy.  The paths
are the ones the dataset serves.  verify_over_repair = repair_s / verify_s.  Prints one JSON line and, with --out, writes it with a heading.

    python tools/block_proofs_rate.py [--slots 128] [--slot-mib 8] [--deep-log2 22] [--repeats 2] [--dir D] [--out FILE]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

CELL, BLOCK = 2048, 65536
CPB = BLOCK // CELL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--slot-mib", type=int, default=8)
    ap.add_argument("--deep-log2", type=int, default=22)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the slot files go (default: a temporary directory, removed at the end)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    ctx = pkg.Context(0)
    d = tempfile.mkdtemp(prefix="block_proofs_rate_", dir=a.dir)
    slot_bytes = a.slot_mib << 20
    n_cells, nb = slot_bytes // CELL, slot_bytes // BLOCK
    n_req = a.slots * nb
    record = {"repeats": a.repeats}

    def timed(f):
        ctx.sync()
        t = time.perf_counter()
        r = f()
        return time.perf_counter() - t, r

    def build(cfg, mode):
        ctx.set_keep_trees(mode)
        try:
            return ctx.dataset(cfg)
        finally:
            ctx.set_keep_trees(-1)

    def compare(ds, geom, reqs, root_block, cand, pinned):
        """repair (check only) and verify alternated, pageable and pinned; every candidate is right, so every verdict is a match"""
        roots = ds.local_roots()
        _, paths = ds.block_proofs(reqs)
        legs = {
            "repair": lambda: ds.repair_blocks(reqs, cand, check_only=True)[0],
            "verify": lambda: ctx.blocks_verify(*geom, roots, root_block, cand, paths, want_roots=False)[0],
            "repair_pin": lambda: ds.repair_blocks(reqs, pinned, check_only=True)[0],
            "verify_pin": lambda: ctx.blocks_verify(*geom, roots, root_block, pinned, paths, want_roots=False)[0],
        }
        times = {k: [] for k in legs}
        for k, f in legs.items():                                 # warm-up
            assert (timed(f)[1] == 0).all(), k
        for _ in range(a.repeats):
            for k, f in legs.items():
                times[k].append(timed(f)[0])
        med = {k: statistics.median(v) for k, v in times.items()}
        gb = cand.nbytes / 1e9
        out = {"depth": int(paths.shape[1]), "path_MiB": round(paths.nbytes / 2**20, 2)}
        out.update({k + "_s": round(v, 4) for k, v in med.items()})
        out.update({k + "_GBps": round(gb / v, 2) for k, v in med.items()})
        out["verify_over_repair"] = round(med["repair"] / med["verify"], 3)
        out["verify_pin_over_repair_pin"] = round(med["repair_pin"] / med["verify_pin"], 3)
        return out

    try:
        # ---- files: every block of every slot file, in (slot, block) order
        base = os.path.join(d, "slot_")
        rng = np.random.default_rng(7)
        parts = []
        for k in range(a.slots):
            b = rng.integers(0, 256, slot_bytes, dtype=np.uint8)
            b.tofile("%s%d.dat" % (base, k))
            parts.append(b)
        cand = np.concatenate(parts)
        del parts
        pinned = torch.from_numpy(cand).pin_memory().numpy()
        reqs = np.array([(s, b) for s in range(a.slots) for b in range(nb)], dtype=np.uint64)
        cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (a.slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=a.slots,
                              nCells=n_cells, nSamples=100, seed=1, file=base)
        record["files"] = {"workload": "%d slot files x %d MiB (2^%d cells x 2048 B, 64 KiB blocks), page cache; %d candidate blocks (%d MiB), compact dataset" %
                           (a.slots, a.slot_mib, n_cells.bit_length() - 1, n_req, n_req * BLOCK >> 20)}
        ds = build(cfg, 2)
        record["files"].update(compare(ds, (CELL, BLOCK, n_cells), reqs, reqs, cand, pinned))
        # ---- serve: the proofs of those requests from the compact layers and from every node
        serve = {}
        for mode in (2, 1):
            if mode == 1:
                ds.free()
                ds = build(cfg, 1)
            timed(lambda: ds.block_proofs(reqs))
            ts = [timed(lambda: ds.block_proofs(reqs))[0] for _ in range(2 * a.repeats)]
            serve["mode%d_s" % mode] = round(statistics.median(ts), 5)
            serve["mode%d_proofs_per_s" % mode] = round(n_req / statistics.median(ts))
        ds.free()
        record["serve"] = dict(serve, requests=n_req, depth=record["files"]["depth"])
        del pinned, cand
        # ---- deep: the first n_req blocks of one fake-source slot of 2^deep_log2 cells
        deep_cells = 1 << a.deep_log2
        dcfg = pkg.make_config(maxDepth=32, maxLog2NSlots=1, cellSize=CELL, blockSize=BLOCK, nSlots=1, nCells=deep_cells, nSamples=100, seed=1)
        ds = build(dcfg, 2)
        n_deep = min(n_req, deep_cells // CPB)
        cand = ctx.gen_fake_cells(ctx.slot_seed(1, 0), 0, n_deep * CPB, CELL).reshape(-1)
        pinned = torch.from_numpy(cand).pin_memory().numpy()
        reqs = np.array([(0, b) for b in range(n_deep)], dtype=np.uint64)
        record["deep"] = {"workload": "one fake-source compact slot of 2^%d cells x 2048 B (%d blocks); its first %d blocks as candidates (%d MiB)" %
                          (a.deep_log2, deep_cells // CPB, n_deep, n_deep * BLOCK >> 20)}
        record["deep"].update(compare(ds, (CELL, BLOCK, deep_cells), reqs, reqs, cand, pinned))
        ds.free()
    finally:
        shutil.rmtree(d, ignore_errors=True)
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        # the heading names the workload's arguments only: where the files and the record went is not part of the measurement
        args = ["--slots %d" % a.slots, "--slot-mib %d" % a.slot_mib, "--deep-log2 %d" % a.deep_log2, "--repeats %d" % a.repeats]
        with open(a.out, "w") as f:
            f.write("tools/block_proofs_rate.py on one MI355X (%s; medians of alternated repair / verify / repair_pin / verify_pin rounds after a "
                    "warm-up):\n%s\n" % (" ".join(args), line))


if __name__ == "__main__":
    main()
