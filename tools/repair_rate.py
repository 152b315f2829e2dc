"""Rate of cp2_dataset_repair_blocks against cp2_hash_cells over the same host bytes, from slot files in the page cache.

Workload (defaults = configs[3]'s geometry): --slots 128 files of --slot-mib 8 MiB (2^12 cells x 2048 B, 64 KiB blocks), every block of
every slot a candidate: 16 384 blocks, 1 GiB.  For a compact dataset (keep-trees 2) and a full one (1), in one process, after a warm-up
of each leg, --repeats rounds of the four legs alternated:
  hash        cp2_hash_cells over the candidate bytes (pageable): the yardstick
  check       repair_blocks(check_only) from the same pageable bytes
  check_pin   repair_blocks(check_only) from a pinned copy (read in place)
  write       repair_blocks: check, then every block written back (the same bytes) and each file synced
The block trees add 31 compressions per 32 cells of 34 permutations each (about 3 %), so a check is expected at 0.9 or more of the
hash's rate (check_over_hash = hash_s / check_s).  Prints one JSON line and, with --out, writes it with a heading.

    python tools/repair_rate.py [--slots 128] [--slot-mib 8] [--repeats 2] [--dir D] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--slot-mib", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the slot files go (default: a temporary directory, removed at the end)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    ctx = pkg.Context(0)
    d = tempfile.mkdtemp(prefix="repair_rate_", dir=a.dir)
    slot_bytes = a.slot_mib << 20
    n_cells, nb = slot_bytes // CELL, slot_bytes // BLOCK
    record = {"repeats": a.repeats, "workload": "%d slot files x %d MiB (2^%d cells x 2048 B, 64 KiB blocks), page cache; %d candidate blocks (%d MiB)" %
              (a.slots, a.slot_mib, n_cells.bit_length() - 1, a.slots * nb, a.slots * a.slot_mib)}
    try:
        base = os.path.join(d, "slot_")
        rng = np.random.default_rng(7)
        parts = []
        for k in range(a.slots):
            b = rng.integers(0, 256, slot_bytes, dtype=np.uint8)
            b.tofile("%s%d.dat" % (base, k))
            parts.append(b)
        cand = np.concatenate(parts)                              # every block of every slot, in (slot, block) order
        del parts
        pinned = torch.from_numpy(cand).pin_memory().numpy()
        reqs = np.array([(s, b) for s in range(a.slots) for b in range(nb)], dtype=np.uint64)
        cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (a.slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=a.slots,
                              nCells=n_cells, nSamples=100, seed=1, file=base)
        for mode in (2, 1):
            ctx.set_keep_trees(mode)
            ds = ctx.dataset(cfg)
            ctx.set_keep_trees(-1)

            def timed(f):
                ctx.sync()
                t = time.perf_counter()
                r = f()
                return time.perf_counter() - t, r

            legs = {
                "hash": lambda: ctx.hash_cells(cand, CELL),
                "check": lambda: ds.repair_blocks(reqs, cand, check_only=True),
                "check_pin": lambda: ds.repair_blocks(reqs, pinned, check_only=True),
                "write": lambda: ds.repair_blocks(reqs, cand),
            }
            times = {k: [] for k in legs}
            for k, f in legs.items():                             # warm-up
                _, r = timed(f)
                if k != "hash":
                    assert (r[0] == pkg.REPAIR_MATCH).all() and r[1] == (0 if k != "write" else len(reqs)), (k, r[1])
            for _ in range(a.repeats):
                for k, f in legs.items():
                    times[k].append(timed(f)[0])
            med = {k: statistics.median(v) for k, v in times.items()}
            gb = cand.nbytes / 1e9
            out = {k + "_s": round(v, 4) for k, v in med.items()}
            out.update({k + "_GBps": round(gb / v, 2) for k, v in med.items()})
            out["check_over_hash"] = round(med["hash"] / med["check"], 3)
            out["check_pin_over_hash"] = round(med["hash"] / med["check_pin"], 3)
            record["mode%d" % mode] = out
            ds.free()
    finally:
        shutil.rmtree(d, ignore_errors=True)
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        # the heading names the workload's arguments only: where the files and the record went is not part of the measurement
        args = ["--slots %d" % a.slots, "--slot-mib %d" % a.slot_mib, "--repeats %d" % a.repeats]
        with open(a.out, "w") as f:
            f.write("tools/repair_rate.py on one MI355X (%s; medians of alternated hash / check / check_pin / write rounds after a warm-up):\n%s\n" %
                    (" ".join(args), line))


if __name__ == "__main__":
    main()
