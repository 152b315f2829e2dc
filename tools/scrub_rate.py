"""Rate of cp2_dataset_scrub against the build it re-does, from slot files in the page cache.

Legs (defaults = the storage-node shapes):
  small   --slots 4096 files of --slot-mib 8 MiB (configs[3]: 2^12 cells x 2048 B, 64 KiB blocks), keep-trees modes 1 and 2
  large   --big-slots 16 files of --big-gib 8 GiB (2^22 cells), mode 2
For each leg and mode, in one process: the files are written (and so sit in the page cache), one build and one scrub as a warm-up,
then --repeats rounds of (build, scrub) alternated.  A scrub hashes the same bytes as the build and compares instead of copying out,
so the rate ratio build_s / scrub_s is expected at 0.95 or more.  Prints one JSON line and, with --out, writes it with a heading.

    python tools/scrub_rate.py [--slots 4096] [--slot-mib 8] [--big-slots 16] [--big-gib 8] [--repeats 2] [--dir D] [--out FILE]
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


def write_files(base, n_slots, slot_bytes):
    """n_slots files of slot_bytes each, from one random 64 MiB pattern (hashing cost does not depend on the bytes)"""
    pat = np.random.default_rng(7).integers(0, 256, min(slot_bytes, 64 << 20), dtype=np.uint8).tobytes()
    for k in range(n_slots):
        with open("%s%d.dat" % (base, k), "wb") as f:
            left = slot_bytes
            while left:
                n = min(left, len(pat))
                f.write(pat[:n])
                left -= n


def leg(pkg, ctx, base, n_slots, n_cells, modes, repeats):
    cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (n_slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=n_slots,
                          nCells=n_cells, nSamples=100, seed=1, file=base)
    out = {}
    for mode in modes:
        ctx.set_keep_trees(mode)

        def build():
            ctx.sync()
            t = time.perf_counter()
            ds = ctx.dataset(cfg)
            return ds, time.perf_counter() - t

        ds, _ = build()                                          # warm-up
        assert ds.scrub(cap=16)[2] == 0
        ds.free()
        b_s, s_s = [], []
        for _ in range(repeats):
            ds, t = build()
            b_s.append(t)
            t = time.perf_counter()
            gr, bad, n = ds.scrub(cap=16)
            s_s.append(time.perf_counter() - t)
            assert n == 0, bad
            ds.free()
        ctx.set_keep_trees(-1)
        b, s = statistics.median(b_s), statistics.median(s_s)
        data = n_slots * n_cells * CELL
        out["mode%d" % mode] = {"build_s": round(b, 4), "scrub_s": round(s, 4), "build_GBps": round(data / b / 1e9, 2),
                                "scrub_GBps": round(data / s / 1e9, 2), "scrub_over_build_rate": round(b / s, 3), "granularity": gr}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--slot-mib", type=int, default=8)
    ap.add_argument("--big-slots", type=int, default=16)
    ap.add_argument("--big-gib", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the slot files go (default: a temporary directory, removed at the end)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = g.load_package()
    ctx = pkg.Context(0)
    d = tempfile.mkdtemp(prefix="scrub_rate_", dir=a.dir)
    record = {"repeats": a.repeats}
    try:
        if a.slots:
            cells = (a.slot_mib << 20) // CELL
            base = os.path.join(d, "small_")
            write_files(base, a.slots, cells * CELL)
            record["small"] = dict(workload="%d slot files x %d MiB (2^%d cells x 2048 B), page cache" % (a.slots, a.slot_mib, cells.bit_length() - 1),
                                   **leg(pkg, ctx, base, a.slots, cells, (1, 2), a.repeats))
            shutil.rmtree(d)
            os.makedirs(d)
        if a.big_slots:
            cells = (a.big_gib << 30) // CELL
            base = os.path.join(d, "large_")
            write_files(base, a.big_slots, cells * CELL)
            record["large"] = dict(workload="%d slot files x %d GiB (2^%d cells x 2048 B), page cache" % (a.big_slots, a.big_gib, cells.bit_length() - 1),
                                   **leg(pkg, ctx, base, a.big_slots, cells, (2,), a.repeats))
    finally:
        shutil.rmtree(d, ignore_errors=True)
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/scrub_rate.py on one MI355X (%s; medians of alternated build / scrub rounds after a warm-up):\n%s\n" %
                    (" ".join(sys.argv[1:]) or "defaults", line))


if __name__ == "__main__":
    main()
