"""Rate of cp2_datasets_scrub_many against the loop over cp2_dataset_scrub it replaces and against one dataset holding the same slots.

Data (defaults = the storage node's shape): --slots 4096 slot files of --slot-mib 8 MiB (2^12 cells x 2048 B, 64 KiB blocks), written
once and so in the page cache; every dataset built compact (keep-trees mode 2).  Legs, timed in one process over the same files:
  (a) loop    cp2_dataset_scrub of each of the 4096 one-slot datasets (first_slot = k, n_local = 1), one call after the other
  (b) many    one cp2_datasets_scrub_many over the same 4096 datasets
  (c) single  one cp2_dataset_scrub of a single dataset whose 4096 local slots are those files
A warm-up round first ((a) over the first --warm-loop datasets only: it warms the same code and pools), then --repeats rounds of (a),
(b), (c) alternated; medians.  (a) and (c) are the yardsticks; (b) moves the same bytes through the same kernels in the same turns as
(c) plus one address table per batch, so it is expected within 10 % of (c) plus the spread (c) shows between its rounds; (a) / (b) is
recorded as measured, with b_clearly_beats_a = every round of (b) took at most half of every round of (a).  One more (b) runs at the
end, untimed, with CP2_TRACE set: its account of where the time went (the call's own line and the first batches' turn lines) goes into
the record as b_trace.  Prints one JSON line and, with --out, writes it with a heading.

    python tools/scrub_many_rate.py [--slots 4096] [--slot-mib 8] [--repeats 2] [--warm-loop 256] [--dir D] [--out FILE]
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
    """n_slots files of slot_bytes each, from one random pattern (hashing cost does not depend on the bytes), as tools/scrub_rate.py"""
    pat = np.random.default_rng(7).integers(0, 256, min(slot_bytes, 64 << 20), dtype=np.uint8).tobytes()
    for k in range(n_slots):
        with open("%s%d.dat" % (base, k), "wb") as f:
            left = slot_bytes
            while left:
                n = min(left, len(pat))
                f.write(pat[:n])
                left -= n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--slot-mib", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--warm-loop", type=int, default=256)
    ap.add_argument("--dir", default=None, help="where the slot files go (default: a temporary directory, removed at the end)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = g.load_package()
    ctx = pkg.Context(0)
    d = tempfile.mkdtemp(prefix="scrub_many_rate_", dir=a.dir)
    n, cells = a.slots, (a.slot_mib << 20) // CELL
    data = n * cells * CELL
    try:
        base = os.path.join(d, "slot_")
        write_files(base, n, cells * CELL)
        cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (n - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=n, nCells=cells,
                              nSamples=100, seed=1, file=base)
        ctx.set_keep_trees(2)
        t = time.perf_counter()
        ones = [ctx.dataset(cfg, first_slot=k, n_local=1) for k in range(n)]
        build_ones_s = time.perf_counter() - t
        t = time.perf_counter()
        whole = ctx.dataset(cfg)
        build_whole_s = time.perf_counter() - t
        ctx.set_keep_trees(-1)

        def loop(datasets):
            ctx.sync()
            t = time.perf_counter()
            bad = sum(ds.scrub(cap=16)[2] for ds in datasets)
            return time.perf_counter() - t, bad

        def many():
            ctx.sync()
            t = time.perf_counter()
            bad = ctx.scrub_many(ones, cap=16)[3]
            return time.perf_counter() - t, bad

        def single():
            ctx.sync()
            t = time.perf_counter()
            bad = whole.scrub(cap=16)[2]
            return time.perf_counter() - t, bad

        for f in (lambda: loop(ones[:max(1, min(n, a.warm_loop))]), many, single):     # warm-up
            assert f()[1] == 0
        rounds = {"loop": [], "many": [], "single": []}
        for _ in range(a.repeats):
            for name, f in (("loop", lambda: loop(ones)), ("many", many), ("single", single)):
                s, bad = f()
                assert bad == 0, (name, bad)
                rounds[name].append(s)
        med = {k: statistics.median(v) for k, v in rounds.items()}
        spread_c = (max(rounds["single"]) - min(rounds["single"])) / med["single"]
        margin = 0.10 + spread_c
        record = {
            "workload": "%d slot files x %d MiB (2^%d cells x 2048 B, 64 KiB blocks), page cache, compact datasets" % (n, a.slot_mib, cells.bit_length() - 1),
            "repeats": a.repeats,
            "build_one_slot_datasets_s": round(build_ones_s, 3), "build_single_dataset_s": round(build_whole_s, 3),
            "a_loop_s": round(med["loop"], 4), "b_many_s": round(med["many"], 4), "c_single_s": round(med["single"], 4),
            "a_loop_GBps": round(data / med["loop"] / 1e9, 2), "b_many_GBps": round(data / med["many"] / 1e9, 2),
            "c_single_GBps": round(data / med["single"] / 1e9, 2),
            "rounds_s": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
            "c_spread_between_rounds": round(spread_c, 3),
            "b_over_c_time": round(med["many"] / med["single"], 3), "b_within_margin_of_c": bool(med["many"] <= med["single"] * (1 + margin)),
            "margin": round(margin, 3),
            "a_over_b_time": round(med["loop"] / med["many"], 2),
            "b_clearly_beats_a": bool(max(rounds["many"]) * 2 <= min(rounds["loop"])),      # every round of (b) at most half of every round of (a)
        }
        # where (b)'s time goes: one more call, untimed, with CP2_TRACE set and the library's stderr caught in a file
        sys.stderr.flush()
        keep = os.dup(2)
        with tempfile.TemporaryFile() as tf:
            os.dup2(tf.fileno(), 2)
            os.environ["CP2_TRACE"] = "1"
            try:
                many()
            finally:
                del os.environ["CP2_TRACE"]
                os.dup2(keep, 2)
                os.close(keep)
            tf.seek(0)
            trace = [ln.strip() for ln in tf.read().decode(errors="replace").splitlines() if "[cp2 trace]" in ln]
        slot_lines = [ln for ln in trace if "slot files:" in ln and "turn(s)" in ln]
        record["b_trace"] = [ln for ln in trace if "scrub many:" in ln] + slot_lines[:4]
        record["b_trace_lines_in_all"] = len(trace)
        for ds in ones:
            ds.free()
        whole.free()
    finally:
        shutil.rmtree(d, ignore_errors=True)
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/scrub_many_rate.py on one MI355X (%s; medians of alternated loop / many / single rounds after a warm-up):\n%s\n" %
                    (" ".join(sys.argv[1:]) or "defaults", line))


if __name__ == "__main__":
    main()
