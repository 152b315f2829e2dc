"""Rate of cp2_datasets_build_many against the loop over cp2_dataset_build it replaces and against one dataset holding the same slots.

Data (defaults = the storage node's shape, profiles/scrub_many_rate.txt's): --slots 4096 slot files of --slot-mib 8 MiB (2^12 cells x 2048
B, 64 KiB blocks), written once and so in the page cache; every dataset built compact (keep-trees mode 2).  Legs, timed in one process
over the same files, every leg's datasets freed outside the timed part:
  (a) loop    cp2_dataset_build of each of the 4096 one-slot requests (first_slot = k, n_local = 1), one call after the other
  (b) many    one cp2_datasets_build_many of the same 4096 requests
  (c) single  one cp2_dataset_build of a single dataset whose 4096 local slots are those files
A warm-up of the three legs first ((a) over the first --warm-loop requests only: it warms the same code and pools), then --repeats
rounds of (a), (b), (c) alternated; medians.  (a) and (c) are the yardsticks.  (b) moves the same bytes through the same kernels in the
same turns as (c); beyond (c) it makes 4096 dataset objects and their share of a few allocations, so it is DONE when
(b) <= (1 + 0.10 + the relative spread of (c)'s rounds) x (c), the margin tools/scrub_many_rate.py uses for the same comparison; (a) / (b)
is recorded as measured.  Also timed, with no threshold: (b) keeping the roots only (mode 0) and every node (mode 1), and the loop of 4096
cp2_dataset_set_roots calls a node makes after the build (not batched by this call).  The roots of (b) must equal those of (c) slot for
slot: asserted.  One more (b) runs at the end, untimed, with CP2_TRACE set: the call's own lines (the pass, and the allocation of the
dataset objects against it) and the first batches' turn lines go into the record as b_trace.  Prints one JSON line and, with --out,
writes it with a heading.

    python tools/build_many_rate.py [--slots 4096] [--slot-mib 8] [--repeats 2] [--warm-loop 256] [--dir D] [--out FILE]
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
    """n_slots files of slot_bytes each, from one random pattern shifted by the slot number (so that the slots' roots differ)"""
    pat = np.random.default_rng(7).integers(0, 256, min(slot_bytes, 64 << 20) + n_slots, dtype=np.uint8).tobytes()
    for k in range(n_slots):
        with open("%s%d.dat" % (base, k), "wb") as f:
            left = slot_bytes
            while left:
                n = min(left, len(pat) - n_slots)
                f.write(pat[k:k + n])
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
    d = tempfile.mkdtemp(prefix="build_many_rate_", dir=a.dir)
    n, cells = a.slots, (a.slot_mib << 20) // CELL
    data = n * cells * CELL
    try:
        base = os.path.join(d, "slot_")
        write_files(base, n, cells * CELL)
        cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (n - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=n, nCells=cells,
                              nSamples=100, seed=1, file=base)
        requests = [(cfg, k, 1) for k in range(n)]

        def timed(build, mode=2):
            """(seconds, the datasets) of one leg under a named kept mode"""
            ctx.set_keep_trees(mode)
            try:
                ctx.sync()
                t = time.perf_counter()
                out = build()
                return time.perf_counter() - t, out
            finally:
                ctx.set_keep_trees(-1)

        def free(datasets):
            for ds in datasets:
                ds.free()

        legs = (("loop", lambda k=n: [ctx.dataset(cfg, first_slot=i, n_local=1) for i in range(k)]),
                ("many", lambda: ctx.build_many(requests)),
                ("single", lambda: [ctx.dataset(cfg)]))
        free(timed(lambda: legs[0][1](max(1, min(n, a.warm_loop))))[1])            # warm-up
        for name, f in legs[1:]:
            free(timed(f)[1])
        rounds = {"loop": [], "many": [], "single": []}
        for _ in range(a.repeats):
            for name, f in legs:
                s, out = timed(f)
                assert all(ds.tree_mode == 2 for ds in out[:4])
                rounds[name].append(s)
                free(out)
        med = {k: statistics.median(v) for k, v in rounds.items()}
        spread_c = (max(rounds["single"]) - min(rounds["single"])) / med["single"]
        margin = 0.10 + spread_c
        record = {
            "workload": "%d slot files x %d MiB (2^%d cells x 2048 B, 64 KiB blocks), page cache, compact datasets; one box's figures" % (n, a.slot_mib, cells.bit_length() - 1),
            "repeats": a.repeats,
            "a_loop_s": round(med["loop"], 4), "b_many_s": round(med["many"], 4), "c_single_s": round(med["single"], 4),
            "a_loop_GBps": round(data / med["loop"] / 1e9, 2), "b_many_GBps": round(data / med["many"] / 1e9, 2),
            "c_single_GBps": round(data / med["single"] / 1e9, 2),
            "rounds_s": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
            "c_spread_between_rounds": round(spread_c, 3),
            "b_over_c_time": round(med["many"] / med["single"], 3), "b_within_margin_of_c": bool(med["many"] <= med["single"] * (1 + margin)),
            "margin": round(margin, 3),
            "a_over_b_time": round(med["loop"] / med["many"], 2),
            "a_ms_per_dataset": round(med["loop"] / n * 1e3, 3), "b_ms_per_dataset": round(med["many"] / n * 1e3, 4),
        }
        # the other two modes, no threshold
        for mode, key in ((0, "b_many_roots_only_s"), (1, "b_many_every_node_s")):
            s, out = timed(legs[1][1], mode)
            assert all(ds.tree_mode == mode for ds in out[:4])
            record[key] = round(s, 4)
            free(out)
        # (b)'s roots against (c)'s, slot for slot; then what a node still does per dataset after the build: cp2_dataset_set_roots
        _, whole = timed(legs[2][1])
        _, many = timed(legs[1][1])
        all_roots = whole[0].local_roots()
        got = np.concatenate([ds.local_roots() for ds in many])
        assert got.shape == all_roots.shape and np.array_equal(got, all_roots), "the roots of (b) differ from those of (c)"
        assert len({bytes(r) for r in all_roots}) == n
        record["b_roots_equal_c"] = True
        ctx.sync()
        t = time.perf_counter()
        for ds in many:
            ds.set_roots(all_roots)
        record["set_roots_loop_s"] = round(time.perf_counter() - t, 4)
        record["set_roots_ms_per_dataset"] = round(record["set_roots_loop_s"] / n * 1e3, 4)
        assert np.array_equal(many[n // 2].root(), whole[0].root())
        free(many + whole)
        # where (b)'s time goes: one more call, untimed, with CP2_TRACE set and the library's stderr caught in a file
        sys.stderr.flush()
        keep = os.dup(2)
        with tempfile.TemporaryFile() as tf:
            os.dup2(tf.fileno(), 2)
            os.environ["CP2_TRACE"] = "1"
            try:
                free(timed(legs[1][1])[1])
            finally:
                del os.environ["CP2_TRACE"]
                os.dup2(keep, 2)
                os.close(keep)
            tf.seek(0)
            trace = [ln.strip() for ln in tf.read().decode(errors="replace").splitlines() if "[cp2 trace]" in ln]
        slot_lines = [ln for ln in trace if "slot files:" in ln and "turn(s)" in ln]
        record["b_trace"] = [ln for ln in trace if "build many:" in ln] + slot_lines[:4]
        record["b_trace_lines_in_all"] = len(trace)
    finally:
        shutil.rmtree(d, ignore_errors=True)
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/build_many_rate.py on one MI355X (%s; one box's figures; medians of alternated loop / many / single rounds after a warm-up):\n%s\n" %
                    (" ".join(sys.argv[1:]) or "defaults", line))
    if not record["b_within_margin_of_c"]:
        sys.exit("(b) %.4f s is not within %.3f of (c) %.4f s" % (record["b_many_s"], record["margin"], record["c_single_s"]))


if __name__ == "__main__":
    main()
