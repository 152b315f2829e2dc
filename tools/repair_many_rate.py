"""What cp2_datasets_repair_blocks_many costs against the one-dataset repair of the same bytes, and what the loop it replaces costs.

--datasets 4096 one-slot compact fake-source datasets of --slot-mib 1 MiB slots (16 blocks of 64 KiB, depth 4) on one context -- dataset k
holds slot k of one configuration, so the same slots also stand in ONE dataset of 4096 slots; each gets --per-slot 4 random blocks: 16 384
candidates, 1 GiB, check only, from pageable and from caller-pinned memory.  Legs:
  one        the yardstick: ONE cp2_dataset_repair_blocks (check only) over the single 4096-slot dataset, the same bytes in the same order
  many       one cp2_datasets_repair_blocks_many over the 4096 datasets, no paths
  loop       4096 cp2_dataset_repair_blocks calls over the same requests, dataset by dataset (recorded, one round, pinned)
  verify / many_paths   every request with its whole path: cp2_blocks_verify on the same bytes against the call (pinned)
  many_mix   every other request with its path, the rest without: the divergence of lanes that walk beside lanes that do not, against the two
             pure runs (pinned)
  write_1 / write_4 / write_16 / write_loop   --write-datasets 512 file-sourced one-slot datasets, their 4 blocks each written into
             page-cached slot files by the call on 1, 4 and 16 writer threads (cp2_set_ingest), against the per-dataset loop
In one process, after a warm-up of each leg, --repeats rounds of the legs alternated; medians, each leg's rounds printed.  Acceptance: the
median of `many` is at most 1.10 times the median of `one` plus the spread (max - min) of one's rounds, pageable and pinned; a miss is
printed as a miss.  Prints one JSON line and, with --out, writes it with a heading.

    python tools/repair_many_rate.py [--datasets 4096] [--slot-mib 1] [--per-slot 4] [--write-datasets 512] [--repeats 2] [--out profiles/repair_many_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

CELL, BLOCK = 2048, 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", type=int, default=4096)
    ap.add_argument("--slot-mib", type=int, default=1)
    ap.add_argument("--per-slot", type=int, default=4)
    ap.add_argument("--write-datasets", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as g
    import torch
    pkg = g.load_package()
    ctx = pkg.Context(0)
    S, W = a.datasets, min(a.write_datasets, a.datasets)
    n_cells, nb = (a.slot_mib << 20) // CELL, (a.slot_mib << 20) // BLOCK
    n = S * a.per_slot
    record = {"datasets": S, "blocks": n, "bytes": n * BLOCK, "repeats": a.repeats}

    def timed(f):
        ctx.sync()
        t = time.perf_counter()
        r = f()
        return time.perf_counter() - t, r

    def config(base=None):
        return pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (S - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=S, nCells=n_cells,
                               nSamples=100, seed=1, **({"file": base} if base else {}))

    try:
        big = config()
        ctx.set_keep_trees(2)
        try:
            one = ctx.dataset(big)
            sets = ctx.build_many([(big, k, 1) for k in range(S)])
        finally:
            ctx.set_keep_trees(-1)
        roots = one.local_roots()
        rng = np.random.default_rng(11)
        pairs = np.array([(s, b) for s in range(S) for b in sorted(rng.choice(nb, a.per_slot, replace=False))], dtype=np.uint64)
        by_slot = np.empty((n, BLOCK), dtype=np.uint8)
        slots = []
        for s in range(S):                                                              # the bytes slot by slot, then shuffled like the requests
            cells = np.ascontiguousarray(ctx.gen_fake_cells(ctx.slot_seed(1, s), 0, n_cells, CELL)).reshape(nb, BLOCK)
            if s < W:
                slots.append(cells.copy())
            by_slot[s * a.per_slot:(s + 1) * a.per_slot] = cells[pairs[s * a.per_slot:(s + 1) * a.per_slot, 1].astype(np.int64)]
        shuffle = rng.permutation(n)                                                    # the candidates arrive interleaved across the datasets
        pairs = np.ascontiguousarray(pairs[shuffle])
        cand = np.ascontiguousarray(by_slot[shuffle])
        del by_slot
        _, paths = one.block_proofs(pairs)
        depth = int(paths.shape[1])
        req = np.ascontiguousarray(np.stack([pairs[:, 0], pairs[:, 0], pairs[:, 1]], axis=1))   # dataset k holds slot k
        order = np.argsort(pairs[:, 0], kind="stable")
        record.update(depth=depth, workload="%d one-slot compact fake-source datasets of %d MiB slots (%d blocks of 64 KiB, depth %d), %d random "
                      "blocks each, check only: %d blocks, %d MiB" % (S, a.slot_mib, nb, depth, a.per_slot, n, n * BLOCK >> 20))
        packed = np.ascontiguousarray(paths.reshape(-1, 32))
        off_all = (np.arange(n + 1, dtype=np.uint64) * depth)
        half = np.arange(n) % 2 == 0                                                   # every other request brings its path
        off_mix = np.concatenate([[0], np.cumsum(np.where(half, depth, 0))]).astype(np.uint64)
        packed_mix = np.ascontiguousarray(paths[half].reshape(-1, 32))

        def all_match(st):
            assert (st == 0).all()

        def leg_one(data):
            dt, (st, _) = timed(lambda: one.repair_blocks(pairs, data, check_only=True))
            all_match(st)
            return dt

        def leg_many(data, rows=None, off=None):
            dt, (st, _) = timed(lambda: ctx.repair_blocks_many(sets, req, data, rows, off, check_only=True))
            all_match(st)
            return dt

        def leg_verify(data):
            dt, (st, _) = timed(lambda: ctx.blocks_verify(CELL, BLOCK, n_cells, roots, pairs, data, paths, want_roots=False))
            all_match(st)
            return dt

        def leg_loop(data):
            rows = [order[k * a.per_slot:(k + 1) * a.per_slot] for k in range(S)]
            sub = [(np.ascontiguousarray(pairs[r]), np.ascontiguousarray(data[r])) for r in rows]
            ctx.sync()
            t = time.perf_counter()
            for ds, (sb, d) in zip(sets, sub):
                ds.repair_blocks(sb, d, check_only=True)
            return time.perf_counter() - t

        def rounds(legs, tag, blocks=n):
            times = {k: [] for k in legs}
            for f in legs.values():                                                    # warm-up
                f()
            for _ in range(a.repeats):
                for k, f in legs.items():
                    times[k].append(f())
            for k, v in times.items():
                record[k + tag + "_rounds_s"] = [round(x, 4) for x in v]
                record[k + tag + "_s"] = round(statistics.median(v), 4)
                record[k + tag + "_GBps"] = round(blocks * BLOCK / 1e9 / statistics.median(v), 2)
            return {k: statistics.median(v) for k, v in times.items()}, times

        pinned = torch.from_numpy(cand).pin_memory().numpy()
        for tag, data in (("", cand), ("_pin", pinned)):
            med, times = rounds({"one": lambda: leg_one(data), "many": lambda: leg_many(data)}, tag)
            spread = max(times["one"]) - min(times["one"])
            record["many_over_one" + tag] = round(med["many"] / med["one"], 3)
            record["one" + tag + "_spread_s"] = round(spread, 4)
            record["accepted" + tag] = bool(med["many"] <= 1.10 * med["one"] + spread)
        med, _ = rounds({"verify": lambda: leg_verify(pinned), "many_paths": lambda: leg_many(pinned, packed, off_all),
                         "many_mix": lambda: leg_many(pinned, packed_mix, off_mix)}, "_pin")
        record["many_paths_over_verify_pin"] = round(med["many_paths"] / med["verify"], 3)
        record["many_mix_over_mean_of_pure_pin"] = round(med["many_mix"] / ((record["many_pin_s"] + med["many_paths"]) / 2), 3)
        record["loop_pin_s"] = round(leg_loop(pinned), 4)
        record["loop_over_many_pin"] = round(record["loop_pin_s"] / record["many_pin_s"], 1)
        record["many_not_slower_than_loop"] = bool(record["many_pin_s"] <= record["loop_pin_s"])
        for ds in sets:
            ds.free()
        one.free()
        # ---- the writer: W file-sourced one-slot datasets, their blocks written into page-cached slot files ------------------------------------
        with tempfile.TemporaryDirectory() as d:
            base = os.path.join(d, "w_")
            for s in range(W):
                slots[s].tofile("%s%d.dat" % (base, s))
            filed = config(base)
            ctx.set_keep_trees(2)
            try:
                wsets = ctx.build_many([(filed, k, 1) for k in range(W)])
            finally:
                ctx.set_keep_trees(-1)
            mine = np.flatnonzero(pairs[:, 0] < W)
            wreq, wdata = np.ascontiguousarray(req[mine]), np.ascontiguousarray(pinned[mine])
            worder = np.argsort(wreq[:, 0], kind="stable")
            wsub = [(np.ascontiguousarray(wreq[r][:, 1:]), np.ascontiguousarray(wdata[r])) for r in np.split(worder, W)]

            def leg_write(threads):
                ctx.set_ingest(fill_threads=threads)
                dt, (st, w) = timed(lambda: ctx.repair_blocks_many(wsets, wreq, wdata))
                assert (st == 0).all() and w == len(mine)
                return dt

            def leg_write_loop():
                ctx.sync()
                t = time.perf_counter()
                for ds, (sb, dd) in zip(wsets, wsub):
                    ds.repair_blocks(sb, dd)
                return time.perf_counter() - t

            med, _ = rounds({"write_1": lambda: leg_write(1), "write_4": lambda: leg_write(4), "write_16": lambda: leg_write(16),
                             "write_loop": leg_write_loop}, "_pin", blocks=len(mine))
            ctx.set_ingest()
            record.update(write_datasets=W, write_blocks=int(len(mine)), write_loop_over_write_16=round(med["write_loop"] / med["write_16"], 1),
                          write_1_over_write_16=round(med["write_1"] / med["write_16"], 2))
            for ds in wsets:
                ds.free()
    finally:
        ctx.close()
    line = json.dumps(record)
    print(line)
    gates = ["gate%s: many %.4f s against 1.10 x %.4f s + %.4f s: %s" % (tag, record["many" + tag + "_s"], record["one" + tag + "_s"],
                                                                        record["one" + tag + "_spread_s"], "met" if record["accepted" + tag] else "MISSED")
             for tag in ("", "_pin")]
    print("\n".join(gates))
    if a.out:
        args = ["--datasets %d" % a.datasets, "--slot-mib %d" % a.slot_mib, "--per-slot %d" % a.per_slot, "--write-datasets %d" % a.write_datasets,
                "--repeats %d" % a.repeats]
        with open(a.out, "w") as f:
            f.write("tools/repair_many_rate.py on one MI355X (%s; medians of alternated rounds after a warm-up of each leg):\n%s\n%s\n"
                    % (" ".join(args), line, "\n".join(gates)))

if __name__ == "__main__":
    main()
