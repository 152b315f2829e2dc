"""What cp2_fills_add_many costs against the one-session add of the same bytes, and what the loop it replaces costs.

--sessions 4096 one-slot fake-source sessions of --slot-mib 1 MiB slots (16 blocks of 64 KiB, depth 4) on one context; each receives
--per-slot 4 random blocks with their whole paths in ONE cp2_fills_add_many: 16 384 blocks, 1 GiB, from pageable and from caller-pinned
memory.  The yardstick exists without the call: one cp2_fill_add of the same bytes and the same paths into ONE session whose 4096 local
slots are those slots (a slot's tree does not depend on which dataset it belongs to).  Legs, every timed leg into fresh sessions (begun,
and where it applies keeping turned on, outside the timing):
  one        the yardstick: one cp2_fill_add into the one session of 4096 local slots
  many       one cp2_fills_add_many over the 4096 sessions, levels == NULL
  loop       4096 cp2_fill_add calls over the same requests, session by session (recorded, one round)
  one_keep / many_keep   the same two with every session keeping nodes
  one_low / many_low     lowest anchors in --batches 16 batches across the sessions (the anchor queries and the packing of the paths are
             outside the timing), keeping sessions: cp2_fill_add_anchored into the one session against cp2_fills_add_many with levels
  files      the many-call into page-cached slot files, with the seconds its CP2_TRACE line says it spent writing (the writes are serial)
In one process, after a warm-up of each leg, --repeats rounds of the legs alternated; medians, each leg's rounds printed.  Acceptance: the
median of `many` is at most 1.10 times the median of `one` plus the spread (max - min) of one's rounds, pageable and pinned.  Prints one
JSON line and, with --out, writes it with a heading.

    python tools/fill_many_rate.py [--sessions 4096] [--slot-mib 1] [--per-slot 4] [--batches 16] [--repeats 2] [--out profiles/fill_many_rate.txt]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

CELL, BLOCK = 2048, 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--slot-mib", type=int, default=1)
    ap.add_argument("--per-slot", type=int, default=4)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as g
    import torch
    pkg = g.load_package()
    ctx = pkg.Context(0)
    S = a.sessions
    n_cells, nb = (a.slot_mib << 20) // CELL, (a.slot_mib << 20) // BLOCK
    n = S * a.per_slot
    record = {"sessions": S, "blocks": n, "bytes": n * BLOCK, "repeats": a.repeats}

    def timed(f):
        ctx.sync()
        t = time.perf_counter()
        r = f()
        return time.perf_counter() - t, r

    try:
        big = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (S - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=S, nCells=n_cells,
                              nSamples=100, seed=1)
        ctx.set_keep_trees(2)
        try:
            ds = ctx.dataset(big)
        finally:
            ctx.set_keep_trees(-1)
        roots = ds.local_roots()
        rng = np.random.default_rng(11)
        pairs = np.array([(s, b) for s in range(S) for b in sorted(rng.choice(nb, a.per_slot, replace=False))], dtype=np.uint64)
        by_slot = np.empty((n, BLOCK), dtype=np.uint8)
        for s in range(S):                                                              # the bytes slot by slot, then shuffled like the requests
            cells = np.ascontiguousarray(ctx.gen_fake_cells(ctx.slot_seed(1, s), 0, n_cells, CELL)).reshape(nb, BLOCK)
            by_slot[s * a.per_slot:(s + 1) * a.per_slot] = cells[pairs[s * a.per_slot:(s + 1) * a.per_slot, 1].astype(np.int64)]
        shuffle = rng.permutation(n)                                                    # arrivals interleaved across the sessions
        pairs = np.ascontiguousarray(pairs[shuffle])
        cand = np.ascontiguousarray(by_slot[shuffle])
        del by_slot
        _, paths = ds.block_proofs(pairs)
        depth = int(paths.shape[1])
        ds.free()
        order = np.argsort(pairs[:, 0], kind="stable")
        req = np.ascontiguousarray(np.stack([pairs[:, 0], np.zeros(n, np.uint64), pairs[:, 1]], axis=1))   # session k's one slot is its slot 0
        record.update(depth=depth, workload="%d one-slot fake-source sessions of %d MiB slots (%d blocks of 64 KiB, depth %d), %d random blocks each "
                      "with whole paths: %d blocks, %d MiB" % (S, a.slot_mib, nb, depth, a.per_slot, n, n * BLOCK >> 20))
        one_cfg = lambda base=None: pkg.make_config(maxDepth=32, maxLog2NSlots=1, cellSize=CELL, blockSize=BLOCK, nSlots=1, nCells=n_cells,   # noqa: E731
                                                    nSamples=100, seed=1, **({"file": base} if base else {}))
        small = one_cfg()

        def sessions(keep=False, directory=None):
            out = []
            for k in range(S):
                f = ctx.fill(one_cfg(os.path.join(directory, "d%d_" % k)) if directory else small, roots[k:k + 1], 0, 1)
                if keep:
                    f.keep_nodes()
                out.append(f)
            return out

        def one_session(keep=False):
            f = ctx.fill(big, roots)
            if keep:
                f.keep_nodes()
            return f

        def free(fs):
            for f in fs:
                f.free()

        def leg_one(data, keep=False):
            f = one_session(keep)
            dt, (st, new) = timed(lambda: f.add(pairs, data, paths))
            f.free()
            assert new == n and (st == 0).all()
            return dt

        def leg_many(data, keep=False, directory=None):
            fs = sessions(keep, directory)
            dt, (st, new) = timed(lambda: pkg.fills_add_many(ctx, fs, req, data, paths.reshape(-1, 32)))
            free(fs)
            assert sum(new) == n and (st == 0).all()
            return dt

        def leg_loop(data):
            fs = sessions()
            rows = [order[k * a.per_slot:(k + 1) * a.per_slot] for k in range(S)]
            sub = [(np.ascontiguousarray(req[r][:, 1:]), np.ascontiguousarray(data[r]), np.ascontiguousarray(paths[r])) for r in rows]
            ctx.sync()
            t = time.perf_counter()
            for f, (sb, d, p) in zip(fs, sub):
                f.add(sb, d, p)
            dt = time.perf_counter() - t
            free(fs)
            return dt

        per = (n + a.batches - 1) // a.batches

        def leg_one_low(data):
            f = one_session(True)
            total = 0.0
            for c0 in range(0, n, per):
                sb = pairs[c0:c0 + per]
                lv = f.anchors(sb)
                packed = np.concatenate([paths[c0 + i][:int(x)] for i, x in enumerate(lv)] + [np.zeros((0, 32), np.uint8)])
                dt, (st, new) = timed(lambda: f.add_anchored(sb, data[c0:c0 + per], lv, packed))
                total += dt
                assert new == len(sb)
            f.free()
            return total

        def leg_many_low(data):
            fs = sessions(True)
            total, siblings = 0.0, 0
            for c0 in range(0, n, per):
                rq = req[c0:c0 + per]

                def anchors():
                    return np.array([int(fs[int(k)].anchors([(0, int(b))])[0]) for k, _, b in rq], dtype=np.uint32)
                lv = anchors()
                packed = np.concatenate([paths[c0 + i][:int(x)] for i, x in enumerate(lv)] + [np.zeros((0, 32), np.uint8)])
                dt, (st, new) = timed(lambda: pkg.fills_add_many(ctx, fs, rq, data[c0:c0 + per], packed if packed.size else None, lv))
                total += dt
                siblings += int(lv.sum())
                assert sum(new) == len(rq)
            free(fs)
            record["many_low_siblings"] = siblings
            return total

        def rounds(legs, tag):
            times = {k: [] for k in legs}
            for f in legs.values():                                                    # warm-up
                f()
            for _ in range(a.repeats):
                for k, f in legs.items():
                    times[k].append(f())
            for k, v in times.items():
                record[k + tag + "_rounds_s"] = [round(x, 4) for x in v]
                record[k + tag + "_s"] = round(statistics.median(v), 4)
                record[k + tag + "_GBps"] = round(n * BLOCK / 1e9 / statistics.median(v), 2)
            return {k: statistics.median(v) for k, v in times.items()}, times

        pinned = torch.from_numpy(cand).pin_memory().numpy()
        for tag, data in (("", cand), ("_pin", pinned)):
            med, times = rounds({"one": lambda: leg_one(data), "many": lambda: leg_many(data)}, tag)
            spread = max(times["one"]) - min(times["one"])
            record["many_over_one" + tag] = round(med["many"] / med["one"], 3)
            record["one" + tag + "_spread_s"] = round(spread, 4)
            record["accepted" + tag] = bool(med["many"] <= 1.10 * med["one"] + spread)
        med, _ = rounds({"one_keep": lambda: leg_one(pinned, True), "many_keep": lambda: leg_many(pinned, True)}, "_pin")
        record["many_keep_over_one_keep_pin"] = round(med["many_keep"] / med["one_keep"], 3)
        med, _ = rounds({"one_low": lambda: leg_one_low(pinned), "many_low": lambda: leg_many_low(pinned)}, "_pin")
        record["many_low_over_one_low_pin"] = round(med["many_low"] / med["one_low"], 3)
        record["loop_pin_s"] = round(leg_loop(pinned), 4)
        record["loop_over_many_pin"] = round(record["loop_pin_s"] / record["many_pin_s"], 1)
        # page-cached slot files: the call's own trace line says how long it wrote
        with tempfile.TemporaryDirectory() as d:
            log = os.path.join(d, "trace.txt")
            saved, fd = os.dup(2), os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
            os.environ["CP2_TRACE"] = "1"
            try:
                os.dup2(fd, 2)
                files_s = leg_many(pinned, directory=d)
            finally:
                os.dup2(saved, 2)
                os.close(fd)
                os.close(saved)
                del os.environ["CP2_TRACE"]
            m = re.findall(r"fills add many: .* ([0-9.]+) s writing", open(log).read())
            record.update(files_pin_s=round(files_s, 4), files_writing_s=float(m[-1]) if m else None,
                          files_device_pass_s=round(files_s - float(m[-1]), 4) if m else None)
    finally:
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        args = ["--sessions %d" % a.sessions, "--slot-mib %d" % a.slot_mib, "--per-slot %d" % a.per_slot, "--batches %d" % a.batches,
                "--repeats %d" % a.repeats]
        with open(a.out, "w") as f:
            f.write("tools/fill_many_rate.py on one MI355X (%s; medians of alternated rounds after a warm-up of each leg):\n%s\n" % (" ".join(args), line))


if __name__ == "__main__":
    main()
