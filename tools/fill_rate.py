"""Rate of cp2_fill_add against cp2_blocks_verify over the same blocks, and the time of cp2_fill_finish against the cp2_dataset_build it replaces.

A fill session's add is verify's data path with one more store per proved block (k_block_path_commit writes the block root into layer 0
of the session's compact buffer), plus the host's bitmap.  The source is fake, so no file system is in any number.
  slots   --slots 128 fake slots of --slot-mib 8 MiB (2^12 cells x 2048 B, 64 KiB blocks: 128 blocks, depth 7), every block sent once:
          16 384 blocks, 1 GiB.  finish turns the full session into a compact dataset; build is cp2_dataset_build (compact) of the same slots.
  deep    the same number of blocks into a session over ONE fake slot of 2^--deep-log2 cells (2^22: 131 072 blocks, depth 17), where the
          walk is longest (the session stays incomplete: no finish)
In one process, after a warm-up of each leg, --repeats rounds of the legs alternated; pageable blocks and a pinned copy.  Every timed add
goes into a fresh session (begun outside the timing), so every block is NEW.  The paths are the ones the built dataset serves.
fill_over_verify = verify_s / fill_s.  Prints one JSON line and, with --out, writes it with a heading.

    python tools/fill_rate.py [--slots 128] [--slot-mib 8] [--deep-log2 22] [--repeats 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    ctx = pkg.Context(0)
    slot_bytes = a.slot_mib << 20
    n_cells, nb = slot_bytes // CELL, slot_bytes // BLOCK
    n_req = a.slots * nb
    record = {"repeats": a.repeats}

    def timed(f):
        ctx.sync()
        t = time.perf_counter()
        r = f()
        return time.perf_counter() - t, r

    def build(cfg):
        ctx.set_keep_trees(2)
        try:
            return ctx.dataset(cfg)
        finally:
            ctx.set_keep_trees(-1)

    def compare(cfg, geom, roots, reqs, paths, cand, pinned):
        """verify and fill alternated, pageable and pinned; every block is right and new, so every status is 0"""
        def fill(data):
            f = ctx.fill(cfg, roots)                              # (begin and free are outside the timing)
            ctx.sync()
            t = time.perf_counter()
            st, n_new = f.add(reqs, data, paths)
            dt = time.perf_counter() - t
            f.free()
            assert n_new == len(reqs)
            return dt, st

        times = {k: [] for k in ("verify", "fill", "verify_pin", "fill_pin")}
        legs = {
            "verify": lambda: timed(lambda: ctx.blocks_verify(*geom, roots, reqs, cand, paths, want_roots=False)[0]),
            "fill": lambda: fill(cand),
            "verify_pin": lambda: timed(lambda: ctx.blocks_verify(*geom, roots, reqs, pinned, paths, want_roots=False)[0]),
            "fill_pin": lambda: fill(pinned),
        }
        for k, f in legs.items():                                 # warm-up
            assert (f()[1] == 0).all(), k
        for _ in range(a.repeats):
            for k, f in legs.items():
                times[k].append(f()[0])
        med = {k: statistics.median(v) for k, v in times.items()}
        gb = cand.nbytes / 1e9
        out = {"depth": int(paths.shape[1]), "path_MiB": round(paths.nbytes / 2**20, 2)}
        out.update({k + "_s": round(v, 4) for k, v in med.items()})
        out.update({k + "_GBps": round(gb / v, 2) for k, v in med.items()})
        out["fill_over_verify"] = round(med["verify"] / med["fill"], 3)
        out["fill_pin_over_verify_pin"] = round(med["verify_pin"] / med["fill_pin"], 3)
        return out

    try:
        # ---- slots: every block of every fake slot, in (slot, block) order
        cfg = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (a.slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=a.slots,
                              nCells=n_cells, nSamples=100, seed=1)
        cand = np.concatenate([ctx.gen_fake_cells(ctx.slot_seed(1, s), 0, n_cells, CELL).reshape(-1) for s in range(a.slots)])
        pinned = torch.from_numpy(cand).pin_memory().numpy()
        reqs = np.array([(s, b) for s in range(a.slots) for b in range(nb)], dtype=np.uint64)
        ds = build(cfg)
        roots = ds.local_roots()
        _, paths = ds.block_proofs(reqs)
        ds.free()
        record["slots"] = {"workload": "%d fake slots x %d MiB (2^%d cells x 2048 B, 64 KiB blocks); %d blocks (%d MiB), each sent once" %
                           (a.slots, a.slot_mib, n_cells.bit_length() - 1, n_req, n_req * BLOCK >> 20)}
        record["slots"].update(compare(cfg, (CELL, BLOCK, n_cells), roots, reqs, paths, cand, pinned))

        # ---- finish against the rebuild it replaces
        def finish():
            f = ctx.fill(cfg, roots)
            assert f.add(reqs, pinned, paths)[1] == n_req
            dt, filled = timed(f.finish)
            same = filled.local_roots().tobytes() == roots.tobytes()
            filled.free()
            f.free()
            return dt, same

        def rebuild():
            dt, built = timed(lambda: build(cfg))
            same = built.local_roots().tobytes() == roots.tobytes()
            built.free()
            return dt, same

        times = {"finish": [], "build": []}
        for k, f in (("finish", finish), ("build", rebuild)):     # warm-up
            assert f()[1], k
        for _ in range(a.repeats):
            for k, f in (("finish", finish), ("build", rebuild)):
                times[k].append(f()[0])
        fin, bld = statistics.median(times["finish"]), statistics.median(times["build"])
        record["finish"] = {"slots": a.slots, "blocks_per_slot": nb, "layers_built": int(paths.shape[1]), "finish_s": round(fin, 5),
                            "build_compact_s": round(bld, 4), "build_over_finish": round(bld / fin, 1)}
        del pinned, cand
        # ---- deep: the first n_req blocks of one fake slot of 2^deep_log2 cells
        deep_cells = 1 << a.deep_log2
        dcfg = pkg.make_config(maxDepth=32, maxLog2NSlots=1, cellSize=CELL, blockSize=BLOCK, nSlots=1, nCells=deep_cells, nSamples=100, seed=1)
        ds = build(dcfg)
        n_deep = min(n_req, deep_cells // CPB)
        cand = ctx.gen_fake_cells(ctx.slot_seed(1, 0), 0, n_deep * CPB, CELL).reshape(-1)
        pinned = torch.from_numpy(cand).pin_memory().numpy()
        reqs = np.array([(0, b) for b in range(n_deep)], dtype=np.uint64)
        roots = ds.local_roots()
        _, paths = ds.block_proofs(reqs)
        ds.free()
        record["deep"] = {"workload": "a session over one fake slot of 2^%d cells x 2048 B (%d blocks); its first %d blocks (%d MiB)" %
                          (a.deep_log2, deep_cells // CPB, n_deep, n_deep * BLOCK >> 20)}
        record["deep"].update(compare(dcfg, (CELL, BLOCK, deep_cells), roots, reqs, paths, cand, pinned))
    finally:
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        args = ["--slots %d" % a.slots, "--slot-mib %d" % a.slot_mib, "--deep-log2 %d" % a.deep_log2, "--repeats %d" % a.repeats]
        with open(a.out, "w") as f:
            f.write("tools/fill_rate.py on one MI355X (%s; medians of alternated verify / fill / verify_pin / fill_pin rounds, and of alternated "
                    "finish / build rounds, after a warm-up):\n%s\n" % (" ".join(args), line))


if __name__ == "__main__":
    main()
