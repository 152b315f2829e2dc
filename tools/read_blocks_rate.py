"""Rate of the verified read-back (cp2_datasets_read_blocks / cp2_dataset_read_blocks) against what it is made of and what it replaces.

  check   every block of --slots 128 page-cached slot files of --slot-mib 8 MiB (2^12 cells x 2048 B, 64 KiB blocks: 16 384 blocks, 1 GiB)
          in one check-only call with data == NULL, against cp2_dataset_scrub over the same files (compact) and against check-only
          cp2_dataset_repair_blocks on the same bytes already in memory: what the reads cost and whether they hide behind the hashing
  serve   the same requests with data returned, pageable and caller-pinned, against the unverified alternative: cp2_dataset_block_proofs
          plus a plain pread loop here: the price of the check
  spot    --many 4096 one-slot compact datasets of --many-slot-mib 1 MiB, --per 4 random blocks each, in one cp2_datasets_read_blocks call
          against the loop of cp2_dataset_read_blocks calls, one per dataset
In one process, after a warm-up of each leg, --repeats rounds of the legs alternated; medians.  Prints one JSON line and, with --out, writes
it with a heading.

    python tools/read_blocks_rate.py [--slots 128] [--slot-mib 8] [--many 4096] [--many-slot-mib 1] [--per 4] [--repeats 2] [--dir D] [--out FILE]
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
    ap.add_argument("--many", type=int, default=4096)
    ap.add_argument("--many-slot-mib", type=int, default=1)
    ap.add_argument("--per", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the slot files go (default: a temporary directory, removed at the end)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    ctx = pkg.Context(0)
    d = tempfile.mkdtemp(prefix="read_blocks_rate_", dir=a.dir)
    record = {"repeats": a.repeats}

    def timed(f):
        ctx.sync()
        t = time.perf_counter()
        r = f()
        return time.perf_counter() - t, r

    def rounds(legs, check):
        times = {k: [] for k in legs}
        for k, f in legs.items():                                     # warm-up
            check(k, timed(f)[1])
        for _ in range(a.repeats):
            for k, f in legs.items():
                times[k].append(timed(f)[0])
        return {k: statistics.median(v) for k, v in times.items()}, times

    def build(cfg):
        ctx.set_keep_trees(2)
        try:
            return ctx.dataset(cfg)
        finally:
            ctx.set_keep_trees(-1)

    try:
        # ---- check and serve: every block of every slot file, in shuffled order
        slot_bytes = a.slot_mib << 20
        n_cells, nb = slot_bytes // CELL, slot_bytes // BLOCK
        base = os.path.join(d, "slot_")
        rng = np.random.default_rng(7)
        parts = []
        for k in range(a.slots):
            b = rng.integers(0, 256, slot_bytes, dtype=np.uint8)
            b.tofile("%s%d.dat" % (base, k))
            parts.append(b)
        whole = np.concatenate(parts).reshape(a.slots * nb, BLOCK)
        del parts
        order = rng.permutation(a.slots * nb)
        reqs = np.array([(i // nb, i % nb) for i in order], dtype=np.uint64)
        cand = np.ascontiguousarray(whole[order])
        del whole
        n = reqs.shape[0]
        gb = n * BLOCK / 1e9
        ds = build(pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (a.slots - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=a.slots,
                                   nCells=n_cells, nSamples=100, seed=1, file=base))
        pinned_out = torch.empty((n, BLOCK), dtype=torch.uint8).pin_memory().numpy()
        pageable_out = np.empty((n, BLOCK), dtype=np.uint8)

        def plain():
            roots, paths = ds.block_proofs(reqs)
            fds = {}
            for i in range(n):
                s, b = int(reqs[i, 0]), int(reqs[i, 1])
                if s not in fds:
                    fds[s] = os.open("%s%d.dat" % (base, s), os.O_RDONLY)
                pageable_out[i] = np.frombuffer(os.pread(fds[s], BLOCK, b * BLOCK), dtype=np.uint8)
            for fd in fds.values():
                os.close(fd)
            return None

        legs = {
            "check_null": lambda: ds.read_blocks(reqs, check_only=True, want_data=False)[4],
            "scrub": lambda: n - ds.scrub()[2],
            "repair_check": lambda: int((ds.repair_blocks(reqs, cand, check_only=True)[0] == 0).sum()),
            "read_pageable": lambda: ds.read_blocks(reqs, data=pageable_out)[4],
            "read_pinned": lambda: ds.read_blocks(reqs, data=pinned_out)[4],
            "proofs_plus_pread": plain,
        }

        def all_ok(k, r):
            assert r is None or r == n, (k, r)

        med, times = rounds(legs, all_ok)
        assert np.array_equal(pinned_out, cand) and np.array_equal(pageable_out, cand)
        rec = {"workload": "%d slot files x %d MiB (2^%d cells x 2048 B, 64 KiB blocks), page cache, compact dataset; all %d blocks (%d MiB) in shuffled order" %
               (a.slots, a.slot_mib, n_cells.bit_length() - 1, n, n * BLOCK >> 20)}
        rec.update({k + "_s": round(v, 4) for k, v in med.items()})
        rec.update({k + "_GBps": round(gb / v, 2) for k, v in med.items()})
        rec["rounds_s"] = {k: [round(x, 4) for x in v] for k, v in times.items()}
        rec["check_null_over_scrub_time"] = round(med["check_null"] / med["scrub"], 3)
        rec["check_null_over_repair_check_time"] = round(med["check_null"] / med["repair_check"], 3)
        rec["read_pageable_over_plain_time"] = round(med["read_pageable"] / med["proofs_plus_pread"], 3)
        rec["read_pinned_over_plain_time"] = round(med["read_pinned"] / med["proofs_plus_pread"], 3)
        record["files"] = rec
        ds.free()
        del cand, pinned_out, pageable_out
        # ---- spot: a few random blocks of each of many one-slot datasets
        mb = a.many_slot_mib << 20
        m_cells, m_nb = mb // CELL, mb // BLOCK
        seedbuf = rng.integers(0, 256, mb + a.many, dtype=np.uint8)
        t0 = time.perf_counter()
        sets = []
        for k in range(a.many):
            mbase = os.path.join(d, "m%d_" % k)
            seedbuf[k:k + mb].tofile(mbase + "0.dat")
            sets.append(build(pkg.make_config(maxDepth=32, maxLog2NSlots=1, cellSize=CELL, blockSize=BLOCK, nSlots=1, nCells=m_cells, nSamples=100, seed=1,
                                              file=mbase)))
        build_s = time.perf_counter() - t0
        blocks = rng.integers(0, m_nb, (a.many, a.per))
        many_reqs = np.array([(k, 0, int(b)) for k in range(a.many) for b in blocks[k]], dtype=np.uint64)
        per_ds = [np.array([(0, int(b)) for b in blocks[k]], dtype=np.uint64) for k in range(a.many)]
        total = a.many * a.per

        def loop():
            return sum(sets[k].read_blocks(per_ds[k], check_only=True, want_data=False)[4] for k in range(a.many))

        legs = {"loop": loop, "one_call": lambda: ctx.read_blocks(sets, many_reqs, check_only=True, want_data=False)[5]}

        def all_ok2(k, r):
            assert r == total, (k, r)

        med, times = rounds(legs, all_ok2)
        record["spot"] = {"workload": "%d one-slot compact datasets over page-cached slot files of %d MiB, %d random blocks of each (%d blocks, %d MiB), check only" %
                          (a.many, a.many_slot_mib, a.per, total, total * BLOCK >> 20),
                          "build_datasets_s": round(build_s, 2), "loop_s": round(med["loop"], 4), "one_call_s": round(med["one_call"], 4),
                          "loop_ms_per_dataset": round(med["loop"] / a.many * 1e3, 3), "one_call_GBps": round(total * BLOCK / 1e9 / med["one_call"], 2),
                          "loop_over_one_call_time": round(med["loop"] / med["one_call"], 2),
                          "rounds_s": {k: [round(x, 4) for x in v] for k, v in times.items()}}
        for s in sets:
            s.free()
    finally:
        shutil.rmtree(d, ignore_errors=True)
        ctx.close()
    line = json.dumps(record)
    print(line)
    if a.out:
        # the heading names the workload's arguments only: where the files and the record went is not part of the measurement
        args = ["--slots %d" % a.slots, "--slot-mib %d" % a.slot_mib, "--many %d" % a.many, "--many-slot-mib %d" % a.many_slot_mib, "--per %d" % a.per,
                "--repeats %d" % a.repeats]
        with open(a.out, "w") as f:
            f.write("tools/read_blocks_rate.py on one MI355X (%s; medians of alternated rounds after a warm-up of each leg):\n%s\n" % (" ".join(args), line))


if __name__ == "__main__":
    main()
