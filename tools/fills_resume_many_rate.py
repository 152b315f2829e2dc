"""What cp2_fills_resume_many costs: against the yardstick of its data path, against the loop of cp2_fill_resume it replaces, and against
cp2_dataset_scrub over the same files.

Per leg (--legs small,large) on one MI355X in one process: --sessions one-slot file-sourced sessions of --slot-mib MiB slots (64 KiB
blocks, 2 KiB cells), every block present, the files page-cached (written moments before).  The slot files are written once from fake
cells; the 4096-slot dataset that is scrubbed and the one-slot sessions name the same files (hard links), and the checkpoints are
written from the documented layout (tests/fill_resume_models.py) with the block roots that dataset keeps.  A warm-up of every timed call,
then --repeats rounds alternated; medians, every round printed so the spread shows.

  many        one cp2_fills_resume_many with the re-check          many_trust   the same with CP2_RESUME_TRUST_FILES
  loop        one cp2_fill_resume per session, with the re-check   loop_trust   the same trusting the files
  yardstick   check-only, no-data cp2_datasets_read_blocks over the same blocks through one compact dataset per session: the same
              reader and the same data path
  scrub       cp2_dataset_scrub of ONE dataset of all the slots over the same files (recorded: GB/s)
GATE: many <= 1.10 x yardstick + the yardstick's spread between its rounds (the margin is what the call adds: checkpoint reads, session
opens, the layer-0 upload).  REQUIRED: many <= loop and many_trust <= loop_trust; both ratios are recorded.  The call's own CP2_TRACE line
gives its split: checkpoints, opens and uploads, re-check, host drops.  Prints one JSON line per leg and, with --out, writes them with a
heading.

    python tools/fills_resume_many_rate.py --dir DIR [--legs small,large] [--repeats 2] [--out profiles/fills_resume_many_rate.txt]
"""
import argparse
import json
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import fill_resume_models as M  # noqa: E402  (the checkpoint's documented layout, written without the library)

CELL, BLOCK = 2048, 65536
CPB = BLOCK // CELL


def traced(f):
    """f() with CP2_TRACE set and stderr in a file: (f's result, the text)"""
    with tempfile.TemporaryDirectory() as d:
        log = os.path.join(d, "trace.txt")
        saved, fd = os.dup(2), os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        os.environ["CP2_TRACE"] = "1"
        try:
            os.dup2(fd, 2)
            out = f()
        finally:
            os.dup2(saved, 2)
            os.close(fd)
            os.close(saved)
            del os.environ["CP2_TRACE"]
        return out, open(log).read()


def leg(pkg, ctx, a, name, S, slot_mib):
    d = os.path.join(a.dir, name)
    os.makedirs(d)
    n_cells = (slot_mib << 20) // CELL
    nb = n_cells // CPB
    geom = dict(maxDepth=32, cellSize=CELL, blockSize=BLOCK, nCells=n_cells, nSamples=100, seed=1)

    def timed(f):
        ctx.sync()
        t = time.perf_counter()
        r = f()
        return time.perf_counter() - t, r

    def compact(f):
        ctx.set_keep_trees(2)
        try:
            return f()
        finally:
            ctx.set_keep_trees(-1)

    for s in range(S):                                               # one file, two names: slot s of the big dataset, slot 0 of session s
        cells = ctx.gen_fake_cells(ctx.slot_seed(1, s), 0, n_cells, CELL)
        np.ascontiguousarray(cells).tofile(os.path.join(d, "slot%d.dat" % s))
        os.link(os.path.join(d, "slot%d.dat" % s), os.path.join(d, "one%d_0.dat" % s))
    big = compact(lambda: ctx.dataset(pkg.make_config(file=os.path.join(d, "slot"), nSlots=S, maxLog2NSlots=max(1, (S - 1).bit_length()), **geom)))
    roots = big.local_roots().copy()
    pairs = np.array([(s, b) for s in range(S) for b in range(nb)], dtype=np.uint64)
    block_roots = big.block_proofs(pairs)[0].reshape(S, nb, 32)
    cfgs = [pkg.make_config(file=os.path.join(d, "one%d_" % s), nSlots=1, maxLog2NSlots=1, **geom) for s in range(S)]
    paths = [os.path.join(d, "session%d.ckpt" % s) for s in range(S)]
    for s in range(S):
        c = dict(cell_size=CELL, block_size=BLOCK, n_cells=n_cells, n_slots=1, first_slot=0, n_local=1, source=M.SRC_FILE, seed=1, n_blocks=nb,
                 file_base=os.fsencode(os.path.join(d, "one%d_" % s)), roots=roots[s:s + 1], bits=[1] * nb, layer0=block_roots[s])
        open(paths[s], "wb").write(M.write_checkpoint(c))
    one_roots = [roots[s:s + 1] for s in range(S)]
    dss = compact(lambda: ctx.build_many([(cfgs[s], 0, 1) for s in range(S)]))
    req = np.array([(s, 0, b) for s in range(S) for b in range(nb)], dtype=np.uint64)
    n = len(req)
    print("[%s] %d files, checkpoints and compact datasets are there" % (name, S), file=sys.stderr, flush=True)

    def free(hs):
        for h in hs:
            h.free()

    def many(trust):
        dt, (fs, dropped) = timed(lambda: pkg.fills_resume_many(ctx, cfgs, one_roots, paths, trust_files=trust))
        ok = int(dropped.sum()) == 0 and all(f.missing(0)[1] == 0 for f in fs[::max(1, S // 16)])
        free(fs)
        return dt, ok

    def loop(trust):
        dt, fs = timed(lambda: [ctx.fill_resume(cfgs[s], one_roots[s], paths[s], trust_files=trust) for s in range(S)])
        ok = all(f.n_dropped == 0 for f in fs) and all(f.missing(0)[1] == 0 for f in fs[::max(1, S // 16)])
        free(fs)
        return dt, ok

    def yardstick():
        dt, r = timed(lambda: ctx.read_blocks(dss, req, check_only=True, want_data=False, want_paths=False))
        return dt, r[5] == n

    legs = {"many": lambda: many(False), "yardstick": yardstick, "loop": lambda: loop(False), "many_trust": lambda: many(True),
            "loop_trust": lambda: loop(True), "scrub": lambda: (lambda r: (r[0], r[1][2] == 0))(timed(big.scrub))}
    times = {k: [] for k in legs}
    for k, fn in legs.items():                                       # warm-up
        assert fn()[1], k
    for r in range(a.repeats):
        for k, fn in legs.items():
            dt, ok = fn()
            assert ok, k
            times[k].append(dt)
        print("[%s] round %d: %s" % (name, r, ", ".join("%s %.3f s" % (k, v[-1]) for k, v in times.items())), file=sys.stderr, flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    data_gb = S * n_cells * CELL / 1e9
    out = {"leg": name, "workload": "%d one-slot file-sourced sessions of %d MiB slots (%d blocks of 64 KiB each), every block present, page-cached" %
           (S, slot_mib, nb), "sessions": S, "blocks": n, "repeats": a.repeats}
    for k, v in times.items():
        out[k + "_rounds_s"] = [round(x, 4) for x in v]
        out[k + "_s"] = round(med[k], 4)
    spread = max(times["yardstick"]) - min(times["yardstick"])
    out["yardstick_spread_s"] = round(spread, 4)
    out["many_over_yardstick"] = round(med["many"] / med["yardstick"], 3)
    out["gate"] = "many <= 1.10 x yardstick + the yardstick's spread"
    out["gate_met"] = bool(med["many"] <= 1.10 * med["yardstick"] + spread)
    out["loop_over_many"] = round(med["loop"] / med["many"], 2)
    out["loop_trust_over_many_trust"] = round(med["loop_trust"] / med["many_trust"], 2)
    out["not_slower_than_the_loop"] = bool(med["many"] <= med["loop"] and med["many_trust"] <= med["loop_trust"])
    out["many_GBps"] = round(data_gb / med["many"], 2)
    out["yardstick_GBps"] = round(data_gb / med["yardstick"], 2)
    out["loop_GBps"] = round(data_gb / med["loop"], 2)
    out["scrub_GBps"] = round(data_gb / med["scrub"], 2)
    out["many_over_scrub_rate"] = round(med["scrub"] / med["many"], 3)
    (fs, _), text = traced(lambda: pkg.fills_resume_many(ctx, cfgs, one_roots, paths))
    free(fs)
    m = re.search(r"fills resume many: .* ([0-9.]+) s \(([0-9.]+) GB/s; ([0-9.]+) checkpoints, ([0-9.]+) opens and uploads, ([0-9.]+) re-check, "
                  r"([0-9.]+) host drops\)", text)
    if m:
        out["call_split_s"] = dict(zip(("total", "GBps", "checkpoints", "opens_and_uploads", "recheck", "host_drops"), map(float, m.groups())))
    out["trace"] = [ln for ln in text.splitlines() if "fills resume many:" in ln][-1:]
    free(dss)
    big.free()
    shutil.rmtree(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="an empty or new directory for the slot files and checkpoints; removed at the end")
    ap.add_argument("--legs", default="small,large")
    ap.add_argument("--sessions", type=int, default=4096, help="the small leg's sessions")
    ap.add_argument("--slot-mib", type=int, default=1, help="the small leg's slots")
    ap.add_argument("--large-sessions", type=int, default=128)
    ap.add_argument("--large-slot-mib", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg = g.load_package()
    ctx = pkg.Context(0)
    shapes = {"small": (a.sessions, a.slot_mib), "large": (a.large_sessions, a.large_slot_mib)}
    lines = []
    try:
        os.makedirs(a.dir, exist_ok=True)
        for name in a.legs.split(","):
            lines.append(json.dumps(leg(pkg, ctx, a, name, *shapes[name])))
            print(lines[-1], flush=True)
    finally:
        ctx.close()
        shutil.rmtree(a.dir, ignore_errors=True)
    if a.out:
        args = "--legs %s --sessions %d --slot-mib %d --large-sessions %d --large-slot-mib %d --repeats %d" % (
            a.legs, a.sessions, a.slot_mib, a.large_sessions, a.large_slot_mib, a.repeats)
        with open(a.out, "w") as f:
            f.write("tools/fills_resume_many_rate.py on one MI355X (%s; medians of alternated rounds after a warm-up of each leg):\n%s\n" % (args, "\n".join(lines)))


if __name__ == "__main__":
    main()
