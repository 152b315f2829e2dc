"""What cp2_fills_finish_many costs against the loop of cp2_fill_finish it replaces, and its level launches against k_compress_layer.

Three parts (--parts call,levels,mixed), each on one MI355X in one process: a warm-up of every leg, then --repeats rounds of the legs
alternated; medians, every leg's rounds printed so the spread shows.  A finish consumes its sessions, so every round refills them with
cp2_fills_add_many (one cp2_fill_add for the one-session leg) OUTSIDE the timed region.

  call    --sessions 4096 one-slot fake-source sessions of --slot-mib 1 MiB slots (16 blocks of 64 KiB, depth 4), filled completely.
          many: one cp2_fills_finish_many.  loop: 4096 cp2_fill_finish, the only way without the call and the yardstick.  one: one
          cp2_fill_finish of ONE session whose 4096 local slots are those slots (recorded: it makes one dataset object, the call 4096).
          REQUIRED: many is not slower than loop.  The call's own CP2_TRACE line gives its split: planning, the device interval (tables
          up, level launches, verdicts down: queued on one stream and drained once, so the host sees one interval), saving, objects and
          hand-over.
  levels  the level launches alone, through tests/device_check/libfill_finish_many_unit.so on torch tensors: --trees 4096 sessions x 1
          slot x --leaves 4096 block roots (2^24 leaves), against k_compress_layer over the same leaves layer by layer (libkernel_unit.so);
          each round is the median of --inner 5 runs; both results must be equal.  GATE, the project's convention for a table-driven twin
          of a uniform kernel: at most 1.10 times the yardstick plus the yardstick's spread between its rounds.
  mixed   --mixed-sessions 4096 sessions cycling through 1, 2, 16, 256 and 4096 blocks and 1 to 3 slots (cells of 64 bytes, blocks of 256),
          the call against the loop.  Recorded only.
Prints one JSON line per part and, with --out, writes them with a heading.

    python tools/fill_finish_many_rate.py [--parts call,levels,mixed] [--repeats 2] [--out profiles/fill_finish_many_rate.txt]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL, BLOCK = 2048, 65536


def layer_sizes(n):
    sizes, m = [n], n
    while True:
        m = (m + 1) // 2
        sizes.append(m)
        if m == 1:
            return sizes


def rounds(record, legs, repeats):
    """a warm-up of each leg, then the legs alternated; the medians, with every round in the record"""
    times = {k: [] for k in legs}
    for f in legs.values():
        f()
    for _ in range(repeats):
        for k, f in legs.items():
            times[k].append(f())
    for k, v in times.items():
        record[k + "_rounds_s"] = [round(x, 6) for x in v]
        record[k + "_s"] = round(statistics.median(v), 6)
    return {k: statistics.median(v) for k, v in times.items()}, times


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


def timed(ctx, f):
    ctx.sync()
    t = time.perf_counter()
    r = f()
    return time.perf_counter() - t, r


def free(hs):
    for h in hs:
        h.free()


def part_call(pkg, ctx, a):
    S = a.sessions
    n_cells, nb = (a.slot_mib << 20) // CELL, (a.slot_mib << 20) // BLOCK
    big = pkg.make_config(maxDepth=32, maxLog2NSlots=max(1, (S - 1).bit_length()), cellSize=CELL, blockSize=BLOCK, nSlots=S, nCells=n_cells, nSamples=100,
                          seed=1)
    small = pkg.make_config(maxDepth=32, maxLog2NSlots=1, cellSize=CELL, blockSize=BLOCK, nSlots=1, nCells=n_cells, nSamples=100, seed=1)
    ctx.set_keep_trees(2)
    try:
        ds = ctx.dataset(big)
    finally:
        ctx.set_keep_trees(-1)
    roots = ds.local_roots()
    pairs = np.array([(s, b) for s in range(S) for b in range(nb)], dtype=np.uint64)
    n = len(pairs)
    cand = np.empty((n, BLOCK), dtype=np.uint8)
    for s in range(S):
        cand[s * nb:(s + 1) * nb] = np.ascontiguousarray(ctx.gen_fake_cells(ctx.slot_seed(1, s), 0, n_cells, CELL)).reshape(nb, BLOCK)
    _, paths = ds.block_proofs(pairs)
    ds.free()
    depth = int(paths.shape[1])
    req = np.ascontiguousarray(np.stack([pairs[:, 0], np.zeros(n, np.uint64), pairs[:, 1]], axis=1))   # session k's one slot is its slot 0
    record = {"part": "call", "sessions": S, "blocks": n, "depth": depth, "repeats": a.repeats,
              "workload": "%d one-slot fake-source sessions of %d MiB slots (%d blocks of 64 KiB, depth %d), filled completely" % (S, a.slot_mib, nb, depth)}

    def filled():
        fs = [ctx.fill(small, roots[k:k + 1], 0, 1) for k in range(S)]
        st, new = pkg.fills_add_many(ctx, fs, req, cand, paths.reshape(-1, 32))
        assert sum(new) == n and (st == 0).all()
        return fs

    def check(dss):
        assert all(d.local_roots().tobytes() == roots[k].tobytes() for k, d in list(enumerate(dss))[::max(1, S // 16)])

    def leg_many():
        fs = filled()
        dt, dss = timed(ctx, lambda: pkg.fills_finish_many(ctx, fs))
        check(dss)
        free(dss + fs)
        return dt

    def leg_loop():
        fs = filled()
        dt, dss = timed(ctx, lambda: [f.finish() for f in fs])
        check(dss)
        free(dss + fs)
        return dt

    def leg_one():
        f = ctx.fill(big, roots)
        st, new = f.add(pairs, cand, paths)
        assert new == n
        dt, d = timed(ctx, f.finish)
        assert d.local_roots().tobytes() == roots.tobytes()
        free([d, f])
        return dt

    med, times = rounds(record, {"many": leg_many, "loop": leg_loop, "one": leg_one}, a.repeats)
    record["loop_over_many"] = round(med["loop"] / med["many"], 2)
    record["many_over_one"] = round(med["many"] / med["one"], 2)
    record["not_slower_than_the_loop"] = bool(med["many"] <= med["loop"])
    fs = filled()
    dss, text = traced(lambda: pkg.fills_finish_many(ctx, fs))
    free(dss + fs)
    m = re.search(r"fills finish many: .*launch\(es\), \d+ kept form\(s\) saved, ([0-9.]+) ms \(([0-9.]+) planning, ([0-9.]+) tables up \+ launches \+ verdicts down, "
                  r"([0-9.]+) saving, ([0-9.]+) objects and hand-over\)", text)
    if m:
        record["call_split_ms"] = dict(zip(("total", "planning", "tables_up_launches_verdicts_down", "saving", "objects_and_hand_over"), map(float, m.groups())))
    record["trace"] = [ln for ln in text.splitlines() if "fills finish many:" in ln][-1:]
    return record


def part_levels(pkg, a):
    import torch
    pkg.load_library()
    dc = os.path.join(ROOT, "tests", "device_check")
    lf, lk = ctypes.CDLL(os.path.join(dc, "libfill_finish_many_unit.so")), ctypes.CDLL(os.path.join(dc, "libkernel_unit.so"))
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    lf.ffm_finish_layers_many.restype, lf.ffm_finish_layers_many.argtypes = ctypes.c_int, [vp, u64, vp, vp, vp, vp, vp, vp, sz, vp]
    lk.ku_compress_layer.restype, lk.ku_compress_layer.argtypes = ctypes.c_int, [vp, vp, sz, sz, ctypes.c_int, sz, sz]
    T, n = a.trees, a.leaves
    sizes = layer_sizes(n)
    total, depth = sum(sizes), len(sizes) - 1
    off = [sum(sizes[:k]) for k in range(depth + 1)]
    gen = torch.Generator(device="cuda").manual_seed(7)
    uniform = torch.zeros((T, total, 32), dtype=torch.uint8, device="cuda")
    uniform[:, :n, :31] = torch.randint(0, 256, (T, n, 31), dtype=torch.uint8, device="cuda", generator=gen)
    many = uniform.clone()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()   # noqa: E731

    def run_uniform():
        for k in range(depth):
            st = lk.ku_compress_layer(uniform.data_ptr() + 32 * off[k], uniform.data_ptr() + 32 * off[k + 1], sizes[k], T, int(k == 0), total, total)
            assert st == 0, st

    run_uniform()
    torch.cuda.synchronize()
    stated = uniform[:, total - 1, :].contiguous()                         # the yardstick's roots as the stated ones: every verdict 0
    tab = np.zeros((T, 7), dtype=np.uint64)
    for k in range(T):
        tab[k] = (many.data_ptr() + 32 * total * k, total, stated.data_ptr() + 32 * k, 1, 0, n, depth)
    prefix = np.concatenate([np.arange(1, T + 1, dtype=np.uint64) * np.uint64(sizes[k + 1]) for k in range(depth)])
    sess_of = np.tile(np.arange(T, dtype=np.uint32), depth)
    l_off = np.arange(depth, dtype=np.uint64) * np.uint64(T)
    l_cnt = np.full(depth, T, dtype=np.uint64)
    l_work = np.array([T * sizes[k + 1] for k in range(depth)], dtype=np.uint64)
    d_tab, d_voff, d_prefix, d_sess = up(tab), up(np.arange(T, dtype=np.uint64)), up(prefix), up(sess_of)
    verdict = torch.full((T,), 7, dtype=torch.int32, device="cuda")

    def run_many():
        st = lf.ffm_finish_layers_many(d_tab.data_ptr(), T, d_voff.data_ptr(), d_prefix.data_ptr(), d_sess.data_ptr(), l_off.ctypes.data, l_cnt.ctypes.data,
                                       l_work.ctypes.data, depth, verdict.data_ptr())
        assert st == 0, st

    def leg(f):
        def one():
            v = []
            for _ in range(a.inner):
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                v.append(time.perf_counter() - t)
            return statistics.median(v)
        return one

    record = {"part": "levels", "trees": T, "leaves_per_tree": n, "levels": depth, "nodes_built": T * (total - n), "repeats": a.repeats, "inner": a.inner}
    med, times = rounds(record, {"k_compress_layer": leg(run_uniform), "k_finish_layer_many": leg(run_many)}, a.repeats)
    record["equal_results"] = bool(torch.equal(uniform, many)) and bool((verdict == 0).all())
    spread = max(times["k_compress_layer"]) - min(times["k_compress_layer"])
    record["yardstick_spread_s"] = round(spread, 6)
    record["many_over_uniform"] = round(med["k_finish_layer_many"] / med["k_compress_layer"], 3)
    record["gate"] = "k_finish_layer_many <= 1.10 x k_compress_layer + the yardstick's spread"
    record["accepted"] = bool(med["k_finish_layer_many"] <= 1.10 * med["k_compress_layer"] + spread)
    return record


def part_mixed(pkg, ctx, a):
    S, cell, block = a.mixed_sessions, 64, 256
    blocks, per = (1, 2, 16, 256, 4096), 256 // 64
    shape = [(blocks[k % 5], 1 + k % 3) for k in range(S)]
    cfgs = [pkg.make_config(maxDepth=32, maxLog2NSlots=2, cellSize=cell, blockSize=block, nSlots=4, nCells=per * nb, nSamples=5, seed=3000 + k)
            for k, (nb, _) in enumerate(shape)]
    ctx.set_keep_trees(2)
    try:
        built = ctx.build_many([(cfgs[k], 0, nl) for k, (_, nl) in enumerate(shape)])
    finally:
        ctx.set_keep_trees(-1)
    roots, req, data, paths = [], [], [], []
    for k, ((nb, nl), d) in enumerate(zip(shape, built)):
        roots.append(d.local_roots())
        sb = np.stack(np.meshgrid(np.arange(nl, dtype=np.uint64), np.arange(nb, dtype=np.uint64), indexing="ij"), axis=-1).reshape(-1, 2)
        paths.append(d.block_proofs(sb)[1].reshape(-1, 32))
        req.append(np.concatenate([np.full((len(sb), 1), k, dtype=np.uint64), sb], axis=1))
        data += [np.ascontiguousarray(ctx.gen_fake_cells(ctx.slot_seed(3000 + k, s), 0, per * nb, cell)).reshape(nb, block) for s in range(nl)]
        d.free()
    req, data, paths = np.concatenate(req), np.concatenate(data), np.concatenate(paths)
    record = {"part": "mixed", "sessions": S, "blocks": int(len(req)), "slots": sum(nl for _, nl in shape), "repeats": a.repeats,
              "workload": "%d sessions cycling through 1, 2, 16, 256 and 4096 blocks and 1 to 3 slots (cells of 64 bytes, blocks of 256)" % S}

    def filled():
        fs = [ctx.fill(cfgs[k], roots[k], 0, nl) for k, (_, nl) in enumerate(shape)]
        st, new = pkg.fills_add_many(ctx, fs, req, data, paths)
        assert sum(new) == len(req) and (st == 0).all()
        return fs

    def check(dss):
        assert all(d.local_roots().tobytes() == roots[k].tobytes() for k, d in list(enumerate(dss))[::max(1, S // 64)])

    def leg_many():
        fs = filled()
        dt, dss = timed(ctx, lambda: pkg.fills_finish_many(ctx, fs))
        check(dss)
        free(dss + fs)
        return dt

    def leg_loop():
        fs = filled()
        dt, dss = timed(ctx, lambda: [f.finish() for f in fs])
        check(dss)
        free(dss + fs)
        return dt

    med, _ = rounds(record, {"many": leg_many, "loop": leg_loop}, a.repeats)
    record["loop_over_many"] = round(med["loop"] / med["many"], 2)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="call,levels,mixed")
    ap.add_argument("--sessions", type=int, default=4096)
    ap.add_argument("--slot-mib", type=int, default=1)
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--leaves", type=int, default=4096)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--mixed-sessions", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    import torch  # noqa: F401  (its HIP runtime first, as the package does)
    pkg = g.load_package()
    parts, lines = a.parts.split(","), []
    ctx = pkg.Context(0)
    try:
        for p in parts:
            record = {"call": lambda: part_call(pkg, ctx, a), "levels": lambda: part_levels(pkg, a), "mixed": lambda: part_mixed(pkg, ctx, a)}[p]()
            lines.append(json.dumps(record))
            print(lines[-1], flush=True)
    finally:
        ctx.close()
    if a.out:
        args = "--parts %s --sessions %d --slot-mib %d --trees %d --leaves %d --inner %d --mixed-sessions %d --repeats %d" % (
            a.parts, a.sessions, a.slot_mib, a.trees, a.leaves, a.inner, a.mixed_sessions, a.repeats)
        with open(a.out, "w") as f:
            f.write("tools/fill_finish_many_rate.py on one MI355X (%s; medians of alternated rounds after a warm-up of each leg):\n%s\n" % (args, "\n".join(lines)))


if __name__ == "__main__":
    main()
