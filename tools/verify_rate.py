"""Rate of cp2_proof_inputs_verify on configs[3]'s shape: 4096 inputs of a 4096-slot x 2^12-cell dataset, 100 samples each.

Reports, as one JSON line:
  objects   the whole call on the producer's objects (cell bytes -> felts while packing, copies, kernel, verdicts), and the same
            call on parsed objects (felts copied as held): the difference is the bytes -> felts packing
  texts     parsing the 4096 input.json texts on 16 host threads, then the call: the `verify` program's path
  cpu       the C oracle's time for 64 of the inputs: their permutation count (2 index + ceil((nf+1)/2) leaf + the path levels per
            sample, the top path per input) at the oracle's measured permutation rate on 16 threads
Usage: python tools/verify_rate.py [--repeat 3]   (needs an MI355X; test infrastructure: the oracle is only timed here)"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    C, _ = g.load_oracle()
    C.build()
    c = dict(maxDepth=32, maxLog2NSlots=12, cellSize=2048, blockSize=65536, nSlots=4096, nCells=4096, nSamples=100, seed=99)
    cfg = pkg.make_config(**c)
    ctx = pkg.Context(0)
    ctx.set_keep_trees(2)
    ds = ctx.dataset(cfg)
    objs = ds.proof_inputs(list(range(c["nSlots"])), 31337)
    ds.free()
    n, ns = len(objs), c["nSamples"]

    def best(f):
        ts = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            out = f()
            ts.append(time.perf_counter() - t0)
        return min(ts), out

    ctx.verify_proof_inputs(objs[:64])                                   # warm-up: code object, pinned and device blocks
    t_obj, (st, ok) = best(lambda: ctx.verify_proof_inputs(objs))
    assert not st.any() and ok.all()
    texts = [p.json() for p in objs]
    cfg0 = pkg.make_config(**dict(c, nSamples=0))
    with ThreadPoolExecutor(16) as ex:
        t_parse, parsed = best(lambda: list(ex.map(lambda t: pkg.parse_proof_input(cfg0, t), texts)))
    t_felt, (st, ok) = best(lambda: ctx.verify_proof_inputs(parsed))
    assert not st.any() and ok.all()
    # the C oracle: permutations of 64 inputs at its measured rate
    nf = (c["cellSize"] + 1 + 30) // 31
    bd = (c["blockSize"] // c["cellSize"]).bit_length() - 1
    k = c["nCells"].bit_length() - 1
    per_sample = 2 + (nf + 2) // 2 + min(bd, k) + max(1, min(c["maxDepth"] - bd, k - bd))
    perms64 = 64 * (ns * per_sample + c["maxLog2NSlots"])
    states = np.random.default_rng(1).integers(0, 256, (1 << 17, 96), dtype=np.uint8)
    states[:, 31::32] = 0
    t0 = time.perf_counter()
    C.permute_batch(states, threads=16)
    oracle_rate = states.shape[0] / (time.perf_counter() - t0)
    rec = {
        "workload": "4096 inputs x 100 samples, 4096 slots x 2^12 cells of 2048 B, maxDepth 32 (configs[3] shape)",
        "objects_s": round(t_obj, 4), "objects_samples_per_s": round(n * ns / t_obj), "objects_inputs_per_s": round(n / t_obj),
        "parsed_objects_s": round(t_felt, 4), "packing_bytes_to_felts_s": round(t_obj - t_felt, 4),
        "texts_parse_s": round(t_parse, 4), "texts_total_s": round(t_parse + t_felt, 4),
        "texts_inputs_per_s": round(n / (t_parse + t_felt)), "texts_samples_per_s": round(n * ns / (t_parse + t_felt)),
        "perms_per_sample": per_sample, "c_oracle_perm_per_s_16t": round(oracle_rate), "c_oracle_64_inputs_s": round(perms64 / oracle_rate, 3),
    }
    print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
