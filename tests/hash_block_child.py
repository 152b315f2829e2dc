"""A fresh process for tests/test_gpu_kernel_edges.py::test_hash_cells_workgroups_of_64_lanes: the workgroup shape of k_hash_cells
(CP2_HASH_BLOCK, set by the parent) is read by the library once per process.

  hash_block_child.py <npz>    sizes, rows: the cell sizes and how many cells of each the parent hashed with the oracle;
                               want: those digests, size after size; cases: (cell_size, a, n_cells) rows
The cells are made here again from the size (test_gpu_kernel_edges.cells_for), laid out and hashed as in the parent's sweeps.
Prints the failures, then one JSON line {"block", "runs", "distinct", "failed"}; exit status 1 if anything failed."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402
import test_gpu_kernel_edges as E  # noqa: E402


def main():
    z = np.load(sys.argv[1])
    want, at = {}, 0
    for s, r in zip(z["sizes"].tolist(), z["rows"].tolist()):
        want[s] = z["want"][at:at + r]
        at += r
    cases = [(s, a, n, None, False) for s, a, n in z["cases"].tolist()]
    import torch
    pkg = g.load_package()
    ctx = pkg.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    need = E.cells_needed(cases)
    assert all(need[k] == want[k[0]].shape[0] for k in need)
    by_key = {}
    for c in cases:
        by_key.setdefault((c[0], c[3]), []).append(c)
    bad = []
    for chunk in E.chunks_of(need):
        items = []
        for k in chunk:
            cells = E.cells_for(k[0], need[k])
            items += [c + (cells, want[k[0]]) for c in by_key[k]]
        bad += E.run_hash_batch(torch, ctx, items)
    torch.cuda.synchronize()
    ctx.reset_stream()
    ctx.close()
    for b in bad[:400]:
        print(b)
    print(json.dumps({"block": os.environ.get("CP2_HASH_BLOCK"), "runs": len(cases), "distinct": E.distinct(cases), "failed": len(bad)}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
