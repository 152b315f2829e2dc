"""Plain references for cp2_datasets_scrub_many: the compare kernel behind an address table, the grouping of requests into classes,
and the merge of the classes' reports.

scrub_many_model restates what csrc/kernels.hpp documents for k_scrub_compare_many: the kept row of global row g lies at
kept_addr[g / rows] + (g % rows) * 32; bits, counts and the zero words past the last row are k_scrub_compare's.  "Memory" is one flat
byte array and an address is an offset into it, so a case may put its items anywhere, in any order, with anything between them.
group_classes and merge_reports restate what include/codex_p2.h says of the call; none of this shares code with the product.
tests/test_scrub_many_cpu.py holds the model against kernel_models.scrub_model and the two plain functions against brute force."""
import collections

import numpy as np

import kernel_models as K

SCRUB_TILE = K.SCRUB_TILE
scrub_groups = K.scrub_groups


def scrub_many_model(fresh, fstride, memory, kept_addr, rows, n_items):
    """(bits, counts): bit g % 64 of bits[g / 64] is set where fresh row (g / rows) * fstride + g % rows differs from the 32 bytes of
    `memory` at kept_addr[g / rows] + (g % rows) * 32; the words run to the end of the last tile; counts[w] = set bits of tile w."""
    fresh = np.asarray(fresh, dtype=np.uint8).reshape(-1, 32)
    memory = np.asarray(memory, dtype=np.uint8).reshape(-1)
    addr = np.asarray(kept_addr, dtype=np.int64).reshape(-1)
    total = rows * n_items
    item, r = np.divmod(np.arange(total, dtype=np.int64), rows)
    at = addr[item] + r * 32
    kept = memory[at[:, None] + np.arange(32, dtype=np.int64)[None, :]] if total else np.zeros((0, 32), np.uint8)
    flags = np.zeros(scrub_groups(total) * SCRUB_TILE, dtype=bool)
    flags[:total] = (fresh[item * fstride + r] != kept).any(axis=1)
    bits = np.packbits(flags.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)
    counts = flags.reshape(-1, SCRUB_TILE).sum(axis=1).astype(np.uint32)
    return bits, counts


def decode(bits, rows, n_items):
    """The host collector: (item, row) of every set bit, in order."""
    flags = np.unpackbits(np.asarray(bits, dtype="<u8").view(np.uint8), bitorder="little")
    g = np.nonzero(flags)[0]
    assert g.size == 0 or g[-1] < rows * n_items
    return [(int(x // rows), int(x % rows)) for x in g]


# ---- classes and the merge ----------------------------------------------------------------------------------------------------------
# a request as the grouping sees it: the geometry, the level its dataset keeps, the source kind and its local slots
Request = collections.namedtuple("Request", "cell_size block_size n_cells level from_file first_slot n_local")
Class = collections.namedtuple("Class", "key items")          # items: (request index, dataset slot number) in request order


def group_classes(requests):
    """(file classes in order of first appearance, indices of the fake-source requests).  A class is the requests of equal (cell_size,
    block_size, n_cells, level) among the file-sourced ones; its items are their (request, slot) pairs, requests in the caller's order,
    slots ascending.  Fake-source requests form no class: they run one by one."""
    classes, fake = collections.OrderedDict(), []
    for i, q in enumerate(requests):
        if not q.from_file:
            fake.append(i)
            continue
        key = (q.cell_size, q.block_size, q.n_cells, q.level)
        classes.setdefault(key, []).extend((i, q.first_slot + s) for s in range(q.n_local))
    return [Class(k, v) for k, v in classes.items()], fake


def class_report(cls, item_rows, cap):
    """What the batch loop hands back for a class: ((item, row) pairs in order, at most cap; the total; the count of every item).
    item_rows[j] = the sorted mismatching rows of item j."""
    pairs = [(j, r) for j in range(len(cls.items)) for r in item_rows[j]]
    return pairs[:cap], len(pairs), [len(item_rows[j]) for j in range(len(cls.items))]


def merge_reports(n_requests, classes, reports, cap):
    """(triples: the lowest min(cap, n_bad) in (request, slot, index) order, n_bad, counts per request).  reports[k] = class_report of
    classes[k]: every class kept its lowest `cap`, so the lowest `cap` of all are among what they kept."""
    triples, n_bad, counts = [], 0, [0] * n_requests
    for cls, (pairs, total, per_item) in zip(classes, reports):
        n_bad += total
        for (request, _), c in zip(cls.items, per_item):
            counts[request] += c
        triples += [(cls.items[j][0], cls.items[j][1], r) for j, r in pairs]
    return sorted(triples)[:cap], n_bad, counts
