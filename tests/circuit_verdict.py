"""TEST INFRASTRUCTURE: what SampleAndProve accepts, written down once for the verifier's tests.

circuit/codex/sample_cells.circom:58-148 (with single_cell.circom:30-73, merkle.circom:44-114, lib/log2.circom, misc.circom ToBits),
over the FIELD ELEMENTS the circuit reads, not over bytes: a proof input here is a dict

    {"dataSetRoot", "entropy", "nCellsPerSlot", "nSlotsPerDataSet", "slotIndex", "slotRoot": int,
     "slotProof": [int] * maxLog2NSlots, "cellData": [[int] * nf] * nSamples, "merklePaths": [[int] * maxDepth] * nSamples}

(the keys of input.json).  verdict() returns the status bits of include/codex_p2.h (CP2_VERIFY_*) and one 0/1 per sample, where
oracle.poseidon2_ref.circuit_check stops at the first failure and takes bytes.  The hashing is the oracle's circom-side restatement
(oracle.circom_ref.Poseidon2_hash_rate2, oracle.poseidon2_ref.circuit_root_from_path)."""
import json

from oracle.circom_ref import Poseidon2_hash_rate2
from oracle.poseidon2_ref import R_MOD, bytes_to_felts, circuit_root_from_path

DATASET_ROOT, SAMPLE, SHAPE = 1, 2, 4
KEYS = ("dataSetRoot", "entropy", "nCellsPerSlot", "nSlotsPerDataSet", "slotIndex", "slotRoot", "slotProof", "cellData", "merklePaths")


def from_text(text):
    """input.json text -> felt dict (numbers quoted or bare)."""
    d = json.loads(text)
    out = {k: int(d[k]) for k in KEYS[:6]}
    out["slotProof"] = [int(x) for x in d["slotProof"]]
    out["cellData"] = [[int(x) for x in row] for row in d["cellData"]]
    out["merklePaths"] = [[int(x) for x in row] for row in d["merklePaths"]]
    return out


def from_oracle(p):
    """oracle.poseidon2_ref.generate_proof_input's dict (cells as bytes) -> felt dict."""
    return {"dataSetRoot": p["dataSetRoot"], "entropy": p["entropy"], "nCellsPerSlot": p["nCells"], "nSlotsPerDataSet": p["nSlots"],
            "slotIndex": p["slotIndex"], "slotRoot": p["slotRoot"], "slotProof": list(p["slotProof"]["merklePath"]),
            "cellData": [bytes_to_felts(q["cellData"]) for q in p["proofInputs"]],
            "merklePaths": [list(q["merkleProof"]["merklePath"]) for q in p["proofInputs"]]}


def to_text(d):
    """felt dict -> input.json text (compact; felts as quoted decimals, the three counts bare)."""
    o = {k: (str(d[k]) if k in ("dataSetRoot", "entropy", "slotRoot") else d[k]) for k in KEYS[:6]}
    o["slotProof"] = [str(x) for x in d["slotProof"]]
    o["cellData"] = [[str(x) for x in row] for row in d["cellData"]]
    o["merklePaths"] = [[str(x) for x in row] for row in d["merklePaths"]]
    return json.dumps(o)


def copy(d):
    return {k: ([list(r) for r in v] if k in ("cellData", "merklePaths") else list(v) if k == "slotProof" else v) for k, v in d.items()}


def block_tree_depth(cfg):
    cpb = cfg["blockSize"] // cfg["cellSize"]
    assert cpb * cfg["cellSize"] == cfg["blockSize"] and cpb >= 2 and cpb & (cpb - 1) == 0, "the circuit needs blockTreeDepth >= 1"
    return cpb.bit_length() - 1


def shape_ok(d, cfg):
    """Witness generation's assertions: Log2_CircomWitnessCalc_Hack(maxDepth) of nCellsPerSlot (mask[0] === 1, mask[n] === 0,
    inp === sum), ToBits(maxLog2NSlots) of nSlotsPerDataSet - 1 (CeilingLog2) and of slotIndex."""
    nc, ns, si, m = d["nCellsPerSlot"], d["nSlotsPerDataSet"], d["slotIndex"], cfg["maxLog2NSlots"]
    if nc < 2 or nc & (nc - 1) or nc.bit_length() - 1 > cfg["maxDepth"]:
        return False
    if not 1 <= ns <= (1 << m):
        return False
    return 0 <= si < (1 << m)


def top_root(d, cfg):
    """RootFromMerklePath(maxLog2NSlots) of slotRoot, sample_cells.circom:95-109."""
    m, last = cfg["maxLog2NSlots"], d["nSlotsPerDataSet"] - 1
    sbits = [(d["slotIndex"] >> i) & 1 for i in range(m)]
    lbits = [(last >> i) & 1 for i in range(m)]
    mask = [1 if (last >> i) != 0 else 0 for i in range(m)] + [0]        # CeilingLog2, lib/log2.circom:108-130
    return circuit_root_from_path(d["slotRoot"], sbits, lbits, mask, d["slotProof"])


def sample_index(d, cfg, cnt):
    """CalculateCellIndexBits (sample_cells.circom:23-48) for counter cnt + 1, as an integer."""
    h = Poseidon2_hash_rate2([d["entropy"], d["slotRoot"], cnt + 1])
    return h & (d["nCellsPerSlot"] - 1)


def sample_root(d, cfg, cnt):
    """ProveSingleCell (single_cell.circom:30-73): the slot root that sample cnt's cell and path reconstruct."""
    md, bd, nc = cfg["maxDepth"], block_tree_depth(cfg), d["nCellsPerSlot"]
    lgmask = [1 if (1 << i) < nc else 0 for i in range(md + 1)]            # Log2 mask, lib/log2.circom:76-78
    idx = sample_index(d, cfg, cnt)
    bits = [lgmask[i] * ((idx >> i) & 1) for i in range(md)]
    leaf = Poseidon2_hash_rate2(d["cellData"][cnt])
    path = d["merklePaths"][cnt]
    bot = circuit_root_from_path(leaf, bits[:bd], lgmask[:bd], lgmask[:bd] + [0], path[:bd])
    return circuit_root_from_path(bot, bits[bd:], lgmask[bd:md], lgmask[bd:md] + [0], path[bd:])


def verdict(d, cfg):
    """(status bits, [0/1 per sample]) of one proof input under cfg (maxDepth, maxLog2NSlots, cellSize, blockSize)."""
    ns = len(d["cellData"])
    if not shape_ok(d, cfg):
        return SHAPE, [0] * ns
    status = 0 if top_root(d, cfg) == d["dataSetRoot"] % R_MOD else DATASET_ROOT
    ok = [1 if sample_root(d, cfg, c) == d["slotRoot"] % R_MOD else 0 for c in range(ns)]
    if not all(ok):
        status |= SAMPLE
    return status, ok
