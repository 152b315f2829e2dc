"""CPU suite: reading input.json back (cp2_proof_input_parse_json) and the circuit's acceptance rule written down in
tests/circuit_verdict.py, checked against the oracle.  No GPU."""
import json

import numpy as np
import pytest

import circuit_verdict as V
from oracle_helpers import expected_proof_input_fast

GOLDENS = ("testmain_small", "odd_slots_one_block", "params_default")


def _cfg(pkg, c, **kw):
    return pkg.make_config(**dict(c, **kw))


def _model(golden, name):
    return golden("proof_inputs.json")["inputs"][name]


def test_parser_round_trip_on_the_goldens(pkg, golden, oracle):
    """parse -> json() reproduces the producer's text byte for byte; the roots, the slot proof and the cell bytes are what the
    fixtures and the oracle say; the parsed object has no cell indices or leaf hashes."""
    C, P = oracle
    for name in GOLDENS:
        m = _model(golden, name)
        c = m["config"]
        text = golden("input_%s.json" % name)
        p = pkg.parse_proof_input(_cfg(pkg, c), text)
        assert p.json() == text
        d, s, e = p.roots()
        assert pkg.array_to_felts(d)[0] == int(m["dataSetRoot"]) and pkg.array_to_felts(s)[0] == int(m["slotRoot"])
        assert pkg.array_to_felts(e)[0] == m["entropy"]
        assert p.shape() == (c["nCells"], c["nSlots"], m["slotIndex"])
        want = expected_proof_input_fast(C, P, c, m["slotIndex"], m["entropy"], threads=4)
        assert pkg.array_to_felts(p.slot_proof()) == list(want["slotProof"]["merklePath"])
        cells = p.cell_data()
        assert cells.shape == (c["nSamples"], c["cellSize"])
        for i, q in enumerate(want["proofInputs"]):
            assert cells[i].tobytes() == q["cellData"]
            assert pkg.array_to_felts(p.cell_felts()[i]) == P.bytes_to_felts(q["cellData"])
            assert pkg.array_to_felts(p.merkle_paths()[i]) == list(q["merkleProof"]["merklePath"])
        assert p.cell_indices() is None and p.leaf_hashes() is None
        # nSamples = 0: as many rows as the text has
        assert pkg.parse_proof_input(_cfg(pkg, c, nSamples=0), text).json() == text


def test_reordered_keys_and_compact_whitespace_parse_to_the_same_object(pkg, golden):
    for name in GOLDENS:
        c = _model(golden, name)["config"]
        text = golden("input_%s.json" % name)
        d = json.loads(text)
        keys = list(d.keys())[::-1]
        compact = json.dumps({k: d[k] for k in keys}, separators=(",", ":"))
        assert pkg.parse_proof_input(_cfg(pkg, c), compact).json() == text
        bare = json.dumps({k: ([int(x) for x in v] if k == "slotProof" else v) for k, v in d.items()}, indent="\t")
        assert pkg.parse_proof_input(_cfg(pkg, c), bare).json() == text


R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _refused(pkg, cfg, text, *words):
    with pytest.raises(pkg.CodexP2Error) as e:
        pkg.parse_proof_input(cfg, text)
    assert e.value.status == -1
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_parser_refusals_name_the_key_and_row(pkg, golden):
    name = "odd_slots_one_block"
    c = _model(golden, name)["config"]
    cfg = _cfg(pkg, c)
    text = golden("input_%s.json" % name)
    d = json.loads(text)

    def dump(o):
        return json.dumps(o)

    _refused(pkg, cfg, dump({k: v for k, v in d.items() if k != "slotRoot"}), "missing key", "slotRoot")
    _refused(pkg, cfg, dump(dict(d, extra="1")), "unknown key", "extra")
    _refused(pkg, cfg, text.replace("{\n", '{\n  "entropy": "5",\n', 1), "repeated key", "entropy")
    _refused(pkg, cfg, dump(dict(d, slotProof=d["slotProof"][:-1])), "slotProof", "entries")
    _refused(pkg, cfg, dump(dict(d, cellData=d["cellData"][:-1])), "cellData", "rows")
    _refused(pkg, cfg, dump(dict(d, merklePaths=[d["merklePaths"][0], d["merklePaths"][1][:-1], d["merklePaths"][2]])),
             "merklePaths row 1", "entries")
    bad = [list(r) for r in d["cellData"]]
    bad[2][1] = str(R)
    _refused(pkg, cfg, dump(dict(d, cellData=bad)), "cellData row 2 column 1", ">= r")
    bad[2][1] = "-5"
    _refused(pkg, cfg, dump(dict(d, cellData=bad)), "cellData row 2 column 1", "sign")
    bad[2][1] = "12a"
    _refused(pkg, cfg, dump(dict(d, cellData=bad)), "cellData row 2 column 1", "digit")
    _refused(pkg, cfg, dump(dict(d, entropy=str(R))), "entropy", ">= r")
    _refused(pkg, cfg, dump(dict(d, dataSetRoot=str(R - 1))).replace(str(R - 1), str(R - 1) + "0"), "dataSetRoot")
    _refused(pkg, cfg, dump(dict(d, nCellsPerSlot=1 << 64)), "nCellsPerSlot", "64 bits")
    _refused(pkg, cfg, text + "}", "trailing text")
    _refused(pkg, cfg, "", "'{'")
    # a value r - 1 is a field element: accepted
    assert pkg.parse_proof_input(cfg, dump(dict(d, entropy=str(R - 1)))).roots()[2].tobytes() == (R - 1).to_bytes(32, "little")
    # truncation at every 97th byte (and just before the closing brace) fails
    for cut in list(range(0, len(text) - 2, 97)) + [len(text) - 2]:
        with pytest.raises(pkg.CodexP2Error):
            pkg.parse_proof_input(cfg, text[:cut])


def test_rows_that_encode_no_bytes_keep_their_felts(pkg, golden):
    """A cell row with a felt >= 2^248 (or a wrong padding byte) is what the circuit reads all the same: the object keeps the
    felts and prints them back, and cell_data() is None."""
    c = _model(golden, "odd_slots_one_block")["config"]
    d = V.from_text(golden("input_odd_slots_one_block.json"))
    d["cellData"][1][0] = (1 << 250) + 7
    p = pkg.parse_proof_input(_cfg(pkg, c), V.to_text(d))
    assert p.cell_data() is None
    assert pkg.array_to_felts(p.cell_felts()[1]) == d["cellData"][1]
    assert V.from_text(p.json()) == d


def test_the_helper_accepts_the_goldens(golden):
    for name in GOLDENS:
        c = _model(golden, name)["config"]
        d = V.from_text(golden("input_%s.json" % name))
        assert V.verdict(d, c) == (0, [1] * c["nSamples"])


def _oracle_raises(P, p, c):
    try:
        P.circuit_check(p, c)
        return False
    except AssertionError:
        return True


def test_the_helper_agrees_with_the_oracles_circuit_check(oracle, golden):
    """Single-felt mutations of a byte-level proof input: circuit_check raises exactly when the helper rejects; a padding-level
    path entry set to 1 is accepted by both."""
    C, P = oracle
    m = _model(golden, "odd_slots_one_block")
    c = m["config"]
    base = expected_proof_input_fast(C, P, c, m["slotIndex"], m["entropy"], threads=4)

    def mutated(f):
        p = json.loads(json.dumps({k: v for k, v in base.items() if k != "proofInputs"}))
        p["proofInputs"] = [{"cellData": q["cellData"], "merkleProof": {"merklePath": list(q["merkleProof"]["merklePath"])}}
                            for q in base["proofInputs"]]
        p["slotProof"] = {"merklePath": list(base["slotProof"]["merklePath"])}
        f(p)
        return p

    def set_path(s, i, v):
        return lambda p: p["proofInputs"][s]["merkleProof"]["merklePath"].__setitem__(i, v)

    def set_cell_byte(s, b):
        def f(p):
            cell = bytearray(p["proofInputs"][s]["cellData"])
            cell[b] ^= 0x5A
            p["proofInputs"][s]["cellData"] = bytes(cell)
        return f

    cases = {
        "none": (lambda p: None, False),
        "dataSetRoot": (lambda p: p.__setitem__("dataSetRoot", p["dataSetRoot"] + 1), True),
        "slotRoot": (lambda p: p.__setitem__("slotRoot", p["slotRoot"] + 1), True),
        "entropy": (lambda p: p.__setitem__("entropy", p["entropy"] + 1), None),
        "slotProof[0]": (lambda p: p["slotProof"]["merklePath"].__setitem__(0, 5), True),
        "path below": (set_path(1, 0, 12345), True),
        "path padding": (set_path(0, c["maxDepth"] - 1, 1), False),
        "cell byte": (set_cell_byte(2, 3), True),
    }
    for what, (f, want) in cases.items():
        p = mutated(f)
        status, ok = V.verdict(V.from_oracle(p), c)
        raised = _oracle_raises(P, p, c)
        assert raised == (status != 0), (what, status, ok, raised)
        if want is not None:
            assert raised == want, what


def test_shape_failures_are_reported_alone(golden):
    c = _model(golden, "odd_slots_one_block")["config"]
    d = V.from_text(golden("input_odd_slots_one_block.json"))
    for k, v in (("nCellsPerSlot", 1), ("nCellsPerSlot", 3), ("nCellsPerSlot", 1 << (c["maxDepth"] + 1)),
                 ("nSlotsPerDataSet", 0), ("nSlotsPerDataSet", (1 << c["maxLog2NSlots"]) + 1), ("slotIndex", 1 << c["maxLog2NSlots"])):
        e = V.copy(d)
        e[k] = v
        assert V.verdict(e, c) == (V.SHAPE, [0] * c["nSamples"]), (k, v)
    e = V.copy(d)
    e["nSlotsPerDataSet"] = 1 << c["maxLog2NSlots"]          # the largest allowed: not a shape failure (the root no longer matches)
    assert V.verdict(e, c)[0] == V.DATASET_ROOT


def test_verify_refuses_without_a_context_argument(pkg):
    """The ABI answers a NULL context with CP2_ERR_INVALID before it touches any device."""
    L = pkg.load_library()
    st = np.zeros(1, dtype=np.uint32)
    assert L.cp2_proof_inputs_verify(None, None, 0, None, None) == -1
    assert L.cp2_proof_input_cell_felts(None, None) == -1
    assert L.cp2_proof_input_shape(None, None, None, None) == -1
    del st
