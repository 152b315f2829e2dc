"""CPU suite: the input.json reader (csrc/json_parse.hpp, behind cp2_proof_input_parse_json) compiled alone for the host under
AddressSanitizer + UBSan: random round trips through the byte-exact writer, every truncation refused with a message, random
overwrites refused or parsed without a report.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_json_reader_round_trips_and_truncations_with_sanitizers(tmp_path):
    exe = str(tmp_path / "json_parse_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "codex-storage-proofs-circuits_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_check", "json_parse_check.cpp")])
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "json parse ok: 300 round trips" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr, r.stdout + r.stderr[-2000:]
