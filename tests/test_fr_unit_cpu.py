"""CPU suite: the device field arithmetic one primitive at a time, at the bounds its comments claim.

tests/host_check runs whole permutations, whose intermediates are pseudorandom after the first round: limbs at 2.02 U / 2.47 U,
columns near 2^64, all-ones quotient digits, reduce_wide's last table rows and the c == N branch of to_canonical_words are never
met there.  Here every primitive of csrc/fr_gfx950.hpp and csrc/poseidon2_dev.hpp is called directly on raw limb vectors
(tests/device_check/fr_unit_ops.hpp) by the host twin, built from the same source with CP2_HOST_CHECK under AddressSanitizer +
UBSan (128-bit shadow accumulator, asserted bounds), and every result is judged by plain big-int arithmetic (tests/fr_model.py).
tests/test_gpu_fr_unit.py runs the same cases through the gfx950 build.

Counts: the structured families are what the generators make (about 12 000 cases, 5000 of them reduce_wide's 96 rows x
offsets x writings); the seeded random part is 2000 cases per op (40 000): 52 111 in all.  Measured on the build machine: generating
them with every precondition asserted 1.5 s, the sanitizer build 8 s, its twenty runs and the judging 2 s, the plan check 0.6 s --
13 s for the module, below the first test of tests/test_host_check.py (the module this one sits beside)."""
import pytest

import fr_model as M


@pytest.fixture(scope="module")
def cases():
    M.check_device_constants()
    return M.build_cases(M.N_RANDOM)


def test_every_case_on_the_host_twin_with_sanitizers(cases, tmp_path, oracle):
    sections = M.to_sections(cases.items)
    exe = M.build_host_twin(str(tmp_path / "fr_unit_host"))
    results, aborts = M.run_host_twin(exe, sections, tmp_path)
    assert not aborts, "bound violations on legal cases:\n" + "\n".join(aborts)
    judged, failures = M.judge_sections(sections, results, M.oracle_permute_both)
    assert judged == len(cases.items)
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), judged, "\n".join(failures[:40]))


def test_plan(cases):
    """From the model alone: every op has every family of its plan, the unmasked quotient digits reach both extremes in every
    column, and reduce_wide meets every table row with the exact quotient and with the estimate one short."""
    have = {(op, fam) for op, fam, _ in cases.items}
    assert set(M.PLAN) == set(M.OPS)
    missing = [(op, fam) for op in M.OPS for fam in M.PLAN[op] if (op, fam) not in have]
    assert not missing, missing

    for op, masked in (("mul_u", False), ("sqr_u", False), ("mul_m", True), ("sqr_m", True)):
        top_set, top_clear, all_mask, all_zero = set(), set(), False, False
        for o, _, rec in cases.items:
            if o != op:
                continue
            a = M.fe(rec)
            digits = M.mont_columns(a, a if op.startswith("sqr") else M.fe(rec, 1), masked)[1]
            all_mask |= all(d == M.MASK for d in digits)
            all_zero |= all(d == 0 for d in digits) and any(a)
            for k, d in enumerate(digits):
                if d >> 29 == 7:
                    top_set.add(k)
                if d >> 29 == 0:
                    top_clear.add(k)
        assert all_zero, op + ": no case with A*B = 0 mod R (all digits zero)"
        if masked:
            assert op == "sqr_m" or all_mask, op + ": no case with every digit MASK"
        else:
            assert top_set == set(range(9)) and top_clear == set(range(9)), (op, sorted(top_set), sorted(top_clear))

    exact, short = set(), set()
    for o, _, rec in cases.items:
        if o == "reduce_wide":
            w = M.wd(rec, 0)
            q, est = M.wval(w) // M.N, M.reduce_estimate(w)
            assert est in (q, q - 1)
            (exact if est == q else short).add(est)
    assert exact == set(range(M.QTAB_ROWS)), sorted(set(range(M.QTAB_ROWS)) - exact)
    assert short == set(range(M.QTAB_ROWS - 1)), sorted(set(range(M.QTAB_ROWS - 1)) - short)

    # to_canonical_words: every non-zero multiple of N below R, normalised and lazy (the c == N branch)
    ks = {M.val(M.fe(rec)) // M.N for o, f, rec in cases.items if o == "to_canonical" and f == "multN" and M.val(M.fe(rec)) % M.N == 0}
    assert ks == set(range(M.R // M.N + 1))
