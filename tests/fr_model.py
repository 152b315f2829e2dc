"""Big-int model of the device field arithmetic (csrc/fr_gfx950.hpp, csrc/poseidon2_dev.hpp), one primitive at a time.

Used by tests/test_fr_unit_cpu.py and tests/test_gpu_fr_unit.py.  It builds the cases of tests/device_check/fr_unit_ops.hpp
(records of 32 words, layout in that header) and judges the result records.  Everything is judged on VALUES: limbs are turned
into one integer and compared with plain modular arithmetic; the column algorithm is not restated, with one exception
(`mont_columns`, see there).  Every generator asserts the documented preconditions of its op on every case it emits (PRE):
a case outside them is a bug of this file, not a finding.

Case families (the plan, checked by test_plan): fill, max, hot, alt, digits, multN, q, worst, zero, index, edge, random.
"""
import os
import re

import numpy as np

from oracle.p2_consts import ROUND_CONSTS
from oracle.poseidon2_ref import R_MOD as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_INC = os.path.join(ROOT, "codex-storage-proofs-circuits_amd", "csrc", "p2_consts_dev.inc")

REC = 32
NL, NW = 9, 5
U = 1 << 29
MASK = U - 1
W = 1 << 58
MASK58 = W - 1
M32 = (1 << 32) - 1
R = 1 << 261
RINV = pow(R, -1, N)
NPRIME = (-pow(N, -1, U)) % U            # FR_NPRIME: -N^-1 mod 2^29
NINV_R = pow(N, -1, R)
NTOP = N >> 232                           # 0x30644e
QTAB_ROWS = 96

OPS = ("norm", "norm_full", "add_lazy", "mul_m", "mul_u", "sqr_m", "sqr_u", "sbox_m", "sbox_u", "to_wide", "from_wide",
       "reduce_wide", "half_round", "round_pair", "ext_u", "ext_m", "from_words", "to_mont", "to_canonical", "permute")
OP_ID = {name: i for i, name in enumerate(OPS)}
EXT_BASES = (0, 3, 6, 9, 68, 71, 74, 77)


def limbs_of(x):
    """Normalised limbs: 0..7 < U, the rest in the top limb."""
    return [(x >> (29 * i)) & MASK for i in range(NL - 1)] + [x >> 232]


def val(l):
    return sum(int(v) << (29 * i) for i, v in enumerate(l))


def wide_of(x):
    return [(x >> (58 * j)) & MASK58 for j in range(NW - 1)] + [x >> 232]


def wval(w):
    return sum(int(v) << (58 * j) for j, v in enumerate(w))


N_LIMBS = limbs_of(N)
RC_MONT = [c * R % N for c in ROUND_CONSTS]               # P2_RC_MONT
RCW_MONT = RC_MONT[12:68] + [0]                           # P2_RCW_MONT, row 56 is zero
R2 = R * R % N


def check_device_constants():
    """The tables the kernels read (p2_consts_dev.inc) are exactly what this model uses: it cannot drift from them."""
    text = open(DEV_INC).read()

    def table(name):
        m = re.search(r"\b%s(?:\[\d+\])+ = \{(.*?)\};" % name, text, re.S)
        assert m, name
        return [int(t.rstrip("uUL"), 16) for t in re.findall(r"0x[0-9a-fA-F]+U?L*u?", m.group(1))]

    assert table("FR_N") == N_LIMBS
    assert table("FR_R2") == limbs_of(R2)
    assert table("FR_R1") == limbs_of(R % N)
    m = re.search(r"FR_NPRIME = (0x[0-9a-f]+)u", text)
    assert int(m.group(1), 16) == NPRIME
    assert table("P2_RC_MONT") == [l for c in RC_MONT for l in limbs_of(c)]
    assert table("P2_RCW_MONT") == [l for c in RCW_MONT for l in wide_of(c)]
    assert table("FR_QN_TABW") == [l for q in range(QTAB_ROWS) for l in wide_of(q * N)]
    assert re.search(r"FR_TWO29 = 0x20000000u", text)


# ---- the one allowed emulation ------------------------------------------------------------------------------------------------
def mont_columns(a, b, masked):
    """Transcription of the digit rule of mont_mul / mont_sqr: column k adds a_i b_(k-i) and m_i N_(k-i), the quotient digit is
    m_k = low 32 bits of acc * N' (low 29 when masked).  Allowed because with unmasked digits the result is NOT determined by
    its congruence class; kept to these ten lines.  Returns (result limbs, digits, largest column sum)."""
    acc, m, out, peak = 0, [], [], 0
    for k in range(2 * NL - 1):
        acc += sum(a[i] * b[k - i] for i in range(NL) if 0 <= k - i < NL)
        acc += sum(m[i] * N_LIMBS[k - i] for i in range(min(k, NL)) if k - i < NL)
        if k < NL:
            m.append(((acc & M32) * NPRIME) & (MASK if masked else M32))
            acc += m[k] * N_LIMBS[0]
        else:
            out.append(acc & MASK)
        peak, acc = max(peak, acc), acc >> 29
    return out + [acc], m, peak


# ---- preconditions (what the comments in the two headers allow) -----------------------------------------------------------------
def fe(rec, k=0):
    return rec[9 * k:9 * k + 9]


def wd(rec, off):
    return [rec[off + 2 * j] | (rec[off + 2 * j + 1] << 32) for j in range(NW)]


def put_wide(w):
    out = []
    for v in w:
        out += [v & M32, v >> 32]
    return out


def _pre_mul(a, b, masked):
    assert all(x < 5 * U for x in a + b), "mont_mul operand limb >= 5U"
    la, lb = max(a), max(b)
    assert la * lb * 1000 < (6100 if masked else 4088) * U * U, "La * Lb beyond 6.1 / 4.088 U^2"
    assert mont_columns(a, b, masked)[2] < 1 << 64


def _pre_sqr(a, masked):
    assert all(x * 100 < (247 if masked else 202) * U for x in a), "mont_sqr operand limb beyond 2.47U / 2.02U"
    assert mont_columns(a, a, masked)[2] < 1 << 64


def _pre_sbox(a):
    assert all(x * 100 < 202 * U for x in a[:8]) and val(a) < 60 * N and a[8] < 60 * 3171407


# the two entries of a half round the comments derive: (xin, Y, Z) bounds in tenths of N, limb bounds of Y and Z in W
HALF_A = (302, 186, 206)       # xin_A < 30.2N, Y2 < b + 6N = 18.6N (limbs < 4W), Z2 < b + 8N = 20.6N (limbs < 5W)
HALF_B = (596, 20, 20)         # xin_B < 59.6N, Y1 and Z1 reduced: below 2N


def _pre_half(rec, entries):
    xin, Y, Z = fe(rec), wd(rec, 10), wd(rec, 20)
    assert all(x * 100 < 202 * U for x in xin[:8]) and xin[8] < 60 * 3171407
    assert all(y < 4 * W + 64 for y in Y) and all(z < 5 * W + 64 for z in Z)
    assert any(val(xin) * 10 < e[0] * N and wval(Y) * 10 < e[1] * N and wval(Z) * 10 < e[2] * N for e in entries), "not a documented entry"


def _pre_state(rec, limb, tenths):
    for k in range(3):
        a = fe(rec, k)
        assert all(x < limb for x in a[:8]) and val(a) * 10 < tenths * N


def reduce_estimate(w):
    return (((w[4] + (w[3] >> 58)) & M32) * 1354) >> 32


def _pre_reduce(w):
    assert all(x < 1 << 63 for x in w[:4]) and w[4] < 1 << 31
    assert wval(w) < QTAB_ROWS * N and reduce_estimate(w) < QTAB_ROWS


def _pre_to_mont(a):
    assert all(x < U + 8 for x in a[:8]) and a[8] < (1 << 24) + 8
    assert val(a) * R2 < N * R        # so that A * R2 / R + N < 2N


PRE = {
    "norm": lambda r: _assert(all(x <= M32 for x in fe(r)[:8]) and fe(r)[8] < 1 << 31),
    # a[i] + carry must not wrap: carries are at most 7
    "norm_full": lambda r: _assert(all(x <= M32 - 8 for x in fe(r)[:8]) and fe(r)[8] < 1 << 31),
    "add_lazy": lambda r: _assert(all(x + y <= M32 for x, y in zip(fe(r), fe(r, 1)))),
    "mul_m": lambda r: _pre_mul(fe(r), fe(r, 1), True),
    "mul_u": lambda r: _pre_mul(fe(r), fe(r, 1), False),
    "sqr_m": lambda r: _pre_sqr(fe(r), True),
    "sqr_u": lambda r: _pre_sqr(fe(r), False),
    "sbox_m": lambda r: _pre_sbox(fe(r)),
    "sbox_u": lambda r: _pre_sbox(fe(r)),
    "to_wide": lambda r: _assert(all(x <= M32 for x in fe(r))),
    "from_wide": lambda r: _assert(all(x <= MASK58 for x in wd(r, 0)[:4]) and wd(r, 0)[4] <= M32),
    "reduce_wide": lambda r: _pre_reduce(wd(r, 0)),
    "half_round": lambda r: (_pre_half(r, (HALF_A, HALF_B)), _assert(r[30] <= 56)),
    "round_pair": lambda r: (_pre_half(r, (HALF_A,)), _assert(r[30] <= 54)),
    "ext_u": lambda r: (_pre_state(r, U + 8, 510), _assert(r[30] in EXT_BASES)),
    "ext_m": lambda r: (_pre_state(r, U + 8, 510), _assert(r[30] in EXT_BASES)),
    "from_words": lambda r: _assert(all(x <= M32 for x in r[:8])),
    "to_mont": lambda r: _pre_to_mont(fe(r)),
    "to_canonical": lambda r: _assert(all(x * 100 < 247 * U for x in fe(r)) and val(fe(r)) < R),
    "permute": lambda r: _pre_state(r, U + 16, 120),
}


def _assert(c):
    assert c, "precondition"


# ---- judges: None, or a short text naming what is wrong ---------------------------------------------------------------------------
def _limbs_below(l, bound, what):
    for i in range(NL - 1):
        if l[i] >= bound:
            return "%s: limb %d = %#x not below %#x" % (what, i, l[i], bound)
    return None


def _first_diff(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "%s: first differing limb %d: got %#x want %#x" % (what, i, g, w)
    return None


def _judge_mont(a, b, out, masked):
    A, B = val(a), val(b)
    err = _limbs_below(out, U, "result")
    if err:
        return err
    if masked:       # the exact value is determined
        want = (A * B + ((-A * B * NINV_R) % R) * N) // R
        return _first_diff(out, limbs_of(want), "exact masked result")
    v = val(out)
    if (v - A * B * RINV) % N:
        return "not congruent to A*B/R"
    if v * R * 100 >= A * B * 100 + 801 * N * R:
        return "value not below A*B/R + 8.01N"
    return _first_diff(out, mont_columns(a, b, False)[0], "digit-rule transcription")


def _judge_sbox(a, out, masked):
    A, v = val(a), val(out)
    if (v - pow(A, 5, N) * pow(RINV, 4, N)) % N:
        return "not congruent to A^5 R^-4"
    if v * 10 >= (24 if masked else 127) * N:
        return "value %.3f N beyond the documented bound" % (v / N)
    return _limbs_below(out, U, "result")


def sbox_mont(A):
    return pow(A, 5, N) * pow(RINV, 4, N) % N


def _judge_half(rec, out):
    xin, Y, Z, idx = val(fe(rec)), wval(wd(rec, 10)), wval(wd(rec, 20)), rec[30]
    xo, Yo, Zo = fe(out), wd(out, 10), wd(out, 20)
    xp = wval(Yo) - 2 * Y - Z                       # the S-box output the kernel used, as an integer
    if xp < 0 or (xp - sbox_mont(xin)) % N or xp * 10 >= 127 * N:
        return "Y' - 2Y - Z is not an S-box output below 12.7N"
    if wval(Zo) != xp + Y + 3 * Z:
        return "Z' != x' + Y + 3Z"
    if val(xo) != 2 * xp + Y + Z + RCW_MONT[idx]:
        return "xin' != 2x' + Y + Z + c"
    for j in range(NW):                              # Y + S and 2Z + S with Y < 4W+64, Z < 5W+64, S < 10W+64
        if Yo[j] >= 14 * W + 128 or Zo[j] >= 20 * W + 192:
            return "wide limb %d beyond 14W / 20W" % j
    return _limbs_below(xo, 2 * U + 64, "xin'")


def _judge_pair(rec, out):
    xin, Y, Z, r = val(fe(rec)), wval(wd(rec, 10)), wval(wd(rec, 20)), rec[30]
    xo, Yo, Zo = fe(out), wd(out, 10), wd(out, 20)
    a = sbox_mont(xin)
    Y1, Z1, xb = a + 2 * Y + Z, a + Y + 3 * Z, 2 * a + Y + Z + RCW_MONT[r + 1]
    b = sbox_mont(xb)
    for name, got, want, tenths in (("Y", wval(Yo), b + 2 * Y1 + Z1, 186), ("Z", wval(Zo), b + Y1 + 3 * Z1, 206),
                                    ("xin", val(xo), 2 * b + Y1 + Z1 + RCW_MONT[r + 2], 302)):
        if (got - want) % N:
            return "%s not congruent to the two rounds of the specification" % name
        if got * 10 >= tenths * N:
            return "%s = %.3f N beyond %.1f N" % (name, got / N, tenths / 10)
    for j in range(NW):
        if Yo[j] >= 4 * W + 64 or Zo[j] >= 5 * W + 64:
            return "wide limb %d beyond 4W+64 / 5W+64" % j
    return _limbs_below(xo, 2 * U + 64, "xin")


def _judge_ext(rec, out, masked):
    base = rec[30]
    p = [sbox_mont(val(fe(rec, k)) + RC_MONT[base + k]) for k in range(3)]
    s = sum(p)
    for k in range(3):
        o = fe(out, k)
        if (val(o) - p[k] - s) % N:
            return "element %d not congruent to the round of the specification" % k
        if val(o) * 10 >= (96 if masked else 510) * N:
            return "element %d = %.3f N beyond its bound" % (k, val(o) / N)
        err = _limbs_below(o, U + 8, "element %d" % k)
        if err:
            return err
    return None


def canonical_state(rec):
    return tuple(val(fe(rec, k)) * RINV % N for k in range(3))


def _judge_permute(rec, out, want):
    for k in range(3):
        o = fe(out, k)
        if val(o) * RINV % N != want[k]:
            return "element %d: canonical form differs from the oracle's permutation" % k
        if val(o) * 10 >= 96 * N:
            return "element %d = %.3f N beyond 9.6N" % (k, val(o) / N)
        err = _limbs_below(o, U + 8, "element %d" % k)
        if err:
            return err
    return None


def _judge_reduce(w, out):
    v, o = wval(w), wval(out)
    if (o - v) % N or o >= 2 * N or o < 0:
        return "value %.4f N is not v mod N below 2N" % (o / N)
    for j in range(4):
        if out[j] >= W:
            return "limb %d = %#x not below 2^58" % (j, out[j])
    return None if out[4] < 1 << 24 else "top limb %#x not below 2^24" % out[4]


def judge(op, rec, out, oracle_perm=None):
    """rec, out: lists of 32 ints.  oracle_perm: the expected canonical state for permute (from the oracle)."""
    a, b = fe(rec), fe(rec, 1)
    o = fe(out)
    if op == "norm":
        return (val(o) != val(a) and "value changed") or _limbs_below(o, U + 8, "result")
    if op == "norm_full":
        return (val(o) != val(a) and "value changed") or _limbs_below(o, U, "result")
    if op == "add_lazy":
        return _first_diff(o, [x + y for x, y in zip(a, b)], "limb-wise sum")
    if op in ("mul_m", "mul_u"):
        return _judge_mont(a, b, o, op == "mul_m")
    if op in ("sqr_m", "sqr_u"):
        return _judge_mont(a, a, o, op == "sqr_m")
    if op in ("sbox_m", "sbox_u"):
        return _judge_sbox(a, o, op == "sbox_m")
    if op == "to_wide":
        got = wd(out, 0)
        return _first_diff(got, [a[2 * j] + (a[2 * j + 1] << 29) for j in range(4)] + [a[8]], "w[j] = l[2j] + l[2j+1] 2^29")
    if op == "from_wide":
        return (val(o) != wval(wd(rec, 0)) and "value changed") or _limbs_below(o, U, "result")
    if op == "reduce_wide":
        return _judge_reduce(wd(rec, 0), wd(out, 0))
    if op == "half_round":
        return _judge_half(rec, out)
    if op == "round_pair":
        return _judge_pair(rec, out)
    if op in ("ext_u", "ext_m"):
        return _judge_ext(rec, out, op == "ext_m")
    if op == "from_words":
        x = sum(w << (32 * i) for i, w in enumerate(rec[:8]))
        return (val(o) != x and "value changed") or _limbs_below(o, U, "result") or (o[8] >= 1 << 24 and "top limb beyond 24 bits") or None
    if op == "to_mont":
        v = val(o)
        return ((v - val(a) * R) % N and "not congruent to A*R") or (v >= 2 * N and "value not below 2N") or _limbs_below(o, U, "result")
    if op == "to_canonical":
        got = sum(w << (32 * i) for i, w in enumerate(out[:8]))
        want = val(a) * RINV % N
        return None if got == want else "got %#x want %#x" % (got, want)
    if op == "permute":
        return _judge_permute(rec, out, oracle_perm)
    raise KeyError(op)


# ---- case generators --------------------------------------------------------------------------------------------------------------
def lazy_limbs(x, limit):
    """x written with borrowed limbs: limb i takes one unit (2^29) of limb i+1 wherever that keeps every limb below limit."""
    l = limbs_of(x)
    for i in range(NL - 1):
        if l[i + 1] >= 1 and l[i] + U < limit:
            l[i] += U
            l[i + 1] -= 1
    assert val(l) == x
    return l


def inflate_wide(w):
    """The same value with every lower limb pushed towards 2^63 by borrowing up to 31 units from the limb above."""
    w = list(w)
    for j in range(NW - 1):
        b = min(w[j + 1], 31)
        w[j] += b << 58
        w[j + 1] -= b
    return w


def ripple_wide(w):
    """The writing that makes the estimate's t one short: a unit of the top limb is spread as 2^58-1 in limb 3 plus 2^58 in limb 2."""
    if w[4] < 1 or w[3] != 0:
        return None
    return [w[0], w[1], w[2] + W, MASK58, w[4] - 1]


def rec_of(*parts, index=None):
    r = []
    for p in parts:
        r += list(p)
    r += [0] * (REC - len(r))
    if index is not None:
        r[30] = index
    assert len(r) == REC
    return r


def fills(limit, top=None):
    """Structured limb fills below `limit` (exclusive); `top` replaces the top limb where the op bounds the value."""
    out = []
    for v in (0, 1, MASK, U, U + 7, limit - 1):
        if v < limit:
            out.append(("max" if v == limit - 1 else "fill", [v] * NL))
    out.append(("alt", [(limit - 1) if i % 2 == 0 else 0 for i in range(NL)]))
    out.append(("alt", [(limit - 1) if i % 2 else 0 for i in range(NL)]))
    if top is not None:
        out = [(f, l[:8] + [min(l[8], top)]) for f, l in out]
    return out


def top_for(tenths, slack):
    """Largest top limb that keeps a value below tenths/10 * N when the lower limbs add less than slack * 2^232."""
    return ((tenths * N // 10) >> 232) - slack


class Cases:
    def __init__(self):
        self.items = []          # (op, family, record)

    def add(self, op, family, rec):
        try:
            PRE[op](rec)
        except AssertionError as e:
            raise AssertionError("generator bug: %s/%s violates the op's preconditions: %s" % (op, family, e))
        self.items.append((op, family, rec))


def random_records(op, n, seed):
    """Seeded random records inside op's bounds, built with numpy only (the bulk device-against-host run uses large n)."""
    rng = np.random.default_rng([seed, OP_ID[op]])
    r = np.zeros((n, REC), dtype=np.uint32)

    def limbs(count, low_limit, top_limit, tight=True):
        # per record, the lower-limb bound is the op's own or (a third of the time each) U or 2U where that is smaller
        lim = np.full((count, 1), low_limit, dtype=np.int64)
        if tight:
            pick = rng.integers(0, 3, size=(count, 1))
            lim = np.where(pick == 1, min(U, low_limit), np.where(pick == 2, min(2 * U, low_limit), lim))
        a = (rng.random((count, NL)) * lim).astype(np.int64)
        a = np.minimum(a, lim - 1)
        a[:, 8] = rng.integers(0, top_limit, size=count)
        return a.astype(np.uint32)

    def wides(count, limit, top_limit):
        w = rng.integers(0, limit, size=(count, NW), dtype=np.uint64)
        w[:, 4] = rng.integers(0, top_limit, size=count, dtype=np.uint64)
        out = np.zeros((count, 2 * NW), dtype=np.uint32)
        out[:, 0::2] = (w & np.uint64(M32)).astype(np.uint32)
        out[:, 1::2] = (w >> np.uint64(32)).astype(np.uint32)
        return out

    if op in ("norm", "norm_full"):
        r[:, :9] = limbs(n, M32 - 7, 1 << 31)
    elif op == "add_lazy":
        r[:, :9] = limbs(n, 1 << 31, 1 << 31)
        r[:, 9:18] = limbs(n, 1 << 31, 1 << 31)
    elif op == "mul_m":
        r[:, :9] = limbs(n, 2469 * U // 1000, 2469 * U // 1000)
        r[:, 9:18] = limbs(n, 2469 * U // 1000, 2469 * U // 1000)
    elif op == "mul_u":
        r[:, :9] = limbs(n, 202 * U // 100, 202 * U // 100)
        r[:, 9:18] = limbs(n, 202 * U // 100, 202 * U // 100)
    elif op == "sqr_m":
        r[:, :9] = limbs(n, 247 * U // 100, 247 * U // 100)
    elif op == "sqr_u":
        r[:, :9] = limbs(n, 202 * U // 100, 202 * U // 100)
    elif op in ("sbox_m", "sbox_u"):
        r[:, :9] = limbs(n, 202 * U // 100, top_for(600, 3))
    elif op == "to_wide":
        r[:, :9] = limbs(n, 1 << 32, 1 << 32)
    elif op == "from_wide":
        r[:, :10] = wides(n, W, 1 << 32)
    elif op == "reduce_wide":
        r[:, :10] = wides(n, 1 << 63, 95 * 3172003 - 40)     # t below 95 * 2^32/1354: the estimate stays below 96, the value below 96N
    elif op in ("half_round", "round_pair"):
        entry_b = (rng.integers(0, 2, size=n) == 1) if op == "half_round" else np.zeros(n, dtype=bool)
        xa, xb = limbs(n, 2 * U + 64, top_for(302, 3), tight=False), limbs(n, 2 * U + 64, top_for(596, 3), tight=False)
        r[:, :9] = np.where(entry_b[:, None], xb, xa)
        r[:, 10:20] = np.where(entry_b[:, None], wides(n, W, top_for(20, 2)), wides(n, 4 * W + 64, top_for(186, 6)))
        r[:, 20:30] = np.where(entry_b[:, None], wides(n, W, top_for(20, 2)), wides(n, 5 * W + 64, top_for(206, 7)))
        r[:, 30] = rng.integers(0, 57 if op == "half_round" else 55, size=n)
    elif op in ("ext_u", "ext_m"):
        for k in range(3):
            r[:, 9 * k:9 * k + 9] = limbs(n, U + 8, top_for(510, 2), tight=False)
        r[:, 30] = np.array(EXT_BASES, dtype=np.uint32)[rng.integers(0, 8, size=n)]
    elif op == "from_words":
        r[:, :8] = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    elif op == "to_mont":
        r[:, :9] = limbs(n, U + 8, (1 << 24) + 8, tight=False)
    elif op == "to_canonical":
        r[:, :9] = limbs(n, 247 * U // 100, U - 3)
    elif op == "permute":
        for k in range(3):
            r[:, 9 * k:9 * k + 9] = limbs(n, U + 16, top_for(120, 2), tight=False)
    else:
        raise KeyError(op)
    return r


def _mult_n_values(limit_value):
    k = 0
    while k * N - 1 < limit_value:
        for d in (-1, 0, 1):
            if 0 <= k * N + d < limit_value:
                yield k, k * N + d
        k += 1


def build_cases(n_random):
    """n_random: {op: count} of seeded random cases judged by the model.  Returns Cases."""
    c = Cases()
    L247, L202, L5 = 247 * U // 100, 202 * U // 100, 5 * U
    some_b = limbs_of(0x1234567 * R % N)                       # an ordinary normalised operand

    # -- one-operand limb shuffles
    for op, lim in (("norm", 1 << 32), ("norm_full", M32 - 7), ("to_wide", 1 << 32)):
        for fam, l in fills(lim, top=(1 << 31) - 1 if op != "to_wide" else None):
            c.add(op, fam, rec_of(l))
        for i in range(NL):
            hot = [0] * NL
            hot[i] = min(lim - 1, (1 << 31) - 1) if i == 8 and op != "to_wide" else lim - 1
            c.add(op, "hot", rec_of(hot))
    for fam, l in fills(1 << 31):
        c.add("add_lazy", fam, rec_of(l, l))
    c.add("add_lazy", "max", rec_of([M32] * NL, [0] * NL))
    c.add("add_lazy", "max", rec_of([M32 - 5] * NL, [5] * NL))
    for i in range(NL):
        hot = [0] * NL
        hot[i] = M32 - MASK
        c.add("add_lazy", "hot", rec_of(hot, [MASK] * NL))

    # -- the Montgomery products: limb fills at the column budget, every column alone, the digit extremes, multiples of N
    for op, masked, square in (("mul_m", True, False), ("mul_u", False, False), ("sqr_m", True, True), ("sqr_u", False, True)):
        # limb bound with both operands equal: 2.47^2 is just beyond 6.1, so a masked product stops at 2.469U
        own = (L247 if square else 2469 * U // 1000) if masked else L202
        prod = (6100 if masked else 4088) * U * U // 1000      # La * Lb strictly below this (fr_gfx950.hpp: 6.1 U^2 / 4.088 U^2)
        for fam, l in fills(own):
            c.add(op, fam, rec_of(l, [] if square else l))
        if not square:
            for fam, l in fills(own):
                c.add(op, fam, rec_of(l, some_b))
                c.add(op, fam, rec_of(some_b, l))
            for la in (L5 - 1, 4 * U, 3 * U + 1):              # uneven split of the product bound, each limb below 5U
                lb = (prod - 1) // la
                c.add(op, "max", rec_of([la] * NL, [lb] * NL))
                c.add(op, "max", rec_of([lb] * NL, [la] * NL))
        for i in range(NL):                                    # one hot limb against a full operand: every column hit alone
            if square:
                hot = [0] * NL
                hot[i] = own - 1
                c.add(op, "hot", rec_of(hot))
                cold = [own - 1] * NL
                cold[i] = 0
                c.add(op, "hot", rec_of(cold))
            else:
                la = L5 - 1
                hot = [0] * NL
                hot[i] = la
                full = [(prod - 1) // la] * NL
                c.add(op, "hot", rec_of(hot, full))
                c.add(op, "hot", rec_of(full, hot))
        # quotient digits: A = 1, B = N: every masked digit is MASK; A * B = R: every digit zero
        one, two116, two145 = limbs_of(1), limbs_of(1 << 116), limbs_of(1 << 145)
        if square:
            c.add(op, "digits", rec_of(limbs_of(0)))
            c.add(op, "digits", rec_of(limbs_of(1)))
            c.add(op, "digits", rec_of(limbs_of(1 << 232)))    # A^2 = 2^464 = 0 mod R
            c.add(op, "digits", rec_of(limbs_of(N)))
            c.add(op, "digits", rec_of(limbs_of(R - 1)))
        else:
            c.add(op, "digits", rec_of(one, N_LIMBS))
            c.add(op, "digits", rec_of(N_LIMBS, one))
            c.add(op, "digits", rec_of(two116, two145))        # 2^261 = R
            c.add(op, "digits", rec_of(limbs_of(0), [own - 1] * NL))
            c.add(op, "digits", rec_of(limbs_of(R - 1), limbs_of(R - 1)))
        for k, x in _mult_n_values(R):
            for l in (limbs_of(x), lazy_limbs(x, own)):
                c.add(op, "multN", rec_of(l, [] if square else some_b))
            if not square and k % 8 == 0:
                c.add(op, "multN", rec_of(some_b, lazy_limbs(x, own)))
                c.add(op, "multN", rec_of(limbs_of(x), limbs_of(x)))

    # -- S-box: limbs at 2.02U with the value at 60N, multiples of N below 60N
    top60 = top_for(600, 3)
    for op in ("sbox_m", "sbox_u"):
        for fam, l in fills(L202, top=top60):
            c.add(op, fam, rec_of(l))
        c.add(op, "max", rec_of(limbs_of(60 * N - 1)))
        c.add(op, "max", rec_of(lazy_limbs(60 * N - 1, L202)))
        for i in range(NL):
            hot = [0] * NL
            hot[i] = top60 if i == 8 else L202 - 1
            c.add(op, "hot", rec_of(hot))
        for k, x in _mult_n_values(60 * N):
            c.add(op, "multN", rec_of(limbs_of(x)))
            c.add(op, "multN", rec_of(lazy_limbs(x, L202)))

    # -- wide limbs
    for v in (0, 1, MASK58, N, 2 * N - 1, R - 1, (1 << 264) - 1):
        c.add("from_wide", "fill", rec_of(put_wide(wide_of(v))))
    c.add("from_wide", "max", rec_of(put_wide([MASK58] * 4 + [M32])))
    for j in range(NW):
        hot = [0] * NW
        hot[j] = M32 if j == 4 else MASK58
        c.add("from_wide", "hot", rec_of(put_wide(hot)))
    c.add("from_wide", "alt", rec_of(put_wide([MASK58, 0, MASK58, 0, M32])))
    c.add("from_wide", "alt", rec_of(put_wide([0, MASK58, 0, MASK58, 0])))

    # -- reduce_wide: every table row from both sides, the steps of the estimate, three writings of each value
    def reduce_value(v, fam):
        w = wide_of(v)
        for cand in (w, inflate_wide(w), ripple_wide(w)):
            if cand is not None and wval(cand) < QTAB_ROWS * N and reduce_estimate(cand) < QTAB_ROWS:
                c.add("reduce_wide", fam, rec_of(put_wide(cand)))

    for q in range(QTAB_ROWS):
        for d in (0, 1, N - 1):
            reduce_value(q * N + d, "q")
    for q in range(1, QTAB_ROWS):
        t = -(-(q << 32) // 1354)                  # the smallest t whose estimate is q
        for tt in (t - 1, t, q * 3171408 - 1, q * 3171408):
            for low in (0, 1, (1 << 232) - 1, MASK58 << 116):
                if (tt << 232) + low < QTAB_ROWS * N:
                    reduce_value((tt << 232) + low, "q")
    for v in (0, 1, W, (1 << 232) - 1, 1 << 232):
        reduce_value(v, "fill")
    top95 = 95 * 3172003 - 40
    c.add("reduce_wide", "max", rec_of(put_wide([(1 << 63) - 1] * 4 + [top95])))
    c.add("reduce_wide", "alt", rec_of(put_wide([(1 << 63) - 1, 0, (1 << 63) - 1, 0, top95])))
    c.add("reduce_wide", "alt", rec_of(put_wide([0, (1 << 63) - 1, 0, (1 << 63) - 1, 0])))
    for j in range(NW):
        hot = [0] * NW
        hot[j] = top95 if j == 4 else (1 << 63) - 1
        c.add("reduce_wide", "hot", rec_of(put_wide(hot)))

    # -- the rounds: the fixed-point worst case of the comments, zero, every index
    def lazy_wide(tenths, limb_limit):
        """A value just under tenths/10 N written with every lower limb at limb_limit - 1."""
        target = tenths * N // 10 - 1
        low = sum((limb_limit - 1) << (58 * j) for j in range(4))
        return [limb_limit - 1] * 4 + [(target - low) >> 232]

    def lazy_fe(tenths, limb_limit):
        target = tenths * N // 10 - 1
        low = sum((limb_limit - 1) << (29 * i) for i in range(8))
        return [limb_limit - 1] * 8 + [(target - low) >> 232]

    worst_a = (lazy_fe(302, 2 * U + 64), lazy_wide(186, 4 * W + 64), lazy_wide(206, 5 * W + 64))
    worst_a_norm = (limbs_of(302 * N // 10 - 1), wide_of(186 * N // 10 - 1), wide_of(206 * N // 10 - 1))
    worst_b = (lazy_fe(596, 2 * U + 64), wide_of(2 * N - 1), wide_of(2 * N - 1))
    worst_b_lazy = (limbs_of(596 * N // 10 - 1), [MASK58] * 4 + [(2 * N - 1 >> 232) - 1], [MASK58] * 4 + [(2 * N - 1 >> 232) - 1])
    first_pair = (lazy_fe(106, 2 * U + 8), wide_of(96 * N // 10 - 1), wide_of(96 * N // 10 - 1))
    zero = ([0] * NL, [0] * NW, [0] * NW)

    def round_rec(state, idx):
        return rec_of(state[0], [0], put_wide(state[1]), put_wide(state[2]), index=idx)

    for idx in range(57):
        for st in (worst_a, worst_b):
            c.add("half_round", "index", round_rec(st, idx))
        c.add("half_round", "zero", round_rec(zero, idx))
    for st in (worst_a, worst_a_norm, worst_b, worst_b_lazy, first_pair):
        for idx in (0, 1, 55, 56):
            c.add("half_round", "worst", round_rec(st, idx))
    for r in range(55):
        c.add("round_pair", "index", round_rec(worst_a, r))
        c.add("round_pair", "zero", round_rec(zero, r))
    for st in (worst_a, worst_a_norm, first_pair):
        for r in (0, 2, 26, 54):
            c.add("round_pair", "worst", round_rec(st, r))
    for op in ("half_round", "round_pair"):      # x alone, Y alone, Z alone at the worst case
        for keep in range(3):
            st = tuple(worst_a[k] if k == keep else zero[k] for k in range(3))
            c.add(op, "hot", round_rec(st, 4))

    top51 = top_for(510, 2)
    for op in ("ext_u", "ext_m"):
        for base in EXT_BASES:
            for v in (0, 1, MASK, U, U + 7):
                l = [v] * 8 + [min(v, top51)]
                c.add(op, "zero" if v == 0 else "fill", rec_of(l, l, l, index=base))
            worst = [U + 7] * 8 + [top51]
            c.add(op, "worst", rec_of(worst, worst, worst, index=base))
            c.add(op, "index", rec_of(limbs_of(51 * N - 1), limbs_of(N), limbs_of(50 * N + 1), index=base))
            for keep in range(3):
                c.add(op, "hot", rec_of(*[worst if k == keep else [0] * NL for k in range(3)], index=base))

    # -- conversions
    for v in (0, 1, N - 1, N, N + 1, (1 << 256) - 1, (1 << 255), (1 << 232) - 1, 1 << 232):
        c.add("from_words", "fill", rec_of([(v >> (32 * i)) & M32 for i in range(8)]))
    c.add("from_words", "max", rec_of([M32] * 8))
    for i in range(8):
        c.add("from_words", "hot", rec_of([M32 if j == i else 0 for j in range(8)]))
        c.add("from_words", "hot", rec_of([0 if j == i else M32 for j in range(8)]))
    for b in range(256):                           # every single bit: each limb border of from_words
        c.add("from_words", "alt", rec_of([((1 << b) >> (32 * i)) & M32 for i in range(8)]))
    for fam, l in fills(U + 8, top=(1 << 24) + 7):
        c.add("to_mont", fam, rec_of(l))
    for i in range(NL):
        hot = [0] * NL
        hot[i] = (1 << 24) + 7 if i == 8 else U + 7
        c.add("to_mont", "hot", rec_of(hot))
    for k, x in _mult_n_values(1 << 256):
        c.add("to_mont", "multN", rec_of(limbs_of(x)))
    for fam, l in fills(L247, top=U - 3):
        c.add("to_canonical", fam, rec_of(l))
    for i in range(NL):
        hot = [0] * NL
        hot[i] = U - 3 if i == 8 else L247 - 1
        c.add("to_canonical", "hot", rec_of(hot))
    c.add("to_canonical", "max", rec_of(limbs_of(R - 1)))
    for k, x in _mult_n_values(R):                 # k N is the c == N branch: must come out 0, its neighbours +-R^-1
        c.add("to_canonical", "multN", rec_of(limbs_of(x)))
        c.add("to_canonical", "multN", rec_of(lazy_limbs(x, L247)))

    # -- permute: Montgomery-domain states at the edge of its input bound
    top12 = top_for(120, 2)
    edge = [U + 15] * 8
    small = limbs_of(R % N)
    for k in range(12):
        for pos in range(3):
            for l in (limbs_of(k * N), limbs_of(k * N + 1), limbs_of(k * N + 5), edge + [max(0, ((k + 1) * N >> 232) - 2)]):
                st = [small, small, small]
                st[pos] = l
                c.add("permute", "edge", rec_of(*st))
        l = edge + [max(0, ((k + 1) * N >> 232) - 2)]
        c.add("permute", "edge", rec_of(l, l, l))
    c.add("permute", "zero", rec_of([0] * NL, [0] * NL, [0] * NL))
    c.add("permute", "max", rec_of(edge + [top12], edge + [top12], edge + [top12]))
    for v in (1, MASK, U, U + 7):
        l = [v] * 8 + [min(v, top12)]
        c.add("permute", "fill", rec_of(l, l, l))

    # -- seeded random limbs inside each op's bound
    for op in OPS:
        for rec in random_records(op, n_random[op], 20261017).tolist():
            c.add(op, "random", rec)
    return c


# which families every op must have (test_plan)
PLAN = {
    "norm": ("fill", "max", "hot", "alt", "random"), "norm_full": ("fill", "max", "hot", "alt", "random"),
    "add_lazy": ("fill", "max", "hot", "alt", "random"), "to_wide": ("fill", "max", "hot", "alt", "random"),
    "mul_m": ("fill", "max", "hot", "alt", "digits", "multN", "random"), "mul_u": ("fill", "max", "hot", "alt", "digits", "multN", "random"),
    "sqr_m": ("fill", "max", "hot", "alt", "digits", "multN", "random"), "sqr_u": ("fill", "max", "hot", "alt", "digits", "multN", "random"),
    "sbox_m": ("fill", "max", "hot", "alt", "multN", "random"), "sbox_u": ("fill", "max", "hot", "alt", "multN", "random"),
    "from_wide": ("fill", "max", "hot", "alt", "random"), "reduce_wide": ("fill", "max", "hot", "alt", "q", "random"),
    "half_round": ("worst", "zero", "index", "hot", "random"), "round_pair": ("worst", "zero", "index", "hot", "random"),
    "ext_u": ("fill", "worst", "zero", "index", "hot", "random"), "ext_m": ("fill", "worst", "zero", "index", "hot", "random"),
    "from_words": ("fill", "max", "hot", "alt", "random"), "to_mont": ("fill", "max", "hot", "alt", "multN", "random"),
    "to_canonical": ("fill", "max", "hot", "alt", "multN", "random"), "permute": ("fill", "max", "zero", "edge", "random"),
}


def to_sections(items):
    """Group (op, family, record) by op, keeping order: [(op, [families], uint32 array (n, 32))]."""
    out = []
    for op in OPS:
        sel = [(f, r) for o, f, r in items if o == op]
        if sel:
            out.append((op, [f for f, _ in sel], np.array([r for _, r in sel], dtype=np.uint64).astype(np.uint32)))
    return out


def write_case_file(path, sections):
    with open(path, "wb") as f:
        for op, _, arr in sections:
            f.write(np.array([OP_ID[op], arr.shape[0]], dtype=np.uint32).tobytes())
            f.write(np.ascontiguousarray(arr, dtype=np.uint32).tobytes())


def read_result_file(path, sections):
    data = np.fromfile(path, dtype=np.uint32)
    assert data.size == sum(arr.size for _, _, arr in sections), "result file has the wrong size"
    out, at = [], 0
    for _, _, arr in sections:
        out.append(data[at:at + arr.size].reshape(arr.shape))
        at += arr.size
    return out


def judge_sections(sections, results, oracle_permute):
    """oracle_permute(list of canonical states) -> list of expected canonical states.  Returns (judged, failures) with failures as
    'op/family case i: what'."""
    failures, judged = [], 0
    for (op, fams, arr), res in zip(sections, results):
        if res is None:          # the host twin aborted on this op: reported by run_host_twin
            continue
        recs, outs = arr.tolist(), res.tolist()
        want = oracle_permute([canonical_state(r) for r in recs]) if op == "permute" else [None] * len(recs)
        for i, (rec, out) in enumerate(zip(recs, outs)):
            err = judge(op, rec, out, want[i])
            judged += 1
            if err:
                failures.append("%s/%s case %d: %s" % (op, fams[i], i, err))
    return judged, failures


# ---- running the host twin (tests/device_check/fr_unit_host.cpp) --------------------------------------------------------------------
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
PLAIN = ("-O2",)


def build_host_twin(exe, flags=SANITIZE):
    import subprocess
    subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, os.path.join(ROOT, "tests", "device_check", "fr_unit_host.cpp")])
    return exe


def run_host_twin(exe, sections, workdir, tag="cases"):
    """Runs every section through the host twin, one process per op, so that a bound violation or a shadow-accumulator trap
    (which aborts the twin) is charged to its op, family and case and hides no other op.  Returns (results, aborts): the result
    array of each section (None where the twin aborted) and one line per abort."""
    import subprocess
    results, aborts = [], []
    for op, fams, arr in sections:
        cases, out = os.path.join(str(workdir), "%s_%s.bin" % (tag, op)), os.path.join(str(workdir), "%s_%s.out" % (tag, op))
        write_case_file(cases, [(op, fams, arr)])
        r = subprocess.run([exe, cases, out], capture_output=True, text=True, timeout=1800)
        if r.returncode == 0 and "no bound violations" in r.stdout:
            results.append(read_result_file(out, [(op, fams, arr)])[0])
            os.remove(cases)
            os.remove(out)
            continue
        m = re.search(r"ABORTED in op (\d+) case (\d+)", r.stderr)
        where = "%s/%s case %s" % (op, fams[int(m.group(2))] if fams else "random", m.group(2)) if m else op
        aborts.append("%s: host twin exit %d: %s" % (where, r.returncode, " | ".join(r.stderr.strip().splitlines()[:3])))
        results.append(None)
    return results, aborts


def oracle_permute_both(states):
    """Expected canonical states from the Python restatement of the specification AND the C oracle (they must agree)."""
    from oracle import c_oracle, poseidon2_ref
    want = [tuple(poseidon2_ref.permutation(s)) for s in states]
    if states:
        flat = c_oracle.felts_to_array([v for s in states for v in s]).reshape(-1, 96)
        got = c_oracle.array_to_felts(c_oracle.permute_batch(flat, threads=4))
        assert [tuple(got[3 * i:3 * i + 3]) for i in range(len(states))] == want, "the two oracles disagree"
    return want


# Random cases judged by the model, per op (the counts and what they cost are in the header of tests/test_fr_unit_cpu.py)
N_RANDOM = {op: 2000 for op in OPS}
BULK_RANDOM = {op: 1 << 18 for op in OPS}     # device against host twin, word for word: no big-int work
BULK_RANDOM["permute"] = 1 << 16
BULK_RANDOM["round_pair"] = 1 << 17
