// input.json text -> the field elements SampleAndProve reads (include/codex_p2.h: cp2_proof_input_parse_json), host only.
// No HIP, no library calls: tests/host_check/json_parse_check.cpp builds it alone under AddressSanitizer + UBSan.
//
// Accepted: any JSON whitespace and key order; every number a quoted decimal string or a bare non-negative integer.
// Refused, with a message that names the key (and row / column): a missing, unknown or repeated key, an array of the wrong
// length, a field element >= r, a sign, a non-digit, an escape in a key, trailing text, and any truncation.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace cp2parse {

// r of BN254, little-endian 64-bit limbs
constexpr uint64_t R_LIMBS[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};

// cp2_felts_per_bytes: cell bytes, the 0x01 marker, zero padding to 31-byte chunks (Slot.hs:243-270)
inline size_t felts_per_bytes(size_t len) { return (len + 1 + 30) / 31; }

struct Parsed {
  uint8_t dataset_root[32], entropy[32], slot_root[32];
  uint64_t n_cells = 0, n_slots = 0, slot_idx = 0;   // as read: a shape failure is the verifier's to report
  size_t n_samples = 0;
  std::vector<uint8_t> slot_proof;   // max_log2_nslots x 32
  std::vector<uint8_t> cell_felts;   // n_samples x nf x 32
  std::vector<uint8_t> paths;        // n_samples x max_depth x 32
};

// Decode one cellData row (nf felts) back into the cell_size bytes it encodes: true when every felt is < 2^248 and the
// 0x01 marker and zero padding sit where cp2_bytes_to_felts puts them.
inline bool felts_to_cell_bytes(const uint8_t* felts, size_t nf, size_t cell_size, uint8_t* out) {
  if (nf != felts_per_bytes(cell_size)) return false;
  for (size_t k = 0; k < nf; ++k) {
    const uint8_t* f = felts + 32 * k;
    if (f[31] != 0) return false;
    for (size_t b = 0; b < 31; ++b) {
      const size_t at = 31 * k + b;
      if (at < cell_size) out[at] = f[b];
      else if (f[b] != (at == cell_size ? 1 : 0)) return false;
    }
  }
  return true;
}

class Parser {
 public:
  Parser(const char* s, size_t n, std::string* err) : s_(s), n_(n), err_(err) {}

  // cfg values: md = maxDepth, m = maxLog2NSlots, nf = felts per cell row, ns = rows (0: as many as the text has)
  bool parse(size_t md, size_t m, size_t nf, size_t ns, Parsed& out) {
    enum { K_DROOT, K_ENT, K_NCELLS, K_NSLOTS, K_SIDX, K_SROOT, K_SPROOF, K_CELLS, K_PATHS, NKEYS };
    static const char* const NAMES[NKEYS] = {"dataSetRoot", "entropy", "nCellsPerSlot", "nSlotsPerDataSet", "slotIndex",
                                             "slotRoot", "slotProof", "cellData", "merklePaths"};
    bool seen[NKEYS] = {};
    size_t rows_cells = 0, rows_paths = 0;
    ws();
    if (!expect('{', "the text: expected '{'")) return false;
    ws();
    if (peek() == '}') return fail("the text: no keys");
    for (;;) {
      std::string key;
      ws();
      if (!read_key(key)) return false;
      int k = -1;
      for (int j = 0; j < NKEYS; ++j)
        if (key == NAMES[j]) k = j;
      if (k < 0) return fail("unknown key \"" + key + "\"");
      if (seen[k]) return fail("repeated key \"" + key + "\"");
      seen[k] = true;
      ws();
      if (!expect(':', key + ": expected ':'")) return false;
      ws();
      bool ok = true;
      switch (k) {
        case K_DROOT: ok = felt(out.dataset_root, key); break;
        case K_ENT: ok = felt(out.entropy, key); break;
        case K_SROOT: ok = felt(out.slot_root, key); break;
        case K_NCELLS: ok = u64(&out.n_cells, key); break;
        case K_NSLOTS: ok = u64(&out.n_slots, key); break;
        case K_SIDX: ok = u64(&out.slot_idx, key); break;
        case K_SPROOF: ok = felt_list(out.slot_proof, m, key); break;
        case K_CELLS: ok = felt_matrix(out.cell_felts, ns, nf, key, &rows_cells); break;
        case K_PATHS: ok = felt_matrix(out.paths, ns, md, key, &rows_paths); break;
      }
      if (!ok) return false;
      ws();
      if (peek() == ',') { ++i_; continue; }
      if (peek() == '}') { ++i_; break; }
      return fail(key + ": expected ',' or '}' after the value");
    }
    ws();
    if (i_ != n_) return fail("trailing text after the closing '}'");
    for (int j = 0; j < NKEYS; ++j)
      if (!seen[j]) return fail(std::string("missing key \"") + NAMES[j] + "\"");
    if (rows_cells != rows_paths)
      return fail("merklePaths: " + std::to_string(rows_paths) + " rows, cellData has " + std::to_string(rows_cells));
    out.n_samples = rows_cells;
    return true;
  }

 private:
  const char* s_;
  size_t n_, i_ = 0;
  std::string* err_;

  int peek() const { return i_ < n_ ? (unsigned char)s_[i_] : -1; }
  void ws() {
    while (i_ < n_ && (s_[i_] == ' ' || s_[i_] == '\t' || s_[i_] == '\n' || s_[i_] == '\r')) ++i_;
  }
  bool fail(const std::string& what) {
    if (err_ && err_->empty()) *err_ = what + (i_ < n_ ? " (byte " + std::to_string(i_) + ")" : " (end of text)");
    return false;
  }
  bool expect(char c, const std::string& what) {
    if (peek() != (unsigned char)c) return fail(what);
    ++i_;
    return true;
  }
  bool read_key(std::string& key) {
    if (peek() != '"') return fail("expected a key in quotes");
    ++i_;
    const size_t a = i_;
    while (i_ < n_ && s_[i_] != '"') {
      if (s_[i_] == '\\') return fail("escape in a key");
      ++i_;
    }
    if (i_ >= n_) return fail("unterminated key");
    key.assign(s_ + a, i_ - a);
    ++i_;
    return true;
  }
  // a non-negative integer below 2^256, quoted or bare
  bool number(uint64_t (&w)[4], const std::string& where) {
    w[0] = w[1] = w[2] = w[3] = 0;
    const bool quoted = peek() == '"';
    if (quoted) ++i_;
    if (peek() == '-' || peek() == '+') return fail(where + ": a sign");
    size_t digits = 0;
    while (i_ < n_ && s_[i_] >= '0' && s_[i_] <= '9') {
      unsigned __int128 carry = (unsigned)(s_[i_] - '0');
      for (int k = 0; k < 4; ++k) {
        const unsigned __int128 v = (unsigned __int128)w[k] * 10u + carry;
        w[k] = (uint64_t)v;
        carry = v >> 64;
      }
      if (carry) return fail(where + ": more than 256 bits");
      ++i_;
      ++digits;
    }
    if (i_ >= n_) return fail(where + ": truncated number");
    if (!digits) return fail(where + ": not a decimal digit");
    if (quoted) {
      if (s_[i_] != '"') return fail(where + ": not a decimal digit");
      ++i_;
    } else if (s_[i_] != ',' && s_[i_] != ']' && s_[i_] != '}' && s_[i_] != ' ' && s_[i_] != '\t' && s_[i_] != '\n' && s_[i_] != '\r') {
      return fail(where + ": not a decimal digit");
    }
    return true;
  }
  bool felt(uint8_t* out, const std::string& where) {
    uint64_t w[4];
    if (!number(w, where)) return false;
    bool ge = true;   // w >= r ?
    for (int k = 3; k >= 0; --k) {
      if (w[k] != R_LIMBS[k]) { ge = w[k] > R_LIMBS[k]; break; }
    }
    if (ge) return fail(where + ": field element >= r");
    std::memcpy(out, w, 32);   // little-endian host
    return true;
  }
  bool u64(uint64_t* out, const std::string& where) {
    uint64_t w[4];
    if (!number(w, where)) return false;
    if (w[1] | w[2] | w[3]) return fail(where + ": does not fit 64 bits");
    *out = w[0];
    return true;
  }
  // "[ x, y, ... ]" of exactly `count` field elements, appended to out
  bool felt_list(std::vector<uint8_t>& out, size_t count, const std::string& where) {
    if (!expect('[', where + ": expected '['")) return false;
    ws();
    size_t got = 0;
    if (peek() == ']') {
      ++i_;
    } else {
      for (;;) {
        if (got == count) return fail(where + ": more than " + std::to_string(count) + " entries");
        uint8_t f[32];
        ws();
        if (!felt(f, where + " column " + std::to_string(got))) return false;
        out.insert(out.end(), f, f + 32);
        ++got;
        ws();
        if (peek() == ',') { ++i_; continue; }
        if (peek() == ']') { ++i_; break; }
        return fail(where + ": expected ',' or ']'");
      }
    }
    if (got != count) return fail(where + ": " + std::to_string(got) + " entries, expected " + std::to_string(count));
    return true;
  }
  // "[ row, row, ... ]": `rows` rows (0: any number) of `cols` field elements
  bool felt_matrix(std::vector<uint8_t>& out, size_t rows, size_t cols, const std::string& where, size_t* got_rows) {
    if (!expect('[', where + ": expected '['")) return false;
    ws();
    size_t got = 0;
    if (peek() == ']') {
      ++i_;
    } else {
      for (;;) {
        if (rows && got == rows) return fail(where + ": more than " + std::to_string(rows) + " rows");
        ws();
        if (!felt_list(out, cols, where + " row " + std::to_string(got))) return false;
        ++got;
        ws();
        if (peek() == ',') { ++i_; continue; }
        if (peek() == ']') { ++i_; break; }
        return fail(where + ": expected ',' or ']'");
      }
    }
    if (rows && got != rows) return fail(where + ": " + std::to_string(got) + " rows, expected " + std::to_string(rows));
    *got_rows = got;
    return true;
  }
};

inline bool parse_proof_input(const char* text, size_t len, size_t max_depth, size_t max_log2_nslots, size_t cell_size,
                              size_t n_samples, Parsed& out, std::string* err) {
  out = Parsed();
  Parser p(text, len, err);
  return p.parse(max_depth, max_log2_nslots, felts_per_bytes(cell_size), n_samples, out);
}

}  // namespace cp2parse
