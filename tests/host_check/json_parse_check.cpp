// The input.json reader (csrc/json_parse.hpp) on the CPU under AddressSanitizer + UBSan: random proof inputs written by the
// byte-exact writer (csrc/json_text.hpp, text_head + text_body_felts) parse back to the same field elements, every prefix of a
// text that lacks its closing brace is refused with a message, and texts with random bytes overwritten are refused or parsed
// without a report.
// Prints "json parse ok: <n> round trips, <m> prefixes" on success.  No GPU, no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "json_parse.hpp"
#include "json_text.hpp"

// the two library functions json_text.hpp refers to, restated (cp2_bytes_to_felts is not reached by text_body_felts)
extern "C" size_t cp2_felts_per_bytes(size_t len) { return cp2parse::felts_per_bytes(len); }
extern "C" int cp2_bytes_to_felts(const uint8_t*, size_t, uint8_t*) { std::abort(); }

static std::mt19937_64 rng(20261016);

static void random_felt(uint8_t* out) {   // uniform-ish below r: the top limb below r's
  uint64_t w[4] = {rng(), rng(), rng(), rng() % cp2parse::R_LIMBS[3]};
  switch (rng() % 6) {                   // small values and the edges show up too
    case 0: w[1] = w[2] = w[3] = 0; w[0] %= 1000; break;
    case 1: std::memcpy(w, cp2parse::R_LIMBS, 32); w[0] -= 1; break;
    default: break;
  }
  std::memcpy(out, w, 32);
}

int main(int argc, char** argv) {
  const int trips = argc > 1 ? std::atoi(argv[1]) : 300;
  size_t prefixes = 0;
  int bad = 0;
  for (int it = 0; it < trips; ++it) {
    cp2_config cfg{};
    cfg.max_depth = 1 + (int)(rng() % 12);
    cfg.max_log2_nslots = 1 + (int)(rng() % 6);
    cfg.cell_size = 1 + rng() % 200;
    cfg.n_cells = rng() % 3 == 0 ? rng() : (1ULL << (rng() % 20));
    cfg.n_slots = rng() % 300;
    const size_t ns = 1 + rng() % 5, nf = cp2parse::felts_per_bytes(cfg.cell_size), md = (size_t)cfg.max_depth,
                 m = (size_t)cfg.max_log2_nslots;
    cfg.n_samples = ns;
    const uint64_t slot = rng() % 1000;
    uint8_t droot[32], ent[32], sroot[32];
    random_felt(droot);
    random_felt(ent);
    random_felt(sroot);
    std::vector<uint8_t> proof(m * 32), felts(ns * nf * 32), paths(ns * md * 32);
    for (size_t i = 0; i < m; ++i) random_felt(&proof[i * 32]);
    for (size_t i = 0; i < ns * nf; ++i) random_felt(&felts[i * 32]);
    for (size_t i = 0; i < ns * md; ++i) random_felt(&paths[i * 32]);
    std::string text;
    cp2text::text_head(text, cfg, slot, droot, ent, sroot, proof.data());
    cp2text::text_body_felts(text, cfg, ns, felts.data(), paths.data());

    cp2parse::Parsed p;
    std::string err;
    const size_t want_ns = rng() % 2 ? ns : 0;
    if (!cp2parse::parse_proof_input(text.data(), text.size(), md, m, cfg.cell_size, want_ns, p, &err)) {
      std::printf("round trip %d refused: %s\n", it, err.c_str());
      ++bad;
      continue;
    }
    if (std::memcmp(p.dataset_root, droot, 32) || std::memcmp(p.entropy, ent, 32) || std::memcmp(p.slot_root, sroot, 32) ||
        p.n_cells != cfg.n_cells || p.n_slots != cfg.n_slots || p.slot_idx != slot || p.n_samples != ns || p.slot_proof != proof ||
        p.cell_felts != felts || p.paths != paths) {
      std::printf("round trip %d: values differ\n", it);
      ++bad;
    }
    // every prefix that lacks the closing brace is refused with a message (a copy of exactly that length, so that ASan sees any
    // read past it)
    if (it % 10 == 0) {
      for (size_t cut = 0; cut + 1 < text.size(); ++cut) {
        std::vector<char> buf(text.begin(), text.begin() + (long)cut);
        std::string e2;
        cp2parse::Parsed q;
        if (cp2parse::parse_proof_input(buf.data(), buf.size(), md, m, cfg.cell_size, want_ns, q, &e2) || e2.empty()) {
          std::printf("round trip %d: prefix of %zu bytes accepted or refused without a message\n", it, cut);
          ++bad;
        }
        ++prefixes;
      }
    }
    // random bytes overwritten: refused with a message, or parsed; never a sanitizer report
    for (int k = 0; k < 20; ++k) {
      std::vector<char> buf(text.begin(), text.end());
      for (int j = 0; j < 1 + (int)(rng() % 3); ++j) buf[rng() % buf.size()] = (char)(rng() % 256);
      std::string e3;
      cp2parse::Parsed q;
      if (!cp2parse::parse_proof_input(buf.data(), buf.size(), md, m, cfg.cell_size, want_ns, q, &e3) && e3.empty()) {
        std::printf("round trip %d: refused without a message\n", it);
        ++bad;
      }
    }
  }
  // cell rows that encode bytes decode back to them; others do not
  for (int it = 0; it < 2000; ++it) {
    const size_t cs = 1 + rng() % 300, nf = cp2parse::felts_per_bytes(cs);
    std::vector<uint8_t> cell(cs), stream(31 * nf, 0), felts(nf * 32, 0), back(cs);
    for (auto& b : cell) b = (uint8_t)rng();
    std::memcpy(stream.data(), cell.data(), cs);
    stream[cs] = 1;
    for (size_t k = 0; k < nf; ++k) std::memcpy(&felts[k * 32], &stream[k * 31], 31);
    if (!cp2parse::felts_to_cell_bytes(felts.data(), nf, cs, back.data()) || back != cell) {
      std::printf("cell of %zu bytes does not decode\n", cs);
      ++bad;
    }
    felts[(rng() % nf) * 32 + (rng() % 2 ? 31 : 30)] ^= 0x80;   // a felt >= 2^248, a wrong padding byte or another data byte
    if (cp2parse::felts_to_cell_bytes(felts.data(), nf, cs, back.data()) && back == cell) {
      std::printf("cell of %zu bytes: a flipped high bit still decodes to the same bytes\n", cs);
      ++bad;
    }
  }
  if (bad) {
    std::printf("json parse FAILED: %d problems\n", bad);
    return 1;
  }
  std::printf("json parse ok: %d round trips, %zu prefixes\n", trips, prefixes);
  return 0;
}
