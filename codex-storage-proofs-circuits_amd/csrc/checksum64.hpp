// The checksum of the library's own files: the tree cache and the kept form (cache_file.hpp, cache_file.cpp), fill checkpoints (fill_checkpoint.hpp).
// No HIP in here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace cp2i {

// 64-bit multiply-mix over 8-byte words (not cryptographic: detects truncation and bit rot, not an adversary), fed chunk by
// chunk while the nodes stream between the device and the file.  Every chunk but the last must be a multiple of 32 bytes.
struct Checksum64 {
  uint64_t h[4] = {0x9e3779b97f4a7c15ULL, 0xc2b2ae3d27d4eb4fULL, 0x165667b19e3779f9ULL, 0x27d4eb2f165667c5ULL};
  uint64_t total = 0;
  uint64_t tail = 0;
  bool tailed = false;
  void update(const uint8_t* p, size_t n) {
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
      uint64_t w[4];
      std::memcpy(w, p + i, 32);
      for (int k = 0; k < 4; ++k) {
        h[k] = (h[k] ^ w[k]) * 0x100000001b3ULL;
        h[k] = (h[k] << 29) | (h[k] >> 35);
      }
    }
    total += n;
    if (i < n) {                 // only ever the last chunk
      tailed = true;
      tail = h[0] ^ (h[1] * 3) ^ (h[2] * 5) ^ (h[3] * 7) ^ total;
      for (; i < n; ++i) tail = (tail ^ p[i]) * 0x100000001b3ULL;
    }
  }
  uint64_t finish() const {
    uint64_t r = tailed ? tail : (h[0] ^ (h[1] * 3) ^ (h[2] * 5) ^ (h[3] * 7) ^ total);
    r ^= r >> 33; r *= 0xff51afd7ed558ccdULL; r ^= r >> 33;
    return r;
  }
};

}  // namespace cp2i
