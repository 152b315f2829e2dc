// Host twin of fr_unit.hip: the same op table (fr_unit_ops.hpp) over the same device source compiled with CP2_HOST_CHECK,
// so every column accumulator has its 128-bit shadow and every documented bound is asserted.  A bound violation aborts;
// the SIGABRT handler then names the op and the case, which is what the tests report.
// Usage: fr_unit_host <cases> <results>
//   <cases>  : sections of { u32 op, u32 n, n records of 32 u32 }, back to back;  <results> : the n result records of each
//              section, in the same order.
#define CP2_HOST_CHECK 1
#include <csignal>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include <vector>

#include "fr_unit_ops.hpp"

static fr::QTab g_qtab;
static volatile int g_op = -1;
static volatile long g_case = -1;

static void on_abort(int) {
  char msg[96];
  int len = std::snprintf(msg, sizeof msg, "ABORTED in op %d case %ld\n", g_op, g_case);
  if (len > 0) (void)!write(2, msg, (size_t)len);
}

template <int OP>
static void run_all(const uint32_t* in, size_t n, uint32_t* out) {
  for (size_t i = 0; i < n; ++i) {
    g_case = (long)i;
    fru::run<OP>(in + i * fru::REC, out + i * fru::REC, g_qtab);
  }
}

static bool run_op(int op, const uint32_t* in, size_t n, uint32_t* out) {
  switch (op) {
#define FRU_CASE(OP) case fru::OP: run_all<fru::OP>(in, n, out); return true;
    FRU_CASE(OP_NORM) FRU_CASE(OP_NORM_FULL) FRU_CASE(OP_ADD_LAZY) FRU_CASE(OP_MUL_MASKED) FRU_CASE(OP_MUL_UNMASKED)
    FRU_CASE(OP_SQR_MASKED) FRU_CASE(OP_SQR_UNMASKED) FRU_CASE(OP_SBOX_MASKED) FRU_CASE(OP_SBOX_UNMASKED) FRU_CASE(OP_TO_WIDE)
    FRU_CASE(OP_FROM_WIDE) FRU_CASE(OP_REDUCE_WIDE) FRU_CASE(OP_HALF_ROUND) FRU_CASE(OP_ROUND_PAIR) FRU_CASE(OP_EXT_UNMASKED)
    FRU_CASE(OP_EXT_MASKED) FRU_CASE(OP_FROM_WORDS) FRU_CASE(OP_TO_MONT) FRU_CASE(OP_TO_CANONICAL) FRU_CASE(OP_PERMUTE)
#undef FRU_CASE
    default: return false;
  }
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: fr_unit_host <cases> <results>\n"); return 2; }
  std::signal(SIGABRT, on_abort);
  for (int i = 0; i < fr::QTAB_WORDS; ++i) fr::qtab_fill(g_qtab, i, fr::QTAB_WORDS);
  FILE* fi = std::fopen(argv[1], "rb");
  FILE* fo = std::fopen(argv[2], "wb");
  if (!fi || !fo) { std::fprintf(stderr, "cannot open files\n"); return 2; }
  size_t total = 0, sections = 0;
  uint32_t head[2];
  while (std::fread(head, sizeof(uint32_t), 2, fi) == 2) {
    const size_t words = (size_t)head[1] * fru::REC;
    std::vector<uint32_t> in(words), out(words);
    if (words && std::fread(in.data(), sizeof(uint32_t), words, fi) != words) { std::fprintf(stderr, "short section\n"); return 2; }
    g_op = (int)head[0];
    if (!run_op((int)head[0], in.data(), head[1], out.data())) { std::fprintf(stderr, "unknown op %u\n", head[0]); return 2; }
    if (words && std::fwrite(out.data(), sizeof(uint32_t), words, fo) != words) { std::fprintf(stderr, "short write\n"); return 2; }
    total += head[1];
    ++sections;
  }
  if (std::fclose(fo) != 0) { std::fprintf(stderr, "close failed\n"); return 2; }
  std::fclose(fi);
  std::printf("fr_unit_host: %zu cases in %zu sections, no bound violations\n", total, sections);
  return 0;
}
