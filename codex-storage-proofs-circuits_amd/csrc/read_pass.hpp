// The chunked pass over listed blocks of many owners that cp2_datasets_read_blocks (read_blocks.cpp) and cp2_fills_resume_many
// (fills_resume_many.cpp) share: chunk k + 1 read on the context's ingestion threads into the other of two pooled pinned buffers while
// chunk k is uploaded, hashed and reduced to block roots on repair's data path (repair_check_with, repair.cpp), fake-source requests
// regenerated on the device in between, and one judge launch per chunk over one absolute address per request.  What differs between
// the two calls is the judge and whether anything is gathered afterwards.  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "dataset_obj.hpp"
#include "repair.hpp"
#include "workers.hpp"

namespace cp2i {

// Where the blocks of a pass come from.  read: the file-sourced requests of chunk k, each into row_of(i), on host threads (false: *err
// is the message, CP2_ERR_IO).  fake (may be empty: none): per request, whether the device regenerates it from seeds[i] (cp2_slot_seed)
// and firsts[i] (its first cell).  A later source over a fill session's present blocks is another `read` and nothing else.
struct BlockSource {
  size_t n_chunks = 0;
  std::function<bool(size_t k, const std::function<uint8_t*(size_t)>& row_of, std::string* err)> read;
  std::vector<uint8_t> fake;
  std::vector<uint64_t> seeds, firsts;
};

// The last device step of a chunk: the m fresh block roots of requests [c0, c0 + m) (32-byte rows) against the 32 bytes at d_addr[0..m),
// the device copy of addr + c0, one verdict word each (0 match), queued on st.  cp2_datasets_read_blocks compares
// (launch_repair_compare_addr); cp2_fills_resume_many compares and zeroes what differs (launch_block_root_recheck_addr).
using ReadJudge = std::function<hipError_t(const uint8_t* fresh, const uint64_t* d_addr, size_t m, uint32_t* verdict, hipStream_t st)>;

// The middle of the pass: n requests in chunks of `chunk`, request i judged by judge_rows against the 32 bytes at addr[i]; addr (n + path
// rows entries, read_blocks_addr_table) gathered whole into `gathered` (host, addr.size() x 32 bytes; NULL: nothing is gathered, and addr
// may end with its n-th entry).  data (n x block_size, may be NULL):
// every row is filled; nothing is zeroed here.  *touched: the requests whose rows may hold file bytes when the pass fails.
inline int read_pass(cp2_ctx* ctx, size_t cell_size, size_t block_size, size_t n, size_t chunk, const std::vector<uint64_t>& addr, BlockSource& src,
                     const ReadJudge& judge_rows, uint8_t* data, uint8_t* gathered, uint32_t* status, size_t* touched) {
  const size_t cpb = block_size / cell_size;
  const bool any_fake = !src.fake.empty();
  PinBuf ring[2];                                    // check only: two chunk buffers, whatever n is
  if (!data)
    for (auto& b : ring) CP2_TRY(b.alloc(ctx, std::min(n, chunk) * block_size));
  DevBuf d_addr, d_gen;                              // (go after the streams have drained: DevBuf::release)
  std::string read_err[2];
  bool read_ok[2] = {true, true};
  auto base_of = [&](size_t k) { return data ? data + k * chunk * block_size : ring[k & 1].u8(); };
  {
    Workers reader(1);                               // one chunk ahead; the chunk's files are spread over the ingestion threads inside
    auto start = [&](size_t k) {
      if (k >= src.n_chunks) return;
      *touched = std::min(n, (k + 1) * chunk);
      uint8_t* base = base_of(k);
      const size_t c0 = k * chunk;
      reader.submit([&, k, base, c0] {
        read_ok[k & 1] = src.read(k, [&](size_t i) { return base + (i - c0) * block_size; }, &read_err[k & 1]);
      });
    };
    // chunk k's rows, read; chunk k + 1 started.  A ring buffer is read into again only after the chunk that was uploaded from it is done.
    auto take = [&](size_t c0, const uint8_t** out) -> int {
      const size_t k = c0 / chunk;
      reader.wait_idle();
      if (!read_ok[k & 1]) {
        ctx->err = read_err[k & 1];
        return CP2_ERR_IO;
      }
      if (!data && k > 0) CP2_HIP(ctx, hipStreamSynchronize(ctx->stream));
      start(k + 1);
      *out = base_of(k);
      return CP2_OK;
    };
    RepairJudge judge;
    judge.begin = [&](size_t) -> int {
      CP2_TRY(d_addr.scratch(ctx, n * 8));
      CP2_HIP(ctx, hipMemcpyAsync(d_addr.p, addr.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
      if (any_fake) {
        CP2_TRY(d_gen.scratch(ctx, n * 16));
        CP2_HIP(ctx, hipMemcpyAsync(d_gen.p, src.seeds.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
        CP2_HIP(ctx, hipMemcpyAsync(d_gen.u8() + n * 8, src.firsts.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
      }
      start(0);
      return CP2_OK;
    };
    judge.host = [&](size_t c0, size_t, const uint8_t** out) -> int { return take(c0, out); };
    judge.host_pinned = data ? host_array_pinned(data, n * block_size, (size_t)128 << 20) : true;
    if (any_fake) {
      // a chunk with regenerated blocks is put together on the device: runs of file rows uploaded, runs of fake rows generated in place
      // (and downloaded into the caller's rows), all on the stream the chunk is hashed on
      judge.cells = [&](size_t c0, size_t m, uint8_t* d_cells, hipStream_t st) -> int {
        const uint8_t* rows = nullptr;
        CP2_TRY(take(c0, &rows));
        const uint64_t* seeds = static_cast<const uint64_t*>(d_gen.p);
        for (size_t a = 0; a < m;) {
          size_t b = a + 1;
          while (b < m && src.fake[c0 + b] == src.fake[c0 + a]) ++b;
          const size_t off = a * block_size, len = (b - a) * block_size;
          if (src.fake[c0 + a]) {
            CP2_HIP(ctx, cp2k::launch_gen_fake_cells_many(seeds + c0 + a, seeds + n + c0 + a, cpb, (b - a) * cpb, cell_size, d_cells + off, st));
            if (data) CP2_HIP(ctx, hipMemcpyAsync(data + (c0 + a) * block_size, d_cells + off, len, hipMemcpyDeviceToHost, st));
          } else {
            CP2_HIP(ctx, hipMemcpyAsync(d_cells + off, rows + off, len, hipMemcpyHostToDevice, st));
          }
          a = b;
        }
        return CP2_OK;
      };
    }
    judge.verdicts = [&](const uint8_t* fresh, size_t c0, size_t m, uint32_t* verdict, hipStream_t st) -> int {
      CP2_HIP(ctx, judge_rows(fresh, static_cast<const uint64_t*>(d_addr.p) + c0, m, verdict, st));
      return CP2_OK;
    };
    const int r = repair_check_with(ctx, cell_size, block_size, nullptr, n, status, judge);
    reader.wait_idle();                              // (a chunk read ahead of a pass that failed writes into rows of this scope)
    if (r != CP2_OK) {
      (void)hipStreamSynchronize(ctx->stream);       // nothing of the pass reads a ring buffer or writes a caller's row after this
      return r;
    }
  }
  return gathered ? gather_rows_by_addr(ctx, addr, gathered) : CP2_OK;
}

}  // namespace cp2i
