// The op table of fr_unit_ops.hpp on gfx950: one case per lane, 256-lane workgroups, the lazy-reduction table in LDS
// filled by qtab_fill exactly as the product kernels fill it.  Built by the package Makefile as libfr_unit.so with the
// product's flags; tests/test_gpu_fr_unit.py loads it with ctypes.  Plain HIP, no link to libcodex_p2.so.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fr_unit_ops.hpp"

namespace {
constexpr int TPB = 256;
constexpr size_t MAX_CASES = (size_t)1 << 24;   // 2 GiB of records each way: beyond any plan of the test

template <int OP>
__global__ void __launch_bounds__(TPB) k_fr_unit(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
  __shared__ fr::QTab qtab;
  fr::qtab_fill(qtab, threadIdx.x, TPB);
  __syncthreads();
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i < n) fru::run<OP>(in + i * fru::REC, out + i * fru::REC, qtab);
}

template <int OP>
hipError_t launch(const uint32_t* in, size_t n, uint32_t* out) {
  k_fr_unit<OP><<<dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB)>>>(in, n, out);
  return hipGetLastError();
}

hipError_t launch_op(int op, const uint32_t* in, size_t n, uint32_t* out) {
  switch (op) {
#define FRU_CASE(OP) case fru::OP: return launch<fru::OP>(in, n, out);
    FRU_CASE(OP_NORM) FRU_CASE(OP_NORM_FULL) FRU_CASE(OP_ADD_LAZY) FRU_CASE(OP_MUL_MASKED) FRU_CASE(OP_MUL_UNMASKED)
    FRU_CASE(OP_SQR_MASKED) FRU_CASE(OP_SQR_UNMASKED) FRU_CASE(OP_SBOX_MASKED) FRU_CASE(OP_SBOX_UNMASKED) FRU_CASE(OP_TO_WIDE)
    FRU_CASE(OP_FROM_WIDE) FRU_CASE(OP_REDUCE_WIDE) FRU_CASE(OP_HALF_ROUND) FRU_CASE(OP_ROUND_PAIR) FRU_CASE(OP_EXT_UNMASKED)
    FRU_CASE(OP_EXT_MASKED) FRU_CASE(OP_FROM_WORDS) FRU_CASE(OP_TO_MONT) FRU_CASE(OP_TO_CANONICAL) FRU_CASE(OP_PERMUTE)
#undef FRU_CASE
    default: return hipErrorInvalidValue;
  }
}
}  // namespace

extern "C" int fru_n_ops() { return fru::N_OPS; }
extern "C" int fru_record_words() { return fru::REC; }

// Runs op over n records of REC words: upload, launch, synchronise, download.  Returns 0, the first hipError_t met, or
// FRU_GUARD_DISTURBED when a kernel wrote outside its n records (the device buffer carries GUARD records of 0xA5 on both
// sides); everything allocated is freed either way.  n == 0 is a no-op; an unknown op or an n beyond MAX_CASES is refused.
constexpr int FRU_GUARD_DISTURBED = -1;
constexpr size_t GUARD = 8;   // records

extern "C" int fru_run(int op, const void* in, size_t n, void* out) {
  if (op < 0 || op >= fru::N_OPS || n > MAX_CASES || (n && (!in || !out))) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t rec = fru::REC * sizeof(uint32_t), bytes = n * rec, gbytes = GUARD * rec;
  uint32_t* din = nullptr;
  uint8_t* dout = nullptr;
  uint8_t guard[2 * GUARD * fru::REC * sizeof(uint32_t)];
  hipError_t e = hipMalloc((void**)&din, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, bytes + 2 * gbytes);
  if (e == hipSuccess) e = hipMemcpy(din, in, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xA5, bytes + 2 * gbytes);
  if (e == hipSuccess) e = launch_op(op, din, n, (uint32_t*)(dout + gbytes));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout + gbytes, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(guard, dout, gbytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(guard + gbytes, dout + gbytes + bytes, gbytes, hipMemcpyDeviceToHost);
  int status = (int)e;
  if (e == hipSuccess)
    for (size_t i = 0; i < sizeof(guard); ++i)
      if (guard[i] != 0xA5) status = FRU_GUARD_DISTURBED;
  hipError_t f = din ? hipFree(din) : hipSuccess;
  if (status == 0) status = (int)f;
  f = dout ? hipFree(dout) : hipSuccess;
  if (status == 0) status = (int)f;
  return status;
}
