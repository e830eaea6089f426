// On-device training data: the counter-based label sampler (sq_sample_kernel) and the stream position's advance
// (stream_advance_kernel).  The rule is documented in include/sqr.h (sqr_sq_sample); sqr/cpu.py restates it in
// numpy and tests/_philox_ref.py in Python ints.
#include "sqr_common.h"

namespace sqr {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// Philox4x32-10 (Salmon et al., SC'11): ten rounds of two 32x32 -> 64 multiplies, the key bumped by the Weyl
// constants after each round
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
    const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// One thread per sample.  The position is read from memory (never a kernel argument), so a replayed graph
// draws new samples once stream_advance_kernel has moved it.
__global__ void __launch_bounds__(256) sq_sample_kernel(const uint64_t* __restrict__ position, uint32_t seed_lo,
                                                        uint32_t seed_hi, uint32_t substream, uint64_t offset, int B,
                                                        float* __restrict__ params, uint32_t* __restrict__ raw) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const uint64_t i = *position + offset + (uint64_t)b;  // wraps modulo 2^64
  uint32_t w[12];
#pragma unroll
  for (int call = 0; call < 3; ++call)
    philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)call, substream, seed_lo, seed_hi, w + 4 * call);
  float u[11];
#pragma unroll
  for (int j = 0; j < 11; ++j) u[j] = (float)(w[j] >> 8) * 0x1p-24f;  // exact, in [0, 1)
  float* p = params + (size_t)b * 12;
#pragma unroll
  for (int j = 0; j < 3; ++j) p[j] = fmaf(50.f, u[j], 25.f) / 255.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) p[3 + j] = fmaf(0.9f, u[3 + j], 0.1f);
#pragma unroll
  for (int j = 0; j < 3; ++j) p[5 + j] = fmaf(80.f, u[5 + j], 88.f) / 255.f;
  // 2 u is exact, and sincospif reduces its argument exactly: no rounded 2 pi u
  const float r1 = sqrtf(1.f - u[8]), r2 = sqrtf(u[8]);
  float s1, c1, s2, c2;
  sincospif(2.f * u[9], &s1, &c1);
  sincospif(2.f * u[10], &s2, &c2);
  p[8] = r1 * s1;
  p[9] = r1 * c1;
  p[10] = r2 * s2;
  p[11] = r2 * c2;
  if (raw) {
    uint32_t* q = raw + (size_t)b * 12;
#pragma unroll
    for (int j = 0; j < 12; ++j) q[j] = w[j];
  }
}

// One thread: an ordinary load, add and store.  Stream order has retired every read of the old value.
__global__ void stream_advance_kernel(uint64_t* position, uint64_t stride) { *position = *position + stride; }

}  // namespace sqr

using namespace sqr;

extern "C" int sqr_sq_sample(const uint64_t* position, uint64_t seed, uint32_t substream, uint64_t offset, int B,
                             float* params, uint32_t* raw, void* stream) {
  SQR_CHECK_ARG(B >= 1 && B <= 65535, "sq_sample: B=%d out of range [1,65535]", B);
  SQR_CHECK_ARG(position && params, "sq_sample: null pointer");
  hipLaunchKernelGGL(sq_sample_kernel, dim3((B + 255) / 256), dim3(256), 0, as_stream(stream), position,
                     (uint32_t)seed, (uint32_t)(seed >> 32), substream, offset, B, params, raw);
  SQR_HIP_LAUNCH_CHECK("sq_sample_kernel");
  return SQR_OK;
}

extern "C" int sqr_sq_stream_advance(uint64_t* position, uint64_t stride, void* stream) {
  SQR_CHECK_ARG(position, "sq_stream_advance: null pointer");
  hipLaunchKernelGGL(stream_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), position, stride);
  SQR_HIP_LAUNCH_CHECK("stream_advance_kernel");
  return SQR_OK;
}
