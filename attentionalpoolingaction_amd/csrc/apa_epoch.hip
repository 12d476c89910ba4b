// apa_epoch.hip -- the visiting order of one epoch over a resident feature cache, drawn on the device in ONE launch
// (apa.h: apa_epoch_order): order[i] = the image visited at position i, a permutation of [0, T) that every element
// computes on its own from (seed, epoch, i, T).  No atomics, no workspace, no sort, no allocation; capturable.
//
// The rule (apa.h states it for a host restatement; custom_ops_factory._epoch_order_rule_cpu is one):
//   b  = max(2, number of bits of T - 1): the walk's domain is [0, 2^b), the smallest power of two >= max(T, 4)
//   lb = b / 2 bits in the left half, rb = b - lb in the right half: x = (L << rb) | R
//   h  = splitmix64(seed, epoch), key_r = splitmix64(h, r) for r = 0..5 -- rng_key's derivation (apa_internal.h), the
//        low word of key_r is k0, the high word k1
//   round r even: L ^= rng_hash(R, k0, k1) & (2^lb - 1);  r odd: R ^= rng_hash(L, k0, k1) & (2^rb - 1)
//        (rng_hash: the dropout mask's two-round 24-bit multiply-xorshift mix, apa_device.h)
//   six rounds are one bijection of the domain; it is applied to i, and again while the image is >= T (cycle walking:
//   the orbit of i < T returns below T after at most 2^b - T + 1 applications; 2^b < 2 T for T >= 3, so two on average).
#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

constexpr int EPOCH_ROUNDS = 6;
struct EpochKeys { uint32_t k0[EPOCH_ROUNDS], k1[EPOCH_ROUNDS]; };

__device__ __forceinline__ uint32_t epoch_feistel(uint32_t x, const EpochKeys& k, int rb, uint32_t mL, uint32_t mR) {
  uint32_t L = x >> rb, R = x & mR;
#pragma unroll
  for (int r = 0; r < EPOCH_ROUNDS; r += 2) {
    L ^= rng_hash(R, k.k0[r], k.k1[r]) & mL;
    R ^= rng_hash(L, k.k0[r + 1], k.k1[r + 1]) & mR;
  }
  return (L << rb) | R;
}

__global__ __launch_bounds__(256) void epoch_order_kernel(int32_t* __restrict__ order, uint32_t T, EpochKeys k, int rb,
                                                          uint32_t mL, uint32_t mR) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= T) return;
  uint32_t x = epoch_feistel((uint32_t)i, k, rb, mL, mR);
  while (x >= T) x = epoch_feistel(x, k, rb, mL, mR);
  order[i] = (int32_t)x;
}

}  // namespace apa

using namespace apa;

extern "C" int apa_epoch_order(int32_t* order, int T, uint64_t seed, uint64_t epoch, void* stream) {
  const char* fn = "apa_epoch_order";
  if (!order || (reinterpret_cast<uintptr_t>(order) & 3)) {
    set_error("%s: order must be a 4-byte aligned device pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (T < 1) {
    set_error("%s: T=%d: an epoch visits at least one image", fn, T);
    return APA_ERR_INVALID_ARG;
  }
  int b = 2;
  while (b < 31 && (1u << b) < (uint32_t)T) ++b;
  const int lb = b / 2, rb = b - lb;
  EpochKeys k;
  uint32_t h0, h1;
  rng_key(seed, epoch, &h0, &h1);
  const uint64_t h = ((uint64_t)h1 << 32) | h0;
  for (int r = 0; r < EPOCH_ROUNDS; ++r) rng_key(h, (uint64_t)r, &k.k0[r], &k.k1[r]);
  const unsigned blocks = (unsigned)(((size_t)T + 255) / 256);
  hipLaunchKernelGGL(epoch_order_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), order,
                     (uint32_t)T, k, rb, (1u << lb) - 1u, (1u << rb) - 1u);
  APA_LAUNCH_CHECK("epoch_order_kernel");
  return APA_OK;
}
