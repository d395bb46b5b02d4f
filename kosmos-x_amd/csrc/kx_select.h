// What the token kernels share (kx_sample.hip, kx_beam.hip): the order-preserving float key, the fixed-point softmax mass and the
// 1024-thread block reductions.  Everything here is an exact integer operation or a single fp32 expression per element, which is
// what makes both files' results independent of the order in which lanes, waves or atomics run.
#pragma once
#include "kx_common.h"

namespace {

constexpr int SB = 1024;                          // threads per workgroup (16 waves)
constexpr int SW = SB / 64;
constexpr unsigned KEY_MIN_VALID = 0x00800000u;   // key(-FLT_MAX): every finite value and +inf map at or above it, -inf below

__device__ __forceinline__ unsigned f2key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// exp(x - m) in 2^-40 fixed point (truncated); x == m gives exactly 2^40, also when both are +inf
__device__ __forceinline__ unsigned long long mass_fix(float x, float m) {
  const float e = x == m ? 1.0f : expf(x - m);
  return (unsigned long long)(e * 1099511627776.0f);
}

__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = red[0];
#pragma unroll
  for (int w = 1; w < SW; ++w) r = red[w] > r ? red[w] : r;
  __syncthreads();
  return r;
}
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = red[0];
#pragma unroll
  for (int w = 1; w < SW; ++w) r += red[w];
  __syncthreads();
  return r;
}

}  // namespace
