// What the split-precision convolution (conv_x3.hip) and its gradients (conv_x3_bwd.hip) share: the operand split, the packed
// operand's header and the power-of-two scale rule.
#pragma once
#include "conv_kernel.hpp"

namespace upf {
namespace convx3 {
using namespace upf::conv;

__host__ __device__ constexpr int pad16(int v) { return (v + 15) / 16 * 16; }

constexpr int HDR_F16 = 512;                          // packed-operand header size in fp16 elements (1 KB)

// 8 consecutive fp32 pixels of one channel row -> 4 dwords of fp16 hi halves, 4 dwords of fp16 lo halves
__device__ __forceinline__ void split8(const float (&v)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int pp = 0; pp < 4; ++pp) {
    const uint32_t h = pack2<f16_t>(v[2 * pp], v[2 * pp + 1]);
    const float r0 = v[2 * pp] - f16_bits_to_f32(h & 0xffffu), r1 = v[2 * pp + 1] - f16_bits_to_f32(h >> 16);
    hi[pp] = h;
    lo[pp] = pack2<f16_t>(r0, r1);
  }
}

// The power of two 2^s that puts a tensor's |.|max (given as the bits of a non-negative float) into [2^13, 2^14): hi / lo halves of
// everything down to 2^-16 of the maximum are then normal fp16 numbers.  1 for an all-zero, non-finite or NaN maximum.
__device__ __forceinline__ float x3_scale_of(uint32_t absmax_bits) {
  const float m = __uint_as_float(absmax_bits);
  if (!(m > 0.f) || m > 3.0e38f) return 1.f;
  int e = (int)((absmax_bits >> 23) & 0xffu) - 127;   // floor(log2(m)) for normal m (a subnormal maximum: e = -127, clamped below)
  int sft = 13 - e;
  sft = sft > 100 ? 100 : (sft < -100 ? -100 : sft);
  return __uint_as_float((uint32_t)(127 + sft) << 23);
}

// conv_x3.hip: zeroes the packed operand's 1 KB header and leaves the bits of max |w| over the nw weights in header[0]
// (the first two launches of upf_conv_x3_pack_weights and upf_conv_x3_pack_weights_dgrad)
void launch_header_absmax(const float* w, long long nw, void* w_packed, hipStream_t stream);

}  // namespace convx3
}  // namespace upf
