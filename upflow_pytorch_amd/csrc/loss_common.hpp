// The reduction core and the small device functions shared by the loss-side kernels (loss.hip, loss_variants.hip) and by the
// other deterministic reductions of the library (misc.hip: feature normalisation, sgu_blend.hip: pyramid distillation).  These
// define the bits of the training trajectory, so each exists exactly once.  Every includer is compiled with -ffp-contract=off.
#pragma once
#include "common.hpp"

namespace upf {

// Sum of v over the NT threads of a workgroup, returned to every thread: xor-shuffle tree 32 -> 1 inside each wave, lane 0 of
// each wave to LDS, then the NT / 64 slots added serially in index order.  sh: NT / 64 floats of LDS, reusable right after.
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) r += sh[k];
  return r;
}

// x^e for x > 0 through the hardware's log2 / exp2 (1 ulp each): the libm powf of the composition is ~60 instructions, and the
// distillation term is evaluated ~20 M times per direction in the backward (the launch was 122 us, bound by it).  The default
// 'abs_robust' photometric term keeps libm's powf: the two round differently.
__device__ __forceinline__ float fast_pow(float x, float e) { return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x)); }

namespace loss {

constexpr int NT = 256;

// workgroups of a reduction over n elements: one per NT elements, at most 1024 (the kernels stride over the rest)
static int red_blocks(long long n) {
  long long b = (n + NT - 1) / NT;
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

__device__ __forceinline__ float sgn(float d) { return (d > 0.f) ? 1.0f : ((d < 0.f) ? -1.0f : 0.f); }

// ---- edge-aware smoothness, order 1 and 2 ----------------------------------------------------------------------------------
// exp(-mean_c |img[a] - img[b]|): the weight of the difference between pixels a and b of one image
__device__ __forceinline__ float edge_w(const float* __restrict__ img, int Ci, int HW, int a, int b) {
  float s = 0.f;
  for (int c = 0; c < Ci; ++c) s += fabsf(img[(size_t)c * HW + a] - img[(size_t)c * HW + b]);
  return expf(-(s / (float)Ci));
}
// (p0 - p1) - (p1 - p2): gradient_x(gradient_x(pred)) in the reference's order
__device__ __forceinline__ float dd(const float* __restrict__ p, int a, int s) { return (p[a] - p[a + s]) - (p[a + s] - p[a + 2 * s]); }

// |difference of order ORDER| at pixel q along stride s, in the channel plane that starts at pred[plane]
template <int ORDER>
__device__ __forceinline__ float smooth_term(const float* __restrict__ pred, size_t plane, int q, int s) {
  if constexpr (ORDER == 1) return fabsf(pred[plane + q] - pred[plane + q + s]);
  else return fabsf(dd(pred + plane, q, s));
}

// partials[block] = { sum over i + ORDER < H of term(i,j) * wx(i,j),  sum over j + ORDER < W of term(i,j) * wy(i,j) }:
//   order 1: term = |pred(i,j) - pred(i+1,j)|, order 2: term = |xx(i,j)| (dd); the weight spans the term's reach, ORDER pixels
template <int ORDER>
__global__ __launch_bounds__(NT)
void smooth_fwd_kernel(const float* __restrict__ img, const float* __restrict__ pred, float* __restrict__ partials,
                       int Ci, int Cp, int H, int W, long long npix) {
  static_assert(ORDER == 1 || ORDER == 2, "first or second differences");
  __shared__ float sh[NT / 64];
  const int HW = H * W;
  float sx = 0.f, sy = 0.f;
  for (long long p = blockIdx.x * (long long)NT + threadIdx.x; p < npix; p += (long long)gridDim.x * NT) {
    const long long n = p / HW;
    const int q = (int)(p - n * HW), i = q / W, j = q - i * W;
    const float* im = img + (size_t)n * Ci * HW;
    const float* pr = pred + (size_t)n * Cp * HW;
    if (i + ORDER < H) {
      const float wgt = edge_w(im, Ci, HW, q, q + ORDER * W);
      float t = 0.f;
      for (int c = 0; c < Cp; ++c) t += smooth_term<ORDER>(pr, (size_t)c * HW, q, W);
      sx += t * wgt;
    }
    if (j + ORDER < W) {
      const float wgt = edge_w(im, Ci, HW, q, q + ORDER);
      float t = 0.f;
      for (int c = 0; c < Cp; ++c) t += smooth_term<ORDER>(pr, (size_t)c * HW, q, 1);
      sy += t * wgt;
    }
  }
  const float a = block_sum<NT>(sx, sh), b = block_sum<NT>(sy, sh);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = a; partials[2 * blockIdx.x + 1] = b; }
}

}  // namespace loss
}  // namespace upf
