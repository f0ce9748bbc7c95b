// Gradients of the split-precision convolution (conv_x3.hip): the fp32 training step on the fp16 matrix cores — gfx950.
//
// A layer y = LeakyReLU(conv(x, w) + b) with fp32 tensors; backward, from grad_y:
//   1. upf_act_grad_x3:  grad_pre = grad_y * (y > 0 ? 1 : slope), its |.|max on the device, and — second launch — the copy
//      gs = grad_pre * 2^s with 2^s = the power of two that puts that maximum into [2^13, 2^14) (x3_scale_of: the rule of the packed
//      weights), plus the first stage of the bias gradient (sums of gs).  The "slot" {|.|max bits, 2^s, 2^-s, 0} stays on the device.
//      WHY: the split a = fp16(a) + fp16(a - fp16(a)) has an absolute floor — below 2^-3 the low half is subnormal, below 6e-8
//      both halves are zero — and the losses are mean()-reduced, so grad_pre is routinely 1e-6 ... 1e-9.  Scaled, everything down
//      to 2^-16 of the tensor's maximum keeps 22 bits (below: up to 2^-38 * max of absolute error per element, the floor stated in
//      include/upflow_hip.h, GRADIENT RANGE; the activations of the weight gradient are split un-scaled).  Powers of two only: scaling and un-scaling are exact, so the results for
//      grad_y and grad_y * 2^-k are the same bits up to the factor (tests/test_hip_conv_x3_train.py).  No host synchronisation.
//   2. data gradient, stride 1 (upf_conv_x3_dgrad): upf_conv_x3_forward of gs with the flipped, transposed kernel
//      (upf_conv_x3_pack_weights_dgrad).  The forward kernel multiplies its sums by the header's 2^-s_w; a one-thread launch sets
//      that field to 2^-s_w * 2^-s first, so the un-scaling costs no pass.  Stride 2 (3x3): a plain fp32 gather kernel on the master
//      weights (any H, W; these layers hold ~2 % of the step's flops), un-scaled by 2^-s.
//   3. weight gradient (upf_conv_x3_wgrad): grad_w[co][ci][tap] = sum over pixels gs[co][pixel] * x[ci][pixel shifted by the tap], an
//      MFMA GEMM whose K dimension is the PIXELS of all levels, flattened (n, y, x) -> q: a lane holds 8 consecutive q of one
//      channel, so any H, W >= 1 and either stride take the same kernel (the pixel coordinates are carried incrementally).  Both
//      operands are split on the way into the registers; three v_mfma_f32_16x16x32_f16 per operand pair, the low-order products
//      in their own accumulators (a third of the rounding chain, conv_x3.hip SPLITACC).  Deterministic split-K: a workgroup owns
//      64 co x 32 ci x all taps and one K slice of one level, writes its partial block to the workspace, and one reduction launch
//      sums the slices in order, each times its level's 2^-s, and finishes the bias gradient (no float atomics).
#include <cstdint>
#include "conv_x3_common.hpp"

namespace upf {
namespace x3bwd {
using namespace upf::conv;
using namespace upf::convx3;

constexpr int BIAS_NCH = 32;             // first-stage bias sums per channel
constexpr int MAXLV = 6;

// ---------------------------------------------------------------------------------------------------------------------
// activation gradient + range scale
__global__ void slot_zero_kernel(uint32_t* slot) { if (threadIdx.x < 4) slot[threadIdx.x] = 0u; }

// the elements of channel c = blockIdx.x / 32 are cut into 32 runs; run j = blockIdx.x % 32 belongs to this workgroup
struct Run { int c; long long begin, end; };
__device__ __forceinline__ Run run_of_block(int B, int HW) {
  Run r;
  r.c = blockIdx.x / BIAS_NCH;
  const int j = blockIdx.x - r.c * BIAS_NCH;
  const long long T = (long long)B * HW, per = (T + BIAS_NCH - 1) / BIAS_NCH;
  r.begin = j * per;
  r.end = r.begin + per < T ? r.begin + per : T;
  return r;
}

__global__ __launch_bounds__(256)
void grad_absmax_kernel(const float* __restrict__ gy, long long gbs, const float* __restrict__ y, long long ybs, uint32_t* slot,
                        int B, int HW, float slope) {
  const Run r = run_of_block(B, HW);
  float m = 0.f;
  for (long long i = r.begin + threadIdx.x; i < r.end; i += 256) {
    const int n = (int)(i / HW), p = (int)(i - (long long)n * HW);
    float v = gy[(size_t)n * gbs + (size_t)r.c * HW + p];
    if (y && !(y[(size_t)n * ybs + (size_t)r.c * HW + p] > 0.f)) v *= slope;
    const float a = fabsf(v);
    m = (a == a && a > m) ? a : m;                    // (NaN gradients do not define the scale)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float wmax[4];
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x != 0) return;
  m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  // One atomic per workgroup, and only where it can still raise the maximum: thousands of atomics on one address were this
  // kernel's whole time.  (The plain read may be stale, and then only lets an atomic through that changes nothing.)
  const uint32_t bits = __float_as_uint(m);            // non-negative floats order like their bit patterns
  if (m > 0.f && bits > *reinterpret_cast<volatile uint32_t*>(slot)) atomicMax(slot, bits);
}

__global__ __launch_bounds__(256)
void act_grad_x3_kernel(const float* __restrict__ gy, long long gbs, const float* __restrict__ y, long long ybs, float* __restrict__ dst,
                        long long dbs, float* __restrict__ part, float* slot, int B, int HW, float slope) {
  __shared__ float wsum[4];
  const Run r = run_of_block(B, HW);
  const float sc = x3_scale_of(reinterpret_cast<const uint32_t*>(slot)[0]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    slot[1] = sc;
    slot[2] = 1.0f / sc;
  }
  float sum = 0.f;
  for (long long i = r.begin + threadIdx.x; i < r.end; i += 256) {
    const int n = (int)(i / HW), p = (int)(i - (long long)n * HW);
    float v = gy[(size_t)n * gbs + (size_t)r.c * HW + p];
    if (y && !(y[(size_t)n * ybs + (size_t)r.c * HW + p] > 0.f)) v *= slope;
    v *= sc;
    dst[(size_t)n * dbs + (size_t)r.c * HW + p] = v;
    sum += v;
  }
  if (!part) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);         // (a fixed tree: the same bits every run)
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// ---------------------------------------------------------------------------------------------------------------------
// data gradient
// conv_x3.hip's pack_x3_kernel for the convolution [Cout -> Cin] with the kernel wT[ci][co][tap] = w[co][ci][ntaps - 1 - tap].
// Header: {|w|max bits, 2^s, 2^-s (times the gradient's 2^-s while a data gradient runs: dgrad_hdr_kernel), 2^-s}.
__global__ void pack_x3_dgrad_kernel(const float* __restrict__ w, f16_t* __restrict__ wp, int Cin, int Cout, int ntaps) {
  const int kp = pad16(Cout), op = pad32(Cin), nk = kp / 16;          // K = the layer's output channels, rows = its input channels
  const float sc = x3_scale_of(reinterpret_cast<const uint32_t*>(wp)[0]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    reinterpret_cast<float*>(wp)[1] = sc;
    reinterpret_cast<float*>(wp)[2] = 1.0f / sc;
    reinterpret_cast<float*>(wp)[3] = 1.0f / sc;
  }
  f16_t* blocks = wp + HDR_F16;
  const long long total = (long long)ntaps * op * kp * 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i & 7), px = (int)((i >> 3) & 31), kg = (int)((i >> 8) & 1), hl = (int)((i >> 9) & 1);
    const long long b = i >> 10;                     // (slab * nk + kstep) * ntaps + tap
    const int tap = (int)(b % ntaps), kstep = (int)((b / ntaps) % nk), slab = (int)(b / ((long long)ntaps * nk));
    const int ci = slab * 32 + px, co = kstep * 16 + kg * 8 + j;
    float v = 0.f;
    if (ci < Cin && co < Cout) v = w[((size_t)co * Cin + ci) * ntaps + (ntaps - 1 - tap)] * sc;
    const uint16_t h = f32_to_f16_bits(v);
    blocks[i].v = hl ? f32_to_f16_bits(v - f16_bits_to_f32(h)) : h;
  }
}
__global__ void dgrad_hdr_kernel(float* hdr, const float* __restrict__ slot) { if (threadIdx.x == 0) hdr[2] = hdr[3] * slot[2]; }

// Stride-2 3x3 layer: gx[n][ci][iy][ix] = 2^-s * sum_{co, ky, kx : iy + 1 - ky = 2 oy, ix + 1 - kx = 2 ox} w[co][ci][ky][kx] * gs[n][co][oy][ox]
// in fp32 (1, 2 or 4 taps per pixel).  A workgroup: 256 pixels of one (n, ci); w[:, ci] in LDS.
__global__ __launch_bounds__(256)
void dgrad_s2_kernel(const float* __restrict__ gs, long long gbs, const float* __restrict__ w, float* __restrict__ gx, long long xbs,
                     const float* __restrict__ slot, int Cin, int Cout, int H, int W, int Ho, int Wo) {
  extern __shared__ float wl[];                       // [Cout][9]
  const int ci = blockIdx.y, n = blockIdx.z;
  for (int i = threadIdx.x; i < Cout * 9; i += 256) wl[i] = w[((size_t)(i / 9) * Cin + ci) * 9 + i % 9];
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int iy = p / W, ix = p - iy * W;
  int off[4], tap[4], nt = 0;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ty = iy + 1 - ky, tx = ix + 1 - kx;
      if (ty >= 0 && tx >= 0 && !(ty & 1) && !(tx & 1) && (ty >> 1) < Ho && (tx >> 1) < Wo) {
        off[nt] = (ty >> 1) * Wo + (tx >> 1);
        tap[nt] = ky * 3 + kx;
        ++nt;
      }
    }
  const float* gn = gs + (size_t)n * gbs;
  const int HoWo = Ho * Wo;
  float sum = 0.f;
  for (int co = 0; co < Cout; ++co)
    for (int t = 0; t < nt; ++t) sum += gn[(size_t)co * HoWo + off[t]] * wl[co * 9 + tap[t]];
  gx[(size_t)n * xbs + (size_t)ci * H * W + p] = sum * slot[2];
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient
struct Lv {
  const float* x; const float* g; const float* slot; const float* bpart;
  long long xbs, gbs;
  int B, H, W, Ho, Wo;
  int nch;                                            // 32-pixel K chunks of this level
  int slice0, nslices, cps;                           // its K slices: [slice0, slice0 + nslices), cps chunks each
};
struct Params { Lv lv[MAXLV]; int nlevels; };

constexpr int KCH = 32;                               // pixels per chunk (one MFMA's K)
constexpr int TCO = 64, TCI = 32;                     // a workgroup's block of grad_w: 2 x 2 waves of 32 co x 16 ci

template <int NT>
__global__ __launch_bounds__(256)
void wgrad_x3_kernel(const Params P, float* __restrict__ ws, int Cin, int Cout, int d, int s, int ntile_ci) {
  const int slice = blockIdx.y;
  int lsel = 0;
#pragma unroll
  for (int l = 1; l < MAXLV; ++l)
    if (l < P.nlevels && slice >= P.lv[l].slice0) lsel = l;
  Lv L = P.lv[0];
#pragma unroll
  for (int l = 1; l < MAXLV; ++l)
    if (l == lsel) L = P.lv[l];

  const int tco = blockIdx.x / ntile_ci, tci = blockIdx.x - tco * ntile_ci;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, kq = lane >> 4;
  const int co_base = tco * TCO + (wave & 1) * 32, ci_base = tci * TCI + (wave >> 1) * 16;
  const int HW = L.H * L.W, HoWo = L.Ho * L.Wo;
  const unsigned Tq = (unsigned)L.B * (unsigned)HoWo;
  const int ci = ci_base + r;
  const bool ci_ok = ci < Cin;

  f32x4 acc[2][NT], accs[2][NT];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[f][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      accs[f][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  const int c0 = (slice - L.slice0) * L.cps, c1 = (c0 + L.cps < L.nch) ? c0 + L.cps : L.nch;
  for (int ch = c0; ch < c1; ++ch) {
    // this lane's 8 consecutive pixels q0 .. q0 + 7 of the flattened (n, oy, ox) order
    const unsigned q0 = (unsigned)ch * KCH + (unsigned)kq * 8;
    unsigned n = q0 / (unsigned)HoWo;
    const unsigned p0 = q0 - n * (unsigned)HoWo;
    int oy = (int)(p0 / (unsigned)L.Wo), ox = (int)(p0 - (unsigned)oy * (unsigned)L.Wo);
    bool ok[8];
    long long gofs[8], xofs[8];                       // element offsets of (n, channel 0, pixel) in g / of (n, channel 0, s*oy, s*ox) in x
    int iy0[8], ix0[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ok[e] = q0 + (unsigned)e < Tq;
      gofs[e] = (long long)n * L.gbs + (long long)oy * L.Wo + ox;
      iy0[e] = oy * s;
      ix0[e] = ox * s;
      xofs[e] = (long long)n * L.xbs + (long long)iy0[e] * L.W + ix0[e];
      if (++ox == L.Wo) {
        ox = 0;
        if (++oy == L.Ho) { oy = 0; ++n; }
      }
    }
    u32x4 ahi[2], alo[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int co = co_base + 16 * f + r;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (ok[e] && co < Cout) ? L.g[gofs[e] + (long long)co * HoWo] : 0.f;
      split8(v, ahi[f], alo[f]);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int dy = NT == 1 ? 0 : (t / 3 - 1) * d, dx = NT == 1 ? 0 : (t % 3 - 1) * d;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int iy = iy0[e] + dy, ix = ix0[e] + dx;
        const bool in = ok[e] && ci_ok && iy >= 0 && iy < L.H && ix >= 0 && ix < L.W;
        v[e] = in ? L.x[xofs[e] + (long long)ci * HW + (long long)dy * L.W + dx] : 0.f;
      }
      u32x4 bhi, blo;
      split8(v, bhi, blo);
      const uint4 bh = __builtin_bit_cast(uint4, bhi), bl = __builtin_bit_cast(uint4, blo);
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const uint4 ah = __builtin_bit_cast(uint4, ahi[f]), al = __builtin_bit_cast(uint4, alo[f]);
        accs[f][t] = Mma16<f16_t>::mma(al, bh, accs[f][t]);
        accs[f][t] = Mma16<f16_t>::mma(ah, bl, accs[f][t]);
        acc[f][t] = Mma16<f16_t>::mma(ah, bh, acc[f][t]);
      }
    }
  }

  // partial block of this slice: lane holds rows co = 4 * kq + i of column ci = r
  const size_t E = (size_t)Cout * Cin * NT;
  float* out = ws + (size_t)slice * E;
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = co_base + 16 * f + 4 * kq + i;
      if (co < Cout && ci_ok) {
#pragma unroll
        for (int t = 0; t < NT; ++t) out[((size_t)co * Cin + ci) * NT + t] = acc[f][t][i] + accs[f][t][i];
      }
    }
}

// grad_w[e] = sum over the slices, in order, of partial[slice][e] * 2^-s(level of the slice);  threads beyond E: the bias gradient
// grad_b[co] = sum over the levels of (sum of the 32 first-stage sums) * 2^-s(level)
__global__ __launch_bounds__(256)
void wgrad_x3_reduce_kernel(const Params P, const float* __restrict__ ws, float* __restrict__ gw, long long E, float* __restrict__ gb, int Cout) {
  const long long idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx < E) {
    float sum = 0.f;
#pragma unroll
    for (int l = 0; l < MAXLV; ++l) {
      if (l >= P.nlevels) break;
      const float inv = P.lv[l].slot ? P.lv[l].slot[2] : 1.f;
      for (int sl = P.lv[l].slice0; sl < P.lv[l].slice0 + P.lv[l].nslices; ++sl) sum += ws[(size_t)sl * E + idx] * inv;
    }
    gw[idx] = sum;
    return;
  }
  const long long co = idx - (E + 255) / 256 * 256;
  if (!gb || co < 0 || co >= Cout) return;
  float total = 0.f;
#pragma unroll
  for (int l = 0; l < MAXLV; ++l) {
    if (l >= P.nlevels) break;
    if (!P.lv[l].bpart) continue;
    const float inv = P.lv[l].slot ? P.lv[l].slot[2] : 1.f;
    float t = 0.f;
    for (int j = 0; j < BIAS_NCH; ++j) t += P.lv[l].bpart[co * BIAS_NCH + j];
    total += t * inv;
  }
  gb[co] = total;
}

// the K split: -> number of slices (workspace = slices * Cout * Cin * taps floats), or -1 for a bad level list
static long long plan(const upf_wgrad_level* levels, const float* const* slots, const float* const* bparts, int nlevels, int Cin, int Cout,
                      int k, int dilation, int stride, Params& P) {
  if (!levels || nlevels < 1 || nlevels > MAXLV || Cin < 1 || Cout < 1 || (k != 1 && k != 3) || dilation < 1 || dilation > MAXD) return -1;
  if (!(stride == 1 || (stride == 2 && k == 3 && dilation == 1))) return -1;
  long long total_ch = 0;
  for (int l = 0; l < nlevels; ++l) {
    const upf_wgrad_level& u = levels[l];
    if (!u.x || !u.grad_pre || u.B < 1 || u.H < 1 || u.W < 1) return -1;
    Lv& L = P.lv[l];
    L.x = (const float*)u.x;
    L.g = (const float*)u.grad_pre;
    L.slot = slots ? slots[l] : nullptr;
    L.bpart = bparts ? bparts[l] : nullptr;
    L.B = u.B; L.H = u.H; L.W = u.W;
    L.Ho = (u.H - 1) / stride + 1;
    L.Wo = (u.W - 1) / stride + 1;
    L.xbs = u.x_batch_stride ? u.x_batch_stride : (long long)Cin * u.H * u.W;
    L.gbs = u.g_batch_stride ? u.g_batch_stride : (long long)Cout * L.Ho * L.Wo;
    if (L.xbs < (long long)Cin * u.H * u.W || L.gbs < (long long)Cout * L.Ho * L.Wo) return -1;
    const long long pix = (long long)u.B * L.Ho * L.Wo;
    if (pix + KCH >= (1ll << 31)) return -1;
    L.nch = (int)((pix + KCH - 1) / KCH);
    total_ch += L.nch;
  }
  P.nlevels = nlevels;
  const long long E = (long long)Cout * Cin * k * k;
  const long long tiles = (long long)cdiv(Cout, TCO) * cdiv(Cin, TCI);
  long long nsplit = 2048 / tiles;
  const long long by_bytes = (64ll << 20) / (E * 4);                  // at most 64 MB of partial blocks
  nsplit = nsplit > by_bytes ? by_bytes : nsplit;
  nsplit = nsplit > 256 ? 256 : (nsplit < 1 ? 1 : nsplit);
  long long cps = (total_ch + nsplit - 1) / nsplit;
  cps = cps < 4 ? 4 : cps;
  int s0 = 0;
  for (int l = 0; l < nlevels; ++l) {
    Lv& L = P.lv[l];
    L.cps = (int)cps;
    L.slice0 = s0;
    L.nslices = (int)((L.nch + cps - 1) / cps);
    s0 += L.nslices;
  }
  return s0;
}

}  // namespace x3bwd
}  // namespace upf

extern "C" int upf_act_grad_x3(const float* grad_y, long long gy_batch_stride, const float* y, long long y_batch_stride, float* grad_pre_scaled,
                               long long dst_batch_stride, float* bias_partial, float* scale_slot, int B, int C, int HW, float slope,
                               void* stream) {
  using namespace upf;
  UPF_REQUIRE(grad_y && grad_pre_scaled && scale_slot && B > 0 && C > 0 && HW > 0, UPF_EINVAL, "act_grad_x3: bad arguments");
  UPF_REQUIRE(slope >= 0.f && slope <= 1.f, UPF_EINVAL, "act_grad_x3: slope %g not in [0,1]", (double)slope);
  UPF_REQUIRE((long long)C * x3bwd::BIAS_NCH < (1ll << 31), UPF_EINVAL, "act_grad_x3: too many channels");
  const long long gbs = gy_batch_stride ? gy_batch_stride : (long long)C * HW, ybs = y_batch_stride ? y_batch_stride : (long long)C * HW,
                  dbs = dst_batch_stride ? dst_batch_stride : (long long)C * HW;
  UPF_REQUIRE(gbs >= (long long)C * HW && ybs >= (long long)C * HW && dbs >= (long long)C * HW, UPF_EINVAL, "act_grad_x3: batch stride below C*HW");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(C * x3bwd::BIAS_NCH));
  hipLaunchKernelGGL(x3bwd::slot_zero_kernel, dim3(1), dim3(64), 0, s, (uint32_t*)scale_slot);
  hipLaunchKernelGGL(x3bwd::grad_absmax_kernel, grid, dim3(256), 0, s, grad_y, gbs, y, ybs, (uint32_t*)scale_slot, B, HW, slope);
  hipLaunchKernelGGL(x3bwd::act_grad_x3_kernel, grid, dim3(256), 0, s, grad_y, gbs, y, ybs, grad_pre_scaled, dbs, bias_partial, scale_slot, B, HW, slope);
  return check_launch("act_grad_x3");
}

extern "C" int upf_conv_x3_pack_weights_dgrad(const float* w, void* w_packed, int Cin, int Cout, int kernel_size, void* stream) {
  using namespace upf;
  UPF_REQUIRE(w && w_packed && Cin > 0 && Cout > 0, UPF_EINVAL, "conv_x3_pack_weights_dgrad: bad arguments");
  UPF_REQUIRE(kernel_size == 3 || kernel_size == 1, UPF_EUNSUPPORTED, "conv_x3_pack_weights_dgrad: kernel_size %d (1 or 3)", kernel_size);
  const int ntaps = kernel_size * kernel_size;
  const long long total = (long long)ntaps * conv::pad32(Cin) * convx3::pad16(Cout) * 2;
  const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  const long long nw = (long long)Cout * Cin * ntaps;
  hipStream_t s = (hipStream_t)stream;
  convx3::launch_header_absmax(w, nw, w_packed, s);
  hipLaunchKernelGGL(x3bwd::pack_x3_dgrad_kernel, dim3(blocks), dim3(256), 0, s, w, (f16_t*)w_packed, Cin, Cout, ntaps);
  return check_launch("conv_x3_pack_weights_dgrad");
}

extern "C" int upf_conv_x3_dgrad(const float* grad_pre_scaled, long long g_batch_stride, const float* scale_slot, const float* w,
                                 void* w_packed_dgrad, const float* zero_bias, float* grad_x, long long gx_batch_stride, int B, int Cin,
                                 int Cout, int H, int W, int kernel_size, int dilation, int stride, void* stream) {
  using namespace upf;
  UPF_REQUIRE(grad_pre_scaled && scale_slot && grad_x, UPF_EINVAL, "conv_x3_dgrad: null pointer");
  UPF_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, UPF_EINVAL, "conv_x3_dgrad: bad shape B=%d Cin=%d Cout=%d H=%d W=%d", B, Cin, Cout, H, W);
  hipStream_t s = (hipStream_t)stream;
  if (stride == 1) {
    UPF_REQUIRE(w_packed_dgrad && zero_bias, UPF_EINVAL, "conv_x3_dgrad: stride 1 needs the packed operand and a zero bias of Cin floats");
    hipLaunchKernelGGL(x3bwd::dgrad_hdr_kernel, dim3(1), dim3(64), 0, s, (float*)w_packed_dgrad, scale_slot);
    return upf_conv_x3_forward(grad_pre_scaled, g_batch_stride, w_packed_dgrad, zero_bias, grad_x, gx_batch_stride, B, Cout, Cin, H, W,
                               kernel_size, dilation, 1, 0.f, 3, stream);
  }
  UPF_REQUIRE(stride == 2 && kernel_size == 3 && dilation == 1, UPF_EUNSUPPORTED, "conv_x3_dgrad: stride %d (1, or 2 for a 3x3 with dilation 1)", stride);
  UPF_REQUIRE(w, UPF_EINVAL, "conv_x3_dgrad: stride 2 needs the fp32 weights");
  UPF_REQUIRE(Cin <= 65535 && B <= 65535 && (long long)Cout * 36 <= 49152, UPF_EUNSUPPORTED, "conv_x3_dgrad: stride 2 with Cin %d, Cout %d, B %d", Cin, Cout, B);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long gbs = g_batch_stride ? g_batch_stride : (long long)Cout * Ho * Wo, xbs = gx_batch_stride ? gx_batch_stride : (long long)Cin * H * W;
  UPF_REQUIRE(gbs >= (long long)Cout * Ho * Wo && xbs >= (long long)Cin * H * W && (long long)H * W < (1ll << 30), UPF_EINVAL, "conv_x3_dgrad: bad strides / size");
  hipLaunchKernelGGL(x3bwd::dgrad_s2_kernel, dim3((unsigned)cdiv(H * W, 256), (unsigned)Cin, (unsigned)B), dim3(256), (size_t)Cout * 36, s,
                     grad_pre_scaled, gbs, w, grad_x, xbs, scale_slot, Cin, Cout, H, W, Ho, Wo);
  return check_launch("conv_x3_dgrad");
}

extern "C" int upf_conv_x3_wgrad_workspace_bytes(const upf_wgrad_level* levels, int nlevels, int Cin, int Cout, int kernel_size,
                                                 int dilation, int stride, long long* bytes) {
  using namespace upf;
  UPF_REQUIRE(bytes, UPF_EINVAL, "conv_x3_wgrad_workspace_bytes: null pointer");
  x3bwd::Params P;
  const long long slices = x3bwd::plan(levels, nullptr, nullptr, nlevels, Cin, Cout, kernel_size, dilation, stride, P);
  UPF_REQUIRE(slices > 0, UPF_EINVAL, "conv_x3_wgrad_workspace_bytes: bad level list / geometry (1..6 levels; 1x1, or 3x3 with dilation 1..16 at stride 1 or dilation 1 at stride 2)");
  *bytes = slices * (long long)Cout * Cin * kernel_size * kernel_size * 4;
  return 0;
}

extern "C" int upf_conv_x3_wgrad(const upf_wgrad_level* levels, const float* const* scale_slots, int nlevels, float* grad_w, void* workspace,
                                 int Cin, int Cout, int kernel_size, int dilation, int stride, const float* const* bias_partials,
                                 float* grad_bias, void* stream) {
  using namespace upf;
  UPF_REQUIRE(grad_w && workspace, UPF_EINVAL, "conv_x3_wgrad: null pointer");
  UPF_REQUIRE(!grad_bias || bias_partials, UPF_EINVAL, "conv_x3_wgrad: grad_bias needs the first-stage sums of every level");
  x3bwd::Params P;
  const long long slices = x3bwd::plan(levels, scale_slots, bias_partials, nlevels, Cin, Cout, kernel_size, dilation, stride, P);
  UPF_REQUIRE(slices > 0, UPF_EINVAL, "conv_x3_wgrad: bad level list / geometry (1..6 levels; 1x1, or 3x3 with dilation 1..16 at stride 1 or dilation 1 at stride 2)");
  hipStream_t s = (hipStream_t)stream;
  const int ntile_ci = cdiv(Cin, x3bwd::TCI);
  const dim3 grid((unsigned)(cdiv(Cout, x3bwd::TCO) * ntile_ci), (unsigned)slices);
  if (kernel_size == 3)
    hipLaunchKernelGGL(x3bwd::wgrad_x3_kernel<9>, grid, dim3(256), 0, s, P, (float*)workspace, Cin, Cout, dilation, stride, ntile_ci);
  else
    hipLaunchKernelGGL(x3bwd::wgrad_x3_kernel<1>, grid, dim3(256), 0, s, P, (float*)workspace, Cin, Cout, 1, stride, ntile_ci);
  const long long E = (long long)Cout * Cin * kernel_size * kernel_size;
  const long long nb = (E + 255) / 256 + (grad_bias ? cdiv(Cout, 256) : 0);
  hipLaunchKernelGGL(x3bwd::wgrad_x3_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, s, P, (const float*)workspace, grad_w, E, grad_bias, Cout);
  return check_launch("conv_x3_wgrad");
}
