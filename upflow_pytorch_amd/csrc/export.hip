// Evaluation results on the device (include/upflow_hip.h has the contract): from a dense fp32 prediction [B,2,H,W], and
// optionally a validity plane, the payloads of the three files the reference's runner saves per pair —
//   kitti  uint16 [B,H,W,3]   the KITTI flow PNG's samples (utils/flow_io.py: write_kitti_png_file's encode)
//   rgb    uint8  [B,H,W,3]   the Middlebury colour rendering (tools.flow_to_image)
//   flo    fp32   [B,H,W,2]   the body of a .flo file
// in ONE launch, or in two when the colour scale is the item's own largest radius:
//   1. maxrad: every workgroup leaves the largest fp32 radius of its pixels of ONE item in the workspace;
//   2. render: every workgroup folds its item's partial maxima (a maximum: any order gives the same bits) and writes.
// No atomics, no workgroup waits for another.  A lane takes G = 4 consecutive pixels of an item: 16 bytes of each input plane,
// 24 / 12 / 32 contiguous bytes of the outputs, moved with the widest access their address allows (planes and items start
// wherever H * W puts them); the ragged tail of H * W goes pixel by pixel in the same kernel.
//
// Built with -ffp-contract=off: the arithmetic is the host writer's and the reference renderer's operation by operation (fp32
// up to the maximum, float64 after it; tests/_export_model.py states it in numpy).  sqrtf / sqrt / the divisions are correctly
// rounded as hipcc lowers them without fast-math; atan2 is the one operation that is not an IEEE-exact one.
#include "loss_common.hpp"

namespace upf {
namespace exportk {

using loss::NT;
constexpr int G = 4;                                         // pixels per lane
constexpr int MAX_PARTIALS = 1024;                           // workgroups per item of the maxrad launch (they stride over the rest)

// ---- moving G pixels with the widest access the address allows (the same choice in every lane: addresses differ by 16 * k) ----
__device__ __forceinline__ void load4(const float* __restrict__ p, float (&x)[G]) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 15) == 0) {
    const float4 t = *(const float4*)p;
    x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
  } else if ((a & 7) == 0) {
    const float2 t = *(const float2*)p, s = *(const float2*)(p + 2);
    x[0] = t.x; x[1] = t.y; x[2] = s.x; x[3] = s.y;
  } else {
    x[0] = p[0]; x[1] = p[1]; x[2] = p[2]; x[3] = p[3];
  }
}

struct Dwords3 { uint32_t x, y, z; };

// 12 uint16 samples (the low halves of k[]) -> 24 bytes
__device__ __forceinline__ void store_kitti4(uint16_t* __restrict__ q, const uint32_t (&k)[3 * G]) {
  const uintptr_t a = (uintptr_t)q;
  if ((a & 3) == 0) {
    uint32_t w[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = k[2 * i] | (k[2 * i + 1] << 16);
    if ((a & 7) == 0) {
      uint2* d = (uint2*)q;
      d[0] = make_uint2(w[0], w[1]); d[1] = make_uint2(w[2], w[3]); d[2] = make_uint2(w[4], w[5]);
    } else {
      uint32_t* d = (uint32_t*)q;
#pragma unroll
      for (int i = 0; i < 6; ++i) d[i] = w[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 3 * G; ++i) q[i] = (uint16_t)k[i];
  }
}

// 12 bytes (the low bytes of c[])
__device__ __forceinline__ void store_rgb4(uint8_t* __restrict__ q, const uint32_t (&c)[3 * G]) {
  if (((uintptr_t)q & 3) == 0) {
    Dwords3 w;
    w.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    w.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
    w.z = c[8] | (c[9] << 8) | (c[10] << 16) | (c[11] << 24);
    *(Dwords3*)q = w;
  } else {
#pragma unroll
    for (int i = 0; i < 3 * G; ++i) q[i] = (uint8_t)c[i];
  }
}

// (u, v) x 4 -> 32 bytes
__device__ __forceinline__ void store_flo4(float* __restrict__ q, const float (&u)[G], const float (&v)[G]) {
  const uintptr_t a = (uintptr_t)q;
  if ((a & 15) == 0) {
    float4* d = (float4*)q;
    d[0] = make_float4(u[0], v[0], u[1], v[1]); d[1] = make_float4(u[2], v[2], u[3], v[3]);
  } else if ((a & 7) == 0) {
    float2* d = (float2*)q;
#pragma unroll
    for (int i = 0; i < G; ++i) d[i] = make_float2(u[i], v[i]);
  } else {
#pragma unroll
    for (int i = 0; i < G; ++i) { q[2 * i] = u[i]; q[2 * i + 1] = v[i]; }
  }
}

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------
// a pixel that is rendered black and counts as (0, 0) for the item's maximum: unknown (|u| or |v| > 1e7, +-inf among them) or NaN
__device__ __forceinline__ bool is_black(float u, float v) { return fabsf(u) > 1e7f || fabsf(v) > 1e7f || u != u || v != v; }

__device__ __forceinline__ float radius(float u, float v) { return is_black(u, v) ? 0.f : sqrtf(u * u + v * v); }

// np.clip(float64(x) * 64 + 2^15, 0, 65535).astype(uint16); a NaN never gets here
__device__ __forceinline__ uint32_t kitti_sample(float x) {
  double t = (double)x * 64.0 + 32768.0;
  t = t < 0.0 ? 0.0 : (t > 65535.0 ? 65535.0 : t);
  return (uint32_t)t;
}

__device__ __forceinline__ void kitti_pixel(float u, float v, float valid, uint32_t* k) {
  if (u != u || v != v) { k[0] = k[1] = k[2] = 0; return; }
  k[0] = kitti_sample(u);
  k[1] = kitti_sample(v);
  k[2] = (valid != valid) ? 0u : (uint32_t)fminf(fmaxf(valid, 0.f), 65535.f);          // truncated; out of range saturates
}

// entry k = 0..54 of the Middlebury wheel: segments of 15, 6, 4, 11, 13, 6 entries, ramps floor(255 * i / n)
__device__ __forceinline__ void wheel(int k, int& r, int& g, int& b) {
  if (k < 15) { r = 255; g = 255 * k / 15; b = 0; }
  else if (k < 21) { r = 255 - 255 * (k - 15) / 6; g = 255; b = 0; }
  else if (k < 25) { r = 0; g = 255; b = 255 * (k - 21) / 4; }
  else if (k < 36) { r = 0; g = 255 - 255 * (k - 25) / 11; b = 255; }
  else if (k < 49) { r = 255 * (k - 36) / 13; g = 0; b = 255; }
  else { r = 255; g = 0; b = 255 - 255 * (k - 49) / 6; }
}

__device__ __forceinline__ uint32_t shade(double c0, double c1, double f, double rad) {
  double c = (1.0 - f) * (c0 / 255.0) + f * (c1 / 255.0);
  c = (rad <= 1.0) ? 1.0 - rad * (1.0 - c) : c * 0.75;
  return (uint32_t)(int)floor(255.0 * c);
}

// d = double(maxrad) + 2^-52
__device__ __forceinline__ void rgb_pixel(float uf, float vf, double d, uint32_t* c) {
  if (is_black(uf, vf)) { c[0] = c[1] = c[2] = 0; return; }
  const double u = (double)uf / d, v = (double)vf / d;
  const double rad = sqrt(u * u + v * v);
  const double a = atan2(-v, -u) / 3.141592653589793;
  const double fk = (a + 1.0) / 2.0 * 54.0 + 1.0;
  const double fl = floor(fk);
  int k0 = (int)fl;
  k0 = k0 < 1 ? 1 : (k0 > 55 ? 55 : k0);                     // (fk is in [1, 55] for an atan2 within [-pi, pi])
  const int k1 = (k0 == 55) ? 1 : k0 + 1;
  const double f = fk - fl;
  int r0, g0, b0, r1, g1, b1;
  wheel(k0 - 1, r0, g0, b0);
  wheel(k1 - 1, r1, g1, b1);
  c[0] = shade((double)r0, (double)r1, f, rad);
  c[1] = shade((double)g0, (double)g1, f, rad);
  c[2] = shade((double)b0, (double)b1, f, rad);
}

// largest v over the workgroup, in every thread (v >= 0, never a NaN); sh: NT / 64 floats
__device__ __forceinline__ float block_max(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int k = 1; k < NT / 64; ++k) r = fmaxf(r, sh[k]);
  return r;
}

// partials[b * mb + j] = largest radius over the lane groups j, j + mb, ... of item b; grid = B * mb workgroups
__global__ __launch_bounds__(NT)
void maxrad_kernel(const float* __restrict__ pred, float* __restrict__ partials, uint32_t HW, uint32_t mb) {
  __shared__ float sh[NT / 64];
  const uint32_t b = blockIdx.x / mb, j = blockIdx.x - b * mb;
  const float* __restrict__ pu = pred + (size_t)b * 2 * HW;
  const float* __restrict__ pv = pu + HW;
  float m = 0.f;
  for (unsigned long long p = ((unsigned long long)j * NT + threadIdx.x) * G; p < HW; p += (unsigned long long)mb * NT * G) {
    if (p + G <= HW) {
      float u[G], v[G];
      load4(pu + p, u);
      load4(pv + p, v);
#pragma unroll
      for (int i = 0; i < G; ++i) m = fmaxf(m, radius(u[i], v[i]));
    } else {
      for (uint32_t q = (uint32_t)p; q < HW; ++q) m = fmaxf(m, radius(pu[q], pv[q]));
    }
  }
  m = block_max(m, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

// grid = B * bpi workgroups, bpi = ceil(HW / (NT * G)); any of kitti / rgb / flo may be null; partials: null = the scale is max_rad
__global__ __launch_bounds__(NT)
void render_kernel(const float* __restrict__ pred, const float* __restrict__ valid, uint16_t* __restrict__ kitti,
                   uint8_t* __restrict__ rgb, float* __restrict__ flo, const float* __restrict__ partials, uint32_t mb,
                   float max_rad, uint32_t HW, uint32_t bpi) {
  __shared__ float sh[NT / 64];
  const uint32_t b = blockIdx.x / bpi, j = blockIdx.x - b * bpi;
  float maxrad = max_rad;
  if (rgb && partials) {                                     // (uniform over the grid)
    float m = 0.f;
    for (uint32_t i = threadIdx.x; i < mb; i += NT) m = fmaxf(m, partials[(size_t)b * mb + i]);
    maxrad = block_max(m, sh);
  }
  const double d = (double)maxrad + 2.220446049250313e-16;
  const uint32_t p = (j * NT + threadIdx.x) * G;             // < HW + NT * G: no wrap below 2^31 pixels
  if (p >= HW) return;
  const size_t item = (size_t)b * HW;
  const float* __restrict__ pu = pred + 2 * item + p;
  const float* __restrict__ pv = pu + HW;
  const float* __restrict__ pm = valid ? valid + item + p : nullptr;
  const size_t o = item + p;
  if (p + G <= HW) {
    float u[G], v[G], m[G] = {1.f, 1.f, 1.f, 1.f};
    load4(pu, u);
    load4(pv, v);
    if (pm) load4(pm, m);
    if (kitti) {
      uint32_t k[3 * G];
#pragma unroll
      for (int i = 0; i < G; ++i) kitti_pixel(u[i], v[i], m[i], k + 3 * i);
      store_kitti4(kitti + 3 * o, k);
    }
    if (rgb) {
      uint32_t c[3 * G];
#pragma unroll
      for (int i = 0; i < G; ++i) rgb_pixel(u[i], v[i], d, c + 3 * i);
      store_rgb4(rgb + 3 * o, c);
    }
    if (flo) store_flo4(flo + 2 * o, u, v);
  } else {
    for (uint32_t i = 0; p + i < HW; ++i) {
      const float u = pu[i], v = pv[i];
      if (kitti) {
        uint32_t k[3];
        kitti_pixel(u, v, pm ? pm[i] : 1.f, k);
        uint16_t* q = kitti + 3 * (o + i);
        q[0] = (uint16_t)k[0]; q[1] = (uint16_t)k[1]; q[2] = (uint16_t)k[2];
      }
      if (rgb) {
        uint32_t c[3];
        rgb_pixel(u, v, d, c);
        uint8_t* q = rgb + 3 * (o + i);
        q[0] = (uint8_t)c[0]; q[1] = (uint8_t)c[1]; q[2] = (uint8_t)c[2];
      }
      if (flo) { flo[2 * (o + i)] = u; flo[2 * (o + i) + 1] = v; }
    }
  }
}

static int check_shape(const char* what, int B, int H, int W, long long* n) {
  UPF_REQUIRE(B > 0 && H > 0 && W > 0, UPF_EINVAL, "%s: B, H, W must be positive (got %d, %d, %d)", what, B, H, W);
  *n = (long long)B * H * W;
  UPF_REQUIRE(*n < (1ll << 31), UPF_EUNSUPPORTED, "%s: %lld pixels (2^31 or more)", what, *n);
  return UPF_OK;
}

// workgroups per item: of the render launch, and of the maxrad launch
static long long render_blocks(long long HW) { return (HW + NT * G - 1) / (NT * G); }
static long long maxrad_blocks(long long HW) {
  const long long b = render_blocks(HW);
  return b > MAX_PARTIALS ? MAX_PARTIALS : b;
}

}  // namespace exportk
}  // namespace upf

extern "C" int upf_flow_export_workspace_bytes(int B, int H, int W, long long* bytes) {
  using namespace upf;
  UPF_REQUIRE(bytes, UPF_EINVAL, "flow_export_workspace_bytes: null pointer");
  long long n;
  if (int rc = exportk::check_shape("flow_export_workspace_bytes", B, H, W, &n)) return rc;
  *bytes = (long long)B * exportk::maxrad_blocks((long long)H * W) * (long long)sizeof(float);
  return UPF_OK;
}

extern "C" int upf_flow_export(const float* pred, const float* valid, unsigned short* kitti, unsigned char* rgb, float* flo,
                               float max_rad, void* workspace, int B, int H, int W, void* stream) {
  using namespace upf;
  UPF_REQUIRE(pred, UPF_EINVAL, "flow_export: null prediction");
  UPF_REQUIRE(kitti || rgb || flo, UPF_EINVAL, "flow_export: no output requested (kitti, rgb and flo are all null)");
  long long n;
  if (int rc = exportk::check_shape("flow_export", B, H, W, &n)) return rc;
  const bool per_item = rgb && !(max_rad > 0.f);             // (a NaN max_rad: per item)
  UPF_REQUIRE(!per_item || workspace, UPF_EINVAL, "flow_export: a per-item colour scale needs the workspace");
  UPF_REQUIRE(aligned_to(pred, 4) && aligned_to(valid, 4) && aligned_to(kitti, 2) && aligned_to(flo, 4) && aligned_to(workspace, 4),
              UPF_EALIGN, "flow_export: pred, valid, flo and workspace must be 4-byte, kitti 2-byte aligned");
  const long long HW = (long long)H * W;
  const long long bpi = exportk::render_blocks(HW), mb = exportk::maxrad_blocks(HW);
  if (per_item) {
    hipLaunchKernelGGL(exportk::maxrad_kernel, dim3((unsigned)(B * mb)), dim3(exportk::NT), 0, (hipStream_t)stream, pred,
                       (float*)workspace, (uint32_t)HW, (uint32_t)mb);
    if (int rc = check_launch("flow_export (maxrad)")) return rc;
  }
  hipLaunchKernelGGL(exportk::render_kernel, dim3((unsigned)(B * bpi)), dim3(exportk::NT), 0, (hipStream_t)stream, pred, valid,
                     kitti, rgb, flo, per_item ? (const float*)workspace : (const float*)nullptr, (uint32_t)mb, max_rad,
                     (uint32_t)HW, (uint32_t)bpi);
  return check_launch("flow_export");
}
