// KITTI error maps on the device (include/upflow_hip.h has the contract): the devkit's rendering of |pred - gt| against the
// ground truth (the reference's tools.lib_to_show_flow.flow_error_image_np), from the prediction and the two uint16 ground-truth
// PNG payloads as the files hold them, as the uint8 [B,H,W,3] payload of an 8-bit RGB PNG.  ONE launch, no workspace:
//   dilate = 0   render_kernel: a lane takes G = 4 consecutive pixels of an item — 16 bytes of each prediction plane, 24 bytes of
//                each ground-truth array, 12 bytes out — moved with the widest access their address allows (items and planes start
//                wherever H * W puts them); the ragged tail of H * W goes pixel by pixel in the same kernel.
//   dilate = r   dilate_kernel: a workgroup renders a TH x TW tile plus its halo of r pixels ONCE into LDS (colour and validity in
//                one word), takes per row the last valid word of every horizontal window, then per pixel the last valid row of its
//                vertical window — "last in raster order" is separable, so a pixel costs 2 * (2r + 1) LDS words, not (2r + 1)^2 —
//                and writes 4 consecutive pixels per lane.
// No atomics, no workgroup waits for another, nothing but rgb is written: the same bytes run to run.
//
// Built with -ffp-contract=off: each per-pixel step is one separately rounded fp32 operation, the divisions are IEEE divisions and
// the square root is sqrtf, correctly rounded as hipcc lowers them without fast-math (tests/_errmap_model.py states it in numpy).
#include "loss_common.hpp"
#include "kitti_gt.hpp"

namespace upf {
namespace errmap {

using loss::NT;
constexpr int G = 4;                                         // pixels per lane
constexpr int RMAX = 4;                                      // largest dilate radius
constexpr int TH = 32, TW = 64;                              // the dilate kernel's tile of output pixels
constexpr int AWS = TW + 2 * RMAX;                           // the row pitch of its halo image in LDS (words)
static_assert(TW % G == 0 && (AWS * 4) % 16 == 0, "16-byte LDS reads of 4 pixels");

// the log-colour bins: err in [LO[i], LO[i + 1]) takes row i; LO[10] = 1e9 (all exact in fp32)
constexpr int BINS = 10;
__device__ constexpr float LO[BINS] = {0.f, 0.0625f, 0.125f, 0.25f, 0.5f, 1.f, 2.f, 4.f, 8.f, 16.f};
constexpr float ERR_END = 1e9f;
// the reference's colour table, and rint(255 * (float32(c / 255) * 0.5)) of each entry: what an occluded pixel gets
__device__ constexpr uint8_t FULL[BINS][3] = {{49, 54, 149},   {69, 117, 180},  {116, 173, 209}, {171, 217, 233}, {224, 243, 248},
                                   {254, 224, 144}, {253, 174, 97},  {244, 109, 67},  {215, 48, 39},   {165, 0, 38}};
__device__ constexpr uint8_t HALF[BINS][3] = {{25, 27, 75},    {35, 59, 90},    {58, 87, 105},   {86, 109, 117},  {112, 122, 124},
                                   {127, 112, 72},  {127, 87, 49},   {122, 55, 34},   {108, 24, 20},   {83, 0, 19}};

// R | G << 8 | B << 16 of a table row
__host__ __device__ constexpr uint32_t packed(const uint8_t (&t)[BINS][3], int i) {
  return (uint32_t)t[i][0] | ((uint32_t)t[i][1] << 8) | ((uint32_t)t[i][2] << 16);
}

constexpr uint32_t VALID = 1u << 24;                         // bit 24 of a rendered word: m_occ != 0

// np.minimum: a NaN on either side gives a NaN
__device__ __forceinline__ float min_nan(float a, float b) {
  float r = a < b ? a : b;                                   // (b where b is a NaN)
  if (a != a) r = a;
  return r;
}

// one pixel: R, G, B of gt_occ, B of gt_noc (low 16 bits) and the prediction -> R | G << 8 | B << 16 | VALID; 0 where m_occ == 0
__device__ __forceinline__ uint32_t pixel(uint32_t ro, uint32_t go, uint32_t bo, uint32_t bn, float pu, float pv, int log_colors) {
  const float gu = kitti::gt_flow(ro), gv = kitti::gt_flow(go);
  const float m_occ = (float)kitti::gt_mask(bo), m_noc = (float)kitti::gt_mask(bn);
  if (!(m_occ != 0.f)) return 0u;
  const bool noc = m_noc == 1.f;
  const float du = pu - gu, dv = pv - gv;
  const float diff = sqrtf(du * du + dv * dv);
  uint32_t c = 0u;
  if (log_colors) {
    const float mag = sqrtf(gu * gu + gv * gv);
    const float err = min_nan(diff / 3.0f, (20.0f * diff) / (mag + 1e-7f));
    if (err >= LO[0] && err < ERR_END) {                     // (false for a NaN: no bin, black)
      uint32_t cf = packed(FULL, 0), ch = packed(HALF, 0);
#pragma unroll
      for (int i = 1; i < BINS; ++i)
        if (err >= LO[i]) { cf = packed(FULL, i); ch = packed(HALF, i); }
      c = noc ? cf : ch;
    }
  } else {
    const float e = min_nan(diff, 5.0f) / 5.0f;
    const uint32_t b = (e != e) ? 0u : (uint32_t)rint((double)e * 255.0);
    c = noc ? b * 0x010101u : b;                             // an occluded pixel is red
  }
  return c | VALID;
}

// ---- moving G pixels with the widest access the address allows (the same choice in every lane: addresses differ by a multiple
// of 16, 24 and 12 bytes) ---------------------------------------------------------------------------------------------------------
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

// 12 uint16 samples (4 pixels of a ground-truth array) -> s[]
__device__ __forceinline__ void load_gt4(const uint16_t* __restrict__ p, uint32_t (&s)[3 * G]) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 3) == 0) {
    uint32_t w[6];
    if ((a & 7) == 0) {
      const uint2* q = (const uint2*)p;
      const uint2 t0 = q[0], t1 = q[1], t2 = q[2];
      w[0] = t0.x; w[1] = t0.y; w[2] = t1.x; w[3] = t1.y; w[4] = t2.x; w[5] = t2.y;
    } else {
      const uint32_t* q = (const uint32_t*)p;
#pragma unroll
      for (int i = 0; i < 6; ++i) w[i] = q[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) { s[2 * i] = w[i] & 0xffffu; s[2 * i + 1] = w[i] >> 16; }
  } else {
#pragma unroll
    for (int i = 0; i < 3 * G; ++i) s[i] = p[i];
  }
}

struct Dwords3 { uint32_t x, y, z; };

// 4 rendered words -> 12 bytes at q: three dwords, or six halves, or a byte, five halves and a byte
__device__ __forceinline__ void store_rgb4(uint8_t* __restrict__ q, const uint32_t (&c)[G]) {
  const uint32_t c0 = c[0] & 0xffffffu, c1 = c[1] & 0xffffffu, c2 = c[2] & 0xffffffu, c3 = c[3] & 0xffffffu;
  Dwords3 w;
  w.x = c0 | (c1 << 24);
  w.y = (c1 >> 8) | (c2 << 16);
  w.z = (c2 >> 16) | (c3 << 8);
  const uintptr_t a = (uintptr_t)q;
  if ((a & 3) == 0) {
    *(Dwords3*)q = w;
  } else if ((a & 1) == 0) {
    uint16_t* d = (uint16_t*)q;
    d[0] = (uint16_t)w.x; d[1] = (uint16_t)(w.x >> 16); d[2] = (uint16_t)w.y; d[3] = (uint16_t)(w.y >> 16);
    d[4] = (uint16_t)w.z; d[5] = (uint16_t)(w.z >> 16);
  } else {
    uint16_t* d = (uint16_t*)(q + 1);
    q[0] = (uint8_t)w.x;
    d[0] = (uint16_t)(w.x >> 8); d[1] = (uint16_t)((w.x >> 24) | (w.y << 8)); d[2] = (uint16_t)(w.y >> 8);
    d[3] = (uint16_t)((w.y >> 24) | (w.z << 8)); d[4] = (uint16_t)(w.z >> 8);
    q[11] = (uint8_t)(w.z >> 24);
  }
}

__device__ __forceinline__ void store_rgb1(uint8_t* __restrict__ q, uint32_t c) {
  q[0] = (uint8_t)c; q[1] = (uint8_t)(c >> 8); q[2] = (uint8_t)(c >> 16);
}

// ---- dilate = 0: grid = B * bpi workgroups, bpi = ceil(HW / (NT * G)) ---------------------------------------------------------------
__global__ __launch_bounds__(NT)
void render_kernel(const float* __restrict__ pred, const uint16_t* __restrict__ occ, const uint16_t* __restrict__ noc,
                   uint8_t* __restrict__ rgb, int log_colors, uint32_t HW, uint32_t bpi) {
  const uint32_t b = blockIdx.x / bpi, j = blockIdx.x - b * bpi;
  const uint32_t p = (j * NT + threadIdx.x) * G;             // < HW + NT * G: no wrap below 2^31 pixels
  if (p >= HW) return;
  const size_t item = (size_t)b * HW, o = item + p;
  const float* __restrict__ pu = pred + 2 * item + p;
  const float* __restrict__ pv = pu + HW;
  if (p + G <= HW) {
    float u[G], v[G];
    uint32_t so[3 * G], sn[3 * G], c[G];
    load4(pu, u);
    load4(pv, v);
    load_gt4(occ + 3 * o, so);
    load_gt4(noc + 3 * o, sn);
#pragma unroll
    for (int i = 0; i < G; ++i) c[i] = pixel(so[3 * i], so[3 * i + 1], so[3 * i + 2], sn[3 * i + 2], u[i], v[i], log_colors);
    store_rgb4(rgb + 3 * o, c);
  } else {
    for (uint32_t i = 0; p + i < HW; ++i) {
      const size_t g = 3 * (o + i);
      store_rgb1(rgb + g, pixel(occ[g], occ[g + 1], occ[g + 2], noc[g + 2], pu[i], pv[i], log_colors));
    }
  }
}

// ---- dilate = r in 1..RMAX: grid = B * tiles_y * tiles_x workgroups, one TH x TW tile each ------------------------------------------
__global__ __launch_bounds__(NT)
void dilate_kernel(const float* __restrict__ pred, const uint16_t* __restrict__ occ, const uint16_t* __restrict__ noc,
                   uint8_t* __restrict__ rgb, int log_colors, int r, int H, int W, uint32_t tiles_x, uint32_t tiles_y) {
  // sa: the rendered words of rows y0 - r .. y0 + TH + r and columns x0 - r .. x0 + TW + r; column x0 + k sits at word RMAX + k of
  //     its row, so that the 4 pixels of a lane are one aligned 16-byte read.  Outside the image: 0 (not valid).
  // sb: per row of sa and column x0 + k, k < TW: the valid word with the greatest x' in |x' - x| <= r, else 0.
  __shared__ __attribute__((aligned(16))) uint32_t sa[(TH + 2 * RMAX) * AWS];
  __shared__ __attribute__((aligned(16))) uint32_t sb[(TH + 2 * RMAX) * TW];
  const uint32_t tiles = tiles_x * tiles_y;
  const uint32_t b = blockIdx.x / tiles, t = blockIdx.x - b * tiles, ty = t / tiles_x, tx = t - ty * tiles_x;
  const int y0 = (int)ty * TH, x0 = (int)tx * TW;
  const int AH = TH + 2 * r, AW = TW + 2 * r, off = RMAX - r;
  const size_t HW = (size_t)H * W, item = (size_t)b * HW;
  for (int i = threadIdx.x; i < AH * AW; i += NT) {
    const int ay = i / AW, ax = i - ay * AW;
    const int y = y0 - r + ay, x = x0 - r + ax;
    uint32_t w = 0u;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t p = (size_t)y * W + x, g = 3 * (item + p);
      const float* __restrict__ pu = pred + 2 * item + p;
      w = pixel(occ[g], occ[g + 1], occ[g + 2], noc[g + 2], pu[0], pu[HW], log_colors);
    }
    sa[ay * AWS + off + ax] = w;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < AH * TW; i += NT) {
    const int ay = i / TW, k = i - ay * TW;
    const uint32_t* __restrict__ row = sa + ay * AWS + off + k;              // columns x - r .. x + r of x = x0 + k
    uint32_t w = 0u;
    for (int d = 0; d <= 2 * r; ++d) {                                       // ascending: the greatest x' is kept
      const uint32_t v = row[d];
      w = (v & VALID) ? v : w;
    }
    sb[i] = w;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TH * (TW / G); i += NT) {
    const int ly = i / (TW / G), lx = (i - ly * (TW / G)) * G;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const uint4 own = *(const uint4*)(sa + (ly + r) * AWS + RMAX + lx);
    uint32_t c[G] = {own.x, own.y, own.z, own.w};
    if (!(own.x & own.y & own.z & own.w & VALID)) {
      uint32_t w[G] = {0u, 0u, 0u, 0u};
      for (int d = 0; d <= 2 * r; ++d) {                                     // rows y - r .. y + r, ascending: the greatest y'
        const uint4 v = *(const uint4*)(sb + (ly + d) * TW + lx);
        w[0] = (v.x & VALID) ? v.x : w[0];
        w[1] = (v.y & VALID) ? v.y : w[1];
        w[2] = (v.z & VALID) ? v.z : w[2];
        w[3] = (v.w & VALID) ? v.w : w[3];
      }
#pragma unroll
      for (int k = 0; k < G; ++k) c[k] = (c[k] & VALID) ? c[k] : w[k];
    }
    uint8_t* __restrict__ q = rgb + 3 * (item + (size_t)y * W + x);
    if (x + G <= W) {
      store_rgb4(q, c);
    } else {
      for (int k = 0; x + k < W; ++k) store_rgb1(q + 3 * k, c[k]);
    }
  }
}

static int check_shape(const char* what, int B, int H, int W, int dilate, long long* n) {
  UPF_REQUIRE(B > 0 && H > 0 && W > 0, UPF_EINVAL, "%s: B, H, W must be positive (got %d, %d, %d)", what, B, H, W);
  UPF_REQUIRE(dilate >= 0 && dilate <= RMAX, UPF_EINVAL, "%s: dilate must be in 0..%d (got %d)", what, RMAX, dilate);
  *n = (long long)B * H * W;
  UPF_REQUIRE(*n < (1ll << 31), UPF_EUNSUPPORTED, "%s: %lld pixels (2^31 or more)", what, *n);
  return UPF_OK;
}

// the bytes of workspace a call needs: none — the dilated map goes through LDS
static long long workspace_bytes(int B, int H, int W, int dilate) { return 0; }

}  // namespace errmap
}  // namespace upf

extern "C" int upf_flow_error_image_workspace_bytes(int B, int H, int W, int dilate, long long* bytes) {
  using namespace upf;
  UPF_REQUIRE(bytes, UPF_EINVAL, "flow_error_image_workspace_bytes: null pointer");
  long long n;
  if (int rc = errmap::check_shape("flow_error_image_workspace_bytes", B, H, W, dilate, &n)) return rc;
  *bytes = errmap::workspace_bytes(B, H, W, dilate);
  return UPF_OK;
}

extern "C" int upf_flow_error_image(const float* pred, const unsigned short* gt_occ, const unsigned short* gt_noc,
                                    unsigned char* rgb, int log_colors, int dilate, void* workspace, int B, int H, int W,
                                    void* stream) {
  using namespace upf;
  UPF_REQUIRE(pred && gt_occ && gt_noc && rgb, UPF_EINVAL, "flow_error_image: null pointer");
  long long n;
  if (int rc = errmap::check_shape("flow_error_image", B, H, W, dilate, &n)) return rc;
  UPF_REQUIRE(workspace || errmap::workspace_bytes(B, H, W, dilate) == 0, UPF_EINVAL, "flow_error_image: the workspace is needed and null");
  UPF_REQUIRE(aligned_to(pred, 8) && aligned_to(gt_occ, 4) && aligned_to(gt_noc, 4), UPF_EALIGN,
              "flow_error_image: pred must be 8-byte, the ground truth 4-byte aligned");
  const long long HW = (long long)H * W;
  if (dilate == 0) {
    const long long bpi = (HW + errmap::NT * errmap::G - 1) / (errmap::NT * errmap::G);
    hipLaunchKernelGGL(errmap::render_kernel, dim3((unsigned)(B * bpi)), dim3(errmap::NT), 0, (hipStream_t)stream, pred, gt_occ,
                       gt_noc, rgb, log_colors, (uint32_t)HW, (uint32_t)bpi);
  } else {
    const long long tx = (W + errmap::TW - 1) / errmap::TW, ty = (H + errmap::TH - 1) / errmap::TH;
    hipLaunchKernelGGL(errmap::dilate_kernel, dim3((unsigned)(B * tx * ty)), dim3(errmap::NT), 0, (hipStream_t)stream, pred, gt_occ,
                       gt_noc, rgb, log_colors, dilate, H, W, (uint32_t)tx, (uint32_t)ty);
  }
  return check_launch("flow_error_image");
}
