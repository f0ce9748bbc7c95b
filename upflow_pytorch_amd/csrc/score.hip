// KITTI scoring on the device (include/upflow_hip.h has the contract): the four numbers of dataset/kitti_dataset.py's
// Evaluation_bench — average end-point error over all / non-occluded / occluded-only pixels and the outlier rate F1 — of one
// batch, from the prediction and the two uint16 ground-truth PNG payloads as the files hold them, in two launches:
//   1. partials: every workgroup strides over pairs of adjacent pixels and leaves its seven sums in the workspace;
//   2. finish:   one workgroup adds the workgroups' sums in a fixed order and writes the result row of 12 doubles.
// No atomics, no workgroup waits for another, so the row has the same bits run to run.  Float terms are summed in double, masks
// and counts as 64-bit integers (exact).
//
// Built with -ffp-contract=off: each per-pixel step is one separately rounded fp32 operation, and the square root is sqrtf —
// correctly rounded as hipcc lowers it without fast-math, unlike the native 1-ulp instruction — so the outlier count is an exact
// function of the inputs (tests/_score_model.py states it in numpy).
#include "loss_common.hpp"
#include "kitti_gt.hpp"

namespace upf {
namespace score {

using loss::NT;

// the seven sums, in the order of the workspace's 8-byte words
struct Sums {
  double s_occ, s_noc, s_oo;
  long long n_occ, c_out, n_noc, n_oo;
};
constexpr int WORDS = 7;
static_assert(sizeof(Sums) == WORDS * 8, "one 8-byte word per sum");

// one pixel: R, G, B of both ground-truth files (low 16 bits) and the prediction
__device__ __forceinline__ void pixel(Sums& a, uint32_t ro, uint32_t go, uint32_t bo, uint32_t rn, uint32_t gn, uint32_t bn,
                                      float pu, float pv) {
  const float gu = kitti::gt_flow(ro), gv = kitti::gt_flow(go);                                        // exact
  const int io = kitti::gt_mask(bo), in = kitti::gt_mask(bn);                                          // np.uint8() wraps
  const float m_occ = (float)io, m_noc = (float)in;
  float du = gu - pu, dv = gv - pv;
  const float e_occ = sqrtf(du * du + dv * dv);
  const float thr = fmaxf(3.0f, sqrtf(gu * gu + gv * gv) * 0.05f);
  const float d_occ = e_occ * m_occ;
  du = kitti::gt_flow(rn) - pu;
  dv = kitti::gt_flow(gn) - pv;
  const float e_noc = sqrtf(du * du + dv * dv);
  a.s_occ += (double)d_occ;
  a.n_occ += io;
  a.c_out += (d_occ > thr) ? 1 : 0;                          // (false for a NaN)
  a.s_noc += (double)(e_noc * m_noc);
  a.n_noc += in;
  a.s_oo += (double)(e_occ * (m_occ - m_noc));
  a.n_oo += io - in;
}

__device__ __forceinline__ void pixel_at(Sums& a, const uint16_t* __restrict__ occ, const uint16_t* __restrict__ noc,
                                         const float* __restrict__ pred, uint32_t p, uint32_t HW) {
  const uint32_t b = p / HW, r = p - b * HW;
  const size_t o = (size_t)b * 2 * HW + r, g = (size_t)p * 3;
  pixel(a, occ[g], occ[g + 1], occ[g + 2], noc[g], noc[g + 1], noc[g + 2], pred[o], pred[o + HW]);
}

struct Dwords3 { uint32_t x, y, z; };                        // two pixels of a ground-truth array: 12 bytes, 4-byte aligned

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup in a fixed order (xor tree inside each wave, then the waves in index order), valid in thread 0
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
  v = wave_sum(v);
  __syncthreads();                                           // (sh is reused from one sum to the next)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = sh[0];
#pragma unroll
  for (int k = 1; k < NT / 64; ++k) r += sh[k];
  return r;
}

__device__ __forceinline__ Sums block_sums(const Sums& a, double* shd, long long* shl) {
  Sums t;
  t.s_occ = block_sum(a.s_occ, shd);
  t.s_noc = block_sum(a.s_noc, shd);
  t.s_oo = block_sum(a.s_oo, shd);
  t.n_occ = block_sum(a.n_occ, shl);
  t.c_out = block_sum(a.c_out, shl);
  t.n_noc = block_sum(a.n_noc, shl);
  t.n_oo = block_sum(a.n_oo, shl);
  return t;
}

// partials[blockIdx.x] = this workgroup's sums over the pixel pairs q = block * NT + thread, + gridDim.x * NT, ...; an odd pixel
// count leaves the last pixel to thread 0 of workgroup 0.  n = B * HW < 2^31.
__global__ __launch_bounds__(NT)
void partials_kernel(const float* __restrict__ pred, const uint16_t* __restrict__ occ, const uint16_t* __restrict__ noc,
                     Sums* __restrict__ partials, uint32_t HW, uint32_t n) {
  __shared__ double shd[NT / 64];
  __shared__ long long shl[NT / 64];
  Sums a = {0.0, 0.0, 0.0, 0, 0, 0, 0};
  const uint32_t npairs = n >> 1;
  const Dwords3* __restrict__ occ3 = (const Dwords3*)occ;
  const Dwords3* __restrict__ noc3 = (const Dwords3*)noc;
  for (long long q = blockIdx.x * (long long)NT + threadIdx.x; q < npairs; q += (long long)gridDim.x * NT) {
    const Dwords3 o = occ3[q], c = noc3[q];
    const uint32_t p = 2u * (uint32_t)q;
    float u0, u1, v0, v1;
    if ((HW & 1u) == 0) {                                    // even planes: the pair lies in one row of planes, 8-byte aligned
      const uint32_t b = p / HW, r = p - b * HW;
      const size_t at = (size_t)b * 2 * HW + r;
      const float2 u = *(const float2*)(pred + at), v = *(const float2*)(pred + at + HW);
      u0 = u.x; u1 = u.y; v0 = v.x; v1 = v.y;
    } else {                                                 // odd planes: a pair may straddle two items
      const uint32_t b0 = p / HW, r0 = p - b0 * HW, b1 = (p + 1) / HW, r1 = p + 1 - b1 * HW;
      const size_t at0 = (size_t)b0 * 2 * HW + r0, at1 = (size_t)b1 * 2 * HW + r1;
      u0 = pred[at0]; v0 = pred[at0 + HW]; u1 = pred[at1]; v1 = pred[at1 + HW];
    }
    pixel(a, o.x & 0xffffu, o.x >> 16, o.y & 0xffffu, c.x & 0xffffu, c.x >> 16, c.y & 0xffffu, u0, v0);
    pixel(a, o.y >> 16, o.z & 0xffffu, o.z >> 16, c.y >> 16, c.z & 0xffffu, c.z >> 16, u1, v1);
  }
  if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) pixel_at(a, occ, noc, pred, n - 1, HW);
  const Sums t = block_sums(a, shd, shl);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// one workgroup: thread t adds partials t, t + NT, ... in index order, the threads' sums go through block_sums; thread 0 writes
// the row
__global__ __launch_bounds__(NT)
void finish_kernel(const Sums* __restrict__ partials, int n_partials, double batch, double* __restrict__ row) {
  __shared__ double shd[NT / 64];
  __shared__ long long shl[NT / 64];
  Sums a = {0.0, 0.0, 0.0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n_partials; i += NT) {
    const Sums p = partials[i];
    a.s_occ += p.s_occ; a.s_noc += p.s_noc; a.s_oo += p.s_oo;
    a.n_occ += p.n_occ; a.c_out += p.c_out; a.n_noc += p.n_noc; a.n_oo += p.n_oo;
  }
  const Sums t = block_sums(a, shd, shl);
  if (threadIdx.x == 0) {
    const double n_occ = (double)t.n_occ, c_out = (double)t.c_out, n_noc = (double)t.n_noc, n_oo = (double)t.n_oo;
    row[0] = t.s_occ / (n_occ + 1e-6);
    row[1] = c_out / n_occ * 100.0;                          // (an empty mask: 0 / 0 = NaN, as the reference)
    row[2] = t.s_noc / (n_noc + 1e-6);
    row[3] = t.s_oo / (n_oo + 1e-6);
    row[4] = t.s_occ; row[5] = n_occ; row[6] = c_out; row[7] = t.s_noc; row[8] = n_noc; row[9] = t.s_oo; row[10] = n_oo;
    row[11] = batch;
  }
}

// the workgroups of the partials launch: loss::red_blocks over the pixel pairs
static int check_shape(const char* what, int B, int H, int W, long long* n) {
  UPF_REQUIRE(B > 0 && H > 0 && W > 0, UPF_EINVAL, "%s: B, H, W must be positive (got %d, %d, %d)", what, B, H, W);
  *n = (long long)B * H * W;
  UPF_REQUIRE(*n < (1ll << 31), UPF_EUNSUPPORTED, "%s: %lld pixels (2^31 or more)", what, *n);
  return UPF_OK;
}

}  // namespace score
}  // namespace upf

extern "C" int upf_kitti_score_workspace_bytes(int B, int H, int W, long long* bytes) {
  using namespace upf;
  UPF_REQUIRE(bytes, UPF_EINVAL, "kitti_score_workspace_bytes: null pointer");
  long long n;
  if (int rc = score::check_shape("kitti_score_workspace_bytes", B, H, W, &n)) return rc;
  *bytes = (long long)loss::red_blocks(n >> 1) * (long long)sizeof(score::Sums);
  return UPF_OK;
}

extern "C" int upf_kitti_score(const float* pred, const unsigned short* gt_occ, const unsigned short* gt_noc, void* workspace,
                               double* row, int B, int H, int W, void* stream) {
  using namespace upf;
  UPF_REQUIRE(pred && gt_occ && gt_noc && workspace && row, UPF_EINVAL, "kitti_score: null pointer");
  long long n;
  if (int rc = score::check_shape("kitti_score", B, H, W, &n)) return rc;
  UPF_REQUIRE(aligned_to(pred, 8) && aligned_to(gt_occ, 4) && aligned_to(gt_noc, 4) && aligned_to(workspace, 8) && aligned_to(row, 8),
              UPF_EALIGN, "kitti_score: pred, workspace and row must be 8-byte, the ground truth 4-byte aligned");
  const int blocks = loss::red_blocks(n >> 1);
  hipLaunchKernelGGL(score::partials_kernel, dim3(blocks), dim3(score::NT), 0, (hipStream_t)stream, pred, gt_occ, gt_noc,
                     (score::Sums*)workspace, (uint32_t)(H * W), (uint32_t)n);
  if (int rc = check_launch("kitti_score (partials)")) return rc;
  hipLaunchKernelGGL(score::finish_kernel, dim3(1), dim3(score::NT), 0, (hipStream_t)stream, (const score::Sums*)workspace, blocks,
                     (double)B, row);
  return check_launch("kitti_score");
}
