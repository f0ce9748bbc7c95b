// 81-neighbour cost volume, forward — hand-written for gfx950 (MI355X / CDNA4).
//
// Replaces correlation_forward<T> + 2x channels_first<T> of the reference
// (model/correlation_package/correlation_cuda_kernel.cu:15-114, :302-393), which run
// one 32-thread block per output pixel, 81 barrier+serial-reduce rounds, on padded NHWC copies.
//
// Three kernels, all reading NCHW directly (no NHWC staging pass).  WHICH ONE A LAUNCH TAKES is stated in one
// place, `route()` below; the launch functions only launch what it returns.
//   corr81_allc_kernel.hpp  all-channels matrix-core kernel — bf16/fp16 with C <= 208: almost every 16-bit launch
//     * no channel loop: a workgroup stages ALL channel quads of its f1 tile and f2 tile + halo at once (every global load in
//       flight together, ONE barrier), then computes and stores unit after unit with the 16-block 4x4x4 MFMA;
//     * four tile geometries (AllcGeos), so that the tile shrinks as C grows (LDS) and as the image shrinks (more workgroups);
//     * aligned and ragged rows, pitched rows, NCHW or channel-octet output, and optionally the normalisation of both inputs
//       fused into its loader (upf_corr81_norm_forward*: one statistics launch, norm_stats, then this kernel);
//   corr81_mfma_kernel.hpp  channel-chunked matrix-core kernel — aligned bf16/fp16 that the first leaves: C > 208, and C > 40 on
//     large grids, where its 8x32 tile stages fewer bytes per pixel
//     * the same MFMA contraction (4.4x the rate of v_dot2c's half-rate issue, 75 % of its products wanted: dense 12-candidate
//       band) over chunks of 32 channels, double-buffered in LDS;
//     * finished units are de-skewed, transposed through a per-wave LDS patch and stored while the next
//       unit computes, so HBM writes overlap the matrix work.
//   corr81_fwd_kernel.hpp   wave-level VALU kernel — fp32 (the parity mode) and the 16-bit launches neither matrix kernel takes
//     * workgroup = 9 waves = one 8x32 pixel tile; wave w owns displacement row dy = w-4, a lane owns 4
//       consecutive pixels of one row and keeps 9(dx) x 4(px) fp32 accumulators;
//     * LDS holds the f1 tile and the f2 tile + 4-pixel halo for a chunk of KC "k-slots" (one fp32
//       channel, or a PAIR of 16-bit channels interleaved per pixel so one v_dot2c retires two channels),
//       double-buffered: the next chunk's global loads are in flight during the MAC loop of this one;
//     * aligned inputs are staged with raw buffer loads whose bounds check supplies every zero (halo
//       outside the image, channels beyond C); per k-slot a lane issues 4 ds_read_b128 for 36 MACs;
//       the lane -> (row, x-block) map follows the hardware's 16-lane ds_read_b128 service groups.
// Common: epilogue divides by C (like `reduce_sum / nelems`, correlation_cuda_kernel.cu:108), optionally
// applies LeakyReLU (model/upflow.py:563-564), writes 4-8 pixels per store, optionally into a wider
// channel buffer (out_batch_stride); blockIdx is remapped so each XCD (private L2) gets a contiguous
// run of tiles.
#include "corr81_fwd_kernel.hpp"
#include "corr81_mfma_kernel.hpp"
#include "corr81_allc_kernel.hpp"
#include "internal.hpp"
#include <hip/hip_ext.h>
#include <stdlib.h>
#include <string.h>
#include <tuple>
#include <utility>
#include <vector>

namespace upf {
namespace corr {

#ifndef UPF_CORR_KC
#define UPF_CORR_KC 4
#endif

static int g_variant = -1;     // upf_corr_set_option("variant"): -1 = choose, 0..3 = force where it fits
static int g_old_path = 0;     // upf_corr_set_option("old_path"): 1 = the chunked round-1 kernels (A/B runs)

// ---- the tile geometries of the all-channels kernel (corr81_allc_kernel.hpp) -------------------------------------------------
// (unit width, units per tile, staging tasks per thread), largest tile first: 8x32, 4x32, 2x32, 4x16 pixels
template <int UW_, int NU_, int NT_> struct AllcGeo {
  static constexpr int UW = UW_, NU = NU_, NT = NT_;
  using Tile = corrx::Geo<UW_, NU_>;
};
using AllcGeos = std::tuple<AllcGeo<32, 4, 4>, AllcGeo<32, 2, 8>, AllcGeo<32, 1, 8>, AllcGeo<16, 1, 8>>;
constexpr int NALLC = (int)std::tuple_size<AllcGeos>::value;
constexpr size_t LDS_MAX = 160 * 1024;

// f(G{}) for geometry `v` of the list — G::UW / G::NU / G::NT are constants inside f; a value-initialised result for any other v
template <typename F, size_t... I>
auto with_variant(int v, F&& f, std::index_sequence<I...>) {
  decltype(f(std::tuple_element_t<0, AllcGeos>{})) r{};
  (void)((v == (int)I && ((r = f(std::tuple_element_t<I, AllcGeos>{})), true)) || ...);
  return r;
}
template <typename F>
auto with_variant(int v, F&& f) { return with_variant(v, f, std::make_index_sequence<NALLC>{}); }

static size_t allc_lds(int v, int KQ, bool ragged, bool norm) {
  return with_variant(v, [&](auto g) { using G = decltype(g); return corrx::lds_bytes<G::UW, G::NU>(KQ, ragged, norm); });
}
static bool allc_fits(int v, int KQ, bool ragged, bool norm) {
  return with_variant(v, [&](auto g) {
    using G = decltype(g);
    return corrx::ntasks<G::UW, G::NU>(KQ) <= G::NT * corrx::NTHREADS && corrx::lds_bytes<G::UW, G::NU>(KQ, ragged, norm) <= LDS_MAX;
  });
}
static long long allc_nwg(int v, int B, int H, int W) {
  return with_variant(v, [&](auto g) { using T = typename decltype(g)::Tile; return (long long)B * cdiv(H, T::TH) * cdiv(W, T::TW); });
}

// ---- which kernel a launch takes --------------------------------------------------------------------------------------------
struct Route {
  enum Kind { NONE, ALLC, MFMA, CHUNKED } kind;   // NONE: no kernel applies (the normalising forms only: just ALLC normalises)
  int variant;                                    // ALLC: index into AllcGeos
  bool aligned;                                   // ALLC, CHUNKED: the kernel's aligned form, else its ragged one (octet output: PADW)
  bool single;                                    // MFMA: the channel depth is a single chunk
};
struct RouteQuery {
  int B, C, H, W, fpitch, elem_bytes;
  bool vec4, vec16;                   // W, row pitch and out_batch_stride whole 4-pixel vectors / 16-byte groups, f1 / f2 / out aligned to one
  bool norm, oc8;                     // normalising form; octet output (its entry point has checked the 16-byte alignment of everything but W)
  int variant, old_path;              // the options and the environment, as read for THIS launch
  bool no_mfma;
};

// All-channels geometry by shape (measured on MI355X, tools/corr_levels.py -> profiles/r02_corr81_levels.txt):
//   * never a geometry whose grid needs a second round of workgroups when a smaller tile fits in one round
//     (workgroups per CU = min(2, 160 KB / LDS per workgroup));
//   * with >= 200 workgroups in one round: the LARGEST such tile (least halo staging per output pixel);
//   * fewer than that (the coarse levels): the geometry with the MOST workgroups — the kernel is a latency chain there
//     and a smaller tile shortens it;
//   * everything needs several rounds (the large levels): the largest tile.
// No geometry fits C > 208.  C > 40 on a grid of >= 160 8x32 tiles: the channel-chunked kernels, whose larger tile stages 36 %
// fewer bytes per pixel, win there (1/8-resolution level of the large configurations) — not for pitched or ragged rows.
static Route route(const RouteQuery& q) {
  const bool bits16 = q.elem_bytes == 2;
  const bool in_range = (size_t)q.C * q.H * q.fpitch * q.elem_bytes < (1ull << 31);      // a batch item inside the buffer-descriptor range
  // (the NCHW output is written in 8-pixel segments by the aligned form: W % 8 == 0; a pitched input with a ragged W takes the ragged form)
  const bool ragged = !q.oc8 && !q.vec16;
  if (bits16 && in_range && (q.norm || (!q.old_path && !q.no_mfma)) && !(ragged && q.W < 4)) {     // (W < 4: rows shorter than a staging quad)
    const int KQ = (q.C + 3) / 4;
    int v = -1;
    if (q.variant >= 0 && q.variant < NALLC && allc_fits(q.variant, KQ, ragged, q.norm)) v = q.variant;
    else if (q.norm || ragged || q.fpitch != q.W || q.C <= 40 || (long long)q.B * cdiv(q.H, 8) * cdiv(q.W, 32) < 160) {
      int first = -1, big = -1, most = -1;
      long long most_n = -1;
      for (int i = 0; i < NALLC; ++i) {
        if (!allc_fits(i, KQ, ragged, q.norm)) continue;
        if (first < 0) first = i;
        const long long nwg = allc_nwg(i, q.B, q.H, q.W);
        const long long per_cu = LDS_MAX / allc_lds(i, KQ, ragged, q.norm) >= 2 ? 2 : 1;
        if (nwg > 256 * per_cu) continue;                              // more than one round
        if (nwg >= 200 && big < 0) big = i;
        if (nwg > most_n) { most = i; most_n = nwg; }
      }
      v = big >= 0 ? big : most >= 0 ? most : first;
    }
    if (v >= 0) return {Route::ALLC, v, q.oc8 ? q.W % 8 == 0 : q.vec16, false};
  }
  if (q.norm) return {Route::NONE, -1, false, false};
  const bool aligned = q.vec4 && in_range;
  if (bits16 && aligned && q.vec16 && !q.no_mfma) return {Route::MFMA, -1, true, q.C <= 4 * corrm::KQ};
  return {Route::CHUNKED, -1, aligned, false};
}

// One cost-volume launch as the entry points hand it down (fpitch: elements between the rows of f1 / f2, W when contiguous)
struct Call {
  const void *f1, *f2;
  void* out;
  int B, C, H, W, fpitch;
  long long out_bs;
  float slope;
  hipStream_t stream;
  const float *ws1 = nullptr, *ws2 = nullptr;      // the normalising forms: norm_stats
  int nseg = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;         // the timed entry points: recorded right around the kernel
};

static RouteQuery route_query(const Call& a, int elem_bytes, bool norm, bool oc8) {
  auto ptrs = [&](size_t n) { return aligned_to(a.f1, n) && aligned_to(a.f2, n) && aligned_to(a.out, n); };
  RouteQuery q;
  q.B = a.B; q.C = a.C; q.H = a.H; q.W = a.W; q.fpitch = a.fpitch; q.elem_bytes = elem_bytes;
  q.vec4 = (a.W % 4 == 0) && (a.out_bs % 4 == 0) && ptrs(4 * (size_t)elem_bytes);
  q.vec16 = (a.W % 8 == 0) && (a.fpitch % 8 == 0) && (a.out_bs % 8 == 0) && ptrs(16);
  q.norm = norm; q.oc8 = oc8;
  q.variant = g_variant; q.old_path = g_old_path;
  q.no_mfma = elem_bytes == 2 && !norm && getenv("UPF_CORR_NO_MFMA") != nullptr;      // (nothing else asks)
  return q;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------
// hipExtLaunchKernelGGL == hipLaunchKernelGGL plus optional start/stop events recorded right around
// THIS kernel on its stream (the timed entry points; null events = plain launch)
template <typename T, int KC>
void launch_kc(const Call& a, bool aligned, unsigned nblocks, int tiles_x, int tiles_y) {
  static LdsOptIn opt_a, opt_u;   // > 48 KiB of dynamic LDS: opted into per kernel and per device
  opt_a.ensure(reinterpret_cast<const void*>(&corr81_fwd_kernel<T, true, KC>), lds_bytes(KC));
  opt_u.ensure(reinterpret_cast<const void*>(&corr81_fwd_kernel<T, false, KC>), lds_bytes(KC));
  if (aligned)
    hipExtLaunchKernelGGL((corr81_fwd_kernel<T, true, KC>), dim3(nblocks), dim3(NTHREADS), lds_bytes(KC), a.stream, a.ev0, a.ev1, 0,
                          (const T*)a.f1, (const T*)a.f2, (T*)a.out, a.C, a.H, a.W, tiles_x, tiles_y, a.out_bs, a.slope);
  else
    hipExtLaunchKernelGGL((corr81_fwd_kernel<T, false, KC>), dim3(nblocks), dim3(NTHREADS), lds_bytes(KC), a.stream, a.ev0, a.ev1, 0,
                          (const T*)a.f1, (const T*)a.f2, (T*)a.out, a.C, a.H, a.W, tiles_x, tiles_y, a.out_bs, a.slope);
}

template <typename T, bool SINGLE>
void launch_mfma(const Call& a, unsigned nblocks, int tiles_x, int tiles_y) {
  static LdsOptIn opt;
  opt.ensure(reinterpret_cast<const void*>(&corrm::corr81_mfma_kernel<T, SINGLE>), corrm::LDS_BYTES);
  hipExtLaunchKernelGGL((corrm::corr81_mfma_kernel<T, SINGLE>), dim3(nblocks), dim3(corrm::NTHREADS), corrm::LDS_BYTES, a.stream, a.ev0, a.ev1, 0,
                        (const T*)a.f1, (const T*)a.f2, (T*)a.out, a.C, a.H, a.W, tiles_x, tiles_y, a.out_bs, a.slope);
}

template <typename T, typename TO, typename G, bool RAGGED, bool NORM, bool OC8, bool PADW>
int launch_allc_one(const Call& a) {
  using Tile = typename G::Tile;
  const int tiles_x = cdiv(a.W, Tile::TW), tiles_y = cdiv(a.H, Tile::TH);
  const long long nblocks = (long long)a.B * tiles_x * tiles_y;
  UPF_REQUIRE(nblocks < (1ll << 31), UPF_EINVAL, "corr81_forward: grid too large");
  const size_t lds = corrx::lds_bytes<G::UW, G::NU>((a.C + 3) / 4, RAGGED, NORM);
  static LdsOptIn opt;
  auto kern = &corrx::corr81_allc_kernel<T, G::UW, G::NU, G::NT, RAGGED, NORM, 1, OC8, PADW, TO>;
  opt.ensure(reinterpret_cast<const void*>(kern), lds);
  // (the timed entry points pass start / stop events -> hipExtLaunchKernel; everything else takes the ordinary launch path)
  if (a.ev0 || a.ev1)
    hipExtLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(corrx::NTHREADS), lds, a.stream, a.ev0, a.ev1, 0,
                          (const T*)a.f1, (const T*)a.f2, (TO*)a.out, a.C, a.H, a.W, tiles_x, tiles_y, a.out_bs, a.slope, a.ws1, a.ws2, a.nseg, (int)nblocks, a.fpitch);
  else
    hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(corrx::NTHREADS), lds, a.stream,
                       (const T*)a.f1, (const T*)a.f2, (TO*)a.out, a.C, a.H, a.W, tiles_x, tiles_y, a.out_bs, a.slope, a.ws1, a.ws2, a.nseg, (int)nblocks, a.fpitch);
  return check_launch("corr81_forward");
}

// an ALLC route.  Octet output (`oc8`, the normalising forms only): !RAGGED, OC8, and PADW for a ragged logical W on pitched rows
template <typename T, typename TO, bool NORM>
int launch_allc(const Route& r, bool oc8, const Call& a) {
  UPF_REQUIRE(r.variant >= 0 && r.variant < NALLC, UPF_EUNSUPPORTED, "corr81_forward: internal routing error (variant %d)", r.variant);
  return with_variant(r.variant, [&](auto g) {
    using G = decltype(g);
    if constexpr (NORM)
      if (oc8) return r.aligned ? launch_allc_one<T, TO, G, false, true, true, false>(a) : launch_allc_one<T, TO, G, false, true, true, true>(a);
    return r.aligned ? launch_allc_one<T, TO, G, false, NORM, false, false>(a) : launch_allc_one<T, TO, G, true, NORM, false, false>(a);
  });
}

template <typename T>
int launch_fwd(const Call& a) {
  constexpr int ES = sizeof(typename Elem<T>::store_t);
  const int tiles_x = cdiv(a.W, TW), tiles_y = cdiv(a.H, TH);       // (the 8x32 tiles of the two chunked kernels)
  const long long nblocks = (long long)a.B * tiles_x * tiles_y;
  UPF_REQUIRE(nblocks < (1ll << 31), UPF_EINVAL, "corr81_forward: grid too large");
  const Route r = route(route_query(a, ES, false, false));
  if constexpr (ES == 2) {
    if (r.kind == Route::ALLC) return launch_allc<T, T, false>(r, false, a);
    if (r.kind == Route::MFMA) {
      if (r.single) launch_mfma<T, true>(a, (unsigned)nblocks, tiles_x, tiles_y);
      else launch_mfma<T, false>(a, (unsigned)nblocks, tiles_x, tiles_y);
      return check_launch("corr81_forward");
    }
  }
  // chunk depth: deeper chunks mean fewer workgroup barriers, shallower ones a shorter exposed prologue
  // and three workgroups per CU; measured on MI355X (tools/corr_ablate.hip) KC = 4 wins at every level
  launch_kc<T, UPF_CORR_KC>(a, r.aligned, (unsigned)nblocks, tiles_x, tiles_y);
  return check_launch("corr81_forward");
}

// launch(start event, stop event) -> rc, `nrep` times, each between its own pair of HIP events on `s` -> average and minimum (us)
template <typename Launch>
int time_launches(const char* who, hipStream_t s, int nrep, float* avg_us, float* min_us, Launch&& launch) {
  std::vector<hipEvent_t> ev(2 * (size_t)nrep);
  for (hipEvent_t& e : ev) (void)hipEventCreate(&e);
  int rc = UPF_OK;
  for (int i = 0; i < nrep && rc == UPF_OK; ++i) rc = launch(ev[2 * i], ev[2 * i + 1]);
  const hipError_t err = hipStreamSynchronize(s);
  if (rc == UPF_OK && err != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(err)); rc = (int)err; }
  double sum = 0.0, mn = 1e30;
  if (rc == UPF_OK)
    for (int i = 0; i < nrep; ++i) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
      sum += ms; if (ms < mn) mn = ms;
    }
  for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
  if (rc == UPF_OK) { *avg_us = (float)(sum / nrep * 1e3); if (min_us) *min_us = (float)(mn * 1e3); }
  return rc;
}

// ---- normalisation fused into the cost volume's loader ----------------------------------------------------------------------
// Workspace: the (count, mean, M2) partials of the 2 * B*C rows, [nseg][3] floats each, rounded up to 16 bytes; behind them the
// final (mean, 1/std) pairs, float2 [2 * B*C] (upf_corr81_norm_workspace_bytes).
static size_t norm_partial_floats(long long N, int HW) { return ((size_t)2 * N * misc::stats2_nseg(N, HW) * 3 + 3) / 4 * 4; }

// the statistics launch of a normalising form -> a.ws1 / a.ws2 / a.nseg
static int norm_stats(Call& a, int dtype, void* workspace, const char* what) {
  const long long N = (long long)a.B * a.C;
  float* part = (float*)workspace;
  float2* fin = reinterpret_cast<float2*>(part + norm_partial_floats(N, a.H * a.W));
  a.nseg = misc::launch_stats2(a.f1, a.f2, part, fin, N, a.H * a.W, dtype, a.stream, a.W, a.fpitch);
  a.ws1 = reinterpret_cast<const float*>(fin);            // what the cost volume reads: final pairs of f1's rows ...
  a.ws2 = reinterpret_cast<const float*>(fin + N);        // ... and of f2's
  return check_launch(what);
}

// f(input type, output type) of a normalising form: bf16 / fp16 features, either of the two for the output
template <typename F>
int with_type_pair(int dtype, int out_dtype, F&& f) {
  if (dtype == UPF_BF16) return out_dtype == UPF_F16 ? f(bf16_t{}, f16_t{}) : f(bf16_t{}, bf16_t{});
  return out_dtype == UPF_BF16 ? f(f16_t{}, bf16_t{}) : f(f16_t{}, f16_t{});
}

// The normalising forms behind their entry points' validation: the statistics launch, the route, then ONE launch of the cost volume
// — or, for the timed entry points (avg_us), nrep launches each between its own pair of events, like upf_corr81_forward_timed
// (the statistics launch runs once, untimed).
static int norm_run(const char* who, bool oc8, Call a, int dtype, int out_dtype, void* workspace,
                    int nrep = 0, float* avg_us = nullptr, float* min_us = nullptr) {
  const char* const tag = avg_us ? "corr81_norm_forward_timed" : who;      // (both timed forms report launch errors under this name)
  char what[64];
  snprintf(what, sizeof(what), "%s (statistics)", tag);
  const int rc = norm_stats(a, dtype, workspace, what);
  if (rc != UPF_OK) return rc;
  const Route r = route(route_query(a, 2, true, oc8));
  if (oc8) UPF_REQUIRE(r.kind == Route::ALLC, UPF_EUNSUPPORTED, "%s: no kernel variant fits C=%d", who, a.C);
  UPF_REQUIRE(r.kind == Route::ALLC, UPF_EUNSUPPORTED, "%s: no kernel variant fits C=%d W=%d%s", who, a.C, a.W, avg_us ? "" : " (W >= 4 required)");
  auto launch = [&](hipEvent_t ev0, hipEvent_t ev1) {
    a.ev0 = ev0; a.ev1 = ev1;
    return with_type_pair(dtype, out_dtype, [&](auto ti, auto to) { return launch_allc<decltype(ti), decltype(to), true>(r, oc8, a); });
  };
  return avg_us ? time_launches(tag, a.stream, nrep, avg_us, min_us, launch) : launch(nullptr, nullptr);
}

// ---- general-parameter fallback: one thread per output element --------------------------------
// Same arithmetic as correlation_forward<T> (correlation_cuda_kernel.cu:41-114) on virtual zero
// padding; used only for parameter sets the model never instantiates.
template <typename T>
__global__ void corr_general_kernel(const T* __restrict__ in1, const T* __restrict__ in2, T* __restrict__ out,
                                    int B, int C, int H, int W, int pad, int kr, int md, int s1, int s2,
                                    int dr, int oH, int oW, int ksize) {
  const int ds = 2 * dr + 1;
  const long long total = (long long)B * ds * ds * oH * oW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % oW);
    const int oy = (int)((i / oW) % oH);
    const int tc = (int)((i / ((long long)oW * oH)) % (ds * ds));
    const int n = (int)(i / ((long long)oW * oH * ds * ds));
    const int ti = tc % ds - dr, tj = tc / ds - dr;
    const int y1 = oy * s1 + md - pad, x1 = ox * s1 + md - pad;        // un-padded coordinates
    const int y2 = y1 + tj * s2, x2 = x1 + ti * s2;
    float acc = 0.f;
    for (int j = -kr; j <= kr; ++j)
      for (int ii = -kr; ii <= kr; ++ii) {
        const int ya = y1 + j, xa = x1 + ii, yb = y2 + j, xb = x2 + ii;
        if (ya < 0 || ya >= H || xa < 0 || xa >= W || yb < 0 || yb >= H || xb < 0 || xb >= W) continue;
        for (int c = 0; c < C; ++c)
          acc += Elem<T>::load(in1 + (((size_t)n * C + c) * H + ya) * W + xa) * Elem<T>::load(in2 + (((size_t)n * C + c) * H + yb) * W + xb);
      }
    Elem<T>::store(out + i, acc / (float)(ksize * ksize * C));
  }
}

}  // namespace corr
}  // namespace upf

extern "C" int upf_corr81_forward(const void* f1, const void* f2, void* out, int B, int C, int H, int W, int dtype,
                                  long long out_batch_stride, float leaky_slope, void* stream) {
  using namespace upf;
  UPF_REQUIRE(f1 && f2 && out, UPF_EINVAL, "corr81_forward: null pointer");
  UPF_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, UPF_EINVAL, "corr81_forward: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  if (out_batch_stride == 0) out_batch_stride = (long long)corr::ND * H * W;
  UPF_REQUIRE(out_batch_stride >= (long long)corr::ND * H * W, UPF_EINVAL, "corr81_forward: out_batch_stride %lld < 81*H*W", out_batch_stride);
  const corr::Call a{f1, f2, out, B, C, H, W, W, out_batch_stride, leaky_slope, (hipStream_t)stream};
  UPF_DISPATCH(dtype, T, return corr::launch_fwd<T>(a));
  return UPF_OK;
}

extern "C" int upf_corr81_forward_timed(const void* f1, const void* f2, void* out, int B, int C, int H, int W, int dtype,
                                        long long out_batch_stride, float leaky_slope, void* stream, int nrep,
                                        float* avg_us, float* min_us) {
  using namespace upf;
  UPF_REQUIRE(f1 && f2 && out && avg_us, UPF_EINVAL, "corr81_forward_timed: null pointer");
  UPF_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && nrep > 0 && nrep <= 1024, UPF_EINVAL, "corr81_forward_timed: bad arguments");
  if (out_batch_stride == 0) out_batch_stride = (long long)corr::ND * H * W;
  corr::Call a{f1, f2, out, B, C, H, W, W, out_batch_stride, leaky_slope, (hipStream_t)stream};
  return corr::time_launches("corr81_forward_timed", a.stream, nrep, avg_us, min_us, [&](hipEvent_t ev0, hipEvent_t ev1) -> int {
    a.ev0 = ev0; a.ev1 = ev1;
    UPF_DISPATCH(dtype, T, return corr::launch_fwd<T>(a));
    return UPF_OK;
  });
}

extern "C" int upf_correlation_out_shape(int H, int W, int pad_size, int kernel_size, int max_displacement,
                                         int stride1, int stride2, int* out_channels, int* out_h, int* out_w) {
  using namespace upf;
  UPF_REQUIRE(stride1 > 0 && stride2 > 0 && kernel_size > 0 && pad_size >= 0 && max_displacement >= 0, UPF_EINVAL,
              "correlation: bad parameters pad=%d k=%d md=%d s1=%d s2=%d", pad_size, kernel_size, max_displacement, stride1, stride2);
  const int kr = (kernel_size - 1) / 2, br = kr + max_displacement;             // correlation_cuda.cc:24-25
  const int dr = max_displacement / stride2;
  const int oh = (H + 2 * pad_size - 2 * br + stride1 - 1) / stride1;           // ceil, :33-34
  const int ow = (W + 2 * pad_size - 2 * br + stride1 - 1) / stride1;
  UPF_REQUIRE(oh > 0 && ow > 0, UPF_EINVAL, "correlation: empty output %dx%d", oh, ow);
  if (out_channels) *out_channels = (2 * dr + 1) * (2 * dr + 1);
  if (out_h) *out_h = oh;
  if (out_w) *out_w = ow;
  return UPF_OK;
}

extern "C" int upf_correlation_forward(const void* in1, const void* in2, void* out, int B, int C, int H, int W, int dtype,
                                       int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                       int corr_type_multiply, void* stream) {
  using namespace upf;
  (void)corr_type_multiply;   // accepted and unused, like correlation_cuda_kernel.cu:302-393
  if (pad_size == 4 && kernel_size == 1 && max_displacement == 4 && stride1 == 1 && stride2 == 1)
    return upf_corr81_forward(in1, in2, out, B, C, H, W, dtype, 0, 0.f, stream);
  int oc, oh, ow;
  int rc = upf_correlation_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2, &oc, &oh, &ow);
  if (rc != UPF_OK) return rc;
  UPF_REQUIRE(in1 && in2 && out && B > 0 && C > 0, UPF_EINVAL, "correlation_forward: bad arguments");
  // correlation_forward<T> reads padded rows y1 + tj*stride2 + j >= max_displacement - (md/s2)*s2 - kernel_rad (correlation_cuda_kernel.cu:62,
  // :87-91): negative = the reference reads what precedes its buffer (undefined) — nothing to be a drop-in for
  UPF_REQUIRE(max_displacement - (max_displacement / stride2) * stride2 - (kernel_size - 1) / 2 >= 0, UPF_EUNSUPPORTED,
              "correlation_forward: (k=%d, md=%d, s2=%d) — the reference reads outside its padded buffer for these parameters (undefined)",
              kernel_size, max_displacement, stride2);
  const long long total = (long long)B * oc * oh * ow;
  const int threads = 256;
  const int blocks = (int)((total + threads - 1) / threads > 65535 * 16 ? 65535 * 16 : (total + threads - 1) / threads);
  const int kr = (kernel_size - 1) / 2, dr = max_displacement / stride2;
  UPF_DISPATCH(dtype, T,
               hipLaunchKernelGGL((corr::corr_general_kernel<T>), dim3(blocks), dim3(threads), 0, (hipStream_t)stream,
                                  (const T*)in1, (const T*)in2, (T*)out, B, C, H, W, pad_size, kr, max_displacement,
                                  stride1, stride2, dr, oh, ow, kernel_size));
  return check_launch("correlation_forward");
}

// ---- the normalising entry points ---------------------------------------------------------------------------------------------
extern "C" int upf_corr81_norm_supported(int C, int dtype) {
  return (dtype == UPF_F16 || dtype == UPF_BF16) && C > 0 && upf::corr::allc_fits(upf::corr::NALLC - 1, (C + 3) / 4, true, true);
}

extern "C" long long upf_corr81_norm_workspace_bytes(int B, int C, int H, int W) {
  const long long N = (long long)B * C;
  return (long long)(upf::corr::norm_partial_floats(N, H * W) * sizeof(float)) + 2 * N * (long long)sizeof(float2);
}

extern "C" int upf_corr81_norm_forward_mixed(const void* f1, const void* f2, int f_row_pitch, void* out, int B, int C, int H, int W, int dtype, int out_dtype,
                                             long long out_batch_stride, float leaky_slope, void* workspace, void* stream) {
  using namespace upf;
  UPF_REQUIRE(out_dtype == dtype || ((dtype == UPF_F16 || dtype == UPF_BF16) && (out_dtype == UPF_F16 || out_dtype == UPF_BF16)), UPF_EDTYPE,
              "corr81_norm_forward: out_dtype %d (bf16 / fp16)", out_dtype);
  UPF_REQUIRE(f1 && f2 && out && workspace, UPF_EINVAL, "corr81_norm_forward: null pointer");
  UPF_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, UPF_EINVAL, "corr81_norm_forward: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  UPF_REQUIRE(upf_corr81_norm_supported(C, dtype), UPF_EUNSUPPORTED,
              "corr81_norm_forward: bf16 / fp16 with C <= 208 only (dtype %d, C %d): use upf_normalize_forward + upf_corr81_forward", dtype, C);
  const int fp = f_row_pitch ? f_row_pitch : W;
  UPF_REQUIRE(fp >= W, UPF_EINVAL, "corr81_norm_forward: row pitch %d < W = %d", fp, W);
  UPF_REQUIRE((size_t)C * H * fp * 2 < (1ull << 31), UPF_EUNSUPPORTED, "corr81_norm_forward: batch item >= 2 GiB");
  if (out_batch_stride == 0) out_batch_stride = (long long)corr::ND * H * W;
  UPF_REQUIRE(out_batch_stride >= (long long)corr::ND * H * W, UPF_EINVAL, "corr81_norm_forward: out_batch_stride %lld < 81*H*W", out_batch_stride);
  return corr::norm_run("corr81_norm_forward", false, {f1, f2, out, B, C, H, W, fp, out_batch_stride, leaky_slope, (hipStream_t)stream},
                        dtype, out_dtype, workspace);
}

extern "C" int upf_corr81_norm_forward_pitched(const void* f1, const void* f2, int f_row_pitch, void* out, int B, int C, int H, int W, int dtype,
                                               long long out_batch_stride, float leaky_slope, void* workspace, void* stream) {
  return upf_corr81_norm_forward_mixed(f1, f2, f_row_pitch, out, B, C, H, W, dtype, dtype, out_batch_stride, leaky_slope, workspace, stream);
}

extern "C" int upf_corr81_norm_forward(const void* f1, const void* f2, void* out, int B, int C, int H, int W, int dtype,
                                       long long out_batch_stride, float leaky_slope, void* workspace, void* stream) {
  return upf_corr81_norm_forward_pitched(f1, f2, 0, out, B, C, H, W, dtype, out_batch_stride, leaky_slope, workspace, stream);
}

// octet output: the feature rows must be 16-byte aligned — W % 8 == 0, or (round 5) any W on rows PITCHED to a multiple of 8 elements
static int norm_c8_check(const void* f1, const void* f2, const void* out8, long long out8_batch_stride, int H, int W, int fp, const char* who) {
  using namespace upf;
  UPF_REQUIRE(fp >= W && fp % 8 == 0 && aligned_to(f1, 16) && aligned_to(f2, 16) && aligned_to(out8, 16) && out8_batch_stride % 8 == 0, UPF_EUNSUPPORTED,
              "%s: the feature rows must be 16-byte aligned (W %% 8 == 0, or a row pitch that is a multiple of 8) and the operands 16-byte aligned (W = %d, pitch = %d)", who, W, fp);
  UPF_REQUIRE(W >= 4, UPF_EUNSUPPORTED, "%s: W = %d < 4", who, W);
  UPF_REQUIRE(out8_batch_stride >= (long long)11 * H * W * 8, UPF_EINVAL, "%s: out8_batch_stride %lld < 11 octets", who, out8_batch_stride);
  return UPF_OK;
}

extern "C" int upf_corr81_norm_forward_c8_mixed(const void* f1, const void* f2, int f_row_pitch, void* out8, long long out8_batch_stride, int B, int C, int H, int W,
                                                int dtype, int out_dtype, float leaky_slope, void* workspace, void* stream) {
  using namespace upf;
  UPF_REQUIRE(out_dtype == dtype || ((dtype == UPF_F16 || dtype == UPF_BF16) && (out_dtype == UPF_F16 || out_dtype == UPF_BF16)), UPF_EDTYPE,
              "corr81_norm_forward_c8: out_dtype %d (bf16 / fp16)", out_dtype);
  UPF_REQUIRE(f1 && f2 && out8 && workspace, UPF_EINVAL, "corr81_norm_forward_c8: null pointer");
  UPF_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, UPF_EINVAL, "corr81_norm_forward_c8: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  UPF_REQUIRE(upf_corr81_norm_supported(C, dtype), UPF_EUNSUPPORTED,
              "corr81_norm_forward_c8: bf16 / fp16 with C <= 208 only (dtype %d, C %d)", dtype, C);
  const int fp = f_row_pitch ? f_row_pitch : W;
  UPF_REQUIRE((size_t)C * H * fp * 2 < (1ull << 31), UPF_EUNSUPPORTED, "corr81_norm_forward_c8: batch item >= 2 GiB");
  const int rc = norm_c8_check(f1, f2, out8, out8_batch_stride, H, W, fp, "corr81_norm_forward_c8");
  if (rc != UPF_OK) return rc;
  return corr::norm_run("corr81_norm_forward_c8", true, {f1, f2, out8, B, C, H, W, fp, out8_batch_stride, leaky_slope, (hipStream_t)stream},
                        dtype, out_dtype, workspace);
}

extern "C" int upf_corr81_norm_forward_c8_pitched(const void* f1, const void* f2, int f_row_pitch, void* out8, long long out8_batch_stride, int B, int C, int H, int W,
                                                  int dtype, float leaky_slope, void* workspace, void* stream) {
  return upf_corr81_norm_forward_c8_mixed(f1, f2, f_row_pitch, out8, out8_batch_stride, B, C, H, W, dtype, dtype, leaky_slope, workspace, stream);
}

extern "C" int upf_corr81_norm_forward_c8(const void* f1, const void* f2, void* out8, long long out8_batch_stride, int B, int C, int H, int W,
                                          int dtype, float leaky_slope, void* workspace, void* stream) {
  return upf_corr81_norm_forward_c8_pitched(f1, f2, 0, out8, out8_batch_stride, B, C, H, W, dtype, leaky_slope, workspace, stream);
}

// The NORM cost volume — the variant inside the inference step — timed like upf_corr81_forward_timed (norm_run).
static int norm_forward_timed_impl(bool c8, const void* f1, const void* f2, void* out, int B, int C, int H, int W, int dtype,
                                   long long out_batch_stride, float leaky_slope, void* workspace, void* stream, int nrep,
                                   float* avg_us, float* min_us, int fp = 0, int out_dtype = -1) {
  using namespace upf;
  if (out_dtype < 0) out_dtype = dtype;
  UPF_REQUIRE(out_dtype == dtype || (c8 && dtype == UPF_F16 && out_dtype == UPF_BF16), UPF_EUNSUPPORTED,
              "corr81_norm_forward_timed: a second output type is timed for fp16 features -> bf16 octets only (the `pyramid_dtype` step)");
  UPF_REQUIRE(f1 && f2 && out && workspace && avg_us, UPF_EINVAL, "corr81_norm_forward_timed: null pointer");
  UPF_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && nrep > 0 && nrep <= 1024, UPF_EINVAL, "corr81_norm_forward_timed: bad arguments");
  if (fp == 0) fp = W;
  UPF_REQUIRE(upf_corr81_norm_supported(C, dtype) && (size_t)C * H * fp * 2 < (1ull << 31), UPF_EUNSUPPORTED, "corr81_norm_forward_timed: unsupported shape / dtype");
  if (c8) {
    const int rc8 = norm_c8_check(f1, f2, out, out_batch_stride, H, W, fp, "corr81_norm_forward_c8_timed");
    if (rc8 != UPF_OK) return rc8;
  } else if (out_batch_stride == 0) out_batch_stride = (long long)corr::ND * H * W;
  return corr::norm_run(c8 ? "corr81_norm_forward_c8_timed" : "corr81_norm_forward_timed", c8,
                        {f1, f2, out, B, C, H, W, fp, out_batch_stride, leaky_slope, (hipStream_t)stream}, dtype, out_dtype, workspace, nrep, avg_us, min_us);
}

extern "C" int upf_corr81_norm_forward_timed(const void* f1, const void* f2, void* out, int B, int C, int H, int W, int dtype,
                                             long long out_batch_stride, float leaky_slope, void* workspace, void* stream, int nrep,
                                             float* avg_us, float* min_us) {
  return norm_forward_timed_impl(false, f1, f2, out, B, C, H, W, dtype, out_batch_stride, leaky_slope, workspace, stream, nrep, avg_us, min_us);
}
extern "C" int upf_corr81_norm_forward_c8_timed(const void* f1, const void* f2, void* out8, long long out8_batch_stride, int B, int C, int H, int W,
                                                int dtype, float leaky_slope, void* workspace, void* stream, int nrep, float* avg_us, float* min_us) {
  return norm_forward_timed_impl(true, f1, f2, out8, B, C, H, W, dtype, out8_batch_stride, leaky_slope, workspace, stream, nrep, avg_us, min_us);
}

extern "C" int upf_corr81_norm_forward_c8_timed_pitched(const void* f1, const void* f2, int f_row_pitch, void* out8, long long out8_batch_stride, int B, int C, int H, int W,
                                                        int dtype, float leaky_slope, void* workspace, void* stream, int nrep, float* avg_us, float* min_us) {
  return norm_forward_timed_impl(true, f1, f2, out8, B, C, H, W, dtype, out8_batch_stride, leaky_slope, workspace, stream, nrep, avg_us, min_us, f_row_pitch);
}

extern "C" int upf_corr81_norm_forward_c8_timed_mixed(const void* f1, const void* f2, int f_row_pitch, void* out8, long long out8_batch_stride, int B, int C, int H, int W,
                                                      int dtype, int out_dtype, float leaky_slope, void* workspace, void* stream, int nrep, float* avg_us, float* min_us) {
  return norm_forward_timed_impl(true, f1, f2, out8, B, C, H, W, dtype, out8_batch_stride, leaky_slope, workspace, stream, nrep, avg_us, min_us, f_row_pitch, out_dtype);
}

extern "C" int upf_corr_set_option(const char* name, int value) {
  using namespace upf::corr;
  int* slot = nullptr;
  if (name && !strcmp(name, "variant")) slot = &g_variant;
  else if (name && !strcmp(name, "old_path")) slot = &g_old_path;
  if (!slot) return -1000;
  const int prev = *slot;
  *slot = value;
  return prev;
}
