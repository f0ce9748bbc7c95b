// Batch assembly from uint8 frames (include/upflow_hip.h: upf_frames_u8_assemble): horizontal flip, normalisation, HWC -> CHW
// transpose and the training crop of the host data path (dataset/kitti_dataset.py: img_func.get_process_img_only_img,
// kitti_data_with_start_point.random_crop), one launch on the stream — so it is captured with the training step, and a replay
// reads the crop offsets and flip flags of the NEXT batch from device memory.
//
// Arithmetic: the host computes (uint8 - mean[c]) / stddev in float64 and np_2_tensor rounds once to fp32.  There are only
// 3 x 256 different operands, so every workgroup evaluates exactly that expression (IEEE double subtraction and division, one
// conversion to fp32; -ffp-contract=off) into a 3 KB table in LDS and the pixels are look-ups: the output equals the host path's
// bit for bit, with no double arithmetic per pixel.
//
// Data movement.  A workgroup owns (frame, batch item, ONE row, a tile of TX output pixels of it):
//   * the tile's source bytes — 3 bytes per pixel, a row is 3W bytes so its dword phase changes from row to row — are read ONCE,
//     as aligned dwords (a dword that is not wholly inside the tensor is assembled from guarded byte loads), into LDS; the loads
//     are in flight while the table is computed;
//   * the un-cropped frame and the crop are both written from that LDS copy, as groups of four consecutive floats of one channel.
//     A group starts where the DESTINATION address is 16-byte aligned (raw rows start at any multiple of 4 bytes: W = 1242; the
//     crop's phase depends on nothing the raw frame's does), so interior groups are one 16-byte store per lane and a row's first
//     and last group fall back to dword stores.  A group belongs to the tile its first pixel inside the row lies in; it may end
//     up to HALO pixels past the tile, which is why a tile stages HALO more pixels than it owns.
// Measured on MI355X at B = 4, 375x1242 -> 256x832 (tools/ingest_u8_measure.py): one row per workgroup 16.6 us per launch; 2 / 4 /
// 8 rows per workgroup with the next row's loads in flight behind the conversion 17.3 / 20.6 / 33 us (fewer, longer workgroups
// hide less latency than the table costs); tiles of 672 / 448 / 336 pixels 17.8 / 20.6 / 22.3 us.
// `aug` is device memory: x, y are clamped to [0, W-pw] x [0, H-ph] and flip is `!= 0` here, so no value of it makes the kernel
// read outside `src` or write outside the outputs (the host cannot look at it without a synchronisation).
//
// 16-bit inference ingest (upf_frames_u8_stack16): the same workgroup, the same staged row, no crop; the two frame sets go to the
// two halves of ONE stacked [2B,3,H,W] fp16 / bf16 tensor — and, where the decoder runs in the other 16-bit type, of a second one
// from the same staged bytes.  The table holds, per operand, the fp32 value above rounded to nearest-even to each requested type
// (what ATen's copy_ of the fp32 tensor stores), both in one dword, so a pixel is one byte read and one table read whatever the
// number of outputs.  A group is EIGHT consecutive values of one channel = one 16-byte store where the destination is 16-byte
// aligned: every group of a pitched row (ops.empty_nchw: the tail group ends in the padding columns) and of a W % 8 == 0 row;
// contiguous ragged rows have a first and a last group of 2-byte stores.
#include "common.hpp"

namespace upf {
namespace ingest {

constexpr int NT = 256;
constexpr int TX = 1344;                 // output pixels of a row per workgroup (KITTI's 1242 is one tile)
constexpr int HALO = 3;                  // fp32 groups: four values
constexpr int HALO16 = 7;                // 16-bit groups: eight
constexpr int NDW = (3 + 3 * (TX + HALO16) + 4 * NT - 1) / (4 * NT);    // staged dwords per thread
constexpr int ROWDW = NT * NDW;
constexpr int NG = TX / 4 + 2;           // >= the 16-byte groups of one channel that can start inside a tile
constexpr int NG16 = TX / 8 + 2;
static_assert(TX % 8 == 0 && HALO <= HALO16 && 3 + 3 * (TX + HALO16) <= 4 * ROWDW,
              "a staged tile (plus up to 3 bytes of dword phase) must fit the row buffer");
static_assert((TX + HALO + 3) / 4 + 1 <= NG, "group starts within TX + HALO pixels");
static_assert((TX + HALO16 + 7) / 8 + 1 <= NG16, "group starts within TX + HALO16 pixels");

struct Args {
  const uint8_t* src1;
  const uint8_t* src2;
  const int* aug;
  float* raw1;
  float* raw2;
  float* crop1;
  float* crop2;
  float* start;
  int B, H, W, ph, pw, nf;
  double mean0, mean1, mean2, stddev;
};

// the tile's source bytes of row y -> this thread's NDW dwords.  a0: offset in src of the first needed byte; every dword is
// aligned in MEMORY (mis = the address of that byte mod 4); src[0, total) is the whole tensor and nothing outside it is touched.
__device__ __forceinline__ void stage_load(uint32_t (&v)[NDW], const uint8_t* __restrict__ src, long long a0, int mis, int nbytes,
                                           long long total) {
  const long long aa = a0 - mis;                     // (may be -3 .. -1 at the very start of the tensor)
  const int ndw = (mis + nbytes + 3) >> 2;
#pragma unroll
  for (int k = 0; k < NDW; ++k) {
    const int i = (int)threadIdx.x + k * NT;
    uint32_t w = 0;
    if (i < ndw) {
      const long long d = aa + 4ll * i;
      if (d >= 0 && d + 4 <= total) {
        w = *reinterpret_cast<const uint32_t*>(src + d);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (d + j >= 0 && d + j < total) w |= (uint32_t)src[d + j] << (8 * j);
      }
    }
    v[k] = w;
  }
}

// One row's tile, shared by the two kernels.  stage_tile starts the loads of the source pixels behind output pixels [o0, o1s) of
// row y of item b — pixels [lo, lo + o1s - o0) of the source row, lo = o0 or, flipped, W - o1s — and stage_commit puts them into
// the row buffer (the caller computes its table between the two): rowbuf bytes [mis + 3 * s + c] = channel c of source pixel lo + s.
struct Tile {
  int lo, mis;
};

__device__ __forceinline__ Tile stage_tile(uint32_t (&pre)[NDW], const uint8_t* __restrict__ src, int b, int y, int o0, int o1s, int flip,
                                           int B, int H, int W) {
  Tile t;
  t.lo = flip ? W - o1s : o0;
  const long long a0 = ((long long)b * H + y) * 3 * W + 3 * t.lo;
  t.mis = (int)((a0 + (long long)(reinterpret_cast<uintptr_t>(src) & 3)) & 3);
  stage_load(pre, src, a0, t.mis, 3 * (o1s - o0), (long long)B * H * W * 3);
  return t;
}

__device__ __forceinline__ void stage_commit(uint32_t* rowbuf, const uint32_t (&pre)[NDW]) {
#pragma unroll
  for (int k = 0; k < NDW; ++k) rowbuf[(int)threadIdx.x + k * NT] = pre[k];
  __syncthreads();
}

// four consecutive floats of one channel: dst_row[d0 + e] (written where 0 <= d0 + e < n) = pixel x0 + e of the output row, from
// the staged bytes: lb[3 * s] is that channel of source pixel lo + s, and output pixel x is source pixel flip ? W-1-x : x.
__device__ __forceinline__ void emit_group(float* __restrict__ dst_row, int d0, int n, const uint8_t* lb, const float* tab_c,
                                           int x0, int flip, int W, int lo) {
  float v[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ok[e] = d0 + e >= 0 && d0 + e < n;
    const int x = x0 + e;
    const int s = (flip ? W - 1 - x : x) - lo;
    v[e] = ok[e] ? tab_c[lb[3 * s]] : 0.f;
  }
  if (ok[0] && ok[3]) {
    *reinterpret_cast<float4*>(dst_row + d0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (ok[e]) dst_row[d0 + e] = v[e];
  }
}

__global__ __launch_bounds__(NT) void assemble_kernel(const Args a) {
  __shared__ float tab[3 * 256];
  __shared__ uint32_t rowbuf[ROWDW];
  const int tid = threadIdx.x;
  const int H = a.H, W = a.W, ph = a.ph, pw = a.pw;
  const int f = (int)blockIdx.z % a.nf, b = (int)blockIdx.z / a.nf;
  const int y = blockIdx.y;
  const int o0 = (int)blockIdx.x * TX, o1 = min(W, o0 + TX), o1s = min(W, o1 + HALO);
  int xb = 0, yb = 0, flip = 0;
  if (a.aug) {
    xb = a.aug[3 * b];
    yb = a.aug[3 * b + 1];
    flip = a.aug[3 * b + 2] != 0;
  }
  xb = max(min(xb, W - pw), 0);
  yb = max(min(yb, H - ph), 0);
  if (a.start && f == 0 && blockIdx.x == 0 && y == 0 && tid == 0) {
    a.start[2 * b] = (float)xb;
    a.start[2 * b + 1] = (float)yb;
  }
  const uint8_t* src = f ? a.src2 : a.src1;
  float* __restrict__ raw = f ? a.raw2 : a.raw1;
  float* __restrict__ crop = f ? a.crop2 : a.crop1;

  // the row's bytes are on their way while the table is computed
  uint32_t pre[NDW];
  const Tile t = stage_tile(pre, src, b, y, o0, o1s, flip, a.B, H, W);
  const int lo = t.lo;                               // first staged source pixel
  tab[tid] = (float)(((double)tid - a.mean0) / a.stddev);
  tab[256 + tid] = (float)(((double)tid - a.mean1) / a.stddev);
  tab[512 + tid] = (float)(((double)tid - a.mean2) / a.stddev);
  stage_commit(rowbuf, pre);

  const uint8_t* lb0 = reinterpret_cast<const uint8_t*>(rowbuf) + t.mis;
  const int pm_raw = (int)((reinterpret_cast<uintptr_t>(raw) >> 2) & 3);
  const int pm_crop = (int)((reinterpret_cast<uintptr_t>(crop) >> 2) & 3);
  const int jlo = max(o0 - xb, 0);                   // first crop column this tile can own
  const int ci = y - yb;                             // crop row
  const bool in_crop = crop != nullptr && ci >= 0 && ci < ph;
  for (int q = tid; q < 3 * NG; q += NT) {
    const int c = q / NG, g = q - c * NG;
    const uint8_t* lb = lb0 + c;
    const float* tab_c = tab + 256 * c;
    {
      const long long e0 = (((long long)b * 3 + c) * H + y) * W;
      const int phase = (int)((e0 + pm_raw) & 3);
      const int d0 = 4 * ((o0 + phase) / 4 + g) - phase;         // the group's first column (may be < 0 or end >= W)
      const int own = max(d0, 0);
      if (own >= o0 && own < o1) emit_group(raw + e0, d0, W, lb, tab_c, d0, flip, W, lo);
    }
    if (in_crop) {
      const long long e0 = (((long long)b * 3 + c) * ph + ci) * pw;
      const int phase = (int)((e0 + pm_crop) & 3);
      const int d0 = 4 * ((jlo + phase) / 4 + g) - phase;        // crop column
      const int own = max(d0, 0);
      if (own < pw && xb + own >= o0 && xb + own < o1) emit_group(crop + e0, d0, pw, lb, tab_c, xb + d0, flip, W, lo);
    }
  }
}

// ---- 16-bit stacked frames ------------------------------------------------------------------------------------------------------
struct Args16 {
  const uint8_t* src1;
  const uint8_t* src2;
  const int* flip;
  uint16_t* x;
  uint16_t* xd;                           // null: one output
  long long x_bs, xd_bs;                  // batch strides, elements
  int x_pitch, xd_pitch, x_bf16, xd_bf16;
  int B, H, W;
  double mean0, mean1, mean2, stddev;
};

// fp32 -> the bits of the 16-bit type, round to nearest even (ATen's copy_: v_cvt_f16_f32 / c10::BFloat16's integer rounding)
__device__ __forceinline__ uint32_t round16(float f, int bf16) {
  if (bf16) {
    const uint32_t u = __float_as_uint(f);
    return f != f ? 0x7fc0u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  }
  return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
}

// the table words of output pixels x0 .. x0 + 7 of one channel (lb, tab_c: that channel's).  A column outside [0, W) — never
// stored, or stored into the padding of a pitched row — takes the nearest pixel's, so every read stays inside the staged tile.
__device__ __forceinline__ void gather_group16(uint32_t (&u)[8], int x0, const uint8_t* lb, const uint32_t* tab_c, int flip, int W, int lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int x = min(max(x0 + e, 0), W - 1);
    u[e] = tab_c[lb[3 * ((flip ? W - 1 - x : x) - lo)]];
  }
}

// dst_row[d0 + e] (written where 0 <= d0 + e < n) = bits [sh, sh + 16) of u[e]; dst_row + d0 is 16-byte aligned
__device__ __forceinline__ void store_group16(uint16_t* __restrict__ dst_row, int d0, int n, const uint32_t (&u)[8], int sh) {
  if (d0 >= 0 && d0 + 8 <= n) {
    uint4 v;
    v.x = ((u[0] >> sh) & 0xffffu) | ((u[1] >> sh) << 16);
    v.y = ((u[2] >> sh) & 0xffffu) | ((u[3] >> sh) << 16);
    v.z = ((u[4] >> sh) & 0xffffu) | ((u[5] >> sh) << 16);
    v.w = ((u[6] >> sh) & 0xffffu) | ((u[7] >> sh) << 16);
    *reinterpret_cast<uint4*>(dst_row + d0) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (d0 + e >= 0 && d0 + e < n) dst_row[d0 + e] = (uint16_t)(u[e] >> sh);
  }
}

__global__ __launch_bounds__(NT) void stack16_kernel(const Args16 a) {
  __shared__ uint32_t tab[3 * 256];       // low half: the operand in x's type, high half: in xd's
  __shared__ uint32_t rowbuf[ROWDW];
  const int tid = threadIdx.x;
  const int H = a.H, W = a.W;
  const int f = (int)blockIdx.z & 1, b = (int)blockIdx.z >> 1;
  const int y = blockIdx.y;
  const int o0 = (int)blockIdx.x * TX, o1 = min(W, o0 + TX), o1s = min(W, o1 + HALO16);
  const int flip = a.flip ? a.flip[b] != 0 : 0;

  uint32_t pre[NDW];
  const Tile t = stage_tile(pre, f ? a.src2 : a.src1, b, y, o0, o1s, flip, a.B, H, W);
  const double mean[3] = {a.mean0, a.mean1, a.mean2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = (float)(((double)tid - mean[c]) / a.stddev);
    tab[256 * c + tid] = round16(v, a.x_bf16) | (a.xd ? round16(v, a.xd_bf16) << 16 : 0u);
  }
  stage_commit(rowbuf, pre);

  const uint8_t* lb0 = reinterpret_cast<const uint8_t*>(rowbuf) + t.mis;
  const long long item = (long long)f * a.B + b;     // X = [frames 1; frames 2]
  for (int q = tid; q < 3 * NG16; q += NT) {
    const int c = q / NG16, g = q - c * NG16;
    const uint8_t* lb = lb0 + c;
    const uint32_t* tab_c = tab + 256 * c;
    const long long row = (long long)c * H + y;
    uint32_t u[8];
    int have = -8 - TX;                              // the column u was gathered for (none yet)
    {
      uint16_t* dst = a.x + item * a.x_bs + row * a.x_pitch;
      const int phase = (int)((reinterpret_cast<uintptr_t>(dst) >> 1) & 7);
      const int d0 = 8 * ((o0 + phase) / 8 + g) - phase;         // the group's first column (may be < 0 or end >= W)
      const int own = max(d0, 0);
      if (own >= o0 && own < o1) {
        gather_group16(u, d0, lb, tab_c, flip, W, t.lo);
        have = d0;
        store_group16(dst, d0, a.x_pitch, u, 0);
      }
    }
    if (a.xd) {
      uint16_t* dst = a.xd + item * a.xd_bs + row * a.xd_pitch;
      const int phase = (int)((reinterpret_cast<uintptr_t>(dst) >> 1) & 7);
      const int d0 = 8 * ((o0 + phase) / 8 + g) - phase;
      const int own = max(d0, 0);
      if (own >= o0 && own < o1) {
        if (have != d0) gather_group16(u, d0, lb, tab_c, flip, W, t.lo);
        store_group16(dst, d0, a.xd_pitch, u, 16);
      }
    }
  }
}

}  // namespace ingest
}  // namespace upf

extern "C" int upf_frames_u8_assemble(const unsigned char* src1, const unsigned char* src2, const int* aug, float* raw1, float* raw2,
                                      float* crop1, float* crop2, float* start, int B, int H, int W, int ph, int pw, double mean0,
                                      double mean1, double mean2, double stddev, void* stream) {
  using namespace upf;
  UPF_REQUIRE(B > 0 && H > 0 && W > 0, UPF_EINVAL, "frames_u8_assemble: B, H, W must be positive (got %d, %d, %d)", B, H, W);
  UPF_REQUIRE(src1 && raw1, UPF_EINVAL, "frames_u8_assemble: null src1 / raw1");
  UPF_REQUIRE(!src2 || raw2, UPF_EINVAL, "frames_u8_assemble: src2 given without raw2");
  UPF_REQUIRE(ph >= 0 && pw >= 0 && (ph > 0) == (pw > 0), UPF_EINVAL,
              "frames_u8_assemble: crop %d x %d (both positive, or both 0 for no crops)", ph, pw);
  UPF_REQUIRE(ph <= H && pw <= W, UPF_EINVAL, "frames_u8_assemble: crop %d x %d larger than the %d x %d frame", ph, pw, H, W);
  if (ph > 0) UPF_REQUIRE(crop1 && (!src2 || crop2), UPF_EINVAL, "frames_u8_assemble: crop size given without crop buffers");
  UPF_REQUIRE(stddev == stddev && stddev != 0.0, UPF_EINVAL, "frames_u8_assemble: stddev must be a non-zero number");
  UPF_REQUIRE(3ll * H * W * 4 < (1ll << 31), UPF_EUNSUPPORTED, "frames_u8_assemble: a batch item of 3 x %d x %d fp32 is 2 GiB or more", H, W);
  UPF_REQUIRE(aligned_to(raw1, 4) && aligned_to(raw2, 4) && aligned_to(crop1, 4) && aligned_to(crop2, 4) && aligned_to(start, 4) &&
                  aligned_to(aug, 4), UPF_EALIGN, "frames_u8_assemble: fp32 / int32 operands must be 4-byte aligned");
  const int nf = src2 ? 2 : 1;
  const long long gz = (long long)B * nf;
  const int gy = H, gx = cdiv(W, ingest::TX);
  UPF_REQUIRE(gz <= 65535 && gy <= 65535, UPF_EUNSUPPORTED, "frames_u8_assemble: %lld frames x %d rows exceed the launch grid", gz, H);
  const bool crops = ph > 0;
  const ingest::Args a{src1, src2, aug, raw1, src2 ? raw2 : nullptr, crops ? crop1 : nullptr, crops && src2 ? crop2 : nullptr, start,
                       B, H, W, ph, pw, nf, mean0, mean1, mean2, stddev};
  hipLaunchKernelGGL(ingest::assemble_kernel, dim3(gx, gy, (unsigned)gz), dim3(ingest::NT), 0, (hipStream_t)stream, a);
  return check_launch("frames_u8_assemble");
}

extern "C" int upf_frames_u8_stack16(const unsigned char* src1, const unsigned char* src2, const int* flip, void* x, int x_dtype,
                                     long long x_pitch, long long x_batch_stride, void* xd, int xd_dtype, long long xd_pitch,
                                     long long xd_batch_stride, int B, int H, int W, double mean0, double mean1, double mean2,
                                     double stddev, void* stream) {
  using namespace upf;
  UPF_REQUIRE(B > 0 && H > 0 && W > 0, UPF_EINVAL, "frames_u8_stack16: B, H, W must be positive (got %d, %d, %d)", B, H, W);
  UPF_REQUIRE(src1 && src2 && x, UPF_EINVAL, "frames_u8_stack16: null src1 / src2 / x");
  UPF_REQUIRE(stddev == stddev && stddev != 0.0, UPF_EINVAL, "frames_u8_stack16: stddev must be a non-zero number");
  UPF_REQUIRE(aligned_to(flip, 4) && aligned_to(x, 2) && aligned_to(xd, 2), UPF_EALIGN,
              "frames_u8_stack16: flip must be 4-byte aligned, x / xd 2-byte aligned");
  const struct { const char* name; const void* p; int dtype; long long pitch, bs; } outs[2] = {
      {"x", x, x_dtype, x_pitch, x_batch_stride}, {"xd", xd, xd_dtype, xd_pitch, xd_batch_stride}};
  for (const auto& o : outs) {
    if (!o.p) continue;
    UPF_REQUIRE(o.dtype == UPF_F16 || o.dtype == UPF_BF16, UPF_EDTYPE, "frames_u8_stack16: %s must be UPF_F16 or UPF_BF16 (got %d)", o.name,
                o.dtype);
    // contiguous rows, or the padding ops.empty_nchw makes: a tail group may end in columns [W, pitch), nowhere else
    UPF_REQUIRE(o.pitch == W || (o.pitch > W && o.pitch % 8 == 0 && o.pitch - W < 8), UPF_EINVAL,
                "frames_u8_stack16: %s pitch %lld for W = %d (W, or W rounded up to a multiple of 8)", o.name, o.pitch, W);
    UPF_REQUIRE(o.bs >= 3ll * H * o.pitch, UPF_EINVAL, "frames_u8_stack16: %s batch stride %lld is less than an item (3 x %d x %lld)", o.name,
                o.bs, H, o.pitch);
  }
  const long long gz = 2ll * B;
  const int gy = H, gx = cdiv(W, ingest::TX);
  UPF_REQUIRE(gz <= 65535 && gy <= 65535, UPF_EUNSUPPORTED, "frames_u8_stack16: %lld frames x %d rows exceed the launch grid", gz, H);
  const ingest::Args16 a{src1, src2, flip, static_cast<uint16_t*>(x), static_cast<uint16_t*>(xd), x_batch_stride, xd ? xd_batch_stride : 0,
                         (int)x_pitch, xd ? (int)xd_pitch : 0, x_dtype == UPF_BF16, xd && xd_dtype == UPF_BF16, B, H, W,
                         mean0, mean1, mean2, stddev};
  hipLaunchKernelGGL(ingest::stack16_kernel, dim3(gx, gy, (unsigned)gz), dim3(ingest::NT), 0, (hipStream_t)stream, a);
  return check_launch("frames_u8_stack16");
}
