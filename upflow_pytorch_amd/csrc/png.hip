// PNG compression on the device (include/upflow_hip.h has the contract; DESIGN §13 the reasoning): from the samples of B images,
// uint8 / uint16 [B,H,W,C], one complete zlib stream per image — header, ONE final dynamic-Huffman deflate block whose every symbol
// is a literal, Adler-32 — in three launches, none of which waits for another workgroup:
//   1. filter: a workgroup takes CHUNK bytes of the flat filtered stream (filter type 2, then cur - above over the big-endian
//      sample bytes), stores them in the workspace with the chunk's 256 byte counts (uint16) and its two Adler sums, and zeroes
//      its share of the image's output slot;
//   2. code, one workgroup per image: adds up the counts, builds the Huffman code (rank sort, two-queue merge on one lane, halving
//      beyond 15 bits), weighs the flat 8 / 9-bit code against it, writes the block header, the table for launch 3, every chunk's
//      bit offset (counts x lengths, then a scan), and the tail: end-of-block, Adler-32, the stream's length;
//   3. pack: a workgroup packs its chunk into LDS at the chunk's bit offset modulo 32 and copies the words out: the interior with
//      plain stores, the first and the last word, which a neighbour shares, with atomicOr into the zeroed slot.
// Integer arithmetic throughout, and the OR of disjoint bits: the same bytes whatever the order.  tests/_png_model.py states the
// encoder in Python; the tests compare byte for byte.
#include "common.hpp"

namespace upf {
namespace png {

constexpr int CHUNK = 4096;                                  // bytes of the filtered stream per workgroup of launches 1 and 3
constexpr int NT = 256;                                      // threads of those workgroups: 16 bytes each
constexpr int BPT = CHUNK / NT;
constexpr int NT2 = 1024;                                    // threads of the coding workgroup
constexpr int NSYM = 257, EOB = 256;
constexpr int MAX_BITS = 15;
constexpr int HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 4;  // 1106
constexpr int DATA_START = 16 + HEADER_BITS;                 // the first literal's bit in the slot
constexpr int HEADER_WORDS = (DATA_START + 31) / 32;
constexpr int PACK_WORDS = (31 + CHUNK * MAX_BITS + 31) / 32 + 3;
constexpr uint32_t ADLER = 65521;
static_assert(BPT == 16 && CHUNK <= 65535, "16 bytes per lane; a chunk's counts are uint16");

// the workspace of one image (byte offsets; every part 16-byte aligned)
struct Layout {
  size_t filt, chist, adler, goff, ctab, total;
};
__host__ __device__ inline Layout layout(size_t nchunks) {
  Layout l;
  l.filt = 0;
  l.chist = l.filt + nchunks * CHUNK;                        // uint16 [nchunks][256]
  l.adler = l.chist + nchunks * 512;                         // uint32 [nchunks][2]: sum of bytes, sum of (end - i) * byte, mod 65521
  l.goff = l.adler + nchunks * 8;                            // uint64 [nchunks]: the chunk's first bit in the slot
  l.ctab = l.goff + nchunks * 8;                             // uint32 [NSYM]: reversed code | length << 16
  l.total = (l.ctab + NSYM * 4 + 255) / 256 * 256;
  return l;
}

struct Shape {
  uint32_t H, stride, n, nchunks, cap;                       // stride: bytes of a row of samples; n = H * (stride + 1)
  int swap;                                                  // 1: 16-bit samples, byte k of a row is memory byte k ^ 1
};

// ---- launch 1 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT)
void filter_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ ws, uint32_t* __restrict__ out, Shape s) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t red[2 * NT / 64];
  const uint32_t t = threadIdx.x;
  const uint32_t b = blockIdx.x / s.nchunks, j = blockIdx.x - b * s.nchunks;
  const Layout l = layout(s.nchunks);
  uint8_t* __restrict__ w = ws + (size_t)b * l.total;
  const uint8_t* __restrict__ im = img + (size_t)b * s.H * s.stride;
  hist[t] = 0;
  __syncthreads();
  const uint32_t rowlen = s.stride + 1;
  const uint32_t c0 = j * CHUNK, len = min((uint32_t)CHUNK, s.n - c0);
  const uint32_t p0 = c0 + t * BPT;
  uint32_t row = p0 / rowlen, col = p0 - row * rowlen;
  uint32_t v[BPT / 4] = {0, 0, 0, 0};
  uint32_t s1 = 0, s2 = 0;
  if (p0 < s.n) {
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
      if (p0 + i < s.n) {
        uint32_t x = 2;
        if (col) {
          const size_t a = (size_t)row * s.stride + ((col - 1) ^ s.swap);
          x = im[a];
          if (row) x = (x - im[a - s.stride]) & 255u;
        }
        v[i >> 2] |= x << (8 * (i & 3));
        atomicAdd(&hist[x], 1u);
        s1 += x;
        s2 += (len - (t * BPT + i)) * x;                     // < 16 * 4096 * 255
        if (++col == rowlen) { col = 0; ++row; }
      }
    }
  }
  *(uint4*)(w + l.filt + (size_t)c0 + t * BPT) = make_uint4(v[0], v[1], v[2], v[3]);
  s2 %= ADLER;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  if ((t & 63) == 0) { red[t >> 6] = s1; red[NT / 64 + (t >> 6)] = s2; }
  __syncthreads();
  if (t == 0) {
    uint32_t a = 0, c = 0;
    for (int k = 0; k < NT / 64; ++k) { a += red[k]; c += red[NT / 64 + k]; }
    ((uint2*)(w + l.adler))[j] = make_uint2(a % ADLER, c % ADLER);
  }
  if (t < 128) ((uint32_t*)(w + l.chist))[(size_t)j * 128 + t] = hist[2 * t] | (hist[2 * t + 1] << 16);
  // this chunk's share of the slot's words
  const uint32_t capw = s.cap / 4, per = (capw + s.nchunks - 1) / s.nchunks;
  const uint32_t hi = min(capw, (j + 1) * per);
  uint32_t* __restrict__ o = out + (size_t)b * capw;
  for (uint32_t k = j * per + t; k < hi; k += NT) o[k] = 0;
}

// ---- launch 2 ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool before(uint32_t fa, int a, uint32_t fb, int b) { return fa < fb || (fa == fb && a < b); }

__device__ __forceinline__ void lds_put(uint32_t* buf, uint32_t pos, uint32_t value, int nbits) {   // nbits <= 32
  const uint64_t x = (uint64_t)value << (pos & 31);
  if ((uint32_t)x) atomicOr(&buf[pos >> 5], (uint32_t)x);
  if (x >> 32) atomicOr(&buf[(pos >> 5) + 1], (uint32_t)(x >> 32));
}

__device__ __forceinline__ void global_put(uint32_t* out, uint64_t pos, uint32_t value) {
  const uint64_t x = (uint64_t)value << (pos & 31);
  if ((uint32_t)x) atomicOr(&out[pos >> 5], (uint32_t)x);
  if (x >> 32) atomicOr(&out[(pos >> 5) + 1], (uint32_t)(x >> 32));
}

__global__ __launch_bounds__(NT2)
void code_kernel(uint8_t* __restrict__ ws, uint32_t* __restrict__ out, int* __restrict__ lengths, Shape s) {
  __shared__ uint32_t ftrue[NSYM], f[NSYM], lw[NSYM], iw[NSYM];
  __shared__ uint16_t order[NSYM], pl[NSYM], pi[NSYM], di[NSYM];
  __shared__ uint8_t len[264], flat[264];
  __shared__ uint32_t nxt[MAX_BITS + 2], hdr[HEADER_WORDS], wtot[NT2 / 64];
  __shared__ unsigned long long cost[2], adl[2];
  __shared__ uint32_t eob, nsym, deep, count[MAX_BITS + 1];
  const int t = threadIdx.x;
  const uint32_t b = blockIdx.x;
  const Layout l = layout(s.nchunks);
  uint8_t* __restrict__ w = ws + (size_t)b * l.total;
  const uint16_t* __restrict__ chist = (const uint16_t*)(w + l.chist);
  uint32_t* __restrict__ o = out + (size_t)b * (s.cap / 4);

  // the image's counts: the sum over its chunks; one end-of-block
  if (t < NSYM) ftrue[t] = (t == EOB);
  if (t < 264) len[t] = 0;
  if (t < HEADER_WORDS) hdr[t] = 0;
  if (t < 2) { cost[t] = 0; adl[t] = 0; }
  __syncthreads();
  {
    uint32_t acc = 0;
    for (uint32_t c = t >> 8; c < s.nchunks; c += NT2 / 256) acc += chist[(size_t)c * 256 + (t & 255)];
    atomicAdd(&ftrue[t & 255], acc);
  }
  __syncthreads();
  // the flat code: 9 bits for the two first symbols in (count, symbol) order, 8 for the rest
  if (t < NSYM) {
    const uint32_t ft = ftrue[t];
    int r = 0;
    for (int k = 0; k < NSYM; ++k) r += before(ftrue[k], k, ft, t);
    flat[t] = r < 2 ? 9 : 8;
    f[t] = ft;
  }
  // the Huffman code of f; counts halved until its deepest leaf fits 15 bits
  for (int round = 0; round < 32; ++round) {                 // (31 halvings leave every count at 1: a tree of 9 levels)
    if (t == 0) { nsym = 0; deep = 0; }
    __syncthreads();
    const uint32_t ft = t < NSYM ? f[t] : 0;
    if (ft) {
      int r = 0;
      for (int k = 0; k < NSYM; ++k) r += (f[k] != 0) && before(f[k], k, ft, t);
      order[r] = (uint16_t)t;
      lw[r] = ft;
      atomicAdd(&nsym, 1u);
    }
    __syncthreads();
    const int m = (int)nsym;
    if (t == 0 && m > 1) {
      int li = 0, ii = 0;
      for (int k = 0; k < m - 1; ++k) {                      // two queues: the sorted leaves, the nodes made so far
        uint32_t sum = 0;
        for (int h = 0; h < 2; ++h) {
          if (li < m && (ii >= k || lw[li] <= iw[ii])) { sum += lw[li]; pl[li++] = (uint16_t)k; }
          else { sum += iw[ii]; pi[ii++] = (uint16_t)k; }
        }
        iw[k] = sum;
      }
      di[m - 2] = 0;
      for (int k = m - 3; k >= 0; --k) di[k] = di[pi[k]] + 1;
    }
    __syncthreads();
    if (t < m) {
      const int mine = m > 1 ? di[pl[t]] + 1 : 1;
      len[order[t]] = (uint8_t)min(mine, 255);
      if (mine > MAX_BITS) deep = 1;
    }
    __syncthreads();
    if (!deep) break;
    if (ft) f[t] = (ft + 1) >> 1;
    __syncthreads();                                         // (everyone has read `deep` before lane 0 clears it)
  }
  // whichever is cheaper over the true counts; the flat code on strictly fewer bits only
  if (t < NSYM) {
    atomicAdd(&cost[0], (unsigned long long)ftrue[t] * len[t]);
    atomicAdd(&cost[1], (unsigned long long)ftrue[t] * flat[t]);
  }
  __syncthreads();
  if (cost[1] < cost[0] && t < NSYM) len[t] = flat[t];
  __syncthreads();
  // canonical codes, bit-reversed: deflate packs from the least significant bit, Huffman codes go in most significant bit first
  if (t == 0) {
    for (int k = 0; k <= MAX_BITS; ++k) count[k] = 0;
    for (int k = 0; k < NSYM; ++k) count[len[k]]++;
    count[0] = 0;
    uint32_t code = 0;
    nxt[0] = 0;
    for (int k = 1; k <= MAX_BITS; ++k) { code = (code + count[k - 1]) << 1; nxt[k] = code; }
    // the block header up to the lengths: 78 01; BFINAL 1, BTYPE 2, HLIT 0, HDIST 0, HCLEN 15; 3 bits per code-length code
    lds_put(hdr, 0, 0x0178, 16);
    lds_put(hdr, 16, 1 | (2 << 1) | (15u << 13), 17);
    for (int k = 3; k < 19; ++k) lds_put(hdr, 33 + 3 * k, 4, 3);       // (16, 17, 18 come first and take none)
  }
  __syncthreads();
  if (t < NSYM) {
    const int lt = len[t];
    uint32_t e = 0;
    if (lt) {
      uint32_t c = nxt[lt];
      for (int k = 0; k < t; ++k) c += (len[k] == lt);
      e = (__brev(c) >> (32 - lt)) | ((uint32_t)lt << 16);
    }
    ((uint32_t*)(w + l.ctab))[t] = e;
    if (t == EOB) eob = e & 0xffff;
  }
  if (t < 258) {                                             // 257 lengths and the one distance code of length 1; symbol k has code k
    const uint32_t lt = t < NSYM ? len[t] : 1;
    lds_put(hdr, 16 + 74 + 4 * t, __brev(lt) >> 28, 4);
  }
  __syncthreads();
  if (t < HEADER_WORDS) o[t] = hdr[t];
  // every chunk's first bit: its counts times the lengths, scanned
  uint64_t carry = DATA_START;
  uint64_t* __restrict__ goff = (uint64_t*)(w + l.goff);
  for (uint32_t base = 0; base < s.nchunks; base += NT2) {
    const uint32_t c = base + t;
    uint32_t bits = 0;
    if (c < s.nchunks) {
      const uint4* __restrict__ h = (const uint4*)(chist + (size_t)c * 256);
      for (int q = 0; q < 32; ++q) {
        const uint4 x = h[q];
        const uint8_t* lq = len + 8 * q;
        bits += (x.x & 0xffff) * lq[0] + (x.x >> 16) * lq[1] + (x.y & 0xffff) * lq[2] + (x.y >> 16) * lq[3] +
                (x.z & 0xffff) * lq[4] + (x.z >> 16) * lq[5] + (x.w & 0xffff) * lq[6] + (x.w >> 16) * lq[7];
      }
    }
    uint32_t inc = bits;                                     // (a tile: at most 1024 * 4096 * 15 bits)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(inc, d, 64);
      if ((t & 63) >= d) inc += up;
    }
    if ((t & 63) == 63) wtot[t >> 6] = inc;
    __syncthreads();
    uint32_t pre = 0, all = 0;
    for (int k = 0; k < NT2 / 64; ++k) {
      if (k < (t >> 6)) pre += wtot[k];
      all += wtot[k];
    }
    if (c < s.nchunks) goff[c] = carry + pre + inc - bits;
    carry += all;
    __syncthreads();
  }
  // Adler-32 from the chunks' sums: A = 1 + sum s1, B = n + sum (s2 + s1 * (n - end of the chunk))
  {
    const uint2* __restrict__ ad = (const uint2*)(w + l.adler);
    unsigned long long a = 0, c2 = 0;
    for (uint32_t c = t; c < s.nchunks; c += NT2) {
      const uint2 x = ad[c];
      const uint32_t end = min(s.n, (c + 1) * (uint32_t)CHUNK);
      a += x.x;
      c2 += x.y + (unsigned long long)x.x * ((s.n - end) % ADLER);
    }
    if (a) atomicAdd(&adl[0], a);
    if (c2) atomicAdd(&adl[1], c2 % ADLER);
  }
  __syncthreads();
  if (t == 0) {
    const uint32_t el = len[EOB];
    const uint64_t end = carry + el;
    const uint64_t nbytes = (end + 7) / 8 + 4;
    if (nbytes > s.cap) {
      lengths[b] = -1;                                       // (cannot happen with the cap of upf_png_encode_workspace_bytes)
    } else {
      global_put(o, carry, eob);
      const uint32_t A = (uint32_t)((1 + adl[0]) % ADLER), B = (uint32_t)((s.n + adl[1]) % ADLER);
      const uint32_t ad32 = (B << 16) | A;
      global_put(o, (nbytes - 4) * 8, __builtin_bswap32(ad32));
      lengths[b] = (int)nbytes;
    }
  }
}

// ---- launch 3 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT)
void pack_kernel(const uint8_t* __restrict__ ws, uint32_t* __restrict__ out, const int* __restrict__ lengths, Shape s) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t buf[PACK_WORDS];
  __shared__ uint32_t wtot[NT / 64];
  const uint32_t t = threadIdx.x;
  const uint32_t b = blockIdx.x / s.nchunks, j = blockIdx.x - b * s.nchunks;
  if (lengths[b] < 0) return;                                // (uniform over the workgroup)
  const Layout l = layout(s.nchunks);
  const uint8_t* __restrict__ w = ws + (size_t)b * l.total;
  tab[t] = ((const uint32_t*)(w + l.ctab))[t];
  for (uint32_t k = t; k < PACK_WORDS; k += NT) buf[k] = 0;
  const uint64_t g = ((const uint64_t*)(w + l.goff))[j];
  const uint32_t c0 = j * CHUNK, p0 = c0 + t * BPT;
  const uint4 raw = *(const uint4*)(w + l.filt + (size_t)p0);
  const uint32_t v[4] = {raw.x, raw.y, raw.z, raw.w};
  const int cnt = p0 < s.n ? (int)min((uint32_t)BPT, s.n - p0) : 0;
  __syncthreads();
  uint64_t acc[4];                                           // four codes (at most 60 bits) each
  uint32_t al[4], bits = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc[q] = 0;
    al[q] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (4 * q + i < cnt) {
        const uint32_t e = tab[(v[q] >> (8 * i)) & 255u];
        acc[q] |= (uint64_t)(e & 0xffff) << al[q];
        al[q] += e >> 16;
      }
    }
    bits += al[q];
  }
  uint32_t inc = bits;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if ((t & 63) >= (uint32_t)d) inc += up;
  }
  if ((t & 63) == 63) wtot[t >> 6] = inc;
  __syncthreads();
  uint32_t pre = 0, all = 0;
  for (uint32_t k = 0; k < NT / 64; ++k) {
    if (k < (t >> 6)) pre += wtot[k];
    all += wtot[k];
  }
  const uint32_t sh = (uint32_t)(g & 31);
  uint32_t pos = sh + pre + inc - bits;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (al[q]) {
      const uint32_t k = pos >> 5, r = pos & 31;
      const uint32_t w0 = (uint32_t)(acc[q] << r);
      const uint64_t rest = acc[q] >> (32 - r);              // (r = 0: the upper word)
      if (w0) atomicOr(&buf[k], w0);
      if ((uint32_t)rest) atomicOr(&buf[k + 1], (uint32_t)rest);
      if (rest >> 32) atomicOr(&buf[k + 2], (uint32_t)(rest >> 32));
      pos += al[q];
    }
  }
  __syncthreads();
  const uint32_t nw = (sh + all + 31) >> 5;
  uint32_t* __restrict__ o = out + (size_t)b * (s.cap / 4) + (size_t)(g >> 5);
  for (uint32_t k = t; k < nw; k += NT) {
    const uint32_t x = buf[k];
    if (k == 0 || k == nw - 1) {
      if (x) atomicOr(&o[k], x);
    } else {
      o[k] = x;
    }
  }
}

static int shape_of(const char* what, int B, int H, int W, int C, int depth, Shape* s) {
  UPF_REQUIRE(B > 0 && H > 0 && W > 0, UPF_EINVAL, "%s: B, H, W must be positive (got %d, %d, %d)", what, B, H, W);
  UPF_REQUIRE(C >= 1 && C <= 4, UPF_EINVAL, "%s: 1..4 channels (got %d)", what, C);
  UPF_REQUIRE(depth == 8 || depth == 16, UPF_EINVAL, "%s: 8 or 16 bits per sample (got %d)", what, depth);
  const long long stride = (long long)W * C * (depth / 8);
  const long long n = (long long)H * (stride + 1);
  const long long cap = (n + n / 8 + 1024 + 15) / 16 * 16;
  UPF_REQUIRE(cap < (1ll << 31), UPF_EUNSUPPORTED, "%s: a filtered stream of %lld bytes (its slot would reach 2^31)", what, n);
  // header, 9 bits at most for every byte and for the end-of-block, Adler-32
  UPF_REQUIRE(2 + (HEADER_BITS + 9 * (n + 1) + 7) / 8 + 4 <= cap, UPF_EINVAL, "%s: the slot does not hold the flat code", what);
  const long long nchunks = (n + CHUNK - 1) / CHUNK;
  UPF_REQUIRE((long long)B * nchunks < (1ll << 31), UPF_EUNSUPPORTED, "%s: %lld chunks (2^31 or more)", what, (long long)B * nchunks);
  s->H = (uint32_t)H;
  s->stride = (uint32_t)stride;
  s->n = (uint32_t)n;
  s->nchunks = (uint32_t)nchunks;
  s->cap = (uint32_t)cap;
  s->swap = depth == 16;
  return UPF_OK;
}

}  // namespace png
}  // namespace upf

extern "C" int upf_png_encode_workspace_bytes(int B, int H, int W, int C, int depth, long long* bytes, long long* cap) {
  using namespace upf;
  UPF_REQUIRE(bytes && cap, UPF_EINVAL, "png_encode_workspace_bytes: null pointer");
  png::Shape s;
  if (int rc = png::shape_of("png_encode_workspace_bytes", B, H, W, C, depth, &s)) return rc;
  *bytes = (long long)B * (long long)png::layout(s.nchunks).total;
  *cap = s.cap;
  return UPF_OK;
}

extern "C" int upf_png_encode(const void* img, unsigned char* out, int* lengths, void* workspace, int B, int H, int W, int C,
                              int depth, void* stream) {
  using namespace upf;
  UPF_REQUIRE(img && out && lengths && workspace, UPF_EINVAL, "png_encode: null pointer");
  png::Shape s;
  if (int rc = png::shape_of("png_encode", B, H, W, C, depth, &s)) return rc;
  UPF_REQUIRE(aligned_to(img, depth / 8) && aligned_to(out, 4) && aligned_to(lengths, 4) && aligned_to(workspace, 16), UPF_EALIGN,
              "png_encode: img must be sample-aligned, out and lengths 4-byte, workspace 16-byte aligned");
  const unsigned grid = (unsigned)B * s.nchunks;
  hipLaunchKernelGGL(png::filter_kernel, dim3(grid), dim3(png::NT), 0, (hipStream_t)stream, (const uint8_t*)img, (uint8_t*)workspace,
                     (uint32_t*)out, s);
  if (int rc = check_launch("png_encode (filter)")) return rc;
  hipLaunchKernelGGL(png::code_kernel, dim3((unsigned)B), dim3(png::NT2), 0, (hipStream_t)stream, (uint8_t*)workspace, (uint32_t*)out,
                     lengths, s);
  if (int rc = check_launch("png_encode (code)")) return rc;
  hipLaunchKernelGGL(png::pack_kernel, dim3(grid), dim3(png::NT), 0, (hipStream_t)stream, (const uint8_t*)workspace, (uint32_t*)out,
                     (const int*)lengths, s);
  return check_launch("png_encode (pack)");
}
