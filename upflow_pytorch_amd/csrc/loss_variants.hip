// Non-default loss variants of the unsupervised training step — gfx950, fp32, contiguous NCHW.
//
//   smooth_edge2    network_tools.edge_aware_smoothness_order2 (the reference's model/upflow.py:220-243): second differences of
//                   the flow weighted by exp(-mean_c |image difference at stride 2|), both directions.
//   smooth_delta    network_tools.flow_smooth_delta (model/upflow.py:245-263): mean |first differences|, optionally plus the
//                   four second differences built from the first ones in the reference's order, each with its own mean.
//   ssim           network_tools.weighted_ssim (model/upflow.py:139-195) for c1 = inf, finite c2: nine avg_pool2d calls and
//                   ~25 element-wise passes forward (and their backward) of the reference become one launch each way.
// Conventions of loss.hip: NT threads, every workgroup writes its partial sums (summed in fixed order by the caller), backward
// kernels are gathers (no float atomics), nothing synchronises with the host.  Compiled with -ffp-contract=off.
// The reduction core, sgn, edge_w and the smoothness forward kernel come from loss_common.hpp; the 'charbonnier' and 'L1'
// photometric kinds (upf_pointwise_loss_*) are instantiations of the point-wise kernel pair of loss.hip.
//
// The SSIM second moments are evaluated in the centred form  sigma_x = sum_i w_i (x_i - mu_x)^2 / sum_i w_i  over the nine taps
// of a window (held in LDS), which equals the reference's  wpool(x^2) - mu_x^2  in exact arithmetic because the pooled weights
// (w + eps) / 9 * 1 / (pool(w) + eps) sum to one — without that expression's cancellation (the fp32 torch composition loses
// three to four digits there).  The derivative simplifies the same way: d sigma_y / d y_q = 2 w_q (y_q - mu_y) / sum w,
// d sigma_xy / d y_q = w_q (x_q - mu_x) / sum w  (the terms through mu vanish since sum_i w_i (y_i - mu_y) = 0).
#include "loss_common.hpp"

namespace upf {
namespace lossv {

using namespace loss;                             // NT, red_blocks, sgn, edge_w, dd, smooth_fwd_kernel (loss_common.hpp)
constexpr int TW = 32, TH = 8;                     // SSIM tile (TW * TH == NT)

// ---- second-order edge-aware smoothness ---------------------------------------------------------------------------------
// forward: smooth_fwd_kernel<2> (loss_common.hpp), shared with the first-order form of loss.hip
// gather: pixel (i,j) enters the row terms that start at i, i-1, i-2 with coefficients 1, -2, 1 (columns likewise)
__global__ __launch_bounds__(NT)
void smooth2_bwd_kernel(const float* __restrict__ img, const float* __restrict__ pred, const float* __restrict__ gup,
                        float* __restrict__ gpred, int Ci, int Cp, int H, int W, long long npix, float inv_nx, float inv_ny) {
  const long long p = blockIdx.x * (long long)NT + threadIdx.x;
  if (p >= npix) return;
  const int HW = H * W;
  const long long n = p / HW;
  const int q = (int)(p - n * HW), i = q / W, j = q - i * W;
  const float* im = img + (size_t)n * Ci * HW;
  const float* pr = pred + (size_t)n * Cp * HW;
  const float cx = gup[0] * inv_nx, cy = gup[0] * inv_ny;
  const float coef[3] = {1.0f, -2.0f, 1.0f};
  float wr[3], wc[3];
  bool vr[3], vc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {                       // term starting k rows above / k columns left of this pixel
    vr[k] = (i - k >= 0) && (i - k + 2 < H);
    vc[k] = (j - k >= 0) && (j - k + 2 < W);
    wr[k] = vr[k] ? edge_w(im, Ci, HW, q - k * W, q - k * W + 2 * W) : 0.f;
    wc[k] = vc[k] ? edge_w(im, Ci, HW, q - k, q - k + 2) : 0.f;
  }
  for (int c = 0; c < Cp; ++c) {
    const float* pc = pr + (size_t)c * HW;
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (vr[k]) g += coef[k] * (cx * wr[k] * sgn(dd(pc, q - k * W, W)));
      if (vc[k]) g += coef[k] * (cy * wc[k] * sgn(dd(pc, q - k, 1)));
    }
    gpred[((size_t)n * Cp + c) * HW + q] = g;
  }
}

// ---- delta smoothness ---------------------------------------------------------------------------------------------------
// One [H,W] plane; callers guarantee that every index read is in range.
struct Plane {
  const float* f; int W;
  __device__ __forceinline__ float dx(int i, int j) const { return f[i * W + j + 1] - f[i * W + j]; }       // j < W-1
  __device__ __forceinline__ float dy(int i, int j) const { return f[(i + 1) * W + j] - f[i * W + j]; }     // i < H-1
  __device__ __forceinline__ float dx2(int i, int j) const { return dx(i, j + 1) - dx(i, j); }              // j < W-2
  __device__ __forceinline__ float dxdy(int i, int j) const { return dx(i + 1, j) - dx(i, j); }             // i < H-1, j < W-1
  __device__ __forceinline__ float dydx(int i, int j) const { return dy(i, j + 1) - dy(i, j); }             // i < H-1, j < W-1
  __device__ __forceinline__ float dy2(int i, int j) const { return dy(i + 1, j) - dy(i, j); }              // i < H-2
};

// partials[block][k] (k = 2 or 6) = sums of |dx|, |dy| [, |dx2|, |dxdy|, |dydx|, |dy2|] over the block's elements
__global__ __launch_bounds__(NT)
void delta_fwd_kernel(const float* __restrict__ flow, float* __restrict__ partials, int H, int W, long long total, int second) {
  __shared__ float sh[NT / 64];
  const int HW = H * W;
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
    const long long n = e / HW;
    const int q = (int)(e - n * HW), i = q / W, j = q - i * W;
    const Plane P = {flow + (size_t)n * HW, W};
    if (j + 1 < W) s[0] += fabsf(P.dx(i, j));
    if (i + 1 < H) s[1] += fabsf(P.dy(i, j));
    if (second) {
      if (j + 2 < W) s[2] += fabsf(P.dx2(i, j));
      if (i + 1 < H && j + 1 < W) { s[3] += fabsf(P.dxdy(i, j)); s[4] += fabsf(P.dydx(i, j)); }
      if (i + 2 < H) s[5] += fabsf(P.dy2(i, j));
    }
  }
  const int k = second ? 6 : 2;
  for (int t = 0; t < k; ++t) {
    const float a = block_sum<NT>(s[t], sh);
    if (threadIdx.x == 0) partials[(size_t)k * blockIdx.x + t] = a;
  }
}

struct DeltaInv { float v[6]; };                  // 1 / element count of each term

__global__ __launch_bounds__(NT)
void delta_bwd_kernel(const float* __restrict__ flow, const float* __restrict__ gup, float* __restrict__ gflow,
                      int H, int W, long long total, int second, DeltaInv inv) {
  const long long e = blockIdx.x * (long long)NT + threadIdx.x;
  if (e >= total) return;
  const int HW = H * W;
  const long long n = e / HW;
  const int q = (int)(e - n * HW), i = q / W, j = q - i * W;
  const Plane P = {flow + (size_t)n * HW, W};
  const float u = gup[0];
  float g = 0.f;
  {
    const float c0 = u * inv.v[0], c1 = u * inv.v[1];
    if (j + 1 < W) g -= c0 * sgn(P.dx(i, j));
    if (j > 0) g += c0 * sgn(P.dx(i, j - 1));
    if (i + 1 < H) g -= c1 * sgn(P.dy(i, j));
    if (i > 0) g += c1 * sgn(P.dy(i - 1, j));
  }
  if (second) {
    const float c2 = u * inv.v[2], c3 = u * inv.v[3], c4 = u * inv.v[4], c5 = u * inv.v[5];
    // dx2(i,j) = (f(j+2) - f(j+1)) - (f(j+1) - f(j)): coefficients 1, -2, 1 on f(j), f(j+1), f(j+2)
    if (j + 2 < W) g += c2 * sgn(P.dx2(i, j));
    if (j >= 1 && j + 1 < W) g -= 2.0f * (c2 * sgn(P.dx2(i, j - 1)));
    if (j >= 2) g += c2 * sgn(P.dx2(i, j - 2));
    if (i + 2 < H) g += c5 * sgn(P.dy2(i, j));
    if (i >= 1 && i + 1 < H) g -= 2.0f * (c5 * sgn(P.dy2(i - 1, j)));
    if (i >= 2) g += c5 * sgn(P.dy2(i - 2, j));
    // the mixed terms at (a,b) touch f(a,b), f(a,b+1), f(a+1,b), f(a+1,b+1) with coefficients +1, -1, -1, +1
    const bool dn = i + 1 < H, up = i >= 1, rt = j + 1 < W, lf = j >= 1;
    if (dn && rt) g += c3 * sgn(P.dxdy(i, j)) + c4 * sgn(P.dydx(i, j));
    if (dn && lf) g -= c3 * sgn(P.dxdy(i, j - 1)) + c4 * sgn(P.dydx(i, j - 1));
    if (up && rt) g -= c3 * sgn(P.dxdy(i - 1, j)) + c4 * sgn(P.dydx(i - 1, j));
    if (up && lf) g += c3 * sgn(P.dxdy(i - 1, j - 1)) + c4 * sgn(P.dydx(i - 1, j - 1));
  }
  gflow[e] = g;
}

// ---- weighted SSIM (c1 = inf) -------------------------------------------------------------------------------------------
struct Tile { long long n; int oy, ox; };
__device__ __forceinline__ Tile tile_of(long long t, int tiles_x, int tiles_y) {
  Tile r;
  const long long per = (long long)tiles_x * tiles_y;
  r.n = t / per;
  const int k = (int)(t - r.n * per);
  r.oy = (k / tiles_x) * TH;
  r.ox = (k % tiles_x) * TW;
  return r;
}

constexpr int FW = TW + 2, FH = TH + 2;            // forward: input tile of a TW x TH tile of windows
// window statistics from nine taps of an LDS tile of row pitch `pitch` whose top-left tap is at `o`
struct Win { float mux, muy, sx, sy, sxy; };
__device__ __forceinline__ Win window_stats(const float* sW, const float* sX, const float* sY, int o, int pitch, float eps, float r) {
  float ax = 0.f, ay = 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int k = o + dy * pitch + dx;
      const float we = sW[k] + eps;
      ax += we * sX[k];
      ay += we * sY[k];
    }
  Win w;
  w.mux = ax * r;
  w.muy = ay * r;
  float vx = 0.f, vy = 0.f, vxy = 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int k = o + dy * pitch + dx;
      const float we = sW[k] + eps;
      const float cx = sX[k] - w.mux, cy = sY[k] - w.muy;
      vx += we * (cx * cx);
      vy += we * (cy * cy);
      vxy += we * (cx * cy);
    }
  w.sx = vx * r;
  w.sy = vy * r;
  w.sxy = vxy * r;
  return w;
}
// sum of the raw weights and of (w + eps) over a window
__device__ __forceinline__ void window_weight(const float* sW, int o, int pitch, float eps, float& sum_w, float& sum_we) {
  float a = 0.f, b = 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float w = sW[o + dy * pitch + dx];
      a += w;
      b += w + eps;
    }
  sum_w = a;
  sum_we = b;
}

// map [B,C,H-2,W-2], w_avg [B,1,H-2,W-2] and partials[block] = { sum loss * w_avg, sum w_avg, sum loss } — each optional
__global__ __launch_bounds__(NT)
void ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ wgt,
                     float* __restrict__ map, float* __restrict__ wavg_out, float* __restrict__ partials,
                     int C, int H, int W, int tiles_x, int tiles_y, long long ntiles, float c2, float eps) {
  __shared__ float sW[FW * FH], sX[FW * FH], sY[FW * FH];
  __shared__ float sh[NT / 64];
  const int OH = H - 2, OW = W - 2;
  const size_t HW = (size_t)H * W, OHW = (size_t)OH * OW;
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  float s_lw = 0.f, s_w = 0.f, s_l = 0.f;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const Tile T = tile_of(t, tiles_x, tiles_y);
    __syncthreads();                                   // (the previous tile's readers are done)
    for (int k = threadIdx.x; k < FW * FH; k += NT) {
      const int iy = T.oy + k / FW, ix = T.ox + k % FW;
      sW[k] = (iy < H && ix < W) ? wgt[(size_t)T.n * HW + (size_t)iy * W + ix] : 0.f;
    }
    __syncthreads();
    const int py = T.oy + ty, px = T.ox + tx;
    const bool valid = py < OH && px < OW;
    const int o = ty * FW + tx;
    float sum_w, sum_we;
    window_weight(sW, o, FW, eps, sum_w, sum_we);
    const float wavg = sum_w / 9.0f, r = 1.0f / sum_we;
    if (valid) {
      s_w += wavg;
      if (wavg_out) wavg_out[(size_t)T.n * OHW + (size_t)py * OW + px] = wavg;
    }
    for (int c = 0; c < C; ++c) {
      if (c) __syncthreads();
      const float* xc = x + ((size_t)T.n * C + c) * HW;
      const float* yc = y + ((size_t)T.n * C + c) * HW;
      for (int k = threadIdx.x; k < FW * FH; k += NT) {
        const int iy = T.oy + k / FW, ix = T.ox + k % FW;
        const bool in = iy < H && ix < W;
        sX[k] = in ? xc[(size_t)iy * W + ix] : 0.f;
        sY[k] = in ? yc[(size_t)iy * W + ix] : 0.f;
      }
      __syncthreads();
      if (valid) {
        const Win w = window_stats(sW, sX, sY, o, FW, eps, r);
        const float num = 2.0f * w.sxy + c2, den = (w.sx + w.sy) + c2;
        const float v = (1.0f - num / den) / 2.0f;
        const float l = fminf(fmaxf(v, 0.f), 1.0f);
        if (map) map[((size_t)T.n * C + c) * OHW + (size_t)py * OW + px] = l;
        s_lw += l * wavg;
        s_l += l;
      }
    }
  }
  if (partials) {
    const float a = block_sum<NT>(s_lw, sh), b = block_sum<NT>(s_w, sh), c = block_sum<NT>(s_l, sh);
    if (threadIdx.x == 0) { partials[3 * (size_t)blockIdx.x] = a; partials[3 * (size_t)blockIdx.x + 1] = b; partials[3 * (size_t)blockIdx.x + 2] = c; }
  }
}

constexpr int BW = TW + 4, BH = TH + 4;            // backward: input tile of a TW x TH tile of pixels
constexpr int CW = TW + 2, CH = TH + 2;            //           the windows that contain one of those pixels
// upstream gradient of window p, channel c:  grad_map[p,c] (if given) + coef_w[0] * w_avg(p) (if given) + coef_u[0] (if given).
// One launch: the window coefficients of the tile plus its one-window halo are computed once into LDS, then gathered.
__global__ __launch_bounds__(NT)
void ssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ wgt,
                     const float* __restrict__ gmap, const float* __restrict__ coef_w, const float* __restrict__ coef_u,
                     float* __restrict__ gx, float* __restrict__ gy,
                     int C, int H, int W, int tiles_x, int tiles_y, long long ntiles, float c2, float eps) {
  __shared__ float sW[BW * BH], sX[BW * BH], sY[BW * BH];
  __shared__ float sR[CW * CH], sA[CW * CH], sP[CW * CH], sQ[CW * CH], sMx[CW * CH], sMy[CW * CH];
  const int OH = H - 2, OW = W - 2;
  const size_t HW = (size_t)H * W, OHW = (size_t)OH * OW;
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  const float cw = coef_w ? coef_w[0] : 0.f, cu = coef_u ? coef_u[0] : 0.f;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const Tile T = tile_of(t, tiles_x, tiles_y);
    const int y0 = T.oy - 2, x0 = T.ox - 2;             // top-left input pixel of the staged tile = top-left window
    __syncthreads();
    for (int k = threadIdx.x; k < BW * BH; k += NT) {
      const int iy = y0 + k / BW, ix = x0 + k % BW;
      sW[k] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? wgt[(size_t)T.n * HW + (size_t)iy * W + ix] : 0.f;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < CW * CH; k += NT) {
      const int wy = k / CW, wx = k % CW;
      const int py = y0 + wy, px = x0 + wx;
      float r = 0.f, a = 0.f;
      if (py >= 0 && py < OH && px >= 0 && px < OW) {
        float sum_w, sum_we;
        window_weight(sW, wy * BW + wx, BW, eps, sum_w, sum_we);
        a = sum_w / 9.0f;
        r = 1.0f / sum_we;
      }
      sR[k] = r;                                          // 0: no such window
      sA[k] = a;
    }
    for (int c = 0; c < C; ++c) {
      __syncthreads();                                   // (sR / sA written; the previous channel's gather is done)
      const float* xc = x + ((size_t)T.n * C + c) * HW;
      const float* yc = y + ((size_t)T.n * C + c) * HW;
      for (int k = threadIdx.x; k < BW * BH; k += NT) {
        const int iy = y0 + k / BW, ix = x0 + k % BW;
        const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
        sX[k] = in ? xc[(size_t)iy * W + ix] : 0.f;
        sY[k] = in ? yc[(size_t)iy * W + ix] : 0.f;
      }
      __syncthreads();
      for (int k = threadIdx.x; k < CW * CH; k += NT) {
        const int wy = k / CW, wx = k % CW;
        const float r = sR[k];
        float P = 0.f, Q = 0.f, mx = 0.f, my = 0.f;
        if (r != 0.f) {
          const int py = y0 + wy, px = x0 + wx;
          const Win w = window_stats(sW, sX, sY, wy * BW + wx, BW, eps, r);
          const float num = 2.0f * w.sxy + c2, den = (w.sx + w.sy) + c2;
          const float v = (1.0f - num / den) / 2.0f;
          float g = cw * sA[k] + cu;
          if (gmap) g += gmap[((size_t)T.n * C + c) * OHW + (size_t)py * OW + px];
          if (!(v >= 0.f && v <= 1.0f)) g = 0.f;          // clamp(., 0, 1) passes the gradient on [0, 1] inclusive
          const float gr = g * r;
          P = -(gr / den);                                 // d loss / d sigma_xy        * g / sum(w + eps)
          Q = gr * (num / (den * den));                    // 2 d loss / d sigma_{x,y}   * g / sum(w + eps)
          mx = w.mux;
          my = w.muy;
        }
        sP[k] = P; sQ[k] = Q; sMx[k] = mx; sMy[k] = my;
      }
      __syncthreads();
      const int qy = T.oy + ty, qx = T.ox + tx;
      if (qy < H && qx < W) {
        const int ki = (ty + 2) * BW + (tx + 2);
        const float xq = sX[ki], yq = sY[ki], we = sW[ki] + eps;
        float ax = 0.f, ay = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int k = (ty + dy) * CW + (tx + dx);    // windows whose top-left is 2-dy rows / 2-dx columns before the pixel
            const float ex = xq - sMx[k], ey = yq - sMy[k];
            ay += sP[k] * ex + sQ[k] * ey;
            ax += sP[k] * ey + sQ[k] * ex;
          }
        const size_t e = ((size_t)T.n * C + c) * HW + (size_t)qy * W + qx;
        if (gy) gy[e] = we * ay;
        if (gx) gx[e] = we * ax;
      }
    }
  }
}

static int tile_grid(long long ntiles) { return (int)(ntiles < 1 ? 1 : (ntiles > (1ll << 20) ? (1ll << 20) : ntiles)); }

}  // namespace lossv
}  // namespace upf

extern "C" int upf_smooth_edge2_forward(const float* img, const float* pred, float* partials,
                                        int B, int Ci, int Cp, int H, int W, void* stream) {
  using namespace upf;
  UPF_REQUIRE(img && pred && partials, UPF_EINVAL, "smooth_edge2_forward: null pointer");
  UPF_REQUIRE(B > 0 && Ci > 0 && Cp > 0 && H >= 3 && W >= 3 && (long long)H * W < (1ll << 31), UPF_EINVAL, "smooth_edge2_forward: bad shape");
  const long long npix = (long long)B * H * W;
  hipLaunchKernelGGL(lossv::smooth_fwd_kernel<2>, dim3(lossv::red_blocks(npix)), dim3(lossv::NT), 0, (hipStream_t)stream,
                     img, pred, partials, Ci, Cp, H, W, npix);
  return check_launch("smooth_edge2_forward");
}

extern "C" int upf_smooth_edge2_backward(const float* img, const float* pred, const float* grad_up, float* grad_pred,
                                         int B, int Ci, int Cp, int H, int W, void* stream) {
  using namespace upf;
  UPF_REQUIRE(img && pred && grad_up && grad_pred, UPF_EINVAL, "smooth_edge2_backward: null pointer");
  UPF_REQUIRE(B > 0 && Ci > 0 && Cp > 0 && H >= 3 && W >= 3 && (long long)H * W < (1ll << 31), UPF_EINVAL, "smooth_edge2_backward: bad shape");
  const long long npix = (long long)B * H * W;
  UPF_REQUIRE((npix + lossv::NT - 1) / lossv::NT < (1ll << 31), UPF_EINVAL, "smooth_edge2_backward: grid too large");
  const float inv_nx = (float)(1.0 / ((double)B * Cp * (H - 2) * W)), inv_ny = (float)(1.0 / ((double)B * Cp * H * (W - 2)));
  hipLaunchKernelGGL(lossv::smooth2_bwd_kernel, dim3((unsigned)((npix + lossv::NT - 1) / lossv::NT)), dim3(lossv::NT), 0, (hipStream_t)stream,
                     img, pred, grad_up, grad_pred, Ci, Cp, H, W, npix, inv_nx, inv_ny);
  return check_launch("smooth_edge2_backward");
}

extern "C" int upf_smooth_delta_forward(const float* flow, float* partials, int BC, int H, int W, int second_order, void* stream) {
  using namespace upf;
  const int m = second_order ? 3 : 2;
  UPF_REQUIRE(flow && partials, UPF_EINVAL, "smooth_delta_forward: null pointer");
  UPF_REQUIRE(BC > 0 && H >= m && W >= m && (long long)H * W < (1ll << 31), UPF_EINVAL, "smooth_delta_forward: bad shape");
  const long long total = (long long)BC * H * W;
  hipLaunchKernelGGL(lossv::delta_fwd_kernel, dim3(lossv::red_blocks(total)), dim3(lossv::NT), 0, (hipStream_t)stream,
                     flow, partials, H, W, total, second_order ? 1 : 0);
  return check_launch("smooth_delta_forward");
}

extern "C" int upf_smooth_delta_backward(const float* flow, const float* grad_up, float* grad_flow, int BC, int H, int W,
                                         int second_order, void* stream) {
  using namespace upf;
  const int m = second_order ? 3 : 2;
  UPF_REQUIRE(flow && grad_up && grad_flow, UPF_EINVAL, "smooth_delta_backward: null pointer");
  UPF_REQUIRE(BC > 0 && H >= m && W >= m && (long long)H * W < (1ll << 31), UPF_EINVAL, "smooth_delta_backward: bad shape");
  const long long total = (long long)BC * H * W;
  UPF_REQUIRE((total + lossv::NT - 1) / lossv::NT < (1ll << 31), UPF_EINVAL, "smooth_delta_backward: grid too large");
  lossv::DeltaInv inv;
  const double n = (double)BC;
  inv.v[0] = (float)(1.0 / (n * H * (W - 1)));
  inv.v[1] = (float)(1.0 / (n * (H - 1) * W));
  inv.v[2] = second_order ? (float)(1.0 / (n * H * (W - 2))) : 0.f;
  inv.v[3] = inv.v[4] = second_order ? (float)(1.0 / (n * (H - 1) * (W - 1))) : 0.f;
  inv.v[5] = second_order ? (float)(1.0 / (n * (H - 2) * W)) : 0.f;
  hipLaunchKernelGGL(lossv::delta_bwd_kernel, dim3((unsigned)((total + lossv::NT - 1) / lossv::NT)), dim3(lossv::NT), 0, (hipStream_t)stream,
                     flow, grad_up, grad_flow, H, W, total, second_order ? 1 : 0, inv);
  return check_launch("smooth_delta_backward");
}

extern "C" int upf_ssim_forward(const float* x, const float* y, const float* weight, float* map, float* w_avg, float* partials,
                                int B, int C, int H, int W, float c2, float weight_epsilon, void* stream) {
  using namespace upf;
  UPF_REQUIRE(x && y && weight && (map || w_avg || partials), UPF_EINVAL, "ssim_forward: null pointer");
  UPF_REQUIRE(B > 0 && C > 0 && H >= 3 && W >= 3 && (long long)H * W < (1ll << 31), UPF_EINVAL, "ssim_forward: bad shape");
  UPF_REQUIRE(c2 > 0.f && c2 < INFINITY && weight_epsilon > 0.f, UPF_EINVAL, "ssim_forward: c2 and weight_epsilon must be positive and finite");
  const int tiles_x = cdiv(W - 2, lossv::TW), tiles_y = cdiv(H - 2, lossv::TH);
  const long long ntiles = (long long)B * tiles_x * tiles_y;
  // with partials the grid is upf_loss_partials(B*(H-2)*(W-2)) workgroups (the caller sized the buffer by it)
  const int grid = partials ? lossv::red_blocks((long long)B * (H - 2) * (W - 2)) : lossv::tile_grid(ntiles);
  hipLaunchKernelGGL(lossv::ssim_fwd_kernel, dim3(grid), dim3(lossv::NT), 0, (hipStream_t)stream,
                     x, y, weight, map, w_avg, partials, C, H, W, tiles_x, tiles_y, ntiles, c2, weight_epsilon);
  return check_launch("ssim_forward");
}

extern "C" int upf_ssim_backward(const float* x, const float* y, const float* weight, const float* grad_map,
                                 const float* coef_w, const float* coef_u, float* grad_x, float* grad_y,
                                 int B, int C, int H, int W, float c2, float weight_epsilon, void* stream) {
  using namespace upf;
  UPF_REQUIRE(x && y && weight && (grad_map || coef_w || coef_u) && (grad_x || grad_y), UPF_EINVAL, "ssim_backward: null pointer");
  UPF_REQUIRE(B > 0 && C > 0 && H >= 3 && W >= 3 && (long long)H * W < (1ll << 31), UPF_EINVAL, "ssim_backward: bad shape");
  UPF_REQUIRE(c2 > 0.f && c2 < INFINITY && weight_epsilon > 0.f, UPF_EINVAL, "ssim_backward: c2 and weight_epsilon must be positive and finite");
  const int tiles_x = cdiv(W, lossv::TW), tiles_y = cdiv(H, lossv::TH);
  const long long ntiles = (long long)B * tiles_x * tiles_y;
  hipLaunchKernelGGL(lossv::ssim_bwd_kernel, dim3(lossv::tile_grid(ntiles)), dim3(lossv::NT), 0, (hipStream_t)stream,
                     x, y, weight, grad_map, coef_w, coef_u, grad_x, grad_y, C, H, W, tiles_x, tiles_y, ntiles, c2, weight_epsilon);
  return check_launch("ssim_backward");
}
