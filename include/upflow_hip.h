/*
 * upflow_hip.h — C-ABI of libupflow_hip.so: the MI355X (gfx950) native operators of the UPFlow
 * hot path.  Plain pointers, sizes and a HIP stream; no torch types.
 *
 * This is the drop-in boundary.  The reference crosses Python -> native exactly once on this path,
 * through the pybind11 module `correlation_cuda`
 *     /root/reference/model/correlation_package/correlation_cuda.cc:169-172
 *         forward (input1,input2,rInput1,rInput2,output, pad,k,max_disp,s1,s2,mult)      :10-87
 *         backward(input1,input2,rInput1,rInput2,gradOutput,gradInput1,gradInput2, ...)  :89-167
 * and reaches ATen's native grid_sample / interpolate kernels at
 *     model/pwc_modules.py:79,200,205   utils/tools.py:1304   model/upflow.py:79-88.
 * Each entry point below names the reference interface it replaces.  The reference-side binding
 * a maintainer would add is in INTEGRATION.md; ours is upflow_pytorch_amd/_lib.py (ctypes).
 *
 * Conventions (all entry points)
 *   - device pointers, tensors are contiguous NCHW (the reference kernels assume that too,
 *     correlation_cuda_kernel.cu:15-39 ignores the strides it is handed);
 *   - `dtype` selects the element type of feature-like tensors: UPF_F32 / UPF_F16 / UPF_BF16;
 *     flows, sampling positions, masks and every accumulator are always fp32;
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); calls only enqueue work, they
 *     never synchronise, allocate or free, so they can be captured into a hipGraph;
 *   - return value: 0 (UPF_OK) on success, a negative UPF_E* code on a rejected argument, a
 *     positive hipError_t if the launch failed; upf_last_error() gives the message of the last
 *     failure on the calling thread (the reference printf()s and returns 0,
 *     correlation_cuda_kernel.cu:383-392, which its .cc turns into AT_ERROR, :81-83);
 *   - threading: like the reference's FFI (called with the GIL held, one process per GPU) the library expects
 *     one calling thread per device at a time; its only process-wide state is launch bookkeeping (kernel
 *     attributes set on first use, the heuristics of upf_conv_set_option) — no allocations, no caches of data.
 */
#ifndef UPFLOW_HIP_H
#define UPFLOW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

enum { UPF_F32 = 0, UPF_F16 = 1, UPF_BF16 = 2 };
enum { UPF_OK = 0, UPF_EINVAL = -1, UPF_EDTYPE = -2, UPF_EALIGN = -3, UPF_EUNSUPPORTED = -4 };
enum { UPF_MASK_NONE = 0, UPF_MASK_LITERAL = 1, UPF_MASK_ROBUST = 2 };

/* library identity: "upflow_hip <version> gfx950" */
const char* upf_version(void);
const char* upf_last_error(void);

/* ---- cost volume ------------------------------------------------------------------------------
 * 81-neighbour correlation, (pad,k,max_disp,s1,s2) = (4,1,4,1,1), the only configuration the model
 * instantiates (model/upflow.py:561-562):
 *     out[n, 9*(dy+4)+(dx+4), y, x] = (1/C) * sum_c f1[n,c,y,x] * f2[n,c,y+dy,x+dx]   (f2 = 0 outside)
 * Replaces correlation_cuda.forward (correlation_cuda.cc:10-87 -> correlation_cuda_kernel.cu:302-393:
 * 2x channels_first + correlation_forward) without the padded-NHWC staging copies.
 *   f1,f2 : [B,C,H,W] of `dtype`;  out : [B,81,H,W] of `dtype`, batch stride `out_batch_stride`
 *   elements (0 = 81*H*W) so the volume can be written straight into the first 81 channels of the
 *   115-channel estimator input (model/upflow.py:565).
 *   leaky_slope != 0 fuses LeakyReLU(slope) (model/upflow.py:563-564); 0 = plain correlation.
 * fp32 accumulation for every dtype.  The scale: 16-bit outputs round fp32(sum * fp32(1/C)) once (after the LeakyReLU); an fp32
 * output is the correctly rounded sum / C.  A non-finite sum gives the Inf / NaN the division would (in fp32 too).
 */
int upf_corr81_forward(const void* f1, const void* f2, void* out,
                       int B, int C, int H, int W, int dtype,
                       long long out_batch_stride, float leaky_slope, void* stream);

/* Measurement helper (bench.py's `roofline` object): `nrep` back-to-back launches of the kernel above,
 * each bracketed by its own pair of HIP events recorded on `stream` right around the kernel
 * (hipExtLaunchKernel start/stop events); synchronises the stream and returns the average and the
 * minimum kernel duration in microseconds.  Not capturable (it synchronises). */
int upf_corr81_forward_timed(const void* f1, const void* f2, void* out,
                             int B, int C, int H, int W, int dtype,
                             long long out_batch_stride, float leaky_slope, void* stream,
                             int nrep, float* avg_us, float* min_us);

/* Feature normalisation fused into the cost volume (model/upflow.py:549-562):
 *     out = corr81(normalize(f1), normalize(f2))        normalize = upf_normalize_forward's arithmetic, per tensor
 * in TWO launches — one statistics pass over both tensors, then the cost volume whose loader normalises every element
 * (and re-rounds it to `dtype`) on its way into LDS — instead of four, and without writing / re-reading the two
 * normalised feature maps.  Bit-identical to upf_normalize_forward x2 + upf_corr81_forward.  bf16 / fp16, C <= 208
 * (upf_corr81_norm_supported), W >= 4; `workspace`: upf_corr81_norm_workspace_bytes(B,C,H,W) bytes of device memory. */
int upf_corr81_norm_supported(int C, int dtype);
long long upf_corr81_norm_workspace_bytes(int B, int C, int H, int W);
int upf_corr81_norm_forward(const void* f1, const void* f2, void* out,
                            int B, int C, int H, int W, int dtype,
                            long long out_batch_stride, float leaky_slope, void* workspace, void* stream);
/* The same into channel octets (round 3; the flow estimator's input buffer in the C8 layout of upf_conv_forward_c8):
 * out8 = the first of 11 octets of a [n][octet][H][W][8] buffer, out8_batch_stride its batch stride in elements.
 * Octet j < 9: displacements (dy = j-4, dx = -4..+3) in positions 0..7; octet 9 position p: (dy = p-4, dx = +4);
 * octet 10 position 0: (+4,+4), positions 1..7 zero.  The convolution reading it learns this order through the k-map
 * of upf_conv_pack_weights_kmap.  Values are bit-identical to upf_corr81_norm_forward's.  W % 8 == 0. */
int upf_corr81_norm_forward_c8(const void* f1, const void* f2, void* out8, long long out8_batch_stride,
                               int B, int C, int H, int W, int dtype, float leaky_slope, void* workspace, void* stream);
/* PITCHED feature rows (round 5): the H rows of every channel plane of f1 / f2 are f_row_pitch elements apart (>= W; plane stride
 * H * f_row_pitch, item stride C * H * f_row_pitch; 0 = W, i.e. the contiguous forms above).  With a pitch that is a multiple of 8
 * every row is 16-byte aligned whatever W is, so RAGGED pyramid levels — KITTI's native 375x1242 frames: W = 311, 156, 78, 39, 20,
 * the frame size the reference's evaluation feeds (test.py:40-47, dataset/kitti_dataset.py:609-631) — keep the aligned loads and,
 * for the octet form, any W >= 4 is accepted (one 16-byte entry per pixel: the output is aligned for every W).  Nothing depends on
 * what the pitch padding holds (the loader masks it; the statistics skip it); results are bit-identical to the contiguous forms. */
int upf_corr81_norm_forward_pitched(const void* f1, const void* f2, int f_row_pitch, void* out,
                                    int B, int C, int H, int W, int dtype,
                                    long long out_batch_stride, float leaky_slope, void* workspace, void* stream);
int upf_corr81_norm_forward_c8_pitched(const void* f1, const void* f2, int f_row_pitch, void* out8, long long out8_batch_stride,
                                       int B, int C, int H, int W, int dtype, float leaky_slope, void* workspace, void* stream);
/* MIXED storage types (round 5, the `pyramid_dtype` option: fp16 pyramid features, bf16 decoder buffers): the features are `dtype`,
 * the cost volume is rounded ONCE from its fp32 sums to `out_dtype` (the other 16-bit type, or the same: the entry points above). */
int upf_corr81_norm_forward_mixed(const void* f1, const void* f2, int f_row_pitch, void* out,
                                  int B, int C, int H, int W, int dtype, int out_dtype,
                                  long long out_batch_stride, float leaky_slope, void* workspace, void* stream);
int upf_corr81_norm_forward_c8_mixed(const void* f1, const void* f2, int f_row_pitch, void* out8, long long out8_batch_stride,
                                     int B, int C, int H, int W, int dtype, int out_dtype, float leaky_slope, void* workspace, void* stream);
/* measurement helper (bench.py): one statistics launch, then nrep launches of the normalising cost volume, each between
 * its own pair of HIP events on `stream` — the kernel that runs inside the inference step */
int upf_corr81_norm_forward_timed(const void* f1, const void* f2, void* out,
                                  int B, int C, int H, int W, int dtype,
                                  long long out_batch_stride, float leaky_slope, void* workspace, void* stream,
                                  int nrep, float* avg_us, float* min_us);
/* ... and of upf_corr81_norm_forward_c8 (the form the step launches at the levels whose estimator runs on octets) */
int upf_corr81_norm_forward_c8_timed(const void* f1, const void* f2, void* out8, long long out8_batch_stride,
                                     int B, int C, int H, int W, int dtype, float leaky_slope, void* workspace, void* stream,
                                     int nrep, float* avg_us, float* min_us);

int upf_corr81_norm_forward_c8_timed_pitched(const void* f1, const void* f2, int f_row_pitch, void* out8, long long out8_batch_stride,
                                             int B, int C, int H, int W, int dtype, float leaky_slope, void* workspace, void* stream,
                                             int nrep, float* avg_us, float* min_us);

/* ... with the output's storage type given separately (upf_corr81_norm_forward_c8_mixed: fp16 features -> bf16 octets, what the
 * bf16 step launches since its feature pyramid stays fp16 — UPFlow_net.to_inference, round 6) */
int upf_corr81_norm_forward_c8_timed_mixed(const void* f1, const void* f2, int f_row_pitch, void* out8, long long out8_batch_stride,
                                           int B, int C, int H, int W, int dtype, int out_dtype, float leaky_slope, void* workspace, void* stream,
                                           int nrep, float* avg_us, float* min_us);

/* Launch heuristics of the 16-bit cost volume, for tuning and for the tests to reach every kernel variant:
 *   "variant"  (-1)  -1 = choose by shape; 0..3 = force tile geometry 8x32 / 4x32 / 2x32 / 4x16 where C fits
 *   "old_path" (0)   1 = the channel-chunked kernels (corr81_mfma_kernel / corr81_fwd_kernel) instead of the
 *                    all-channels-in-LDS kernel
 * returns the previous value, or -1000 for an unknown name. */
int upf_corr_set_option(const char* name, int value);

/* Gradients of the above (correlation_cuda.backward, correlation_cuda.cc:89-167 ->
 * correlation_cuda_kernel.cu:116-300, 396-530):
 *   g1[n,c,y,x] = (1/C) sum_d gO[n,d,y,x]       * f2[n,c,y+dy,x+dx]
 *   g2[n,c,y,x] = (1/C) sum_d gO[n,d,y-dy,x-dx] * f1[n,c,y-dy,x-dx]
 * grad_out : [B,81,H,W] of `dtype` (contiguous);  g1,g2 : [B,C,H,W] of `dtype`.
 * Outside the image f2 = 0, as in the forward: a g1 term whose f2 pixel lies outside is gO times that zero — nothing for a
 * finite gO, NaN for an Inf / NaN one (every kernel, the W < 4 fallback included).  A g2 term whose source pixel (y-dy, x-dx)
 * lies outside does not exist.  The scale is the product with the fp32 reciprocal of C. */
int upf_corr81_backward(const void* f1, const void* f2, const void* grad_out, void* g1, void* g2,
                        int B, int C, int H, int W, int dtype, void* stream);

/* General-parameter cost volume with the reference's full argument list (correlation_cuda.cc:10-17):
 * any pad/kernel/max_displacement/stride1/stride2; output [B,(2*(md/s2)+1)^2,outH,outW] with
 * outH = ceil((H+2*pad-2*((k-1)/2+md))/s1) (correlation_cuda.cc:24-34).  Dispatches to the tuned
 * 81-neighbour kernel for (4,1,4,1,1), otherwise to a plain one-thread-per-output kernel.
 * corr_type_multiply is accepted and unused, as in the reference (correlation_cuda_kernel.cu:302+). */
int upf_correlation_forward(const void* in1, const void* in2, void* out,
                            int B, int C, int H, int W, int dtype,
                            int pad_size, int kernel_size, int max_displacement,
                            int stride1, int stride2, int corr_type_multiply, void* stream);
/* Gradients of upf_correlation_forward (correlation_cuda.backward with the full argument list, correlation_cuda.cc:89-167 ->
 * correlation_cuda_kernel.cu:116-300): the tuned kernels for (4,1,4,1,1); a plain one-thread-per-element kernel for any
 * (pad, md, stride2) with kernel_size 1 and stride1 1 — the parameter sets for which the reference's backward kernels are the
 * gradient of its forward (their block -> pixel map and (ymin, ymax) windows, :129-141, :222-256, are not for stride1 > 1 or
 * kernel_size > 1); UPF_EUNSUPPORTED otherwise.  grad_out [B,(2*(md/s2)+1)^2,outH,outW], g1 / g2 [B,C,H,W], all of `dtype`.
 * upf_correlation_forward itself returns UPF_EUNSUPPORTED where the reference reads outside its padded buffers
 * (kernel_size > 1 with md - (md/s2)*s2 < (k-1)/2: correlation_cuda_kernel.cu:62, :87-91). */
int upf_correlation_backward(const void* in1, const void* in2, const void* grad_out, void* g1, void* g2,
                             int B, int C, int H, int W, int dtype,
                             int pad_size, int kernel_size, int max_displacement,
                             int stride1, int stride2, int corr_type_multiply, void* stream);
/* output geometry of upf_correlation_forward */
int upf_correlation_out_shape(int H, int W, int pad_size, int kernel_size, int max_displacement,
                              int stride1, int stride2, int* out_channels, int* out_h, int* out_w);

/* ---- backward warp ----------------------------------------------------------------------------
 * y[n,c,i,j] = bilinear sample of x[n,c] at (j + flow[n,0,i,j], i + flow[n,1,i,j]), zeros outside,
 * torch-1.1 grid_sample semantics (align_corners=True), times a validity mask:
 *   UPF_MASK_NONE    tools.torch_warp                  utils/tools.py:1274-1319
 *   UPF_MASK_LITERAL WarpingLayer_no_div.forward       model/pwc_modules.py:184-207
 *                    mask = grid_sample(ones) >= 1.0, reproduced bit-exactly: the four weight*tap
 *                    products in fp32, summed ((nw+ne)+sw)+se, no FMA contraction
 *   UPF_MASK_ROBUST  exact in-bounds predicate (non-default; SURVEY.md §7-H2 protocol P3b)
 *   x,y : [B,C,H,W] of `dtype`;  flow : [B,2,H,W] fp32.
 *   batch_shift: output item n samples x[(n + batch_shift) % B] — with both frames of a pair stacked along
 *   the batch ([im1 features; im2 features]) batch_shift = B/2 warps "the other frame" for both flow
 *   directions in one launch, no gather copy.  0 = plain. */
int upf_warp_forward(const void* x, const float* flow, void* y,
                     int B, int C, int H, int W, int dtype, int mask_mode, int batch_shift, void* stream);
/* same, x / y being channel slices of wider contiguous NCHW buffers (batch strides in elements, 0 = C*H*W): the
 * inference path warps straight out of / into the concatenation buffers the convolutions read (no slot copies). */
int upf_warp_forward_strided(const void* x, long long x_batch_stride, const float* flow, void* y, long long y_batch_stride,
                             int B, int C, int H, int W, int dtype, int mask_mode, int batch_shift, void* stream);
/* same with PITCHED rows (round 5): rows of x / y are x_row_pitch / y_row_pitch elements apart (>= W, 0 = W; plane stride H * pitch,
 * batch strides 0 = C * H * pitch); the flow stays a contiguous fp32 tensor.  With an even y pitch odd-width levels keep the 4-byte
 * (two-pixel) stores — the pixel beyond W lands in the row's own padding.  Same values as the contiguous forms.
 * Batch strides: at least C * H * pitch - (pitch - W), i.e. the padding of an image's last row need not exist.  A y_batch_stride of
 * C * H * pitch or more (or 0) PROMISES that every row of every image, the last included, owns its full pitch: only then is
 * column W of an odd-width row written (with an unspecified value); below that nothing outside the [.., :W] view is touched. */
int upf_warp_forward_pitched(const void* x, long long x_batch_stride, int x_row_pitch, const float* flow, void* y, long long y_batch_stride,
                             int y_row_pitch, int B, int C, int H, int W, int dtype, int mask_mode, int batch_shift, void* stream);
/* same on CHANNEL-OCTET tensors ("C8": [n][C/8][H][W][8], see upf_conv_forward_c8; bf16 / fp16): x8 / y8 point at the first
 * octet plane of octet slices of C8 buffers (batch strides in elements), n_oct octets.  Values equal the NCHW kernel's. */
int upf_warp_forward_c8(const void* x8, long long x_batch_stride, const float* flow, void* y8, long long y_batch_stride,
                        int B, int n_oct, int H, int W, int dtype, int mask_mode, int batch_shift, void* stream);
/* Gradients of the warp: gx [B,C,H,W] of `dtype` (wrt x; with batch_shift it lands on the item that was sampled) and
 * gflow [B,2,H,W] fp32.  The scatter into gx is accumulated in 64-bit fixed point (value * 2^44, integer atomics), so the
 * result is bit-reproducible run to run; `workspace`: upf_warp_backward_workspace_bytes(B,C,H,W) bytes of device memory
 * (zero-filled by the call itself).  grad_y : [B,C,H,W] of `dtype`. */
long long upf_warp_backward_workspace_bytes(int B, int C, int H, int W);
int upf_warp_backward(const void* x, const float* flow, const void* grad_y,
                      void* gx, float* gflow, void* workspace,
                      int B, int C, int H, int W, int dtype, int mask_mode, int batch_shift, void* stream);

/* ---- flow up-sampling -------------------------------------------------------------------------
 * upsample2d_flow_as / upsample_flow (model/pwc_modules.py:77-104): bilinear align_corners=True
 * resize [B,C,h,w] -> [B,C,H,W] fp32; with if_rate channel 0 *= W/w and channel 1 *= H/h. */
int upf_flow_upsample_forward(const float* x, float* y, int B, int C, int h, int w, int H, int W,
                              int if_rate, void* stream);
int upf_flow_upsample_backward(const float* grad_y, float* gx, int B, int C, int h, int w, int H, int W,
                               int if_rate, void* stream);

/* ---- SGU interpolation-blend  (model/upflow.py:79-88) -----------------------------------------
 * x_out [B,3,h,w] of `dtype` = (inter_flow_x, inter_flow_y, mask_logit) from the SGU estimator.
 *   inter_flow = x_out[:, :2]; inter_mask = sigmoid(x_out[:, 2])
 *   decoder level (Hf = h, Wf = w):      flow_init [B,2,h,w]
 *   final level   (Hf,Wf = full size):   inter_flow, inter_mask bilinearly up-sampled (align_corners,
 *                                        flow channels * Wf/w, Hf/h), flow_init = output_level_flow
 *   flow_up = torch_warp(flow_init, inter_flow) * (1 - inter_mask) + flow_init * inter_mask
 * flow_init, flow_up : [B,2,Hf,Wf] fp32; inter_flow [B,2,Hf,Wf], inter_mask [B,1,Hf,Wf] fp32 are
 * optional outputs (NULL = do not materialise).  One launch instead of ~8 ATen launches.
 * At the final level the sigmoid of the mask logits is evaluated once per LOW-resolution pixel into `workspace`
 * (upf_sgu_blend_forward_workspace_bytes(B,h,w,Hf,Wf) bytes; 0 / NULL at a decoder level) and interpolated from there. */
long long upf_sgu_blend_forward_workspace_bytes(int B, int h, int w, int Hf, int Wf);
int upf_sgu_blend_forward(const float* flow_init, const void* x_out, float* flow_up,
                          float* inter_flow, float* inter_mask, void* workspace,
                          int B, int h, int w, int Hf, int Wf, int dtype, void* stream);
/* The decoder-level blend (x_out at the flow's own resolution) that ALSO stores the blended flow rounded to x_out's 16-bit type into the
 * flow estimator's input buffer — two NCHW planes [B,2,H,W] (batch stride given) or one octet entry per pixel [u, v, 0 x 6] — which
 * upf_flow_update / upf_flow_update_c8 wrote in a launch of their own (round 6; inference). */
int upf_sgu_blend_forward_flow16(const float* flow_init, const void* x_out, float* flow_up, void* flow16, long long flow16_batch_stride,
                                 int flow16_is_c8, int B, int H, int W, int dtype, void* stream);
/* g_flow_init32 [B,2,Hf,Wf] and g_x_out32 [B,3,h,w] fp32, fully produced by the call.  The scatters accumulate in 64-bit
 * fixed point (bit-reproducible); `workspace`: upf_sgu_blend_backward_workspace_bytes(B,h,w,Hf,Wf) bytes, zero-filled
 * by the call itself on `stream`. */
long long upf_sgu_blend_backward_workspace_bytes(int B, int h, int w, int Hf, int Wf);
int upf_sgu_blend_backward(const float* flow_init, const void* x_out, const float* grad_flow_up,
                           float* g_flow_init32, float* g_x_out32, void* workspace,
                           int B, int h, int w, int Hf, int Wf, int dtype, void* stream);

/* ---- feature normalisation  (network_tools.normalize_features, model/upflow.py:94-137) ---------
 * inference flags of test.py:22-30: per sample, per channel mean and UNBIASED variance over H*W,
 * y = (x - mean) / sqrt(var + 1e-16).  x,y : [N,HW] rows (N = B*C) of `dtype`;
 * mean, rstd : [N] fp32 optional outputs (saved for backward).  Rows are split over several workgroups
 * (two launches, deterministic merge): `workspace` must hold upf_normalize_workspace_bytes(N, HW) bytes. */
long long upf_normalize_workspace_bytes(long long N, int HW);
int upf_normalize_forward(const void* x, void* y, float* mean, float* rstd, void* workspace,
                          long long N, int HW, int dtype, void* stream);
int upf_normalize_backward(const void* y, const void* grad_y, const float* rstd, void* gx,
                           long long N, int HW, int dtype, void* stream);

/* ---- convolution on the matrix cores   -------------------------------------
 * The dense flow-estimator / context / SGU-estimator / pyramid convolutions (model/pwc_modules.py:122-142,
 * :250-286, :396-412; model/upflow.py:24-60, :349-353), bf16 / fp16 only (fp32 stays with MIOpen = the
 * parity mode), kernel_size 3 (dilation d <= 16, padding d; stride 1, or 2 with d = 1) or 1 (stride 1):
 *   y[n,co,i,j] = act(bias[co] + sum_{ci,ky,kx} w[co,ci,ky,kx] * x[n,ci, s*i+(ky-1)d, s*j+(kx-1)d])
 * output (H-1)/s+1 x (W-1)/s+1.  x / y point at the FIRST input / output channel of channel slices of larger
 * contiguous NCHW buffers (batch strides in elements), so the estimator's growing concatenation needs no
 * copies.  w_packed: upf_conv_pack_weights() output (MFMA lane order, zero padded to pad32(Cout) x pad32(Cin),
 * done once per layer).  Any Cout; any W >= 8 (rows that are not 16-byte aligned take a slightly slower
 * staging path); Cin*H*W*2 < 2^31.
 * upf_conv_set_option: launch heuristics, for tuning and for the tests to reach every kernel variant:
 *   "sk_grid"    (48)  grids of at most this many 8x32 pixel tiles use the split-K kernel (0 = never);
 *   "sk_grid_narrow" (96) the same bound for layers with Cout <= 64;  "sk_grid_d4" (16) for dilation 4
 *   "small_grid" (256) at most this many tiles: narrower workgroups, output channels over blockIdx.y
 *   "rpw4_min"   (256) at least this many 16x32 tiles: Cout <= 32 layers use 16-row tiles
 *   "ph_fit"     (1)   dilated layers: tile height (8 / 6 / 4 rows) fitted to the rows of a row phase (0 = always 8)
 *   "force_mtw"  (0)   experiments: 1 / 2 / 4 output-channel blocks per workgroup whatever the grid (0 = heuristic)
 *   "force_sk"   (-1)  experiments: 0 = never the split-K kernel, 1 = wherever it applies (-1 = heuristic)
 *   "ablate"     (0)   experiments: bit mask — 1 no matrix phase, 2 no x loads, 4 no LDS staging writes, 8 no weight loads
 * returns the previous value, or INT32_MIN for an unknown name. */
long long upf_conv_packed_bytes(int Cin, int Cout, int kernel_size);
int upf_conv_pack_weights(const void* w /* [Cout,Cin,k,k] */, void* w_packed, int Cin, int Cout, int kernel_size,
                          int dtype, void* stream);
int upf_conv_forward(const void* x, long long x_batch_stride, const void* w_packed, const float* bias,
                     void* y, long long y_batch_stride, int B, int Cin, int Cout, int H, int W,
                     int kernel_size, int dilation, int stride, float leaky_slope, int dtype, void* stream);
/* PITCHED rows (round 5): the rows of x / y are x_row_pitch / y_row_pitch elements apart (>= W / Wo; 0 = contiguous; plane stride
 * rows * pitch).  A pitch that is a multiple of 8 (with 16-byte aligned bases and batch strides) selects the aligned staging and the
 * 16-byte epilogue for ANY logical width: the 8-pixel group that straddles W is loaded in place and its trailing pixels replaced by
 * the zero padding, an output segment that straddles Wo is stored whole (its tail lands in the row's own padding).  Nothing depends
 * on what the padding holds; results are bit-identical to upf_conv_forward on contiguous copies. */
int upf_conv_forward_pitched(const void* x, long long x_batch_stride, int x_row_pitch, const void* w_packed, const float* bias,
                             void* y, long long y_batch_stride, int y_row_pitch, int B, int Cin, int Cout, int H, int W,
                             int kernel_size, int dilation, int stride, float leaky_slope, int dtype, void* stream);
/* 1x1 convolution, Cout <= 32, whose OUTPUT type is the other 16-bit type (`pyramid_dtype`: the projection of the fp16 pyramid features
 * into the bf16 estimator / SGU buffers): x, w_packed of `dtype`, fp32 sums rounded once to `out_dtype`; y = NCHW planes (pitched like
 * upf_conv_forward_pitched) or, y_is_c8, channel octets (x rows 16-byte aligned). */
int upf_conv1x1_forward_mixed(const void* x, long long x_batch_stride, int x_row_pitch, const void* w_packed, const float* bias,
                              void* y, long long y_batch_stride, int y_row_pitch, int y_is_c8, int B, int Cin, int Cout, int H, int W,
                              float leaky_slope, int dtype, int out_dtype, void* stream);
/* The 1x1 projection of a level's features, NCHW -> octets, stored into TWO octet buffers by one launch (round 6): it is the input of
 * both dense stacks of a level — the flow estimator's buffer and the SGU estimator's (model/upflow.py:546-553 with :71-75) — and
 * used to be computed twice.  Same arithmetic and bits as upf_conv_forward_c8 / upf_conv1x1_forward_mixed (out_dtype may equal dtype). */
int upf_conv1x1_forward_c8_dual(const void* x, long long x_batch_stride, int x_row_pitch, const void* w_packed, const float* bias,
                                void* y8_a, long long ya_batch_stride, void* y8_b, long long yb_batch_stride,
                                int B, int Cin, int Cout, int H, int W, float leaky_slope, int dtype, int out_dtype, void* stream);
int upf_conv_set_option(const char* name, int value);

/* ---- the same convolutions for the fp32 PARITY mode: split-precision products on the fp16 matrix cores  (round 4;
 * csrc/conv_x3.hip).  The reference's convolutions are fp32 (model/pwc_modules.py:122-142, :250-286, :396-412,
 * model/upflow.py:24-60; cuDNN there, MIOpen here until round 4).  x, y, bias and w are fp32; both operands are split into two
 * fp16 halves (a = fp16(a) + fp16(a - fp16(a)), 22-23 bits) on the way into the kernel and every product is formed as
 * a_hi*b_hi + a_lo*b_hi + a_hi*b_lo (nprod = 3; nprod = 11: the low-order products accumulate in their own registers and
 * join the sum once, a third of the rounding chain) with fp32 accumulation in the MFMA: fp32-class results at about a third of
 * the 16-bit rate.  The weights are scaled by a per-layer power of two (computed on the device at pack time, stored in the packed
 * operand's 1 KB header) so that their low halves are normal fp16 numbers.  Range: |x| < 65504.
 * 3x3 with dilation 1..16 at stride 1, 3x3 at stride 2, 1x1; any H, W >= 1 (element-wise bounds at ragged / unaligned rows);
 * x / y are channel slices of contiguous NCHW fp32 buffers (batch strides in elements).  w_packed: upf_conv_x3_packed_bytes
 * bytes, filled by upf_conv_x3_pack_weights from w [Cout,Cin,k,k] fp32. */
long long upf_conv_x3_packed_bytes(int Cin, int Cout, int kernel_size);
int upf_conv_x3_pack_weights(const float* w, void* w_packed, int Cin, int Cout, int kernel_size, void* stream);
int upf_conv_x3_forward(const float* x, long long x_batch_stride, const void* w_packed, const float* bias, float* y,
                        long long y_batch_stride, int B, int Cin, int Cout, int H, int W, int kernel_size, int dilation,
                        int stride, float leaky_slope, int nprod, void* stream);
/* launch heuristics of upf_conv_x3_forward, for tuning and for the tests to reach both kernels: "sk_max_tiles" (96) — the split-K
 * kernel (2 x 32-pixel tiles, the four waves of a workgroup split the input channels; stride 1, >= 64 input channels, 3 products)
 * is chosen where the batch has at most this many 8 x 32-pixel tiles (0: never; 1 << 30: wherever eligible).
 * Returns the previous value, INT32_MIN for an unknown name. */
int upf_conv_x3_set_option(const char* name, int value);
/* writes 2^-6 to out_device[0] if v_mfma_f32_32x32x16_f16 multiplies fp16 SUBNORMAL inputs un-flushed (what the low halves of
 * small operands rely on), 0 if it flushes them */
int upf_mfma_f16_denorm_probe(float* out_device, void* stream);

/* ---- the same convolutions with operands in the channel-octet layout  (round 3; csrc/conv_c8.hip) -----------------------
 * "C8": [n][ceil(C/8)][H][W][8] — the 8 channels of a pixel are one 16-byte entry, which is one entry of the kernel's LDS
 * tile image and one k-octet of an MFMA operand.  Between the convolutions of a dense stack (model/pwc_modules.py:279-286,
 * model/upflow.py:53-60) and of the context network (:396-412) this layout removes the register transposition on the way
 * into LDS and the LDS transposition on the way out, and the tile image is filled by LDS-DMA into the other of two LDS buffers
 * under the matrix phase of the current chunk.  Tensors that other operators write or read plane-wise stay NCHW:
 *   input  = a C8 slice (x8: first octet plane, n8_oct octets; may be absent) followed — in the K order of the packed
 *            weights — by an NCHW part (x2, C2 planes; may be absent);  K = pad32(8*n8_oct) + pad32(C2) = upf_conv_c8_k()
 *   output = C8 octets (y_is_c8; channels that pad the last octet are written as zeros) or NCHW planes.
 * upf_conv_pack_weights_kmap gathers the input channels of w through kmap[K] (-1 = zero) into that K order.
 * stride 1, 16-byte aligned operands; kernel 3x3 with dilation 1 (any layout combination) or 2 / 4 / 8 / 16 (C8 in,
 * C8 out), or 1x1 (NCHW in, C8 out, Cout <= 32); stride 2 for a 3x3 with an NCHW input of > 16 channels and a C8 output of
 * <= 32.  Everything else: upf_conv_forward.
 * Width (round 5): C8 operands take ANY W (a pixel is one 16-byte entry: rows are always aligned); an NCHW input part needs
 * 16-byte aligned rows — W % 8 == 0, or (upf_conv_forward_c8_pitched) a row pitch that is a multiple of 8 with any logical W;
 * an NCHW output may be pitched too (y_row_pitch, 0 = Wo). */
long long upf_conv_packed_bytes_k(int K, int Cout, int kernel_size);
int upf_conv_c8_k(int n8_oct, int C2);
int upf_conv_pack_weights_kmap(const void* w /* [Cout,Cin,k,k] */, void* w_packed, int Cin, int Cout, int kernel_size,
                               const int* kmap /* device, [K] */, int K, int dtype, void* stream);
int upf_conv_forward_c8(const void* x8, long long x8_batch_stride, int n8_oct, const void* x2, long long x2_batch_stride, int C2,
                        const void* w_packed, const float* bias, void* y, long long y_batch_stride, int y_is_c8,
                        int B, int Cout, int H, int W, int kernel_size, int dilation, int stride, float leaky_slope,
                        int dtype, void* stream);
int upf_conv_forward_c8_pitched(const void* x8, long long x8_batch_stride, int n8_oct, const void* x2, long long x2_batch_stride, int x2_row_pitch, int C2,
                                const void* w_packed, const float* bias, void* y, long long y_batch_stride, int y_row_pitch, int y_is_c8,
                                int B, int Cout, int H, int W, int kernel_size, int dilation, int stride, float leaky_slope,
                                int dtype, void* stream);
int upf_conv_c8_set_option(const char* name, int value);   /* "rpw4" (1): Cout <= 32 on large grids: 16-row tiles */
/* Layers with Cout <= 16 (the 2- / 3-channel heads of the dense stacks, 176->8, 160->16; model/pwc_modules.py:262-263,
 * model/upflow.py:36-41) on the 16-output-channel matrix instruction: half the matrix work of a 32-channel block that would be
 * mostly padding.  3x3, dilation 1, stride 1, input = C8 octets only (k-map as in upf_conv_pack_weights_kmap, K % 32 == 0);
 * the same products as upf_conv_forward_c8, summed 32 input channels per instruction instead of 16 (fp32 sums may differ in
 * the last bit). */
long long upf_conv_packed_bytes_k16(int K, int Cout);
int upf_conv_pack_weights_kmap16(const void* w /* [Cout,Cin,3,3] */, void* w_packed, int Cin, int Cout,
                                 const int* kmap /* device, [K] */, int K, int dtype, void* stream);
int upf_conv_forward_c8_narrow(const void* x8, long long x8_batch_stride, int n8_oct, const void* w_packed16, const float* bias,
                               void* y, long long y_batch_stride, int y_is_c8, int B, int Cout, int H, int W, float leaky_slope,
                               int dtype, void* stream);
/* The MERGED NARROW TAIL of a dense stack (round 6).  The layers of a dense stack read nested channel suffixes of one buffer
 * (model/pwc_modules.py:279-286: x = cat([conv_k(x), x]); model/upflow.py:53-60), so the head reads [conv5's output | what
 * conv5 read]:  conv_last = W_last[:, conv5 part] * conv5_out + W_last[:, rest] * rest,  and the second term shares its input
 * with conv5.  A launch with 2 ... 32 output channels costs what the staging of its input costs, so
 *   upf_conv_forward_c8_split: ONE pass over the shared octet input computes a layer of C_main (a multiple of 8) output channels
 *     completely — bias, LeakyReLU, octets into y8 — and, as output channels [C_main, Cout) of the same packed operand (Cout <=
 *     128: they occupy what would be padding of the layer's last 32-channel block(s)), the shared-input part of later layers INCLUDING their bias: raw fp32,
 *     as planes of channel quads partial[n][partial_pitch / 4][y][x][4] (channel c -> float c - C_main; 16 bytes per pixel and quad);
 *   upf_conv_forward_c8_narrow_init: upf_conv_forward_c8_narrow (Cout <= 16) for a later layer on the channels the tail itself
 *     produced, its accumulators starting from floats [partial_offset, +Cout) of that record instead of from a bias.
 * The result is the layer's own fp32 sum in another order; nothing is rounded to 16 bits in between.  3x3, dilation 1, stride 1. */
int upf_conv_forward_c8_split(const void* x8, long long x8_batch_stride, int n8_oct, const void* w_packed /* upf_conv_pack_weights_kmap, Cout rows */,
                              const float* bias /* [Cout] */, void* y8, long long y_batch_stride, int C_main,
                              float* partial, long long partial_batch_stride /* floats */, int partial_pitch /* partial channels per pixel, % 4 == 0 */,
                              int B, int Cout, int H, int W, float leaky_slope, int dtype, void* stream);
int upf_conv_forward_c8_narrow_init(const void* x8, long long x8_batch_stride, int n8_oct, const void* w_packed16,
                                    const float* partial, long long partial_batch_stride, int partial_pitch, int partial_offset /* % 4 == 0 */,
                                    void* y, long long y_batch_stride, int y_is_c8, int B, int Cout, int H, int W, float leaky_slope,
                                    int dtype, void* stream);

/* TWO convolutions as one launch (round 6): a 3x3 layer (Cin <= 16 -> C1 = 16 | 32 channels, LeakyReLU) followed by a 3x3 layer (C1 -> C2 <= 32
 * channels, LeakyReLU) with strides (1, 2) — the two halves of the SGU guidance stem (model/upflow.py:30-33: conv(3, 16), conv(16, 16, stride=2),
 * conv(16, 32), conv(32, 32, stride=2) on both frames at full resolution) — or (2, 1) — the first two stages of the feature pyramid
 * (model/pwc_modules.py:122-142) — whose intermediate (126 / 63 / 31 / 16 MB at 384x1280) then never leaves the chip: a workgroup computes the
 * first layer on the pixels its tile of the second layer reads — rounded to the 16-bit type, zero outside the image: the values the two-launch
 * form reads back — into LDS and multiplies from there.
 * x: NCHW [B,Cin,H,W] with an EVEN row pitch (rows are read as pixel pairs); y: NCHW [B,C2,Ho,Wo] (row pitch given) or, strides (1, 2) only,
 * octets [B,ceil(C2/8),Ho,Wo,8]; Ho = ceil(H/2), Wo = ceil(W/2).  leaky slope 0 = no activation.
 * Packed operands (16-bit, MFMA lane order; lane = co + 32 kg, 8 consecutive k per lane):
 *   wa [S][64][8], S = 3 for Cin <= 4 (k-octet kg of step s = taps 4s + 2kg and 4s + 2kg + 1, 4 channels each), S = 5 for Cin <= 8 (k-octet kg of
 *   step s = tap 2s + kg, channels 0..7), S = 9 for Cin <= 16 (step = tap, kg = channel octet);
 *   wb [9][C1/16][64][8] (tap, k-step of 16 channels, kg = channel octet within the step); rows co >= C / absent taps / channels are zero.
 * The sums are the layers' own fp32 sums in another order than upf_conv_forward's (two taps per instruction in the first layer). */
int upf_conv_pair_forward(const void* x, long long x_batch_stride, int x_row_pitch, int Cin,
                          const void* wa_packed, const float* bias_a /* [C1] */, float slope_a, int C1, int stride_a,
                          const void* wb_packed, const float* bias_b /* [C2] */, float slope_b, int C2, int stride_b,
                          void* y, long long y_batch_stride, int y_row_pitch, int y_is_c8,
                          int B, int H, int W, int dtype, void* stream);

/* ---- the same convolutions under autograd: training on the matrix cores  (model/pwc_modules.py:250-286, :396-412) ----
 * forward      upf_conv_forward on weights packed straight from the fp32 master copy: upf_conv_pack_weights_f32(dgrad=0)
 * data grad    of a stride-1 convolution = the same convolution of grad_y with the flipped, transposed kernel:
 *              upf_conv_pack_weights_f32(dgrad=1) (packs [Cin x Cout], upf_conv_packed_bytes(Cout, Cin, k) bytes), then
 *              upf_conv_forward(grad_pre, ..., Cin := Cout, Cout := Cin, leaky_slope 0, zero bias)
 * activation   upf_leaky_backward: grad_pre = grad_y * (y > 0 ? 1 : slope), y = the forward OUTPUT (n % 8 == 0 elements)
 * weight grad  upf_conv_wgrad: grad_w[co][ci][ky][kx] = sum_{n,y,x} grad_pre[n,co,y,x] * x[n,ci,y+(ky-1)d,x+(kx-1)d], fp32
 *              [Cout,Cin,k,k], an MFMA GEMM with K = pixels, deterministic split-K (workspace:
 *              upf_conv_wgrad_workspace_bytes).  bf16 / fp16, stride 1, W >= 8, 3x3 with d in {1,2,4,8,16} or 1x1
 *              (upf_conv_wgrad_supported); x / grad_pre may be channel slices of wider buffers (batch strides in elements).
 * bias grad    upf_conv_bias_grad: grad_b[co] = sum_{n,y,x} grad_pre[n,co,y,x], fp32, fixed summation order (workspace:
 *              upf_conv_bias_grad_workspace_bytes). */
int upf_conv_pack_weights_f32(const float* w /* [Cout,Cin,k,k] fp32 */, void* w_packed, int Cin, int Cout, int kernel_size,
                              int dtype, int dgrad, void* stream);
/* njobs of the above in one launch (host arrays of the per-layer arguments): a training step re-packs every layer from its
 * fp32 master weights after the optimiser step */
int upf_conv_pack_weights_f32_multi(const float* const* w, void* const* w_packed, const int* Cin, const int* Cout, const int* kernel_size,
                                    const int* dgrad, int njobs, int dtype, void* stream);
/* The data-gradient operands of a DENSE STACK in one launch (round 5).  Layers j = 0..nlayers-1 ([Cout_j, Cin_j, 3, 3] fp32 masters,
 * ordered like the stack's gradient buffer: last layer first) read the buffer channels [first_channel_j, first_channel_j + Cin_j).
 * Slice t = buffer channels [slice_channel_t, + slice_width_t), read by the first nconsumers_t layers: w_packed[t] (upf_conv_packed_bytes(
 * sum Cout_j, slice_width_t, 3) bytes) = upf_conv_pack_weights_f32(dgrad = 1) of the concatenation along Cout of
 * w_j[:, slice_channel_t - first_channel_j : + slice_width_t] — bit-identical, without the concatenation.  nlayers, nslices <= 8. */
int upf_conv_pack_stacked_dgrad(const float* const* w, const int* Cin, const int* Cout, const int* first_channel, int nlayers,
                                void* const* w_packed, const int* slice_channel, const int* slice_width, const int* nconsumers,
                                int nslices, int dtype, void* stream);
int upf_leaky_backward(const void* grad_y, const void* y, void* grad_pre, long long n, float slope, int dtype, void* stream);
int upf_conv_wgrad_supported(int Cin, int Cout, int H, int W, int kernel_size, int dilation, int stride, int dtype);
long long upf_conv_wgrad_workspace_bytes(int B, int Cin, int Cout, int H, int W, int kernel_size, int dilation);
int upf_conv_wgrad(const void* x, long long x_batch_stride, const void* grad_pre, long long g_batch_stride, float* grad_w,
                   void* workspace, int B, int Cin, int Cout, int H, int W, int kernel_size, int dilation, int dtype, void* stream);
/* One weight gradient over SEVERAL uses of the same weights (the decoder is shared by the five pyramid levels,
 * model/upflow.py:535-573): the pixels of every level are one K dimension, so the levels share the K-split launches, the
 * partial blocks and the one ordered reduction (instead of a launch pair per level plus fp32 adds of the results).
 * 1..6 levels of any sizes (each: upf_conv_wgrad_supported); aligned and ragged levels share ONE launch (the staging of a
 * ragged level's border blocks is chosen per tile).  Query the workspace size with the same level array.
 * Environment (A/B runs): UPF_WGRAD_SPLIT="slices,J" overrides the K-split, UPF_WGRAD_ABLATE the experiments of tools/wgrad_ablate.py. */
typedef struct {
  const void* x;        long long x_batch_stride;      /* [B, Cin, H, W] slice, batch stride in elements (0 = dense) */
  const void* grad_pre; long long g_batch_stride;      /* [B, Cout, H, W] slice */
  int B, H, W;
} upf_wgrad_level;
long long upf_conv_wgrad_multi_workspace_bytes(const upf_wgrad_level* levels, int nlevels, int Cin, int Cout, int kernel_size, int dilation);
int upf_conv_wgrad_multi(const upf_wgrad_level* levels /* host array */, int nlevels, float* grad_w, void* workspace, int Cin, int Cout,
                         int kernel_size, int dilation, int dtype, void* stream);
/* ... and, in the same reduction launch, the second stage of the layer's BIAS gradient (upf_conv_bias_grad_finish over
 * 1..8 first-stage buffers; model/pwc_modules.py:250-286 — every decoder layer has a bias): one launch fewer per layer and step.
 * npartials = 0: exactly upf_conv_wgrad_multi. */
int upf_conv_wgrad_multi_bias(const upf_wgrad_level* levels, int nlevels, float* grad_w, void* workspace, int Cin, int Cout,
                              int kernel_size, int dilation, const float* const* bias_partials /* host array */, int npartials, float* grad_bias,
                              int dtype, void* stream);
/* Stride-2 3x3 layers (feature pyramid, SGU guidance; model/pwc_modules.py:95, model/upflow.py:53-55) take the stride-1
 * gradient kernels through their space-to-depth form: xs[(ci,p,q), i, j] = x[ci, 2i+p, 2j+q] (upf_space_to_depth2; inverse = 1
 * for the way back) convolved at stride 1 with a kernel that is w at 9 of its 36 (phase, tap) positions.
 *   weight gradient: upf_conv_wgrad_s2d — levels hold xs ([B, 4*Cin, H/2, W/2]) and grad_pre; grad_w is [Cout, Cin, 3, 3]
 *                    (workspace: upf_conv_wgrad_multi_workspace_bytes with Cin := 4*Cin)
 *   data gradient:   upf_conv_pack_weights_f32(w, ..., dgrad = 2) (upf_conv_packed_bytes(Cout, 4*Cin, 3) bytes), then
 *                    upf_conv_forward(grad_pre, ..., Cin := Cout, Cout := 4*Cin) and upf_space_to_depth2(inverse = 1).
 *                    Exact on finite operands (tests/test_hip_conv_exact.py), but the 27 structural zeros of the packed kernel
 *                    are multiplied like any weight: a NaN / inf element of grad_pre makes its whole 3x3 neighbourhood of xs
 *                    pixels — a 6x6 block of x pixels — NaN where the layer's footprint is 3x3 (0 * NaN = NaN).  A caller that
 *                    needs non-finite gradients confined to the layer's footprint takes the TRANSPOSED form instead, as the
 *                    Python training path does (ops.ConvTrainFunction): grad_pre copied to the even pixels of a zero
 *                    [B, Cout, H, W] tensor, then the stride-1 data gradient (dgrad = 1) — the same flops, the zeros are data. */
int upf_space_to_depth2(const void* src, void* dst, int B, int C /* of x */, int H, int W /* of x, even */, int inverse, int dtype, void* stream);
int upf_conv_wgrad_s2d(const upf_wgrad_level* levels, int nlevels, float* grad_w, void* workspace, int Cin, int Cout, int dtype, void* stream);
/* dst = (src + add) * (y > 0 ? 1 : slope) over channel-sliced [B, C, HW] tensors (add, y optional; dst may be src):
 * the gradient entering a layer's pre-activation, with the first stage of the bias gradient (bias_partial: C x 32 fp32,
 * optional) from the same pass; dst = NULL: the bias sums only.  upf_conv_bias_grad_finish sums the first-stage buffers of 1..8 uses in order. */
int upf_act_grad(const void* src, long long src_batch_stride, const void* add, long long add_batch_stride, const void* y,
                 long long y_batch_stride, void* dst, long long dst_batch_stride, float* bias_partial, int B, int C, int HW,
                 float slope, int dtype, void* stream);
/* The 3x3 stride-1 convolution with upf_act_grad's arithmetic in its epilogue (round 5): y = (round16(round16(conv(x)) + add))
 * * (act > 0 ? 1 : mask_slope), bit-identical to upf_conv_forward_pitched (bias as given, no activation) followed by
 * upf_act_grad(src = dst = y, add, y := act, mask_slope).  add and act (either may be NULL, not both): [B,Cout,H,W] channel slices
 * with y's row pitch.
 * The data-gradient convolutions of the dense stacks (reference: autograd through model/pwc_modules.py's estimator / context
 * stacks); their bias sums are then ONE upf_act_grad(dst = NULL) pass over the stack's whole gradient buffer. */
int upf_conv_forward_gated(const void* x, long long x_batch_stride, int x_row_pitch, const void* w_packed, const float* bias,
                           void* y, long long y_batch_stride, int y_row_pitch, const void* add, long long add_batch_stride,
                           const void* act, long long act_batch_stride, float mask_slope,
                           int B, int Cin, int Cout, int H, int W, int dtype, void* stream);
int upf_conv_bias_grad_finish(const float* const* partials /* host array of device pointers */, int npartials, float* grad_bias,
                              int Cout, void* stream);
long long upf_conv_bias_grad_workspace_bytes(int Cout);
int upf_conv_bias_grad(const void* grad_pre, long long g_batch_stride, float* grad_bias, void* workspace, int B, int Cout, int HW,
                       int dtype, void* stream);

/* ---- gradients of the split-precision convolution: fp32 training on the fp16 matrix cores  (csrc/conv_x3_bwd.hip) ----------
 * y = LeakyReLU_slope(conv(x, w) + b), fp32 tensors and fp32 gradients, no host synchronisation (the step captures into a hipGraph).
 * GRADIENT RANGE.  The operand split has an absolute floor (an un-scaled operand below 2^-3 has a subnormal low half, below 6e-8 both
 * halves are zero) and the losses are mean()-reduced: grad_pre is routinely 1e-6 ... 1e-9.  So the gradient that enters a layer's
 * pre-activation only exists SCALED by a per-tensor power of two taken from its device-side |.|max (the rule of the packed weights:
 * the maximum lands in [2^13, 2^14)); every consumer un-scales exactly.  Results for grad_y and grad_y * 2^-k are the same bits up
 * to that factor, as long as the scale's exponent stays inside its clamp of +-100 (2^-87 <= max |grad_pre| < 2^114); beyond it the
 * scale is 2^+-100, for an all-zero or non-finite maximum 1 (NaN elements do not define the maximum; NaN and inf propagate).
 * Two floors remain (tests/test_hip_conv_x3_bwd_ops.py, modelled in tests/_x3_model.py):
 *   - ONE scale per tensor: an element of grad_pre below 2^-16 of the tensor's maximum (|gs| < 2^-3) has a subnormal low half and
 *     carries up to 2^-25 of absolute error in gs, i.e. 2^-38 * max |grad_pre|: grad_x (stride 1) is off by up to that times
 *     max_ci sum_{co,tap} |w|, a row of grad_w by up to that times sum_{n,pixel} |x[n,ci]|.  Down to 2^-14 of the maximum whole regions
 *     (an occluded half, one sample, a group of channels) keep fp32-class error relative to their OWN maximum; below, the floor.
 *     The stride-2 data gradient (plain fp32) and the bias gradient have no such floor.
 *   - the ACTIVATION operand of upf_conv_x3_wgrad is split un-scaled, like the forward's: |x| < 2^-3 carries up to 2^-25 of
 *     absolute error, grad_w up to 2^-25 * max_co sum_{n,pixel} |grad_pre[n,co]|.  fp32-class for O(1) activations and above (up to
 *     fp16's range), a floor for tiny ones.
 *   upf_act_grad_x3   gs = grad_y * (y > 0 ? 1 : slope) * 2^s  (y NULL: no activation) over [B,C,HW] channel slices (batch strides in
 *                     elements, 0 = dense);  scale_slot: 4 floats on the device, written {|.|max bits, 2^s, 2^-s, 0};  bias_partial
 *                     (optional): C x 32 sums of gs, the first stage of the bias gradient, fixed order.  Three launches.
 *   upf_conv_x3_pack_weights_dgrad   the operand of the data gradient of a stride-1 layer: upf_conv_x3_pack_weights of the flipped,
 *                     transposed kernel (upf_conv_x3_packed_bytes(Cout, Cin, k) bytes; same header and per-layer scale).  NOT read-only
 *                     afterwards: upf_conv_x3_dgrad rewrites one header field per call (stream ordered).
 *   upf_conv_x3_dgrad grad_x [B,Cin,H,W] from gs [B,Cout,Ho,Wo]: stride 1 (3x3 with dilation 1..16, 1x1) = upf_conv_x3_forward on
 *                     w_packed_dgrad, the un-scaling folded into the operand header's 2^-s (zero_bias: Cin zeros; w unused);
 *                     stride 2 (3x3) = a plain fp32 kernel on the master weights w [Cout,Cin,3,3] (w_packed_dgrad, zero_bias unused).
 *                     Any H, W >= 1.
 *   upf_conv_x3_wgrad grad_w [Cout,Cin,k,k] = sum over 1..6 levels (uses of the same weights: x [B,Cin,H,W], grad_pre = gs
 *                     [B,Cout,Ho,Wo], each with its own scale_slots[l]; NULL array or NULL entry = that grad_pre is
 *                     UN-SCALED and taken as it is: for O(1) gradients only, the split's absolute floor applies) of the pixel sums
 *                     gs[n,co,y,x] * x[n,ci,y*s+(ky-1)d,x*s+(kx-1)d]: both operands split into fp16 halves on the way into the
 *                     registers, three v_mfma_f32_16x16x32_f16 per pair, K = the flattened pixels (any H, W >= 1, either stride),
 *                     deterministic split-K (per-slice partial blocks in `workspace`, one ordered reduction that also applies each
 *                     level's 2^-s).  grad_bias (optional) [Cout]: finished by the same reduction from bias_partials[l] (the C x 32
 *                     buffers of upf_act_grad_x3, one per level).  Workspace: upf_conv_x3_wgrad_workspace_bytes (the size through *bytes; UPF_EINVAL for what the kernel does not take). */
int upf_act_grad_x3(const float* grad_y, long long gy_batch_stride, const float* y, long long y_batch_stride, float* grad_pre_scaled,
                    long long dst_batch_stride, float* bias_partial, float* scale_slot, int B, int C, int HW, float slope, void* stream);
int upf_conv_x3_pack_weights_dgrad(const float* w, void* w_packed, int Cin, int Cout, int kernel_size, void* stream);
int upf_conv_x3_dgrad(const float* grad_pre_scaled, long long g_batch_stride, const float* scale_slot, const float* w,
                      void* w_packed_dgrad, const float* zero_bias, float* grad_x, long long gx_batch_stride, int B, int Cin,
                      int Cout, int H, int W, int kernel_size, int dilation, int stride, void* stream);
int upf_conv_x3_wgrad_workspace_bytes(const upf_wgrad_level* levels, int nlevels, int Cin, int Cout, int kernel_size,
                                      int dilation, int stride, long long* bytes /* host, out */);
int upf_conv_x3_wgrad(const upf_wgrad_level* levels /* host array */, const float* const* scale_slots /* host array */, int nlevels,
                      float* grad_w, void* workspace, int Cin, int Cout, int kernel_size, int dilation, int stride,
                      const float* const* bias_partials /* host array */, float* grad_bias, void* stream);

/* ---- flow bookkeeping of a pyramid level  (model/upflow.py:566-572) -------------------------------
 * out[n,:] = cast(a + (b + c)) in fp32, b and c optional: `flow_up + res` into the context network's input,
 * `flow_up + (res + fine)` for the next level, or a plain fp32 -> 16-bit copy of a flow into an estimator slot.
 * a : [N,per_item] fp32;  b, c : [N,per_item] of `dtype` (bf16 / fp16) or NULL;  out : fp32 (out_is_f32) or `dtype`,
 * rows out_batch_stride elements apart (0 = per_item). */
int upf_flow_update(const float* a, const void* b, const void* c, void* out, long long out_batch_stride,
                    int out_is_f32, int N, int per_item, int dtype, void* stream);
/* The same sum of a 2-channel flow a : [N,2,HW] (b, c likewise) written as one octet of a C8 buffer: positions 0, 1 = the two
 * components, positions 2..7 = 0.  out8 : the octet, out8_batch_stride in elements. */
int upf_flow_update_c8(const float* a, const void* b, const void* c, void* out8, long long out8_batch_stride,
                       int N, int HW, int dtype, void* stream);

/* ---- occlusion check  (tools.occ_check_model(obj), utils/tools.py:519-588, 641-677) -------------
 * flow_f, flow_b : [B,2,H,W] fp32 -> occ_fw, occ_bw : [B,1,H,W] fp32 in {0,1}. */
int upf_occ_check(const float* flow_f, const float* flow_b, float* occ_fw, float* occ_bw,
                  int B, int H, int W, float alpha1, float alpha2, void* stream);

/* Self-test of the division-free, correctly rounded quotient the sampling kernels use for 2(j+fx)/(W-1) (csrc/sampling.hpp:
 * div_by_const): compares it with the IEEE division over ALL 2^32 bit patterns of the numerator for the divisor
 * max(size-1, 1) and adds the number of differing results to *mismatches (device memory, zeroed by the caller).  ~30 ms. */
int upf_div_selftest(int size, unsigned long long* mismatches, void* stream);

/* ---- soft census distance of the photometric loss  (utils/loss.py:50-91) ----
 * gray1, gray2 : [B,1,H,W] fp32 grey images (0.2989 r + 0.5870 g + 0.1140 b);  dist : [B,1,H,W] fp32,
 *   dist(p) = sum_k d_k/(0.1+d_k),  d_k = (t_k(gray1,p) - t_k(gray2,p))^2,  t_k(I,p) = u/sqrt(0.81+u^2),  u = I(p+k) - I(p),
 * k over the (2*max_distance+1)^2 offsets, images zero padded — the reference's 49-channel identity conv2d + ~10
 * element-wise passes in one launch.  Backward: gradients wrt either grey image (a NULL output is skipped), gather
 * formulation, deterministic. */
int upf_census_forward(const float* gray1, const float* gray2, float* dist, int B, int H, int W, int max_distance, void* stream);
int upf_census_backward(const float* gray1, const float* gray2, const float* grad_dist, float* g_gray1, float* g_gray2,
                        int B, int H, int W, int max_distance, void* stream);

/* ---- loss-side operators of the unsupervised training step  (SURVEY.md §8f rank 3), fp32 ---------------------------
 * boundary-dilated warp, tools.boundary_dilated_warp.warp_im (utils/tools.py:351-499): out[n,c,i,j] = clamp-to-edge
 * bilinear sample of the UN-cropped frame image[n,c] ([B,C,Hi,Wi]) at (j + start[n,0] + flow[n,0,i,j],
 * i + start[n,1] + flow[n,1,i,j]), weights from the clamped corner coordinates.  flow [B,2,h,w], start [B,2] (x, y),
 * out [B,C,h,w].  Backward: gradient wrt the flow (the image is data). */
int upf_boundary_warp_forward(const float* image, const float* flow, const float* start, float* out,
                              int B, int C, int Hi, int Wi, int h, int w, void* stream);
int upf_boundary_warp_backward(const float* image, const float* flow, const float* start, const float* grad_out,
                               float* grad_flow, int B, int C, int Hi, int Wi, int h, int w, void* stream);

/* Deterministic reductions: a forward call writes upf_loss_partials(n_pixels) pairs of floats (one per workgroup) that
 * the caller sums in order; n_pixels = B*H*W. */
int upf_loss_partials(long long n_pixels);

/* 'abs_robust' photometric / distillation term, network_tools.photo_loss_multi_type (model/upflow.py:265-288):
 *   partials[k] = { sum (|x - y| + eps)^q * occ,  sum occ }   over workgroup k's pixels, all C channels;
 * x, y [B,C,HW]; occ [B,HW] or NULL (= 1).  Backward: grad_x = coef[0] * occ * q * (|d|+eps)^(q-1) * sign(d),
 * grad_y = -grad_x (either may be NULL); coef is a DEVICE scalar (upstream gradient / the loss's denominator).
 * (The kernel pair is templated on the point-wise kind; this is its abs_robust instantiation, upf_pointwise_loss_* the others.) */
int upf_robust_loss_forward(const float* x, const float* y, const float* occ, float* partials,
                            int B, int C, int HW, float eps, float q, void* stream);
int upf_robust_loss_backward(const float* x, const float* y, const float* occ, const float* coef,
                             float* grad_x, float* grad_y, int B, int C, int HW, float eps, float q, void* stream);

/* grey = 0.2989 r + 0.5870 g + 0.1140 b of an RGB image [B,3,HW] -> [B,1,HW], the reference's left-to-right evaluation
 * (utils/loss.py:53-55). */
int upf_grey_forward(const float* image, float* grey, int B, int HW, void* stream);

/* Pyramid-distillation term, style 'upup' (model/upflow.py:461-487, network_tools.photo_loss_multi_type 'abs_robust' on
 * upsample_flow(level flow, label)), ONE direction, all levels:
 *   out2[0] = weight * sum_l [ sum (|up(x_l) - y| + eps)^q * occ ] / den,   out2[1] = den = sum occ + 1e-6  (occ NULL: B*2*H*W)
 * x_low[l] [B,2,hs[l],ws[l]] fp32 (1..6 levels, ws >= 2), up = bilinear, align_corners, times the size ratio per component
 * (pwc_modules.py:77-90); y [B,2,H,W] the detached label, occ [B,1,H,W] or NULL.  Forward: one pass over the label + one finishing
 * launch (partials: upf_msd_upup_partials(B,H,W) x 7 floats).  Backward: grad_x_low[l] = d out2[0] / d x_low[l] * grad_out[0],
 * one launch for all levels (deterministic gathers).  x_low / grad_x_low / hs / ws are HOST arrays. */
int upf_msd_upup_partials(int B, int H, int W);
int upf_msd_upup_forward(const float* const* x_low, const int* hs, const int* ws, int nlevels, const float* y, const float* occ,
                         float* partials, float* out2, int B, int H, int W, float weight, float eps, float q, void* stream);
int upf_msd_upup_backward(const float* const* x_low, float* const* grad_x_low, const int* hs, const int* ws, int nlevels, const float* y,
                          const float* occ, const float* grad_out, const float* fwd_out2, int B, int H, int W, float weight, float eps, float q,
                          void* stream);

/* first-order edge-aware smoothness, network_tools.edge_aware_smoothness_order1 (model/upflow.py:197-216):
 *   partials[k] = { sum |pred(i,j)-pred(i+1,j)| * exp(-mean_c |img(i,j)-img(i+1,j)|),  the same along j };
 * loss = sum_x / (B*Cp*(H-1)*W) + sum_y / (B*Cp*H*(W-1)).  img [B,Ci,H,W], pred [B,Cp,H,W].
 * Backward: gradient wrt pred of that loss times the device scalar grad_up[0] (gather, deterministic). */
int upf_smooth_edge1_forward(const float* img, const float* pred, float* partials,
                             int B, int Ci, int Cp, int H, int W, void* stream);
int upf_smooth_edge1_backward(const float* img, const float* pred, const float* grad_up, float* grad_pred,
                              int B, int Ci, int Cp, int H, int W, void* stream);

/* ---- non-default loss variants (csrc/loss_variants.hip; upf_pointwise_loss_*: csrc/loss.hip); fp32 contiguous NCHW, deterministic, no host synchronisation ---- */

/* second-order edge-aware smoothness, network_tools.edge_aware_smoothness_order2 (model/upflow.py:220-243):
 *   xx(i,j) = (p(i,j) - p(i+1,j)) - (p(i+1,j) - p(i+2,j)),  wx(i,j) = exp(-mean_c |img(i,j) - img(i+2,j)|),  i < H-2; columns likewise;
 *   partials[k] = { sum |xx| * wx, sum |yy| * wy }  (upf_loss_partials(B*H*W) pairs);
 *   loss = sum_x / (B*Cp*(H-2)*W) + sum_y / (B*Cp*H*(W-2)).  H, W >= 3.
 * Backward: gradient wrt pred of that loss times the device scalar grad_up[0] (gather over up to three row and three column
 * terms with coefficients 1, -2, 1; sign(0) = 0).  No gradient wrt img. */
int upf_smooth_edge2_forward(const float* img, const float* pred, float* partials,
                             int B, int Ci, int Cp, int H, int W, void* stream);
int upf_smooth_edge2_backward(const float* img, const float* pred, const float* grad_up, float* grad_pred,
                              int B, int Ci, int Cp, int H, int W, void* stream);

/* delta smoothness, network_tools.flow_smooth_delta (model/upflow.py:245-263) on BC = B*C planes [H,W]:
 *   dx = f(i,j+1) - f(i,j), dy = f(i+1,j) - f(i,j); second_order adds dx2, dxdy (horizontal / vertical difference of dx) and
 *   dydx, dy2 (of dy), each built from the first differences;
 *   partials[k][0..1] (or [0..5]) = sums of |dx|, |dy| [, |dx2|, |dxdy|, |dydx|, |dy2|]  (upf_loss_partials(BC*H*W) rows);
 *   loss = sum of the terms' means.  H, W >= 2 (>= 3 with second_order).
 * Backward: gradient of that loss times the device scalar grad_up[0] (one gather). */
int upf_smooth_delta_forward(const float* flow, float* partials, int BC, int H, int W, int second_order, void* stream);
int upf_smooth_delta_backward(const float* flow, const float* grad_up, float* grad_flow, int BC, int H, int W,
                              int second_order, void* stream);

/* point-wise photometric kinds of network_tools.photo_loss_multi_type (model/upflow.py:273-278, :284-287): the kernel pair of
 * upf_robust_loss_* with another compile-time kind (csrc/loss.hip):  UPF_LOSS_CHARBONNIER ((x-y)^2 + 1e-6)^q,  UPF_LOSS_L1 |x - y + 1e-6|  (q unused);
 *   partials[k] = { sum loss * occ, sum occ }  (upf_loss_partials(B*HW) pairs; occ [B,HW] or NULL = 1, summed once per pixel).
 * Backward: grad_x = coef[0] * occ * d loss / d (x-y), grad_y = -grad_x (either may be NULL); coef is a DEVICE scalar. */
enum { UPF_LOSS_CHARBONNIER = 0, UPF_LOSS_L1 = 1 };
int upf_pointwise_loss_forward(const float* x, const float* y, const float* occ, float* partials,
                               int B, int C, int HW, int kind, float q, void* stream);
int upf_pointwise_loss_backward(const float* x, const float* y, const float* occ, const float* coef,
                                float* grad_x, float* grad_y, int B, int C, int HW, int kind, float q, void* stream);

/* weighted SSIM, network_tools.weighted_ssim (model/upflow.py:139-195) with c1 = inf and finite c2 > 0:  x, y [B,C,H,W],
 * weight [B,1,H,W], 3x3 VALID windows, H, W >= 3.  Forward, one launch, every output optional (NULL):
 *   map [B,C,H-2,W-2] = clamp((1 - (2 sigma_xy + c2) / (sigma_x + sigma_y + c2)) / 2, 0, 1),  w_avg [B,1,H-2,W-2] = avg_pool(weight),
 *   partials[k] = { sum map * w_avg, sum w_avg (once per window), sum map }  (upf_loss_partials(B*(H-2)*(W-2)) triples).
 * Backward, one launch: the upstream gradient of window p, channel c is
 *   grad_map[p,c] (if given) + coef_w[0] * w_avg(p) (if given) + coef_u[0] (if given)      — coef_w, coef_u DEVICE scalars;
 * grad_x / grad_y (either may be NULL) gather it through at most nine windows per pixel; the clamp passes the gradient on
 * [0,1] inclusive.  No gradient wrt weight. */
int upf_ssim_forward(const float* x, const float* y, const float* weight, float* map, float* w_avg, float* partials,
                     int B, int C, int H, int W, float c2, float weight_epsilon, void* stream);
int upf_ssim_backward(const float* x, const float* y, const float* weight, const float* grad_map,
                      const float* coef_w, const float* coef_u, float* grad_x, float* grad_y,
                      int B, int C, int H, int W, float c2, float weight_epsilon, void* stream);

/* ---- optimiser step and dynamic loss scaling on the device (csrc/optim.hip) ---------------------------------------------
 * The reference trains with torch.optim.Adam(lr=1e-4, amsgrad=True, weight_decay=1e-4) (scripts/simple_train.py:121); these
 * entry points are that update, torch/optim/adam.py in its capturable form, plus the state machine of a GradScaler, as
 * launches that only enqueue: fp16 training multiplies the gradient fed to backward by a loss scale S, and the check, the
 * un-scaling, the skipped step and the scale update all happen inside the captured step.
 *
 * Multi-tensor launches: one upf_mt_launch is ONE kernel launch over up to UPF_MT_TENSORS fp32 tensors and UPF_MT_BLOCKS
 * workgroups; workgroup b takes elements [block_chunk[b] * UPF_MT_CHUNK, + UPF_MT_CHUNK) of tensor block_tensor[b].  The
 * table is a HOST structure that is passed to the kernel by value (the addresses of a captured step's gradients are not
 * known before the capture, and a host-to-device copy cannot be captured), so it stays under the 4 KB argument limit and a
 * longer tensor list is split over several launches (ops.mt_plan).  Pointers need 4-byte alignment only (gradients under
 * DDP are views into bucket storage); numel is any positive count. */
#define UPF_MT_TENSORS 48
#define UPF_MT_BLOCKS 256
#define UPF_MT_CHUNK 16384
typedef struct {
  void* param[UPF_MT_TENSORS];
  void* grad[UPF_MT_TENSORS];
  void* exp_avg[UPF_MT_TENSORS];
  void* exp_avg_sq[UPF_MT_TENSORS];
  void* max_exp_avg_sq[UPF_MT_TENSORS];
  int numel[UPF_MT_TENSORS];
  int block_chunk[UPF_MT_BLOCKS];
  unsigned char block_tensor[UPF_MT_BLOCKS];
  int n_tensors, n_blocks;
} upf_mt_launch;
/* flag[0] = 1 if any element of the launch's gradients is NaN or +-inf (read-only pass; only `grad` and `numel` of the
 * table are read; a plain store, never cleared here). */
int upf_grads_nonfinite_check(const upf_mt_launch* launch, int* flag, void* stream);
/* torch.optim.Adam(amsgrad=True, maximize=False) with L2 weight decay on the launch's tensors, all operands DEVICE scalars:
 *   g = grad / loss_scale[0] (a power of two: exact) + weight_decay * p;   t = step[0] + 1   (step is NOT advanced here)
 *   m = lerp(m, g, 1 - beta1);   v = beta2 v + (1 - beta2) g^2;   vmax = max(vmax, v)
 *   p -= (lr[0] / (1 - beta1^t)) * m / (sqrt(vmax) / sqrt(1 - beta2^t) + eps)
 * fp32 state, double hyper-parameters, the rounding points of torch's multi-tensor kernel.  flag[0] != 0: nothing is
 * written (parameters, both moments and the running maximum keep their bits). */
int upf_adam_amsgrad_step(const upf_mt_launch* launch, const float* lr, const float* step, const float* loss_scale,
                          const int* flag, double beta1, double beta2, double eps, double weight_decay, void* stream);
/* ---- a bound on the global gradient norm, and the norm as a statistic (torch.nn.utils.clip_grad_norm_, L2, inside the step).
 * For ONE optimizer step over ALL launches of ALL parameter groups:
 *   1. sumsq = sum of (double)g * (double)g over every gradient element, the gradients still multiplied by the loss scale S
 *      (exact products; a sum of finite fp32 squares cannot overflow a double).  Accumulated in double in a FIXED order, no
 *      atomics: each thread its strided elements in index order, a 256-wide tree through LDS, one partial per workgroup, then
 *      the partials in index order by one workgroup and the same tree — the same bits run to run for the same addresses.
 *   2. norm = (float)(sqrt(sumsq) / (double)S): the L2 norm of the UN-scaled gradients before clipping (S a power of two).
 *   3. coef = (float)fmin((double)max_norm / ((double)norm + 1e-6), 1.0): evaluated in double from the fp32 norm and rounded
 *      once, so a host reproduces it bit for bit from norm.  max_norm = +inf: coef == 1.0f exactly (measure only).
 *   4. Adam reads g = grad * (1 / S); g = g * coef — two separately rounded fp32 multiplies — then weight decay and the rest as
 *      upf_adam_amsgrad_step.  The gradient tensors themselves are NOT modified (unlike torch): the coefficient is folded into
 *      the read.
 *   5. The non-finite flag is raised in the same pass, exactly as upf_grads_nonfinite_check raises it, and norm is non-finite
 *      IF AND ONLY IF the flag was raised (squares are >= 0: no inf - inf; finite squares cannot overflow).  On such a step
 *      Adam writes nothing; coef is then unspecified and is read by nothing that writes.
 *
 * upf_grads_sumsq_check: upf_grads_nonfinite_check plus partials[b] = the sum of squares of workgroup b's chunk, for the
 * launch's n_blocks workgroups (every one is written; 8-byte aligned device memory).  A step of several launches gives each
 * its own range of one vector: the count is host arithmetic over the launch plan (the sum of n_blocks). */
int upf_grads_sumsq_check(const upf_mt_launch* launch, double* partials /* n_blocks of them */, int* flag, void* stream);
/* One workgroup: sumsq = partials[0..n_partials) summed in the fixed order above; norm_out[0], coef_out[0] (fp32 DEVICE
 * scalars) as in 2. and 3. from the DEVICE scalar loss_scale[0].  UPF_EINVAL: a null pointer, n_partials <= 0, max_norm that is
 * not positive (NaN included). */
int upf_grad_norm_clip_coef(const double* partials, int n_partials, const float* loss_scale, float max_norm,
                            float* norm_out, float* coef_out, void* stream);
/* upf_adam_amsgrad_step with g = (grad / loss_scale[0]) * clip_coef[0] (4. above; clip_coef a DEVICE scalar, read only when
 * flag[0] == 0).  clip_coef[0] == 1.0f gives the bits of upf_adam_amsgrad_step. */
int upf_adam_amsgrad_step_clipped(const upf_mt_launch* launch, const float* lr, const float* step, const float* loss_scale,
                                  const float* clip_coef, const int* flag, double beta1, double beta2, double eps,
                                  double weight_decay, void* stream);
/* The end of a step, one thread (torch.amp.GradScaler.update with a floor):
 *   flag set:   loss_scale = max(loss_scale * backoff_factor, 1), growth_tracker = 0, skipped_steps += 1
 *   flag clear: steps[0..nsteps) += 1 (the step counters of the parameter groups), growth_tracker += 1, and when it reaches
 *               growth_interval: loss_scale *= growth_factor, growth_tracker = 0
 *   either way flag = 0.   growth_interval <= 0: a FIXED scale (loss_scale and growth_tracker are left alone; a non-finite
 *   step is still skipped and counted). */
int upf_loss_scale_update(float* loss_scale, int* growth_tracker, int* skipped_steps, int* flag, float* steps, int nsteps,
                          float growth_factor, float backoff_factor, int growth_interval, void* stream);

/* ---- batch assembly from uint8 frames ----------------------------------------------------------------------------------------
 * The host data path of the reference (dataset/kitti_dataset.py:62-80, 268-342: img_func.get_process_img_only_img — flip,
 * (image - mean) / stddev in float64, HWC -> CHW — then kitti_data_with_start_point.random_crop and the fp32 conversion) as ONE
 * launch:
 *   raw[b,c,y,x]  = (float)(((double)src[b, y, flip_b ? W-1-x : x, c] - mean_c) / stddev)     IEEE double, one rounding to fp32
 *   crop[b,c,i,j] = raw[b,c,y_b+i,x_b+j]            start[b] = (x_b, y_b)
 * src1 / src2 uint8 [B,H,W,3] contiguous (src2 may be NULL: one frame set; raw2 / crop2 are then ignored); raw1 / raw2 fp32
 * [B,3,H,W]; crop1 / crop2 fp32 [B,3,ph,pw] (ph = pw = 0: no crops, the pointers are ignored); start fp32 [B,2] or NULL.
 * aug int32 [B,3] = (x, y, flip) in DEVICE memory, read by the kernel (NULL: all zero): x is clamped to [0, W-pw], y to
 * [0, H-ph], flip is `!= 0`, and start reports the clamped values — no value of aug makes the kernel leave src or the outputs.
 * mean = 0,0,0 and stddev = 1 give the un-normalised frames (normalize=False).  Every source byte is read once; the frame and
 * its crop are written from the same pass.  UPF_EINVAL: non-positive sizes, a crop larger than the frame, null src1 / outputs;
 * UPF_EUNSUPPORTED: a batch item of 2 GiB or more. */
int upf_frames_u8_assemble(const unsigned char* src1, const unsigned char* src2, const int* aug, float* raw1, float* raw2,
                           float* crop1, float* crop2, float* start, int B, int H, int W, int ph, int pw,
                           double mean0, double mean1, double mean2, double stddev, void* stream);

/* The 16-bit inference ingest: both frame sets, normalised as above and rounded to nearest-even to fp16 / bf16 — the bits of
 * upf_frames_u8_assemble's raw frames followed by ATen's cast — stacked along the batch in ONE launch:
 *   x[n,c,y,x]     = (x_dtype)raw1[n,c,y,x]   for n < B,        x[n+B,c,y,x] = (x_dtype)raw2[n,c,y,x]
 *   xd, if not NULL: the same values in xd_dtype (the decoder's type where it differs from the pyramid's), from the same pass.
 * src1 / src2 uint8 [B,H,W,3] contiguous, at any byte address.  x / xd [2B,3,H,W] of UPF_F16 or UPF_BF16 (chosen independently;
 * UPF_EDTYPE otherwise), unit-stride rows, planes H * pitch elements apart, any batch stride >= 3 * H * pitch (elements).
 * pitch == W: contiguous rows, nothing outside [.., :W] is written.  Otherwise the pitch of ops.empty_nchw — a multiple of 8 with
 * fewer than 8 padding columns — and columns [W, pitch) of a row may receive anything; any other pitch is UPF_EINVAL.
 * flip int32 [B] in DEVICE memory or NULL: `!= 0` mirrors that item of both frame sets.  Eight consecutive values of a channel
 * are one 16-byte store wherever the destination is 16-byte aligned (every group of a pitched or W % 8 == 0 row of an aligned
 * buffer).  UPF_EALIGN: x / xd not 2-byte, flip not 4-byte aligned. */
int upf_frames_u8_stack16(const unsigned char* src1, const unsigned char* src2, const int* flip,
                          void* x, int x_dtype, long long x_pitch, long long x_batch_stride,
                          void* xd, int xd_dtype, long long xd_pitch, long long xd_batch_stride,
                          int B, int H, int W, double mean0, double mean1, double mean2, double stddev, void* stream);

/* ---- KITTI scoring from the uint16 ground truth --------------------------------------------------------------------------------
 * The evaluation metrics of the reference (dataset/kitti_dataset.py:379-499: flow_error_avg three times, outlier_pct once) of one
 * batch as ONE result row, from the prediction and the payload of the two KITTI flow PNGs as the files hold it:
 *   pred            fp32   [B,2,H,W] contiguous
 *   gt_occ, gt_noc  uint16 [B,H,W,3] contiguous: R = u*64 + 2^15, G = v*64 + 2^15, B = valid
 * Per pixel, every step ONE fp32 operation rounded to nearest (no contraction), sqrt the CORRECTLY ROUNDED fp32 square root:
 *   gu = (float)((int)R - 32768) * 0.015625f, gv likewise   (exact: the host path's float64 decode, rounded to fp32)
 *   m_occ = (float)(B_occ & 255), m_noc = (float)(B_noc & 255)                     (the host path's np.uint8() wraps)
 *   du = gu - pu, dv = gv - pv        (from gt_occ for the occ / F1 / occluded-only terms, from gt_noc for the noc term)
 *   e   = sqrt(du*du + dv*dv)
 *   thr = max(3.0f, sqrt(gu*gu + gv*gv) * 0.05f)              (gt_occ; 0.05 as fp32)
 *   d_occ = e_occ * m_occ;   outlier = d_occ > thr (never for a NaN);   w_oo = m_occ - m_noc  (negative where noc is not in occ)
 * Sums over the B*H*W pixels, float terms in double, masks and counts as exact integers:
 *   S_occ = sum d_occ, N_occ = sum m_occ, C_out = sum outlier, S_noc = sum e_noc*m_noc, N_noc = sum m_noc,
 *   S_oo = sum e_occ*w_oo, N_oo = sum w_oo
 *   row[0..12) = { S_occ/(N_occ+1e-6), C_out/N_occ*100, S_noc/(N_noc+1e-6), S_oo/(N_oo+1e-6),
 *                  S_occ, N_occ, C_out, S_noc, N_noc, S_oo, N_oo, (double)B }
 * (an empty mask: F1 = 0/0 = NaN and EPE = 0, as the reference; a NaN in pred makes the S sums it enters NaN.)  Why the square
 * root is pinned: the F1 count is made of `d_occ > thr` comparisons, and a 1-ulp square root (the native instruction, or torch's
 * vectorised CPU sqrt) flips the ones whose error sits on the threshold.
 * Two launches on `stream`: partial sums per workgroup into `workspace` (upf_kitti_score_workspace_bytes(B,H,W) bytes through
 * *bytes, 8-byte aligned), then one workgroup adds them in a fixed order and writes row — 12 doubles of DEVICE memory, e.g.
 * table + 12 * index; nothing else is written.  No atomics and no workgroup waits for another: the row is bit-reproducible run to
 * run.  UPF_EINVAL: null pointers, non-positive sizes; UPF_EUNSUPPORTED: 2^31 pixels or more; UPF_EALIGN: pred / workspace / row
 * not 8-byte, gt_occ / gt_noc not 4-byte aligned. */
int upf_kitti_score_workspace_bytes(int B, int H, int W, long long* bytes);
int upf_kitti_score(const float* pred, const unsigned short* gt_occ, const unsigned short* gt_noc, void* workspace,
                    double* row, int B, int H, int W, void* stream);

/* ---- evaluation results: KITTI PNG samples, Middlebury colours, .flo body ---------------------------------------------------------
 * What the reference's runner saves per pair (utils/tools.py:1342-1480 flow_to_image, :1482-1525 write_flow_png, :1556-1632
 * write_flo), as the PAYLOADS of the three files, from the prediction on the device:
 *   pred   fp32   [B,2,H,W] contiguous;   valid  fp32 [B,1,H,W] contiguous or NULL (= 1 everywhere)
 *   kitti  uint16 [B,H,W,3]   R, G = clip(double(x) * 64.0 + 32768.0, 0, 65535) truncated (the bits of flow_io.write_kitti_png_file's
 *                             encode; +-inf clamp), B = valid truncated to uint16 (saturating; NaN -> 0).  A NaN component of
 *                             the flow makes the pixel (0, 0, 0): the host's cast of a NaN is undefined, this is defined.
 *   rgb    uint8  [B,H,W,3]   flow_to_image as it evaluates for a float32 frame (below)
 *   flo    fp32   [B,H,W,2]   the two planes interleaved, bit for bit
 * Each output may be NULL (not wanted); all three NULL is UPF_EINVAL.
 * rgb.  In fp32, each step rounded on its own, sqrt correctly rounded: a pixel with |u| or |v| > 1e7 (unknown) or with a NaN
 * component is BLACK and counts as (0,0); maxrad = max over the ITEM of sqrt(u*u + v*v).  (The reference lets a NaN turn the whole
 * frame's scale into -1; here it is one black pixel.)  max_rad > 0 replaces maxrad for every item; max_rad <= 0 (or NaN) = per item.
 * Then in float64: d = double(maxrad) + 2^-52, u = double(u)/d, v likewise, rad = sqrt(u*u + v*v),
 *   fk = (atan2(-v,-u)/pi + 1)/2 * 54 + 1, k0 = floor(fk), k1 = k0 + 1 (56 -> 1), f = fk - k0,
 *   c = (1-f) * wheel[k0-1]/255 + f * wheel[k1-1]/255 per channel (the 55-entry Middlebury wheel: segments of 15, 6, 4, 11, 13, 6
 *   entries, ramps floor(255*i/n)),  c = rad <= 1 ? 1 - rad*(1-c) : c*0.75,  stored floor(255*c).
 * Every operation but atan2 is IEEE-exact, so a value differs from the host's only where the angle's last bit moves a floor.
 * Launches on `stream`: ONE when no per-item maximum is needed (rgb NULL, or max_rad > 0) — the workspace is then not touched and
 * may be NULL; else two: per-workgroup partial maxima into `workspace` (upf_flow_export_workspace_bytes(B,H,W) bytes through
 * *bytes), then every workgroup folds its item's and renders.  No atomics, no workgroup waits for another; nothing but the
 * requested outputs and the workspace is written; same bits run to run.  Four consecutive pixels per lane, moved with the widest
 * access the addresses allow (any H*W; 16-byte aligned bases and H*W % 4 == 0 give the widest).
 * UPF_EINVAL: null pred, no output, a needed workspace missing, non-positive sizes; UPF_EUNSUPPORTED: 2^31 pixels or more;
 * UPF_EALIGN: pred / valid / flo / workspace not 4-byte, kitti not 2-byte aligned. */
int upf_flow_export_workspace_bytes(int B, int H, int W, long long* bytes);
int upf_flow_export(const float* pred, const float* valid, unsigned short* kitti, unsigned char* rgb, float* flo,
                    float max_rad, void* workspace, int B, int H, int W, void* stream);

/* ---- PNG compression: filter, Huffman code, zlib stream ----------------------------------------------------------------------------
 * From the samples of B images — img uint8 (depth 8) or uint16 (depth 16) [B,H,W,C] contiguous, C in 1..4: the `kitti` and `rgb`
 * tensors of upf_flow_export — the complete zlib stream of each image's PNG, i.e. the body of its IDAT chunk:
 *   out      uint8 [B,cap]  slot b holds image b's stream from its first byte; the rest of the slot is zero
 *   lengths  int32 [B]      the stream's bytes; negative: the stream would not have fitted the slot and is not complete (cannot
 *                           happen with the cap below; nothing is ever written beyond a slot)
 * upf_png_encode_workspace_bytes gives the workspace's bytes and cap, the pitch of `out`: n + n/8 + 1024 rounded up to 16, where
 * n = H * (stride + 1), stride = W * C * depth / 8, is the length of the filtered stream.
 * The filtered stream is flow_io.write_png's: per row the filter type 2 (Up), then cur - above mod 256 over the big-endian sample
 * bytes; the first row has above = 0.  The zlib stream: 78 01; ONE final deflate block with dynamic Huffman codes, every symbol a
 * literal (no matches); the Adler-32, big-endian.  The block header: BFINAL 1, BTYPE 2, HLIT 0 (257 literal/length codes), HDIST 0
 * (one distance code, length 1, never used), HCLEN 15; the code-length code gives 4 bits to the symbols 0..15 and none to 16..18;
 * then 258 lengths of 4 bits.  The literal code, one per image, from the 256 byte counts and one end-of-block:
 *   Huffman: the symbols with a count sorted by (count, symbol), merged with two queues (the leaves; the nodes in the order they
 *     were made; on equal weights a leaf first); while the deepest leaf is beyond 15 bits every count becomes (count + 1) >> 1;
 *   flat: 9 bits for the two first symbols in (count, symbol) order over all 257, 8 bits for the rest;
 *   the flat code is taken when it costs strictly fewer bits over the true counts, so a stream is at most
 *   2 + ceil((1106 + 9 * (n + 1)) / 8) + 4 bytes <= cap.  Canonical codes (RFC 1951 3.2.2).
 * tests/_png_model.py states all of it in Python and gives the same bytes.  A constant image costs 1 bit per byte.
 * Three launches on `stream` (filter + counts + Adler sums per 4096-byte chunk; the code, per image; the packing per chunk); no
 * host synchronisation, no allocation, no workgroup waits for another; integer adds and ORs of disjoint bits only: the same bytes
 * run to run.  Nothing but `out`, `lengths` and the workspace is written.
 * UPF_EINVAL: null pointers, non-positive sizes, C outside 1..4, depth not 8 / 16; UPF_EUNSUPPORTED: a slot of 2^31 bytes or
 * more; UPF_EALIGN: img not sample-aligned, out / lengths not 4-byte, workspace not 16-byte aligned. */
int upf_png_encode_workspace_bytes(int B, int H, int W, int C, int depth, long long* bytes, long long* cap);
int upf_png_encode(const void* img, unsigned char* out, int* lengths, void* workspace, int B, int H, int W, int C, int depth,
                   void* stream);

/* ---- KITTI error maps from the uint16 ground truth ---------------------------------------------------------------------------------
 * The devkit's rendering of the end-point error against the ground truth, as the reference draws it (utils/tools.py:702-758,
 * lib_to_show_flow.flow_error_image_np), as the payload of an 8-bit RGB PNG:
 *   pred            fp32   [B,2,H,W] contiguous
 *   gt_occ, gt_noc  uint16 [B,H,W,3] contiguous, as upf_kitti_score takes them
 *   rgb             uint8  [B,H,W,3] R, G, B: what flow_io.write_png and upf_png_encode take as it is
 * Per pixel, every step ONE fp32 operation rounded to nearest (no contraction), the divisions IEEE divisions (never a reciprocal
 * multiply), sqrt the CORRECTLY ROUNDED fp32 square root:
 *   gu, gv, m_occ = (float)(B_occ & 255), m_noc = (float)(B_noc & 255) exactly as upf_kitti_score; the flow is gt_occ's
 *   diff = sqrt((pu-gu)*(pu-gu) + (pv-gv)*(pv-gv));   mag = sqrt(gu*gu + gv*gv)
 * log_colors != 0:  err = min(diff / 3.0f, (20.0f * diff) / (mag + 1e-7f)), min as numpy's minimum (a NaN on either side gives NaN);
 *   the colour is row i of the table, i the bin with lo[i] <= err < lo[i+1], lo = 0, 0.0625, 0.125, 0.25, 0.5, 1, 2, 4, 8, 16, 1e9:
 *     (49,54,149) (69,117,180) (116,173,209) (171,217,233) (224,243,248) (254,224,144) (253,174,97) (244,109,67) (215,48,39) (165,0,38)
 *   where m_noc == 1, else row i of the HALVED table — rint(255 * x) of what the reference returns, which stores float32(c/255)
 *   and halves that; a constant table of its own, never a formula —
 *     (25,27,75) (35,59,90) (58,87,105) (86,109,117) (112,122,124) (127,112,72) (127,87,49) (122,55,34) (108,24,20) (83,0,19)
 *   no bin (err NaN, +-inf or >= 1e9): BLACK, as the reference.  m_occ == 0: (0,0,0).
 * log_colors == 0:  e = min(diff, 5.0f) / 5.0f, b = rint((double)e * 255.0), a NaN gives 0;
 *   R = b where m_occ != 0; G = B = b where m_occ != 0 and m_noc == 1; 0 everywhere else.
 * Masks outside {0, 1}: a pixel is VALID when m_occ != 0 and NON-OCCLUDED when m_noc == 1.  The reference multiplies the image by
 * mask_occ, so for masks outside {0, 1} this is a deviation; KITTI files hold only 0 and 1.
 * dilate = r, 0 <= r <= 4 (not in the reference; KITTI ground truth is sparse and the plain map a dot pattern): a valid pixel keeps
 * its colour; an invalid pixel takes the colour of the valid pixel that comes LAST in raster order (greatest y', then greatest x')
 * within |y'-y| <= r, |x'-x| <= r inside the image; black when there is none.  r = 0 is the plain map.
 * ONE launch on `stream` for every r: r = 0 renders 4 consecutive pixels per lane with the widest access the addresses allow (any
 * H*W); r > 0 renders each 32 x 64 tile plus its halo once into LDS and resolves the windows there.  No workspace is needed:
 * upf_flow_error_image_workspace_bytes answers 0 and `workspace` may be NULL (both are kept so that a later form may need one).
 * No atomics, no workgroup waits for another; nothing but rgb is written; same bytes run to run.
 * UPF_EINVAL: null pointers, non-positive sizes, dilate outside 0..4, a needed workspace missing; UPF_EUNSUPPORTED: 2^31 pixels or
 * more; UPF_EALIGN: pred not 8-byte, gt_occ / gt_noc not 4-byte aligned (rgb: any address). */
int upf_flow_error_image_workspace_bytes(int B, int H, int W, int dilate, long long* bytes);
int upf_flow_error_image(const float* pred, const unsigned short* gt_occ, const unsigned short* gt_noc, unsigned char* rgb,
                         int log_colors, int dilate, void* workspace, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UPFLOW_HIP_H */
