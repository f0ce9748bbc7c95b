// Device-side optimiser step of the training loop: non-finite check of the gradients, Adam (amsgrad, L2 weight decay) with the
// loss scale divided out as the gradient is read, and the dynamic loss-scale state machine — all on the stream, no host
// synchronisation, so the whole of it is captured into the training step's hipGraph (include/upflow_hip.h has the contract).
// With a bound on the global gradient norm the check pass also takes the sum of squares (double, one partial per workgroup, a
// fixed-order finish: no atomics, the same bits run to run) and Adam multiplies the clip coefficient in where it reads the gradient.
//
// Multi-tensor launches: the tensors' addresses travel BY VALUE in the kernel arguments (upf_mt_launch, < 4 KB): the
// gradients of a captured step are allocated during the capture, and a host-to-device copy of a pointer table cannot be
// captured.  One workgroup takes one UPF_MT_CHUNK-element chunk of one tensor.
//
// Alignment: parameters and moments come from the allocator, but gradients under DDP are views into bucket storage — 4-byte
// aligned, odd lengths.  A workgroup whose five chunk addresses are all 16-byte aligned moves float4s and finishes the chunk's
// ragged end element by element; any other workgroup stays scalar per element (coalesced dwords).  The arithmetic per element
// is the same function either way, so the result does not depend on the route.
//
// Built with -ffp-contract=off: the operation order below is the one torch's multi-tensor Adam kernel compiles to (fp32 state,
// double hyper-parameters, every expression evaluated in double and rounded to fp32 where it is assigned).
#include "common.hpp"

namespace upf {
namespace optim {

constexpr int NT = 256;

static_assert(sizeof(upf_mt_launch) <= 3840, "upf_mt_launch and the scalar arguments must fit the 4 KB kernel-argument block");
static_assert(UPF_MT_TENSORS <= 256, "block_tensor is a byte");
static_assert(UPF_MT_CHUNK % (4 * NT) == 0, "a chunk is whole float4 rounds of the workgroup");

__device__ __forceinline__ int nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// ---- 1. any NaN / inf in the gradients -> *flag = 1 (plain store: every writer writes the same value) ---------------------
__global__ __launch_bounds__(NT) void nonfinite_kernel(const upf_mt_launch L, int* __restrict__ flag) {
  const int b = blockIdx.x;
  const int t = L.block_tensor[b];
  const long long first = (long long)L.block_chunk[b] * UPF_MT_CHUNK;
  const int n = (int)min((long long)UPF_MT_CHUNK, (long long)L.numel[t] - first);
  const float* __restrict__ g = (const float*)L.grad[t] + first;
  int bad = 0;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int n4 = n >> 2;
    const float4* __restrict__ g4 = (const float4*)g;
    for (int i = threadIdx.x; i < n4; i += NT) {
      const float4 v = g4[i];
      bad |= nonfinite(v.x) | nonfinite(v.y) | nonfinite(v.z) | nonfinite(v.w);
    }
    done = n4 << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += NT) bad |= nonfinite(g[i]);
  if (bad) *flag = 1;
}

// ---- 1b. the same pass with the sum of squares: partials[b] = sum over workgroup b's chunk of (double)g * (double)g ---------
// (the product of two fp32 values is exact in double; squares are >= 0 and a finite fp32 square is < 2^256, so the sum is
// non-finite if and only if an element is — the same condition the flag reports)
__device__ __forceinline__ double block_sum(double acc, double* s_red) {
  s_red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {                     // a fixed tree: the order does not depend on timing
    if ((int)threadIdx.x < w) s_red[threadIdx.x] = s_red[threadIdx.x] + s_red[threadIdx.x + w];
    __syncthreads();
  }
  return s_red[0];
}

__global__ __launch_bounds__(NT) void sumsq_check_kernel(const upf_mt_launch L, double* __restrict__ partials, int* __restrict__ flag) {
  __shared__ double s_red[NT];
  const int b = blockIdx.x;
  const int t = L.block_tensor[b];
  const long long first = (long long)L.block_chunk[b] * UPF_MT_CHUNK;
  const int n = (int)min((long long)UPF_MT_CHUNK, (long long)L.numel[t] - first);
  const float* __restrict__ g = (const float*)L.grad[t] + first;
  int bad = 0;
  int done = 0;
  double acc = 0.0;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int n4 = n >> 2;
    const float4* __restrict__ g4 = (const float4*)g;
    for (int i = threadIdx.x; i < n4; i += NT) {
      const float4 v = g4[i];
      bad |= nonfinite(v.x) | nonfinite(v.y) | nonfinite(v.z) | nonfinite(v.w);
      acc += (double)v.x * (double)v.x;
      acc += (double)v.y * (double)v.y;
      acc += (double)v.z * (double)v.z;
      acc += (double)v.w * (double)v.w;
    }
    done = n4 << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += NT) {
    const float v = g[i];
    bad |= nonfinite(v);
    acc += (double)v * (double)v;
  }
  if (bad) *flag = 1;
  const double total = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[b] = total;
}

// ---- 1c. one workgroup: the partials in index order -> norm of the UN-scaled gradients, clip coefficient ------------------
__global__ __launch_bounds__(NT) void norm_finish_kernel(const double* __restrict__ partials, int n_partials,
                                                         const float* __restrict__ scale_p, float max_norm,
                                                         float* __restrict__ norm_out, float* __restrict__ coef_out) {
  __shared__ double s_red[NT];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += NT) acc += partials[i];
  const double sumsq = block_sum(acc, s_red);
  if (threadIdx.x == 0) {
    const float norm = (float)(sqrt(sumsq) / (double)scale_p[0]);            // (S a power of two: the division is exact)
    norm_out[0] = norm;
    coef_out[0] = (float)fmin((double)max_norm / ((double)norm + 1e-6), 1.0);  // torch's max_norm / (total_norm + 1e-6), clamped
  }
}

// ---- 2. Adam + amsgrad + L2 weight decay (torch/optim/adam.py, the capturable form) -----------------------------------------
struct Hyper {
  double beta1, beta2, eps, weight_decay;
};
static_assert(sizeof(upf_mt_launch) + sizeof(Hyper) + 5 * sizeof(void*) <= 4096, "the clipped Adam launch: table, Hyper, five pointers");

// one element; lr, bc1, bc2_sqrt as torch's kernel holds them (lr double from the device float, the corrections fp32)
// CLIP: the gradient is multiplied by the clip coefficient after the un-scaling (two separately rounded fp32 multiplies)
template <bool CLIP>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float& vmax, const Hyper& h, float inv_scale,
                                             float coef, double lr, float bc1, float bc2_sqrt) {
  g = g * inv_scale;                                        // (a power of two: exact)
  if (CLIP) g = g * coef;
  if (h.weight_decay != 0.0) g = (float)(g + p * h.weight_decay);
  const double w = 1.0 - h.beta1;                           // lerp(m, g, 1 - beta1)
  m = w < 0.5 ? (float)(m + w * (g - m)) : (float)(g - (g - m) * (1.0 - w));
  v = (float)(h.beta2 * v + (1.0 - h.beta2) * g * g);
  const float step_size = (float)(lr / bc1);
  vmax = fmaxf(vmax, v);
  const float denom = (float)((sqrtf(vmax) / bc2_sqrt) + h.eps);
  p = p - step_size * m / denom;
}

// the body of both Adam kernels; coef_p is read when CLIP only (the unclipped launch does not carry it)
template <bool CLIP>
__device__ __forceinline__ void adam_body(const upf_mt_launch& L, const Hyper& h, const float* __restrict__ lr_p,
                                          const float* __restrict__ step_p, const float* __restrict__ scale_p,
                                          const float* __restrict__ coef_p, const int* __restrict__ flag) {
  // a non-finite gradient anywhere: this step changes nothing (the flag is uniform over the grid: the check ran before, the
  // state machine that clears it runs after)
  if (*flag != 0) return;
  __shared__ float s_bc[2];
  if (threadIdx.x == 0) {
    const double step = (double)step_p[0] + 1.0;            // (the counter itself is advanced by upf_loss_scale_update)
    s_bc[0] = (float)(1.0 - pow(h.beta1, step));
    const float bc2 = (float)(1.0 - pow(h.beta2, step));
    s_bc[1] = sqrtf(bc2);
  }
  __syncthreads();
  const float bc1 = s_bc[0], bc2_sqrt = s_bc[1];
  const double lr = (double)lr_p[0];
  const float inv_scale = 1.f / scale_p[0];
  const float coef = CLIP ? coef_p[0] : 1.f;                // (read only behind the flag: unspecified on a non-finite step)

  const int b = blockIdx.x;
  const int t = L.block_tensor[b];
  const long long first = (long long)L.block_chunk[b] * UPF_MT_CHUNK;
  const int n = (int)min((long long)UPF_MT_CHUNK, (long long)L.numel[t] - first);
  float* __restrict__ p = (float*)L.param[t] + first;
  const float* __restrict__ g = (const float*)L.grad[t] + first;
  float* __restrict__ m = (float*)L.exp_avg[t] + first;
  float* __restrict__ v = (float*)L.exp_avg_sq[t] + first;
  float* __restrict__ x = (float*)L.max_exp_avg_sq[t] + first;
  int done = 0;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                         reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(x);
  if ((bits & 15) == 0) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += NT) {
      float4 P = ((float4*)p)[i], M = ((float4*)m)[i], V = ((float4*)v)[i], X = ((float4*)x)[i];
      const float4 G = ((const float4*)g)[i];
      adam_element<CLIP>(P.x, G.x, M.x, V.x, X.x, h, inv_scale, coef, lr, bc1, bc2_sqrt);
      adam_element<CLIP>(P.y, G.y, M.y, V.y, X.y, h, inv_scale, coef, lr, bc1, bc2_sqrt);
      adam_element<CLIP>(P.z, G.z, M.z, V.z, X.z, h, inv_scale, coef, lr, bc1, bc2_sqrt);
      adam_element<CLIP>(P.w, G.w, M.w, V.w, X.w, h, inv_scale, coef, lr, bc1, bc2_sqrt);
      ((float4*)p)[i] = P;
      ((float4*)m)[i] = M;
      ((float4*)v)[i] = V;
      ((float4*)x)[i] = X;
    }
    done = n4 << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += NT) {
    float P = p[i], M = m[i], V = v[i], X = x[i];
    adam_element<CLIP>(P, g[i], M, V, X, h, inv_scale, coef, lr, bc1, bc2_sqrt);
    p[i] = P;
    m[i] = M;
    v[i] = V;
    x[i] = X;
  }
}

__global__ __launch_bounds__(NT) void adam_kernel(const upf_mt_launch L, const Hyper h, const float* __restrict__ lr_p,
                                                  const float* __restrict__ step_p, const float* __restrict__ scale_p,
                                                  const int* __restrict__ flag) {
  adam_body<false>(L, h, lr_p, step_p, scale_p, nullptr, flag);
}

// (one more pointer in the argument block: 3400 + 32 + 5 * 8 bytes, inside the static_assert above)
__global__ __launch_bounds__(NT) void adam_clipped_kernel(const upf_mt_launch L, const Hyper h, const float* __restrict__ lr_p,
                                                          const float* __restrict__ step_p, const float* __restrict__ scale_p,
                                                          const float* __restrict__ coef_p, const int* __restrict__ flag) {
  adam_body<true>(L, h, lr_p, step_p, scale_p, coef_p, flag);
}

// ---- 3. the loss-scale state machine (torch.amp.GradScaler.update, with a floor of 1), one thread ------------------------
__global__ void scale_update_kernel(float* __restrict__ scale, int* __restrict__ tracker, int* __restrict__ skipped,
                                    int* __restrict__ flag, float* __restrict__ steps, int nsteps, float growth, float backoff,
                                    int interval) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (*flag != 0) {
    if (interval > 0) {
      *scale = fmaxf(*scale * backoff, 1.f);
      *tracker = 0;
    }
    *skipped += 1;
  } else {
    for (int i = 0; i < nsteps; ++i) steps[i] += 1.f;
    if (interval > 0) {
      const int tr = *tracker + 1;
      if (tr >= interval) {
        *scale = *scale * growth;
        *tracker = 0;
      } else {
        *tracker = tr;
      }
    }
  }
  *flag = 0;
}

static int check_plan(const upf_mt_launch* L, const char* what, bool all_lists) {
  UPF_REQUIRE(L, UPF_EINVAL, "%s: null launch table", what);
  UPF_REQUIRE(L->n_tensors > 0 && L->n_tensors <= UPF_MT_TENSORS && L->n_blocks > 0 && L->n_blocks <= UPF_MT_BLOCKS, UPF_EINVAL,
              "%s: %d tensors / %d workgroups outside the table (%d / %d)", what, L->n_tensors, L->n_blocks, UPF_MT_TENSORS, UPF_MT_BLOCKS);
  for (int t = 0; t < L->n_tensors; ++t) {
    UPF_REQUIRE(L->numel[t] > 0, UPF_EINVAL, "%s: tensor %d has %d elements", what, t, L->numel[t]);
    UPF_REQUIRE(L->grad[t] && aligned_to(L->grad[t], 4), UPF_EINVAL, "%s: gradient %d is null or not 4-byte aligned", what, t);
    if (all_lists)
      UPF_REQUIRE(L->param[t] && L->exp_avg[t] && L->exp_avg_sq[t] && L->max_exp_avg_sq[t] && aligned_to(L->param[t], 4) &&
                      aligned_to(L->exp_avg[t], 4) && aligned_to(L->exp_avg_sq[t], 4) && aligned_to(L->max_exp_avg_sq[t], 4),
                  UPF_EINVAL, "%s: parameter / moment pointer %d is null or not 4-byte aligned", what, t);
  }
  // every workgroup's chunk must START inside its tensor: that is what bounds every address the kernels form
  for (int b = 0; b < L->n_blocks; ++b) {
    const int t = L->block_tensor[b];
    UPF_REQUIRE(t < L->n_tensors && L->block_chunk[b] >= 0 && (long long)L->block_chunk[b] * UPF_MT_CHUNK < L->numel[t], UPF_EINVAL,
                "%s: workgroup %d addresses chunk %d of tensor %d (%d elements)", what, b, L->block_chunk[b], t,
                t < L->n_tensors ? L->numel[t] : -1);
  }
  return UPF_OK;
}

}  // namespace optim
}  // namespace upf

extern "C" int upf_grads_nonfinite_check(const upf_mt_launch* launch, int* flag, void* stream) {
  using namespace upf;
  UPF_REQUIRE(flag, UPF_EINVAL, "grads_nonfinite_check: null flag");
  if (int rc = optim::check_plan(launch, "grads_nonfinite_check", false)) return rc;
  hipLaunchKernelGGL(optim::nonfinite_kernel, dim3(launch->n_blocks), dim3(optim::NT), 0, (hipStream_t)stream, *launch, flag);
  return check_launch("grads_nonfinite_check");
}

extern "C" int upf_adam_amsgrad_step(const upf_mt_launch* launch, const float* lr, const float* step, const float* loss_scale,
                                     const int* flag, double beta1, double beta2, double eps, double weight_decay, void* stream) {
  using namespace upf;
  UPF_REQUIRE(lr && step && loss_scale && flag, UPF_EINVAL, "adam_amsgrad_step: null pointer");
  UPF_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0, UPF_EINVAL,
              "adam_amsgrad_step: betas in [0, 1), eps and weight_decay >= 0");
  if (int rc = optim::check_plan(launch, "adam_amsgrad_step", true)) return rc;
  const optim::Hyper h{beta1, beta2, eps, weight_decay};
  hipLaunchKernelGGL(optim::adam_kernel, dim3(launch->n_blocks), dim3(optim::NT), 0, (hipStream_t)stream, *launch, h, lr, step,
                     loss_scale, flag);
  return check_launch("adam_amsgrad_step");
}

extern "C" int upf_grads_sumsq_check(const upf_mt_launch* launch, double* partials, int* flag, void* stream) {
  using namespace upf;
  UPF_REQUIRE(partials && flag, UPF_EINVAL, "grads_sumsq_check: null pointer");
  UPF_REQUIRE(aligned_to(partials, 8), UPF_EINVAL, "grads_sumsq_check: partials not 8-byte aligned");
  if (int rc = optim::check_plan(launch, "grads_sumsq_check", false)) return rc;
  hipLaunchKernelGGL(optim::sumsq_check_kernel, dim3(launch->n_blocks), dim3(optim::NT), 0, (hipStream_t)stream, *launch, partials,
                     flag);
  return check_launch("grads_sumsq_check");
}

extern "C" int upf_grad_norm_clip_coef(const double* partials, int n_partials, const float* loss_scale, float max_norm,
                                       float* norm_out, float* coef_out, void* stream) {
  using namespace upf;
  UPF_REQUIRE(partials && loss_scale && norm_out && coef_out, UPF_EINVAL, "grad_norm_clip_coef: null pointer");
  UPF_REQUIRE(n_partials > 0, UPF_EINVAL, "grad_norm_clip_coef: %d partials", n_partials);
  UPF_REQUIRE(max_norm > 0.f, UPF_EINVAL, "grad_norm_clip_coef: max_norm must be positive (+inf: measure only)");
  hipLaunchKernelGGL(optim::norm_finish_kernel, dim3(1), dim3(optim::NT), 0, (hipStream_t)stream, partials, n_partials, loss_scale,
                     max_norm, norm_out, coef_out);
  return check_launch("grad_norm_clip_coef");
}

extern "C" int upf_adam_amsgrad_step_clipped(const upf_mt_launch* launch, const float* lr, const float* step, const float* loss_scale,
                                             const float* clip_coef, const int* flag, double beta1, double beta2, double eps,
                                             double weight_decay, void* stream) {
  using namespace upf;
  UPF_REQUIRE(lr && step && loss_scale && clip_coef && flag, UPF_EINVAL, "adam_amsgrad_step_clipped: null pointer");
  UPF_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0, UPF_EINVAL,
              "adam_amsgrad_step_clipped: betas in [0, 1), eps and weight_decay >= 0");
  if (int rc = optim::check_plan(launch, "adam_amsgrad_step_clipped", true)) return rc;
  const optim::Hyper h{beta1, beta2, eps, weight_decay};
  hipLaunchKernelGGL(optim::adam_clipped_kernel, dim3(launch->n_blocks), dim3(optim::NT), 0, (hipStream_t)stream, *launch, h, lr, step,
                     loss_scale, clip_coef, flag);
  return check_launch("adam_amsgrad_step_clipped");
}

extern "C" int upf_loss_scale_update(float* loss_scale, int* growth_tracker, int* skipped_steps, int* flag, float* steps, int nsteps,
                                     float growth_factor, float backoff_factor, int growth_interval, void* stream) {
  using namespace upf;
  UPF_REQUIRE(loss_scale && growth_tracker && skipped_steps && flag && (steps || nsteps == 0) && nsteps >= 0, UPF_EINVAL,
              "loss_scale_update: null pointer");
  UPF_REQUIRE(growth_interval <= 0 || (growth_factor >= 1.f && backoff_factor > 0.f && backoff_factor <= 1.f), UPF_EINVAL,
              "loss_scale_update: growth_factor >= 1 and 0 < backoff_factor <= 1");
  hipLaunchKernelGGL(optim::scale_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss_scale, growth_tracker, skipped_steps,
                     flag, steps, nsteps, growth_factor, backoff_factor, growth_interval);
  return check_launch("loss_scale_update");
}
