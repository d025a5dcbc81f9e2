// Fused multi-tensor Adam step: the optimizer the
// reference builds at main_mp.py:92 (torch.optim.Adam(policy.parameters(),
// lr=1e-3)) and steps at main_mp.py:78, as ONE launch over every parameter
// tensor instead of torch's per-op foreach kernels (lerp, mul, addcmul, sqrt,
// div, add, addcdiv = 7 passes over the optimizer state).
//
// Per element, in the op order of torch's _multi_tensor_adam (fp32 opmath):
//   g  = grad (+ weight_decay * p)          (-grad when maximize)
//   m  = lerp(m, g, 1 - beta1)
//   v  = v * beta2 + (1 - beta2) * g * g
//   vm = max(vmax, v) when amsgrad (vmax <- vm), else v
//   p  = p + (-lr / (1 - beta1^step)) * m / (sqrt(vm) / sqrt(1 - beta2^step) + eps)
// The step-dependent scalars are computed in double and rounded to fp32 once,
// as torch does: on the host from the caller's step, or -- with a device step
// counter (aaa_adam_step_counted) -- by each workgroup from that counter, so a
// step the guard skipped does not advance the bias corrections.  HBM traffic: 16 B read + 12 B written per element
// (20 + 16 with amsgrad) -- the kernel is bound by HBM (or Infinity Cache)
// bandwidth, so it streams 16-byte vectors, 4 per thread.
#include <cmath>

#include "common.h"
#include "optim.h"

namespace aaa {

struct AdamScalars {
  float wd, one_m_b1, b2, one_m_b2, step_size_neg, bc2_sqrt, eps;
  int amsgrad, maximize;
  const float* guard;   // skip the whole update when *guard != 0 (aaa_adam_step_guarded), or nullptr
  const int* step_dev;  // device step counter (aaa_adam_step_counted), or nullptr: the scalars above hold
  const float* stats;   // k_gradsq_finish's stats (aaa_adam_step_clipped), read only by k_adam<true>
  double lr, beta1, beta2;   // the host's doubles (torch's Python floats), read only with step_dev
};

// Bias-corrected scalars of update number *step_dev + 1, in double as on the host.
__device__ __forceinline__ void adam_device_step(AdamScalars& s) {
  const double step = (double)(*s.step_dev) + 1.0;
  s.step_size_neg = (float)(-(s.lr / (1.0 - pow(s.beta1, step))));
  s.bc2_sqrt = (float)sqrt(1.0 - pow(s.beta2, step));
}

__device__ __forceinline__ float adam_elem(float& p, float g, float& m, float& v, float* vmax, const AdamScalars& s) {
  if (s.maximize) g = -g;
  if (s.wd != 0.f) g = g + s.wd * p;
  // torch lerp: weight < 0.5 -> self + w * (end - self)
  m = m + s.one_m_b1 * (g - m);
  v = v * s.b2;
  v = v + s.one_m_b2 * g * g;
  float vv = v;
  if (vmax) { vv = fmaxf(*vmax, v); *vmax = vv; }
  const float denom = sqrtf(vv) / s.bc2_sqrt + s.eps;
  p = p + s.step_size_neg * (m / denom);
  return p;
}

constexpr int kAdamThreads = 256;
constexpr int kAdamVec = 4;                                   // floats per 16-byte access
constexpr int kAdamChunk = kAdamThreads * kAdamVec * 4;       // elements per workgroup

// The chunk walk of every multi-tensor kernel here.  Workgroup -> (tensor,
// chunk) through the chunk prefix table, then the chunk's elements in a fixed
// order (k_gradsq's per-thread sum is defined by it): a tensor whose streams
// are all 16-byte aligned in 4 rounds of 16-byte accesses, a vector short of
// the end element by element by the same thread; any other tensor in 16
// scalar rounds.  vec4(S, i): the caller's work on elements [i, i + 4) of
// the tensor's streams S; one(S, j): the same on element j.
template <int K, class Vec4, class One>
__device__ __forceinline__ void chunk_walk(const TensorTable<K>& tab, Vec4&& vec4, One&& one) {
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < tab.n && tab.chunk0[t + 1] <= b) ++t;
  const size_t n = tab.numel[t];
  const size_t base = (size_t)(b - tab.chunk0[t]) * kAdamChunk;
  float* S[K];
#pragma unroll
  for (int k = 0; k < K; ++k) S[k] = tab.s[k][t];
  if (tab.vec[t]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t i = base + ((size_t)r * kAdamThreads + threadIdx.x) * kAdamVec;
      if (i + kAdamVec <= n) {
        vec4(S, i);
      } else {
        for (size_t j = i; j < n; ++j) one(S, j);
      }
    }
  } else {
    for (int r = 0; r < kAdamVec * 4; ++r) {
      const size_t j = base + (size_t)r * kAdamThreads + threadIdx.x;
      if (j < n) one(S, j);
    }
  }
}

// The walk for a body stated once, elem(x) on one element's values x[K].
// kLoad / kStore: the streams read into x before it and written back after
// it, one bit per stream; a stream not loaded is 0 in x and never touched.
template <unsigned kLoad, unsigned kStore, int K, class Elem>
__device__ __forceinline__ void chunk_walk_elem(const TensorTable<K>& tab, Elem&& elem) {
  chunk_walk(
      tab,
      [&](float* const (&S)[K], size_t i) {
        f32x4 v[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
          v[k] = (kLoad >> k & 1) ? *reinterpret_cast<const f32x4*>(S[k] + i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float x[K];
#pragma unroll
          for (int k = 0; k < K; ++k) x[k] = v[k][e];
          elem(x);
#pragma unroll
          for (int k = 0; k < K; ++k) v[k][e] = x[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (kStore >> k & 1) *reinterpret_cast<f32x4*>(S[k] + i) = v[k];
      },
      [&](float* const (&S)[K], size_t j) {
        float x[K];
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = (kLoad >> k & 1) ? S[k][j] : 0.f;
        elem(x);
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (kStore >> k & 1) S[k][j] = x[k];
      });
}

constexpr unsigned stream_bit(int k) { return 1u << k; }

// One workgroup's chunk of one tensor.  kScale: the gradient is grad * coef,
// rounded to fp32 before anything else reads it (grad.mul_(coef)): __fmul_rn
// keeps the product out of a contraction with adam_elem's first add.
// max_exp_avg_sq is there or not at run time, so Adam gives the walk its own
// two forms; which multiply of adam_elem fuses with which add follows from
// how the compiler packs exactly these forms, so they stay as they are.
template <bool kScale>
__device__ __forceinline__ void adam_chunk(const TensorTable<5>& tab, const AdamScalars& s, float coef) {
  auto grad = [&](float g) { return kScale ? __fmul_rn(g, coef) : g; };
  chunk_walk(
      tab,
      [&](float* const (&S)[5], size_t i) {
        float* X = S[kMaxExpAvgSq];
        f32x4 p = *reinterpret_cast<const f32x4*>(S[kParam] + i);
        const f32x4 g = *reinterpret_cast<const f32x4*>(S[kGrad] + i);
        f32x4 m = *reinterpret_cast<const f32x4*>(S[kExpAvg] + i);
        f32x4 v = *reinterpret_cast<const f32x4*>(S[kExpAvgSq] + i);
        f32x4 x = X ? *reinterpret_cast<const f32x4*>(X + i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = p[e], me = m[e], ve = v[e], xe = x[e];
          adam_elem(pe, grad(g[e]), me, ve, X ? &xe : nullptr, s);
          p[e] = pe; m[e] = me; v[e] = ve; x[e] = xe;
        }
        *reinterpret_cast<f32x4*>(S[kParam] + i) = p;
        *reinterpret_cast<f32x4*>(S[kExpAvg] + i) = m;
        *reinterpret_cast<f32x4*>(S[kExpAvgSq] + i) = v;
        if (X) *reinterpret_cast<f32x4*>(X + i) = x;
      },
      [&](float* const (&S)[5], size_t j) {
        float* X = S[kMaxExpAvgSq];
        adam_elem(S[kParam][j], grad(S[kGrad][j]), S[kExpAvg][j], S[kExpAvgSq][j], X ? X + j : nullptr, s);
      });
}

// kClip (aaa_adam_step_clipped): no update either when the gradient norm was
// not finite (stats[2]); otherwise the gradient is grad * stats[1].  The
// coefficient is the same for the whole grid, so a step the clip leaves alone
// (exactly 1.0f) takes the unscaled path.
template <bool kClip>
__global__ void __launch_bounds__(kAdamThreads) k_adam(TensorTable<5> tab, AdamScalars s) {
  if (s.guard && *s.guard != 0.f) return;   // gradients of a stranded launch: no update on any rank
  float coef = 1.f;
  if (kClip) {
    if (s.stats[2] != 0.f) return;          // an inf or NaN gradient: no update on any rank
    coef = s.stats[1];
  }
  if (s.step_dev) adam_device_step(s);
  if (kClip && coef != 1.f) adam_chunk<true>(tab, s, coef);
  else adam_chunk<false>(tab, s, 1.f);
}

// After k_adam in stream order: count the update iff the guard (and, clipped, the norm's flag) let it through.
__global__ void k_adam_advance(const float* __restrict__ guard, const float* __restrict__ stats,
                               int* __restrict__ step_dev) {
  if (threadIdx.x == 0 && !(guard && *guard != 0.f) && !(stats && stats[2] != 0.f)) step_dev[0] = step_dev[0] + 1;
}

hipError_t adam_launch(const TensorTable<5>& tab, int nchunks, const AdamHost& h, hipStream_t st, bool advance) {
  AdamScalars s;
  s.wd = (float)h.weight_decay;
  s.one_m_b1 = (float)(1.0 - h.beta1);
  s.b2 = (float)h.beta2;
  s.one_m_b2 = (float)(1.0 - h.beta2);
  s.step_size_neg = (float)(-(h.lr / (1.0 - std::pow(h.beta1, (double)h.step))));
  s.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(h.beta2, (double)h.step));
  s.eps = (float)h.eps;
  s.amsgrad = h.amsgrad;
  s.maximize = h.maximize;
  s.guard = h.guard;
  s.step_dev = h.step_dev;
  s.stats = h.stats;
  s.lr = h.lr;
  s.beta1 = h.beta1;
  s.beta2 = h.beta2;
  if (nchunks > 0) {
    if (h.stats) hipLaunchKernelGGL(k_adam<true>, dim3(nchunks), dim3(kAdamThreads), 0, st, tab, s);
    else hipLaunchKernelGGL(k_adam<false>, dim3(nchunks), dim3(kAdamThreads), 0, st, tab, s);
  }
  if (h.step_dev && advance)
    hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(64), 0, st, h.guard, h.stats, h.step_dev);
  return hipGetLastError();
}

// ---- RMSProp (aaa_rmsprop_step) ----
// torch.optim.RMSprop's _single_tensor_rmsprop per element, in fp32 (the op
// order is in include/aaa.h), with k_adam's structure, guard, clip and device
// step counter.  The learning rate follows a linear anneal over the updates
// APPLIED so far, so a skipped step does not move the schedule.  HBM traffic
// of IMPALA's variant (momentum 0, not centered): 12 B read + 8 B written per
// element; 4 + 4 more for each of the momentum buffer and grad_avg.
struct RmspropScalars {
  float wd, alpha, one_m_alpha, eps, momentum, lr_t;
  int maximize, eps_in_sqrt;
  const float* guard;
  const int* step_dev;       // or nullptr: lr_t above holds
  const float* stats;        // read only by k_rmsprop<true, ., .>
  double lr, lr_end;         // the host's doubles, read only with step_dev
  long anneal_steps;
};

// The lr of the update after n applied ones, in double.  One statement for the
// host count and the device count; no contraction, so both round alike.
__host__ __device__ inline double rmsprop_lr(double lr, double lr_end, long anneal_steps, double n) {
#pragma clang fp contract(off)
  if (anneal_steps <= 0) return lr;
  double f = 1.0 - n / (double)anneal_steps;
  if (f < 0.0) f = 0.0;
  return lr_end + (lr - lr_end) * f;
}

template <bool kMom, bool kCent>
__device__ __forceinline__ void rmsprop_elem(float& p, float g, float& v, float& b, float& a, const RmspropScalars& s) {
  if (s.maximize) g = -g;
  if (s.wd != 0.f) g = g + s.wd * p;
  v = v * s.alpha;
  v = v + s.one_m_alpha * g * g;
  float sq = v;
  if (kCent) {
    a = a + s.one_m_alpha * (g - a);   // torch lerp, weight < 0.5
    sq = v - a * a;
  }
  const float avg = s.eps_in_sqrt ? sqrtf(sq + s.eps) : sqrtf(sq) + s.eps;
  if (kMom) {
    b = b * s.momentum + g / avg;
    p = p - s.lr_t * b;
  } else {
    p = p - s.lr_t * (g / avg);
  }
}

// One workgroup's chunk of one tensor; kScale as in adam_chunk.  The momentum buffer is touched only with kMom, grad_avg only with kCent.
template <bool kScale, bool kMom, bool kCent>
__device__ __forceinline__ void rmsprop_chunk(const TensorTable<5>& tab, const RmspropScalars& s, float coef) {
  constexpr unsigned kState = stream_bit(kParam) | stream_bit(kSquareAvg) | (kMom ? stream_bit(kMomentumBuf) : 0u) |
                              (kCent ? stream_bit(kGradAvg) : 0u);
  chunk_walk_elem<kState | stream_bit(kGrad), kState>(tab, [&](float (&x)[5]) {
    rmsprop_elem<kMom, kCent>(x[kParam], kScale ? __fmul_rn(x[kGrad], coef) : x[kGrad], x[kSquareAvg],
                              x[kMomentumBuf], x[kGradAvg], s);
  });
}

// k_adam's skips, in its order: the guard, then (kClip) the norm's flag, both before any load.
template <bool kClip, bool kMom, bool kCent>
__global__ void __launch_bounds__(kAdamThreads) k_rmsprop(TensorTable<5> tab, RmspropScalars s) {
  if (s.guard && *s.guard != 0.f) return;
  float coef = 1.f;
  if (kClip) {
    if (s.stats[2] != 0.f) return;
    coef = s.stats[1];
  }
  if (s.step_dev) s.lr_t = (float)rmsprop_lr(s.lr, s.lr_end, s.anneal_steps, (double)(*s.step_dev));
  if (kClip && coef != 1.f) rmsprop_chunk<true, kMom, kCent>(tab, s, coef);
  else rmsprop_chunk<false, kMom, kCent>(tab, s, 1.f);
}

template <bool kClip, bool kMom>
static void rmsprop_dispatch(bool cent, int nchunks, hipStream_t st, const TensorTable<5>& tab, const RmspropScalars& s) {
  if (cent) hipLaunchKernelGGL((k_rmsprop<kClip, kMom, true>), dim3(nchunks), dim3(kAdamThreads), 0, st, tab, s);
  else hipLaunchKernelGGL((k_rmsprop<kClip, kMom, false>), dim3(nchunks), dim3(kAdamThreads), 0, st, tab, s);
}

hipError_t rmsprop_launch(const TensorTable<5>& tab, int nchunks, const RmspropHost& h, hipStream_t st, bool advance) {
  RmspropScalars s;
  s.wd = (float)h.weight_decay;
  s.alpha = (float)h.alpha;
  s.one_m_alpha = (float)(1.0 - h.alpha);
  s.eps = (float)h.eps;
  s.momentum = (float)h.momentum;
  s.lr_t = (float)rmsprop_lr(h.lr, h.lr_end, h.anneal_steps, (double)(h.step - 1));
  s.maximize = h.maximize;
  s.eps_in_sqrt = h.eps_in_sqrt;
  s.guard = h.guard;
  s.step_dev = h.step_dev;
  s.stats = h.stats;
  s.lr = h.lr;
  s.lr_end = h.lr_end;
  s.anneal_steps = h.anneal_steps;
  if (nchunks > 0) {
    const bool mom = h.momentum > 0.0, cent = h.centered != 0;
    if (h.stats) {
      if (mom) rmsprop_dispatch<true, true>(cent, nchunks, st, tab, s);
      else rmsprop_dispatch<true, false>(cent, nchunks, st, tab, s);
    } else {
      if (mom) rmsprop_dispatch<false, true>(cent, nchunks, st, tab, s);
      else rmsprop_dispatch<false, false>(cent, nchunks, st, tab, s);
    }
  }
  if (h.step_dev && advance)
    hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(64), 0, st, h.guard, h.stats, h.step_dev);
  return hipGetLastError();
}

// ---- global gradient norm (aaa_grad_norm) ----
// sum g^2 over every tensor, in double: the product of two fp32 values is
// exact there, so the only rounding is the summation's (N * 2^-53 relative,
// far inside half an fp32 ulp of the norm for any order).  The order is fixed
// all the same -- per thread, then the wave's butterfly, then the 4 waves,
// then the partials -- so identical buffers give bit-identical stats: the
// ranks of a data-parallel learner decide alike without a collective.  No
// atomics; one double per workgroup goes to scratch[chunk].
__device__ __forceinline__ double wg_sum_fixed(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);   // a + b == b + a: every lane holds the same sum
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(kAdamThreads) k_gradsq(TensorTable<1> tab, double* __restrict__ scratch, int chunk_base) {
  __shared__ double red[kAdamThreads / 64];
  double acc = 0.0;
  chunk_walk_elem<stream_bit(kGradOnly), 0u>(tab, [&](float (&x)[1]) { acc += (double)x[0] * (double)x[0]; });
  const double tot = wg_sum_fixed(acc, red);
  if (threadIdx.x == 0) scratch[(size_t)chunk_base + blockIdx.x] = tot;
}

// One workgroup: the partials in a fixed order, then the four stats (include/aaa.h).
__global__ void __launch_bounds__(kAdamThreads) k_gradsq_finish(const double* __restrict__ scratch, int nchunks,
                                                                 double max_norm, float* __restrict__ stats) {
  __shared__ double red[kAdamThreads / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nchunks; i += kAdamThreads) acc += scratch[i];
  const double norm = sqrt(wg_sum_fixed(acc, red));
  if (threadIdx.x == 0) {
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0); a NaN stays NaN
    const double c = max_norm / (norm + 1e-6);
    f32x4 o;
    o[0] = (float)norm;
    o[1] = (float)(c > 1.0 ? 1.0 : c);
    o[2] = isfinite(norm) ? 0.f : 1.f;
    o[3] = (float)max_norm;
    *reinterpret_cast<f32x4*>(stats) = o;
  }
}

hipError_t gradsq_launch(const TensorTable<1>& tab, int nchunks, int chunk_base, double* scratch, hipStream_t st) {
  if (nchunks > 0) hipLaunchKernelGGL(k_gradsq, dim3(nchunks), dim3(kAdamThreads), 0, st, tab, scratch, chunk_base);
  return hipGetLastError();
}

hipError_t gradsq_finish_launch(const double* scratch, int nchunks, double max_norm, float* stats, hipStream_t st) {
  hipLaunchKernelGGL(k_gradsq_finish, dim3(1), dim3(kAdamThreads), 0, st, scratch, nchunks, max_norm, stats);
  return hipGetLastError();
}

// g *= stats[1] in place; nothing to do (and nothing written) when the clip left the step alone.
__global__ void __launch_bounds__(kAdamThreads) k_grad_scale(TensorTable<1> tab, const float* __restrict__ stats) {
  const float coef = stats[1];
  if (coef == 1.f) return;
  chunk_walk_elem<stream_bit(kGradOnly), stream_bit(kGradOnly)>(tab, [&](float (&x)[1]) { x[0] = x[0] * coef; });
}

hipError_t grad_scale_launch(const TensorTable<1>& tab, int nchunks, const float* stats, hipStream_t st) {
  if (nchunks > 0) hipLaunchKernelGGL(k_grad_scale, dim3(nchunks), dim3(kAdamThreads), 0, st, tab, stats);
  return hipGetLastError();
}

// The partner timeouts of the frame-resident kernels reported since the last
// k_pair_flag on this device, as one float, in stream order: the report word
// is monotonic (rt_core.hip), ``base`` is this reader's own snapshot of it.
__global__ void k_pair_flag(const int* __restrict__ report, int* __restrict__ base, float* __restrict__ dst) {
  if (threadIdx.x == 0) {
    const int cur = __hip_atomic_load(report, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const int b = __hip_atomic_load(base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    dst[0] = (float)(unsigned)(cur - b);
    __hip_atomic_store(base, cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

hipError_t pair_flag_launch(const int* report, int* base, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(k_pair_flag, dim3(1), dim3(64), 0, st, report, base, dst);
  return hipGetLastError();
}

long adam_chunks(size_t numel) { return (long)((numel + kAdamChunk - 1) / kAdamChunk); }

}  // namespace aaa
