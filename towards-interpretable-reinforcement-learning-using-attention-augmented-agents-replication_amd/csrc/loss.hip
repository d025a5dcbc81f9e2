// REINFORCE loss on device: the reference's
// finish_episode (main_mp.py:62-77) for B independent episodes of T steps,
// fused into one kernel that also produces the loss cotangent the learner's
// backward consumes -- so an episode update needs no host round trip for the
// returns and no autograd graph over T per-step Categorical objects.
//
// Per episode b (one workgroup):
//   R_t  = r_t + gamma * R_{t+1}               (Python float = double in the reference, :66-68)
//   R^_t = (R_t - mean R) / (std R + eps)      (float32 tensor ops, unbiased std, eps = f32 eps, :69-70)
//   logp = log(clamp(p_{a_t}, eps, 1 - eps)),  p = softmax(logits_t) / sum   (Categorical(probs=..)
//          as built at main_mp.py:55-58: probs_to_logits clamps the probabilities)
//   loss_b = sum_t -logp_t * R^_t               (:71-73, :76)
//   dlogits[t][b][k] = -R^_t * (1[k == a_t] - p_k), zero where the clamp is active.
// The discounted return is a linear recurrence, so it runs as a parallel scan
// of affine maps x -> r + gamma x (in double) over the workgroup's threads.
#include <cfloat>
#include <cmath>

#include "common.h"
#include "optim.h"
#include "sampling.h"

namespace aaa {

constexpr int kRfThreads = 256;

__device__ __forceinline__ double wg_sum_d(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < kRfThreads / 64; ++w) t += red[w];
  return t;
}

// rn: (T, B) scratch for the normalised returns (always written).
__global__ void __launch_bounds__(kRfThreads)
k_reinforce(int T, int B, int A, const float* __restrict__ logits, const int* __restrict__ actions,
            const float* __restrict__ rewards, double gamma, float* __restrict__ loss, float* __restrict__ rn,
            float* __restrict__ dlogits) {
  __shared__ double sa[kRfThreads], sb[kRfThreads];   // affine map of each thread's chunk: R_in -> a*R_in + b
  __shared__ double red[kRfThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int per = (T + kRfThreads - 1) / kRfThreads;
  const int t0 = min(T, tid * per), t1 = min(T, t0 + per);
  // 1. chunk-local backward scan: R_t = r_t + gamma R_{t+1} with R_{t1} = x  ->  R_{t0} = a x + b
  double ca = 1.0, cb = 0.0;
  for (int t = t1 - 1; t >= t0; --t) {
    cb = (double)rewards[(size_t)t * B + b] + gamma * cb;
    ca *= gamma;
  }
  sa[tid] = ca;
  sb[tid] = cb;
  __syncthreads();
  // 2. incoming return of every chunk: compose the maps of the chunks to its right
  //    (one thread; kRfThreads affine compositions)
  if (tid == 0) {
    double x = 0.0;
    for (int k = kRfThreads - 1; k >= 0; --k) {
      const double nx = sa[k] * x + sb[k];
      sa[k] = x;          // R entering chunk k from the right
      x = nx;
    }
  }
  __syncthreads();
  // 3. returns of this chunk (double -> float32 as torch.tensor(returns) does)
  double x = sa[tid], s1 = 0.0;
  for (int t = t1 - 1; t >= t0; --t) {
    x = (double)rewards[(size_t)t * B + b] + gamma * x;
    const float rf = (float)x;
    rn[(size_t)t * B + b] = rf;
    s1 += (double)rf;
  }
  const double mean = wg_sum_d(s1, red) / (double)T;
  double s2 = 0.0;
  for (int t = t0; t < t1; ++t) {
    const double d = (double)rn[(size_t)t * B + b] - mean;
    s2 += d * d;
  }
  const double var = wg_sum_d(s2, red) / (double)(T - 1);   // T == 1 -> nan, as torch.std
  const float sd = (float)sqrt(var);
  const float meanf = (float)mean;
  const float eps = FLT_EPSILON;
  // 4. per-step softmax, clamped log-prob and cotangent (each thread its chunk of steps)
  double lsum = 0.0;
  for (int t = t0; t < t1; ++t) {
    const float Rh = (rn[(size_t)t * B + b] - meanf) / (sd + eps);
    rn[(size_t)t * B + b] = Rh;
    const float* l = logits + ((size_t)t * B + b) * A;
    float* dl = dlogits + ((size_t)t * B + b) * A;
    float mx = -INFINITY;
    for (int k = 0; k < A; ++k) mx = fmaxf(mx, l[k]);
    float z = 0.f;
    for (int k = 0; k < A; ++k) z += expf(l[k] - mx);
    const int a = actions[(size_t)t * B + b];
    const float pa = expf(l[a] - mx) / z;
    const bool clamped = !(pa >= eps && pa <= 1.f - eps);   // clamp's backward passes at the bounds
    const float lp = logf(fminf(fmaxf(pa, eps), 1.f - eps));
    lsum += (double)(-lp * Rh);
    for (int k = 0; k < A; ++k) {
      const float pk = expf(l[k] - mx) / z;
      dl[k] = clamped ? 0.f : -Rh * ((k == a ? 1.f : 0.f) - pk);
    }
  }
  const double tot = wg_sum_d(lsum, red);
  if (tid == 0) loss[b] = (float)tot;
}

hipError_t reinforce_launch(int T, int B, int A, const float* logits, const int* actions, const float* rewards,
                            double gamma, float* loss, float* rn, float* dlogits, hipStream_t st) {
  hipLaunchKernelGGL(k_reinforce, dim3(B), dim3(kRfThreads), 0, st, T, B, A, logits, actions, rewards, gamma, loss,
                     rn, dlogits);
  return hipGetLastError();
}

}  // namespace aaa

namespace aaa {

// --------------------------------------------------- V-trace actor-critic ---
// The IMPALA loss of B unrolls of T steps and its cotangents (include/aaa.h
// aaa_vtrace has the definitions).  The learner's T is 20-50, so the shape is
// not k_reinforce's (one workgroup per row, threads chunking T): one wavefront
// owns a row, its lanes are time steps, kVtRows rows share a workgroup.  Each
// lane does its own step's A-wide softmax (fp32, max-subtracted) and the
// per-step scalars in double; the recursion x_t = delta_t + g_t x_{t+1},
// g_t = gamma_t c_t, is a backward scan of the affine maps x -> delta_t + g_t x
// over the wave (shuffles, double).  T > 64 runs in chunks of 64 steps from
// the last to the first, carrying x, vs and V of the chunk to the right.  A
// done step has g_t = 0 exactly, which wipes everything to its right out of
// the composed maps bit for bit.  The loss parts are per-lane double sums
// reduced over the wave in a fixed order.
constexpr int kVtRows = 4;   // wavefronts (rows) per workgroup

struct VtraceArgs {
  aaa_vtrace_desc d;
  aaa_vtrace_io io;
};

__global__ void __launch_bounds__(kVtRows * 64) k_vtrace(const VtraceArgs P) {
  const int T = P.d.T, B = P.d.B, A = P.d.A, vc = P.d.value_col;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kVtRows + (threadIdx.x >> 6);
  if (b >= B) return;   // whole wave; no workgroup barrier below
  const float* __restrict__ logits = P.io.logits;
  const float* __restrict__ values = P.io.values;
  const int* __restrict__ actions = P.io.actions;
  const float nanf_ = __uint_as_float(0x7fc00000u);
  // an action outside [0, A) anywhere in the row: nothing is read through it, the row's outputs are NaN
  int bad = 0;
  for (int t = lane; t < T; t += 64) bad |= (unsigned)actions[(size_t)t * B + b] >= (unsigned)A;
  bad = __any(bad);
  const double gamma = P.d.gamma, lambda = P.d.lambda, rho_bar = P.d.rho_bar, c_bar = P.d.c_bar,
               pg_rho_bar = P.d.pg_rho_bar;
  const float scale = (float)P.d.scale, ec = (float)P.d.entropy_cost;
  const double vcoef = -P.d.scale * P.d.baseline_cost;
  const double boot = P.io.bootstrap ? (double)P.io.bootstrap[b] : 0.0;
  double x_in = 0.0, vs_in = boot, V_in = boot;   // x, vs and V of the first step to the right of the chunk
  double l0 = 0.0, l1 = 0.0, l2 = 0.0;
  for (int c = (T - 1) / 64; c >= 0; --c) {
    const int t = c * 64 + lane;
    const bool on = t < T;
    const size_t tb = (size_t)(on ? t : T - 1) * B + b;   // idle lanes redo the last step, write nothing
    const float* l = logits + tb * A;
    // softmax pieces: z = sum e^{l - mx}, s = sum e^{l - mx} (l - mx)  ->  H = log z - s / z
    float mx = -INFINITY;
    for (int k = 0; k < A; ++k) mx = fmaxf(mx, l[k]);
    float z = 0.f, s = 0.f;
    for (int k = 0; k < A; ++k) {
      const float d = l[k] - mx, e = expf(d);
      z += e;
      s += e * d;
    }
    const float logz = logf(z), H = logz - s / z;
    const int a_raw = actions[tb];
    const int a = (unsigned)a_raw < (unsigned)A ? a_raw : 0;
    const float lpa = (l[a] - mx) - logz;
    const double V = (double)values[tb * A + vc];
    const double r = (double)P.io.rewards[tb];
    const bool dn = P.io.done ? P.io.done[tb] != 0.f : false;
    const double g_t = dn ? 0.0 : gamma;
    const double ratio = P.io.behaviour_logp ? exp((double)lpa - (double)P.io.behaviour_logp[tb]) : 1.0;   // NULL: on-policy
    const double rho = fmin(rho_bar, ratio), ct = lambda * fmin(c_bar, ratio), rho_pg = fmin(pg_rho_bar, ratio);
    // V_{t+1}: the next lane's, or the carried one at the chunk's (or the unroll's) last step
    double Vn = __shfl_down(V, 1, 64);
    const bool edge = lane == 63 || t == T - 1;
    if (edge) Vn = V_in;
    const double delta = rho * (dn ? r - V : r + g_t * Vn - V);
    // backward inclusive scan of x -> mb + ma x over the lanes; idle lanes are the identity
    double ma = on ? g_t * ct : 1.0, mb = on ? delta : 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double ra = __shfl_down(ma, o, 64), rb = __shfl_down(mb, o, 64);
      if (lane + o < 64) {
        mb = mb + ma * rb;
        ma = ma * ra;
      }
    }
    const double x = mb + ma * x_in;
    const double vs = V + x;
    double vsn = __shfl_down(vs, 1, 64);
    if (edge) vsn = vs_in;
    const double adv = rho_pg * (dn ? r - V : r + g_t * vsn - V);
    x_in = __shfl(x, 0, 64);
    vs_in = __shfl(vs, 0, 64);
    V_in = __shfl(V, 0, 64);
    if (!on) continue;
    l0 += -adv * (double)lpa;
    l1 += 0.5 * x * x;
    l2 += (double)H;
    const float advf = (float)adv, iz = 1.f / z;
    float* dl = P.io.dlogits + tb * A;
    float* dv = P.io.dvalues + tb * A;
    for (int k = 0; k < A; ++k) {
      const float d = l[k] - mx, p = expf(d) * iz, lp = d - logz;
      const float g = scale * (-advf * ((k == a ? 1.f : 0.f) - p) + ec * p * (lp + H));
      dl[k] = bad ? nanf_ : g;
      dv[k] = bad ? nanf_ : (k == vc ? (float)(vcoef * x) : 0.f);
    }
    if (P.io.vs) P.io.vs[tb] = bad ? nanf_ : (float)vs;
    if (P.io.pg_adv) P.io.pg_adv[tb] = bad ? nanf_ : advf;
  }
  if (P.io.loss) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      l0 += __shfl_xor(l0, o, 64);
      l1 += __shfl_xor(l1, o, 64);
      l2 += __shfl_xor(l2, o, 64);
    }
    if (lane < 3) P.io.loss[(size_t)b * 3 + lane] = bad ? nanf_ : (float)(lane == 0 ? l0 : lane == 1 ? l1 : l2);
  }
}

hipError_t vtrace_launch(const aaa_vtrace_desc& d, const aaa_vtrace_io& io, hipStream_t st) {
  VtraceArgs P{d, io};
  hipLaunchKernelGGL(k_vtrace, dim3((d.B + kVtRows - 1) / kVtRows), dim3(kVtRows * 64), 0, st, P);
  return hipGetLastError();
}

}  // namespace aaa

namespace aaa {

// ------------------------------------------------------ actor sampling ---
// Policy.forward's action draw for B rows of logits, on device, one wavefront
// per row (the per-row draw is draw_row, sampling.h).  The draw index
// ``counter`` lives in device memory and is advanced by one per launch, so a
// captured graph replays fresh draws without a host round trip.
constexpr int kSmpThreads = 256;

__global__ void __launch_bounds__(kSmpThreads)
k_sample_actions(int B, int A, const float* __restrict__ logits, uint64_t seed, unsigned long long* counter,
                 int* __restrict__ actions, float* __restrict__ logp, float* __restrict__ jac) {
  const int wave = threadIdx.x >> 6;
  const uint64_t ctr = counter ? (uint64_t)*counter : 0ull;
  for (int b = wave; b < B; b += kSmpThreads / 64) draw_row(logits + (size_t)b * A, A, seed, ctr, b, actions, logp, jac);
  __syncthreads();   // every wave has read the counter
  if (counter && threadIdx.x == 0) *counter = ctr + 1ull;
}

hipError_t sample_launch(int B, int A, const float* logits, uint64_t seed, unsigned long long* counter, int* actions,
                         float* logp, float* jac, hipStream_t st) {
  hipLaunchKernelGGL(k_sample_actions, dim3(1), dim3(kSmpThreads), 0, st, B, A, logits, seed, counter, actions, logp,
                     jac);
  return hipGetLastError();
}

}  // namespace aaa
