#pragma once
#include "aaa.h"
#include "common.h"

namespace aaa {

constexpr int kAdamMaxTensors = 48;   // per launch (kernel-argument table)

// The kernel-argument table of every multi-tensor kernel (optim.hip chunk_walk): K device
// streams per tensor, all nullptr for a stream the launch does not use.  K = 5 for Adam and
// RMSProp, 1 for the gradient kernels (aaa_grad_norm / aaa_grad_scale).
template <int K>
struct TensorTable {
  float* s[K][kAdamMaxTensors];
  size_t numel[kAdamMaxTensors];
  int chunk0[kAdamMaxTensors];        // first workgroup of each tensor
  unsigned char vec[kAdamMaxTensors]; // every stream in use 16-byte aligned
  int n;
};

// A table's streams, in the order of the C entries' arrays.
enum { kParam = 0, kGrad = 1, kExpAvg = 2, kExpAvgSq = 3, kMaxExpAvgSq = 4,   // Adam
       kSquareAvg = 2, kMomentumBuf = 3, kGradAvg = 4,                        // RMSProp (the last two when used)
       kGradOnly = 0 };                                                       // K = 1 (read-only for the norm)

struct AdamHost {
  double lr, beta1, beta2, eps, weight_decay;
  long step;
  int amsgrad, maximize;
  const float* guard = nullptr;   // device float: skip the update when != 0
  int* step_dev = nullptr;        // device step counter (aaa_adam_step_counted): step = *step_dev + 1,
                                  // advanced in stream order only when the update was applied
  const float* stats = nullptr;   // aaa_grad_norm's stats (aaa_adam_step_clipped): g = grad * stats[1], and
                                  // no update (nor count) when stats[2] != 0
};

struct RmspropHost {
  double lr, alpha, eps, weight_decay, momentum, lr_end;
  long anneal_steps;              // 0: constant lr
  long step;                      // the host's count after this update; read only without step_dev
  int centered, maximize, eps_in_sqrt;
  const float* guard = nullptr;   // as AdamHost's
  int* step_dev = nullptr;        // updates applied so far: the schedule's n, advanced only by an applied update
  const float* stats = nullptr;   // aaa_grad_norm's stats: g = grad * stats[1], no update (nor count) when stats[2] != 0
};

long adam_chunks(size_t numel);   // workgroups of one tensor; long, so a caller can refuse a count no grid holds
// advance: count this update on h.step_dev after the launch (the last table of a step)
hipError_t rmsprop_launch(const TensorTable<5>& tab, int nchunks, const RmspropHost& h, hipStream_t st, bool advance);
// advance: count this update on h.step_dev after the launch (the last table of a step)
hipError_t adam_launch(const TensorTable<5>& tab, int nchunks, const AdamHost& h, hipStream_t st, bool advance);
// one double per workgroup to scratch[chunk_base + workgroup]; then one workgroup over all nchunks partials
hipError_t gradsq_launch(const TensorTable<1>& tab, int nchunks, int chunk_base, double* scratch, hipStream_t st);
hipError_t gradsq_finish_launch(const double* scratch, int nchunks, double max_norm, float* stats, hipStream_t st);
hipError_t grad_scale_launch(const TensorTable<1>& tab, int nchunks, const float* stats, hipStream_t st);
hipError_t pair_flag_launch(const int* report, int* base, float* dst, hipStream_t st);

// loss.hip: REINFORCE (finish_episode) loss + logits cotangent, one workgroup per episode
hipError_t reinforce_launch(int T, int B, int A, const float* logits, const int* actions, const float* rewards,
                            double gamma, float* loss, float* rn, float* dlogits, hipStream_t st);
// loss.hip: V-trace actor-critic loss + logits / values cotangents, one wavefront per row (arguments checked by the caller)
hipError_t vtrace_launch(const aaa_vtrace_desc& d, const aaa_vtrace_io& io, hipStream_t st);
hipError_t sample_launch(int B, int A, const float* logits, uint64_t seed, unsigned long long* counter, int* actions,
                         float* logp, float* jac, hipStream_t st);
// unroll.hip: the actor's unroll recorder (arguments checked by the caller); workgroups per row of each launch
int unroll_begin_chunks(const aaa_unroll_desc& d);
int unroll_record_chunks(const aaa_unroll_desc& d);
hipError_t unroll_begin_launch(const aaa_unroll_desc& d, const aaa_unroll_io& io, hipStream_t st);
// the frame rows, then the one-workgroup launch that writes the per-row scalars and advances io.pos
hipError_t unroll_record_launch(const aaa_unroll_desc& d, const aaa_unroll_io& io, hipStream_t st);

}  // namespace aaa
