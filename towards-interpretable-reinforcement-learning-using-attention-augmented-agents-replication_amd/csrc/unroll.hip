// Recording actor unrolls on the device (aaa_unroll_begin / aaa_unroll_record;
// include/aaa.h has the contract).  Around every actor step two small launches
// move that step's products into the time-major buffers the learner trains on:
//   k_unroll_begin    before the step: zero the state rows whose episode ended,
//                     and at an unroll boundary copy the state BEFORE the step
//                     into the bank it starts (about 2 x 62 KB per row at 84x84);
//   k_unroll_record   after it: the frame row (21 KB at 84x84) into slot t, and
//                     at the boundary into slot 0 of the other bank as well;
//   k_unroll_advance  one workgroup, last: the per-row scalars, then the cursor.
// The write position is the device cursor pos = [t, bank, completed, 0]: every
// workgroup of the first two kernels reads it and none writes it.  The trailing
// one-workgroup launch reads it, __syncthreads(), then writes it, as
// k_sample_actions does with its draw counter -- it runs after the others in
// stream order, so no reader can see the new value.  The kernel arguments never
// change, which is what lets a captured graph replay them.
// A cursor outside its range writes nothing: no index derived from device memory
// reaches an address without that check.
#include <algorithm>

#include "common.h"
#include "optim.h"

namespace aaa {

constexpr int kUnrThreads = 256;
constexpr int kUnrPasses = 4;
constexpr int kUnrChunk = kUnrThreads * kUnrPasses;   // 16-byte pieces per workgroup

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct UnrollPos {
  int t, k;
  bool ok;
};

__device__ __forceinline__ UnrollPos unroll_pos(const int* pos, int T) {
  const int t = pos[0], k = pos[1];
  return {t, k, t >= 0 && t < T && (k == 0 || k == 1)};
}

// Workgroup -> (row b, chunk of the row's 16-byte state pieces); chunk 0 also
// takes the policy core's rows and ``first``.  live[i] is read and written by
// the same thread only.
__global__ void __launch_bounds__(kUnrThreads) k_unroll_begin(aaa_unroll_desc d, aaa_unroll_io io, int chunks) {
  const UnrollPos p = unroll_pos(io.pos, d.T);
  if (!p.ok) return;
  const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
  const bool done = io.done_in[b] != 0.f;
  const int dst = p.t == 0 ? p.k : (p.t == d.T - 1 ? 1 - p.k : -1);   // the bank this step starts, if any
  if (!done && dst < 0) return;
  const size_t row = (size_t)d.b0 + b;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto rows = [&](float* live_, float* bank_, size_t nv, size_t i) {
    f32x4* live = reinterpret_cast<f32x4*>(live_) + (size_t)b * nv + i;
    f32x4 v = zero;
    if (done) *live = zero;   // a select: whatever the row held, NaN included, is gone
    else v = *live;
    if (dst >= 0) reinterpret_cast<f32x4*>(bank_)[row * nv + i] = v;
  };
  const size_t nv = d.state_floats / 4;
#pragma unroll
  for (int r = 0; r < kUnrPasses; ++r) {
    const size_t i = (size_t)ch * kUnrChunk + (size_t)r * kUnrThreads + threadIdx.x;
    if (i < nv) {
      rows(io.h, dst >= 0 ? io.bank[dst].h0 : nullptr, nv, i);
      rows(io.c, dst >= 0 ? io.bank[dst].c0 : nullptr, nv, i);
    }
  }
  if (ch != 0) return;
  const size_t nc = (size_t)d.core / 4;
  for (size_t i = threadIdx.x; i < nc; i += kUnrThreads) {
    rows(io.core_h, dst >= 0 ? io.bank[dst].core_h0 : nullptr, nc, i);
    rows(io.core_c, dst >= 0 ? io.bank[dst].core_c0 : nullptr, nc, i);
  }
  if (threadIdx.x == 0 && dst >= 0) io.bank[dst].first[row] = done ? 1.f : 0.f;
}

// Workgroup -> (row b, chunk of kUnrChunk * 16 bytes of the row's frame).
// kVec: frame_bytes % 16 == 0 and the bases are 16-byte aligned, so every row
// is; otherwise the rows start anywhere and move byte by byte.
template <bool kVec>
__global__ void __launch_bounds__(kUnrThreads) k_unroll_record(aaa_unroll_desc d, aaa_unroll_io io, int chunks) {
  const UnrollPos p = unroll_pos(io.pos, d.T);
  if (!p.ok) return;
  const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
  const size_t row = (size_t)d.b0 + b, fb = d.frame_bytes;
  const bool last = p.t == d.T - 1;
  const unsigned char* src = static_cast<const unsigned char*>(io.frame) + (size_t)b * fb;
  unsigned char* cur = static_cast<unsigned char*>(io.bank[p.k].frames) + ((size_t)p.t * d.Bu + row) * fb;
  unsigned char* nxt = last ? static_cast<unsigned char*>(io.bank[1 - p.k].frames) + row * fb : nullptr;   // its slot 0
  if (kVec) {
    const size_t nv = fb / 16;
#pragma unroll
    for (int r = 0; r < kUnrPasses; ++r) {
      const size_t i = (size_t)ch * kUnrChunk + (size_t)r * kUnrThreads + threadIdx.x;
      if (i < nv) {
        const u32x4 v = reinterpret_cast<const u32x4*>(src)[i];
        reinterpret_cast<u32x4*>(cur)[i] = v;
        if (nxt) reinterpret_cast<u32x4*>(nxt)[i] = v;
      }
    }
  } else {
    const size_t base = (size_t)ch * kUnrChunk * 16;
    for (int j = threadIdx.x; j < kUnrChunk * 16; j += kUnrThreads) {
      const size_t i = base + j;
      if (i < fb) {
        const unsigned char v = src[i];
        cur[i] = v;
        if (nxt) nxt[i] = v;
      }
    }
  }
}

// One workgroup, after k_unroll_record in stream order: the per-row scalars of
// this step, then the cursor.  NaN rewards stay NaN through the clip (no fminf).
__global__ void __launch_bounds__(kUnrThreads) k_unroll_advance(aaa_unroll_desc d, aaa_unroll_io io) {
  const UnrollPos p = unroll_pos(io.pos, d.T);
  const int completed = io.pos[2];
  const bool last = p.t == d.T - 1;
  if (p.ok) {
    const aaa_unroll_bank cur = io.bank[p.k], nxt = io.bank[1 - p.k];
    const float clip = (float)d.reward_clip;
    for (int b = threadIdx.x; b < d.B; b += kUnrThreads) {
      const size_t row = (size_t)d.b0 + b, at = (size_t)p.t * d.Bu + row;
      const int a = io.actions[b];
      const float lp = io.logp[b];
      cur.actions[at] = a;
      cur.logp[at] = lp;
      if (p.t >= 1) {
        float r = io.reward_in[b];
        if (clip > 0.f) r = r < -clip ? -clip : (r > clip ? clip : r);
        cur.rewards[at - d.Bu] = r;
        cur.done[at - d.Bu] = io.done_in[b] != 0.f ? 1.f : 0.f;
      }
      if (last) {
        nxt.actions[row] = a;
        nxt.logp[row] = lp;
        cur.rewards[at] = 0.f;
        cur.done[at] = 0.f;
      }
    }
  }
  __syncthreads();   // every thread has read the cursor
  if (p.ok && threadIdx.x == 0) {
    const i32x4 np = last ? i32x4{1, 1 - p.k, completed + 1, 0} : i32x4{p.t + 1, p.k, completed, 0};
    *reinterpret_cast<i32x4*>(io.pos) = np;
  }
}

int unroll_begin_chunks(const aaa_unroll_desc& d) {
  const size_t nv = d.state_floats / 4;
  return (int)std::max<size_t>(1, (nv + kUnrChunk - 1) / kUnrChunk);
}

int unroll_record_chunks(const aaa_unroll_desc& d) {
  return (int)((d.frame_bytes + (size_t)kUnrChunk * 16 - 1) / ((size_t)kUnrChunk * 16));
}

hipError_t unroll_begin_launch(const aaa_unroll_desc& d, const aaa_unroll_io& io, hipStream_t st) {
  const int chunks = unroll_begin_chunks(d);
  hipLaunchKernelGGL(k_unroll_begin, dim3(d.B * chunks), dim3(kUnrThreads), 0, st, d, io, chunks);
  return hipGetLastError();
}

hipError_t unroll_record_launch(const aaa_unroll_desc& d, const aaa_unroll_io& io, hipStream_t st) {
  const int chunks = unroll_record_chunks(d);
  if (d.frame_bytes % 16 == 0)
    hipLaunchKernelGGL(k_unroll_record<true>, dim3(d.B * chunks), dim3(kUnrThreads), 0, st, d, io, chunks);
  else
    hipLaunchKernelGGL(k_unroll_record<false>, dim3(d.B * chunks), dim3(kUnrThreads), 0, st, d, io, chunks);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_unroll_advance, dim3(1), dim3(kUnrThreads), 0, st, d, io);
  return hipGetLastError();
}

}  // namespace aaa
