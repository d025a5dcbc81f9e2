// Frame-resident fp32 (split-product) vision-encoder BACKWARD: k_vision_bwd_frames'
// plan (vision_bwd.h: one persistent workgroup per CU, one frame at a time, all
// three products in the launch, the weight-gradient accumulators in registers
// across a workgroup's frames, per-workgroup partials summed in order by
// k_vbwd_reduce) at fp32 accuracy on the bf16 MFMA (gemm.h SPLIT6).  It replaces
// the fp32 path's three layered launches (halo conv2 dgrad, conv2 / conv1 weight
// gradients with split-K atomics), between which dY1 went out to HBM and came
// back and which gathered Y1 and the fp32 bordered frames Xp through L2.  Here
// dY1 never leaves the chip, the RGBx image is rebuilt from the uint8
// observation, and there are no atomics: the result is deterministic.
//
// Products (every fp32 operand split once into hi / mid / lo bf16 parts where it
// is committed to LDS, gemm.h split3_bf16's split):
//   conv2 wgrad  gW2[64][512] += dY2^T x im2col(Y1): six products, SPLIT6's order
//   conv2 dgrad  dY1 = WdT2[4 classes x 32][256] x gather(dY2): the PRE-SPLIT
//                weights (k_WdT2s, streamed from L2 two k steps ahead) against the
//                three dY2 planes, six products
//   conv1 wgrad  gW1[32][256] += dY1^T x im2col(RGBx): dY1 in three parts, the
//                uint8 image exact in bf16: three products (GemmCfgS6LBX's)
//   conv1 bias   column sums of the fp32 dY1 accumulators
//
// LDS (156 KB in phases; byte offsets below):
//   1. conv2 wgrad  dY2 planes [0, 49152) + Y1 planes [49152, 159744)
//   2. conv2 dgrad  reads the dY2 planes, commits the dY1 planes [79872, 159744)
//                   over the end of the (dead) Y1 region
//   3. conv1 wgrad  the RGBx image [0, 59392) over the (dead) dY2 planes and the
//                   head of the Y1 region, against the dY1 planes
// No phase leaves room for the next frame's operands, so they are prefetched into
// registers (105 per lane) while conv1's weight gradient runs, and split into the
// planes at the top of the next frame.  Every zero the products rely on (dY2
// pixels past the grid, Y1's and the image's borders, dY1's k-pad rows) lies in a
// region another phase overwrites, so it is rewritten every frame.
// Wave roles, fragment reads and the accumulator layouts are k_vision_bwd_frames'.
#pragma once
#include "vision_bwd.h"

namespace aaa {

constexpr int kVqD = 0;                         // dY2 planes: part q at kVqD + q * kVbDB
constexpr int kVqY = 3 * kVbDB;                 // Y1 planes: part q at kVqY + q * kVbYB
constexpr int kVqLds = kVqY + 3 * kVbYB;        // 159744
constexpr int kVqT = kVqLds - 3 * kVbTB;        // dY1 planes: part q at kVqT + q * kVbTB
constexpr int kVqX = 0;                         // RGBx image
constexpr int kVqWs = 4 * 16 * 3 * 64 * 16;     // pre-split conv2 dgrad weights, bytes: [class][ks][part][lane] x 16 B
static_assert(kVqLds <= 160 * 1024, "phase 1: three dY2 and three Y1 planes");
static_assert(kVqT >= kVqD + 3 * kVbDB, "phase 2: the dY1 planes clear of the dY2 planes the dgrad reads");
static_assert(kVqX + kVisXB <= kVqT, "phase 3: the RGBx image clear of the dY1 planes");
static_assert(kVqT % 16 == 0 && kVqY % 16 == 0, "16-B LDS accesses");
static_assert(kVbK1 % 16 == 0 && kVbDN * 64 == 8 * 256 * 4 && kVbK1 * 32 <= 13 * 256 * 4, "register prefetch slots");
static_assert(256 * 16 * 4 <= kVqLds, "bias-sum scratch");

struct VisBwdF32Params {
  const void* frames;   // (F, H, W, 3) uint8: the observation the forward read
  const float* dY2;     // (F, P, 64) conv2 output gradient
  const float* Y1;      // (F, P1, 32) conv1 output (forward)
  const bf16x8* Ws;     // pre-split conv2 dgrad weights (k_WdT2s; misc.hip vis_split_el, 128 rows, nks 16)
  float* part;          // [gridDim.x][kVbPart] <- per-workgroup partials
  float* dy1;           // (F, P1, 32) <- dY1 as committed (DY1 instantiation only: the checker entry)
  int F, H, W, H1, W1, h, w;
};

// vbwd_fits without its one-row-wrap rule (W1 > 16): this kernel's conv1 weight gradient wraps twice
inline bool vbwd_f32_fits(int H, int W, int H1, int W1, int h, int w) {
  const int Ha = (H1 + 1) / 2, Wa = (W1 + 1) / 2;
  return vis_fits(H, W, H1, W1, h, w) && h * w <= kVbDN - 1 && H1 * W1 <= kVbK1 && Ha * Wa <= 128 && w < 128 &&
         (H1 + 4) * (W1 + 4) * 64 <= kVbYB && Ha <= h && Wa <= w && W1 >= 8;
}

// v[0..3] -> part q (0 hi, 1 mid, 2 lo) at base + q * plane (gemm.h split3_bf16's split)
__device__ __forceinline__ void vq_commit4(unsigned char* base, int plane, const f32x4& v) {
  bf16x4 ph, pm, pl;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ph[e] = (__bf16)v[e];
    const float r = v[e] - (float)ph[e];
    pm[e] = (__bf16)r;
    pl[e] = (__bf16)(r - (float)pm[e]);
  }
  *reinterpret_cast<bf16x4*>(base) = ph;
  *reinterpret_cast<bf16x4*>(base + plane) = pm;
  *reinterpret_cast<bf16x4*>(base + 2 * plane) = pl;
}

template <bool DY1>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_vision_bwd_f32(VisBwdF32Params p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kVqLds];
  unsigned char* const dpl = lds + kVqD;
  unsigned char* const ypl = lds + kVqY;
  unsigned char* const tpl = lds + kVqT;
  unsigned char* const xim = lds + kVqX;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5;
  const int Wp = p.W + 2, W1p = p.W1 + 4, P = p.h * p.w, P1 = p.H1 * p.W1;
  const int Ha = (p.H1 + 1) / 2, Wa = (p.W1 + 1) / 2, NA = Ha * Wa;
  const int G4 = p.H * p.W / 4;
  const int KS1 = (P1 + 15) / 16;   // conv1-wgrad k steps

  {  // zero the whole array once
    u32x4* z = reinterpret_cast<u32x4*>(lds);
    for (int i = tid; i < kVqLds / 16; i += 256) z[i] = u32x4{0u, 0u, 0u, 0u};
  }

  // ---- frame f's operands into registers: dY2 (8 x 4 floats), Y1 (13 x 4), the observation (uint8);
  // unconditional (clamped) loads
  f32x4 rd[8], ry[13];
  uint32_t raw[kVisNG][3];
  auto fetch = [&](int f, int tid) {   // (tid, here and below: the caller's laundered copy)
    const f32x4* d = reinterpret_cast<const f32x4*>(p.dY2 + (size_t)f * P * 64);
#pragma unroll
    for (int k = 0; k < 8; ++k) rd[k] = d[min(tid + 256 * k, P * 16 - 1)];
    const f32x4* y = reinterpret_cast<const f32x4*>(p.Y1 + (size_t)f * P1 * 32);
#pragma unroll
    for (int k = 0; k < 13; ++k) ry[k] = y[min(tid + 256 * k, P1 * 8 - 1)];
    // a group's 12 bytes as an 8-B and a 4-B load whose offsets the compiler cannot relate: one 12-B load
    // lands in an even-aligned register triple, and packing the triples waits for every load right here
    const uint32_t* src =
        reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(p.frames) + (size_t)f * p.H * p.W * 3);
    int two = 2;
    asm volatile("" : "+s"(two));
#pragma unroll
    for (int i = 0; i < kVisNG; ++i) {
      const int g = min(tid + 256 * i, G4 - 1);
      const uint2 v = *reinterpret_cast<const uint2*>(src + (size_t)g * 3);
      raw[i][0] = v.x;
      raw[i][1] = v.y;
      raw[i][2] = src[(size_t)g * 3 + two];
    }
  };
  // the fetched dY2 / Y1 split into their planes; dY2 pixels P .. 127 and Y1's border rewritten as zeros
  auto commit = [&](int tid) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // slot i: channels 4 (i % 16) .. +3 of image pixel i / 16 (all 128 pixels)
      const int i = tid + 256 * k, pix = i >> 4, ch = (i & 15) * 4;
      const f32x4 v = pix < P ? rd[k] : f32x4{0.f, 0.f, 0.f, 0.f};
      vq_commit4(dpl + vb_dofs(pix, ch), kVbDB, v);
    }
#pragma unroll
    for (int k = 0; k < 13; ++k) {   // slot i: channels 4 (i % 8) .. +3 of conv1 pixel i / 8
      const int i = tid + 256 * k, p1 = i >> 3, ch = (i & 7) * 4;
      if (p1 < P1) {
        const int y = p1 / p.W1, x = p1 - y * p.W1;
        vq_commit4(ypl + ((y + 2) * W1p + x + 2) * 64 + ch * 2, kVbYB, ry[k]);
      }
    }
    for (int i = tid; i < (p.H1 + 4) * W1p; i += 256) {
      const int y = i / W1p, x = i - y * W1p;
      if (y < 2 || y >= p.H1 + 2 || x < 2 || x >= p.W1 + 2) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          u32x4* z = reinterpret_cast<u32x4*>(ypl + q * kVbYB + i * 64);
#pragma unroll
          for (int c = 0; c < 4; ++c) z[c] = u32x4{0u, 0u, 0u, 0u};
        }
      }
    }
  };
  auto build = [&](int tid) {   // as k_vision_fwd: bf16 RGBx, channel 3 zero; the border rewritten as zeros
    for (int i = tid; i < 2 * Wp + 2 * p.H; i += 256) {
      const int px = i < 2 * Wp ? (i < Wp ? i : (p.H + 1) * Wp + i - Wp)
                                : (1 + ((i - 2 * Wp) >> 1)) * Wp + ((i & 1) ? Wp - 1 : 0);
      *reinterpret_cast<uint2*>(xim + px * 8) = uint2{0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < kVisNG; ++i) {
      const int g = tid + 256 * i;
      if (g < G4) {
        const int pix = 4 * g, y = pix / p.W, x = pix - y * p.W;
        unsigned char* d = xim + ((y + 1) * Wp + x + 1) * 8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int e = 3 * j + c;
            v[c] = (float)((raw[i][e >> 2] >> (8 * (e & 3))) & 255u);
          }
          *reinterpret_cast<bf16x4*>(d + j * 8) = bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)0.f};
        }
      }
    }
  };

  // ---- frame-invariant lane geometry (k_vision_bwd_frames')
  const int rw16 = (65536 + p.w - 1) / p.w;
  auto ypo = [&](int pix) {
    pix = pix < P ? pix : 0;   // (A is zero past the grid: any finite B)
    const int y2 = (pix * rw16) >> 16, x2 = pix - y2 * p.w;
    return (2 * y2 * W1p + 2 * x2) * 64;
  };

  f32x16 acc2[2][4], acc1[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc2[r][j][e] = 0.f;
    acc1[0][e] = acc1[1][e] = 0.f;
  }
  float bsum[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) bsum[i] = 0.f;
  const int py = wave >> 1, px = wave & 1;   // the wave's dgrad parity class

  int f = blockIdx.x;
  if (f < p.F) fetch(f, tid);
  barrier_lds();   // array zeroed
  for (; f < p.F; f += gridDim.x) {
    // The thread / lane id laundered once per phase: the phases' addresses are frame-invariant, and hoisted out
    // of the frame loop they would hold a few hundred registers across all three phases
    auto launder = [&](int l = 0) {
      asm volatile("" : "+v"(l));
      return l;
    };
    commit(tid + launder());
    barrier_lds();   // dY2 and Y1 planes complete

    // ---- phase 1, conv2 wgrad: gW2[64 o][tap 4w + j, ci] += sum_pixels dY2[pix][o] Y1[window(pix, tap)][ci]
    {
      const int wl = lane + launder(), r32 = wl & 31, hh = wl >> 5, tq = (wl & 15) >> 2, tp = wl & 3;   // (glds.h frag_rc)
      bf16x8 a2[2][2][3], b2[2][4][3];   // [buffer][row block | tap][part]
      // fragment i (0..17) of k step s: A (rows o = 32 rb + (r32 & 16) + 4 tp .. +3 at pixels 16 s + 8 hh + tq
      // (+4)) then B (rows ci = (r32 & 16) + 4 tp .. +3 of tap 4 wave + j)
      auto ld2 = [&](int s, int i) {
        const int k0 = 16 * s + 8 * hh + tq;
        if (i < 6) {
          const int rb = i / 3, q = i % 3, o0 = 32 * rb + (r32 & 16) + 4 * tp;
          a2[s & 1][rb][q] = vb_tr(dpl + q * kVbDB, vb_dofs(k0, o0), vb_dofs(k0 + 4, o0));
        } else {
          const int j = (i - 6) / 3, q = (i - 6) % 3;
          const int tap = 4 * wave + j, ky = tap >> 2, kx = tap & 3;
          const int off = (ky * W1p + kx) * 64 + ((r32 & 16) + 4 * tp) * 2;
          b2[s & 1][j][q] = vb_tr(ypl + q * kVbYB, ypo(k0) + off, ypo(k0 + 4) + off);
        }
      };
#pragma unroll
      for (int i = 0; i < 18; ++i) ld2(0, i);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        // gemm.h SPLIT6's order (smallest first): lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi; the next
        // step's fragments are requested three per product
        constexpr int qa[6] = {2, 0, 1, 1, 0, 0}, qb[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int g = 0; g < 6; ++g) {
          if (s + 1 < 8) {
#pragma unroll
            for (int i = 3 * g; i < 3 * g + 3; ++i) ld2(s + 1, i);
          }
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc2[rb][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[s & 1][rb][qa[g]], b2[s & 1][j][qb[g]],
                                                                    acc2[rb][j], 0, 0, 0);
        }
      }
    }
    barrier_lds();   // every wave is done with the Y1 planes: the dY1 planes may overwrite them

    // ---- phase 2, conv2 dgrad (wave = parity class): D[32 c][class grid] = WdT2[class rows] x dY2 gather
    {
      const int wl = lane + launder(), r32 = wl & 31, hh = wl >> 5;
      // (the lane's dgrad columns, recomputed per frame: eight registers less across the other phases)
      int dpb[4], dvm[4];
    #pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int n = 32 * cb + r32, a = n / Wa, b = n - a * Wa;
        dpb[cb] = a * p.w + b;
        dvm[cb] = 0;
    #pragma unroll
        for (int t = 0; t < 4; ++t)
          if (n < NA && a + (t >> 1) < p.h && b + (t & 1) < p.w) dvm[cb] |= 1 << t;
      }
      auto dpix = [&](int cb, int t) { return (dvm[cb] >> t) & 1 ? dpb[cb] + (t >> 1) * p.w + (t & 1) : kVbDN - 1; };
      f32x16 acc[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[cb][e] = 0.f;
      bf16x8 a[3][3], b[2][4][3];   // [ring][part], [buffer][column block][part]
      const bf16x8* Ws = p.Ws + (size_t)wave * 16 * 3 * 64 + wl;
      auto lda = [&](int s) {
#pragma unroll
        for (int q = 0; q < 3; ++q) a[s % 3][q] = Ws[(s * 3 + q) * 64];
      };
      auto ldb = [&](int s, int i) {   // fragment i (0..11): column block i / 3, part i % 3
        const int t = s >> 2, ch = 16 * (s & 3) + 8 * hh, cb = i / 3, q = i % 3;
        b[s & 1][cb][q] = *reinterpret_cast<const bf16x8*>(dpl + q * kVbDB + vb_dofs(dpix(cb, t), ch));
      };
      lda(0);
      lda(1);
#pragma unroll
      for (int i = 0; i < 12; ++i) ldb(0, i);
      // the dY1 planes' k-pad rows (P1 .. 16 KS1 - 1): zeros for conv1's weight gradient
      for (int i = tid; i < (16 * KS1 - P1) * 12; i += 256) {
        const int q = i % 3, r = i / 3;
        *reinterpret_cast<u32x4*>(tpl + q * kVbTB + (P1 + (r >> 2)) * 64 + (r & 3) * 16) = u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        if (s + 2 < 16) lda(s + 2);
        __builtin_amdgcn_sched_barrier(0);   // (else the loads sink to their first use, each with a vmcnt(0) behind it)
        constexpr int qa[6] = {2, 0, 1, 1, 0, 0}, qb[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int g = 0; g < 6; ++g) {
          if (s + 1 < 16) {
            ldb(s + 1, 2 * g);
            ldb(s + 1, 2 * g + 1);
          }
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s % 3][qa[g]], b[s & 1][cb][qb[g]], acc[cb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // dY1 (class pixels) split into the dY1 planes; the bias sums from fp32
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int n = 32 * cb + r32, a0 = n / Wa, b0 = n - a0 * Wa, y1 = 2 * a0 + py, x1 = 2 * b0 + px;
        if (n < NA && y1 < p.H1 && x1 < p.W1) {
          const int p1 = y1 * p.W1 + x1;
#pragma unroll
          for (int g = 0; g < 4; ++g) {   // channels 8g + 4hh .. +3
            const f32x4 v = {acc[cb][4 * g], acc[cb][4 * g + 1], acc[cb][4 * g + 2], acc[cb][4 * g + 3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) bsum[4 * g + e] += v[e];
            vq_commit4(tpl + p1 * 64 + (8 * g + 4 * hh) * 2, kVbTB, v);
            if constexpr (DY1) *reinterpret_cast<f32x4*>(p.dy1 + ((size_t)f * P1 + p1) * 32 + 8 * g + 4 * hh) = v;
          }
        }
      }
    }
    barrier_lds();   // the dY1 planes complete; every wave is done with the dY2 planes

    const int tl = tid + launder();
    build(tl);   // the frame's RGBx image over the dY2 planes
    const int fn = f + (int)gridDim.x;
    if (fn < p.F) fetch(fn, tl);   // the next frame's operands land under conv1's weight gradient
    barrier_lds();   // image complete; the next frame's loads stay in flight

    // ---- phase 3, conv1 wgrad: gW1[32 o][ky = 2w + j, kx, c] += sum_pixels dY1[pix][o] X[4 oy + ky][4 ox + kx][c]
    {
      const int wl = lane + launder(), r32 = wl & 31, hh = wl >> 5, tq = (wl & 15) >> 2, tp = wl & 3;
      int oy[2], ox[2];   // the k-rows' conv1 output pixels, advanced 16 per k step
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int pix = 8 * hh + tq + 4 * u;
        oy[u] = pix / p.W1;
        ox[u] = pix - oy[u] * p.W1;
      }
      const int ao = 8 * hh * 64 + tq * 64 + ((r32 & 16) + 4 * tp) * 2;
      const int kxo = (((r32 & 16) >> 2) + tp) * 8;
      auto frags = [&](int s, bf16x8 (&a1)[3], bf16x8 (&b1)[2]) {
#pragma unroll
        for (int q = 0; q < 3; ++q) a1[q] = vb_tr(tpl + q * kVbTB, ao + 16 * s * 64, ao + 16 * s * 64 + 4 * 64);
        int xo[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bool ok = 16 * s + 8 * hh + tq + 4 * u < P1;   // past P1: the dY1 rows are zero, any finite B
          xo[u] = ok ? (4 * oy[u] * Wp + 4 * ox[u]) * 8 + kxo : kxo;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) b1[j] = vb_tr(xim, xo[0] + (2 * wave + j) * Wp * 8, xo[1] + (2 * wave + j) * Wp * 8);
#pragma unroll
        for (int u = 0; u < 2; ++u) {   // k += 16: W1 >= 8, so at most two row wraps
          ox[u] += 16;
          if (ox[u] >= p.W1) { ox[u] -= p.W1; ++oy[u]; }
          if (ox[u] >= p.W1) { ox[u] -= p.W1; ++oy[u]; }
        }
      };
      bf16x8 ac[3], bc[2];
      frags(0, ac, bc);
      for (int s = 0; s < KS1; ++s) {   // the next step's reads issued before this step's MFMAs
        bf16x8 an[3], bn[2];
        if (s + 1 < KS1) frags(s + 1, an, bn);
#pragma unroll
        for (int q = 2; q >= 0; --q)   // smallest first: lo, mid, hi against the exact image
#pragma unroll
          for (int j = 0; j < 2; ++j) acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ac[q], bc[j], acc1[j], 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 3; ++q) ac[q] = an[q];
        bc[0] = bn[0];
        bc[1] = bn[1];
      }
    }
    barrier_lds();   // every wave is done with the image and the dY1 planes
  }

  // ---- this workgroup's partials (k_vision_bwd_frames' layout): gW2, gW1, conv1 bias
  float* pt = p.part + (size_t)blockIdx.x * kVbPart;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          pt[(32 * rb + 8 * g + 4 * hh + e) * 512 + 32 * (4 * wave + j) + r32] = acc2[rb][j][4 * g + e];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        pt[32768 + (8 * g + 4 * hh + e) * 256 + 32 * (2 * wave + j) + r32] = acc1[j][4 * g + e];
  float* red = reinterpret_cast<float*>(lds);   // (free: the loop ended on a barrier)
#pragma unroll
  for (int i = 0; i < 16; ++i) red[(wave * 64 + lane) * 16 + i] = bsum[i];
  __syncthreads();
  if (tid < 32) {   // channel c = 8 g + 4 hh + e: rows 4 g + e of the lanes with that hh, every class
    const int g = tid >> 3, h2 = (tid >> 2) & 1, e = tid & 3;
    float t = 0.f;
    for (int w = 0; w < 4; ++w)
      for (int l = 0; l < 32; ++l) t += red[(w * 64 + 32 * h2 + l) * 16 + 4 * g + e];
    pt[40960 + tid] = t;
  }
}

// Workgroups for F frames: the fewest that keep the frame rounds of one workgroup per CU
// (ceil(F / ceil(F / cus)): 640 frames on 256 CUs are three rounds either way, with 214 partials
// instead of 256), no more than the lent room holds (kVbPart floats each) nor than max_groups (> 0).
inline int vbwd_f32_groups(int F, int cus, size_t part_bytes, int max_groups = 0) {
  const int rounds = (F + cus - 1) / cus;
  int g = (F + rounds - 1) / rounds;
  g = (int)std::min<size_t>((size_t)g, part_bytes / ((size_t)kVbPart * 4));
  if (max_groups > 0) g = std::min(g, max_groups);
  return g;
}

inline hipError_t vision_bwd_frames_f32(const VisBwdF32Params& p, int nwg, float* gW2, float* gW1, float* gb1,
                                        hipStream_t st) {
  if (!vbwd_f32_fits(p.H, p.W, p.H1, p.W1, p.h, p.w) || p.F < 1 || nwg < 1) return hipErrorInvalidValue;
  if (p.dy1) hipLaunchKernelGGL((k_vision_bwd_f32<true>), dim3(nwg), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((k_vision_bwd_f32<false>), dim3(nwg), dim3(256), 0, st, p);
  hipLaunchKernelGGL(k_vbwd_reduce, dim3((kVbPart + 63) / 64), dim3(256), 0, st, p.part, nwg, gW2, gW1, gb1);
  return hipGetLastError();
}

}  // namespace aaa
