// Frame-resident fp32 (split-product) vision encoder forward: k_vision_fwd's
// plan (vision.h: one persistent workgroup per CU, one frame at a time, images
// in LDS) at fp32 accuracy on the bf16 MFMA (gemm.h SPLIT6).  It replaces the
// fp32 path's three layered launches (frames_rgbx, conv1 im2col ring, conv2
// im2col GEMM), which write the fp32 RGBx image and Y1 only to gather them again.
//
// Per frame:
//   image  the observation (H, W, 3) -> zero-bordered RGBx bf16 image in LDS
//          (uint8 frames: exact, one image; fp32 frames: the hi / mid / lo bf16
//          parts of the frame, one image after the other) and, where the caller
//          asks for it (the XP instantiation: the checker entries; the learner
//          stores none), from the same registers the fp32 bordered image Xp in HBM
//          (the layered conv1 weight gradient's operand: bit for bit k_frames_rgbx's).
//   conv1  D[32][P1] from the image against the PRE-SPLIT conv1 weights (hi / mid /
//          lo bf16 fragments, streamed from L2 a few k steps ahead), all of a
//          wave's column blocks (<= 4) accumulated in registers.  Products per k
//          step smallest first: W_lo.x, W_mid.x, W_hi.x (GemmCfgS6BX's); fp32
//          frames add, before them, the image passes x_lo: W_hi and x_mid: W_mid,
//          W_hi -- all exact zeros on integer-valued frames, so the result is
//          then bit for bit the uint8 instantiation's.
//   Y1     + bias -> fp32 to HBM (the backward reads it) and, split once,
//          into the hi / mid / lo planes of a zero-bordered Y1 image in LDS.
//   conv2  D[64][P] from the three planes against the pre-split conv2 weights
//          (streamed from L2), six products per k step in SPLIT6's order, + bias
//          -> fp32 into the ConvLSTM operand slot (columns 0..63 of ``out``).
//
// LDS (160 KB): the three Y1 planes (3 x 46080 B at kVisYP's 80-B pixel pitch)
// and the RGBx image (59392 B) do not fit side by side, and conv1's
// accumulators live in registers, so the image is dead when Y1 is committed:
// the planes sit at [0, 138240), the image at the end of the array
// [103424, 162816).  They share 34816 B of plane 2; its border and the image's
// border are re-zeroed every frame (14 KB of LDS stores per frame).
#pragma once
#include "vision.h"

namespace aaa {

constexpr int kVfLds = 160 * 1024 - 1024;   // the image/plane array (the rest: biases)
constexpr int kVfXOff = kVfLds - kVisXB;    // the RGBx image's offset in it
static_assert(3 * kVisYB <= kVfLds && kVfXOff % 16 == 0 && kVfXOff >= 2 * kVisYB, "LDS plan");
constexpr int kVfW1 = 16 * 3 * 64 * 16;       // pre-split conv1 weights, bytes: [ks][part][lane] x 16 B
constexpr int kVfW2 = 2 * 32 * 3 * 64 * 16;   // pre-split conv2 weights: [row block][ks][part][lane] x 16 B

// The fragment order of both (misc.hip vis_split_el): element (row, k) of a [rows][16 nks] matrix is
// split as gemm.h split3_bf16 does; lane (row % 32, (k / 8) % 2) of k step k / 16 of row block
// row / 32 holds 8 consecutive k, and a fragment's parts follow each other (0 hi, 1 mid, 2 lo).

struct VisF32Params {
  const void* frames;   // (F, H, W, 3) uint8 or fp32
  const bf16x8* W1s;    // pre-split conv1 weights (nks 16)
  const float* b1;      // [32]
  const bf16x8* W2s;    // pre-split conv2 weights (nks 32)
  const float* b2;      // [64]
  float* Xp;            // (F, H+2, W+2, 4) <- bordered RGBx frames (conv1's weight-gradient operand), or null
  float* Y1;            // (F, H1*W1, 32) <- conv1 output
  float* out;           // (F, h*w, out_ld) <- conv2 output, channels 0..63
  int out_ld, F, H, W, H1, W1, h, w;
};

// One image pass of conv1: NB column blocks of the wave against weight parts NW-1 .. 0 (lo .. hi:
// smallest first).  Two k steps per group; the B fragments of the next group and the weight
// fragments two groups ahead are requested before a group's MFMAs.
template <int NB, int NW>
__device__ __forceinline__ void vf_conv1_pass(const unsigned char* xim, const bf16x8* W1s, int wl, const int (&bo)[4],
                                              int Wp, f32x16 (&acc)[4]) {
  bf16x8 a[3][2][NW], b[2][2][NB];
  auto lda = [&](int g) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int q = 0; q < NW; ++q) a[g % 3][k][q] = W1s[((2 * g + k) * 3 + q) * 64 + wl];
  };
  auto ldb = [&](int g) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int ks = 2 * g + k;
#pragma unroll
      for (int j = 0; j < NB; ++j)
        b[g & 1][k][j] = *reinterpret_cast<const bf16x8*>(xim + bo[j] + ((ks >> 1) * Wp + (ks & 1) * 4) * 8);
    }
  };
  lda(0);
  lda(1);
  ldb(0);
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    if (g + 2 < 8) lda(g + 2);
    if (g + 1 < 8) ldb(g + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int q = NW - 1; q >= 0; --q)
#pragma unroll
        for (int j = 0; j < NB; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[g % 3][k][q], b[g & 1][k][j], acc[j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// XP: the fp32 bordered image Xp is stored (p.Xp set).  Off, the instantiation holds none of the store's
// conversions, border stores or address arithmetic.
template <typename TI, bool XP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_vision_fwd_f32(VisF32Params p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kVfLds];
  __shared__ float sb[96];
  unsigned char* const xim = lds + kVfXOff;   // RGBx image; Y1 planes hi, mid, lo at lds + part * kVisYB
  constexpr bool U8 = sizeof(TI) == 1;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5;
  const int Wp = p.W + 2, W1p = p.W1 + 4;
  const int P1 = p.H1 * p.W1, P = p.h * p.w, NC1 = (P1 + 31) / 32, G4 = p.H * p.W / 4;

  {  // zero the whole array once (the borders of planes hi and mid are never written), biases into LDS
    u32x4* z = reinterpret_cast<u32x4*>(lds);
    for (int i = tid; i < kVfLds / 16; i += 256) z[i] = u32x4{0u, 0u, 0u, 0u};
    if (tid < 32) sb[tid] = p.b1[tid];
    else if (tid < 96) sb[tid] = p.b2[tid - 32];
  }

  // the frame's pixels, 4 at a time (12 channel values: 3 dwords of uint8 or 3 x 16 B of fp32)
  constexpr int RW = U8 ? 1 : 4;   // 4-byte words per 4 channel values
  uint32_t raw[kVisNG][3 * RW];
  auto fetch = [&](int f) {
    const uint32_t* src =
        reinterpret_cast<const uint32_t*>(reinterpret_cast<const TI*>(p.frames) + (size_t)f * p.H * p.W * 3);
#pragma unroll
    for (int i = 0; i < kVisNG; ++i) {   // unconditional (clamped) loads
      const int g = min(tid + 256 * i, G4 - 1);
      if constexpr (RW == 4) {
#pragma unroll
        for (int q = 0; q < 12; q += 4) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(src + (size_t)g * 12 + q);
          raw[i][q] = v[0]; raw[i][q + 1] = v[1]; raw[i][q + 2] = v[2]; raw[i][q + 3] = v[3];
        }
      } else {
#pragma unroll
        for (int q = 0; q < 3; ++q) raw[i][q] = src[(size_t)g * 3 + q];
      }
    }
  };
  auto chan = [&](int i, int c) -> float {   // channel value c (0..11) of group i
    if constexpr (RW == 4) return __builtin_bit_cast(float, raw[i][c]);
    else return (float)((raw[i][c >> 2] >> (8 * (c & 3))) & 255u);
  };
  auto part_of = [&](float v, int part) -> __bf16 {   // part 0 hi, 1 mid, 2 lo (gemm.h split3_bf16)
    const __bf16 hi = (__bf16)v;
    if (part == 0) return hi;
    const float r = v - (float)hi;
    const __bf16 mid = (__bf16)r;
    if (part == 1) return mid;
    return (__bf16)(r - (float)mid);
  };
  // the fetched pixels' part ``part`` into the RGBx image; with xo (XP only), the pixels themselves into Xp's interior
  auto build = [&](int part, float* xo) {
#pragma unroll
    for (int i = 0; i < kVisNG; ++i) {
      const int g = tid + 256 * i;
      if (g < G4) {
        const int pix = 4 * g, y = pix / p.W, x = pix - y * p.W;
        unsigned char* d = xim + ((y + 1) * Wp + x + 1) * 8;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<bf16x4*>(d + j * 8) = bf16x4{part_of(chan(i, 3 * j), part), part_of(chan(i, 3 * j + 1), part),
                                                         part_of(chan(i, 3 * j + 2), part), (__bf16)0.f};
        if (XP && xo) {
          f32x4* xd = reinterpret_cast<f32x4*>(xo + ((size_t)(y + 1) * Wp + x + 1) * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) xd[j] = f32x4{chan(i, 3 * j), chan(i, 3 * j + 1), chan(i, 3 * j + 2), 0.f};
        }
      }
    }
  };

  // conv1: wave w takes column blocks w, w + 4, ... (<= 4: P1 <= 512); lane (r32, hh)'s window origin per block
  const int nb1 = (NC1 + 3) / 4;   // the workgroup's largest share
  int bo[4], pp1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    pp1[j] = (wave + 4 * j) * 32 + r32;
    const int pp = min(pp1[j], P1 - 1), oy = pp / p.W1, ox = pp - oy * p.W1;
    bo[j] = (4 * oy * Wp + 4 * ox) * 8 + hh * 16;
  }
  // conv2: wave w takes row block w % 2 over column blocks 2 (w / 2), 2 (w / 2) + 1
  const int rb = wave & 1, cb2 = 2 * (wave >> 1);
  int yb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int pp = min((cb2 + j) * 32 + r32, P - 1), y2 = pp / p.w, x2 = pp - y2 * p.w;
    yb[j] = (2 * y2 * W1p + 2 * x2) * kVisYP + hh * 16;
  }

  int f = blockIdx.x;
  if constexpr (U8)
    if (f < p.F) fetch(f);
  __syncthreads();   // array zeroed, biases in
  for (; f < p.F; f += gridDim.x) {
    int wl = lane;   // laundered: the weight fragments are streamed per frame, not hoisted out of the frame loop
    asm volatile("" : "+v"(wl));
    float* xo = nullptr;
    if constexpr (XP) xo = p.Xp + (size_t)f * (p.H + 2) * Wp * 4;
    // the image's border (plane lo of the previous frame lay over part of it), and Xp's
    for (int i = tid; i < 2 * Wp + 2 * p.H; i += 256) {
      const int px = i < 2 * Wp ? (i < Wp ? i : (p.H + 1) * Wp + i - Wp)
                                : (1 + ((i - 2 * Wp) >> 1)) * Wp + ((i & 1) ? Wp - 1 : 0);
      *reinterpret_cast<uint2*>(xim + px * 8) = uint2{0u, 0u};
      if constexpr (XP) *reinterpret_cast<f32x4*>(xo + (size_t)px * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    if constexpr (U8) {
      build(0, xo);
      if (f + (int)gridDim.x < p.F) fetch(f + gridDim.x);   // next frame's pixels, under this one's convs
      barrier_lds();   // image complete; the next frame's loads stay in flight
      if (nb1 <= 2) vf_conv1_pass<2, 3>(xim, p.W1s, wl, bo, Wp, acc);
      else vf_conv1_pass<4, 3>(xim, p.W1s, wl, bo, Wp, acc);
    } else {
      // fp32 frames: the lo, mid and hi part images in turn (no register prefetch: the frame is re-read per part)
#pragma unroll 1
      for (int part = 2; part >= 0; --part) {
        fetch(f);
        if (part < 2) barrier_lds();   // every wave is done with the previous part image
        build(part, part == 2 ? xo : nullptr);
        barrier_lds();
        if (part == 2) {
          if (nb1 <= 2) vf_conv1_pass<2, 1>(xim, p.W1s, wl, bo, Wp, acc);
          else vf_conv1_pass<4, 1>(xim, p.W1s, wl, bo, Wp, acc);
        } else if (part == 1) {
          if (nb1 <= 2) vf_conv1_pass<2, 2>(xim, p.W1s, wl, bo, Wp, acc);
          else vf_conv1_pass<4, 2>(xim, p.W1s, wl, bo, Wp, acc);
        } else {
          if (nb1 <= 2) vf_conv1_pass<2, 3>(xim, p.W1s, wl, bo, Wp, acc);
          else vf_conv1_pass<4, 3>(xim, p.W1s, wl, bo, Wp, acc);
        }
      }
    }
    barrier_lds();   // every wave is done with the image: plane lo may overwrite it
    // plane lo's border (the image lay over part of it)
    for (int i = tid; i < (p.H1 + 4) * W1p; i += 256) {
      const int y = i / W1p, x = i - y * W1p;
      if (y < 2 || y >= p.H1 + 2 || x < 2 || x >= p.W1 + 2) {
        u32x4* z = reinterpret_cast<u32x4*>(lds + 2 * kVisYB + i * kVisYP);
#pragma unroll
        for (int q = 0; q < 4; ++q) z[q] = u32x4{0u, 0u, 0u, 0u};
      }
    }
    // Y1 = conv1 + bias: fp32 to HBM, its three parts into the planes (interior at +2, +2)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (wave + 4 * j < NC1 && pp1[j] < P1) {
        const int oy = pp1[j] / p.W1, ox = pp1[j] - oy * p.W1;
        unsigned char* yd = lds + ((oy + 2) * W1p + ox + 2) * kVisYP;
        float* yo = p.Y1 + ((size_t)f * P1 + pp1[j]) * 32;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = 8 * g + 4 * hh;
          bf16x4 ph, pm, pl;
          f32x4 y;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            y[e] = acc[j][4 * g + e] + sb[c + e];
            ph[e] = (__bf16)y[e];
            const float r = y[e] - (float)ph[e];
            pm[e] = (__bf16)r;
            pl[e] = (__bf16)(r - (float)pm[e]);
          }
          *reinterpret_cast<f32x4*>(yo + c) = y;
          *reinterpret_cast<bf16x4*>(yd + c * 2) = ph;
          *reinterpret_cast<bf16x4*>(yd + kVisYB + c * 2) = pm;
          *reinterpret_cast<bf16x4*>(yd + 2 * kVisYB + c * 2) = pl;
        }
      }
    }
    barrier_lds();   // Y1 planes complete
    // conv2 -> the ConvLSTM operand slot
    f32x16 acc2[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc2[j][e] = 0.f;
    {
      bf16x8 a[3][2][3], b[2][2][3][2];   // [ring][k step][part]( [column block] )
      const bf16x8* W2 = p.W2s + (size_t)rb * 32 * 3 * 64 + wl;
      auto lda = [&](int g) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
          for (int q = 0; q < 3; ++q) a[g % 3][k][q] = W2[((2 * g + k) * 3 + q) * 64];
      };
      auto ldb = [&](int g) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int ks = 2 * g + k, tap = ks >> 1, off = ((tap >> 2) * W1p + (tap & 3)) * kVisYP + (ks & 1) * 32;
#pragma unroll
          for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              b[g & 1][k][q][j] = *reinterpret_cast<const bf16x8*>(lds + q * kVisYB + yb[j] + off);
        }
      };
      lda(0);
      lda(1);
      ldb(0);
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        if (g + 2 < 16) lda(g + 2);
        if (g + 1 < 16) ldb(g + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const bf16x8(&A)[3] = a[g % 3][k];
          const bf16x8(&B)[3][2] = b[g & 1][k];
          // gemm.h SPLIT6's order (smallest first): lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi
#pragma unroll
          for (int j = 0; j < 2; ++j) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2], B[0][j], acc2[j], 0, 0, 0);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], B[2][j], acc2[j], 0, 0, 0);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], B[1][j], acc2[j], 0, 0, 0);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], B[0][j], acc2[j], 0, 0, 0);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], B[1][j], acc2[j], 0, 0, 0);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], B[0][j], acc2[j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int pp = (cb2 + j) * 32 + r32;
      if (pp < P) {
        float* o = p.out + ((size_t)f * P + pp) * p.out_ld + 32 * rb;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = 8 * g + 4 * hh;
          const float* bz = sb + 32 + 32 * rb + c;
          *reinterpret_cast<f32x4*>(o + c) = f32x4{acc2[j][4 * g] + bz[0], acc2[j][4 * g + 1] + bz[1],
                                                   acc2[j][4 * g + 2] + bz[2], acc2[j][4 * g + 3] + bz[3]};
        }
      }
    }
    barrier_lds();   // every wave is done with the planes: the next image may overwrite plane lo
  }
}

template <typename TI>
inline hipError_t vision_fwd_frames_f32(const VisF32Params& p, int cus, hipStream_t st) {
  if (!vis_fits(p.H, p.W, p.H1, p.W1, p.h, p.w) || p.F < 1) return hipErrorInvalidValue;
  if (p.Xp) hipLaunchKernelGGL((k_vision_fwd_f32<TI, true>), dim3(std::min(p.F, cus)), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((k_vision_fwd_f32<TI, false>), dim3(std::min(p.F, cus)), dim3(256), 0, st, p);
  return hipGetLastError();
}

}  // namespace aaa
