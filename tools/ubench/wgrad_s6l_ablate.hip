// Phase prices and schedule variants of the fp32 (bf16x6 split products) ConvLSTM weight
// gradient at C2 size (B=32, T=20, 11x11: 77440 pixels of K): D[512][1728] += dZ^T * im2col(XH)
// on the split-at-commit 256x256 BK16 tile (gemm.h gemm_kernel_s6l / gemm_kernel_s6p).
//   - the production lock-step kernel, and a copy of its loop with parts removed (ABL bits below:
//     wrong numerics, diagnostic only);
//   - the paired-segment kernel in its variants V (gemm.h), each checked against the lock-step
//     kernel: bit for bit at one K split, and by max |diff| / max |ref| at the production split.
//   tools/ubench/build.sh wgrad_s6l_ablate.hip && tools/ubench/wgrad_s6l_ablate [B] [T] [h] [w]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "loaders_b.h"
#include "epilogues.h"

using namespace aaa;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

// ABL: 1 = the commit's three-way split and LDS writes removed (the loaded registers are still
// waited for), 2 = the fragment reads hoisted out of the K loop, 4 = no global loads in the loop
template <class C, class LA, class LB, class EP, int ABL>
__global__ void __launch_bounds__(C::NT)
s6l_abl_kernel(typename LA::Params pa, typename LB::Params pb, EP ep, int K, int kchunk, TileMap tm) {
  constexpr int BI = C::BI, BJ = C::BJ, BK = C::BK, WJ = C::WJ;
  constexpr int WTI = BI / C::WI, WTJ = BJ / WJ, MI = WTI / 32, MJ = WTJ / 32;
  static_assert(BK == 16 && C::FD == 2, "the production tile");
  using TA = TileK<__bf16, BI, BK, LA::KC>;
  using TB = TileK<__bf16, BJ, BK, LB::KC>;
  constexpr int PA = TA::ELEMS, PB = TB::ELEMS, STG = 3 * (PA + PB);
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * STG];
  int ti, tj, tz;
  tile_of(tm, ti, tj, tz);
  const int i0 = ti * BI, j0 = tj * BJ;
  const int kb = tz * kchunk;
  const int ke = min(K, kb + kchunk);
  if (kb >= ke) return;
  LA la(pa, i0);
  LB lb(pb, j0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = wave / WJ, wj = wave - (wave / WJ) * WJ;
  const int r32 = lane & 31, h = lane >> 5;
  f32x16 acc[MI][MJ];
#pragma unroll
  for (int a = 0; a < MI; ++a)
#pragma unroll
    for (int b = 0; b < MJ; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  const int nk = (ke - kb + BK - 1) / BK;
  typename LA::Regs ra[2];
  typename LB::Regs rb[2];
  la.fetch(kb, ke, ra[0]);
  lb.fetch(kb, ke, rb[0]);
  la.fetch(kb + BK, ke, ra[1]);
  lb.fetch(kb + BK, ke, rb[1]);
  la.commit3(smem, PA, ra[0]);
  lb.commit3(smem + 3 * PA, PB, rb[0]);
  __syncthreads();
  auto commit = [&](__bf16* dst, const typename LA::Regs& xa, const typename LB::Regs& xb) {
    if constexpr (ABL & 1) {   // consume the registers (the wait for the loads stays), no split, no LDS write
      uint32_t x = 0;
#pragma unroll
      for (int c = 0; c < LA::PER; ++c) x |= xa[c][0] ^ xa[c][1] ^ xa[c][2] ^ xa[c][3];
#pragma unroll
      for (int c = 0; c < LB::PER; ++c) x |= xb[c][0] ^ xb[c][1] ^ xb[c][2] ^ xb[c][3];
      if (x == 0x7fc12345u) dst[threadIdx.x] = (__bf16)1.f;
    } else {
      la.commit3(dst, PA, xa);
      lb.commit3(dst + 3 * PA, PB, xb);
    }
  };
  auto frags = [&](const __bf16* cur, bf16x8 (&af)[MI][3], bf16x8 (&bfr)[MJ][3]) {
    const int kofs = 8 * h;
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
      for (int p = 0; p < 3; ++p) af[a][p] = frag_bf16<TA>(cur + p * PA, wi * WTI + a * 32 + r32, kofs);
#pragma unroll
    for (int b = 0; b < MJ; ++b)
#pragma unroll
      for (int p = 0; p < 3; ++p) bfr[b][p] = frag_bf16<TB>(cur + 3 * PA + p * PB, wj * WTJ + b * 32 + r32, kofs);
  };
  bf16x8 haf[MI][3], hbfr[MJ][3];
  if constexpr (ABL & 2) frags(smem, haf, hbfr);
  auto step = [&](int kt, auto E) {
    constexpr int e = decltype(E)::value;
    const bool more = kt + 1 < nk;
    if constexpr (!(ABL & 4)) {
      la.fetch(kb + (kt + 2) * BK, ke, ra[e]);
      lb.fetch(kb + (kt + 2) * BK, ke, rb[e]);
    }
    bf16x8 laf[MI][3], lbfr[MJ][3];
    if constexpr (!(ABL & 2)) frags(smem + e * STG, laf, lbfr);
    auto& af = (ABL & 2) ? haf : laf;
    auto& bfr = (ABL & 2) ? hbfr : lbfr;
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
      for (int b = 0; b < MJ; ++b) {
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a][2], bfr[b][0], acc[a][b], 0, 0, 0);
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a][0], bfr[b][2], acc[a][b], 0, 0, 0);
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a][1], bfr[b][1], acc[a][b], 0, 0, 0);
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a][1], bfr[b][0], acc[a][b], 0, 0, 0);
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a][0], bfr[b][1], acc[a][b], 0, 0, 0);
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a][0], bfr[b][0], acc[a][b], 0, 0, 0);
      }
    if (more) commit(smem + (e ^ 1) * STG, ra[e ^ 1], rb[e ^ 1]);
    __syncthreads();
  };
  for (int kt = 0; kt < nk; kt += 2) {
    step(kt, std::integral_constant<int, 0>{});
    if (kt + 1 < nk) step(kt + 1, std::integral_constant<int, 1>{});
  }
#pragma unroll
  for (int a = 0; a < MI; ++a)
#pragma unroll
    for (int b = 0; b < MJ; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = i0 + wi * WTI + a * 32 + 8 * g + 4 * h;
        const int j = j0 + wj * WTJ + b * 32 + r32;
        ep(i, j, acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]);
      }
}

template <class F>
static float time_us(F&& launch, int reps = 20) {
  for (int i = 0; i < 3; ++i) launch();
  CK(hipDeviceSynchronize());
  hipEvent_t a, b;
  CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  CK(hipEventRecord(a, 0));
  for (int i = 0; i < reps; ++i) launch();
  CK(hipEventRecord(b, 0));
  CK(hipEventSynchronize(b));
  float ms; CK(hipEventElapsedTime(&ms, a, b));
  return ms * 1e3f / reps;
}

static float* dev_rand(size_t n, unsigned seed) {
  std::vector<float> h(n);
  unsigned s = seed;
  for (auto& v : h) { s = s * 1664525u + 1013904223u; v = ((s >> 8) & 0xffff) / 32768.f - 1.f; }
  float* d; CK(hipMalloc(&d, n * 4)); CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
  return d;
}

using C = GemmCfgS6L<256, 256, 16, 2, 4, 2>;
using CK_ = GemmCfgS6LK<256, 256, 16, 2, 4, 2>;   // the K loop in pairs
using LA = LdRowsTB<float, float, C::BI, C::BK, C::NT>;
using LB = LdIm2colTB<float, float, C::BJ, C::BK, C::NT>;
using CI_ = GemmCfgS6LK<256, 256, 16, 2, 4, 2, 1>;   // and the commit issued among the MFMAs (production)
using EP = EpiStore<true>;

struct Problem {
  const float *dz, *xh;
  float* out;
  int rows, h, w;
  LA::Params pa() const { return {dz, 512, 512, rows}; }
  LB::Params pb() const {
    return {xh, ConvGeo{192, 192, 0, h, w, h, w, 3, 1, 1, 0}.prep(), 1728, (uint32_t)((size_t)rows * 192 * 4)};
  }
  EP ep() const { return {out, 1728, 512, 1728}; }
  int splits(int wgs) const { return std::max(1, std::min(wgs / 14, rows / C::BK)); }
};

// kind: -1 = gemm_kernel_s6l (the parent's loop), 0..7 = gemm_kernel_s6p<V>, 8 = gemm_kernel_s6l on
// GemmCfgS6LK with the K loop in pairs alone, 9 = with the commit among the MFMAs as well (production)
template <int V>
static void launch_p(const Problem& P, int ns) { CK((launch_gemm_s6p<C, LA, LB, V>(P.pa(), P.pb(), P.ep(), 512, 1728, P.rows, ns, 0))); }
static void launch_kind(const Problem& P, int kind, int ns) {
  switch (kind) {
    case -1: CK((launch_gemm<C, LA, LB>(P.pa(), P.pb(), P.ep(), 512, 1728, P.rows, ns, 0))); break;
    case 8: CK((launch_gemm<CK_, LA, LB>(P.pa(), P.pb(), P.ep(), 512, 1728, P.rows, ns, 0))); break;
    case 9: CK((launch_gemm<CI_, LA, LB>(P.pa(), P.pb(), P.ep(), 512, 1728, P.rows, ns, 0))); break;
    case 0: launch_p<0>(P, ns); break;
    case 1: launch_p<1>(P, ns); break;
    case 2: launch_p<2>(P, ns); break;
    case 3: launch_p<3>(P, ns); break;
    case 4: launch_p<4>(P, ns); break;
    case 5: launch_p<5>(P, ns); break;
    case 6: launch_p<6>(P, ns); break;
    default: launch_p<7>(P, ns); break;
  }
}
template <int ABL>
static void run_abl(const char* name, const Problem& P) {
  const int ns = P.splits(256);
  int kchunk = (P.rows + ns - 1) / ns;
  kchunk = (kchunk + C::BK - 1) / C::BK * C::BK;
  dim3 grid(7, 2, (P.rows + kchunk - 1) / kchunk);
  const float us = time_us([&] {
    hipLaunchKernelGGL((s6l_abl_kernel<C, LA, LB, EP, ABL>), grid, dim3(C::NT), 0, 0, P.pa(), P.pb(), P.ep(), P.rows, kchunk,
                       tile_map(grid));
  });
  printf("%-58s %9.1f us\n", name, us);
}
static std::vector<float> result(const Problem& P, int kind, int ns) {
  CK(hipMemset(P.out, 0, (size_t)512 * 1728 * 4));
  launch_kind(P, kind, ns);
  std::vector<float> r((size_t)512 * 1728);
  CK(hipMemcpy(r.data(), P.out, r.size() * 4, hipMemcpyDeviceToHost));
  return r;
}

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 32, T = argc > 2 ? atoi(argv[2]) : 20;
  const int h = argc > 3 ? atoi(argv[3]) : 11, w = argc > 4 ? atoi(argv[4]) : 11;
  const int rows = T * B * h * w;
  Problem P{dev_rand((size_t)rows * 512, 3), dev_rand((size_t)rows * 192, 10), nullptr, rows, h, w};
  CK(hipMalloc(&P.out, (size_t)512 * 1728 * 4));
  printf("rows %d (%dx%d grid), %d K splits\n", rows, h, w, P.splits(256));

  // correctness of the paired variants first: one split is bit for bit, the production split to reorder noise
  const std::vector<float> r1 = result(P, -1, 1), rn = result(P, -1, P.splits(256)), rn2 = result(P, -1, P.splits(256));
  float amax = 0.f, old = 0.f;
  for (size_t i = 0; i < rn.size(); ++i) { amax = std::max(amax, std::fabs(rn[i])); old = std::max(old, std::fabs(rn[i] - rn2[i])); }
  printf("lock-step vs itself at the production split: max |diff| / max |ref| %.3g\n", old / amax);
  bool ok = true;
  for (int v = 0; v < 10; ++v) {
    const std::vector<float> p1 = result(P, v, 1), pn = result(P, v, P.splits(256));
    const bool same = !memcmp(p1.data(), r1.data(), r1.size() * 4);
    float d = 0.f;
    for (size_t i = 0; i < rn.size(); ++i) d = std::max(d, std::fabs(rn[i] - pn[i]));
    printf("kind %d: one split %s, production split max |diff| / max |ref| %.3g\n", v,
           same ? "bit-identical" : "DIFFERS", d / amax);
    ok = ok && same && d / amax < 1e-5f;
  }
  if (!ok) { printf("FAILED: a variant differs from the lock-step kernel\n"); return 1; }

  const int ns = P.splits(256);
  for (int rep = 0; rep < 2; ++rep) {
    printf("%-58s %9.1f us\n", "lock-step gemm_kernel_s6l (the parent's loop)", time_us([&] { launch_kind(P, -1, ns); }));
    printf("%-58s %9.1f us\n", "lock-step, K loop in pairs", time_us([&] { launch_kind(P, 8, ns); }));
    printf("%-58s %9.1f us\n", "lock-step, K loop in pairs, commit among the MFMAs", time_us([&] { launch_kind(P, 9, ns); }));
    for (int v = 0; v < 8; ++v) {
      char name[96];
      snprintf(name, sizeof name, "paired gemm_kernel_s6p V=%d%s%s%s", v, v & 1 ? " prio" : "", v & 2 ? " reads-ahead" : "",
               v & 4 ? " fetch kt+2 first" : "");
      printf("%-58s %9.1f us\n", name, time_us([&] { launch_kind(P, v, ns); }));
    }
  }
  run_abl<0>("lock-step copy (ablation kernel, nothing removed)", P);
  run_abl<1>("  no commit split / LDS writes", P);
  run_abl<2>("  fragment reads hoisted", P);
  run_abl<3>("  neither (MFMA + loads + barriers)", P);
  run_abl<4>("  no global loads in the loop", P);
  run_abl<7>("  MFMA + barriers only", P);
  run_abl<0>("lock-step copy (again)", P);
  return 0;
}
