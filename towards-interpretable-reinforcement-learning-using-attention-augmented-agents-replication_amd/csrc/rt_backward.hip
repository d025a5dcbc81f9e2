// Backward of the unroll (what autograd runs for main_mp.py:77): the batched
// tail backward, the ConvLSTM BPTT (frame-resident / frame-group / per-step),
// the conv / ConvLSTM weight gradients and the vision encoder backward.
#include "rt.h"

namespace aaa {


// conv2 dgrad (stride 2, k4, pad 2) as four parity-class 2x2 convs over dY2:
// output pixel (2a+py, 2b+px) only receives taps ky = py + 2(1-ty), kx = px + 2(1-tx).
template <typename T>
static int conv2_dgrad(const Layout& L, const char* pk, const T* dy2, T* dy1, int frames, float* gbias,
                       hipStream_t s) {
  {
    // small grids: the four classes share one gather (output (a, b) reads dY2
    // (a + ty, b + tx)), so one 128-row tile (class-major rows, [cls][32][256]
    // = k_WdT2) per frame reads the frame's dY2 once as a zero-bordered LDS
    // image (halo.h, KS = 2) -- one launch instead of four 32-row GEMMs whose
    // K = 256 loops were pure latency (4 x 65 us at C3, 0.06 of bf16 peak)
    constexpr int CKd = std::is_same<T, float>::value ? 32 : 64;
    const int Ha = (L.H1 + 1) / 2, Wa = (L.W1 + 1) / 2;
    auto halo4 = [&](auto cfg, auto nbuf) -> int {
      using HC = decltype(cfg);
      EpiStoreParity4<T> ep(dy1, frames * Ha * Wa, Ha, Wa, L.H1, L.W1, gbias);
      const HaloParams hp{pk + L.k_WdT2, 256, 128, dy2, 64, 0, 64, (uint32_t)((size_t)frames * L.P * 64 * L.esz),
                          L.h, L.w, frames, 0, Ha, Wa};
      HIPCHK((launch_halo<HC, EpiStoreParity4<T>, 2, decltype(nbuf)::value>(hp, ep, s)));
      return AAA_OK;
    };
    using NB3 = std::integral_constant<int, 3>;
    auto fits = [&](int fr, int bj, int hmax) {
      return fr * Ha * Wa <= bj && fr * (L.h + 2) * (L.w + 2) + 1 <= hmax && Ha <= L.h && Wa <= L.w;
    };
    // bf16: FR = 2 frames per tile -- the 64 KB weight tile streamed once per two frames and twice the
    // MFMA work per DMA round trip (C3 4.97 -> 4.94 ms); fp32 keeps FR = 1 (C2 4.306 vs 4.341 ms)
    // (profiles/r02/ab/dgrad_fr.txt; AAA_DGRAD2_FR overrides)
    const int fr = ab_int("AAA_DGRAD2_FR", std::is_same<T, float>::value ? 1 : 2);
    if (ab_int("AAA_DGRAD2_HALO", 1)) {
      if (fr == 2 && fits(2, 256, 352)) return halo4(HaloCfg<T, 128, 256, CKd, 2, 2, 2, 352>{}, NB3{});
      if constexpr (std::is_same<T, float>::value) {   // fp32 accuracy on the bf16 MFMA (gemm.h SPLIT6)
        // AAA_DGRAD2_NBUF=2 (A/B): a 2-stage weight ring, 80 KB of LDS -> two workgroups per CU
        if (f32_split6() && fits(1, 128, 192)) {
          if (ab_int("AAA_DGRAD2_NBUF", 3) == 2)
            return halo4(HaloCfgS6<128, 128, CKd, 2, 2, 1, 192>{}, std::integral_constant<int, 2>{});
          return halo4(HaloCfgS6<128, 128, CKd, 2, 2, 1, 192>{}, NB3{});
        }
      }
      if (fits(1, 128, 192)) return halo4(HaloCfg<T, 128, 128, CKd, 2, 2, 1, 192>{}, NB3{});
      // bf16, grids up to 21x21 (168x168 frames, C5): one frame per 512-column tile of 8 waves,
      // 32-channel chunks (two LDS images of 23x23 pixels), the epilogue in two column chunks
      if constexpr (!std::is_same<T, float>::value)
        if (fits(1, 512, 640) && ab_int("AAA_DGRAD2_WIDE", 1)) return halo4(HaloCfg<T, 128, 512, 32, 2, 4, 1, 640>{}, NB3{});
    }
  }
  // One 32-row GEMM per parity class: D[32][rows] = WdT2[cls] x the class's 2x2 gather of dY2 (K = 256);
  // launch(Wc, g, py, px, Ha, Wa, rows) runs it on the ring or register-staged
  const uint32_t dy2_bytes = (uint32_t)((size_t)frames * L.P * 64 * L.esz);
  auto classes = [&](auto launch) -> int {
    for (int cls = 0; cls < 4; ++cls) {
      const int py = cls >> 1, px = cls & 1;
      const int Ha = (L.H1 - py + 1) / 2, Wa = (L.W1 - px + 1) / 2;
      if (Ha <= 0 || Wa <= 0) continue;
      const int rc = launch((const T*)(pk + L.k_WdT2) + (size_t)cls * 32 * 256,
                            ConvGeo{64, 64, 0, L.h, L.w, Ha, Wa, 2, 1, 0, 0}.prep(), py, px, Ha, Wa, frames * Ha * Wa);
      if (rc) return rc;
    }
    return AAA_OK;
  };
  if (ab_int("AAA_CONV2_DGRAD_RING", 1)) {
    // the LDS-DMA ring (dY2 is already in T), dY1 stored in T, conv1's bias
    // gradient summed from the fp32 values in the epilogue (no column-sum pass)
    constexpr int BKd = std::is_same<T, float>::value ? 32 : 64;
    auto ring = [&](auto cfg) -> int {
      using CP = decltype(cfg);
      using PA = GRowsB<T, CP::BI, CP::BK, CP::NT>;
      using PB = GIm2colB<T, CP::BJ, CP::BK, CP::NT>;
      return classes([&](const T* Wc, const ConvGeo& g, int py, int px, int Ha, int Wa, int rows) -> int {
        EpiStoreParityBias<T> ep{dy1, 32, rows, Ha, Wa, L.H1, L.W1, py, px, gbias};
        HIPCHK((launch_pipe<CP, PA, PB, EpiStoreParityBias<T>, 2>(typename PA::Params{Wc, 256, 32},
                                                                  typename PB::Params{dy2, g, rows, dy2_bytes}, ep, 32,
                                                                  rows, 256, 1, s)));
        return AAA_OK;
      });
    };
    // K = 256: four BK steps per tile, so 256 columns per workgroup (twice the MFMA work per DMA round
    // trip of 32x128): C5 14.945 -> 14.74 ms per iteration (profiles/r02/ab/vision_tiles.txt); AAA_DGRAD2_TILE=0 the old tile
    return ab_int("AAA_DGRAD2_TILE", 1) == 1 ? ring(GemmCfg<T, 32, 256, BKd, 1, 4>{})
                                             : ring(GemmCfg<T, 32, 128, BKd, 1, 4>{});
  }
  // register-staged fallback (fp32 only: dY2's loader converts from fp32)
  if constexpr (!std::is_same<T, float>::value) return fail(AAA_E_ARG, "AAA_CONV2_DGRAD_RING=0 needs fp32");
  using C3 = Cfg32For<T>;
  using LA = LdRowsB<T, T, C3::BI, C3::BK, C3::NT>;
  using LB = LdIm2colB<float, T, C3::BJ, C3::BK, C3::NT>;
  return classes([&](const T* Wc, const ConvGeo& g, int py, int px, int Ha, int Wa, int rows) -> int {
    EpiStoreParity ep{(float*)dy1, 32, rows, Ha, Wa, L.H1, L.W1, py, px, FastDiv((uint32_t)(Ha * Wa)),
                      FastDiv((uint32_t)Wa)};
    HIPCHK((launch_gemm<C3, LA, LB>(typename LA::Params{Wc, 256, 32},
                                    typename LB::Params{(const float*)dy2, g, rows, dy2_bytes}, ep, 32, rows, 256, 1, s)));
    return AAA_OK;
  });
}

// conv2 weight gradient over ``frames`` frames: gW[64][(ky*4+kx)*32 + ci] +=
// dY2^T x im2col(Y1) (k = output pixel), split-K atomics into a zeroed gW.
template <typename T>
static int conv2_wgrad(const Layout& L, const T* dy2, const T* y1, int frames, float* gW, hipStream_t s) {
  using C = CfgFor<T>;
  // the problem: A = dY2 (rows x 64), B = im2col(Y1) (512 columns) under g, K = rows, D = gW[64][512]
  const int rows = frames * L.P;
  const ConvGeo g = ConvGeo{32, 32, 0, L.H1, L.W1, L.h, L.w, 4, 2, 2, 0}.prep();
  const uint32_t y1_bytes = (uint32_t)((size_t)frames * L.P1 * 32 * L.esz);
  if constexpr (!std::is_same<T, float>::value) {
    // bf16 (AAA_CONV2_WGRAD_PIPE): the LDS-DMA ring of the ConvLSTM weight gradient, 64x256
    // tiles of 4 waves, split-K over about one wave of workgroups, atomics from the accumulators
    // default 1 (C3 1.063M -> 1.075M frames/s, C5 277.4k -> 279.0k vs the register-staged GEMM;
    // 2 = the read-ahead ring, slower here: profiles/r03/ab/convwgrad/); 0 = register-staged
    const int pipe = env_int("AAA_CONV2_WGRAD_PIPE", 1);
    if (rows % 32 == 0 && pipe) {
      using CW = GemmCfg<T, 64, 256, 32, 1, 4>;
      using PA = GRowsT<T, CW::BI, CW::BK, CW::NT>;
      using PB = GIm2colT<T, CW::BJ, CW::BK, CW::NT>;
      const int ns = std::max(1, std::min(ab_int("AAA_CONV2_WGRAD_WGS", 256) / 2, rows / (8 * CW::BK)));
      const typename PA::Params pa{dy2, 64, 64, rows};
      const typename PB::Params pb{y1, g, 512, y1_bytes};
      const EpiAtomicD ep{{gW, 512, 64, 512}};
      if (pipe == 2) HIPCHK((launch_pipe_ra<CW, PA, PB, EpiAtomicD, 4>(pa, pb, ep, 64, 512, rows, ns, s)));
      else HIPCHK((launch_pipe<CW, PA, PB, EpiAtomicD, 4, 2>(pa, pb, ep, 64, 512, rows, ns, s)));
      return AAA_OK;
    }
  }
  auto staged = [&](auto cfg, int ns) -> int {   // a register-staged tile, ns-way split-K atomics
    using CW = decltype(cfg);
    using LA = LdRowsTB<T, T, CW::BI, CW::BK, CW::NT>;
    using LB = LdIm2colTB<T, T, CW::BJ, CW::BK, CW::NT>;
    HIPCHK((launch_gemm<CW, LA, LB>(typename LA::Params{dy2, 64, 64, rows}, typename LB::Params{y1, g, 512, y1_bytes},
                                    EpiStore<true>{gW, 512, 64, 512}, 64, 512, rows, ns, s)));
    return AAA_OK;
  };
  const int ns = wgrad_splits(cdiv(64, C::BI) * cdiv(512, C::BJ), rows, C::BK);
  if constexpr (std::is_same<T, float>::value) {
    if (f32_split6()) {   // the same tile at fp32 accuracy on the bf16 MFMA (gemm.h SPLIT6)
#ifdef AAA_ABLATION
      // A/B (AAA_CONV2_WGRAD_S6L, ablation builds): split-at-commit tiles -- slower here (C2 59.4 ->
      // 67.9 us for 64x256, profiles/r05/ab/conv_wgrad_s6l/)
      auto s6l = [&](auto cfg, int want) { return staged(cfg, std::max(1, std::min(want, rows / 128))); };
      const int c2s = ab_int("AAA_CONV2_WGRAD_S6L", 0);
      if (c2s == 1) return s6l(GemmCfgS6L<64, 256, 16, 1, 4, 2>{}, 256);
      if (c2s == 2) return s6l(GemmCfgS6L<64, 256, 16, 2, 4, 2>{}, 128);
      if (c2s == 3) return s6l(GemmCfgS6L<64, 128, 16, 1, 2, 2>{}, 256);
#endif
      return staged(typename S6Of<C>::type{}, ns);
    }
  }
  return staged(C{}, ns);
}

// conv1 weight gradient over RGBx frames (Cin 4; the 4th channel's grad is dropped on unpack)
template <typename T>
static int conv1_wgrad(const Layout& L, const T* dy1, const T* xp, int frames, float* gW, hipStream_t s) {
  // the problem: A = dY1 (rows1 x 32), B = im2col(Xp) (256 = 8x8 taps x 4 channels columns) under g,
  // K = rows1, D = gW[32][256]
  const int rows1 = frames * L.P1;
  const ConvGeo g = ConvGeo{4, 4, 0, L.H + 2, L.W + 2, L.H1, L.W1, 8, 4, 0, 0}.prep();
  const uint32_t xp_bytes = (uint32_t)((size_t)frames * (L.H + 2) * (L.W + 2) * 4 * L.esz);
  auto staged = [&](auto cfg, int ns) -> int {   // a register-staged tile, ns-way split-K atomics
    using CW = decltype(cfg);
    using LA = LdRowsTB<T, T, CW::BI, CW::BK, CW::NT>;
    using LB = LdIm2colTB<T, T, CW::BJ, CW::BK, CW::NT>;   // bf16 chunks = 2 taps x 4 ch, in-bounds (bordered image)
    HIPCHK((launch_gemm<CW, LA, LB>(typename LA::Params{dy1, 32, 32, rows1}, typename LB::Params{xp, g, 256, xp_bytes},
                                    EpiStore<true>{gW, 256, 32, 256}, 32, 256, rows1, ns, s)));
    return AAA_OK;
  };
  auto run = [&](auto cfg) -> int {
    using C3 = decltype(cfg);
    const int ns = wgrad_splits(cdiv(32, C3::BI) * cdiv(256, C3::BJ), rows1, C3::BK);
    if constexpr (std::is_same<T, float>::value)
      if (f32_split6()) return staged(typename S6Of<C3>::type{}, ns);   // fp32 accuracy on the bf16 MFMA (gemm.h SPLIT6)
    return staged(cfg, ns);
  };
  if constexpr (!std::is_same<T, float>::value) {
    // bf16 on the LDS-DMA rings (AAA_CONV1_WGRAD_PIPE 1: pipe, 2: read-ahead): one 32x256 tile of 4
    // waves over all (tap, channel) columns, BK = 64 pixels; a 16-B piece = 2 taps x 4 channels,
    // contiguous in the bordered RGBx image (KW = 8 even, pad 0: every piece in bounds)
    // default 1 (C3 +0.5 %, C5 +0.8 % vs the register-staged GEMM: profiles/r03/ab/convwgrad/)
    const int pipe = env_int("AAA_CONV1_WGRAD_PIPE", 1);
    if (rows1 % 64 == 0 && pipe) {
      using CW = GemmCfg<T, 32, 256, 64, 1, 4>;
      using PA = GRowsT<T, CW::BI, CW::BK, CW::NT>;
      using PB = GIm2colT<T, CW::BJ, CW::BK, CW::NT>;
      const typename PA::Params pa{dy1, 32, 32, rows1};
      const typename PB::Params pb{xp, g, 256, xp_bytes};
      const EpiAtomicD ep{{gW, 256, 32, 256}};
      const int ns = std::max(1, std::min(ab_int("AAA_CONV1_WGRAD_WGS", 256), rows1 / (8 * CW::BK)));
      if (pipe == 2) HIPCHK((launch_pipe_ra<CW, PA, PB, EpiAtomicD, 4>(pa, pb, ep, 32, 256, rows1, ns, s)));
      else HIPCHK((launch_pipe<CW, PA, PB, EpiAtomicD, 4, 2>(pa, pb, ep, 32, 256, rows1, ns, s)));
      return AAA_OK;
    }
  }
  if constexpr (std::is_same<T, float>::value) {
    // split-at-commit tile over all 256 (tap, channel) columns (GemmCfgS6L: each operand split once
    // at its LDS commit, two K tiles of loads in flight), 512-way split-K: C2 76.9 -> 66.9 us against
    // the 32x64 split6 tile (AAA_CONV1_WGRAD_S6L=0 in ablation builds; 2, 3: other tiles / splits,
    // slower: profiles/r05/ab/conv_wgrad_s6l/)
    const int c1s = f32_split6() ? ab_int("AAA_CONV1_WGRAD_S6L", 1) : 0;
    auto s6l = [&](auto cfg, int want) { return staged(cfg, std::max(1, std::min(want, rows1 / 128))); };
    if (c1s == 1)   // uint8 frames: the RGBx operand exact in bf16 (GemmCfgS6LBX: three of the six products)
      return L.fu8 && ab_int("AAA_CONV1_BEXACT", 1) ? s6l(GemmCfgS6LBX<32, 256, 16, 1, 4, 2>{}, 512)
                                                     : s6l(GemmCfgS6L<32, 256, 16, 1, 4, 2>{}, 512);
#ifdef AAA_ABLATION
    if (c1s == 2) return s6l(GemmCfgS6L<32, 256, 16, 1, 4, 2>{}, 256);
    if (c1s == 3) return s6l(GemmCfgS6L<32, 128, 16, 1, 2, 2>{}, 512);
#endif
  }
  // AAA_CONV1_WGRAD_TILE=1 (A/B): one 32x256 tile covering every (tap, channel) column, so each
  // pixel's 8x8 window is gathered once instead of by four 64-column tiles
  if (ab_int("AAA_CONV1_WGRAD_TILE", 0) == 1) return run(GemmCfg<T, 32, 256, Cfg32For<T>::BK, 1, 4>{});
  return run(Cfg32For<T>{});
}

// All 8 ConvLSTM weight gradients of ``rows`` pixels at once (attention.py:39-102
// as used at :119-122): gW[512 = 4ch+gate][1728 = tap*192 + c'] += dZ^T x
// im2col(XH) with k = pixel, accumulated (split-K atomics) into a zeroed gW.
// ``aux``: issued on the low-priority overlap stream.
template <typename T>
int lstm_wgrad(const T* dz, const T* xh, int rows, int h, int w, float* gW, hipStream_t s, bool aux) {
  // the problem: A = dZ (rows x 512), B = im2col(XH) (1728 columns) under g, K = rows, D = gW[512][1728]
  const ConvGeo g = ConvGeo{192, 192, 0, h, w, h, w, 3, 1, 1, 0}.prep();
  const uint32_t xh_bytes = (uint32_t)((size_t)rows * 192 * sizeof(T));
  const double flop = 2.0 * 512 * 1728 * rows;
  auto wgrad_lstm = [&](auto cfg) -> int {   // register-staged, split-K atomics
    using CW = decltype(cfg);
    using LA = LdRowsTB<T, T, CW::BI, CW::BK, CW::NT>;
    using LB = LdIm2colTB<T, T, CW::BJ, CW::BK, CW::NT>;
    const typename LA::Params pa{dz, 512, 512, rows};
    const typename LB::Params pb{xh, g, 1728, xh_bytes};
    const EpiStore<true> ep{gW, 1728, 512, 1728};
    const int tiles = cdiv(512, CW::BI) * cdiv(1728, CW::BJ);
    // about two workgroups per CU of splits (both fit a CU; the 1024-WG rule of
    // the other weight gradients doubled the output atomics for the same time:
    // profiles/r02/ab/wgrad_split.txt)
    // (split-at-commit tiles hold 110 KB of LDS: one workgroup per CU, so one split per CU:
    // C2 655 us at 18-way against 679 at 36 and 845 at 27, profiles/r05/ab/wgrad_s6l/)
    const int per_cu = split6l_of<CW>::value ? device_cus() : 512;
    const int ns = std::max(1, std::min(ab_int("AAA_WGRAD_SPLIT", std::max(1, per_cu / tiles)), rows / CW::BK));
    // The production split-at-commit tile (8 waves, two register stages), AAA_WGRAD_S6_PAIRED:
    // 1 (default) = the K loop in whole pairs of tiles and each commit issued among the MFMAs (gemm.h
    // GemmCfgS6LK: the same sums per workgroup), 0 = the loop of gemm_kernel_s6l as it was; ablation
    // builds: 2 = the two-segment paired kernel (gemm_kernel_s6p), 3 = the K loop in pairs alone.
    // C2, two boxes: 603 / 621 (0), 587 / 605 (3), 573 / 588 (1), 643 / 666 (2) us, profiles/r07/ab/wgrad_pp/
    if constexpr (s6p_of<CW>::value) {
      int sched = env_int("AAA_WGRAD_S6_PAIRED", 1);
#ifndef AAA_ABLATION
      if (sched > 1) sched = 1;
#endif
      auto run = [&](auto cfg, const char* what, auto paired) -> int {
        using CK = decltype(cfg);
        TimerScope tim(AAA_TIMER_CORE_WGRAD, s, flop,
                       strf("register-staged %dx%d BK%d (fp32 as bf16x6 split products), %s, %d-way split-K atomics "
                            "[kernel: %s+LdIm2colTB]", CW::BI, CW::BJ, CW::BK, what, ns,
                            decltype(paired)::value ? "gemm_kernel_s6p" : "gemm_kernel_s6l+GemmCfgS6LK"));
        if constexpr (decltype(paired)::value) HIPCHK((launch_gemm_s6p<CK, LA, LB>(pa, pb, ep, 512, 1728, rows, ns, s)));
        else HIPCHK((launch_gemm<CK, LA, LB>(pa, pb, ep, 512, 1728, rows, ns, s)));
        return AAA_OK;
      };
      if (sched == 1)
        return run(GemmCfgS6LK<CW::BI, CW::BJ, CW::BK, CW::WI, CW::WJ, 2, 1>{},
                   "K loop in pairs, commits among the MFMAs", std::false_type{});
#ifdef AAA_ABLATION
      if (sched == 2) return run(CW{}, "paired MFMA / commit segments", std::true_type{});
      if (sched == 3)
        return run(GemmCfgS6LK<CW::BI, CW::BJ, CW::BK, CW::WI, CW::WJ, 2, 0>{}, "K loop in pairs", std::false_type{});
#endif
    }
    TimerScope tim(AAA_TIMER_CORE_WGRAD, s, flop,
                   strf("register-staged %dx%d BK%d%s, %d-way split-K atomics [kernel: gemm_kernel+%d, %d, %d, +LdIm2colTB]",
                        CW::BI, CW::BJ, CW::BK, split6_of<CW>::value ? " (fp32 as bf16x6 split products)" : "", ns,
                        CW::BI, CW::BJ, CW::BK));
    HIPCHK((launch_gemm<CW, LA, LB>(pa, pb, ep, 512, 1728, rows, ns, s)));
    return AAA_OK;
  };
  // LDS-DMA ring with transposed fragment reads for both operands (k = pixel)
  // and the split-K atomics straight from the accumulators
  // ilv: launch_pipe's DMA issue interleave, or kReadAhead for the read-ahead ring (glds.h
  // gemm_pipe_ra_kernel: fragments of tile kt+1 read during the MFMAs of tile kt)
  constexpr int kReadAhead = -1;
  auto wgrad_lstm_pipe = [&](auto cfg, auto nbuf, auto ilv) -> int {
    using CW = decltype(cfg);
    constexpr int NB = decltype(nbuf)::value, IL = decltype(ilv)::value;
    constexpr bool ra = IL == kReadAhead;
    using LA = GRowsT<T, CW::BI, CW::BK, CW::NT>;
    using LB = GIm2colT<T, CW::BJ, CW::BK, CW::NT>;
    const typename LA::Params pa{dz, 512, 512, rows};
    const typename LB::Params pb{xh, g, 1728, xh_bytes};
    const EpiAtomicD ep{{gW, 1728, 512, 1728}};
    const int tiles = cdiv(512, CW::BI) * cdiv(1728, CW::BJ);
    TimerScope tim(AAA_TIMER_CORE_WGRAD, s, flop,
                   strf("LDS-DMA %sring %dx%d BK%d, %d-deep [kernel: %s+GIm2colT]", ra ? "read-ahead " : "", CW::BI, CW::BJ,
                        CW::BK, NB, ra ? "gemm_pipe_ra_kernel" : "gemm_pipe_kernel"));
    // split-K over pixels: about one resident wave of workgroups (fewer
    // passes of the output's atomics than the register path's ~1024)
    const int wgs = ab_int("AAA_WGRAD_WGS", 256);
    const int ns = std::max(1, std::min(wgs / tiles, rows / (8 * CW::BK)));
    if constexpr (ra) HIPCHK((launch_pipe_ra<CW, LA, LB, EpiAtomicD, NB>(pa, pb, ep, 512, 1728, rows, ns, s)));
    else HIPCHK((launch_pipe<CW, LA, LB, EpiAtomicD, NB, IL>(pa, pb, ep, 512, 1728, rows, ns, s)));
    return AAA_OK;
  };
  // bf16 default (9): 256x256 (8 waves of 128x64), BK=32 in a 4-deep read-ahead
  // ring (C3 941 vs 988 us for the same tile with the reads behind each barrier
  // (6), C4 516 vs 531, C5 2206 vs 2235: profiles/r03/ab/wgrad_ra_*.json; round 2:
  // 6 at 1163 us vs 1296 for BK=64 in a 2-deep ring and 1400 register-staged)
  constexpr int WBK = std::is_same<T, float>::value ? 32 : 64;
  // (not on the aux stream: its 128 KB of LDS would keep the chain's step kernels off the CU)
  const int wpipe = rows % WBK == 0 ? env_int("AAA_WGRAD_PIPE", std::is_same<T, float>::value || aux ? 0 : 9) : 0;
  if (wpipe) {
    using I0 = std::integral_constant<int, 0>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    int rc;
    switch (wpipe) {
      case 2: rc = wgrad_lstm_pipe(GemmCfg<T, 256, 128, WBK, 2, 2>{}, I2{}, I0{}); break;
      case 3:   // 8 waves of 128x64 (fp32: spills, so 256x128)
        if constexpr (std::is_same<T, float>::value) rc = wgrad_lstm_pipe(GemmCfg<T, 256, 128, WBK, 2, 2>{}, I2{}, I0{});
        else rc = wgrad_lstm_pipe(GemmCfg<T, 256, 256, WBK, 2, 4>{}, I2{}, I0{});
        break;
      case 4: rc = wgrad_lstm_pipe(GemmCfg<T, 128, 256, WBK, 2, 2>{}, I2{}, I0{}); break;
      case 5: rc = wgrad_lstm_pipe(GemmCfg<T, 256, 128, WBK, 2, 2>{}, I3{}, I0{}); break;
      case 6:   // bf16: 8 waves, BK=32, 4-deep ring, spread DMA issue
      case 7:   // bf16: the same in a 3-deep ring
        if constexpr (std::is_same<T, float>::value)
          rc = wgrad_lstm_pipe(GemmCfg<T, 128, 128, WBK, 2, 2>{}, I3{}, I2{});
        else if (wpipe == 6)
          rc = wgrad_lstm_pipe(GemmCfg<T, 256, 256, 32, 2, 4>{}, std::integral_constant<int, 4>{}, I2{});
        else
          rc = wgrad_lstm_pipe(GemmCfg<T, 256, 256, 32, 2, 4>{}, I3{}, I2{});
        break;
      case 8:   // bf16: 4 waves of 128x128 (half the LDS fragment reads per MFMA of the 8-wave tile), 4-deep ring:
                // measured slower (C3 1367 vs 1079 us, C4 691 vs 561 us: one wave per SIMD hides less)
        if constexpr (std::is_same<T, float>::value)
          rc = wgrad_lstm_pipe(GemmCfg<T, 128, 128, WBK, 2, 2>{}, I3{}, I2{});
        else
          rc = wgrad_lstm_pipe(GemmCfg<T, 256, 256, 32, 2, 2>{}, std::integral_constant<int, 4>{}, I2{});
        break;
      case 9:   // bf16: read-ahead ring, 8 waves, BK=32, 4-deep
        if constexpr (std::is_same<T, float>::value)
          rc = wgrad_lstm_pipe(GemmCfg<T, 128, 128, WBK, 2, 2>{}, I3{}, I2{});
        else
          rc = wgrad_lstm_pipe(GemmCfg<T, 256, 256, 32, 2, 4>{}, std::integral_constant<int, 4>{},
                               std::integral_constant<int, kReadAhead>{});
        break;
      default: rc = wgrad_lstm_pipe(GemmCfg<T, 128, 128, WBK, 2, 2>{}, I2{}, I0{}); break;
    }
    if (rc) return rc;
  } else if (std::is_same<T, float>::value && f32_split6()) {
    // fp32: the register-staged 128x128 tile on the bf16 MFMA with three-way split operands (gemm.h SPLIT6)
    // AAA_WGRAD_S6_TILE (A/B): 0 = 128x128, 1 = 128x256, 2 = 256x128 (4 waves: fewer operand splits per
    // MFMA), 3 = 256x256 (8 waves of 128x64), the default: C2 842 / 936 / 832 / 729 us
    // (profiles/r04/ab/split6_tiles_c2_*.json)
    auto s6 = [&](auto cfg) {
      using CS6 = std::conditional_t<std::is_same<T, float>::value, decltype(cfg), CfgWFor<T>>;
      return wgrad_lstm(CS6{});
    };
    // 4 = 256x256 with each operand split once where it is committed to LDS (GemmCfgS6L, BK16,
    // two stages of bf16 part tiles); 5 = its 256x128 4-wave form; 6 (default) = 4 with two K
    // tiles of loads in flight: C2 633 vs 646 us (4) vs 776 (3) (profiles/r05/ab/wgrad_s6l/)
    // (tiles 0-5: ablation builds only)
#ifdef AAA_ABLATION
    const int tile6 = ab_int("AAA_WGRAD_S6_TILE", 6);
    const int rc = tile6 == 1   ? s6(GemmCfgS6<128, 256, 32, 2, 2>{})
                   : tile6 == 2 ? s6(GemmCfgS6<256, 128, 32, 2, 2>{})
                   : tile6 == 3 ? s6(GemmCfgS6<256, 256, 32, 2, 4>{})
                   : tile6 == 4 ? s6(GemmCfgS6L<256, 256, 16, 2, 4>{})
                   : tile6 == 5 ? s6(GemmCfgS6L<256, 128, 16, 2, 2>{})
                   : tile6 == 6 ? s6(GemmCfgS6L<256, 256, 16, 2, 4, 2>{})
                   : tile6 == 7 ? s6(GemmCfgS6L<256, 192, 16, 4, 2, 2>{})
                                : s6(GemmCfgS6<128, 128, 32, 2, 2>{});
#else
    const int rc = s6(GemmCfgS6L<256, 256, 16, 2, 4, 2>{});
#endif
    if (rc) return rc;
  } else {
    // on the aux stream a small-footprint tile lets the chain's step kernels co-reside on a CU
    const int wide = ab_int("AAA_AUX_WIDE", aux ? 0 : 1);
#ifdef AAA_ABLATION   // AAA_WGRAD_TILE=1: 128x192 tiles, 1728 = 9 x 192 columns without the half-empty last tile
    const int rc = !wide ? wgrad_lstm(CfgFor<T>{})
                   : ab_int("AAA_WGRAD_TILE", 0) == 1 ? wgrad_lstm(GemmCfg<T, 128, 192, 32, 2, 2>{})
                                                       : wgrad_lstm(CfgWFor<T>{});
#else
    const int rc = !wide ? wgrad_lstm(CfgFor<T>{}) : wgrad_lstm(CfgWFor<T>{});
#endif
    if (rc) return rc;
  }
  return AAA_OK;
}

// conv1 weight gradient over n frames whose bordered RGBx image (Xp) is
// rebuilt from the observation in chunks of L.xpc frames into xpbuf (the
// chunk buffer, or the frames' slice of a whole-batch region: L.xpc = F):
// the forward keeps no Xp (a chunk buffer, or a frame-resident encoder, which
// stores none in the learner), and a chunk is written and read back while it
// sits in the memory-side cache (256 MB) instead of all F frames' images
// round-tripping through HBM between the two passes.
template <typename T>
static int conv1_wgrad_frames(const Layout& L, const T* dy1, const void* frames, int n, T* xpbuf, float* gW,
                              hipStream_t s) {
  const size_t fb = (size_t)L.H * L.W * 3 * (L.fu8 ? 1 : 4);
  for (int s0 = 0; s0 < n; s0 += L.xpc) {
    const int m = std::min(L.xpc, n - s0);
    const char* fr = (const char*)frames + (size_t)s0 * fb;
    if (L.fu8) HIPCHK((frames_rgbx<T, uint8_t>(m, L.H, L.W, (const uint8_t*)fr, xpbuf, s)));
    else HIPCHK((frames_rgbx<T, float>(m, L.H, L.W, (const float*)fr, xpbuf, s)));
    const int rc = conv1_wgrad<T>(L, dy1 + (size_t)s0 * L.P1 * 32, xpbuf, m, gW, s);
    if (rc) return rc;
  }
  return AAA_OK;
}

// Vision encoder backward over F frames in descriptor-sized chunks: conv2
// weight grad (gW2 +=), conv2 dgrad -> dY1 with conv1's bias grad (gb1 +=),
// conv1 weight grad (gW1 +=); accumulators zeroed by the caller.  frames:
// xp is rebuilt from them L.xpc frames at a time (conv1_wgrad_frames);
// null: xp holds all F frames' images (the component entries).
template <typename T>
int vision_bwd(const Layout& L, const char* pk, const T* dy2, const T* y1, T* xp, T* dy1, int F,
                      float* gW2, float* gW1, float* gb1, hipStream_t s, const void* frames) {
  const size_t fb = (size_t)L.H * L.W * 3 * (L.fu8 ? 1 : 4);
  for (int f0 = 0; f0 < F; f0 += L.fchunk) {
    const int n = std::min(L.fchunk, F - f0);
    const T* d2 = dy2 + (size_t)f0 * L.P * 64;
    T* d1 = dy1 + (size_t)f0 * L.P1 * 32;
    int rc = conv2_wgrad<T>(L, d2, y1 + (size_t)f0 * L.P1 * 32, n, gW2, s);
    if (!rc) rc = conv2_dgrad<T>(L, pk, d2, d1, n, gb1, s);
    if (!rc && frames) rc = conv1_wgrad_frames<T>(L, d1, (const char*)frames + (size_t)f0 * fb, n, xp, gW1, s);
    else if (!rc) rc = conv1_wgrad<T>(L, d1, xp + (size_t)f0 * (L.H + 2) * (L.W + 2) * 4, n, gW1, s);
    if (rc) return rc;
  }
  return AAA_OK;
}

// The frame-resident vision backward (vision_bwd.h): bf16, uint8 observations (the environment's
// dtype: fp32 frames keep the layered launches), the frame-resident encoder's geometry, and F
// frames' dY1 buffer large enough for the workgroups' partials (AAA_VIS_BWD_FRAMES=0: the three
// layered launches above; AAA_VBWD_MINF: a frames-per-CU floor, 0 by default -- with the partial
// sums reduced 4 waves per 64 columns the fused kernel's fixed cost is ~30 us, below the layered
// launches' own: C3 (20 frames per CU) 281 vs 358 us, C4 (10) 155 vs 199 us).
// part_bytes: the room the caller lends the partials (0: the F frames' dY1 region, as the learner does).
// fp32 (vision_bwd_f32.h, k_vision_bwd_f32): the split-product path (f32_split6) on uint8 observations
// with the same switches; its partials (one per workgroup, vbwd_f32_groups: up to one per frame, which the
// dY1 region cannot hold) go to the frames' Xp region, which the fused path never reads (part_bytes 0: the
// F frames' images, or the chunk buffer's L.xpc); a region too small for the ideal grid runs fewer
// workgroups, and none at all (room for no partial) keeps the layered launches.  AAA_VBWD_MINF is 1 here (at
// least one frame per CU): below that the kernel's fixed cost loses to the layered launches (class time in a
// learner step, fused / layered: F = 32 78.6 / 53.8 us, F = 20 77.6 / 50.4 us; C2's 640 frames 126.9 / 172.8 us).
static size_t vbwd_f32_room(const Layout& L, int F, size_t part_bytes) {
  return part_bytes ? part_bytes : (size_t)(L.xpc < L.F ? L.xpc : F) * (L.H + 2) * (L.W + 2) * 4 * 4;
}
template <typename T>
static bool vbwd_on(const Layout& L, int F, size_t part_bytes = 0) {
  if constexpr (std::is_same<T, float>::value) {
    return f32_split6() && L.fu8 && vbwd_f32_fits(L.H, L.W, L.H1, L.W1, L.h, L.w) && vis_frames_on(L) &&
           env_int("AAA_VIS_BWD_FRAMES", 1) && F >= env_int("AAA_VBWD_MINF", 1) * device_cus() &&
           vbwd_f32_groups(F, device_cus(), vbwd_f32_room(L, F, part_bytes)) >= 1;
  } else if constexpr (!std::is_same<T, __bf16>::value) {
    (void)L; (void)F; (void)part_bytes;
    return false;
  } else {
    if (!part_bytes) part_bytes = (size_t)F * L.P1 * 32 * L.esz;
    return L.fu8 && vbwd_fits(L.H, L.W, L.H1, L.W1, L.h, L.w) && vis_frames_on(L) &&
           env_int("AAA_VIS_BWD_FRAMES", 1) && F >= env_int("AAA_VBWD_MINF", 0) * device_cus() &&
           (size_t)vbwd_groups(F, device_cus()) * kVbPart * 4 <= part_bytes;
  }
}
// F frames from ``f0``: conv2 wgrad (gW2 +=), conv2 dgrad + conv1 wgrad (gW1 +=, conv1 bias gb1 +=),
// the partials in the frames' dY1 region (unused on this path)
template <typename T>
static int vbwd_run(const Layout& L, const char* pk, const void* frames, int f0, int F, const T* dy2, const T* y1,
                    T* dy1, float* gW2, float* gW1, float* gb1, hipStream_t s, size_t part_bytes = 0,
                    int max_groups = 0, float* dy1_out = nullptr, const void* wdt2s = nullptr) {
  if constexpr (std::is_same<T, float>::value) {   // dy1: the partials' room (part_bytes of it)
    VisBwdF32Params vp{(const char*)frames + (size_t)f0 * L.H * L.W * 3, dy2, y1,
                       (const bf16x8*)(wdt2s ? wdt2s : pk + L.k_WdT2s),
                       dy1, dy1_out, F, L.H, L.W, L.H1, L.W1, L.h, L.w};
    HIPCHK(vision_bwd_frames_f32(vp, vbwd_f32_groups(F, device_cus(), part_bytes, max_groups), gW2, gW1, gb1, s));
    return AAA_OK;
  } else if constexpr (!std::is_same<T, __bf16>::value) {
    return fail(AAA_E_ARG, "the frame-resident vision backward is bf16 / fp32 only");
  } else {
    VisBwdParams vp{(const char*)frames + (size_t)f0 * L.H * L.W * 3 * (L.fu8 ? 1 : 4), dy2, y1,
                    (const __bf16*)(pk + L.k_WdT2), (float*)dy1, F, L.H, L.W, L.H1, L.W1, L.h, L.w};
    HIPCHK(vision_bwd_frames(vp, device_cus(), gW2, gW1, gb1, s));
    return AAA_OK;
  }
}

// The VISION phase on its own (backward_impl without CORE in the same call, and the encoder checker
// entry aaa_vision_enc_bwd): the frame-resident launch when vbwd_on says so (its partials in ``part``,
// part_bytes of room; 0 = dy1, the F frames' dY1 region), else the layered launches over all F frames
// (xp_frames: the observation the Xp chunk buffer is rebuilt from, null = xp holds every frame).
// Accumulators zeroed by the caller; *fused (may be null) <- which of the two ran.
// (fp32: the partials default to xp, the frames' Xp region; max_groups > 0 caps the workgroups and dy1_out
// receives the dY1 the fused kernel committed, wdt2s replaces the layout's pre-split dgrad weights -- all three
// for the checker entry aaa_vision_enc_f32_bwd)
const char* vision_bwd_variant(bool fused, bool f32, bool unpack) {
  static const char* const v[3][2] = {
      {"conv2 wgrad + dgrad, conv1 wgrad", "conv2 wgrad + dgrad, conv1 wgrad, grad unpack"},
      {"frame-resident conv2 wgrad + dgrad + conv1 wgrad [kernel: k_vision_bwd_frames]",
       "frame-resident conv2 wgrad + dgrad + conv1 wgrad [kernel: k_vision_bwd_frames], grad unpack"},
      {"frame-resident conv2 wgrad + dgrad + conv1 wgrad [kernel: k_vision_bwd_f32]",
       "frame-resident conv2 wgrad + dgrad + conv1 wgrad [kernel: k_vision_bwd_f32], grad unpack"}};
  return v[!fused ? 0 : f32 ? 2 : 1][unpack];
}
template <typename T>
int vision_bwd_alone(const Layout& L, const char* pk, const void* frames, const T* dy2, const T* y1, T* xp, T* dy1,
                     void* part, size_t part_bytes, int F, float* gW2, float* gW1, float* gb1, hipStream_t st,
                     const void* xp_frames, bool* fused, int max_groups, float* dy1_out, const void* wdt2s) {
  const bool on = vbwd_on<T>(L, F, part_bytes);
  if (fused) *fused = on;
  if (on) {   // the partials' room: the caller's, else the frames' Xp (fp32) / dY1 (bf16) region
    constexpr bool f32 = std::is_same<T, float>::value;
    return vbwd_run<T>(L, pk, frames, 0, F, dy2, y1, part ? (T*)part : f32 ? xp : dy1, gW2, gW1, gb1, st,
                       f32 ? vbwd_f32_room(L, F, part_bytes) : 0, max_groups, dy1_out, wdt2s);
  }
  const int rc = vision_bwd<T>(L, pk, dy2, y1, xp, dy1, F, gW2, gW1, gb1, st, xp_frames);
  if (rc) return rc;
  // fp32 with AAA_CONV2_DGRAD_RING=0: conv1's bias gradient by a column sum
  if (std::is_same<T, float>::value && !ab_int("AAA_CONV2_DGRAD_RING", 1))
    HIPCHK(colsum(dy1, 32, F * L.P1, 32, gb1, st));
  return AAA_OK;
}

// ------------------------------------------------------------ backward ----
// (what the phases of one backward call share: rt.h CallCtx)

// The tail's backward GEMMs.  dgrad: D[Mi][Nj] = Wt^T[Mi][K] x dY[Nj][K]^T through ``ep`` (Wt: the
// weight as stored, K rows of Mi).  wgrad: out[Mi][Nj] += dA^T x X over the F frames (Mi, Nj: the
// operands' columns), split-K atomics into a zeroed ``out``.
template <class EP>
static hipError_t tail_dgrad(const Rows& Wt, const Rows& dY, const EP& ep, int Mi, int Nj, int K, hipStream_t st) {
  return head_gemm<LdRowsT, LdRows>(Wt, dY, ep, Mi, Nj, K, 1, st);
}
static hipError_t tail_wgrad(const Rows& dA, const Rows& X, float* out, int ldo, int F, hipStream_t st) {
  const int Mi = dA.nrows, Nj = X.nrows;
  return head_gemm<LdRowsT, LdRowsT>(dA, X, EpiStore<true>{out, ldo, Mi, Nj}, Mi, Nj, F,
                                     wgrad_splits(cdiv(Mi, 64) * cdiv(Nj, 64), F, CF::BK), st);
}
// The tail's packed gradients into the reference's tensors (stateful: W_hh's too)
static hipError_t tail_unpack(const CallCtx& c, bool stateful) {
  const Layout& L = c.L;
  float* grads = c.grads;
  F32Unpack up;
  up.gW1p = c.Wf(L.gW1p); up.gWihp = c.Wf(L.gWihp); up.gblc = c.Wf(L.gblc); up.gWhd = c.Wf(L.gWhd); up.gbhd = c.Wf(L.gbhd);
  up.a0w = grads + L.poff[A0W]; up.wih = grads + L.poff[WIH]; up.bih = grads + L.poff[BIH];
  up.bhh = grads + L.poff[BHH]; up.pw = grads + L.poff[PW]; up.vw = grads + L.poff[VW];
  up.pb = grads + L.poff[PB]; up.vb = grads + L.poff[VB];
  up.ans_in = L.ans_in; up.ans_ld = L.ans_ld; up.A = L.A;
  if (stateful) {
    up.gWihhp = c.Wf(L.gWihhp);
    up.whh = grads + L.poff[WHH];
  }
  return unpack_f32(up, c.st);
}

// Stateful policy core, backward of the tail (phase HEAD): the dgrad chain runs
// step by step from t = T-1 (the carries dh, dc of the core state flow through
// the LSTMCell's W_hh and the query MLP into step t-1); every weight gradient
// is then one batched GEMM over all frames from the saved per-step operands.
static int head_backward_stateful(const CallCtx& c) {
  const Layout& L = c.L;
  const aaa_io* io = c.io;
  const hipStream_t st = c.st;
  const float *prm = c.prm, *reset = c.reset;
  float* grads = c.grads;
  const int F = L.F, P = L.P, B = L.B, qd = L.qd, da = L.da;
  float *CH = c.Wf(L.CH), *CC = c.Wf(L.CC), *AOX = c.Wf(L.AOX), *dAOX = c.Wf(L.dAOX), *dhc = c.Wf(L.dhc),
        *dcc = c.Wf(L.dcc);
  const size_t sB = (size_t)B * 256 * 4;
  if (io->dcore_hT) HIPCHK(hipMemcpyAsync(dhc, io->dcore_hT, sB, hipMemcpyDeviceToDevice, st));
  else HIPCHK(hipMemsetAsync(dhc, 0, sB, st));
  if (io->dcore_cT) HIPCHK(hipMemcpyAsync(dcc, io->dcore_cT, sB, hipMemcpyDeviceToDevice, st));
  else HIPCHK(hipMemsetAsync(dcc, 0, sB, st));
  for (int t = L.T - 1; t >= 0; --t) {
    const size_t f0 = (size_t)t * B;
    float *dLG = c.Wf(L.dLG) + f0 * 1024, *dH1 = c.Wf(L.dH1) + f0 * 512, *dAns = c.Wf(L.dAns) + f0 * da;
    float *dQf = c.Wf(L.dQf) + f0 * qd, *dq2 = c.Wf(L.dq2s) + f0 * qd, *dq1 = c.Wf(L.dq1s) + f0 * 128;
    // heads dgrad + dh carry -> LSTMCell backward from (c_{t-1}, c_t), dc carry
    HIPCHK(tail_dgrad({(const float*)(c.pk + L.k_Whd), 256, 256}, {c.Wf(L.dY) + f0 * L.ldy, L.ldy, B},
                      EpiLstmCellBwdS{c.Wf(L.LG) + f0 * 1024, CC + f0 * 256, CC + (f0 + B) * 256, dhc, dcc, dLG, B}, 256,
                      B, L.ldy, st));
    // rows that entered step t from reset(): c_{t-1} was 0 (d f-gate stored as 0) and no dc flows to step t-1
    if (reset)
      HIPCHK(reset_rows(reset + f0, B, 1, ResetZeros{}.add(dLG + 1, 1024, 256, 4).add(dcc, 256, 256), nullptr, nullptr,
                        0, st));
    // [d answer | d h_{t-1} (recurrent part)] = [W_ih | W_hh]^T dgates
    HIPCHK(tail_dgrad({(const float*)(c.pk + L.k_Wihhp), 512, 512}, {dLG, 1024, B},
                      EpiStoreT<float>{dAOX + f0 * 512, 512, 512, B, nullptr, 0}, 512, B, 1024, st));
    // answer_processor.2 dgrad fused with the ReLU backward
    HIPCHK(tail_dgrad({prm + L.poff[A2W], 512, 512}, {dAOX + f0 * 512, 512, B},
                      EpiReluBwdT{dH1, c.Wf(L.hid1) + f0 * 512, 512, 512, 512, B}, 512, B, 256, st));
    // answer_processor.0 dgrad: readout and query columns of the answer row
    HIPCHK(tail_dgrad({(const float*)(c.pk + L.k_W1p), L.ans_ld, da}, {dH1, 512, B},
                      EpiStoreT<float>{dAns, da, da, B, nullptr, 0}, da, B, 512, st));
    // readout / softmax / logits backward with this step's queries; dQ gets
    // the logits path plus the answer row's copy of Q
    {
      TimerScope tim(AAA_TIMER_ATTN_BWD, st, (double)B * attn_bwd_bytes(P, L.nq, L.esz), "k_attn_bwd, per-frame query (stateful core)");
      HIPCHK(attn_bwd(readout_h(L, c.ws, c.reset != nullptr).frame(f0, P), io->basis, c.Wf(L.Qf) + f0 * qd, c.Wf(L.Am) + f0 * P * L.nq, dAns,
                      da, B, P, L.nq, c.Wf(L.dO) + f0 * P * 128, dQf, st, qd, 1, (c.plan.cqm & kCqmDO) != 0));
    }
    // query MLP backward to its input h_{t-1}
    HIPCHK(tail_dgrad({prm + L.poff[Q4W], qd, qd}, {dQf, qd, B},
                      EpiReluBwdT{dq2, c.Wf(L.q2s) + f0 * qd, qd, qd, qd, B}, qd, B, qd, st));
    HIPCHK(tail_dgrad({prm + L.poff[Q2W], 128, 128}, {dq2, qd, B},
                      EpiReluBwdT{dq1, c.Wf(L.q1s) + f0 * 128, 128, 128, 128, B}, 128, B, qd, st));
    // dh_{t-1} = W0^T dq1 (query path) + W_hh^T dgates (recurrent path)
    HIPCHK(tail_dgrad({prm + L.poff[Q0W], 256, 256}, {dq1, 128, B},
                      EpiStoreAddT{dhc, dAOX + f0 * 512 + 256, 256, 512, 256, B}, 256, B, 128, st));
    if (reset)   // ... and no dh: h_{t-1} was 0 for both of its readers
      HIPCHK(reset_rows(reset + f0, B, 1, ResetZeros{}.add(dhc, 256, 256), nullptr, nullptr, 0, st));
  }
  if (io->dcore_h0) HIPCHK(hipMemcpyAsync(io->dcore_h0, dhc, sB, hipMemcpyDeviceToDevice, st));
  if (io->dcore_c0) HIPCHK(hipMemcpyAsync(io->dcore_c0, dcc, sB, hipMemcpyDeviceToDevice, st));
  // weight gradients, batched over all T*B frames
  HIPCHK(tail_wgrad({c.Wf(L.dY), L.ldy, L.ldy}, {CH + (size_t)B * 256, 256, 256}, c.Wf(L.gWhd), 256, F, st));
  HIPCHK(colsum(c.Wf(L.dY), L.ldy, F, L.ldy, c.Wf(L.gbhd), st));
  HIPCHK(tail_wgrad({c.Wf(L.dLG), 1024, 1024}, {AOX, 512, 512}, c.Wf(L.gWihhp), 512, F, st));
  HIPCHK(colsum(c.Wf(L.dLG), 1024, F, 1024, c.Wf(L.gblc), st));
  HIPCHK(tail_wgrad({dAOX, 512, 256}, {c.Wf(L.hid1), 512, 512}, grads + L.poff[A2W], 512, F, st));
  HIPCHK(colsum(dAOX, 512, F, 256, grads + L.poff[A2B], st));
  HIPCHK(tail_wgrad({c.Wf(L.dH1), 512, 512}, {c.Wf(L.ans), L.ans_ld, L.ans_ld}, c.Wf(L.gW1p), L.ans_ld, F, st));
  HIPCHK(colsum(c.Wf(L.dH1), 512, F, 512, grads + L.poff[A0B], st));
  HIPCHK(tail_wgrad({c.Wf(L.dQf), qd, qd}, {c.Wf(L.q2s), qd, qd}, grads + L.poff[Q4W], qd, F, st));
  HIPCHK(colsum(c.Wf(L.dQf), qd, F, qd, grads + L.poff[Q4B], st));
  HIPCHK(tail_wgrad({c.Wf(L.dq2s), qd, qd}, {c.Wf(L.q1s), 128, 128}, grads + L.poff[Q2W], 128, F, st));
  HIPCHK(colsum(c.Wf(L.dq2s), qd, F, qd, grads + L.poff[Q2B], st));
  // the query MLP's input: CH slots 0..T-1, or with a mask the h half of the [answer | h] rows it read (zeros
  // in the rows of an episode start: forward_tail_stateful)
  HIPCHK(tail_wgrad({c.Wf(L.dq1s), 128, 128}, reset ? Rows{AOX + 256, 512, 256} : Rows{CH, 256, 256},
                    grads + L.poff[Q0W], 256, F, st));
  HIPCHK(colsum(c.Wf(L.dq1s), 128, F, 128, grads + L.poff[Q0B], st));
  HIPCHK(tail_unpack(c, true));
  return AAA_OK;
}

// Zero-state policy core, backward of the tail (phase HEAD), batched over all T*B frames.
// The dgrad chain (heads -> LSTMCell -> answer MLP -> readout) on st; each layer's weight gradient
// on the side stream once the chain has produced its input gradient (few-tile GEMMs: the two
// streams fill CUs the other leaves idle); joined before the gradients are unpacked.
// Below ~2048 frames the GEMMs are too short for the overlap to pay for the second queue's dispatch
// cost on the rest of the step (C2, 640 frames: tail bwd -20 us but the step +10-15 us;
// profiles/r06/ab/side/): one stream there.
static int head_backward_zero_state(const CallCtx& c) {
  const Layout& L = c.L;
  const hipStream_t st = c.st;
  const float* prm = c.prm;
  float* grads = c.grads;
  const int F = L.F, P = L.P;
  std::unique_ptr<TimerScope> tail(new TimerScope(AAA_TIMER_TAIL_BWD, st, 2.0 * F * (tail_fwd_flop(L) + 2.0 * 256 * L.ldy),
                                                  "heads + LSTMCell + answer MLP backward (fp32 GEMMs)"));
  hipStream_t ss = F >= 2048 ? side_stream() : nullptr;
  hipStream_t ws_ = ss ? ss : st;   // the weight gradients' stream
  if (ss) HIPCHK(stream_order(st, ss));   // the zeroed accumulators, the cotangent concat
  // heads wgrad (dY from the prologue)
  HIPCHK(tail_wgrad({c.Wf(L.dY), L.ldy, L.ldy}, {c.Wf(L.LH), 256, 256}, c.Wf(L.gWhd), 256, F, ws_));
  // heads dgrad fused with the zero-state LSTMCell backward
  HIPCHK(tail_dgrad({(const float*)(c.pk + L.k_Whd), 256, 256}, {c.Wf(L.dY), L.ldy, F},
                    EpiLstmCellBwd{c.Wf(L.LG), c.Wf(L.LC), c.Wf(L.dLG), F}, 256, F, L.ldy, st));
  if (ss) HIPCHK(stream_order(st, ss));   // dLG
  // LSTMCell weight_ih grad (weight_hh grad is exactly zero: h0 = 0, Q1)
  HIPCHK(tail_wgrad({c.Wf(L.dLG), 1024, 1024}, {c.Wf(L.AO), 256, 256}, c.Wf(L.gWihp), 256, F, ws_));
  // LSTMCell input dgrad
  HIPCHK(tail_dgrad({(const float*)(c.pk + L.k_Wihp), 256, 256}, {c.Wf(L.dLG), 1024, F},
                    EpiStoreT<float>{c.Wf(L.dAO), 256, 256, F, nullptr, 0}, 256, F, 1024, st));
  if (ss) HIPCHK(stream_order(st, ss));   // dAO
  // answer_processor.2 wgrad / bias
  HIPCHK(tail_wgrad({c.Wf(L.dAO), 256, 256}, {c.Wf(L.hid1), 512, 512}, grads + L.poff[A2W], 512, F, ws_));
  // answer_processor.2 dgrad fused with ReLU backward
  HIPCHK(tail_dgrad({prm + L.poff[A2W], 512, 512}, {c.Wf(L.dAO), 256, F},
                    EpiReluBwdT{c.Wf(L.dH1), c.Wf(L.hid1), 512, 512, 512, F}, 512, F, 256, st));
  if (ss) HIPCHK(stream_order(st, ss));   // dH1
  // answer_processor.0 wgrad / bias
  HIPCHK(tail_wgrad({c.Wf(L.dH1), 512, 512}, {c.Wf(L.ans), L.ans_ld, L.ans_ld}, c.Wf(L.gW1p), L.ans_ld, F, ws_));
  // answer_processor.0 dgrad (readout columns only)
  HIPCHK(tail_dgrad({(const float*)(c.pk + L.k_W1p), L.ans_ld, L.da}, {c.Wf(L.dH1), 512, F},
                    EpiStoreT<float>{c.Wf(L.dAns), L.da, L.da, F, nullptr, 0}, L.da, F, 512, st));
  tail.reset();
  // attention readout / softmax / logits backward, then the query MLP
  {
    TimerScope tim(AAA_TIMER_ATTN_BWD, st, (double)F * attn_bwd_bytes(P, L.nq, L.esz), "k_attn_bwd, 1 WG per frame");
    HIPCHK(attn_bwd(readout_h(L, c.ws, c.reset != nullptr), c.io->basis, (const float*)(c.pk + L.k_Q), c.Wf(L.Am), c.Wf(L.dAns), L.da, F, P,
                    L.nq, c.Wf(L.dO), c.Wf(L.dQp), st, 0, 0, (c.plan.cqm & kCqmDO) != 0));
  }
  tail.reset(new TimerScope(AAA_TIMER_TAIL_BWD, st, 0.0, "bias column sums, query MLP backward, grad unpack"));
  {  // the bias grads of the heads, the LSTMCell and both answer layers, and dQ summed over frames: one launch
    ColSums cs;
    cs.add(c.Wf(L.dY), L.ldy, L.ldy, c.Wf(L.gbhd));
    cs.add(c.Wf(L.dLG), 1024, 1024, c.Wf(L.gblc));
    cs.add(c.Wf(L.dAO), 256, 256, grads + L.poff[A2B]);
    cs.add(c.Wf(L.dH1), 512, 512, grads + L.poff[A0B]);
    cs.add(c.Wf(L.dQp), L.qd, L.qd, c.Wf(L.dQs));
    HIPCHK(colsum_multi(cs, F, st));
  }
  HIPCHK(query_bwd(c.Wf(L.dQs), grads + L.poff[A0B], prm + L.poff[A0W], L.ans_in, L.nq, prm + L.poff[Q2W],
                   prm + L.poff[Q4W], (const float*)(c.pk + L.k_q1), (const float*)(c.pk + L.k_q2), grads + L.poff[Q4W],
                   grads + L.poff[Q4B], grads + L.poff[Q2W], grads + L.poff[Q2B], grads + L.poff[Q0B], st));
  if (ss) HIPCHK(stream_order(ss, st));   // join: the weight gradients
  HIPCHK(tail_unpack(c, false));
  return AAA_OK;
}

// Phase HEAD: zero the gradients and accumulators, concatenate the cotangents, then the tail's backward.
template <typename T>
static int head_backward(const CallCtx& c) {
  const Layout& L = c.L;
  {
    TimerScope tim(AAA_TIMER_MISC, c.st, 0.0, "grad/accumulator memsets, cotangent concat");
    ZeroRanges z{};   // the grads, the atomic accumulators and the cotangent concat: one launch
    z.add(c.grads, (long)L.ptotal);
    z.add(c.Wf(L.dQs), (long)((L.HR - L.dQs) / 4));   // (up to HR, the last region: not an accumulator)
    HIPCHK(prologue<T>(z, 0, nullptr, (T*)nullptr, L.F, L.A, L.ldy, c.io->dlogits, c.io->dvalues, c.Wf(L.dY), c.st));
  }
  return L.sc ? head_backward_stateful(c) : head_backward_zero_state(c);
}

// conv2 / conv1 backward of the frames of steps [lo, hi) on ``vs`` (needs their dY2 only): one frame-resident
// launch (+ its partials' sum), or conv2 wgrad, conv2 dgrad (4 parity classes) -> dY1, conv1 wgrad / bias: the
// dispatch of the VISION phase on its own (vision_bwd_alone), on this chunk's frames (a chunk is at most
// L.fchunk frames: one pass of its loop)
template <typename T>
static int chunk_vision(const CallCtx& c, int lo, int hi, hipStream_t vs) {
  const Layout& L = c.L;
  const int F1 = (hi - lo) * L.B;
  const size_t f0 = (size_t)lo * L.B;
  const bool on = vbwd_on<T>(L, F1);
  TimerScope tim(AAA_TIMER_VISION_BWD, vs, (double)F1 * vision_bwd_flop(L),
                 vision_bwd_variant(on, std::is_same<T, float>::value, false));
  const void* fr = (const char*)c.io->frames + f0 * L.H * L.W * 3 * (L.fu8 ? 1 : 4);
  const bool chunked = L.xpc < L.F;   // Xp chunk buffer: rebuilt from the observation
  // and so is these frames' own slice of a whole-batch Xp region wherever the forward may have stored none
  const bool rebuild = chunked || vis_frames_layout(L);
  return vision_bwd_alone<T>(L, c.pk, fr, c.Wt<T>(L.dY2) + f0 * L.P * 64, c.Wt<T>(L.Y1) + f0 * L.P1 * 32,
                             chunked ? c.Wt<T>(L.Xp) : c.Wt<T>(L.Xp) + f0 * (L.H + 2) * (L.W + 2) * 4,
                             c.Wt<T>(L.dY1) + f0 * L.P1 * 32, nullptr, 0, F1, c.Wf(L.gWp2), c.Wf(L.gWp1),
                             c.grads + L.poff[C0B], vs, rebuild ? fr : nullptr, nullptr);
}

// dx_t (conv2's output gradient dY2) of steps [lo, hi) in one launch on ``s``:
// D[64][rows] = WdT[0:64] * gather(dZ), conv2's bias gradient summed in the epilogue
template <typename T>
static int batched_dx(const CallCtx& c, int lo, int hi, hipStream_t s) {
  const Layout& L = c.L;
  const int M = L.B * L.P, rows = (hi - lo) * M;
  const T* dz = c.Wt<T>(L.dZ) + (size_t)lo * M * 512;
  float* gb2 = c.grads + L.poff[C1B];
  TimerScope tim(AAA_TIMER_CORE_DX, s, 2.0 * rows * 64 * 4608, "batched dx (conv2-output grad), K=4608 [kernel: EpiStoreBiasT]");
  const ConvGeo g = ConvGeo{512, 512, 0, L.h, L.w, L.h, L.w, 3, 1, 1, 1}.prep();
  const T* WdT = (const T*)(c.pk + L.k_WdTl);
  const uint32_t zb = (uint32_t)((size_t)rows * 512 * L.esz);
  if constexpr (std::is_same<T, float>::value) {
    // 64x64 tiles (64x128 measured slower: occupancy); conv2's bias
    // gradient summed from the tile in the epilogue (no column-sum pass)
    EpiStoreBiasT<float> ep{c.Wf(L.dY2) + (size_t)lo * M * 64, 64, 64, rows, gb2};
    using ED = EpiStoreBiasT<float>;
    const int dx6 = f32_split6() ? ab_int("AAA_DX_S6_TILE", 4) : -1;
    if (dx6 == 4) {   // the ring tile on the bf16 MFMA with three-way split operands (gemm.h SPLIT6):
      // 64x128 with the weights pre-split (k_WdT6 planes), only dZ split in the loop
      // (C2 340 vs 357 us for the in-loop split of both, profiles/r04/ab/README.md)
      using C6 = GemmCfgS6<64, 128, 32, 2, 2>;
      using LA3 = GRows3B<64, 32, C6::NT>;
      using LBx = GIm2colB<float, 128, 32, C6::NT>;
      HIPCHK((launch_pipe<C6, LA3, LBx, ED, 2>(
          typename LA3::Params{(const __bf16*)(c.pk + L.k_WdT6), 4608, 64, (size_t)64 * 4608},
          typename LBx::Params{dz, g, rows, zb}, ep, 64, rows, 4608, 1, s)));
    } else if (dx6 < 0) {   // exact fp32 MFMA (AAA_F32_SPLIT6=0)
      if (pipe_batched())
        HIPCHK((step_gemm<CfgFor<T>, true, T, T, ED>(WdT, 4608, 64, dz, g, rows, zb, ep, 64, 4608, s)));
      else
        HIPCHK((step_gemm<CfgFor<T>, false, T, T, ED>(WdT, 4608, 64, dz, g, rows, zb, ep, 64, 4608, s)));
    } else {
#ifdef AAA_ABLATION
      // the measured-slower variants (ablation builds): 0 = 64x64, 1 = 64x128 in-loop split
      // (C2 355 / 344 us), 2 = 64x64 BK64, 3 = 64x128 channel-chunk-major K order (ConvGeo::cmaj;
      // 365 vs 353 us), 5 = tile 4 with dZ pre-split too (GIm2colB3 over split_planes: 467-473 vs
      // 337 us), 6 = the halo-staged conv on split operands (C2 478 vs 370 us,
      // profiles/r04/ab/halo_dx_f32_c2_*.json)
      using HF6 = HaloCfgS6<64, 128, 32, 1, 2, 1, 176>;   // one 11x11 frame per tile, its dZ image in LDS
      switch (dx6) {
        case 6: {
          if (!halo_fits<HF6>(L.h, L.w, 512)) return fail(AAA_E_ARG, "AAA_DX_S6_TILE=6: grid too large");
          const HaloParams hp{WdT, 4608, 64, dz, 512, 0, 512, zb, L.h, L.w, (hi - lo) * L.B, 1};
          HIPCHK((launch_halo<HF6>(hp, ep, s)));
          break;
        }
        case 3: {
          HIPCHK(reorder_cmaj(WdT, 64, 512, 9, 32, (float*)(c.pk + L.k_WdTc), s));   // its weights, re-laid here
          ConvGeo gc = g;
          gc.cmaj = 32;
          HIPCHK((step_gemm<GemmCfgS6<64, 128, 32, 2, 2>, true, T, T, ED>((const T*)(c.pk + L.k_WdTc), 4608, 64, dz, gc,
                                                                         rows, zb, ep, 64, 4608, s)));
          break;
        }
        case 1:
          HIPCHK((step_gemm<GemmCfgS6<64, 128, 32, 2, 2>, true, T, T, ED>(WdT, 4608, 64, dz, g, rows, zb, ep, 64, 4608, s)));
          break;
        case 5: {
          if (!L.dZ6) return fail(AAA_E_ARG, "AAA_DX_S6_TILE=5 set after the workspace was laid out");
          using C6 = GemmCfgS6<64, 128, 32, 2, 2>;
          using LA3 = GRows3B<64, 32, C6::NT>;
          using LB3 = GIm2colB3<128, 32, C6::NT>;
          __bf16* z6 = (__bf16*)c.Wf(L.dZ6);
          HIPCHK(split_planes(dz, (long)rows * 512, z6, s));
          HIPCHK((launch_pipe<C6, LA3, LB3, ED, 2>(
              typename LA3::Params{(const __bf16*)(c.pk + L.k_WdT6), 4608, 64, (size_t)64 * 4608},
              typename LB3::Params{z6, g, rows, zb / 2, (size_t)rows * 512}, ep, 64, rows, 4608, 1, s)));
          break;
        }
        case 2:
          HIPCHK((step_gemm<GemmCfgS6<64, 64, 64, 2, 2>, true, T, T, ED>(WdT, 4608, 64, dz, g, rows, zb, ep, 64, 4608, s)));
          break;
        default:
          HIPCHK((step_gemm<GemmCfgS6<64, 64, 32, 2, 2>, true, T, T, ED>(WdT, 4608, 64, dz, g, rows, zb, ep, 64, 4608, s)));
      }
#else
      return fail(AAA_E_ARG, "AAA_DX_S6_TILE %d: ablation builds only", dx6);
#endif
    }
  } else {
    // bf16: dY2 stored bf16 (its readers round it to bf16 anyway), conv2's
    // bias gradient summed from the fp32 values in the epilogue
    EpiStoreBiasT<T> ep{c.Wt<T>(L.dY2) + (size_t)lo * M * 64, 64, 64, rows, gb2};
    // small grids: halo-staged conv, one frame per 64x128 tile
    // (tools/ubench/halo_tiles: 658 vs 771 us for the ring at C3)
    using HD = HaloCfg<__bf16, 64, 128, 64, 1, 2, 1, 176>;
    // 21x21 grids (168x168 frames): one frame per 512-column tile of 4 waves, 32-channel chunks
    using HW = HaloCfg<__bf16, 64, 512, 32, 1, 4, 1, 576>;
    const HaloParams hp{WdT, 4608, 64, dz, 512, 0, 512, zb, L.h, L.w, (hi - lo) * L.B, 1};
    if (halo_fits<HD>(L.h, L.w, 512) && ab_int("AAA_HALO_DX", 1)) {
      HIPCHK((launch_halo<HD>(hp, ep, s)));
    } else if (halo_fits<HW>(L.h, L.w, 512) && ab_int("AAA_HALO_DX", 1)) {
      HIPCHK((launch_halo<HW>(hp, ep, s)));
    } else {
      // larger grids (21x21 at 168x168): 64x128 on a 3-stage ring (bf16_tiles at C3: 643 vs 716 us for 64x64)
      HIPCHK((step_gemm<GemmCfg<T, 64, 128, 64, 2, 2>, true, T, T, EpiStoreBiasT<T>, 3>(WdT, 4608, 64, dz, g, rows, zb,
                                                                                        ep, 64, 4608, s)));
    }
  }
  return AAA_OK;
}

// Off-chain backward work for the steps [lo, hi) on ``s``: weight/bias grads of the ConvLSTM, dx (conv2
// output grad) unless the BPTT launch computed it (dx_fused) and -- when VISION runs in the same call
// (vision_here) -- the conv2/conv1 backward of those frames.  Every gradient accumulates atomically
// into zeroed buffers, so chunks may run in any order.
template <typename T>
static int core_chunk(const CallCtx& c, int lo, int hi, hipStream_t s, bool dx_fused, bool vision_here) {
  const Layout& L = c.L;
  const int M = L.B * L.P, rows = (hi - lo) * M;
  // (the layered vision backward on the side stream beside the ConvLSTM weight gradient, ablation
  // builds with AAA_VIS_SIDE=1: C2 232.0k -> 228.6-229.2k, C5 within noise -- the two contend for
  // the CUs; profiles/r06/ab/side/)
  hipStream_t vside = vision_here && dx_fused && !vbwd_on<T>(L, (hi - lo) * L.B) && ab_int("AAA_VIS_SIDE", 0)
                          ? side_stream()
                          : nullptr;
  if (vside) {
    HIPCHK(stream_order(s, vside));
    if (const int rc = chunk_vision<T>(c, lo, hi, vside)) return rc;
  }
  if (const int rc = lstm_wgrad<T>(c.Wt<T>(L.dZ) + (size_t)lo * M * 512, c.Wt<T>(L.XH) + (size_t)lo * M * 192, rows, L.h,
                                   L.w, c.Wf(L.gWpl), s, s != c.st))
    return rc;
  if (!dx_fused)
    if (const int rc = batched_dx<T>(c, lo, hi, s)) return rc;
  if (!vision_here) return AAA_OK;
  if (vside) return stream_order(vside, s) == hipSuccess ? AAA_OK : fail(AAA_E_LAUNCH, "side-stream join");
  return chunk_vision<T>(c, lo, hi, s);
}

// The per-step BPTT chain's tile, from its entry (step_tiles.h).  bj: the pixels per gate-backward workgroup and
// gate-bias partial row -- the GEMM's pixel tile (split-K chain: kSplitBj, finer, so that kernel spreads over the
// chip).  pipe: ring (glds.h) kernels reduce the gate-bias partials in their epilogue; the register-staged ones
// leave the bias to a column sum over dZ.  dh0: the entry that runs t = 0 (dh0).
struct BpttChain {
  int tile, bj;
  bool pipe;
  SplitK split;
  int dh0;
  bool g16;      // fp16 gate storage
  float* part;   // gate-bias partials [T][cdiv(M, bj)][512], or null: the bias is dZ's column sum
};

// Episode starts (reset != null), fp32: the step kernels run as they are, then resets.hip's
// k_reset_gate_bwd rewrites the rows of step t-1's gate backward that an episode start at t or
// t-1 changes.  Called after the gate backward of step t-1 (t = T: the last step's).
// bf16 runs the whole gate backward of a masked call in resets.hip instead (bptt_gates_resets).
template <typename T>
static int bptt_fix(const CallCtx& c, int t) {
  if (!c.reset) return AAA_OK;
  if constexpr (std::is_same<T, float>::value) {
    const Layout& L = c.L;
    const int M = L.B * L.P;
    HIPCHK((reset_gate_bwd(t < L.T ? c.reset + (size_t)t * L.B : nullptr, c.reset + (size_t)(t - 1) * L.B, M,
                                         L.P, c.Wf(L.dO) + (size_t)(t - 1) * M * 128,
                                         c.Wf(L.Gt) + (size_t)(t - 1) * M * 512, c.Wf(L.Cst) + (size_t)(t - 1) * M * 128,
                                         c.Wf(L.Cst) + (size_t)t * M * 128, c.Wf(L.dC),
                                         c.Wf(L.dZ) + (size_t)(t - 1) * M * 512, c.st)));
  }
  return AAA_OK;
}

// bf16 under a mask: the gate backward of step t-1 (t = T: the last step's) with the mask applied, from the raw
// dgrad ``dh`` of dZ_t (t = T: io->dhT or null), its fp32 gate-bias partials into ch.part (resets.hip
// k_gate_bwd_resets).  The rounded dZ never feeds the bias gradient, as without a mask.
static int bptt_gates_resets(const CallCtx& c, const BpttChain& ch, int t, const float* dh) {
  const Layout& L = c.L;
  const int M = L.B * L.P;
  const float* rs_in = t < L.T ? c.reset + (size_t)t * L.B : nullptr;
  const float* rs_c = c.reset + (size_t)(t - 1) * L.B;
  const float* dO = c.Wf(L.dO) + (size_t)(t - 1) * M * 128;
  const float* cprev = c.Wf(L.Cst) + (size_t)(t - 1) * M * 128;
  const float* ccur = c.Wf(L.Cst) + (size_t)t * M * 128;
  __bf16* dz = c.Wt<__bf16>(L.dZ) + (size_t)(t - 1) * M * 512;
  float* part = ch.part ? ch.part + (size_t)(t - 1) * cdiv(M, ch.bj) * 512 : nullptr;
  if (ch.g16)
    HIPCHK((gate_bwd_resets<__bf16, _Float16>(M, ch.bj, L.P, rs_in, rs_c, dO, dh,
                                              (const _Float16*)(c.ws + L.Gt) + (size_t)(t - 1) * M * 512, cprev, ccur,
                                              c.Wf(L.dC), dz, part, c.st)));
  else
    HIPCHK((gate_bwd_resets<__bf16, float>(M, ch.bj, L.P, rs_in, rs_c, dO, dh, c.Wf(L.Gt) + (size_t)(t - 1) * M * 512,
                                           cprev, ccur, c.Wf(L.dC), dz, part, c.st)));
  return AAA_OK;
}

// The gate backward of the last step (dh_T from io->dhT), which starts the per-step and frame-group chains
template <typename T>
static int bptt_last_gates(const CallCtx& c, const BpttChain& ch) {
  const Layout& L = c.L;
  const int M = L.B * L.P, t1 = L.T - 1;
  if constexpr (std::is_same<T, __bf16>::value)
    if (c.reset) return bptt_gates_resets(c, ch, L.T, c.io->dhT);
  float* part = ch.part ? ch.part + (size_t)t1 * cdiv(M, ch.bj) * 512 : nullptr;
  if (ch.g16)
    HIPCHK((gate_bwd_last<T, _Float16>(M, ch.bj, c.Wf(L.dO) + (size_t)t1 * M * 128, c.io->dhT,
                                       (const _Float16*)(c.ws + L.Gt) + (size_t)t1 * M * 512,
                                       c.Wf(L.Cst) + (size_t)t1 * M * 128, c.Wf(L.Cst) + (size_t)(t1 + 1) * M * 128,
                                       c.Wf(L.dC), c.Wt<T>(L.dZ) + (size_t)t1 * M * 512, part, c.st)));
  else
    HIPCHK((gate_bwd_last<T, float>(M, ch.bj, c.Wf(L.dO) + (size_t)t1 * M * 128, c.io->dhT,
                                    c.Wf(L.Gt) + (size_t)t1 * M * 512, c.Wf(L.Cst) + (size_t)t1 * M * 128,
                                    c.Wf(L.Cst) + (size_t)(t1 + 1) * M * 128, c.Wf(L.dC),
                                    c.Wt<T>(L.dZ) + (size_t)t1 * M * 512, part, c.st)));
  return bptt_fix<T>(c, L.T);
}

// bf16: the whole chain in one frame-resident launch (fb workgroups per frame), dx (dY2) and conv2's bias
// gradient included
static int bptt_frames_bf16(const CallCtx& c, int fb) {
  const Layout& L = c.L;
  const aaa_io* io = c.io;
  const int M = L.B * L.P;
  RecBwdParams rp{(const __bf16*)(c.pk + L.k_Wbf), c.Wf(L.dO), (const _Float16*)(c.ws + L.Gt), c.Wf(L.Cst), io->dhT,
                  c.Wf(L.dC), c.Wt<__bf16>(L.dZ), c.Wf(L.dZp), io->dh0, c.Wt<__bf16>(L.dY2), c.Wf(L.dxb),
                  (int*)(c.ws + L.rflags), L.T, L.B, L.h, L.w, L.P, nullptr, pair_budget(L.T),
                  rec_stagger("AAA_REC_STAGGER_BWD"), c.plan.cqm};
  // single-workgroup and paired kernels: row-padded images (recur_bwd.h kBwIBP) where they fit
  // (C3 LDS bank conflicts 52.8 -> 10.0 %: profiles/r04/ab/rowpad_c3/); AAA_BW_ROWPAD=0 (A/B): 272-B rows only
  rp.rowpad = fb <= 2 && ab_int("AAA_BW_ROWPAD", 1) ? bw_rowpad(L.h, L.w) : 0;
  rp.sc1_all = ab_int("AAA_BW_SC1_ALL", 0);   // band kernel (A/B): sc1 for every dZ row, as in round 4
  // single-workgroup kernel: the epilogue's inputs by LDS-DMA into a counted ring (recur_bwd.h RING)
  rp.ring = fb == 1 && ab_int("AAA_BW_RING", 0);   // measured slower: ablation builds only
  if (c.reset) {   // the single-workgroup kernel's mask variant (recur_bwd.h RST; the plan sends no other here)
    if (fb != 1) return fail(AAA_E_LAUNCH, "episode-start masks: no paired or band-mode bf16 BPTT kernel takes one");
    rp.reset = c.reset;
    rp.ring = 0;
  }
  if (fb >= 2)   // paired or band mode: hand-off flags [B][fb]
    if (const int rc = report_word("paired-kernel", &rp.report)) return rc;
  {
    // work: the h rows over T-1 steps (+ dh0) and the dx rows over all T (the batched dx it replaces)
    TimerScope tim(AAA_TIMER_BPTT_STEP, c.st, 2.0 * M * 4608 * (128.0 * (L.T - 1 + (io->dh0 ? 1 : 0)) + 64.0 * L.T),
                   fb == kRecBands && !rec_fits(L.h, L.w)
                       ? strf("bf16 band-mode frame-resident BPTT + dx, %d steps per launch, %d bands per frame, "
                              "fp16 gates [kernel: k_convlstm_bwd_frames<0, true]", L.T, fb)
                       : strf("bf16 frame-resident BPTT + dx, %d steps per launch, %d WG per frame, fp16 gates "
                              "[kernel: %s]%s", L.T, fb, fb == 2 ? "k_convlstm_bwd_pairs" : (rp.ring ? "k_convlstm_bwd_frames<ring>" : "k_convlstm_bwd_frames<0, false"), c.reset ? ", resets" : ""));
    HIPCHK(fb == 2 ? convlstm_bwd_pairs(rp, c.st) : (fb == 1 ? convlstm_bwd_frames(rp, c.st) : convlstm_bwd_band(rp, c.st)));
  }
  HIPCHK(colsum<float>(c.Wf(L.dxb), 64, L.B, 64, c.grads + L.poff[C1B], c.st));
  return AAA_OK;
}

// fp32: the frame-group BPTT (recur_bwd_f32.h, G = 8) behind the forward's frame-group kernel, one launch for
// the dh chain of all steps.  *dx_fused <- with split products it computed dx (dY2) and conv2's bias gradient too.
static int bptt_frames_f32(const CallCtx& c, bool* dx_fused) {
  const Layout& L = c.L;
  const aaa_io* io = c.io;
  const int M = L.B * L.P;
  int* rep = nullptr;
  if (const int rc = report_word("frame-group", &rep)) return rc;
  RecBwdF32Params rp{(const float*)(c.pk + L.k_Wb32), c.Wf(L.dO), c.Wf(L.Gt), c.Wf(L.Cst), c.Wf(L.dC), c.Wf(L.dZ), c.Wf(L.dZp),
                     io->dh0, c.Wf(L.xpart), (int*)(c.ws + L.rflags), rep, pair_budget(L.T), L.T, L.B, L.h, L.w, L.P, {}};
  const bool s6 = f32_split6();
  rp.reset = c.reset;
  rp.Wb6 = (const u32x2*)(c.pk + L.k_Wb6);
  if (s6) {   // dx fused (DX): conv2's output gradient and its bias partials from the same K loop
    rp.Wx6 = (const u32x2*)(c.pk + L.k_Wx6);
    rp.Wb6p = (const u32x4*)(c.pk + L.k_Wb6p);
    rp.Wx6p = (const u32x4*)(c.pk + L.k_Wx6p);
    rp.dx = c.Wf(L.dY2);
    rp.dxb = c.Wf(L.dxb);
  }
  {
    // work: the dh rows over T-1 steps (+ dh0), and with dx fused the dx rows over all T steps (the
    // batched dx it replaces) plus the dh rows of step 0 that the extra iteration computes
    const double dh_steps = L.T - 1 + ((io->dh0 || s6) ? 1 : 0);
    TimerScope tim(AAA_TIMER_BPTT_STEP, c.st, 2.0 * M * 4608 * (128.0 * dh_steps + (s6 ? 64.0 * L.T : 0.0)),
                   s6 ? strf("fp32 frame-group BPTT + dx (bf16x6 split products), %d steps per launch, 8 WG "
                             "per frame [kernel: k_convlstm_bwd_f32]%s", L.T, c.reset ? ", resets" : "")
                      : strf("fp32 frame-group BPTT (dh rows), %d steps per launch, 8 WG per frame "
                             "[kernel: k_convlstm_bwd_f32]", L.T));
    HIPCHK(convlstm_bwd_f32(rp, c.st, s6));
  }
  if (s6) HIPCHK(colsum<float>(c.Wf(L.dxb), 64, L.B, 64, c.grads + L.poff[C1B], c.st));
  *dx_fused = s6;
  return AAA_OK;
}

// One step of the per-step chain: dh_{t-1} = WdT[64:192] x gather(dZ_t) with the gate backward of step t-1 as
// the GEMM's epilogue (t = 0: dh0 out), then the episode-start rewrite of that step's rows
template <typename T>
static int bptt_step(const CallCtx& c, const BpttChain& ch, int t) {
  const Layout& L = c.L;
  const int M = L.B * L.P, ntj = cdiv(M, ch.bj);
  // bf16 under a mask: the GEMM stores the raw dgrad (its t = 0 form) into dO slot t -- dO_t was consumed by the gate
  // backward of step t, the launch before this one -- and the gate backward of step t-1 follows as a launch of its own
  const bool rawdh = c.reset && std::is_same<T, __bf16>::value && t > 0;
  const bool prev = t > 0 && !rawdh;
  const ConvGeo g = ConvGeo{512, 512, 0, L.h, L.w, L.h, L.w, 3, 1, 1, 1}.prep();
  const T* dzt = c.Wt<T>(L.dZ) + (size_t)t * M * 512;
  const uint32_t dz_bytes = (uint32_t)((size_t)M * 512 * L.esz);  // one step slice of dZ
  const T* WdTh = (const T*)(c.pk + L.k_WdTl) + (size_t)64 * 4608;
  float* part = ch.part && prev ? ch.part + (size_t)(t - 1) * ntj * 512 : nullptr;
  TimerScope tim(AAA_TIMER_BPTT_STEP, c.st, 2.0 * M * 128 * 4608, strf("%s dh dgrad + %s gate bwd, K=4608, AAA_BPTT_TILE %d%s%s", std::is_same<T, float>::value ? "fp32" : "bf16", rawdh ? "masked (k_gate_bwd_resets)" : "fused", ch.tile, ch.g16 ? ", fp16 gates [kernel: EpiConvLstmBwd]" : " [kernel: EpiConvLstmBwd]", c.reset ? ", resets" : ""));
  // (the raw-dh form of a masked bf16 step: the plan's tile, as the fused form; a split-K family's through its t = 0 entry)
  const int tile_id = prev || (rawdh && ch.split == SplitK::None) ? ch.tile : ch.dh0;
  auto step = [&](auto gtag) -> int {
    using GT = decltype(gtag);
    using EB = EpiConvLstmBwd<T, GT>;
    const GT* gates = prev ? (const GT*)(c.ws + L.Gt) + (size_t)(t - 1) * M * 512 : nullptr;
    float* cprev = prev ? c.Wf(L.Cst) + (size_t)(t - 1) * M * 128 : nullptr;
    float* dO = prev ? c.Wf(L.dO) + (size_t)(t - 1) * M * 128 : nullptr;
    T* dzp = prev ? c.Wt<T>(L.dZ) + (size_t)(t - 1) * M * 512 : nullptr;
    const EB ep{nullptr, gates, cprev, c.Wf(L.Cst) + (size_t)t * M * 128, dO, c.Wf(L.dC), dzp,
                prev ? nullptr : (rawdh ? c.Wf(L.dO) + (size_t)t * M * 128 : c.io->dh0), prev ? 1 : 0, M, 64, part};
    return for_tile<BpttTiles>(tile_id, (int)AAA_E_ARG, [&](auto tile) -> int {
      using Tl = decltype(tile);
      using CK = typename Tl::template Cfg<T>;
      if constexpr (!Tl::template serves<T, GT>()) {
        // e.g. bf16 with fp32 gate storage and a tile that exists for fp16 gates only: fail loudly, never fall back
        return fail(AAA_E_LAUNCH, "AAA_BPTT_TILE %d: no kernel for this operand / gate storage type", tile_id);
      } else if constexpr (Tl::split != SplitK::None) {
        if (!L.dhs) return fail(AAA_E_ARG, "AAA_BPTT_TILE %d: split-K needs B*P < 8192 (got %d)", ch.tile, M);
        const int ns = splitk_slices(4608, CK::BK, bptt_splitk());   // as launch_pipe rounds it
        float* dhp = c.Wf(L.dhs);
        if constexpr (Tl::split == SplitK::SliceFix) {   // the last slice of each tile runs the gate backward
          int* cnt = (int*)(c.ws + L.dhs + (size_t)std::max(kBpttSplitMax * 128, 4 * 512) * M * 4);
          const EpiSliceFix<EB> ef{dhp, 128, 128, M, (size_t)M * 128, ns, cdiv(M, 32), cnt, ep};   // (ep.part: null)
          HIPCHK((step_gemm_splitk<CK>(WdTh, 4608, 128, dzt, g, M, dz_bytes, ef, 128, 4608, c.st, ns, Tl::ILV)));
        } else {   // K-slice partials, then the gate backward
          const EpiSliceT es{dhp, 128, 128, M, (size_t)M * 128};
          HIPCHK((step_gemm_splitk<CK>(WdTh, 4608, 128, dzt, g, M, dz_bytes, es, 128, 4608, c.st, ns, Tl::ILV)));
          HIPCHK((gate_bwd_last<T, GT>(M, ch.bj, dO, dhp, gates, cprev, c.Wf(L.Cst) + (size_t)t * M * 128, c.Wf(L.dC),
                                       dzp, part, c.st, ns, (size_t)M * 128)));
        }
      } else {
        HIPCHK((step_gemm<CK, Tl::stage != Stage::Reg, T, T, EB, Tl::NBUF, Tl::ILV>(WdTh, 4608, 128, dzt, g, M, dz_bytes,
                                                                                    ep, 128, 4608, c.st)));
      }
      return AAA_OK;
    });
  };
  if (const int rc = ch.g16 ? step(_Float16{}) : step(float{})) return rc;
  if (rawdh) return bptt_gates_resets(c, ch, t, c.Wf(L.dO) + (size_t)t * M * 128);
  return prev ? bptt_fix<T>(c, t) : AAA_OK;
}

// Phase CORE: the ConvLSTM BPTT, t = T-1 .. 0, in one frame-resident (bf16) or frame-group (fp32) launch or step
// by step on c.st -- only the h rows (dh_{t-1}, fused with the gate backward of step t-1) are sequential --
// and everything else in chunks off the chain (core_chunk; with VISION in ``phases`` the vision backward of
// each chunk's frames too).  deferred_unpack: null, or where to leave the ConvLSTM grads' reference tensors
// for the VISION phase of this call, whose launch then unpacks them with the vision grads.
template <typename T>
static int core_backward(const CallCtx& c, int phases, LstmGrads* deferred_unpack) {
  const Layout& L = c.L;
  const aaa_io* io = c.io;
  const hipStream_t st = c.st;
  const int M = L.B * L.P;
  const bool vision_here = (phases & AAA_BWD_VISION) != 0;
  hipStream_t ax = aux_stream();
  hipStream_t os = ax ? ax : st;     // stream for the off-chain chunks
  const int cs = chunk_steps(L);
  std::unique_ptr<TimerScope> misc(new TimerScope(AAA_TIMER_MISC, st, 0.0, "BPTT state in, last-step gate backward"));
  {   // dc_T = 0 (or the carried grad), and the frame kernels' hand-off flags and dx bias partials: one launch
    ZeroRanges z{};
    if (!io->dcT) z.add(c.Wf(L.dC), (long)M * 128);
    z.add(c.Wf(L.rflags), (long)8 * L.B);
    z.add(c.Wf(L.dxb), (long)L.B * 64);
    HIPCHK(prologue<T>(z, 0, nullptr, (T*)nullptr, 0, 0, 1, nullptr, nullptr, nullptr, st));
    if (io->dcT) HIPCHK(hipMemcpyAsync(c.Wf(L.dC), io->dcT, (size_t)M * 128 * 4, hipMemcpyDeviceToDevice, st));
  }
  const int bwd_tile = c.plan.bwd_tile;
  if (bwd_tile < 0) return tile_unknown("AAA_BPTT_TILE");
  BpttChain ch = for_tile<BpttTiles>(bwd_tile, BpttChain{}, [bwd_tile](auto tile) {
    using Tl = decltype(tile);
    return BpttChain{bwd_tile, Tl::split == SplitK::None ? Tl::template Cfg<T>::BJ : kSplitBj, Tl::template pipe<T>(),
                     Tl::split, Tl::dh0, false, nullptr};
  });
  const bool fixk = ch.split == SplitK::SliceFix;   // split-K finished in the GEMM: bias from dZ's column sum
  if (fixk && L.dhs)   // the fixup counters (self-resetting; zeroed per call in case a launch was abandoned)
    HIPCHK(hipMemsetAsync(c.ws + L.dhs + (size_t)std::max(kBpttSplitMax * 128, 4 * 512) * M * 4, 0, 4096, st));
  ch.g16 = c.plan.g16;
  const int fb = c.plan.fb;   // bf16: workgroups per frame of the frame-resident launch, 0: none
  const bool fb32 = c.plan.fb32;   // fp32: the frame-group launch (a mask: its RST variant, with dx fused)
  // Gate-bias partials from the step kernels' epilogues: ring tiles only; not where the frame-group kernel
  // writes its own per-(step, frame) partials (step T-1's included); not under an fp32 mask, where the gate-bias
  // gradient is the column sum of the final (fp32) dZ, not of partials taken before bptt_fix's rewrite.  (bf16
  // under a mask: the masked gate backward writes the partials itself, bptt_gates_resets.)
  ch.part = ch.pipe && !fixk && !fb32 && !(c.reset && std::is_same<T, float>::value) ? c.Wf(L.dZp) : nullptr;
  if (!fb)
    if (const int rc = bptt_last_gates<T>(c, ch)) return rc;
  misc.reset();
  bool dx_fused = false;   // the BPTT launch computed dx (dY2) and conv2's bias gradient itself
  if constexpr (std::is_same<T, float>::value) {
    if (fb32)
      if (const int rc = bptt_frames_f32(c, &dx_fused)) return rc;
  } else if (fb) {
    if (const int rc = bptt_frames_bf16(c, fb)) return rc;
    dx_fused = true;
  }
  int done_hi = L.T;   // chunks [lo, done_hi) not yet issued
  auto flush = [&](int ready_lo) -> int {   // dz of steps >= ready_lo are final
    while (done_hi - ready_lo >= cs || (ready_lo == 0 && done_hi > 0)) {
      const int lo = std::max(ready_lo, done_hi - cs);
      if (ax) HIPCHK(stream_order(st, ax));
      if (const int rc = core_chunk<T>(c, lo, done_hi, os, dx_fused, vision_here)) return rc;
      done_hi = lo;
    }
    return AAA_OK;
  };
  for (int t = (fb || fb32) ? -1 : L.T - 1; t >= 0; --t) {
    if (const int rc = flush(t)) return rc;   // dz_t .. dz_{T-1} are final here
    if (t == 0 && !io->dh0) break;
    if (const int rc = bptt_step<T>(c, ch, t)) return rc;
  }
  if (const int rc = flush(0)) return rc;
  misc.reset(new TimerScope(AAA_TIMER_MISC, st, 0.0, "gate-bias column sums, state grads out, grad unpack"));
  // gate-bias gradient: column sum of the per-(step, tile) partials, or of dZ itself
  if (fb)   // per (step, frame[, pixel half]) partials
    HIPCHK(colsum<float>(c.Wf(L.dZp), 512, L.T * L.B * fb, 512, c.Wf(L.gbl), st));
  else if (fb32)   // per (step, frame) partials
    HIPCHK(colsum<float>(c.Wf(L.dZp), 512, L.T * L.B, 512, c.Wf(L.gbl), st));
  else if (ch.part) HIPCHK(colsum<float>(ch.part, 512, L.T * cdiv(M, ch.bj), 512, c.Wf(L.gbl), st));
  else HIPCHK(colsum<T>(c.Wt<T>(L.dZ), 512, L.F * L.P, 512, c.Wf(L.gbl), st));
  if (c.reset)   // rows whose episode starts at step 0: h0 / c0 were not read, their cotangents are exactly 0
    HIPCHK(reset_rows(c.reset, L.B, L.P, ResetZeros{}.add(c.Wf(L.dC), 128, 128).add(io->dh0, 128, 128), nullptr, nullptr,
                      0, st));
  if (io->dc0) HIPCHK(hipMemcpyAsync(io->dc0, c.Wf(L.dC), (size_t)M * 128 * 4, hipMemcpyDeviceToDevice, st));
  if (ax) HIPCHK(stream_order(ax, st));   // join
  LstmGrads lg;
  for (int g = 0; g < 4; ++g) {
    lg.wx[g] = c.grads + L.poff[XI_W + 3 * g];
    lg.bx[g] = c.grads + L.poff[XI_B + 3 * g];
    lg.wh[g] = c.grads + L.poff[HI_W + 3 * g];
  }
  if (deferred_unpack) *deferred_unpack = lg;
  else HIPCHK(unpack_lstm(c.Wf(L.gWpl), c.Wf(L.gbl), lg, st));
  return AAA_OK;
}

// Phase VISION: the conv2 / conv1 backward over all frames unless CORE ran it chunk by chunk in this call
// (then core_unpack holds the ConvLSTM grads' reference tensors), and the unpack of the packed gradients.
template <typename T>
static int vision_backward(const CallCtx& c, int phases, const LstmGrads& core_unpack) {
  const Layout& L = c.L;
  const bool vision_here = (phases & AAA_BWD_CORE) != 0;   // done with the CORE phase's chunks
  TimerScope tim(AAA_TIMER_VISION_BWD, c.st, vision_here ? 0.0 : (double)L.F * vision_bwd_flop(L),
                 vision_bwd_variant(vbwd_on<T>(L, L.F), std::is_same<T, float>::value));
  if (!vision_here) {   // VISION alone: frame-resident, or its chunk work over all frames, here
    // (layered: the image rebuilt from the observation where Xp is a chunk buffer or the forward may have stored none)
    const bool rebuild = L.xpc < L.F || vis_frames_layout(L);
    const int rc = vision_bwd_alone<T>(L, c.pk, c.io->frames, c.Wt<T>(L.dY2), c.Wt<T>(L.Y1), c.Wt<T>(L.Xp),
                                       c.Wt<T>(L.dY1), nullptr, 0, L.F, c.Wf(L.gWp2), c.Wf(L.gWp1),
                                       c.grads + L.poff[C0B], c.st, rebuild ? c.io->frames : nullptr, nullptr);
    if (rc) return rc;
  }
  HIPCHK(unpack_cv(vision_here ? c.Wf(L.gWpl) : nullptr, c.Wf(L.gbl), core_unpack, c.Wf(L.gWp2),
                   c.grads + L.poff[C1W], c.Wf(L.gWp1), c.grads + L.poff[C0W], c.st));
  return AAA_OK;
}

template <typename T>
int backward_impl(const Layout& L, const aaa_io* io, int phases, hipStream_t st, const float* reset) {
  const CallCtx c(L, io, st, reset, AAA_TIMER_TAIL_BWD);
  const bool vision = (phases & AAA_BWD_VISION) != 0;
  LstmGrads core_unpack{};   // the ConvLSTM grads' reference tensors, unpacked with the vision grads when both run here
  if (phases & AAA_BWD_HEAD)
    if (const int rc = head_backward<T>(c)) return rc;
  if (phases & AAA_BWD_CORE)
    if (const int rc = core_backward<T>(c, phases, vision ? &core_unpack : nullptr)) return rc;
  if (vision)
    if (const int rc = vision_backward<T>(c, phases, core_unpack)) return rc;
  return AAA_OK;
}

template int lstm_wgrad<float>(const float*, const float*, int, int, int, float*, hipStream_t, bool);
template int lstm_wgrad<__bf16>(const __bf16*, const __bf16*, int, int, int, float*, hipStream_t, bool);
template int vision_bwd<float>(const Layout&, const char*, const float*, const float*, float*, float*, int,
                               float*, float*, float*, hipStream_t, const void*);
template int vision_bwd<__bf16>(const Layout&, const char*, const __bf16*, const __bf16*, __bf16*, __bf16*, int,
                                float*, float*, float*, hipStream_t, const void*);
template int vision_bwd_alone<float>(const Layout&, const char*, const void*, const float*, const float*, float*,
                                     float*, void*, size_t, int, float*, float*, float*, hipStream_t, const void*,
                                     bool*, int, float*, const void*);
template int vision_bwd_alone<__bf16>(const Layout&, const char*, const void*, const __bf16*, const __bf16*, __bf16*,
                                      __bf16*, void*, size_t, int, float*, float*, float*, hipStream_t, const void*,
                                      bool*, int, float*, const void*);
template int backward_impl<float>(const Layout&, const aaa_io*, int, hipStream_t, const float*);
template int backward_impl<__bf16>(const Layout&, const aaa_io*, int, hipStream_t, const float*);

}  // namespace aaa
