// Forward of the unroll (attention.py:298-368 over T steps): weight packing,
// the vision encoder, the ConvLSTM recurrence (frame-resident / frame-group /
// per-step kernels) and the batched attention / answer / policy-core / heads tail.
#include "rt.h"

namespace aaa {

// ------------------------------------------------------------- packing ----
template <typename T>
int pack_impl(const Layout& L, const float* prm, char* pk, hipStream_t st) {
  PackAll<T> a;
  a.c1w = prm + L.poff[C0W];
  a.c2w = prm + L.poff[C1W];
  a.Wp1 = (T*)(pk + L.k_Wp1); a.Wp2 = (T*)(pk + L.k_Wp2); a.WdT2 = (T*)(pk + L.k_WdT2);
  if constexpr (std::is_same<T, float>::value) {   // the frame-resident fp32 encoder's pre-split weights (vision_f32.h)
    a.W1s = (__bf16*)(pk + L.k_W1s); a.W2s = (__bf16*)(pk + L.k_W2s);
    a.WdT2s = (__bf16*)(pk + L.k_WdT2s);
  }
  for (int g = 0; g < 4; ++g) {
    a.lstm.wx[g] = prm + L.poff[XI_W + 3 * g];
    a.lstm.bx[g] = prm + L.poff[XI_B + 3 * g];
    a.lstm.wh[g] = prm + L.poff[HI_W + 3 * g];
  }
  a.WpX = (T*)(pk + L.k_WpX); a.WpH = (T*)(pk + L.k_WpH); a.WdT = (T*)(pk + L.k_WdTl);
  a.WpXH = (T*)(pk + L.k_WpXH); a.bl = (float*)(pk + L.k_bl);
  F32Pack& fp = a.f32;
  fp.a0w = prm + L.poff[A0W]; fp.wih = prm + L.poff[WIH]; fp.bih = prm + L.poff[BIH]; fp.bhh = prm + L.poff[BHH];
  fp.pw = prm + L.poff[PW]; fp.vw = prm + L.poff[VW]; fp.pb = prm + L.poff[PB]; fp.vb = prm + L.poff[VB];
  fp.W1p = (float*)(pk + L.k_W1p); fp.Wihp = (float*)(pk + L.k_Wihp); fp.blc = (float*)(pk + L.k_blc);
  fp.Whd = (float*)(pk + L.k_Whd); fp.bhd = (float*)(pk + L.k_bhd);
  fp.ans_in = L.ans_in; fp.ans_ld = L.ans_ld; fp.A = L.A; fp.ldy = L.ldy;
  if (L.sc) {
    fp.whh = prm + L.poff[WHH];
    fp.Wihhp = (float*)(pk + L.k_Wihhp);
  }
  HIPCHK(pack_all<T>(a, st));   // conv1, conv2, conv2 dgrad classes, ConvLSTM layouts, fp32 tail: one launch
  if constexpr (!std::is_same<T, float>::value) {   // fragment orders of the frame-resident kernels (read WpXH / WdT)
    HIPCHK(pack_wfrag((const __bf16*)(pk + L.k_WpXH), (__bf16*)(pk + L.k_Wfr), st));
    HIPCHK(pack_wbfrag((const __bf16*)(pk + L.k_WdTl), (__bf16*)(pk + L.k_Wbf), st));
  } else {   // the fp32 frame-group recurrence's fragment order (recur_f32.h)
    // (pack_all wrote WpXH / WdT first: same stream)
    HIPCHK(pack_frag_f32(FragPack{(const float*)(pk + L.k_WpXH), (const float*)(pk + L.k_WdTl), (float*)(pk + L.k_Wf32),
                                  (u32x2*)(pk + L.k_Wf6), (u32x4*)(pk + L.k_Wf6p), (float*)(pk + L.k_Wb32),
                                  (u32x2*)(pk + L.k_Wb6), (u32x2*)(pk + L.k_Wx6), (u32x4*)(pk + L.k_Wb6p),
                                  (u32x4*)(pk + L.k_Wx6p), (__bf16*)(pk + L.k_WdT6)},
                         st));
  }
  HIPCHK(query_pack(prm + L.poff[Q0B], prm + L.poff[Q2W], prm + L.poff[Q2B], prm + L.poff[Q4W], prm + L.poff[Q4B], L.nq,
                    (float*)(pk + L.k_q1), (float*)(pk + L.k_q2), (float*)(pk + L.k_Q), st));
  return AAA_OK;
}

// Vision encoder over F frames (VisionNetwork.vision_cnn, attention.py:155-170,
// on X.transpose(1,3), :179 -- Q3): frames (F,H,W,3) -> zero-bordered RGBx
// image Xp -> conv 8/4/1 -> Y1 (F,H1,W1,32) -> conv 4/2/2 -> out (F,h,w,64) at
// row pitch out_ld (the ConvLSTM operand slots, or a plain output), no
// activation in between.  Packed conv weights at L.k_Wp1 / L.k_Wp2, biases
// from the flat params (state_dict order: the vision tensors come first).
template <typename T, typename OT>
static int vision_fwd_chunk(const Layout& L, int F, const char* pk, const float* prm, const void* frames, T* Xp, T* Y1,
                      OT* out, int out_ld, hipStream_t st, bool xp_full, std::string* ran) {
  using C = CfgFor<T>;
  constexpr int NT = C::NT;
  const int P = L.P;
  bool banded = false;   // bf16 frames too large for the frame-resident encoder: the banded conv1 (vision.h)
  if constexpr (std::is_same<T, __bf16>::value) {
    if (band_fits(L.H, L.W, L.H1, L.W1) && env_int("AAA_VIS_BAND", 1)) {
      const VisBandParams bp{frames, (const __bf16*)(pk + L.k_Wp1), prm + L.poff[C0B], xp_full ? Xp : nullptr, Y1, F,
                             L.H, L.W, L.H1, L.W1};
      HIPCHK(L.fu8 ? vision_conv1_band<uint8_t>(bp, st) : vision_conv1_band<float>(bp, st));
      banded = true;
    }
  }
  if (!banded) {  // conv1 (attention.py:156-162): frames -> zero-bordered RGBx (Cin 4, pad 1 stored) -> Y1
    // xp_full: Xp holds all F frames (the component entries keep it for their backward);
    // else Xp is the chunk buffer of L.xpc frames, rebuilt per chunk right before conv1 reads it
    const size_t fb = (size_t)L.H * L.W * 3 * (L.fu8 ? 1 : 4), xb = (size_t)(L.H + 2) * (L.W + 2) * 4;
    const int step = xp_full ? F : L.xpc;
    for (int s0 = 0; s0 < F; s0 += step) {
      const int n = std::min(step, F - s0);
      const char* fr = (const char*)frames + (size_t)s0 * fb;
      T* xp = xp_full ? Xp + (size_t)s0 * xb : Xp;
      if (L.fu8) HIPCHK((frames_rgbx<T, uint8_t>(n, L.H, L.W, (const uint8_t*)fr, xp, st)));
      else HIPCHK((frames_rgbx<T, float>(n, L.H, L.W, (const float*)fr, xp, st)));
      // LDS-DMA ring, 32x128 tile over 4 waves (tools/ubench/conv_cfg: 62 vs 90 us register-staged)
      constexpr int BKc = std::is_same<T, float>::value ? 32 : 64;
      EpiStoreT<T> ep{Y1 + (size_t)s0 * L.P1 * 32, 32, 32, n * L.P1, prm + L.poff[C0B], 0};
      auto conv1 = [&](auto cfg) -> int {
        using CP = decltype(cfg);
        using PA = GRowsB<T, CP::BI, CP::BK, CP::NT>;
        using PB = GIm2colB<T, CP::BJ, CP::BK, CP::NT>;
        HIPCHK((launch_pipe<CP, PA, PB, EpiStoreT<T>, 2>(
            typename PA::Params{(const T*)(pk + L.k_Wp1), 256, 32},
            typename PB::Params{xp, ConvGeo{4, 4, 0, L.H + 2, L.W + 2, L.H1, L.W1, 8, 4, 0, 0}.prep(), n * L.P1,
                                (uint32_t)((size_t)n * xb * L.esz)},
            ep, 32, n * L.P1, 256, 1, st)));
        return AAA_OK;
      };
      // K = 256 is four BK steps: a wider column tile does more MFMA work per DMA round trip (A/B: AAA_CONV1_TILE)
      const int c1t = ab_int("AAA_CONV1_TILE", 0);
      int rc;
      if constexpr (std::is_same<T, float>::value) {   // fp32 accuracy on the bf16 MFMA (gemm.h SPLIT6)
        // uint8 frames: the RGBx operand is exact in bf16 (three of the six split products, GemmCfgS6BX)
        if (f32_split6()) rc = L.fu8 && ab_int("AAA_CONV1_BEXACT", 1) ? conv1(GemmCfgS6BX<32, 128, BKc, 1, 4>{})
                                                                      : conv1(GemmCfgS6<32, 128, BKc, 1, 4>{});
        else rc = c1t == 1 ? conv1(GemmCfg<T, 32, 256, BKc, 1, 4>{}) : conv1(GemmCfg<T, 32, 128, BKc, 1, 4>{});
      } else {
        rc = c1t == 1 ? conv1(GemmCfg<T, 32, 256, BKc, 1, 4>{}) : conv1(GemmCfg<T, 32, 128, BKc, 1, 4>{});
      }
      if (rc) return rc;
    }
  }
  if constexpr (std::is_same<T, __bf16>::value && std::is_same<OT, __bf16>::value) {
    // after the banded conv1: the banded conv2 (vision.h), Y1 rows staged in LDS per band
    if (banded && band2_fits(L.H1, L.W1, L.h, L.w) && ab_int("AAA_VIS_BAND2", 1)) {
      const VisBand2Params bp{Y1, (const __bf16*)(pk + L.k_Wp2), prm + L.poff[C1B], out, out_ld, F, L.H1, L.W1, L.h, L.w};
      HIPCHK(vision_conv2_band(bp, st));
      if (ran) *ran = "banded conv1 [kernel: k_vision_conv1_band], banded conv2 [kernel: k_vision_conv2_band]";
      return AAA_OK;
    }
  }
  {  // conv2 (attention.py:163-169): Y1 -> out
    using LA = LdRowsB<T, T, C::BI, C::BK, NT>;
    typename LA::Params pa{(const T*)(pk + L.k_Wp2), 512, 64};
    const ConvGeo g = ConvGeo{32, 32, 0, L.H1, L.W1, L.h, L.w, 4, 2, 2, 0}.prep();
    EpiStoreT<OT> ep{out, out_ld, 64, F * P, prm + L.poff[C1B], 0};
    const uint32_t y1b = (uint32_t)((size_t)F * L.P1 * 32 * L.esz);
    if constexpr (32 % C::BK == 0) {   // LDS-DMA ring (tools/ubench/conv_cfg: 62 vs 67 us)
      if (std::is_same<T, float>::value && f32_split6())   // fp32 accuracy on the bf16 MFMA (gemm.h SPLIT6)
        HIPCHK((step_gemm<std::conditional_t<std::is_same<T, float>::value, typename S6Of<C>::type, C>, true>(
            (const T*)(pk + L.k_Wp2), 512, 64, (const T*)Y1, g, F * P, y1b, ep, 64, 512, st)));
      else
        HIPCHK((step_gemm<C, true>((const T*)(pk + L.k_Wp2), 512, 64, (const T*)Y1, g, F * P, y1b, ep, 64, 512, st)));
    } else if (pipe_batched()) {   // bf16: a BK=32 ring, one 4x4 tap row's 32 channels per K tile
      HIPCHK((step_gemm<GemmCfg<T, 64, 128, 32, 2, 2>, true>((const T*)(pk + L.k_Wp2), 512, 64, (const T*)Y1, g,
                                                           F * P, y1b, ep, 64, 512, st)));
    } else {
      using LB = LdIm2col<T, T, C::BJ, C::BK, NT, true>;
      HIPCHK((launch_gemm<C, LA, LB>(pa, typename LB::Params{Y1, g, F * P}, ep, 64, F * P, 512, 1, st)));
    }
  }
  if (ran)
    *ran = banded ? "banded conv1 [kernel: k_vision_conv1_band], conv2 im2col GEMM"
                  : "layered: frames_rgbx, conv1 im2col ring, conv2 im2col GEMM";
  return AAA_OK;
}


template <typename T, typename OT>
int vision_fwd(const Layout& L, int F, const char* pk, const float* prm, const void* frames, T* Xp, T* Y1,
                      OT* out, int out_ld, hipStream_t st, bool xp_full, std::string* ran, bool resident_xp) {
  // The frame-resident kernels read the observation themselves: Xp is only a by-product for a layered
  // backward, stored for the component and checker entries (resident_xp) and never for the learner, whose
  // backward rebuilds the image wherever one of them can run (rt.h vis_frames_layout).
  T* const rxp = xp_full && resident_xp ? Xp : nullptr;
  if constexpr (std::is_same<T, __bf16>::value && std::is_same<OT, __bf16>::value) {
    // bf16: the frame-resident encoder (vision.h), one launch; AAA_VIS_FRAMES=0 -> the layered kernels
    if (vis_frames_on(L)) {
      VisFwdParams vp{frames, (const __bf16*)(pk + L.k_Wp1), prm + L.poff[C0B], (const __bf16*)(pk + L.k_Wp2),
                      prm + L.poff[C1B], rxp, Y1, out, out_ld, F, L.H, L.W, L.H1, L.W1, L.h, L.w};
      HIPCHK(L.fu8 ? vision_fwd_frames<uint8_t>(vp, device_cus(), st) : vision_fwd_frames<float>(vp, device_cus(), st));
      if (ran) *ran = std::string("frame-resident conv1 + conv2 [kernel: k_vision_fwd]") + (rxp ? "" : ", no Xp");
      return AAA_OK;
    }
  }
  if constexpr (std::is_same<T, float>::value && std::is_same<OT, float>::value) {
    // fp32 split products: the frame-resident encoder (vision_f32.h), one launch, which also writes the
    // fp32 Y1 the backward reads; AAA_VIS_FRAMES=0 -> the layered kernels
    if (f32_split6() && vis_frames_on(L)) {
      VisF32Params vp{frames, (const bf16x8*)(pk + L.k_W1s), prm + L.poff[C0B], (const bf16x8*)(pk + L.k_W2s),
                      prm + L.poff[C1B], rxp, Y1, out, out_ld, F, L.H, L.W, L.H1, L.W1, L.h, L.w};
      HIPCHK(L.fu8 ? vision_fwd_frames_f32<uint8_t>(vp, device_cus(), st)
                   : vision_fwd_frames_f32<float>(vp, device_cus(), st));
      if (ran)
        *ran = std::string("frame-resident conv1 + conv2 (bf16x6 split products) [kernel: k_vision_fwd_f32]") +
               (rxp ? "" : ", no Xp");
      return AAA_OK;
    }
  }
  for (int f0 = 0; f0 < F; f0 += L.fchunk) {   // descriptor-sized frame chunks (check_ranges)
    const int n = std::min(L.fchunk, F - f0);
    const int rc = vision_fwd_chunk<T, OT>(L, n, pk, prm,
                                           (const char*)frames + (size_t)f0 * L.H * L.W * 3 * (L.fu8 ? 1 : 4),
                                           xp_full ? Xp + (size_t)f0 * (L.H + 2) * (L.W + 2) * 4 : Xp,
                                           Y1 + (size_t)f0 * L.P1 * 32, out + (size_t)f0 * L.P * out_ld, out_ld, st,
                                           xp_full, ran);
    if (rc) return rc;
  }
  return AAA_OK;
}

// ------------------------------------------------------------- forward ----
// The phases of one forward call (forward_impl, at the end) share its CallCtx (rt.h).
// conv1 + conv2 over all T*B frames -> XH[:, :, 0:64] of every slot
template <typename T>
static int vision_forward(const CallCtx& c) {
  const Layout& L = c.L;
  TimerScope tim(AAA_TIMER_VISION_FWD, c.st, (double)L.F * vision_fwd_flop(L), "conv1 + conv2 (vision encoder)");
  std::string ran;   // the kernels the dispatch took, for the timer's variant
  const int rc = vision_fwd<T, T>(L, L.F, c.pk, c.prm, c.io->frames, c.Wt<T>(L.Xp), c.Wt<T>(L.Y1), c.Wt<T>(L.XH), 192,
                                  c.st, L.xpc >= L.F, &ran, false);
  if (rc) return rc;
  tim.variant += ": " + ran;
  return AAA_OK;
}

// initial state (reset(): zeros, attention.py:142-149) or carried state
template <typename T>
static int state_in(const CallCtx& c, bool core) {
  const Layout& L = c.L;
  const aaa_io* io = c.io;
  const int M = L.B * L.P;
  TimerScope tim(AAA_TIMER_MISC, c.st, 0.0, "state in/out copies, memsets, bias column sums");
  // one launch: h_0 into XH slot 0, c_0 = 0 (reset) and the hand-off flags of this forward's
  // multi-workgroup recurrence launch (zeroed here for every kernel choice)
  ZeroRanges z{};
  if (!io->c0) z.add(c.Wf(L.Cst), (long)M * 128);
  if (core) z.add(c.Wf(L.rflags), (long)8 * L.B);
  HIPCHK(prologue<T>(z, M, io->h0, c.Wt<T>(L.XH), 0, 0, 1, nullptr, nullptr, nullptr, c.st));
  if (io->c0 && (c.plan.cqm & kCqmC)) HIPCHK(cqm_convert(io->c0, c.Wf(L.Cst), L.B, L.P, 1, c.st));
  else if (io->c0) HIPCHK(hipMemcpyAsync(c.Wf(L.Cst), io->c0, (size_t)M * 128 * 4, hipMemcpyDeviceToDevice, c.st));
  return AAA_OK;
}

// fp32 h_t slice of step t for the readout: fp32 path only (bf16 reads XH, readout_h)
static float* hs_out(const CallCtx& c, int t) {
  return c.L.esz == 4 ? c.Wf(c.L.Hs) + (size_t)t * (c.L.B * c.L.P) * 128 : (float*)nullptr;
}
// Episode starts (reset != null): before step t, zeros in the h half of XH slot t for the rows
// that enter it from reset() and a masked copy of c_{t-1} (in dC: the BPTT's carry, idle in the
// forward) -- Cst slot t keeps the true c_{t-1}, which step t-1's own backward reads (resets.hip).
// bf16: slot t's h half is also the only copy of h_{t-1}, so it goes to HR slot t-1 (the readout's
// copy, rt.h readout_h) before the rows are zeroed.
// *cp <- the c_{t-1} the step's cell update reads.
template <typename T>
static int c_in(const CallCtx& c, int t, const float** cp) {
  const Layout& L = c.L;
  const int M = L.B * L.P;
  *cp = c.Wf(L.Cst) + (size_t)t * M * 128;
  if (!c.reset) return AAA_OK;
  T* xht = c.Wt<T>(L.XH) + (size_t)t * M * 192;
  if constexpr (std::is_same<T, __bf16>::value)
    if (t > 0) HIPCHK(xh_to_hr(M, xht, c.Wt<__bf16>(L.HR) + (size_t)(t - 1) * M * 128, c.st));
  HIPCHK(reset_rows(c.reset + (size_t)t * L.B, L.B, L.P, ResetZerosT<T>{}.add(xht + 64, 192, 128), *cp, c.Wf(L.dC), 128,
                    c.st));
  *cp = c.Wf(L.dC);
  return AAA_OK;
}
// bf16 under a mask, after the last step of a per-step chain: h_{T-1} (XH slot T, which no step zeroes) -> HR
template <typename T>
static int hr_last(const CallCtx& c) {
  if constexpr (std::is_same<T, __bf16>::value) {
    const Layout& L = c.L;
    const size_t M = (size_t)L.B * L.P;
    if (c.reset) HIPCHK(xh_to_hr((long)M, c.Wt<__bf16>(L.XH) + (size_t)L.T * M * 192, c.Wt<__bf16>(L.HR) + (size_t)(L.T - 1) * M * 128, c.st));
  }
  return AAA_OK;
}

// fp32: one frame-group launch for all T steps, x-part included (recur_f32.h); under a mask its RST variant
static int recur_frames_f32(const CallCtx& c) {
  const Layout& L = c.L;
  const aaa_io* io = c.io;
  const int M = L.B * L.P, G = c.plan.fwd_g;
  int* rep = nullptr;
  if (const int rc = report_word("frame-group", &rep)) return rc;
  RecF32Params rp{(const float*)(c.pk + L.k_Wf32), (const float*)(c.pk + L.k_bl), c.Wf(L.XH), c.Wf(L.Cst), c.Wf(L.Hs),
                  c.Wf(L.Gt), (int*)(c.ws + L.rflags), rep, pair_budget(L.T), L.T, L.B, L.h, L.w, L.P, io->h0 ? 0 : 1, {}};
  if (c.reset) {   // slot 0's h half of the rows that start an episode at step 0: the weight gradient's operand
    rp.reset = c.reset;
    if (io->h0)
      HIPCHK(reset_rows(c.reset, L.B, L.P, ResetZeros{}.add(c.Wf(L.XH) + 64, 192, 128), nullptr, nullptr, 0, c.st));
  }
  const bool s6 = f32_split6();
  rp.Wf6 = (const u32x2*)(c.pk + L.k_Wf6);
  rp.Wf6p = (const u32x4*)(c.pk + L.k_Wf6p);
  TimerScope tim(AAA_TIMER_FWD_STEP, c.st, 2.0 * M * 512 * (576.0 * L.T + 1152.0 * (L.T - (io->h0 ? 0 : 1))),
                 strf("fp32 frame-group [x|h] recurrence%s, %d steps per launch, %d WG per frame [kernel: %s]%s",
                      s6 ? " (bf16x6 split products)" : "", L.T, G,
                      f32_fwd_presplit(s6, G, L.P) ? "k_convlstm_fwd_f32ps" : "k_convlstm_fwd_f32<", c.reset ? ", resets" : ""));
  HIPCHK(convlstm_fwd_f32(rp, G, c.st, s6));
  return AAA_OK;
}

// bf16: one frame-resident launch for all T steps (recur.h) -- band mode (fwd_g bands per frame), or one
// workgroup or a pair per frame.  GT: the gate storage type.
template <typename GT>
static int recur_frames_bf16(const CallCtx& c) {
  const Layout& L = c.L;
  const bool band = c.plan.fwd == RecurFwd::BandBf16;
  const int M = L.B * L.P, G = c.plan.fwd_g;
  int* rep = nullptr;
  if (band || G == 2)   // hand-off between a frame's workgroups
    if (const int rc = report_word(band ? "band-mode" : "paired-kernel", &rep)) return rc;
  RecFwdParams<GT> rp{(const __bf16*)(c.pk + L.k_Wfr), (const float*)(c.pk + L.k_bl), c.Wt<__bf16>(L.XH), c.Wf(L.Cst),
                      nullptr, (GT*)(c.ws + L.Gt), (int*)(c.ws + L.rflags), L.T, L.B, L.h, L.w, L.P, rep,
                      pair_budget(L.T), rec_stagger("AAA_REC_STAGGER_FWD")};
  rp.cqm = c.plan.cqm;
  if (c.reset) {   // the single-workgroup kernel's mask variant (recur.h RST; the plan sends no other here)
    if (band || G != 1) return fail(AAA_E_LAUNCH, "episode-start masks: no paired or band-mode bf16 kernel takes one");
    rp.reset = c.reset;
    rp.HR = c.Wt<__bf16>(L.HR);
    // slot 0's h half of the rows that start an episode at step 0: this launch's and the weight gradient's operand
    if (c.io->h0)
      HIPCHK(reset_rows(c.reset, L.B, L.P, ResetZerosT<__bf16>{}.add(c.Wt<__bf16>(L.XH) + 64, 192, 128), nullptr, nullptr, 0,
                        c.st));
  }
  // row-padded h image (recur.h rec_rowpad): measured neutral to 1 % slower (C3 forward 1234-1242 vs
  // 1247-1269 us, profiles/r06/ab/rowpad_fwd/), so an A/B option (AAA_REC_ROWPAD=1, ablation builds)
  if (!band) rp.rowpad = ab_int("AAA_REC_ROWPAD", 0) ? rec_rowpad(L.h, L.w) : 0;
  TimerScope tim(AAA_TIMER_FWD_STEP, c.st, 2.0 * M * 512 * 1728 * L.T,
                 band ? strf("bf16 band-mode frame-resident [x|h] recurrence, %d steps per launch, %d bands per frame "
                             "[kernel: k_convlstm_fwd_frames+Lb1E]", L.T, G)
                      : strf("bf16 frame-resident [x|h] recurrence, %d steps per launch, %d WG per frame%s [kernel: k_convlstm_fwd_frames+Lb0E]%s",
                             L.T, G, rp.rowpad ? ", row-padded h image" : "", c.reset ? ", resets" : ""));
  HIPCHK(band ? convlstm_fwd_frames_band<GT>(rp, c.st) : convlstm_fwd_frames<GT>(rp, G, c.st));
  return AAA_OK;
}

// Per step, the x-part riding in the step's GEMM (K over the whole XH slot, [x_t | h_{t-1}], bias in the
// epilogue): no batched x-part GEMM and no fp32 x-part round trip through HBM (tools/ubench/bf16_tiles: the
// step's epilogue traffic, not its MFMAs, is half its time).  The tiles and their measurements: rt.h fused_step.
template <typename T, typename GT>
static int recur_fused_steps(const CallCtx& c) {
  const Layout& L = c.L;
  const int M = L.B * L.P;
  for (int t = 0; t < L.T; ++t) {   // ConvLSTM (attention.py:110-126), x- and h-part together
    const float* cp;
    if (const int rc = c_in<T>(c, t, &cp)) return rc;
    EpiConvLstmFwd<T, GT> ep{cp, c.Wf(L.Cst) + (size_t)(t + 1) * M * 128, hs_out(c, t),
                             c.Wt<T>(L.XH) + (size_t)(t + 1) * M * 192, (GT*)(c.ws + L.Gt) + (size_t)t * M * 512, M,
                             (const float*)(c.pk + L.k_bl)};
    const int rc = fused_step<T, GT>((const T*)(c.pk + L.k_WpXH), c.Wt<T>(L.XH) + (size_t)t * M * 192, L.h, L.w, M, ep,
                                     c.st, L.dhs ? c.Wf(L.dhs) : nullptr, c.reset != nullptr);
    if (rc) return rc;
  }
  return hr_last<T>(c);
}

// The x-part of the ConvLSTM steps (not recurrent), batched: Gt <- Wx * x_t + b, in chunks of ``cs`` steps on
// the aux stream; then the h-part step by step, step t waiting only for its chunk.
template <typename T>
static int recur_xpart_steps(const CallCtx& c) {
  const Layout& L = c.L;
  const hipStream_t st = c.st;
  const int M = L.B * L.P, fwd_tile = c.plan.fwd_tile;
  hipStream_t ax = aux_stream();
  const int cs = chunk_steps(L);
  hipStream_t xs = ax ? ax : st;
  if (ax) HIPCHK(stream_order(st, ax));
  hipEvent_t xev[64];
  const int nchunks = (L.T + cs - 1) / cs;
  if (ax && nchunks > 48) return fail(AAA_E_ARG, "too many overlap chunks (T=%d, AAA_CHUNK=%d)", L.T, cs);
  for (int k = 0; k < nchunks; ++k) {   // the x-part of steps [lo, hi)
    const int lo = k * cs, hi = std::min(L.T, (k + 1) * cs), rows = (hi - lo) * M;
    // 64x64 tiles (128x128 measured slower: K is only 576)
    const ConvGeo g = ConvGeo{64, 192, 0, L.h, L.w, L.h, L.w, 3, 1, 1, 0}.prep();
    EpiStoreT<float> ep{c.Wf(L.Gt) + (size_t)lo * M * 512, 512, 512, rows, (const float*)(c.pk + L.k_bl), 0};
    const T* WpX = (const T*)(c.pk + L.k_WpX);
    const T* xs0 = c.Wt<T>(L.XH) + (size_t)lo * M * 192;
    const uint32_t xb = (uint32_t)((size_t)(hi - lo) * M * 192 * L.esz);
    switch (pipe_batched() ? ab_int("AAA_XPART_TILE", 0) : -1) {   // A/B: tools/ab_batched.sh
      case -1: HIPCHK((step_gemm<CfgFor<T>, false>(WpX, 576, 512, xs0, g, rows, xb, ep, 512, 576, xs))); break;
#ifdef AAA_ABLATION   // the measured-slower x-part tiles
      using EX = EpiStoreT<float>;
      case 1: HIPCHK((step_gemm<Cfg64For<T>, true>(WpX, 576, 512, xs0, g, rows, xb, ep, 512, 576, xs))); break;
      case 2: HIPCHK((step_gemm<CfgFor<T>, true, T, T, EX, 3, true>(WpX, 576, 512, xs0, g, rows, xb, ep, 512, 576, xs))); break;
      case 3: HIPCHK((step_gemm<CfgJFor<T>, true>(WpX, 576, 512, xs0, g, rows, xb, ep, 512, 576, xs))); break;
      case 4: HIPCHK((step_gemm<CfgSFor<T>, true>(WpX, 576, 512, xs0, g, rows, xb, ep, 512, 576, xs))); break;
      case 5:
        HIPCHK((step_gemm<GemmCfg<T, 128, 128, 32, 2, 2>, true>(WpX, 576, 512, xs0, g, rows, xb, ep, 512, 576, xs)));
        break;
#endif
      default: HIPCHK((step_gemm<CfgFor<T>, true>(WpX, 576, 512, xs0, g, rows, xb, ep, 512, 576, xs))); break;
    }
    if (ax) HIPCHK(record_event(ax, &xev[k]));
  }
  const uint32_t xh_bytes = (uint32_t)((size_t)M * 192 * L.esz);  // one step slice of XH
  for (int t = 0; t < L.T; ++t) {  // ConvLSTM recurrence (attention.py:110-126): h-part only
    if (ax && t % cs == 0) HIPCHK(hipStreamWaitEvent(st, xev[t / cs], 0));   // x-part of steps [t, t+cs) done
    const float* cp;
    if (const int rc = c_in<T>(c, t, &cp)) return rc;
    if (t == 0 && !c.io->h0) {       // zero state: gates come from the x-part alone
      HIPCHK(gate_fwd_zx<T>(M, cp, c.Wf(L.Gt), c.Wf(L.Cst) + (size_t)M * 128, hs_out(c, 0),
                            c.Wt<T>(L.XH) + (size_t)M * 192, st));
      continue;
    }
    EpiConvLstmFwd<T> ep{cp, c.Wf(L.Cst) + (size_t)(t + 1) * M * 128, hs_out(c, t),
                         c.Wt<T>(L.XH) + (size_t)(t + 1) * M * 192, c.Wf(L.Gt) + (size_t)t * M * 512, M};
    const ConvGeo g = ConvGeo{128, 192, 64, L.h, L.w, L.h, L.w, 3, 1, 1, 0}.prep();
    TimerScope tim(AAA_TIMER_FWD_STEP, st, 2.0 * M * 512 * 1152, strf("%s h-part step (x-part batched), K=1152, tile %d [kernel: EpiConvLstmFwd]%s", std::is_same<T, float>::value ? "fp32" : "bf16", fwd_tile, c.reset ? ", resets" : ""));
    const T* WpH = (const T*)(c.pk + L.k_WpH);
    const T* xh = c.Wt<T>(L.XH) + (size_t)t * M * 192;
    const hipError_t e = for_tile<FwdTiles>(fwd_tile, hipErrorInvalidValue, [&](auto tile) {
      using Tl = decltype(tile);
      return step_gemm<typename Tl::template Cfg<T>, Tl::stage != Stage::Reg, T, T, EpiConvLstmFwd<T>, Tl::NBUF, Tl::ILV>(
          WpH, 1152, 512, xh, g, M, xh_bytes, ep, 512, 1152, st);
    });
    HIPCHK(e);
  }
  return hr_last<T>(c);
}

// The ConvLSTM recurrence on the plan's path, with fp16 or fp32 gate storage
template <typename T>
static int core_forward(const CallCtx& c) {
  const RecurPlan& p = c.plan;
  // (the h-part tile of the per-step chain: an unknown id is refused whichever kernel runs)
  if (p.fwd_tile < 0) return tile_unknown("AAA_STEP_TILE");
  if constexpr (std::is_same<T, float>::value) {
    if (p.fwd == RecurFwd::FramesF32) return recur_frames_f32(c);
  } else if (p.fwd == RecurFwd::BandBf16 || p.fwd == RecurFwd::FramesBf16) {
    return p.g16 ? recur_frames_bf16<_Float16>(c) : recur_frames_bf16<float>(c);
  }
  if (p.fwd == RecurFwd::XpartSteps) return recur_xpart_steps<T>(c);
  return p.g16 ? recur_fused_steps<T, _Float16>(c) : recur_fused_steps<T, float>(c);
}

// answer_processor.0 + ReLU and answer_processor.2 (attention.py:277-282, 350) over ``rows`` frames from f0:
// their answer rows -> hid1 -> ``out`` (pitch out_ld)
static int answer_mlp(const CallCtx& c, size_t f0, int rows, float* out, int out_ld) {
  const Layout& L = c.L;
  float* hid = c.Wf(L.hid1) + f0 * 512;
  HIPCHK(tail_gemm({(const float*)(c.pk + L.k_W1p), L.ans_ld, 512}, {c.Wf(L.ans) + f0 * L.ans_ld, L.ans_ld, rows},
                   EpiStoreT<float>{hid, 512, 512, rows, c.prm + L.poff[A0B], 1}, 512, rows, L.ans_ld, c.st));
  HIPCHK(tail_gemm({c.prm + L.poff[A2W], 512, 256}, {hid, 512, rows},
                   EpiStoreT<float>{out, out_ld, 256, rows, c.prm + L.poff[A2B], 0}, 256, rows, 512, c.st));
  return AAA_OK;
}

// Stateful policy core (AAA_FLAG_STATEFUL_CORE; the reference's else branch,
// attention.py:324-331, 356-358): per step t, over the B frames of that step,
//   Q_t = QueryNetwork(h_{t-1}) -> attention readout with the per-frame Q_t ->
//   answer MLP -> LSTMCell([answer | h_{t-1}], c_{t-1}) -> (h_t, c_t).
// State slots CH/CC[t] hold (h, c) entering step t (slot 0 = io->core_*0 or
// zeros); the LSTMCell epilogue also writes h_t into step t+1's [answer | h]
// GEMM row, so each step is five small GEMMs and one attention launch.  The
// heads then run batched over all frames on CH[1..T].
static int forward_tail_stateful(const CallCtx& c) {
  const Layout& L = c.L;
  const aaa_io* io = c.io;
  const hipStream_t st = c.st;
  const float* prm = c.prm;
  const int B = L.B, P = L.P, qd = L.qd;
  const size_t sB = (size_t)B * 256 * 4;
  float *CH = c.Wf(L.CH), *CC = c.Wf(L.CC), *AOX = c.Wf(L.AOX);
  if (io->core_h0) HIPCHK(hipMemcpyAsync(CH, io->core_h0, sB, hipMemcpyDeviceToDevice, st));
  else HIPCHK(hipMemsetAsync(CH, 0, sB, st));
  if (io->core_c0) HIPCHK(hipMemcpyAsync(CC, io->core_c0, sB, hipMemcpyDeviceToDevice, st));
  else HIPCHK(hipMemsetAsync(CC, 0, sB, st));
  HIPCHK(hipMemcpy2DAsync(AOX + 256, 512 * 4, CH, 256 * 4, 256 * 4, B, hipMemcpyDeviceToDevice, st));
  for (int t = 0; t < L.T; ++t) {
    const size_t f0 = (size_t)t * B;
    float* q1 = c.Wf(L.q1s) + f0 * 128;
    float* q2 = c.Wf(L.q2s) + f0 * qd;
    float* Qt = c.Wf(L.Qf) + f0 * qd;
    // Episode starts: zeros in the h half of this step's [answer | h] rows for the rows that enter it
    // from reset(), and a masked copy of c_{t-1} (in dcc: the backward's carry, idle here); the query
    // MLP then reads h_{t-1} from those rows, its second copy.  CH / CC slot t keep the true
    // (h, c)_{t-1}: the heads and step t-1's backward read them.
    const float* hq = CH + f0 * 256;
    const float* cprev = CC + f0 * 256;
    int hq_ld = 256;
    if (c.reset) {
      HIPCHK(reset_rows(c.reset + f0, B, 1, ResetZeros{}.add(AOX + f0 * 512 + 256, 512, 256), cprev, c.Wf(L.dcc), 256, st));
      hq = AOX + f0 * 512 + 256;
      hq_ld = 512;
      cprev = c.Wf(L.dcc);
    }
    // QueryNetwork(prev_output = h_{t-1}) (attention.py:184-198, 331)
    HIPCHK(tail_gemm({prm + L.poff[Q0W], 256, 128}, {hq, hq_ld, B},
                     EpiStoreT<float>{q1, 128, 128, B, prm + L.poff[Q0B], 1}, 128, B, 256, st));
    HIPCHK(tail_gemm({prm + L.poff[Q2W], 128, qd}, {q1, 128, B},
                     EpiStoreT<float>{q2, qd, qd, B, prm + L.poff[Q2B], 1}, qd, B, 128, st));
    HIPCHK(tail_gemm({prm + L.poff[Q4W], qd, qd}, {q2, qd, B}, EpiStoreT<float>{Qt, qd, qd, B, prm + L.poff[Q4B], 0},
                     qd, B, qd, st));
    // attention readout with this step's per-frame queries (basis logits in-kernel)
    {
      TimerScope tim(AAA_TIMER_ATTN_FWD, st, (double)B * attn_fwd_bytes(P, L.nq, L.ans_ld, L.esz), L.esz == 2 ? "k_attn_fwd_mfma, per-frame query (stateful core)" : "k_attn_fwd, per-frame query (stateful core)");
      HIPCHK(attn_fwd(readout_h(L, c.ws, c.reset != nullptr).frame(f0, P), io->basis, Qt, nullptr, io->prev_reward ? io->prev_reward + f0 : nullptr,
                      io->prev_action ? io->prev_action + f0 : nullptr, B, P, L.nq, c.Wf(L.Am) + f0 * P * L.nq,
                      c.Wf(L.ans) + f0 * L.ans_ld, L.ans_ld, st, qd));
    }
    // the answer MLP -> the answer half of this step's [answer | h_{t-1}] rows
    if (const int rc = answer_mlp(c, f0, B, AOX + f0 * 512, 512)) return rc;
    // policy_core LSTMCell from (h_{t-1}, c_{t-1}) (attention.py:356-358)
    HIPCHK(tail_gemm({(const float*)(c.pk + L.k_Wihhp), 512, 1024}, {AOX + f0 * 512, 512, B},
                     EpiLstmCellFwdS{(const float*)(c.pk + L.k_blc), c.Wf(L.LG) + f0 * 1024, cprev, CC + (f0 + B) * 256,
                                     CH + (f0 + B) * 256, t + 1 < L.T ? AOX + (f0 + B) * 512 + 256 : nullptr, B},
                     1024, B, 512, st));
  }
  if (io->attn)
    HIPCHK(hipMemcpyAsync(io->attn, c.Wf(L.Am), (size_t)L.F * P * L.nq * 4, hipMemcpyDeviceToDevice, st));
  return AAA_OK;
}

// The zero-state tail (Q1): the constant query, the attention readout, the answer MLP and the LSTMCell, all
// batched over the T*B frames
static int forward_tail_batched(const CallCtx& c) {
  const Layout& L = c.L;
  const aaa_io* io = c.io;
  const hipStream_t st = c.st;
  const int F = L.F, P = L.P;
  // constant query (Q1) + fused attention readout over all T*B frames
  const float* Qc = (const float*)(c.pk + L.k_Q);
  {
    TimerScope tim(AAA_TIMER_TAIL_FWD, st, 0.0, "query basis logits");
    HIPCHK(query_sq(io->basis, Qc, P, L.nq, c.Wf(L.SQ), st));
  }
  {
    TimerScope tim(AAA_TIMER_ATTN_FWD, st, (double)F * attn_fwd_bytes(P, L.nq, L.ans_ld, L.esz), L.esz == 2 ? "k_attn_fwd_mfma (readout on the MFMA, map and basis in bf16 parts), 1 WG per frame" : "k_attn_fwd (VALU), 1 WG per frame");
    HIPCHK(attn_fwd(readout_h(L, c.ws, c.reset != nullptr), io->basis, Qc, c.Wf(L.SQ), io->prev_reward, io->prev_action, F, P, L.nq,
                    c.Wf(L.Am), c.Wf(L.ans), L.ans_ld, st));
  }
  TimerScope tim(AAA_TIMER_TAIL_FWD, st, (double)F * tail_fwd_flop(L), "answer MLP + LSTMCell + heads (fp32 GEMMs)");
  if (io->attn) HIPCHK(hipMemcpyAsync(io->attn, c.Wf(L.Am), (size_t)F * P * L.nq * 4, hipMemcpyDeviceToDevice, st));
  if (const int rc = answer_mlp(c, 0, F, c.Wf(L.AO), 256)) return rc;
  // policy_core LSTMCell from zero state (attention.py:354-355)
  HIPCHK(tail_gemm({(const float*)(c.pk + L.k_Wihp), 256, 1024}, {c.Wf(L.AO), 256, F},
                   EpiLstmCellFwd{(const float*)(c.pk + L.k_blc), c.Wf(L.LG), c.Wf(L.LC), c.Wf(L.LH), F}, 1024, F, 256, st));
  return AAA_OK;
}

// Everything after the ConvLSTM: query, attention readout, answer MLP, LSTMCell (batched over the T*B frames,
// or step by step for the stateful core), then the heads over all frames and the state outputs.
static int forward_tail(const CallCtx& c) {
  const Layout& L = c.L;
  const aaa_io* io = c.io;
  const hipStream_t st = c.st;
  const int F = L.F, M = L.B * L.P;
  const size_t sB = (size_t)L.B * 256;   // one slot of the stateful core's CH / CC
  if (const int rc = L.sc ? forward_tail_stateful(c) : forward_tail_batched(c)) return rc;
  TimerScope tim(AAA_TIMER_TAIL_FWD, st, L.sc ? 0.0 : 2.0 * F * 256 * 2 * L.A, "policy/value heads + state out");
  // policy / values heads (attention.py:365-367), batched over all frames
  HIPCHK(tail_gemm({(const float*)(c.pk + L.k_Whd), 256, 2 * L.A},
                   {L.sc ? c.Wf(L.CH) + sB : c.Wf(L.LH), 256, F},
                   EpiHeads{io->logits, io->values, (const float*)(c.pk + L.k_bhd), L.A, F}, 2 * L.A, F, 256, st));
  if (io->hT && L.esz == 2)   // h_{T-1} from XH slot T (the bf16 path keeps no fp32 h_t)
    HIPCHK(xh_to_state<__bf16>(M, (const __bf16*)(c.ws + L.XH) + (size_t)L.T * M * 192, io->hT, st));
  else if (io->hT)
    HIPCHK(hipMemcpyAsync(io->hT, c.Wf(L.Hs) + (size_t)(L.T - 1) * M * 128, (size_t)M * 128 * 4,
                          hipMemcpyDeviceToDevice, st));
  if (io->cT && (c.plan.cqm & kCqmC)) HIPCHK(cqm_convert(c.Wf(L.Cst) + (size_t)L.T * M * 128, io->cT, L.B, L.P, 0, st));
  else if (io->cT)
    HIPCHK(hipMemcpyAsync(io->cT, c.Wf(L.Cst) + (size_t)L.T * M * 128, (size_t)M * 128 * 4, hipMemcpyDeviceToDevice, st));
  if (L.sc && io->core_hT) HIPCHK(hipMemcpyAsync(io->core_hT, c.Wf(L.CH) + L.T * sB, sB * 4, hipMemcpyDeviceToDevice, st));
  if (L.sc && io->core_cT) HIPCHK(hipMemcpyAsync(io->core_cT, c.Wf(L.CC) + L.T * sB, sB * 4, hipMemcpyDeviceToDevice, st));
  return AAA_OK;
}

template <typename T>
int forward_impl(const Layout& L, const aaa_io* io, hipStream_t st, int phases, const float* reset) {
  const CallCtx c(L, io, st, reset, AAA_TIMER_TAIL_FWD);
  const bool core = (phases & AAA_FWD_CORE) != 0;
  if (const int rc = vision_forward<T>(c)) return rc;
  if (const int rc = state_in<T>(c, core)) return rc;
  // (no CORE, aaa_forward_phases: aaa_core_import has left the recurrence's products in Gt / Cst / Hs / XH)
  if (core)
    if (const int rc = core_forward<T>(c)) return rc;
  return forward_tail(c);
}

template int pack_impl<float>(const Layout&, const float*, char*, hipStream_t);
template int pack_impl<__bf16>(const Layout&, const float*, char*, hipStream_t);
template int vision_fwd<float, float>(const Layout&, int, const char*, const float*, const void*, float*, float*,
                                      float*, int, hipStream_t, bool, std::string*, bool);
template int vision_fwd<__bf16, __bf16>(const Layout&, int, const char*, const float*, const void*, __bf16*, __bf16*,
                                        __bf16*, int, hipStream_t, bool, std::string*, bool);
template int vision_fwd<__bf16, float>(const Layout&, int, const char*, const float*, const void*, __bf16*, __bf16*,
                                       float*, int, hipStream_t, bool, std::string*, bool);
template int forward_impl<float>(const Layout&, const aaa_io*, hipStream_t, int, const float*);
template int forward_impl<__bf16>(const Layout&, const aaa_io*, hipStream_t, int, const float*);

}  // namespace aaa
