// Internal header of the host runtime (csrc/runtime.hip and the rt_*.hip
// translation units): the buffer layout, error/timing/stream state (defined
// once in rt_core.hip) and the GEMM launch helpers shared by the forward
// (rt_forward.hip), the backward (rt_backward.hip) and the component entries
// (rt_components.hip).  The tile configurations and the per-step kernels'
// tile ids: step_tiles.h.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "aaa.h"
#include "epilogues.h"
#include "gemm.h"
#include "loaders_b.h"
#include "glds.h"
#include "gemm_deep.h"
#include "halo.h"
#include "recur.h"
#include "recur_bwd.h"
#include "recur_f32.h"
#include "recur_bwd_f32.h"
#include "vision.h"
#include "vision_f32.h"
#include "vision_bwd.h"
#include "vision_bwd_f32.h"
#include "misc.h"
#include "optim.h"
#include "actor.h"
#include "step_tiles.h"


namespace aaa {

extern thread_local std::string g_err;   // aaa_last_error()

int fail(int code, const char* fmt, ...);

#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(AAA_E_LAUNCH, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                  __FILE__, __LINE__);                                                    \
  } while (0)

inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// (0 when the padded input is smaller than the kernel: C's division truncates toward zero, and
// (n + 2p - k) / s + 1 would call a 4x4 frame a 1x1 conv1 map whose 8x8 window is not there)
inline int conv_out(int n, int k, int s, int p) {
  const int d = n + 2 * p - k;
  return d < 0 ? 0 : d / s + 1;
}

enum PIdx {
  C0W = 0, C0B, C1W, C1B,
  XI_W, XI_B, HI_W, XF_W, XF_B, HF_W, XC_W, XC_B, HC_W, XO_W, XO_B, HO_W,
  Q0W, Q0B, Q2W, Q2B, Q4W, Q4B, A0W, A0B, A2W, A2B, WIH, WHH, BIH, BHH, PW, PB, VW, VB, NPARAM
};

struct Layout {
  int B, T, F, H, W, H1, W1, P1, h, w, P, nq, A, dt, esz;
  int sc;   // stateful policy core (AAA_FLAG_STATEFUL_CORE)
  int fu8;  // frames are uint8 (AAA_FLAG_FRAMES_U8)
  int br;   // bf16 cfg that takes episode-start masks (AAA_FLAG_BF16_RESETS): the HR region exists
  int fchunk;   // frames per launch of the whole-batch conv GEMMs (< 2 GiB per descriptor, check_ranges)
  int xpc;      // frames of the Xp chunk buffer (conv1's bordered RGBx operand, rebuilt per chunk)
  int qd, da, ans_in, ans_ld, ldy;
  size_t poff[NPARAM], psz[NPARAM], ptotal;
  size_t k_Wp1, k_Wp2, k_WdT2, k_W1s, k_W2s, k_WpX, k_WpH, k_WpXH, k_Wfr, k_Wbf, k_Wf32, k_Wb32, k_Wf6, k_Wf6p, k_Wb6, k_Wx6, k_Wb6p, k_Wx6p, k_WdTl, k_WdTc, k_WdT6, k_bl, k_Wihhp, k_q1, k_q2, k_Q, k_W1p, k_Wihp, k_blc, k_Whd, k_bhd, k_WdT2s, packed;
  size_t Xp, Y1, XH, Hs, HR, Cst, Gt, SQ, Am, ans, hid1, AO, LG, LC, LH;
  size_t dY, dLG, dAO, dH1, dAns, dO, dQp, dQs, dC, dZ, dZp, dY2, dY1, dxb, rflags, xpart, dhs, dZ6;
  size_t gWp1, gWp2, gWpl, gbl, gW1p, gWihp, gblc, gWhd, gbhd, ws;
  // stateful core: state slots, per-step query activations, [answer | h] rows, their grads
  size_t CH, CC, AOX, Qf, q1s, q2s, dAOX, dQf, dq2s, dq1s, dhc, dcc, gWihhp;
};

// Algorithmic FLOP per frame of the other timer classes:
// conv1 (K = 8*8*3) and conv2 (K = 4*4*32) forward; the answer MLP + LSTMCell
// (zero state: W_ih only); their backward is twice that (dgrad + wgrad); the
// conv2 wgrad + dgrad and conv1 wgrad of the vision backward.
inline double vision_fwd_flop(const Layout& L) { return 2.0 * L.P1 * 32 * 192 + 2.0 * L.P * 64 * 512; }
inline double tail_fwd_flop(const Layout& L) {
  return 2.0 * ((double)L.ans_in * 512 + 512.0 * 256 + 256.0 * 1024);
}
inline double vision_bwd_flop(const Layout& L) { return 2.0 * (2.0 * L.P * 64 * 512) + 2.0 * L.P1 * 32 * 192; }

// min_frames: the frames one launch must be able to address (a step's B for
// the unroll; 1 for the frame-independent vision encoder entries).
int build_layout(const aaa_cfg* c, Layout& L, int min_frames = 0);
int check_device();

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------- paired-kernel reports --
// Timed-out partner waits of the multi-workgroup frame kernels (common.h pair_wait), counted per device in a
// host-mapped report word (rt_core.hip); every aaa_forward / aaa_backward entry consumes them: AAA_E_STRANDED.
int pair_budget(int T);    // partner-wait budget of a T-step launch, 100-MHz ticks
int* pair_report(int dev);  // this device's report word, device-mapped (nullptr: cannot map)
int* pair_flag_base(int dev);  // aaa_pair_flag's own snapshot of it, device-mapped
int pair_take();            // pending reports of the current device (consumed)
int pair_peek();            // ... (left pending)
int pair_check();           // AAA_E_STRANDED if any are pending
// *rep <- the current device's report word for a multi-workgroup recurrence (``what`` names its kind)
inline int report_word(const char* what, int** rep) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (!(*rep = pair_report(dev))) return fail(AAA_E_LAUNCH, "cannot map the %s report word", what);
  return AAA_OK;
}

// ----------------------------------------- aux and side streams (rt_core.hip) --
hipStream_t aux_stream();   // nullptr unless AAA_OVERLAP=1 (measured slower on C2, round 1)
hipStream_t side_stream();  // the backward HEAD phase's weight gradients (rt_core.hip); nullptr: AAA_SIDE=0
// Record a pooled event on ``s`` (everything enqueued on s so far).
hipError_t record_event(hipStream_t s, hipEvent_t* out);
// ``to`` waits for everything enqueued on ``from`` so far.
hipError_t stream_order(hipStream_t from, hipStream_t to);

// ------------------------------------------------- optional kernel timing --
// Per timer class: the HIP event pairs of each launch, the launches'
// algorithmic work (FLOP for the MFMA classes, bytes for the HBM ones) and
// the kernel variant dispatched -- so a benchmark reads the roofline inputs
// from the library instead of re-deriving its dispatch rules.
struct Timers {
  std::mutex mu;
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[AAA_TIMER_N];
  double work[AAA_TIMER_N] = {};
  std::string variant[AAA_TIMER_N];
  // the tail GEMMs' dispatch since the class was last read (tail_ran): (kernel/arithmetic, equal launches in a row)
  std::vector<std::pair<std::string, int>> ran[AAA_TIMER_N];
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
};
extern Timers g_timers;

struct TimerScope {
  int kind;
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  double work;
  std::string variant;
  TimerScope(int k, hipStream_t s, double w, std::string v) : kind(k), st(s), work(w), variant(std::move(v)) {
    std::lock_guard<std::mutex> lk(g_timers.mu);
    if (!g_timers.on) return;
    a = g_timers.get();
    b = g_timers.get();
    if (a && b) (void)hipEventRecord(a, st);
  }
  ~TimerScope() {
    if (!a || !b) return;
    (void)hipEventRecord(b, st);
    std::lock_guard<std::mutex> lk(g_timers.mu);
    g_timers.pending[kind].emplace_back(a, b);
    g_timers.work[kind] += work;
    g_timers.variant[kind] = variant;
  }
};

std::string strf(const char* fmt, ...);

// Algorithmic bytes per frame of the fused attention readout kernels (fp32):
// forward reads the frame's O rows (128 ch) and writes its map and answer row;
// backward reads O, the map and the answer grad, writes dO and dQ.
// per frame: O read (oesz bytes per element: 4 fp32 Hs, 2 the bf16 XH copy), A and the answer row written
inline double attn_fwd_bytes(int P, int nq, int ans_ld, int oesz = 4) {
  return oesz * 128.0 * P + 4.0 * (nq * P + ans_ld);
}
// per frame: O read, dO written (fp32), A / da / Q read, dQ written
inline double attn_bwd_bytes(int P, int nq, int oesz = 4) {
  return oesz * 128.0 * P + 4.0 * (128.0 * P + nq * P + 184.0 * nq + 72.0 * nq);
}

// (env_int: common.h)
// A/B-only knobs (the same-box comparisons of tools/gpu_ab*.sh): read from the
// environment only in -DAAA_ABLATION builds (make ablation -> libaaa_ablation.so,
// loaded through AAA_LIB); the product library takes the default.  env_int stays
// for the path selectors the parity tests drive.
inline int ab_int(const char* name, int dflt) {
#ifdef AAA_ABLATION
  return env_int(name, dflt);
#else
  (void)name;
  return dflt;
#endif
}
// Steps per off-chain chunk: the whole unroll unless overlapping, and never
// more than the frames one launch may address (Layout::fchunk).
static int chunk_steps(const Layout& L) {
  const int c = ab_int("AAA_CHUNK", ab_int("AAA_OVERLAP", 0) ? 4 : L.T);
  return std::max(1, std::min({c, L.T, L.fchunk / L.B}));
}
bool f32_split6();   // fp32 path: large GEMMs as bf16x6 split products on the bf16 MFMA (gemm.h SPLIT6; rt_core.hip)
// A frame-resident forward (k_vision_fwd / k_vision_fwd_f32) can run on this layout.  The learner's
// forward then stores no Xp, so the backward never trusts the Xp region's contents where this holds:
// its layered launches rebuild the image from the observation (conv1_wgrad_frames).  Stated on the
// layout alone, not on AAA_VIS_FRAMES / AAA_VIS_BWD_FRAMES, which may change between the two calls.
inline bool vis_frames_layout(const Layout& L) {
  return vis_fits(L.H, L.W, L.H1, L.W1, L.h, L.w) && (L.dt == AAA_BF16 || f32_split6());
}
// ... and this call may run one (AAA_VIS_FRAMES=0: the layered kernels, forward and backward)
inline bool vis_frames_on(const Layout& L) { return vis_fits(L.H, L.W, L.H1, L.W1, L.h, L.w) && env_int("AAA_VIS_FRAMES", 1); }
// A tile variable names an id that no family holds (RecurPlan's tiles < 0, fused_step): the launch site refuses
static int tile_unknown(const char* env) {
  return fail(AAA_E_ARG, "%s %d: no such tile id (csrc/step_tiles.h)", env, env_int(env, -1));
}

// Split-K BPTT (fp32 tiles 30/31): K slices of the per-step dh dgrad, summed by
// the gate backward (misc.hip k_gate_bwd_last).  Only where the step has few
// output tiles (the B=1 episode: 4 x 17), so the partials stay small.
constexpr int kBpttSplitMax = 8;
constexpr int kSplitBj = 8;   // pixels per gate-backward workgroup (and gate-bias partial row) of the split-K chain
static bool bptt_splitk_fits(int M) { return 4L * ((M + 31) / 32) < 1024; }
static int bptt_splitk() { return std::max(2, std::min(kBpttSplitMax, env_int("AAA_BPTT_SPLITK", 4))); }
// K slices launch_pipe actually runs for a requested nsplit (glds.h: whole BK tiles per slice)
inline int splitk_slices(int K, int BK, int nsplit) {
  const int kc = ((K + nsplit - 1) / nsplit + BK - 1) / BK * BK;
  return (K + kc - 1) / kc;
}

// ------------------------------------------------------ recurrence plan --
// How one call runs the ConvLSTM recurrence and how its state lies in the workspace: decided once per call from the
// layout, the environment and the device (recur_plan, rt_core.hip: the rules and their measurements) and read by the
// forward, the BPTT and the entries that describe the workspace, which therefore agree.  Nothing is kept between calls.
enum class RecurFwd {
  FramesF32,    // fp32 frame-group launch, fwd_g workgroups per frame (recur_f32.h)
  BandBf16,     // bf16 band-mode frame-resident launch, fwd_g bands per frame (recur.h BAND)
  FramesBf16,   // bf16 frame-resident launch, fwd_g = 1 or 2 workgroups per frame (recur.h)
  FusedSteps,   // per step, x- and h-part in one GEMM
  XpartSteps    // batched x-part, then the h-part per step
};
struct RecurPlan {
  bool fused_x;             // the x-part rides in the step GEMM (AAA_FUSED_X)
  int bwd_tile, fwd_tile;   // AAA_BPTT_TILE / AAA_STEP_TILE of the per-step chains (step_tiles.h); < 0: no such id
  bool g16;                 // gate activations stored as fp16 (gate_bytes 2), else fp32 (4)
  int gate_bytes;
  RecurFwd fwd;             // the forward's path and its workgroups (bands) per frame, 0 for the per-step paths
  int fwd_g;
  int fb;                   // bf16 frame-resident BPTT: workgroups (bands) per frame, 0: the per-step chain
  bool fb32;                // fp32 frame-group BPTT (G = 8)
  int cqm;                  // recur.h kCqm* mask of the channel-quad-major Cst / Gt / dO slices; 0: all row-major
};
// resets: the call carries an episode-start mask, which not every frame kernel takes (bf16: none of the paired,
// band-mode and BPTT frame kernels)
RecurPlan recur_plan(const Layout& L, bool resets);
bool gates_f16(int dt, int M);   // the plan's g16 for the component cell entries, which have no Layout

// One per-step ConvLSTM GEMM: D[Mi][M] = W[Mi][K] x im2col(src)[K][M] with
// epilogue ep.  PIPE = LDS-DMA ring (glds.h; needs src already in T),
// otherwise the register-staged kernel (which can convert fp32 -> bf16).
template <class CK, bool PIPE, typename T, typename G, class EP, int NBUF = 2, bool ILV = false>
static hipError_t step_gemm(const T* W, int ldw, int wrows, const G* src, const ConvGeo& g, int M, uint32_t src_bytes,
                            const EP& ep, int Mi, int K, hipStream_t st, int nsplit = 1) {
  if constexpr (PIPE && pipe_even<CK>() && std::is_same<G, T>::value) {
    using LA = GRowsB<T, CK::BI, CK::BK, CK::NT>;
    using LB = GIm2colB<T, CK::BJ, CK::BK, CK::NT>;
    return launch_pipe<CK, LA, LB, EP, NBUF, ILV>(typename LA::Params{W, ldw, wrows},
                                                  typename LB::Params{src, g, M, src_bytes}, ep, Mi, M, K, nsplit, st);
  } else {
    if (nsplit != 1) return hipErrorInvalidValue;   // split-K: ring tiles only
    using LA = LdRowsB<T, T, CK::BI, CK::BK, CK::NT>;
    using LB = LdIm2colB<G, T, CK::BJ, CK::BK, CK::NT>;
    return launch_gemm<CK, LA, LB>(typename LA::Params{W, ldw, wrows}, typename LB::Params{src, g, M, src_bytes}, ep,
                                   Mi, M, K, 1, st);
  }
}

// Small GEMMs of the head (F = T*B rows; answer MLP, LSTMCell, policy/value
// heads): 64x64 tiles leave most CUs idle, so below ~192 tiles use the 32x64
// tile with a 4-way in-WG split-K (8 waves per WG: the serial K loop of these
// long-K, few-tile GEMMs is what they wait on; C2 4.487 -> 4.414 ms per
// iteration vs the plain 32x64 tile, tools/ab_head.sh).  AAA_HEAD_TILE=1 forces
// 64x64, =2 the plain 32x64, =3/4/5 the 2-way / 4-way / 4-way BK128 split-K tiles.  (128x128 and 64x128
// tiles, fewer split fragments per MFMA, measured slower: C2 tail 190 -> 370 / 290 us, C3 367 -> 536 / 433.)
// g_tail3 (set per forward / backward call of the bf16 path, TailPrecision):
// the same tiles with fp32 operands split into bf16 pairs on the bf16 MFMA
// (gemm.h GemmCfgS3), ~1e-5 relative per product.
// g_tail6 (set per call of the fp32 path when f32_split6()): the three-way
// split at fp32 accuracy (gemm.h GemmCfgS6).
// g_tail_kind (set with them): the timer class (AAA_TIMER_TAIL_FWD / _BWD) whose variant records which
// kernel and arithmetic each tail GEMM of the call took (tail_ran); -1 outside a forward / backward call.
extern thread_local bool g_tail3, g_tail6;
extern thread_local int g_tail_kind;
struct TailPrecision {
  bool prev3, prev6;
  int prevk;
  explicit TailPrecision(bool split3, bool split6 = false, int kind = -1)
      : prev3(g_tail3), prev6(g_tail6), prevk(g_tail_kind) {
    g_tail3 = split3;
    g_tail6 = split6;
    g_tail_kind = kind;
  }
  ~TailPrecision() {
    g_tail3 = prev3;
    g_tail6 = prev6;
    g_tail_kind = prevk;
  }
};
// One tail GEMM launch for the timers (while enabled): ``kernel`` = skinny1 / skinny8 / CFK4 / CF, on the
// arithmetic of g_tail3 / g_tail6 (the skinny kernels: plain fp32 FMAs, none named), in ``slices`` K slices.
// aaa_timing_stats appends the launches to the class's variant in order, equal neighbours counted:
// "skinny8*15, CFK4/S6, CF/S3 x3" (x3: three split-K slices accumulating with atomics).
void tail_ran(const char* kernel, bool mfma, int slices = 1);
template <class C> struct S3Of { using type = GemmCfgS3<C::BI, C::BJ, C::BK, C::WI, C::WJ, C::WK>; };
template <class C> struct S6Of { using type = GemmCfgS6<C::BI, C::BJ, C::BK, C::WI, C::WJ, C::WK>; };

// The deep-pipeline (gemm_deep.h) form of a tail loader: LdRows -> LdRowsN, LdRowsT -> LdRowsTN.
template <template <typename, typename, int, int, int> class L> struct DeepLd;
template <> struct DeepLd<LdRows> {
  template <typename G, typename T, int R, int BK, int NT> using type = LdRowsN<G, T, R, BK, NT>;
  static bool fits(const void*, int ld, int nrows) { return ld % 4 == 0 && (size_t)nrows * ld * 4 < (1u << 31); }
};
template <> struct DeepLd<LdRowsT> {
  template <typename G, typename T, int R, int BK, int NT> using type = LdRowsTN<G, T, R, BK, NT>;
  static bool fits(const void*, int ld, int nrows) { return ld % 4 == 0 && nrows % 4 == 0; }
};
constexpr int kTailStages = 8;   // K tiles of global loads in flight per workgroup (gemm_kernel_deep)
#ifdef AAA_ABLATION
constexpr bool kAblationBuild = true;
#else
constexpr bool kAblationBuild = false;
#endif

// One operand of a tail GEMM: nrows rows of fp32 at pitch ld (all head_gemm / tail_gemm read of it).
struct Rows {
  const float* src;
  int ld;
  int nrows;
};

template <template <typename, typename, int, int, int> class LA_,
          template <typename, typename, int, int, int> class LB_, class EP>
static hipError_t head_gemm(const Rows& pa, const Rows& pb, const EP& ep, int Mi, int Nj, int K, int nsplit,
                            hipStream_t st) {
  const int mode = ab_int("AAA_HEAD_TILE", 0);
  const long tiles = (long)cdiv(Mi, 64) * cdiv(Nj, 64) * std::max(nsplit, 1);
  // ablation builds, AAA_TAIL_DEEP=1: kTailStages register stages of K tiles in flight (gemm_kernel_deep)
#ifdef AAA_ABLATION   // measured no faster (profiles/r06/ab/tail_deep/): ablation builds only
  const bool deep = ab_int("AAA_TAIL_DEEP", 0) && DeepLd<LA_>::fits(pa.src, pa.ld, pa.nrows) &&
                    DeepLd<LB_>::fits(pb.src, pb.ld, pb.nrows) && (size_t)K * pa.ld * 4 < (1u << 31) &&
                    (size_t)K * pb.ld * 4 < (1u << 31);
#else
  constexpr bool deep = false;
#endif
  auto run = [&](auto cfg) {
    using C = decltype(cfg);
    if constexpr (!kAblationBuild) {
      (void)deep;
    } else if (deep) {
      using A = typename DeepLd<LA_>::template type<float, float, C::BI, C::BK, C::NT>;
      using B = typename DeepLd<LB_>::template type<float, float, C::BJ, C::BK, C::NT>;
      return launch_gemm_deep<C, A, B, EP, kTailStages>(typename A::Params{pa.src, pa.ld, pa.nrows},
                                                        typename B::Params{pb.src, pb.ld, pb.nrows}, ep, Mi, Nj, K,
                                                        nsplit, st);
    }
    using A = LA_<float, float, C::BI, C::BK, C::NT>;
    using B = LB_<float, float, C::BJ, C::BK, C::NT>;
    return launch_gemm<C, A, B>(typename A::Params{pa.src, pa.ld, pa.nrows}, typename B::Params{pb.src, pb.ld, pb.nrows},
                                ep, Mi, Nj, K, nsplit, st);
  };
  auto splitk = [&](auto cfg0) {   // 32x64 tile, in-WG split-K over 2-4 waves (long K, few tiles)
    if (g_tail6) return run(typename S6Of<decltype(cfg0)>::type{});
    if (g_tail3) return run(typename S3Of<decltype(cfg0)>::type{});
    return run(cfg0);
  };
  if (mode == 0 && tiles < 192) {
    tail_ran("CFK4", true, splitk_slices(K, CFK4::BK, std::max(nsplit, 1)));
    return splitk(CFK4{});
  }
  // bf16 path, 64x64 tiles: the operands split once at their LDS commit (hi, lo part tiles, gemm_kernel_s6l),
  // not per wave per fragment read -- the same products in the same order (AAA_TAIL_S3L=1, ablation builds: A/B)
  if (mode == 0 && g_tail3 && ab_int("AAA_TAIL_S3L", 0) && DeepLd<LA_>::fits(pa.src, pa.ld, pa.nrows) &&
      DeepLd<LB_>::fits(pb.src, pb.ld, pb.nrows) && (size_t)K * pa.ld * 4 < (1u << 31) &&
      (size_t)K * pb.ld * 4 < (1u << 31)) {
    using C = GemmCfgS3L<64, 64, 32, 2, 2, 2>;
    using A = typename DeepLd<LA_>::template type<float, float, C::BI, C::BK, C::NT>;
    using B = typename DeepLd<LB_>::template type<float, float, C::BJ, C::BK, C::NT>;
    return launch_gemm<C, A, B>(typename A::Params{pa.src, pa.ld, pa.nrows}, typename B::Params{pb.src, pb.ld, pb.nrows},
                                ep, Mi, Nj, K, nsplit, st);
  }
  if (mode == 1 || (mode == 0 && tiles >= 192)) {
    tail_ran("CF", true, splitk_slices(K, CF::BK, std::max(nsplit, 1)));
    return splitk(CF{});
  }
#ifdef AAA_ABLATION   // the measured-slower tail tiles (AAA_HEAD_TILE 2-5)
  if (mode == 3) return splitk(CFK{});
  if (mode == 4) return splitk(CFK4{});
  if (mode == 5) return splitk(CFK4B{});
  if (g_tail3 || g_tail6) return splitk(CF32{});
  using C = CF32;
  using A = LA_<float, float, C::BI, C::BK, C::NT>;
  using B = LB_<float, float, C::BJ, C::BK, C::NT>;
  return launch_gemm<C, A, B>(typename A::Params{pa.src, pa.ld, pa.nrows}, typename B::Params{pb.src, pb.ld, pb.nrows}, ep,
                              Mi, Nj, K, nsplit, st);
#else
  return hipErrorInvalidValue;   // unreachable: mode is 0 outside ablation builds
#endif
}

// Tail GEMMs with very few columns (the actor's B=1, T=1 step: F = 1):
// D[i][j] = sum_k W[i][k] X[j][k], one wavefront per 4-row group, lanes split
// K in 16-B pieces (coalesced weight rows), butterfly reduction, then the same
// epilogue functor.  A 64x64 tile spends ~20 us on its serial K loop there;
// this reads the weight matrix once at full width.
constexpr int kSkinnyMaxCols = 8;
template <class EP, int NJ>
__global__ void __launch_bounds__(256)
k_skinny_gemm(const float* __restrict__ W, int ldw, int Mi, const float* __restrict__ X, int ldx, int Nj, int K,
              EP ep) {
  const int lane = threadIdx.x & 63;
  const int i = (blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 4;
  if (i >= Mi) return;
  float acc[4][NJ];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[r][j] = 0.f;
  for (int k = lane * 4; k < K; k += 256) {
    f32x4 w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      w[r] = i + r < Mi ? *reinterpret_cast<const f32x4*>(W + (size_t)(i + r) * ldw + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (j < Nj) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(X + (size_t)j * ldx + k);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r][j] += w[r][0] * x[0] + w[r][1] * x[1] + w[r][2] * x[2] + w[r][3] * x[3];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[r][j] += __shfl_xor(acc[r][j], o, 64);
  if (lane == 0)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (j < Nj) ep(i, j, acc[0][j], acc[1][j], acc[2][j], acc[3][j]);
}

// Forward tail GEMM (row-major weights [Mi][K] x activations [Nj][K]): the
// skinny kernel for <= kSkinnyMaxCols columns (AAA_SKINNY=0 disables), else head_gemm.
template <class EP>
static hipError_t tail_gemm(const Rows& pa, const Rows& pb, const EP& ep, int Mi, int Nj, int K, hipStream_t st) {
  if (Nj <= kSkinnyMaxCols && K % 4 == 0 && pa.ld % 4 == 0 && pb.ld % 4 == 0 && ab_int("AAA_SKINNY", 1)) {
    const int blocks = cdiv(cdiv(Mi, 4), 4);
    tail_ran(Nj == 1 ? "skinny1" : "skinny8", false);
    if (Nj == 1)
      hipLaunchKernelGGL((k_skinny_gemm<EP, 1>), dim3(blocks), dim3(256), 0, st, pa.src, pa.ld, Mi, pb.src, pb.ld, Nj,
                         K, ep);
    else
      hipLaunchKernelGGL((k_skinny_gemm<EP, kSkinnyMaxCols>), dim3(blocks), dim3(256), 0, st, pa.src, pa.ld, Mi,
                         pb.src, pb.ld, Nj, K, ep);
    return hipGetLastError();
  }
  return head_gemm<LdRows, LdRows>(pa, pb, ep, Mi, Nj, K, 1, st);
}

// Batched (off-chain) conv GEMMs on the LDS-DMA ring (env AAA_PIPE_BATCHED=0: register-staged).
static bool pipe_batched() { return env_int("AAA_PIPE_BATCHED", 1) != 0; }

static int wgrad_splits(int tiles, int K, int BK) {
  int s = std::max(1, 1024 / std::max(tiles, 1));
  int maxs = std::max(1, K / (8 * BK));
  return std::min(s, maxs);
}

// One fused ConvLSTM forward step (attention.py:110-126): D[512][M] = WpXH x
// im2col([x_t | h_{t-1}]) (K = 9*192), gate math and cell update in the
// epilogue ``ep``.  Tile: AAA_FUSED_TILE, default bf16 128x128 of 4 waves
// (64x64 per wave; tools/ab_fused.sh), fp32 (small M only, e.g. the B=1 actor
// and the standalone cell) 128x64 of 8 waves.
// zpart (fp32, B*P < 8192: Layout::dhs) enables the split-K tiles 17/18: K-slice
// partials of the gate pre-activations, then the cell in gate_fwd_zx.
static int fused_splitk() { return std::max(2, std::min(4, env_int("AAA_FUSED_SPLITK", 3))); }
// Ring depth of the split-K launches (2-4 stages: tiles in flight per workgroup; their few
// k-steps per slice are latency-bound, not MFMA-bound).  AAA_SPLITK_NBUF.
static int splitk_nbuf() { return std::max(2, std::min(4, ab_int("AAA_SPLITK_NBUF", 2))); }
template <class CK, class EP, typename T>
static hipError_t step_gemm_splitk(const T* W, int ldw, int wrows, const T* src, const ConvGeo& g, int M,
                                   uint32_t src_bytes, const EP& ep, int Mi, int K, hipStream_t st, int nsplit,
                                   bool ilv = false) {
  switch (splitk_nbuf() * 2 + (ilv ? 1 : 0)) {
    case 4: return step_gemm<CK, true, T, T, EP, 2, false>(W, ldw, wrows, src, g, M, src_bytes, ep, Mi, K, st, nsplit);
    case 5: return step_gemm<CK, true, T, T, EP, 2, true>(W, ldw, wrows, src, g, M, src_bytes, ep, Mi, K, st, nsplit);
    case 6: return step_gemm<CK, true, T, T, EP, 3, false>(W, ldw, wrows, src, g, M, src_bytes, ep, Mi, K, st, nsplit);
    case 7: return step_gemm<CK, true, T, T, EP, 3, true>(W, ldw, wrows, src, g, M, src_bytes, ep, Mi, K, st, nsplit);
    case 8: return step_gemm<CK, true, T, T, EP, 4, false>(W, ldw, wrows, src, g, M, src_bytes, ep, Mi, K, st, nsplit);
    default: return step_gemm<CK, true, T, T, EP, 4, true>(W, ldw, wrows, src, g, M, src_bytes, ep, Mi, K, st, nsplit);
  }
}
template <typename T, typename GT>
static int fused_step(const T* WpXH, const T* xht, int h, int w, int M, const EpiConvLstmFwd<T, GT>& ep,
                      hipStream_t st, float* zpart = nullptr, bool resets = false) {
  using EF = EpiConvLstmFwd<T, GT>;
  const ConvGeo g = ConvGeo{192, 192, 0, h, w, h, w, 3, 1, 1, 0}.prep();
  const uint32_t xh_bytes = (uint32_t)((size_t)M * 192 * sizeof(T));
  constexpr bool f32 = std::is_same<T, float>::value;
  // fp32 with f32_split6(): the split-product tiles 13-18 (bf16x6 on the bf16
  // MFMA): default 18 = 64x64 BK64 2-way in-WG split-K x 3 K slices + gate_fwd_zx
  // (B=1 episode step, 27x20 grid: 16.2 + 5.0 us vs 68 us for the fp32 128x64
  // tile, 23 us for 13 = 32x64 4-way in-WG; tools/gpu_episode_ab.sh), 13 where
  // there is no split-K scratch
  const int want = env_int("AAA_FUSED_TILE", f32 ? (f32_split6() ? (zpart ? 18 : 13) : 4) : 9);
  // as step_tile: another family's id runs tile 4, an id of no family is refused
  const int ftile = tile_dt(FusedTiles{}, want) ? want : 4;
  if (ftile != want && !tile_known(want)) return tile_unknown("AAA_FUSED_TILE");
  return for_tile<FusedTiles>(ftile, (int)AAA_E_ARG, [&](auto tile) -> int {
    using Tl = decltype(tile);
    using CK = typename Tl::template Cfg<T>;
    constexpr bool slices = Tl::split == SplitK::Slices;
    TimerScope tim(AAA_TIMER_FWD_STEP, st, 2.0 * M * 512 * 1728,
                   strf("%s fused [x|h] step, K=1728, AAA_FUSED_TILE %d%s [kernel: EpiConvLstmFwd]%s", f32 ? "fp32" : "bf16",
                        ftile, f32 && Tl::split_product && !slices ? " (bf16x6 split products)" : "",
                        resets ? ", resets" : ""));
    if constexpr (!Tl::template serves<T, GT>()) {
      return fail(AAA_E_ARG, "AAA_FUSED_TILE %d: fp32 split-product tiles only", ftile);
    } else if constexpr (slices) {   // K-slice partials of the gate pre-activations, then the cell
      if (!zpart || !ep.bias) return fail(AAA_E_ARG, "AAA_FUSED_TILE %d: split-K needs B*P < 8192 (got %d)", ftile, M);
      const int ns = splitk_slices(1728, CK::BK, fused_splitk());
      const EpiSliceT es{zpart, 512, 512, M, (size_t)M * 512};
      HIPCHK((step_gemm_splitk<CK>(WpXH, 1728, 512, xht, g, M, xh_bytes, es, 512, 1728, st, ns, Tl::ILV)));
      // (CK::type is T; spelled through the entry so that the call is only checked where the entry serves GT)
      HIPCHK(gate_fwd_zx<typename CK::type>(M, ep.cprev, ep.gates, ep.cnext, ep.hout, ep.xhnext, st, zpart, ns,
                                            (size_t)M * 512, ep.bias));
    } else {
      HIPCHK((step_gemm<CK, Tl::stage != Stage::Reg, T, T, EF, Tl::NBUF, Tl::ILV>(WpXH, 1728, 512, xht, g, M, xh_bytes, ep, 512,
                                                                                  1728, st)));
    }
    return AAA_OK;
  });
}

// ---------------------------------------------- frame-resident dispatch ----
int device_cus();   // CUs of the current device (which frame kernel runs, and the slices' layout: RecurPlan)
// h_t of all T*B frames as the attention readout reads it: the fp32 Hs slices
// (fp32 path), or the h half of XH slots 1..T (bf16 path: no fp32 copy of h_t
// is kept -- the readout reads the bf16 h the next step's conv and the weight
// gradient read, oracle/ref_cpu.py h_store).  Frame f = t*B + b sits at
// .frame(f, P) either way.
// Under an episode-start mask (bf16, AAA_FLAG_BF16_RESETS) XH's h half holds zeros in the rows that start an
// episode, so the masked forward keeps every h_t in HR as well and the readout of a masked call reads it there.
inline OSrc readout_h(const Layout& L, char* ws, bool masked) {
  if (L.esz == 2 && masked) return o_bf16((const __bf16*)(ws + L.HR), 128);
  if (L.esz == 2) return o_bf16((const __bf16*)(ws + L.XH) + (size_t)L.B * L.P * 192 + 64, 192);
  return o_f32((const float*)(ws + L.Hs));
}
int rec_stagger(const char* env);   // start offset of half the frames, 100-MHz ticks

// ------------------------------------------------------- cross-unit paths --
// What the phases of one forward / backward call share: the layout, the call's buffers, the caller's stream, (fp32)
// the episode-start mask (T, B) or null, the recurrence's plan, and for the call's duration the tail GEMMs' arithmetic
// (bf16 path: split operands on the bf16 MFMA, AAA_TAIL_SPLIT3=0: the fp32 MFMA) under the timer class tail_kind.
struct CallCtx {
  const Layout& L;
  const aaa_io* io;
  char* ws;
  const char* pk;
  const float* prm;
  float* grads;   // (the backward's)
  hipStream_t st;
  const float* reset;
  RecurPlan plan;
  TailPrecision tail;
  CallCtx(const Layout& l, const aaa_io* i, hipStream_t s, const float* r, int tail_kind)
      : L(l), io(i), ws((char*)i->workspace), pk((const char*)i->packed), prm(i->params), grads(i->grads), st(s),
        reset(r), plan(recur_plan(l, r != nullptr)),
        tail(l.dt == AAA_BF16 && env_int("AAA_TAIL_SPLIT3", 1), l.dt == AAA_F32 && f32_split6(), tail_kind) {}
  float* Wf(size_t off) const { return (float*)(ws + off); }
  template <typename T> T* Wt(size_t off) const { return (T*)(ws + off); }
};
template <typename T> int pack_impl(const Layout& L, const float* prm, char* pk, hipStream_t st);
template <typename T, typename OT>
int vision_fwd(const Layout& L, int F, const char* pk, const float* prm, const void* frames, T* Xp, T* Y1, OT* out,
               int out_ld, hipStream_t st, bool xp_full = true, std::string* ran = nullptr,   // ran <- the kernels taken
               bool resident_xp = true);   // false: a frame-resident kernel stores no Xp (the learner; ran says "no Xp")
// reset: the episode-start mask (T, B) of aaa_forward_resets / aaa_backward_resets, or null
template <typename T>
int forward_impl(const Layout& L, const aaa_io* io, hipStream_t st, int phases, const float* reset = nullptr);
template <typename T>
int lstm_wgrad(const T* dz, const T* xh, int rows, int h, int w, float* gW, hipStream_t s, bool aux);
template <typename T>
int vision_bwd(const Layout& L, const char* pk, const T* dy2, const T* y1, T* xp, T* dy1, int F, float* gW2,
               float* gW1, float* gb1, hipStream_t s, const void* frames = nullptr);
// backward_impl's VISION phase on its own (rt_backward.hip), shared with aaa_vision_enc_bwd
const char* vision_bwd_variant(bool fused, bool f32 = false, bool unpack = true);   // the timer's variant string
template <typename T>
int vision_bwd_alone(const Layout& L, const char* pk, const void* frames, const T* dy2, const T* y1, T* xp, T* dy1,
                     void* part, size_t part_bytes, int F, float* gW2, float* gW1, float* gb1, hipStream_t st,
                     const void* xp_frames, bool* fused, int max_groups = 0, float* dy1_out = nullptr,
                     const void* wdt2s = nullptr);
template <typename T>
int backward_impl(const Layout& L, const aaa_io* io, int phases, hipStream_t st, const float* reset = nullptr);

}  // namespace aaa
