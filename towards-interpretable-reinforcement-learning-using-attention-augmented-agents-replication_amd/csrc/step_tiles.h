// The tile ids of the per-step ConvLSTM kernels: one table per family (AAA_STEP_TILE,
// AAA_BPTT_TILE, AAA_FUSED_TILE), one line per id with everything the runtime knows
// about it; rt.h, rt_forward.hip and rt_backward.hip derive the rest through for_tile.
#pragma once
#include <type_traits>

#include "gemm.h"

namespace aaa {

// --------------------------------------------------------- tile configs ---
// fp32 uses the exact v_mfma_f32_32x32x2_f32; bf16 v_mfma_f32_32x32x16_bf16 (fp32 accumulate).
using CF = GemmCfg<float, 64, 64, 32, 2, 2>;      // default 64x64 tile, 4 waves
using CF32 = GemmCfg<float, 32, 64, 32, 1, 2>;    // 32-row tile, 2 waves: small-Mi GEMMs / more WGs
using CFW = GemmCfg<float, 128, 128, 32, 2, 2>;   // long-K weight gradients: 64x64 per wave
using CFK = GemmCfg<float, 32, 64, 64, 1, 2, 2>;  // per-step ConvLSTM kernels: 2-way split-K in the WG
using CFK4 = GemmCfg<float, 32, 64, 64, 1, 2, 4>; // 4-way split-K (8 waves)
using CFK4B = GemmCfg<float, 32, 64, 128, 1, 2, 4>; // 4-way split-K, 2 k-steps per wave per barrier
using CF64 = GemmCfg<float, 64, 64, 64, 2, 2>;     // 64x64, BK 64
using CFJ = GemmCfg<float, 64, 128, 32, 2, 2>;     // 64-row GEMMs with long N (batched dx)
using CFS = GemmCfg<float, 128, 64, 32, 4, 2>;     // forward step: 8 waves, ~1 WG per CU at C2 (balanced)
using CB = GemmCfg<__bf16, 64, 64, 64, 2, 2>;
using CB32 = GemmCfg<__bf16, 32, 64, 64, 1, 2>;
using CBW = GemmCfg<__bf16, 128, 128, 64, 2, 2>;
using CBK = GemmCfg<__bf16, 32, 64, 64, 1, 2, 2>;
using CBK4 = GemmCfg<__bf16, 32, 64, 64, 1, 2, 4>;
using CBK4B = GemmCfg<__bf16, 32, 64, 128, 1, 2, 4>;
using CB64 = GemmCfg<__bf16, 64, 64, 128, 2, 2>;
using CBJ = GemmCfg<__bf16, 64, 128, 64, 2, 2>;
using CBS = GemmCfg<__bf16, 128, 64, 64, 4, 2>;
template <typename T> using CfgFor = std::conditional_t<std::is_same<T, float>::value, CF, CB>;
template <typename T> using Cfg32For = std::conditional_t<std::is_same<T, float>::value, CF32, CB32>;
template <typename T> using CfgWFor = std::conditional_t<std::is_same<T, float>::value, CFW, CBW>;
template <typename T> using CfgKFor = std::conditional_t<std::is_same<T, float>::value, CFK, CBK>;
template <typename T> using CfgK4For = std::conditional_t<std::is_same<T, float>::value, CFK4, CBK4>;
template <typename T> using CfgK4BFor = std::conditional_t<std::is_same<T, float>::value, CFK4B, CBK4B>;
template <typename T> using Cfg64For = std::conditional_t<std::is_same<T, float>::value, CF64, CB64>;
template <typename T> using CfgJFor = std::conditional_t<std::is_same<T, float>::value, CFJ, CBJ>;
template <typename T> using CfgSFor = std::conditional_t<std::is_same<T, float>::value, CFS, CBS>;

// Whether the LDS-DMA ring can run tile config CK (every wave issues the same DMA count).
template <class CK>
constexpr bool pipe_even() {
  constexpr int VG = 16 / (int)sizeof(typename CK::type);
  return (CK::BI * CK::BK / VG) % CK::NT == 0 && (CK::BJ * CK::BK / VG) % CK::NT == 0;
}

// ------------------------------------------------------------ one entry ---
// The GEMM config of an entry, as a function of the operand type T:
template <template <typename> class A> struct Of {   // one of the Cfg*For pairs above
  template <typename T> using Cfg = A<T>;
  static constexpr bool split_product = false;
};
template <int BI, int BJ, int BK, int WI, int WJ, int WK = 1> struct Nat {   // the same shape on T's own MFMA
  template <typename T> using Cfg = GemmCfg<T, BI, BJ, BK, WI, WJ, WK>;
  static constexpr bool split_product = false;
};
template <int BI, int BJ, int BK, int WI, int WJ, int WK = 1> struct S6 {   // fp32 as bf16x6 split products (gemm.h SPLIT6)
  template <typename> using Cfg = GemmCfgS6<BI, BJ, BK, WI, WJ, WK>;
  static constexpr bool split_product = true;
};

// Staging of the operands.  Ring: the LDS-DMA ring of glds.h where the shape is ring-even for the
// operand type (pipe_even), else step_gemm's register-staged kernel -- which writes no gate-bias
// partials: ask pipe<T>(), never the id.  RingOnly: ring-even for every type served, checked here.
enum class Stage { Reg, Ring, RingOnly };
// K slices over several workgroups (step_gemm_splitk: ring depth AAA_SPLITK_NBUF's, kNbufEnv; ILV its ilv
// argument).  Slices: partials summed by the gate kernel that follows (gate_bwd_last / gate_fwd_zx);
// SliceFix: by each tile's last-arriving slice inside the GEMM (EpiSliceFix).
enum class SplitK { None, Slices, SliceFix };
constexpr int kNbufEnv = 0;
constexpr unsigned kF32 = 1, kBf16 = 2, kAnyT = kF32 | kBf16;   // operand types an entry serves
constexpr unsigned kG32 = 1, kG16 = 2, kAnyG = kG32 | kG16;     // gate storage types it serves

template <int ID, class SHAPE, Stage STAGE, int NBUF_, bool ILV_, unsigned DT, unsigned GATES, SplitK SPLIT = SplitK::None,
          int DH0 = ID>
struct StepTile {
  static constexpr int id = ID, NBUF = NBUF_, dh0 = DH0;   // dh0 (BPTT): the entry that runs t = 0 (dh0), where a split-K chain has no gate backward to feed
  static constexpr bool ILV = ILV_;
  static constexpr Stage stage = STAGE;
  static constexpr unsigned dt = DT, gates = GATES;
  static constexpr SplitK split = SPLIT;
  template <typename T> using Cfg = typename SHAPE::template Cfg<T>;
  static constexpr bool split_product = SHAPE::split_product;
  template <typename T> static constexpr bool pipe() { return STAGE != Stage::Reg && pipe_even<Cfg<T>>(); }
  // whether the kernel of this entry exists for operands T with gate storage GT
  template <typename T, typename GT = float> static constexpr bool serves() {
    return (DT & (std::is_same<T, float>::value ? kF32 : kBf16)) && (GATES & (std::is_same<GT, float>::value ? kG32 : kG16));
  }
  static_assert(STAGE != Stage::RingOnly || ((!(DT & kF32) || pipe_even<Cfg<float>>()) && (!(DT & kBf16) || pipe_even<Cfg<__bf16>>())),
                "a ring-only tile whose shape the LDS-DMA ring cannot run");
  static_assert((SPLIT == SplitK::None) == (NBUF_ != kNbufEnv) && (SPLIT == SplitK::None || STAGE == Stage::RingOnly),
                "split-K launches are ring-only, at AAA_SPLITK_NBUF's depth");
};

template <class... Ts> struct TileList {};

// ----------------------------------------------------------- the tables ---
// AAA_STEP_TILE: the forward h-part, D[512][M] = WpH x im2col(h_{t-1}), K = 1152 (EpiConvLstmFwd)
using FwdTiles = TileList<
    //   id  config                          staging      NBUF ILV   operands gates
    StepTile< 0, Of<CfgFor>,                     Stage::Reg,  2, false, kAnyT, kG32>,   // 64x64 BK32 (bf16: BK64)
    StepTile< 1, Of<CfgKFor>,                    Stage::Reg,  2, false, kAnyT, kG32>,   // 32x64 BK64, 2-way in-WG split-K
    StepTile< 2, Of<CfgKFor>,                    Stage::Reg,  2, false, kAnyT, kG32>,   // the same kernel as 1
    StepTile< 3, Of<Cfg64For>,                   Stage::Reg,  2, false, kAnyT, kG32>,   // 64x64 BK64
    StepTile< 4, Of<CfgSFor>,                    Stage::Ring, 2, false, kAnyT, kG32>,   // 128x64, 8 waves
    StepTile< 5, Of<CfgKFor>,                    Stage::Ring, 2, false, kAnyT, kG32>,   // 32x64 BK64, 2-way in-WG split-K
    StepTile< 6, Of<Cfg64For>,                   Stage::Ring, 2, false, kAnyT, kG32>,   // 64x64 BK64
    StepTile<12, Of<CfgKFor>,                    Stage::Ring, 3, true,  kAnyT, kG32>,   // 32x64 BK64, 2-way in-WG split-K, 3-stage ring
    StepTile<14, Nat<32, 32, 64, 1, 1, 4>,       Stage::Ring, 3, true,  kAnyT, kG32>,   // 32x32 BK64, 4-way in-WG split-K, 3-stage ring
    StepTile<17, Nat<64, 32, 64, 2, 1, 2>,       Stage::Ring, 3, true,  kAnyT, kG32>,   // 64x32 BK64, 2-way in-WG split-K, 3-stage ring
    StepTile<18, Of<Cfg64For>,                   Stage::Ring, 3, true,  kAnyT, kG32>,   // 64x64 BK64, 2x2 waves, 3-stage ring
    StepTile<25, Nat<64, 64, 64, 2, 2, 2>,       Stage::Ring, 2, false, kAnyT, kG32>,   // 64x64 BK64, 2-way in-WG split-K (8 waves), 2-stage ring
    StepTile<26, Nat<64, 64, 128, 2, 2, 2>,      Stage::Ring, 2, false, kAnyT, kG32>>;  // 64x64 BK128, 2-way in-WG split-K (8 waves), 2-stage ring

// AAA_BPTT_TILE: the dh dgrad, D[128][M] = WdTh x im2col(dZ_t), K = 4608, with the gate backward of step t-1 in
// its epilogue (EpiConvLstmBwd).  Gate-bias partials per (step, BJ pixels) come from the ring kernels only.
using BpttTiles = TileList<
    //   id  config                          staging          NBUF ILV   operands gates  [split-K, dh0 entry]
    StepTile< 0, Of<CfgFor>,                     Stage::Reg,      2, false, kAnyT, kG32>,   // 64x64 BK32 (bf16: BK64)
    StepTile< 1, Of<CfgKFor>,                    Stage::Reg,      2, false, kAnyT, kG32>,   // 32x64 BK64, 2-way in-WG split-K
    StepTile< 2, Of<CfgK4For>,                   Stage::Reg,      2, false, kAnyT, kG32>,   // 32x64 BK64, 4-way
    StepTile< 3, Of<CfgK4BFor>,                  Stage::Reg,      2, false, kAnyT, kG32>,   // 32x64 BK128, 4-way
    // 3-stage ring, DMA interleaved with the MFMAs (tools/ubench/step_ablate: 57.9 vs 59.4 us)
    StepTile< 4, Of<CfgK4BFor>,                  Stage::Ring,     3, true,  kAnyT, kG32>,   // 32x64 BK128, 4-way
    StepTile< 5, Of<CfgK4For>,                   Stage::Ring,     2, false, kAnyT, kG32>,   // 32x64 BK64, 4-way
    StepTile< 6, Of<CfgFor>,                     Stage::Ring,     2, false, kAnyT, kG32>,   // 64x64
    StepTile< 7, Nat<128, 128, 128, 2, 2, 2>,    Stage::RingOnly, 2, false, kBf16, kAnyG>,  // bf16: 128x128, BK128, 2-way in-WG split-K (tools/ubench/bf16_tiles: 48 vs 53-60 us at C3)
    StepTile< 8, Nat<128, 64, 128, 2, 1, 2>,     Stage::RingOnly, 2, false, kBf16, kAnyG>,  // bf16: 128x64, BK128, 2-way in-WG split-K, 4 waves (small batches)
    StepTile< 9, Nat<64, 32, 128, 2, 1, 4>,      Stage::Ring,     3, true,  kAnyT, kG32>,   // 64x32, BK128, 4-way in-WG split-K, 3-stage ring, interleaved DMA
    StepTile<10, Nat<32, 32, 128, 1, 1, 4>,      Stage::Ring,     2, true,  kAnyT, kG32>,   // 32x32, BK128, 4-way in-WG split-K, 2-stage ring (2 WGs per CU, desynchronised barriers)
    StepTile<11, Nat<32, 32, 64, 1, 1, 4>,       Stage::Ring,     3, true,  kAnyT, kG32>,   // 32x32, BK64, 4-way in-WG split-K, 3-stage ring
    StepTile<12, Nat<32, 32, 64, 1, 1, 4>,       Stage::Ring,     4, true,  kAnyT, kG32>,   // 32x32, BK64, 4-way in-WG split-K, 4-stage ring
    StepTile<13, Nat<32, 32, 128, 1, 1, 8>,      Stage::Ring,     2, true,  kAnyT, kG32>,   // 32x32, BK128, 8-way in-WG split-K (8 waves), 2-stage ring
    StepTile<15, Nat<64, 32, 64, 2, 1, 4>,       Stage::Ring,     3, true,  kAnyT, kG32>,   // 64x32, BK64, 4-way in-WG split-K, 3-stage ring
    StepTile<16, Nat<32, 32, 64, 1, 1, 4>,       Stage::Ring,     3, false, kAnyT, kG32>,   // 32x32, BK64, 4-way in-WG split-K, 3-stage ring, DMA issued before the MFMAs
    // 19-24: bf16 with fp16 gate storage (22 with fp32 gates too: the default small-batch tile under
    // AAA_FUSED_X=0 / AAA_GATES_F16=0)
    StepTile<19, Nat<128, 128, 64, 2, 2>,        Stage::RingOnly, 2, false, kBf16, kG16>,   // 128x128, 4 waves of 64x64, BK64
    StepTile<20, Nat<128, 128, 64, 2, 2>,        Stage::RingOnly, 3, true,  kBf16, kG16>,   // the same on a 3-stage ring
    StepTile<21, Nat<128, 64, 64, 2, 2>,         Stage::RingOnly, 2, false, kBf16, kG16>,   // 128x64, 4 waves of 64x32, BK64
    StepTile<22, Nat<128, 64, 128, 2, 1, 4>,     Stage::RingOnly, 2, false, kBf16, kAnyG>,  // 128x64, BK128, 4-way in-WG split-K (8 waves)
    StepTile<23, Nat<64, 64, 128, 2, 2, 2>,      Stage::RingOnly, 2, false, kBf16, kG16>,   // 64x64, BK128, 2-way in-WG split-K (8 waves)
    StepTile<24, Nat<64, 32, 128, 2, 1, 4>,      Stage::RingOnly, 2, false, kBf16, kG16>,   // 64x32, BK128, 4-way in-WG split-K (8 waves)
    // 27-33: fp32 as bf16x6 split products on the small-batch shapes
    StepTile<27, S6<32, 32, 64, 1, 1, 4>,        Stage::RingOnly, 3, false, kF32,  kG32>,   // tile 16's shape
    StepTile<28, S6<32, 32, 128, 1, 1, 8>,       Stage::RingOnly, 2, true,  kF32,  kG32>,   // 32x32, BK128, 8-way in-WG split-K (8 waves), 2-stage ring
    StepTile<29, S6<64, 32, 128, 2, 1, 4>,       Stage::RingOnly, 3, true,  kF32,  kG32>,   // 64x32, BK128, 4-way in-WG split-K, 3-stage ring
    // split-K over workgroups; t = 0 (dh0) takes tile 27
    StepTile<30, S6<32, 32, 64, 1, 1, 4>,        Stage::RingOnly, kNbufEnv, false, kF32, kG32, SplitK::Slices, 27>,    // tile 27's shape
    StepTile<31, S6<32, 32, 128, 1, 1, 8>,       Stage::RingOnly, kNbufEnv, true,  kF32, kG32, SplitK::Slices, 27>,    // tile 28's shape (interleaved DMA)
    StepTile<32, S6<32, 32, 64, 1, 1, 4>,        Stage::RingOnly, kNbufEnv, false, kF32, kG32, SplitK::SliceFix, 27>,  // 30 with the sum inside the GEMM
    StepTile<33, S6<32, 32, 128, 1, 1, 8>,       Stage::RingOnly, kNbufEnv, true,  kF32, kG32, SplitK::SliceFix, 27>>; // 31 with the sum inside the GEMM

// AAA_FUSED_TILE: the fused forward step, D[512][M] = WpXH x im2col([x_t | h_{t-1}]), K = 1728 (EpiConvLstmFwd)
using FusedTiles = TileList<
    //   id  config                          staging          NBUF ILV   operands gates  [split-K]
    StepTile< 4, Of<CfgSFor>,                    Stage::Ring,     2, false, kAnyT, kAnyG>,   // 128x64, 8 waves
    StepTile< 7, Of<CfgFor>,                     Stage::Ring,     2, false, kAnyT, kAnyG>,   // 64x64
    StepTile< 8, Of<CfgSFor>,                    Stage::Ring,     3, true,  kAnyT, kAnyG>,   // 128x64, 8 waves, 3-stage ring
    StepTile< 9, Nat<128, 128, 64, 2, 2>,        Stage::Ring,     2, false, kAnyT, kAnyG>,   // 128x128, 4 waves of 64x64
    StepTile<10, Of<CfgFor>,                     Stage::Ring,     3, true,  kAnyT, kAnyG>,   // 64x64, 4 waves, 3-stage ring
    StepTile<11, Nat<64, 64, 64, 2, 2, 2>,       Stage::Ring,     2, false, kAnyT, kAnyG>,   // 64x64, 2-way in-WG split-K (8 waves), BK64 (K = 1728 = 27 x 64)
    StepTile<12, Nat<128, 64, 64, 2, 2>,         Stage::Ring,     2, false, kAnyT, kAnyG>,   // 128x64, 2x2 waves of 64x32
    // 13-18: fp32 as bf16x6 split products
    StepTile<13, S6<32, 64, 64, 1, 2, 4>,        Stage::Ring,     2, false, kF32,  kAnyG>,   // 32x64 BK64, 4-way in-WG split-K
    StepTile<14, S6<64, 64, 64, 2, 2, 2>,        Stage::Ring,     2, false, kF32,  kAnyG>,   // 64x64 BK64, 2-way in-WG split-K
    StepTile<15, S6<128, 64, 32, 4, 2>,          Stage::Ring,     2, false, kF32,  kAnyG>,   // 128x64, 8 waves
    StepTile<16, S6<32, 32, 64, 1, 1, 4>,        Stage::Ring,     3, false, kF32,  kAnyG>,   // 32x32 BK64, 4-way in-WG split-K, 3-stage ring
    StepTile<17, S6<32, 64, 64, 1, 2, 4>,        Stage::RingOnly, kNbufEnv, false, kF32, kG32, SplitK::Slices>,    // 13 split over K slices + gate_fwd_zx
    StepTile<18, S6<64, 64, 64, 2, 2, 2>,        Stage::RingOnly, kNbufEnv, false, kF32, kG32, SplitK::Slices>>;   // 14 split over K slices + gate_fwd_zx

// --------------------------------------------------------------- lookup ---
// f(tile) for the entry of Family whose id is ``id`` (tile: a value of the entry's type); ``miss`` if there is none.
template <class R, class F, class... Ts>
inline R for_tile_in(TileList<Ts...>, int id, R r, F&& f) {
  (void)((id == Ts::id && ((r = f(Ts{})), true)) || ...);
  return r;
}
template <class Family, class R, class F> inline R for_tile(int id, R miss, F&& f) { return for_tile_in(Family{}, id, miss, f); }

// The entry's operand-type and gate-type masks (0: the family has no such id).
template <class... Ts> constexpr unsigned tile_dt(TileList<Ts...>, int id) { return ((id == Ts::id ? Ts::dt : 0u) | ...); }
template <class... Ts> constexpr unsigned tile_gates(TileList<Ts...>, int id) { return ((id == Ts::id ? Ts::gates : 0u) | ...); }
constexpr bool tile_known(int id) {   // in any family
  return tile_dt(FwdTiles{}, id) || tile_dt(BpttTiles{}, id) || tile_dt(FusedTiles{}, id);
}

template <class... Ts> constexpr int tile_count(TileList<Ts...>, int id) { return ((id == Ts::id ? 1 : 0) + ...); }
template <class... Ts> constexpr bool tile_ids_unique(TileList<Ts...> l) { return ((tile_count(l, Ts::id) == 1) && ...); }
static_assert(tile_ids_unique(FwdTiles{}) && tile_ids_unique(BpttTiles{}) && tile_ids_unique(FusedTiles{}),
              "a tile id twice in one family");

}  // namespace aaa
