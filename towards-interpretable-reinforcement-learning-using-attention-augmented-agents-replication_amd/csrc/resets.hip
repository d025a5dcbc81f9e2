// Episode-start masks inside an unroll (aaa_forward_resets / aaa_backward_resets,
// the per-step paths of both operand types and the stateful tail; the frame kernels
// apply the mask themselves, recur_f32.h / recur_bwd_f32.h / recur.h RST): reset[t][b] != 0 means row b enters step t from the
// reset() state (attention.py:142-149; the reference calls agent.reset() at every
// episode start, main_mp.py:100).
//
// A reset is a SELECT: nothing of the state before it -- NaN and inf included --
// reaches anything after it.  The step GEMMs stay the kernels they are; the mask is
// applied to their PRIVATE operands and carries by the small kernels here:
//   forward   k_reset_rows, before step t: zeros in the h half of XH slot t (the
//             operand of the h-part and of the weight gradient) and a masked copy of
//             c_{t-1} for the cell update.  The dual-use slots (Cst slot t, CH / CC
//             slot t) keep the true outputs of step t-1: its own backward reads them.
//   backward  k_reset_gate_bwd, after the fused dgrad + gate backward of step t-1:
//             the rows of frames with reset[t] are recomputed from dh = dO alone and a
//             zero dc carry (what the step kernel wrote there is overwritten, never
//             scaled), and d f-gate of frames with reset[t-1] is stored as 0 (c_{t-2}
//             read as 0); k_reset_rows zeroes the state cotangents' rows.
#include "misc.h"

namespace aaa {

// Rows [b*rpb, (b+1)*rpb) belong to frame b.  For every row: dst[row][c] = rs[b] ? 0 : src[row][c]
// (c < cw; dst null: none); for the rows of frames with rs[b] != 0: the zero ranges.
template <typename TE>
__global__ void __launch_bounds__(256)
k_reset_rows(const float* __restrict__ rs, int B, int rpb, ResetZerosT<TE> z, const float* __restrict__ src,
             float* __restrict__ dst, int cw, int wmax) {
  const long n = (long)B * rpb * wmax;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / wmax;
    const int c = (int)(i - row * wmax);
    const bool r = rs[row / rpb] != 0.f;
    if (dst && c < cw) dst[row * cw + c] = r ? 0.f : src[row * cw + c];
    if (!r) continue;
    for (int k = 0; k < z.n; ++k)
      if (c < z.r[k].w) z.r[k].p[row * z.r[k].ld + (long)c * z.r[k].es] = (TE)0.f;
  }
}

template <typename TE>
hipError_t reset_rows(const float* rs, int B, int rpb, const ResetZerosT<TE>& z, const float* src, float* dst, int cw,
                      hipStream_t st) {
  int wmax = dst ? cw : 0;
  for (int k = 0; k < z.n; ++k) wmax = wmax > z.r[k].w ? wmax : z.r[k].w;
  if (wmax <= 0 || B <= 0 || rpb <= 0) return hipSuccess;
  const long n = (long)B * rpb * wmax;
  const int blocks = (int)(n + 255 < 2048L * 256 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_reset_rows<TE>, dim3(blocks), dim3(256), 0, st, rs, B, rpb, z, src, dst, cw, wmax);
  return hipGetLastError();
}
template hipError_t reset_rows<float>(const float*, int, int, const ResetZerosT<float>&, const float*, float*, int,
                                      hipStream_t);
template hipError_t reset_rows<__bf16>(const float*, int, int, const ResetZerosT<__bf16>&, const float*, float*, int,
                                       hipStream_t);

// Gate backward of step t-1 over M = B*P pixels, after the step kernel's own:
//   frames with rs_in[b] (= reset[t][b]):  dh = dO alone, dc carry in = 0 -> dz, dC rewritten
//   frames with rs_c[b] (= reset[t-1][b]): c_{t-2} read as 0 -> d f-gate = 0
// rs_in null: the last step (nothing flows in from t either way), only the f-gate store.
__global__ void __launch_bounds__(256)
k_reset_gate_bwd(const float* __restrict__ rs_in, const float* __restrict__ rs_c, int M, int P,
                 const float* __restrict__ dO, const float* __restrict__ gates, const float* __restrict__ cprev,
                 const float* __restrict__ ccur, float* dC, float* dz) {
  const long n = (long)M * 128;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const int m = (int)(idx >> 7), ch = (int)(idx & 127), b = m / P;
    const bool rin = rs_in && rs_in[b] != 0.f, rc = rs_c && rs_c[b] != 0.f;
    if (rin) {
      const f32x4 g = load_gates(gates + (size_t)m * 512 + 4 * ch);
      float dc = 0.f, di, df, dcg, dout;
      gate_bwd(dO[idx], g, rc ? 0.f : cprev[idx], ccur[idx], dc, di, df, dcg, dout);
      dC[idx] = dc;
      store4(dz + (size_t)m * 512 + 4 * ch, di, rc ? 0.f : df, dcg, dout);
    } else if (rc) {
      dz[(size_t)m * 512 + 4 * ch + 1] = 0.f;
    }
  }
}

hipError_t reset_gate_bwd(const float* rs_in, const float* rs_c, int M, int P, const float* dO, const float* gates,
                          const float* cprev, const float* ccur, float* dC, float* dz, hipStream_t st) {
  const long n = (long)M * 128;
  const int blocks = (int)(n + 255 < 2048L * 256 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_reset_gate_bwd, dim3(blocks), dim3(256), 0, st, rs_in, rs_c, M, P, dO, gates, cprev, ccur, dC,
                     dz);
  return hipGetLastError();
}

// bf16: the whole gate backward of step t-1 under a mask, instead of the step GEMM's fused one plus the rewrite
// above -- dZ is rounded to bf16 there, so a gate-bias gradient summed from the final dZ would carry that
// rounding (measured 6e-4 to 9e-4 norm-relative against the unmasked kernels' fp32 partials).  The step GEMM
// stores the raw dgrad dh (its t = 0 form), and this kernel, shaped as k_gate_bwd_last (one workgroup per tile
// of ``bj`` pixels, fp32 gate-bias partials per tile), applies the mask as selects:
//   frames with rs_in[b] (= reset[t][b]):  dh = dO alone, dc carry in = 0
//   frames with rs_c[b] (= reset[t-1][b]): c_{t-2} read as 0, d f-gate = 0
// dh: the raw dgrad (or the caller's dhT for the last step), or null.  With an all-zero mask it computes what the
// fused epilogue computes: dO + dh in fp32, the same gate_bwd, the same rounding of dZ.
template <typename TZ, typename GT>
__global__ void __launch_bounds__(512)
k_gate_bwd_resets(int M, int bj, int P, const float* __restrict__ rs_in, const float* __restrict__ rs_c,
                  const float* __restrict__ dO, const float* __restrict__ dh, const GT* __restrict__ gates,
                  const float* __restrict__ cprev, const float* __restrict__ ccur, float* dC, TZ* dz, float* part) {
  __shared__ f32x4 red[4][128];
  const int ch = threadIdx.x & 127, sl = threadIdx.x >> 7;
  const int m0 = blockIdx.x * bj, m1 = min(M, m0 + bj);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int m = m0 + sl; m < m1; m += 4) {
    const size_t idx = (size_t)m * 128 + ch;
    const int b = m / P;
    const bool rin = rs_in && rs_in[b] != 0.f, rc = rs_c[b] != 0.f;
    float dhv = dO[idx];
    if (dh && !rin) dhv += dh[idx];
    const f32x4 g = load_gates(gates + (size_t)m * 512 + 4 * ch);
    float dc = rin ? 0.f : dC[idx], di, df, dcg, dout;
    gate_bwd(dhv, g, rc ? 0.f : cprev[idx], ccur[idx], dc, di, df, dcg, dout);
    if (rc) df = 0.f;
    dC[idx] = dc;
    store4(dz + (size_t)m * 512 + 4 * ch, di, df, dcg, dout);
    acc[0] += di; acc[1] += df; acc[2] += dcg; acc[3] += dout;
  }
  if (!part) return;
  red[sl][ch] = acc;
  __syncthreads();
  if (sl == 0) {
    f32x4 t = red[0][ch];
#pragma unroll
    for (int k = 1; k < 4; ++k) { t[0] += red[k][ch][0]; t[1] += red[k][ch][1]; t[2] += red[k][ch][2]; t[3] += red[k][ch][3]; }
    *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * 512 + 4 * ch) = t;
  }
}

template <typename TZ, typename GT>
hipError_t gate_bwd_resets(int M, int bj, int P, const float* rs_in, const float* rs_c, const float* dO, const float* dh,
                           const GT* gates, const float* cprev, const float* ccur, float* dC, TZ* dz, float* part,
                           hipStream_t st) {
  if (M <= 0 || bj <= 0 || P <= 0 || !rs_c) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_gate_bwd_resets<TZ, GT>), dim3((M + bj - 1) / bj), dim3(512), 0, st, M, bj, P, rs_in, rs_c, dO, dh,
                     gates, cprev, ccur, dC, dz, part);
  return hipGetLastError();
}
template hipError_t gate_bwd_resets<__bf16, float>(int, int, int, const float*, const float*, const float*, const float*,
                                                   const float*, const float*, const float*, float*, __bf16*, float*,
                                                   hipStream_t);
template hipError_t gate_bwd_resets<__bf16, _Float16>(int, int, int, const float*, const float*, const float*,
                                                      const float*, const _Float16*, const float*, const float*, float*,
                                                      __bf16*, float*, hipStream_t);

// 16 B (8 channels) per thread: row r's h half xh[r][64..192) -> hr[r][0..128)
__global__ void __launch_bounds__(256) k_xh_to_hr(long rows, const __bf16* __restrict__ xh, __bf16* __restrict__ hr) {
  const long n = rows * 16;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i >> 4;
    const int q = (int)(i & 15);
    *reinterpret_cast<u32x4*>(hr + r * 128 + q * 8) = *reinterpret_cast<const u32x4*>(xh + r * 192 + 64 + q * 8);
  }
}

hipError_t xh_to_hr(long rows, const __bf16* xh, __bf16* hr, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  const long n = rows * 16;
  const int blocks = (int)(n + 255 < 2048L * 256 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_xh_to_hr, dim3(blocks), dim3(256), 0, st, rows, xh, hr);
  return hipGetLastError();
}

}  // namespace aaa
