// Episode-start masks inside an unroll (aaa_forward_resets / aaa_backward_resets,
// fp32 per-step paths and the stateful tail; the frame-group kernels apply the
// mask themselves, recur_f32.h / recur_bwd_f32.h RST): reset[t][b] != 0 means row b enters step t from the
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
__global__ void __launch_bounds__(256)
k_reset_rows(const float* __restrict__ rs, int B, int rpb, ResetZeros z, const float* __restrict__ src,
             float* __restrict__ dst, int cw, int wmax) {
  const long n = (long)B * rpb * wmax;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / wmax;
    const int c = (int)(i - row * wmax);
    const bool r = rs[row / rpb] != 0.f;
    if (dst && c < cw) dst[row * cw + c] = r ? 0.f : src[row * cw + c];
    if (!r) continue;
    for (int k = 0; k < z.n; ++k)
      if (c < z.r[k].w) z.r[k].p[row * z.r[k].ld + (long)c * z.r[k].es] = 0.f;
  }
}

hipError_t reset_rows(const float* rs, int B, int rpb, const ResetZeros& z, const float* src, float* dst, int cw,
                      hipStream_t st) {
  int wmax = dst ? cw : 0;
  for (int k = 0; k < z.n; ++k) wmax = wmax > z.r[k].w ? wmax : z.r[k].w;
  if (wmax <= 0 || B <= 0 || rpb <= 0) return hipSuccess;
  const long n = (long)B * rpb * wmax;
  const int blocks = (int)(n + 255 < 2048L * 256 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_reset_rows, dim3(blocks), dim3(256), 0, st, rs, B, rpb, z, src, dst, cw, wmax);
  return hipGetLastError();
}

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

}  // namespace aaa
