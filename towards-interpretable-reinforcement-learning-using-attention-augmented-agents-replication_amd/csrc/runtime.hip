// Host runtime + C ABI (include/aaa.h): buffer layout, weight packing and the
// launch sequence of the batched unroll forward / hand-written BPTT backward.
//
// Forward (reference attention.py:298-368 over T steps from reset()):
//   conv1, conv2 over all T*B frames at once (no recurrence there), then one
//   fused ConvLSTM kernel per step (x- and h-convs as ONE implicit GEMM over
//   [x_t | h_{t-1}], gate math in the epilogue), then -- because the policy
//   core never carries state (Q1) -- the whole attention / answer / LSTMCell /
//   heads tail batched over all T*B frames.
// Backward (what autograd does for main_mp.py:77): the tail batched over T*B,
// then the only sequential part, the ConvLSTM BPTT (one dgrad GEMM per step
// with the previous step's gate backward fused in its epilogue), then all
// weight gradients as long-K GEMMs over every frame.//
// This unit holds the C ABI of the whole path, the optimizer / loss / sampler
// / actor entries; the layout and state live in rt_core.hip, the forward in
// rt_forward.hip, the backward in rt_backward.hip, the component entries in
// rt_components.hip (shared declarations: rt.h).
#include "rt.h"


using namespace aaa;

// ---- the multi-tensor entries (Adam, RMSProp, clip; optim.h TensorTable) ----
// streams[k]: an entry's k-th array of device pointers, nullptr when the call does not use it.
// The per-tensor refusals, all before the device; who: the entry's message prefix.  The chunks
// that must fit one grid index are one table's (per_table: Adam, RMSProp) or, for the clip
// entries, all tensors': there the partial index runs on through the tables.
template <int K>
static int check_tensors(const char* who, int ntensors, const float* const* const (&streams)[K], const size_t* numel,
                         bool per_table) {
  long nch = 0;
  for (int t = 0; t < ntensors; ++t) {
    if (per_table && t % kAdamMaxTensors == 0) nch = 0;
    if (numel[t] == 0) continue;
    for (int k = 0; k < K; ++k)
      if (streams[k] && !streams[k][t]) return fail(AAA_E_ARG, "%s: NULL pointer for tensor %d", who, t);
    nch += adam_chunks(numel[t]);
    if (nch > (1L << 30)) return fail(AAA_E_ARG, "%s: tensor %d too large", who, t);
  }
  return AAA_OK;
}

// Tensors [t0, t0 + kAdamMaxTensors) as one kernel table, the empty ones left out; returns its chunk count.
template <int K>
static int fill_table(TensorTable<K>& tab, int t0, int ntensors, const float* const* const (&streams)[K],
                      const size_t* numel) {
  memset(&tab, 0, sizeof tab);
  int nch = 0;
  for (int t = t0; t < std::min(ntensors, t0 + kAdamMaxTensors); ++t) {
    if (numel[t] == 0) continue;
    const int i = tab.n++;
    tab.vec[i] = 1;
    for (int k = 0; k < K; ++k) {
      if (!streams[k]) continue;
      tab.s[k][i] = const_cast<float*>(streams[k][t]);
      if (!aligned16(streams[k][t])) tab.vec[i] = 0;
    }
    tab.numel[i] = numel[t];
    tab.chunk0[i] = nch;
    nch += (int)adam_chunks(numel[t]);
  }
  return nch;
}

extern "C" {

int aaa_abi_version(void) { return AAA_ABI_VERSION; }

#ifdef AAA_ABLATION
// Present only in the A/B library (make ablation): tells the tests and tools which build is loaded.
int aaa_ablation_build(void) { return 1; }
#endif

int aaa_fastdiv_check(unsigned d, unsigned lo, unsigned hi, unsigned long long* mismatches) {
  if (!mismatches || d == 0 || d >= (1u << 31) || hi > (1u << 31) || lo > hi)
    return fail(AAA_E_ARG, "fastdiv_check: need 1 <= d < 2^31 and lo <= hi <= 2^31");
  const FastDiv fd(d);
  // exhaustive over [lo, hi): split over host threads; the exact quotient is
  // carried incrementally (no hardware division in the loop)
  const unsigned nthr = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<unsigned long long> bad(nthr, 0);
  std::vector<std::thread> th;
  const unsigned long long span = hi - lo, per = (span + nthr - 1) / nthr;
  for (unsigned t = 0; t < nthr; ++t) {
    th.emplace_back([&, t]() {
      const unsigned long long a = lo + std::min(span, t * per), b = lo + std::min(span, (t + 1) * per);
      if (a >= b) return;
      uint32_t q = (uint32_t)(a / d), r = (uint32_t)(a % d);
      unsigned long long nb = 0;
      for (unsigned long long n = a; n < b; ++n) {
        nb += fd.div((uint32_t)n) != q;
        if (++r == d) { r = 0; ++q; }
      }
      bad[t] = nb;
    });
  }
  for (auto& x : th) x.join();
  unsigned long long tot = 0;
  for (auto v : bad) tot += v;
  *mismatches = tot;
  return AAA_OK;
}

int aaa_divisor_log(int enable, unsigned* out, int cap) {
  DivisorLog& g = divisor_log();
  std::lock_guard<std::mutex> lk(g.mu);
  const int n = (int)g.seen.size();
  if (out)
    for (int i = 0; i < std::min(n, cap); ++i) out[i] = g.seen[i];
  if (enable >= 0) {   // -1: read only
    g.on = enable != 0;
    if (!g.on) g.seen.clear();
  }
  return n;
}

const char* aaa_last_error(void) { return g_err.c_str(); }

int aaa_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_timers.mu);
  g_timers.on = on != 0;
  for (double& w : g_timers.work) w = 0.0;
  for (auto& v : g_timers.variant) v.clear();
  for (auto& v : g_timers.ran) v.clear();
  for (auto& v : g_timers.pending) {
    for (auto& pr : v) { g_timers.pool.push_back(pr.first); g_timers.pool.push_back(pr.second); }
    v.clear();
  }
  return AAA_OK;
}

int aaa_timing_read(int kind, double* total_ms, long* launches) {
  if (!total_ms || !launches) return fail(AAA_E_ARG, "bad timer query");
  aaa_timer_stats s;
  const int rc = aaa_timing_stats(kind, &s);
  *total_ms = s.total_ms;
  *launches = s.launches;
  return rc;
}

int aaa_timing_stats(int kind, aaa_timer_stats* out) {
  if (kind < 0 || kind >= AAA_TIMER_N || !out) return fail(AAA_E_ARG, "bad timer query");
  std::vector<std::pair<hipEvent_t, hipEvent_t>> v;
  memset(out, 0, sizeof *out);
  {
    std::lock_guard<std::mutex> lk(g_timers.mu);
    v.swap(g_timers.pending[kind]);
    out->work = g_timers.work[kind];
    std::string var = g_timers.variant[kind];
    // the tail classes: which kernel and arithmetic each GEMM launch since the last read took (rt.h tail_ran)
    const char* sep = " | ";
    for (const auto& r : g_timers.ran[kind]) {
      var += sep + r.first + (r.second > 1 ? strf("*%d", r.second) : std::string());
      sep = ", ";
    }
    g_timers.ran[kind].clear();
    snprintf(out->variant, sizeof out->variant, "%s", var.c_str());
    g_timers.work[kind] = 0.0;
  }
  double tot = 0.0;
  int rc = AAA_OK;
  for (auto& pr : v) {
    float ms = 0.f;
    if (hipEventSynchronize(pr.second) != hipSuccess || hipEventElapsedTime(&ms, pr.first, pr.second) != hipSuccess)
      rc = fail(AAA_E_LAUNCH, "event timing failed");
    tot += ms;
  }
  {
    std::lock_guard<std::mutex> lk(g_timers.mu);
    for (auto& pr : v) { g_timers.pool.push_back(pr.first); g_timers.pool.push_back(pr.second); }
  }
  out->total_ms = tot;
  out->launches = (long)v.size();
  return rc;
}

int aaa_workspace_region(const aaa_cfg* cfg, int region, size_t* offset, size_t* bytes) {
  if (!offset || !bytes) return fail(AAA_E_ARG, "workspace_region: NULL output");
  Layout L;
  if (int r = build_layout(cfg, L)) return r;
  const size_t F = L.F;
  switch (region) {
    case AAA_WS_ANSWER_HIDDEN: *offset = L.hid1; *bytes = F * 512 * 4; return AAA_OK;
    // the policy tail's GEMM operands, products and cotangents: fp32 in both dtypes and every geometry, each in
    // a buffer of its own that no phase reuses (build_layout), so a checker's fp64 reference of one tail layer
    // reads that layer's input as the kernel stored it
    case AAA_WS_TAIL_ANS: *offset = L.ans; *bytes = F * L.ans_ld * 4; return AAA_OK;
    case AAA_WS_TAIL_GATES: *offset = L.LG; *bytes = F * 1024 * 4; return AAA_OK;
    case AAA_WS_TAIL_DY: *offset = L.dY; *bytes = F * L.ldy * 4; return AAA_OK;
    case AAA_WS_TAIL_DGATES: *offset = L.dLG; *bytes = F * 1024 * 4; return AAA_OK;
    case AAA_WS_TAIL_DHID: *offset = L.dH1; *bytes = F * 512 * 4; return AAA_OK;
    case AAA_WS_TAIL_DANS: *offset = L.dAns; *bytes = F * L.da * 4; return AAA_OK;
    case AAA_WS_TAIL_AO:
    case AAA_WS_TAIL_C:
    case AAA_WS_TAIL_H:
    case AAA_WS_TAIL_DAO:
      if (L.sc) break;
      *offset = region == AAA_WS_TAIL_AO ? L.AO : region == AAA_WS_TAIL_C ? L.LC : region == AAA_WS_TAIL_H ? L.LH : L.dAO;
      *bytes = F * 256 * 4;
      return AAA_OK;
    case AAA_WS_TAIL_AOX:
    case AAA_WS_TAIL_DAOX:
      if (!L.sc) break;
      *offset = region == AAA_WS_TAIL_AOX ? L.AOX : L.dAOX; *bytes = F * 512 * 4; return AAA_OK;
    case AAA_WS_TAIL_CH:
    case AAA_WS_TAIL_CC:
      if (!L.sc) break;
      *offset = region == AAA_WS_TAIL_CH ? L.CH : L.CC; *bytes = (size_t)(L.T + 1) * L.B * 256 * 4; return AAA_OK;
    case AAA_WS_TAIL_QUERY:
    case AAA_WS_TAIL_DQUERY:
    case AAA_WS_TAIL_DQ2:
      if (!L.sc) break;
      *offset = region == AAA_WS_TAIL_QUERY ? L.Qf : region == AAA_WS_TAIL_DQUERY ? L.dQf : L.dq2s;
      *bytes = F * (size_t)L.qd * 4;
      return AAA_OK;
    case AAA_WS_TAIL_DQ1:
      if (!L.sc) break;
      *offset = L.dq1s; *bytes = F * 128 * 4; return AAA_OK;
    case AAA_WS_QUERY_HIDDEN0:
      if (!L.sc) break;
      *offset = L.q1s; *bytes = F * 128 * 4; return AAA_OK;
    case AAA_WS_QUERY_HIDDEN1:
      if (!L.sc) break;
      *offset = L.q2s; *bytes = F * (size_t)L.qd * 4; return AAA_OK;
    // The recurrence's buffers as the kernels store them, each a buffer of its own (a checker's fp64 reference of the
    // ConvLSTM GEMMs reads their own operands and cotangents here).  AAA_WS_CORE_*: fp32 configs only, all row-major.
    // AAA_BF16_WS_*: bf16 configs only; _C / _GATES / _DO channel-quad-major where aaa_core_layout's mask says so.
    case AAA_WS_CORE_XH: case AAA_WS_CORE_DO: case AAA_WS_CORE_DX:
    case AAA_BF16_WS_XH: case AAA_BF16_WS_C: case AAA_BF16_WS_GATES:
    case AAA_BF16_WS_DO: case AAA_BF16_WS_DZ: case AAA_BF16_WS_DX: {
      if ((region <= AAA_WS_CORE_DX) != (L.dt == AAA_F32)) break;
      const size_t M = (size_t)L.B * L.P, e = L.esz;
      if (region == AAA_WS_CORE_XH || region == AAA_BF16_WS_XH) { *offset = L.XH; *bytes = (size_t)(L.T + 1) * M * 192 * e; }
      else if (region == AAA_WS_CORE_DO || region == AAA_BF16_WS_DO) { *offset = L.dO; *bytes = F * L.P * 128 * 4; }
      else if (region == AAA_WS_CORE_DX || region == AAA_BF16_WS_DX) { *offset = L.dY2; *bytes = F * L.P * 64 * e; }
      else if (region == AAA_BF16_WS_C) { *offset = L.Cst; *bytes = (size_t)(L.T + 1) * M * 128 * 4; }
      else if (region == AAA_BF16_WS_DZ) { *offset = L.dZ; *bytes = F * L.P * 512 * 2; }
      else { *offset = L.Gt; *bytes = F * L.P * 512 * recur_plan(L, false).gate_bytes; }
      return AAA_OK;
    }
    case AAA_BF16_WS_HR:   // h_t for the readout of a masked call: bf16 cfgs with AAA_FLAG_BF16_RESETS, the last region
      if (!L.br) break;
      *offset = L.HR; *bytes = F * L.P * 128 * 2; return AAA_OK;
    default: break;
  }
  return fail(AAA_E_ARG, "workspace_region: region %d not computed by this cfg", region);
}

int aaa_core_layout(const aaa_cfg* cfg, int* gate_bytes, int* cqm_mask) {
  if (!gate_bytes || !cqm_mask) return fail(AAA_E_ARG, "core_layout: NULL output");
  Layout L;
  if (int r = build_layout(cfg, L)) return r;
  const RecurPlan plan = recur_plan(L, false);
  *gate_bytes = plan.gate_bytes;
  *cqm_mask = plan.cqm;
  return AAA_OK;
}

int aaa_grid(int H, int W, int* h, int* w) {
  if (!h || !w) return fail(AAA_E_ARG, "NULL output");
  *h = conv_out(conv_out(H, 8, 4, 1), 4, 2, 2);
  *w = conv_out(conv_out(W, 8, 4, 1), 4, 2, 2);
  return (*h >= 1 && *w >= 1) ? AAA_OK : fail(AAA_E_ARG, "frame too small");
}

int aaa_param_layout(const aaa_cfg* cfg, size_t* total, size_t* offsets, size_t* sizes) {
  Layout L;
  int r = build_layout(cfg, L);
  if (r) return r;
  if (total) *total = L.ptotal;
  for (int i = 0; i < NPARAM; ++i) {
    if (offsets) offsets[i] = L.poff[i];
    if (sizes) sizes[i] = L.psz[i];
  }
  return AAA_OK;
}

size_t aaa_packed_bytes(const aaa_cfg* cfg) {
  Layout L;
  return build_layout(cfg, L) ? 0 : L.packed;
}

size_t aaa_workspace_bytes(const aaa_cfg* cfg) {
  Layout L;
  return build_layout(cfg, L) ? 0 : L.ws;
}

int aaa_pack_weights(const aaa_cfg* cfg, const float* params, void* packed, hipStream_t stream) {
  Layout L;
  int r = build_layout(cfg, L);
  if (r) return r;
  if ((r = check_device())) return r;
  if (!params || !packed) return fail(AAA_E_ARG, "NULL params/packed");
  if (!aligned16(params) || !aligned16(packed)) return fail(AAA_E_ALIGN, "params/packed must be 16-byte aligned");
  TimerScope tim(AAA_TIMER_PACK, stream, 0.0, "pack_all + fragment-order copies + query pack");
  return L.dt == AAA_BF16 ? pack_impl<__bf16>(L, params, (char*)packed, stream)
                          : pack_impl<float>(L, params, (char*)packed, stream);
}

static int check_io(const Layout& L, const aaa_io* io, bool bwd) {
  if (!io) return fail(AAA_E_ARG, "io is NULL");
  if (!io->params || !io->packed || !io->basis || !io->frames || !io->workspace)
    return fail(AAA_E_ARG, "params/packed/basis/frames/workspace must be set");
  if (!bwd && (!io->logits || !io->values)) return fail(AAA_E_ARG, "logits/values outputs must be set");
  if (bwd && (!io->dlogits || !io->grads)) return fail(AAA_E_ARG, "dlogits/grads must be set");
  const void* ptrs[] = {io->params, io->packed, io->basis, io->frames, io->workspace, io->h0, io->c0, io->hT,
                        io->cT, io->dhT, io->dcT, io->dh0, io->dc0, io->grads};
  for (const void* p : ptrs)
    if (p && !aligned16(p)) return fail(AAA_E_ALIGN, "buffers must be 16-byte aligned");
  (void)L;
  return AAA_OK;
}

int aaa_forward_phases(const aaa_cfg* cfg, const aaa_io* io, int phases, hipStream_t stream) {
  Layout L;
  int r = build_layout(cfg, L);
  if (r) return r;
  if (phases != AAA_FWD_ALL && phases != (AAA_FWD_VISION | AAA_FWD_TAIL))
    return fail(AAA_E_ARG, "forward phases %d: AAA_FWD_ALL or AAA_FWD_VISION | AAA_FWD_TAIL", phases);
  if (!(phases & AAA_FWD_CORE) && recur_plan(L, false).cqm)
    return fail(AAA_E_ARG, "skipping the core: not with channel-quad-major slices (the frame-resident BPTT's)");
  if ((r = check_device())) return r;
  if ((r = check_io(L, io, false))) return r;
  if (!(cfg->flags & AAA_FLAG_DEFER_STRANDED) && (r = pair_check())) return r;
  return L.dt == AAA_BF16 ? forward_impl<__bf16>(L, io, stream, phases) : forward_impl<float>(L, io, stream, phases);
}

int aaa_forward(const aaa_cfg* cfg, const aaa_io* io, hipStream_t stream) {
  return aaa_forward_phases(cfg, io, AAA_FWD_ALL, stream);
}

// The recurrence's per-step products in the workspace (rt_core.hip
// build_layout): Gt [T][M][512] (fp32, or fp16 on the bf16 path's gate
// storage), Cst [T+1][M][128] fp32 (slot t+1 = c_t), Hs [T][M][128] fp32 (= h_t;
// fp32 path only), XH [T+1][M][192] (channels 64.. of slot t+1 = h_t, in the
// operand type: the bf16 path's only copy of h_t).
// *ge <- bytes of one stored gate activation
static int core_xfer_check(const aaa_cfg* cfg, Layout& L, const void* ws, int t0, int n, size_t* ge) {
  int r = build_layout(cfg, L);
  if (r) return r;
  const RecurPlan plan = recur_plan(L, false);
  *ge = plan.gate_bytes;
  if (plan.cqm) return fail(AAA_E_ARG, "core export/import: channel-quad-major slices unsupported");
  if (!ws || t0 < 0 || n < 1 || t0 + n > L.T) return fail(AAA_E_ARG, "core export/import: steps [%d, %d) of T=%d", t0, t0 + n, L.T);
  return check_device();
}

int aaa_core_elem_bytes(const aaa_cfg* cfg, int* gate_bytes, int* h_bytes) {
  if (!gate_bytes || !h_bytes) return fail(AAA_E_ARG, "core_elem_bytes: NULL output");
  Layout L;
  if (int r = build_layout(cfg, L)) return r;
  const RecurPlan plan = recur_plan(L, false);
  const bool ok = !plan.cqm;   // channel-quad-major slices: no export / import (0 bytes)
  *gate_bytes = ok ? plan.gate_bytes : 0;
  *h_bytes = ok ? L.esz : 0;
  return AAA_OK;
}

int aaa_core_export(const aaa_cfg* cfg, const void* workspace, int t0, int n, void* gates, float* c, void* h,
                    hipStream_t st) {
  Layout L;
  size_t ge;
  if (int r = core_xfer_check(cfg, L, workspace, t0, n, &ge)) return r;
  const char* ws = (const char*)workspace;
  const size_t M = (size_t)L.B * L.P;
  if (gates) HIPCHK(hipMemcpyAsync(gates, ws + L.Gt + (size_t)t0 * M * 512 * ge, (size_t)n * M * 512 * ge, hipMemcpyDeviceToDevice, st));
  if (c) HIPCHK(hipMemcpyAsync(c, ws + L.Cst + (size_t)(t0 + 1) * M * 128 * 4, (size_t)n * M * 128 * 4, hipMemcpyDeviceToDevice, st));
  if (h && L.esz == 4)
    HIPCHK(hipMemcpyAsync(h, ws + L.Hs + (size_t)t0 * M * 128 * 4, (size_t)n * M * 128 * 4, hipMemcpyDeviceToDevice, st));
  else if (h)   // bf16: the h half of XH slots t0+1 .. t0+n (n*M consecutive 192-channel rows)
    HIPCHK(hipMemcpy2DAsync(h, 128 * 2, ws + L.XH + ((size_t)(t0 + 1) * M * 192 + 64) * 2, 192 * 2, 128 * 2, n * M,
                            hipMemcpyDeviceToDevice, st));
  return AAA_OK;
}

int aaa_core_import(const aaa_cfg* cfg, void* workspace, int t0, int n, const void* gates, const float* c,
                    const void* h, hipStream_t st) {
  Layout L;
  size_t ge;
  if (int r = core_xfer_check(cfg, L, workspace, t0, n, &ge)) return r;
  if (!gates || !c || !h) return fail(AAA_E_ARG, "core import: gates, c and h are required");
  char* ws = (char*)workspace;
  const size_t M = (size_t)L.B * L.P;
  HIPCHK(hipMemcpyAsync(ws + L.Gt + (size_t)t0 * M * 512 * ge, gates, (size_t)n * M * 512 * ge, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(ws + L.Cst + (size_t)(t0 + 1) * M * 128 * 4, c, (size_t)n * M * 128 * 4, hipMemcpyDeviceToDevice, st));
  if (L.esz == 4) {
    HIPCHK(hipMemcpyAsync(ws + L.Hs + (size_t)t0 * M * 128 * 4, h, (size_t)n * M * 128 * 4, hipMemcpyDeviceToDevice, st));
    // slots t0+1 .. t0+n of XH are n*M consecutive 192-channel rows: one launch
    HIPCHK(state_to_xh<float>((int)(n * M), (const float*)h, (float*)(ws + L.XH) + (size_t)(t0 + 1) * M * 192, st));
  } else {
    HIPCHK(hipMemcpy2DAsync(ws + L.XH + ((size_t)(t0 + 1) * M * 192 + 64) * 2, 192 * 2, h, 128 * 2, 128 * 2, n * M,
                            hipMemcpyDeviceToDevice, st));
  }
  return AAA_OK;
}

int aaa_backward(const aaa_cfg* cfg, const aaa_io* io, int phases, hipStream_t stream) {
  Layout L;
  int r = build_layout(cfg, L);
  if (r) return r;
  if ((r = check_device())) return r;
  if ((r = check_io(L, io, true))) return r;
  if (phases & ~AAA_BWD_ALL || !phases) return fail(AAA_E_ARG, "bad phase mask %d", phases);
  if (!(cfg->flags & AAA_FLAG_DEFER_STRANDED) && (r = pair_check())) return r;
  return L.dt == AAA_BF16 ? backward_impl<__bf16>(L, io, phases, stream)
                          : backward_impl<float>(L, io, phases, stream);
}

// Episode-start masks (include/aaa.h): what a mask cannot go with, refused before the device is touched.
static int check_reset(const Layout& L, const float* reset, const char* who) {
  if (!reset) return AAA_OK;
  if (L.dt == AAA_BF16 && !L.br)
    return fail(AAA_E_ARG, "%s: an episode-start mask needs an fp32 cfg, or a bf16 cfg with AAA_FLAG_BF16_RESETS (the "
                "bf16 readout reads h_t from the [x | h] operand slots, which a reset zeroes; the flag adds a copy "
                "for it); or pass reset = NULL and cut the unroll at episode ends", who);
  if (!aligned16(reset)) return fail(AAA_E_ALIGN, "%s: the reset mask must be 16-byte aligned", who);
  return AAA_OK;
}

int aaa_forward_resets(const aaa_cfg* cfg, const aaa_io* io, int phases, const float* reset, hipStream_t stream) {
  if (!reset) return aaa_forward_phases(cfg, io, phases, stream);
  Layout L;
  int r = build_layout(cfg, L);
  if (r) return r;
  if (phases != AAA_FWD_ALL && phases != (AAA_FWD_VISION | AAA_FWD_TAIL))
    return fail(AAA_E_ARG, "forward phases %d: AAA_FWD_ALL or AAA_FWD_VISION | AAA_FWD_TAIL", phases);
  if ((r = check_reset(L, reset, "forward_resets"))) return r;
  if (!(phases & AAA_FWD_CORE))
    return fail(AAA_E_ARG, "forward_resets: an episode-start mask needs AAA_FWD_CORE (imported ConvLSTM products "
                "were computed without it)");
  if ((r = check_device())) return r;
  if ((r = check_io(L, io, false))) return r;
  if (!(cfg->flags & AAA_FLAG_DEFER_STRANDED) && (r = pair_check())) return r;
  return L.dt == AAA_BF16 ? forward_impl<__bf16>(L, io, stream, phases, reset)
                          : forward_impl<float>(L, io, stream, phases, reset);
}

int aaa_backward_resets(const aaa_cfg* cfg, const aaa_io* io, int phases, const float* reset, hipStream_t stream) {
  if (!reset) return aaa_backward(cfg, io, phases, stream);
  Layout L;
  int r = build_layout(cfg, L);
  if (r) return r;
  if ((r = check_reset(L, reset, "backward_resets"))) return r;
  if ((r = check_device())) return r;
  if ((r = check_io(L, io, true))) return r;
  if (phases & ~AAA_BWD_ALL || !phases) return fail(AAA_E_ARG, "bad phase mask %d", phases);
  if (!(cfg->flags & AAA_FLAG_DEFER_STRANDED) && (r = pair_check())) return r;
  return L.dt == AAA_BF16 ? backward_impl<__bf16>(L, io, phases, stream, reset)
                          : backward_impl<float>(L, io, phases, stream, reset);
}

int aaa_pair_status(hipStream_t stream, int clear) {
  if (stream && hipStreamSynchronize(stream) != hipSuccess) return fail(AAA_E_LAUNCH, "stream synchronize failed");
  if (!stream && hipDeviceSynchronize() != hipSuccess) return fail(AAA_E_LAUNCH, "device synchronize failed");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fail(AAA_E_DEVICE, "no HIP device");
  return clear ? pair_take() : pair_peek();
}

int aaa_pair_flag(float* dst, hipStream_t stream) {
  if (!dst) return fail(AAA_E_ARG, "pair_flag: NULL dst");
  int r = check_device();
  if (r) return r;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  const int* rep = pair_report(dev);
  int* base = pair_flag_base(dev);
  if (!rep || !base) return fail(AAA_E_LAUNCH, "cannot map the partner-timeout report word");
  HIPCHK(pair_flag_launch(rep, base, dst, stream));
  return AAA_OK;
}

int aaa_pair_flag_at(float* dst, int* base, hipStream_t stream) {
  if (!dst || !base) return fail(AAA_E_ARG, "pair_flag_at: NULL dst or base");
  int r = check_device();
  if (r) return r;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  const int* rep = pair_report(dev);
  if (!rep) return fail(AAA_E_LAUNCH, "cannot map the partner-timeout report word");
  HIPCHK(pair_flag_launch(rep, base, dst, stream));
  return AAA_OK;
}

int aaa_adam_step(const aaa_adam_hparams* hp, long step, int ntensors, float* const* params,
                  const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  float* const* max_exp_avg_sq, const size_t* numel, hipStream_t stream) {
  return aaa_adam_step_guarded(hp, step, nullptr, ntensors, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel,
                               stream);
}

// who: the entry's message prefix; stats: aaa_adam_step_clipped's, or nullptr
static int adam_impl(const aaa_adam_hparams* hp, long step, int* step_dev, const float* guard, int ntensors,
                     float* const* params, const float* const* grads, float* const* exp_avg,
                     float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* numel,
                     hipStream_t stream, const char* who = "adam", const float* stats = nullptr) {
  if (!hp || ntensors < 0 || (ntensors > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numel)))
    return fail(AAA_E_ARG, "%s: NULL argument", who);
  if (!step_dev && step < 1) return fail(AAA_E_ARG, "%s: step must be >= 1 (got %ld)", who, step);
  if (hp->amsgrad && !max_exp_avg_sq) return fail(AAA_E_ARG, "%s: amsgrad needs max_exp_avg_sq", who);
  if (!(hp->lr >= 0.0) || !(hp->eps >= 0.0) || !(hp->beta1 >= 0.0 && hp->beta1 < 1.0) ||
      !(hp->beta2 >= 0.0 && hp->beta2 < 1.0) || !(hp->weight_decay >= 0.0))
    return fail(AAA_E_ARG, "%s: invalid hyper-parameters", who);
  const float* const* const streams[5] = {params, grads, exp_avg, exp_avg_sq, hp->amsgrad ? max_exp_avg_sq : nullptr};
  int r = check_tensors(who, ntensors, streams, numel, true);
  if (r) return r;
  if ((r = check_device())) return r;
  AdamHost h{hp->lr, hp->beta1, hp->beta2, hp->eps, hp->weight_decay, step_dev ? 1 : step, hp->amsgrad ? 1 : 0,
             hp->maximize ? 1 : 0, guard, step_dev, stats};
  for (int t0 = 0; t0 < ntensors; t0 += kAdamMaxTensors) {
    TensorTable<5> tab;
    const int nch = fill_table(tab, t0, ntensors, streams, numel);
    HIPCHK(adam_launch(tab, nch, h, stream, t0 + kAdamMaxTensors >= ntensors));
  }
  if (ntensors == 0 && step_dev) HIPCHK(adam_launch(TensorTable<5>{}, 0, h, stream, true));
  return AAA_OK;
}

int aaa_adam_step_guarded(const aaa_adam_hparams* hp, long step, const float* guard, int ntensors,
                          float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* numel,
                          hipStream_t stream) {
  return adam_impl(hp, step, nullptr, guard, ntensors, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel,
                   stream);
}

int aaa_adam_step_counted(const aaa_adam_hparams* hp, int* step_dev, const float* guard, int ntensors,
                          float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* numel,
                          hipStream_t stream) {
  if (!step_dev) return fail(AAA_E_ARG, "adam: NULL step counter");
  return adam_impl(hp, 0, step_dev, guard, ntensors, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel,
                   stream);
}

// ---- gradient clipping by global norm ----
// The argument checks of aaa_grad_norm / aaa_grad_scale on the gradients, all before the device.
static int clip_check_grads(const char* who, int ntensors, const float* const* const (&grads)[1], const size_t* numel) {
  if (ntensors < 0) return fail(AAA_E_ARG, "%s: ntensors must be >= 0 (got %d)", who, ntensors);
  if (ntensors > 0 && (!grads[0] || !numel)) return fail(AAA_E_ARG, "%s: NULL grads or numel array", who);
  return check_tensors(who, ntensors, grads, numel, false);
}

size_t aaa_grad_norm_scratch_bytes(int ntensors, const size_t* numel) {
  size_t nch = 0;
  for (int t = 0; numel && t < ntensors; ++t) nch += (size_t)adam_chunks(numel[t]);
  return std::max<size_t>(16, (nch * sizeof(double) + 15) & ~(size_t)15);
}

int aaa_grad_norm(double max_norm, int ntensors, const float* const* grads, const size_t* numel, float* stats,
                  void* scratch, hipStream_t stream) {
  const float* const* const streams[1] = {grads};
  int r = clip_check_grads("clip: grad_norm", ntensors, streams, numel);
  if (r) return r;
  if (!stats || !scratch) return fail(AAA_E_ARG, "clip: grad_norm: NULL stats or scratch");
  if (!(max_norm > 0.0)) return fail(AAA_E_ARG, "clip: grad_norm: max_norm must be positive (+inf: norm only)");
  if (!aligned16(stats) || !aligned16(scratch))
    return fail(AAA_E_ALIGN, "clip: grad_norm: stats and scratch must be 16-byte aligned");
  r = check_device();
  if (r) return r;
  int base = 0;   // the partial index runs on through the tables
  for (int t0 = 0; t0 < ntensors; t0 += kAdamMaxTensors) {
    TensorTable<1> tab;
    const int nch = fill_table(tab, t0, ntensors, streams, numel);
    HIPCHK(gradsq_launch(tab, nch, base, (double*)scratch, stream));
    base += nch;
  }
  HIPCHK(gradsq_finish_launch((const double*)scratch, base, max_norm, stats, stream));
  return AAA_OK;
}

int aaa_grad_scale(const float* stats, int ntensors, float* const* grads, const size_t* numel, hipStream_t stream) {
  const float* const* const streams[1] = {grads};
  int r = clip_check_grads("clip: grad_scale", ntensors, streams, numel);
  if (r) return r;
  if (!stats) return fail(AAA_E_ARG, "clip: grad_scale: NULL stats");
  if (!aligned16(stats)) return fail(AAA_E_ALIGN, "clip: grad_scale: stats must be 16-byte aligned");
  r = check_device();
  if (r) return r;
  for (int t0 = 0; t0 < ntensors; t0 += kAdamMaxTensors) {
    TensorTable<1> tab;
    const int nch = fill_table(tab, t0, ntensors, streams, numel);
    HIPCHK(grad_scale_launch(tab, nch, stats, stream));
  }
  return AAA_OK;
}

int aaa_adam_step_clipped(const aaa_adam_hparams* hp, int* step_dev, const float* guard, const float* stats,
                          int ntensors, float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* numel,
                          hipStream_t stream) {
  if (!step_dev || !stats) return fail(AAA_E_ARG, "clip: adam: NULL step counter or stats");
  if (!aligned16(stats)) return fail(AAA_E_ALIGN, "clip: adam: stats must be 16-byte aligned");
  return adam_impl(hp, 0, step_dev, guard, ntensors, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel,
                   stream, "clip: adam", stats);
}

// ---- RMSProp ----
int aaa_rmsprop_step(const aaa_rmsprop_hparams* hp, long step, int* step_dev, const float* guard,
                     const float* stats, int ntensors, float* const* params, const float* const* grads,
                     float* const* square_avg, float* const* momentum_buf, float* const* grad_avg,
                     const size_t* numel, hipStream_t stream) {
  if (!hp) return fail(AAA_E_ARG, "rmsprop: NULL hyper-parameters");
  if (ntensors < 0) return fail(AAA_E_ARG, "rmsprop: ntensors must be >= 0 (got %d)", ntensors);
  if (!(hp->lr >= 0.0) || !(hp->lr_end >= 0.0) || !(hp->alpha >= 0.0) || !(hp->eps >= 0.0) ||
      !(hp->weight_decay >= 0.0) || !(hp->momentum >= 0.0))
    return fail(AAA_E_ARG, "rmsprop: invalid hyper-parameters (lr, lr_end, alpha, eps, weight_decay and momentum "
                           "must be >= 0)");
  if (hp->anneal_steps < 0) return fail(AAA_E_ARG, "rmsprop: anneal_steps must be >= 0 (got %ld)", hp->anneal_steps);
  if (!step_dev && step < 1) return fail(AAA_E_ARG, "rmsprop: step must be >= 1 (got %ld)", step);
  const bool mom = hp->momentum > 0.0, cent = hp->centered != 0;
  if (ntensors > 0 && (!params || !grads || !square_avg || !numel || (mom && !momentum_buf) || (cent && !grad_avg)))
    return fail(AAA_E_ARG, "rmsprop: NULL array (momentum > 0 needs momentum_buf, centered needs grad_avg)");
  const float* const* const streams[5] = {params, grads, square_avg, mom ? momentum_buf : nullptr,
                                          cent ? grad_avg : nullptr};
  int r = check_tensors("rmsprop", ntensors, streams, numel, true);
  if (r) return r;
  if (stats && !aligned16(stats)) return fail(AAA_E_ALIGN, "rmsprop: stats must be 16-byte aligned");
  if ((r = check_device())) return r;
  RmspropHost h{hp->lr, hp->alpha, hp->eps, hp->weight_decay, hp->momentum, hp->lr_end, hp->anneal_steps,
                step_dev ? 1 : step, cent ? 1 : 0, hp->maximize ? 1 : 0, hp->eps_in_sqrt ? 1 : 0, guard, step_dev, stats};
  for (int t0 = 0; t0 < ntensors; t0 += kAdamMaxTensors) {
    TensorTable<5> tab;
    const int nch = fill_table(tab, t0, ntensors, streams, numel);
    HIPCHK(rmsprop_launch(tab, nch, h, stream, t0 + kAdamMaxTensors >= ntensors));
  }
  if (ntensors == 0 && step_dev) HIPCHK(rmsprop_launch(TensorTable<5>{}, 0, h, stream, true));
  return AAA_OK;
}

int aaa_reinforce(int T, int B, int A, const float* logits, const int* actions, const float* rewards, double gamma,
                  float* loss, float* returns_norm, float* dlogits, hipStream_t stream) {
  if (T < 1 || B < 1 || A < 1) return fail(AAA_E_ARG, "reinforce: need T, B, A >= 1 (T=%d B=%d A=%d)", T, B, A);
  if (!logits || !actions || !rewards || !loss || !returns_norm || !dlogits)
    return fail(AAA_E_ARG, "reinforce: NULL argument");
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(AAA_E_ARG, "reinforce: gamma must be in [0, 1]");
  int r = check_device();
  if (r) return r;
  HIPCHK(reinforce_launch(T, B, A, logits, actions, rewards, gamma, loss, returns_norm, dlogits, stream));
  return AAA_OK;
}

int aaa_vtrace(const aaa_vtrace_desc* d, const aaa_vtrace_io* io, hipStream_t stream) {
  if (!d || !io) return fail(AAA_E_ARG, "vtrace: NULL desc or io");
  if (d->T < 1 || d->B < 1 || d->A < 2)
    return fail(AAA_E_ARG, "vtrace: need T, B >= 1 and A >= 2 (T=%d B=%d A=%d)", d->T, d->B, d->A);
  if (d->value_col < 0 || d->value_col >= d->A)
    return fail(AAA_E_ARG, "vtrace: value_col %d outside [0, %d)", d->value_col, d->A);
  if (!(d->gamma >= 0.0 && d->gamma <= 1.0) || !(d->lambda >= 0.0 && d->lambda <= 1.0))
    return fail(AAA_E_ARG, "vtrace: gamma and lambda must be in [0, 1]");
  auto pos = [](double v) { return v > 0.0 && std::isfinite(v); };
  auto nonneg = [](double v) { return v >= 0.0 && std::isfinite(v); };
  if (!pos(d->rho_bar) || !pos(d->c_bar) || !pos(d->pg_rho_bar))
    return fail(AAA_E_ARG, "vtrace: rho_bar, c_bar and pg_rho_bar must be positive and finite");
  if (!nonneg(d->baseline_cost) || !nonneg(d->entropy_cost) || !nonneg(d->scale))
    return fail(AAA_E_ARG, "vtrace: baseline_cost, entropy_cost and scale must be non-negative and finite");
  if (!io->logits || !io->values || !io->actions || !io->rewards || !io->dlogits || !io->dvalues)
    return fail(AAA_E_ARG, "vtrace: NULL argument (logits, values, actions, rewards, dlogits and dvalues are required)");
  if (!aligned16(io->dlogits) || !aligned16(io->dvalues))
    return fail(AAA_E_ALIGN, "vtrace: dlogits and dvalues must be 16-byte aligned");
  int r = check_device();
  if (r) return r;
  HIPCHK(vtrace_launch(*d, *io, stream));
  return AAA_OK;
}

int aaa_sample_actions(int B, int A, const float* logits, unsigned long long seed, unsigned long long* counter,
                       int* actions, float* logp, float* dlogp_dlogits, hipStream_t stream) {
  if (B < 1 || A < 1) return fail(AAA_E_ARG, "sample_actions: need B, A >= 1 (B=%d A=%d)", B, A);
  if (!logits || !actions || !logp) return fail(AAA_E_ARG, "sample_actions: NULL argument");
  int r = check_device();
  if (r) return r;
  HIPCHK(sample_launch(B, A, logits, seed, counter, actions, logp, dlogp_dlogits, stream));
  return AAA_OK;
}

// ---- actor unroll recorder (include/aaa.h; csrc/unroll.hip) ----
// Every refusal of aaa_unroll_begin (record = false) / aaa_unroll_record, before the device.
static int unroll_check(bool record, const aaa_unroll_desc* d, const aaa_unroll_io* io) {
  const char* who = record ? "record" : "begin";
  if (!d || !io) return fail(AAA_E_ARG, "unroll: %s: NULL desc or io", who);
  if (d->T < 2) return fail(AAA_E_ARG, "unroll: %s: T must be >= 2 (got %d): consecutive unrolls share a step", who, d->T);
  if (d->B < 1) return fail(AAA_E_ARG, "unroll: %s: B must be >= 1 (got %d)", who, d->B);
  if (d->b0 < 0 || (long)d->b0 + d->B > (long)d->Bu)
    return fail(AAA_E_ARG, "unroll: %s: rows [b0, b0 + B) = [%d, %ld) lie outside the %d rows of the banks", who, d->b0,
                (long)d->b0 + d->B, d->Bu);
  if (d->frame_bytes == 0) return fail(AAA_E_ARG, "unroll: %s: frame_bytes must be > 0", who);
  if (d->state_floats % 4 != 0)
    return fail(AAA_E_ARG, "unroll: %s: state_floats must be a multiple of 4 (got %zu)", who, d->state_floats);
  if (d->core != 0 && d->core != 256) return fail(AAA_E_ARG, "unroll: %s: core must be 0 or 256 (got %d)", who, d->core);
  if (!(d->reward_clip >= 0.0)) return fail(AAA_E_ARG, "unroll: %s: reward_clip must be >= 0 (0: no clipping)", who);
  // one workgroup per 16 KB of a row: the grid of either launch stays far inside 2^31
  if (d->frame_bytes > ((size_t)1 << 40) || d->state_floats > ((size_t)1 << 40) ||
      (long)d->B * (record ? unroll_record_chunks(*d) : unroll_begin_chunks(*d)) > (1L << 30))
    return fail(AAA_E_ARG, "unroll: %s: B x row size too large for one launch", who);
  if (!io->pos || !io->done_in) return fail(AAA_E_ARG, "unroll: %s: NULL pos or done_in", who);
  if (record) {
    if (!io->frame || !io->actions || !io->logp || !io->reward_in)
      return fail(AAA_E_ARG, "unroll: record: NULL frame, actions, logp or reward_in");
    for (int k = 0; k < 2; ++k) {
      const aaa_unroll_bank& b = io->bank[k];
      if (!b.frames || !b.actions || !b.logp || !b.rewards || !b.done)
        return fail(AAA_E_ARG, "unroll: record: NULL frames, actions, logp, rewards or done in bank %d", k);
    }
  } else {
    if (!io->h || !io->c) return fail(AAA_E_ARG, "unroll: begin: NULL h or c");
    if (d->core && (!io->core_h || !io->core_c)) return fail(AAA_E_ARG, "unroll: begin: core = 256 needs core_h and core_c");
    for (int k = 0; k < 2; ++k) {
      const aaa_unroll_bank& b = io->bank[k];
      if (!b.first || !b.h0 || !b.c0) return fail(AAA_E_ARG, "unroll: begin: NULL first, h0 or c0 in bank %d", k);
      if (d->core && (!b.core_h0 || !b.core_c0))
        return fail(AAA_E_ARG, "unroll: begin: core = 256 needs core_h0 and core_c0 in bank %d", k);
    }
  }
  if (!aligned16(io->pos)) return fail(AAA_E_ALIGN, "unroll: %s: pos must be 16-byte aligned", who);
  // the state pointers are checked by both calls (NULL is aligned): a recorder that begin would refuse is refused at once
  bool ok = aligned16(io->h) && aligned16(io->c) && aligned16(io->core_h) && aligned16(io->core_c);
  for (int k = 0; k < 2; ++k) {
    const aaa_unroll_bank& b = io->bank[k];
    ok = ok && aligned16(b.h0) && aligned16(b.c0) && aligned16(b.core_h0) && aligned16(b.core_c0);
  }
  if (!ok)
    return fail(AAA_E_ALIGN, "unroll: %s: h, c, core_h, core_c and the banks' h0, c0, core_h0, core_c0 must be 16-byte "
                             "aligned", who);
  if (d->frame_bytes % 16 == 0 && (!aligned16(io->frame) || !aligned16(io->bank[0].frames) || !aligned16(io->bank[1].frames)))
    return fail(AAA_E_ALIGN, "unroll: %s: frame and the banks' frames must be 16-byte aligned when frame_bytes %% 16 == 0",
                who);
  return AAA_OK;
}

int aaa_unroll_begin(const aaa_unroll_desc* d, const aaa_unroll_io* io, hipStream_t stream) {
  int r = unroll_check(false, d, io);
  if (r) return r;
  if ((r = check_device())) return r;
  HIPCHK(unroll_begin_launch(*d, *io, stream));
  return AAA_OK;
}

int aaa_unroll_record(const aaa_unroll_desc* d, const aaa_unroll_io* io, hipStream_t stream) {
  int r = unroll_check(true, d, io);
  if (r) return r;
  if ((r = check_device())) return r;
  HIPCHK(unroll_record_launch(*d, *io, stream));
  return AAA_OK;
}

// ---- actor step (include/aaa.h; csrc/actor.hip) ----
// Workspace: conv2 output X (B,P,64), h_t Hs (B,P,128), hid1 (B,512), AO (B,256), LH (B,256),
// the ConvLSTM's split-K partial tiles, the tile and readout counters, the attention logits,
// the readout's chunk partials and the answer row (actor.h).
// The stateful-core entry (core = true) adds Q_t (B, nq*72) and the query MLP's two hidden rows.
constexpr int kActRegions = 13;
static int actor_layout(const aaa_cfg* cfg, Layout& L, size_t off[kActRegions], size_t* total, bool core = false,
                        size_t* bytes = nullptr) {
  int r = build_layout(cfg, L);
  if (r) return r;
  const char* who = core ? "actor_step_core" : "actor_step";
  if (cfg->T != 1) return fail(AAA_E_ARG, "%s: T must be 1 (got %d)", who, cfg->T);
  if (cfg->dtype != AAA_F32) return fail(AAA_E_ARG, "%s: fp32 weights only (bf16 agents use aaa_forward)", who);
  if (L.sc && !core) return fail(AAA_E_ARG, "actor_step: the stateful policy core uses aaa_actor_step_core");
  if (!L.sc && core) return fail(AAA_E_ARG, "actor_step_core: cfg lacks AAA_FLAG_STATEFUL_CORE (use aaa_actor_step)");
  if (cfg->B > 16) return fail(AAA_E_ARG, "%s: B <= 16 (got %d); larger batches use aaa_forward", who, cfg->B);
  if (actor_chunks(L.P) > kActMaxChunks)
    return fail(AAA_E_ARG, "%s: a %dx%d grid exceeds the readout's %d position chunks; use aaa_forward", who,
                L.h, L.w, kActMaxChunks);
  const size_t B = cfg->B, P = L.P;
  const size_t nt = 8 * (size_t)actor_pix_tiles(L.P), nch = actor_chunks(L.P), nq = L.nq;
  const size_t qc = core ? 1 : 0;
  const size_t sz[kActRegions] = {B * P * 64 * 4, B * P * 128 * 4, B * 512 * 4, B * 256 * 4, B * 256 * 4,
                                  B * nt * kActLstmKS * 4096 * 4, (B * nt + B + 1) * 4, B * P * nq * 4,
                                  B * nch * nq * kAttnPart * 4, B * (size_t)L.ans_ld * 4,
                                  qc * B * L.qd * 4, qc * B * 128 * 4, qc * B * L.qd * 4};
  size_t o = 0;
  for (int i = 0; i < kActRegions; ++i) { off[i] = o; o = al256(o + sz[i]); }
  if (bytes)
    for (int i = 0; i < kActRegions; ++i) bytes[i] = sz[i];
  *total = o;
  return AAA_OK;
}

size_t aaa_actor_workspace_bytes(const aaa_cfg* cfg) {
  Layout L;
  size_t off[kActRegions], tot = 0;
  return actor_layout(cfg, L, off, &tot) ? 0 : tot;
}

size_t aaa_actor_core_workspace_bytes(const aaa_cfg* cfg) {
  Layout L;
  size_t off[kActRegions], tot = 0;
  return actor_layout(cfg, L, off, &tot, true) ? 0 : tot;
}

// Checker-only view of that layout (include/aaa.h enum aaa_act_ws_region): the regions a stage hands to the next.
// Host arithmetic only; refused exactly where the step is (actor_layout), the layout chosen by the cfg's flag.
int aaa_actor_workspace_region(const aaa_cfg* cfg, int region, size_t* offset, size_t* bytes) {
  if (!cfg || !offset || !bytes) return fail(AAA_E_ARG, "actor_workspace_region: NULL argument");
  static const int slot[] = {0, 1, 2, 3, 4, 7, 9, 10, 11, 12};   // AAA_ACT_WS_X .. _Q2 -> actor_layout's off[]
  const bool core = (cfg->flags & AAA_FLAG_STATEFUL_CORE) != 0;
  Layout L;
  size_t off[kActRegions], sz[kActRegions], tot = 0;
  if (int r = actor_layout(cfg, L, off, &tot, core, sz)) return r;
  if (region < AAA_ACT_WS_X || region > AAA_ACT_WS_Q2 || (region >= AAA_ACT_WS_QT && !core))
    return fail(AAA_E_ARG, "actor_workspace_region: region %d not computed by this cfg", region);
  *offset = off[slot[region]];
  *bytes = sz[slot[region]];
  return AAA_OK;
}

static int actor_step_impl(const aaa_cfg* cfg, const aaa_actor_io* io, const aaa_actor_core_io* core, bool is_core,
                           hipStream_t stream) {
  Layout L;
  size_t off[kActRegions], tot = 0;
  int r = actor_layout(cfg, L, off, &tot, is_core);
  if (r) return r;
  const char* who = is_core ? "actor_step_core" : "actor_step";
  if (!io || !io->params || !io->packed || !io->basis || !io->frames || !io->h || !io->c || !io->logits ||
      !io->values || !io->workspace)
    return fail(AAA_E_ARG, "%s: NULL argument", who);
  if (is_core && (!core || !core->core_h || !core->core_c))
    return fail(AAA_E_ARG, "actor_step_core: NULL core state (core, core_h and core_c are required)");
  if (!aligned16(io->packed) || !aligned16(io->basis) || !aligned16(io->h) || !aligned16(io->c) ||
      !aligned16(io->workspace) || !aligned16(io->params))
    return fail(AAA_E_ALIGN, "%s: params, packed, basis, h, c and workspace must be 16-byte aligned", who);
  if (is_core && (!aligned16(core->core_h) || !aligned16(core->core_c) || !aligned16(core->core_h_out)))
    return fail(AAA_E_ALIGN, "actor_step_core: core_h, core_c and core_h_out must be 16-byte aligned");
  if ((r = check_device())) return r;
  const char* pk = (const char*)io->packed;
  const float* prm = io->params;
  char* ws = (char*)io->workspace;
  ActorParams p;
  p.B = L.B; p.H = L.H; p.W = L.W; p.H1 = L.H1; p.W1 = L.W1; p.h = L.h; p.w = L.w; p.P = L.P;
  p.nq = L.nq; p.A = L.A; p.ldy = L.ldy; p.ans_in = L.ans_in; p.ans_ld = L.ans_ld; p.u8 = L.fu8;
  p.frames = io->frames; p.basis = io->basis; p.prev_reward = io->prev_reward; p.prev_action = io->prev_action;
  p.Wp1 = (const float*)(pk + L.k_Wp1); p.b1 = prm + L.poff[C0B];
  p.Wp2 = (const float*)(pk + L.k_Wp2); p.b2 = prm + L.poff[C1B];
  p.WpXH = (const float*)(pk + L.k_WpXH); p.bl = (const float*)(pk + L.k_bl);
  p.Q = (const float*)(pk + L.k_Q); p.q_stride = 0;
  p.W1p = (const float*)(pk + L.k_W1p); p.a0b = prm + L.poff[A0B];
  p.A2W = prm + L.poff[A2W]; p.a2b = prm + L.poff[A2B];
  p.Wihp = (const float*)(pk + L.k_Wihp); p.blc = (const float*)(pk + L.k_blc);
  p.Whd = (const float*)(pk + L.k_Whd); p.bhd = (const float*)(pk + L.k_bhd);
  p.hst = io->h; p.cst = io->c; p.logits = io->logits; p.values = io->values; p.attn = io->attn;
  p.gates = io->gates;
  p.hout = io->h_out; p.cout = io->c_out;
  p.X = (float*)(ws + off[0]); p.Hs = (float*)(ws + off[1]); p.hid1 = (float*)(ws + off[2]);
  p.AO = (float*)(ws + off[3]); p.LH = (float*)(ws + off[4]);
  p.Zp = (float*)(ws + off[5]); p.zcnt = (int*)(ws + off[6]);
  p.Lg = (float*)(ws + off[7]); p.Apart = (float*)(ws + off[8]); p.arow = (float*)(ws + off[9]);
  p.seed = io->seed; p.counter = io->counter; p.actions = io->actions; p.logp = io->logp; p.jac = io->dlogp_dlogits;
  p.core_h = p.core_c = p.core_h_out = p.core_c_out = p.query_out = nullptr;
  p.Q0W = p.Q0B = p.Q2W = p.Q2B = p.Q4W = p.Q4B = p.Wihhp = nullptr;
  p.Qt = p.q1 = p.q2 = nullptr;
  if (is_core) {
    p.core_h = core->core_h; p.core_c = core->core_c; p.core_h_out = core->core_h_out; p.core_c_out = core->core_c_out;
    p.query_out = core->query;
    p.Q0W = prm + L.poff[Q0W]; p.Q0B = prm + L.poff[Q0B]; p.Q2W = prm + L.poff[Q2W]; p.Q2B = prm + L.poff[Q2B];
    p.Q4W = prm + L.poff[Q4W]; p.Q4B = prm + L.poff[Q4B];
    p.Wihhp = (const float*)(pk + L.k_Wihhp);
    p.Qt = (float*)(ws + off[10]); p.q1 = (float*)(ws + off[11]); p.q2 = (float*)(ws + off[12]);
    p.Q = p.Qt; p.q_stride = L.qd;
  }
  HIPCHK(actor_launch(p, stream));
  return AAA_OK;
}

int aaa_actor_step(const aaa_cfg* cfg, const aaa_actor_io* io, hipStream_t stream) {
  return actor_step_impl(cfg, io, nullptr, false, stream);
}

int aaa_actor_step_core(const aaa_cfg* cfg, const aaa_actor_io* io, const aaa_actor_core_io* core,
                        hipStream_t stream) {
  return actor_step_impl(cfg, io, core, true, stream);
}

}  // extern "C"
