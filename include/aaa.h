/*
 * aaa.h -- C ABI of the MI355X (gfx950) attention-augmented-agent learner.
 *
 * One shared library (libaaa.so, built by hipcc --offload-arch=gfx950) that
 * replaces the ATen op sequence of the reference's batched unroll: the
 * forward of Agent (reference attention.py:298-368, including
 * VisionNetwork.forward :178-181, ConvLSTMCell.forward :110-126,
 * QueryNetwork :184-198, SpatialBasis.__call__ :228-232, spatial_softmax
 * :235-243, apply_alpha :246-254) over T steps from reset() (:293-296), and
 * the backward that autograd runs for it when main_mp.py:77 calls
 * policy_loss.backward().
 *
 * Conventions
 *  - All pointers are DEVICE pointers on the caller's current HIP device,
 *    except the cfg/io structs themselves (host memory).
 *  - Ownership: the caller owns every buffer (params, packed weights,
 *    workspace, outputs).  The library never allocates or frees device
 *    memory and keeps no device state.
 *  - Streams: all work is enqueued on ``stream``; nothing synchronises.
 *  - Errors: functions return 0 on success, a negative AAA_E* code
 *    otherwise; aaa_last_error() returns a thread-local message.
 *  - Threading: re-entrant; each call only touches the buffers it is given.
 *
 * Layouts
 *  - params / grads: the 34 reference state_dict tensors, fp32, concatenated
 *    in state_dict order (reference attention.py:257-291),
 *    each tensor in its PyTorch (contiguous) layout.  aaa_param_layout()
 *    returns the offsets.  nq != 4 uses the generalised query / answer widths
 *    (query 256->128->72nq->72nq, answer 256nq+2).
 *  - frames: (T, B, H, W, 3) NHWC raw pixels, fp32 (main_mp.py:53 casts the
 *    uint8 observation to float without normalisation) or the uint8
 *    observation itself (AAA_FLAG_FRAMES_U8).
 *  - basis: (h, w, 64) fp32 spatial basis (SpatialBasis.S, attention.py:226).
 *  - logits, values: (T, B, A) fp32; attn: (T, B, h, w, nq) fp32 softmax maps.
 *  - prev_reward / prev_action: (T, B) fp32 or NULL (zeros, :303-312).
 *  - ConvLSTM state h0, c0, hT, cT, dh0, dc0, dhT, dcT: (B, h, w, 128) fp32
 *    NHWC (the reference keeps (B,128,w,h)), NULL = zero /
 *    not requested.
 */
#ifndef AAA_H
#define AAA_H

#include <stddef.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAA_ABI_VERSION 12

enum aaa_status {
  AAA_OK = 0,
  AAA_E_ARG = -1,      /* bad shape / NULL / unsupported configuration */
  AAA_E_ALIGN = -2,    /* a buffer is not 16-byte aligned */
  AAA_E_LAUNCH = -3,   /* a HIP launch or runtime call failed */
  AAA_E_DEVICE = -4,   /* current device is not gfx950 */
  AAA_E_STRANDED = -5  /* a paired frame-resident kernel of an EARLIER call timed out
                          waiting for its partner workgroup: that call's outputs are
                          invalid (reported once, by the next call or aaa_pair_status) */
};

enum aaa_dtype {
  AAA_F32 = 0,   /* conv/ConvLSTM GEMM operands fp32 (exact v_mfma_f32_32x32x2_f32) */
  AAA_BF16 = 1   /* conv/ConvLSTM GEMM operands bf16, fp32 accumulate + gate math */
};

typedef struct aaa_cfg {
  int B;        /* sequences (batch rows)                                    */
  int T;        /* unroll length (steps since reset())                        */
  int H, W;     /* frame size, e.g. 84x84, 168x168, 210x160                    */
  int nq;       /* attention queries (reference: 4, attention.py:265)          */
  int A;        /* actions (Seaquest: 18, main_mp.py:179)                       */
  int dtype;    /* enum aaa_dtype                                             */
  int flags;    /* AAA_FLAG_* (0: the reference's reachable path)             */
} aaa_cfg;

/* Stateful policy core: the reference's `else` branch (attention.py:356-358),
 * taken when agent.prev_hidden holds a tensor -- the query is computed from
 * prev_output = h_{t-1} and the LSTMCell runs from (h_{t-1}, c_{t-1}), both
 * carried across steps (and across calls through io->core_*).  Off, the
 * reference's reachable path: zero query input, zero-state LSTMCell (Q1). */
#define AAA_FLAG_STATEFUL_CORE 1
/* io->frames holds uint8 pixels (T, B, H, W, 3) -- the environment's
 * observation (main_mp.py:49-53 casts it to float on the host); the cast is
 * fused into the kernel that lays the frames out for conv1. */
#define AAA_FLAG_FRAMES_U8 2
/* Do not consume / fail on partner-timeout reports of earlier launches at
 * entry (see aaa_pair_status): the caller checks them itself after the
 * iteration, e.g. through aaa_pair_flag and the guarded optimizer. */
#define AAA_FLAG_DEFER_STRANDED 4
/* (8 is not a flag: it stays refused.)
 * bf16 cfgs: episode-start masks (aaa_forward_resets / aaa_backward_resets).
 * The workspace grows by one region appended behind every other,
 * AAA_BF16_WS_HR: (T, B, P, 128) bf16, h_t as the attention readout reads it
 * under a mask -- the h half of XH slot t+1 then holds zeros for the rows that
 * start an episode at step t+1, which is the operand the next step's conv and
 * the weight gradient read.  Packed bytes, regions 0..29 and aaa_core_layout
 * are what they are without the flag, and a call without a mask launches
 * exactly what the unflagged cfg launches (the readout reads XH; HR stays
 * unwritten).  Accepted and without effect on an fp32 cfg. */
#define AAA_FLAG_BF16_RESETS 16

typedef struct aaa_io {
  /* inputs */
  const float* params;       /* flat fp32 params (state_dict order)            */
  const void* packed;        /* aaa_pack_weights output                        */
  const float* basis;        /* (h, w, 64)                                     */
  const void* frames;        /* (T, B, H, W, 3) fp32, or uint8 with AAA_FLAG_FRAMES_U8 */
  const float* prev_reward;  /* (T, B) or NULL                                 */
  const float* prev_action;  /* (T, B) or NULL                                 */
  const float* h0;           /* (B, h, w, 128) or NULL                         */
  const float* c0;           /* (B, h, w, 128) or NULL                         */
  /* forward outputs */
  float* logits;             /* (T, B, A)                                      */
  float* values;             /* (T, B, A)                                      */
  float* attn;               /* (T, B, h, w, nq) or NULL                       */
  float* hT;                 /* (B, h, w, 128) or NULL                         */
  float* cT;                 /* (B, h, w, 128) or NULL                         */
  /* backward inputs */
  const float* dlogits;      /* (T, B, A)                                      */
  const float* dvalues;      /* (T, B, A) or NULL                              */
  const float* dhT;          /* (B, h, w, 128) or NULL                         */
  const float* dcT;          /* (B, h, w, 128) or NULL                         */
  /* backward outputs */
  float* grads;              /* flat fp32 grads, same layout as params         */
  float* dh0;                /* (B, h, w, 128) or NULL                         */
  float* dc0;                /* (B, h, w, 128) or NULL                         */
  /* scratch */
  void* workspace;           /* aaa_workspace_bytes(); activations saved by
                                aaa_forward for aaa_backward live here        */
  /* stateful policy core (AAA_FLAG_STATEFUL_CORE only; ignored otherwise):
     (B, 256) fp32 (prev_output, prev_hidden) in, out and their grads      */
  const float* core_h0;      /* or NULL (zeros: reset())                       */
  const float* core_c0;      /* or NULL                                        */
  float* core_hT;            /* or NULL                                        */
  float* core_cT;            /* or NULL                                        */
  const float* dcore_hT;     /* backward input or NULL                         */
  const float* dcore_cT;     /* backward input or NULL                         */
  float* dcore_h0;           /* backward output or NULL                        */
  float* dcore_c0;           /* backward output or NULL                        */
} aaa_io;

/* Backward phases, in execution order (DP bucket boundaries). */
enum aaa_bwd_phase {
  AAA_BWD_HEAD = 1,    /* heads, LSTMCell, answer MLP, attention, query MLP */
  AAA_BWD_CORE = 2,    /* ConvLSTM BPTT + ConvLSTM weight/bias grads         */
  AAA_BWD_VISION = 4,  /* conv2 / conv1 weight & bias grads                  */
  AAA_BWD_ALL = 7
};

int aaa_abi_version(void);
const char* aaa_last_error(void);

/* Spatial grid (h, w) the encoder produces for an H x W frame. */
int aaa_grid(int H, int W, int* h, int* w);

/* Number of fp32 params and the offset/size of each of the 34 tensors
 * (state_dict order).  offsets/sizes may be NULL. */
int aaa_param_layout(const aaa_cfg* cfg, size_t* total, size_t* offsets, size_t* sizes);

size_t aaa_packed_bytes(const aaa_cfg* cfg);
size_t aaa_workspace_bytes(const aaa_cfg* cfg);

/* Re-lay the params into the kernels' operand layouts (gate-interleaved
 * ConvLSTM / LSTMCell rows, NHWC tap-major conv weights with the
 * reference's transposed kernel orientation, bf16 when cfg->dtype says so).
 * Must run after every parameter update. */
int aaa_pack_weights(const aaa_cfg* cfg, const float* params, void* packed, hipStream_t stream);

/* T-step forward from reset(); replaces T calls of Agent.forward. */
int aaa_forward(const aaa_cfg* cfg, const aaa_io* io, hipStream_t stream);

/* Forward phases (aaa_forward_phases).  Skipping CORE leaves the ConvLSTM
 * recurrence out: its per-step products -- gate activations, c_t, h_t of
 * every step -- must already be in the workspace (aaa_core_import), as the
 * fused episode backward does with the products each per-step call of the
 * episode exported (episode.py).  VISION and TAIL always run. */
enum aaa_fwd_phase {
  AAA_FWD_VISION = 1,  /* conv1 + conv2 over all T*B frames                   */
  AAA_FWD_CORE = 2,    /* the ConvLSTM recurrence                             */
  AAA_FWD_TAIL = 4,    /* attention readout, answer MLP, LSTMCell, heads      */
  AAA_FWD_ALL = 7
};
/* aaa_forward with a phase mask: AAA_FWD_ALL, or AAA_FWD_VISION |
 * AAA_FWD_TAIL (configs whose slices are row-major: not the frame-resident
 * bf16 BPTT's channel-quad-major ones).  Replaces the recomputation half of the
 * reference's per-step graph (main_mp.py:54 -> attention.py:110-126). */
int aaa_forward_phases(const aaa_cfg* cfg, const aaa_io* io, int phases, hipStream_t stream);

/* The ConvLSTM products of steps [t0, t0+n) between an aaa_forward workspace
 * and flat buffers: gates (n, B*h*w, 512) post-activation (i, f, c~, o
 * interleaved per channel), c (n, B*h*w, 128) = c_t fp32, h (n, B*h*w, 128) =
 * h_t (pixel-major, channel fastest).  Element types (aaa_core_elem_bytes):
 * fp32 configs all fp32; bf16 configs gates in the workspace's gate storage
 * (fp16, or fp32 with AAA_GATES_F16=0) and h bf16 (the operand the next step
 * and the weight gradient read).  Export reads a workspace aaa_forward
 * filled; import writes one for aaa_forward_phases without CORE (and the h
 * half of the [x | h] operand slots).  Not for channel-quad-major slices
 * (large-batch bf16: AAA_E_ARG; aaa_core_elem_bytes reports 0 bytes for such
 * a geometry); device pointers, stream-ordered, no host sync. */
int aaa_core_elem_bytes(const aaa_cfg* cfg, int* gate_bytes, int* h_bytes);
int aaa_core_export(const aaa_cfg* cfg, const void* workspace, int t0, int n, void* gates, float* c, void* h,
                    hipStream_t stream);
int aaa_core_import(const aaa_cfg* cfg, void* workspace, int t0, int n, const void* gates, const float* c,
                    const void* h, hipStream_t stream);

/* Backward of the loss sum(logits*dlogits)+sum(values*dvalues) (+ state
 * cotangents) through the saved activations of the matching aaa_forward.
 * ``phases`` is a mask of aaa_bwd_phase; phases must run in order. grads
 * are overwritten (not accumulated) by the phases that own them. */
int aaa_backward(const aaa_cfg* cfg, const aaa_io* io, int phases, hipStream_t stream);

/* Episode starts inside an unroll (additive, no ABI bump: probe by name).
 * ``reset`` is a (T, B) fp32 mask in device memory, 16-byte aligned;
 * reset[t][b] != 0 means row b enters step t from the reset() state
 * (attention.py:142-149; the reference calls agent.reset() at every episode
 * start, main_mp.py:100): ConvLSTM (h, c) = 0, and with
 * AAA_FLAG_STATEFUL_CORE also the core's (h, c) = 0, so that step's query is
 * QueryNetwork(0).  reset[0][b] != 0 overrides h0 / c0 / core_h0 / core_c0 of
 * that row.  hT / cT and the saved h_t keep the true h_t: the readout of step
 * t-1 is unaffected by a reset at t.
 * A reset is a select, not a multiplication: nothing before it reaches
 * anything after it, NaN and inf included (aaa_vtrace makes the same promise
 * for ``done``).  The backward is the exact gradient of that forward: at a
 * reset step the carried c contributes nothing, no dh / dc / dcore flows from
 * step t to step t-1 of that row, dx of the reset step is still produced, the
 * row's weight-gradient term dZ_t (x) h_{t-1} is zero, and dh0 / dc0 /
 * dcore_h0 / dcore_c0 of a row with reset[0] are exactly 0.
 * The caller passes the SAME mask to both calls; the library keeps no state,
 * and the workspace layout and aaa_workspace_bytes do not change.
 * reset == NULL is exactly aaa_forward_phases / aaa_backward.
 * After the forward, AAA_WS_CORE_XH slot t holds zeros in the h half of the
 * rows with reset[t]: the operand the kernels really used.
 * Refused before the device is touched: AAA_E_ARG for a bf16 cfg without
 * AAA_FLAG_BF16_RESETS with a mask (its readout reads h_t from the [x | h]
 * operand slots, which a reset zeroes: set the flag, or cut bf16 unrolls at
 * episode ends) and for a forward phase mask without AAA_FWD_CORE together
 * with a mask; AAA_E_ALIGN for a mask that is not 16-byte aligned.
 * With a mask the production fp32 frame-group kernels run their mask
 * variants (forward: G = 8 pre-split and G = 4; BPTT: G = 8 with dx fused);
 * every other fp32 dispatch takes the per-step kernels.  The timer variants
 * of AAA_TIMER_FWD_STEP / AAA_TIMER_BPTT_STEP then end in ", resets".
 * bf16 with AAA_FLAG_BF16_RESETS: every h_t is also stored in AAA_BF16_WS_HR
 * slot t, bit for bit the value the next step's conv reads, and the readout
 * (forward and backward) reads it there.  A masked call runs the
 * single-workgroup frame-resident forward's mask variant where the forward's
 * rule gives one workgroup per frame, behind it the single-workgroup
 * frame-resident BPTT's mask variant where AAA_FRAMES_BWD's rule gives 1, and
 * the per-step kernels everywhere else: the paired and band-mode kernels are
 * never launched under a mask.  aaa_core_layout keeps describing the call
 * without a mask; a masked call keeps _C / _GATES / _DO row-major wherever
 * the plan sends its BPTT to the per-step chain (where the unmasked call
 * would run a paired or band-mode kernel, or AAA_FRAMES_BWD gives 0). */
int aaa_forward_resets(const aaa_cfg* cfg, const aaa_io* io, int phases, const float* reset, hipStream_t stream);
int aaa_backward_resets(const aaa_cfg* cfg, const aaa_io* io, int phases, const float* reset, hipStream_t stream);

/* Health of the multi-workgroup frame-resident ConvLSTM kernels (two or more
 * cooperating workgroups per frame: the paired and band-mode bf16 kernels and
 * the fp32 frame-group kernels, launched as ordinary grids that fit one
 * residency wave of an idle chip).  Their partner waits are bounded by a
 * deadline on the 100-MHz real-time counter (1 s + 20 ms per step after a
 * workgroup's first wait); a wait that expires is counted in a word of
 * pinned, device-mapped host memory and the kernel proceeds on a stale
 * partner slice (later waits of that workgroup return at once, so a kernel
 * whose partner never runs ends within about one budget).  The count is
 * monotonic; its two readers keep their own snapshots of it:
 *  - the host: aaa_forward / aaa_backward consume the counts reported since
 *    the host last did and return AAA_E_STRANDED -- unless the cfg carries
 *    AAA_FLAG_DEFER_STRANDED, for a caller that must not fail mid-iteration
 *    (a data-parallel learner whose peers would wait in a collective) and
 *    checks with aaa_pair_status after it; aaa_pair_status synchronises
 *    ``stream`` (NULL: the device) and returns that count (>= 0; clear != 0
 *    consumes it);
 *  - the device: aaa_pair_flag enqueues on ``stream`` a kernel that writes
 *    into dst[0], as a float, the counts reported since the previous
 *    aaa_pair_flag on this device, in stream order.  A learner puts it beside
 *    its gradients so the gradient all-reduce carries it to every rank and
 *    aaa_adam_step_counted / _guarded skips the update of a step whose
 *    gradients came from a stranded launch, with no host sync; host-side
 *    consumption never resets what the device-side reader sees. */
int aaa_pair_status(hipStream_t stream, int clear);
int aaa_pair_flag(float* dst, hipStream_t stream);
/* aaa_pair_flag_at (ABI 9): as aaa_pair_flag, but against the caller's own
 * snapshot ``base`` (one int of device memory the caller owns; the kernel
 * reads it, writes the count past it into dst[0] and advances it), so several
 * readers on one device -- two learners, a learner and a diagnostic -- never
 * take each other's timeouts.  A new reader syncs its base to the current
 * report word with one call whose dst it discards. */
int aaa_pair_flag_at(float* dst, int* base, hipStream_t stream);

/* ---- workspace inspection (checkers, diagnostics) ----
 * Byte offset and size, inside an aaa_forward workspace laid out for ``cfg``,
 * of a forward product a checker may read after the call (the workspace is
 * caller-owned device memory; nothing here syncs or copies):
 *   AAA_WS_ANSWER_HIDDEN  (T*B, 512) fp32: relu(answer_processor.0(answer)),
 *                         attention.py:277-282 -- its > 0 pattern is the
 *                         ReLU mask the hand-written backward applies;
 *   AAA_WS_QUERY_HIDDEN0  (T*B, 128) fp32: relu(query.model.0(h_{t-1})),
 *   AAA_WS_QUERY_HIDDEN1  (T*B, 72 nq) fp32: relu(query.model.2(.)), the
 *                         stateful core's query MLP (attention.py:184-198);
 *                         AAA_FLAG_STATEFUL_CORE only.
 * Frame f = t*B + b.  A test reads these masks to run the oracle's backward
 * through the same ReLU on/off pattern (tests/helpers.py hip_relu_masks).
 * ABI 11, fp32 configs only (bf16 and channel-quad-major geometries: AAA_E_ARG,
 * as aaa_core_export): the operands and cotangents of the fp32 ConvLSTM GEMMs,
 * read-only, M = B*h*w pixel rows per step, pixel-major, channel fastest:
 *   AAA_WS_CORE_XH        (T+1, M, 192) fp32: slot t = [x_t | h_{t-1}], the
 *                         recurrence's and the weight gradient's operand
 *                         (slot T holds h_{T-1} only; after
 *                         aaa_forward_resets the h half of slot t holds
 *                         zeros in the rows with reset[t], the operand the
 *                         kernels really used);
 *   AAA_WS_CORE_DO        (T, M, 128) fp32: the readout's cotangent of h_t,
 *                         valid after AAA_BWD_HEAD;
 *   AAA_WS_CORE_DX        (T, M, 64) fp32: the cotangent of conv2's output
 *                         x_t, valid after AAA_BWD_CORE.
 * With aaa_core_export's gates / c_t / h_t these are everything a checker
 * needs to evaluate the recurrence and its BPTT in fp64 on the kernels' own
 * inputs (tests/f32_split_ref.py, tests/test_gpu_f32_split.py).
 * ABI 12, every cfg (these buffers are fp32 in both dtypes and every geometry):
 * the operands, products and cotangents of the policy tail's GEMMs (everything
 * after the ConvLSTM), read-only, F = T*B rows, frame f = t*B + b.  Each is a
 * buffer of its own that no phase reuses, so with AAA_WS_ANSWER_HIDDEN and the
 * two AAA_WS_QUERY_HIDDEN* a checker evaluates every tail layer in fp64 on the
 * input the kernel really read (tests/tail_ref.py, tests/test_gpu_tail.py).
 * Valid after the forward:
 *   AAA_WS_TAIL_ANS       (F, ans_ld) fp32: the answer row, answer_processor.0's
 *                         operand; ans_ld = 256 nq + 2 rounded up to 8, the
 *                         padding columns zero;
 *   AAA_WS_TAIL_GATES     (F, 1024) fp32: the policy core's gate activations,
 *                         column 4u + g, g = (i, f, c~, o);
 *   AAA_WS_TAIL_AO        (F, 256) fp32: answer_processor.2's output,
 *   AAA_WS_TAIL_C, _H     (F, 256) fp32: the zero-state cell's c and h
 *                         (configs without AAA_FLAG_STATEFUL_CORE);
 *   AAA_WS_TAIL_AOX       (F, 512) fp32: the [answer | h_{t-1}] rows the stateful
 *                         LSTMCell GEMM reads (after aaa_forward_resets: zeros in
 *                         the h half of the rows with reset[t]),
 *   AAA_WS_TAIL_CH, _CC   (T+1, B, 256) fp32: slot t = (h, c) entering step t,
 *                         slot 0 the incoming core state,
 *   AAA_WS_TAIL_QUERY     (F, 72 nq) fp32: the per-frame queries
 *                         (AAA_FLAG_STATEFUL_CORE only).
 * Valid after AAA_BWD_HEAD:
 *   AAA_WS_TAIL_DY        (F, ldy) fp32: [dlogits | dvalues] concatenated,
 *                         ldy = 2A rounded up to 4, the padding columns zero;
 *   AAA_WS_TAIL_DGATES    (F, 1024) fp32: the gate pre-activations' cotangent;
 *   AAA_WS_TAIL_DHID      (F, 512) fp32: answer_processor.0's pre-activation
 *                         cotangent (through the ReLU mask);
 *   AAA_WS_TAIL_DANS      (F, 184 nq | 256 nq stateful) fp32: the answer row's
 *                         cotangent, the columns the readout backward reads;
 *   AAA_WS_TAIL_DAO       (F, 256) fp32: answer_processor.2's output cotangent
 *                         (configs without AAA_FLAG_STATEFUL_CORE);
 *   AAA_WS_TAIL_DAOX      (F, 512) fp32: the [answer | h_{t-1}] rows' cotangent
 *                         (the h half: the recurrent path only),
 *   AAA_WS_TAIL_DQUERY, _DQ2, _DQ1  (F, 72 nq | 72 nq | 128) fp32: the cotangents
 *                         of the queries and of the query MLP's two hidden
 *                         pre-activations (AAA_FLAG_STATEFUL_CORE only).
 * Not exposed: the stateful core's state carries dh, dc (one (B, 256) buffer
 * each, rewritten by every step of the phase that produces them).  A checker
 * reaches them through the next product: step t's carry dh is query.model.0's
 * dgrad of step t+1's _DQ1 rows plus the h half of its _DAOX rows, and step t's
 * _DGATES rows are checked from there.  The packed gradient accumulators are
 * not exposed either: the HEAD phase unpacks every one of them into ``grads``.
 * Added after ABI 12 without a bump (additive: probe aaa_core_layout by name),
 * bf16 configs only (fp32 configs: AAA_E_ARG; they have AAA_WS_CORE_* and
 * aaa_core_export): the bf16 ConvLSTM recurrence's buffers exactly as the
 * kernels store them, read-only, each a buffer of its own that no later phase
 * reuses, M = B*h*w pixel rows per step, P = h*w per frame, frame b of step t
 * at rows t*M + b*P ..:
 *   AAA_BF16_WS_XH     (T+1, M, 192) bf16, row-major: slot t = [x_t | h_{t-1}],
 *                      slot 0's h half the incoming h0 rounded to bf16, slot
 *                      t+1's h half h_t (the only stored copy); after the forward;
 *   AAA_BF16_WS_C      (T+1, M, 128) fp32: slot s+1 = c_s, slot 0 = c0; after
 *                      the forward;
 *   AAA_BF16_WS_GATES  (T, M, 512) post-activation gates in the gate storage
 *                      type (aaa_core_layout: fp16, or fp32); after the forward;
 *   AAA_BF16_WS_DO     (T, M, 128) fp32: the readout's cotangent of h_t; after
 *                      AAA_BWD_HEAD (aaa_backward_resets with a mask on the
 *                      per-step BPTT chain: its AAA_BWD_CORE then leaves the
 *                      raw dgrad dh_{t-1} in slots t >= 1, each consumed
 *                      before it is overwritten);
 *   AAA_BF16_WS_DZ     (T, M, 512) bf16, row-major, column 4*ch + gate: the gate
 *                      pre-activations' cotangent dZ_t, the dgrad's and the
 *                      weight gradient's operand; after AAA_BWD_CORE;
 *   AAA_BF16_WS_DX     (T, M, 64) bf16, row-major: the cotangent of conv2's
 *                      output x_t; after AAA_BWD_CORE;
 *   AAA_BF16_WS_HR     (T, M, 128) bf16, row-major: h_t as the readout reads it
 *                      under an episode-start mask; AAA_FLAG_BF16_RESETS only
 *                      (AAA_E_ARG without it), the last region of the
 *                      workspace, written by aaa_forward_resets with a mask.
 * aaa_core_layout reports the gate storage size in bytes (2 or 4) and which of
 * _C / _GATES / _DO keep their slices channel-quad-major: bit 0 (1) _C, bit 1
 * (2) _GATES, bit 2 (4) _DO; 0 = all row-major (pixel-major, channel fastest;
 * gates column 4*ch + gate, gate = i, f, c~, o), which is exactly where
 * aaa_core_elem_bytes reports non-zero sizes.  A channel-quad-major buffer
 * keeps every (step, frame) slice of P pixels at its row-major position and
 * size and permutes only the inside of that slice -- per frame, not per step:
 * element (pixel pp of the frame, channel ch[, gate]) of the slice sits at
 *   ((ch >> 2) * P + pp) * 4 + (ch & 3)                  _C, _DO (fp32 elements)
 *   ((ch >> 2) * P + pp) * 16 + (ch & 3) * 4 + gate      _GATES (gate elements)
 * (tests/convlstm_bf16_ref.py de-permutes with these on the host;
 * tests/test_gpu_convlstm_bf16.py).
 * AAA_E_ARG for an unknown region or one the cfg does not compute. */
enum aaa_ws_region {
  AAA_WS_ANSWER_HIDDEN = 0, AAA_WS_QUERY_HIDDEN0 = 1, AAA_WS_QUERY_HIDDEN1 = 2,
  AAA_WS_CORE_XH = 3, AAA_WS_CORE_DO = 4, AAA_WS_CORE_DX = 5,
  AAA_WS_TAIL_ANS = 6, AAA_WS_TAIL_GATES = 7, AAA_WS_TAIL_AO = 8, AAA_WS_TAIL_C = 9, AAA_WS_TAIL_H = 10,
  AAA_WS_TAIL_AOX = 11, AAA_WS_TAIL_CH = 12, AAA_WS_TAIL_CC = 13, AAA_WS_TAIL_QUERY = 14,
  AAA_WS_TAIL_DY = 15, AAA_WS_TAIL_DGATES = 16, AAA_WS_TAIL_DHID = 17, AAA_WS_TAIL_DANS = 18,
  AAA_WS_TAIL_DAO = 19, AAA_WS_TAIL_DAOX = 20, AAA_WS_TAIL_DQUERY = 21, AAA_WS_TAIL_DQ2 = 22,
  AAA_WS_TAIL_DQ1 = 23,
  AAA_BF16_WS_XH = 24, AAA_BF16_WS_C = 25, AAA_BF16_WS_GATES = 26, AAA_BF16_WS_DO = 27, AAA_BF16_WS_DZ = 28,
  AAA_BF16_WS_DX = 29,
  AAA_BF16_WS_HR = AAA_BF16_WS_DX + 1   /* 30: not one of the six checker regions above (AAA_FLAG_BF16_RESETS) */
};
int aaa_workspace_region(const aaa_cfg* cfg, int region, size_t* offset, size_t* bytes);
int aaa_core_layout(const aaa_cfg* cfg, int* gate_bytes, int* cqm_mask);

/* ---- optional kernel timing (benchmarks) ----
 * While enabled, the runtime records a hipEvent pair on the launch stream
 * around every launch of the kernel classes below.  aaa_timing_read()
 * waits for the recorded events and returns the summed device time and the
 * number of launches since the last enable/read, then clears that class. */
enum aaa_timer {
  AAA_TIMER_FWD_STEP = 0,    /* fused ConvLSTM forward step (one per t)          */
  AAA_TIMER_BPTT_STEP = 1,   /* ConvLSTM dgrad + fused gate backward (one per t) */
  AAA_TIMER_CORE_WGRAD = 2,  /* ConvLSTM weight-gradient GEMM over all frames    */
  AAA_TIMER_ATTN_FWD = 3,    /* fused spatial-softmax attention readout (HBM)    */
  AAA_TIMER_ATTN_BWD = 4,    /* its backward (HBM)                               */
  /* the rest of a learner iteration, so the classes cover the whole step
     (work in FLOP where a GEMM dominates, 0 for the latency-bound glue):     */
  AAA_TIMER_PACK = 5,        /* aaa_pack_weights (all packed layouts)            */
  AAA_TIMER_VISION_FWD = 6,  /* frames -> conv1 -> conv2 (the vision encoder)    */
  AAA_TIMER_TAIL_FWD = 7,    /* query pack, answer MLP, LSTMCell, heads          */
  AAA_TIMER_TAIL_BWD = 8,    /* their backward (HEAD phase minus the attention)  */
  AAA_TIMER_CORE_DX = 9,     /* batched conv2-output grad dx (when not fused)    */
  AAA_TIMER_VISION_BWD = 10, /* conv2 wgrad + dgrad, conv1 wgrad, grad unpack    */
  AAA_TIMER_MISC = 11,       /* state copies, memsets, bias column sums          */
  AAA_TIMER_N = 12
};
int aaa_timing_enable(int on);
int aaa_timing_read(int kind, double* total_ms, long* launches);
/* The same read with the roofline inputs the runtime knows: the summed
 * algorithmic work of those launches (FLOP for the MFMA classes 0-2 and 6-10:
 * 2*M*N*K of each GEMM; bytes for the HBM classes 3-4: the fp32 tensors each
 * frame must move; 0 for 5 and 11) and the kernel variant (tile / ring)
 * dispatched last.  A "launch" of classes 5-11 is one timed region (a group
 * of consecutive kernels of that class).
 * ABI 12: the variant of classes 7 and 8 ends with " | " and the kernel and
 * arithmetic of every tail GEMM launched since the class was last read, in
 * launch order, equal neighbours counted: "skinny8*18, CFK4/S6",
 * "CFK4/S3 x2, CFK4/S3, CF/S3 x3" (skinny1 / skinny8: k_skinny_gemm<EP, 1 / 8>;
 * CFK4, CF: the 32x64 4-way split-K and the 64x64 tile; f32 / S3 / S6: the
 * fp32 MFMA, GemmCfgS3, GemmCfgS6; xN: N split-K slices summed by atomics). */
typedef struct aaa_timer_stats {
  double total_ms;
  long launches;
  double work;
  char variant[192];
} aaa_timer_stats;
int aaa_timing_stats(int kind, aaa_timer_stats* out);

/* ---- optimizer ----
 * One fused multi-tensor Adam step with torch.optim.Adam semantics (the
 * reference's optimizer: main_mp.py:92 builds Adam(policy.parameters(),
 * lr=1e-3), main_mp.py:78 steps it).  ``step`` is the step count after this
 * update (1 on the first call).  Tensor i has numel[i] fp32 elements at
 * params[i] / grads[i] / exp_avg[i] / exp_avg_sq[i] (and max_exp_avg_sq[i]
 * when amsgrad; the array may be NULL otherwise), all updated in place on
 * ``stream``.  The pointer arrays are host memory; the tensors are device
 * memory.  A flat parameter buffer is simply ntensors = 1. */
typedef struct aaa_adam_hparams {
  double lr, beta1, beta2, eps, weight_decay;
  int amsgrad, maximize;
} aaa_adam_hparams;

int aaa_adam_step(const aaa_adam_hparams* hp, long step, int ntensors, float* const* params,
                  const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  float* const* max_exp_avg_sq, const size_t* numel, hipStream_t stream);
/* The same update, skipped on the device when *guard != 0 (guard: one
 * device float, e.g. the all-reduced aaa_pair_flag slot of the gradients):
 * no parameter or moment is written and no host sync is needed. */
int aaa_adam_step_guarded(const aaa_adam_hparams* hp, long step, const float* guard, int ntensors,
                          float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* numel,
                          hipStream_t stream);
/* The guarded update with the step count kept on the device: *step_dev (one
 * device int, 0 before the first update) is the number of updates applied so
 * far; this one runs as update *step_dev + 1 (torch's bias corrections of
 * that step, in double) and, in stream order after it, *step_dev advances
 * only if the guard let the update through -- so a skipped step leaves the
 * moments AND the bias corrections exactly where they were. */
int aaa_adam_step_counted(const aaa_adam_hparams* hp, int* step_dev, const float* guard, int ntensors,
                          float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* numel,
                          hipStream_t stream);

/* ---- gradient clipping by global norm (added after ABI 11 without a bump: additive, probe by name) ----
 * torch.nn.utils.clip_grad_norm_ (norm_type 2) on the device, with no host
 * read: aaa_grad_norm writes the total norm and the clip coefficient into
 * ``stats``; aaa_grad_scale applies the coefficient in place (the drop-in), or
 * aaa_adam_step_clipped folds it into the counted Adam update and skips the
 * update -- exactly as a non-zero guard does: no parameter or moment written,
 * *step_dev not advanced -- when a gradient element is inf or NaN.
 *
 * The squares are summed in double (the product of two fp32 values is exact
 * there) in a fixed order without atomics: the result is within N * 2^-53
 * relative of the exact sum for N elements, and identical buffers give
 * bit-identical stats, so the replicas of a data-parallel learner clip and
 * skip alike with no extra collective.
 *
 * stats: 4 floats of device memory, 16-byte aligned:
 *   [0] total 2-norm of all gradients: fp32 of sqrt(double sum of exact squares)
 *   [1] coefficient: fp32 of min(1, max_norm / (norm + 1e-6)) evaluated in double with IEEE
 *       semantics as torch.nn.utils.clip_grad_norm_ states it (NaN norm -> NaN, inf norm -> 0,
 *       max_norm = +inf -> 1: "norm only")
 *   [2] 1.0f when the norm is not finite -- which, the squares being summed in double, is
 *       exactly "some gradient element is inf or NaN" -- else 0.0f
 *   [3] max_norm as fp32 (echo, for logs)
 * The flag and the coefficient come from the double norm: finite gradients whose norm exceeds
 * FLT_MAX (two elements near 3e38, say) give [0] = +inf with [2] = 0 and a correct coefficient.
 * scratch: aaa_grad_norm_scratch_bytes() of device memory, 16-byte aligned
 * (one double per workgroup; needs no initialisation, and may be reused by
 * the next call on the same stream).  Tensor i has numel[i] fp32 elements at
 * grads[i]; the pointer arrays are host memory, as for aaa_adam_step.
 * ntensors = 0 or all-empty tensors give norm 0, coefficient 1, flag 0.
 * Refused before the device is touched: AAA_E_ARG for a NULL array, stats,
 * scratch or step_dev, a NULL tensor pointer with numel > 0, ntensors < 0,
 * max_norm NaN or <= 0 (+inf is allowed); AAA_E_ALIGN for a stats or scratch
 * pointer that is not 16-byte aligned.
 *
 * Call order on one stream: backward (and the gradient all-reduce) ->
 * aaa_grad_norm -> aaa_adam_step_clipped with the same stats (or
 * aaa_grad_scale, then any optimizer). */
size_t aaa_grad_norm_scratch_bytes(int ntensors, const size_t* numel);   /* 8 B per chunk, >= 16, multiple of 16 */
int aaa_grad_norm(double max_norm, int ntensors, const float* const* grads, const size_t* numel,
                  float* stats, void* scratch, hipStream_t stream);
/* grads[i] *= stats[1] (one fp32 multiply per element, as grad.mul_(coef));
 * nothing is written when stats[1] is exactly 1.0f. */
int aaa_grad_scale(const float* stats, int ntensors, float* const* grads, const size_t* numel, hipStream_t stream);
/* aaa_adam_step_counted on grads[i] * stats[1] (the fp32 product, then the
 * update unchanged), skipped and not counted when stats[2] != 0 or *guard != 0
 * (guard may be NULL).  With a coefficient of exactly 1.0f and weight_decay =
 * 0 the result is bit-identical to aaa_adam_step_counted. */
int aaa_adam_step_clipped(const aaa_adam_hparams* hp, int* step_dev, const float* guard, const float* stats,
                          int ntensors, float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* numel,
                          hipStream_t stream);

/* ---- RMSProp (added after ABI 11 without a bump: additive, probe by name) ----
 * One fused multi-tensor RMSProp step with torch.optim.RMSprop semantics
 * (torch's _single_tensor_rmsprop op order, fp32), the optimizer IMPALA trains
 * with: momentum 0, alpha 0.99, eps 0.01 or 0.1 inside the square root, and a
 * learning rate annealed linearly to 0.  Per element:
 *   g   = grads[i] * stats[1]   (only with stats: the fp32 product, then the update unchanged)
 *   g   = -g (maximize);  g = g + weight_decay * p (weight_decay != 0)
 *   v   = v * alpha;  v = v + (1 - alpha) * g * g
 *   centered:  a = a + (1 - alpha) * (g - a);  s = v - a * a     else  s = v
 *   avg = eps_in_sqrt ? sqrt(s + eps) : sqrt(s) + eps
 *   momentum > 0:  b = b * momentum + g / avg;  p = p - lr_t * b
 *   else:          p = p - lr_t * (g / avg)
 * eps_in_sqrt = 0 is torch's placement of eps, 1 is TensorFlow's (IMPALA's).
 * With momentum the buffer is torch's, with the learning rate outside it.
 *
 * lr_t = lr_end + (lr - lr_end) * max(0, 1 - n / anneal_steps), evaluated in
 * double and rounded to fp32 once, where n is the number of updates applied
 * before this one: *step_dev (one device int, as aaa_adam_step_counted keeps
 * it), or step - 1 when step_dev is NULL (``step`` is then the count after
 * this update, 1 on the first call, as for aaa_adam_step).  anneal_steps = 0
 * is a constant lr.  Both counts give the same lr_t bit for bit.
 *
 * The update is skipped on the device -- nothing written, *step_dev not
 * advanced, so the schedule stays where it was -- when *guard != 0 (guard may
 * be NULL) or when stats[2] != 0 (stats: aaa_grad_norm's, or NULL: no
 * clipping).  A coefficient stats[1] of exactly 1.0f is bit-identical to
 * stats = NULL.  In stream order after the update *step_dev advances by one
 * iff it was applied.
 *
 * Tensor i has numel[i] fp32 elements at params[i] / grads[i] / square_avg[i],
 * at momentum_buf[i] when momentum > 0 and at grad_avg[i] when centered; an
 * array that is not used may be NULL and is never read.  The pointer arrays
 * are host memory, the tensors device memory, all updated in place on
 * ``stream``.  ntensors = 0 or all-empty tensors launch no update and still
 * count the step when step_dev is set.
 * Refused before the device is touched (messages begin with "rmsprop"):
 * AAA_E_ARG for a NULL hp or required array, a NULL tensor pointer with numel
 * > 0, ntensors < 0, lr, lr_end, alpha, eps, weight_decay or momentum negative
 * or NaN, anneal_steps < 0, step < 1 with step_dev NULL; AAA_E_ALIGN for a
 * stats pointer that is not 16-byte aligned. */
typedef struct aaa_rmsprop_hparams {
  double lr, alpha, eps, weight_decay, momentum;
  double lr_end;
  long anneal_steps;   /* 0: constant lr */
  int centered, maximize, eps_in_sqrt;
} aaa_rmsprop_hparams;
int aaa_rmsprop_step(const aaa_rmsprop_hparams* hp, long step, int* step_dev, const float* guard,
                     const float* stats, int ntensors, float* const* params, const float* const* grads,
                     float* const* square_avg, float* const* momentum_buf, float* const* grad_avg,
                     const size_t* numel, hipStream_t stream);

/* ---- REINFORCE loss ----
 * finish_episode's loss (reference main_mp.py:62-77) for B independent
 * episodes of T steps, on device: discounted returns R_t = r_t + gamma R_{t+1}
 * (double, then fp32), normalised (R - mean) / (std_unbiased + FLT_EPSILON)
 * into returns_norm (T, B); loss[b] = sum_t -log pi(a_t) R^_t with pi =
 * Categorical(softmax(logits_t)) and its probability clamp to [eps, 1-eps]
 * (main_mp.py:55-58); dlogits (T, B, A) = d(sum_b loss[b]) / d logits, the
 * cotangent aaa_backward takes.  logits (T, B, A) fp32, actions (T, B) int32
 * in [0, A), rewards (T, B) fp32; every pointer is device memory. */
int aaa_reinforce(int T, int B, int A, const float* logits, const int* actions, const float* rewards, double gamma,
                  float* loss, float* returns_norm, float* dlogits, hipStream_t stream);

/* ---- V-trace actor-critic loss (added after ABI 11 without a bump: additive, probe by name) ----
 * The IMPALA loss for B unrolls of T steps cut out of longer episodes, on
 * device, in one launch: from the unroll's logits l and values v (T, B, A),
 * the actions a taken, the rewards r and the behaviour policy's log-probs
 * log mu of those actions (aaa_actor_step's logp), the cotangents dlogits and
 * dvalues (T, B, A) that aaa_backward takes.  The baseline is one column of
 * the A-wide value head, V_t = v[t][b][value_col]; every other column gets a
 * zero cotangent.  With log pi_t = log_softmax(l_t) (fp32, no clamp), p its
 * softmax and H_t = -sum_k p_k log pi_k:
 *   log rho_t = log pi_t[a_t] - log mu_t              (0 when behaviour_logp is NULL)
 *   rho_t = min(rho_bar, e^{log rho_t}),  c_t = lambda min(c_bar, e^{log rho_t}),
 *   rho^pg_t = min(pg_rho_bar, e^{log rho_t})
 *   gamma_t = gamma (1 - [done_t != 0])               (done_t: the episode ended with step t's transition)
 *   V_T = bootstrap[b]                                (0 when bootstrap is NULL)
 *   delta_t = rho_t (r_t + gamma_t V_{t+1} - V_t)
 *   x_t = delta_t + gamma_t c_t x_{t+1},  x_T = 0;    vs_t = V_t + x_t,  vs_T = V_T
 *   adv_t = rho^pg_t (r_t + gamma_t vs_{t+1} - V_t)
 *   L = scale sum_{t,b} [ -adv_t log pi_t[a_t] + baseline_cost (vs_t - V_t)^2 / 2 - entropy_cost H_t ]
 * with vs, adv and the ratios constants of the differentiation, so
 *   dlogits[t][b][k] = scale (-adv_t (1[k == a_t] - p_k) + entropy_cost p_k (log pi_k + H_t))
 *   dvalues[t][b][value_col] = -scale baseline_cost (vs_t - V_t),  0 in the other columns.
 * The recursion runs in double.  vs and pg_adv (T, B) receive vs_t and adv_t
 * when set; loss (B, 3) receives the raw per-row parts [sum_t -adv log pi[a],
 * sum_t (vs - V)^2 / 2, sum_t H] (accumulated in double, reduced in a fixed
 * order: no atomics), of which the caller forms scale (l0 + baseline_cost l1
 * - entropy_cost l2).  An action outside [0, A) reads nothing outside its row
 * and makes that row's outputs NaN.  A done inside the unroll cuts the return
 * only; aaa_forward carries the recurrent state across it, and
 * aaa_forward_resets / aaa_backward_resets (fp32; bf16 with
 * AAA_FLAG_BF16_RESETS) cut the state with the mask
 * reset[t] = done[t-1].  Every pointer is device memory; dlogits and dvalues
 * must be 16-byte aligned. */
typedef struct aaa_vtrace_desc {
  int T, B, A, value_col;
  double gamma, lambda, rho_bar, c_bar, pg_rho_bar, baseline_cost, entropy_cost, scale;
} aaa_vtrace_desc;
typedef struct aaa_vtrace_io {
  const float *logits, *values;                 /* (T, B, A) */
  const int* actions;                           /* (T, B) */
  const float *rewards, *behaviour_logp, *done; /* (T, B); the last two may be NULL */
  const float* bootstrap;                       /* (B) or NULL */
  float *dlogits, *dvalues;                     /* (T, B, A), every element written */
  float *vs, *pg_adv;                           /* (T, B) or NULL */
  float* loss;                                  /* (B, 3) or NULL */
} aaa_vtrace_io;
int aaa_vtrace(const aaa_vtrace_desc* d, const aaa_vtrace_io* io, hipStream_t stream);

/* ---- actor: action sampling ----
 * Policy.forward's draw (reference main_mp.py:54-58: F.softmax over the
 * logits, Categorical(probs).sample(), .log_prob(action)) for B rows of
 * logits (B, A) fp32, on device and without a host round trip: actions (B)
 * int32 by inverse-CDF sampling of softmax(logits) with a counter-based
 * uniform u = rng(seed, *counter, row) (splitmix64 finaliser, 24-bit);
 * logp (B) = log(clamp(p_a, FLT_EPSILON, 1 - FLT_EPSILON)) as Categorical
 * computes it; dlogp_dlogits (B, A) = 1[k == a] - p_k (0 where the clamp is
 * active), or NULL.  ``counter`` is a device uint64 advanced by one per call
 * (NULL = draw index 0), so a captured hipGraph replays fresh draws.  The
 * draws are not torch's multinomial stream; the distribution is the same. */
int aaa_sample_actions(int B, int A, const float* logits, unsigned long long seed, unsigned long long* counter,
                       int* actions, float* logp, float* dlogp_dlogits, hipStream_t stream);

/* ---- actor: one environment step ----
 * The acting half of the reference's loop -- Policy.forward (main_mp.py:49-59)
 * = Agent.forward (attention.py:298-368) on one observation per row, with the
 * ConvLSTM state carried (attention.py:125, 142-149), then the draw of
 * aaa_sample_actions -- for B <= 16 rows, as a chain of six launches sized for
 * small B (vision, ConvLSTM step, attention + answer layer 0, answer layer 2,
 * LSTMCell, heads + draw) instead of aaa_forward's whole-batch kernels.
 * Results equal aaa_forward with T = 1, h0 = *h, c0 = *c up to fp32
 * summation order; the draw is bit-identical to aaa_sample_actions on those
 * logits.  cfg: T = 1, dtype AAA_F32, no AAA_FLAG_STATEFUL_CORE (bf16 and
 * T > 1 use aaa_forward, the stateful core aaa_actor_step_core); ``packed`` from aaa_pack_weights with the same cfg.  h, c
 * (B, h, w, 128) are read and overwritten with the step's state (zero them for
 * reset()).  actions == NULL skips the draw (seed/counter/logp/dlogp ignored). */
typedef struct aaa_actor_io {
  const float* params;       /* flat fp32 params                               */
  const void* packed;        /* aaa_pack_weights output (same cfg)             */
  const float* basis;        /* (h, w, 64)                                     */
  const void* frames;        /* (B, H, W, 3) fp32, or uint8 with AAA_FLAG_FRAMES_U8 */
  const float* prev_reward;  /* (B) or NULL                                    */
  const float* prev_action;  /* (B) or NULL                                    */
  float* h;                  /* (B, h, w, 128) ConvLSTM state, in/out          */
  float* c;                  /* (B, h, w, 128) cell state, in/out              */
  float* logits;             /* (B, A)                                         */
  float* values;             /* (B, A)                                         */
  float* attn;               /* (B, h, w, nq) or NULL                          */
  void* workspace;           /* aaa_actor_workspace_bytes()                    */
  unsigned long long seed;   /* action draw: as aaa_sample_actions             */
  unsigned long long* counter;
  int* actions;              /* (B) or NULL (no draw)                          */
  float* logp;               /* (B) or NULL                                    */
  float* dlogp_dlogits;      /* (B, A) or NULL                                 */
  float* gates;              /* (B, h, w, 512) or NULL: the ConvLSTM step's gate
                                activations (i, f, c~, o), row 4*ch + gate -- the
                                products a fused episode backward imports
                                (aaa_core_import) instead of re-running the step */
  float* h_out;              /* (B, h, w, 128) or NULL: h_t written here instead of
                                over ``h`` (which is then only read)         */
  float* c_out;              /* (B, h, w, 128) or NULL: likewise c_t           */
} aaa_actor_io;
size_t aaa_actor_workspace_bytes(const aaa_cfg* cfg);
int aaa_actor_step(const aaa_cfg* cfg, const aaa_actor_io* io, hipStream_t stream);

/* ---- actor: one environment step, stateful policy core ----
 * aaa_actor_step for the agent of AAA_FLAG_STATEFUL_CORE (the reference's
 * `else` branch, attention.py:324-331, 356-358): this step's queries are
 * Q_t = QueryNetwork(core_h) (attention.py:184-198), one set per row, and the
 * LSTMCell runs from (core_h, core_c).  Seven launches: the first layer of the
 * query MLP, then the chain of aaa_actor_step with the MLP's other two layers
 * riding as extra workgroups of its vision and ConvLSTM launches, the readout
 * on per-row queries and the LSTMCell reading [answer | core_h] against
 * [W_ih | W_hh].
 * Results equal aaa_forward with the flag, T = 1, h0 = *h, c0 = *c,
 * core_h0 = *core_h, core_c0 = *core_c up to fp32 summation order; zeroing
 * all four states is reset().  The draw, gates, h_out / c_out, attn and the
 * uint8 / fp32 frames are as in aaa_actor_step.  cfg: T = 1, dtype AAA_F32,
 * B <= 16, AAA_FLAG_STATEFUL_CORE set; ``packed`` from aaa_pack_weights with
 * the same cfg; io->workspace of aaa_actor_core_workspace_bytes().  Anything
 * else is AAA_E_ARG (the workspace query returns 0), checked before the device
 * is touched.  params, packed, basis, h, c, workspace, core_h, core_c and a
 * non-NULL core_h_out must be 16-byte aligned (AAA_E_ALIGN).
 * These two symbols were added after ABI version 11 without a bump (the
 * change is purely additive): probe for them by name, not by version. */
typedef struct aaa_actor_core_io {
  float* core_h;             /* (B, 256) prev_output: read, and overwritten with
                                h_t unless core_h_out                          */
  float* core_c;             /* (B, 256) prev_hidden: likewise                 */
  float* core_h_out;         /* (B, 256) or NULL                               */
  float* core_c_out;         /* (B, 256) or NULL                               */
  float* query;              /* (B, nq, 72) or NULL: this step's Q_t (checkers) */
} aaa_actor_core_io;
size_t aaa_actor_core_workspace_bytes(const aaa_cfg* cfg);
int aaa_actor_step_core(const aaa_cfg* cfg, const aaa_actor_io* io, const aaa_actor_core_io* core,
                        hipStream_t stream);

/* ---- actor: a checker's view of the step's workspace (added after ABI 12 without a bump:
 * additive, probe by name) ----
 * Where the chain's stages hand their products to the next, inside the
 * workspace of aaa_actor_workspace_bytes() -- or, for a cfg with
 * AAA_FLAG_STATEFUL_CORE, of aaa_actor_core_workspace_bytes() -- as (offset,
 * bytes), valid after a step, all fp32, rows of frame b first:
 *   AAA_ACT_WS_X       (B, P, 64)   conv2's output, the ConvLSTM's x
 *   AAA_ACT_WS_HS      (B, P, 128)  h_t as the readout reads it
 *   AAA_ACT_WS_HID1    (B, 512)     relu(answer_processor.0)
 *   AAA_ACT_WS_AO      (B, 256)     answer_processor.2
 *   AAA_ACT_WS_LH      (B, 256)     the LSTMCell's h_t, the heads' input
 *   AAA_ACT_WS_LOGITS  (B, P, nq)   the attention logits K.Q
 *   AAA_ACT_WS_ANSWER  (B, ans_ld)  [readout | Q | prev_reward | prev_action | 0],
 *                                   ans_ld = 256 nq + 2 rounded up to 8
 *   AAA_ACT_WS_QT      (B, nq*72)   stateful core: this step's Q_t
 *   AAA_ACT_WS_Q1      (B, 128)     stateful core: relu(query.model.0)
 *   AAA_ACT_WS_Q2      (B, nq*72)   stateful core: relu(query.model.2)
 * Offsets are 256-byte aligned and the regions disjoint.  Touches no device.
 * AAA_E_ARG for every cfg the step itself refuses, for an unknown region and
 * for _QT / _Q1 / _Q2 on a cfg without the stateful core. */
enum aaa_act_ws_region {
  AAA_ACT_WS_X = 0, AAA_ACT_WS_HS = 1, AAA_ACT_WS_HID1 = 2, AAA_ACT_WS_AO = 3, AAA_ACT_WS_LH = 4,
  AAA_ACT_WS_LOGITS = 5, AAA_ACT_WS_ANSWER = 6, AAA_ACT_WS_QT = 7, AAA_ACT_WS_Q1 = 8, AAA_ACT_WS_Q2 = 9
};
int aaa_actor_workspace_region(const aaa_cfg* cfg, int region, size_t* offset, size_t* bytes);

/* ---- actor: recording unrolls (added after ABI 11 without a bump: additive, probe by name) ----
 * Two small calls around an actor step (aaa_actor_step, aaa_actor_step_core or
 * aaa_forward with T = 1) assemble the time-major unroll the learner trains
 * on, on the device: the frames, actions, behaviour log-probs, rewards and
 * done flags of T steps, which rows start an episode at step 0, and the
 * recurrent state BEFORE step 0 (aaa_io's h0 / c0 / core_h0 / core_c0).  The
 * write position is a device-side cursor ``pos``, so the arguments never
 * change from step to step and the calls can sit in a captured hipGraph with
 * the step between them: aaa_unroll_begin, the step, aaa_unroll_record.
 *
 * Consecutive unrolls share one step: step T-1 of an unroll is step 0 of the
 * next (its value is the bootstrap, bootstrap="last"), so unroll u holds the
 * environment steps u (T-1) .. u (T-1) + T-1, and two banks alternate.  With
 * t = pos[0] and k = pos[1] as read when the launch starts:
 *
 * aaa_unroll_begin, before the step:
 *   rows with done_in[b] != 0 get zeros written into h, c (core_h, core_c): a
 *   select, not a multiply -- a NaN state does not survive an episode end;
 *   t == 0:    the (post-reset) state of every row is copied into bank[k]'s
 *              h0 / c0 / core_h0 / core_c0 rows b0 + b, and
 *              first[b0 + b] = (done_in[b] != 0);
 *   t == T-1:  the same copy and ``first`` go to bank[1-k];
 *   otherwise  it only resets.
 * aaa_unroll_record, after the step:
 *   frame, actions and logp go to slot t of bank[k];
 *   t >= 1:    rewards[t-1] = clip(reward_in), done[t-1] = (done_in != 0);
 *   t == T-1:  slot 0 of bank[1-k] gets the frame, action and logp too,
 *              rewards[T-1] = done[T-1] = 0 in bank[k] (never read with
 *              bootstrap="last"; nothing is left uninitialised), and
 *              pos = [1, 1-k, pos[2] + 1, 0];
 *   otherwise  pos[0] = t + 1.
 * reward_in / done_in (B) are the result of the PREVIOUS step's action, as an
 * environment returns them with the observation of this step; done_in = 1 on
 * an episode's first step.  pos is 4 device ints [t, bank, unrolls completed,
 * 0]; all zero = start (and restart).  After n steps from a zero pos,
 * pos[2] = 0 for n < T, else 1 + (n - T) / (T - 1): a host can tell when an
 * unroll is complete without reading the device.  Unroll u is bank[u % 2]; it
 * is next written T-1 steps after it completed.
 *
 * Rows outside [b0, b0 + B) of the banks, and slots other than those named,
 * are never touched, so several actors fill disjoint row ranges of the same
 * banks, each with a pos of its own.  pos is read by every workgroup and
 * written by a trailing one-workgroup launch, in stream order after them.
 * Everything is enqueued on ``stream`` in order: no side stream, no host sync.
 * A pos outside its range (t not in [0, T), bank not 0 or 1) makes both calls
 * write nothing.  Frame rows move in 16-byte pieces when frame_bytes % 16 == 0
 * (84x84, 168x168 and 210x160 frames), else byte by byte; state rows always in
 * 16-byte pieces.
 * Refused before the device is touched (messages begin with "unroll"):
 * AAA_E_ARG for T < 2, B < 1, b0 < 0, b0 + B > Bu, frame_bytes == 0,
 * state_floats % 4 != 0, core not 0 or 256, reward_clip negative or NaN, a
 * NULL desc, io or pointer the call reads or writes (begin: pos, done_in, h,
 * c and both banks' first, h0, c0; record: pos, frame, actions, logp,
 * reward_in, done_in and both banks' frames, actions, logp, rewards, done;
 * core == 256 adds core_h, core_c and the banks' core_h0, core_c0 to begin);
 * AAA_E_ALIGN for a pos, live-state or bank-state pointer that is not 16-byte
 * aligned, or a frames / frame pointer that is not when frame_bytes % 16 == 0. */
typedef struct aaa_unroll_desc {
  int T;               /* steps per unroll, >= 2; consecutive unrolls share one step */
  int B;               /* rows this actor steps */
  int Bu, b0;          /* rows of the unroll buffers; this actor fills rows [b0, b0 + B) */
  size_t frame_bytes;  /* bytes of one row's observation (H*W*3 uint8) */
  size_t state_floats; /* floats of one row's ConvLSTM h (h*w*128); multiple of 4 */
  int core;            /* 0, or 256: floats per row of core_h / core_c */
  double reward_clip;  /* 0: rewards stored as given; c > 0: clamped to [-c, c] (NaN stays NaN) */
} aaa_unroll_desc;
typedef struct aaa_unroll_bank {   /* one unroll, the layouts the learner's V-trace step takes */
  void* frames;        /* (T, Bu, frame_bytes) uint8 */
  int* actions;        /* (T, Bu) */
  float *logp, *rewards, *done;   /* (T, Bu) */
  float* first;        /* (Bu): 1 where step 0 starts an episode */
  float *h0, *c0;      /* (Bu, state_floats): the state BEFORE step 0 */
  float *core_h0, *core_c0;       /* (Bu, core) or NULL when core == 0 */
} aaa_unroll_bank;
typedef struct aaa_unroll_io {
  aaa_unroll_bank bank[2];
  int* pos;            /* 4 device ints, 16-B aligned: [t, bank, unrolls completed, 0]; zero = start */
  const void* frame;   /* this step, (B, frame_bytes) */
  const int* actions;  /* (B) */
  const float* logp;   /* (B) */
  const float *reward_in, *done_in;  /* (B): result of the PREVIOUS step's action; done_in = 1 on an episode's first step */
  float *h, *c, *core_h, *core_c;    /* the actor's live state, (B, ...) */
} aaa_unroll_io;
int aaa_unroll_begin(const aaa_unroll_desc* d, const aaa_unroll_io* io, hipStream_t stream);   /* before the actor step */
int aaa_unroll_record(const aaa_unroll_desc* d, const aaa_unroll_io* io, hipStream_t stream);  /* after it */

/* ---- single-kernel entry points (unit tests against PyTorch fp32) ---- */

/* NHWC convolution y[n,oy,ox,co] = b[co] + sum w[co,ky,kx,ci] x[n,iy,ix,ci]
 * (weights in [Cout][KH][KW][Cin] order, i.e. torch weight.permute(0,2,3,1)).
 * dtype selects the MFMA operand type.  bias may be NULL. */
typedef struct aaa_conv_desc {
  int N, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, dtype;
} aaa_conv_desc;

int aaa_conv2d_nhwc(const aaa_conv_desc* d, const float* x, const float* w, const float* bias,
                    float* y, hipStream_t stream);
/* dx = conv2d_input(dy, w) (NHWC) */
int aaa_conv2d_nhwc_dgrad(const aaa_conv_desc* d, const float* dy, const float* w, float* dx,
                          hipStream_t stream);
/* dw[co][ky][kx][ci] = conv2d_weight(x, dy), overwritten */
int aaa_conv2d_nhwc_wgrad(const aaa_conv_desc* d, const float* x, const float* dy, float* dw,
                          hipStream_t stream);

/* C[m][n] = sum_k A[m][k] * Bw[n][k] (+ bias[n]) -- torch.nn.functional.linear */
int aaa_linear(int M, int N, int K, const float* x, const float* w, const float* bias, float* y,
               hipStream_t stream);

/* ---- component entry points ----
 * One reference module each, on caller-owned buffers, through the kernels
 * aaa_forward / aaa_backward run for that module.  They back the drop-in's
 * standalone ConvLSTMCell.forward / VisionNetwork.forward and let each piece
 * be checked in isolation.  Layout convention (Q3): the reference's NCHW
 * tensors (B, C, a, b) of the vision core are passed NHWC as
 * x.permute(0, 3, 2, 1) = (B, b, a, C); for the Agent's vision core that is
 * (B, h, w, C) with (h, w) the grid of an H x W frame. */

/* ConvLSTMCell(64, 128, 3) at one step (attention.py:110-126, zero
 * peepholes :132-141).  cell_params: the cell's 12 state_dict tensors fp32,
 * concatenated in state_dict order (W{x,h}{i,f,c,o} as in attention.py:39-102:
 * Wxi.weight, Wxi.bias, Whi.weight, Wxf.weight, ...; 885,248 floats) -- a
 * contiguous slice of aaa_param_layout's params.  x (B,h,w,64); h0, c0, h1,
 * c1 (B,h,w,128); h0/c0 NULL = the zero state of init_hidden (:142-149).
 * The workspace keeps the step's activations for aaa_convlstm_cell_bwd. */
typedef struct aaa_cell_desc {
  int B, h, w, dtype;
} aaa_cell_desc;
size_t aaa_convlstm_packed_bytes(const aaa_cell_desc* d);
size_t aaa_convlstm_workspace_bytes(const aaa_cell_desc* d);
int aaa_convlstm_pack(const aaa_cell_desc* d, const float* cell_params, void* packed, hipStream_t stream);
int aaa_convlstm_cell_fwd(const aaa_cell_desc* d, const void* packed, const float* x, const float* h0,
                          const float* c0, float* h1, float* c1, void* workspace, hipStream_t stream);
/* Backward through the matching forward's workspace: dh1/dc1 (NULL = 0) ->
 * dx (B,h,w,64), dh0, dc0 (each NULL = not wanted) and, when cell_grads is
 * set, the 12 parameter gradients (overwritten) in cell_params' layout. */
int aaa_convlstm_cell_bwd(const aaa_cell_desc* d, const void* packed, const float* dh1, const float* dc1, float* dx,
                          float* dh0, float* dc0, float* cell_grads, void* workspace, hipStream_t stream);

/* VisionNetwork.vision_cnn (attention.py:155-170) applied to X.transpose(1,3)
 * (:179): frames (N,H,W,3) fp32 -> y2 (N,h,w,64) (= the reference's output
 * permuted (0,3,2,1)), y1 (N,H1,W1,32) the conv1 output (NULL = not wanted).
 * cnn_params: vision_cnn.{0,1}.{weight,bias} fp32 in state_dict order (39,008
 * floats, the head of aaa_param_layout's params). */
typedef struct aaa_cnn_desc {
  int N, H, W, dtype;
} aaa_cnn_desc;
size_t aaa_vision_cnn_packed_bytes(const aaa_cnn_desc* d);
size_t aaa_vision_cnn_workspace_bytes(const aaa_cnn_desc* d);
int aaa_vision_cnn_pack(const aaa_cnn_desc* d, const float* cnn_params, void* packed, hipStream_t stream);
int aaa_vision_cnn_fwd(const aaa_cnn_desc* d, const float* cnn_params, const void* packed, const float* frames,
                       float* y1, float* y2, void* workspace, hipStream_t stream);
/* dy2 (N,h,w,64) -> the four parameter gradients (overwritten, cnn_params'
 * layout) and dy1 (N,H1,W1,32) (NULL = not wanted); frames get no gradient. */
int aaa_vision_cnn_bwd(const aaa_cnn_desc* d, const void* packed, const float* dy2, float* dy1, float* cnn_grads,
                       void* workspace, hipStream_t stream);

/* The bf16 encoder exactly as the learner runs it -- checker entries, not for
 * a training host.  aaa_vision_cnn_* above converts to fp32 and so never takes
 * the kernels a bf16 learner step takes (the frame-resident k_vision_fwd, the
 * banded conv1 / conv2 with a bf16 output, the fused backward
 * k_vision_bwd_frames); these two call the learner's own dispatch
 * (vision_fwd<bf16, bf16> and the VISION phase of aaa_backward, with the same
 * environment selectors: AAA_VIS_FRAMES, AAA_VIS_BAND, AAA_VIS_BWD_FRAMES,
 * AAA_CONV1_WGRAD_PIPE, AAA_CONV2_WGRAD_PIPE) on caller-owned buffers and hand
 * back the kernels' raw bf16 products, so a test can evaluate each kernel in
 * fp64 on that kernel's own operands (tests/vision_bf16_ref.py).
 *   desc: dtype must be AAA_BF16; flags 0 (fp32 frames) or AAA_FLAG_FRAMES_U8;
 *         out_ld >= 64 and a multiple of 8 is the row pitch of ``out`` in
 *         elements (the learner's is 192: the x half of its [x | h] rows).
 *   packed: aaa_vision_cnn_pack with an aaa_cnn_desc of the same N, H, W and
 *         AAA_BF16 (the layouts are the same).
 *   fwd:  frames (N,H,W,3) -> xp (N,H+2,W+2,4) bf16 the zero-bordered RGBx
 *         frames (the banded conv1 writes the rows conv1 reads, 0 .. 4*H1+3,
 *         and leaves any below them alone), y1 (N,H1*W1,32) bf16 conv1's output, out (N,h*w,out_ld)
 *         bf16 conv2's output in columns 0..63 (the others are not written).
 *   bwd:  frames, dy2 (N,h*w,64) bf16, y1 and xp of the forward -> cnn_grads
 *         (39,008 fp32, cnn_params' layout, overwritten; conv2's bias gradient
 *         is the column sum of dy2), *fused (host int, may be NULL) = 1 when
 *         k_vision_bwd_frames ran, 0 for the layered launches, which also
 *         write dy1 (N,H1*W1,32) bf16 (the fused kernel keeps it on chip and
 *         leaves dy1 alone).  The workspace lends the fused kernel's partials
 *         their room, so -- unlike a learner step, which takes it from the
 *         frames' dY1 region and so needs about 7 frames -- any N may fuse.
 * Launches are recorded under AAA_TIMER_VISION_FWD / _BWD with the learner's
 * variant strings.  Arguments are checked before the device (a refusal needs
 * no GPU); every pointer 16-byte aligned.  Added after ABI version 11 without
 * a bump (purely additive): probe by name. */
typedef struct aaa_enc_desc {
  int N, H, W, dtype, flags, out_ld;
} aaa_enc_desc;
size_t aaa_vision_enc_workspace_bytes(const aaa_enc_desc* d);
int aaa_vision_enc_fwd(const aaa_enc_desc* d, const float* cnn_params, const void* packed, const void* frames,
                       void* xp, void* y1, void* out, hipStream_t stream);
int aaa_vision_enc_bwd(const aaa_enc_desc* d, const void* packed, const void* frames, const void* dy2,
                       const void* y1, void* xp, void* dy1, float* cnn_grads, int* fused, void* workspace,
                       hipStream_t stream);
/* The fp32 learner's encoder forward the same way (vision_fwd<float, float>:
 * with split products and a geometry the frame-resident kernel takes,
 * k_vision_fwd_f32, else -- or with AAA_VIS_FRAMES=0 -- the layered launches):
 * desc dtype must be AAA_F32, flags 0 or AAA_FLAG_FRAMES_U8, out_ld as above;
 * packed from aaa_vision_cnn_pack with an AAA_F32 aaa_cnn_desc of the same N,
 * H, W.  frames (N,H,W,3) -> xp (N,H+2,W+2,4) fp32 the zero-bordered RGBx
 * frames, y1 (N,H1*W1,32) fp32, out (N,h*w,out_ld) fp32 with conv2's output
 * in columns 0..63 (the others are not written).  Recorded under
 * AAA_TIMER_VISION_FWD; arguments checked before the device.  Added after
 * ABI version 11 without a bump (purely additive): probe by name. */
int aaa_vision_enc_f32_fwd(const aaa_enc_desc* d, const float* cnn_params, const void* packed, const void* frames,
                           float* xp, float* y1, float* out, hipStream_t stream);
/* Its backward the same way (the VISION phase's own dispatch: with split
 * products, uint8 frames and a geometry it takes, the frame-resident
 * k_vision_bwd_f32, else -- or with AAA_VIS_BWD_FRAMES=0 -- the layered
 * launches): frames, dy2 (N,h*w,64) fp32, y1 and xp of the forward ->
 * cnn_grads (39,008 fp32, cnn_params' layout, overwritten; conv2's bias
 * gradient is the column sum of dy2), *fused (host int, may be NULL) = 1 when
 * k_vision_bwd_f32 ran, and dy1 (N,H1*W1,32) fp32 (may be NULL): the layered
 * launches' dY1, or the values the fused kernel committed on chip (it stores
 * them only here, never in a learner step).  max_groups > 0 caps the fused
 * kernel's workgroups (0: its default, one per CU at the most), so that a
 * handful of frames can put several frames on one workgroup.  workspace:
 * aaa_vision_enc_f32_workspace_bytes (accumulators, the fused kernel's
 * partials, a dY1 for the layered launches when dy1 is NULL).  Recorded under
 * AAA_TIMER_VISION_BWD with the learner's variant string.  Added after ABI
 * version 11 without a bump (purely additive): probe by name. */
size_t aaa_vision_enc_f32_workspace_bytes(const aaa_enc_desc* d);
int aaa_vision_enc_f32_bwd(const aaa_enc_desc* d, const void* packed, const void* frames, const float* dy2,
                           const float* y1, float* xp, float* dy1, float* cnn_grads, int* fused, int max_groups,
                           void* workspace, hipStream_t stream);

/* Attention readout of F frames (attention.py:319-348: K/V split + spatial
 * basis, logits K.Q, spatial_softmax :235-243, apply_alpha :246-254, answer
 * assembly): O (F,h,w,128) the vision output, S (h,w,64), Q (nq,72) shared by
 * every frame (q_stride 0, the reference's constant query) or (F,nq,72)
 * (q_stride nq*72), prev_reward/prev_action (F) or NULL (zeros) ->
 * attn (F,h,w,nq) and answer (F, 256nq+2) = [a_0..a_{nq-1} (184 each) |
 * Q_0..Q_{nq-1} (72 each) | r | a_prev], the reference's ``answer`` before
 * answer_processor. */
int aaa_attn_fwd(int F, int h, int w, int nq, const float* O, const float* S, const float* Q, int q_stride,
                 const float* prev_reward, const float* prev_action, float* attn, float* answer, hipStream_t stream);
/* Its backward from danswer (F, 256nq+2): dO (F,h,w,128) and dQ (F,nq,72) per
 * frame (logits path + the answer's Q columns; sum over F for a shared Q). */
int aaa_attn_bwd(int F, int h, int w, int nq, const float* O, const float* S, const float* Q, int q_stride,
                 const float* attn, const float* danswer, float* dO, float* dQ, hipStream_t stream);
/* The same readout on bf16 O, as the bf16 learner runs it (ABI 10): O is bf16,
 * frame rows of h*w positions at a pitch of o_ld elements (the learner reads
 * the h half of its [x | h] rows: pitch 192, pointer 64 elements into the
 * row).  o_ld must be >= 136 and a multiple of 8 (16-byte loads; the last
 * piece a row's load touches reaches 8 elements past the 128 channels, read
 * and not used, so the buffer must extend that far past the last row).
 * sq_scratch (h*w*nq floats, 16-byte aligned) may be set only with q_stride
 * 0: the entry first fills it with the constant query's basis logits
 * S.Q[:, 8:] and the kernels take them from there (the learner's call); NULL:
 * the kernels compute the basis logits per frame (the stateful core's call).
 * Arguments are checked before the device, so a refusal needs no GPU.
 * AAA_ATTN_MFMA (default 1: the readout product on the MFMA; 0: the VALU
 * kernel) is read on every call. */
int aaa_attn_fwd_bf16(int F, int h, int w, int nq, const void* O, int o_ld, const float* S, const float* Q,
                      int q_stride, float* sq_scratch, const float* prev_reward, const float* prev_action,
                      float* attn, float* answer, hipStream_t stream);
/* Its backward.  danswer rows have a pitch of da_ld floats (>= the columns
 * read: the nq*184 readout columns, plus the nq*72 Q columns with add_q);
 * add_q != 0 adds the answer row's Q columns into dQ (the stateful core; the
 * learner passes 0 and adds them downstream).  dO_quad_major != 0 writes dO
 * in the frame-resident BPTT's layout: the frame's value for position p,
 * channels 4k..4k+3, at float offset (k*h*w + p)*4 of the frame's h*w*128
 * floats.  AAA_ATTN_BWD_MFMA (default 1: the dA pass on the MFMA above 256
 * grid positions; 2: everywhere; 0: never) is read on every call. */
int aaa_attn_bwd_bf16(int F, int h, int w, int nq, const void* O, int o_ld, const float* S, const float* Q,
                      int q_stride, const float* attn, const float* danswer, int da_ld, int add_q,
                      int dO_quad_major, float* dO, float* dQ, hipStream_t stream);

/* ---- index-arithmetic self-checks (host only, no device needed) ----
 * Every pixel / tap / tile index in the kernels is divided by a runtime
 * constant through one multiply-shift divider (csrc/common.h FastDiv).
 * aaa_fastdiv_check runs the divider for d on every dividend n in [lo, hi)
 * (hi <= 2^31, the divider's whole domain) against the exact quotient and
 * returns the number of mismatches in *mismatches.  aaa_divisor_log(1, ...)
 * starts recording every divisor the runtime builds for its launches;
 * aaa_divisor_log(-1, out, cap) copies them out; aaa_divisor_log(0, ...)
 * copies, stops and clears.  Returns the number recorded. */
int aaa_fastdiv_check(unsigned d, unsigned lo, unsigned hi, unsigned long long* mismatches);
int aaa_divisor_log(int enable, unsigned* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* AAA_H */
