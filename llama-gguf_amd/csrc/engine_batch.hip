// engine_batch.hip — multi-sequence decode on one GPU: the device side of the reference's BatchedEngine
// (src/engine_batched.rs:23-194 config / request types, 200-330 the loop, 355-400 `step_sequence`).
//
// The reference keeps one InferenceContext (KV cache + position) per ActiveSequence and, every iteration, runs
// `model.forward` for each active sequence in turn: B sequences read the weights B times.  Here a context owns `max_batch`
// SLOTS — a slot = one sequence's KV caches + position — and lgh_forward_multi feeds one token to each listed slot in ONE pass
// over the weights: every quantized mat-vec launch reads its tiles once and multiplies them with all n_seq input vectors
// (matvec_batch.hip), attention / its merge / embedding / arg-max run with the sequence as the grid's second dimension (over f32,
// int8 / FP8 or TurboQuant slots); MoE layers route every sequence to its own experts: from 3 sequences on (moe_group_min) the step's (sequence,
// slot) pairs are grouped by expert and each selected expert is read once — all experts of a layer in one gate | up and one down
// launch, the expert as the grid's third dimension — below that the FFN runs sequence by sequence.  Every sequence's logits are
// bit-identical to what the single-sequence engine computes for the same tokens (tests/test_gpu_batch.py): same kernels'
// arithmetic, same summation orders.
//
// A step is a constant hipGraph per n_seq: tokens, positions and slot numbers live in device words (d_tokens / d_pos /
// d_slot), the arg-max feeds the next token back on the device and `batch_advance` moves the positions, so
// lgh_decode_greedy_multi replays the graph with no host work in between.
#include "engine.h"
#include "xq.h"

#include <algorithm>
#include <cstdlib>
#include <cmath>

using namespace lgh;

namespace lgh {

__global__ void batch_advance_kernel(int* pos, int n) {
  if ((int)threadIdx.x < n) pos[threadIdx.x] += 1;
}

}  // namespace lgh

// ---- shared with the per-launch entry points of ops_api.hip (engine.h)
uint32_t xq_stride_of(uint32_t k) { return (uint32_t)xq_bytes(k); }
uint32_t ssq_stride_of(uint32_t k) { return k / 16 + 64; }

// sequence-0 view of a batch vector is registered in the context's XQ registry under its f32 address (engine_launch.hip: xq_get), the
// other sequences' views follow at the strides above: build_mv_group finds the images it needs there
int register_views(lgh_ctx* c, float* f32, uint8_t* xq, float* ssq, uint32_t k, uint32_t n) {
  for (uint32_t s = 0; s < n; s++) {
    XqBuf q;
    q.f32 = f32 + (size_t)s * k;
    q.k = k;
    q.xq = xq + (size_t)s * xq_stride_of(k);
    q.ssq = ssq + (size_t)s * ssq_stride_of(k);
    c->xqs.push_back(q);
  }
  return LGH_OK;
}

void mark_fresh(lgh_ctx* c, const float* base, uint32_t k, uint32_t n, const float* tag) {
  for (uint32_t s = 0; s < n; s++)
    if (XqBuf* q = xq_find(c, base + (size_t)s * k)) { q->fresh = true; q->tag = tag; }
}

// after a batched launch produced / consumed the images of sequence 0's view, the other sequences' views are in the same state
static void spread_state(lgh_ctx* c, const float* f32, uint32_t k, uint32_t n) {
  XqBuf* q0 = xq_find(c, f32);
  if (!q0) return;
  for (uint32_t s = 1; s < n; s++)
    if (XqBuf* q = xq_find(c, f32 + (size_t)s * k)) { q->fresh = q0->fresh; q->tag = q0->tag; }
}

// MoE layers: from how many sequences on a step reads every selected expert ONCE (one router launch, a grouping launch, gate | up
// and down over all experts with the expert as the grid's third dimension + their epilogue launches, one combine: 7 per layer
// whatever the step's size) instead of running the FFN sequence by sequence (3 launches per sequence).  Measured on Mixtral-8x7B
// Q5_K_M, tokens/s grouped vs sequence by sequence: 2 sequences 363 vs 392, 3: 447 vs 421, 4: 520 vs 436, 8: 764 vs 468,
// 16: 1 030 vs 480 (profiles/r03e_batched_decode.md).
// (LGH_MOE_GROUP_MIN is read once per process: tests/test_gpu_fresh_env.py runs the sequence-by-sequence form at 3 and 16 sequences)
uint32_t moe_group_min() {
  static const uint32_t v = [] { const char* e = std::getenv("LGH_MOE_GROUP_MIN"); return e ? (uint32_t)std::max(2, std::atoi(e)) : 3u; }();
  return v;
}

// the multi-sequence kernels run 8-wave workgroups: the single-sequence plan of a [.., k] matrix must have T x G = 8
bool mvb_k_ok(uint32_t k) {
  MvPlan p{};
  return mvq_plan(k, 16, 1, &p, 16) == hipSuccess && p.threads == 512;
}

// one batched quantized mat-vec launch: `specs` name sequence 0's vectors
int launch_mvb(lgh_ctx* c, int cls, const SegSpec* specs, int nseg, const float* norm_w, uint32_t k, uint32_t n_seq, const uint32_t* out_stride,
               const uint32_t* resid_stride, const uint32_t* xq_out_k, const MvIndirect ind) {
  BatchScratch& Bs = c->batch;
  if (!mvb_k_ok(k))
    return fail(c, LGH_UNSUPPORTED, "multi-sequence mat-vec: k=" + std::to_string(k) + " does not plan to 8-wave workgroups");
  MvLaunch L;
  uint32_t wg = 0, threads = 0;
  uint64_t alg = 0;
  // partial sums of all sequences in LDS: n_seq * npass * T * 16 * R floats <= ~120 KB
  uint32_t cap = 32;
  {
    int npass_max = 1;
    for (int s = 0; s < nseg; s++) npass_max = std::max(npass_max, specs[s].npass);
    const uint32_t budget_floats = 120u * 1024u / 4u / n_seq;
    cap = std::max(1u, budget_floats / ((uint32_t)npass_max * 8u * 16u));
  }
  int rc = build_mv_group(c, specs, nseg, norm_w, k, true, L, wg, threads, alg, cap);
  if (rc) return rc;
  if (mvqb_lds_bytes(n_seq, L.red_floats) > 160 * 1024) return fail(c, LGH_UNSUPPORTED, "multi-sequence mat-vec: partial sums do not fit LDS");
  MvBatch B{};
  B.n_seq = n_seq;
  B.pos = Bs.d_pos;
  B.slot = Bs.d_slot;
  B.cache_stride = c->kvl.stride_floats();
  B.part = Bs.mv_part;
  B.part_floats = Bs.mv_part_floats;
  B.ind_cnt = ind.cnt;
  B.ind_idx = ind.idx;
  B.ind_div = ind.div;
  B.ind_nz = ind.nz;
  B.ind_stride = ind.stride;
  {   // the input vector's images lie at the strides its views were registered with
    const XqBuf* q0 = xq_find(c, specs[0].x[0]);
    const uint32_t kreg = q0 ? q0->k : k;
    B.xq_stride = xq_stride_of(kreg);
    B.ssq_stride = ssq_stride_of(kreg);
  }
  for (int s = 0; s < nseg; s++) {
    B.out_stride[s] = out_stride[s];
    B.resid_stride[s] = resid_stride[s];
    B.xq_out_stride[s] = xq_out_k[s] ? xq_stride_of(xq_out_k[s]) : 0;
    B.ssq_out_stride[s] = xq_out_k[s] ? ssq_stride_of(xq_out_k[s]) : 0;
  }
  return run_k(c, cls, LGH_SYM_OTHER, alg, [&] { return mvqb_launch(L, B, wg, threads, c->stream); });
}

// Q, K, V of layer li for the step's sequences: RoPE at every sequence's own position, K / V rows into its own cache slot
int qkv_forward_multi(lgh_ctx* c, LayerW& Lw, uint32_t li, uint32_t n_seq) {
  BatchScratch& Bs = c->batch;
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size, QD = d.num_heads * d.head_dim;
  const bool staged = c->kvl.staged();   // every quantized cache (TurboQuant, int8, FP8) stages its rows
  const uint32_t KD = d.num_kv_heads * d.head_dim;
  int rc;
  SegSpec sp[3];
  sp[0].W[0] = &Lw.wq; sp[0].x[0] = Bs.hidden; sp[0].epi = EPI_ROPE_Q; sp[0].out = Bs.q; sp[0].bias = Lw.bq;
  // (quantized caches: the rotated K row and the V row stay f32 in a staging vector per sequence; the attention launch compresses them)
  sp[1].W[0] = &Lw.wk; sp[1].x[0] = Bs.hidden; sp[1].epi = staged ? EPI_ROPE_Q : EPI_ROPE_K; sp[1].out = staged ? Bs.kv_tmp : Bs.kv[li].k_f32(); sp[1].bias = Lw.bk;
  sp[2].W[0] = &Lw.wv; sp[2].x[0] = Bs.hidden; sp[2].epi = staged ? EPI_STORE : EPI_V_CACHE; sp[2].out = staged ? Bs.kv_tmp + KD : Bs.kv[li].v_f32(); sp[2].bias = Lw.bv;
  const uint32_t os[3] = {QD, staged ? 2 * KD : 0, staged ? 2 * KD : 0}, rs[3] = {0, 0, 0}, xk[3] = {0, 0, 0};
  if (mv_formats_split(sp, 3)) {   // (one launch each then, as launch_mv does)
    for (int s = 0; s < 3; s++)
      if ((rc = launch_mvb(c, LGH_K_QKV, sp + s, 1, Lw.attn_norm, H, n_seq, os + s, rs + s, xk + s))) return rc;
    return LGH_OK;
  }
  return launch_mvb(c, LGH_K_QKV, sp, 3, Lw.attn_norm, H, n_seq, os, rs, xk);
}

// one Linear of the step for all its sequences (linear_any's counterpart): W — or the SwiGLU pair W | W_up — over sequence 0's vectors
// x -> out, sequence s's output out_stride floats on; a residual lies at the output's stride, and so do the views of an output that
// leaves its image (xq_next / xq_next_nw as SegSpec's); ind: as launch_mvb's.  wo, gate | up, down — dense or the experts' — and the
// output projection of a step are calls of this
int linear_multi(lgh_ctx* c, int cls, const DevWeight& W, const DevWeight* W_up, const float* x, float* out, uint32_t out_stride, uint32_t n_seq,
                 const float* norm_w, const float* resid, const float* bias, int xq_next, const float* xq_next_nw, const MvIndirect ind) {
  SegSpec sp;
  sp.W[0] = &W; sp.x[0] = x;
  if (W_up) { sp.npass = 2; sp.W[1] = W_up; sp.x[1] = x; }
  sp.epi = W_up ? EPI_SWIGLU : resid ? EPI_RESID : EPI_STORE;
  sp.out = out; sp.resid = resid; sp.bias = bias;
  sp.xq_next = xq_next; sp.xq_next_nw = xq_next_nw;
  const uint32_t rs = resid ? out_stride : 0, xk = xq_next ? out_stride : 0;
  if (int rc = launch_mvb(c, cls, &sp, 1, norm_w, W.k, n_seq, &out_stride, &rs, &xk, ind)) return rc;
  spread_state(c, out, out_stride, n_seq);   // (the launch set sequence 0's view: fresh with an image, stale without; no view, nothing to do)
  return LGH_OK;
}

// MoE, every selected expert's matrices read ONCE for the step (MoeLayer::forward per sequence, moe.rs:321-413, regrouped):
// router (route; else the selections and weights already in the scratch) -> the (sequence, slot) pairs grouped by expert -> a gate|up
// launch, every expert over its pairs (SwiGLU, activation + XQ image per pair), and a down launch (output per pair) ->
// h += sum_p w_p * down_p in selection order
int moe_grouped_forward(lgh_ctx* c, LayerW& Lw, uint32_t n_seq, const float* next_nw, bool route) {
  BatchScratch& Bs = c->batch;
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size;
  const uint32_t topk = d.num_experts_per_token, ne = d.num_experts, EF = Lw.gate_exps.n;
  int rc;
  // (the router for all sequences in one launch: selections and weights packed [sequence][top_k])
  if (route && (rc = run_k(c, LGH_K_ROUTER, LGH_SYM_ROUTER, (uint64_t)ne * H * 4, [&] {
                  return moe_router_launch(Bs.hidden, Lw.ffn_norm, d.norm_eps, Lw.router, H, ne, topk, Bs.moe_sel, Bs.moe_w, c->stream, n_seq);
                })))
    return rc;
  if ((rc = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, 0, [&] { return moe_group_launch(Bs.moe_sel, n_seq, topk, ne, Bs.moe_cnt, Bs.moe_idx, kMaxBatch, c->stream); })))
    return rc;
  // all experts of the layer in one launch each (grid z = expert: its count, its entry list, its slice of the stacked matrices)
  const MvIndirect ind_gu{Bs.moe_cnt, Bs.moe_idx, topk, ne, (uint32_t)kMaxBatch}, ind_dn{Bs.moe_cnt, Bs.moe_idx, 1, ne, (uint32_t)kMaxBatch};
  if ((rc = linear_multi(c, LGH_K_GATEUP, Lw.gate_exps, &Lw.up_exps, Bs.hidden, Bs.moe_act, EF, n_seq, Lw.ffn_norm, nullptr, nullptr, 1, nullptr, ind_gu)))
    return rc;
  mark_fresh(c, Bs.moe_act, EF, n_seq * topk, nullptr);   // (a view per pair, not per sequence)
  if ((rc = linear_multi(c, LGH_K_DOWN, Lw.down_exps, nullptr, Bs.moe_act, Bs.moe_tmp, H, n_seq, nullptr, nullptr, nullptr, 0, nullptr, ind_dn))) return rc;
  XqBuf* qh = xq_find(c, Bs.hidden);
  if ((rc = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, 0, [&] {
         return moe_combine_launch(Bs.moe_tmp, Bs.moe_w, topk, Bs.hidden, H, n_seq, next_nw, qh->xq, xq_stride_of(H), qh->ssq, ssq_stride_of(H), c->stream);
       })))
    return rc;
  mark_fresh(c, Bs.hidden, H, n_seq, next_nw);
  return LGH_OK;
}

// the FFN half of a layer for the step's sequences, Bs.hidden -> Bs.hidden (+ its image with next_nw): the dense pair of launches; MoE
// layers from moe_group_min() sequences on every selected expert once (moe_grouped_forward), below that — or where the expert shapes
// do not group — sequence by sequence, every sequence routed to its own experts by the single-sequence launches on its vectors
int ffn_forward_multi(lgh_ctx* c, LayerW& Lw, uint32_t n_seq, const float* next_nw) {
  BatchScratch& Bs = c->batch;
  const uint32_t H = c->d.hidden_size;
  int rc;
  if (!Lw.moe()) {
    if ((rc = linear_multi(c, LGH_K_GATEUP, Lw.gate, &Lw.up, Bs.hidden, Bs.act, Bs.ffn, n_seq, Lw.ffn_norm, nullptr, nullptr, 1))) return rc;
    return linear_multi(c, LGH_K_DOWN, Lw.down, nullptr, Bs.act, Bs.hidden, H, n_seq, nullptr, Bs.hidden, nullptr, 2, next_nw);
  }
  if (Bs.moe_act && n_seq >= moe_group_min()) return moe_grouped_forward(c, Lw, n_seq, next_nw, true);
  for (uint32_t s = 0; s < n_seq; s++) {
    const FfnView v{Bs.hidden + (size_t)s * H, Bs.act + (size_t)s * Bs.ffn, Bs.act2 + (size_t)s * Bs.ffn, Bs.xnorm + (size_t)s * H,
                    Bs.moe_sel + s * 8, Bs.moe_w + s * 8};
    if ((rc = ffn_forward(c, Lw, v, next_nw, true))) return rc;
  }
  return LGH_OK;
}

namespace {

bool batch_weights_ok(const lgh_ctx* c, std::string& why) {
  const lgh_model_desc& d = c->d;
  if (d.hidden_size % 256 || (d.num_heads * d.head_dim) % 256) { why = "hidden size and heads x head_dim must be multiples of 256"; return false; }
  if (d.use_neox_rope) { why = "NeoX RoPE is not fused into the QKV launch"; return false; }
  if (!attn_shape_has_fast_kernel(d.head_dim, d.num_heads / d.num_kv_heads)) { why = "attention shape outside the split kernels"; return false; }
  if (!(c->first && c->last)) { why = "pipeline stages are not batched"; return false; }
  // (what launch_mvb would refuse at the first step: the widths every launch of a step multiplies along)
  auto plans = [&](uint32_t k, const char* what) {
    if (mvb_k_ok(k)) return true;
    why = std::string(what) + " " + std::to_string(k) + " does not plan to 8-wave workgroups";
    return false;
  };
  if (!plans(d.hidden_size, "hidden size") || !plans(d.num_heads * d.head_dim, "heads x head_dim")) return false;
  for (uint32_t i = c->l0; i < c->l1; i++) {
    const LayerW& L = c->layers[i];
    if (!L.moe() && d.intermediate_size % 256 == 0 && !plans(d.intermediate_size, "intermediate size")) return false;
    for (const DevWeight* W : {&L.wq, &L.wk, &L.wv, &L.wo})
      if (!mfma_type(W->type) || W->n % 16) { why = "attention weights of layer " + std::to_string(i) + " are not in a matrix-core tile layout"; return false; }
    if (!L.moe()) {
      if (d.intermediate_size % 256) { why = "intermediate size must be a multiple of 256"; return false; }
      for (const DevWeight* W : {&L.gate, &L.up, &L.down})
        if (!mfma_type(W->type) || W->n % 16) { why = "FFN weights of layer " + std::to_string(i) + " are not in a matrix-core tile layout"; return false; }
      if (L.gate.type != L.up.type) { why = "gate and up differ in format"; return false; }
    }
  }
  if (!mfma_type(c->output.type)) { why = "the output projection is not in a matrix-core tile layout"; return false; }
  return true;
}

// everything one step of n_seq sequences needs, in stream order (eager or under capture); tokens / positions / slots are read
// from the device words
int enqueue_multi(lgh_ctx* c, uint32_t n_seq, int mode) {   // mode 0 logits only, 1 + arg-max, 2 + sampled token
  BatchScratch& Bs = c->batch;
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size;
  int rc;
  auto stale_all = [&] { for (auto& q : c->xqs) q.fresh = false; };
  stale_all();
  // ---- embedding rows + the first layer's XQ image (embed_kernel's arithmetic)
  {
    LayerW& L0 = c->layers[c->l0];
    XqBuf* qh = xq_find(c, Bs.hidden);
    if ((rc = run_k(c, LGH_K_EMBED, LGH_SYM_EMBED, (uint64_t)n_seq * H * blk_bytes(c->embd_type) / blk_elems(c->embd_type), [&] {
           return embed_multi_launch(c->embd_type, c->embd_raw, Bs.d_tokens, Bs.hidden, H, n_seq, qh->xq, L0.attn_norm, qh->ssq, xq_stride_of(H),
                                     ssq_stride_of(H), c->stream);
         })))
      return rc;
    mark_fresh(c, Bs.hidden, H, n_seq, L0.attn_norm);
  }
  const float scale = 1.0f / std::sqrt((float)d.head_dim);
  for (uint32_t li = c->l0; li < c->l1; li++) {
    LayerW& Lw = c->layers[li];
    const float* next_nw = li + 1 < c->l1 ? c->layers[li + 1].attn_norm : c->output_norm;
    // ---- Q, K, V (+ RoPE at every sequence's own position, K / V rows into its own cache slot), attention over every sequence's slot
    if ((rc = qkv_forward_multi(c, Lw, li, n_seq))) return rc;
    if ((rc = attention_forward_multi(c, li, n_seq, scale, true))) return rc;
    // ---- h = x + wo(attn)
    if ((rc = linear_multi(c, LGH_K_WO, Lw.wo, nullptr, Bs.attn_out, Bs.hidden, H, n_seq, nullptr, Bs.hidden, Lw.bo, 2, Lw.ffn_norm))) return rc;
    // ---- FFN
    if ((rc = ffn_forward_multi(c, Lw, n_seq, next_nw))) return rc;
  }
  // ---- compute_logits: final RMSNorm fused into the output projection
  if ((rc = linear_multi(c, LGH_K_OUTPUT, c->output, nullptr, Bs.hidden, Bs.logits, d.vocab_size, n_seq, c->output_norm))) return rc;
  if (mode == 1) {
    // arg-max per sequence (last maximal index), fed back as the next step's token; the positions move on
    if ((rc = run_k(c, LGH_K_ARGMAX, LGH_SYM_ARGMAX, (uint64_t)n_seq * d.vocab_size * 4, [&] {
           return argmax_multi_launch(Bs.logits, d.vocab_size, n_seq, Bs.amax_v, Bs.amax_i, Bs.d_tokens, c->stream);
         })))
      return rc;
  } else if (mode == 2) {
    // each sequence sampled by its slot's sampler (sample.hip), fed back the same way
    if ((rc = run_k(c, LGH_K_ARGMAX, LGH_SYM_OTHER, (uint64_t)n_seq * d.vocab_size * 4, [&] {
           return sample_launch(Bs.samp, Bs.logits, d.vocab_size, n_seq, Bs.d_slot, nullptr, nullptr, Bs.d_tokens, c->stream);
         })))
      return rc;
  }
  if ((rc = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, 0, [&] {
         hipLaunchKernelGGL(batch_advance_kernel, dim3(1), dim3(64), 0, c->stream, Bs.d_pos, (int)n_seq);
         return hipGetLastError();
       })))
    return rc;
  stale_all();
  return LGH_OK;
}

// the step's control words (tokens, positions, slots) of checked sequences to the device
static int stage_words(lgh_ctx* c, const uint32_t* slots, const uint32_t* tokens, uint32_t n_seq) {
  BatchScratch& Bs = c->batch;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));   // the pinned words below are free again
  for (uint32_t i = 0; i < n_seq; i++) {
    Bs.h_ctl[i] = tokens ? (int)tokens[i] : 0;
    Bs.h_ctl[kMaxBatch + i] = (int)Bs.pos[slots[i]];
    Bs.h_ctl[2 * kMaxBatch + i] = (int)slots[i];
  }
  if (tokens) HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(Bs.d_tokens, Bs.h_ctl, (size_t)n_seq * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(Bs.d_pos, Bs.h_ctl + kMaxBatch, (size_t)n_seq * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(Bs.d_slot, Bs.h_ctl + 2 * kMaxBatch, (size_t)n_seq * 4, hipMemcpyHostToDevice, c->stream));
  return LGH_OK;
}

int stage_control(lgh_ctx* c, const uint32_t* slots, const uint32_t* tokens, uint32_t n_seq) {
  BatchScratch& Bs = c->batch;
  const lgh_model_desc& d = c->d;
  if (!Bs.ready) return fail(c, LGH_INVALID_ARGUMENT, "lgh_batch_create has not been called");
  size_t at = 0;
  switch (check_seqs(n_seq, Bs.max_batch, slots, Bs.max_batch, true, [&](size_t i) { return Bs.pos[slots[i]]; }, d.max_seq_len, &at)) {
    case SEQ_OK: break;
    case SEQ_COUNT: return fail(c, LGH_INVALID_ARGUMENT, "n_seq must be 1 .. max_batch");
    case SEQ_SLOT: return fail(c, LGH_INVALID_ARGUMENT, "slot numbers must be distinct and below max_batch");
    case SEQ_POS:
      return fail(c, LGH_INVALID_ARGUMENT, "slot " + std::to_string(slots[at]) + ": position " + std::to_string(Bs.pos[slots[at]]) + " >= max_seq_len");
  }
  for (uint32_t i = 0; tokens && i < n_seq; i++)
    if (tokens[i] >= d.vocab_size) return fail(c, LGH_INVALID_ARGUMENT, "token id exceeds vocab size");
  return stage_words(c, slots, tokens, n_seq);
}

int run_multi(lgh_ctx* c, uint32_t n_seq, int mode) {
  BatchScratch& Bs = c->batch;
  if (c->profiling || (c->d.flags & LGH_FLAG_NO_GRAPH)) {
    int rc = enqueue_multi(c, n_seq, mode);
    if (rc) return rc;
    return c->profiling ? drain_prof(c) : LGH_OK;
  }
  hipGraphExec_t& ge = Bs.graph[n_seq][mode];
  if (!ge)
    if (int rc = capture_graph(c, &ge, [&] { return enqueue_multi(c, n_seq, mode); })) return rc;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipGraphLaunch(ge, c->stream));
  return LGH_OK;
}

// n_steps steps of n_seq sequences in `mode` (1 arg-max, 2 sampler), every token fed back on the device; the steps' tokens come back
// as [step][n_seq], and the slots' positions move on
int decode_multi(lgh_ctx* c, const uint32_t* slots, uint32_t n_seq, int mode, size_t n_steps, uint32_t* tokens_out) {
  BatchScratch& Bs = c->batch;
  for (size_t st = 0; st < n_steps; st++) {
    if (int rc = run_multi(c, n_seq, mode)) return rc;
    if (tokens_out)
      HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(Bs.d_log + st * kMaxBatch, Bs.d_tokens, (size_t)n_seq * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  if (tokens_out && n_steps) {
    std::vector<int> log(n_steps * kMaxBatch);   // the log's rows are kMaxBatch wide
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy(log.data(), Bs.d_log, log.size() * 4, hipMemcpyDeviceToHost));
    for (size_t st = 0; st < n_steps; st++)
      for (uint32_t i = 0; i < n_seq; i++) tokens_out[st * n_seq + i] = (uint32_t)log[st * kMaxBatch + i];
  }
  for (uint32_t i = 0; i < n_seq; i++) Bs.pos[slots[i]] += n_steps;
  c->stats.tokens_processed += n_steps * n_seq;
  return LGH_OK;
}

// the grouped MoE step needs both expert shapes on 8-wave workgroups (as Mixtral's are) and its tables bound top-k and the experts
bool moe_grouped_ok(const lgh_model_desc& d, uint32_t EI) {
  return d.num_experts && EI && EI % 256 == 0 && mvb_k_ok(d.hidden_size) && mvb_k_ok(EI) && d.num_experts_per_token <= 8 && d.num_experts <= 64;
}

}  // namespace

// Partial sums between the two launches of a multi-sequence mat-vec (matvec_batch.hip, mvqb2): the largest region any launch of a
// step of max_batch sequences asks for — mvqb_part_floats knows, per launch, whether the grid keeps one value per (sequence, row) or
// one per k-slice, and an expert launch has a region per expert.  (A launch that finds the buffer too small falls back to the first
// structure, and an expert launch fails.  mvqb_launch lays the buffer out and checks its size with the rule behind mvqb_part_floats
// — matvec_batch.hip: mvqb2_part — and refuses a launch whose k-slices are not the ones mvqb_part_floats assumes for its k.)
uint64_t batch_part_floats(const lgh_ctx* c, uint32_t max_batch) {
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size, QD = d.num_heads * d.head_dim, KD = d.num_kv_heads * d.head_dim;
  const uint32_t EI = d.expert_intermediate_size ? d.expert_intermediate_size : d.intermediate_size;
  auto tiles = [](uint32_t n) { return (n + 15) / 16; };
  uint64_t need = 0;
  auto launch = [&](uint32_t k, uint32_t units, uint32_t nz) {
    if (k && k % 256 == 0 && units) need = std::max(need, mvqb_part_floats(k, units, max_batch, nz));
  };
  launch(H, tiles(QD) + 2 * tiles(KD), 1);                     // fused Q | K | V ...
  launch(H, tiles(QD), 1);                                     // ... or, split by format, one launch each: fewer units, but a launch
  launch(H, tiles(KD), 1);                                     // of its own may keep a value per k-slice where the fused one keeps one per row
  launch(QD, tiles(H), 1);                                     // wo
  launch(H, 2 * tiles(d.intermediate_size), 1);                // gate | up
  launch(d.intermediate_size, tiles(H), 1);                    // down
  launch(H, tiles(d.vocab_size), 1);                           // output projection
  if (moe_grouped_ok(d, EI)) {
    launch(H, 2 * tiles(EI), d.num_experts);                   // every expert's gate | up over its pairs
    launch(EI, tiles(H), d.num_experts);                       // ... and down
  }
  return need;
}

// the scratch of the multi-sequence engine for max_batch slots on a context whose model fields and layers are set: the vectors of the
// sequences side by side with their registered XQ views, the control words, the partial-sum buffer, every slot's caches and the
// grouped MoE step's buffers (lgh_batch_create; the per-launch entry points of ops_api.hip)
int batch_scratch_alloc(lgh_ctx* c, uint32_t max_batch) {
  int rc;
  BatchScratch& Bs = c->batch;
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size, QD = d.num_heads * d.head_dim, G = d.num_heads / d.num_kv_heads;
  const uint32_t EI = d.expert_intermediate_size ? d.expert_intermediate_size : d.intermediate_size;
  const uint32_t ffn = std::max(d.intermediate_size, EI);
  Bs.max_batch = max_batch;
  Bs.ffn = ffn;
  Bs.kv.assign(d.num_layers, KvCache{});
  const size_t B = max_batch;
  Bs.mv_part_floats = batch_part_floats(c, max_batch);
  uint8_t *xq_h = nullptr, *xq_a = nullptr, *xq_f = nullptr, *xq_f2 = nullptr;
  float *ssq_h = nullptr, *ssq_a = nullptr, *ssq_f = nullptr, *ssq_f2 = nullptr;
  const AllocSpec bufs[] = {
      {(void**)&Bs.hidden, B * H * 4},   {(void**)&Bs.xnorm, B * H * 4},   {(void**)&Bs.q, B * QD * 4},   {(void**)&Bs.attn_out, B * QD * 4},
      {(void**)&Bs.act, B * ffn * 4},    {(void**)&Bs.act2, B * ffn * 4},  {(void**)&Bs.logits, B * d.vocab_size * 4},
      {(void**)&Bs.part_ml, B * d.num_kv_heads * c->n_splits * G * 2 * 4}, {(void**)&Bs.part_acc, B * d.num_kv_heads * c->n_splits * G * d.head_dim * 4},
      {(void**)&Bs.mv_part, Bs.mv_part_floats * 4},
      {(void**)&Bs.amax_v, B * 64 * 4},  {(void**)&Bs.amax_i, B * 64 * 4}, {(void**)&Bs.moe_sel, B * 8 * 4}, {(void**)&Bs.moe_w, B * 8 * 4},
      {(void**)&Bs.d_tokens, kMaxBatch * 4}, {(void**)&Bs.d_pos, kMaxBatch * 4}, {(void**)&Bs.d_slot, kMaxBatch * 4},
      {(void**)&Bs.d_log, (size_t)d.max_seq_len * kMaxBatch * 4},
      {(void**)&xq_h, B * xq_stride_of(H)},   {(void**)&ssq_h, B * ssq_stride_of(H) * 4},
      {(void**)&xq_a, B * xq_stride_of(QD)},  {(void**)&ssq_a, B * ssq_stride_of(QD) * 4},
      {(void**)&xq_f, B * xq_stride_of(ffn)}, {(void**)&ssq_f, B * ssq_stride_of(ffn) * 4},
      {(void**)&xq_f2, B * xq_stride_of(ffn)}, {(void**)&ssq_f2, B * ssq_stride_of(ffn) * 4},
  };
  if ((rc = alloc_zeroed(c, bufs, sizeof(bufs) / sizeof(bufs[0]), c->stats.scratch_bytes))) return rc;
  if (c->kvl.staged() && (rc = dev_alloc(c, (void**)&Bs.kv_tmp, B * 2 * d.num_kv_heads * d.head_dim * 4))) return rc;
  for (uint32_t i = c->l0; i < c->l1; i++)   // per layer, every slot's cache
    if ((rc = kv_alloc(c, B, Bs.kv[i]))) return rc;
  {   // MoE layers: the expert-grouped step's buffers ((sequence, slot) pairs)
    bool any_moe = false;
    for (uint32_t i = c->l0; i < c->l1; i++) any_moe = any_moe || c->layers[i].moe();
    if (any_moe && moe_grouped_ok(d, EI)) {
      const size_t np = B * d.num_experts_per_token;
      uint8_t* xq_m = nullptr;
      float* ssq_m = nullptr;
      const AllocSpec mb[] = {
          {(void**)&Bs.moe_act, np * EI * 4}, {(void**)&Bs.moe_tmp, np * H * 4}, {(void**)&Bs.moe_cnt, 64 * 4}, {(void**)&Bs.moe_idx, 64 * kMaxBatch * 4},
          {(void**)&xq_m, np * xq_stride_of(EI)}, {(void**)&ssq_m, np * ssq_stride_of(EI) * 4}};
      if ((rc = alloc_zeroed(c, mb, sizeof(mb) / sizeof(mb[0]), c->stats.scratch_bytes))) return rc;
      register_views(c, Bs.moe_act, xq_m, ssq_m, EI, (uint32_t)np);
    }
  }
  HIP_TRY(c, LGH_ALLOCATION_FAILED, hipHostMalloc((void**)&Bs.h_ctl, 3 * kMaxBatch * 4, hipHostMallocDefault));
  register_views(c, Bs.hidden, xq_h, ssq_h, H, max_batch);
  register_views(c, Bs.attn_out, xq_a, ssq_a, QD, max_batch);
  register_views(c, Bs.act, xq_f, ssq_f, ffn, max_batch);
  register_views(c, Bs.act2, xq_f2, ssq_f2, ffn, max_batch);
  Bs.pos.assign(max_batch, 0);
  return LGH_OK;
}

extern "C" {

int lgh_batch_create(lgh_ctx* c, uint32_t max_batch) {
  int rc = check_ready(c);
  if (rc) return rc;
  BatchScratch& Bs = c->batch;
  if (Bs.ready) return Bs.max_batch == max_batch ? LGH_OK : fail(c, LGH_INVALID_ARGUMENT, "lgh_batch_create was already called with another max_batch");
  if (Bs.max_batch) return fail(c, LGH_OPERATION_FAILED, "an earlier lgh_batch_create failed on this context");   // (its scratch is allocated, not warm)
  if (max_batch == 0 || max_batch > (uint32_t)kMaxBatch) return fail(c, LGH_INVALID_ARGUMENT, "max_batch must be 1 .. 16");
  std::string why;
  if (!batch_weights_ok(c, why)) return fail(c, LGH_UNSUPPORTED, "multi-sequence decode: " + why);
  if ((rc = batch_scratch_alloc(c, max_batch))) return rc;
  // the slots' samplers (allocated before the context counts as ready: the sampler entry points index these per slot)
  if ((rc = samp_alloc(c, Bs.samp, max_batch, max_batch))) return rc;
  Bs.samp_cfg.assign(max_batch, lgh_sampler_config_ex{});
  Bs.samp_set.assign(max_batch, 0);
  // Every kernel instantiation a captured step of 1 .. max_batch sequences can launch is launched here once, eagerly (engine.hip:
  // warm_kernels explains the ROCm trap: a kernel first launched inside a capture is not replayed with the graph, and the result is
  // wrong tokens, not an error).  One sequence; two (the kernels only a step of several sequences launches); then one step per
  // sequence bucket of the multi-sequence mat-vec (matvec_batch.hip: mvqb2_kernel<MASK, NB, *>, NB = 4 up to 4 sequences, 8 up to 8,
  // 16 beyond) that max_batch reaches.  Where MoE layers group their pairs by expert (Bs.moe_act), a bucket's step has at least
  // moe_group_min() sequences if the bucket holds such a count: below it the FFN runs sequence by sequence, and moe_group_kernel,
  // moe_combine_kernel, the multi-token router and the experts' mat-vec instantiations of that bucket would stay cold.  Mode 1
  // launches a superset of mode 0's kernels.  A step of n sequences writes row 0 of the caches of slots 0 .. n - 1, which each slot's
  // first real token overwrites; Bs.pos stays 0.  (tests/test_gpu_fresh_capture.py: captured steps as a process's first GPU work)
  {
    uint32_t slots[kMaxBatch], toks[kMaxBatch];
    for (uint32_t i = 0; i < (uint32_t)kMaxBatch; i++) { slots[i] = i; toks[i] = 0; }
    uint32_t warm[5];
    int n_warm = 0;
    warm[n_warm++] = 1;
    const uint32_t lo[3] = {2, 5, 9}, hi[3] = {4, 8, (uint32_t)kMaxBatch};
    for (int b = 0; b < 3 && max_batch >= lo[b]; b++) {
      const uint32_t top = std::min(hi[b], max_batch), g = moe_group_min();
      if (b == 0 || !(Bs.moe_act && lo[b] < g && g <= top)) warm[n_warm++] = lo[b];
      if (Bs.moe_act && lo[b] < g && g <= top) warm[n_warm++] = g;
    }
    for (int i = 0; i < n_warm; i++) {
      if ((rc = stage_words(c, slots, toks, warm[i]))) return rc;
      if ((rc = enqueue_multi(c, warm[i], 1))) return rc;
      HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
    }
  }
  // the sampling kernels launched eagerly for every n_seq a step can have
  for (uint32_t n = 1; n <= max_batch; n++)
    if ((rc = samp_warm(c, Bs.samp, Bs.logits, n))) return rc;
  Bs.ready = true;   // (only now: a context whose warm-up failed takes no step)
  return LGH_OK;
}

int lgh_batch_reset(lgh_ctx* c, uint32_t slot) {   // create_active_sequence: a fresh context for the slot (O(1): position rewind)
  int rc = check_ready(c);
  if (rc) return rc;
  if (!c->batch.ready || slot >= c->batch.max_batch) return fail(c, LGH_INVALID_ARGUMENT, "no such slot");
  c->batch.pos[slot] = 0;
  return LGH_OK;
}

size_t lgh_batch_position(lgh_ctx* c, uint32_t slot) {
  if (!c || !c->batch.ready || slot >= c->batch.max_batch) return 0;
  return c->batch.pos[slot];
}

int lgh_forward_multi(lgh_ctx* c, const uint32_t* slots, const uint32_t* tokens, uint32_t n_seq, float* logits_out, uint32_t* next_tokens) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!slots || !tokens) return fail(c, LGH_INVALID_ARGUMENT, "slots / tokens is NULL");
  if ((rc = stage_control(c, slots, tokens, n_seq))) return rc;
  if ((rc = run_multi(c, n_seq, next_tokens != nullptr ? 1 : 0))) return rc;
  BatchScratch& Bs = c->batch;
  if (logits_out)
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(logits_out, Bs.logits, (size_t)n_seq * c->d.vocab_size * 4, hipMemcpyDeviceToHost, c->stream));
  if (next_tokens) HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(next_tokens, Bs.d_tokens, (size_t)n_seq * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  for (uint32_t i = 0; i < n_seq; i++) Bs.pos[slots[i]] += 1;
  c->stats.tokens_processed += n_seq;
  return LGH_OK;
}

int lgh_decode_greedy_multi(lgh_ctx* c, const uint32_t* slots, const uint32_t* first_tokens, uint32_t n_seq, size_t n_steps, uint32_t* tokens_out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!slots || !first_tokens) return fail(c, LGH_INVALID_ARGUMENT, "slots / first_tokens is NULL");
  BatchScratch& Bs = c->batch;
  if (Bs.ready)
    for (uint32_t i = 0; i < n_seq && i < (uint32_t)kMaxBatch; i++)
      if (slots[i] < Bs.max_batch && Bs.pos[slots[i]] + n_steps > c->d.max_seq_len) return fail(c, LGH_INVALID_ARGUMENT, "the steps would run past max_seq_len");
  if (n_steps > c->d.max_seq_len) return fail(c, LGH_INVALID_ARGUMENT, "too many steps");
  if ((rc = stage_control(c, slots, first_tokens, n_seq))) return rc;
  return decode_multi(c, slots, n_seq, 1, n_steps, tokens_out);
}

int lgh_batch_set_sampler_ex(lgh_ctx* c, uint32_t slot, const lgh_sampler_config_ex* cfg) {
  int rc = check_ready(c);
  if (rc) return rc;
  BatchScratch& Bs = c->batch;
  if (!Bs.ready || slot >= Bs.max_batch || slot >= Bs.samp_set.size()) return fail(c, LGH_INVALID_ARGUMENT, "no such slot");
  if ((rc = samp_check_ex(c, cfg))) return rc;
  if ((rc = samp_reset(c, Bs.samp, slot, *cfg))) return rc;
  Bs.samp_cfg[slot] = *cfg;
  Bs.samp_set[slot] = 1;
  return LGH_OK;
}

int lgh_batch_set_sampler(lgh_ctx* c, uint32_t slot, const lgh_sampler_config* cfg) {
  if (!cfg) return lgh_batch_set_sampler_ex(c, slot, nullptr);   // (refused there, after the context's and the slot's checks)
  const lgh_sampler_config_ex x = samp_plain(*cfg);
  return lgh_batch_set_sampler_ex(c, slot, &x);
}

int lgh_decode_sample_multi(lgh_ctx* c, const uint32_t* slots, const uint32_t* first_tokens, uint32_t n_seq, const uint32_t* histories,
                            const size_t* history_lens, size_t n_steps, const float* uniforms, uint32_t* tokens_out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!slots || !first_tokens) return fail(c, LGH_INVALID_ARGUMENT, "slots / first_tokens is NULL");
  BatchScratch& Bs = c->batch;
  if (!Bs.ready) return fail(c, LGH_INVALID_ARGUMENT, "lgh_batch_create has not been called");
  // (the count and the slot numbers' range, before the slots' samplers are looked at; stage_control below checks the rest)
  if (const SeqFault f = check_seqs(n_seq, Bs.max_batch, slots, Bs.max_batch, false, nullptr, 0))
    return fail(c, LGH_INVALID_ARGUMENT, f == SEQ_COUNT ? "n_seq must be 1 .. max_batch" : "slot numbers must be distinct and below max_batch");
  if (n_steps > c->d.max_seq_len) return fail(c, LGH_INVALID_ARGUMENT, "too many steps");
  if (Bs.samp_set.size() != Bs.max_batch || Bs.samp_cfg.size() != Bs.max_batch) return fail(c, LGH_INVALID_ARGUMENT, "no samplers");
  size_t hist_off[kMaxBatch];
  size_t off = 0;
  for (uint32_t i = 0; i < n_seq; i++) {
    if (!Bs.samp_set[slots[i]]) return fail(c, LGH_INVALID_ARGUMENT, "slot " + std::to_string(slots[i]) + ": lgh_batch_set_sampler has not been called");
    if (Bs.pos[slots[i]] + n_steps > c->d.max_seq_len) return fail(c, LGH_INVALID_ARGUMENT, "the steps would run past max_seq_len");
    const lgh_sampler_config_ex& g = Bs.samp_cfg[slots[i]];
    if (n_steps && !uniforms && samp_needs_uniforms(g)) return fail(c, LGH_INVALID_ARGUMENT, "uniforms is NULL");
    const size_t n = history_lens ? history_lens[i] : 0;
    if (n && !histories) return fail(c, LGH_INVALID_ARGUMENT, "histories is NULL");
    hist_off[i] = off;
    off += n;
  }
  if ((rc = stage_control(c, slots, first_tokens, n_seq))) return rc;   // (checks the slots and tokens)
  if (n_steps == 0) return LGH_OK;
  for (uint32_t i = 0; i < n_seq; i++)
    if ((rc = samp_begin(c, Bs.samp, slots[i], Bs.samp_cfg[slots[i]], histories ? histories + hist_off[i] : nullptr,
                         history_lens ? history_lens[i] : 0, first_tokens[i], n_steps, uniforms ? uniforms + i : nullptr, n_seq)))
      return rc;
  return decode_multi(c, slots, n_seq, 2, n_steps, tokens_out);
}

}  // extern "C"
