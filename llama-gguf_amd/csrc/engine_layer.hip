// engine_layer.hip — the per-token launch sequence of the single-sequence engine: one transformer layer as three steps on views of
// one sequence's vectors (qkv_forward, attention_forward, ffn_forward; the per-op test entry points of ops_api.hip run these same
// functions), and everything one token needs around the layers (enqueue_token).  The attention step is the multi-sequence engine's
// too (attention_forward_multi: the same function over the batch scratch).
#include "engine.h"
#include "xq.h"

#include <algorithm>
#include <cmath>

using namespace lgh;

namespace lgh {
hipError_t kv_store_launch(const float* k, const float* v, float* kcache, float* vcache, uint32_t n_kv, uint32_t d,
                           uint32_t max_seq, const int* pos, hipStream_t st);
}

// RoPE table [max_seq][head_dim / 2][cos, sin] in the reference's own arithmetic (ops.rs:1303-1313): libm powf / cosf / sinf on the host
void rope_table_host(const lgh_model_desc& d, std::vector<float>& cs) {
  const uint32_t half = d.head_dim / 2;
  cs.assign((size_t)d.max_seq_len * half * 2, 0.0f);
  for (uint32_t p = 0; p < d.max_seq_len; p++) {
    const float position = (float)p / d.rope_freq_scale;
    for (uint32_t i = 0; i < half; i++) {
      const float freq = 1.0f / std::pow(d.rope_freq_base, (float)(2 * i) / (float)d.head_dim);
      const float theta = position * freq;
      cs[((size_t)p * half + i) * 2] = std::cos(theta);
      cs[((size_t)p * half + i) * 2 + 1] = std::sin(theta);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// the FFN half of a layer on one sequence's vectors: FeedForward::forward (layers.rs:908-929) or MoeLayer::forward
// (moe.rs:321-413), residual included.  The single-sequence path passes the context's own buffers; the multi-sequence path
// (engine_batch.hip) runs MoE layers through here sequence by sequence — every sequence selects its own experts.
// ------------------------------------------------------------------------------------------------
// The dense FFN up to its activation: v.act = silu(gate x') * (up x'), x' = RMSNorm(v.hidden) with ffn_norm (layers.rs:908-925).  What
// follows is the down projection — ffn_forward's, with the residual, or a tensor-parallel rank's over its k-shard (tensor_parallel.hip).
int ffn_gateup_forward(lgh_ctx* c, LayerW& Lw, const FfnView& v) {
  int rc;
  if (fused_type(Lw.gate.type) && Lw.gate.type == Lw.up.type) {  // FeedForward::forward (layers.rs:908-929)
    SegSpec sp;
    sp.npass = 2;
    sp.W[0] = &Lw.gate; sp.W[1] = &Lw.up;
    sp.x[0] = sp.x[1] = v.hidden;
    sp.epi = EPI_SWIGLU;
    sp.out = v.act;
    sp.xq_next = mfma_type(Lw.down.type) ? 1 : 0;
    return launch_mv(c, LGH_K_GATEUP, &sp, 1, Lw.ffn_norm, c->d.hidden_size);
  }
  if ((rc = linear_any(c, LGH_K_GATEUP, Lw.gate, v.hidden, v.act, Lw.ffn_norm, nullptr, nullptr))) return rc;
  if ((rc = linear_any(c, LGH_K_GATEUP, Lw.up, v.hidden, v.act2, Lw.ffn_norm, nullptr, nullptr))) return rc;
  if ((rc = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, 0, [&] { return silu_mul_launch(v.act, v.act2, v.act, Lw.gate.n, c->stream); }))) return rc;
  xq_stale(c, v.act);
  return LGH_OK;
}

int ffn_forward(lgh_ctx* c, LayerW& Lw, const FfnView& v, const float* next_nw, bool next_mfma) {
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size;
  int rc;
  // ---- FFN
  if (!Lw.moe()) {
    if ((rc = ffn_gateup_forward(c, Lw, v))) return rc;
    return linear_any(c, LGH_K_DOWN, Lw.down, v.act, v.hidden, nullptr, v.hidden, nullptr, next_mfma ? 2 : 0, next_nw);
  }
  // ---- MoE (moe.rs:321-413): router + top-k on device, experts selected by device-side index
  const uint32_t topk = d.num_experts_per_token;
  if ((rc = run_k(c, LGH_K_ROUTER, LGH_SYM_ROUTER, (uint64_t)d.num_experts * H * 4, [&] {
         return moe_router_launch(v.hidden, Lw.ffn_norm, d.norm_eps, Lw.router, H, d.num_experts, topk, v.moe_sel, v.moe_w, c->stream);
       })))
    return rc;
  return moe_experts_forward(c, Lw, v, next_nw, next_mfma);
}

// The expert half of MoeLayer::forward: the num_experts_per_token experts in v.moe_sel (device), weighted by v.moe_w, plus the residual.
int moe_experts_forward(lgh_ctx* c, LayerW& Lw, const FfnView& v, const float* next_nw, bool next_mfma) {
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size;
  const uint32_t topk = d.num_experts_per_token;
  int rc;
  if (!fused_type(Lw.gate_exps.type) || Lw.gate_exps.type != Lw.up_exps.type || !fused_type(Lw.down_exps.type) || topk > 8)
    return fail(c, LGH_UNSUPPORTED, "MoE needs fused-format experts and top-k <= 8");
  // The selected experts run two at a time (a launch carries up to four passes: gate and up of two experts).  Every group
  // reads the SAME normalised h, so the running sum lives in a scratch vector until the last group writes the residual
  // stream: tmp = 0 + w0 e0 + w1 e1; tmp = tmp + w2 e2 + w3 e3; ...; h = (tmp + ...) + h — moe.rs:363-368's order exactly:
  // one sum over the weighted expert outputs in selection order, then the residual.
  for (uint32_t g0 = 0; g0 < topk; g0 += 2) {
    const uint32_t ng = std::min(2u, topk - g0);
    const bool first_g = g0 == 0, last_g = g0 + ng >= topk;
    {
      SegSpec sp;
      sp.npass = (int)(2 * ng);
      for (uint32_t s = 0; s < ng; s++) {
        sp.W[2 * s] = &Lw.gate_exps; sp.W[2 * s + 1] = &Lw.up_exps;
        sp.x[2 * s] = sp.x[2 * s + 1] = v.hidden;
        sp.sel[2 * s] = sp.sel[2 * s + 1] = v.moe_sel + g0 + s;
      }
      sp.epi = EPI_MOE_SWIGLU;
      sp.out = v.act; sp.out2 = v.act2;
      sp.xq_next = mfma_type(Lw.down_exps.type) ? 1 : 0;
      if ((rc = launch_mv(c, LGH_K_GATEUP, &sp, 1, Lw.ffn_norm, H))) return rc;
    }
    {
      SegSpec sp;
      sp.npass = (int)ng;
      for (uint32_t s = 0; s < ng; s++) {
        sp.W[s] = &Lw.down_exps;
        sp.x[s] = s == 0 ? v.act : v.act2;
        sp.sel[s] = v.moe_sel + g0 + s;
      }
      sp.epi = EPI_MOE_DOWN;
      sp.out = last_g ? v.hidden : v.xnorm;
      sp.out2 = first_g ? nullptr : v.xnorm;     // (EPI_MOE_DOWN: the running sum of the earlier groups)
      sp.resid = last_g ? v.hidden : nullptr;
      sp.moe_w = v.moe_w + g0;
      sp.xq_next = last_g && next_mfma ? 2 : 0; sp.xq_next_nw = next_nw;
      if ((rc = launch_mv(c, LGH_K_DOWN, &sp, 1, nullptr, Lw.down_exps.k))) return rc;
    }
  }
  return LGH_OK;
}

// ------------------------------------------------------------------------------------------------
// the attention half of a layer on one sequence's vectors, up to attn_out (layers.rs:438-600)
// ------------------------------------------------------------------------------------------------
int qkv_forward(lgh_ctx* c, LayerW& Lw, const AttnView& v) {
  const lgh_model_desc& d = c->d;
  int rc;
  const bool staged = c->kvl.staged();
  float* const k_new = v.kv_tmp;                                                     // staged formats: the current token's rotated K row ...
  float* const v_new = k_new ? k_new + (size_t)d.num_kv_heads * d.head_dim : nullptr;   // ... and V row, f32, quantized by the attention launch
  const bool fused = fused_type(Lw.wq.type) && fused_type(Lw.wk.type) && fused_type(Lw.wv.type) && !d.use_neox_rope;
  if (!k_new && (staged || !fused)) return fail(c, LGH_INVALID_ARGUMENT, "qkv_forward: this layer stages its K / V rows and the view has no kv_tmp");
  if (fused) {
    SegSpec sp[3];
    sp[0].W[0] = &Lw.wq; sp[0].x[0] = v.hidden; sp[0].epi = EPI_ROPE_Q; sp[0].out = v.q; sp[0].bias = Lw.bq;
    sp[1].W[0] = &Lw.wk; sp[1].x[0] = v.hidden; sp[1].epi = staged ? EPI_ROPE_Q : EPI_ROPE_K; sp[1].out = staged ? k_new : Lw.kv.k_f32(); sp[1].bias = Lw.bk;
    sp[2].W[0] = &Lw.wv; sp[2].x[0] = v.hidden; sp[2].epi = staged ? EPI_STORE : EPI_V_CACHE; sp[2].out = staged ? v_new : Lw.kv.v_f32(); sp[2].bias = Lw.bv;
    return launch_mv(c, LGH_K_QKV, sp, 3, Lw.attn_norm, d.hidden_size);
  }
  if ((rc = linear_any(c, LGH_K_QKV, Lw.wq, v.hidden, v.q, Lw.attn_norm, nullptr, Lw.bq))) return rc;
  if ((rc = linear_any(c, LGH_K_QKV, Lw.wk, v.hidden, k_new, Lw.attn_norm, nullptr, Lw.bk))) return rc;
  if ((rc = linear_any(c, LGH_K_QKV, Lw.wv, v.hidden, v_new, Lw.attn_norm, nullptr, Lw.bv))) return rc;
  xq_stale(c, v.q);
  if ((rc = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, 0, [&] {
         return rope_launch(v.q, k_new, d.num_heads, d.num_kv_heads, d.head_dim, c->state + ST_POS, c->rope_cs, (int)d.use_neox_rope, c->stream);
       })))
    return rc;
  if (staged) return LGH_OK;
  return run_k(c, LGH_K_MISC, LGH_SYM_OTHER, 0, [&] {
    return kv_store_launch(k_new, v_new, Lw.kv.k_f32(), Lw.kv.v_f32(), d.num_kv_heads, d.head_dim, d.max_seq_len, c->state + ST_POS, c->stream);
  });
}

// Where a decode-attention step's vectors live: the context's own sequence (n_seq 0: an AttnView, the context's partials and position
// word, the layer's cache) or the n_seq sequences of a multi-sequence step side by side in the batch scratch, over the layer's slots
struct AttnStep {
  const float *q, *kv_new;
  float *out, *part_ml, *part_acc;
  const int *pos, *slot;
  const KvCache& kv;
  uint32_t n_seq;
};
static AttnStep attn_step_own(const lgh_ctx* c, const LayerW& Lw, const AttnView& v) {
  return {v.q, v.kv_tmp, v.attn_out, c->part_ml, c->part_acc, c->state + ST_POS, nullptr, Lw.kv, 0};
}
static AttnStep attn_step_batch(const lgh_ctx* c, uint32_t li, uint32_t n_seq) {
  const BatchScratch& Bs = c->batch;
  return {Bs.q, Bs.kv_tmp, Bs.attn_out, Bs.part_ml, Bs.part_acc, Bs.d_pos, Bs.d_slot, Bs.kv[li], n_seq};
}

// wo's input as XQ records, where the caller asks for it: the image the step's last launch writes.  Own sequence: the output's image,
// registered at first use; batch: sequence 0's registered view, the others' follow at xq_stride_of (nullptr: no views, no image)
static XqBuf* attn_image(lgh_ctx* c, const AttnStep& s, bool xq_out) {
  if (!xq_out) return nullptr;
  return s.n_seq ? xq_find(c, s.out) : xq_get(c, s.out, c->d.num_heads * c->d.head_dim);
}
// ... and the registry after the step: the image(s) fresh with no norm weights in them, or the output's image(s) stale
static void attn_image_done(lgh_ctx* c, const AttnStep& s, XqBuf* qa) {
  const uint32_t QD = c->d.num_heads * c->d.head_dim;
  if (s.n_seq && qa) return mark_fresh(c, s.out, QD, s.n_seq, nullptr);
  if (qa) { qa->fresh = true; qa->tag = nullptr; }
  else
    for (uint32_t i = 0; i < std::max(s.n_seq, 1u); i++) xq_stale(c, s.out + (size_t)i * QD);
}

// attention_cached (ops.rs:1479-1537) over layer li's cache, whatever its format and for either engine: one branch per path, each ending
// in the launch that writes the output — and, where that launch can and the caller asks, wo's input as XQ straight from it
static int attention_step(lgh_ctx* c, uint32_t li, const AttnStep& s, float scale, bool xq_out) {
  const lgh_model_desc& d = c->d;
  int rc;
  const KvLayout& kvl = c->kvl;
  const uint64_t kv_bytes = s.n_seq ? 0 : kvl.launch_bytes(c->pos + 1);
  const bool one_launch = !s.n_seq && kvl.f32();   // the context's own f32 cache: the paths of one launch, by the context's fields
  XqBuf* qa = nullptr;
  if (one_launch && c->attn_generic) {   // any head size / group size: f32 out, no image
    rc = run_k(c, LGH_K_ATTN, LGH_SYM_ATTN, kv_bytes, [&] {
      return attn_decode_any_launch(s.q, s.kv.k_f32(), s.kv.v_f32(), s.out, d.num_heads, d.num_kv_heads, d.head_dim, d.max_seq_len, scale, s.pos, c->stream);
    });
  } else if (one_launch && c->attn_direct == ATTN_VAR_HEAD) {   // contexts up to direct_attn_max_kv rows: one launch, a workgroup per query head
    if (c->pos + 1 > c->direct_attn_max_kv)   // (the kernel's LDS arrays end there: it would attend to a truncated context)
      return fail(c, LGH_INVALID_ARGUMENT, "single-launch attention at position " + std::to_string(c->pos) + " past its " +
                                               std::to_string(c->direct_attn_max_kv) + " rows");
    qa = attn_image(c, s, xq_out);
    rc = run_k(c, LGH_K_ATTN, LGH_SYM_ATTN, kv_bytes, [&] {
      return attn_head_launch(s.q, s.kv.k_f32(), s.kv.v_f32(), d.num_heads, d.num_kv_heads, d.head_dim, d.max_seq_len, scale, s.pos, c->direct_attn_max_kv,
                              s.out, qa ? qa->xq : nullptr, c->stream);
    });
  } else if (one_launch && c->attn_direct == ATTN_VAR_DIRECT) {   // one launch, a workgroup per kv head
    qa = attn_image(c, s, xq_out);
    rc = run_k(c, LGH_K_ATTN, LGH_SYM_ATTN, kv_bytes, [&] {
      return attn_direct_launch(s.q, s.kv.k_f32(), s.kv.v_f32(), d.num_heads, d.num_kv_heads, d.head_dim, d.max_seq_len, scale, s.pos, s.out,
                                qa ? qa->xq : nullptr, c->stream);
    });
  } else {
    // n_splits ranges of the context, then their merge.  The launchers take the format from the layout: the staged formats' partial
    // launch also compresses and stores the current token's rows (kv_quantized.rs, kv_turboquant.rs write_kv), the TurboQuant merge also
    // inverts the V rotation
    AttnDecode a{};
    a.n_heads = d.num_heads; a.scale = scale;
    a.q = s.q; a.kv_new = s.kv_new;
    a.pos = s.pos; a.slot = s.slot; a.n_seq = s.n_seq;
    a.n_splits = c->n_splits; a.part_ml = s.part_ml; a.part_acc = s.part_acc;
    if (kvl.tq()) { const TqLayer t = tq_layer(c, li); a.signs = t.signs; a.qjl_s = t.qjl_s; }
    a.out = s.out;
    a.st = c->stream;
    if ((rc = run_k(c, LGH_K_ATTN, LGH_SYM_ATTN, kv_bytes, [&] { return attn_split_launch(kvl, s.kv, a); }))) return rc;
    qa = attn_image(c, s, xq_out);
    a.xq_out = qa ? qa->xq : nullptr;
    a.xq_stride = s.n_seq ? xq_stride_of(d.num_heads * d.head_dim) : 0;
    rc = run_k(c, LGH_K_ATTN_COMBINE, LGH_SYM_ATTN_COMBINE, 0, [&] { return attn_merge_launch(kvl, a); });
  }
  if (rc) return rc;
  attn_image_done(c, s, qa);
  return LGH_OK;
}

int attention_forward(lgh_ctx* c, LayerW& Lw, uint32_t li, const AttnView& v, float scale, bool xq_out) {
  return attention_step(c, li, attn_step_own(c, Lw, v), scale, xq_out);
}
int attention_forward_multi(lgh_ctx* c, uint32_t li, uint32_t n_seq, float scale, bool xq_out) {
  return attention_step(c, li, attn_step_batch(c, li, n_seq), scale, xq_out);
}

// ------------------------------------------------------------------------------------------------
// one transformer layer (TransformerLayer::forward serial-residual branch, layers.rs:1187-1244)
// ------------------------------------------------------------------------------------------------
// `next_nw` / `next_mfma`: the norm weights and kernel family of whatever consumes this layer's output (the next layer's
// QKV, or the output projection)
static int layer_forward(lgh_ctx* c, uint32_t li, const float* next_nw, bool next_mfma) {
  LayerW& Lw = c->layers[li];
  const AttnView av{c->hidden, c->q, c->kv_tmp, c->attn_out};
  int rc;
  if ((rc = qkv_forward(c, Lw, av))) return rc;
  if ((rc = attention_forward(c, Lw, li, av, 1.0f / std::sqrt((float)c->d.head_dim), mfma_type(Lw.wo.type)))) return rc;   // scale: layers.rs:374
  // ---- h = x + wo(attn)   (layers.rs:700-701, 1201-1208)
  const bool ffn_mfma = Lw.moe() ? mfma_type(Lw.gate_exps.type) : mfma_type(Lw.gate.type);
  if ((rc = linear_any(c, LGH_K_WO, Lw.wo, c->attn_out, c->hidden, nullptr, c->hidden, Lw.bo, ffn_mfma ? 2 : 0, Lw.ffn_norm))) return rc;
  if (c->profiling) {  // an EMPTY event bracket in mid-stream: what the measurement itself adds to every sample (at the
    // head of a token, on an idle stream, the same bracket reads differently from run to run)
    if ((rc = run_k(c, -1, -1, 0, [&] { return hipSuccess; }))) return rc;
  }
  return ffn_forward(c, Lw, FfnView{c->hidden, c->act, c->act2, c->xnorm, c->moe_sel, c->moe_w}, next_nw, next_mfma);
}

// Opens a token on a context that holds the embedding table: the row of the token in the device state into c->hidden (and the position
// advanced), and — when the first layer's QKV runs on the matrix cores — its XQ image with that layer's norm weights
int embed_forward(lgh_ctx* c) {
  const lgh_model_desc& d = c->d;
  XqBuf* qh = nullptr;
  const float* nw0 = nullptr;
  if (c->l0 < c->l1 && mfma_type(c->layers[c->l0].wq.type) && d.hidden_size % 256 == 0) {
    qh = xq_get(c, c->hidden, d.hidden_size);
    nw0 = c->layers[c->l0].attn_norm;
  }
  if (int rc = run_k(c, LGH_K_EMBED, LGH_SYM_EMBED, (uint64_t)d.hidden_size * blk_bytes(c->embd_type) / blk_elems(c->embd_type), [&] {
        return embed_launch(c->embd_type, c->embd_raw, c->state + ST_TOKEN, c->hidden, d.hidden_size, c->state,
                            qh ? qh->xq : nullptr, nw0, qh ? qh->ssq : nullptr, c->stream);
      }))
    return rc;
  if (qh) { qh->fresh = true; qh->tag = nw0; }
  return LGH_OK;
}

// Everything one token needs, in stream order.  Used eagerly and under graph capture.
int enqueue_token(lgh_ctx* c, int mode) {
  const lgh_model_desc& d = c->d;
  int rc;
  for (auto& q : c->xqs) q.fresh = false;   // the residual stream is (re)written in f32 now (embedding / previous stage)
  if (c->first) {
    if ((rc = embed_forward(c))) return rc;
  } else {
    if ((rc = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, 0, [&] { return advance_launch(c->state, c->stream); }))) return rc;
  }
  for (uint32_t li = c->l0; li < c->l1; li++) {
    // who consumes this layer's output: the next layer's QKV (attn_norm), the output projection (output_norm), or — at a
    // pipeline-stage boundary and at the end of a prefill step — nobody on this device
    const float* next_nw = nullptr;
    bool next_mfma = false;
    if (li + 1 < c->l1) {
      next_nw = c->layers[li + 1].attn_norm;
      next_mfma = mfma_type(c->layers[li + 1].wq.type);
    } else if (c->last && mode != MODE_PREFILL) {
      next_nw = c->output_norm;
      next_mfma = mfma_type(c->output.type);
    }
    if ((rc = layer_forward(c, li, next_nw, next_mfma))) return rc;
  }
  if (c->last && mode != MODE_PREFILL) {
    // compute_logits (llama.rs:247-266): final RMSNorm fused into the output projection
    // Greedy: a static-plan output projection leaves each workgroup's arg-max part next to the logits, and only the merge follows.
    uint32_t parts = 0;
    const bool greedy = mode == MODE_GREEDY;
    if ((rc = linear_any(c, LGH_K_OUTPUT, c->output, c->hidden, c->logits, c->output_norm, nullptr, nullptr, 0, nullptr, greedy ? c->amax_v : nullptr,
                         greedy ? c->amax_i : nullptr, greedy ? &parts : nullptr)))
      return rc;
    if (mode == MODE_GREEDY) {
      if ((rc = run_k(c, LGH_K_ARGMAX, LGH_SYM_ARGMAX, parts ? (uint64_t)parts * 8 : (uint64_t)d.vocab_size * 4, [&] {
             return parts ? argmax_merge_launch(c->amax_v, c->amax_i, parts, c->state, c->tok_log, c->stream)
                          : argmax_launch(c->logits, d.vocab_size, c->amax_v, c->amax_i, c->state, c->tok_log, c->stream);
           })))
        return rc;
    } else if (mode == MODE_SAMPLE) {   // Sampler::sample in place of the arg-max (sample.hip); the token lands where the arg-max's does
      if ((rc = run_k(c, LGH_K_ARGMAX, LGH_SYM_OTHER, (uint64_t)d.vocab_size * 4, [&] {
             return sample_launch(c->samp, c->logits, d.vocab_size, 1, nullptr, c->state, c->tok_log, nullptr, c->stream);
           })))
        return rc;
    }
  }
  // in-graph hops to a stage on the same device (lgh_stage_set_forward_targets)
  if (c->fwd_hidden && !c->last &&
      (rc = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, (uint64_t)d.hidden_size * 8, [&] { return copy_words_launch(c->fwd_hidden, c->hidden, d.hidden_size, c->stream); })))
    return rc;
  if (c->fwd_token && c->last && mode == MODE_GREEDY &&
      (rc = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, 8, [&] { return copy_words_launch(c->fwd_token, c->state + ST_ARGMAX, 1, c->stream); })))
    return rc;
  return LGH_OK;
}
