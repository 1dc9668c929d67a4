// engine_prefill.hip — the batched prompt driver: which contexts have the path (pf_eligible), its scratch (pf_ensure) and one block
// of up to 128 prompt tokens through every owned layer (prefill_block), for the context's own sequence or a slot of the
// multi-sequence engine.
#include "engine.h"
#include "prefill.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace lgh;

// ------------------------------------------------------------------------------------------------
// batched prompt processing (prefill.hip)
// ------------------------------------------------------------------------------------------------
bool pf_eligible(const lgh_ctx* c, bool slot) {
  const lgh_model_desc& d = c->d;
  if (d.flags & LGH_FLAG_EXACT_PREFILL) return false;
  // The batched path writes f32 K/V rows.  The f32 cache takes them as they are; a TurboQuantMSE cache (tq2 / tq3) takes them through an
  // f32 scratch (pf_tq_rows below), for the own sequence of a context that owns every layer.  A byte cache (int8 / FP8) takes them
  // through a scratch of the block's rows and a store launch (pf_kv8_store below), own sequence, slots and stage contexts alike, on
  // a context that opted in (lgh_set_prefill_policy): the pass is not bit-identical to the token-by-token one.  The QJL formats, and
  // slots of the multi-sequence engine and stage contexts with a TurboQuant cache, stay token by token.
  if (c->kvl.tq()) {
    if (d.kv_cache_type != LGH_KV_TQ2 && d.kv_cache_type != LGH_KV_TQ3) return false;
    if (slot || !c->first || !c->last) return false;
  } else if (c->kvl.staged() && !(c->pf_policy & LGH_PREFILL_BATCH_BYTE_KV)) {
    return false;
  }
  const uint32_t QD = d.num_heads * d.head_dim, KD = d.num_kv_heads * d.head_dim, g = d.num_heads / d.num_kv_heads;
  if (d.hidden_size % 256 || d.hidden_size > 2048u * kPfSsqChunks || QD % 256 || KD % 16) return false;
  if ((d.head_dim != 64 && d.head_dim != 128) || (g != 1 && g != 2 && g != 4 && g != 8)) return false;
  for (uint32_t i = c->l0; i < c->l1; i++) {
    const LayerW& L = c->layers[i];
    for (const DevWeight* W : {&L.wq, &L.wk, &L.wv, &L.wo})
      if (!pf_supported_type(W->type) || W->n % 16) return false;
    if (L.moe()) {   // experts: tokens are grouped by expert (prefill.hip); up to 8 selected, at most 64 experts
      if (d.num_experts > (uint32_t)kPfMaxExperts || d.num_experts_per_token == 0 || d.num_experts_per_token > (uint32_t)kPfMaxTopK ||
          (uint32_t)kPfTokens * d.num_experts_per_token + 15 * d.num_experts > (uint32_t)kPfMoeRows)
        return false;
      for (const DevWeight* W : {&L.gate_exps, &L.up_exps, &L.down_exps})
        if (!pf_supported_type(W->type) || W->n % 16 || W->k % 256) return false;
    } else {
      if (d.intermediate_size % 256) return false;
      for (const DevWeight* W : {&L.gate, &L.up, &L.down})
        if (!pf_supported_type(W->type) || W->n % 16) return false;
    }
  }
  return true;
}

// a byte cache (the context reaches the batched path with one only through the policy: pf_eligible)
static bool pf_kv8(const lgh_ctx* c) { return c->kvl.staged() && !c->kvl.tq(); }

int pf_ensure(lgh_ctx* c) {
  PfScratch& P = c->pf;
  if (P.ready) return LGH_OK;
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size, QD = d.num_heads * d.head_dim, KD = d.num_kv_heads * d.head_dim;
  bool any_moe = false, any_dense = false;
  for (uint32_t i = c->l0; i < c->l1; i++) (c->layers[i].moe() ? any_moe : any_dense) = true;
  const uint32_t F = any_dense ? d.intermediate_size : 0;
  const uint32_t EI = any_moe ? (d.expert_intermediate_size ? d.expert_intermediate_size : d.intermediate_size) : 0;
  const uint32_t qkv[3] = {QD, KD, KD}, one[1] = {H};
  size_t pb = pf_part_bytes(qkv, 3, H);
  pb = std::max(pb, pf_part_bytes(one, 1, QD));
  if (F) { const uint32_t gu[2] = {F, F}; pb = std::max({pb, pf_part_bytes(gu, 2, H), pf_part_bytes(one, 1, F)}); }
  if (EI) { const uint32_t gu[2] = {EI, EI}; pb = std::max({pb, pf_part_bytes(gu, 2, H, kPfMoeRows), pf_part_bytes(one, 1, EI, kPfMoeRows)}); }
  const uint32_t topk = d.num_experts_per_token ? d.num_experts_per_token : 1;
  const AllocSpec bufs[] = {
      {(void**)&P.xh_h, xh_bytes(H)},           {(void**)&P.xh_attn, xh_bytes(QD)},
      {(void**)&P.xh_act, xh_bytes(std::max(F, EI))}, {(void**)&P.hidden, (size_t)kPfTokens * H * 4},
      {(void**)&P.q, (size_t)kPfTokens * QD * 4},
      {(void**)&P.part, pb},                    {(void**)&P.tokens, (size_t)kPfTokens * 4},
      {(void**)&P.ssq, (size_t)kPfTokens * kPfSsqChunks * 4},
      {(void**)&P.moe_sel, any_moe ? (size_t)kPfTokens * topk * 4 : 0},  {(void**)&P.moe_w, any_moe ? (size_t)kPfTokens * topk * 4 : 0},
      {(void**)&P.moe_cnt, any_moe ? (size_t)kPfMaxExperts * 4 : 0},    {(void**)&P.moe_list, any_moe ? (size_t)kPfMaxExperts * kPfTokens * 4 : 0},
      {(void**)&P.moe_base, any_moe ? (size_t)kPfMaxExperts * 4 : 0},   {(void**)&P.moe_rowmap, any_moe ? (size_t)kPfMoeRows * 4 : 0},
      {(void**)&P.moe_tokmap, any_moe ? (size_t)kPfTokens * kPfMaxTopK * 4 : 0},
      {(void**)&P.xh_gather, any_moe ? xh_bytes(H) * d.num_experts : 0}, {(void**)&P.xh_act_e, any_moe ? xh_bytes(EI) * d.num_experts : 0},
      {(void**)&P.tq_kv, c->kvl.tq() ? (size_t)2 * c->kvl.stride_floats() * 4 : 0},   // (scratch, not KV bytes)
      {(void**)&P.kv8_rows, pf_kv8(c) ? (size_t)2 * d.num_kv_heads * kPfTokens * d.head_dim * 4 : 0},   // (the block only; scratch too)
  };
  if (int rc = alloc_zeroed(c, bufs, sizeof(bufs) / sizeof(bufs[0]), c->stats.scratch_bytes)) return rc;
  // the zero-fills are done before anybody else (another stream, a peer's copy into the stage block) touches the buffers
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  P.part_bytes = pb;
  P.ready = true;
  return LGH_OK;
}

static int pf_k(lgh_ctx* c, hipError_t e, const char* what) {
  return e == hipSuccess ? LGH_OK : fail(c, LGH_OPERATION_FAILED, std::string("batched prefill, ") + what + ": " + hipGetErrorString(e));
}

// the block of hidden vectors in pf.hidden as it is -> XH(h * nw) in pf.xh_h, the tokens' sums of squares in pf.ssq
int pf_block_input(lgh_ctx* c, const float* nw, uint32_t m) {
  PfScratch& P = c->pf;
  return pf_k(c, pf_row_epi_launch(nullptr, 0, 0, 0, nullptr, P.hidden, c->d.hidden_size, nw, P.xh_h, P.ssq, m, c->stream), "attn_norm");
}

// ---- the steps of one layer over a block of m tokens, on the context's scratch (c->pf); prefill_block strings them together, the
// per-step test entry points (ops_api.hip) run them one at a time ----
// XH(h * attn_norm) in pf.xh_h + the tokens' sums of squares in pf.ssq -> q in pf.q, K / V rows pos0 .. pos0+m-1 of the given caches
int pf_qkv_step(lgh_ctx* c, LayerW& L, float* kcache, float* vcache, uint32_t pos0, uint32_t m, uint32_t cache_rows) {
  PfScratch& P = c->pf;
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size, QD = d.num_heads * d.head_dim, KD = d.num_kv_heads * d.head_dim;
  hipStream_t st = c->stream;
  int rc;
  uint32_t S = 0, nc = 0;
  const DevWeight* qkv[3] = {&L.wq, &L.wk, &L.wv};
  if ((rc = pf_k(c, pf_gemm_launch(qkv, 3, P.xh_h, P.part, P.part_bytes, m, &S, &nc, st), "qkv GEMM"))) return rc;
  return pf_k(c, pf_qkv_epi_launch(P.part, S, nc, QD, KD, d.head_dim, L.bq, L.bk, L.bv, c->rope_cs, pos0, cache_rows ? cache_rows : d.max_seq_len, P.q, kcache, vcache, P.ssq, H,
                                   d.norm_eps, (int)d.use_neox_rope, m, st),
              "qkv epilogue");
}

// TurboQuantMSE cache, after pf_qkv_step has left the block's f32 K / V rows in the scratch pf.tq_kv: their codes into layer li's code
// cache and their centroids back into the scratch (TurboQuantKVCache::write_kv); with `attend`, also the block's queries rotated in
// place and rows 0 .. pos0-1 of the scratch filled from the cached codes, which is what the block attention reads
static int pf_tq_rows(lgh_ctx* c, LayerW& L, uint32_t li, uint32_t pos0, uint32_t m, bool attend) {
  PfScratch& P = c->pf;
  const lgh_model_desc& d = c->d;
  float* const vscr = P.tq_kv + c->kvl.stride_floats();
  return pf_k(c, tq_pf_rows_launch(c->kvl.tq_bits(), P.tq_kv, vscr, L.kv.k_bytes(), L.kv.v_bytes(), attend ? P.q : nullptr, tq_layer(c, li).signs, d.num_heads,
                                   d.num_kv_heads, d.head_dim, d.max_seq_len, pos0, m, attend ? m : 0, attend ? pos0 : 0, c->stream),
              "TurboQuant rows");
}

// byte cache, after pf_qkv_step has left the block's f32 K / V rows in the scratch pf.kv8_rows: rows pos0 .. pos0+m-1 of the target's byte
// tensors (and scales), quantized as the decode attention quantizes a token's rows
static int pf_kv8_store(lgh_ctx* c, const KvCache& kv, uint32_t pos0, uint32_t m) {
  const lgh_model_desc& d = c->d;
  const float* const krows = c->pf.kv8_rows;
  return pf_k(c, kv8_pf_store_launch(d.kv_cache_type, krows, krows + (size_t)d.num_kv_heads * kPfTokens * d.head_dim, kPfTokens, kv, d.num_kv_heads, d.head_dim,
                                     d.max_seq_len, pos0, m, c->stream),
              "byte cache rows");
}

// q in pf.q + the stored rows 0 .. pos0+m-1 of layer li's cache kv (a TurboQuant cache: of the scratch pf.tq_kv) -> XH(attention output)
// in pf.xh_attn
int pf_attn_step(lgh_ctx* c, uint32_t li, const KvCache& kv, uint32_t pos0, uint32_t m) {
  PfScratch& P = c->pf;
  AttnBlock a{};
  a.n_heads = c->d.num_heads;
  a.scale = 1.0f / std::sqrt((float)c->d.head_dim);   // layers.rs:374
  a.q = P.q;
  a.pos0 = pos0;
  a.m_tokens = m;
  a.tq_kv = P.tq_kv;
  a.signs = c->kvl.tq() ? tq_layer(c, li).signs : nullptr;
  a.xh_out = P.xh_attn;
  a.st = c->stream;
  return pf_k(c, attn_block_launch(c->kvl, kv, a), "attention");
}

// XH(attention output) in pf.xh_attn -> pf.hidden += wo . attn (+ bo), XH(h * ffn_norm) in pf.xh_h, sums of squares in pf.ssq
int pf_wo_step(lgh_ctx* c, LayerW& L, uint32_t m) {
  PfScratch& P = c->pf;
  const uint32_t H = c->d.hidden_size;
  hipStream_t st = c->stream;
  int rc;
  uint32_t S = 0, nc = 0;
  const DevWeight* wo[1] = {&L.wo};
  if ((rc = pf_k(c, pf_gemm_launch(wo, 1, P.xh_attn, P.part, P.part_bytes, m, &S, &nc, st), "wo GEMM"))) return rc;
  return pf_k(c, pf_row_epi_launch(P.part, S, nc, 0, L.bo, P.hidden, H, L.ffn_norm, P.xh_h, P.ssq, m, st), "wo epilogue");
}

// dense FFN: XH(h * ffn_norm) in pf.xh_h -> pf.hidden += down . (silu(gate) * up); next_nw: the next layer's XH (h * next_nw) into
// pf.xh_h, nullptr: none (the block leaves as f32)
int pf_ffn_step(lgh_ctx* c, LayerW& L, const float* next_nw, uint32_t m) {
  PfScratch& P = c->pf;
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size, F = d.intermediate_size;
  hipStream_t st = c->stream;
  uint8_t* next_xh = next_nw ? P.xh_h : nullptr;
  int rc;
  uint32_t S = 0, nc = 0;
  const DevWeight* gu[2] = {&L.gate, &L.up};
  if ((rc = pf_k(c, pf_gemm_launch(gu, 2, P.xh_h, P.part, P.part_bytes, m, &S, &nc, st), "gate/up GEMM"))) return rc;
  if ((rc = pf_k(c, pf_swiglu_launch(P.part, S, F, P.xh_act, P.ssq, H, d.norm_eps, m, st), "SwiGLU"))) return rc;
  const DevWeight* dn[1] = {&L.down};
  if ((rc = pf_k(c, pf_gemm_launch(dn, 1, P.xh_act, P.part, P.part_bytes, m, &S, &nc, st), "down GEMM"))) return rc;
  return pf_k(c, pf_row_epi_launch(P.part, S, nc, 0, nullptr, P.hidden, H, next_nw, next_xh, P.ssq, m, st), "down epilogue");
}

// MoE FFN (moe.rs:321-413): route every token of the block (f32, the decode router), group the (token, slot) pairs by
// expert, and run each expert once over its rows: gather -> gate|up GEMM -> SwiGLU -> down GEMM -> rows back to tokens
int pf_moe_step(lgh_ctx* c, LayerW& L, const float* next_nw, uint32_t m) {
  PfScratch& P = c->pf;
  const lgh_model_desc& d = c->d;
  const uint32_t H = d.hidden_size;
  hipStream_t st = c->stream;
  uint8_t* next_xh = next_nw ? P.xh_h : nullptr;
  int rc;
  uint32_t S = 0, nc = 0;
  const uint32_t topk = d.num_experts_per_token, EI = L.gate_exps.n;
  if ((rc = pf_k(c, moe_router_launch(P.hidden, L.ffn_norm, d.norm_eps, L.router, H, d.num_experts, topk, P.moe_sel, P.moe_w, st, m), "router"))) return rc;
  if ((rc = pf_k(c, pf_moe_group_launch(P.moe_sel, m, topk, d.num_experts, P.moe_cnt, P.moe_base, P.moe_list, P.moe_rowmap, P.moe_tokmap, st), "expert grouping")))
    return rc;
  if ((rc = pf_k(c, pf_moe_gather_launch(P.xh_h, H, P.moe_list, P.moe_cnt, P.xh_gather, d.num_experts, st), "expert gather"))) return rc;
  for (uint32_t e = 0; e < d.num_experts; e++) {   // every expert's gate|up over its rows, partial sums side by side in one row space
    const DevWeight* gu[2] = {&L.gate_exps, &L.up_exps};
    if ((rc = pf_k(c, pf_gemm_launch(gu, 2, P.xh_gather + (size_t)e * xh_bytes(H), P.part, P.part_bytes, kPfTokens, &S, &nc, st, e, P.moe_cnt + e, kPfMoeRows,
                                     P.moe_base + e),
                   "expert gate/up GEMM")))
      return rc;
  }
  if ((rc = pf_k(c, pf_moe_swiglu_launch(P.part, S, EI, P.xh_act_e, P.moe_rowmap, P.moe_list, P.ssq, H, d.norm_eps, st), "expert SwiGLU"))) return rc;
  for (uint32_t e = 0; e < d.num_experts; e++) {
    const DevWeight* dn[1] = {&L.down_exps};
    if ((rc = pf_k(c, pf_gemm_launch(dn, 1, P.xh_act_e + (size_t)e * xh_bytes(EI), P.part, P.part_bytes, kPfTokens, &S, &nc, st, e, P.moe_cnt + e, kPfMoeRows,
                                     P.moe_base + e),
                   "expert down GEMM")))
      return rc;
  }
  // h += sum over the selected experts, in selection order, of routing weight * expert output (moe.rs:363-368), then the
  // next layer's input
  return pf_k(c, pf_moe_combine_launch(P.part, S, P.moe_tokmap, P.moe_w, topk, P.hidden, H, next_nw, next_xh, P.ssq, m, st), "MoE combine");
}

// the m token ids of a block at positions pos0 .. pos0+m-1 onto the device and their embedding rows into pf.hidden (after pf_ensure)
int pf_embed_tokens(lgh_ctx* c, uint32_t pos0, const uint32_t* tokens, uint32_t m) {
  PfScratch& P = c->pf;
  const lgh_model_desc& d = c->d;
  hipStream_t st = c->stream;
  // The caller's `tokens` may be freed as soon as this returns (lgh_stage_prefill_batch does not synchronise), so the ids
  // go through a context-owned PINNED buffer, one slot per position; a slot is only rewritten after the copy that last
  // read it has completed (reset + a second prompt before the first one has run).
  if (!P.tok_pinned) {
    HIP_TRY(c, LGH_ALLOCATION_FAILED, hipHostMalloc((void**)&P.tok_pinned, (size_t)d.max_seq_len * 4, hipHostMallocDefault));
    HIP_TRY(c, LGH_OPERATION_FAILED, hipEventCreateWithFlags(&P.tok_copied, hipEventDisableTiming));
  } else if (pos0 < P.tok_hi && pos0 + m > P.tok_lo) {
    // only when a slot about to be rewritten may still be read: a reset / shift / truncate followed by a new prompt.  The blocks
    // of ONE prompt use ascending slots and never wait here (lgh_stage_prefill_batch stays asynchronous).
    HIP_TRY(c, LGH_OPERATION_FAILED, hipEventSynchronize(P.tok_copied));
    P.tok_lo = P.tok_hi = 0;
  }
  if (P.tok_hi == P.tok_lo) { P.tok_lo = pos0; P.tok_hi = pos0 + m; }
  else { P.tok_lo = std::min(P.tok_lo, pos0); P.tok_hi = std::max(P.tok_hi, pos0 + m); }
  std::memcpy(P.tok_pinned + pos0, tokens, (size_t)m * 4);
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(P.tokens, P.tok_pinned + pos0, (size_t)m * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipEventRecord(P.tok_copied, st));
  return pf_k(c, embed_batch_launch(c->embd_type, c->embd_raw, P.tokens, P.hidden, d.hidden_size, m, st), "embedding");
}

// m <= 128 prompt tokens at positions t.pos0 .. t.pos0+m-1 of the target sequence: fills every owned layer's K/V rows of that
// sequence; the caller moves the sequence's position.  The first stage starts from the tokens' embedding rows, any other stage
// from the block of hidden vectors its predecessor left in pf.hidden; a stage that is not the last leaves its output block there
// (the last one stops after its final layer's K/V rows: nothing else of a prefill survives).
int prefill_block(lgh_ctx* c, const PfTarget& t, const uint32_t* tokens, uint32_t m) {
  int rc = pf_ensure(c);
  if (rc) return rc;
  PfScratch& P = c->pf;
  const lgh_model_desc& d = c->d;
  const uint32_t pos0 = (uint32_t)t.pos0;
  if (c->first && (rc = pf_embed_tokens(c, pos0, tokens, m))) return rc;
  if ((rc = pf_block_input(c, c->layers[c->l0].attn_norm, m))) return rc;
  const bool tq = c->kvl.tq(), kv8 = pf_kv8(c);
  if (tq && t.slot >= 0) return fail(c, LGH_UNSUPPORTED, "TurboQuant slots have no batched prompt path");
  for (uint32_t li = c->l0; li < c->l1; li++) {
    LayerW& L = c->layers[li];
    // (a TurboQuant cache: the scratch stands in for the layer's f32 cache; pf_eligible admits the context's own sequence only)
    const KvCache kv = kv_of(c, li, t.slot);
    // (a byte cache: the scratch of the block's rows, its row 0 standing for position pos0; the attention reads the stored bytes only)
    const size_t kv8_off = (size_t)pos0 * d.head_dim;
    float* const kcache = tq ? P.tq_kv : kv8 ? P.kv8_rows - kv8_off : kv.k_f32();
    float* const vcache = tq ? P.tq_kv + c->kvl.stride_floats() : kv8 ? P.kv8_rows + (size_t)d.num_kv_heads * kPfTokens * d.head_dim - kv8_off : kv.v_f32();
    const bool attend = !(li + 1 == c->l1 && c->last);   // the model's last layer: its K/V rows are written, its output would be discarded
    if ((rc = pf_qkv_step(c, L, kcache, vcache, pos0, m, kv8 ? (uint32_t)kPfTokens : 0))) return rc;
    if (tq && (rc = pf_tq_rows(c, L, li, pos0, m, attend))) return rc;
    if (kv8 && (rc = pf_kv8_store(c, kv, pos0, m))) return rc;
    if (!attend) break;
    if ((rc = pf_attn_step(c, li, kv, pos0, m))) return rc;
    if ((rc = pf_wo_step(c, L, m))) return rc;
    const float* next_nw = li + 1 < c->l1 ? c->layers[li + 1].attn_norm : nullptr;   // nullptr: the block goes to the next stage as f32
    if ((rc = L.moe() ? pf_moe_step(c, L, next_nw, m) : pf_ffn_step(c, L, next_nw, m))) return rc;
  }
  c->stats.tokens_processed += m;
  return LGH_OK;
}

// a prompt of the context's own sequence, block by block: its caches, its position, and the device's word of the next position
int prefill_own(lgh_ctx* c, const uint32_t* tokens, size_t n) {
  for (size_t i = 0; i < n; i += kPfTokens) {
    const uint32_t m = (uint32_t)std::min<size_t>(kPfTokens, n - i);
    if (int rc = prefill_block(c, PfTarget{c->pos, -1}, tokens ? tokens + i : nullptr, m)) return rc;
    c->pos += m;
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetD32Async((hipDeviceptr_t)(c->state + ST_NEXT), (int)c->pos, 1, c->stream));
  }
  return LGH_OK;
}
