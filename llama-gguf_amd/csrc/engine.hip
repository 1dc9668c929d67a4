// engine.hip — GPU-resident decode engine: the C ABI and the context's lifecycle (weight store, KV cache, hipGraph replay of the
// per-token launch sequence; the sequence itself is engine_layer.hip, its building blocks engine_launch.hip, the batched prompt
// pass engine_prefill.hip).  Mirrors what the reference's GpuOnlyInference does around its kernels
// (src/backend/cuda/gpu_only.rs:426-1024) with an MI355X-first structure:
//
//   reference (per token)                                   here
//   ------------------------------------------------------- ---------------------------------------------
//   H2D embedding row from a host f32 table (849-858)        row dequantized on device from the quantized table
//   ~20 driver calls per layer, no graph (860-1024)          5-6 launches per layer, one hipGraph replay per token
//   norm, QKV x3, dtod, rope, kv write (865-875,1056-1281)   ONE launch: RMSNorm prologue + QKV + RoPE + cache write
//   add + dtod after wo / down (969-978, 1012-1021)          residual add is the mat-vec epilogue, in place
//   gate, up, silu(+alloc+dtod), mul (1605-1651)             ONE launch with a SwiGLU epilogue
//   MoE: D2H router logits, host top-k, 3 expert matrices    router + top-k on device; experts resident in HBM and
//   re-uploaded per expert per layer per token (1765-2011)   selected by a device-side index
//   D2H full logits every token (764-767)                    kept for lgh_forward; lgh_decode_greedy feeds the
//                                                            arg-max back on device
//   reset() zero-fills every cache over PCIe (808-843)       O(1): position rewind
#include "engine.h"
#include "prefill.h"
#include "xq.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace lgh;

// Contexts up to this many rows run the single-launch decode attention (attention.hip: attn_head_kernel, one workgroup per
// query head) unless the flags say otherwise: the largest multiple of 64 rows at which it beats split + combine by more than
// the run-to-run spread.  Measured on Llama-3-8B Q4_K_M (profiles/r06_attn_head.md): 743 vs 694 tokens/s at kv 65..128,
// 730 vs 693 at 129..192, 718 vs 692 at 193..256, 685 vs 685 at 257..320, 668 vs 683 at 321..384.  (The kernel it replaced
// here, one workgroup per KV head with an online softmax per row, lost from 128 rows on: it was bound by vector issue, about
// 16 vector instructions per row and head and merges full of exponentials, not by one CU's memory path as this comment said.)
constexpr uint32_t kDirectAttnDefaultKv = 256;

// One token through the context's kernels, launched eagerly, before any of them is first launched inside a stream
// capture.  Measured on ROCm 7.0 / MI355X: a kernel whose FIRST launch in the process happens during a capture is not
// replayed with the graph — a pipeline stage behind the first (advance + stand-alone XQ kernels, which only such stages
// use) then decoded from a stale position in a fresh process and correctly in every later context of the same process
// (tools/diag_stage_first_capture.py).  Token 0 at position 0 with whatever is in the buffers: it writes K/V
// row 0 of every layer, which the sequence's real first token overwrites before anything reads it.
static int warm_kernels(lgh_ctx* c) {
  if (c->d.flags & LGH_FLAG_NO_GRAPH) return LGH_OK;
  int rc = LGH_OK;
  const AttnVariant keep_direct = c->attn_direct;
  for (int v = 0; v < 2 && !rc; v++) {
    if (v == 1 && c->direct_attn_max_kv == 0) continue;
    c->attn_direct = v == 1 ? ATTN_VAR_HEAD : ATTN_VAR_SPLIT;
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetAsync(c->state, 0, ST_WORDS * 4, c->stream));
    for (int mode : {c->last ? MODE_GREEDY : MODE_PREFILL, MODE_PREFILL})   // the last stage: with and without the output head
      if (!rc) rc = enqueue_token(c, mode);
  }
  c->attn_direct = keep_direct;
  for (auto& q : c->xqs) q.fresh = false;
  if (rc) return rc;
  if (c->samp.ctl && (rc = samp_warm(c, c->samp, c->logits, 1))) return rc;   // the sampling kernels of MODE_SAMPLE
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetAsync(c->state, 0, ST_WORDS * 4, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

static int ensure_graph(lgh_ctx* c, int mode) {
  const int var = c->attn_direct ? 1 : 0;
  if (c->graph[mode][var]) return LGH_OK;
  size_t n_nodes = 0;
  const int rc = capture_graph(c, &c->graph[mode][var], [&] { return enqueue_token(c, mode); }, &n_nodes);
  if (n_nodes && (mode == MODE_GREEDY || (c->graph_nodes == 0 && mode != MODE_SAMPLE))) c->graph_nodes = n_nodes;
  return rc;
}

// run one token in `mode` (token id already in the device state)
static int step(lgh_ctx* c, int mode) {
  if (c->pos >= c->d.max_seq_len)  // the reference has no such check: OOB write past the KV capacity
    return fail(c, LGH_INVALID_ARGUMENT, "position " + std::to_string(c->pos) + " >= max_seq_len " + std::to_string(c->d.max_seq_len));
  int rc;
  c->attn_direct = c->pos + 1 <= c->direct_attn_max_kv ? ATTN_VAR_HEAD : ATTN_VAR_SPLIT;   // the token at position pos attends to pos + 1 rows
  if (c->profiling || (c->d.flags & LGH_FLAG_NO_GRAPH)) {
    if ((rc = enqueue_token(c, mode))) return rc;
    if (c->profiling && (rc = drain_prof(c))) return rc;
  } else {
    if ((rc = ensure_graph(c, mode))) return rc;
    HIP_TRY(c, LGH_OPERATION_FAILED, hipGraphLaunch(c->graph[mode][c->attn_direct ? 1 : 0], c->stream));
  }
  c->pos += 1;
  c->stats.tokens_processed += 1;
  return LGH_OK;
}

static void drop_graphs(lgh_ctx* c) {
  for (int m = 0; m < MODE_COUNT; m++)
    for (int v = 0; v < 2; v++)
      if (c->graph[m][v]) { (void)hipGraphExecDestroy(c->graph[m][v]); c->graph[m][v] = nullptr; }
  for (auto& gg : c->batch.graph)
    for (auto& ge : gg)
      if (ge) { (void)hipGraphExecDestroy(ge); ge = nullptr; }
}

static int bind(const lgh_ctx* c) { return hipSetDevice(c->device) == hipSuccess ? LGH_OK : LGH_NOT_AVAILABLE; }

int check_ready(lgh_ctx* c) {
  if (!c) return LGH_INVALID_ARGUMENT;
  if (!c->finalized) return fail(c, LGH_INVALID_ARGUMENT, "context not finalized");
  if (bind(c)) return fail(c, LGH_NOT_AVAILABLE, "hipSetDevice failed");
  return LGH_OK;
}

// n_steps tokens in `mode` (GREEDY / SAMPLE), each fed back on the device: argmax_stage2 / samp_merge write the token into state[TOKEN]
// and into tok_log[position]
static int decode_steps(lgh_ctx* c, int mode, size_t n_steps, uint32_t* tokens_out) {
  const size_t pos0 = c->pos;
  for (size_t i = 0; i < n_steps; i++)
    if (int rc = step(c, mode)) return rc;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(tokens_out, c->tok_log + pos0, n_steps * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

static int set_token(lgh_ctx* c, uint32_t token) {
  if (c->first && token >= c->d.vocab_size) return fail(c, LGH_INVALID_ARGUMENT, "token id exceeds vocab size");  // llama.rs:296-302
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetD32Async((hipDeviceptr_t)(c->state + ST_TOKEN), (int)token, 1, c->stream));
  return LGH_OK;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// What the engine's kernels are built for, checked BEFORE anything is allocated or uploaded (a Qwen2-7B, 28 / 4 = 7 query
// heads per kv head, used to fail only in lgh_finalize's warm-up with a generic launch error).
// The cache format a descriptor asks for (type F32 with LGH_FLAG_KV_INT8 is the older spelling of int8; nothing else reads the flag)
static uint32_t desc_kv_type(const lgh_model_desc& d) {
  return d.kv_cache_type == LGH_KV_F32 && (d.flags & LGH_FLAG_KV_INT8) ? (uint32_t)LGH_KV_INT8 : d.kv_cache_type;
}

// A caller's descriptor as lgh_create reads it (one from before kv_cache_type was appended is still taken), the cache type resolved
static int desc_normalize(const lgh_model_desc* desc, lgh_model_desc& d) {
  if (!desc || (desc->struct_size != sizeof(lgh_model_desc) && desc->struct_size != offsetof(lgh_model_desc, kv_cache_type))) return LGH_INVALID_ARGUMENT;
  d = lgh_model_desc{};
  std::memcpy(&d, desc, desc->struct_size);
  d.struct_size = sizeof(lgh_model_desc);
  if (d.kv_cache_type > LGH_KV_TQ3_QJL) return LGH_INVALID_ARGUMENT;
  d.kv_cache_type = desc_kv_type(d);
  return LGH_OK;
}

int engine_shape_check(const lgh_model_desc& d, std::string& why) {
  const KvLayout kvl(desc_kv_type(d), d.num_kv_heads, d.max_seq_len, d.head_dim);
  if (!d.hidden_size || !d.num_layers || !d.num_heads || !d.num_kv_heads || !d.head_dim || !d.vocab_size || !d.max_seq_len) {
    why = "a model dimension is zero";
    return LGH_INVALID_ARGUMENT;
  }
  if (d.num_heads % d.num_kv_heads || d.head_dim % 2 || d.hidden_size % 32) {
    why = "num_heads must be a multiple of num_kv_heads, head_dim even, hidden_size a multiple of 32";
    return LGH_INVALID_ARGUMENT;
  }
  const uint32_t g = d.num_heads / d.num_kv_heads;
  // head_dim 64 / 128 with 1, 2, 4, 8 query heads per kv head take the split attention kernels; every other shape takes the
  // one-workgroup-per-head kernel (attention.hip: attn_decode_any_kernel), whose scores live in LDS
  if (!attn_shape_has_fast_kernel(d.head_dim, g) && (size_t)d.max_seq_len * 4 > 150 * 1024) {
    why = "head_dim " + std::to_string(d.head_dim) + " with " + std::to_string(g) + " query heads per kv head runs the generic attention "
          "kernel, which holds max_seq_len scores in LDS: max_seq_len must be <= 38400 for it (got " + std::to_string(d.max_seq_len) + ")";
    return LGH_UNSUPPORTED;
  }
  if (kvl.staged() && !attn_shape_has_fast_kernel(d.head_dim, g)) {
    why = "the int8 KV cache runs on the split attention kernels (head_dim 64 / 128; 1, 2, 4 or 8 query heads per kv head) of the default decode path";
    return LGH_UNSUPPORTED;
  }
  if (kvl.tq() && (d.head_dim != 64 && d.head_dim != 128)) {
    why = "the TurboQuant KV cache rotates rows of 64 or 128 values (head_dim a power of two)";
    return LGH_UNSUPPORTED;
  }
  if (d.num_experts && (d.num_experts_per_token == 0 || d.num_experts_per_token > 8 || d.num_experts_per_token > d.num_experts || d.num_experts > 64)) {
    why = "MoE layers route top-1 .. top-8 over at most 64 experts; this model routes top-" +
          std::to_string(d.num_experts_per_token) + " over " + std::to_string(d.num_experts);
    return LGH_UNSUPPORTED;
  }
  return LGH_OK;
}

extern "C" {

int lgh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int lgh_create(const lgh_model_desc* desc, lgh_ctx** out) {
  if (!out) return LGH_INVALID_ARGUMENT;
  lgh_model_desc d;
  if (int rc = desc_normalize(desc, d)) return rc;
  *out = nullptr;
  if (d.flags & LGH_FLAG_REMOVED_MASK) return LGH_UNSUPPORTED;   // the decode structures removed in round 3 (llama_gguf_hip.h)
  std::string why;
  if (int rc = engine_shape_check(d, why)) return rc;
  int ndev = lgh_device_count();
  if (ndev <= 0 || d.device_id < 0 || d.device_id >= ndev) return LGH_NOT_AVAILABLE;
  lgh_ctx* c = new lgh_ctx();
  c->d = d;
  c->kvl = KvLayout(d);
  c->device = d.device_id;
  c->l0 = d.layer_begin;
  c->l1 = d.layer_end == 0 ? d.num_layers : d.layer_end;
  if (c->l0 >= c->l1 || c->l1 > d.num_layers) { delete c; return LGH_INVALID_ARGUMENT; }
  c->first = c->l0 == 0;
  c->last = c->l1 == d.num_layers;
  c->layers.resize(d.num_layers);
  for (uint32_t i = c->l0; i < c->l1; i++) c->layers[i].owned = true;
  if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return LGH_INITIALIZATION_FAILED;
  }
  c->stream = c->own_stream;
  uint32_t splits = (d.flags >> LGH_FLAG_ATTN_SPLITS_SHIFT) & 0xFFu;
  if (!splits) {  // one attention workgroup per CU (measured: 605 vs 596 tokens/s at kv 272 and 470 vs 383 at kv 4000 against 128 workgroups)
    splits = 256 / d.num_kv_heads;
    if (splits < 1) splits = 1;
    if (splits > 32) splits = 32;
  }
  if (splits > 32) splits = 32;   // the split merge keeps one partial per split in registers
  c->n_splits = splits;
  const uint32_t dsel = (d.flags >> LGH_FLAG_ATTN_DIRECT_SHIFT) & 0xFFu;
  c->direct_attn_max_kv = dsel == 255 ? 0 : dsel ? dsel * 64 : kDirectAttnDefaultKv;
  c->attn_generic = !attn_shape_has_fast_kernel(d.head_dim, d.num_heads / d.num_kv_heads);
  if (c->kvl.staged()) c->direct_attn_max_kv = 0;   // the staged formats have one attention structure: splits + combine
  *out = c;
  return LGH_OK;
}

int lgh_kv_cache_layout(const lgh_model_desc* desc, lgh_kv_layout* out) {
  lgh_model_desc d;
  if (int rc = desc_normalize(desc, d)) return rc;
  if (!out) return LGH_INVALID_ARGUMENT;
  const KvLayout l(d);
  *out = lgh_kv_layout{l.type, (uint32_t)l.row_bytes(), (uint32_t)l.scale_bytes(), (uint32_t)l.qjl_bytes(), l.rows(),
                       l.slot_bytes(KV_K), l.slot_bytes(KV_V), l.slot_bytes(KV_KSCALE), l.slot_bytes(KV_VSCALE), l.slot_bytes(KV_KX),
                       l.slot_bytes()};
  return LGH_OK;
}

// The sign vectors of the TurboQuant rotations (HadamardRotation::signs(), src/model/turboquant/rotation.rs:126-129), before
// lgh_finalize: [owned layer][kv head][k engine, v engine][head_dim] values of +1 / -1 — what the reference draws per engine from
// its seeds (kv_turboquant.rs:44-71: base = layer * kv_heads + head; rotation seeds 4 base and 4 base + 2).
int lgh_set_kv_rotation_signs(lgh_ctx* c, const float* signs, size_t n) {
  if (!c) return LGH_INVALID_ARGUMENT;
  if (c->finalized) return fail(c, LGH_INVALID_ARGUMENT, "the rotation signs must be given before lgh_finalize");
  if (!c->kvl.tq()) return fail(c, LGH_INVALID_ARGUMENT, "this context has no TurboQuant KV cache");
  const size_t want = (size_t)(c->l1 - c->l0) * c->d.num_kv_heads * 2 * c->d.head_dim;
  if (!signs || n != want) return fail(c, LGH_INVALID_ARGUMENT, "expected " + std::to_string(want) + " sign values");
  for (size_t i = 0; i < n; i++)
    if (signs[i] != 1.0f && signs[i] != -1.0f) return fail(c, LGH_INVALID_ARGUMENT, "sign values must be +1 or -1");
  c->tq_signs_host.assign(signs, signs + n);
  return LGH_OK;
}

// The QJL projection matrices of the K engines (TurboQuantProd; QjlProjector, src/model/turboquant/qjl.rs:21-62), before lgh_finalize:
// [owned layer][kv head][head_dim][head_dim] in the order the reference draws them (row i, then column j).
int lgh_set_kv_qjl_matrices(lgh_ctx* c, const float* m, size_t n) {
  if (!c) return LGH_INVALID_ARGUMENT;
  if (c->finalized) return fail(c, LGH_INVALID_ARGUMENT, "the QJL matrices must be given before lgh_finalize");
  if (!c->kvl.qjl()) return fail(c, LGH_INVALID_ARGUMENT, "this context has no TurboQuantProd (QJL) KV cache");
  const size_t want = (size_t)(c->l1 - c->l0) * c->d.num_kv_heads * c->d.head_dim * c->d.head_dim;
  if (!m || n != want) return fail(c, LGH_INVALID_ARGUMENT, "expected " + std::to_string(want) + " matrix elements");
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(m[i])) return fail(c, LGH_INVALID_ARGUMENT, "QJL matrix elements must be finite");
  c->tq_qjl_host.assign(m, m + n);
  return LGH_OK;
}

static bool parse_layer_name(const char* name, uint32_t* layer, std::string* sub) {
  if (std::strncmp(name, "blk.", 4) != 0) return false;
  char* end = nullptr;
  unsigned long l = std::strtoul(name + 4, &end, 10);
  if (end == name + 4 || *end != '.') return false;
  *layer = (uint32_t)l;
  *sub = end + 1;
  return true;
}

int lgh_upload_tensor(lgh_ctx* c, const char* name, uint32_t type, const uint64_t ne[4], const void* host, size_t nbytes) {
  if (!c || !name || !ne || !host) return LGH_INVALID_ARGUMENT;
  if (bind(c)) return fail(c, LGH_NOT_AVAILABLE, "hipSetDevice failed");
  if (c->finalized) return fail(c, LGH_INVALID_ARGUMENT, "upload after finalize");
  const lgh_model_desc& d = c->d;
  const std::string nm(name);
  const uint64_t n0 = ne[0], n1 = ne[1] ? ne[1] : 1, n2 = ne[2] ? ne[2] : 1;
  if (nm == "token_embd.weight") {
    if (n0 != d.hidden_size || n1 != d.vocab_size) return fail(c, LGH_SHAPE_MISMATCH, "token_embd.weight shape");
    const uint32_t be = blk_elems((int)type);
    if (!be || n0 % be || nbytes != n0 / be * blk_bytes((int)type) * n1) return fail(c, LGH_SHAPE_MISMATCH, "token_embd.weight bytes");
    if (c->first) {
      int rc = dev_alloc(c, (void**)&c->embd_raw, nbytes);
      if (rc) return rc;
      HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy(c->embd_raw, host, nbytes, hipMemcpyHostToDevice));
      c->stats.weight_bytes += nbytes;
    }
    c->embd_type = (int)type;
    c->embd_bytes = nbytes;
    if (c->last && !c->output.present()) c->embd_host.assign((const uint8_t*)host, (const uint8_t*)host + nbytes);  // tied output?
    return LGH_OK;
  }
  if (nm == "output_norm.weight") {
    if (!c->last) return LGH_OK;
    if (n0 != d.hidden_size) return fail(c, LGH_SHAPE_MISMATCH, "output_norm.weight shape");
    return upload_f32(c, &c->output_norm, (int)type, n0, host, nbytes);
  }
  if (nm == "output.weight") {
    if (!c->last) return LGH_OK;
    if (n0 != d.hidden_size || n1 != d.vocab_size) return fail(c, LGH_SHAPE_MISMATCH, "output.weight shape");
    c->embd_host.clear();
    c->embd_host.shrink_to_fit();
    return upload_matrix(c, c->output, (int)type, (uint32_t)n0, (uint32_t)n1, 1, -1, host, nbytes);
  }
  uint32_t li = 0;
  std::string sub;
  if (!parse_layer_name(name, &li, &sub)) return fail(c, LGH_INVALID_ARGUMENT, "unknown tensor name " + nm);
  if (li >= d.num_layers) return fail(c, LGH_INVALID_ARGUMENT, "layer index out of range: " + nm);
  LayerW& L = c->layers[li];
  if (!L.owned) return LGH_OK;  // another pipeline stage owns it
  const uint32_t H = d.hidden_size, QD = d.num_heads * d.head_dim, KD = d.num_kv_heads * d.head_dim;
  auto mat = [&](DevWeight& W, uint64_t k, uint64_t n) -> int {
    if (n0 != k || n1 != n) return fail(c, LGH_SHAPE_MISMATCH, nm + ": expected [" + std::to_string(k) + "," + std::to_string(n) + "]");
    return upload_matrix(c, W, (int)type, (uint32_t)k, (uint32_t)n, 1, -1, host, nbytes);
  };
  auto vec = [&](float** dst, uint64_t n) -> int {
    if (n0 * n1 != n) return fail(c, LGH_SHAPE_MISMATCH, nm + ": expected " + std::to_string(n) + " elements");
    return upload_f32(c, dst, (int)type, n, host, nbytes);
  };
  const uint32_t EI = d.expert_intermediate_size ? d.expert_intermediate_size : d.intermediate_size;
  if (sub == "attn_norm.weight") return vec(&L.attn_norm, H);
  if (sub == "ffn_norm.weight") return vec(&L.ffn_norm, H);
  if (sub == "attn_q.weight") return mat(L.wq, H, QD);
  if (sub == "attn_k.weight") return mat(L.wk, H, KD);
  if (sub == "attn_v.weight") return mat(L.wv, H, KD);
  if (sub == "attn_output.weight") return mat(L.wo, QD, H);
  if (sub == "attn_q.bias") return vec(&L.bq, QD);
  if (sub == "attn_k.bias") return vec(&L.bk, KD);
  if (sub == "attn_v.bias") return vec(&L.bv, KD);
  if (sub == "attn_output.bias") return vec(&L.bo, H);
  if (sub == "ffn_gate.weight") return mat(L.gate, H, d.intermediate_size);
  if (sub == "ffn_up.weight") return mat(L.up, H, d.intermediate_size);
  if (sub == "ffn_down.weight") return mat(L.down, d.intermediate_size, H);
  if (sub == "ffn_gate_inp.weight") {  // router [hidden, n_experts], must be F32 (moe.rs:132-135)
    if (type != LGH_TYPE_F32) return fail(c, LGH_DTYPE_MISMATCH, "router weight must be F32");
    return vec(&L.router, (uint64_t)H * d.num_experts);
  }
  // expert stacks: 3-D [in, out, n_expert], expert outermost (loader.rs:1256-1303)
  auto stack = [&](DevWeight& W, uint64_t k, uint64_t n) -> int {
    if (n0 != k || n1 != n || n2 != d.num_experts) return fail(c, LGH_SHAPE_MISMATCH, nm + ": bad expert stack shape");
    return upload_matrix(c, W, (int)type, (uint32_t)k, (uint32_t)n, d.num_experts, -1, host, nbytes);
  };
  if (sub == "ffn_gate_exps.weight") return stack(L.gate_exps, H, EI);
  if (sub == "ffn_up_exps.weight") return stack(L.up_exps, H, EI);
  if (sub == "ffn_down_exps.weight") return stack(L.down_exps, EI, H);
  // per-expert tensors as the loader renames them: ffn_gate.{e}.weight (loader.rs:1171-1173)
  auto one_expert = [&](const char* prefix, DevWeight& W, uint64_t k, uint64_t n) -> int {
    size_t pl = std::strlen(prefix);
    if (sub.compare(0, pl, prefix) != 0) return -1;
    char* end = nullptr;
    unsigned long e = std::strtoul(sub.c_str() + pl, &end, 10);
    if (end == sub.c_str() + pl || std::strcmp(end, ".weight") != 0) return -1;
    if (e >= d.num_experts) return fail(c, LGH_INVALID_ARGUMENT, nm + ": expert index out of range");
    if (n0 != k || n1 != n) return fail(c, LGH_SHAPE_MISMATCH, nm + ": bad expert shape");
    return upload_matrix(c, W, (int)type, (uint32_t)k, (uint32_t)n, d.num_experts, (int)e, host, nbytes);
  };
  int r;
  if ((r = one_expert("ffn_gate.", L.gate_exps, H, EI)) >= 0) return r;
  if ((r = one_expert("ffn_up.", L.up_exps, H, EI)) >= 0) return r;
  if ((r = one_expert("ffn_down.", L.down_exps, EI, H)) >= 0) return r;
  return fail(c, LGH_INVALID_ARGUMENT, "unknown tensor name " + nm);
}

int lgh_finalize(lgh_ctx* c) {
  if (!c) return LGH_INVALID_ARGUMENT;
  if (bind(c)) return fail(c, LGH_NOT_AVAILABLE, "hipSetDevice failed");
  if (c->finalized) return LGH_OK;
  const lgh_model_desc& d = c->d;
  int rc;
  if (c->first && !c->embd_raw) return fail(c, LGH_INITIALIZATION_FAILED, "missing token_embd.weight");
  if (c->last) {
    if (!c->output_norm) return fail(c, LGH_INITIALIZATION_FAILED, "missing output_norm.weight");
    if (!c->output.present()) {  // tied output projection (loader.rs:348-355)
      if (c->embd_host.empty()) return fail(c, LGH_INITIALIZATION_FAILED, "missing output.weight and token_embd.weight");
      if ((rc = upload_matrix(c, c->output, c->embd_type, d.hidden_size, d.vocab_size, 1, -1, c->embd_host.data(), c->embd_host.size()))) return rc;
    }
    c->embd_host.clear();
    c->embd_host.shrink_to_fit();
  }
  for (uint32_t i = c->l0; i < c->l1; i++) {
    LayerW& L = c->layers[i];
    const std::string p = "blk." + std::to_string(i) + ".";
    if (!L.attn_norm || !L.ffn_norm) return fail(c, LGH_INITIALIZATION_FAILED, "missing norm weights of " + p);
    if (!L.wq.present() || !L.wk.present() || !L.wv.present() || !L.wo.present()) return fail(c, LGH_INITIALIZATION_FAILED, "missing attention weights of " + p);
    if (L.moe()) {
      if (!L.gate_exps.present() || !L.up_exps.present() || !L.down_exps.present()) return fail(c, LGH_INITIALIZATION_FAILED, "missing expert stacks of " + p);
      // experts uploaded one at a time (blk.N.ffn_{gate,up,down}.E.weight): every slot of every stack must have arrived,
      // otherwise the layer would decode from whatever the allocation held
      const std::pair<const char*, const DevWeight*> stacks[3] = {{"ffn_gate", &L.gate_exps}, {"ffn_up", &L.up_exps}, {"ffn_down", &L.down_exps}};
      for (const auto& sk : stacks) {
        std::string missing;
        for (uint32_t e = 0; e < sk.second->n_stack; e++)
          if (e >= sk.second->filled.size() || !sk.second->filled[e]) missing += (missing.empty() ? "" : ", ") + std::to_string(e);
        if (!missing.empty())
          return fail(c, LGH_INITIALIZATION_FAILED, "missing expert tensors " + p + sk.first + ".{" + missing + "}.weight");
      }
    } else if (!L.gate.present() || !L.up.present() || !L.down.present()) {
      return fail(c, LGH_INITIALIZATION_FAILED, "missing FFN weights of " + p);
    }
    if ((rc = kv_alloc(c, 1, L.kv))) return rc;   // the own sequence's cache
  }
  const uint32_t EI = d.expert_intermediate_size ? d.expert_intermediate_size : d.intermediate_size;
  const size_t ffn = std::max<size_t>(d.intermediate_size, EI);
  const size_t G = d.num_heads / d.num_kv_heads;
  const AllocSpec bufs[] = {
      {(void**)&c->hidden, (size_t)d.hidden_size * 4},
      {(void**)&c->xnorm, (size_t)d.hidden_size * 4},
      {(void**)&c->q, (size_t)d.num_heads * d.head_dim * 4},
      {(void**)&c->kv_tmp, (size_t)2 * d.num_kv_heads * d.head_dim * 4},
      {(void**)&c->attn_out, (size_t)d.num_heads * d.head_dim * 4},
      {(void**)&c->act, ffn * 4},
      {(void**)&c->act2, ffn * 4},
      {(void**)&c->logits, (size_t)d.vocab_size * 4},
      {(void**)&c->part_ml, (size_t)d.num_kv_heads * c->n_splits * G * 2 * 4},
      {(void**)&c->part_acc, (size_t)d.num_kv_heads * c->n_splits * G * d.head_dim * 4},
      {(void**)&c->rope_cs, (size_t)d.max_seq_len * d.head_dim * 4},
      {(void**)&c->moe_w, 8 * 4},
      {(void**)&c->moe_sel, 8 * 4},
      {(void**)&c->state, ST_WORDS * 4},
      {(void**)&c->amax_v, kAmaxPartsMax * 4},
      {(void**)&c->amax_i, kAmaxPartsMax * 4},
      {(void**)&c->tok_log, (size_t)d.max_seq_len * 4},
  };
  if ((rc = alloc_zeroed(c, bufs, sizeof(bufs) / sizeof(bufs[0]), c->stats.scratch_bytes))) return rc;
  if (c->kvl.tq()) {
    // the rotations' sign vectors, [owned layer][kv head][k, v][head_dim]: given through lgh_set_kv_rotation_signs (the Rust host
    // passes every engine's HadamardRotation::signs()), otherwise a deterministic stand-in — NOT the reference's StdRng stream
    const size_t n = (size_t)(c->l1 - c->l0) * d.num_kv_heads * 2 * d.head_dim;
    if (c->tq_signs_host.empty()) {
      c->tq_signs_host.resize(n);
      for (size_t i = 0; i < n; i++) {
        const uint64_t engine = (uint64_t)c->l0 * d.num_kv_heads * 2 + i / d.head_dim;   // (layer * kv_heads + head) * 2 + {k, v}
        uint64_t z = (engine * 0x9E3779B97F4A7C15ull) ^ ((i % d.head_dim) * 0xBF58476D1CE4E5B9ull);
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
        c->tq_signs_host[i] = (z & 1) ? 1.0f : -1.0f;
      }
    }
    if (c->tq_signs_host.size() != n) return fail(c, LGH_INVALID_ARGUMENT, "the rotation sign vector has the wrong length for this context");
    if ((rc = dev_alloc(c, (void**)&c->tq_signs, n * 4))) return rc;
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy(c->tq_signs, c->tq_signs_host.data(), n * 4, hipMemcpyHostToDevice));
    if (c->kvl.qjl()) {
      // the K engines' projection matrices, [owned layer][kv head][head_dim][head_dim]: given through lgh_set_kv_qjl_matrices, otherwise
      // a deterministic stand-in (Box-Muller over a counter hash: i.i.d. N(0, 1), NOT the reference's StdRng / ziggurat stream)
      const size_t nm = (size_t)(c->l1 - c->l0) * d.num_kv_heads * d.head_dim * d.head_dim;
      if (c->tq_qjl_host.empty()) {
        c->tq_qjl_host.resize(nm);
        auto mix = [](uint64_t z) { z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31; return z; };
        const uint64_t base = (uint64_t)c->l0 * d.num_kv_heads * d.head_dim * d.head_dim;
        for (size_t i = 0; i < nm; i += 2) {
          const uint64_t a = mix((base + i) * 0x9E3779B97F4A7C15ull + 0x51ED270B7F4A7C15ull), b = mix(a + 0xD1B54A32D192ED03ull);
          const double u1 = ((double)(a >> 11) + 1.0) * (1.0 / 9007199254740993.0), u2 = (double)(b >> 11) * (1.0 / 9007199254740992.0);
          const double r = std::sqrt(-2.0 * std::log(u1)), th = 6.283185307179586 * u2;
          c->tq_qjl_host[i] = (float)(r * std::cos(th));
          if (i + 1 < nm) c->tq_qjl_host[i + 1] = (float)(r * std::sin(th));
        }
      }
      if (c->tq_qjl_host.size() != nm) return fail(c, LGH_INVALID_ARGUMENT, "the QJL matrices have the wrong size for this context");
      if ((rc = dev_alloc(c, (void**)&c->tq_qjl, nm * 4))) return rc;
      HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy(c->tq_qjl, c->tq_qjl_host.data(), nm * 4, hipMemcpyHostToDevice));
    }
  }
  if (c->first && c->last && (rc = samp_alloc(c, c->samp, 1, 1))) return rc;   // lgh_decode_sample's sampler
  // XQ images of the vectors that feed quantized mat-vecs (allocated here, never during a graph capture)
  if (!xq_get(c, c->hidden, d.hidden_size) || !xq_get(c, c->attn_out, d.num_heads * d.head_dim) || !xq_get(c, c->act, (uint32_t)ffn) ||
      !xq_get(c, c->act2, (uint32_t)ffn))
    return fail(c, LGH_ALLOCATION_FAILED, "XQ image allocation failed");
  {
    std::vector<float> cs;
    rope_table_host(d, cs);
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy(c->rope_cs, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  c->finalized = true;
  c->pos = 0;
  return warm_kernels(c);
}

void lgh_destroy(lgh_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  drop_graphs(c);
  for (auto& r : c->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  kv_prefix_release(c);
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->batch.h_ctl) (void)hipHostFree(c->batch.h_ctl);
  if (c->pf.tok_pinned) (void)hipHostFree(c->pf.tok_pinned);
  if (c->pf.tok_copied) (void)hipEventDestroy(c->pf.tok_copied);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

int lgh_forward(lgh_ctx* c, uint32_t token, float* logits_out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!logits_out) return fail(c, LGH_INVALID_ARGUMENT, "logits_out is NULL");
  if (!c->first || !c->last) return fail(c, LGH_INVALID_ARGUMENT, "lgh_forward needs a single-stage context; use lgh_stage_forward");
  if ((rc = set_token(c, token))) return rc;
  if ((rc = step(c, MODE_FORWARD))) return rc;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(logits_out, c->logits, (size_t)c->d.vocab_size * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

int lgh_prefill_token(lgh_ctx* c, uint32_t token) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!c->first || !c->last) return fail(c, LGH_INVALID_ARGUMENT, "lgh_prefill_token needs a single-stage context");
  if ((rc = set_token(c, token))) return rc;
  return step(c, MODE_PREFILL);
}

int lgh_prefill_is_batched(lgh_ctx* c) { return c && c->finalized && pf_eligible(c) ? 1 : 0; }

int lgh_set_prefill_policy(lgh_ctx* c, uint32_t policy) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (policy & ~(uint32_t)LGH_PREFILL_BATCH_BYTE_KV) return fail(c, LGH_INVALID_ARGUMENT, "unknown prefill policy bits");
  c->pf_policy = policy;   // read by pf_eligible at every prompt call; the scratch it needs is made by pf_ensure at the first one
  return LGH_OK;
}

int lgh_stage_hidden_block_buffer(lgh_ctx* c, void** p) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!p) return fail(c, LGH_INVALID_ARGUMENT, "p is NULL");
  if (!pf_eligible(c)) return fail(c, LGH_UNSUPPORTED, "this context has no batched prompt path");
  if ((rc = pf_ensure(c))) return rc;
  *p = c->pf.hidden;
  return LGH_OK;
}

int lgh_stage_prefill_batch(lgh_ctx* c, const uint32_t* tokens, size_t n) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!pf_eligible(c)) return fail(c, LGH_UNSUPPORTED, "this context has no batched prompt path");
  if (n == 0 || n > (size_t)kPfTokens) return fail(c, LGH_INVALID_ARGUMENT, "a stage block holds 1..128 tokens");
  if (c->first && !tokens) return fail(c, LGH_INVALID_ARGUMENT, "the first stage needs the token ids");
  if (c->pos + n > c->d.max_seq_len) return fail(c, LGH_INVALID_ARGUMENT, "prompt block exceeds max_seq_len");
  if (c->first)
    for (size_t i = 0; i < n; i++)
      if (tokens[i] >= c->d.vocab_size) return fail(c, LGH_INVALID_ARGUMENT, "token id exceeds vocab size");
  return prefill_own(c, tokens, n);
}

int lgh_prefill_batch(lgh_ctx* c, const uint32_t* tokens, size_t n) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (n && !tokens) return fail(c, LGH_INVALID_ARGUMENT, "tokens is NULL");
  if (n >= 2 && c->first && c->last && pf_eligible(c)) {
    if (c->pos + n > c->d.max_seq_len)
      return fail(c, LGH_INVALID_ARGUMENT, "prompt of " + std::to_string(n) + " tokens at position " + std::to_string(c->pos) + " exceeds max_seq_len");
    for (size_t i = 0; i < n; i++)
      if (tokens[i] >= c->d.vocab_size) return fail(c, LGH_INVALID_ARGUMENT, "token id exceeds vocab size");
    if ((rc = prefill_own(c, tokens, n))) return rc;
    HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
    return LGH_OK;
  }
  for (size_t i = 0; i < n; i++)
    if ((rc = lgh_prefill_token(c, tokens[i]))) return rc;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

// The prompt of one slot of the multi-sequence engine (engine_batch.hip): the batched prompt path on the slot's caches and
// position (same kernels, so the slot's K / V rows are the ones lgh_prefill_batch would write); the context's own sequence, its
// position and the device's word of it stay as they are.
int lgh_batch_prefill(lgh_ctx* c, uint32_t slot, const uint32_t* tokens, size_t n) {
  int rc = check_ready(c);
  if (rc) return rc;
  BatchScratch& Bs = c->batch;
  if (!Bs.ready || slot >= Bs.max_batch) return fail(c, LGH_INVALID_ARGUMENT, "no such slot (lgh_batch_create first)");
  if (n && !tokens) return fail(c, LGH_INVALID_ARGUMENT, "tokens is NULL");
  if (Bs.pos[slot] + n > c->d.max_seq_len) return fail(c, LGH_INVALID_ARGUMENT, "prompt exceeds max_seq_len");
  for (size_t i = 0; i < n; i++)
    if (tokens[i] >= c->d.vocab_size) return fail(c, LGH_INVALID_ARGUMENT, "token id exceeds vocab size");
  if (n == 0) return LGH_OK;
  if (!pf_eligible(c, true)) {   // no batched prompt path for this model or cache: token by token through the multi-sequence step
    for (size_t i = 0; i < n; i++)
      if ((rc = lgh_forward_multi(c, &slot, tokens + i, 1, nullptr, nullptr))) return rc;
    return LGH_OK;
  }
  for (size_t i = 0; i < n && !rc; i += kPfTokens)
    rc = prefill_block(c, PfTarget{Bs.pos[slot] + i, (int)slot}, tokens + i, (uint32_t)std::min<size_t>(kPfTokens, n - i));
  if (!rc) Bs.pos[slot] += n;
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(c, LGH_OPERATION_FAILED, "hipStreamSynchronize");
  return rc;
}

void lgh_reset(lgh_ctx* c) {
  if (!c || !c->finalized) return;
  if (bind(c)) return;
  (void)hipMemsetD32Async((hipDeviceptr_t)(c->state + ST_NEXT), 0, 1, c->stream);
  c->pos = 0;
}

size_t lgh_position(const lgh_ctx* c) { return c ? c->pos : 0; }

int lgh_kv_truncate(lgh_ctx* c, size_t new_len) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (new_len < c->pos) {   // KVCache::truncate (model/mod.rs:130-134): only ever shortens
    c->pos = new_len;
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetD32Async((hipDeviceptr_t)(c->state + ST_NEXT), (int)c->pos, 1, c->stream));
  }
  return LGH_OK;
}

int lgh_kv_shift_left(lgh_ctx* c, size_t amount) {
  int rc = check_ready(c);
  if (rc) return rc;
  const lgh_model_desc& d = c->d;
  if (amount == 0 || amount >= c->pos) {   // model/mod.rs:143-146 — a shift by 0 clears the cache too
    c->pos = 0;
  } else {
    // rows [amount, pos) of every kv head move to [0, pos - amount) (model/mod.rs:148-169).  The ranges overlap, so each
    // tensor goes through a scratch buffer: two strided device-to-device copies instead of the host's memmove.
    const size_t new_len = c->pos - amount, row = (size_t)d.head_dim * 4;
    if (!c->kv_shift_tmp && (rc = dev_alloc(c, (void**)&c->kv_shift_tmp, (size_t)d.num_kv_heads * d.max_seq_len * row))) return rc;
    // (base, bytes per position) of every tensor the format has: KVCache::shift_left, QuantizedKVCache::shift_left (kv_quantized.rs:
    // 330-372: rows and scales), TurboQuantKVCache::shift_left (kv_turboquant.rs:245-266: code rows)
    for (uint32_t li = c->l0; li < c->l1; li++)
      for (int kind = 0; kind < KV_KINDS; kind++) {
        uint8_t* const b = (uint8_t*)c->layers[li].kv.t[kind];
        const size_t rb = c->kvl.pos_bytes(kind);
        if (!rb) continue;
        HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy2DAsync(c->kv_shift_tmp, new_len * rb, b + amount * rb, (size_t)d.max_seq_len * rb, new_len * rb,
                                                          d.num_kv_heads, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy2DAsync(b, (size_t)d.max_seq_len * rb, c->kv_shift_tmp, new_len * rb, new_len * rb, d.num_kv_heads,
                                                          hipMemcpyDeviceToDevice, c->stream));
      }
    c->pos = new_len;
  }
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetD32Async((hipDeviceptr_t)(c->state + ST_NEXT), (int)c->pos, 1, c->stream));
  return LGH_OK;
}

int lgh_forward_argmax(lgh_ctx* c, uint32_t token, uint32_t* next_token) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!next_token) return fail(c, LGH_INVALID_ARGUMENT, "next_token is NULL");
  if (!c->first || !c->last) return fail(c, LGH_INVALID_ARGUMENT, "needs a single-stage context");
  if ((rc = set_token(c, token))) return rc;
  if ((rc = step(c, MODE_GREEDY))) return rc;
  int tok = 0;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(&tok, c->state + ST_ARGMAX, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  *next_token = (uint32_t)tok;
  return LGH_OK;
}

int lgh_decode_greedy(lgh_ctx* c, uint32_t first_token, size_t n_steps, uint32_t* tokens_out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (n_steps && !tokens_out) return fail(c, LGH_INVALID_ARGUMENT, "tokens_out is NULL");
  if (!c->first || !c->last) return fail(c, LGH_INVALID_ARGUMENT, "needs a single-stage context");
  if (c->pos + n_steps > c->d.max_seq_len) return fail(c, LGH_INVALID_ARGUMENT, "decode would exceed max_seq_len");
  if ((rc = set_token(c, first_token))) return rc;
  return decode_steps(c, MODE_GREEDY, n_steps, tokens_out);
}

int lgh_set_sampler_ex(lgh_ctx* c, const lgh_sampler_config_ex* cfg) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!c->samp.ctl) return fail(c, LGH_INVALID_ARGUMENT, "sampling needs a single-stage context");
  if ((rc = samp_check_ex(c, cfg))) return rc;
  if ((rc = samp_reset(c, c->samp, 0, *cfg))) return rc;
  c->samp_cfg = *cfg;
  c->samp_set = true;
  return LGH_OK;
}

int lgh_set_sampler(lgh_ctx* c, const lgh_sampler_config* cfg) {
  if (!cfg) return lgh_set_sampler_ex(c, nullptr);   // (refused there, after the context's own checks)
  const lgh_sampler_config_ex x = samp_plain(*cfg);
  return lgh_set_sampler_ex(c, &x);
}

int lgh_get_sampler_mu(lgh_ctx* c, int slot, float* mu) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!mu) return fail(c, LGH_INVALID_ARGUMENT, "mu is NULL");
  if (slot < 0) {
    if (!c->samp.ctl || !c->samp_set) return fail(c, LGH_INVALID_ARGUMENT, "lgh_set_sampler has not been called");
    return samp_mu(c, c->samp, 0, mu);
  }
  BatchScratch& Bs = c->batch;
  if (!Bs.ready || (uint32_t)slot >= Bs.max_batch || (size_t)slot >= Bs.samp_set.size() || !Bs.samp_set[slot])
    return fail(c, LGH_INVALID_ARGUMENT, "no sampler in that slot");
  return samp_mu(c, Bs.samp, (uint32_t)slot, mu);
}

int lgh_decode_sample(lgh_ctx* c, uint32_t first_token, const uint32_t* history, size_t n_history, size_t n_steps, const float* uniforms,
                      uint32_t* tokens_out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!c->samp.ctl) return fail(c, LGH_INVALID_ARGUMENT, "sampling needs a single-stage context");
  if (!c->samp_set) return fail(c, LGH_INVALID_ARGUMENT, "lgh_set_sampler has not been called");
  if (n_steps && !tokens_out) return fail(c, LGH_INVALID_ARGUMENT, "tokens_out is NULL");
  if (n_history && !history) return fail(c, LGH_INVALID_ARGUMENT, "history is NULL");
  if (n_steps && !uniforms && samp_needs_uniforms(c->samp_cfg)) return fail(c, LGH_INVALID_ARGUMENT, "uniforms is NULL");
  if (c->pos + n_steps > c->d.max_seq_len) return fail(c, LGH_INVALID_ARGUMENT, "decode would exceed max_seq_len");
  if (n_steps == 0) return LGH_OK;
  if ((rc = set_token(c, first_token))) return rc;
  if ((rc = samp_begin(c, c->samp, 0, c->samp_cfg, history, n_history, first_token, n_steps, uniforms, 1))) return rc;
  return decode_steps(c, MODE_SAMPLE, n_steps, tokens_out);
}

const char* lgh_last_error(const lgh_ctx* c) { return c ? c->err.c_str() : "null context"; }

int lgh_get_stats(lgh_ctx* c, lgh_stats* out) {
  if (!c || !out) return LGH_INVALID_ARGUMENT;
  c->stats.graph_nodes = c->graph_nodes;
  // algorithmic bytes of one decode step at the current position
  uint64_t b = 0;
  const lgh_model_desc& d = c->d;
  if (c->finalized) {
    if (c->first) b += (uint64_t)d.hidden_size * blk_bytes(c->embd_type) / blk_elems(c->embd_type);
    for (uint32_t i = c->l0; i < c->l1; i++) {
      const LayerW& L = c->layers[i];
      b += L.wq.bytes + L.wk.bytes + L.wv.bytes + L.wo.bytes;
      if (L.moe()) b += (uint64_t)d.num_experts_per_token * (L.gate_exps.bytes + L.up_exps.bytes + L.down_exps.bytes) + (uint64_t)d.num_experts * d.hidden_size * 4;
      else b += L.gate.bytes + L.up.bytes + L.down.bytes;
      b += (uint64_t)2 * d.hidden_size * 4;                                       // norm weights
      b += c->kvl.step_alg_bytes(c->pos + 1);                                     // KV read (kv_len = pos+1) + write
    }
    if (c->last) b += c->output.bytes + (uint64_t)d.hidden_size * 4 + (uint64_t)d.vocab_size * 4;
  }
  c->stats.step_alg_bytes = b;
  c->stats.overlapped_edges = 0;
  *out = c->stats;
  return LGH_OK;
}

int lgh_set_profiling(lgh_ctx* c, int on) {
  if (!c) return LGH_INVALID_ARGUMENT;
  c->profiling = on != 0;
  if (on) {
    std::memset(c->stats.k_launches, 0, sizeof(c->stats.k_launches));
    std::memset(c->stats.k_time_us, 0, sizeof(c->stats.k_time_us));
    std::memset(c->stats.k_alg_bytes, 0, sizeof(c->stats.k_alg_bytes));
    std::memset(c->stats.sym_launches, 0, sizeof(c->stats.sym_launches));
    std::memset(c->stats.sym_time_us, 0, sizeof(c->stats.sym_time_us));
    std::memset(c->stats.sym_alg_bytes, 0, sizeof(c->stats.sym_alg_bytes));
    c->stats.event_bracket_us = 0.0;
    c->stats.event_bracket_samples = 0;
  }
  return LGH_OK;
}

int lgh_set_stream(lgh_ctx* c, void* s) {
  if (!c) return LGH_INVALID_ARGUMENT;
  if (bind(c)) return LGH_NOT_AVAILABLE;
  (void)hipStreamSynchronize(c->stream);
  hipStream_t ns = s ? (hipStream_t)s : c->own_stream;
  if (ns != c->stream) drop_graphs(c);
  c->stream = ns;
  return LGH_OK;
}

int lgh_stage_set_forward_targets(lgh_ctx* c, void* hidden_dst, void* token_dst) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (hidden_dst && c->last) return fail(c, LGH_INVALID_ARGUMENT, "the last stage hands no hidden vector on");
  if (token_dst && !c->last) return fail(c, LGH_INVALID_ARGUMENT, "only the last stage produces the arg-max token");
  if (hidden_dst == c->hidden) return fail(c, LGH_INVALID_ARGUMENT, "hidden_dst is this stage's own buffer");
  (void)hipStreamSynchronize(c->stream);
  if (hidden_dst != c->fwd_hidden || token_dst != c->fwd_token) drop_graphs(c);
  c->fwd_hidden = hidden_dst;
  c->fwd_token = token_dst;
  // first launch outside any capture (see warm_kernels); what it copies is overwritten before anything reads it
  if (hidden_dst) HIP_TRY(c, LGH_OPERATION_FAILED, copy_words_launch(hidden_dst, c->hidden, c->d.hidden_size, c->stream));
  if (token_dst) HIP_TRY(c, LGH_OPERATION_FAILED, copy_words_launch(token_dst, c->state + ST_ARGMAX, 1, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

void* lgh_get_stream(lgh_ctx* c) { return c ? (void*)c->stream : nullptr; }

int lgh_synchronize(lgh_ctx* c) {
  if (!c) return LGH_INVALID_ARGUMENT;
  if (bind(c)) return LGH_NOT_AVAILABLE;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

int lgh_read_hidden(lgh_ctx* c, float* out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!out) return fail(c, LGH_INVALID_ARGUMENT, "out is NULL");
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(out, c->hidden, (size_t)c->d.hidden_size * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

int lgh_stage_hidden_buffer(lgh_ctx* c, void** p) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!p) return LGH_INVALID_ARGUMENT;
  *p = c->hidden;
  return LGH_OK;
}

int lgh_stage_forward(lgh_ctx* c, uint32_t token, int want_logits, float* logits_out, uint32_t* next_token) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->first && (rc = set_token(c, token))) return rc;
  int mode = MODE_PREFILL;
  if (c->last && want_logits) mode = next_token ? MODE_GREEDY : MODE_FORWARD;
  if ((rc = step(c, mode))) return rc;
  if (c->last && want_logits) {
    int tok = 0;
    if (logits_out) HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(logits_out, c->logits, (size_t)c->d.vocab_size * 4, hipMemcpyDeviceToHost, c->stream));
    if (next_token) HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(&tok, c->state + ST_ARGMAX, 4, hipMemcpyDeviceToHost, c->stream));
    if (logits_out || next_token) HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
    if (next_token) *next_token = (uint32_t)tok;
  }
  return LGH_OK;
}

// ---- device-side token feedback for multi-process pipelines: no host value crosses a stage boundary per token ----
int lgh_stage_io_buffers(lgh_ctx* c, void** token_in, void** argmax_out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (token_in) *token_in = c->state + ST_TOKEN;
  if (argmax_out) *argmax_out = c->state + ST_ARGMAX;
  return LGH_OK;
}

int lgh_stage_step(lgh_ctx* c, int mode) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (mode < 0 || mode > MODE_GREEDY) return fail(c, LGH_INVALID_ARGUMENT, "mode must be 0 (layers only), 1 (logits) or 2 (arg-max)");
  if (!c->last) mode = MODE_PREFILL;
  return step(c, mode);
}

int lgh_stage_read_logits(lgh_ctx* c, float* logits_out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!logits_out) return fail(c, LGH_INVALID_ARGUMENT, "logits_out is NULL");
  if (!c->last) return fail(c, LGH_INVALID_ARGUMENT, "only the last stage holds logits");
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(logits_out, c->logits, (size_t)c->d.vocab_size * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

int lgh_stage_read_tokens(lgh_ctx* c, size_t pos0, size_t n, uint32_t* out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!out && n) return fail(c, LGH_INVALID_ARGUMENT, "out is NULL");
  if (!c->last) return fail(c, LGH_INVALID_ARGUMENT, "only the last stage logs the arg-max tokens");
  if (pos0 + n > c->d.max_seq_len) return fail(c, LGH_INVALID_ARGUMENT, "token log range exceeds max_seq_len");
  if (n) HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(out, c->tok_log + pos0, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

}  // extern "C"
