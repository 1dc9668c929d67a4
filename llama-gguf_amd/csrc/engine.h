// engine.h — the GPU-resident decode engine behind the lgh_* C ABI (internal).
#pragma once

#include <functional>
#include <string>
#include <vector>

#include "common.h"
#include "kv_cache.h"
#include "sample.h"

namespace lgh {

struct LayerW {
  bool owned = false;  // layer belongs to this pipeline stage
  DevWeight wq, wk, wv, wo, gate, up, down;           // dense
  DevWeight gate_exps, up_exps, down_exps;            // MoE stacks [in, out, n_expert]
  float* attn_norm = nullptr;
  float* ffn_norm = nullptr;
  float* router = nullptr;                            // [n_experts][hidden] f32
  float* bq = nullptr; float* bk = nullptr; float* bv = nullptr; float* bo = nullptr;
  KvCache kv;   // the own sequence's cache (one slot), in the context's format (lgh_ctx::kvl)
  bool moe() const { return router != nullptr; }
};

// decode attention over the f32 cache: splits + combine, attn_partial_kernel<.., DIRECT> (one workgroup per kv head; the per-op surface only)
// or attn_head_kernel (one workgroup per query head: the engine's single launch)
enum AttnVariant : uint8_t { ATTN_VAR_SPLIT = 0, ATTN_VAR_DIRECT = 1, ATTN_VAR_HEAD = 2 };
enum TokenMode { MODE_PREFILL = 0, MODE_FORWARD = 1, MODE_GREEDY = 2, MODE_SAMPLE = 3, MODE_COUNT = 4 };   // SAMPLE: GREEDY with the sampler (sample.hip) for the arg-max

// The XQ image (xq.h) of an f32 activation buffer, for int8-MFMA consumers.  `fresh` = the image matches the buffer's
// current contents; `tag` = the RMSNorm weights it was multiplied with (nullptr: none).
struct XqBuf { const float* f32 = nullptr; uint8_t* xq = nullptr; float* ssq = nullptr; uint32_t k = 0; bool fresh = false; const float* tag = nullptr; };

// scratch of the batched prompt path (prefill.hip), allocated at the first lgh_prefill_batch that uses it
struct PfScratch {
  bool ready = false;
  uint8_t *xh_h = nullptr, *xh_attn = nullptr, *xh_act = nullptr;   // XH activations: [128][hidden], [128][QD], [128][ffn]
  float *hidden = nullptr, *q = nullptr, *part = nullptr, *ssq = nullptr;
  size_t part_bytes = 0;
  int* tokens = nullptr;
  uint32_t* tok_pinned = nullptr;      // pinned host staging of the prompt's token ids, one slot per position
  hipEvent_t tok_copied = nullptr;     // recorded behind the last copy out of it
  uint32_t tok_lo = 0, tok_hi = 0;     // slots [tok_lo, tok_hi) may still be read by a copy enqueued since the last wait for tok_copied
  // MoE layers: routing of the block's tokens, tokens grouped by expert, one expert's gathered input, per-slot expert outputs
  int *moe_sel = nullptr, *moe_cnt = nullptr, *moe_base = nullptr, *moe_list = nullptr, *moe_rowmap = nullptr, *moe_tokmap = nullptr;
  float* moe_w = nullptr;
  uint8_t *xh_gather = nullptr, *xh_act_e = nullptr;   // per expert: gathered inputs [E][xh_bytes(H)], activations [E][xh_bytes(EI)]
  // TurboQuantMSE caches: one layer's rows as f32 in the rotated space (centroids of the codes), K then V, each [kv head][max_seq][head_dim];
  // rebuilt by every layer of every block (attention_tq.hip tq_pf_rows_kernel)
  float* tq_kv = nullptr;
  // byte caches (int8 / FP8): the block's K rows after RoPE, then its V rows, f32 [kv head][128][head_dim] each — the block only; the
  // store launch (attention.hip kv8_pf_store_kernel) turns them into the target's cache rows
  float* kv8_rows = nullptr;
};

struct ProfRec { int cls; int sym; uint64_t bytes; hipEvent_t a, b; };

// multi-sequence decode (engine_batch.hip): `max_batch` slots, each one sequence's KV caches and position, and the vectors of
// up to max_batch sequences side by side ([sequence][...], sequence s of a step at s times the vector's length)
struct BatchScratch {
  bool ready = false;
  uint32_t max_batch = 0, ffn = 0;
  float *hidden = nullptr, *xnorm = nullptr, *q = nullptr, *attn_out = nullptr, *act = nullptr, *act2 = nullptr, *logits = nullptr,
        *part_ml = nullptr, *part_acc = nullptr, *amax_v = nullptr, *moe_w = nullptr, *mv_part = nullptr;
  uint64_t mv_part_floats = 0;
  int *amax_i = nullptr, *moe_sel = nullptr;
  int *d_tokens = nullptr, *d_pos = nullptr, *d_slot = nullptr, *d_log = nullptr;   // the step's control words (device), the greedy token log
  int* h_ctl = nullptr;                               // pinned staging of the control words
  std::vector<KvCache> kv;                            // per layer: the max_batch slots' caches, in the context's format (lgh_ctx::kvl)
  float* kv_tmp = nullptr;                            // staged formats: the step's K rows after RoPE | V rows, f32, [sequence][K row | V row]
  // MoE layers, experts read once per step (top-k <= 8): the (sequence, slot) pairs' activations [pair][ffn] (+ XQ views) and expert
  // outputs [pair][hidden]; per expert the number of pairs that chose it and their list
  float *moe_act = nullptr, *moe_tmp = nullptr;
  int *moe_cnt = nullptr, *moe_idx = nullptr;
  std::vector<size_t> pos;                            // per slot: tokens in its cache
  hipGraphExec_t graph[kMaxBatch + 1][3] = {};        // [n_seq][0 logits only, 1 + arg-max fed back, 2 + sampled token fed back]
  SampBufs samp;                                      // one sampler per slot (lgh_batch_set_sampler)
  std::vector<lgh_sampler_config_ex> samp_cfg;
  std::vector<uint8_t> samp_set;
};

}  // namespace lgh

struct lgh_ctx {
  lgh_model_desc d{};
  lgh::KvLayout kvl;   // d's cache format and its sizes (lgh_create; the bare contexts of ops_api.hip set it with the fields it is made of)
  int device = 0;
  uint32_t l0 = 0, l1 = 0;
  bool first = true, last = true;
  hipStream_t own_stream = nullptr, stream = nullptr;
  std::vector<lgh::LayerW> layers;
  // embedding table in native GGUF layout (row-dequantized per token) and the output projection
  uint8_t* embd_raw = nullptr;
  int embd_type = -1;
  size_t embd_bytes = 0;
  std::vector<uint8_t> embd_host;  // kept only until finalize, for a tied output projection
  lgh::DevWeight output;
  float* output_norm = nullptr;
  // scratch (device)
  void *fwd_hidden = nullptr, *fwd_token = nullptr;   // in-graph hops to a same-device stage (lgh_stage_set_forward_targets)
  float *hidden = nullptr, *xnorm = nullptr, *q = nullptr, *kv_tmp = nullptr, *attn_out = nullptr, *act = nullptr,
        *act2 = nullptr, *logits = nullptr, *part_ml = nullptr, *part_acc = nullptr, *rope_cs = nullptr, *moe_w = nullptr,
        *amax_v = nullptr;
  int *moe_sel = nullptr, *state = nullptr, *amax_i = nullptr, *tok_log = nullptr;
  uint32_t n_splits = 8;
  // host mirrors
  size_t pos = 0;
  bool finalized = false;
  bool profiling = false;
  std::string err;
  hipGraphExec_t graph[lgh::MODE_COUNT][2] = {};   // [mode][attention variant: 0 split + combine, 1 single launch (contexts up to direct_attn_max_kv rows)]
  lgh::AttnVariant attn_direct = lgh::ATTN_VAR_SPLIT;   // variant of the token being enqueued (chosen by the host-side position)
  bool attn_generic = false;                       // the shape has no split kernel: every token runs attn_decode_any_kernel (a field, not
                                                   // re-derived from the shape, so that lgh_op_attention_decode can run that kernel on any shape)
  uint32_t direct_attn_max_kv = 0;                 // contexts up to this many rows take the single-launch attention
  uint64_t graph_nodes = 0;
  // accounting
  lgh_stats stats{};
  std::vector<lgh::ProfRec> prof;
  std::vector<void*> allocs;  // everything hipMalloc'ed by this context
  std::vector<lgh::XqBuf> xqs;
  lgh::PfScratch pf;
  uint32_t pf_policy = 0;                      // LGH_PREFILL_* (lgh_set_prefill_policy)
  lgh::BatchScratch batch;
  float* tq_signs = nullptr;                   // TurboQuant KV cache: [owned layer][kv head][k, v][head_dim] rotation signs (device)
  std::vector<float> tq_signs_host;
  float* tq_qjl = nullptr;                     // TurboQuantProd: [owned layer][kv head][head_dim][head_dim] QJL projection matrices (device)
  std::vector<float> tq_qjl_host;
  float* kv_shift_tmp = nullptr;               // scratch of lgh_kv_shift_left (one cache tensor), allocated at first use
  lgh::SampBufs samp;                          // single-stage contexts: the sampler of lgh_set_sampler / lgh_decode_sample
  lgh_sampler_config_ex samp_cfg{};
  bool samp_set = false;
  // device prompt cache (kv_prefix.hip): the live prefixes this context made, and the device tables of its cache tensors ([0] the own
  // sequence's, [1] the slots'), built at first use
  std::vector<lgh_prefix*> prefixes;
  void* prefix_tab[2] = {nullptr, nullptr};
  uint32_t prefix_tab_n[2] = {0, 0};
};

// ---- what crosses the engine's files: engine_launch.hip (uploads, mat-vec launch assembly, XQ registry), engine_layer.hip (the
// per-layer decode sequence), engine_prefill.hip (the batched prompt driver), engine.hip / engine_batch.hip / sample.hip /
// ops_api.hip (the C ABI) ----
#include <cstring>

int fail(lgh_ctx* c, int status, const std::string& msg);
#define HIP_TRY(c, status, expr)                                                                      \
  do {                                                                                                \
    hipError_t e__ = (expr);                                                                          \
    if (e__ != hipSuccess)                                                                            \
      return fail((c), (status), std::string(#expr) + ": " + hipGetErrorString(e__));                 \
  } while (0)

struct LayoutInfo {
  int dev_type;
  int nplanes;
  uint32_t bpb[4];      // bytes per block, per plane
  uint32_t belems;      // elements per block
};

struct SegSpec {
  int npass = 1;
  // also leave `out` as an XQ image for the next (int8-MFMA) consumer: 0 no, 1 plain, 2 multiplied by xq_next_nw (+ sum of squares)
  int xq_next = 0;
  const float* xq_next_nw = nullptr;
  const lgh::DevWeight* W[4] = {nullptr, nullptr, nullptr, nullptr};
  const float* x[4] = {nullptr, nullptr, nullptr, nullptr};
  const int* sel[4] = {nullptr, nullptr, nullptr, nullptr};
  int epi = lgh::EPI_STORE;
  float* out = nullptr;
  float* out2 = nullptr;
  const float* resid = nullptr;
  const float* bias = nullptr;
  const float* moe_w = nullptr;
  // single-segment launches: ask the launch to leave each workgroup's arg-max part (MvLaunch::amax_v / amax_i, kAmaxPartsMax slots);
  // *amax_parts receives how many it left — 0 when it ran without a static plan and both arg-max stages are still needed
  float* amax_v = nullptr;
  int* amax_i = nullptr;
  uint32_t* amax_parts = nullptr;
};

// the vectors the FFN half of a layer works on (one sequence's)
struct FfnView { float* hidden; float* act; float* act2; float* xnorm; int* moe_sel; float* moe_w; };
// ... and the attention half: kv_tmp = the current token's K row | V row, f32 (unfused QKV, and the byte caches, whose attention launch
// quantizes and stores them; nothing else reads it, so a caller with fused f32-cache launches only may pass nullptr)
struct AttnView { float* hidden; float* q; float* kv_tmp; float* attn_out; };
struct AllocSpec { void** p; size_t n; };

int build_mv_group(lgh_ctx* c, const SegSpec* specs, int nseg, const float* norm_w, uint32_t k, bool mfma, lgh::MvLaunch& L, uint32_t& wg,
                   uint32_t& threads, uint64_t& alg, uint32_t tile_cap);
int qkv_forward(lgh_ctx* c, lgh::LayerW& Lw, const AttnView& v);   // norm -> q, k, v -> RoPE -> cache write (or kv_tmp, staged formats)
// attention over layer li's cache into v.attn_out, by the context's path (cache type, attn_generic, attn_direct, n_splits); xq_out: also
// leave attn_out's XQ image, where the path's last launch can write one.  One function behind this and attention_forward_multi
// (engine_layer.hip: attention_step): the split paths build an AttnDecode for attn_split_launch / attn_merge_launch
int attention_forward(lgh_ctx* c, lgh::LayerW& Lw, uint32_t li, const AttnView& v, float scale, bool xq_out);
// layer li's TurboQuant inputs: its rotation signs [kv head][k, v][head_dim] and, for the QJL formats (else nullptr), its projection
// matrices [kv head][head_dim][head_dim]
struct TqLayer { const float *signs, *qjl_s; };
inline TqLayer tq_layer(const lgh_ctx* c, uint32_t li) {
  const size_t kd = (size_t)(li - c->l0) * c->d.num_kv_heads * c->d.head_dim;
  return {c->tq_signs + kd * 2, c->kvl.qjl() ? c->tq_qjl + kd * c->d.head_dim : nullptr};
}
int ffn_forward(lgh_ctx* c, lgh::LayerW& Lw, const FfnView& v, const float* next_nw, bool next_mfma);
int ffn_gateup_forward(lgh_ctx* c, lgh::LayerW& Lw, const FfnView& v);   // the dense FFN up to v.act (gate | up + SwiGLU), no down projection
int embed_forward(lgh_ctx* c);   // the token's embedding row into c->hidden, the position advanced
int moe_experts_forward(lgh_ctx* c, lgh::LayerW& Lw, const FfnView& v, const float* next_nw, bool next_mfma);   // given v.moe_sel / v.moe_w
void rope_table_host(const lgh_model_desc& d, std::vector<float>& cs);
int engine_shape_check(const lgh_model_desc& d, std::string& why);   // LGH_OK, or the status lgh_create returns and why
int dev_alloc(lgh_ctx* c, void** p, size_t bytes);
// every buffer of the table with a size, in order: allocated, zeroed on the context's stream, added to `counter`
int alloc_zeroed(lgh_ctx* c, const AllocSpec* bufs, size_t count, uint64_t& counter);
LayoutInfo layout_for(int src_type);
bool fused_type(int t);
int upload_matrix(lgh_ctx* c, lgh::DevWeight& W, int src_type, uint32_t k, uint32_t n, uint32_t n_stack, int slot,
                  const void* host, size_t nbytes);
int upload_f32(lgh_ctx* c, float** dst, int src_type, uint64_t n, const void* host, size_t nbytes);
int launch_mv(lgh_ctx* c, int cls, const SegSpec* specs, int nseg, const float* norm_w, uint32_t k);
// ---- multi-sequence decode (engine_batch.hip).  One batched quantized mat-vec launch over the context's batch scratch: `specs` name
// sequence 0's vectors, sequence s follows at the strides (floats; xq_out_k: the k its output's views were registered with, 0 = no image).
// ind: the launch works on indirect (sequence, top-k slot) entries, one list per expert (MvBatch::ind_*)
struct MvIndirect { const int* cnt = nullptr; const int* idx = nullptr; uint32_t div = 0, nz = 0, stride = 0; };
int launch_mvb(lgh_ctx* c, int cls, const SegSpec* specs, int nseg, const float* norm_w, uint32_t k, uint32_t n_seq, const uint32_t* out_stride,
               const uint32_t* resid_stride, const uint32_t* xq_out_k, const MvIndirect ind = MvIndirect{});
bool mvb_k_ok(uint32_t k);                           // a [.., k] matrix plans to the 8-wave workgroups the multi-sequence kernels run
uint32_t xq_stride_of(uint32_t k);                   // bytes / floats between two sequences' images and sum-of-squares partials
uint32_t ssq_stride_of(uint32_t k);
int register_views(lgh_ctx* c, float* f32, uint8_t* xq, float* ssq, uint32_t k, uint32_t n);   // n sequences' views of a batch vector, at those strides
uint64_t batch_part_floats(const lgh_ctx* c, uint32_t max_batch);
// one layer's cache for n_slots sequences in the context's format: allocated, zeroed, counted as KV bytes
int kv_alloc(lgh_ctx* c, size_t n_slots, lgh::KvCache& kv);
// layer li's cache of slot `slot` of the multi-sequence engine (slot < 0: the context's own)
inline lgh::KvCache kv_of(const lgh_ctx* c, uint32_t li, int slot) {
  return slot < 0 ? c->layers[li].kv : c->batch.kv[li].slot(c->kvl, (size_t)slot);
}
int batch_scratch_alloc(lgh_ctx* c, uint32_t max_batch);
// the step of a layer over the batch scratch (c->batch), one function each, shared by enqueue_multi and the per-launch entry points
int qkv_forward_multi(lgh_ctx* c, lgh::LayerW& Lw, uint32_t li, uint32_t n_seq);
int attention_forward_multi(lgh_ctx* c, uint32_t li, uint32_t n_seq, float scale, bool xq_out);   // Bs.q -> Bs.attn_out (+ its images); engine_layer.hip
// a launch left the images of n vectors of k floats from `base` on, multiplied with the norm weights `tag` (nullptr: none)
void mark_fresh(lgh_ctx* c, const float* base, uint32_t k, uint32_t n, const float* tag);
int linear_multi(lgh_ctx* c, int cls, const lgh::DevWeight& W, const lgh::DevWeight* W_up, const float* x, float* out, uint32_t out_stride,
                 uint32_t n_seq, const float* norm_w, const float* resid = nullptr, const float* bias = nullptr, int xq_next = 0,
                 const float* xq_next_nw = nullptr, const MvIndirect ind = MvIndirect{});
int ffn_forward_multi(lgh_ctx* c, lgh::LayerW& Lw, uint32_t n_seq, const float* next_nw);
int moe_grouped_forward(lgh_ctx* c, lgh::LayerW& Lw, uint32_t n_seq, const float* next_nw, bool route);
// What every entry point asks of a step's sequences: n_seq in 1 .. max_n; every slot number in [0, n_slots) and, with `distinct`, listed
// once; every position — pos(i), sequence i's; an empty function: not checked — in [0, max_seq).  The first condition that fails, and
// in *at which sequence it failed for
enum SeqFault { SEQ_OK = 0, SEQ_COUNT, SEQ_SLOT, SEQ_POS };
template <class T>
inline SeqFault check_seqs(size_t n_seq, size_t max_n, const T* slot, size_t n_slots, bool distinct, const std::function<uint64_t(size_t)>& pos,
                           size_t max_seq, size_t* at = nullptr) {
  if (n_seq == 0 || n_seq > max_n) return SEQ_COUNT;
  for (size_t i = 0; i < n_seq; i++) {
    if (at) *at = i;
    if ((uint64_t)(int64_t)slot[i] >= n_slots) return SEQ_SLOT;   // (a negative number: far above)
    for (size_t j = 0; distinct && j < i; j++)
      if (slot[j] == slot[i]) return SEQ_SLOT;
    if (pos && pos(i) >= max_seq) return SEQ_POS;
  }
  return SEQ_OK;
}
// matrix-core segments in formats without a common instantiation (Q4_K with Q5_K, Q8_0 / Q4_0 with anything else): one launch each
bool mv_formats_split(const SegSpec* specs, int nseg);
lgh::XqBuf* xq_get(lgh_ctx* c, const float* f32, uint32_t k);   // finds or registers (allocating) the image of a buffer
lgh::XqBuf* xq_find(lgh_ctx* c, const float* f32);              // the image registered under exactly this address, or nullptr
void xq_stale(lgh_ctx* c, const float* f32);
int linear_any(lgh_ctx* c, int cls, const lgh::DevWeight& W, const float* x, float* out, const float* norm_w,
               const float* resid, const float* bias, int xq_next = 0, const float* xq_next_nw = nullptr, float* amax_v = nullptr,
               int* amax_i = nullptr, uint32_t* amax_parts = nullptr);   // amax_*: as SegSpec's
int drain_prof(lgh_ctx* c);
int check_ready(lgh_ctx* c);   // what every entry point on a finalized context starts with: LGH_OK and the device bound, or the status
// captures what `enqueue` puts on the context's stream and instantiates it into *exec; n_nodes: the graph's node count
int capture_graph(lgh_ctx* c, hipGraphExec_t* exec, const std::function<int()>& enqueue, size_t* n_nodes = nullptr);
int enqueue_token(lgh_ctx* c, int mode);   // everything one token needs, in stream order (eager or under capture)
// batched prompt path (engine_prefill.hip).  The sequence a block of prompt tokens belongs to: the position of the block's first token,
// and whose K / V rows it fills — the context's own (slot < 0) or a slot's of the multi-sequence engine (kv_of)
struct PfTarget { size_t pos0; int slot; };
// slot: the target is a slot of the multi-sequence engine (TurboQuant slots stay token by token: bit-identical to the single-sequence engine).
// The byte caches (int8 / FP8) have the path for the own sequence, slots and stage contexts alike, on contexts that asked for it
// (lgh_set_prefill_policy: lgh_ctx::pf_policy)
bool pf_eligible(const lgh_ctx* c, bool slot = false);
int pf_ensure(lgh_ctx* c);
int prefill_block(lgh_ctx* c, const PfTarget& t, const uint32_t* tokens, uint32_t m);
// prefill_block's steps over the m tokens in the context's scratch (c->pf, after pf_ensure); next_nw: the norm weight of the step's
// consumer, nullptr = leave no XH
int pf_embed_tokens(lgh_ctx* c, uint32_t pos0, const uint32_t* tokens, uint32_t m);   // ids through the pinned ring, embedding rows into pf.hidden
int pf_block_input(lgh_ctx* c, const float* nw, uint32_t m);
// cache_rows: rows per kv head of kcache / vcache whose row 0 is position 0 (0: max_seq_len, a whole cache).  The byte caches' block scratch
// has 128 rows per head and row 0 = position pos0: the caller passes 128 and bases shifted back by pos0 rows
int pf_qkv_step(lgh_ctx* c, lgh::LayerW& L, float* kcache, float* vcache, uint32_t pos0, uint32_t m, uint32_t cache_rows = 0);
int pf_attn_step(lgh_ctx* c, uint32_t li, const lgh::KvCache& kv, uint32_t pos0, uint32_t m);
int pf_wo_step(lgh_ctx* c, lgh::LayerW& L, uint32_t m);
int pf_ffn_step(lgh_ctx* c, lgh::LayerW& L, const float* next_nw, uint32_t m);
int pf_moe_step(lgh_ctx* c, lgh::LayerW& L, const float* next_nw, uint32_t m);
int prefill_own(lgh_ctx* c, const uint32_t* tokens, size_t n);   // the context's own sequence: blocks of <= 128, position and ST_NEXT moved
// device prompt cache (kv_prefix.hip).  Rows [0, n_rows) of every tensor of every owned layer of one sequence (slot < 0: the context's
// own) to (restore: from) a packed buffer of n_stride rows, [layer][kind][kv head][n_stride][bytes per position]: one launch on the
// context's stream
int kv_prefix_copy(lgh_ctx* c, int slot, uint32_t n_rows, uint32_t n_stride, void* packed, bool restore);
uint64_t kv_prefix_bytes(const lgh_ctx* c, uint64_t n_rows);   // bytes of n_rows packed rows of this context's layers
void kv_prefix_release(lgh_ctx* c);                            // frees the live prefixes (lgh_destroy)
// sampler plumbing (sample.hip)
int samp_alloc(lgh_ctx* c, lgh::SampBufs& B, uint32_t n_slots, uint32_t n_rows);
int samp_check(lgh_ctx* c, const lgh_sampler_config* cfg);
int samp_check_ex(lgh_ctx* c, const lgh_sampler_config_ex* cfg);
lgh_sampler_config_ex samp_plain(const lgh_sampler_config& cfg);   // cfg with min_p 0 and Mirostat off
bool samp_needs_uniforms(const lgh_sampler_config_ex& cfg);        // anything but the greedy settings draws
int samp_reset(lgh_ctx* c, lgh::SampBufs& B, uint32_t slot, const lgh_sampler_config_ex& cfg);   // Sampler::new: zero the slot's counts, mu = 2 * tau
int samp_mu(lgh_ctx* c, lgh::SampBufs& B, uint32_t slot, float* mu);   // the slot's mirostat_mu (synchronises)
// before the first step of a decode call: the slot's config, window, leaving tokens and draws (synchronises)
int samp_begin(lgh_ctx* c, lgh::SampBufs& B, uint32_t slot, const lgh_sampler_config_ex& cfg, const uint32_t* hist, size_t n_hist,
               uint32_t first, size_t n_steps, const float* uni, size_t uni_stride);
int samp_warm(lgh_ctx* c, lgh::SampBufs& B, const float* logits, uint32_t n_seq);   // eager launch of the sampling kernels (before any capture)
int samp_one(lgh_ctx* c, lgh::SampBufs& B, const lgh_sampler_config_ex& cfg, const uint32_t* recent, size_t n_recent, const uint32_t* counts,
             float uniform, float mu_in, const float* d_logits, uint32_t* token_out, float* mu_out);   // lgh_op_sample(_ex)

// ------------------------------------------------------------------------------------------------
// launch recording (profiling mode: hipEvent pair per launch, on the launch stream)
// ------------------------------------------------------------------------------------------------
template <class F>
inline int run_k(lgh_ctx* c, int cls, int sym, uint64_t alg_bytes, F&& f) {
  lgh::ProfRec rec{cls, sym, alg_bytes, nullptr, nullptr};
  if (c->profiling) {
    if (hipEventCreate(&rec.a) != hipSuccess || hipEventCreate(&rec.b) != hipSuccess) return fail(c, LGH_OPERATION_FAILED, "hipEventCreate");
    (void)hipEventRecord(rec.a, c->stream);
  }
  hipError_t e = f();
  if (e != hipSuccess) return fail(c, LGH_OPERATION_FAILED, std::string("kernel launch (class ") + std::to_string(cls) + "): " + hipGetErrorString(e));
  if (c->profiling) {
    (void)hipEventRecord(rec.b, c->stream);
    c->prof.push_back(rec);
  }
  return LGH_OK;
}

