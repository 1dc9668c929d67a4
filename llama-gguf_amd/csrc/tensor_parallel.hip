// tensor_parallel.hip — tensor-parallel decode INSIDE the library: one process, N rank contexts on N devices (or all on one), every
// rank reading 1/N of each layer's weight bytes for the SAME token.
//
// The reference states the scheme in src/backend/tensor_parallel.rs: attention heads split over the devices, gate / up split by
// output columns, down (and wo) by input rows, an all-reduce after each (lines 1-6); ShardingPlan::from_config (54-107) holds the
// divisibility rules.  Its shard_weight (115-) refuses quantized tensors; this engine keeps weights quantized, so lgh_tp_shard
// slices GGUF payloads by whole rows or whole 256-element blocks.
//
// A rank is an ordinary lgh_ctx with num_heads / N, num_kv_heads / N and intermediate_size / N (head_dim is its own field of the
// descriptor).  The driver below walks the layer-step functions of engine_layer.hip — the ones the single-sequence engine runs —
// and stops at the two places of a layer where the ranks' results meet: wo and down store a PARTIAL vector (plain store, no
// residual), and tp_reduce_kernel, the one new kernel, leaves on every rank  h = resid + (((p0 + p1) + p2) ...)  — the all-reduce
// followed by the residual add (layers.rs:1201-1208) — together with the XQ image of h times the next consumer's norm weights and
// the per-chunk sums of h^2, exactly what the mat-vec epilogues leave for a matrix-core consumer.  The sum runs in rank order on
// every rank, so all ranks hold the same bits.
//
// A prompt goes through lgh_tp_prefill_batch in blocks of up to 128 tokens (tp_prefill_block below): the single context's GEMMs, QKV
// epilogue, block attention and SwiGLU on every rank, and at the two meeting places tp_prefill.hip's block forms of the reduce.
//
// Ranks that share a device share ONE stream and the whole token is ONE linear captured graph (no parallel branches, no event
// nodes), like the same-device stages of pipeline.hip.  Ranks on distinct devices run the same launch order eagerly on their own
// streams, with one event per synchronisation point and rank, waited for by the peers, and read the peers' partial vectors
// through peer-mapped pointers.
#include "engine.h"
#include "tp_prefill.h"
#include "xq.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace lgh;

namespace lgh {

constexpr int kTpMaxRanks = 8;
struct TpPeers { const float* p[kTpMaxRanks - 1]; };   // the partial vectors of ranks 1 .. N - 1 (rank 0's is an argument of its own)

// One wave per 256 elements (one XQ record).  A lane sums 4 consecutive elements with 16-byte loads, all of them requested before
// the first is used; for the image the wave's 256 values cross LDS once, from 4 elements per lane to one element per lane of a
// 16-lane row (what xq_store_chunk takes).  Rows of 64 values sit 80 floats apart in LDS, so the two rows of a 32-lane half read
// different banks.  `out` may be `resid` (the rank's residual stream, in place): a lane reads and writes the same 4 elements.
template <int N>
__global__ void __launch_bounds__(64) tp_reduce_kernel(const float* p0, const float* resid, const float* nw, float* out, uint8_t* xq,
                                                       float* ssq, uint32_t H, TpPeers peers) {
  __shared__ __attribute__((aligned(16))) float s_v[320], s_h[320];
  const uint32_t lane = threadIdx.x, e0 = blockIdx.x * 256 + lane * 4;
  const bool ok = e0 < H;
  const uint32_t ec = ok ? e0 : 0;   // clamped: the loads are unconditional
  f32x4 p[N];
  p[0] = *reinterpret_cast<const f32x4*>(p0 + ec);
#pragma unroll
  for (int r = 1; r < N; r++) p[r] = *reinterpret_cast<const f32x4*>(peers.p[r - 1] + ec);
  f32x4 rs = (f32x4)(0.0f), w = (f32x4)(1.0f);
  if (resid) rs = *reinterpret_cast<const f32x4*>(resid + ec);   // (uniform branches: every load is requested before the first is used;
  if (xq && nw) w = *reinterpret_cast<const f32x4*>(nw + ec);    //  selecting the address instead made the compiler wait in between)
  f32x4 s = p[0];
#pragma unroll
  for (int r = 1; r < N; r++) s += p[r];   // rank order, one rounding per add
  const f32x4 h = resid ? rs + s : s;
  if (ok) *reinterpret_cast<f32x4*>(out + e0) = h;
  if (!xq) return;
  const uint32_t slot = lane * 4 + (lane >> 4) * 16;
  *reinterpret_cast<f32x4*>(s_v + slot) = nw ? h * w : h;
  *reinterpret_cast<f32x4*>(s_h + slot) = h;
  __syncthreads();
#pragma unroll
  for (uint32_t c = 0; c < 4; c++) {
    const uint32_t row = lane >> 4, e = blockIdx.x * 256 + row * 64 + c * 16 + (lane & 15);
    const uint32_t at = row * 80 + c * 16 + (lane & 15);
    if (e < H) xq_store_chunk(xq, e >> 4, s_v[at], ssq, s_h[at], lane);   // (H % 16 == 0: a 16-lane row is in or out as a whole)
  }
}

// parts[r]: rank r's partial vector [H] (n of them, H % 16 == 0, everything 16-byte aligned); resid / nw / xq / ssq may be null
hipError_t tp_reduce_launch(const float* const* parts, uint32_t n, const float* resid, const float* nw, uint32_t H, float* out, uint8_t* xq,
                            float* ssq, hipStream_t st) {
  if (n < 1 || n > (uint32_t)kTpMaxRanks || H == 0 || H % 16) return hipErrorInvalidValue;
  TpPeers peers{};
  for (uint32_t r = 1; r < n; r++) peers.p[r - 1] = parts[r];
  const dim3 g((H + 255) / 256), t(64);
  switch (n) {
    case 1: hipLaunchKernelGGL(tp_reduce_kernel<1>, g, t, 0, st, parts[0], resid, nw, out, xq, ssq, H, peers); break;
    case 2: hipLaunchKernelGGL(tp_reduce_kernel<2>, g, t, 0, st, parts[0], resid, nw, out, xq, ssq, H, peers); break;
    case 3: hipLaunchKernelGGL(tp_reduce_kernel<3>, g, t, 0, st, parts[0], resid, nw, out, xq, ssq, H, peers); break;
    case 4: hipLaunchKernelGGL(tp_reduce_kernel<4>, g, t, 0, st, parts[0], resid, nw, out, xq, ssq, H, peers); break;
    case 5: hipLaunchKernelGGL(tp_reduce_kernel<5>, g, t, 0, st, parts[0], resid, nw, out, xq, ssq, H, peers); break;
    case 6: hipLaunchKernelGGL(tp_reduce_kernel<6>, g, t, 0, st, parts[0], resid, nw, out, xq, ssq, H, peers); break;
    case 7: hipLaunchKernelGGL(tp_reduce_kernel<7>, g, t, 0, st, parts[0], resid, nw, out, xq, ssq, H, peers); break;
    default: hipLaunchKernelGGL(tp_reduce_kernel<8>, g, t, 0, st, parts[0], resid, nw, out, xq, ssq, H, peers); break;
  }
  return hipGetLastError();
}

}  // namespace lgh

struct lgh_tp {
  std::vector<lgh_ctx*> rank;
  std::vector<int> device;
  lgh_model_desc d{};                        // the WHOLE model's descriptor
  bool one_stream = true;                    // all ranks on one device: one stream, one graph per token
  bool finalized = false;
  std::vector<float*> part[2];               // [synchronisation point of a layer: 0 after wo, 1 after down][rank] f32[hidden]
  std::vector<float*> pf_part[2];            // the batched prompt pass: the same two points, [rank] f32[128][hidden] (first lgh_tp_prefill_batch)
  bool pf_ready = false;
  std::vector<hipEvent_t> ev[3];             // distinct devices: [synchronisation point; 2 = the logits slices][rank]
  hipEvent_t token_back = nullptr;           // ... and rank 0's arg-max has been copied into every rank's token word
  std::vector<uint32_t> out_row0, out_rows;  // rank r's rows of the output projection
  hipGraphExec_t graph[3][2] = {};           // [mode][attention variant], as lgh_ctx::graph
  uint64_t graph_nodes = 0;
  size_t pos = 0;
  std::string err;
};

namespace {

thread_local std::string g_create_err;   // why the last lgh_tp_create of this thread failed (lgh_tp_last_error(NULL))

int tfail(lgh_tp* t, int status, const std::string& msg) {
  if (t) t->err = msg;
  else g_create_err = msg;
  return status;
}

int rank_fail(lgh_tp* t, size_t r, int status) { return tfail(t, status, "rank " + std::to_string(r) + ": " + lgh_last_error(t->rank[r])); }

#define TP_HIP(t, expr)                                                                                                \
  do {                                                                                                                 \
    hipError_t e__ = (expr);                                                                                           \
    if (e__ != hipSuccess) return tfail((t), LGH_OPERATION_FAILED, std::string(#expr) + ": " + hipGetErrorString(e__)); \
  } while (0)

bool tile_type(uint32_t t) {
  return t == LGH_TYPE_Q4_K || t == LGH_TYPE_Q5_K || t == LGH_TYPE_Q6_K || t == LGH_TYPE_Q8_0 || t == LGH_TYPE_Q4_0;
}

// rank `rank`'s rows of a tensor of ne1 rows: equal ranges where n divides ne1 (whole heads, the FFN's columns); otherwise whole
// 16-row tiles, the same number for every rank, the last rank also taking what is left (output.weight)
int row_range(uint64_t ne1, int rank, int n, uint64_t* r0, uint64_t* r1) {
  if (ne1 % (uint64_t)n == 0) {
    *r0 = ne1 / n * rank;
    *r1 = *r0 + ne1 / n;
    return LGH_OK;
  }
  const uint64_t per = (ne1 + 15) / 16 / (uint64_t)n;
  if (!per) return LGH_UNSUPPORTED;
  *r0 = per * 16 * rank;
  *r1 = rank + 1 == n ? ne1 : *r0 + per * 16;
  return LGH_OK;
}

}  // namespace

extern "C" {

int lgh_tp_shard(uint32_t type, const uint64_t ne[4], int axis, int rank, int n_ranks, const void* src, size_t src_bytes, void* dst,
                 size_t dst_bytes, size_t* written) {
  if (written) *written = 0;
  if (!ne || !src || !dst || !written) return LGH_INVALID_ARGUMENT;
  if (n_ranks < 1 || n_ranks > kTpMaxRanks || rank < 0 || rank >= n_ranks || (axis != 0 && axis != 1)) return LGH_INVALID_ARGUMENT;
  const uint32_t bs = blk_elems((int)type), bb = blk_bytes((int)type);
  if (!bs) return LGH_UNSUPPORTED_DTYPE;
  const uint64_t ne0 = ne[0], ne1 = ne[1] ? ne[1] : 1;
  if (ne[2] > 1 || ne[3] > 1) return LGH_UNSUPPORTED;   // (expert stacks: MoE over tensor parallelism is not built)
  if (!ne0 || ne0 % bs) return LGH_SHAPE_MISMATCH;
  const uint64_t row_bytes = ne0 / bs * bb;
  if (src_bytes != ne1 * row_bytes) return LGH_SHAPE_MISMATCH;
  const uint8_t* s = (const uint8_t*)src;
  if (axis == 0) {
    uint64_t r0 = 0, r1 = 0;
    if (int rc = row_range(ne1, rank, n_ranks, &r0, &r1)) return rc;
    const uint64_t need = (r1 - r0) * row_bytes;
    if (dst_bytes < need) return LGH_INVALID_ARGUMENT;
    std::memcpy(dst, s + r0 * row_bytes, need);
    *written = need;
    return LGH_OK;
  }
  // k-shards are whole 256-element blocks of every row: what a matrix-core tile holds of one row
  if (ne0 % (256ull * (uint64_t)n_ranks)) return LGH_UNSUPPORTED;
  const uint64_t seg = row_bytes / (uint64_t)n_ranks, need = ne1 * seg;
  if (dst_bytes < need) return LGH_INVALID_ARGUMENT;
  for (uint64_t r = 0; r < ne1; r++) std::memcpy((uint8_t*)dst + r * seg, s + r * row_bytes + (uint64_t)rank * seg, seg);
  *written = need;
  return LGH_OK;
}

// ShardingPlan::from_config (tensor_parallel.rs:69-106) plus what the tile layouts and this engine's scope need
int lgh_tp_create(const lgh_model_desc* desc, const int* device_ids, int n_ranks, lgh_tp** out) {
  g_create_err.clear();
  if (!desc || !out || desc->struct_size != sizeof(lgh_model_desc)) return tfail(nullptr, LGH_INVALID_ARGUMENT, "descriptor or out is NULL, or struct_size is wrong");
  *out = nullptr;
  const lgh_model_desc& d = *desc;
  const std::string ws = "world_size (" + std::to_string(n_ranks) + ")";
  if (n_ranks < 1 || n_ranks > kTpMaxRanks) return tfail(nullptr, LGH_INVALID_ARGUMENT, ws + " must be between 1 and 8");
  const uint32_t N = (uint32_t)n_ranks;
  if (d.layer_begin != 0 || (d.layer_end != 0 && d.layer_end != d.num_layers))
    return tfail(nullptr, LGH_INVALID_ARGUMENT, "a layer_begin / layer_end range cannot be combined with tensor parallelism");
  if (d.num_experts) return tfail(nullptr, LGH_UNSUPPORTED, "MoE models are not sharded over tensor-parallel ranks");
  if (d.kv_cache_type != LGH_KV_F32 || (d.flags & LGH_FLAG_KV_INT8))
    return tfail(nullptr, LGH_UNSUPPORTED, "tensor-parallel decode runs over the f32 KV cache only (kv_cache_type " + std::to_string(d.kv_cache_type) + ")");
  if (d.num_heads % N) return tfail(nullptr, LGH_INVALID_ARGUMENT, "num_heads (" + std::to_string(d.num_heads) + ") must be divisible by " + ws);
  if (d.num_kv_heads % N) return tfail(nullptr, LGH_INVALID_ARGUMENT, "num_kv_heads (" + std::to_string(d.num_kv_heads) + ") must be divisible by " + ws);
  if (d.intermediate_size % N) return tfail(nullptr, LGH_INVALID_ARGUMENT, "ffn_dim (" + std::to_string(d.intermediate_size) + ") must be divisible by " + ws);
  const uint32_t qd = d.num_heads / N * d.head_dim, fd = d.intermediate_size / N;
  if (!qd || qd % 256)
    return tfail(nullptr, LGH_UNSUPPORTED, "a rank's attention width (num_heads / world_size) * head_dim = " + std::to_string(qd) +
                                           " must be a multiple of 256: attn_output is split by whole 256-element blocks");
  if (!fd || fd % 256)
    return tfail(nullptr, LGH_UNSUPPORTED, "a rank's FFN width intermediate_size / world_size = " + std::to_string(fd) +
                                           " must be a multiple of 256: ffn_down is split by whole 256-element blocks");
  if (!d.hidden_size || d.hidden_size % 256)
    return tfail(nullptr, LGH_UNSUPPORTED, "hidden_size " + std::to_string(d.hidden_size) + " must be a multiple of 256 (matrix-core tile layouts)");
  if ((d.vocab_size + 15) / 16 < N) return tfail(nullptr, LGH_UNSUPPORTED, "vocab_size " + std::to_string(d.vocab_size) + " has fewer 16-row tiles than ranks");
  lgh_tp* t = new lgh_tp();
  t->d = d;
  for (uint32_t r = 0; r < N; r++) {
    lgh_model_desc rd = d;
    rd.device_id = device_ids ? device_ids[r] : d.device_id;
    rd.num_heads = d.num_heads / N;
    rd.num_kv_heads = d.num_kv_heads / N;
    rd.intermediate_size = fd;
    rd.flags |= LGH_FLAG_NO_GRAPH;   // a rank never replays a graph of its own: the token's graph is the driver's (tp_step)
    lgh_ctx* c = nullptr;
    const int rc = lgh_create(&rd, &c);
    if (rc) {
      std::string why;
      (void)engine_shape_check(rd, why);
      for (lgh_ctx* q : t->rank) lgh_destroy(q);
      delete t;
      return tfail(nullptr, rc, "rank " + std::to_string(r) + ": lgh_create failed" + (why.empty() ? "" : ": " + why));
    }
    t->rank.push_back(c);
    t->device.push_back(rd.device_id);
    if (rd.device_id != t->device[0]) t->one_stream = false;
  }
  *out = t;
  return LGH_OK;
}

int lgh_tp_upload_tensor(lgh_tp* t, const char* name, uint32_t type, const uint64_t ne[4], const void* host, size_t nbytes) {
  if (!t || !name || !ne || !host) return LGH_INVALID_ARGUMENT;
  if (t->finalized) return tfail(t, LGH_INVALID_ARGUMENT, "upload after finalize");
  const std::string nm(name);
  const int N = (int)t->rank.size();
  auto ends_with = [&](const char* suffix) {
    const size_t n = std::strlen(suffix);
    return nm.size() >= n && nm.compare(nm.size() - n, n, suffix) == 0;
  };
  // axis: -1 every rank takes the whole tensor, -2 rank 0 alone takes it, 0 / 1 lgh_tp_shard's
  int axis;
  bool matrix = true;
  if (nm == "token_embd.weight" || ends_with("_norm.weight")) { axis = -1; matrix = false; }
  else if (nm == "output.weight" || ends_with(".attn_q.weight") || ends_with(".attn_k.weight") || ends_with(".attn_v.weight") ||
           ends_with(".ffn_gate.weight") || ends_with(".ffn_up.weight")) axis = 0;
  else if (ends_with(".attn_q.bias") || ends_with(".attn_k.bias") || ends_with(".attn_v.bias")) { axis = 0; matrix = false; }
  else if (ends_with(".attn_output.weight") || ends_with(".ffn_down.weight")) axis = 1;
  else if (ends_with(".attn_output.bias")) { axis = -2; matrix = false; }
  else if (nm.find("_exps.") != std::string::npos || nm.find("ffn_gate_inp") != std::string::npos)
    return tfail(t, LGH_UNSUPPORTED, nm + ": MoE models are not sharded over tensor-parallel ranks");
  else return tfail(t, LGH_INVALID_ARGUMENT, "unknown tensor name " + nm);
  if (matrix && (!tile_type(type) || ne[0] % 256))
    return tfail(t, LGH_UNSUPPORTED, nm + ": ggml type " + std::to_string(type) + " with " + std::to_string(ne[0]) +
                                     " input features is outside the matrix-core tile layouts (Q4_K, Q5_K, Q6_K, Q8_0, Q4_0; k a multiple of 256)");
  if (axis < 0) {
    for (int r = 0; r < (axis == -2 ? 1 : N); r++)
      if (int rc = lgh_upload_tensor(t->rank[r], name, type, ne, host, nbytes)) return rank_fail(t, r, rc);
    return LGH_OK;
  }
  // a bias is a vector of ne[0] values: its rows are its elements
  uint64_t sne[4] = {ne[0], ne[1], ne[2], ne[3]};
  if (!matrix) {
    if (blk_elems((int)type) != 1) return tfail(t, LGH_UNSUPPORTED, nm + ": a sharded bias must be F32 / F16 / BF16");
    sne[0] = 1; sne[1] = ne[0] * (ne[1] ? ne[1] : 1);
  }
  std::vector<uint8_t> buf(nbytes);
  for (int r = 0; r < N; r++) {
    size_t got = 0;
    const int rs = lgh_tp_shard(type, sne, axis, r, N, host, nbytes, buf.data(), buf.size(), &got);
    if (rs) return tfail(t, rs, nm + ": cannot be split over " + std::to_string(N) + " ranks along " + (axis ? "k" : "its rows"));
    const uint32_t bs = blk_elems((int)type), bb = blk_bytes((int)type);
    uint64_t rne[4] = {ne[0], ne[1], 0, 0};
    if (!matrix) rne[0] = got / bb, rne[1] = 0;
    else if (axis == 0) rne[1] = got / (ne[0] / bs * bb);
    else rne[0] = ne[0] / (uint64_t)N;
    lgh_ctx* c = t->rank[r];
    int rc;
    if (nm == "output.weight") {   // a rank's rows of the output projection: not vocab_size of them, so past lgh_upload_tensor's shape check
      if (hipSetDevice(c->device) != hipSuccess) return tfail(t, LGH_NOT_AVAILABLE, "hipSetDevice failed");
      if (ne[0] != c->d.hidden_size || (ne[1] ? ne[1] : 1) != c->d.vocab_size) return tfail(t, LGH_SHAPE_MISMATCH, "output.weight shape");
      c->embd_host.clear();
      c->embd_host.shrink_to_fit();
      rc = upload_matrix(c, c->output, (int)type, (uint32_t)rne[0], (uint32_t)rne[1], 1, -1, buf.data(), got);
    } else {
      rc = lgh_upload_tensor(c, name, type, rne, buf.data(), got);
    }
    if (rc) return rank_fail(t, r, rc);
  }
  return LGH_OK;
}

}  // extern "C"

namespace {

hipStream_t stream_of(lgh_ctx* c) { return c->stream; }

// Synchronisation point `which` of the token: every rank has launched what the others are about to read.  On one stream the
// launch order is the dependency; across devices every rank records its event and waits for the peers'.
int sync_point(lgh_tp* t, int which) {
  if (t->one_stream) return LGH_OK;
  const size_t n = t->rank.size();
  for (size_t r = 0; r < n; r++) {
    TP_HIP(t, hipSetDevice(t->device[r]));
    TP_HIP(t, hipEventRecord(t->ev[which][r], stream_of(t->rank[r])));
  }
  for (size_t r = 0; r < n; r++) {
    TP_HIP(t, hipSetDevice(t->device[r]));
    for (size_t q = 0; q < n; q++)
      if (q != r && stream_of(t->rank[q]) != stream_of(t->rank[r])) TP_HIP(t, hipStreamWaitEvent(stream_of(t->rank[r]), t->ev[which][q], 0));
  }
  return LGH_OK;
}

int bind_rank(lgh_tp* t, size_t r) {
  if (!t->one_stream) TP_HIP(t, hipSetDevice(t->device[r]));
  return LGH_OK;
}

// the rank's residual stream after a synchronisation point: hidden = hidden + sum of the ranks' partials, and the image for `nw`'s consumer
int reduce_step(lgh_tp* t, size_t r, int which, const float* nw, bool image) {
  lgh_ctx* c = t->rank[r];
  const uint32_t H = c->d.hidden_size;
  XqBuf* qh = image ? xq_get(c, c->hidden, H) : nullptr;
  if (image && !qh) return tfail(t, LGH_ALLOCATION_FAILED, "XQ image allocation failed");
  const int rc = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, (uint64_t)(t->rank.size() + 2) * H * 4, [&] {
    return tp_reduce_launch(t->part[which].data(), (uint32_t)t->rank.size(), c->hidden, qh ? nw : nullptr, H, c->hidden, qh ? qh->xq : nullptr,
                            qh && nw ? qh->ssq : nullptr, c->stream);
  });
  if (rc) return rank_fail(t, r, rc);
  if (qh) { qh->fresh = true; qh->tag = nw; }
  else xq_stale(c, c->hidden);
  return LGH_OK;
}

// Everything one token needs on every rank, in launch order (eager or under capture).  mode: TokenMode's PREFILL / FORWARD / GREEDY.
int tp_enqueue(lgh_tp* t, int mode) {
  const size_t n = t->rank.size();
  const lgh_model_desc& d = t->d;
  int rc;
#define RANK_TRY(r, expr)                           \
  do {                                              \
    if ((rc = bind_rank(t, (r)))) return rc;        \
    if ((rc = (expr))) return rank_fail(t, (r), rc); \
  } while (0)
  for (size_t r = 0; r < n; r++) {   // every rank dequantizes the token's row itself: identical bits, nothing to broadcast
    lgh_ctx* c = t->rank[r];
    for (auto& q : c->xqs) q.fresh = false;
    RANK_TRY(r, embed_forward(c));
  }
  const float scale = 1.0f / std::sqrt((float)d.head_dim);   // layers.rs:374
  for (uint32_t li = 0; li < d.num_layers; li++) {
    for (size_t r = 0; r < n; r++) {   // own heads over own KV cache, then wo over the k-shard: a partial of the whole hidden vector
      lgh_ctx* c = t->rank[r];
      LayerW& Lw = c->layers[li];
      const AttnView av{c->hidden, c->q, c->kv_tmp, c->attn_out};
      RANK_TRY(r, qkv_forward(c, Lw, av));
      RANK_TRY(r, attention_forward(c, Lw, li, av, scale, mfma_type(Lw.wo.type)));
      RANK_TRY(r, linear_any(c, LGH_K_WO, Lw.wo, c->attn_out, t->part[0][r], nullptr, nullptr, Lw.bo));
    }
    if ((rc = sync_point(t, 0))) return rc;
    for (size_t r = 0; r < n; r++) {
      if ((rc = bind_rank(t, r))) return rc;
      LayerW& Lw = t->rank[r]->layers[li];
      if ((rc = reduce_step(t, r, 0, Lw.ffn_norm, mfma_type(Lw.gate.type)))) return rc;
    }
    for (size_t r = 0; r < n; r++) {   // own columns of gate | up, then down over the k-shard
      lgh_ctx* c = t->rank[r];
      LayerW& Lw = c->layers[li];
      RANK_TRY(r, ffn_gateup_forward(c, Lw, FfnView{c->hidden, c->act, c->act2, c->xnorm, c->moe_sel, c->moe_w}));
      RANK_TRY(r, linear_any(c, LGH_K_DOWN, Lw.down, c->act, t->part[1][r], nullptr, nullptr, nullptr));
    }
    if ((rc = sync_point(t, 1))) return rc;
    for (size_t r = 0; r < n; r++) {   // the next consumer: the next layer's QKV, the output projection, or (a prompt token) nobody
      if ((rc = bind_rank(t, r))) return rc;
      lgh_ctx* c = t->rank[r];
      const float* next_nw = nullptr;
      bool next_mfma = false;
      if (li + 1 < d.num_layers) { next_nw = c->layers[li + 1].attn_norm; next_mfma = mfma_type(c->layers[li + 1].wq.type); }
      else if (mode != MODE_PREFILL) { next_nw = c->output_norm; next_mfma = mfma_type(c->output.type); }
      if ((rc = reduce_step(t, r, 1, next_nw, next_mfma))) return rc;
    }
  }
  if (mode == MODE_PREFILL) return LGH_OK;
  // compute_logits (llama.rs:247-266): every rank's rows of the output projection, straight into rank 0's logits vector
  lgh_ctx* c0 = t->rank[0];
  for (size_t r = 0; r < n; r++) {
    lgh_ctx* c = t->rank[r];
    RANK_TRY(r, linear_any(c, LGH_K_OUTPUT, c->output, c->hidden, c0->logits + t->out_row0[r], c->output_norm, nullptr, nullptr));
  }
  if ((rc = sync_point(t, 2)) || mode != MODE_GREEDY) return rc;   // (rank 0's stream now follows every rank's slice)
  RANK_TRY(0, run_k(c0, LGH_K_ARGMAX, LGH_SYM_ARGMAX, (uint64_t)d.vocab_size * 4, [&] {
             return argmax_launch(c0->logits, d.vocab_size, c0->amax_v, c0->amax_i, c0->state, c0->tok_log, c0->stream);
           }));
  for (size_t r = 1; r < n; r++)   // the greedy token into every rank's token word, on the device
    RANK_TRY(0, run_k(c0, LGH_K_MISC, LGH_SYM_OTHER, 8, [&] { return copy_words_launch(t->rank[r]->state + ST_TOKEN, c0->state + ST_ARGMAX, 1, c0->stream); }));
  if (!t->one_stream) {
    TP_HIP(t, hipEventRecord(t->token_back, c0->stream));
    for (size_t r = 1; r < n; r++) {
      TP_HIP(t, hipSetDevice(t->device[r]));
      if (stream_of(t->rank[r]) != c0->stream) TP_HIP(t, hipStreamWaitEvent(stream_of(t->rank[r]), t->token_back, 0));
    }
  }
#undef RANK_TRY
  return LGH_OK;
}

void tp_drop_graphs(lgh_tp* t) {
  for (auto& gm : t->graph)
    for (auto& ge : gm)
      if (ge) { (void)hipGraphExecDestroy(ge); ge = nullptr; }
}

bool tp_eager(const lgh_tp* t) { return !t->one_stream || (t->d.flags & LGH_FLAG_NO_GRAPH); }

// one token in `mode`, the token id already in every rank's device state
int tp_step(lgh_tp* t, int mode) {
  if (t->pos >= t->d.max_seq_len)
    return tfail(t, LGH_INVALID_ARGUMENT, "position " + std::to_string(t->pos) + " >= max_seq_len " + std::to_string(t->d.max_seq_len));
  bool direct = false;
  for (lgh_ctx* c : t->rank) {   // (every rank has the same thresholds: one attention variant per token)
    c->pos = t->pos;
    c->attn_direct = c->pos + 1 <= c->direct_attn_max_kv ? ATTN_VAR_HEAD : ATTN_VAR_SPLIT;
    direct = c->attn_direct != ATTN_VAR_SPLIT;
  }
  int rc;
  TP_HIP(t, hipSetDevice(t->device[0]));
  if (tp_eager(t)) {
    if ((rc = tp_enqueue(t, mode))) return rc;
  } else {
    lgh_ctx* c0 = t->rank[0];
    hipGraphExec_t& g = t->graph[mode][direct ? 1 : 0];
    if (!g) {
      size_t nodes = 0;
      int inner = LGH_OK;
      rc = capture_graph(c0, &g, [&] { return inner = tp_enqueue(t, mode); }, &nodes);
      if (rc) return inner ? rc : rank_fail(t, 0, rc);
      if (nodes && (mode == MODE_GREEDY || !t->graph_nodes)) t->graph_nodes = nodes;
    }
    TP_HIP(t, hipGraphLaunch(g, c0->stream));
  }
  t->pos += 1;
  for (lgh_ctx* c : t->rank) { c->pos = t->pos; c->stats.tokens_processed += 1; }
  return LGH_OK;
}

int tp_set_token(lgh_tp* t, uint32_t token) {
  if (token >= t->d.vocab_size) return tfail(t, LGH_INVALID_ARGUMENT, "token id exceeds vocab size");   // llama.rs:296-302
  for (size_t r = 0; r < t->rank.size(); r++) {
    TP_HIP(t, hipSetDevice(t->device[r]));
    TP_HIP(t, hipMemsetD32Async((hipDeviceptr_t)(t->rank[r]->state + ST_TOKEN), (int)token, 1, stream_of(t->rank[r])));
  }
  return LGH_OK;
}

int tp_sync_all(lgh_tp* t) {
  for (size_t r = 0; r < t->rank.size(); r++) {
    if (t->one_stream && r > 0) break;
    if (int rc = lgh_synchronize(t->rank[r])) return rank_fail(t, r, rc);
  }
  return LGH_OK;
}

int tp_ready(lgh_tp* t) {
  if (!t) return LGH_INVALID_ARGUMENT;
  if (!t->finalized) return tfail(t, LGH_INVALID_ARGUMENT, "tensor-parallel context not finalized");
  return LGH_OK;
}

// ---- the batched prompt pass (tp_prefill.hip; the single context's is engine_prefill.hip's prefill_block) ----
bool tp_pf_eligible(const lgh_tp* t) {
  for (const lgh_ctx* c : t->rank)
    if (!pf_eligible(c, false)) return false;
  return true;
}

// every rank's prompt scratch and its two compact partial blocks, peer-readable as part[] is (peer access was enabled at finalize)
int tp_pf_ensure(lgh_tp* t) {
  if (t->pf_ready) return LGH_OK;
  const size_t n = t->rank.size();
  int rc;
  for (int w = 0; w < 2; w++) t->pf_part[w].assign(n, nullptr);
  for (size_t r = 0; r < n; r++) {
    lgh_ctx* c = t->rank[r];
    TP_HIP(t, hipSetDevice(t->device[r]));
    if ((rc = pf_ensure(c))) return rank_fail(t, r, rc);
    const size_t bytes = (size_t)kPfTokens * t->d.hidden_size * 4;
    const AllocSpec bufs[] = {{(void**)&t->pf_part[0][r], bytes}, {(void**)&t->pf_part[1][r], bytes}};
    if ((rc = alloc_zeroed(c, bufs, 2, c->stats.scratch_bytes))) return rank_fail(t, r, rc);
    TP_HIP(t, hipStreamSynchronize(c->stream));   // the zero-fills are done before a peer touches the blocks
  }
  t->pf_ready = true;
  return LGH_OK;
}

int tp_pf_k(lgh_tp* t, size_t r, hipError_t e, const char* what) {
  if (e == hipSuccess) return LGH_OK;
  return tfail(t, LGH_OPERATION_FAILED, "rank " + std::to_string(r) + ": batched prefill, " + what + ": " + hipGetErrorString(e));
}

// the rank's split-K partial sums of a wo / down GEMM -> its compact block of synchronisation point `which`
int tp_pf_partial_step(lgh_tp* t, size_t r, int which, uint32_t S, uint32_t ncols, const float* bias, uint32_t m) {
  lgh_ctx* c = t->rank[r];
  return tp_pf_k(t, r, tp_pf_partial_launch(c->pf.part, S, ncols, 0, bias, t->pf_part[which][r], c->d.hidden_size, m, c->stream), "partial block");
}

// the rank's block of residual rows after a synchronisation point, the XH of hidden * nw for the next GEMM (nw nullptr: none)
int tp_pf_reduce_step(lgh_tp* t, size_t r, int which, const float* nw, uint32_t m) {
  lgh_ctx* c = t->rank[r];
  PfScratch& P = c->pf;
  return tp_pf_k(t, r, tp_pf_reduce_launch(t->pf_part[which].data(), (uint32_t)t->rank.size(), P.hidden, c->d.hidden_size, nw, nw ? P.xh_h : nullptr, P.ssq, m,
                                           c->stream),
                 "reduce");
}

// One block of m <= 128 prompt tokens at positions t->pos .. t->pos + m - 1 on every rank, eagerly (never captured), in tp_enqueue's
// pattern: a loop over the ranks per stretch between two synchronisation points.  The distinct-device branch (sync_point's events,
// peer-mapped blocks) is the decode driver's and has NOT been executed: the development box has one GPU.
int tp_prefill_block(lgh_tp* t, const uint32_t* tokens, uint32_t m) {
  const size_t n = t->rank.size();
  const lgh_model_desc& d = t->d;
  const uint32_t pos0 = (uint32_t)t->pos;
  int rc;
  TP_HIP(t, hipSetDevice(t->device[0]));
#define RANK_TRY(r, expr)                           \
  do {                                              \
    if ((rc = bind_rank(t, (r)))) return rc;        \
    if ((rc = (expr))) return rank_fail(t, (r), rc); \
  } while (0)
  for (size_t r = 0; r < n; r++) {   // every rank dequantizes the block's rows itself: identical bits, nothing to broadcast
    lgh_ctx* c = t->rank[r];
    RANK_TRY(r, pf_embed_tokens(c, pos0, tokens, m));
    RANK_TRY(r, pf_block_input(c, c->layers[0].attn_norm, m));
  }
  for (uint32_t li = 0; li < d.num_layers; li++) {
    const bool attend = li + 1 < d.num_layers;   // the model's last layer: its K / V rows are written, its output would be discarded
    for (size_t r = 0; r < n; r++) {   // own heads into own cache rows, block attention over them, wo over the k-shard
      lgh_ctx* c = t->rank[r];
      LayerW& L = c->layers[li];
      PfScratch& P = c->pf;
      RANK_TRY(r, pf_qkv_step(c, L, L.kv.k_f32(), L.kv.v_f32(), pos0, m));
      if (!attend) continue;
      RANK_TRY(r, pf_attn_step(c, li, L.kv, pos0, m));
      uint32_t S = 0, nc = 0;
      const DevWeight* wo[1] = {&L.wo};
      if ((rc = tp_pf_k(t, r, pf_gemm_launch(wo, 1, P.xh_attn, P.part, P.part_bytes, m, &S, &nc, c->stream), "wo GEMM"))) return rc;
      if ((rc = tp_pf_partial_step(t, r, 0, S, nc, L.bo, m))) return rc;
    }
    if (!attend) break;
    if ((rc = sync_point(t, 0))) return rc;
    for (size_t r = 0; r < n; r++) {
      if ((rc = bind_rank(t, r))) return rc;
      if ((rc = tp_pf_reduce_step(t, r, 0, t->rank[r]->layers[li].ffn_norm, m))) return rc;
    }
    for (size_t r = 0; r < n; r++) {   // own columns of gate | up, SwiGLU, down over the k-shard
      lgh_ctx* c = t->rank[r];
      LayerW& L = c->layers[li];
      PfScratch& P = c->pf;
      const lgh_model_desc& rd = c->d;
      if ((rc = bind_rank(t, r))) return rc;
      uint32_t S = 0, nc = 0;
      const DevWeight* gu[2] = {&L.gate, &L.up};
      if ((rc = tp_pf_k(t, r, pf_gemm_launch(gu, 2, P.xh_h, P.part, P.part_bytes, m, &S, &nc, c->stream), "gate/up GEMM"))) return rc;
      if ((rc = tp_pf_k(t, r, pf_swiglu_launch(P.part, S, rd.intermediate_size, P.xh_act, P.ssq, rd.hidden_size, rd.norm_eps, m, c->stream), "SwiGLU"))) return rc;
      const DevWeight* dn[1] = {&L.down};
      if ((rc = tp_pf_k(t, r, pf_gemm_launch(dn, 1, P.xh_act, P.part, P.part_bytes, m, &S, &nc, c->stream), "down GEMM"))) return rc;
      if ((rc = tp_pf_partial_step(t, r, 1, S, nc, nullptr, m))) return rc;
    }
    if ((rc = sync_point(t, 1))) return rc;
    for (size_t r = 0; r < n; r++) {   // (li + 1 exists: the last layer left above)
      if ((rc = bind_rank(t, r))) return rc;
      if ((rc = tp_pf_reduce_step(t, r, 1, t->rank[r]->layers[li + 1].attn_norm, m))) return rc;
    }
  }
#undef RANK_TRY
  t->pos += m;
  for (size_t r = 0; r < n; r++) {
    lgh_ctx* c = t->rank[r];
    if ((rc = bind_rank(t, r))) return rc;
    c->pos = t->pos;
    c->stats.tokens_processed += m;
    TP_HIP(t, hipMemsetD32Async((hipDeviceptr_t)(c->state + ST_NEXT), (int)c->pos, 1, c->stream));
  }
  return LGH_OK;
}

}  // namespace

extern "C" {

int lgh_tp_finalize(lgh_tp* t) {
  if (!t) return LGH_INVALID_ARGUMENT;
  if (t->finalized) return LGH_OK;
  const size_t n = t->rank.size();
  const uint32_t H = t->d.hidden_size;
  int rc;
  t->out_row0.assign(n, 0);
  t->out_rows.assign(n, 0);
  for (size_t r = 0; r < n; r++) {
    lgh_ctx* c = t->rank[r];
    TP_HIP(t, hipSetDevice(t->device[r]));
    uint64_t r0 = 0, r1 = 0;
    if ((rc = row_range(t->d.vocab_size, (int)r, (int)n, &r0, &r1))) return tfail(t, rc, "vocab_size has fewer 16-row tiles than ranks");
    t->out_row0[r] = (uint32_t)r0;
    t->out_rows[r] = (uint32_t)(r1 - r0);
    if (!c->output.present() && !c->embd_host.empty()) {   // tied output projection (loader.rs:348-355): the rank's rows of token_embd
      if (!tile_type((uint32_t)c->embd_type))
        return tfail(t, LGH_UNSUPPORTED, "the tied output projection (token_embd.weight, ggml type " + std::to_string(c->embd_type) +
                                         ") is outside the matrix-core tile layouts");
      const uint64_t ne[4] = {H, t->d.vocab_size, 0, 0};
      std::vector<uint8_t> buf(c->embd_host.size());
      size_t got = 0;
      if ((rc = lgh_tp_shard((uint32_t)c->embd_type, ne, 0, (int)r, (int)n, c->embd_host.data(), c->embd_host.size(), buf.data(), buf.size(), &got)))
        return tfail(t, rc, "token_embd.weight cannot be split by rows for the tied output projection");
      if ((rc = upload_matrix(c, c->output, c->embd_type, H, t->out_rows[r], 1, -1, buf.data(), got))) return rank_fail(t, r, rc);
      c->embd_host.clear();
      c->embd_host.shrink_to_fit();
    }
    if (c->output.present() && c->output.n != t->out_rows[r]) return tfail(t, LGH_SHAPE_MISMATCH, "output.weight shard has the wrong number of rows");
    if ((rc = lgh_finalize(c))) return rank_fail(t, r, rc);
    for (uint32_t li = 0; li < t->d.num_layers; li++) {
      const LayerW& L = c->layers[li];
      for (const DevWeight* W : {&L.wq, &L.wk, &L.wv, &L.wo, &L.gate, &L.up, &L.down})
        if (!mfma_type(W->type)) return tfail(t, LGH_UNSUPPORTED, "blk." + std::to_string(li) + ": a weight is outside the matrix-core tile layouts");
    }
    if (!mfma_type(c->output.type)) return tfail(t, LGH_UNSUPPORTED, "the output projection is outside the matrix-core tile layouts");
  }
  // ranks on one device run on ONE stream (in launch order, no events between them): the first such rank's
  for (size_t r = 1; r < n; r++)
    for (size_t q = 0; q < r; q++)
      if (t->device[q] == t->device[r]) {
        if ((rc = lgh_set_stream(t->rank[r], lgh_get_stream(t->rank[q])))) return rank_fail(t, r, rc);
        break;
      }
  // every rank reads every peer's partial vectors and writes rank 0's logits and the peers' token words: direct peer access
  // between all pairs of distinct devices ("already enabled" is fine)
  for (size_t a = 0; a < n; a++)
    for (size_t b = 0; b < n; b++) {
      if (t->device[a] == t->device[b]) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, t->device[a], t->device[b]) != hipSuccess || !can)
        return tfail(t, LGH_NOT_AVAILABLE, "device " + std::to_string(t->device[a]) + " cannot access device " + std::to_string(t->device[b]) + " directly");
      TP_HIP(t, hipSetDevice(t->device[a]));
      const hipError_t e = hipDeviceEnablePeerAccess(t->device[b], 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return tfail(t, LGH_INITIALIZATION_FAILED, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
      (void)hipGetLastError();
    }
  for (int w = 0; w < 2; w++) t->part[w].assign(n, nullptr);
  for (size_t r = 0; r < n; r++) {
    lgh_ctx* c = t->rank[r];
    TP_HIP(t, hipSetDevice(t->device[r]));
    const AllocSpec bufs[] = {{(void**)&t->part[0][r], (size_t)H * 4}, {(void**)&t->part[1][r], (size_t)H * 4}};
    if ((rc = alloc_zeroed(c, bufs, 2, c->stats.scratch_bytes))) return rank_fail(t, r, rc);
    if (!t->one_stream)
      for (int w = 0; w < 3; w++) {
        t->ev[w].resize(n, nullptr);
        TP_HIP(t, hipEventCreateWithFlags(&t->ev[w][r], hipEventDisableTiming));
      }
  }
  if (!t->one_stream) {
    TP_HIP(t, hipSetDevice(t->device[0]));
    TP_HIP(t, hipEventCreateWithFlags(&t->token_back, hipEventDisableTiming));
  }
  t->finalized = true;
  t->pos = 0;
  // One token through every kernel of the step, launched eagerly, before any of them is first launched inside a stream capture
  // (engine.hip warm_kernels: a kernel whose first launch of the process happens during a capture is not replayed).  Token 0 at
  // position 0: it writes K / V row 0 of every layer, which the sequence's real first token overwrites before anything reads it.
  if (!tp_eager(t)) {
    for (int v = 0; v < 2; v++) {
      if (v == 1 && t->rank[0]->direct_attn_max_kv == 0) continue;
      for (int mode : {MODE_GREEDY, MODE_PREFILL}) {
        for (lgh_ctx* c : t->rank) {
          c->pos = 0;
          c->attn_direct = v == 1 ? ATTN_VAR_HEAD : ATTN_VAR_SPLIT;
          TP_HIP(t, hipMemsetAsync(c->state, 0, ST_WORDS * 4, c->stream));
        }
        if ((rc = tp_enqueue(t, mode))) return rc;
      }
    }
  }
  for (lgh_ctx* c : t->rank) {
    TP_HIP(t, hipSetDevice(c->device));
    c->pos = 0;
    for (auto& q : c->xqs) q.fresh = false;
    TP_HIP(t, hipMemsetAsync(c->state, 0, ST_WORDS * 4, c->stream));
  }
  return tp_sync_all(t);
}

void lgh_tp_destroy(lgh_tp* t) {
  if (!t) return;
  for (lgh_ctx* c : t->rank) (void)lgh_synchronize(c);
  tp_drop_graphs(t);
  for (auto& evs : t->ev)
    for (hipEvent_t e : evs)
      if (e) (void)hipEventDestroy(e);
  if (t->token_back) (void)hipEventDestroy(t->token_back);
  for (lgh_ctx* c : t->rank) lgh_destroy(c);
  delete t;
}

int lgh_tp_forward(lgh_tp* t, uint32_t token, float* logits_out) {
  int rc = tp_ready(t);
  if (rc) return rc;
  if (!logits_out) return tfail(t, LGH_INVALID_ARGUMENT, "logits_out is NULL");
  if (t->pos >= t->d.max_seq_len)
    return tfail(t, LGH_INVALID_ARGUMENT, "position " + std::to_string(t->pos) + " >= max_seq_len " + std::to_string(t->d.max_seq_len));
  if ((rc = tp_set_token(t, token)) || (rc = tp_step(t, MODE_FORWARD))) return rc;
  lgh_ctx* c0 = t->rank[0];   // (its stream has waited for every rank's slice of the logits)
  TP_HIP(t, hipSetDevice(t->device[0]));
  TP_HIP(t, hipMemcpyAsync(logits_out, c0->logits, (size_t)t->d.vocab_size * 4, hipMemcpyDeviceToHost, c0->stream));
  TP_HIP(t, hipStreamSynchronize(c0->stream));
  return LGH_OK;
}

int lgh_tp_prefill_token(lgh_tp* t, uint32_t token) {
  int rc = tp_ready(t);
  if (rc) return rc;
  if (t->pos >= t->d.max_seq_len)
    return tfail(t, LGH_INVALID_ARGUMENT, "position " + std::to_string(t->pos) + " >= max_seq_len " + std::to_string(t->d.max_seq_len));
  if ((rc = tp_set_token(t, token))) return rc;
  return tp_step(t, MODE_PREFILL);
}

int lgh_tp_prefill_is_batched(lgh_tp* t) { return t && t->finalized && tp_pf_eligible(t) ? 1 : 0; }

// GpuOnlyInference::forward_batch minus the last token (gpu_only.rs:776-790) over the ranks: blocks of up to 128 tokens on the batched
// path, or n exact lgh_tp_prefill_tokens.  Everything is checked before anything moves.
int lgh_tp_prefill_batch(lgh_tp* t, const uint32_t* tokens, size_t n) {
  int rc = tp_ready(t);
  if (rc) return rc;
  if (n && !tokens) return tfail(t, LGH_INVALID_ARGUMENT, "tokens is NULL");
  if (t->pos + n > t->d.max_seq_len)
    return tfail(t, LGH_INVALID_ARGUMENT, "prompt of " + std::to_string(n) + " tokens at position " + std::to_string(t->pos) + " exceeds max_seq_len");
  for (size_t i = 0; i < n; i++)
    if (tokens[i] >= t->d.vocab_size) return tfail(t, LGH_INVALID_ARGUMENT, "token id exceeds vocab size");
  if (n >= 2 && tp_pf_eligible(t)) {
    if ((rc = tp_pf_ensure(t))) return rc;
    for (size_t i = 0; i < n; i += kPfTokens)
      if ((rc = tp_prefill_block(t, tokens + i, (uint32_t)std::min<size_t>(kPfTokens, n - i)))) return rc;
  } else {
    for (size_t i = 0; i < n; i++)
      if ((rc = lgh_tp_prefill_token(t, tokens[i]))) return rc;
  }
  return tp_sync_all(t);
}

int lgh_tp_get_stats(lgh_tp* t, int rank, lgh_stats* out) {
  if (!t || !out || rank < 0 || (size_t)rank >= t->rank.size()) return LGH_INVALID_ARGUMENT;
  return lgh_get_stats(t->rank[(size_t)rank], out);
}

int lgh_tp_decode_greedy(lgh_tp* t, uint32_t first_token, size_t n_steps, uint32_t* tokens_out) {
  int rc = tp_ready(t);
  if (rc) return rc;
  if (n_steps && !tokens_out) return tfail(t, LGH_INVALID_ARGUMENT, "tokens_out is NULL");
  if (t->pos + n_steps > t->d.max_seq_len) return tfail(t, LGH_INVALID_ARGUMENT, "decode would exceed max_seq_len");
  const size_t pos0 = t->pos;
  if ((rc = tp_set_token(t, first_token))) return rc;
  for (size_t i = 0; i < n_steps; i++)
    if ((rc = tp_step(t, MODE_GREEDY))) return rc;
  lgh_ctx* c0 = t->rank[0];
  TP_HIP(t, hipSetDevice(t->device[0]));
  if (n_steps) TP_HIP(t, hipMemcpyAsync(tokens_out, c0->tok_log + pos0, n_steps * 4, hipMemcpyDeviceToHost, c0->stream));
  return tp_sync_all(t);
}

void lgh_tp_reset(lgh_tp* t) {
  if (!t || !t->finalized) return;
  for (lgh_ctx* c : t->rank) lgh_reset(c);
  t->pos = 0;
}

size_t lgh_tp_position(const lgh_tp* t) { return t ? t->pos : 0; }

// KVCache::truncate on every rank (src/model/mod.rs:130-134: the positions from new_len on are forgotten)
int lgh_tp_kv_truncate(lgh_tp* t, size_t new_len) {
  int rc = tp_ready(t);
  if (rc) return rc;
  if (new_len > t->pos) return tfail(t, LGH_INVALID_ARGUMENT, "new_len exceeds the current position");
  for (size_t r = 0; r < t->rank.size(); r++)
    if ((rc = lgh_kv_truncate(t->rank[r], new_len))) return rank_fail(t, r, rc);
  t->pos = new_len;
  return LGH_OK;
}

int lgh_tp_ranks(const lgh_tp* t) { return t ? (int)t->rank.size() : 0; }

uint64_t lgh_tp_graph_nodes(const lgh_tp* t) { return t ? t->graph_nodes : 0; }

const char* lgh_tp_last_error(const lgh_tp* t) { return t ? t->err.c_str() : g_create_err.c_str(); }

// The synchronisation-point kernel on its own.  `out`, `xq_image` and `ssq_parts` are in / out: the device buffers start from the
// host's bytes, so that a caller sees which bytes the kernel wrote; every device buffer also sits between two guard bands, and a
// changed guard byte is reported as OperationFailed.
int lgh_op_tp_reduce(int device, const float* partials, uint32_t n, const float* resid, const float* norm_w, size_t H, float* out, uint8_t* xq_image,
                     float* ssq_parts) {
  if (!partials || !out || n < 1 || n > (uint32_t)kTpMaxRanks || H == 0 || H % 16 || H > (1u << 30)) return LGH_INVALID_ARGUMENT;
  if (ssq_parts && !xq_image) return LGH_INVALID_ARGUMENT;
  const int nd = lgh_device_count();
  if (nd <= 0 || device < 0 || device >= nd) return LGH_NOT_AVAILABLE;
  if (hipSetDevice(device) != hipSuccess) return LGH_NOT_AVAILABLE;
  constexpr size_t kGuard = 256;
  constexpr uint8_t kPattern = 0xA5;
  std::vector<void*> allocs;
  std::vector<std::pair<uint8_t*, size_t>> guarded;   // (base, payload bytes)
  hipStream_t st = nullptr;
  auto cleanup = [&](int rc) {
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (void* p : allocs) (void)hipFree(p);
    return rc;
  };
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return LGH_INITIALIZATION_FAILED;
  auto up = [&](const void* host, size_t bytes) -> uint8_t* {   // payload rounded up to 256 bytes so that the next guard stays aligned
    const size_t padded = (bytes + 255) / 256 * 256;
    uint8_t* base = nullptr;
    if (hipMalloc((void**)&base, padded + 2 * kGuard) != hipSuccess) return nullptr;
    allocs.push_back(base);
    if (hipMemsetAsync(base, kPattern, padded + 2 * kGuard, st) != hipSuccess) return nullptr;
    if (host && hipMemcpyAsync(base + kGuard, host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
    guarded.push_back({base, bytes});
    return base + kGuard;
  };
  const float* parts[kTpMaxRanks] = {};
  for (uint32_t r = 0; r < n; r++) {
    parts[r] = (const float*)up(partials + (size_t)r * H, H * 4);
    if (!parts[r]) return cleanup(LGH_ALLOCATION_FAILED);
  }
  const float* d_res = resid ? (const float*)up(resid, H * 4) : nullptr;
  const float* d_nw = norm_w ? (const float*)up(norm_w, H * 4) : nullptr;
  float* d_out = (float*)up(out, H * 4);
  uint8_t* d_xq = xq_image ? up(xq_image, xq_bytes(H)) : nullptr;
  float* d_ssq = ssq_parts ? (float*)up(ssq_parts, H / 16 * 4) : nullptr;
  if ((resid && !d_res) || (norm_w && !d_nw) || !d_out || (xq_image && !d_xq) || (ssq_parts && !d_ssq)) return cleanup(LGH_ALLOCATION_FAILED);
  if (tp_reduce_launch(parts, n, d_res, d_nw, (uint32_t)H, d_out, d_xq, d_ssq, st) != hipSuccess) return cleanup(LGH_OPERATION_FAILED);
  bool ok = hipMemcpyAsync(out, d_out, H * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (d_xq) ok = ok && hipMemcpyAsync(xq_image, d_xq, xq_bytes(H), hipMemcpyDeviceToHost, st) == hipSuccess;
  if (d_ssq) ok = ok && hipMemcpyAsync(ssq_parts, d_ssq, H / 16 * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
  ok = ok && hipStreamSynchronize(st) == hipSuccess;
  std::vector<uint8_t> g;
  for (size_t i = 0; i < guarded.size() && ok; i++) {   // the bands in front of and behind every buffer (the payload's rounding included)
    const size_t bytes = guarded[i].second, total = (bytes + 255) / 256 * 256 + 2 * kGuard;
    g.resize(total);
    ok = hipMemcpy(g.data(), guarded[i].first, total, hipMemcpyDeviceToHost) == hipSuccess;
    for (size_t j = 0; j < total && ok; j++)
      if ((j < kGuard || j >= kGuard + bytes) && g[j] != kPattern) ok = false;
  }
  return cleanup(ok ? LGH_OK : LGH_OPERATION_FAILED);
}

}  // extern "C"
