// ops_api.hip — the per-op C entry points (host tensors in / host tensors out) that mirror the
// reference's `Backend` trait ops on the decode path (src/backend/mod.rs:29-265), plus the kernel
// micro-benchmark.  They run the SAME kernels the engine runs, on a throw-away context, so that each
// kernel can be checked against the CPU backend in isolation.
#include "engine.h"
#include "xq.h"
#include "prefill.h"

#include <cmath>
#include <vector>

using namespace lgh;

#include <algorithm>

#ifdef LGH_STAMPS
namespace lgh { hipError_t pf_read_stamps(unsigned long long* host, size_t n); }
extern "C" int lgh_debug_pf_stamps(unsigned long long* out, size_t n) { return lgh::pf_read_stamps(out, n) == hipSuccess ? 0 : 10; }
namespace lgh { hipError_t mv_read_stamps(unsigned long long* host, size_t n); hipError_t mvq_read_stamps(unsigned long long* host, size_t n); hipError_t mvq_read_wave_stamps(unsigned long long* host, size_t n); hipError_t mvq_spans(unsigned long long* host, int reset); }
#include <cstdio>
#include "timeline.h"
namespace lgh { hipError_t tl_read_mvq(void*); hipError_t tl_read_attn(void*); hipError_t tl_read_deq(void*); hipError_t tl_read_misc(void*); }
// the per-node timeline buffers of the four translation units on the decode path (timeline.h), `which` = 0..3;
// out: sizeof(TlBuf) bytes.  Returns the buffer size when out == nullptr.
extern "C" long long lgh_debug_timeline(int which, void* out) {
  if (!out) return (long long)sizeof(lgh::TlBuf);
  hipError_t e = which == 0 ? lgh::tl_read_mvq(out) : which == 1 ? lgh::tl_read_attn(out) : which == 2 ? lgh::tl_read_deq(out) : lgh::tl_read_misc(out);
  return e == hipSuccess ? 0 : -1;
}
#endif

namespace {

uint32_t g_op_flags = 0;   // lgh_op_set_flags: the LGH_FLAG_* bits of the bare contexts the lgh_op_* / lgh_bench_* entry points run on

struct Tmp {  // bare context: stream, device state words, tracked allocations
  lgh_ctx* c = nullptr;
  int rc = LGH_OK;
  explicit Tmp(int device) {
    int n = lgh_device_count();
    if (n <= 0 || device < 0 || device >= n) { rc = LGH_NOT_AVAILABLE; return; }
    c = new lgh_ctx();
    c->device = device;
    c->d.norm_eps = 1e-5f;
    c->d.flags = g_op_flags;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
      rc = LGH_INITIALIZATION_FAILED;
      delete c;
      c = nullptr;
      return;
    }
    c->stream = c->own_stream;
    if ((rc = dev_alloc(c, (void**)&c->state, ST_WORDS * 4))) return;
    (void)hipMemsetAsync(c->state, 0, ST_WORDS * 4, c->stream);
  }
  ~Tmp() {
    if (!c) return;
    (void)hipStreamSynchronize(c->stream);
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->batch.h_ctl) (void)hipHostFree(c->batch.h_ctl);   // (the multi-sequence entry points: batch_scratch_alloc's pinned words)
    (void)hipStreamDestroy(c->own_stream);
    delete c;
  }
  float* up(const float* host, size_t n) {  // device copy of a host f32 vector (nullptr on failure)
    float* d = nullptr;
    if (dev_alloc(c, (void**)&d, n * 4)) return nullptr;
    if (host && hipMemcpyAsync(d, host, n * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return nullptr;
    return d;
  }
  int down(float* host, const float* dev, size_t n) {
    if (hipMemcpyAsync(host, dev, n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
    return hipStreamSynchronize(c->stream) == hipSuccess ? LGH_OK : LGH_OPERATION_FAILED;
  }
};

bool signs_ok(const float* signs, size_t n) {   // rotation signs: +1 or -1
  for (size_t i = 0; i < n; i++)
    if (signs[i] != 1.0f && signs[i] != -1.0f) return false;
  return true;
}

}  // namespace

extern "C" {

int lgh_op_dequantize(int device, uint32_t type, const void* src, size_t n, float* dst) {
  Tmp t(device);
  if (t.rc) return t.rc;
  const uint32_t be = blk_elems((int)type);
  if (!be || n % be) return LGH_UNSUPPORTED_DTYPE;
  const size_t nbytes = n / be * blk_bytes((int)type);
  uint8_t* raw = nullptr;
  float* out = nullptr;
  if (dev_alloc(t.c, (void**)&raw, nbytes) || dev_alloc(t.c, (void**)&out, n * 4)) return LGH_ALLOCATION_FAILED;
  if (hipMemcpyAsync(raw, src, nbytes, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if (dequant_launch((int)type, raw, out, n, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return t.down(dst, out, n);
}

static int vec_mat_impl(int device, uint32_t type, const void* w, const void* w2, const float* x, const float* norm_w,
                        float eps, const float* resid, float* out, size_t k, size_t n) {
  Tmp t(device);
  if (t.rc) return t.rc;
  t.c->d.norm_eps = eps;
  const uint32_t be = blk_elems((int)type);
  if (!be || k % be) return LGH_SHAPE_MISMATCH;
  const size_t nbytes = n * (k / be) * blk_bytes((int)type);
  DevWeight W, W2;
  int rc;
  if ((rc = upload_matrix(t.c, W, (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w, nbytes))) return rc;
  if (w2 && (rc = upload_matrix(t.c, W2, (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w2, nbytes))) return rc;
  float* dx = t.up(x, k);
  float* dnw = norm_w ? t.up(norm_w, k) : nullptr;
  float* dres = resid ? t.up(resid, n) : nullptr;
  float* dout = t.up(nullptr, n);
  if (!dx || !dout || (norm_w && !dnw) || (resid && !dres)) return LGH_ALLOCATION_FAILED;
  if (w2) {
    if (!fused_type(W.type)) return LGH_UNSUPPORTED;
    SegSpec sp;
    sp.npass = 2;
    sp.W[0] = &W; sp.W[1] = &W2;
    sp.x[0] = sp.x[1] = dx;
    sp.epi = EPI_SWIGLU;
    sp.out = dout;
    if ((rc = launch_mv(t.c, LGH_K_GATEUP, &sp, 1, dnw, (uint32_t)k))) return rc;
  } else if ((rc = linear_any(t.c, LGH_K_MISC, W, dx, dout, dnw, dres, nullptr))) {
    return rc;
  }
  return t.down(out, dout, n);
}

int lgh_op_vec_mat(int device, uint32_t type, const void* w, const float* x, float* out, size_t k, size_t n) {
  return vec_mat_impl(device, type, w, nullptr, x, nullptr, 1e-5f, nullptr, out, k, n);
}

int lgh_op_norm_vec_mat(int device, uint32_t type, const void* w, const float* x, const float* norm_w, float eps, float* out,
                        size_t k, size_t n) {
  return vec_mat_impl(device, type, w, nullptr, x, norm_w, eps, nullptr, out, k, n);
}

int lgh_op_swiglu_vec_mat(int device, uint32_t type, const void* w_gate, const void* w_up, const float* x,
                          const float* norm_w, float eps, float* out, size_t k, size_t n) {
  return vec_mat_impl(device, type, w_gate, w_up, x, norm_w, eps, nullptr, out, k, n);
}

// out[m][n] = x[m][k] . W^T on the batched-prefill GEMM path (prefill.hip): f16 operands, f32 accumulation
int lgh_op_mat_mat(int device, uint32_t type, const void* w, const float* x, float* out, size_t k, size_t n, size_t m) {
  Tmp t(device);
  if (t.rc) return t.rc;
  const uint32_t be = blk_elems((int)type);
  if (!be || k % be || m == 0 || m > (size_t)kPfTokens) return LGH_SHAPE_MISMATCH;
  const size_t nbytes = n * (k / be) * blk_bytes((int)type);
  DevWeight W;
  int rc;
  if ((rc = upload_matrix(t.c, W, (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w, nbytes))) return rc;
  if (!pf_supported_type(W.type) || n % 16) return LGH_UNSUPPORTED;
  const uint32_t nr[1] = {(uint32_t)n};
  const size_t pb = pf_part_bytes(nr, 1, (uint32_t)k);
  float* dx = t.up(x, m * k);
  float* dout = t.up(nullptr, (size_t)kPfTokens * n);
  uint8_t* xh = nullptr;
  float *part = nullptr, *ssq = nullptr;
  if (!dx || !dout || dev_alloc(t.c, (void**)&xh, xh_bytes((uint32_t)k)) || dev_alloc(t.c, (void**)&part, pb) ||
      dev_alloc(t.c, (void**)&ssq, (size_t)kPfTokens * kPfSsqChunks * 4))
    return LGH_ALLOCATION_FAILED;
  hipStream_t st = t.c->stream;
  if (hipMemsetAsync(dout, 0, (size_t)kPfTokens * n * 4, st) != hipSuccess || hipMemsetAsync(xh, 0, xh_bytes((uint32_t)k), st) != hipSuccess)
    return LGH_OPERATION_FAILED;
  const DevWeight* Ws[1] = {&W};
  uint32_t S = 0, nc = 0;
  if (pf_to_xh_launch(dx, (uint32_t)k, xh, (uint32_t)m, st) != hipSuccess) return LGH_OPERATION_FAILED;
  if (pf_gemm_launch(Ws, 1, xh, part, pb, (uint32_t)m, &S, &nc, st) != hipSuccess) return LGH_OPERATION_FAILED;
  // (no sums of squares for rows wider than the epilogue keeps them for: the GEMM's plan, not the norm, is what such a shape is for)
  if (pf_row_epi_launch(part, S, nc, 0, nullptr, dout, (uint32_t)n, nullptr, nullptr, n > 2048u * kPfSsqChunks ? nullptr : ssq, (uint32_t)m, st) != hipSuccess)
    return LGH_OPERATION_FAILED;
  return t.down(out, dout, m * n);
}

int lgh_op_rms_norm(int device, const float* x, const float* w, float eps, float* out, size_t n) {
  Tmp t(device);
  if (t.rc) return t.rc;
  float *dx = t.up(x, n), *dw = t.up(w, n), *dout = t.up(nullptr, n);
  if (!dx || !dw || !dout) return LGH_ALLOCATION_FAILED;
  if (rms_norm_launch(dx, dw, eps, dout, (uint32_t)n, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return t.down(out, dout, n);
}

int lgh_op_rope(int device, float* q, float* k, size_t n_heads, size_t n_kv, size_t d, size_t pos, float freq_base,
                float freq_scale, int neox) {
  Tmp t(device);
  if (t.rc) return t.rc;
  const size_t half = d / 2;
  std::vector<float> cs(half * 2);  // table row for `pos`, reference arithmetic (ops.rs:1300-1313)
  const float position = (float)pos / freq_scale;
  for (size_t i = 0; i < half; i++) {
    const float freq = 1.0f / std::pow(freq_base, (float)(2 * i) / (float)d);
    const float theta = position * freq;
    cs[2 * i] = std::cos(theta);
    cs[2 * i + 1] = std::sin(theta);
  }
  float *dq = t.up(q, n_heads * d), *dk = t.up(k, n_kv * d), *dcs = t.up(cs.data(), cs.size());
  if (!dq || !dk || !dcs) return LGH_ALLOCATION_FAILED;
  // state[ST_POS] stays 0: the one-row table is indexed at position 0
  if (rope_launch(dq, dk, (uint32_t)n_heads, (uint32_t)n_kv, (uint32_t)d, t.c->state + ST_POS, dcs, neox, t.c->stream) != hipSuccess)
    return LGH_OPERATION_FAILED;
  int rc = t.down(q, dq, n_heads * d);
  if (rc) return rc;
  return t.down(k, dk, n_kv * d);
}

// Split + merge over an f32 cache of max_seq rows per kv head with the first kv_len of them attended to, the length given by the host
// (no position word): the statuses lgh_op_attention_cached and lgh_op_attention always answered — a refused partial launch Unsupported, a
// refused merge (in particular more than 32 splits, which only the merge used to refuse) OperationFailed
static int attn_fixed_len(hipStream_t st, const float* q, float* kc, float* vc, size_t n_heads, size_t n_kv, size_t d, size_t max_seq, float scale,
                          size_t kv_len, int n_splits, float* pml, float* pacc, float* out) {
  if (n_splits > 32) return LGH_OPERATION_FAILED;
  const KvLayout l(LGH_KV_F32, n_kv, max_seq, d);
  KvCache kv;
  kv.t[KV_K] = kc; kv.t[KV_V] = vc;
  AttnDecode a{};
  a.n_heads = (uint32_t)n_heads; a.scale = scale;
  a.q = q; a.kv_len_fixed = (int)kv_len;
  a.n_splits = (uint32_t)n_splits; a.part_ml = pml; a.part_acc = pacc;
  a.out = out;
  a.st = st;
  if (attn_split_launch(l, kv, a) != hipSuccess) return LGH_UNSUPPORTED;
  return attn_merge_launch(l, a) == hipSuccess ? LGH_OK : LGH_OPERATION_FAILED;
}

int lgh_op_attention_cached(int device, const float* q, const float* kc, const float* vc, float* out, size_t n_heads,
                            size_t n_kv, size_t d, size_t max_seq, float scale, size_t kv_len, int n_splits) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (kv_len == 0 || kv_len > max_seq || n_kv == 0 || n_heads % n_kv) return LGH_INVALID_ARGUMENT;
  if (n_splits <= 0) n_splits = 8;
  const size_t g = n_heads / n_kv, cache = n_kv * max_seq * d;
  float *dq = t.up(q, n_heads * d), *dk = t.up(kc, cache), *dv = t.up(vc, cache), *dout = t.up(nullptr, n_heads * d);
  float *pml = t.up(nullptr, n_kv * n_splits * g * 2), *pacc = t.up(nullptr, n_kv * n_splits * g * d);
  if (!dq || !dk || !dv || !dout || !pml || !pacc) return LGH_ALLOCATION_FAILED;
  if (!((d == 64 || d == 128) && (g == 1 || g == 2 || g == 4 || g == 8))) {   // shapes outside the engine's kernels
    if (attn_generic_launch(dq, dk, dv, dout, (uint32_t)n_heads, (uint32_t)n_kv, 1, (uint32_t)kv_len, (uint32_t)max_seq, (uint32_t)d, scale,
                            t.c->stream) != hipSuccess)
      return LGH_UNSUPPORTED;
    return t.down(out, dout, n_heads * d);
  }
  if (int rc = attn_fixed_len(t.c->stream, dq, dk, dv, n_heads, n_kv, d, max_seq, scale, kv_len, n_splits, pml, pacc, dout)) return rc;
  return t.down(out, dout, n_heads * d);
}

int lgh_op_silu_mul(int device, const float* gate, const float* up, float* out, size_t n) {
  Tmp t(device);
  if (t.rc) return t.rc;
  float *dg = t.up(gate, n), *du = t.up(up, n), *dout = t.up(nullptr, n);
  if (!dg || !du || !dout) return LGH_ALLOCATION_FAILED;
  if (silu_mul_launch(dg, du, dout, (uint32_t)n, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return t.down(out, dout, n);
}

// ---- Sampler::sample (sampling/mod.rs:188-304) through the kernels of lgh_decode_sample ----
int lgh_op_sample_ex(int device, const float* logits, size_t vocab, const lgh_sampler_config_ex* config, const uint32_t* recent,
                     size_t n_recent, const uint32_t* counts, float uniform, float mu_in, uint32_t* token_out, float* mu_out) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!logits || !token_out || vocab == 0 || vocab > 0x7FFFFFFFu || (n_recent && !recent)) return LGH_INVALID_ARGUMENT;
  int rc = samp_check_ex(t.c, config);
  if (rc) return rc;
  if (config->mirostat && !(mu_in >= 0.0f && mu_in <= 20.0f)) return LGH_INVALID_ARGUMENT;   // what the reference's clamp keeps mu in
  t.c->d.vocab_size = (uint32_t)vocab;
  t.c->d.max_seq_len = 1;
  SampBufs B;
  if ((rc = samp_alloc(t.c, B, 1, 1))) return rc;
  const float* dl = t.up(logits, vocab);
  if (!dl) return LGH_ALLOCATION_FAILED;
  return samp_one(t.c, B, *config, recent, n_recent, counts, uniform, mu_in, dl, token_out, mu_out);
}

int lgh_op_sample(int device, const float* logits, size_t vocab, const lgh_sampler_config* config, const uint32_t* recent, size_t n_recent,
                  const uint32_t* counts, float uniform, uint32_t* token_out) {
  if (!config) return LGH_INVALID_ARGUMENT;
  const lgh_sampler_config_ex x = samp_plain(*config);
  return lgh_op_sample_ex(device, logits, vocab, &x, recent, n_recent, counts, uniform, 0.0f, token_out, nullptr);
}

// ---- Backend::add / mul / scale / silu / gelu / softmax / matmul / matvec / matvec_q / attention (backend/mod.rs:29-265) ----
static int ewise_impl(int device, int op, const float* a, const float* b, float s, float* out, size_t n) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (n == 0) return LGH_OK;
  if (!a || !out || ((op == 0 || op == 1) && !b)) return LGH_INVALID_ARGUMENT;
  float *da = t.up(a, n), *db = b ? t.up(b, n) : nullptr, *dout = t.up(nullptr, n);
  if (!da || !dout || (b && !db)) return LGH_ALLOCATION_FAILED;
  if (ewise_launch(op, da, db, s, dout, n, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return t.down(out, dout, n);
}
int lgh_op_add(int device, const float* a, const float* b, float* out, size_t n) { return ewise_impl(device, 0, a, b, 0.0f, out, n); }
int lgh_op_mul(int device, const float* a, const float* b, float* out, size_t n) { return ewise_impl(device, 1, a, b, 0.0f, out, n); }
int lgh_op_scale(int device, const float* a, float scalar, float* out, size_t n) { return ewise_impl(device, 2, a, nullptr, scalar, out, n); }
int lgh_op_silu(int device, const float* x, float* out, size_t n) { return ewise_impl(device, 3, x, nullptr, 0.0f, out, n); }
int lgh_op_gelu(int device, const float* x, float* out, size_t n) { return ewise_impl(device, 4, x, nullptr, 0.0f, out, n); }

int lgh_op_softmax(int device, const float* x, float* out, size_t rows, size_t last_dim) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (rows * last_dim == 0) return LGH_OK;
  if (!x || !out || rows > 0x7FFFFFFFu || last_dim > 0xFFFFFFFFu) return LGH_INVALID_ARGUMENT;
  float *dx = t.up(x, rows * last_dim), *dout = t.up(nullptr, rows * last_dim);
  if (!dx || !dout) return LGH_ALLOCATION_FAILED;
  if (softmax_rows_launch(dx, dout, (uint32_t)rows, (uint32_t)last_dim, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return t.down(out, dout, rows * last_dim);
}

int lgh_op_kv_roundtrip(int device, uint32_t kv_cache_type, const float* row, size_t n, uint8_t* bytes_out, float* scale_out, float* back_out) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (kv_cache_type < LGH_KV_INT8 || kv_cache_type > LGH_KV_FP8_E5M2) return LGH_UNSUPPORTED;
  if (n == 0) return LGH_OK;
  if (!row || !bytes_out || !back_out || n > 0x7FFFFFFFu) return LGH_INVALID_ARGUMENT;
  float *dx = t.up(row, n), *dback = t.up(nullptr, n), *dsc = t.up(nullptr, 1);
  uint8_t* db = reinterpret_cast<uint8_t*>(t.up(nullptr, (n + 3) / 4));
  if (!dx || !dback || !dsc || !db) return LGH_ALLOCATION_FAILED;
  if (kv_roundtrip_launch((int)kv_cache_type, dx, (uint32_t)n, db, dsc, dback, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  std::vector<float> tmp((n + 3) / 4);
  int rc = t.down(tmp.data(), reinterpret_cast<float*>(db), (n + 3) / 4);
  if (rc) return rc;
  std::memcpy(bytes_out, tmp.data(), n);
  float sc = 1.0f;
  if (kv_cache_type == LGH_KV_INT8 && (rc = t.down(&sc, dsc, 1))) return rc;
  if (scale_out) *scale_out = sc;
  return t.down(back_out, dback, n);
}

// One row through TurboQuantMSE::compress; qjl: also the QJL sign bits and the residual norm of TurboQuantProd
static int tq_compress_op(int device, int bits, const float* x, size_t dim, const float* signs, bool qjl, const float* qjl_matrix, uint8_t* codes,
                          uint64_t* qjl_bits, float* residual_norm) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!x || !signs || !codes || (qjl && (!qjl_matrix || !qjl_bits || !residual_norm))) return LGH_INVALID_ARGUMENT;
  if ((bits != 2 && bits != 3) || (dim != 64 && dim != 128)) return LGH_UNSUPPORTED;
  if (!signs_ok(signs, dim)) return LGH_INVALID_ARGUMENT;
  float *dx = t.up(x, dim), *ds = t.up(signs, dim), *dS = qjl ? t.up(qjl_matrix, dim * dim) : nullptr;
  const size_t rb = tq_row_bytes_host(bits, (uint32_t)dim), xw = dim / 32 + 1;
  uint8_t* dc = reinterpret_cast<uint8_t*>(t.up(nullptr, (rb + 3) / 4));
  uint32_t* dq = qjl ? reinterpret_cast<uint32_t*>(t.up(nullptr, xw)) : nullptr;
  if (!dx || !ds || !dc || (qjl && (!dS || !dq))) return LGH_ALLOCATION_FAILED;
  if (tq_compress_launch(bits, dx, (uint32_t)dim, ds, dc, t.c->stream, dS, dq) != hipSuccess) return LGH_OPERATION_FAILED;
  std::vector<float> tmp((rb + 3) / 4), tq(xw);
  int rc = t.down(tmp.data(), reinterpret_cast<float*>(dc), (rb + 3) / 4);
  if (rc) return rc;
  std::memcpy(codes, tmp.data(), rb);
  if (!qjl) return LGH_OK;
  if ((rc = t.down(tq.data(), reinterpret_cast<float*>(dq), xw))) return rc;
  uint32_t w[8] = {};
  std::memcpy(w, tq.data(), xw * 4);
  for (size_t i = 0; i < dim / 64; i++) qjl_bits[i] = (uint64_t)w[2 * i] | (uint64_t)w[2 * i + 1] << 32;
  std::memcpy(residual_norm, &w[dim / 32], 4);
  return LGH_OK;
}

int lgh_op_tq_compress(int device, int bits, const float* x, size_t dim, const float* signs, uint8_t* codes) {
  return tq_compress_op(device, bits, x, dim, signs, false, nullptr, codes, nullptr, nullptr);
}

int lgh_op_tq_compress_qjl(int device, int bits, const float* x, size_t dim, const float* signs, const float* qjl_matrix, uint8_t* codes,
                           uint64_t* qjl_bits, float* residual_norm) {
  return tq_compress_op(device, bits, x, dim, signs, true, qjl_matrix, codes, qjl_bits, residual_norm);
}

int lgh_op_matmul(int device, const float* a, const float* b, float* out, size_t m, size_t k, size_t n) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!a || !b || !out || m == 0 || n == 0 || m > 65535) return LGH_INVALID_ARGUMENT;
  float *da = t.up(a, m * k), *db = t.up(b, k * n), *dout = t.up(nullptr, m * n);
  if (!da || !db || !dout) return LGH_ALLOCATION_FAILED;
  if (matmul_f32_launch(da, db, dout, (uint32_t)m, (uint32_t)k, (uint32_t)n, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return t.down(out, dout, m * n);
}

int lgh_op_matvec(int device, const float* a, const float* x, float* out, size_t m, size_t k) {
  // [m,k] row-major times [k]: the memory layout of vec_mat's GGUF-order weight with n = m (ops.rs:531-570 vs 959-1002)
  return vec_mat_impl(device, LGH_TYPE_F32, a, nullptr, x, nullptr, 1e-5f, nullptr, out, k, m);
}

int lgh_op_matvec_q(int device, uint32_t type, const void* a, const float* x, float* out, size_t m, size_t k) {
  // quantized rows of k elements, m of them: the same bytes vec_mat_q reads (ops.rs:922-950 vs 1008-1039)
  return vec_mat_impl(device, type, a, nullptr, x, nullptr, 1e-5f, nullptr, out, k, m);
}

int lgh_op_attention(int device, const float* q, const float* k, const float* v, float* out, size_t n_heads, size_t n_kv, size_t seq_len,
                     size_t kv_len, size_t d, float scale) {
  // q / out [heads, seq, d], k / v [kv_heads, kv_len, d]; query s sits at position kv_len - seq_len + s and sees the
  // rows up to itself (ops.rs:1353-1472).  One split-attention pass per query position over the SAME kernels the engine
  // runs: k / v are a cache with max_seq = kv_len.
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!q || !k || !v || !out || n_kv == 0 || n_heads % n_kv || seq_len == 0 || kv_len == 0) return LGH_INVALID_ARGUMENT;
  const size_t g = n_heads / n_kv, cache = n_kv * kv_len * d;
  const int n_splits = 8;
  float *dq = t.up(q, n_heads * seq_len * d), *dk = t.up(k, cache), *dv = t.up(v, cache), *dout = t.up(nullptr, n_heads * seq_len * d);
  float *qs = t.up(nullptr, n_heads * d), *os = t.up(nullptr, n_heads * d);
  float *pml = t.up(nullptr, n_kv * n_splits * g * 2), *pacc = t.up(nullptr, n_kv * n_splits * g * d);
  if (!dq || !dk || !dv || !dout || !qs || !os || !pml || !pacc) return LGH_ALLOCATION_FAILED;
  hipStream_t st = t.c->stream;
  const bool fast = (d == 64 || d == 128) && (g == 1 || g == 2 || g == 4 || g == 8);
  if (!fast) {   // shapes outside the engine's kernels: the generic kernel
    if (attn_generic_launch(dq, dk, dv, dout, (uint32_t)n_heads, (uint32_t)n_kv, (uint32_t)seq_len, (uint32_t)kv_len, (uint32_t)kv_len, (uint32_t)d, scale, st) != hipSuccess)
      return LGH_UNSUPPORTED;
    return t.down(out, dout, n_heads * seq_len * d);
  }
  for (size_t s = 0; s < seq_len; s++) {
    const size_t q_abs = (kv_len >= seq_len ? kv_len - seq_len : 0) + s;   // saturating_sub (ops.rs:1411)
    const size_t visible = q_abs + 1 < kv_len ? q_abs + 1 : kv_len;
    if (hipMemcpy2DAsync(qs, d * 4, dq + s * d, seq_len * d * 4, d * 4, n_heads, hipMemcpyDeviceToDevice, st) != hipSuccess) return LGH_OPERATION_FAILED;
    if (int rc = attn_fixed_len(st, qs, dk, dv, n_heads, n_kv, d, kv_len, scale, visible, n_splits, pml, pacc, os)) return rc;
    if (hipMemcpy2DAsync(dout + s * d, seq_len * d * 4, os, d * 4, d * 4, n_heads, hipMemcpyDeviceToDevice, st) != hipSuccess) return LGH_OPERATION_FAILED;
  }
  return t.down(out, dout, n_heads * seq_len * d);
}

// ---- the engine's attention step (engine_layer.hip: attention_forward) one path at a time (test surface: tests/test_gpu_attention.py
// holds each to a float64 restatement).  The bare context's fields select the path as a real context's do; the caches come from the
// host, the position through the device word the engine's kernels read (state[ST_POS]); nothing falls back to another kernel: a
// shape the path has no kernel for answers LGH_UNSUPPORTED.  The *_multi entry points do the same with the multi-sequence step's
// attention (engine_layer.hip: attention_forward_multi) on the batch scratch of a bare context (attn_multi_setup). ----
}  // extern "C"

namespace {

void* up_bytes(Tmp& t, const void* host, size_t n) {   // device copy of n host bytes (nullptr on failure)
  void* d = nullptr;
  if (dev_alloc(t.c, &d, n ? n : 4)) return nullptr;
  if (host && n && hipMemcpyAsync(d, host, n, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return nullptr;
  return d;
}

int down_bytes(Tmp& t, void* host, const void* dev, size_t n) {
  if (n && hipMemcpyAsync(host, dev, n, hipMemcpyDeviceToHost, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return hipStreamSynchronize(t.c->stream) == hipSuccess ? LGH_OK : LGH_OPERATION_FAILED;
}

int set_pos(Tmp& t, size_t pos) {   // the engine's position word
  const int p = (int)pos;
  t.c->pos = pos;
  if (hipMemcpyAsync(t.c->state + ST_POS, &p, 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return hipStreamSynchronize(t.c->stream) == hipSuccess ? LGH_OK : LGH_OPERATION_FAILED;
}

// the bare context as attention_forward reads it: shapes, the cache format, the split count and its partial-result buffers (of n_seq
// sequences)
int attn_setup(Tmp& t, uint32_t kv_cache_type, size_t n_heads, size_t n_kv, size_t head_dim, size_t max_seq, int n_splits, size_t n_seq = 1) {
  lgh_ctx* c = t.c;
  c->d.num_heads = (uint32_t)n_heads;
  c->d.num_kv_heads = (uint32_t)n_kv;
  c->d.head_dim = (uint32_t)head_dim;
  c->d.max_seq_len = (uint32_t)max_seq;
  c->d.kv_cache_type = kv_cache_type;
  c->kvl = KvLayout(c->d);
  c->n_splits = (uint32_t)n_splits;
  const size_t parts = n_seq * n_kv * (size_t)n_splits * (n_heads / n_kv);
  if (!parts) return LGH_OK;   // (a one-launch path: no partial results)
  c->part_ml = t.up(nullptr, parts * 2);
  c->part_acc = t.up(nullptr, parts * head_dim);
  return c->part_ml && c->part_acc ? LGH_OK : LGH_ALLOCATION_FAILED;
}

// a step's control words in the batch scratch: positions and cache slots of its sequences (nullptr: position 0, slot = sequence)
int mb_control(Tmp& t, const int* pos, const int* slot, size_t n_seq) {
  int p[kMaxBatch] = {}, sl[kMaxBatch];
  for (size_t i = 0; i < (size_t)kMaxBatch; i++) { sl[i] = (int)i; if (i < n_seq && pos) p[i] = pos[i]; if (i < n_seq && slot) sl[i] = slot[i]; }
  const BatchScratch& Bs = t.c->batch;
  if (hipMemcpyAsync(Bs.d_pos, p, sizeof(p), hipMemcpyHostToDevice, t.c->stream) != hipSuccess ||
      hipMemcpyAsync(Bs.d_slot, sl, sizeof(sl), hipMemcpyHostToDevice, t.c->stream) != hipSuccess)
    return LGH_OPERATION_FAILED;
  return hipStreamSynchronize(t.c->stream) == hipSuccess ? LGH_OK : LGH_OPERATION_FAILED;
}

// what the multi-sequence entry points ask of their sequences (engine.h: check_seqs), positions and slots as the caller's ints
bool seqs_ok(size_t n_seq, size_t max_n, const int* slot, size_t n_slots, bool distinct, const int* pos, size_t max_seq) {
  return check_seqs(n_seq, max_n, slot, n_slots, distinct, [&](size_t i) { return (uint64_t)(int64_t)pos[i]; }, max_seq) == SEQ_OK;
}

// the step's K row | V row per sequence, side by side as the engine's kv_tmp holds them, from k_new / v_new [n_seq][kd]
float* up_kv_new(Tmp& t, const float* k_new, const float* v_new, size_t kd, size_t n_seq = 1) {
  float* d = t.up(nullptr, n_seq * 2 * kd);
  for (size_t s = 0; d && s < n_seq; s++)
    if (hipMemcpyAsync(d + s * 2 * kd, k_new + s * kd, kd * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess ||
        hipMemcpyAsync(d + s * 2 * kd + kd, v_new + s * kd, kd * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess)
      return nullptr;
  return d;
}

// the bare context as attention_forward_multi reads it, for one layer (0) of cache slots: attn_setup's fields, and of the batch scratch
// the sequences' queries, staged rows ([sequence][K row | V row]; k_new: staged formats only) and outputs, the partial results and the
// control words.  The caller puts its caches into the layer's entry (Bs.kv[0])
int attn_multi_setup(Tmp& t, uint32_t kv_cache_type, const float* q, const float* k_new, const float* v_new, size_t n_heads, size_t n_kv,
                     size_t head_dim, size_t max_seq, size_t n_seq, const int* pos, const int* slot, int n_splits) {
  lgh_ctx* c = t.c;
  BatchScratch& Bs = c->batch;
  if (int rc = attn_setup(t, kv_cache_type, n_heads, n_kv, head_dim, max_seq, n_splits, n_seq)) return rc;
  c->d.num_layers = 1;
  Bs.kv.assign(1, KvCache{});
  const size_t QD = n_heads * head_dim, KD = n_kv * head_dim;
  Bs.part_ml = c->part_ml;
  Bs.part_acc = c->part_acc;
  Bs.q = t.up(q, n_seq * QD);
  Bs.attn_out = t.up(nullptr, n_seq * QD);
  Bs.kv_tmp = k_new ? up_kv_new(t, k_new, v_new, KD, n_seq) : nullptr;
  Bs.d_pos = (int*)up_bytes(t, nullptr, kMaxBatch * 4);
  Bs.d_slot = (int*)up_bytes(t, nullptr, kMaxBatch * 4);
  if (!Bs.q || !Bs.attn_out || (k_new && !Bs.kv_tmp) || !Bs.d_pos || !Bs.d_slot) return LGH_ALLOCATION_FAILED;
  return mb_control(t, pos, slot, n_seq);
}

// A cache's tensors for n_slots slots of one layer, between the caller's host arrays (in KvKind order) and the device.  Up: every
// tensor the format has.  An f32 cache gets kAttnSlackRows rows of NaN behind its last head: a decode attention kernel whose row
// clamp is off by up to a first batch of rows (32 splits x 8 waves x 4 rows) reads those, not whatever follows the allocation
constexpr size_t kAttnSlackRows = 1024;
int kv_upload(Tmp& t, const KvLayout& l, size_t n_slots, const void* const* host, KvCache& kv) {
  const size_t slack = l.f32() ? kAttnSlackRows * l.row_bytes() : 0;
  for (int kind = 0; kind < KV_KINDS; kind++) {
    const size_t n = n_slots * l.slot_bytes(kind);
    if (!n) continue;
    if (dev_alloc(t.c, &kv.t[kind], n + slack)) return LGH_ALLOCATION_FAILED;
    if (hipMemcpyAsync(kv.t[kind], host[kind], n, hipMemcpyHostToDevice, t.c->stream) != hipSuccess ||
        (slack && hipMemsetAsync((uint8_t*)kv.t[kind] + n, 0xFF, slack, t.c->stream) != hipSuccess))
      return LGH_OPERATION_FAILED;
  }
  return LGH_OK;
}

// ... and down: every tensor the format has and the caller gave an array for
int kv_download(Tmp& t, const KvLayout& l, size_t n_slots, void* const* host, const KvCache& kv) {
  for (int kind = 0; kind < KV_KINDS; kind++)
    if (host[kind] && l.pos_bytes(kind))
      if (int rc = down_bytes(t, host[kind], kv.t[kind], n_slots * l.slot_bytes(kind))) return rc;
  return LGH_OK;
}

// wo's input as the merge leaves it (xq.h), when an attention entry point is asked for it.  One sequence: attention_forward registered
// the image of attn_out through xq_get; its xq_bytes(qd) bytes come back
int attn_image_down(Tmp& t, const float* attn_out, size_t qd, uint8_t* image_out) {
  const XqBuf* qa = xq_find(t.c, attn_out);
  if (!qa || !qa->fresh) return LGH_OPERATION_FAILED;
  return down_bytes(t, image_out, qa->xq, xq_bytes(qd));
}

// Several sequences: views of Bs.attn_out for n_seq + 1 sequences at the step's stride, as batch_scratch_alloc registers them for
// max_batch, every byte the scratch poison 0x7FC0BEEF: the view behind the last sequence must come back untouched
int attn_multi_images(Tmp& t, size_t n_seq, size_t qd) {
  const size_t n = n_seq + 1, xb = n * xq_stride_of((uint32_t)qd), sf = n * ssq_stride_of((uint32_t)qd);
  uint8_t* xq = (uint8_t*)up_bytes(t, nullptr, xb);
  float* ssq = t.up(nullptr, sf);
  if (!xq || !ssq) return LGH_ALLOCATION_FAILED;
  if (hipMemsetD32Async((hipDeviceptr_t)xq, (int)0x7FC0BEEFu, xb / 4, t.c->stream) != hipSuccess ||
      hipMemsetD32Async((hipDeviceptr_t)ssq, (int)0x7FC0BEEFu, sf, t.c->stream) != hipSuccess)
    return LGH_OPERATION_FAILED;
  return register_views(t.c, t.c->batch.attn_out, xq, ssq, (uint32_t)qd, (uint32_t)n);
}

int attn_multi_images_down(Tmp& t, size_t n_seq, size_t qd, uint8_t* image_out) {
  const XqBuf* qa = xq_find(t.c, t.c->batch.attn_out);
  if (!qa || !qa->fresh) return LGH_OPERATION_FAILED;
  return down_bytes(t, image_out, qa->xq, (n_seq + 1) * xq_stride_of((uint32_t)qd));
}

// The single-sequence step on the context attn_setup has shaped: the cache from the caller's arrays, attention_forward over it; back
// come the output, wo's input where asked for and (down: its arrays) the cache with the row the launch stored
int attn_run(Tmp& t, const AttnView& v, const void* const* up, void* const* down, float scale, float* out, uint8_t* image_out) {
  const size_t qd = (size_t)t.c->d.num_heads * t.c->d.head_dim;
  LayerW Lw;   // (the one layer of a context that owns layer 0: its signs and matrices are the context's first)
  int rc;
  if ((rc = kv_upload(t, t.c->kvl, 1, up, Lw.kv))) return rc;
  if (attention_forward(t.c, Lw, 0, v, scale, image_out != nullptr)) return LGH_OPERATION_FAILED;   // (a failed launch, as these entry points always answered)
  if (image_out && (rc = attn_image_down(t, v.attn_out, qd, image_out))) return rc;
  if (down && (rc = kv_download(t, t.c->kvl, 1, down, Lw.kv))) return rc;
  return t.down(out, v.attn_out, qd);
}

// ... and the multi-sequence step on the context attn_multi_setup has shaped, over n_slots slots
int attn_multi_run(Tmp& t, size_t n_slots, size_t n_seq, const void* const* up, void* const* down, float scale, float* out, uint8_t* image_out) {
  BatchScratch& Bs = t.c->batch;
  const size_t qd = (size_t)t.c->d.num_heads * t.c->d.head_dim;
  int rc;
  if ((rc = kv_upload(t, t.c->kvl, n_slots, up, Bs.kv[0]))) return rc;
  if (image_out && (rc = attn_multi_images(t, n_seq, qd))) return rc;
  if (attention_forward_multi(t.c, 0, (uint32_t)n_seq, scale, image_out != nullptr)) return LGH_OPERATION_FAILED;   // (a failed launch, as these entry points always answered)
  if (image_out && (rc = attn_multi_images_down(t, n_seq, qd, image_out))) return rc;
  if (down && (rc = kv_download(t, t.c->kvl, n_slots, down, Bs.kv[0]))) return rc;
  return t.down(out, Bs.attn_out, n_seq * qd);
}

float half_to_float(uint16_t h) {
  const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
  float v;
  if (e == 0) v = (float)m * 0x1p-24f;
  else if (e == 31) v = m ? NAN : INFINITY;
  else v = std::ldexp((float)(m | 0x400u), (int)e - 25);
  uint32_t b;
  std::memcpy(&b, &v, 4);
  b |= s;
  std::memcpy(&v, &b, 4);
  return v;
}

}  // namespace

extern "C" {

int lgh_op_attention_decode(int device, int path, const float* q, const float* k_cache, const float* v_cache, float* out, size_t n_heads,
                            size_t n_kv, size_t head_dim, size_t max_seq, float scale, size_t pos, int n_splits, uint8_t* image_out) {
  // Backend::attention_cached (ops.rs:1479-1537) as the engine's decode step runs it over the f32 cache
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!q || !k_cache || !v_cache || !out || n_kv == 0 || n_heads % n_kv || head_dim == 0 || pos >= max_seq || max_seq > 0x7FFFFFFFu)
    return LGH_INVALID_ARGUMENT;
  if (path < 0 || path > 3 || (path == 2 && image_out)) return LGH_INVALID_ARGUMENT;   // (the any-shape kernel leaves no image)
  const size_t g = n_heads / n_kv;
  const bool fast = attn_shape_has_fast_kernel((uint32_t)head_dim, (uint32_t)g);
  if (path != 2 && !fast) return LGH_UNSUPPORTED;
  if (path == 0 && (n_splits < 1 || n_splits > 32)) return LGH_INVALID_ARGUMENT;
  if (path == 2 && max_seq * 4 > 150 * 1024) return LGH_UNSUPPORTED;   // the scores of a head live in LDS
  if (path == 3 && max_seq > kAttnHeadMaxRows) return LGH_UNSUPPORTED;   // (here too)
  const AttnView v{nullptr, t.up(q, n_heads * head_dim), nullptr, t.up(nullptr, n_heads * head_dim)};   // (f32 cache: no staged rows)
  if (!v.q || !v.attn_out) return LGH_ALLOCATION_FAILED;
  int rc;
  if ((rc = attn_setup(t, LGH_KV_F32, n_heads, n_kv, head_dim, max_seq, path == 0 ? n_splits : 0)) || (rc = set_pos(t, pos))) return rc;
  // 0: split + merge (attn_split_launch picks 4 or 8 waves from max_seq); 1: one launch (engine: pos + 1 <= direct_attn_max_kv); 2: the
  // kernel of the shapes the others do not cover (engine: every token of such a model), here on any head_dim / group size; 3: one launch,
  // a workgroup per query head (engine: pos + 1 <= direct_attn_max_kv)
  t.c->attn_direct = path == 1 ? ATTN_VAR_DIRECT : path == 3 ? ATTN_VAR_HEAD : ATTN_VAR_SPLIT;
  if (path == 3) t.c->direct_attn_max_kv = (uint32_t)max_seq;   // the launch sizes its LDS arrays by it: any pos < max_seq fits
  t.c->attn_generic = path == 2;
  const void* const caches[KV_KINDS] = {k_cache, v_cache};
  return attn_run(t, v, caches, nullptr, scale, out, image_out);
}

int lgh_op_attention_decode_multi(int device, const float* q, const float* k_cache, const float* v_cache, float* out, size_t n_heads, size_t n_kv,
                                  size_t head_dim, size_t max_seq, size_t n_slots, size_t n_seq, const int* pos, const int* slot, float scale,
                                  int n_splits, uint8_t* image_out) {
  // the multi-sequence decode step's attention (engine_layer.hip: attention_forward_multi) over f32 cache slots
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!q || !k_cache || !v_cache || !out || !pos || !slot || n_kv == 0 || n_heads % n_kv || head_dim == 0 || max_seq == 0 || max_seq > 0x7FFFFFFFu ||
      n_slots == 0 || n_splits < 1 || n_splits > 32 || !seqs_ok(n_seq, kMaxBatch, slot, n_slots, false, pos, max_seq))
    return LGH_INVALID_ARGUMENT;
  if (!attn_shape_has_fast_kernel((uint32_t)head_dim, (uint32_t)(n_heads / n_kv))) return LGH_UNSUPPORTED;
  if (int rc = attn_multi_setup(t, LGH_KV_F32, q, nullptr, nullptr, n_heads, n_kv, head_dim, max_seq, n_seq, pos, slot, n_splits)) return rc;
  const void* const caches[KV_KINDS] = {k_cache, v_cache};
  return attn_multi_run(t, n_slots, n_seq, caches, nullptr, scale, out, image_out);
}

int lgh_op_attention_kv8(int device, uint32_t kv_cache_type, const float* q, int8_t* k_bytes, int8_t* v_bytes, float* k_scale, float* v_scale,
                         const float* k_new, const float* v_new, float* out, size_t n_heads, size_t n_kv, size_t head_dim, size_t max_seq,
                         float scale, size_t pos, int n_splits, uint8_t* image_out) {
  // QuantizedKVCache (kv_quantized.rs:143-300): the attention launch also quantizes the current rows and stores them at `pos`
  Tmp t(device);
  if (t.rc) return t.rc;
  if (kv_cache_type < LGH_KV_INT8 || kv_cache_type > LGH_KV_FP8_E5M2) return LGH_UNSUPPORTED;
  const bool i8 = kv_cache_type == LGH_KV_INT8;
  if (!q || !k_bytes || !v_bytes || !k_new || !v_new || !out || (i8 && (!k_scale || !v_scale))) return LGH_INVALID_ARGUMENT;
  if (n_kv == 0 || n_heads % n_kv || pos >= max_seq || max_seq > 0x7FFFFFFFu || n_splits < 1 || n_splits > 32) return LGH_INVALID_ARGUMENT;
  if (!attn_shape_has_fast_kernel((uint32_t)head_dim, (uint32_t)(n_heads / n_kv))) return LGH_UNSUPPORTED;
  const AttnView v{nullptr, t.up(q, n_heads * head_dim), up_kv_new(t, k_new, v_new, n_kv * head_dim), t.up(nullptr, n_heads * head_dim)};
  if (!v.q || !v.kv_tmp || !v.attn_out) return LGH_ALLOCATION_FAILED;
  int rc;
  if ((rc = attn_setup(t, kv_cache_type, n_heads, n_kv, head_dim, max_seq, n_splits)) || (rc = set_pos(t, pos))) return rc;
  void* const caches[KV_KINDS] = {k_bytes, v_bytes, k_scale, v_scale};
  return attn_run(t, v, caches, caches, scale, out, image_out);
}

int lgh_op_attention_kv8_multi(int device, uint32_t kv_cache_type, const float* q, int8_t* k_bytes, int8_t* v_bytes, float* k_scale, float* v_scale,
                               const float* k_new, const float* v_new, float* out, size_t n_heads, size_t n_kv, size_t head_dim, size_t max_seq,
                               size_t n_slots, size_t n_seq, const int* pos, const int* slot, float scale, int n_splits, uint8_t* image_out) {
  // the multi-sequence decode step's attention (engine_layer.hip: attention_forward_multi) over byte-cache slots
  Tmp t(device);
  if (t.rc) return t.rc;
  if (kv_cache_type < LGH_KV_INT8 || kv_cache_type > LGH_KV_FP8_E5M2) return LGH_UNSUPPORTED;
  const bool i8 = kv_cache_type == LGH_KV_INT8;
  if (!q || !k_bytes || !v_bytes || !k_new || !v_new || !out || !pos || !slot || (i8 && (!k_scale || !v_scale))) return LGH_INVALID_ARGUMENT;
  // (two sequences on one slot would both store a row into it)
  if (n_kv == 0 || n_heads % n_kv || head_dim == 0 || max_seq == 0 || max_seq > 0x7FFFFFFFu || n_slots == 0 || n_slots > (size_t)kMaxBatch ||
      n_splits < 1 || n_splits > 32 || !seqs_ok(n_seq, kMaxBatch, slot, n_slots, true, pos, max_seq))
    return LGH_INVALID_ARGUMENT;
  if (!attn_shape_has_fast_kernel((uint32_t)head_dim, (uint32_t)(n_heads / n_kv))) return LGH_UNSUPPORTED;
  if (int rc = attn_multi_setup(t, kv_cache_type, q, k_new, v_new, n_heads, n_kv, head_dim, max_seq, n_seq, pos, slot, n_splits)) return rc;
  void* const caches[KV_KINDS] = {k_bytes, v_bytes, k_scale, v_scale};
  return attn_multi_run(t, n_slots, n_seq, caches, caches, scale, out, image_out);
}

int lgh_op_attention_tq(int device, uint32_t kv_cache_type, const float* q, uint8_t* k_codes, uint8_t* v_codes, uint32_t* k_qjl, const float* k_new,
                        const float* v_new, const float* signs, const float* qjl_matrices, float* out, size_t n_heads, size_t n_kv, size_t head_dim,
                        size_t max_seq, float scale, size_t pos, int n_splits, uint8_t* image_out) {
  // TurboQuantKVCache::write_kv + attention_layer (kv_turboquant.rs:88-201): the split launch compresses and stores the current
  // rows, the merge inverts the V rotation
  Tmp t(device);
  if (t.rc) return t.rc;
  const KvLayout l(kv_cache_type, n_kv, max_seq, head_dim);
  if (!l.tq()) return LGH_UNSUPPORTED;
  const bool qjl = l.qjl();
  if (!q || !k_codes || !v_codes || !k_new || !v_new || !signs || !out || (qjl && (!k_qjl || !qjl_matrices))) return LGH_INVALID_ARGUMENT;
  if (n_kv == 0 || n_heads % n_kv || pos >= max_seq || max_seq > 0x7FFFFFFFu || n_splits < 1 || n_splits > 32) return LGH_INVALID_ARGUMENT;
  const size_t d = head_dim;
  if (!attn_shape_has_fast_kernel((uint32_t)d, (uint32_t)(n_heads / n_kv))) return LGH_UNSUPPORTED;
  if (!signs_ok(signs, n_kv * 2 * d)) return LGH_INVALID_ARGUMENT;
  t.c->tq_signs = t.up(signs, n_kv * 2 * d);
  t.c->tq_qjl = qjl ? t.up(qjl_matrices, n_kv * d * d) : nullptr;
  const AttnView v{nullptr, t.up(q, n_heads * d), up_kv_new(t, k_new, v_new, n_kv * d), t.up(nullptr, n_heads * d)};
  if (!v.q || !v.kv_tmp || !t.c->tq_signs || (qjl && !t.c->tq_qjl) || !v.attn_out) return LGH_ALLOCATION_FAILED;
  int rc;
  if ((rc = attn_setup(t, kv_cache_type, n_heads, n_kv, d, max_seq, n_splits)) || (rc = set_pos(t, pos))) return rc;
  void* const caches[KV_KINDS] = {k_codes, v_codes, nullptr, nullptr, k_qjl};
  return attn_run(t, v, caches, caches, scale, out, image_out);
}

int lgh_op_attention_tq_multi(int device, uint32_t kv_cache_type, const float* q, uint8_t* k_codes, uint8_t* v_codes, uint32_t* k_qjl,
                              const float* k_new, const float* v_new, const float* signs, const float* qjl_matrices, float* out, size_t n_heads,
                              size_t n_kv, size_t head_dim, size_t max_seq, size_t n_slots, size_t n_seq, const int* pos, const int* slot, float scale,
                              int n_splits, uint8_t* image_out) {
  // the multi-sequence decode step's attention (engine_layer.hip: attention_forward_multi) over TurboQuant cache slots
  Tmp t(device);
  if (t.rc) return t.rc;
  const KvLayout l(kv_cache_type, n_kv, max_seq, head_dim);
  if (!l.tq()) return LGH_UNSUPPORTED;
  const bool qjl = l.qjl();
  if (!q || !k_codes || !v_codes || !k_new || !v_new || !signs || !out || !pos || !slot || (qjl && (!k_qjl || !qjl_matrices))) return LGH_INVALID_ARGUMENT;
  // (two sequences on one slot would both store a row into it)
  if (n_kv == 0 || n_heads % n_kv || head_dim == 0 || max_seq == 0 || max_seq > 0x7FFFFFFFu || n_slots == 0 || n_slots > (size_t)kMaxBatch ||
      n_splits < 1 || n_splits > 32 || !seqs_ok(n_seq, kMaxBatch, slot, n_slots, true, pos, max_seq))
    return LGH_INVALID_ARGUMENT;
  const size_t d = head_dim;
  if (!attn_shape_has_fast_kernel((uint32_t)d, (uint32_t)(n_heads / n_kv))) return LGH_UNSUPPORTED;
  if (!signs_ok(signs, n_kv * 2 * d)) return LGH_INVALID_ARGUMENT;
  if (int rc = attn_multi_setup(t, kv_cache_type, q, k_new, v_new, n_heads, n_kv, d, max_seq, n_seq, pos, slot, n_splits)) return rc;
  t.c->tq_signs = t.up(signs, n_kv * 2 * d);   // (the one layer of a context that owns layer 0: its signs and matrices are the context's first)
  t.c->tq_qjl = qjl ? t.up(qjl_matrices, n_kv * d * d) : nullptr;
  if (!t.c->tq_signs || (qjl && !t.c->tq_qjl)) return LGH_ALLOCATION_FAILED;
  void* const caches[KV_KINDS] = {k_codes, v_codes, nullptr, nullptr, k_qjl};
  return attn_multi_run(t, n_slots, n_seq, caches, caches, scale, out, image_out);
}

// an XH matrix's first m rows, un-swizzled and widened to f32: out [m][k]
static int xh_down(Tmp& t, const uint8_t* xh, size_t m, size_t k, float* out) {
  const size_t xb = xh_bytes((uint32_t)k);
  std::vector<uint8_t> host(xb);
  int rc = down_bytes(t, host.data(), xh, xb);
  if (rc) return rc;
  for (size_t tk = 0; tk < m; tk++)
    for (size_t i = 0; i < k; i++) {
      uint16_t h;
      std::memcpy(&h, host.data() + xh_offset((uint32_t)tk, (uint32_t)i), 2);
      out[tk * k + i] = half_to_float(h);
    }
  return LGH_OK;
}

// what the three block-attention entry points share once their cache is on the device: the block's queries dq (uploaded by the
// caller; a TurboQuant cache: rotated by now, scr its filled scratch, signs the layer's), a zeroed XH, the launch, the XH's rows as f32.
// refused: the status of a launch that did not start
static int attn_block_run(Tmp& t, const KvLayout& l, const KvCache& kv, const float* dq, const float* scr, const float* signs, size_t n_heads, float scale,
                          size_t pos0, size_t m_tokens, int refused, float* out) {
  const size_t qd = n_heads * l.d, xb = xh_bytes((uint32_t)qd);
  uint8_t* xh = (uint8_t*)up_bytes(t, nullptr, xb);
  if (!dq || !xh) return LGH_ALLOCATION_FAILED;
  hipStream_t st = t.c->stream;
  if (hipMemsetAsync(xh, 0, xb, st) != hipSuccess) return LGH_OPERATION_FAILED;
  const AttnBlock a{(uint32_t)n_heads, scale, dq, (uint32_t)pos0, (uint32_t)m_tokens, scr, signs, xh, st};
  if (attn_block_launch(l, kv, a) != hipSuccess) return refused;
  return xh_down(t, xh, m_tokens, qd, out);
}

int lgh_op_attention_prefill(int device, const float* q, const float* k_cache, const float* v_cache, float* out, size_t n_heads, size_t n_kv,
                             size_t head_dim, size_t max_seq, float scale, size_t pos0, size_t m_tokens) {
  // causal Backend::attention (ops.rs:1353-1472) of a block of prompt tokens as the batched prefill runs it: the f16 XH matrix that
  // the wo GEMM reads, un-swizzled here and widened to f32
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!q || !k_cache || !v_cache || !out || n_kv == 0 || n_heads % n_kv || max_seq > 0x7FFFFFFFu) return LGH_INVALID_ARGUMENT;
  const size_t qd = n_heads * head_dim;
  if (m_tokens == 0 || m_tokens > (size_t)kPfTokens || qd % 256 || pos0 + m_tokens > max_seq) return LGH_INVALID_ARGUMENT;
  const KvLayout l(LGH_KV_F32, n_kv, max_seq, head_dim);
  KvCache kv;
  const void* const host[KV_KINDS] = {k_cache, v_cache};
  if (int rc = kv_upload(t, l, 1, host, kv)) return rc;
  return attn_block_run(t, l, kv, t.up(q, m_tokens * qd), nullptr, nullptr, n_heads, scale, pos0, m_tokens, LGH_UNSUPPORTED, out);
}

// the f32 scratch of the TurboQuant prompt pass, NaN-filled: K then V, each [n_kv][max_seq][head_dim]
static float* pf_tq_scratch(Tmp& t, size_t cache) {
  float* s = t.up(nullptr, 2 * cache);
  if (s && hipMemsetD32Async((hipDeviceptr_t)s, (int)0x7FC00000u, 2 * cache, t.c->stream) != hipSuccess) return nullptr;
  return s;
}

int lgh_op_pf_tq_store(int device, uint32_t kv_cache_type, const float* k_rows, const float* v_rows, size_t m, size_t n_kv, size_t head_dim,
                       size_t max_seq, size_t pos0, const float* signs, uint8_t* k_codes, uint8_t* v_codes) {
  // TurboQuantKVCache::write_kv (kv_turboquant.rs:88-122) for a block of prompt rows, as the batched prefill runs it
  Tmp t(device);
  if (t.rc) return t.rc;
  if (kv_cache_type != LGH_KV_TQ2 && kv_cache_type != LGH_KV_TQ3) return LGH_UNSUPPORTED;
  if (head_dim != 64 && head_dim != 128) return LGH_UNSUPPORTED;
  if (!k_rows || !v_rows || !signs || !k_codes || !v_codes || n_kv == 0 || max_seq > 0x7FFFFFFFu) return LGH_INVALID_ARGUMENT;
  if (m == 0 || m > (size_t)kPfTokens || pos0 + m > max_seq || !signs_ok(signs, n_kv * 2 * head_dim)) return LGH_INVALID_ARGUMENT;
  const KvLayout l(kv_cache_type, n_kv, max_seq, head_dim);
  const size_t d = head_dim, cache = l.stride_floats();
  float* scr = pf_tq_scratch(t, cache);
  KvCache kv;
  void* const codes[KV_KINDS] = {k_codes, v_codes};
  if (int rc = kv_upload(t, l, 1, codes, kv)) return rc;
  float* ds = t.up(signs, n_kv * 2 * d);
  if (!scr || !ds) return LGH_ALLOCATION_FAILED;
  hipStream_t st = t.c->stream;
  // the block's rows where the QKV epilogue leaves them: rows pos0 .. pos0+m-1 of every kv head
  for (size_t h = 0; h < n_kv; h++) {
    if (hipMemcpyAsync(scr + (h * max_seq + pos0) * d, k_rows + h * m * d, m * d * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(scr + cache + (h * max_seq + pos0) * d, v_rows + h * m * d, m * d * 4, hipMemcpyHostToDevice, st) != hipSuccess)
      return LGH_OPERATION_FAILED;
  }
  if (tq_pf_rows_launch(l.tq_bits(), scr, scr + cache, kv.k_bytes(), kv.v_bytes(), nullptr, ds, (uint32_t)n_kv, (uint32_t)n_kv, (uint32_t)d, (uint32_t)max_seq, (uint32_t)pos0,
                        (uint32_t)m, 0, 0, st) != hipSuccess)
    return LGH_OPERATION_FAILED;
  return kv_download(t, l, 1, codes, kv);
}

int lgh_op_kv_prefix_copy(int device, uint32_t kv_cache_type, uint32_t n_kv, uint32_t max_seq, uint32_t head_dim, uint32_t n_layers, uint32_t n_slots,
                          void* const* caches, uint32_t slot, uint32_t n_rows, void* packed, int restore) {
  // the copy of PrefixSharing::save_prefix / try_restore (cache.rs:287-326) as lgh_prefix_save / lgh_prefix_restore launch it, over the
  // slots' caches of a bare context
  Tmp t(device);
  if (t.rc) return t.rc;
  if (kv_cache_type > LGH_KV_TQ3_QJL) return LGH_INVALID_ARGUMENT;
  if (head_dim != 64 && head_dim != 128) return LGH_UNSUPPORTED;
  if (!caches || !packed || !n_kv || !max_seq || max_seq > 0x7FFFFFFFu || !n_layers || !n_slots || n_slots > (uint32_t)kMaxBatch) return LGH_INVALID_ARGUMENT;
  if (slot >= n_slots || n_rows == 0 || n_rows > max_seq) return LGH_INVALID_ARGUMENT;
  lgh_ctx* c = t.c;
  c->d.num_kv_heads = n_kv;
  c->d.head_dim = head_dim;
  c->d.max_seq_len = max_seq;
  c->d.kv_cache_type = kv_cache_type;
  c->d.num_layers = n_layers;
  c->kvl = KvLayout(c->d);
  c->l0 = 0;
  c->l1 = n_layers;
  for (uint32_t li = 0; li < n_layers; li++)
    for (int kind = 0; kind < KV_KINDS; kind++)
      if (c->kvl.pos_bytes(kind) && !caches[li * KV_KINDS + kind]) return LGH_INVALID_ARGUMENT;
  BatchScratch& Bs = c->batch;
  Bs.max_batch = n_slots;
  Bs.kv.assign(n_layers, KvCache{});
  for (uint32_t li = 0; li < n_layers; li++)
    if (int rc = kv_upload(t, c->kvl, n_slots, caches + li * KV_KINDS, Bs.kv[li])) return rc;
  const size_t bytes = (size_t)kv_prefix_bytes(c, n_rows);
  void* dp = up_bytes(t, restore ? packed : nullptr, bytes);
  if (!dp) return LGH_ALLOCATION_FAILED;
  if (int rc = kv_prefix_copy(c, (int)slot, n_rows, n_rows, dp, restore != 0)) return rc;
  if (!restore) return down_bytes(t, packed, dp, bytes);
  for (uint32_t li = 0; li < n_layers; li++)
    if (int rc = kv_download(t, c->kvl, n_slots, caches + li * KV_KINDS, Bs.kv[li])) return rc;
  return LGH_OK;
}

int lgh_op_attention_prefill_tq(int device, uint32_t kv_cache_type, const float* q, const uint8_t* k_codes, const uint8_t* v_codes, const float* signs,
                                float* out, size_t n_heads, size_t n_kv, size_t head_dim, size_t max_seq, float scale, size_t pos0, size_t m_tokens) {
  // TurboQuantKVCache::attention_layer (kv_turboquant.rs:127-201) for a block of prompt tokens, as the batched prefill runs it
  Tmp t(device);
  if (t.rc) return t.rc;
  if (kv_cache_type != LGH_KV_TQ2 && kv_cache_type != LGH_KV_TQ3) return LGH_UNSUPPORTED;
  if (head_dim != 64 && head_dim != 128) return LGH_UNSUPPORTED;
  if (!q || !k_codes || !v_codes || !signs || !out || n_kv == 0 || n_heads % n_kv || max_seq > 0x7FFFFFFFu) return LGH_INVALID_ARGUMENT;
  const size_t g = n_heads / n_kv;
  if (g != 1 && g != 2 && g != 4 && g != 8) return LGH_UNSUPPORTED;   // (pf_eligible's group sizes)
  const KvLayout l(kv_cache_type, n_kv, max_seq, head_dim);
  const size_t d = head_dim, qd = n_heads * d, cache = l.stride_floats();
  if (m_tokens == 0 || m_tokens > (size_t)kPfTokens || qd % 256 || pos0 + m_tokens > max_seq || !signs_ok(signs, n_kv * 2 * d))
    return LGH_INVALID_ARGUMENT;
  float *dq = t.up(q, m_tokens * qd), *ds = t.up(signs, n_kv * 2 * d), *scr = pf_tq_scratch(t, cache);
  KvCache kv;
  const void* const codes[KV_KINDS] = {k_codes, v_codes};
  if (int rc = kv_upload(t, l, 1, codes, kv)) return rc;
  if (!dq || !ds || !scr) return LGH_ALLOCATION_FAILED;
  if (tq_pf_rows_launch(l.tq_bits(), scr, scr + cache, kv.k_bytes(), kv.v_bytes(), dq, ds, (uint32_t)n_heads, (uint32_t)n_kv, (uint32_t)d, (uint32_t)max_seq, (uint32_t)pos0, 0,
                        (uint32_t)m_tokens, (uint32_t)(pos0 + m_tokens), t.c->stream) != hipSuccess)
    return LGH_OPERATION_FAILED;
  return attn_block_run(t, l, kv, dq, scr, ds, n_heads, scale, pos0, m_tokens, LGH_OPERATION_FAILED, out);
}

int lgh_op_pf_kv8_store(int device, uint32_t kv_cache_type, const float* k_rows, const float* v_rows, size_t m, size_t n_kv, size_t head_dim,
                        size_t max_seq, size_t pos0, uint8_t* k_bytes, uint8_t* v_bytes, float* k_scales, float* v_scales) {
  // QuantizedKVCache's row write for a block of prompt rows, as the batched prefill over a byte cache runs it
  Tmp t(device);
  if (t.rc) return t.rc;
  if (kv_cache_type != LGH_KV_INT8 && kv_cache_type != LGH_KV_FP8_E4M3 && kv_cache_type != LGH_KV_FP8_E5M2) return LGH_UNSUPPORTED;
  if (head_dim != 64 && head_dim != 128) return LGH_UNSUPPORTED;
  const KvLayout l(kv_cache_type, n_kv, max_seq, head_dim);
  if (!k_rows || !v_rows || !k_bytes || !v_bytes || (l.has_scales() && (!k_scales || !v_scales)) || n_kv == 0 || max_seq > 0x7FFFFFFFu)
    return LGH_INVALID_ARGUMENT;
  if (m == 0 || m > (size_t)kPfTokens || pos0 > max_seq || pos0 + m > max_seq) return LGH_INVALID_ARGUMENT;
  KvCache kv;
  void* const host[KV_KINDS] = {k_bytes, v_bytes, k_scales, v_scales};
  if (int rc = kv_upload(t, l, 1, host, kv)) return rc;
  const size_t rows = n_kv * m * head_dim;
  float *dk = t.up(k_rows, rows), *dv = t.up(v_rows, rows);
  if (!dk || !dv) return LGH_ALLOCATION_FAILED;
  if (kv8_pf_store_launch(kv_cache_type, dk, dv, (uint32_t)m, kv, (uint32_t)n_kv, (uint32_t)head_dim, (uint32_t)max_seq, (uint32_t)pos0, (uint32_t)m,
                          t.c->stream) != hipSuccess)
    return LGH_OPERATION_FAILED;
  return kv_download(t, l, 1, host, kv);
}

int lgh_op_attention_prefill_kv8(int device, uint32_t kv_cache_type, const float* q, const uint8_t* k_bytes, const uint8_t* v_bytes, const float* k_scales,
                                 const float* v_scales, float* out, size_t n_heads, size_t n_kv, size_t head_dim, size_t max_seq, float scale, size_t pos0,
                                 size_t m_tokens) {
  // QuantizedKVCache::attention for a block of prompt tokens, as the batched prefill over a byte cache runs it
  Tmp t(device);
  if (t.rc) return t.rc;
  if (kv_cache_type != LGH_KV_INT8 && kv_cache_type != LGH_KV_FP8_E4M3 && kv_cache_type != LGH_KV_FP8_E5M2) return LGH_UNSUPPORTED;
  if (head_dim != 64 && head_dim != 128) return LGH_UNSUPPORTED;
  const KvLayout l(kv_cache_type, n_kv, max_seq, head_dim);
  if (!q || !k_bytes || !v_bytes || (l.has_scales() && (!k_scales || !v_scales)) || !out || n_kv == 0 || n_heads % n_kv || max_seq > 0x7FFFFFFFu)
    return LGH_INVALID_ARGUMENT;
  const size_t g = n_heads / n_kv;
  if (g != 1 && g != 2 && g != 4 && g != 8) return LGH_UNSUPPORTED;   // (pf_eligible's group sizes)
  const size_t qd = n_heads * head_dim;
  if (m_tokens == 0 || m_tokens > (size_t)kPfTokens || qd % 256 || pos0 > max_seq || pos0 + m_tokens > max_seq) return LGH_INVALID_ARGUMENT;
  KvCache kv;
  const void* const host[KV_KINDS] = {k_bytes, v_bytes, k_scales, v_scales};
  if (int rc = kv_upload(t, l, 1, host, kv)) return rc;
  return attn_block_run(t, l, kv, t.up(q, m_tokens * qd), nullptr, nullptr, n_heads, scale, pos0, m_tokens, LGH_OPERATION_FAILED, out);
}

// ---- device-resident weights by tensor name: CudaBackend::load_model_weights + the `b.name()` lookups of its vec_mat /
// vec_mat_q (src/backend/cuda/mod.rs:121-146, 436-470, 511-575; store: cuda/dequant_weights.rs) ----
}  // extern "C"

#include <map>
#include <memory>
#include <mutex>
#include <string>

struct lgh_backend {
  std::unique_ptr<Tmp> t;
  std::map<std::string, DevWeight> weights;
  float *x = nullptr, *out = nullptr;   // staging, grown on demand
  size_t x_cap = 0, out_cap = 0;
  uint64_t hits = 0;
  std::mutex mu;   // `Backend: Send + Sync` (backend/mod.rs:29): calls on one handle may come from several threads
};

extern "C" {

int lgh_backend_create(int device, lgh_backend** out) {
  if (!out) return LGH_INVALID_ARGUMENT;
  *out = nullptr;
  auto be = std::make_unique<lgh_backend>();
  be->t = std::make_unique<Tmp>(device);
  if (be->t->rc) return be->t->rc;
  *out = be.release();
  return LGH_OK;
}

void lgh_backend_destroy(lgh_backend* be) { delete be; }

int lgh_backend_load_weight(lgh_backend* be, const char* name, uint32_t type, const void* w, size_t k, size_t n) {
  if (!be || !name || !w) return LGH_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(be->mu);
  lgh_ctx* c = be->t->c;
  if (hipSetDevice(c->device) != hipSuccess) return LGH_NOT_AVAILABLE;
  const uint32_t bs = blk_elems((int)type);
  if (!bs || k % bs) return LGH_SHAPE_MISMATCH;
  if (be->weights.count(name)) return fail(c, LGH_INVALID_ARGUMENT, std::string("weight already loaded: ") + name);
  DevWeight W;
  int rc = upload_matrix(c, W, (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w, n * (k / bs) * blk_bytes((int)type));
  if (rc) return rc;
  be->weights.emplace(name, W);
  return LGH_OK;
}

int lgh_backend_has_weight(const lgh_backend* be, const char* name) {
  if (!be || !name) return 0;
  std::lock_guard<std::mutex> lock(const_cast<lgh_backend*>(be)->mu);
  return be->weights.count(name) ? 1 : 0;
}

int lgh_backend_vec_mat_q(lgh_backend* be, const char* name, const float* x, float* out, size_t k, size_t n) {
  if (!be || !name || !x || !out) return LGH_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(be->mu);
  lgh_ctx* c = be->t->c;
  if (hipSetDevice(c->device) != hipSuccess) return LGH_NOT_AVAILABLE;
  auto it = be->weights.find(name);
  if (it == be->weights.end()) return fail(c, LGH_INVALID_ARGUMENT, std::string("no device-resident weight named ") + name);
  const DevWeight& W = it->second;
  if (W.k != k || W.n != n) return fail(c, LGH_SHAPE_MISMATCH, std::string(name) + ": vec_mat_q dimension mismatch");   // cuda/mod.rs:528-534
  if (k > be->x_cap) { if (dev_alloc(c, (void**)&be->x, k * 4)) return LGH_ALLOCATION_FAILED; be->x_cap = k; }
  if (n > be->out_cap) { if (dev_alloc(c, (void**)&be->out, n * 4)) return LGH_ALLOCATION_FAILED; be->out_cap = n; }
  if (hipMemcpyAsync(be->x, x, k * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  xq_stale(c, be->x);
  int rc = linear_any(c, LGH_K_MISC, W, be->x, be->out, nullptr, nullptr, nullptr);
  if (rc) return rc;
  be->hits++;
  return be->t->down(out, be->out, n);
}

const char* lgh_backend_last_error(const lgh_backend* be) { return be ? be->t->c->err.c_str() : "null backend"; }

int lgh_bench_vec_mat(int device, uint32_t type, const void* w, const void* w2, size_t k, size_t n, int mode, int iters,
                      int copies, double* avg_us) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!avg_us || iters <= 0) return LGH_INVALID_ARGUMENT;
  const bool two_streams = (mode & 16) != 0;
  mode &= 15;
  const uint32_t be = blk_elems((int)type);
  if (!be || k % be) return LGH_SHAPE_MISMATCH;
  const size_t nbytes = n * (k / be) * blk_bytes((int)type);
  if (copies < 1) copies = 1;
  if (copies > 64) copies = 64;
  // `copies` distinct device copies are cycled so that consecutive launches do not re-read weights that the
  // 256 MiB Infinity Cache still holds (in the engine a token streams GBs between two uses of a matrix)
  std::vector<DevWeight> Ws(copies), W2s(copies);
  int rc;
  for (int i = 0; i < copies; i++) {
    if ((rc = upload_matrix(t.c, Ws[i], (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w, nbytes))) return rc;
    if (mode == 2 && (rc = upload_matrix(t.c, W2s[i], (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w2 ? w2 : w, nbytes))) return rc;
  }
  // mode bit 4 (experiment): consecutive launches alternate between two streams with nothing ordering them — how much of a
  // launch's fixed cost hides behind its neighbour when the hardware may overlap them
  hipStream_t s2 = nullptr;
  if (two_streams && hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) return LGH_OPERATION_FAILED;
  hipStream_t s1 = t.c->stream;
  int flip = 0;
  int cur = 0;
  std::vector<float> hx(k), hw(k, 1.0f);
  for (size_t i = 0; i < k; i++) hx[i] = 0.001f * (float)((i * 2654435761u) % 2001) - 1.0f;
  float *dx = t.up(hx.data(), k), *dnw = t.up(hw.data(), k), *dout = t.up(nullptr, n);
  std::vector<float> hn(n, 1.0f);
  float* dnext = mode == 3 ? t.up(hn.data(), n) : nullptr;
  if (!dx || !dnw || !dout || (mode == 3 && (!dnext || !xq_get(t.c, dout, (uint32_t)n)))) return LGH_ALLOCATION_FAILED;
  if (mode == 3 && hipMemsetAsync(dout, 0, n * 4, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  auto once = [&]() -> int {
    DevWeight& W = Ws[cur];
    DevWeight& W2 = W2s[cur];
    cur = (cur + 1) % copies;
    if (two_streams) { t.c->stream = (flip ^= 1) ? s2 : s1; for (auto& q : t.c->xqs) q.fresh = true; }
    if (mode == 2) {
      SegSpec sp;
      sp.npass = 2;
      sp.W[0] = &W; sp.W[1] = &W2;
      sp.x[0] = sp.x[1] = dx;
      sp.epi = EPI_SWIGLU;
      sp.out = dout;
      return launch_mv(t.c, LGH_K_GATEUP, &sp, 1, dnw, (uint32_t)k);
    }
    // mode 3: wo / down as the engine launches them — residual in place, XQ image of the output times the next norm's weights
    if (mode == 3) return linear_any(t.c, LGH_K_MISC, W, dx, dout, nullptr, dout, nullptr, 2, dnext);
    return linear_any(t.c, LGH_K_MISC, W, dx, dout, mode == 1 ? dnw : nullptr, nullptr, nullptr);
  };
  for (int i = 0; i < 3; i++)
    if ((rc = once())) return rc;
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return LGH_OPERATION_FAILED;
#ifdef LGH_STAMPS
  (void)lgh::mvq_spans(nullptr, 1);
#endif
  if (two_streams) { (void)hipStreamSynchronize(s1); (void)hipStreamSynchronize(s2); t.c->stream = s1; }
  (void)hipEventRecord(a, s1);
  if (two_streams) { (void)hipStreamWaitEvent(s2, a, 0); }
  for (int i = 0; i < iters; i++)
    if ((rc = once())) break;
  if (two_streams) {   // b on s1 after both streams have drained
    hipEvent_t j;
    (void)hipEventCreateWithFlags(&j, hipEventDisableTiming);
    (void)hipEventRecord(j, s2);
    (void)hipStreamWaitEvent(s1, j, 0);
    t.c->stream = s1;
  }
  (void)hipEventRecord(b, s1);
  hipError_t e = hipEventSynchronize(b);
  if (s2) { (void)hipStreamSynchronize(s2); (void)hipStreamDestroy(s2); }
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  if (rc) return rc;
  if (e != hipSuccess) return LGH_OPERATION_FAILED;
  *avg_us = (double)ms * 1000.0 / iters;
#ifdef LGH_STAMPS
  {  // phase profile of the LAST launch: per stamp, min / median / max over workgroups, relative to the first start
    std::vector<unsigned long long> st(8192 * 8);
    if ((mfma_type(Ws[0].type) ? lgh::mvq_read_stamps(st.data(), st.size()) : lgh::mv_read_stamps(st.data(), st.size())) == hipSuccess) {
      MvPlan plan;
      if (mfma_type(Ws[0].type)) (void)mvq_plan((uint32_t)k, (uint32_t)n, mode == 2 ? 2 : 1, &plan, (uint32_t)n);
      else (void)mv_plan(Ws[0].type, (uint32_t)k, (uint32_t)n, mode == 2 ? 2 : 1, &plan, (uint32_t)n, 0);
      size_t nwg = std::min<size_t>(plan.n_wg, 8192);
      unsigned long long t0 = ~0ull;
      for (size_t w = 0; w < nwg; w++) t0 = std::min(t0, st[w * 8]);
      std::fprintf(stderr, "  stamps (us since first workgroup start; %zu workgroups x %u threads, rows/wg %u):\n", nwg, plan.threads, plan.rows_per_wg);
      const char* names[8] = {"start", "x published", "first item done", "stream done", "after barrier", "end", "loads issued", "x staged"};
      for (int i = 0; i < 8; i++) {
        std::vector<double> v;
        for (size_t w = 0; w < nwg; w++) v.push_back((double)(st[w * 8 + i] - t0) / 100.0);
        std::sort(v.begin(), v.end());
        std::fprintf(stderr, "    %-16s min %6.2f  p50 %6.2f  p90 %6.2f  max %6.2f\n", names[i], v[0], v[v.size() / 2], v[v.size() * 9 / 10], v.back());
      }
      if (mfma_type(Ws[0].type)) {
        unsigned long long sp[128];
        if (lgh::mvq_spans(sp, 0) == hipSuccess) {   // consecutive launches: busy span and idle gap between them
          std::vector<double> busy, idle;
          for (int i = 0; i < 64; i++) {
            const int j = (i + 63) & 63;
            if (sp[2 * i] == ~0ull || sp[2 * j] == ~0ull || sp[2 * i] < sp[2 * j]) continue;
            busy.push_back((double)(sp[2 * i + 1] - sp[2 * i]) / 100.0);
            idle.push_back((double)((long long)sp[2 * i] - (long long)sp[2 * j + 1]) / 100.0);
          }
          std::sort(busy.begin(), busy.end());
          std::sort(idle.begin(), idle.end());
          if (!busy.empty())
            std::fprintf(stderr, "    launch spans (%zu): first start -> last end p50 %.2f us; previous last end -> first start p50 %.2f us (min %.2f)\n",
                         busy.size(), busy[busy.size() / 2], idle[idle.size() / 2], idle[0]);
        }
        std::vector<unsigned long long> ws(2048 * 16 * 8);
        if (lgh::mvq_read_wave_stamps(ws.data(), ws.size()) == hipSuccess) {
          const size_t nw = plan.threads / 64, ng = std::min<size_t>(nwg, 2048);
          const char* wn[8] = {"start", "scalars", "pre-x", "issued", "x here", "staged", "streamed", "end"};
          for (int i = 0; i < 8; i++) {
            std::fprintf(stderr, "    per-wave %-8s p50:", wn[i]);
            for (size_t w = 0; w < nw; w++) {
              std::vector<double> v;
              for (size_t g = 0; g < ng; g++) v.push_back((double)(ws[(g * 16 + w) * 8 + i] - t0) / 100.0);
              std::sort(v.begin(), v.end());
              std::fprintf(stderr, " %5.2f", v[v.size() / 2]);
            }
            std::fprintf(stderr, "\n");
          }
        }
      }
    }
  }
#endif
  return LGH_OK;
}

int lgh_bench_hbm_read(int device, size_t bytes, int iters, double* gbps) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!gbps || iters <= 0 || bytes < (1u << 20)) return LGH_INVALID_ARGUMENT;
  bytes &= ~(size_t)4095;
  uint8_t* buf = nullptr;
  float* sink = nullptr;
  if (dev_alloc(t.c, (void**)&buf, bytes) || dev_alloc(t.c, (void**)&sink, 4096 * 4)) return LGH_ALLOCATION_FAILED;
  if (hipMemsetAsync(buf, 1, bytes, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  double best = 0.0;
  for (int nt = 0; nt < 2; nt++) {   // both cache policies; the better one is the ceiling
    if (hbm_read_launch(buf, bytes, sink, nt, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;   // warm-up
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return LGH_OPERATION_FAILED;
    (void)hipEventRecord(a, t.c->stream);
    hipError_t e = hipSuccess;
    for (int i = 0; i < iters && e == hipSuccess; i++) e = hbm_read_launch(buf, bytes, sink, nt, t.c->stream);
    (void)hipEventRecord(b, t.c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (e != hipSuccess) return LGH_OPERATION_FAILED;
    best = std::max(best, (double)bytes * iters / ((double)ms * 1e-3) / 1e9);
  }
  *gbps = best;
  return LGH_OK;
}

// ------------------------------------------------------------------------------------------------
// The engine's mat-vec launch assembly (launch_mv -> build_mv_group -> mvq_launch / mv_launch) one call site at a time, for
// kernel-level tests (tests/test_gpu_matvec.py).  Test surface: not part of the inference API.
// ------------------------------------------------------------------------------------------------
static size_t weight_bytes(uint32_t type, size_t k, size_t n) {
  const uint32_t be = blk_elems((int)type);
  return be && k % be == 0 ? n * (k / be) * blk_bytes((int)type) : 0;
}

int lgh_op_linear_chain(int device, uint32_t type_a, const void* w_a, const void* w_a_up, const float* bias_a, size_t k, size_t n_a,
                        const float* x, const float* norm_w, float eps, const float* resid, int xq_next, const float* next_nw,
                        uint32_t type_b, const void* w_b, size_t n_b, float* out_a, float* out_b, float* out_b_requant, int* image_used) {
  // launch A (linear_any: STORE / RESID with bias; or the SWIGLU gate-up launch), asked to leave its output's XQ image; then launch B
  // on A's output twice: first as the engine runs it (from A's image when A left one), then after marking the image stale
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w_a || !x || !w_b || !out_a || !out_b || !out_b_requant || xq_next < 0 || xq_next > 2 || (xq_next == 2 && !next_nw) ||
      (w_a_up && (resid || bias_a)))
    return LGH_INVALID_ARGUMENT;
  t.c->d.norm_eps = eps;
  const size_t nba = weight_bytes(type_a, k, n_a), nbb = weight_bytes(type_b, n_a, n_b);
  if (!nba || !nbb) return LGH_SHAPE_MISMATCH;
  DevWeight WA, WU, WB;
  int rc;
  if ((rc = upload_matrix(t.c, WA, (int)type_a, (uint32_t)k, (uint32_t)n_a, 1, -1, w_a, nba))) return rc;
  if (w_a_up && (rc = upload_matrix(t.c, WU, (int)type_a, (uint32_t)k, (uint32_t)n_a, 1, -1, w_a_up, nba))) return rc;
  if ((rc = upload_matrix(t.c, WB, (int)type_b, (uint32_t)n_a, (uint32_t)n_b, 1, -1, w_b, nbb))) return rc;
  if (w_a_up && !fused_type(WA.type)) return LGH_UNSUPPORTED;
  float *dx = t.up(x, k), *dnw = norm_w ? t.up(norm_w, k) : nullptr, *dres = resid ? t.up(resid, n_a) : nullptr;
  float *dbias = bias_a ? t.up(bias_a, n_a) : nullptr, *dnext = next_nw ? t.up(next_nw, n_a) : nullptr;
  float *da = t.up(nullptr, n_a), *db = t.up(nullptr, n_b), *db2 = t.up(nullptr, n_b);
  if (!dx || (norm_w && !dnw) || (resid && !dres) || (bias_a && !dbias) || (next_nw && !dnext) || !da || !db || !db2) return LGH_ALLOCATION_FAILED;
  XqBuf* qa = xq_get(t.c, da, (uint32_t)n_a);   // A's output has an image slot, as the engine's activation buffers do
  if (!qa) return LGH_ALLOCATION_FAILED;
  if (w_a_up) {
    SegSpec sp;
    sp.npass = 2;
    sp.W[0] = &WA; sp.W[1] = &WU;
    sp.x[0] = sp.x[1] = dx;
    sp.epi = EPI_SWIGLU;
    sp.out = da;
    sp.xq_next = xq_next; sp.xq_next_nw = dnext;
    if ((rc = launch_mv(t.c, LGH_K_GATEUP, &sp, 1, dnw, (uint32_t)k))) return rc;
  } else if ((rc = linear_any(t.c, LGH_K_MISC, WA, dx, da, dnw, dres, dbias, xq_next, dnext))) {
    return rc;
  }
  qa = xq_get(t.c, da, (uint32_t)n_a);   // (A's launch may have registered more images: look it up again)
  if (image_used) *image_used = qa && qa->fresh ? 1 : 0;
  const float* bnw = xq_next == 2 ? dnext : nullptr;
  if ((rc = linear_any(t.c, LGH_K_MISC, WB, da, db, bnw, nullptr, nullptr))) return rc;
  xq_stale(t.c, da);
  if ((rc = linear_any(t.c, LGH_K_MISC, WB, da, db2, bnw, nullptr, nullptr))) return rc;
  if ((rc = t.down(out_a, da, n_a)) || (rc = t.down(out_b, db, n_b))) return rc;
  return t.down(out_b_requant, db2, n_b);
}

// Test surface: the context flags of every later lgh_op_* / lgh_bench_* call of this process (LGH_FLAG_MV_GENERIC: the same launch
// with and without the static launch plans).  Returns the previous value.
uint64_t lgh_debug_static_launches(void) { return lgh::mvq_static_launches(); }

int lgh_debug_mv_plan(uint32_t k, uint32_t n_rows, uint32_t launch_rows, uint32_t out[7]) {
  if (!out) return LGH_INVALID_ARGUMENT;
  lgh::MvPlan p;
  if (lgh::mvq_plan(k, n_rows, 1, &p, launch_rows) != hipSuccess) return LGH_UNSUPPORTED;
  out[0] = p.T; out[1] = p.G; out[2] = p.units; out[3] = p.rows_per_wg; out[4] = p.n_wg; out[5] = p.threads; out[6] = p.red_floats;
  return LGH_OK;
}

uint32_t lgh_op_set_flags(uint32_t flags) {
  const uint32_t prev = g_op_flags;
  g_op_flags = flags;
  return prev;
}

int lgh_op_linear_image(int device, uint32_t type, const void* w, const void* w_up, const float* bias, size_t k, size_t n, const float* x,
                        const float* norm_w, float eps, const float* resid, int xq_next, const float* next_nw, int want_argmax, float* out,
                        uint8_t* image_out, float* ssq_out, int* image_used, int* token_out, int* argmax_parts, int* static_launches) {
  // ONE launch as the engine assembles it (linear_any: STORE / RESID with bias; or the SWIGLU gate-up launch) and everything it leaves:
  // the f32 output, its XQ image (xq_bytes(n) bytes) and the image's sums of squares (n / 16), and — want_argmax, the greedy step's
  // output projection — the token the arg-max that follows picks, with the number of parts the launch itself left (0: two stages)
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w || !x || !out || xq_next < 0 || xq_next > 2 || (xq_next == 2 && !next_nw) || (w_up && (resid || bias)) || (want_argmax && !token_out))
    return LGH_INVALID_ARGUMENT;
  t.c->d.norm_eps = eps;
  const size_t nb = weight_bytes(type, k, n);
  if (!nb) return LGH_SHAPE_MISMATCH;
  DevWeight WA, WU;
  int rc;
  if ((rc = upload_matrix(t.c, WA, (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w, nb))) return rc;
  if (w_up && (rc = upload_matrix(t.c, WU, (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w_up, nb))) return rc;
  if (w_up && !fused_type(WA.type)) return LGH_UNSUPPORTED;
  float *dx = t.up(x, k), *dnw = norm_w ? t.up(norm_w, k) : nullptr, *dres = resid ? t.up(resid, n) : nullptr;
  float *dbias = bias ? t.up(bias, n) : nullptr, *dnext = next_nw ? t.up(next_nw, n) : nullptr, *da = t.up(nullptr, n);
  if (!dx || (norm_w && !dnw) || (resid && !dres) || (bias && !dbias) || (next_nw && !dnext) || !da) return LGH_ALLOCATION_FAILED;
  XqBuf* qa = n % 256 == 0 || n % 16 == 0 ? xq_get(t.c, da, (uint32_t)n) : nullptr;
  if (qa) {   // what the launch does not write must not look written
    if (hipMemsetAsync(qa->xq, 0xA5, xq_bytes(n), t.c->stream) != hipSuccess || hipMemsetAsync(qa->ssq, 0xA5, (n / 16) * 4, t.c->stream) != hipSuccess)
      return LGH_OPERATION_FAILED;
  }
  if (want_argmax) {
    if (dev_alloc(t.c, (void**)&t.c->amax_v, kAmaxPartsMax * 4) || dev_alloc(t.c, (void**)&t.c->amax_i, kAmaxPartsMax * 4)) return LGH_ALLOCATION_FAILED;
  }
  uint32_t parts = 0;
  const uint64_t static_before = lgh::mvq_static_launches();
  if (w_up) {
    SegSpec sp;
    sp.npass = 2;
    sp.W[0] = &WA; sp.W[1] = &WU;
    sp.x[0] = sp.x[1] = dx;
    sp.epi = EPI_SWIGLU;
    sp.out = da;
    sp.xq_next = xq_next; sp.xq_next_nw = dnext;
    rc = launch_mv(t.c, LGH_K_GATEUP, &sp, 1, dnw, (uint32_t)k);
  } else {
    rc = linear_any(t.c, LGH_K_MISC, WA, dx, da, dnw, dres, dbias, xq_next, dnext, want_argmax ? t.c->amax_v : nullptr,
                    want_argmax ? t.c->amax_i : nullptr, want_argmax ? &parts : nullptr);
  }
  if (rc) return rc;
  if (static_launches) *static_launches = (int)(lgh::mvq_static_launches() - static_before);
  if (want_argmax) {
    hipError_t e = parts ? argmax_merge_launch(t.c->amax_v, t.c->amax_i, parts, t.c->state, nullptr, t.c->stream)
                         : argmax_launch(da, (uint32_t)n, t.c->amax_v, t.c->amax_i, t.c->state, nullptr, t.c->stream);
    if (e != hipSuccess) return LGH_OPERATION_FAILED;
    if (argmax_parts) *argmax_parts = (int)parts;
    if (hipMemcpyAsync(token_out, t.c->state + ST_ARGMAX, 4, hipMemcpyDeviceToHost, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  }
  qa = xq_find(t.c, da);
  const bool used = qa && qa->fresh;
  if (image_used) *image_used = used ? 1 : 0;
  if (used && image_out && hipMemcpyAsync(image_out, qa->xq, xq_bytes(n), hipMemcpyDeviceToHost, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if (used && ssq_out && hipMemcpyAsync(ssq_out, qa->ssq, (n / 16) * 4, hipMemcpyDeviceToHost, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return t.down(out, da, n);
}

int lgh_op_moe_experts(int device, uint32_t type_gate_up, const void* w_gate, const void* w_up, uint32_t type_down, const void* w_down,
                       size_t n_experts, size_t hidden, size_t ffn, size_t top_k, const float* router, const int* sel, const float* sel_w,
                       const float* x, const float* norm_w, float eps, float* out, int* sel_out, float* sel_w_out) {
  // ffn_forward's MoE half on x (also the residual): with `router` the device router picks the experts, otherwise the given
  // selection and weights drive the same expert launches
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w_gate || !w_up || !w_down || !x || !norm_w || !out || (!router && (!sel || !sel_w)) || top_k == 0 || top_k > 8 ||
      top_k > n_experts || n_experts > 64)
    return LGH_INVALID_ARGUMENT;
  if (sel)
    for (size_t i = 0; i < top_k; i++)
      if (sel[i] < 0 || (size_t)sel[i] >= n_experts) return LGH_INVALID_ARGUMENT;
  lgh_model_desc& d = t.c->d;
  d.norm_eps = eps;
  d.hidden_size = (uint32_t)hidden;
  d.num_experts = (uint32_t)n_experts;
  d.num_experts_per_token = (uint32_t)top_k;
  const size_t ngu = weight_bytes(type_gate_up, hidden, ffn), nd = weight_bytes(type_down, ffn, hidden);
  if (!ngu || !nd) return LGH_SHAPE_MISMATCH;
  LayerW Lw;
  const uint32_t E = (uint32_t)n_experts;
  int rc;
  if ((rc = upload_matrix(t.c, Lw.gate_exps, (int)type_gate_up, (uint32_t)hidden, (uint32_t)ffn, E, -1, w_gate, ngu * E)) ||
      (rc = upload_matrix(t.c, Lw.up_exps, (int)type_gate_up, (uint32_t)hidden, (uint32_t)ffn, E, -1, w_up, ngu * E)) ||
      (rc = upload_matrix(t.c, Lw.down_exps, (int)type_down, (uint32_t)ffn, (uint32_t)hidden, E, -1, w_down, nd * E)))
    return rc;
  Lw.ffn_norm = t.up(norm_w, hidden);
  if (router) Lw.router = t.up(router, n_experts * hidden);
  FfnView v{t.up(x, hidden), t.up(nullptr, ffn), t.up(nullptr, ffn), t.up(nullptr, hidden), nullptr, nullptr};
  v.moe_sel = (int*)up_bytes(t, sel, top_k * 4);
  v.moe_w = t.up(sel_w, top_k);
  if (!Lw.ffn_norm || (router && !Lw.router) || !v.hidden || !v.act || !v.act2 || !v.xnorm || !v.moe_sel || !v.moe_w) return LGH_ALLOCATION_FAILED;
  // the engine's activation buffers have XQ image slots (the residual stream, act, act2), the scratch running sum has none
  if (!xq_get(t.c, v.hidden, (uint32_t)hidden) || !xq_get(t.c, v.act, (uint32_t)ffn) || !xq_get(t.c, v.act2, (uint32_t)ffn)) return LGH_ALLOCATION_FAILED;
  if ((rc = router ? ffn_forward(t.c, Lw, v, nullptr, false) : moe_experts_forward(t.c, Lw, v, nullptr, false))) return rc;
  if (sel_out && (rc = down_bytes(t, sel_out, v.moe_sel, top_k * 4))) return rc;
  if (sel_w_out && (rc = t.down(sel_w_out, v.moe_w, top_k))) return rc;
  return t.down(out, v.hidden, hidden);
}

// ------------------------------------------------------------------------------------------------
// The batched prompt path's layer steps (engine_prefill.hip: pf_block_input, pf_qkv_step, pf_wo_step, pf_ffn_step, pf_moe_step) one at
// a time on a bare one-layer context with the path's own scratch (pf_ensure), for kernel-level tests
// (tests/test_gpu_prefill_ref.py).  Test support: not part of the inference API.
// Before the first launch every scratch buffer the kernels read is filled with NaN bit patterns (f32 0x7FC0BEEF, f16 0x7E5A), so that
// anything consumed without having been produced shows in the output; the padding rows of an XH block ARE read by the MFMAs and their
// partial sums are never consumed.  The MoE index tables get in-range sentinels instead (a NaN pattern read as an index would address
// outside the buffers), each one a value the kernels must NOT leave there: lists 0x7F7F, tokmap kPfMoeRows - 1, rowmap 0 (expert 0,
// row 0 — what a zero-filled table holds; the grouping kernel's own -1 on every padding row has to replace it), everything else 0x55.
// ------------------------------------------------------------------------------------------------
static bool pf_poison(lgh_ctx* c, void* p, size_t bytes, uint32_t word) {
  return !p || !bytes || hipMemsetD32Async((hipDeviceptr_t)p, (int)word, bytes / 4, c->stream) == hipSuccess;
}

// the model fields, the layer and the scratch of a one-layer context; F = dense FFN width (0: none), E / top_k / EI = experts (0: none)
static int pf_test_ctx(Tmp& t, const LayerW& Lw, size_t H, size_t head_dim, size_t n_heads, size_t n_kv, size_t F, size_t E, size_t top_k, size_t EI,
                       float eps) {
  lgh_ctx* c = t.c;
  lgh_model_desc& d = c->d;
  d.norm_eps = eps;
  d.hidden_size = (uint32_t)H;
  d.head_dim = (uint32_t)head_dim;
  d.num_heads = (uint32_t)n_heads;
  d.num_kv_heads = (uint32_t)n_kv;
  d.intermediate_size = (uint32_t)F;
  d.num_experts = (uint32_t)E;
  d.num_experts_per_token = (uint32_t)top_k;
  d.expert_intermediate_size = (uint32_t)EI;
  c->layers.assign(1, Lw);
  c->l0 = 0;
  c->l1 = 1;
  if (int rc = pf_ensure(c)) return rc;
  const PfScratch& P = c->pf;
  const uint32_t QD = d.num_heads * d.head_dim, kF32 = 0x7FC0BEEFu, kF16 = 0x7E5A7E5Au;
  const bool ok =
      pf_poison(c, P.xh_h, xh_bytes(d.hidden_size), kF16) && pf_poison(c, P.xh_attn, xh_bytes(QD), kF16) &&
      pf_poison(c, P.xh_act, xh_bytes((uint32_t)std::max(F, EI)), kF16) && pf_poison(c, P.hidden, (size_t)kPfTokens * H * 4, kF32) &&
      pf_poison(c, P.q, (size_t)kPfTokens * QD * 4, kF32) && pf_poison(c, P.part, P.part_bytes, kF32) &&
      pf_poison(c, P.ssq, (size_t)kPfTokens * kPfSsqChunks * 4, kF32) && pf_poison(c, P.moe_w, E ? (size_t)kPfTokens * top_k * 4 : 0, kF32) &&
      pf_poison(c, P.moe_sel, E ? (size_t)kPfTokens * top_k * 4 : 0, 0x55u) && pf_poison(c, P.moe_cnt, E ? (size_t)kPfMaxExperts * 4 : 0, 0x55u) &&
      pf_poison(c, P.moe_base, E ? (size_t)kPfMaxExperts * 4 : 0, 0x55u) &&
      pf_poison(c, P.moe_list, E ? (size_t)kPfMaxExperts * kPfTokens * 4 : 0, 0x7F7Fu) &&
      pf_poison(c, P.moe_rowmap, E ? (size_t)kPfMoeRows * 4 : 0, 0u) &&
      pf_poison(c, P.moe_tokmap, E ? (size_t)kPfTokens * kPfMaxTopK * 4 : 0, (uint32_t)kPfMoeRows - 1) &&
      pf_poison(c, P.xh_gather, E ? xh_bytes(d.hidden_size) * E : 0, kF16) && pf_poison(c, P.xh_act_e, E ? xh_bytes((uint32_t)EI) * E : 0, kF16);
  return ok ? LGH_OK : LGH_OPERATION_FAILED;
}

static int pf_up_weight(Tmp& t, DevWeight& W, uint32_t type, const void* w, size_t k, size_t n, size_t n_stack = 1) {
  const size_t nb = weight_bytes(type, k, n);
  if (!nb || !w) return LGH_SHAPE_MISMATCH;
  if (int rc = upload_matrix(t.c, W, (int)type, (uint32_t)k, (uint32_t)n, (uint32_t)n_stack, -1, w, nb * n_stack)) return rc;
  return pf_supported_type(W.type) && n % 16 == 0 ? LGH_OK : LGH_UNSUPPORTED;
}

// hidden, the next XH (when a next norm weight was given) and the sums of squares of the first m tokens
static int pf_down_block(Tmp& t, size_t m, size_t H, bool with_xh, float* hidden_out, float* xh_out, float* ssq_out) {
  const PfScratch& P = t.c->pf;
  int rc;
  if ((rc = t.down(hidden_out, P.hidden, m * H)) || (rc = t.down(ssq_out, P.ssq, m * kPfSsqChunks))) return rc;
  return with_xh ? xh_down(t, P.xh_h, m, H, xh_out) : LGH_OK;
}

static bool pf_block_shape_ok(size_t H, size_t m) { return H && H % 256 == 0 && H <= 2048u * kPfSsqChunks && m >= 1 && m <= (size_t)kPfTokens; }

int lgh_op_pf_qkv(int device, const uint32_t* types, const void* const* w, const float* const* bias, const float* hidden, const float* norm_w,
                  float eps, size_t hidden_size, size_t head_dim, size_t n_heads, size_t n_kv_heads, int neox, size_t max_seq_len, size_t pos0,
                  size_t m_tokens, float rope_base, float rope_scale, float* q_out, float* k_cache, float* v_cache) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!types || !w || !hidden || !norm_w || !q_out || !k_cache || !v_cache || n_kv_heads == 0 || n_heads % n_kv_heads || rope_scale == 0.0f ||
      max_seq_len > 0x7FFFFFFFu || !pf_block_shape_ok(hidden_size, m_tokens) || pos0 + m_tokens > max_seq_len)
    return LGH_INVALID_ARGUMENT;
  const size_t H = hidden_size, QD = n_heads * head_dim, KD = n_kv_heads * head_dim, rows[3] = {QD, KD, KD};
  if ((head_dim != 64 && head_dim != 128) || QD % 256 || KD % 16) return LGH_UNSUPPORTED;   // (pf_eligible's shapes)
  LayerW Lw;
  DevWeight* const W[3] = {&Lw.wq, &Lw.wk, &Lw.wv};
  float** const db[3] = {&Lw.bq, &Lw.bk, &Lw.bv};
  int rc;
  for (int s = 0; s < 3; s++) {
    if ((rc = pf_up_weight(t, *W[s], types[s], w[s], H, rows[s]))) return rc;
    if (bias && bias[s] && !(*db[s] = t.up(bias[s], rows[s]))) return LGH_ALLOCATION_FAILED;
  }
  lgh_model_desc& d = t.c->d;
  d.max_seq_len = (uint32_t)max_seq_len;
  d.rope_freq_base = rope_base;
  d.rope_freq_scale = rope_scale;
  d.use_neox_rope = neox ? 1 : 0;
  d.head_dim = (uint32_t)head_dim;
  std::vector<float> cs;
  rope_table_host(d, cs);
  t.c->rope_cs = t.up(cs.data(), cs.size());
  Lw.attn_norm = t.up(norm_w, H);
  const KvLayout l(LGH_KV_F32, n_kv_heads, max_seq_len, head_dim);
  void* const caches[KV_KINDS] = {k_cache, v_cache};
  if ((rc = kv_upload(t, l, 1, caches, Lw.kv))) return rc;
  if (!t.c->rope_cs || !Lw.attn_norm) return LGH_ALLOCATION_FAILED;
  if ((rc = pf_test_ctx(t, Lw, H, head_dim, n_heads, n_kv_heads, 0, 0, 0, 0, eps))) return rc;
  if (hipMemcpyAsync(t.c->pf.hidden, hidden, m_tokens * H * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if ((rc = pf_block_input(t.c, Lw.attn_norm, (uint32_t)m_tokens))) return rc;
  if ((rc = pf_qkv_step(t.c, t.c->layers[0], Lw.kv.k_f32(), Lw.kv.v_f32(), (uint32_t)pos0, (uint32_t)m_tokens))) return rc;
  if ((rc = t.down(q_out, t.c->pf.q, m_tokens * QD))) return rc;
  return kv_download(t, l, 1, caches, Lw.kv);
}

int lgh_op_pf_linear(int device, uint32_t type, const void* w, const float* bias, const float* x, size_t k, size_t hidden_size, const float* resid,
                     const float* next_nw, size_t m_tokens, float* hidden_out, float* xh_out, float* ssq_out) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w || !x || !resid || !next_nw || !hidden_out || !xh_out || !ssq_out || !pf_block_shape_ok(hidden_size, m_tokens) || k == 0 || k % 256)
    return LGH_INVALID_ARGUMENT;
  const size_t H = hidden_size;
  LayerW Lw;
  int rc;
  if ((rc = pf_up_weight(t, Lw.wo, type, w, k, H))) return rc;
  if (bias && !(Lw.bo = t.up(bias, H))) return LGH_ALLOCATION_FAILED;
  Lw.ffn_norm = t.up(next_nw, H);
  float* dx = t.up(x, m_tokens * k);
  if (!Lw.ffn_norm || !dx) return LGH_ALLOCATION_FAILED;
  if ((rc = pf_test_ctx(t, Lw, H, 64, k / 64, k / 64, 0, 0, 0, 0, 1e-5f))) return rc;   // (the wo input is [tokens][heads * head_dim] = k wide)
  const PfScratch& P = t.c->pf;
  if (hipMemcpyAsync(P.hidden, resid, m_tokens * H * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if (pf_to_xh_launch(dx, (uint32_t)k, P.xh_attn, (uint32_t)m_tokens, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if ((rc = pf_wo_step(t.c, t.c->layers[0], (uint32_t)m_tokens))) return rc;
  return pf_down_block(t, m_tokens, H, true, hidden_out, xh_out, ssq_out);
}

int lgh_op_pf_ffn(int device, uint32_t type_gate_up, const void* w_gate, const void* w_up, uint32_t type_down, const void* w_down,
                  const float* hidden, const float* norm_w, const float* next_nw, float eps, size_t hidden_size, size_t ffn, size_t m_tokens,
                  float* hidden_out, float* xh_out, float* ssq_out, float* act_out) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w_gate || !w_up || !w_down || !hidden || !norm_w || !hidden_out || !ssq_out || (next_nw && !xh_out) ||
      !pf_block_shape_ok(hidden_size, m_tokens) || ffn == 0 || ffn % 256)
    return LGH_INVALID_ARGUMENT;
  const size_t H = hidden_size;
  LayerW Lw;
  int rc;
  if ((rc = pf_up_weight(t, Lw.gate, type_gate_up, w_gate, H, ffn)) || (rc = pf_up_weight(t, Lw.up, type_gate_up, w_up, H, ffn)) ||
      (rc = pf_up_weight(t, Lw.down, type_down, w_down, ffn, H)))
    return rc;
  Lw.ffn_norm = t.up(norm_w, H);
  float* dnext = next_nw ? t.up(next_nw, H) : nullptr;
  if (!Lw.ffn_norm || (next_nw && !dnext)) return LGH_ALLOCATION_FAILED;
  if ((rc = pf_test_ctx(t, Lw, H, 64, H / 64, H / 64, ffn, 0, 0, 0, eps))) return rc;
  if (hipMemcpyAsync(t.c->pf.hidden, hidden, m_tokens * H * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if ((rc = pf_block_input(t.c, Lw.ffn_norm, (uint32_t)m_tokens))) return rc;
  if ((rc = pf_ffn_step(t.c, t.c->layers[0], dnext, (uint32_t)m_tokens))) return rc;
  if (act_out && (rc = xh_down(t, t.c->pf.xh_act, m_tokens, ffn, act_out))) return rc;
  return pf_down_block(t, m_tokens, H, dnext != nullptr, hidden_out, xh_out, ssq_out);
}

int lgh_op_pf_moe(int device, uint32_t type_gate_up, const void* w_gate, const void* w_up, uint32_t type_down, const void* w_down,
                  const float* router, size_t n_experts, size_t top_k, const float* hidden, const float* norm_w, const float* next_nw, float eps,
                  size_t hidden_size, size_t ffn, size_t m_tokens, float* hidden_out, float* xh_out, float* ssq_out, int* sel_out, float* sel_w_out,
                  int* counts_out, int* bases_out, int* lists_out, int* rowmap_out, int* tokmap_out, float* act_out) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w_gate || !w_up || !w_down || !router || !hidden || !norm_w || !hidden_out || !ssq_out || (next_nw && !xh_out) || !sel_out || !sel_w_out ||
      !counts_out || !bases_out || !lists_out || !rowmap_out || !tokmap_out || !pf_block_shape_ok(hidden_size, m_tokens) || ffn == 0 || ffn % 256 ||
      top_k == 0 || top_k > n_experts)
    return LGH_INVALID_ARGUMENT;
  if (n_experts > (size_t)kPfMaxExperts || top_k > (size_t)kPfMaxTopK || (size_t)kPfTokens * top_k + 15 * n_experts > (size_t)kPfMoeRows)
    return LGH_UNSUPPORTED;   // (pf_eligible's condition)
  const size_t H = hidden_size, E = n_experts;
  LayerW Lw;
  int rc;
  if ((rc = pf_up_weight(t, Lw.gate_exps, type_gate_up, w_gate, H, ffn, E)) || (rc = pf_up_weight(t, Lw.up_exps, type_gate_up, w_up, H, ffn, E)) ||
      (rc = pf_up_weight(t, Lw.down_exps, type_down, w_down, ffn, H, E)))
    return rc;
  Lw.ffn_norm = t.up(norm_w, H);
  Lw.router = t.up(router, E * H);
  float* dnext = next_nw ? t.up(next_nw, H) : nullptr;
  if (!Lw.ffn_norm || !Lw.router || (next_nw && !dnext)) return LGH_ALLOCATION_FAILED;
  if ((rc = pf_test_ctx(t, Lw, H, 64, H / 64, H / 64, 0, E, top_k, ffn, eps))) return rc;
  const PfScratch& P = t.c->pf;
  if (hipMemcpyAsync(P.hidden, hidden, m_tokens * H * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if ((rc = pf_block_input(t.c, Lw.ffn_norm, (uint32_t)m_tokens))) return rc;
  if ((rc = pf_moe_step(t.c, t.c->layers[0], dnext, (uint32_t)m_tokens))) return rc;
  if ((rc = down_bytes(t, sel_out, P.moe_sel, m_tokens * top_k * 4)) || (rc = t.down(sel_w_out, P.moe_w, m_tokens * top_k)) ||
      (rc = down_bytes(t, counts_out, P.moe_cnt, E * 4)) || (rc = down_bytes(t, bases_out, P.moe_base, E * 4)) ||
      (rc = down_bytes(t, lists_out, P.moe_list, E * kPfTokens * 4)) || (rc = down_bytes(t, rowmap_out, P.moe_rowmap, (size_t)kPfMoeRows * 4)) ||
      (rc = down_bytes(t, tokmap_out, P.moe_tokmap, m_tokens * top_k * 4)))
    return rc;
  for (size_t e = 0; act_out && e < E; e++)   // every expert's SwiGLU rows as the down GEMM reads them, rows past its count included
    if ((rc = xh_down(t, P.xh_act_e + e * xh_bytes((uint32_t)ffn), kPfTokens, ffn, act_out + e * kPfTokens * ffn))) return rc;
  return pf_down_block(t, m_tokens, H, dnext != nullptr, hidden_out, xh_out, ssq_out);
}

// ------------------------------------------------------------------------------------------------
// The multi-sequence step's mat-vec launches (engine_batch.hip: linear_multi, qkv_forward_multi, moe_grouped_forward, each through
// launch_mvb -> build_mv_group -> mvqb_launch) one at a time on a bare one-layer context with the engine's own batch scratch (batch_scratch_alloc), for
// kernel-level tests (tests/test_gpu_matvec_multi.py).  Test support: not part of the inference API.
// Before the first launch every vector, image, partial-sum and cache buffer of the scratch holds the NaN pattern 0x7FC0BEEF; the MoE
// tables hold in-range sentinels the kernels must not leave: counts 0x55, entry lists max_batch * top_k - 1 (the last pair), selections 0x55.
// ------------------------------------------------------------------------------------------------
struct MbShape { size_t H = 256, head_dim = 64, n_heads = 4, n_kv = 4, F = 0, vocab = 16, max_seq = 1, E = 0, top_k = 0, EI = 0; };

static int mb_test_ctx(Tmp& t, const LayerW& Lw, const MbShape& s, float eps, size_t max_batch, bool staged_kv) {
  lgh_ctx* c = t.c;
  lgh_model_desc& d = c->d;
  d.norm_eps = eps;
  d.hidden_size = (uint32_t)s.H;
  d.head_dim = (uint32_t)s.head_dim;
  d.num_heads = (uint32_t)s.n_heads;
  d.num_kv_heads = (uint32_t)s.n_kv;
  d.intermediate_size = (uint32_t)s.F;
  d.vocab_size = (uint32_t)s.vocab;
  d.max_seq_len = (uint32_t)s.max_seq;
  d.num_layers = 1;
  d.num_experts = (uint32_t)s.E;
  d.num_experts_per_token = (uint32_t)s.top_k;
  d.expert_intermediate_size = (uint32_t)s.EI;
  if (staged_kv) d.kv_cache_type = LGH_KV_INT8;
  c->kvl = KvLayout(d);
  c->layers.assign(1, Lw);
  c->l0 = 0;
  c->l1 = 1;
  if (int rc = batch_scratch_alloc(c, (uint32_t)max_batch)) return rc;
  const BatchScratch& Bs = c->batch;
  const size_t B = max_batch, H = s.H, QD = s.n_heads * s.head_dim, KD = s.n_kv * s.head_dim, np = B * s.top_k;
  const uint32_t kF32 = 0x7FC0BEEFu;
  bool ok = pf_poison(c, Bs.hidden, B * H * 4, kF32) && pf_poison(c, Bs.xnorm, B * H * 4, kF32) && pf_poison(c, Bs.q, B * QD * 4, kF32) &&
            pf_poison(c, Bs.attn_out, B * QD * 4, kF32) && pf_poison(c, Bs.act, B * Bs.ffn * 4, kF32) && pf_poison(c, Bs.act2, B * Bs.ffn * 4, kF32) &&
            pf_poison(c, Bs.logits, B * s.vocab * 4, kF32) && pf_poison(c, Bs.mv_part, Bs.mv_part_floats * 4, kF32) &&
            pf_poison(c, Bs.moe_w, B * 8 * 4, kF32) && pf_poison(c, Bs.moe_sel, B * 8 * 4, 0x55u) && pf_poison(c, Bs.kv_tmp, B * 2 * KD * 4, kF32) &&
            pf_poison(c, Bs.kv[0].t[KV_K], c->kvl.f32() ? B * c->kvl.slot_bytes(KV_K) : 0, kF32) &&
            pf_poison(c, Bs.kv[0].t[KV_V], c->kvl.f32() ? B * c->kvl.slot_bytes(KV_V) : 0, kF32) &&
            pf_poison(c, Bs.moe_act, np * s.EI * 4, kF32) && pf_poison(c, Bs.moe_tmp, np * H * 4, kF32) && pf_poison(c, Bs.moe_cnt, 64 * 4, 0x55u) &&
            pf_poison(c, Bs.moe_idx, (size_t)64 * kMaxBatch * 4, np ? (uint32_t)np - 1 : 0u);
  for (const XqBuf& q : c->xqs) ok = ok && pf_poison(c, q.xq, xq_bytes(q.k), kF32) && pf_poison(c, q.ssq, (size_t)ssq_stride_of(q.k) * 4, kF32);
  return ok ? LGH_OK : LGH_OPERATION_FAILED;
}

// n vectors of k floats from `base` on: the images their producers in the step would have left (the engine's own producer on each
// registered view, multiplied with `tag`), marked fresh
static int mb_produce_images(lgh_ctx* c, const float* base, uint32_t k, size_t n, const float* tag) {
  for (size_t s = 0; s < n; s++) {
    XqBuf* q = xq_find(c, base + s * k);
    if (!q) return LGH_OPERATION_FAILED;
    if (xq_quantize_launch(q->f32, tag, q->xq, tag ? q->ssq : nullptr, k, c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
    q->fresh = true;
    q->tag = tag;
  }
  return LGH_OK;
}

static void mb_structures(int* out, const uint64_t before[3]) {
  uint64_t now[3];
  lgh::mvqb_structure_launches(now);
  for (int i = 0; out && i < 3; i++) out[i] = (int)(now[i] - before[i]);
}

void lgh_debug_mvqb_structures(uint64_t* out) { lgh::mvqb_structure_launches(out); }

// What a launch of the step multiplies: A = the SwiGLU gate | up pair (w_up: hidden -> act), a residual launch (resid: attn_out -> hidden,
// wo and down) or a plain store (hidden -> logits, the output projection).  The model fields follow from the launch's k and n.
struct MbLinear {
  DevWeight WA, WU;
  float *dnw = nullptr, *dbias = nullptr, *dnext = nullptr;
  float *in = nullptr, *out = nullptr;
  // floats between two sequences' outputs: n — or, for a store, n rounded up to a whole tile, so that whatever a launch writes past
  // row n of ANY sequence lands in floats nobody owns (the step's logits rows lie n apart; the stride is the launch's parameter)
  size_t out_stride = 0;
  int role = 0;   // 0 store, 1 residual, 2 SwiGLU
};

static int mb_linear_setup(Tmp& t, MbLinear& M, uint32_t type, const void* w, const void* w_up, const float* bias, size_t k, size_t n, size_t n_seq,
                           size_t max_batch, const float* x, const float* norm_w, float eps, const float* resid, const float* next_nw, size_t vocab) {
  if (k == 0 || k % 256 || !mvb_k_ok((uint32_t)k)) return LGH_UNSUPPORTED;   // (what lgh_batch_create refuses: batch_weights_ok)
  const size_t nb = weight_bytes(type, k, n);
  if (!nb) return LGH_SHAPE_MISMATCH;
  int rc;
  if ((rc = upload_matrix(t.c, M.WA, (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w, nb))) return rc;
  if (w_up && (rc = upload_matrix(t.c, M.WU, (int)type, (uint32_t)k, (uint32_t)n, 1, -1, w_up, nb))) return rc;
  if (!mfma_type(M.WA.type)) return LGH_UNSUPPORTED;
  M.role = w_up ? 2 : resid ? 1 : 0;
  if (M.role && n % 256) return LGH_UNSUPPORTED;   // (hidden and ffn widths)
  M.dnw = norm_w ? t.up(norm_w, k) : nullptr;
  M.dbias = bias ? t.up(bias, n) : nullptr;
  M.dnext = next_nw ? t.up(next_nw, n) : nullptr;
  if ((norm_w && !M.dnw) || (bias && !M.dbias) || (next_nw && !M.dnext)) return LGH_ALLOCATION_FAILED;
  MbShape s;
  s.vocab = vocab;
  if (M.role == 2) { s.H = k; s.F = n; }
  else if (M.role == 1) { s.H = n; s.n_heads = s.n_kv = k / 64; }   // (the launch's input is [sequence][heads x head_dim] wide)
  else { s.H = k; s.vocab = (n + 15) / 16 * 16; }
  M.out_stride = M.role ? n : s.vocab;
  if ((rc = mb_test_ctx(t, LayerW{}, s, eps, max_batch, false)) || (rc = mb_control(t, nullptr, nullptr, n_seq))) return rc;
  const BatchScratch& Bs = t.c->batch;
  M.in = M.role == 1 ? Bs.attn_out : Bs.hidden;
  M.out = M.role == 2 ? Bs.act : M.role == 1 ? Bs.hidden : Bs.logits;
  if (hipMemcpyAsync(M.in, x, n_seq * k * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if (resid && hipMemcpyAsync(Bs.hidden, resid, n_seq * n * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  return mb_produce_images(t.c, M.in, (uint32_t)k, n_seq, M.dnw);
}

// launch A by the step's own linear_multi, as enqueue_multi makes gate | up (SwiGLU), wo (residual) and the output projection (store)
static int mb_linear_launch(Tmp& t, MbLinear& M, size_t n_seq, int xq_next) {
  const int cls = M.role == 2 ? LGH_K_GATEUP : M.role == 1 ? LGH_K_WO : LGH_K_OUTPUT;
  return linear_multi(t.c, cls, M.WA, M.role == 2 ? &M.WU : nullptr, M.in, M.out, (uint32_t)M.out_stride, (uint32_t)n_seq, M.dnw,
                      M.role == 1 ? M.out : nullptr, M.dbias, xq_next, xq_next == 2 ? M.dnext : nullptr);
}

int lgh_op_linear_multi(int device, uint32_t type, const void* w, const void* w_up, const float* bias, size_t k, size_t n, size_t n_seq,
                        size_t max_batch, const float* x, const float* norm_w, float eps, const float* resid, int xq_next, const float* next_nw,
                        float* out, uint8_t* image_out, float* ssq_out, int* image_used, int* structures) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w || !x || !out || n_seq == 0 || n_seq > max_batch || max_batch > (size_t)kMaxBatch || xq_next < 0 || xq_next > 2 || (xq_next == 2 && !next_nw) ||
      (w_up && (resid || bias)) || (!w_up && !resid && xq_next))
    return LGH_INVALID_ARGUMENT;
  MbLinear M;
  int rc;
  if ((rc = mb_linear_setup(t, M, type, w, w_up, bias, k, n, n_seq, max_batch, x, norm_w, eps, resid, next_nw, 16))) return rc;
  uint64_t before[3];
  lgh::mvqb_structure_launches(before);
  if ((rc = mb_linear_launch(t, M, n_seq, xq_next))) return rc;
  mb_structures(structures, before);
  const XqBuf* qo = M.role ? xq_find(t.c, M.out) : nullptr;
  const bool used = qo && qo->fresh;
  if (image_used) *image_used = used ? 1 : 0;
  // (the views of the sequences lie side by side: all max_batch of them come back, written or not)
  if (qo && image_out && (rc = down_bytes(t, image_out, qo->xq, max_batch * xq_stride_of((uint32_t)n)))) return rc;
  if (qo && ssq_out && (rc = t.down(ssq_out, qo->ssq, max_batch * ssq_stride_of((uint32_t)n)))) return rc;
  return t.down(out, M.out, max_batch * M.out_stride);
}

int lgh_op_linear_chain_multi(int device, uint32_t type_a, const void* w_a, const void* w_a_up, const float* bias_a, size_t k, size_t n_a, size_t n_seq,
                              size_t max_batch, const float* x, const float* norm_w, float eps, const float* resid, int xq_next, const float* next_nw,
                              uint32_t type_b, const void* w_b, size_t n_b, float* out_a, float* out_b, float* out_b_requant, int* image_used) {
  // launch A (the SwiGLU pair, or a residual launch) leaving every sequence's image; then the store launch B on A's outputs twice: from
  // A's images, then after marking them stale and producing them again with the engine's converter
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w_a || !x || !w_b || !out_a || !out_b || !out_b_requant || n_seq == 0 || n_seq > max_batch || max_batch > (size_t)kMaxBatch || xq_next < 1 ||
      xq_next > 2 || (xq_next == 2 && !next_nw) || (w_a_up && (resid || bias_a)) || (!w_a_up && !resid))
    return LGH_INVALID_ARGUMENT;
  MbLinear M;
  int rc;
  if ((rc = mb_linear_setup(t, M, type_a, w_a, w_a_up, bias_a, k, n_a, n_seq, max_batch, x, norm_w, eps, resid, next_nw, n_b))) return rc;
  const size_t nbb = weight_bytes(type_b, n_a, n_b);
  if (!nbb) return LGH_SHAPE_MISMATCH;
  DevWeight WB;
  if ((rc = upload_matrix(t.c, WB, (int)type_b, (uint32_t)n_a, (uint32_t)n_b, 1, -1, w_b, nbb))) return rc;
  if (!mfma_type(WB.type)) return LGH_UNSUPPORTED;
  if ((rc = mb_linear_launch(t, M, n_seq, xq_next))) return rc;
  const XqBuf* qa = xq_find(t.c, M.out);
  if (image_used) *image_used = qa && qa->fresh ? 1 : 0;
  const BatchScratch& Bs = t.c->batch;
  const float* bnw = xq_next == 2 ? M.dnext : nullptr;
  auto store_b = [&] { return linear_multi(t.c, LGH_K_OUTPUT, WB, nullptr, M.out, Bs.logits, (uint32_t)n_b, (uint32_t)n_seq, bnw); };
  if ((rc = store_b())) return rc;
  if ((rc = t.down(out_b, Bs.logits, n_seq * n_b))) return rc;
  for (size_t s = 0; s < n_seq; s++) xq_stale(t.c, M.out + s * n_a);
  if ((rc = mb_produce_images(t.c, M.out, (uint32_t)n_a, n_seq, bnw))) return rc;
  if ((rc = store_b())) return rc;
  if ((rc = t.down(out_b_requant, Bs.logits, n_seq * n_b))) return rc;
  return t.down(out_a, M.out, n_seq * n_a);
}

int lgh_op_qkv_rope_multi(int device, const uint32_t* types, const void* const* w, const float* const* bias, const float* x, const float* norm_w,
                          float eps, size_t hidden, size_t head_dim, size_t n_heads, size_t n_kv_heads, size_t max_seq_len, size_t n_seq,
                          size_t max_batch, const int* pos, const int* slot, float rope_base, float rope_scale, int staged, float* q_out,
                          float* k_cache, float* v_cache, float* staged_out, int* structures) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!types || !w || !x || !norm_w || !pos || !slot || !q_out || (staged ? !staged_out : (!k_cache || !v_cache)) || hidden == 0 || head_dim == 0 ||
      head_dim % 2 || n_kv_heads == 0 || n_heads % n_kv_heads || max_seq_len == 0 || max_seq_len > 0x7FFFFFFFu || rope_scale == 0.0f ||
      max_batch > (size_t)kMaxBatch || !seqs_ok(n_seq, max_batch, slot, max_batch, true, pos, max_seq_len))
    return LGH_INVALID_ARGUMENT;
  const size_t QD = n_heads * head_dim, KD = n_kv_heads * head_dim, rows[3] = {QD, KD, KD};
  if (hidden % 256 || QD % 256 || KD % 16 || !mvb_k_ok((uint32_t)hidden)) return LGH_UNSUPPORTED;
  LayerW Lw;
  DevWeight* const W[3] = {&Lw.wq, &Lw.wk, &Lw.wv};
  float** const db[3] = {&Lw.bq, &Lw.bk, &Lw.bv};
  int rc;
  for (int s = 0; s < 3; s++) {
    const size_t nb = weight_bytes(types[s], hidden, rows[s]);
    if (!nb || !w[s]) return LGH_SHAPE_MISMATCH;
    if ((rc = upload_matrix(t.c, *W[s], (int)types[s], (uint32_t)hidden, (uint32_t)rows[s], 1, -1, w[s], nb))) return rc;
    if (!mfma_type(W[s]->type)) return LGH_UNSUPPORTED;
    if (bias && bias[s] && !(*db[s] = t.up(bias[s], rows[s]))) return LGH_ALLOCATION_FAILED;
  }
  Lw.attn_norm = t.up(norm_w, hidden);
  if (!Lw.attn_norm) return LGH_ALLOCATION_FAILED;
  MbShape sh;
  sh.H = hidden; sh.head_dim = head_dim; sh.n_heads = n_heads; sh.n_kv = n_kv_heads; sh.max_seq = max_seq_len;
  if ((rc = mb_test_ctx(t, Lw, sh, eps, max_batch, staged != 0)) || (rc = mb_control(t, pos, slot, n_seq))) return rc;
  lgh_model_desc& d = t.c->d;
  d.rope_freq_base = rope_base;
  d.rope_freq_scale = rope_scale;
  std::vector<float> cs;
  rope_table_host(d, cs);
  if (!(t.c->rope_cs = t.up(cs.data(), cs.size()))) return LGH_ALLOCATION_FAILED;
  const BatchScratch& Bs = t.c->batch;
  if (hipMemcpyAsync(Bs.hidden, x, n_seq * hidden * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if ((rc = mb_produce_images(t.c, Bs.hidden, (uint32_t)hidden, n_seq, Lw.attn_norm))) return rc;
  uint64_t before[3];
  lgh::mvqb_structure_launches(before);
  if ((rc = qkv_forward_multi(t.c, t.c->layers[0], 0, (uint32_t)n_seq))) return rc;
  mb_structures(structures, before);
  if ((rc = t.down(q_out, Bs.q, max_batch * QD))) return rc;
  if (staged) return t.down(staged_out, Bs.kv_tmp, max_batch * 2 * KD);
  void* const caches[KV_KINDS] = {k_cache, v_cache};
  return kv_download(t, t.c->kvl, max_batch, caches, Bs.kv[0]);
}

int lgh_op_moe_multi(int device, uint32_t type_gate_up, const void* w_gate, const void* w_up, uint32_t type_down, const void* w_down, size_t n_experts,
                     size_t hidden, size_t ffn, size_t top_k, size_t n_seq, size_t max_batch, const float* router, const int* sel, const float* sel_w,
                     const float* x, const float* norm_w, const float* next_nw, float eps, float* out, uint8_t* image_out, float* ssq_out,
                     uint8_t* image_requant, float* ssq_requant, int* sel_out, float* sel_w_out, int* cnt_out, int* idx_out, int* structures) {
  // the grouped MoE half of a step on x [n_seq][hidden] (also the residual): with `router` the device router picks every sequence's
  // experts, otherwise the given selections and weights [n_seq][top_k] drive the same launches
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w_gate || !w_up || !w_down || !x || !norm_w || !next_nw || !out || !image_out || !ssq_out || !image_requant || !ssq_requant || !cnt_out ||
      !idx_out || (!router && (!sel || !sel_w)) || top_k == 0 || top_k > 8 || top_k > n_experts || n_experts > 64 || n_seq < 2 || n_seq > max_batch ||
      max_batch > (size_t)kMaxBatch)
    return LGH_INVALID_ARGUMENT;
  for (size_t s = 0; sel && !router && s < n_seq; s++)   // (a sequence selects an expert at most once: an expert's list holds <= n_seq pairs)
    for (size_t i = 0; i < top_k; i++) {
      if (sel[s * top_k + i] < 0 || (size_t)sel[s * top_k + i] >= n_experts) return LGH_INVALID_ARGUMENT;
      for (size_t j = 0; j < i; j++)
        if (sel[s * top_k + j] == sel[s * top_k + i]) return LGH_INVALID_ARGUMENT;
    }
  const size_t H = hidden, E = n_experts;
  if (H % 256 || ffn % 256) return LGH_UNSUPPORTED;
  const size_t ngu = weight_bytes(type_gate_up, H, ffn), nd = weight_bytes(type_down, ffn, H);
  if (!ngu || !nd) return LGH_SHAPE_MISMATCH;
  LayerW Lw;
  int rc;
  if ((rc = upload_matrix(t.c, Lw.gate_exps, (int)type_gate_up, (uint32_t)H, (uint32_t)ffn, (uint32_t)E, -1, w_gate, ngu * E)) ||
      (rc = upload_matrix(t.c, Lw.up_exps, (int)type_gate_up, (uint32_t)H, (uint32_t)ffn, (uint32_t)E, -1, w_up, ngu * E)) ||
      (rc = upload_matrix(t.c, Lw.down_exps, (int)type_down, (uint32_t)ffn, (uint32_t)H, (uint32_t)E, -1, w_down, nd * E)))
    return rc;
  if (!mfma_type(Lw.gate_exps.type) || !mfma_type(Lw.down_exps.type)) return LGH_UNSUPPORTED;
  Lw.ffn_norm = t.up(norm_w, H);
  Lw.router = t.up(router, E * H);   // (without a router matrix: what makes the layer an MoE layer for the scratch; never read)
  float* dnext = t.up(next_nw, H);
  if (!Lw.ffn_norm || !Lw.router || !dnext) return LGH_ALLOCATION_FAILED;
  MbShape sh;
  sh.H = H; sh.n_heads = sh.n_kv = H / 64; sh.E = E; sh.top_k = top_k; sh.EI = ffn;
  if ((rc = mb_test_ctx(t, Lw, sh, eps, max_batch, false)) || (rc = mb_control(t, nullptr, nullptr, n_seq))) return rc;
  const BatchScratch& Bs = t.c->batch;
  if (!Bs.moe_act) return LGH_UNSUPPORTED;   // (the shape does not group: the engine runs such layers sequence by sequence)
  if (hipMemcpyAsync(Bs.hidden, x, n_seq * H * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  if (!router && (hipMemcpyAsync(Bs.moe_sel, sel, n_seq * top_k * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess ||
                  hipMemcpyAsync(Bs.moe_w, sel_w, n_seq * top_k * 4, hipMemcpyHostToDevice, t.c->stream) != hipSuccess))
    return LGH_OPERATION_FAILED;
  if ((rc = mb_produce_images(t.c, Bs.hidden, (uint32_t)H, n_seq, Lw.ffn_norm))) return rc;   // (as wo's epilogue leaves them)
  uint64_t before[3];
  lgh::mvqb_structure_launches(before);
  if ((rc = moe_grouped_forward(t.c, t.c->layers[0], (uint32_t)n_seq, dnext, router != nullptr))) return rc;
  mb_structures(structures, before);
  // the new rows' images once more, by the engine's converter, for comparison with what the combine launch left
  const size_t xs = xq_stride_of((uint32_t)H), ss = ssq_stride_of((uint32_t)H);
  uint8_t* xq2 = (uint8_t*)up_bytes(t, nullptr, max_batch * xs);
  float* ssq2 = t.up(nullptr, max_batch * ss);
  if (!xq2 || !ssq2 || !pf_poison(t.c, xq2, max_batch * xs, 0x7FC0BEEFu) || !pf_poison(t.c, ssq2, max_batch * ss * 4, 0x7FC0BEEFu)) return LGH_ALLOCATION_FAILED;
  for (size_t s = 0; s < n_seq; s++)
    if (xq_quantize_launch(Bs.hidden + s * H, dnext, xq2 + s * xs, ssq2 + s * ss, (uint32_t)H, t.c->stream) != hipSuccess) return LGH_OPERATION_FAILED;
  const XqBuf* qh = xq_find(t.c, Bs.hidden);
  if ((rc = down_bytes(t, image_out, qh->xq, max_batch * xs)) || (rc = t.down(ssq_out, qh->ssq, max_batch * ss)) ||
      (rc = down_bytes(t, image_requant, xq2, max_batch * xs)) || (rc = t.down(ssq_requant, ssq2, max_batch * ss)) ||
      (rc = down_bytes(t, cnt_out, Bs.moe_cnt, 64 * 4)) || (rc = down_bytes(t, idx_out, Bs.moe_idx, (size_t)64 * kMaxBatch * 4)))
    return rc;
  if (sel_out && (rc = down_bytes(t, sel_out, Bs.moe_sel, n_seq * top_k * 4))) return rc;
  if (sel_w_out && (rc = t.down(sel_w_out, Bs.moe_w, n_seq * top_k))) return rc;
  return t.down(out, Bs.hidden, max_batch * H);
}

// ------------------------------------------------------------------------------------------------
// The launches of a step AROUND the fused mat-vecs, one at a time (tests/test_gpu_step_launches.py): the three embedding launches,
// qkv_forward with everything it branches on (NeoX, expanded types, staged rows), ffn_gateup_forward's unfused pair with silu_mul in
// place, and the two-stage arg-max of one row and of n_seq rows.  Test surface: not part of the inference API.
// ------------------------------------------------------------------------------------------------
int lgh_op_embed(int device, int mode, uint32_t type, const void* table, size_t vocab, size_t hidden, const int* tokens, size_t n,
                 const float* norm_w, int fill, int* state_io, float* rows_out, uint8_t* image_out, float* ssq_out, int* image_used) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!table || !rows_out || vocab == 0 || hidden == 0 || hidden > 0x7FFFFFFFu || mode < 0 || mode > 2 || n == 0) return LGH_INVALID_ARGUMENT;
  if (mode == 0 ? (n != 1 || !state_io) : !tokens) return LGH_INVALID_ARGUMENT;
  if ((mode == 1 && n > (size_t)kMaxBatch) || (mode == 2 && n > (size_t)kPfTokens)) return LGH_INVALID_ARGUMENT;
  for (size_t i = 0; i < n; i++) {
    const int tok = mode == 0 ? state_io[ST_TOKEN] : tokens[i];
    if (tok < 0 || (size_t)tok >= vocab) return LGH_INVALID_ARGUMENT;
  }
  const size_t tb = weight_bytes(type, hidden, vocab);
  if (!tb) return LGH_SHAPE_MISMATCH;
  lgh_ctx* c = t.c;
  const uint32_t H = (uint32_t)hidden;
  // mode 0: one sequence's buffers; modes 1 and 2: one sequence more than the launch covers, which must come back untouched
  const size_t nb = mode == 0 ? 1 : n + 1, xs = xq_stride_of(H), ss = ssq_stride_of(H);
  c->d.hidden_size = H;
  c->embd_type = (int)type;
  c->embd_raw = (uint8_t*)up_bytes(t, table, tb);
  c->embd_bytes = tb;
  c->hidden = t.up(nullptr, nb * hidden);
  int* d_tok = mode ? (int*)up_bytes(t, tokens, n * 4) : nullptr;
  // norm_w: the first layer's QKV weights run on the matrix cores, which is when the engine asks the embedding for their input's image
  // (embed_forward looks at the weight's device type and at hidden % 256; enqueue_multi runs only where batch_weights_ok held both)
  c->layers.resize(1);
  c->l0 = 0; c->l1 = 1;
  LayerW& L0 = c->layers[0];
  if (norm_w) {
    L0.wq.type = kDevQ4K_T16;
    if (!(L0.attn_norm = t.up(norm_w, hidden))) return LGH_ALLOCATION_FAILED;
  }
  const bool want_img = mode != 2 && norm_w && hidden % 256 == 0;
  if (want_img && (!image_out || !ssq_out)) return LGH_INVALID_ARGUMENT;
  if (!c->embd_raw || !c->hidden || (mode && !d_tok)) return LGH_ALLOCATION_FAILED;
  uint8_t* xq = nullptr;
  float* ssq = nullptr;
  hipStream_t st = c->stream;
  if (hipMemsetAsync(c->hidden, fill, nb * hidden * 4, st) != hipSuccess) return LGH_OPERATION_FAILED;
  if (want_img) {
    xq = (uint8_t*)up_bytes(t, nullptr, nb * xs);
    ssq = t.up(nullptr, nb * ss);
    if (!xq || !ssq) return LGH_ALLOCATION_FAILED;
    if (hipMemsetAsync(xq, fill, nb * xs, st) != hipSuccess || hipMemsetAsync(ssq, fill, nb * ss * 4, st) != hipSuccess) return LGH_OPERATION_FAILED;
    register_views(c, c->hidden, xq, ssq, H, (uint32_t)nb);
  }
  int rc;
  bool used = false;
  if (mode == 0) {
    if (hipMemcpyAsync(c->state, state_io, ST_WORDS * 4, hipMemcpyHostToDevice, st) != hipSuccess) return LGH_OPERATION_FAILED;
    if ((rc = embed_forward(c))) return rc;
    const XqBuf* qh = xq_find(c, c->hidden);
    used = qh && qh->fresh;
    if ((rc = down_bytes(t, state_io, c->state, ST_WORDS * 4))) return rc;
  } else if (mode == 1) {   // as enqueue_multi launches it
    if (embed_multi_launch(c->embd_type, c->embd_raw, d_tok, c->hidden, H, (uint32_t)n, xq, want_img ? L0.attn_norm : nullptr, ssq, (uint32_t)xs,
                           (uint32_t)ss, st) != hipSuccess)
      return LGH_OPERATION_FAILED;
    used = want_img;
  } else {                  // as prefill_block launches it
    if (embed_batch_launch(c->embd_type, c->embd_raw, d_tok, c->hidden, H, (uint32_t)n, st) != hipSuccess) return LGH_OPERATION_FAILED;
  }
  if (image_used) *image_used = used ? 1 : 0;
  if (want_img && ((rc = down_bytes(t, image_out, xq, nb * xs)) || (rc = t.down(ssq_out, ssq, nb * ss)))) return rc;
  return t.down(rows_out, c->hidden, nb * hidden);
}

// qkv_forward on one layer's weights and a view of its own.  fused_only (lgh_op_qkv_rope): the fused launch alone — another layout is
// refused, the view has no staged rows and none come back
static int qkv_forward_op(int device, const uint32_t* types, const void* const* w, const float* const* bias, const float* x, const float* norm_w,
                          float eps, size_t hidden, size_t head_dim, size_t n_heads, size_t n_kv_heads, size_t max_seq_len, size_t pos,
                          float rope_base, float rope_scale, int neox, int staged, bool fused_only, float* q_out, float* k_cache, float* v_cache,
                          float* staged_out, char* err, size_t errlen) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (err && errlen) err[0] = 0;
  if (!types || !w || !x || !norm_w || !q_out || !k_cache || !v_cache || (!fused_only && !staged_out) || hidden == 0 || head_dim == 0 || head_dim % 2 ||
      n_kv_heads == 0 || n_heads % n_kv_heads || pos >= max_seq_len || max_seq_len > 0x7FFFFFFFu || rope_scale == 0.0f)
    return LGH_INVALID_ARGUMENT;
  lgh_model_desc& d = t.c->d;
  d.norm_eps = eps;
  d.hidden_size = (uint32_t)hidden;
  d.head_dim = (uint32_t)head_dim;
  d.num_heads = (uint32_t)n_heads;
  d.num_kv_heads = (uint32_t)n_kv_heads;
  d.max_seq_len = (uint32_t)max_seq_len;
  d.rope_freq_base = rope_base;
  d.rope_freq_scale = rope_scale;
  d.use_neox_rope = neox ? 1 : 0;
  // staged: the path of every byte-per-element and TurboQuant cache, whose rows stay in kv_tmp for the attention launch; the int8
  // format stands for them.  The f32 caches are uploaded either way and come back untouched then
  if (staged) d.kv_cache_type = LGH_KV_INT8;
  t.c->kvl = KvLayout(d);
  const KvLayout f32l(LGH_KV_F32, n_kv_heads, max_seq_len, head_dim);
  const size_t rows[3] = {n_heads * head_dim, n_kv_heads * head_dim, n_kv_heads * head_dim}, KD = rows[1];
  LayerW Lw;
  DevWeight* const W[3] = {&Lw.wq, &Lw.wk, &Lw.wv};
  int rc;
  for (int s = 0; s < 3; s++) {
    const size_t nb = weight_bytes(types[s], hidden, rows[s]);
    if (!nb || !w[s]) return LGH_SHAPE_MISMATCH;
    if ((rc = upload_matrix(t.c, *W[s], (int)types[s], (uint32_t)hidden, (uint32_t)rows[s], 1, -1, w[s], nb))) return rc;
    if (fused_only && !fused_type(W[s]->type)) return LGH_UNSUPPORTED;   // the engine runs such layers unfused
  }
  std::vector<float> cs;
  rope_table_host(d, cs);
  t.c->rope_cs = t.up(cs.data(), cs.size());
  // the view has staged rows as the engine's always has (c->kv_tmp); q and the rows start as the NaN pattern
  const AttnView v{t.up(x, hidden), t.up(nullptr, rows[0]), fused_only ? nullptr : t.up(nullptr, 2 * KD), nullptr};
  Lw.attn_norm = t.up(norm_w, hidden);
  void* const caches[KV_KINDS] = {k_cache, v_cache};
  if ((rc = kv_upload(t, f32l, 1, caches, Lw.kv))) return rc;
  float** const db[3] = {&Lw.bq, &Lw.bk, &Lw.bv};
  for (int s = 0; s < 3; s++)
    if (bias && bias[s] && !(*db[s] = t.up(bias[s], rows[s]))) return LGH_ALLOCATION_FAILED;
  if (!t.c->rope_cs || !v.hidden || !Lw.attn_norm || !v.q || (!fused_only && !v.kv_tmp)) return LGH_ALLOCATION_FAILED;
  if (!pf_poison(t.c, v.q, rows[0] * 4, 0x7FC0BEEFu) || !pf_poison(t.c, v.kv_tmp, 2 * KD * 4, 0x7FC0BEEFu)) return LGH_OPERATION_FAILED;
  if ((rc = set_pos(t, pos))) return rc;
  if ((rc = qkv_forward(t.c, Lw, v))) {
    if (err && errlen) { std::strncpy(err, t.c->err.c_str(), errlen - 1); err[errlen - 1] = 0; }
    return rc;
  }
  if ((rc = t.down(q_out, v.q, rows[0])) || (staged_out && (rc = t.down(staged_out, v.kv_tmp, 2 * KD)))) return rc;
  return kv_download(t, f32l, 1, caches, Lw.kv);
}

int lgh_op_qkv_forward(int device, const uint32_t* types, const void* const* w, const float* const* bias, const float* x, const float* norm_w,
                       float eps, size_t hidden, size_t head_dim, size_t n_heads, size_t n_kv_heads, size_t max_seq_len, size_t pos,
                       float rope_base, float rope_scale, int neox, int staged, float* q_out, float* k_cache, float* v_cache, float* staged_out,
                       char* err, size_t errlen) {
  return qkv_forward_op(device, types, w, bias, x, norm_w, eps, hidden, head_dim, n_heads, n_kv_heads, max_seq_len, pos, rope_base, rope_scale, neox,
                        staged, false, q_out, k_cache, v_cache, staged_out, err, errlen);
}

int lgh_op_qkv_rope(int device, const uint32_t* types, const void* const* w, const float* const* bias, const float* x, const float* norm_w,
                    float eps, size_t hidden, size_t head_dim, size_t n_heads, size_t n_kv_heads, size_t max_seq_len, size_t pos,
                    float rope_base, float rope_scale, float* q_out, float* k_cache, float* v_cache) {
  // qkv_forward's fused QKV launch: RMSNorm prologue, Q with RoPE, K with RoPE into cache row `pos`, V into cache row `pos`
  return qkv_forward_op(device, types, w, bias, x, norm_w, eps, hidden, head_dim, n_heads, n_kv_heads, max_seq_len, pos, rope_base, rope_scale, 0, 0,
                        true, q_out, k_cache, v_cache, nullptr, nullptr, 0);
}

int lgh_op_ffn_gateup(int device, uint32_t type_gate, const void* w_gate, uint32_t type_up, const void* w_up, const float* x, const float* norm_w,
                      float eps, size_t hidden, size_t ffn, float* act_out) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!w_gate || !w_up || !x || !norm_w || !act_out || hidden == 0 || ffn == 0) return LGH_INVALID_ARGUMENT;
  t.c->d.norm_eps = eps;
  t.c->d.hidden_size = (uint32_t)hidden;
  const size_t ng = weight_bytes(type_gate, hidden, ffn), nu = weight_bytes(type_up, hidden, ffn);
  if (!ng || !nu) return LGH_SHAPE_MISMATCH;
  LayerW Lw;   // (no down projection: nobody asks the fused launch for act's image)
  int rc;
  if ((rc = upload_matrix(t.c, Lw.gate, (int)type_gate, (uint32_t)hidden, (uint32_t)ffn, 1, -1, w_gate, ng)) ||
      (rc = upload_matrix(t.c, Lw.up, (int)type_up, (uint32_t)hidden, (uint32_t)ffn, 1, -1, w_up, nu)))
    return rc;
  Lw.ffn_norm = t.up(norm_w, hidden);
  const FfnView v{t.up(x, hidden), t.up(nullptr, ffn), t.up(nullptr, ffn), nullptr, nullptr, nullptr};
  if (!Lw.ffn_norm || !v.hidden || !v.act || !v.act2) return LGH_ALLOCATION_FAILED;
  if (!pf_poison(t.c, v.act, ffn * 4, 0x7FC0BEEFu) || !pf_poison(t.c, v.act2, ffn * 4, 0x7FC0BEEFu)) return LGH_OPERATION_FAILED;
  if ((rc = ffn_gateup_forward(t.c, Lw, v))) return rc;
  return t.down(act_out, v.act, ffn);
}

int lgh_op_argmax(int device, const float* logits, size_t n, size_t n_seq, int* tokens_out) {
  Tmp t(device);
  if (t.rc) return t.rc;
  if (!logits || !tokens_out || n == 0 || n > 0x7FFFFFFFu || n_seq > (size_t)kMaxBatch) return LGH_INVALID_ARGUMENT;
  const size_t rows = n_seq ? n_seq : 1;
  const float* dl = t.up(logits, rows * n);
  // parts: 64 per row (misc.hip: kArgmaxParts), as lgh_finalize / batch_scratch_alloc size amax_v / amax_i
  float* pv = t.up(nullptr, rows * 64);
  int* pi = (int*)up_bytes(t, nullptr, rows * 64 * 4);
  int* next = (int*)up_bytes(t, nullptr, rows * 4);
  if (!dl || !pv || !pi || !next) return LGH_ALLOCATION_FAILED;
  hipStream_t st = t.c->stream;
  if (!pf_poison(t.c, pv, rows * 64 * 4, 0x7FC0BEEFu) || hipMemsetAsync(pi, 0xFF, rows * 64 * 4, st) != hipSuccess ||
      hipMemsetAsync(next, 0xFF, rows * 4, st) != hipSuccess)
    return LGH_OPERATION_FAILED;
  if (n_seq == 0) {   // the greedy step's: the token goes to the state words
    if (argmax_launch(dl, (uint32_t)n, pv, pi, t.c->state, nullptr, st) != hipSuccess) return LGH_OPERATION_FAILED;
    int words[ST_WORDS];
    if (int rc = down_bytes(t, words, t.c->state, sizeof(words))) return rc;
    if (words[ST_TOKEN] != words[ST_ARGMAX]) return LGH_OPERATION_FAILED;   // (the token fed back is the arg-max)
    tokens_out[0] = words[ST_ARGMAX];
    return LGH_OK;
  }
  if (argmax_multi_launch(dl, (uint32_t)n, (uint32_t)n_seq, pv, pi, next, st) != hipSuccess) return LGH_OPERATION_FAILED;
  return down_bytes(t, tokens_out, next, n_seq * 4);
}

}  // extern "C"
