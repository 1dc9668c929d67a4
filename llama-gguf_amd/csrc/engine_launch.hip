// engine_launch.hip — what every launch sequence of the engine is built from: error plumbing and tracked allocations, weight upload
// into the device layouts, the profiling drain, the XQ registry, the fused mat-vec launch assembly (build_mv_group, launch_mv,
// linear_any) and graph capture.
#include "engine.h"
#include "xq.h"

#include <algorithm>
#include <cstring>

using namespace lgh;

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
int fail(lgh_ctx* c, int status, const std::string& msg) {
  if (c) c->err = msg;
  return status;
}

int dev_alloc(lgh_ctx* c, void** p, size_t bytes) {
  if (bytes == 0) bytes = 4;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) return fail(c, LGH_ALLOCATION_FAILED, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
  c->allocs.push_back(*p);
  return LGH_OK;
}

// An entry of size 0 is skipped and its pointer stays null (pf_ensure and the per-format KV tables rely on it).  The scratch
// tables of lgh_finalize, lgh_batch_create and samp_alloc used to get a 4-byte buffer for such an entry; none of theirs is 0 for
// a model that passes engine_shape_check.
int alloc_zeroed(lgh_ctx* c, const AllocSpec* bufs, size_t count, uint64_t& counter) {
  for (size_t i = 0; i < count; i++) {
    const AllocSpec& b = bufs[i];
    if (!b.n) continue;
    if (int rc = dev_alloc(c, b.p, b.n)) return rc;
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetAsync(*b.p, 0, b.n, c->stream));
    counter += b.n;
  }
  return LGH_OK;
}

// The tensors the format has (KvLayout), each for n_slots sequences; the others stay null.  lgh_finalize: the own sequence's,
// batch_scratch_alloc: the slots'
int kv_alloc(lgh_ctx* c, size_t n_slots, KvCache& kv) {
  AllocSpec bufs[KV_KINDS];
  for (int kind = 0; kind < KV_KINDS; kind++) bufs[kind] = {&kv.t[kind], n_slots * c->kvl.slot_bytes(kind)};
  return alloc_zeroed(c, bufs, KV_KINDS, c->stats.kv_bytes);
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------------
// device layouts
// ------------------------------------------------------------------------------------------------
LayoutInfo layout_for(int src_type) {
  switch (src_type) {
    case LGH_TYPE_Q4_K: return {LGH_TYPE_Q4_K, 1, {144, 0, 0, 0}, 256};
    case LGH_TYPE_Q5_K: return {LGH_TYPE_Q5_K, 1, {176, 0, 0, 0}, 256};
    case LGH_TYPE_Q6_K: return {LGH_TYPE_Q6_K, 4, {128, 64, 16, 2}, 256};
    case LGH_TYPE_Q8_0: return {LGH_TYPE_Q8_0, 2, {32, 2, 0, 0}, 32};
    case LGH_TYPE_Q4_0: return {LGH_TYPE_Q4_0, 2, {16, 2, 0, 0}, 32};
    default: return {LGH_TYPE_F32, 1, {4, 0, 0, 0}, 1};
  }
}

bool fused_type(int t) {
  return mfma_type(t) || t == LGH_TYPE_Q4_K || t == LGH_TYPE_Q5_K || t == LGH_TYPE_Q6_K || t == LGH_TYPE_Q8_0 || t == LGH_TYPE_Q4_0;
}

// Upload one matrix (or expert `slot` of a stack, or the whole stack when slot < 0) given in native
// GGUF order.  The first call for a DevWeight allocates it.
int upload_matrix(lgh_ctx* c, DevWeight& W, int src_type, uint32_t k, uint32_t n, uint32_t n_stack, int slot,
                         const void* host, size_t nbytes) {
  const uint32_t sbe = blk_elems(src_type), sbb = blk_bytes(src_type);
  if (!sbe) return fail(c, LGH_UNSUPPORTED_DTYPE, "unsupported ggml type " + std::to_string(src_type));
  if (k % sbe) return fail(c, LGH_SHAPE_MISMATCH, "in_features not a multiple of the block size");
  LayoutInfo li = layout_for(src_type);
  const uint64_t per_expert_src = (uint64_t)n * (k / sbe) * sbb;
  const uint32_t n_in_payload = slot < 0 ? n_stack : 1;
  if (nbytes != per_expert_src * n_in_payload) return fail(c, LGH_SHAPE_MISMATCH, "tensor byte size does not match its shape");
  uint64_t blocks_per_expert = (uint64_t)n * (k / li.belems);
  // int8-MFMA tile layouts (16 rows x 256 elements, rows padded to 16) for the five fused formats when k allows it
  const bool t16 = k % 256 == 0 && (src_type == LGH_TYPE_Q4_K || src_type == LGH_TYPE_Q6_K || src_type == LGH_TYPE_Q5_K ||
                                    src_type == LGH_TYPE_Q8_0 || src_type == LGH_TYPE_Q4_0);
  if (t16) {
    li.nplanes = 1;
    li.belems = 256;
    li.bpb[1] = li.bpb[2] = li.bpb[3] = 0;
    switch (src_type) {   // bytes per row-block = tile bytes / 16
      case LGH_TYPE_Q4_K: li.dev_type = kDevQ4K_T16; li.bpb[0] = 144; break;
      case LGH_TYPE_Q6_K: li.dev_type = kDevQ6K_T16; li.bpb[0] = 212; break;
      case LGH_TYPE_Q5_K: li.dev_type = kDevQ5K_T16; li.bpb[0] = 176; break;
      case LGH_TYPE_Q8_0: li.dev_type = kDevQ80_T16; li.bpb[0] = 272; break;
      default: li.dev_type = kDevQ40_T16; li.bpb[0] = 144; break;
    }
    blocks_per_expert = (uint64_t)((n + 15) / 16) * 16 * (k / 256);
  }
  if (!W.present()) {
    uint64_t off = 0;
    uint64_t plane_off[4] = {0, 0, 0, 0};
    for (int p = 0; p < li.nplanes; p++) {
      plane_off[p] = off;
      W.stack_stride[p] = blocks_per_expert * li.bpb[p];
      off = align_up(off + W.stack_stride[p] * n_stack, 256);
    }
    void* base = nullptr;
    int rc = dev_alloc(c, &base, off + 256);
    if (rc) return rc;
    W.base = (uint8_t*)base;
    for (int p = 0; p < li.nplanes; p++) W.plane[p] = W.base + plane_off[p];
    W.type = li.dev_type;
    W.src_type = src_type;
    W.k = k; W.n = n; W.n_stack = n_stack;
    W.bytes = 0;
    for (int p = 0; p < li.nplanes; p++) W.bytes += W.stack_stride[p];  // per expert
    if (t16) W.bytes = per_expert_src;                                  // algorithmic bytes exclude the row padding
    c->stats.weight_bytes += (li.dev_type == LGH_TYPE_F32 ? (uint64_t)n * k * 4 : per_expert_src) * n_stack;
    W.filled.assign(n_stack, false);
  } else if (W.src_type != src_type || W.k != k || W.n != n || W.n_stack != n_stack) {
    return fail(c, LGH_SHAPE_MISMATCH, "expert tensors of one stack differ in type or shape");
  }
  const uint32_t e0 = slot < 0 ? 0 : (uint32_t)slot;
  for (uint32_t i = 0; i < n_in_payload; i++) W.filled[e0 + i] = true;   // lgh_finalize refuses a stack with an empty slot
  if (li.dev_type == src_type && li.nplanes == 1 && !t16) {  // native layout: straight copy
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy((void*)(W.plane[0] + (uint64_t)e0 * W.stack_stride[0]), host, nbytes, hipMemcpyHostToDevice));
    return LGH_OK;
  }
  void* raw = nullptr;
  HIP_TRY(c, LGH_ALLOCATION_FAILED, hipMalloc(&raw, nbytes));
  hipError_t e = hipMemcpy(raw, host, nbytes, hipMemcpyHostToDevice);
  for (uint32_t i = 0; i < n_in_payload && e == hipSuccess; i++) {
    const uint8_t* src = (const uint8_t*)raw + (uint64_t)i * per_expert_src;
    if (li.dev_type == LGH_TYPE_F32) {
      e = dequant_launch(src_type, src, (float*)(W.plane[0] + (uint64_t)(e0 + i) * W.stack_stride[0]), (uint64_t)n * k, c->stream);
    } else if (t16) {
      e = repack_t16_launch(li.dev_type, src, W.base + (uint64_t)(e0 + i) * W.stack_stride[0], n, k / 256, c->stream);
    } else {
      uint64_t po[4];
      for (int p = 0; p < 4; p++) po[p] = (uint64_t)(W.plane[p] - W.base) + (uint64_t)(e0 + i) * W.stack_stride[p];
      e = repack_launch(src_type, src, W.base, po, blocks_per_expert, c->stream);
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(raw);
  if (e != hipSuccess) return fail(c, LGH_OPERATION_FAILED, std::string("weight re-layout: ") + hipGetErrorString(e));
  return LGH_OK;
}

// 1-D tensors (norm weights, biases) and the f32 router matrix: always f32 on device
int upload_f32(lgh_ctx* c, float** dst, int src_type, uint64_t n, const void* host, size_t nbytes) {
  const uint32_t sbe = blk_elems(src_type), sbb = blk_bytes(src_type);
  if (!sbe || n % sbe || nbytes != n / sbe * sbb) return fail(c, LGH_SHAPE_MISMATCH, "vector byte size does not match its shape");
  if (!*dst) {
    int rc = dev_alloc(c, (void**)dst, n * 4);
    if (rc) return rc;
    c->stats.weight_bytes += n * 4;
  }
  if (src_type == LGH_TYPE_F32) {
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy(*dst, host, nbytes, hipMemcpyHostToDevice));
    return LGH_OK;
  }
  void* raw = nullptr;
  HIP_TRY(c, LGH_ALLOCATION_FAILED, hipMalloc(&raw, nbytes));
  hipError_t e = hipMemcpy(raw, host, nbytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = dequant_launch(src_type, (const uint8_t*)raw, *dst, n, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(raw);
  if (e != hipSuccess) return fail(c, LGH_OPERATION_FAILED, std::string("vector upload: ") + hipGetErrorString(e));
  return LGH_OK;
}

int drain_prof(lgh_ctx* c) {
  if (c->prof.empty()) return LGH_OK;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  for (auto& r : c->prof) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess && r.cls < 0) {
      const double n = (double)c->stats.event_bracket_samples;
      c->stats.event_bracket_us = (c->stats.event_bracket_us * n + (double)ms * 1000.0) / (n + 1.0);
      c->stats.event_bracket_samples += 1;
    } else if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      c->stats.k_time_us[r.cls] += (double)ms * 1000.0;
      c->stats.k_launches[r.cls] += 1;
      c->stats.k_alg_bytes[r.cls] += r.bytes;
      c->stats.sym_time_us[r.sym] += (double)ms * 1000.0;
      c->stats.sym_launches[r.sym] += 1;
      c->stats.sym_alg_bytes[r.sym] += r.bytes;
    }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  c->prof.clear();
  return LGH_OK;
}

// ------------------------------------------------------------------------------------------------
// XQ images of activation buffers (xq.h)
// ------------------------------------------------------------------------------------------------
XqBuf* xq_get(lgh_ctx* c, const float* f32, uint32_t k) {
  for (auto& q : c->xqs)
    if (q.f32 == f32 && q.k >= k) return &q;
  XqBuf q;
  q.f32 = f32;
  q.k = k;
  if (dev_alloc(c, (void**)&q.xq, xq_bytes(k)) || dev_alloc(c, (void**)&q.ssq, (size_t)(k / 16 + 64) * 4)) return nullptr;
  c->xqs.push_back(q);
  return &c->xqs.back();
}
XqBuf* xq_find(lgh_ctx* c, const float* f32) {
  for (auto& q : c->xqs)
    if (q.f32 == f32) return &q;
  return nullptr;
}
void xq_stale(lgh_ctx* c, const float* f32) {
  if (XqBuf* q = xq_find(c, f32)) q->fresh = false;
}

static uint32_t g_launch_seq = 0;   // diagnostic builds: consecutive launches get consecutive span slots
// Assembles the launch descriptor of one group of segments (and keeps the XQ bookkeeping: images this launch consumes are
// converted here if their producer did not leave them; images it produces are marked fresh).
// `tile_cap` (multi-sequence launches, engine_batch.hip): at most that many 16-row tiles per workgroup — the partial sums of
// every sequence of the step must fit LDS.  It changes which workgroup computes a row, never the row's arithmetic.
int build_mv_group(lgh_ctx* c, const SegSpec* specs, int nseg, const float* norm_w, uint32_t k, bool mfma, MvLaunch& L,
                   uint32_t& wg, uint32_t& threads, uint64_t& alg, uint32_t tile_cap) {
  std::memset(&L, 0, sizeof(L));
  L.nseg = nseg;
  L.k = k;
  L.do_norm = norm_w != nullptr;
  L.eps = c->d.norm_eps;
  L.norm_w = norm_w;
  L.pos = c->state + ST_POS;
  L.rope_cs = c->rope_cs;
  L.dbg_slot = g_launch_seq++ & 63u;
  wg = 0; threads = 0; alg = 0;
  uint32_t launch_rows = 0;
  uint32_t wave_cap = 16;
  for (int s = 0; s < nseg; s++) {
    launch_rows += specs[s].W[0]->n;
    if (!mfma) wave_cap = std::min(wave_cap, mv_wave_cap(specs[s].W[0]->type));
  }
  if (!mfma && nseg > 1) {  // mixed-type launches run in the 512-thread instantiations
    for (int s = 1; s < nseg; s++)
      if (specs[s].W[0]->type != specs[0].W[0]->type) wave_cap = std::min(wave_cap, 8u);
  }
  // A fused launch over formats with different bytes per tile (the "_M" mixes: Q and K in Q4_K, V in Q6_K) is as long as its
  // heaviest workgroup: the segments in the heavier format get fewer tiles per workgroup, as long as the launch still fits one
  // workgroup per CU.  (Llama-3-8B QKV: 2 / 2 / 1 tiles -> 224 workgroups whose heaviest streams 2 x 2304 B per block instead
  // of 192 whose heaviest streams 2 x 3392.)
  uint32_t force_tiles[3] = {0, 0, 0};
  if (mfma && nseg > 1) {
    uint32_t R[3], Gs[3], tiles[3], w[3];
    bool ok = true, mixed = false;
    for (int s = 0; s < nseg && ok; s++) {
      const DevWeight& W0 = *specs[s].W[0];
      MvPlan p;
      ok = mvq_plan(W0.k, W0.n, specs[s].npass, &p, launch_rows) == hipSuccess;
      R[s] = p.rows_per_wg / 16; Gs[s] = p.G; tiles[s] = (W0.n + 15) / 16;
      w[s] = mvq_tile_bytes(W0.type) * (uint32_t)specs[s].npass;
      ok = ok && w[s] != 0;
      mixed = mixed || w[s] != w[0];
    }
    for (int it = 0; ok && mixed && it < 32; it++) {
      int h = 0;
      for (int s = 1; s < nseg; s++)
        if ((uint64_t)R[s] * w[s] > (uint64_t)R[h] * w[h]) h = s;
      if (R[h] < 2 * Gs[h]) break;                                    // (a workgroup keeps at least one tile per row group)
      uint32_t wgs = 0;
      for (int s = 0; s < nseg; s++) { const uint32_t r = s == h ? R[h] - Gs[h] : R[s]; wgs += (tiles[s] + r - 1) / r; }
      if (wgs > (uint32_t)kNumCU) break;
      R[h] -= Gs[h];
    }
    if (ok && mixed)
      for (int s = 0; s < nseg; s++) force_tiles[s] = R[s];
  }
  if (mfma && tile_cap) {
    for (int s = 0; s < nseg; s++) {
      const DevWeight& W0 = *specs[s].W[0];
      MvPlan p;
      if (mvq_plan(W0.k, W0.n, specs[s].npass, &p, launch_rows, force_tiles[s]) != hipSuccess) continue;
      if (p.rows_per_wg / 16 > tile_cap) force_tiles[s] = std::max(p.G, tile_cap / p.G * p.G);
    }
  }
  for (int s = 0; s < nseg; s++) {
    const SegSpec& sp = specs[s];
    const DevWeight& W0 = *sp.W[0];
    MvPlan plan;
    hipError_t pe = mfma ? mvq_plan(W0.k, W0.n, sp.npass, &plan, launch_rows, force_tiles[s])
                         : mv_plan(W0.type, W0.k, W0.n, sp.npass, &plan, launch_rows, wave_cap);
    if (pe != hipSuccess)
      return fail(c, LGH_UNSUPPORTED, "no fused mat-vec plan for type " + std::to_string(W0.type) + " k=" + std::to_string(W0.k));
    MvSeg& S = L.seg[s];
    S.type = W0.type;
    S.epi = sp.epi;
    S.n_rows = W0.n;
    S.nblk = mfma ? W0.k / 256 : W0.k / layout_for(W0.src_type).belems;
    S.units = plan.units; S.T = plan.T; S.G = plan.G;
    S.rows_per_wg = plan.rows_per_wg;
    S.wg_begin = wg;
    S.npass = sp.npass;
    for (int p = 0; p < sp.npass; p++) {
      const DevWeight& W = *sp.W[p];
      if (W.type != W0.type || W.k != W0.k || W.n != W0.n) return fail(c, LGH_SHAPE_MISMATCH, "passes of one segment differ in type/shape");
      for (int i = 0; i < 4; i++) { S.pass[p].plane[i] = W.plane[i]; S.pass[p].sel_stride[i] = W.stack_stride[i]; }
      S.pass[p].x = sp.x[p];
      S.pass[p].sel = sp.sel[p];
      if (mfma) {   // the input vector as XQ records: left by its producer, or converted here
        XqBuf* q = xq_get(c, sp.x[p], k);
        if (!q) return fail(c, LGH_ALLOCATION_FAILED, "XQ image allocation failed");
        if (!q->fresh || q->tag != norm_w) {
          int rq = run_k(c, LGH_K_MISC, LGH_SYM_OTHER, (uint64_t)k * 4, [&] {
            return xq_quantize_launch(sp.x[p], norm_w, q->xq, norm_w ? q->ssq : nullptr, k, c->stream);
          });
          if (rq) return rq;
          q->fresh = true;
          q->tag = norm_w;
        }
        S.pass[p].xq = q->xq;
        if (norm_w) { L.ssq_part = q->ssq; L.n_ssq_part = k / 16; }
      }
      alg += W.bytes;
    }
    S.out = sp.out; S.out2 = sp.out2; S.resid = sp.resid; S.bias = sp.bias; S.moe_w = sp.moe_w;
    {  // XQ image of the output for the next consumer, where this epilogue can write one
      XqBuf* qo = sp.out ? xq_find(c, sp.out) : nullptr;
      const bool can = sp.xq_next && qo && W0.n % 16 == 0 && W0.n <= qo->k && plan.rows_per_wg % 16 == 0 &&   // thread t <-> row t, chunk-aligned
                       (sp.epi == EPI_STORE || sp.epi == EPI_RESID || sp.epi == EPI_SWIGLU || sp.epi == EPI_MOE_DOWN);
      if (can) {
        S.xq_out = qo->xq;
        S.xq_nw = sp.xq_next == 2 ? sp.xq_next_nw : nullptr;
        S.xq_ssq = sp.xq_next == 2 ? qo->ssq : nullptr;
        qo->fresh = true;
        qo->tag = S.xq_nw;
      } else if (sp.xq_next && qo && sp.epi == EPI_MOE_SWIGLU && W0.n % 16 == 0 && W0.n <= qo->k && plan.rows_per_wg % 16 == 0) {
        XqBuf* q2 = sp.out2 ? xq_find(c, sp.out2) : nullptr;
        S.xq_out = qo->xq;
        qo->fresh = true; qo->tag = nullptr;
        if (q2 && sp.npass > 2) { S.xq_out2 = q2->xq; q2->fresh = true; q2->tag = nullptr; }
      } else if (qo && sp.epi != EPI_ROPE_K && sp.epi != EPI_V_CACHE) {
        qo->fresh = false;
      }
      if (sp.out2 && !S.xq_out2) xq_stale(c, sp.out2);
    }
    S.head_dim = c->d.head_dim;
    S.max_seq = c->d.max_seq_len;
    wg += plan.n_wg;
    if (plan.threads > threads) threads = plan.threads;
    if (plan.red_floats > L.red_floats) L.red_floats = plan.red_floats;
  }
  alg += (uint64_t)k * 4 * (norm_w ? 2 : 1);
  return LGH_OK;
}

static int mvq_symbol(const MvLaunch& L) {
  bool has[8] = {false, false, false, false, false, false, false, false};
  for (int s = 0; s < L.nseg; s++) {
    const int t = L.seg[s].type;
    has[t == kDevQ4K_T16 ? 0 : t == kDevQ6K_T16 ? 1 : t == kDevQ5K_T16 ? 2 : t == kDevQ80_T16 ? 3 : 4] = true;
  }
  return has[2] ? LGH_SYM_MVQ_Q5K : (has[3] || has[4]) ? LGH_SYM_MVQ_Q80_Q40 : (has[0] && has[1]) ? LGH_SYM_MVQ_MIXED
         : has[1] ? LGH_SYM_MVQ_Q6K : LGH_SYM_MVQ_Q4K;
}

static int launch_mv_group(lgh_ctx* c, int cls, const SegSpec* specs, int nseg, const float* norm_w, uint32_t k, bool mfma) {
  MvLaunch L;
  uint32_t wg, threads;
  uint64_t alg;
  int rc = build_mv_group(c, specs, nseg, norm_w, k, mfma, L, wg, threads, alg, 0);
  if (rc) return rc;
  if (specs[0].amax_parts) *specs[0].amax_parts = 0;
  if (mfma) {
    // (a static launch plan, where the table of matvec_mfma.hip has one for this geometry; asked to, the output projection of a
    // greedy step then also leaves the arg-max parts of its workgroups)
    if (nseg == 1) { L.amax_v = specs[0].amax_v; L.amax_i = specs[0].amax_i; }
    bool amax_done = false;
    rc = run_k(c, cls, mvq_symbol(L), alg, [&] { return mvq_launch(L, wg, threads, c->stream, (c->d.flags & LGH_FLAG_MV_GENERIC) != 0, &amax_done); });
    if (!rc && amax_done && specs[0].amax_parts) *specs[0].amax_parts = wg;
    return rc;
  }
  return run_k(c, cls, mv_symbol(L), alg, [&] { return mv_launch(L, wg, threads, c->stream); });
}

// The formats that have a common instantiation: Q4_K + Q6_K, Q5_K + Q6_K (the "_M" mixes).
bool mv_formats_split(const SegSpec* specs, int nseg) {
  bool q4 = false, q5 = false, other = false, uniform = true;
  for (int s = 0; s < nseg; s++) {
    const int t = specs[s].W[0]->type;
    q4 |= t == kDevQ4K_T16; q5 |= t == kDevQ5K_T16; other |= t == kDevQ80_T16 || t == kDevQ40_T16;
    uniform &= t == specs[0].W[0]->type;
  }
  return !uniform && ((q4 && q5) || other);
}

// Segments are independent (disjoint outputs), so a launch whose matrices live in different kernel families
// (Q4_K on the matrix cores, the rest on the VALU kernel) is issued as one launch per family.
int launch_mv(lgh_ctx* c, int cls, const SegSpec* specs, int nseg, const float* norm_w, uint32_t k) {
  SegSpec a[3], b[3];
  int na = 0, nb = 0;
  for (int s = 0; s < nseg; s++) {
    if (mfma_type(specs[s].W[0]->type)) a[na++] = specs[s];
    else b[nb++] = specs[s];
  }
  int rc = LGH_OK;
  if (mv_formats_split(a, na)) {
    for (int s = 0; s < na; s++)
      if ((rc = launch_mv_group(c, cls, a + s, 1, norm_w, k, true))) return rc;
    na = 0;
  }
  if (na && (rc = launch_mv_group(c, cls, a, na, norm_w, k, true))) return rc;
  if (nb && (rc = launch_mv_group(c, cls, b, nb, norm_w, k, false))) return rc;
  return rc;
}

// one Linear with optional norm prologue / residual epilogue, any device type
int linear_any(lgh_ctx* c, int cls, const DevWeight& W, const float* x, float* out, const float* norm_w,
                      const float* resid, const float* bias, int xq_next, const float* xq_next_nw, float* amax_v, int* amax_i, uint32_t* amax_parts) {
  if (amax_parts) *amax_parts = 0;
  if (fused_type(W.type)) {
    SegSpec sp;
    sp.W[0] = &W; sp.x[0] = x;
    sp.epi = resid ? EPI_RESID : EPI_STORE;
    sp.out = out; sp.resid = resid; sp.bias = bias;
    sp.xq_next = xq_next; sp.xq_next_nw = xq_next_nw;
    sp.amax_v = amax_v; sp.amax_i = amax_i; sp.amax_parts = amax_parts;
    return launch_mv(c, cls, &sp, 1, norm_w, W.k);
  }
  xq_stale(c, out);
  if (bias) return fail(c, LGH_UNSUPPORTED, "bias on a non-quantized linear layer is not supported");
  return run_k(c, cls, LGH_SYM_F32_MATVEC, (uint64_t)W.n * W.k * 4, [&] {
    return f32_matvec_launch((const float*)W.plane[0], x, out, W.k, W.n, norm_w, c->d.norm_eps, resid, c->stream);
  });
}

// ------------------------------------------------------------------------------------------------
// graph capture
// ------------------------------------------------------------------------------------------------
int capture_graph(lgh_ctx* c, hipGraphExec_t* exec, const std::function<int()>& enqueue, size_t* n_nodes) {
  hipGraph_t g = nullptr;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  int rc = enqueue();
  hipError_t e = hipStreamEndCapture(c->stream, &g);
  if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
  if (e != hipSuccess) return fail(c, LGH_OPERATION_FAILED, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
  if (n_nodes) (void)hipGraphGetNodes(g, nullptr, n_nodes);
  e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return fail(c, LGH_OPERATION_FAILED, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
  return LGH_OK;
}
