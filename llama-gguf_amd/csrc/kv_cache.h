// kv_cache.h — the one description of a layer's KV cache, for every kv_cache_type and both decode engines (the context's own sequence
// and the slots of the multi-sequence engine).  Host-only plain C++: sizes, strides and pointers, no HIP calls.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/llama_gguf_hip.h"

namespace lgh {

uint32_t tq_row_bytes_host(int bits, uint32_t d);   // attention_tq.hip: the packed codes of one TurboQuant row

// the tensors a layer's cache can have, each [slot][kv head][max_seq][bytes per position]
enum KvKind { KV_K = 0, KV_V, KV_KSCALE, KV_VSCALE, KV_KX, KV_KINDS };

// A cache format's arithmetic, from (kv_cache_type, num_kv_heads, max_seq_len, head_dim):
//   f32     K / V rows [kv_heads, max_seq, head_dim] (gpu_only.rs:555-572)
//   int8    QuantizedKVCache::new (kv_quantized.rs:57-102): byte rows + an f32 scale per (kv head, position); the FP8 formats have no
//           scales (kv_quantized.rs:31-35)
//   TQ      TurboQuantKVCache::new (kv_turboquant.rs:36-86): packed codes, no scales, no norms; with QJL + per K row the sign bits of
//           the projected residual and its norm (quant.rs:176-186)
struct KvLayout {
  uint32_t type, n_kv, max_seq, d;
  KvLayout(uint32_t type_ = LGH_KV_F32, size_t n_kv_ = 0, size_t max_seq_ = 0, size_t d_ = 0)
      : type(type_), n_kv((uint32_t)n_kv_), max_seq((uint32_t)max_seq_), d((uint32_t)d_) {}
  explicit KvLayout(const lgh_model_desc& m) : KvLayout(m.kv_cache_type, m.num_kv_heads, m.max_seq_len, m.head_dim) {}

  bool f32() const { return type == LGH_KV_F32; }
  // every other format: the current token's K / V rows stay f32 in kv_tmp, the attention launch compresses and stores them
  bool staged() const { return !f32(); }
  bool tq() const { return type >= LGH_KV_TQ2 && type <= LGH_KV_TQ3_QJL; }
  bool qjl() const { return type == LGH_KV_TQ2_QJL || type == LGH_KV_TQ3_QJL; }
  bool has_scales() const { return type == LGH_KV_INT8; }
  int tq_bits() const { return type == LGH_KV_TQ2 || type == LGH_KV_TQ2_QJL ? 2 : 3; }

  // per (kv head, position): one K or V row, its scale, the K row's QJL words (sign bits, then the residual norm)
  size_t row_bytes() const { return f32() ? (size_t)d * 4 : tq() ? tq_row_bytes_host(tq_bits(), d) : d; }
  size_t scale_bytes() const { return has_scales() ? 4 : 0; }
  size_t qjl_bytes() const { return qjl() ? (size_t)(d / 32 + 1) * 4 : 0; }
  size_t pos_bytes(int kind) const { return kind <= KV_V ? row_bytes() : kind <= KV_VSCALE ? scale_bytes() : qjl_bytes(); }

  // per slot of one layer
  size_t rows() const { return (size_t)n_kv * max_seq; }
  size_t slot_bytes(int kind) const { return rows() * pos_bytes(kind); }
  size_t slot_bytes() const { return rows() * (2 * (row_bytes() + scale_bytes()) + qjl_bytes()); }

  // the distance between two slots' tensors, in the units the kernels take: floats (MvBatch::cache_stride — the multi-sequence mat-vec
  // carries it whatever the format — and the f32 attention), code bytes and QJL words (the TurboQuant attention; the words for every TQ
  // format).  attn_split_launch (common.h) reads them here; no caller passes a stride
  uint64_t stride_floats() const { return (uint64_t)rows() * d; }
  uint64_t stride_bytes() const { return staged() ? (uint64_t)rows() * row_bytes() : 0; }
  uint64_t stride_words() const { return tq() ? (uint64_t)rows() * (d / 32 + 1) : 0; }

  // The accounting's two byte counts of attention over kv_len cached rows.  They differ for the QJL formats: the step count takes the
  // code rows only, the profiling record adds the K rows' QJL words and the projection matrices.
  //   lgh_get_stats' step_alg_bytes: kv_len rows read + the current row written, K and V, with their scales
  uint64_t step_alg_bytes(uint64_t kv_len) const { return (uint64_t)2 * n_kv * (kv_len + 1) * (row_bytes() + scale_bytes()); }
  //   attention_forward's profiling record: what the launch reads
  uint64_t launch_bytes(uint64_t kv_len) const {
    return (uint64_t)n_kv * kv_len * (2 * (row_bytes() + scale_bytes()) + qjl_bytes()) + (qjl() ? (uint64_t)n_kv * d * d * 4 : 0);
  }
};

// One layer's cache tensors, for 1 or N slots, by KvKind (null: the format has no such tensor; KvLayout says how large the others
// are): K / V rows in the format's element type, the int8 rows' scales, the K rows' QJL words
struct KvCache {
  void* t[KV_KINDS] = {};
  float* k_f32() const { return (float*)t[KV_K]; }
  float* v_f32() const { return (float*)t[KV_V]; }
  int8_t* k_i8() const { return (int8_t*)t[KV_K]; }
  int8_t* v_i8() const { return (int8_t*)t[KV_V]; }
  uint8_t* k_bytes() const { return (uint8_t*)t[KV_K]; }
  uint8_t* v_bytes() const { return (uint8_t*)t[KV_V]; }
  float* kscale() const { return (float*)t[KV_KSCALE]; }
  float* vscale() const { return (float*)t[KV_VSCALE]; }
  uint32_t* kx() const { return (uint32_t*)t[KV_KX]; }
  KvCache slot(const KvLayout& l, size_t s) const {   // slot s of a cache of several
    KvCache o;
    for (int kind = 0; kind < KV_KINDS; kind++)
      if (t[kind]) o.t[kind] = (uint8_t*)t[kind] + s * l.slot_bytes(kind);
    return o;
  }
};

}  // namespace lgh
