/*
 * include/llama_gguf_hip.h — C ABI of the MI355X (gfx950) GPU-resident decode engine for llama-gguf.
 *
 * This is the drop-in boundary.  The reference (Lexmata/llama-gguf v0.14.0, Rust; paths below are
 * relative to /root/reference) talks to every GPU engine through
 *
 *     pub trait GpuInference: Send {                       // src/backend/mod.rs:283-296
 *         fn forward(&mut self, token_id: u32) -> BackendResult<Vec<f32>>;
 *         fn prefill_token(&mut self, token_id: u32) -> BackendResult<()>;
 *         fn reset(&mut self);
 *         fn position(&self) -> usize;
 *     }
 *     pub fn from_model(model: LlamaModel, max_seq_len: usize) -> BackendResult<Self>
 *                                                          // src/backend/cuda/gpu_only.rs:426
 *
 * and adapts it to `trait Model` with GpuModelWrapper (src/backend/mod.rs:302-364).  A Rust
 * `impl GpuInference for HipGpuInference` binds the lgh_* entry points below 1:1 (binding shown in
 * INTEGRATION.md); each declaration cites the reference item it replaces.
 *
 * Conventions: plain pointers and sizes, opaque handle, `int` status (0 = ok).  Status codes map
 * 1:1 onto the reference's BackendError variants (src/backend/error.rs:3-37).  The library keeps no
 * thread-local state and binds its device on every call, so a context may be used from any one
 * thread at a time (the reference serialises access with a Mutex, src/backend/mod.rs:303,328-332).
 * All tensor payloads are handed over in NATIVE GGUF order (a weight [in, out] is `out` rows of
 * in/block_size blocks, src/backend/cpu/ops.rs:1120-1122); the library owns any device re-layout.
 */
#ifndef LLAMA_GGUF_HIP_H
#define LLAMA_GGUF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* BackendError variants, src/backend/error.rs:3-37 */
typedef enum lgh_status {
  LGH_OK = 0,
  LGH_NOT_AVAILABLE = 1,         /* BackendError::NotAvailable         (no HIP device) */
  LGH_SHAPE_MISMATCH = 2,        /* BackendError::ShapeMismatch */
  LGH_DTYPE_MISMATCH = 3,        /* BackendError::DTypeMismatch */
  LGH_UNSUPPORTED_DTYPE = 4,     /* BackendError::UnsupportedDType */
  LGH_UNSUPPORTED = 5,           /* BackendError::Unsupported */
  LGH_INVALID_ARGUMENT = 6,      /* BackendError::InvalidArgument      (incl. pos >= max_seq_len) */
  LGH_TENSOR_ERROR = 7,          /* BackendError::Tensor(_) */
  LGH_INITIALIZATION_FAILED = 8, /* BackendError::InitializationFailed */
  LGH_ALLOCATION_FAILED = 9,     /* BackendError::AllocationFailed */
  LGH_OPERATION_FAILED = 10      /* BackendError::OperationFailed      (launch / sync / copy) */
} lgh_status;

/* ggml type ids, src/gguf/constants.rs:92-126 */
typedef enum lgh_ggml_type {
  LGH_TYPE_F32 = 0, LGH_TYPE_F16 = 1, LGH_TYPE_Q4_0 = 2, LGH_TYPE_Q4_1 = 3, LGH_TYPE_Q5_0 = 6,
  LGH_TYPE_Q5_1 = 7, LGH_TYPE_Q8_0 = 8, LGH_TYPE_Q8_1 = 9, LGH_TYPE_Q2_K = 10, LGH_TYPE_Q3_K = 11,
  LGH_TYPE_Q4_K = 12, LGH_TYPE_Q5_K = 13, LGH_TYPE_Q6_K = 14, LGH_TYPE_Q8_K = 15, LGH_TYPE_BF16 = 30
} lgh_ggml_type;

/* What GpuOnlyInference::from_model reads out of ModelConfig and the per-layer Attention scalars
 * (src/backend/cuda/gpu_only.rs:488-502, 527-533, 555-572; src/model/layers.rs:262-298). */
typedef struct lgh_model_desc {
  uint32_t struct_size;              /* sizeof(lgh_model_desc), for ABI evolution */
  uint32_t hidden_size;
  uint32_t intermediate_size;
  uint32_t num_layers;               /* layers of the WHOLE model */
  uint32_t num_heads;
  uint32_t num_kv_heads;
  uint32_t head_dim;                 /* key_length == value_length */
  uint32_t vocab_size;
  uint32_t max_seq_len;              /* KV capacity (the engine's gpu_seq_len, src/engine.rs:554-564) */
  uint32_t num_experts;              /* 0 = dense FFN */
  uint32_t num_experts_per_token;
  uint32_t expert_intermediate_size;
  uint32_t use_neox_rope;            /* RopeType::NeoX vs Normal, src/model/loader.rs:145-162 */
  float norm_eps;
  float rope_freq_base;
  float rope_freq_scale;
  int32_t device_id;                 /* HIP device ordinal */
  /* pipeline stage (src/distributed/pipeline.rs:50-96 partitioning): this context owns layers
   * [layer_begin, layer_end); 0,0 means all.  The first stage owns the embedding, the last one the
   * final norm + output projection. */
  uint32_t layer_begin;
  uint32_t layer_end;
  uint32_t flags;                    /* LGH_FLAG_* */
  uint32_t kv_cache_type;            /* LGH_KV_*.  What the reference's `--kv-cache-type` can select is KVCacheType::{F32, TurboQuantMSE,
                                        TurboQuantProd} (src/config.rs:808-817): LGH_KV_F32, LGH_KV_TQ2 / TQ3, LGH_KV_TQ2_QJL / TQ3_QJL here.
                                        LGH_KV_INT8 / FP8_* are the formats of QuantizedKVCache (src/model/kv_quantized.rs:
                                        11-20), which the reference exports (model/mod.rs:31, lib.rs:77) but which NO forward path and no
                                        CLI flag of it reaches; they are offered for hosts that use that cache type directly.
                                        0 = f32, or int8 when LGH_FLAG_KV_INT8 is set (the field was added after the flag) */
} lgh_model_desc;

enum {
  LGH_KV_F32 = 0,
  LGH_KV_INT8 = 1,                   /* int8 rows + one f32 scale per (kv head, position) */
  LGH_KV_FP8_E4M3 = 2,               /* one byte per element, no scales: the reference's quantize_fp8_e4m3 (mantissa truncated) */
  LGH_KV_FP8_E5M2 = 3,
  /* KVCacheType::TurboQuantMSE { bits } (src/model/mod.rs:182-213): what `--kv-cache-type turboquant2 | tq2` / `turboquant3 | tq3`
   * selects (src/config.rs:808-817) — randomized Hadamard rotation + Lloyd-Max scalar codes, src/model/turboquant/, cache and
   * attention src/model/kv_turboquant.rs.  head_dim 64 or 128. */
  LGH_KV_TQ2 = 4,
  LGH_KV_TQ3 = 5,
  /* KVCacheType::TurboQuantProd { bits }: `turboquant2-qjl | tq2-qjl` / `turboquant3-qjl | tq3-qjl` — the same codes plus, per K row,
   * the sign bits of a Gaussian projection of the quantization residual and the residual's norm (QJL, src/model/turboquant/qjl.rs);
   * scores = codes' dot product + the QJL correction (quant.rs:133-168).  The projection matrices are an input:
   * lgh_set_kv_qjl_matrices. */
  LGH_KV_TQ2_QJL = 6,
  LGH_KV_TQ3_QJL = 7,
};

enum {
  LGH_FLAG_NO_GRAPH = 1u << 0,       /* launch kernels eagerly instead of replaying a hipGraph */
  LGH_FLAG_EXACT_PREFILL = 1u << 2,  /* lgh_prefill_batch feeds the tokens one by one (f32 throughout) instead of the batched f16 GEMM path
                                        (f32 and TurboQuantMSE tq2 / tq3 caches have that path; with this flag a tq2 / tq3 context is
                                        bit-identical to lgh_prefill_token) */
  LGH_FLAG_KV_INT8 = 1u << 4,        /* KV cache as the reference's QuantizedKVCache with KVCacheFormat::Int8 (src/model/kv_quantized.rs): int8
                                        rows + one f32 scale per (kv head, position), a quarter of the f32 cache.  (Same as kv_cache_type =
                                        LGH_KV_INT8; no CLI flag of the reference reaches this format, see kv_cache_type.) */
  /* bits 1, 3, 5, 6, 7 and 24..30 selected the decode structures that round 2 built and measured SLOWER than the default graph of
   * one launch per op (chained FFN with grid barriers, persistent token kernel, flag-ordered launches on two streams, flow
   * launch, split attention merged by the last split / by the output projection: profiles/r02_decode_experiments.md).  They
   * were removed in round 3; lgh_create answers LGH_UNSUPPORTED when one of them is set. */
  LGH_FLAG_REMOVED_MASK = (1u << 1) | (1u << 3) | (1u << 5) | (1u << 6) | (1u << 7) | (0x7Fu << 24),
  LGH_FLAG_MV_GENERIC = 1u << 31,    /* every matrix-core mat-vec runs the generic kernel: the table of static launch plans (compile-time
                                        geometry for the dense 4096 / 14336 shapes, csrc/matvec_mfma.hip) is ignored and the arg-max
                                        keeps both stages.  Same bits either way; for A/B measurements and tests. */
  LGH_FLAG_ATTN_SPLITS_SHIFT = 8,    /* bits 8..15: KV splits per kv-head in decode attention (0 = auto) */
  LGH_FLAG_ATTN_DIRECT_SHIFT = 16    /* bits 16..23: contexts of up to 64 * n rows use the single-launch decode attention (one workgroup
                                        per query head, no split + combine pair); 0 = the tuned default, 255 = never */
};

typedef struct lgh_ctx lgh_ctx;

/* kernel classes reported by lgh_get_stats (profiling mode) */
enum {
  LGH_K_EMBED = 0, LGH_K_QKV = 1, LGH_K_ATTN = 2, LGH_K_ATTN_COMBINE = 3, LGH_K_WO = 4, LGH_K_GATEUP = 5,
  LGH_K_DOWN = 6, LGH_K_ROUTER = 7, LGH_K_OUTPUT = 8, LGH_K_ARGMAX = 9, LGH_K_MISC = 10,
  LGH_K_TOKEN = 11,   /* (unused since round 3: was the persistent token kernel) */
  LGH_K_COUNT = 16
};

/* kernel SYMBOLS reported by lgh_get_stats (profiling mode): what `rocprofv3 --kernel-trace --stats` groups by.
 * LGH_SYM_MV_* are the instantiations of lgh::mv_kernel<MASK, MAXT> (the VALU dequant mat-vec, csrc/matvec.hip; MASK bits:
 * Q4_K 1, Q5_K 2, Q6_K 4, Q8_0 8, Q4_0 16; MAXT = the instantiation's thread cap).  LGH_SYM_MVQ_* are the instantiations of
 * lgh::mvq_kernel<MASK> (the int8 matrix-core mat-vec, csrc/matvec_mfma.hip; ITS mask bits: Q4_K 1, Q6_K 2, Q5_K 4, Q8_0 8,
 * Q4_0 16). */
enum {
  LGH_SYM_MV_Q4K = 0,      /* lgh::mv_kernel<1u, 1024>  : every matrix of the launch Q4_K */
  LGH_SYM_MV_Q80 = 1,      /* lgh::mv_kernel<8u, 1024>  : Q8_0 */
  LGH_SYM_MV_Q40 = 2,      /* lgh::mv_kernel<16u, 1024> : Q4_0 */
  LGH_SYM_MV_Q5K = 3,      /* lgh::mv_kernel<2u, 768>   : Q5_K */
  LGH_SYM_MV_Q6K = 4,      /* lgh::mv_kernel<4u, 512>   : Q6_K */
  LGH_SYM_MV_Q4K_Q6K = 5,  /* lgh::mv_kernel<5u, 512>   : Q4_K + Q6_K in one launch (fused QKV of Q4_K_M) */
  LGH_SYM_MV_Q5K_Q6K = 6,  /* lgh::mv_kernel<6u, 512>   : Q5_K + Q6_K */
  LGH_SYM_MV_ALL = 7,      /* lgh::mv_kernel<31u, 512>  : any other mix */
  LGH_SYM_F32_MATVEC = 8,  /* lgh::f32_matvec_kernel */
  LGH_SYM_ATTN = 9,        /* lgh::attn_partial_kernel<D, G> */
  LGH_SYM_ATTN_COMBINE = 10,
  LGH_SYM_EMBED = 11,
  LGH_SYM_ARGMAX = 12,     /* argmax_stage1 + argmax_stage2 (two launches, timed together) */
  LGH_SYM_ROUTER = 13,
  LGH_SYM_OTHER = 14,
  LGH_SYM_MVQ_Q4K = 15,    /* lgh::mvq_kernel<1u> : int8 matrix-core mat-vec, every matrix of the launch Q4_K */
  LGH_SYM_MVQ_Q6K = 16,    /* lgh::mvq_kernel<2u> : ... every matrix Q6_K */
  LGH_SYM_MVQ_MIXED = 17,  /* lgh::mvq_kernel<3u> : ... Q4_K and Q6_K matrices in one launch (fused QKV of Q4_K_M) */
  LGH_SYM_MVQ_Q5K = 18,    /* lgh::mvq_kernel<4u> / <6u> : Q5_K (and Q5_K + Q6_K) */
  LGH_SYM_MVQ_Q80_Q40 = 19, /* lgh::mvq_kernel<8u> / <16u> : Q8_0 / Q4_0 */
  LGH_SYM_PTOK = 20,       /* (unused since round 3) */
  LGH_SYM_COUNT = 24
};

typedef struct lgh_stats {
  uint64_t weight_bytes;             /* quantized + f32 weight bytes resident in HBM */
  uint64_t kv_bytes;                 /* KV cache bytes */
  uint64_t scratch_bytes;
  uint64_t tokens_processed;
  uint64_t graph_nodes;              /* kernel nodes in one decode-step graph */
  /* profiling mode only: per-class launches, device time (hipEvent) and algorithmic HBM bytes */
  uint64_t k_launches[LGH_K_COUNT];
  double k_time_us[LGH_K_COUNT];
  uint64_t k_alg_bytes[LGH_K_COUNT];
  /* the same, grouped by kernel symbol (LGH_SYM_*) */
  uint64_t sym_launches[LGH_SYM_COUNT];
  double sym_time_us[LGH_SYM_COUNT];
  uint64_t sym_alg_bytes[LGH_SYM_COUNT];
  /* algorithmic bytes of one decode step at the current position (SURVEY.md §8d formula) */
  uint64_t step_alg_bytes;
  /* profiling mode: mean elapsed time of an EMPTY hipEvent bracket on the launch stream, measured once per
   * profiled token — the fixed cost every k_time_us / sym_time_us sample carries on top of the kernel itself */
  double event_bracket_us;
  uint64_t event_bracket_samples;
  uint64_t overlapped_edges;         /* always 0 (reserved: belonged to the flag-ordered launches removed in round 3) */
} lgh_stats;

/* ---- lifecycle: replaces GpuOnlyInference::from_model (src/backend/cuda/gpu_only.rs:426-726) ---- */

/* Number of HIP devices visible (0 when none / no driver).  Never fails. */
int lgh_device_count(void);

/* CudaDevice::new + scratch/KV allocation (gpu_only.rs:438-440, 527-598). */
int lgh_create(const lgh_model_desc* desc, lgh_ctx** out);

/* The KV cache a descriptor asks for, without a device (a host sizes its memory with it): bytes per (kv head, position) and the
 * bytes of one slot (one sequence of max_seq_len positions) of one layer.  A context holds num_layers such slots for its own
 * sequence, lgh_batch_create(max_batch) adds max_batch per layer; lgh_stats.kv_bytes counts exactly these.  Reads kv_cache_type,
 * flags, num_kv_heads, max_seq_len and head_dim of the descriptors lgh_create takes (LGH_FLAG_KV_INT8 with type 0 included);
 * InvalidArgument for a kv_cache_type above LGH_KV_TQ3_QJL. */
typedef struct lgh_kv_layout {
  uint32_t kv_cache_type;            /* LGH_KV_*, the flag spelling resolved */
  uint32_t row_bytes;                /* one K or V row: 4 * head_dim (f32), head_dim (int8 / FP8), head_dim / 4 or head_dim / 8 * 3 (TQ codes) */
  uint32_t scale_bytes;              /* per K and per V row: 4 (int8), else 0 */
  uint32_t qjl_bytes;                /* per K row: head_dim / 8 + 4 (the QJL formats: sign bits + residual norm), else 0 */
  uint64_t rows;                     /* num_kv_heads * max_seq_len */
  uint64_t k_bytes, v_bytes, k_scale_bytes, v_scale_bytes, k_qjl_bytes;   /* one slot's tensors: rows * the per-position bytes */
  uint64_t slot_bytes;               /* their sum */
} lgh_kv_layout;
int lgh_kv_cache_layout(const lgh_model_desc* desc, lgh_kv_layout* out);

/* upload_model_weights (src/backend/cuda/dequant_weights.rs:244-505): one call per tensor, GGUF name
 * (`token_embd.weight`, `blk.{i}.attn_q.weight`, ... `blk.{i}.ffn_gate_exps.weight` or the loader's
 * per-expert `blk.{i}.ffn_gate.{e}.weight`, `output_norm.weight`, `output.weight`), GGML dims (dim 0
 * fastest), host bytes in native GGUF order.  Tensors of layers outside this stage are ignored. */
int lgh_upload_tensor(lgh_ctx* ctx, const char* gguf_name, uint32_t ggml_type, const uint64_t ne[4],
                      const void* host_bytes, size_t nbytes);

/* Validates that every tensor the stage needs is present, builds RoPE tables and the hipGraphs. */
int lgh_finalize(lgh_ctx* ctx);

/* impl Drop */
void lgh_destroy(lgh_ctx* ctx);

/* ---- GpuInference (src/backend/mod.rs:283-296) ---- */

/* GpuInference::forward (gpu_only.rs:728-771): logits_out = vocab_size f32, caller-owned. */
int lgh_forward(lgh_ctx* ctx, uint32_t token_id, float* logits_out);
/* GpuInference::prefill_token (gpu_only.rs:792-806) */
int lgh_prefill_token(lgh_ctx* ctx, uint32_t token_id);
/* GpuOnlyInference::forward_batch minus the last token (gpu_only.rs:776-790: n prefill_tokens).  Single-stage models
 * (dense or MoE) whose 2-D weights are all in matrix-core tile layouts (Q4_K, Q5_K, Q6_K, Q8_0, Q4_0 with k % 256 == 0)
 * take the batched path: blocks of up to 128 tokens, one f16-MFMA GEMM per weight (MoE: per expert, over
 * the tokens routed to it), causal attention over the block; the KV cache it leaves equals the token-by-token one within
 * 1e-2 relative (f16 operands, f32 accumulation).  KV caches: f32, and TurboQuantMSE (LGH_KV_TQ2 / TQ3), whose rows are compressed as
 * write_kv does and attended through their codes, the block's own rows included.  The byte caches (LGH_KV_INT8 / FP8_E4M3 / FP8_E5M2)
 * take it on a context that asked for it with lgh_set_prefill_policy.  Everything else (the QJL caches, TurboQuant pipeline stages),
 * and any context created with LGH_FLAG_EXACT_PREFILL, runs n exact prefill_tokens. */
int lgh_prefill_batch(lgh_ctx* ctx, const uint32_t* tokens, size_t n);
/* 1 when lgh_prefill_batch will take the batched GEMM path for this (finalized) context, else 0 */
int lgh_prefill_is_batched(lgh_ctx* ctx);
/* Which prompt path a context takes where it has a choice.  A call on a finalized context, at any time between calls; unknown bits answer
 * InvalidArgument and change nothing.  The word is open for further bits.
 *   LGH_PREFILL_BATCH_BYTE_KV  int8 / FP8 caches take the batched path: the context's own sequence (lgh_prefill_batch), the slots of the
 *     multi-sequence engine (lgh_batch_prefill) and stage contexts (lgh_stage_prefill_batch).  A block's K / V rows are quantized by the
 *     decode attention's own quantizers (same bytes and scales for the same f32 row) and every token attends to the stored bytes, the
 *     block's own rows included.  Like every batched pass it differs from n prefill_tokens within the 1e-2 relative above, which is why
 *     it is not the default: without the bit a byte cache's prompt is bit-identical to the token-by-token engine's.  All other
 *     conditions of the batched path still apply, LGH_FLAG_EXACT_PREFILL still wins, and the bit does nothing on f32 and TurboQuant
 *     contexts.  lgh_prefill_is_batched reports the result.
 * TurboQuant slots and the QJL formats stay token by token whatever the word says; the lgh_tp_* and lgh_pipeline_* handles have no
 * setter. */
enum { LGH_PREFILL_DEFAULT = 0, LGH_PREFILL_BATCH_BYTE_KV = 1u << 0 };
int lgh_set_prefill_policy(lgh_ctx* ctx, uint32_t policy);
/* GpuInference::reset (gpu_only.rs:808-843) — O(1): only the position is rewound (model/mod.rs:110-117) */
void lgh_reset(lgh_ctx* ctx);
/* GpuInference::position (gpu_only.rs:845-847) */
size_t lgh_position(const lgh_ctx* ctx);
/* KVCache::truncate (src/model/mod.rs:130-134): forget the rows from new_len on (no-op when new_len >= position). */
int lgh_kv_truncate(lgh_ctx* ctx, size_t new_len);
/* KVCache::shift_left (src/model/mod.rs:142-172) on the DEVICE cache, with the position following as ChatEngine does
 * (src/engine.rs:1394-1411: the reference shifts its host-side cache only, so a GPU engine keeps the untrimmed rows).
 * Rows [amount, position) move to the front; amount == 0 or >= position clears the cache, as in the reference.  The rows
 * keep the RoPE rotation of their old positions (the reference does not re-rotate either). */
int lgh_kv_shift_left(lgh_ctx* ctx, size_t amount);

/* forward + the bench's arg-max (src/main.rs:1812-1822; ties -> LAST maximal index) on device:
 * only 4 bytes cross PCIe. */
int lgh_forward_argmax(lgh_ctx* ctx, uint32_t token_id, uint32_t* next_token);
/* n_steps of greedy decode with the token fed back ON DEVICE (the loop of src/main.rs:1812-1822);
 * tokens_out[i] = arg-max after step i.  One host sync at the end. */
int lgh_decode_greedy(lgh_ctx* ctx, uint32_t first_token, size_t n_steps, uint32_t* tokens_out);

/* TurboQuant KV cache: the sign vectors of the rotations, [owned layer][kv head][k engine, v engine][head_dim] values of +1 / -1 =
 * HadamardRotation::signs() (src/model/turboquant/rotation.rs:126-129) of TurboQuantKVCache's engines_k / engines_v
 * (src/model/kv_turboquant.rs:44-71).  Call between lgh_create and lgh_finalize; without it the library uses a deterministic
 * stand-in (valid rotations, but not the reference's StdRng stream). */
int lgh_set_kv_rotation_signs(lgh_ctx* ctx, const float* signs, size_t n);
/* one row through the TurboQuant compressor (TurboQuantEngine::compress without QJL, src/model/turboquant/quant.rs:71-103):
 * x[dim] (dim 64 or 128), bits 2 or 3, signs[dim] -> codes[dim / 4 or dim / 8 * 3].  Bit-exact with the reference's arithmetic. */
int lgh_op_tq_compress(int device, int bits, const float* x, size_t dim, const float* signs, uint8_t* codes);
/* TurboQuantProd: the QJL projection matrices of the K engines, [owned layer][kv head][head_dim][head_dim] f32, row i = the i-th
 * projection vector in the order QjlProjector draws it (src/model/turboquant/qjl.rs:44-52: StdRng::seed_from_u64(seed), one
 * StandardNormal sample per (i, j), j fastest; the K engine's seed is 4 * (layer * kv_heads + head) + 1, kv_turboquant.rs:55-58).
 * Call between lgh_create and lgh_finalize on a context with kv_cache_type LGH_KV_TQ2_QJL / TQ3_QJL; without it the library uses
 * a deterministic stand-in (i.i.d. N(0, 1), but not the reference's RNG stream).  (The V engines' projectors are not needed: the
 * reference never reads the QJL bits of V rows, kv_turboquant.rs:154-170.) */
int lgh_set_kv_qjl_matrices(lgh_ctx* ctx, const float* matrices, size_t n);
/* lgh_op_tq_compress with use_qjl (quant.rs:71-103): + qjl_matrix[dim][dim] -> qjl_bits[dim / 64] (bit i % 64 of word i / 64 =
 * (S r)_i >= 0, r the residual) and *residual_norm.  Bit-exact with the reference's arithmetic for the given matrix. */
int lgh_op_tq_compress_qjl(int device, int bits, const float* x, size_t dim, const float* signs, const float* qjl_matrix, uint8_t* codes,
                           uint64_t* qjl_bits, float* residual_norm);

/* ---- multi-sequence decode: the device side of BatchedEngine (src/engine_batched.rs:23-194, 200-330, 355-400) ----
 * The reference keeps one InferenceContext (KV cache + position) per ActiveSequence (engine_batched.rs:84-100, 332-353) and every
 * iteration of its loop calls model.forward for each active sequence in turn (236-290 -> step_sequence 355-400): B sequences read
 * the weights B times.  Here a finalized single-stage context owns `max_batch` <= 16 SLOTS (a slot = one sequence's KV caches
 * + position), and one step feeds one token to each listed slot while reading every weight tile ONCE.  Every sequence's
 * logits are bit-identical to what lgh_forward returns for the same token history (same arithmetic, same summation orders).
 * Dense and MoE models whose matrices are in the matrix-core tile layouts (Q4_K / Q5_K / Q6_K / Q8_0 / Q4_0, k % 256 == 0);
 * anything else answers LGH_UNSUPPORTED.  The slots' caches have the context's kv_cache_type: f32, int8 / FP8
 * (LGH_KV_INT8 / FP8_E4M3 / FP8_E5M2: per slot a byte per element, + one f32 scale per int8 row: about a quarter of the f32 slots'
 * memory) or the TurboQuant formats (LGH_KV_TQ2 / TQ3 / TQ2_QJL / TQ3_QJL: per slot the packed code rows (+ QJL rows)); the
 * reference's BatchedEngine itself only ever creates f32 caches, engine_batched.rs:355-357.  Slots with a TurboQuant cache take
 * their prompt token by token (lgh_batch_prefill), and so do int8 / FP8 slots unless the context set LGH_PREFILL_BATCH_BYTE_KV
 * (lgh_set_prefill_policy).  The single-sequence entry points keep working on the context's own cache.  (A serving context is better created with 8 attention splits — flags bits 8..15 — than with
 * the single-sequence default: the split count also sizes the multi-sequence attention launch, profiles/r03e_batched_decode.md.) */
int lgh_batch_create(lgh_ctx* ctx, uint32_t max_batch);                 /* BatchedEngineConfig::max_batch_size (engine_batched.rs:23-41) */
int lgh_batch_reset(lgh_ctx* ctx, uint32_t slot);                       /* create_active_sequence: model.create_context (332-353); O(1) */
size_t lgh_batch_position(lgh_ctx* ctx, uint32_t slot);                 /* ActiveSequence.ctx.position */
/* the slot's prompt (step_sequence's first call: position == 0 -> the whole prompt, 373-379), on the batched prompt path */
int lgh_batch_prefill(lgh_ctx* ctx, uint32_t slot, const uint32_t* tokens, size_t n);
/* One iteration of the loop (236-290): tokens[i] goes to slot slots[i] (distinct slots, 1 <= n_seq <= max_batch).
 * logits_out: n_seq x vocab f32 (row i = sequence i) or NULL; next_tokens: the greedy choice per sequence (last maximal index)
 * or NULL.  InvalidArgument when a slot is full (position >= max_seq_len), nothing is changed then. */
int lgh_forward_multi(lgh_ctx* ctx, const uint32_t* slots, const uint32_t* tokens, uint32_t n_seq, float* logits_out, uint32_t* next_tokens);
/* n_steps greedy iterations with every sequence's token fed back on the device; tokens_out[step * n_seq + i] (or NULL).  One host
 * synchronisation at the end (the bench's timed region for --batch). */
int lgh_decode_greedy_multi(lgh_ctx* ctx, const uint32_t* slots, const uint32_t* first_tokens, uint32_t n_seq, size_t n_steps, uint32_t* tokens_out);

/* ---- sampling on the device: Sampler::sample and sample_mirostat (src/sampling/mod.rs:188-387) inside the per-token
 * graph, so that the reference's default generation settings (EngineConfig::default, src/engine.rs:117-130) stay on the
 * graph-replayed decode loop.  Steps as the reference does them, all in f32: repetition penalty once per occurrence in the
 * window (x > 0: x /= p, else x *= p), frequency then presence penalty for every token this sampler emitted, x *= 1.0f / T,
 * softmax, greedy (T == 0 or top_k == 1: the LAST index of the maximal probability; no draw, not counted), stable sort by
 * probability, top-k, top-p (a cutoff at position 0 truncates nothing), renormalize, draw (first r < cumulative sum, else the
 * last kept token), count.  min-p and Mirostat come with lgh_sampler_config_ex below.  The random draws are INPUTS: uniforms[i] is what the reference's `self.rng.gen::<f32>()` returns at
 * step i, so a host that draws them from its own StdRng gets the reference's tokens.  Single-stage contexts
 * only; bad configs (non-finite or negative temperature, top_p outside (0, 1], repeat_penalty <= 0, non-finite penalties)
 * and sampling without a prior set_sampler answer LGH_INVALID_ARGUMENT. ---- */
typedef struct lgh_sampler_config {   /* SamplerConfig (sampling/mod.rs:37-62) minus seed / typical_p; min_p and mirostat: lgh_sampler_config_ex */
  float temperature;
  uint32_t top_k;                     /* 0: no top-k truncation */
  float top_p;
  float repeat_penalty;
  uint32_t repeat_window;             /* 0: every token so far */
  float frequency_penalty;
  float presence_penalty;
  int32_t eos_token;                  /* -1: none.  Within one call, steps after the step that sampled it do not update the counts
                                         (the reference stops there; the host truncates the KV cache with lgh_kv_truncate) */
} lgh_sampler_config;

/* Sampler::new (mod.rs:150-165): the config and zeroed counts.  The counts persist across decode calls until the next call. */
int lgh_set_sampler(lgh_ctx* ctx, const lgh_sampler_config* config);
/* Engine::generate's loop (src/engine.rs:424-431) with the token fed back on the device: n_steps tokens, the first from the
 * logits of first_token at the current position.  history: the tokens in the context before first_token (at least
 * min(position, repeat_window) of them, all when the window is 0); the device appends first_token and every sampled token.
 * uniforms[n_steps] (may be NULL under a greedy config).  One host synchronisation at the end. */
int lgh_decode_sample(lgh_ctx* ctx, uint32_t first_token, const uint32_t* history, size_t n_history, size_t n_steps,
                      const float* uniforms, uint32_t* tokens_out);
/* BatchedEngine's per-sequence sampler (src/engine_batched.rs:358, 397): lgh_set_sampler for one slot */
int lgh_batch_set_sampler(lgh_ctx* ctx, uint32_t slot, const lgh_sampler_config* config);
/* lgh_decode_greedy_multi with each sequence sampled by its slot's sampler.  histories: the n_seq histories back to back,
 * history_lens[n_seq] long; uniforms[n_steps][n_seq]; tokens_out[n_steps][n_seq]. */
int lgh_decode_sample_multi(lgh_ctx* ctx, const uint32_t* slots, const uint32_t* first_tokens, uint32_t n_seq,
                            const uint32_t* histories, const size_t* history_lens, size_t n_steps, const float* uniforms,
                            uint32_t* tokens_out);

/* SamplerConfig's remaining fields that Sampler::sample reads (typical_p is stored but never read; the seed stays with the
 * host's rng).  lgh_set_sampler(cfg) is lgh_set_sampler_ex with min_p 0 and mirostat 0.
 *   min_p (mod.rs:248-258): after the stable sort and before top-k the order is cut at the first probability below
 *     p[order[0]] * min_p (never to nothing); top-k then compares against the cut length, and top-p's cutoff-0 quirk keeps the
 *     min-p set.  Ignored under a greedy config (the greedy return comes first).
 *   mirostat (MirostatConfig, mod.rs:15-34; sample_mirostat 304-387; mod.rs:210-213): after the penalties, and INSTEAD of the
 *     temperature, the greedy test, min-p, top-k and top-p: softmax, stable descending sort; v2 keeps the ranks before the
 *     first whose -log2(p) exceeds mu (at least one), v1 keeps clamp((2^mu * vocab) as usize, 1, vocab) = all of them (mu >= 0,
 *     see below); r = uniform * sum of the kept, unnormalized; the first token whose cumulative sum exceeds r, else the TOP
 *     token; mu -= eta * (-log2(p_token) - tau), clamped to [0, 20]; the token is always counted.  Every step needs its
 *     uniform, whatever temperature and top_k say.
 * InvalidArgument: struct_size != sizeof, min_p outside [0, 1] or not finite, mirostat > 2, tau or eta not finite, tau < 0 (a
 * narrowing of the reference, which takes any f32: with tau >= 0, mu starts at 2 * tau >= 0 and stays in [0, 20], which is
 * what makes v1's candidate count the whole vocabulary). */
typedef struct lgh_sampler_config_ex {
  uint32_t struct_size;               /* sizeof(lgh_sampler_config_ex) */
  lgh_sampler_config base;
  float min_p;                        /* 0: off */
  uint32_t mirostat;                  /* 0: off, 1, 2 (MirostatConfig::version) */
  float mirostat_tau, mirostat_eta;   /* MirostatConfig::tau, eta (default 5.0, 0.1) */
} lgh_sampler_config_ex;
/* Sampler::new (mod.rs:150-169): the config, zeroed counts and mirostat_mu = 2 * tau.  Counts and mu persist across decode
 * calls until the next set_sampler; within one call, steps after the step that sampled eos_token update neither. */
int lgh_set_sampler_ex(lgh_ctx* ctx, const lgh_sampler_config_ex* config);
/* lgh_set_sampler_ex for one slot (src/engine_batched.rs:358, 397); slots may mix Mirostat and ordinary samplers in one step */
int lgh_batch_set_sampler_ex(lgh_ctx* ctx, uint32_t slot, const lgh_sampler_config_ex* config);
/* Sampler::mirostat_mu (mod.rs:144-145) of the context's own sampler (slot -1) or of a batch slot, after the steps enqueued so
 * far (synchronises).  10.0 when Mirostat is off, as Sampler::new leaves it (mod.rs:161). */
int lgh_get_sampler_mu(lgh_ctx* ctx, int slot, float* mu);

/* ---- device prompt cache: the KV rows of a prompt kept on the device, restored and shared by copying.  The device side of
 * PromptCache / PrefixSharing (src/model/cache.rs:67-345, re-exported at src/lib.rs:75), whose CachedPrefix (cache.rs:28-65) clones
 * every layer's K / V tensors on the host; the LRU table, the longest-match lookup and the reference counts stay with the host
 * (llama-gguf_amd/hip_backend.py restates them).  A prefix holds rows [0, n_rows) of every cache tensor of every
 * layer the context owns, packed [layer][K, V, K scales, V scales, K QJL words: those the format has][kv head][n_rows][bytes per
 * position] (lgh_kv_cache_layout), in ONE device allocation of
 *     layers * num_kv_heads * n_rows * (2 * (row_bytes + scale_bytes) + qjl_bytes)  bytes.
 * slot: -1 = the context's own sequence, else a slot of lgh_batch_create.  A save or a restore is one kernel launch, enqueued on
 * the context's stream: a decode call issued after a restore is ordered behind it.  A stage context of the layer pipeline saves
 * and restores its own layers; the lgh_tp_* and lgh_pipeline_* handles have no prefix entry points (their rank / stage contexts
 * are not reachable through this ABI).  lgh_stats is not changed by any of these calls: lgh_prefix_total_bytes reports the prefixes.
 * TurboQuant rows mean something only under the rotation signs and QJL matrices they were written with (lgh_set_kv_rotation_signs,
 * lgh_set_kv_qjl_matrices): a host that imports a prefix into another context must give that context the same ones; the library
 * does not try to detect a change.
 * InvalidArgument, with nothing changed: a NULL pointer; a slot >= max_batch, or any slot before lgh_batch_create; n_rows beyond
 * the source's position (save) or the prefix's rows (restore); nothing to save (position 0); a handle that is not one of this
 * context's live prefixes (freed, or made by another context: handles are looked up, never dereferenced first); an import whose
 * header or size does not match the context.  AllocationFailed, with nothing changed, when the device allocation fails. ---- */
typedef struct lgh_prefix lgh_prefix;   /* owned by the context that made it; lgh_destroy frees the live ones */
typedef struct lgh_prefix_info {
  uint32_t struct_size;              /* sizeof(lgh_prefix_info) */
  uint32_t kv_cache_type;            /* LGH_KV_* */
  uint32_t n_rows;                   /* CachedPrefix::seq_len (cache.rs:38) */
  uint32_t layer_begin, layer_end;   /* the layers it holds: the context's */
  uint64_t bytes;                    /* device bytes = CachedPrefix::memory_size (cache.rs:60-64) without the tokens */
} lgh_prefix_info;
/* PrefixSharing::save_prefix (cache.rs:313-326): rows [0, n_rows) of the sequence (n_rows 0: up to its position) into a new prefix.
 * The source is not changed. */
int lgh_prefix_save(lgh_ctx* ctx, int slot, size_t n_rows, lgh_prefix** out);
/* PrefixSharing::try_restore's copy (cache.rs:287-306): the target reset, then a prompt of n_rows tokens, done by copying (n_rows 0:
 * all of the prefix; fewer is valid, KV is causal).  Writes rows [0, n_rows) and sets the position as the prompt path does (the own
 * sequence's position and its device word, or the slot's position); the sampler state stays as it is. */
int lgh_prefix_restore(lgh_ctx* ctx, const lgh_prefix* prefix, int slot, size_t n_rows);
/* PromptCache::remove_prefix (cache.rs:191-195): frees the device memory.  Synchronises the stream first. */
int lgh_prefix_free(lgh_ctx* ctx, lgh_prefix* prefix);
int lgh_prefix_get_info(lgh_ctx* ctx, const lgh_prefix* prefix, lgh_prefix_info* info);
/* PromptCacheStats::memory_used (cache.rs:203-210) without the tokens: device bytes of the context's live prefixes */
uint64_t lgh_prefix_total_bytes(lgh_ctx* ctx);
/* A prefix as host bytes (a session file; CachedPrefix is Clone, cache.rs:29): a fixed header — magic, version, kv_cache_type,
 * num_kv_heads, head_dim, layer_begin, layer_end, n_rows (uint32 each), payload bytes (uint64) — then the packed rows.  *needed
 * receives the total; dst NULL only asks for it.  Synchronises the stream first. */
int lgh_prefix_export(lgh_ctx* ctx, const lgh_prefix* prefix, void* dst, size_t dst_bytes, size_t* needed);
/* ... and back: every header field is checked against the context, the size against the header. */
int lgh_prefix_import(lgh_ctx* ctx, const void* src, size_t bytes, lgh_prefix** out);

const char* lgh_last_error(const lgh_ctx* ctx);
int lgh_get_stats(lgh_ctx* ctx, lgh_stats* out);
/* on: run eagerly with hipEvent pairs around every launch and accumulate lgh_stats.k_* */
int lgh_set_profiling(lgh_ctx* ctx, int on);
/* Use an external HIP stream for all work; NULL = the context's own (a non-blocking stream).  NB the handle of the legacy
 * default stream IS NULL: a caller whose other work runs on the default stream (torch without an explicit stream) must create
 * a stream, run that work on it and pass it here — otherwise nothing orders that work against the context's kernels. */
int lgh_set_stream(lgh_ctx* ctx, void* hip_stream);
void* lgh_get_stream(lgh_ctx* ctx);
int lgh_synchronize(lgh_ctx* ctx);

/* debug tap: copy the hidden state (f32[hidden_size]) of the last processed token to host */
int lgh_read_hidden(lgh_ctx* ctx, float* out);

/* ---- pipeline stages over xGMI (replaces ShardServer::forward, src/distributed/shard.rs:377-445) ----
 * The hop between stages is one f32[hidden_size] vector; the host side moves it with RCCL
 * send/recv (or a peer copy) between the device buffers returned here. */
int lgh_stage_hidden_buffer(lgh_ctx* ctx, void** device_ptr);     /* in/out residual stream buffer */
/* Run this stage's layers for one token at the context's position.  First stage: embeds token_id;
 * other stages: consume the hidden buffer.  Last stage with want_logits: final norm + output
 * projection (+ device arg-max into *next_token if non-NULL).  Asynchronous on the stream unless
 * logits_out / next_token are requested. */
int lgh_stage_forward(lgh_ctx* ctx, uint32_t token_id, int want_logits, float* logits_out, uint32_t* next_token);
/* A block of up to 128 prompt tokens through this stage's layers on the batched path (lgh_prefill_batch's, for layer
 * ranges).  The first stage reads `tokens`; any other stage reads the block of hidden vectors [n][hidden_size] f32 at
 * lgh_stage_hidden_block_buffer, where a stage that is not the last leaves its output block for the next hop.
 * LGH_UNSUPPORTED when the context has no batched path (feed the tokens through lgh_stage_forward then). */
int lgh_stage_prefill_batch(lgh_ctx* ctx, const uint32_t* tokens, size_t n);
int lgh_stage_hidden_block_buffer(lgh_ctx* ctx, void** device_ptr);
/* Token feedback WITHOUT the host (the reference's coordinator carries every token through host memory,
 * src/distributed/pipeline.rs:50-96): *token_in = the device word the first stage embeds from, *argmax_out = the device word
 * the last stage's arg-max lands in (int32 each).  The host side moves argmax_out -> token_in with an RCCL send/recv or a
 * peer copy on the stages' streams. */
int lgh_stage_io_buffers(lgh_ctx* ctx, void** token_in, void** argmax_out);
/* Stages that share a DEVICE and a stream (lgh_set_stream) can hop inside the producing stage's graph: from now on every token
 * of `ctx` ends with hidden -> *hidden_dst (the next stage's lgh_stage_hidden_buffer; not the last stage) and, in mode 2,
 * arg-max -> *token_dst (the first stage's token_in; last stage only).  NULL switches a hop off.  Both addresses must be memory
 * of ctx's device.  Measured on one MI355X: a hop as a runtime copy between two graph launches costs 12-18 us, as a graph node
 * 3 us (profiles/r03d_pipeline_boundary.md). */
int lgh_stage_set_forward_targets(lgh_ctx* ctx, void* hidden_dst, void* token_dst);
/* lgh_stage_forward without any host value: the token is already in *token_in (first stage) / the hidden vector in the
 * stage's hidden buffer; nothing is copied back and nothing is waited for.  mode 0 = this stage's layers only, 1 = + final
 * norm and output projection (last stage), 2 = + device arg-max into *argmax_out and the token log (last stage). */
int lgh_stage_step(lgh_ctx* ctx, int mode);
/* Last stage: the arg-max tokens logged at positions [pos0, pos0 + n) (one device-to-host copy, synchronises). */
int lgh_stage_read_tokens(lgh_ctx* ctx, size_t pos0, size_t n, uint32_t* out);
/* Last stage: the logits of the last lgh_stage_step(ctx, 1 or 2) (vocab_size f32; one device-to-host copy, synchronises). */
int lgh_stage_read_logits(lgh_ctx* ctx, float* logits_out);

/* ---- the layer pipeline inside the library: ONE process, n_stages stage contexts on the given devices (device_ids NULL:
 * all on desc->device_id), contiguous near-equal layer ranges (earlier stages take the remainder).  Replaces
 * PipelineExecutor::forward (src/distributed/pipeline.rs:50-96) + ShardServer::forward (src/distributed/shard.rs:377-445)
 * for a host that links this library: per token and stage boundary one f32[hidden_size] peer copy over xGMI on the producing
 * stage's stream and an event the consuming stage waits for; in lgh_pipeline_decode_greedy the arg-max token goes from the
 * last stage's device word into the first stage's the same way — no host value crosses a stage boundary per token.  The
 * entry points mirror the single-context ones (GpuInference, src/backend/mod.rs:283-296), so GpuModelWrapper drives a
 * pipeline handle unchanged. ---- */
typedef struct lgh_pipeline lgh_pipeline;
int lgh_pipeline_create(const lgh_model_desc* desc, const int* device_ids, int n_stages, lgh_pipeline** out);
int lgh_pipeline_upload_tensor(lgh_pipeline* p, const char* gguf_name, uint32_t ggml_type, const uint64_t ne[4],
                               const void* host_bytes, size_t nbytes);
int lgh_pipeline_finalize(lgh_pipeline* p);
void lgh_pipeline_destroy(lgh_pipeline* p);
int lgh_pipeline_forward(lgh_pipeline* p, uint32_t token_id, float* logits_out);      /* GpuInference::forward */
int lgh_pipeline_prefill_token(lgh_pipeline* p, uint32_t token_id);                   /* GpuInference::prefill_token */
int lgh_pipeline_decode_greedy(lgh_pipeline* p, uint32_t first_token, size_t n_steps, uint32_t* tokens_out);
void lgh_pipeline_reset(lgh_pipeline* p);                                             /* GpuInference::reset */
size_t lgh_pipeline_position(const lgh_pipeline* p);                                  /* GpuInference::position */
int lgh_pipeline_kv_truncate(lgh_pipeline* p, size_t new_len);                         /* lgh_kv_truncate on every stage */
int lgh_pipeline_stages(const lgh_pipeline* p);
const char* lgh_pipeline_last_error(const lgh_pipeline* p);

/* ---- tensor-parallel decode inside the library: ONE process, n_ranks (1..8) rank contexts on the given devices (device_ids may
 * repeat a device — the single-device rehearsal; NULL: all on desc->device_id).  The scheme is the reference's
 * (src/backend/tensor_parallel.rs:1-6): attention heads split over the ranks, ffn_gate / ffn_up by output rows, attn_output /
 * ffn_down by input (k), a sum over the ranks after each — here one kernel per rank that also adds the residual
 * (layers.rs:1201-1208) and leaves the next mat-vec's input image.  Every rank reads 1/N of a layer's weight bytes for the same
 * token, so this is the structure in which more GPUs make ONE stream faster.  Ranks on one device share one stream and the token
 * is one linear captured graph; ranks on distinct devices run eagerly on their own streams with events and peer-mapped buffers
 * (NOT executed so far: the development box has one GPU).  The entry points mirror the single-context ones (GpuInference,
 * src/backend/mod.rs:283-296), so GpuModelWrapper drives a handle unchanged.
 *
 * lgh_tp_create is ShardingPlan::from_config (tensor_parallel.rs:69-106): InvalidArgument "num_heads (..) must be divisible by
 * world_size (..)" (likewise num_kv_heads, ffn_dim), n_ranks outside 1..8, or a layer_begin / layer_end range; Unsupported for
 * MoE models, a kv_cache_type other than f32, and widths (num_heads / N) * head_dim, intermediate_size / N or hidden_size that
 * are not multiples of 256 (the k-shards are whole 256-element blocks).  lgh_tp_upload_tensor answers Unsupported for a 2-D
 * weight outside the matrix-core tile layouts (Q4_K, Q5_K, Q6_K, Q8_0, Q4_0 with k % 256 == 0).  Why a create failed:
 * lgh_tp_last_error(NULL), per thread.  Quantized caches, MoE, sampling and multi-sequence slots over tensor parallelism are not
 * built. ---- */
typedef struct lgh_tp lgh_tp;
int lgh_tp_create(const lgh_model_desc* desc, const int* device_ids, int n_ranks, lgh_tp** out);   /* TPConfig + ShardingPlan::from_config */
/* the WHOLE tensor, as lgh_pipeline_upload_tensor takes it; every rank gets its part through lgh_tp_shard (in place of
 * shard_weight, tensor_parallel.rs:115-, which refuses quantized tensors) */
int lgh_tp_upload_tensor(lgh_tp* tp, const char* gguf_name, uint32_t ggml_type, const uint64_t ne[4], const void* data, size_t nbytes);
int lgh_tp_finalize(lgh_tp* tp);
void lgh_tp_destroy(lgh_tp* tp);
int lgh_tp_forward(lgh_tp* tp, uint32_t token_id, float* logits_out);          /* GpuInference::forward */
int lgh_tp_prefill_token(lgh_tp* tp, uint32_t token_id);                       /* GpuInference::prefill_token */
/* GpuOnlyInference::forward_batch minus the last token (gpu_only.rs:776-790) over the ranks.  When every rank context has the
 * single context's batched path — head_dim 64 or 128, 1 / 2 / 4 / 8 query heads per kv head, LGH_FLAG_EXACT_PREFILL off;
 * lgh_tp_create's width rules give the 256-multiples — the prompt runs in blocks of up to 128 tokens: every rank runs
 * lgh_prefill_batch's GEMMs, QKV epilogue, block attention and SwiGLU over its own heads and FFN columns, and at the two
 * synchronisation points of a layer each rank collapses its split-K partial sums into one [128][hidden] f32 block and every rank
 * adds the ranks' blocks to its residual rows in rank order (all ranks hold the same bits).  One rank gives lgh_prefill_batch's
 * bits.  The tolerance contract is lgh_prefill_batch's (the KV cache equals the token-by-token one within 1e-2 relative), because
 * tensor parallelism only regroups the f32 sums of wo and down.  The pass runs eagerly, never inside a graph capture.  On distinct
 * devices it uses decode's events and peer-mapped blocks (NOT executed so far, as above).  Any other handle runs n exact
 * lgh_tp_prefill_tokens.  InvalidArgument, with the position unchanged and nothing enqueued: a token id >= vocab_size, position + n
 * > max_seq_len, a handle that is not finalized. */
int lgh_tp_prefill_batch(lgh_tp* tp, const uint32_t* tokens, size_t n);
/* 1 when lgh_tp_prefill_batch will take the batched path for this (finalized) handle, else 0 (gpu_only.rs:776-790) */
int lgh_tp_prefill_is_batched(lgh_tp* tp);
int lgh_tp_decode_greedy(lgh_tp* tp, uint32_t first_token, size_t n_steps, uint32_t* tokens_out);   /* lgh_decode_greedy over the ranks */
void lgh_tp_reset(lgh_tp* tp);                                                 /* GpuInference::reset */
size_t lgh_tp_position(const lgh_tp* tp);                                      /* GpuInference::position */
int lgh_tp_kv_truncate(lgh_tp* tp, size_t new_len);                            /* KVCache::truncate on every rank */
int lgh_tp_ranks(const lgh_tp* tp);                                            /* TensorParallel::world_size */
uint64_t lgh_tp_graph_nodes(const lgh_tp* tp);   /* nodes of the captured token graph (0 before the first replay, and on distinct devices) */
const char* lgh_tp_last_error(const lgh_tp* tp);
int lgh_tp_get_stats(lgh_tp* tp, int rank, lgh_stats* out);   /* lgh_get_stats of one rank's context (its weights, KV rows and scratch) */
/* Host only, no device needed: rank `rank`'s shard of a [ne1 rows][ne0 elements] tensor in GGUF order (shard_weight's job, for
 * quantized payloads too).  axis 0 = rows (out features): a contiguous row range — ne1 / n_ranks rows where n_ranks divides ne1
 * (whole heads, FFN columns), otherwise the same number of whole 16-row tiles for every rank and the remainder to the last one
 * (output.weight).  axis 1 = k (in features): blocks [rank * k / (n * bs), (rank + 1) * k / (n * bs)) of every row; k must hold
 * whole 256-element blocks per rank (Unsupported otherwise).  rank >= n_ranks or dst_bytes too small: InvalidArgument.
 * *written = the shard's bytes; nothing past them is touched, and nothing at all when the call is refused. */
int lgh_tp_shard(uint32_t ggml_type, const uint64_t ne[4], int axis, int rank, int n_ranks, const void* src, size_t src_bytes, void* dst,
                 size_t dst_bytes, size_t* written);
/* The synchronisation-point kernel on its own (TensorParallel::all_reduce_sum + the residual add, host tensors in and out):
 * out = resid + (((p0 + p1) + p2) ...) over the n partial vectors [n][H] in rank order (resid NULL: the sum alone); with
 * xq_image also the matrix-core input image of out * norm_w (norm_w NULL: of out), and with ssq_parts the H / 16 per-chunk sums
 * of out^2.  H % 16 == 0.  out, xq_image and ssq_parts are in / out: bytes the kernel does not write keep the caller's. */
int lgh_op_tp_reduce(int device, const float* partials, uint32_t n, const float* resid, const float* norm_w, size_t H, float* out,
                     uint8_t* xq_image, float* ssq_parts);
/* The two row-wise launches of a tensor-parallel prompt block on their own (host tensors in and out).  partials: n ranks' split-K
 * partial sums [n][S][128][ncols], the block's columns at col0 .. col0 + H - 1; bias [H] or NULL (rank 0's); resid [m][H]; norm_w
 * [H] or NULL.  path 0: every rank's partials collapsed into its compact block
 *   a_r[t][i] = ((0 + part[0][t][col0 + i]) + part[1][t][col0 + i]) + ... (+ bias[i], rank 0),
 * then hidden[t][i] = resid[t][i] + (((a_0 + a_1) + a_2) ...) in rank order, the XH image of f16(f32(hidden * norm_w)) (none without
 * norm_w) and the per-2048-column sums of hidden^2.  path 1 (n == 1 only): lgh_prefill_batch's own row epilogue on rank 0's
 * partials — what path 0 has to equal bit for bit.  hidden_io [128][H], xh_image (ceil(H / 256) * 65536 bytes) and ssq_io [128][8]
 * are in / out: rows t >= m and bytes the kernels do not own keep the caller's.  InvalidArgument: n outside 1..8, m outside 1..128,
 * H % 8, ncols % 4, col0 % 4, col0 + H > ncols, path 1 with n != 1. */
int lgh_op_tp_pf_reduce(int device, int path, const float* partials, uint32_t n, uint32_t n_splits, size_t ncols, size_t col0,
                        const float* bias, const float* resid, const float* norm_w, size_t H, size_t m, float* hidden_io,
                        uint8_t* xh_image, float* ssq_io);

/* ---- per-op surface: the `Backend` trait ops on the path (src/backend/mod.rs:29-265), host tensors
 * in / host tensors out, for parity tests of each kernel against the CPU backend. ---- */
int lgh_op_dequantize(int device, uint32_t ggml_type, const void* src, size_t n_elems, float* dst);
/* Backend::vec_mat_q / vec_mat: out[j] = sum_i x[i] * W[i,j], W = n rows of k/bs blocks */
int lgh_op_vec_mat(int device, uint32_t ggml_type, const void* w, const float* x, float* out, size_t k, size_t n);
/* out[m][n] = x[m][k] . W^T through the batched-prefill GEMM (f16 matrix cores, f32 accumulation; m <= 128, n % 16 == 0,
 * k % 256 == 0, type in {Q4_K, Q5_K, Q6_K, Q8_0, Q4_0}); no reference counterpart */
int lgh_op_mat_mat(int device, uint32_t type, const void* w, const float* x, float* out, size_t k, size_t n, size_t m);
int lgh_op_rms_norm(int device, const float* x, const float* w, float eps, float* out, size_t n);
/* Backend::rope with seq_len 1: q [n_heads, d], k [n_kv_heads, d] rotated in place */
int lgh_op_rope(int device, float* q, float* k, size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t pos,
                float freq_base, float freq_scale, int use_neox);
/* Backend::attention_cached: caches [n_kv_heads, max_seq_len, d] */
int lgh_op_attention_cached(int device, const float* q, const float* k_cache, const float* v_cache, float* out,
                            size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_seq_len, float scale,
                            size_t kv_len, int n_splits);
/* simd::silu_mul_inplace: out = silu(gate) * up */
int lgh_op_silu_mul(int device, const float* gate, const float* up, float* out, size_t n);
/* The rest of the per-op `Backend` trait (src/backend/mod.rs:29-265; CPU: src/backend/cpu/ops.rs), host tensors in and out,
 * for `select_gpu_backend` (src/engine.rs:738-812).  add / mul / scale (ops.rs:24-300) and matmul (row-major [m,k] @ [k,n],
 * ops.rs:429-528) are bit-exact with the CPU backend; silu / gelu / softmax (ops.rs:303-385, softmax along the last
 * dimension of [rows, last_dim]) differ by the device exp / tanh only; matvec ([m,k] @ [k], ops.rs:531-570) and matvec_q
 * (ops.rs:922-950) read the same bytes as vec_mat / vec_mat_q with n = m; attention is the causal GQA attention of
 * ops.rs:1353-1472 (q, out [heads, seq, d]; k, v [kv_heads, kv_len, d]). */
int lgh_op_add(int device, const float* a, const float* b, float* out, size_t n);
int lgh_op_mul(int device, const float* a, const float* b, float* out, size_t n);
int lgh_op_scale(int device, const float* a, float scalar, float* out, size_t n);
/* One row of n values through a KV cache format and back: quantize_int8 / quantize_fp8_e4m3 / quantize_fp8_e5m2 and their
 * dequantizers (src/model/kv_quantized.rs:385-565) as the attention launch applies them.  kv_cache_type LGH_KV_INT8 /
 * LGH_KV_FP8_E4M3 / LGH_KV_FP8_E5M2; bytes_out[n]; *scale_out = the int8 row scale (1 for the FP8 formats; may be NULL). */
int lgh_op_kv_roundtrip(int device, uint32_t kv_cache_type, const float* row, size_t n, uint8_t* bytes_out, float* scale_out, float* back_out);
/* One Sampler::sample call (sampling/mod.rs:188-304) through the device kernels of lgh_decode_sample: logits[vocab]; recent =
 * the recent_tokens argument (the window is taken from its end); counts[vocab] = the sampler's token_counts (NULL: zero);
 * `uniform` = the draw (ignored under a greedy config). */
int lgh_op_sample(int device, const float* logits, size_t vocab, const lgh_sampler_config* config, const uint32_t* recent,
                  size_t n_recent, const uint32_t* counts, float uniform, uint32_t* token_out);
/* lgh_op_sample with min-p / Mirostat (sampling/mod.rs:248-258, 304-387): mu_in = the sampler's mirostat_mu before the call
 * (in [0, 20] under Mirostat, else InvalidArgument; ignored when Mirostat is off), *mu_out = after it (may be NULL). */
int lgh_op_sample_ex(int device, const float* logits, size_t vocab, const lgh_sampler_config_ex* config, const uint32_t* recent,
                     size_t n_recent, const uint32_t* counts, float uniform, float mu_in, uint32_t* token_out, float* mu_out);
int lgh_op_silu(int device, const float* x, float* out, size_t n);
int lgh_op_gelu(int device, const float* x, float* out, size_t n);
int lgh_op_softmax(int device, const float* x, float* out, size_t rows, size_t last_dim);
int lgh_op_matmul(int device, const float* a, const float* b, float* out, size_t m, size_t k, size_t n);
int lgh_op_matvec(int device, const float* a, const float* x, float* out, size_t m, size_t k);
int lgh_op_matvec_q(int device, uint32_t ggml_type, const void* a, const float* x, float* out, size_t m, size_t k);
int lgh_op_attention(int device, const float* q, const float* k, const float* v, float* out, size_t n_heads, size_t n_kv_heads,
                     size_t seq_len, size_t kv_len, size_t head_dim, float scale);
/* The engine's attention launch sequences, one path at a time, for kernel-level tests.  Each takes the cache contents from the
 * host and the position `pos` through the device word the engine's kernels read; the token at `pos` attends to rows 0..pos.
 * A shape the chosen path has no kernel for answers LGH_UNSUPPORTED (never another kernel).  q / out [n_heads][head_dim].
 *
 * Backend::attention_cached (ops.rs:1479-1537) over the f32 cache [n_kv_heads][max_seq_len][head_dim], rows 0..pos already
 * stored (as after the engine's kv_store).  path 0: split + merge (4 or 8 waves per workgroup, chosen from max_seq_len as in
 * the engine; n_splits 1..32); path 1: the single-launch kernel with one workgroup per kv head; path 2: the kernel of any head_dim / group
 * size (max_seq_len <= 38400); path 3: the engine's single-launch kernel, one workgroup per query head (max_seq_len <= 16384).
 *
 * image_out (every entry point of this group; may be NULL): wo's input as the launch that writes `out` leaves it for the mat-vec, the XQ
 * image of `out` (1280 bytes per 256 elements, rounded up).  One sequence: (n_heads * head_dim + 255) / 256 * 1280 bytes; path 2
 * writes none and answers LGH_INVALID_ARGUMENT when asked.  The *_multi entry points: n_seq + 1 images, one per sequence at the
 * step's stride (the size of one image), over a buffer filled with the word 0x7FC0BEEF first: the image behind the last sequence
 * comes back as that pattern.  Without image_out the launches are those of a caller that wants no image, and `out` has the same bits. */
int lgh_op_attention_decode(int device, int path, const float* q, const float* k_cache, const float* v_cache, float* out, size_t n_heads,
                            size_t n_kv_heads, size_t head_dim, size_t max_seq_len, float scale, size_t pos, int n_splits,
                            uint8_t* image_out);
/* The same split + merge as the multi-sequence decode step runs it: sequence s of n_seq (<= 16) attends, with q [n_seq][n_heads][head_dim],
 * to rows 0..pos[s] of cache slot slot[s]; caches [n_slots][n_kv_heads][max_seq_len][head_dim]; out [n_seq][n_heads][head_dim]. */
int lgh_op_attention_decode_multi(int device, const float* q, const float* k_cache, const float* v_cache, float* out, size_t n_heads,
                                  size_t n_kv_heads, size_t head_dim, size_t max_seq_len, size_t n_slots, size_t n_seq, const int* pos,
                                  const int* slot, float scale, int n_splits, uint8_t* image_out);
/* QuantizedKVCache (kv_quantized.rs:143-300, 385-565): kv_cache_type LGH_KV_INT8 / FP8_E4M3 / FP8_E5M2.  k_bytes / v_bytes
 * [n_kv_heads][max_seq_len][head_dim] and (int8 only; may be NULL otherwise) k_scale / v_scale [n_kv_heads][max_seq_len] are in / out:
 * rows 0..pos-1 are read, row `pos` comes back as the launch quantized and stored k_new / v_new [n_kv_heads][head_dim]. */
int lgh_op_attention_kv8(int device, uint32_t kv_cache_type, const float* q, int8_t* k_bytes, int8_t* v_bytes, float* k_scale, float* v_scale,
                         const float* k_new, const float* v_new, float* out, size_t n_heads, size_t n_kv_heads, size_t head_dim,
                         size_t max_seq_len, float scale, size_t pos, int n_splits, uint8_t* image_out);
/* The same over the byte-cache slots of a multi-sequence decode step: sequence s of n_seq (1..16) attends, with q [n_seq][n_heads][head_dim],
 * to rows 0..pos[s]-1 of slot slot[s] and to its own k_new / v_new [n_seq][n_kv_heads][head_dim], which the launch quantizes and stores
 * at row pos[s] of that slot.  k_bytes / v_bytes [n_slots][n_kv_heads][max_seq_len][head_dim] and (int8 only; may be NULL otherwise)
 * k_scale / v_scale [n_slots][n_kv_heads][max_seq_len] are in / out; out [n_seq][n_heads][head_dim].  Every sequence's output is
 * bit-identical to lgh_op_attention_kv8 on its slot alone with the same n_splits.  LGH_UNSUPPORTED: a kv_cache_type outside int8 /
 * FP8, a shape without a kernel; LGH_INVALID_ARGUMENT: pos[s] >= max_seq_len, slot[s] >= n_slots, a slot listed twice, n_seq or
 * n_slots outside 1..16. */
int lgh_op_attention_kv8_multi(int device, uint32_t kv_cache_type, const float* q, int8_t* k_bytes, int8_t* v_bytes, float* k_scale,
                               float* v_scale, const float* k_new, const float* v_new, float* out, size_t n_heads, size_t n_kv_heads,
                               size_t head_dim, size_t max_seq_len, size_t n_slots, size_t n_seq, const int* pos, const int* slot, float scale,
                               int n_splits, uint8_t* image_out);
/* TurboQuantKVCache::write_kv + attention_layer (kv_turboquant.rs:88-201): kv_cache_type LGH_KV_TQ2 / TQ3 / TQ2_QJL / TQ3_QJL.
 * k_codes / v_codes [n_kv_heads][max_seq_len][row bytes] and, for the QJL types, k_qjl [n_kv_heads][max_seq_len][head_dim / 32 + 1]
 * words (sign bits, then the residual norm's bits) are in / out: row `pos` comes back as the launch compressed k_new / v_new.
 * signs [n_kv_heads][k, v][head_dim] (+1 / -1); qjl_matrices [n_kv_heads][head_dim][head_dim] (QJL types; NULL otherwise). */
int lgh_op_attention_tq(int device, uint32_t kv_cache_type, const float* q, uint8_t* k_codes, uint8_t* v_codes, uint32_t* k_qjl,
                        const float* k_new, const float* v_new, const float* signs, const float* qjl_matrices, float* out, size_t n_heads,
                        size_t n_kv_heads, size_t head_dim, size_t max_seq_len, float scale, size_t pos, int n_splits, uint8_t* image_out);
/* The same over the TurboQuant cache slots of a multi-sequence decode step: sequence s of n_seq (1..16) attends, with q [n_seq][n_heads][head_dim],
 * to rows 0..pos[s]-1 of slot slot[s] and to its own k_new / v_new [n_seq][n_kv_heads][head_dim], which the launch compresses into row
 * pos[s] of that slot.  k_codes / v_codes [n_slots][n_kv_heads][max_seq_len][row bytes] and (QJL types) k_qjl
 * [n_slots][n_kv_heads][max_seq_len][head_dim / 32 + 1] are in / out; signs and qjl_matrices as above; out [n_seq][n_heads][head_dim].
 * Every sequence's output is bit-identical to lgh_op_attention_tq on its slot alone with the same n_splits.  LGH_UNSUPPORTED: a
 * kv_cache_type that is not TurboQuant, a shape without a kernel; LGH_INVALID_ARGUMENT: pos[s] >= max_seq_len, slot[s] >= n_slots, a
 * slot listed twice, n_seq or n_slots outside 1..16, n_splits outside 1..32, a sign other than +1 / -1. */
int lgh_op_attention_tq_multi(int device, uint32_t kv_cache_type, const float* q, uint8_t* k_codes, uint8_t* v_codes, uint32_t* k_qjl,
                              const float* k_new, const float* v_new, const float* signs, const float* qjl_matrices, float* out, size_t n_heads,
                              size_t n_kv_heads, size_t head_dim, size_t max_seq_len, size_t n_slots, size_t n_seq, const int* pos,
                              const int* slot, float scale, int n_splits, uint8_t* image_out);
/* Causal Backend::attention (ops.rs:1353-1472) of m_tokens prompt tokens at positions pos0.. as the batched prefill runs it:
 * q [m_tokens][n_heads][head_dim]; the f32 caches hold rows 0..pos0 + m_tokens - 1; out [m_tokens][n_heads * head_dim] = the
 * kernel's f16 results widened to f32.  m_tokens <= 128, n_heads * head_dim % 256 == 0, pos0 + m_tokens <= max_seq_len. */
int lgh_op_attention_prefill(int device, const float* q, const float* k_cache, const float* v_cache, float* out, size_t n_heads,
                             size_t n_kv_heads, size_t head_dim, size_t max_seq_len, float scale, size_t pos0, size_t m_tokens);
/* TurboQuantKVCache::write_kv (kv_turboquant.rs:88-122) for a block of m <= 128 prompt rows as the batched prefill over a
 * TurboQuantMSE cache runs it: kv_cache_type LGH_KV_TQ2 / TQ3; k_rows / v_rows [n_kv_heads][m][head_dim] are the block's RoPE'd f32 rows;
 * k_codes / v_codes [n_kv_heads][max_seq_len][row bytes] are in / out: rows pos0 .. pos0+m-1 come back as the launch compressed them
 * (the bits of lgh_op_tq_compress), every other row as it was.  signs [n_kv_heads][k, v][head_dim] (+1 / -1). */
int lgh_op_pf_tq_store(int device, uint32_t kv_cache_type, const float* k_rows, const float* v_rows, size_t m, size_t n_kv_heads, size_t head_dim,
                       size_t max_seq_len, size_t pos0, const float* signs, uint8_t* k_codes, uint8_t* v_codes);
/* TurboQuantKVCache::attention_layer (kv_turboquant.rs:127-201) for m_tokens prompt tokens at positions pos0.. as the batched prefill
 * over a TurboQuantMSE cache runs it: the code caches already hold rows 0..pos0 + m_tokens - 1; they are expanded into a NaN-filled f32
 * scratch, q [m_tokens][n_heads][head_dim] is rotated, and the block attention's TurboQuant variant runs over the scratch.
 * out [m_tokens][n_heads * head_dim] = the kernel's f16 results widened to f32.  Limits as lgh_op_attention_prefill; head_dim 64 / 128,
 * n_heads / n_kv_heads in {1, 2, 4, 8}. */
int lgh_op_attention_prefill_tq(int device, uint32_t kv_cache_type, const float* q, const uint8_t* k_codes, const uint8_t* v_codes,
                                const float* signs, float* out, size_t n_heads, size_t n_kv_heads, size_t head_dim, size_t max_seq_len,
                                float scale, size_t pos0, size_t m_tokens);
/* QuantizedKVCache's row write (kv_quantized.rs:143-300) for a block of m <= 128 prompt rows as the batched prefill over a byte cache
 * runs it (kv8_pf_store_kernel): kv_cache_type LGH_KV_INT8 / FP8_E4M3 / FP8_E5M2 (anything else: Unsupported); k_rows / v_rows
 * [n_kv_heads][m][head_dim] are the block's f32 rows; k_bytes / v_bytes [n_kv_heads][max_seq_len][head_dim] and, int8, k_scales /
 * v_scales [n_kv_heads][max_seq_len] (ignored for FP8, may be NULL) are in / out: rows pos0 .. pos0+m-1 come back as the launch
 * quantized them (the bytes and scale of lgh_op_kv_roundtrip), every other row as it was.  head_dim 64 / 128 (else Unsupported);
 * pos0 + m <= max_seq_len (else InvalidArgument). */
int lgh_op_pf_kv8_store(int device, uint32_t kv_cache_type, const float* k_rows, const float* v_rows, size_t m, size_t n_kv_heads, size_t head_dim,
                        size_t max_seq_len, size_t pos0, uint8_t* k_bytes, uint8_t* v_bytes, float* k_scales, float* v_scales);
/* The block attention over a byte cache (attn_pf_kv8_kernel) for m_tokens prompt tokens at positions pos0.. as the batched prefill
 * runs it: the caches already hold rows 0..pos0 + m_tokens - 1, and no row past them is read.  q [m_tokens][n_heads][head_dim];
 * out [m_tokens][n_heads * head_dim] = the kernel's f16 results widened to f32.  Limits as lgh_op_attention_prefill; Unsupported for
 * any other kv_cache_type, head_dim outside {64, 128} and n_heads / n_kv_heads outside {1, 2, 4, 8}; InvalidArgument past max_seq_len. */
int lgh_op_attention_prefill_kv8(int device, uint32_t kv_cache_type, const float* q, const uint8_t* k_bytes, const uint8_t* v_bytes,
                                 const float* k_scales, const float* v_scales, float* out, size_t n_heads, size_t n_kv_heads, size_t head_dim,
                                 size_t max_seq_len, float scale, size_t pos0, size_t m_tokens);
/* kv_prefix_copy_kernel (the one launch of lgh_prefix_save / lgh_prefix_restore, src/model/cache.rs:287-326) over host arrays, with the
 * engine's own table builder and launch: caches [n_layers][5] = per layer the K, V, K scale, V scale and K QJL tensors of n_slots
 * slots as lgh_kv_cache_layout sizes them (NULL where the format has none).  restore 0: rows [0, n_rows) of `slot` come back in
 * packed ([layer][kind][kv head][n_rows][bytes per position]); restore 1: packed goes into those rows, and every cache array comes
 * back as the device holds it afterwards. */
int lgh_op_kv_prefix_copy(int device, uint32_t kv_cache_type, uint32_t n_kv_heads, uint32_t max_seq_len, uint32_t head_dim, uint32_t n_layers,
                          uint32_t n_slots, void* const* caches, uint32_t slot, uint32_t n_rows, void* packed, int restore);
/* The engine's quantized mat-vec launches (launch_mv), one call site at a time, for kernel-level tests.  Test surface: these
 * exist to hold the kernels to a reference and are not part of the inference API.  Weights are native GGUF bytes, row-major
 * [out][in]; the library re-lays them out as lgh_upload_tensor does, so each weight runs on the kernel family the engine picks.
 *
 * layer_forward's fused QKV launch: types / w / bias hold Q, K, V (bias entries may be NULL); RMSNorm(x) * norm_w feeds all
 * three; q_out [n_heads * head_dim] is rotated at `pos` (through the device position word), and row `pos` of every head of the
 * caches [n_kv_heads][max_seq_len][head_dim] (in / out) receives the rotated K and the plain V.  Non-fused types: LGH_UNSUPPORTED. */
int lgh_op_qkv_rope(int device, const uint32_t* types, const void* const* w, const float* const* bias, const float* x, const float* norm_w,
                    float eps, size_t hidden, size_t head_dim, size_t n_heads, size_t n_kv_heads, size_t max_seq_len, size_t pos,
                    float rope_base, float rope_scale, float* q_out, float* k_cache, float* v_cache);
/* Launch A then launch B on A's output.  A: out_a = W_a . (RMSNorm(x) * norm_w, or x when norm_w is NULL) + bias_a (+ resid), or
 * with w_a_up the SwiGLU gate-up launch silu(W_a . x') * (W_a_up . x') (no bias / resid); A is asked to leave the XQ image of
 * out_a for its consumer: xq_next 0 no, 1 plain, 2 multiplied by next_nw.  B: out_b = W_b . (RMSNorm(out_a) * next_nw when
 * xq_next == 2, else out_a), [n_b][n_a], run as the engine runs it (from A's image when one was left: *image_used = 1); then
 * again into out_b_requant after the image is marked stale, which converts out_a afresh. */
int lgh_op_linear_chain(int device, uint32_t type_a, const void* w_a, const void* w_a_up, const float* bias_a, size_t k, size_t n_a,
                        const float* x, const float* norm_w, float eps, const float* resid, int xq_next, const float* next_nw,
                        uint32_t type_b, const void* w_b, size_t n_b, float* out_a, float* out_b, float* out_b_requant, int* image_used);
/* ONE launch as lgh_op_linear_chain's launch A, and everything it leaves: out [n]; with an XQ image left (*image_used = 1) the image
 * (image_out, 1280 bytes per 256 elements of n) and its n / 16 sums of squares (ssq_out, xq_next == 2 only); and with want_argmax —
 * the output projection of a greedy step — the token of the last-max arg-max that follows (*token_out), with *argmax_parts = the
 * parts the launch itself left for the merge (0: both arg-max stages ran over `out`).  *static_launches (may be NULL) = 1 when the
 * launch ran a static launch plan of csrc/matvec_mfma.hip, 0 when it ran the generic kernel. */
int lgh_op_linear_image(int device, uint32_t type, const void* w, const void* w_up, const float* bias, size_t k, size_t n, const float* x,
                        const float* norm_w, float eps, const float* resid, int xq_next, const float* next_nw, int want_argmax, float* out,
                        uint8_t* image_out, float* ssq_out, int* image_used, int* token_out, int* argmax_parts, int* static_launches);
/* The LGH_FLAG_* bits of the bare contexts every later lgh_op_* / lgh_bench_* call of this process runs on (LGH_FLAG_MV_GENERIC: the
 * same launch with and without the static launch plans).  Returns the previous value. */
uint32_t lgh_op_set_flags(uint32_t flags);
/* How many matrix-core mat-vec launches of this process ran a static launch plan so far (tests: which kernel a launch took). */
uint64_t lgh_debug_static_launches(void);
/* The matrix-core mat-vec planner's answer for a [n_rows][k] weight inside a launch of launch_rows rows in all (host only, no device):
 * out[0..6] = T k-slices, G row groups, blocks per k-slice, rows per workgroup, workgroups, threads, partial-sum floats (npass = 1).
 * Returns LGH_OK, or LGH_UNSUPPORTED for a k the planner refuses. */
int lgh_debug_mv_plan(uint32_t k, uint32_t n_rows, uint32_t launch_rows, uint32_t out[7]);
/* ffn_forward's MoE half: out = x + sum_p sel_w[p] * down_e(silu(gate_e . x') * (up_e . x')), e = sel[p], x' = RMSNorm(x) * norm_w.
 * Expert stacks in GGUF order: w_gate / w_up [n_experts][ffn][hidden], w_down [n_experts][hidden][ffn].  With `router`
 * ([n_experts][hidden] f32) the device router selects (sel / sel_w are ignored); otherwise sel / sel_w (top_k entries) drive the
 * same expert launches.  sel_out / sel_w_out (may be NULL) receive the selection used.  top_k <= 8, n_experts <= 64. */
int lgh_op_moe_experts(int device, uint32_t type_gate_up, const void* w_gate, const void* w_up, uint32_t type_down, const void* w_down,
                       size_t n_experts, size_t hidden, size_t ffn, size_t top_k, const float* router, const int* sel, const float* sel_w,
                       const float* x, const float* norm_w, float eps, float* out, int* sel_out, float* sel_w_out);
/* The multi-sequence step's mat-vec launches (lgh_forward_multi's own assembly), one at a time on n_seq <= max_batch <= 16 sequences,
 * for kernel-level tests.  Test support: not part of the inference API.  They run on the scratch lgh_batch_create allocates (the same
 * sizing rules) for a one-layer model whose widths follow from the launch; before the first launch every vector, XQ image,
 * partial-sum and cache buffer holds the NaN pattern 0x7FC0BEEF, the MoE tables in-range values: counts and selections 0x55, entry
 * lists max_batch * top_k - 1.  Every sequence's input image is made by the engine's converter, as the step's producers leave it.
 * Buffers come back for all max_batch sequences, so that rows no sequence of the call owns show the pattern.  Weights are native GGUF
 * bytes in the five matrix-core formats; a k that does not plan to 8-wave workgroups: LGH_UNSUPPORTED.  structures (int[3], may be
 * NULL): how many launches of the call ran as mvqb, as mvqb2 with the k-slices in the grid, and as mvqb2 SEQ.
 *
 * One launch on x [n_seq][k].  w_up: the SwiGLU gate | up pair (norm prologue, the step's hidden -> act); resid [n_seq][n]: a residual
 * launch with bias (wo, down: attn_out -> hidden); neither: a store (the output projection: hidden -> logits, any n; xq_next must be 0).
 * out [max_batch][n] — a store's rows lie n rounded up to a multiple of 16 apart, [max_batch][(n + 15) / 16 * 16], so that floats past
 * row n of every sequence show the pattern; image_out [max_batch][1280 bytes per 256 elements of n] and ssq_out [max_batch][n / 16 + 64] when the output has
 * image slots (the first two kinds), *image_used = 1 when the launch left them. */
int lgh_op_linear_multi(int device, uint32_t type, const void* w, const void* w_up, const float* bias, size_t k, size_t n, size_t n_seq,
                        size_t max_batch, const float* x, const float* norm_w, float eps, const float* resid, int xq_next, const float* next_nw,
                        float* out, uint8_t* image_out, float* ssq_out, int* image_used, int* structures);
/* lgh_op_linear_chain for n_seq sequences: launch A (the SwiGLU pair or a residual launch, xq_next 1 or 2) leaves every sequence's
 * image; B (a store, [n_b][n_a]) runs on A's outputs from those images, then again after they were marked stale and converted afresh.
 * out_a [n_seq][n_a]; out_b, out_b_requant [n_seq][n_b]. */
int lgh_op_linear_chain_multi(int device, uint32_t type_a, const void* w_a, const void* w_a_up, const float* bias_a, size_t k, size_t n_a, size_t n_seq,
                              size_t max_batch, const float* x, const float* norm_w, float eps, const float* resid, int xq_next, const float* next_nw,
                              uint32_t type_b, const void* w_b, size_t n_b, float* out_a, float* out_b, float* out_b_requant, int* image_used);
/* The step's fused QKV launch (three launches for formats without a common instantiation) on x [n_seq][hidden]: sequence s is rotated
 * at pos[s] and writes row pos[s] of cache slot slot[s] (distinct, < max_batch).  q_out [max_batch][n_heads * head_dim]; k_cache /
 * v_cache [max_batch][n_kv_heads][max_seq_len][head_dim] (out only); staged != 0: the quantized caches' variant — the rotated K row and
 * the V row of every sequence in staged_out [max_batch][2 * n_kv_heads * head_dim], the caches untouched (may be NULL). */
int lgh_op_qkv_rope_multi(int device, const uint32_t* types, const void* const* w, const float* const* bias, const float* x, const float* norm_w,
                          float eps, size_t hidden, size_t head_dim, size_t n_heads, size_t n_kv_heads, size_t max_seq_len, size_t n_seq,
                          size_t max_batch, const int* pos, const int* slot, float rope_base, float rope_scale, int staged, float* q_out,
                          float* k_cache, float* v_cache, float* staged_out, int* structures);
/* The grouped MoE half of a step on x [n_seq][hidden] (also the residual), n_seq >= 2: router (or the given sel / sel_w
 * [n_seq][top_k], a sequence's experts distinct), grouping, every expert's gate | up and down over its pairs, combine.  Expert stacks
 * as lgh_op_moe_experts.  out [max_batch][hidden]; image_out / ssq_out: the rows' XQ images (times next_nw) and sums of squares as
 * the combine launch left them, image_requant / ssq_requant: as the engine's converter makes them from `out` (same sizes as
 * lgh_op_linear_multi's); cnt_out [64], idx_out [64][16]: the grouping tables.  A shape the engine would not group: LGH_UNSUPPORTED. */
int lgh_op_moe_multi(int device, uint32_t type_gate_up, const void* w_gate, const void* w_up, uint32_t type_down, const void* w_down, size_t n_experts,
                     size_t hidden, size_t ffn, size_t top_k, size_t n_seq, size_t max_batch, const float* router, const int* sel, const float* sel_w,
                     const float* x, const float* norm_w, const float* next_nw, float eps, float* out, uint8_t* image_out, float* ssq_out,
                     uint8_t* image_requant, float* ssq_requant, int* sel_out, float* sel_w_out, int* cnt_out, int* idx_out, int* structures);
/* The launches of a step around the fused mat-vecs, one at a time, for kernel-level tests.  Test support: not part of the inference API.
 *
 * The embedding launches on a table of `type` (any type with a block size: F32, F16, BF16 and the quantized types), native GGUF bytes
 * [vocab][hidden].  mode 0: the single-sequence launch through embed_forward — state_io (8 ints, in / out) are the device state words
 * (token, position, next position, arg-max) before and after it; the token is state_io[0]; n = 1.  mode 1: the multi-sequence step's
 * launch over tokens[0..n), n <= 16.  mode 2: the batched prompt path's over tokens[0..n), n <= 128.  norm_w (may be NULL): the first
 * layer's QKV weights run on the matrix cores and this is their norm weight — modes 0 and 1 then also leave each row's XQ image
 * (times norm_w) and sums of squares when hidden % 256 == 0, as the engine asks for them (*image_used = 1).  Every output buffer starts
 * filled with the byte `fill`.  Modes 1 and 2 return n + 1 sequences' buffers (mode 0: one): rows_out [n + 1][hidden], image_out
 * [n + 1][1280 bytes per 256 elements of hidden], ssq_out [n + 1][hidden / 16 + 64]; the last one belongs to no sequence of the launch. */
int lgh_op_embed(int device, int mode, uint32_t type, const void* table, size_t vocab, size_t hidden, const int* tokens, size_t n,
                 const float* norm_w, int fill, int* state_io, float* rows_out, uint8_t* image_out, float* ssq_out, int* image_used);
/* qkv_forward, every branch: arguments as lgh_op_qkv_rope's, with weights of any type lgh_upload_tensor takes (the fused launch, or
 * three launches + RoPE + the cache store when a type is expanded to f32 or neox != 0: pairs (i, i + head_dim / 2)).  staged != 0: the
 * byte and TurboQuant caches' variant — the rotated K row and the V row stay in staged_out [2 * n_kv_heads * head_dim] for the
 * attention launch and the caches (in / out) are not written.  Otherwise staged_out holds what the branch staged on its way to the
 * caches (the fused launch: nothing, the NaN pattern 0x7FC0BEEF).  A refusal's message goes to err (errlen bytes; may be NULL). */
int lgh_op_qkv_forward(int device, const uint32_t* types, const void* const* w, const float* const* bias, const float* x, const float* norm_w,
                       float eps, size_t hidden, size_t head_dim, size_t n_heads, size_t n_kv_heads, size_t max_seq_len, size_t pos,
                       float rope_base, float rope_scale, int neox, int staged, float* q_out, float* k_cache, float* v_cache, float* staged_out,
                       char* err, size_t errlen);
/* ffn_gateup_forward: act_out [ffn] = silu(W_gate . x') * (W_up . x'), x' = RMSNorm(x) * norm_w, gate and up [ffn][hidden] of independent
 * types: one fused launch when both are the same fused type, else two launches and silu_mul in place on the gate's output. */
int lgh_op_ffn_gateup(int device, uint32_t type_gate, const void* w_gate, uint32_t type_up, const void* w_up, const float* x, const float* norm_w,
                      float eps, size_t hidden, size_t ffn, float* act_out);
/* The two-stage arg-max (the last maximal index wins).  n_seq == 0: the greedy step's launch over logits [n], tokens_out[0] = the token
 * it leaves in the state words; n_seq in 1 .. 16: the multi-sequence step's over logits [n_seq][n], tokens_out [n_seq]. */
int lgh_op_argmax(int device, const float* logits, size_t n, size_t n_seq, int* tokens_out);
/* Multi-sequence mat-vec launches of this process per structure so far: out[0] mvqb, out[1] mvqb2 with the k-slices in the grid,
 * out[2] mvqb2 SEQ (tests: a launch whose partial-sum buffer is too small falls back to mvqb without a word). */
void lgh_debug_mvqb_structures(uint64_t* out);
/* The batched prompt path's layer steps (prefill_block's own launch sequences), one at a time on a block of m_tokens <= 128 tokens,
 * for kernel-level tests.  Test support: not part of the inference API.  Weights are native GGUF bytes, row-major [out][in], of the
 * types the batched path takes (Q4_K, Q5_K, Q6_K, Q8_0, Q4_0); hidden_size % 256 == 0.  Before the first launch the scratch the kernels
 * read is filled with NaN bit patterns (f32 0x7FC0BEEF, f16 0x7E5A), so that a value consumed without having been produced shows in
 * the outputs.  The MoE index tables get in-range values instead, none of which the kernels may leave in a produced entry (a NaN
 * pattern read as an index would address outside the buffers): lists 0x7F7F, tokmap 383, rowmap 0, selection / counts / bases 0x55.
 *
 * QKV step: hidden [m_tokens][hidden_size] f32 -> XH(hidden * norm_w) and sums of squares, the q|k|v GEMM, then 1/rms, bias, RoPE
 * (neox: pairs (i, i + d/2)) at positions pos0 + t.  q_out [m_tokens][n_heads * head_dim]; the caches
 * [n_kv_heads][max_seq_len][head_dim] are in / out (the caller's sentinels survive outside rows pos0 .. pos0 + m_tokens - 1). */
int lgh_op_pf_qkv(int device, const uint32_t* types, const void* const* w, const float* const* bias, const float* hidden, const float* norm_w,
                  float eps, size_t hidden_size, size_t head_dim, size_t n_heads, size_t n_kv_heads, int neox, size_t max_seq_len, size_t pos0,
                  size_t m_tokens, float rope_base, float rope_scale, float* q_out, float* k_cache, float* v_cache);
/* wo step: x [m_tokens][k] f32 (-> XH as the attention output arrives), hidden_out = resid + W . x (+ bias), W [hidden_size][k];
 * xh_out [m_tokens][hidden_size] = the next XH f16(hidden_out * next_nw) widened to f32; ssq_out [m_tokens][8] = the tokens' sums of
 * squares per 2048 columns (entries past the row's chunks are not written). */
int lgh_op_pf_linear(int device, uint32_t type, const void* w, const float* bias, const float* x, size_t k, size_t hidden_size, const float* resid,
                     const float* next_nw, size_t m_tokens, float* hidden_out, float* xh_out, float* ssq_out);
/* dense FFN step: hidden_out = hidden + W_down . (silu(W_gate . x') * (W_up . x')), x' = RMSNorm(hidden) * norm_w; next_nw may be NULL
 * (no next XH is written; xh_out is untouched).  act_out (may be NULL) [m_tokens][ffn]: the f16 SwiGLU output the down GEMM read. */
int lgh_op_pf_ffn(int device, uint32_t type_gate_up, const void* w_gate, const void* w_up, uint32_t type_down, const void* w_down,
                  const float* hidden, const float* norm_w, const float* next_nw, float eps, size_t hidden_size, size_t ffn, size_t m_tokens,
                  float* hidden_out, float* xh_out, float* ssq_out, float* act_out);
/* MoE FFN step: the device router, the grouping of the (token, slot) pairs by expert, every expert once over its rows, the combine.
 * Expert stacks as lgh_op_moe_experts.  sel_out / sel_w_out / tokmap_out [m_tokens][top_k]; counts_out / bases_out [n_experts];
 * lists_out [n_experts][128] (entries past an expert's count keep the fill 0x7F7F); rowmap_out [384], the whole table (expert |
 * row << 8, -1 written by the grouping kernel on every padding row); act_out (may be NULL) [n_experts][128][ffn]: every expert's f16 SwiGLU rows as its
 * down GEMM read them (rows past the expert's count hold the NaN fill).  LGH_UNSUPPORTED where the batched path does not take the routing shape
 * (128 * top_k + 15 * n_experts > 384). */
int lgh_op_pf_moe(int device, uint32_t type_gate_up, const void* w_gate, const void* w_up, uint32_t type_down, const void* w_down,
                  const float* router, size_t n_experts, size_t top_k, const float* hidden, const float* norm_w, const float* next_nw, float eps,
                  size_t hidden_size, size_t ffn, size_t m_tokens, float* hidden_out, float* xh_out, float* ssq_out, int* sel_out, float* sel_w_out,
                  int* counts_out, int* bases_out, int* lists_out, int* rowmap_out, int* tokmap_out, float* act_out);
/* Device-resident weights by tensor name for the per-op surface: `CudaBackend::load_model_weights` and the `b.name()`
 * lookups in its vec_mat / vec_mat_q (src/backend/cuda/mod.rs:121-146, 436-470, 511-575).  A weight is uploaded once
 * (native GGUF bytes; the library re-lays it out as lgh_upload_tensor does) and later calls name it. */
typedef struct lgh_backend lgh_backend;
int lgh_backend_create(int device, lgh_backend** out);
void lgh_backend_destroy(lgh_backend* be);
int lgh_backend_load_weight(lgh_backend* be, const char* name, uint32_t ggml_type, const void* w, size_t k, size_t n);
int lgh_backend_has_weight(const lgh_backend* be, const char* name);
int lgh_backend_vec_mat_q(lgh_backend* be, const char* name, const float* x, float* out, size_t k, size_t n);
const char* lgh_backend_last_error(const lgh_backend* be);
/* fused decode kernels, for kernel-level parity: out = resid + W.(rms_norm(x)*norm_w) etc. */
int lgh_op_norm_vec_mat(int device, uint32_t ggml_type, const void* w, const float* x, const float* norm_w, float eps,
                        float* out, size_t k, size_t n);
int lgh_op_swiglu_vec_mat(int device, uint32_t ggml_type, const void* w_gate, const void* w_up, const float* x,
                          const float* norm_w, float eps, float* out, size_t k, size_t n);

/* Micro-benchmark of the fused quantized mat-vec kernel on device-resident synthetic data:
 * `iters` back-to-back launches timed with hipEvents on the launch stream.  mode 0 = plain matvec,
 * 1 = rmsnorm prologue, 2 = gate/up SwiGLU pair.  `copies` device copies of the weights are cycled so the
 * 256 MiB Infinity Cache does not serve re-reads.  avg_us = mean device time per launch. */
int lgh_bench_vec_mat(int device, uint32_t ggml_type, const void* w, const void* w2, size_t k, size_t n, int mode,
                      int iters, int copies, double* avg_us);

/* ---- GGUF -> HBM direct loader: replaces GgufReader + ModelLoader::parse_config + from_model for this engine
 * (src/gguf/reader.rs:49-104, src/model/loader.rs:62-170, src/backend/cuda/dequant_weights.rs:244-505).  The file is mapped
 * and every tensor the engine knows is uploaded straight from the mapping in native GGUF layout. ---- */
typedef struct lgh_gguf_info {
  uint32_t version;                  /* GGUF version (1..3) */
  uint32_t alignment;                /* general.alignment (default 32) */
  uint64_t n_tensors, n_kv;
  uint64_t data_offset, file_bytes;
  char architecture[64];             /* general.architecture */
  lgh_model_desc desc;               /* what ModelLoader::parse_config reads from the `{arch}.*` keys; max_seq_len = context_length */
} lgh_gguf_info;
/* GgufReader::new + read (src/gguf/reader.rs:24-104), header only, no GPU needed.  Accepts every well-formed GGUF v1-v3 as
 * the reference's reader does; when the `{arch}.*` keys of a model this engine runs are absent, desc.struct_size is 0 (and
 * `err` says which key is missing) while version / counts / alignment / data_offset are still filled.  Failures carry the
 * reference's GgufError texts (src/gguf/error.rs:2-19): "Invalid magic number: ...", "Unsupported GGUF version: N"
 * (status LGH_UNSUPPORTED), "Unexpected end of file". */
int lgh_gguf_inspect(const char* path, lgh_gguf_info* out, char* err, size_t errlen);
/* One metadata value by key: GgufData::get_string / get_u32 / get_u64 / get_f32 / get_bool (src/gguf/types.rs:71-104).
 * type = GGUF value type (0 u8, 1 i8, 2 u16, 3 i16, 4 u32, 5 i32, 6 f32, 7 bool, 8 string, 9 array, 10 u64, 11 i64, 12 f64);
 * integers (sign-extended) and bools in `u`, floats in `f`, strings in `s` (truncated to 255 bytes), arrays: only `arr_len`. */
typedef struct lgh_gguf_value {
  uint32_t type;
  uint32_t reserved;
  uint64_t u;
  double f;
  uint64_t arr_len;
  char s[256];
} lgh_gguf_value;
int lgh_gguf_get(const char* path, const char* key, lgh_gguf_value* out, char* err, size_t errlen);
/* create + upload + finalize from a GGUF file.  max_seq_len 0 = the file's context_length; layer_begin/end 0,0 = all. */
int lgh_load_gguf(const char* path, uint32_t max_seq_len, int device, uint32_t flags, uint32_t layer_begin, uint32_t layer_end,
                  lgh_ctx** out, char* err, size_t errlen);

/* Streaming-read probe: `iters` passes over a `bytes`-long device buffer with 16-byte non-temporal loads from every CU
 * (the access pattern of the weight stream); gbps = bytes * iters / device time.  The practical HBM ceiling the decode
 * roofline is also quoted against (bench.py: hbm_roofline.measured_read_peak_GBps). */
int lgh_bench_hbm_read(int device, size_t bytes, int iters, double* gbps);

#ifdef __cplusplus
}
#endif
#endif
