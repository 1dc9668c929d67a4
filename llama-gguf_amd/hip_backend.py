"""Host-side mirror of the reference's GPU-engine interface over the C ABI (include/llama_gguf_hip.h).

The reference drives every GPU engine through ``trait GpuInference`` (src/backend/mod.rs:283-296:
``forward / prefill_token / reset / position``), builds it with ``from_model(model, max_seq_len)``
(src/backend/cuda/gpu_only.rs:426) and adapts it to ``trait Model`` with ``GpuModelWrapper``
(src/backend/mod.rs:302-364).  The reference is Rust and this image has no Rust toolchain, so the
Rust shim is shipped as source in INTEGRATION.md; this module is the same surface — same names,
argument meaning and error behaviour — for the tests and the benchmark.  Nothing here computes: every
call goes through ``lib/libllama_gguf_hip.so`` and FAILS LOUDLY if that library or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LGH_LIB_VARIANT=stamps selects the diagnostic build (in-kernel phase stamps; tools/microbench.py only)
LIB_PATH = os.path.join(_HERE, "lib", "libllama_gguf_hip%s.so" % ("_" + os.environ["LGH_LIB_VARIANT"] if os.environ.get("LGH_LIB_VARIANT") else ""))

# every symbol include/llama_gguf_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = (
    "lgh_device_count", "lgh_create", "lgh_upload_tensor", "lgh_finalize", "lgh_destroy", "lgh_forward",
    "lgh_prefill_token", "lgh_prefill_batch", "lgh_prefill_is_batched", "lgh_set_prefill_policy", "lgh_op_mat_mat",
    "lgh_op_kv_roundtrip", "lgh_op_add", "lgh_op_mul", "lgh_op_scale", "lgh_op_silu", "lgh_op_gelu", "lgh_op_softmax", "lgh_op_matmul", "lgh_op_matvec",
    "lgh_op_matvec_q", "lgh_op_attention", "lgh_backend_create", "lgh_backend_destroy", "lgh_backend_load_weight",
    "lgh_backend_has_weight", "lgh_backend_vec_mat_q", "lgh_backend_last_error", "lgh_reset", "lgh_position", "lgh_kv_truncate", "lgh_kv_shift_left", "lgh_stage_prefill_batch", "lgh_stage_hidden_block_buffer", "lgh_forward_argmax", "lgh_decode_greedy",
    "lgh_last_error", "lgh_get_stats", "lgh_set_profiling", "lgh_set_stream", "lgh_get_stream", "lgh_synchronize",
    "lgh_read_hidden", "lgh_stage_hidden_buffer", "lgh_stage_forward", "lgh_op_dequantize", "lgh_op_vec_mat",
    "lgh_op_rms_norm", "lgh_op_rope", "lgh_op_attention_cached", "lgh_op_silu_mul", "lgh_op_norm_vec_mat",
    "lgh_op_swiglu_vec_mat", "lgh_bench_vec_mat", "lgh_bench_hbm_read", "lgh_gguf_inspect", "lgh_load_gguf",
    "lgh_stage_io_buffers", "lgh_stage_set_forward_targets", "lgh_stage_step", "lgh_stage_read_tokens", "lgh_gguf_get", "lgh_stage_read_logits",
    "lgh_pipeline_create", "lgh_pipeline_upload_tensor", "lgh_pipeline_finalize", "lgh_pipeline_destroy", "lgh_pipeline_forward",
    "lgh_pipeline_prefill_token", "lgh_pipeline_decode_greedy", "lgh_pipeline_reset", "lgh_pipeline_position", "lgh_pipeline_kv_truncate", "lgh_pipeline_stages",
    "lgh_pipeline_last_error",
    "lgh_tp_create", "lgh_tp_upload_tensor", "lgh_tp_finalize", "lgh_tp_destroy", "lgh_tp_forward", "lgh_tp_prefill_token", "lgh_tp_decode_greedy",
    "lgh_tp_reset", "lgh_tp_position", "lgh_tp_kv_truncate", "lgh_tp_ranks", "lgh_tp_graph_nodes", "lgh_tp_last_error", "lgh_tp_shard", "lgh_op_tp_reduce",
    "lgh_tp_prefill_batch", "lgh_tp_prefill_is_batched", "lgh_tp_get_stats", "lgh_op_tp_pf_reduce",
    "lgh_set_kv_rotation_signs", "lgh_op_tq_compress", "lgh_set_kv_qjl_matrices", "lgh_op_tq_compress_qjl",
    "lgh_batch_create", "lgh_batch_reset", "lgh_batch_position", "lgh_batch_prefill", "lgh_forward_multi", "lgh_decode_greedy_multi",
    "lgh_set_sampler", "lgh_decode_sample", "lgh_batch_set_sampler", "lgh_decode_sample_multi", "lgh_op_sample",
    "lgh_set_sampler_ex", "lgh_batch_set_sampler_ex", "lgh_get_sampler_mu", "lgh_op_sample_ex",
    "lgh_op_attention_decode", "lgh_op_attention_decode_multi", "lgh_op_attention_kv8", "lgh_op_attention_tq", "lgh_op_attention_prefill",
    "lgh_op_qkv_rope", "lgh_op_linear_chain", "lgh_op_moe_experts", "lgh_op_linear_image", "lgh_op_set_flags", "lgh_debug_static_launches", "lgh_debug_mv_plan",
    "lgh_op_pf_qkv", "lgh_op_pf_linear", "lgh_op_pf_ffn", "lgh_op_pf_moe",
    "lgh_op_linear_multi", "lgh_op_linear_chain_multi", "lgh_op_qkv_rope_multi", "lgh_op_moe_multi", "lgh_debug_mvqb_structures",
    "lgh_op_pf_tq_store", "lgh_op_attention_prefill_tq", "lgh_op_pf_kv8_store", "lgh_op_attention_prefill_kv8", "lgh_op_attention_kv8_multi", "lgh_op_attention_tq_multi",
    "lgh_op_embed", "lgh_op_qkv_forward", "lgh_op_ffn_gateup", "lgh_op_argmax", "lgh_kv_cache_layout",
    "lgh_prefix_save", "lgh_prefix_restore", "lgh_prefix_free", "lgh_prefix_get_info", "lgh_prefix_total_bytes", "lgh_prefix_export",
    "lgh_prefix_import", "lgh_op_kv_prefix_copy",
)

K_NAMES = ("embed", "qkv", "attn", "attn_combine", "wo", "gate_up", "down", "router", "output", "argmax", "misc", "token")
K_COUNT = 16
SYM_COUNT = 24
# kernel symbols as rocprofv3 prints them (LGH_SYM_* order)
SYM_NAMES = ("lgh::mv_kernel<1u, 1024>", "lgh::mv_kernel<8u, 1024>", "lgh::mv_kernel<16u, 1024>",
             "lgh::mv_kernel<2u, 768>", "lgh::mv_kernel<4u, 512>", "lgh::mv_kernel<5u, 512>", "lgh::mv_kernel<6u, 512>",
             "lgh::mv_kernel<31u, 512>", "lgh::f32_matvec_kernel", "lgh::attn_partial_kernel", "lgh::attn_combine_kernel",
             "lgh::embed_kernel", "lgh::argmax_stage1+2", "lgh::moe_router_kernel", "other", "lgh::mvq_kernel<1u>", "lgh::mvq_kernel<2u>", "lgh::mvq_kernel<3u>", "lgh::mvq_kernel<4u>",
             "lgh::mvq_kernel<8u>", "unused")
FLAG_NO_GRAPH = 1
PREFILL_BATCH_BYTE_KV = 1   # lgh_set_prefill_policy: int8 / FP8 caches take the batched prompt pass (own sequence, slots, stage contexts)
FLAG_EXACT_PREFILL = 4   # forward_batch feeds tokens one by one (f32 throughout) instead of the batched f16 GEMM path
KV_F32, KV_INT8, KV_FP8_E4M3, KV_FP8_E5M2 = 0, 1, 2, 3   # lgh_model_desc.kv_cache_type: f32, or QuantizedKVCache's formats (kv_quantized.rs; no CLI flag reaches them)
KV_TQ2, KV_TQ3 = 4, 5   # KVCacheType::TurboQuantMSE { bits: 2 | 3 }: what `--kv-cache-type tq2 | tq3` selects (src/config.rs:808-817)
KV_TQ2_QJL, KV_TQ3_QJL = 6, 7   # KVCacheType::TurboQuantProd { bits: 2 | 3 }: `tq2-qjl | tq3-qjl`
FLAG_KV_INT8 = 16   # KV cache in the reference's int8 format (kv_quantized.rs: int8 rows + one scale per head and position)
FLAG_MV_GENERIC = 1 << 31   # matrix-core mat-vecs ignore the static launch plans (A/B runs, tests); same bits
FLAG_REMOVED_MASK = 2 | 8 | 32 | 64 | 128 | (0x7F << 24)   # round-2 decode experiments, removed in round 3: lgh_create answers Unsupported


class BackendError(RuntimeError):
    """The reference's BackendError (src/backend/error.rs:3-37); `.variant` names the Rust variant."""
    VARIANTS = {1: "NotAvailable", 2: "ShapeMismatch", 3: "DTypeMismatch", 4: "UnsupportedDType", 5: "Unsupported",
                6: "InvalidArgument", 7: "Tensor", 8: "InitializationFailed", 9: "AllocationFailed",
                10: "OperationFailed"}

    def __init__(self, status: int, message: str = ""):
        self.status = status
        self.variant = self.VARIANTS.get(status, f"Status{status}")
        super().__init__(f"{self.variant}: {message}" if message else self.variant)


class ModelDesc(C.Structure):
    _fields_ = ([(n, C.c_uint32) for n in (
        "struct_size", "hidden_size", "intermediate_size", "num_layers", "num_heads", "num_kv_heads", "head_dim",
        "vocab_size", "max_seq_len", "num_experts", "num_experts_per_token", "expert_intermediate_size",
        "use_neox_rope")]
                + [(n, C.c_float) for n in ("norm_eps", "rope_freq_base", "rope_freq_scale")]
                + [("device_id", C.c_int32), ("layer_begin", C.c_uint32), ("layer_end", C.c_uint32),
                   ("flags", C.c_uint32), ("kv_cache_type", C.c_uint32)])


class KvLayout(C.Structure):
    """lgh_kv_layout: a KV cache format's bytes per (kv head, position) and per slot of one layer."""
    _fields_ = ([(n, C.c_uint32) for n in ("kv_cache_type", "row_bytes", "scale_bytes", "qjl_bytes")]
                + [(n, C.c_uint64) for n in ("rows", "k_bytes", "v_bytes", "k_scale_bytes", "v_scale_bytes", "k_qjl_bytes", "slot_bytes")])


class PrefixInfo(C.Structure):
    """lgh_prefix_info: what a saved KV prefix holds."""
    _fields_ = ([(n, C.c_uint32) for n in ("struct_size", "kv_cache_type", "n_rows", "layer_begin", "layer_end")] + [("bytes", C.c_uint64)])


class GgufInfo(C.Structure):
    _fields_ = [("version", C.c_uint32), ("alignment", C.c_uint32), ("n_tensors", C.c_uint64), ("n_kv", C.c_uint64),
                ("data_offset", C.c_uint64), ("file_bytes", C.c_uint64), ("architecture", C.c_char * 64), ("desc", ModelDesc)]


class GgufValue(C.Structure):
    _fields_ = [("type", C.c_uint32), ("reserved", C.c_uint32), ("u", C.c_uint64), ("f", C.c_double), ("arr_len", C.c_uint64),
                ("s", C.c_char * 256)]


class SamplerConfig(C.Structure):
    """lgh_sampler_config: SamplerConfig (src/sampling/mod.rs:37-62) minus seed / typical_p; min_p and mirostat: SamplerConfigEx."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_uint32), ("top_p", C.c_float), ("repeat_penalty", C.c_float),
                ("repeat_window", C.c_uint32), ("frequency_penalty", C.c_float), ("presence_penalty", C.c_float),
                ("eos_token", C.c_int32)]


class SamplerConfigEx(C.Structure):
    """lgh_sampler_config_ex: lgh_sampler_config plus min_p (mod.rs:248-258) and MirostatConfig (mod.rs:15-34)."""
    _fields_ = [("struct_size", C.c_uint32), ("base", SamplerConfig), ("min_p", C.c_float), ("mirostat", C.c_uint32),
                ("mirostat_tau", C.c_float), ("mirostat_eta", C.c_float)]


# SamplerConfig presets of the reference (sampling/mod.rs:64-122) and EngineConfig::default's settings (src/engine.rs:117-130)
SAMPLER_PRESETS = {
    "engine_default": dict(temperature=0.7, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_window=64),
    "sampler_default": dict(temperature=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_window=64),
    "greedy": dict(temperature=0.0, top_k=1, top_p=1.0, repeat_penalty=1.0, repeat_window=0),
    "creative": dict(temperature=1.0, top_k=0, top_p=0.9, repeat_penalty=1.2, repeat_window=64),
    # SamplerConfig::creative as the reference has it, min_p included (sampling/mod.rs:100-114)
    "creative_ref": dict(temperature=1.0, top_k=0, top_p=0.9, repeat_penalty=1.2, repeat_window=64, min_p=0.05),
    # SamplerConfig::mirostat_v2(5.0, 0.1) (sampling/mod.rs:116-135; MirostatConfig::default's tau and eta)
    "mirostat_v2": dict(temperature=1.0, top_k=0, top_p=1.0, repeat_penalty=1.0, repeat_window=0, mirostat=2, tau=5.0, eta=0.1),
}


def sampler_config(temperature: float = 0.8, top_k: int = 40, top_p: float = 0.95, repeat_penalty: float = 1.1,
                   repeat_window: int = 64, frequency_penalty: float = 0.0, presence_penalty: float = 0.0,
                   eos_token: int = -1) -> SamplerConfig:
    """An lgh_sampler_config; the defaults are SamplerConfig::default's (sampling/mod.rs:64-80)."""
    return SamplerConfig(temperature, top_k, top_p, repeat_penalty, repeat_window, frequency_penalty, presence_penalty, eos_token)


_EX_KEYS = ("min_p", "mirostat", "tau", "eta")


def sampler_config_ex(min_p: float = 0.0, mirostat: int = 0, tau: float = 5.0, eta: float = 0.1, **cfg) -> SamplerConfigEx:
    """An lgh_sampler_config_ex: `sampler_config`'s keywords plus min_p and mirostat (0 off, 1, 2) with tau / eta, whose defaults
    are MirostatConfig::default's (sampling/mod.rs:26-34)."""
    return SamplerConfigEx(C.sizeof(SamplerConfigEx), sampler_config(**cfg), min_p, mirostat, tau, eta)


def _is_ex(cfg) -> bool:
    return any(k in cfg for k in _EX_KEYS)


class Stats(C.Structure):
    _fields_ = [("weight_bytes", C.c_uint64), ("kv_bytes", C.c_uint64), ("scratch_bytes", C.c_uint64),
                ("tokens_processed", C.c_uint64), ("graph_nodes", C.c_uint64),
                ("k_launches", C.c_uint64 * K_COUNT), ("k_time_us", C.c_double * K_COUNT),
                ("k_alg_bytes", C.c_uint64 * K_COUNT),
                ("sym_launches", C.c_uint64 * SYM_COUNT), ("sym_time_us", C.c_double * SYM_COUNT),
                ("sym_alg_bytes", C.c_uint64 * SYM_COUNT), ("step_alg_bytes", C.c_uint64),
                ("event_bracket_us", C.c_double), ("event_bracket_samples", C.c_uint64), ("overlapped_edges", C.c_uint64)]


_lib = None


def load_library() -> C.CDLL:
    """dlopen the engine.  Raises (never falls back) when the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendError(8, f"{LIB_PATH} is missing: build it with `make -C {_HERE}` or __graft_entry__.build()")
    L = C.CDLL(LIB_PATH)
    vp, sz, u32, f32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_float
    sig = {
        "lgh_device_count": (C.c_int, []),
        "lgh_create": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(vp)]),
        "lgh_upload_tensor": (C.c_int, [vp, C.c_char_p, u32, C.POINTER(C.c_uint64), vp, sz]),
        "lgh_finalize": (C.c_int, [vp]), "lgh_destroy": (None, [vp]),
        "lgh_forward": (C.c_int, [vp, u32, vp]), "lgh_prefill_token": (C.c_int, [vp, u32]),
        "lgh_prefill_batch": (C.c_int, [vp, vp, sz]), "lgh_prefill_is_batched": (C.c_int, [vp]),
        "lgh_set_prefill_policy": (C.c_int, [vp, C.c_uint32]),
        "lgh_op_mat_mat": (C.c_int, [C.c_int, u32, vp, vp, vp, sz, sz, sz]), "lgh_reset": (None, [vp]), "lgh_position": (sz, [vp]),
        "lgh_kv_truncate": (C.c_int, [vp, sz]), "lgh_kv_shift_left": (C.c_int, [vp, sz]),
        "lgh_stage_prefill_batch": (C.c_int, [vp, vp, sz]), "lgh_stage_hidden_block_buffer": (C.c_int, [vp, C.POINTER(vp)]),
        "lgh_forward_argmax": (C.c_int, [vp, u32, C.POINTER(u32)]),
        "lgh_decode_greedy": (C.c_int, [vp, u32, sz, vp]),
        "lgh_last_error": (C.c_char_p, [vp]), "lgh_get_stats": (C.c_int, [vp, C.POINTER(Stats)]),
        "lgh_set_profiling": (C.c_int, [vp, C.c_int]), "lgh_set_stream": (C.c_int, [vp, vp]),
        "lgh_get_stream": (vp, [vp]), "lgh_synchronize": (C.c_int, [vp]), "lgh_read_hidden": (C.c_int, [vp, vp]),
        "lgh_stage_hidden_buffer": (C.c_int, [vp, C.POINTER(vp)]),
        "lgh_stage_forward": (C.c_int, [vp, u32, C.c_int, vp, C.POINTER(u32)]),
        "lgh_op_dequantize": (C.c_int, [C.c_int, u32, vp, sz, vp]),
        "lgh_op_vec_mat": (C.c_int, [C.c_int, u32, vp, vp, vp, sz, sz]),
        "lgh_op_rms_norm": (C.c_int, [C.c_int, vp, vp, f32, vp, sz]),
        "lgh_op_rope": (C.c_int, [C.c_int, vp, vp, sz, sz, sz, sz, f32, f32, C.c_int]),
        "lgh_op_attention_cached": (C.c_int, [C.c_int, vp, vp, vp, vp, sz, sz, sz, sz, f32, sz, C.c_int]),
        "lgh_op_silu_mul": (C.c_int, [C.c_int, vp, vp, vp, sz]),
        "lgh_op_norm_vec_mat": (C.c_int, [C.c_int, u32, vp, vp, vp, f32, vp, sz, sz]),
        "lgh_op_swiglu_vec_mat": (C.c_int, [C.c_int, u32, vp, vp, vp, vp, f32, vp, sz, sz]),
        "lgh_op_add": (C.c_int, [C.c_int, vp, vp, vp, sz]), "lgh_op_mul": (C.c_int, [C.c_int, vp, vp, vp, sz]),
        "lgh_op_kv_roundtrip": (C.c_int, [C.c_int, C.c_uint32, vp, sz, vp, vp, vp]),
        "lgh_op_scale": (C.c_int, [C.c_int, vp, f32, vp, sz]), "lgh_op_silu": (C.c_int, [C.c_int, vp, vp, sz]),
        "lgh_op_gelu": (C.c_int, [C.c_int, vp, vp, sz]), "lgh_op_softmax": (C.c_int, [C.c_int, vp, vp, sz, sz]),
        "lgh_op_matmul": (C.c_int, [C.c_int, vp, vp, vp, sz, sz, sz]), "lgh_op_matvec": (C.c_int, [C.c_int, vp, vp, vp, sz, sz]),
        "lgh_op_matvec_q": (C.c_int, [C.c_int, u32, vp, vp, vp, sz, sz]),
        "lgh_op_attention": (C.c_int, [C.c_int, vp, vp, vp, vp, sz, sz, sz, sz, sz, f32]),
        "lgh_backend_create": (C.c_int, [C.c_int, C.POINTER(vp)]), "lgh_backend_destroy": (None, [vp]),
        "lgh_backend_load_weight": (C.c_int, [vp, C.c_char_p, u32, vp, sz, sz]), "lgh_backend_has_weight": (C.c_int, [vp, C.c_char_p]),
        "lgh_backend_vec_mat_q": (C.c_int, [vp, C.c_char_p, vp, vp, sz, sz]), "lgh_backend_last_error": (C.c_char_p, [vp]),
        "lgh_bench_vec_mat": (C.c_int, [C.c_int, u32, vp, vp, sz, sz, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
        "lgh_bench_hbm_read": (C.c_int, [C.c_int, sz, C.c_int, C.POINTER(C.c_double)]),
        "lgh_gguf_inspect": (C.c_int, [C.c_char_p, C.POINTER(GgufInfo), C.c_char_p, sz]),
        "lgh_load_gguf": (C.c_int, [C.c_char_p, u32, C.c_int, u32, u32, u32, C.POINTER(vp), C.c_char_p, sz]),
        "lgh_stage_io_buffers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]), "lgh_stage_set_forward_targets": (C.c_int, [vp, vp, vp]), "lgh_stage_step": (C.c_int, [vp, C.c_int]),
        "lgh_stage_read_tokens": (C.c_int, [vp, sz, sz, vp]),
        "lgh_gguf_get": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(GgufValue), C.c_char_p, sz]),
        "lgh_stage_read_logits": (C.c_int, [vp, vp]),
        "lgh_pipeline_create": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]),
        "lgh_pipeline_upload_tensor": (C.c_int, [vp, C.c_char_p, u32, C.POINTER(C.c_uint64), vp, sz]),
        "lgh_pipeline_finalize": (C.c_int, [vp]), "lgh_pipeline_destroy": (None, [vp]),
        "lgh_pipeline_forward": (C.c_int, [vp, u32, vp]), "lgh_pipeline_prefill_token": (C.c_int, [vp, u32]),
        "lgh_pipeline_decode_greedy": (C.c_int, [vp, u32, sz, vp]), "lgh_pipeline_reset": (None, [vp]),
        "lgh_pipeline_position": (sz, [vp]), "lgh_pipeline_kv_truncate": (C.c_int, [vp, sz]), "lgh_pipeline_stages": (C.c_int, [vp]), "lgh_pipeline_last_error": (C.c_char_p, [vp]),
        "lgh_tp_create": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]),
        "lgh_tp_upload_tensor": (C.c_int, [vp, C.c_char_p, u32, C.POINTER(C.c_uint64), vp, sz]),
        "lgh_tp_finalize": (C.c_int, [vp]), "lgh_tp_destroy": (None, [vp]),
        "lgh_tp_forward": (C.c_int, [vp, u32, vp]), "lgh_tp_prefill_token": (C.c_int, [vp, u32]),
        "lgh_tp_decode_greedy": (C.c_int, [vp, u32, sz, vp]), "lgh_tp_reset": (None, [vp]),
        "lgh_tp_position": (sz, [vp]), "lgh_tp_kv_truncate": (C.c_int, [vp, sz]), "lgh_tp_ranks": (C.c_int, [vp]),
        "lgh_tp_graph_nodes": (C.c_uint64, [vp]), "lgh_tp_last_error": (C.c_char_p, [vp]),
        "lgh_tp_shard": (C.c_int, [u32, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, vp, sz, vp, sz, C.POINTER(sz)]),
        "lgh_op_tp_reduce": (C.c_int, [C.c_int, vp, u32, vp, vp, sz, vp, vp, vp]),
        "lgh_tp_prefill_batch": (C.c_int, [vp, vp, sz]), "lgh_tp_prefill_is_batched": (C.c_int, [vp]),
        "lgh_tp_get_stats": (C.c_int, [vp, C.c_int, C.POINTER(Stats)]),
        "lgh_op_tp_pf_reduce": (C.c_int, [C.c_int, C.c_int, vp, u32, u32, sz, sz, vp, vp, vp, sz, sz, vp, vp, vp]),
        "lgh_set_kv_rotation_signs": (C.c_int, [vp, vp, sz]), "lgh_op_tq_compress": (C.c_int, [C.c_int, C.c_int, vp, sz, vp, vp]),
        "lgh_set_kv_qjl_matrices": (C.c_int, [vp, vp, sz]), "lgh_op_tq_compress_qjl": (C.c_int, [C.c_int, C.c_int, vp, sz, vp, vp, vp, vp, vp]),
        "lgh_batch_create": (C.c_int, [vp, u32]), "lgh_batch_reset": (C.c_int, [vp, u32]), "lgh_batch_position": (sz, [vp, u32]),
        "lgh_batch_prefill": (C.c_int, [vp, u32, vp, sz]), "lgh_forward_multi": (C.c_int, [vp, vp, vp, u32, vp, vp]),
        "lgh_decode_greedy_multi": (C.c_int, [vp, vp, vp, u32, sz, vp]),
        "lgh_set_sampler": (C.c_int, [vp, C.POINTER(SamplerConfig)]),
        "lgh_decode_sample": (C.c_int, [vp, u32, vp, sz, sz, vp, vp]),
        "lgh_batch_set_sampler": (C.c_int, [vp, u32, C.POINTER(SamplerConfig)]),
        "lgh_decode_sample_multi": (C.c_int, [vp, vp, vp, u32, vp, vp, sz, vp, vp]),
        "lgh_op_sample": (C.c_int, [C.c_int, vp, sz, C.POINTER(SamplerConfig), vp, sz, vp, f32, C.POINTER(u32)]),
        "lgh_set_sampler_ex": (C.c_int, [vp, C.POINTER(SamplerConfigEx)]),
        "lgh_batch_set_sampler_ex": (C.c_int, [vp, u32, C.POINTER(SamplerConfigEx)]),
        "lgh_get_sampler_mu": (C.c_int, [vp, C.c_int, C.POINTER(f32)]),
        "lgh_op_sample_ex": (C.c_int, [C.c_int, vp, sz, C.POINTER(SamplerConfigEx), vp, sz, vp, f32, f32, C.POINTER(u32), C.POINTER(f32)]),
        "lgh_op_attention_decode": (C.c_int, [C.c_int, C.c_int, vp, vp, vp, vp, sz, sz, sz, sz, f32, sz, C.c_int, vp]),
        "lgh_op_attention_decode_multi": (C.c_int, [C.c_int, vp, vp, vp, vp, sz, sz, sz, sz, sz, sz, vp, vp, f32, C.c_int, vp]),
        "lgh_op_attention_kv8": (C.c_int, [C.c_int, u32, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, sz, f32, sz, C.c_int, vp]),
        "lgh_op_attention_kv8_multi": (C.c_int, [C.c_int, u32, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, sz, sz, sz, vp, vp, f32, C.c_int, vp]),
        "lgh_op_attention_tq": (C.c_int, [C.c_int, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, sz, f32, sz, C.c_int, vp]),
        "lgh_op_attention_tq_multi": (C.c_int, [C.c_int, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, sz, sz, sz, vp, vp, f32, C.c_int, vp]),
        "lgh_op_attention_prefill": (C.c_int, [C.c_int, vp, vp, vp, vp, sz, sz, sz, sz, f32, sz, sz]),
        "lgh_op_pf_tq_store": (C.c_int, [C.c_int, u32, vp, vp, sz, sz, sz, sz, sz, vp, vp, vp]),
        "lgh_op_attention_prefill_tq": (C.c_int, [C.c_int, u32, vp, vp, vp, vp, vp, sz, sz, sz, sz, f32, sz, sz]),
        "lgh_op_pf_kv8_store": (C.c_int, [C.c_int, u32, vp, vp, sz, sz, sz, sz, sz, vp, vp, vp, vp]),
        "lgh_op_attention_prefill_kv8": (C.c_int, [C.c_int, u32, vp, vp, vp, vp, vp, vp, sz, sz, sz, sz, f32, sz, sz]),
        "lgh_op_qkv_rope": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, f32, sz, sz, sz, sz, sz, sz, f32, f32, vp, vp, vp]),
        "lgh_op_linear_image": (C.c_int, [C.c_int, u32, vp, vp, vp, sz, sz, vp, vp, f32, vp, C.c_int, vp, C.c_int, vp, vp, vp,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "lgh_op_set_flags": (u32, [u32]),
        "lgh_debug_static_launches": (C.c_uint64, []),
        "lgh_debug_mv_plan": (C.c_int, [u32, u32, u32, C.POINTER(C.c_uint32)]),
        "lgh_op_linear_chain": (C.c_int, [C.c_int, u32, vp, vp, vp, sz, sz, vp, vp, f32, vp, C.c_int, vp, u32, vp, sz, vp, vp, vp,
                                          C.POINTER(C.c_int)]),
        "lgh_op_moe_experts": (C.c_int, [C.c_int, u32, vp, vp, u32, vp, sz, sz, sz, sz, vp, vp, vp, vp, vp, f32, vp, vp, vp]),
        "lgh_op_linear_multi": (C.c_int, [C.c_int, u32, vp, vp, vp, sz, sz, sz, sz, vp, vp, f32, vp, C.c_int, vp, vp, vp, vp, C.POINTER(C.c_int), vp]),
        "lgh_op_linear_chain_multi": (C.c_int, [C.c_int, u32, vp, vp, vp, sz, sz, sz, sz, vp, vp, f32, vp, C.c_int, vp, u32, vp, sz, vp, vp, vp,
                                                C.POINTER(C.c_int)]),
        "lgh_op_qkv_rope_multi": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, f32, sz, sz, sz, sz, sz, sz, sz, vp, vp, f32, f32, C.c_int, vp, vp, vp, vp, vp]),
        "lgh_op_moe_multi": (C.c_int, [C.c_int, u32, vp, vp, u32, vp, sz, sz, sz, sz, sz, sz, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp,
                                       vp, vp, vp]),
        "lgh_debug_mvqb_structures": (None, [vp]),
        "lgh_op_pf_qkv": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, f32, sz, sz, sz, sz, C.c_int, sz, sz, sz, f32, f32, vp, vp, vp]),
        "lgh_op_pf_linear": (C.c_int, [C.c_int, u32, vp, vp, vp, sz, sz, vp, vp, sz, vp, vp, vp]),
        "lgh_op_pf_ffn": (C.c_int, [C.c_int, u32, vp, vp, u32, vp, vp, vp, vp, f32, sz, sz, sz, vp, vp, vp, vp]),
        "lgh_op_pf_moe": (C.c_int, [C.c_int, u32, vp, vp, u32, vp, vp, sz, sz, vp, vp, vp, f32, sz, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                    vp, vp]),
        "lgh_op_embed": (C.c_int, [C.c_int, C.c_int, u32, vp, sz, sz, vp, sz, vp, C.c_int, vp, vp, vp, vp, C.POINTER(C.c_int)]),
        "lgh_op_qkv_forward": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, f32, sz, sz, sz, sz, sz, sz, f32, f32, C.c_int, C.c_int, vp, vp, vp, vp,
                                         C.c_char_p, sz]),
        "lgh_op_ffn_gateup": (C.c_int, [C.c_int, u32, vp, u32, vp, vp, vp, f32, sz, sz, vp]),
        "lgh_op_argmax": (C.c_int, [C.c_int, vp, sz, sz, vp]),
        "lgh_kv_cache_layout": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(KvLayout)]),
        "lgh_prefix_save": (C.c_int, [vp, C.c_int, sz, C.POINTER(vp)]), "lgh_prefix_restore": (C.c_int, [vp, vp, C.c_int, sz]),
        "lgh_prefix_free": (C.c_int, [vp, vp]), "lgh_prefix_get_info": (C.c_int, [vp, vp, C.POINTER(PrefixInfo)]),
        "lgh_prefix_total_bytes": (C.c_uint64, [vp]), "lgh_prefix_export": (C.c_int, [vp, vp, vp, sz, C.POINTER(sz)]),
        "lgh_prefix_import": (C.c_int, [vp, vp, sz, C.POINTER(vp)]),
        "lgh_op_kv_prefix_copy": (C.c_int, [C.c_int, u32, u32, u32, u32, u32, u32, C.POINTER(vp), u32, u32, vp, C.c_int]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def device_count() -> int:
    return load_library().lgh_device_count()


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _chk(status: int, what: str = "") -> None:
    if status != 0:
        raise BackendError(status, what)


class HipGpuInference:
    """`impl GpuInference for HipGpuInference` (src/backend/mod.rs:283-296), one context per GPU."""

    def __init__(self):
        self._h = C.c_void_p()
        self.config = None
        self.vocab_size = 0

    # -- pub fn from_model(model: LlamaModel, max_seq_len: usize) -> BackendResult<Self>  (gpu_only.rs:426)
    @classmethod
    def from_model(cls, model, max_seq_len: int, device: int = 0, layer_range: Optional[Sequence[int]] = None,
                   flags: int = 0, attn_splits: int = 0, attn_direct: int = 0, kv_cache_type: int = 0,
                   kv_rotation_signs=None, kv_qjl_matrices=None, prefill_policy: int = 0) -> "HipGpuInference":
        """`model` hands over what LlamaModel::into_parts does (llama.rs:138-160): `.config` and
        `.tensors(layers)` yielding (gguf_name, ggml_type, ne, host bytes)."""
        L = load_library()
        self = cls()
        cfg = model.config
        d = ModelDesc()
        d.struct_size = C.sizeof(ModelDesc)
        for k in ("hidden_size", "intermediate_size", "num_layers", "num_heads", "num_kv_heads", "head_dim",
                  "vocab_size", "num_experts", "num_experts_per_token", "expert_intermediate_size"):
            setattr(d, k, int(getattr(cfg, k)))
        d.max_seq_len = int(max_seq_len)
        d.use_neox_rope = int(cfg.use_neox_rope)
        d.norm_eps, d.rope_freq_base, d.rope_freq_scale = cfg.norm_eps, cfg.rope_freq_base, cfg.rope_freq_scale
        d.device_id = device
        lb, le = (0, cfg.num_layers) if layer_range is None else (layer_range[0], layer_range[1])
        d.layer_begin, d.layer_end = lb, le
        # attn_direct: 64-row units, 0 = tuned default, 255 = never
        d.flags = flags | ((attn_splits & 0xFF) << 8) | ((attn_direct & 0xFF) << 16)
        d.kv_cache_type = int(kv_cache_type)
        _chk(L.lgh_create(C.byref(d), C.byref(self._h)), "lgh_create (is a HIP device visible?)")
        self.config, self.vocab_size, self.hidden_size = cfg, cfg.vocab_size, cfg.hidden_size
        try:
            if kv_rotation_signs is not None:      # TurboQuant: HadamardRotation::signs() of every (layer, kv head, k / v) engine
                sg = np.ascontiguousarray(kv_rotation_signs, dtype=np.float32)
                self._call(L.lgh_set_kv_rotation_signs(self._h, sg.ctypes.data, sg.size))
            if kv_qjl_matrices is not None:        # TurboQuantProd: the K engines' QjlProjector matrices [layer][kv head][d][d]
                qm = np.ascontiguousarray(kv_qjl_matrices, dtype=np.float32)
                self._call(L.lgh_set_kv_qjl_matrices(self._h, qm.ctypes.data, qm.size))
            for name, t, ne, data in model.tensors(range(lb, le)):
                self.upload_tensor(name, t, ne, data)
            self._call(L.lgh_finalize(self._h))
            if prefill_policy:
                self.set_prefill_policy(prefill_policy)
        except Exception:
            self.close()
            raise
        return self

    @classmethod
    def from_gguf(cls, path: str, max_seq_len: int = 0, device: int = 0, layer_range: Optional[Sequence[int]] = None,
                  flags: int = 0) -> "HipGpuInference":
        """GGUF -> HBM direct load (lgh_load_gguf): header parsed and tensors uploaded by the library itself."""
        L = load_library()
        info = gguf_inspect(path)
        self = cls()
        err = C.create_string_buffer(512)
        lb, le = (0, 0) if layer_range is None else (layer_range[0], layer_range[1])
        rc = L.lgh_load_gguf(path.encode(), int(max_seq_len), device, flags, lb, le, C.byref(self._h), err, len(err))
        if rc:
            raise BackendError(rc, "lgh_load_gguf: " + err.value.decode(errors="replace"))
        d = info["desc"]
        self.vocab_size, self.hidden_size = d["vocab_size"], d["hidden_size"]
        self.config = None
        return self

    def upload_tensor(self, name: str, ggml_type: int, ne: Iterable[int], data: np.ndarray) -> None:
        data = np.ascontiguousarray(data)
        ne = list(ne)
        ne4 = (C.c_uint64 * 4)(*(ne + [0] * (4 - len(ne))))
        self._call(load_library().lgh_upload_tensor(self._h, name.encode(), ggml_type, ne4, data.ctypes.data, data.nbytes))

    def _call(self, status: int) -> None:
        if status != 0:
            raise BackendError(status, load_library().lgh_last_error(self._h).decode())

    # -- GpuInference
    def forward(self, token_id: int) -> np.ndarray:
        logits = np.empty(self.vocab_size, dtype=np.float32)
        self._call(load_library().lgh_forward(self._h, token_id, logits.ctypes.data))
        return logits

    def prefill_token(self, token_id: int) -> None:
        self._call(load_library().lgh_prefill_token(self._h, token_id))

    def forward_batch(self, tokens: Sequence[int]) -> None:  # gpu_only.rs:776-790 minus the final forward
        toks = np.ascontiguousarray(tokens, dtype=np.uint32)
        self._call(load_library().lgh_prefill_batch(self._h, toks.ctypes.data, toks.size))

    def prefill_is_batched(self) -> bool:
        return bool(load_library().lgh_prefill_is_batched(self._h))

    def set_prefill_policy(self, policy: int) -> None:
        """lgh_set_prefill_policy: PREFILL_BATCH_BYTE_KV lets int8 / FP8 caches take the batched prompt pass; 0 restores the default."""
        self._call(load_library().lgh_set_prefill_policy(self._h, policy))

    def reset(self) -> None:
        load_library().lgh_reset(self._h)

    def position(self) -> int:
        return load_library().lgh_position(self._h)

    def kv_truncate(self, new_len: int) -> None:       # KVCache::truncate (model/mod.rs:130-134)
        self._call(load_library().lgh_kv_truncate(self._h, new_len))

    def kv_shift_left(self, amount: int) -> None:      # KVCache::shift_left (model/mod.rs:142-172) on the device cache
        self._call(load_library().lgh_kv_shift_left(self._h, amount))

    # -- bench fast paths
    def forward_argmax(self, token_id: int) -> int:
        nxt = C.c_uint32()
        self._call(load_library().lgh_forward_argmax(self._h, token_id, C.byref(nxt)))
        return nxt.value

    def decode_greedy(self, first_token: int, n_steps: int) -> np.ndarray:
        out = np.zeros(n_steps, dtype=np.uint32)
        self._call(load_library().lgh_decode_greedy(self._h, first_token, n_steps, out.ctypes.data))
        return out

    # -- multi-sequence decode: the device side of BatchedEngine (src/engine_batched.rs; include/llama_gguf_hip.h lgh_batch_*)
    def batch_create(self, max_batch: int) -> None:
        """`max_batch` slots (BatchedEngineConfig::max_batch_size), each one sequence's KV caches + position."""
        self._call(load_library().lgh_batch_create(self._h, max_batch))

    def batch_reset(self, slot: int) -> None:          # create_active_sequence: a fresh context for the slot
        self._call(load_library().lgh_batch_reset(self._h, slot))

    def batch_position(self, slot: int) -> int:
        return load_library().lgh_batch_position(self._h, slot)

    def batch_prefill(self, slot: int, tokens: Sequence[int]) -> None:
        toks = np.ascontiguousarray(tokens, dtype=np.uint32)
        self._call(load_library().lgh_batch_prefill(self._h, slot, toks.ctypes.data, toks.size))

    def forward_multi(self, slots: Sequence[int], tokens: Sequence[int], want_logits: bool = True, greedy: bool = False):
        """One iteration of the batched loop (engine_batched.rs:236-290): tokens[i] to slot slots[i], every weight read once.
        Returns (logits [n_seq, vocab] or None, next tokens [n_seq] or None)."""
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        tk = np.ascontiguousarray(tokens, dtype=np.uint32)
        assert sl.size == tk.size
        logits = np.empty((sl.size, self.vocab_size), dtype=np.float32) if want_logits else None
        nxt = np.zeros(sl.size, dtype=np.uint32) if greedy else None
        self._call(load_library().lgh_forward_multi(self._h, sl.ctypes.data, tk.ctypes.data, sl.size,
                                                    logits.ctypes.data if logits is not None else None,
                                                    nxt.ctypes.data if nxt is not None else None))
        return logits, nxt

    def decode_greedy_multi(self, slots: Sequence[int], first_tokens: Sequence[int], n_steps: int) -> np.ndarray:
        """n_steps greedy iterations, tokens fed back on the device; returns [n_steps, n_seq]."""
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        tk = np.ascontiguousarray(first_tokens, dtype=np.uint32)
        out = np.zeros((n_steps, sl.size), dtype=np.uint32)
        self._call(load_library().lgh_decode_greedy_multi(self._h, sl.ctypes.data, tk.ctypes.data, sl.size, n_steps, out.ctypes.data))
        return out

    # -- sampling on the device (Sampler::sample, src/sampling/mod.rs:188-304; include/llama_gguf_hip.h lgh_set_sampler)
    def set_sampler(self, **cfg) -> None:
        """Sampler::new: the config (keyword arguments of `sampler_config`, or of `sampler_config_ex` when min_p / mirostat / tau /
        eta is among them), zeroed counts and mu = 2 * tau."""
        if _is_ex(cfg):
            self._call(load_library().lgh_set_sampler_ex(self._h, C.byref(sampler_config_ex(**cfg))))
        else:
            self._call(load_library().lgh_set_sampler(self._h, C.byref(sampler_config(**cfg))))

    def sampler_mu(self, slot: int = -1) -> float:
        """Sampler::mirostat_mu of the context's sampler (slot -1) or of a batch slot."""
        mu = C.c_float()
        self._call(load_library().lgh_get_sampler_mu(self._h, slot, C.byref(mu)))
        return mu.value

    def decode_sample(self, first_token: int, history: Sequence[int], n_steps: int, uniforms=None) -> np.ndarray:
        """n_steps sampled tokens fed back on the device; history = the context's tokens before first_token, uniforms[n_steps] =
        the reference's rng.gen::<f32>() draws (None under a greedy config)."""
        h = np.ascontiguousarray(history, dtype=np.uint32)
        u = _f32(uniforms) if uniforms is not None else None
        if u is not None:
            assert u.size >= n_steps
        out = np.zeros(n_steps, dtype=np.uint32)
        self._call(load_library().lgh_decode_sample(self._h, first_token, h.ctypes.data if h.size else None, h.size, n_steps,
                                                    u.ctypes.data if u is not None else None, out.ctypes.data))
        return out

    def batch_set_sampler(self, slot: int, **cfg) -> None:
        if _is_ex(cfg):
            self._call(load_library().lgh_batch_set_sampler_ex(self._h, slot, C.byref(sampler_config_ex(**cfg))))
        else:
            self._call(load_library().lgh_batch_set_sampler(self._h, slot, C.byref(sampler_config(**cfg))))

    def decode_sample_multi(self, slots: Sequence[int], first_tokens: Sequence[int], histories: Sequence[Sequence[int]], n_steps: int,
                            uniforms=None) -> np.ndarray:
        """decode_greedy_multi with each slot's sampler; uniforms [n_steps, n_seq]; returns [n_steps, n_seq]."""
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        tk = np.ascontiguousarray(first_tokens, dtype=np.uint32)
        assert sl.size == tk.size == len(histories)
        lens = np.array([len(h) for h in histories], dtype=np.uint64)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.uint32) for h in histories]) if lens.sum() else
                                    np.zeros(0, dtype=np.uint32), dtype=np.uint32)
        u = _f32(uniforms).reshape(-1) if uniforms is not None else None
        if u is not None:
            assert u.size >= n_steps * sl.size
        out = np.zeros((n_steps, sl.size), dtype=np.uint32)
        self._call(load_library().lgh_decode_sample_multi(self._h, sl.ctypes.data, tk.ctypes.data, sl.size,
                                                          flat.ctypes.data if flat.size else None, lens.ctypes.data, n_steps,
                                                          u.ctypes.data if u is not None else None, out.ctypes.data))
        return out

    # -- device prompt cache (PrefixSharing::save_prefix / try_restore, src/model/cache.rs:269-326; include/llama_gguf_hip.h lgh_prefix_*)
    def prefix_save(self, n: Optional[int] = None, slot: int = -1) -> "KvPrefix":
        """Rows [0, n) (None: up to the position) of the own sequence (slot -1) or of a batch slot, copied into a new device prefix."""
        h = C.c_void_p()
        self._call(load_library().lgh_prefix_save(self._h, slot, 0 if n is None else n, C.byref(h)))
        return KvPrefix(self, h)

    def prefix_restore(self, prefix: "KvPrefix", slot: int = -1, n: Optional[int] = None) -> None:
        """The target reset, then a prompt of n tokens (None: the whole prefix) by copying; the position follows."""
        self._call(load_library().lgh_prefix_restore(self._h, prefix._h, slot, 0 if n is None else n))

    def prefix_from_bytes(self, blob) -> "KvPrefix":
        """KvPrefix.to_bytes() back into a device prefix of this context (every header field is checked against it)."""
        b = np.frombuffer(bytes(blob), dtype=np.uint8)
        h = C.c_void_p()
        self._call(load_library().lgh_prefix_import(self._h, b.ctypes.data if b.size else None, b.size, C.byref(h)))
        return KvPrefix(self, h)

    def prefix_total_bytes(self) -> int:
        """Device bytes of this context's live prefixes (not part of stats())."""
        return int(load_library().lgh_prefix_total_bytes(self._h))

    # -- pipeline stage
    def stage_hidden_ptr(self) -> int:
        p = C.c_void_p()
        self._call(load_library().lgh_stage_hidden_buffer(self._h, C.byref(p)))
        return p.value

    def stage_hidden_block_ptr(self) -> int:
        """Device address of the [128][hidden] f32 block the batched prompt path hands from stage to stage."""
        p = C.c_void_p()
        self._call(load_library().lgh_stage_hidden_block_buffer(self._h, C.byref(p)))
        return p.value

    def stage_prefill_batch(self, tokens: Optional[Sequence[int]], n: int) -> None:
        """Up to 128 prompt tokens through this stage's layers on the batched path (`tokens` is read on the first stage)."""
        toks = np.ascontiguousarray(tokens, dtype=np.uint32) if tokens is not None else None
        self._call(load_library().lgh_stage_prefill_batch(self._h, toks.ctypes.data if toks is not None else None, n))

    def stage_forward(self, token_id: int = 0, want_logits: bool = False, argmax: bool = False):
        logits = np.empty(self.vocab_size, dtype=np.float32) if (want_logits and not argmax) else None
        nxt = C.c_uint32()
        self._call(load_library().lgh_stage_forward(
            self._h, token_id, int(want_logits), logits.ctypes.data if logits is not None else None,
            C.byref(nxt) if (want_logits and argmax) else None))
        return nxt.value if (want_logits and argmax) else logits

    def stage_io_ptrs(self):
        """(token_in, argmax_out): device addresses of the int32 words the first stage embeds from / the last stage's
        arg-max lands in — the token is fed back between them without the host."""
        a, b = C.c_void_p(), C.c_void_p()
        self._call(load_library().lgh_stage_io_buffers(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def stage_step(self, mode: int = 0) -> None:
        """One token through this stage with no host value in or out (0 layers only, 1 + logits, 2 + device arg-max)."""
        self._call(load_library().lgh_stage_step(self._h, mode))

    def stage_read_tokens(self, pos0: int, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=np.uint32)
        self._call(load_library().lgh_stage_read_tokens(self._h, pos0, n, out.ctypes.data))
        return out

    def set_stream(self, stream_handle: int) -> None:
        self._call(load_library().lgh_set_stream(self._h, stream_handle))

    def synchronize(self) -> None:
        self._call(load_library().lgh_synchronize(self._h))

    def read_hidden(self) -> np.ndarray:
        out = np.empty(self.hidden_size, dtype=np.float32)
        self._call(load_library().lgh_read_hidden(self._h, out.ctypes.data))
        return out

    def set_profiling(self, on: bool) -> None:
        self._call(load_library().lgh_set_profiling(self._h, int(on)))

    def stats(self) -> dict:
        s = Stats()
        self._call(load_library().lgh_get_stats(self._h, C.byref(s)))
        out = {k: getattr(s, k) for k in ("weight_bytes", "kv_bytes", "scratch_bytes", "tokens_processed",
                                          "graph_nodes", "step_alg_bytes", "event_bracket_us", "overlapped_edges")}
        out["kernels"] = {K_NAMES[i]: {"launches": s.k_launches[i], "time_us": s.k_time_us[i],
                                       "alg_bytes": s.k_alg_bytes[i]}
                          for i in range(len(K_NAMES)) if s.k_launches[i]}
        out["symbols"] = {SYM_NAMES[i]: {"launches": s.sym_launches[i], "time_us": s.sym_time_us[i],
                                         "alg_bytes": s.sym_alg_bytes[i]}
                          for i in range(len(SYM_NAMES)) if s.sym_launches[i]}
        return out

    def close(self) -> None:
        if self._h:
            load_library().lgh_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KvPrefix:
    """A saved KV prefix on the device (lgh_prefix; CachedPrefix's k_cache / v_cache, src/model/cache.rs:28-43).  Owned by the engine
    that made it: `free()` releases the device memory, closing the engine releases what is left."""

    def __init__(self, engine: HipGpuInference, handle: C.c_void_p):
        self._engine, self._h = engine, handle
        info = self.info()
        self.n_rows, self.nbytes = int(info.n_rows), int(info.bytes)

    def info(self) -> PrefixInfo:
        out = PrefixInfo()
        self._engine._call(load_library().lgh_prefix_get_info(self._engine._h, self._h, C.byref(out)))
        return out

    def free(self) -> None:
        self._engine._call(load_library().lgh_prefix_free(self._engine._h, self._h))

    def to_bytes(self) -> bytes:
        """The exported blob (header + packed rows), for a session file or HipGpuInference.prefix_from_bytes."""
        need = C.c_size_t(0)
        L = load_library()
        self._engine._call(L.lgh_prefix_export(self._engine._h, self._h, None, 0, C.byref(need)))
        buf = np.empty(need.value, dtype=np.uint8)
        self._engine._call(L.lgh_prefix_export(self._engine._h, self._h, buf.ctypes.data, buf.nbytes, C.byref(need)))
        return buf.tobytes()


# ---- PromptCache / PrefixSharing (src/model/cache.rs:67-345) over device prefixes.  The reference's entries clone the K / V tensors
# of every layer; here an entry holds the handle `engine.prefix_save()` returned — anything with `.nbytes` and `.free()` — and the
# copy is the engine's `prefix_restore`.  Restated as written, quirks included; nothing here touches a GPU by itself. ----
class PromptCacheConfig:
    """PromptCacheConfig and its Default (cache.rs:67-89)."""

    def __init__(self, max_entries: int = 100, max_memory: int = 1024 * 1024 * 1024, min_prefix_len: int = 32,
                 cache_system_prompts: bool = True):
        self.max_entries, self.max_memory, self.min_prefix_len = max_entries, max_memory, min_prefix_len
        self.cache_system_prompts = cache_system_prompts


class PromptCacheStats:
    """PromptCacheStats (cache.rs:238-247)."""

    def __init__(self, num_entries: int, memory_used: int, total_tokens_cached: int):
        self.num_entries, self.memory_used, self.total_tokens_cached = num_entries, memory_used, total_tokens_cached

    def __repr__(self):
        return f"PromptCacheStats(num_entries={self.num_entries}, memory_used={self.memory_used}, total_tokens_cached={self.total_tokens_cached})"


def prefix_id(tokens: Sequence[int]) -> int:
    """PrefixId::from_tokens (cache.rs:18-25): a 64-bit hash of the tokens.  Rust's DefaultHasher is unspecified, so its values are
    not reproduced: FNV-1a over the length and the little-endian u32 tokens."""
    h = 0xCBF29CE484222325
    for b in len(tokens).to_bytes(8, "little") + b"".join(int(t).to_bytes(4, "little") for t in tokens):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


class CachedPrefix:
    """CachedPrefix (cache.rs:28-65): the tokens and the device handle of their KV rows."""

    def __init__(self, tokens: Sequence[int], handle, stamp: int):
        self.tokens = [int(t) for t in tokens]
        self.handle = handle
        self.seq_len = len(self.tokens)
        self.ref_count = 0
        self.last_access = stamp      # a counter, not a clock: later accesses have larger stamps

    def memory_size(self) -> int:     # cache.rs:60-64: K bytes + V bytes + 4 per token
        return int(self.handle.nbytes) + 4 * len(self.tokens)


class PromptCache:
    """PromptCache (cache.rs:91-236)."""

    def __init__(self, config: Optional[PromptCacheConfig] = None):
        self.config = config or PromptCacheConfig()
        self.entries = {}
        self.memory_used = 0
        self._clock = 0

    def _now(self) -> int:
        self._clock += 1
        return self._clock

    def cache_prefix(self, tokens: Sequence[int], handle) -> int:
        """cache.rs:112-150.  A known id bumps ref_count and refreshes the stamp; a prompt below min_prefix_len is not stored; in
        both cases the caller's new handle is freed (the reference drops the tensors it was given).  Eviction stops when no
        entry has ref_count 0, and the new entry is inserted anyway."""
        pid = prefix_id(tokens)
        entry = self.entries.get(pid)
        if entry is not None:
            entry.ref_count += 1
            entry.last_access = self._now()
            if handle is not None and handle is not entry.handle:
                handle.free()
            return pid
        if len(tokens) < self.config.min_prefix_len:
            if handle is not None:
                handle.free()
            return pid
        prefix = CachedPrefix(tokens, handle, self._now())
        size = prefix.memory_size()
        while self.memory_used + size > self.config.max_memory or len(self.entries) >= self.config.max_entries:
            if not self._evict_lru():
                break
        self.memory_used += size
        self.entries[pid] = prefix
        return pid

    def get_prefix(self, pid: int) -> Optional[CachedPrefix]:          # cache.rs:153-161
        entry = self.entries.get(pid)
        if entry is not None:
            entry.ref_count += 1
            entry.last_access = self._now()
        return entry

    def find_matching_prefix(self, tokens: Sequence[int]):             # cache.rs:164-188 -> (id, length) or None
        toks = [int(t) for t in tokens]
        best = None
        for pid, entry in self.entries.items():
            n = len(entry.tokens)
            if len(toks) >= n and toks[:n] == entry.tokens and (best is None or n > best[1]):
                best = (pid, n)
        if best is not None:
            entry = self.entries[best[0]]
            entry.last_access = self._now()
            entry.ref_count += 1
        return best

    def remove_prefix(self, pid: int) -> None:                          # cache.rs:191-195; the device memory is freed
        entry = self.entries.pop(pid, None)
        if entry is not None:
            self.memory_used = max(0, self.memory_used - entry.memory_size())
            entry.handle.free()

    def clear(self) -> None:                                            # cache.rs:198-201
        for entry in self.entries.values():
            entry.handle.free()
        self.entries.clear()
        self.memory_used = 0

    def stats(self) -> PromptCacheStats:                                # cache.rs:204-210
        return PromptCacheStats(len(self.entries), self.memory_used, sum(e.seq_len for e in self.entries.values()))

    def _evict_lru(self) -> bool:                                       # cache.rs:213-228
        idle = [(e.last_access, pid) for pid, e in self.entries.items() if e.ref_count == 0]
        if not idle:
            return False
        self.remove_prefix(min(idle)[1])
        return True

    def release_prefix(self, pid: int) -> None:                         # cache.rs:231-235
        entry = self.entries.get(pid)
        if entry is not None:
            entry.ref_count = max(0, entry.ref_count - 1)


class PrefixSharing:
    """PrefixSharing (cache.rs:250-345) over any engine object with `prefix_save(n, slot)` / `prefix_restore(prefix, slot, n)`."""

    def __init__(self, config: Optional[PromptCacheConfig] = None):
        self.cache = PromptCache(config)
        self.active_prefix = None

    def try_restore(self, tokens: Sequence[int], engine, slot: int = -1) -> int:
        """cache.rs:269-310: the longest cached prefix of `tokens` copied into the engine's sequence; returns the tokens restored
        (0: no match).  find_matching_prefix and get_prefix each bump ref_count, so a restore bumps it twice."""
        m = self.cache.find_matching_prefix(tokens)
        if m is None:
            return 0
        pid, match_len = m
        prefix = self.cache.get_prefix(pid)
        if prefix is None:
            return 0
        engine.prefix_restore(prefix.handle, slot, match_len)
        self.active_prefix = pid
        return match_len

    def save_prefix(self, tokens: Sequence[int], engine, slot: int = -1) -> int:
        """cache.rs:313-326: the first len(tokens) rows of the engine's sequence cached under the tokens' id."""
        pid = self.cache.cache_prefix(tokens, engine.prefix_save(len(tokens), slot))
        self.active_prefix = pid
        return pid

    def release_active(self) -> None:                                   # cache.rs:329-333: drops ref_count once
        if self.active_prefix is not None:
            self.cache.release_prefix(self.active_prefix)
            self.active_prefix = None

    def stats(self) -> PromptCacheStats:
        return self.cache.stats()

    def clear(self) -> None:                                            # cache.rs:341-344
        self.active_prefix = None
        self.cache.clear()


class HipPipeline:
    """The in-library layer pipeline behind the GpuInference surface (lgh_pipeline_*): one process, `n_stages` stage contexts
    on `devices` (default: all on device 0), hidden vector and greedy token hopped device to device.  `GpuModelWrapper`
    drives it like a single HipGpuInference."""

    def __init__(self):
        self._h = C.c_void_p()
        self.config = None
        self.vocab_size = 0

    @classmethod
    def from_model(cls, model, max_seq_len: int, n_stages: int, devices: Optional[Sequence[int]] = None, flags: int = 0,
                   attn_direct: int = 0) -> "HipPipeline":
        """`attn_direct` as in HipGpuInference.from_model (64-row units, 0 = tuned default, 255 = never), for every stage; the same
        selector is bits 16..23 of `flags`: give one of the two."""
        if attn_direct and flags & (0xFF << 16):
            raise ValueError("attn_direct and bits 16..23 of flags are the same selector: give one")
        L = load_library()
        self = cls()
        cfg = model.config
        d = ModelDesc()
        d.struct_size = C.sizeof(ModelDesc)
        for k in ("hidden_size", "intermediate_size", "num_layers", "num_heads", "num_kv_heads", "head_dim",
                  "vocab_size", "num_experts", "num_experts_per_token", "expert_intermediate_size"):
            setattr(d, k, int(getattr(cfg, k)))
        d.max_seq_len = int(max_seq_len)
        d.use_neox_rope = int(cfg.use_neox_rope)
        d.norm_eps, d.rope_freq_base, d.rope_freq_scale = cfg.norm_eps, cfg.rope_freq_base, cfg.rope_freq_scale
        d.device_id, d.flags = 0, flags | ((attn_direct & 0xFF) << 16)
        devs = (C.c_int * n_stages)(*devices) if devices is not None else None
        _chk(L.lgh_pipeline_create(C.byref(d), devs, n_stages, C.byref(self._h)), "lgh_pipeline_create (is a HIP device visible?)")
        self.config, self.vocab_size, self.hidden_size = cfg, cfg.vocab_size, cfg.hidden_size
        try:
            for name, t, ne, data in model.tensors():
                data = np.ascontiguousarray(data)
                ne = list(ne)
                ne4 = (C.c_uint64 * 4)(*(ne + [0] * (4 - len(ne))))
                self._call(L.lgh_pipeline_upload_tensor(self._h, name.encode(), t, ne4, data.ctypes.data, data.nbytes))
            self._call(L.lgh_pipeline_finalize(self._h))
        except Exception:
            self.close()
            raise
        return self

    def _call(self, status: int) -> None:
        if status != 0:
            raise BackendError(status, load_library().lgh_pipeline_last_error(self._h).decode())

    def forward(self, token_id: int) -> np.ndarray:
        logits = np.empty(self.vocab_size, dtype=np.float32)
        self._call(load_library().lgh_pipeline_forward(self._h, token_id, logits.ctypes.data))
        return logits

    def prefill_token(self, token_id: int) -> None:
        self._call(load_library().lgh_pipeline_prefill_token(self._h, token_id))

    def decode_greedy(self, first_token: int, n_steps: int) -> np.ndarray:
        out = np.zeros(n_steps, dtype=np.uint32)
        self._call(load_library().lgh_pipeline_decode_greedy(self._h, first_token, n_steps, out.ctypes.data))
        return out

    def reset(self) -> None:
        load_library().lgh_pipeline_reset(self._h)

    def position(self) -> int:
        return load_library().lgh_pipeline_position(self._h)

    def kv_truncate(self, new_len: int) -> None:
        self._call(load_library().lgh_pipeline_kv_truncate(self._h, int(new_len)))

    def stages(self) -> int:
        return load_library().lgh_pipeline_stages(self._h)

    def close(self) -> None:
        if self._h:
            load_library().lgh_pipeline_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipTensorParallel:
    """Tensor-parallel decode behind the GpuInference surface (lgh_tp_*): one process, `n_ranks` rank contexts on `devices`
    (default: all on device 0 — the single-device rehearsal), every rank holding 1/N of the heads and of the FFN.
    `GpuModelWrapper` drives it like a single HipGpuInference."""

    def __init__(self):
        self._h = C.c_void_p()
        self.config = None
        self.vocab_size = 0

    @classmethod
    def from_model(cls, model, max_seq_len: int, n_ranks: int, devices: Optional[Sequence[int]] = None, flags: int = 0,
                   kv_cache_type: int = 0, layer_range: Optional[Sequence[int]] = None, attn_direct: int = 0) -> "HipTensorParallel":
        """`kv_cache_type` / `layer_range` exist to be refused: tensor parallelism runs whole models over the f32 cache.
        `attn_direct` as in HipGpuInference.from_model (64-row units, 0 = tuned default, 255 = never), for every rank; the same selector
        is bits 16..23 of `flags`: give one of the two."""
        if attn_direct and flags & (0xFF << 16):
            raise ValueError("attn_direct and bits 16..23 of flags are the same selector: give one")
        L = load_library()
        self = cls()
        cfg = model.config
        d = ModelDesc()
        d.struct_size = C.sizeof(ModelDesc)
        for k in ("hidden_size", "intermediate_size", "num_layers", "num_heads", "num_kv_heads", "head_dim",
                  "vocab_size", "num_experts", "num_experts_per_token", "expert_intermediate_size"):
            setattr(d, k, int(getattr(cfg, k)))
        d.max_seq_len = int(max_seq_len)
        d.use_neox_rope = int(cfg.use_neox_rope)
        d.norm_eps, d.rope_freq_base, d.rope_freq_scale = cfg.norm_eps, cfg.rope_freq_base, cfg.rope_freq_scale
        d.device_id, d.flags, d.kv_cache_type = 0, flags | ((attn_direct & 0xFF) << 16), int(kv_cache_type)
        if layer_range is not None:
            d.layer_begin, d.layer_end = layer_range
        if devices is not None and len(devices) != n_ranks:
            raise ValueError("one device per rank")
        devs = (C.c_int * n_ranks)(*devices) if devices is not None else None
        status = L.lgh_tp_create(C.byref(d), devs, n_ranks, C.byref(self._h))
        if status != 0:
            raise BackendError(status, (L.lgh_tp_last_error(None) or b"").decode() or "lgh_tp_create (is a HIP device visible?)")
        self.config, self.vocab_size, self.hidden_size = cfg, cfg.vocab_size, cfg.hidden_size
        try:
            for name, t, ne, data in model.tensors():
                data = np.ascontiguousarray(data)
                ne = list(ne)
                ne4 = (C.c_uint64 * 4)(*(ne + [0] * (4 - len(ne))))
                self._call(L.lgh_tp_upload_tensor(self._h, name.encode(), t, ne4, data.ctypes.data, data.nbytes))
            self._call(L.lgh_tp_finalize(self._h))
        except Exception:
            self.close()
            raise
        return self

    def _call(self, status: int) -> None:
        if status != 0:
            raise BackendError(status, load_library().lgh_tp_last_error(self._h).decode())

    def forward(self, token_id: int) -> np.ndarray:
        logits = np.empty(self.vocab_size, dtype=np.float32)
        self._call(load_library().lgh_tp_forward(self._h, token_id, logits.ctypes.data))
        return logits

    def prefill_token(self, token_id: int) -> None:
        self._call(load_library().lgh_tp_prefill_token(self._h, token_id))

    def forward_batch(self, tokens: Sequence[int]) -> None:  # gpu_only.rs:776-790 minus the final forward, over the ranks
        toks = np.ascontiguousarray(tokens, dtype=np.uint32)
        self._call(load_library().lgh_tp_prefill_batch(self._h, toks.ctypes.data, toks.size))

    def prefill_is_batched(self) -> bool:
        return bool(load_library().lgh_tp_prefill_is_batched(self._h))

    def stats(self, rank: int = 0) -> dict:
        """weight / KV / scratch bytes and tokens processed of one rank's context"""
        s = Stats()
        self._call(load_library().lgh_tp_get_stats(self._h, int(rank), C.byref(s)))
        return {k: getattr(s, k) for k in ("weight_bytes", "kv_bytes", "scratch_bytes", "tokens_processed")}

    def decode_greedy(self, first_token: int, n_steps: int) -> np.ndarray:
        out = np.zeros(n_steps, dtype=np.uint32)
        self._call(load_library().lgh_tp_decode_greedy(self._h, first_token, n_steps, out.ctypes.data))
        return out

    def reset(self) -> None:
        load_library().lgh_tp_reset(self._h)

    def position(self) -> int:
        return load_library().lgh_tp_position(self._h)

    def kv_truncate(self, new_len: int) -> None:
        self._call(load_library().lgh_tp_kv_truncate(self._h, int(new_len)))

    def ranks(self) -> int:
        return load_library().lgh_tp_ranks(self._h)

    def graph_nodes(self) -> int:
        return int(load_library().lgh_tp_graph_nodes(self._h))

    def close(self) -> None:
        if self._h:
            load_library().lgh_tp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class InferenceContext:
    """The fields of the reference's InferenceContext that GpuModelWrapper touches (model/mod.rs:222-326)."""

    def __init__(self):
        self.position = 0
        self.kv_seq_len = 0

    def reset(self) -> None:
        self.position = 0
        self.kv_seq_len = 0


class GpuModelWrapper:
    """GpuModelWrapper<T: GpuInference> (src/backend/mod.rs:302-364): adapts the engine to `Model::forward`."""

    def __init__(self, gpu: HipGpuInference, config=None):
        self.gpu = gpu
        self.config = config if config is not None else gpu.config

    def forward(self, tokens: Sequence[int], ctx: InferenceContext) -> np.ndarray:
        if ctx.position == 0 and self.gpu.position() > 0:  # mod.rs:334-336
            self.gpu.reset()
        if len(tokens) == 0:
            raise ValueError("No tokens to process")           # mod.rs:338-342
        for t in tokens[:-1]:                                   # mod.rs:344-347
            self.gpu.prefill_token(int(t))
        logits = self.gpu.forward(int(tokens[-1]))              # mod.rs:349
        ctx.position += len(tokens)
        ctx.kv_seq_len = ctx.position
        return logits


# ---- per-op surface (the `Backend` trait ops on the path, src/backend/mod.rs:29-265) ----
def op_dequantize(ggml_type: int, raw: np.ndarray, n_elems: int, device: int = 0) -> np.ndarray:
    raw = np.ascontiguousarray(raw)
    out = np.empty(n_elems, dtype=np.float32)
    _chk(load_library().lgh_op_dequantize(device, ggml_type, raw.ctypes.data, n_elems, out.ctypes.data), "dequantize")
    return out


def op_vec_mat(ggml_type: int, w: np.ndarray, x, n: int, device: int = 0) -> np.ndarray:
    w, x = np.ascontiguousarray(w), _f32(x)
    out = np.empty(n, dtype=np.float32)
    _chk(load_library().lgh_op_vec_mat(device, ggml_type, w.ctypes.data, x.ctypes.data, out.ctypes.data, x.size, n), "vec_mat")
    return out


def op_mat_mat(ggml_type: int, w: np.ndarray, x, n: int, device: int = 0) -> np.ndarray:
    """x [m][k] . W^T -> [m][n] on the batched-prefill GEMM path (f16 matrix cores, f32 accumulation)."""
    w, x = np.ascontiguousarray(w), _f32(x)
    m, k = x.shape
    out = np.empty((m, n), dtype=np.float32)
    _chk(load_library().lgh_op_mat_mat(device, ggml_type, w.ctypes.data, x.ctypes.data, out.ctypes.data, k, n, m), "mat_mat")
    return out


def op_norm_vec_mat(ggml_type: int, w: np.ndarray, x, norm_w, eps: float, n: int, device: int = 0) -> np.ndarray:
    w, x, nw = np.ascontiguousarray(w), _f32(x), _f32(norm_w)
    out = np.empty(n, dtype=np.float32)
    _chk(load_library().lgh_op_norm_vec_mat(device, ggml_type, w.ctypes.data, x.ctypes.data, nw.ctypes.data, eps,
                                            out.ctypes.data, x.size, n), "norm_vec_mat")
    return out


def op_swiglu_vec_mat(ggml_type: int, w_gate: np.ndarray, w_up: np.ndarray, x, norm_w, eps: float, n: int,
                      device: int = 0) -> np.ndarray:
    wg, wu, x = np.ascontiguousarray(w_gate), np.ascontiguousarray(w_up), _f32(x)
    nw = _f32(norm_w) if norm_w is not None else None
    out = np.empty(n, dtype=np.float32)
    _chk(load_library().lgh_op_swiglu_vec_mat(device, ggml_type, wg.ctypes.data, wu.ctypes.data, x.ctypes.data,
                                              nw.ctypes.data if nw is not None else None, eps, out.ctypes.data,
                                              x.size, n), "swiglu_vec_mat")
    return out


def op_rms_norm(x, w, eps: float, device: int = 0) -> np.ndarray:
    x, w = _f32(x), _f32(w)
    out = np.empty_like(x)
    _chk(load_library().lgh_op_rms_norm(device, x.ctypes.data, w.ctypes.data, eps, out.ctypes.data, x.size), "rms_norm")
    return out


def op_rope(q, k, pos: int, freq_base: float, freq_scale: float, neox: bool, device: int = 0):
    q, k = _f32(q).copy(), _f32(k).copy()  # [n_heads, d], [n_kv, d]
    _chk(load_library().lgh_op_rope(device, q.ctypes.data, k.ctypes.data, q.shape[0], k.shape[0], q.shape[1], pos,
                                    freq_base, freq_scale, int(neox)), "rope")
    return q, k


def op_attention_cached(q, k_cache, v_cache, scale: float, kv_len: int, n_splits: int = 8, device: int = 0) -> np.ndarray:
    q, kc, vc = _f32(q), _f32(k_cache), _f32(v_cache)  # [nh, d], [nkv, max_seq, d]
    out = np.empty_like(q)
    _chk(load_library().lgh_op_attention_cached(device, q.ctypes.data, kc.ctypes.data, vc.ctypes.data, out.ctypes.data,
                                                q.shape[0], kc.shape[0], q.shape[1], kc.shape[1], scale, kv_len,
                                                n_splits), "attention_cached")
    return out


ATTN_SPLIT, ATTN_DIRECT, ATTN_ANY, ATTN_HEAD = 0, 1, 2, 3   # lgh_op_attention_decode paths


def _attn_image(q, n_images: int = 1):
    """The buffer for the XQ images of attention outputs of q's last two axes [nh, d]: [n_images, bytes] (one image: [bytes])."""
    nb = _xq_bytes(q.shape[-2] * q.shape[-1])
    return np.zeros(nb if n_images == 1 else (n_images, nb), np.uint8)


def op_attention_decode(path: int, q, k_cache, v_cache, scale: float, pos: int, n_splits: int = 8, device: int = 0, *, image: bool = False):
    """One decode step's attention over the f32 cache (rows 0..pos stored) on the engine path `path`: ATTN_SPLIT (split + merge),
    ATTN_DIRECT (one launch, a workgroup per kv head), ATTN_HEAD (one launch, a workgroup per query head: the engine's single launch;
    max_seq <= 16384, its scores live in LDS) or ATTN_ANY (any head_dim / group size).  q [nh, d]; caches [nkv, max_seq, d]; pos via the
    device word.
    image: -> (out, wo's input as the launch leaves it: the XQ image of out, uint8 [bytes]); ATTN_ANY writes none (InvalidArgument)."""
    q, kc, vc = _f32(q), _f32(k_cache), _f32(v_cache)
    out = np.empty_like(q)
    img = _attn_image(q) if image else None
    _chk(load_library().lgh_op_attention_decode(device, path, q.ctypes.data, kc.ctypes.data, vc.ctypes.data, out.ctypes.data, q.shape[0],
                                                kc.shape[0], q.shape[1], kc.shape[1], scale, pos, n_splits, _ptr(img)), "attention_decode")
    return (out, img) if image else out


def op_attention_decode_multi(q, k_cache, v_cache, scale: float, pos, slot, n_splits: int = 8, device: int = 0, *, image: bool = False):
    """The multi-sequence decode step's split + merge attention: sequence s attends to rows 0..pos[s] of cache slot slot[s].
    q [n_seq, nh, d]; caches [n_slots, nkv, max_seq, d]; -> [n_seq, nh, d].
    image: -> (out, images uint8 [n_seq + 1, bytes]): every sequence's XQ image of its output, and the one behind the last sequence,
    which no launch may touch (the buffer held the word 0x7FC0BEEF throughout before the launch)."""
    q, kc, vc = _f32(q), _f32(k_cache), _f32(v_cache)
    pos, slot = np.ascontiguousarray(pos, dtype=np.int32), np.ascontiguousarray(slot, dtype=np.int32)
    out = np.empty_like(q)
    img = _attn_image(q, q.shape[0] + 1) if image else None
    _chk(load_library().lgh_op_attention_decode_multi(device, q.ctypes.data, kc.ctypes.data, vc.ctypes.data, out.ctypes.data, q.shape[1],
                                                      kc.shape[1], q.shape[2], kc.shape[2], kc.shape[0], q.shape[0], pos.ctypes.data,
                                                      slot.ctypes.data, scale, n_splits, _ptr(img)), "attention_decode_multi")
    return (out, img) if image else out


def _ptr(a):
    return None if a is None else a.ctypes.data


def op_qkv_rope(types, ws, biases, x, norm_w, eps: float, head_dim: int, n_heads: int, n_kv: int, k_cache, v_cache, pos: int,
                rope_base: float, rope_scale: float, device: int = 0):
    """layer_forward's fused QKV launch (norm, Q / K / V with their own types, RoPE on Q and K, K and V into cache row `pos`).
    ws: three native GGUF byte arrays; biases: three f32 vectors or None; caches [n_kv, max_seq, head_dim].
    -> (q [n_heads * head_dim], k_cache, v_cache) after the call (copies; the inputs are untouched)."""
    x, nw = _f32(x), _f32(norm_w)
    kc, vc = np.array(k_cache, dtype=np.float32, copy=True), np.array(v_cache, dtype=np.float32, copy=True)
    ws = [np.ascontiguousarray(w, dtype=np.uint8) for w in ws]
    bs = [None if b is None else _f32(b) for b in biases]
    tarr = np.array(types, dtype=np.uint32)
    warr = (C.c_void_p * 3)(*[w.ctypes.data for w in ws])
    barr = (C.c_void_p * 3)(*[_ptr(b) for b in bs])
    q = np.empty(n_heads * head_dim, np.float32)
    _chk(load_library().lgh_op_qkv_rope(device, tarr.ctypes.data, C.cast(warr, C.c_void_p), C.cast(barr, C.c_void_p), x.ctypes.data,
                                        nw.ctypes.data, eps, x.size, head_dim, n_heads, n_kv, kc.shape[1], pos, rope_base, rope_scale,
                                        q.ctypes.data, kc.ctypes.data, vc.ctypes.data), "qkv_rope")
    return q, kc, vc


def op_qkv_forward(types, ws, biases, x, norm_w, eps: float, head_dim: int, n_heads: int, n_kv: int, k_cache, v_cache, pos: int,
                   rope_base: float, rope_scale: float, *, neox: bool = False, staged: bool = False, device: int = 0):
    """qkv_forward, whichever branch the types / neox / staged select (op_qkv_rope's arguments; any uploadable weight type).
    -> (q, k_cache, v_cache, staged rows [2, n_kv * head_dim]: K row | V row as kv_tmp holds them after the call).  A refusal raises
    BackendError with the engine's message."""
    x, nw = _f32(x), _f32(norm_w)
    kc, vc = np.array(k_cache, dtype=np.float32, copy=True), np.array(v_cache, dtype=np.float32, copy=True)
    ws = [np.ascontiguousarray(w, dtype=np.uint8) for w in ws]
    bs = [None if b is None else _f32(b) for b in biases]
    tarr = np.array(types, dtype=np.uint32)
    warr = (C.c_void_p * 3)(*[w.ctypes.data for w in ws])
    barr = (C.c_void_p * 3)(*[_ptr(b) for b in bs])
    q = np.empty(n_heads * head_dim, np.float32)
    st = np.empty((2, n_kv * head_dim), np.float32)
    err = C.create_string_buffer(512)
    rc = load_library().lgh_op_qkv_forward(device, tarr.ctypes.data, C.cast(warr, C.c_void_p), C.cast(barr, C.c_void_p), x.ctypes.data,
                                           nw.ctypes.data, eps, x.size, head_dim, n_heads, n_kv, kc.shape[1], pos, rope_base, rope_scale,
                                           int(neox), int(staged), q.ctypes.data, kc.ctypes.data, vc.ctypes.data, st.ctypes.data, err, 512)
    _chk(rc, err.value.decode(errors="replace") or "qkv_forward")
    return q, kc, vc, st


def op_ffn_gateup(type_gate: int, w_gate, type_up: int, w_up, x, norm_w, eps: float, ffn: int, device: int = 0) -> np.ndarray:
    """ffn_gateup_forward: silu(W_gate x') * (W_up x'), x' = RMSNorm(x) * norm_w, gate and up of independent types -> act [ffn]."""
    x, nw = _f32(x), _f32(norm_w)
    wg, wu = np.ascontiguousarray(w_gate, dtype=np.uint8), np.ascontiguousarray(w_up, dtype=np.uint8)
    out = np.empty(ffn, np.float32)
    _chk(load_library().lgh_op_ffn_gateup(device, type_gate, wg.ctypes.data, type_up, wu.ctypes.data, x.ctypes.data, nw.ctypes.data, eps,
                                          x.size, ffn, out.ctypes.data), "ffn_gateup")
    return out


def op_argmax(logits, multi: bool = False, device: int = 0) -> np.ndarray:
    """The two-stage arg-max: logits [n] through the greedy step's launch, or (multi) logits [n_seq, n] through the multi-sequence
    step's.  -> tokens int32 [1] or [n_seq]."""
    lg = _f32(logits)
    n_seq = lg.shape[0] if multi else 0
    out = np.full(max(n_seq, 1), -2, np.int32)
    _chk(load_library().lgh_op_argmax(device, lg.ctypes.data, lg.shape[-1], n_seq, out.ctypes.data), "argmax")
    return out


def op_embed(mode: int, ggml_type: int, table, vocab: int, hidden: int, tokens, *, norm_w=None, fill: int = 0x5A, state=None,
             device: int = 0):
    """The embedding launches on a [vocab, hidden] table of native GGUF bytes.  mode 0: embed_forward (one token; state = (token,
    next position) preset in the device state words, the position word a sentinel); 1: the multi-sequence launch; 2: the batched
    prompt path's.  -> dict(rows f32 [nb, hidden], image uint8 [nb, 1280 per 256 elements] or None, ssq f32 [nb, hidden / 16 + 64] or
    None, state int32 [8] (mode 0)), nb = 1 (mode 0) or len(tokens) + 1; every buffer starts filled with the byte `fill`."""
    tb = np.ascontiguousarray(table, dtype=np.uint8)
    toks = None if mode == 0 else np.ascontiguousarray(tokens, dtype=np.int32)
    n = 1 if mode == 0 else toks.size
    nb = 1 if mode == 0 else n + 1
    nw = None if norm_w is None else _f32(norm_w)
    words = np.zeros(8, np.int32)
    if mode == 0:
        words[0], words[1], words[2] = state[0], -0x5A5A5A5B, state[1]
    rows = np.full(nb * hidden * 4, fill, np.uint8).view(np.float32).reshape(nb, hidden)
    img = np.full((nb, _xq_bytes(hidden)), fill, np.uint8)
    ssq = np.full(nb * (hidden // 16 + 64) * 4, fill, np.uint8).view(np.float32).reshape(nb, -1)
    used = C.c_int(0)
    _chk(load_library().lgh_op_embed(device, mode, ggml_type, tb.ctypes.data, vocab, hidden, _ptr(toks), n, _ptr(nw), fill, words.ctypes.data,
                                     rows.ctypes.data, img.ctypes.data, ssq.ctypes.data, C.byref(used)), "embed")
    return {"rows": rows, "image": img if used.value else None, "ssq": ssq if used.value else None, "state": words}


def op_linear_chain(type_a: int, w_a, k: int, n_a: int, x, type_b: int, w_b, n_b: int, *, w_a_up=None, bias_a=None, norm_w=None,
                    eps: float = 1e-5, resid=None, xq_next: int = 0, next_nw=None, device: int = 0):
    """Launch A (STORE / RESID + bias, or SwiGLU with w_a_up) leaving its output's XQ image (xq_next 0 / 1 / 2), then launch B on
    A's output from that image and again from a fresh conversion.  -> (out_a, out_b, out_b_requant, image_used)."""
    x = _f32(x)
    wa, wb = np.ascontiguousarray(w_a, dtype=np.uint8), np.ascontiguousarray(w_b, dtype=np.uint8)
    wu = None if w_a_up is None else np.ascontiguousarray(w_a_up, dtype=np.uint8)
    ba, nw, rs, nn = (None if v is None else _f32(v) for v in (bias_a, norm_w, resid, next_nw))
    oa, ob, ob2 = np.empty(n_a, np.float32), np.empty(n_b, np.float32), np.empty(n_b, np.float32)
    used = C.c_int(-1)
    _chk(load_library().lgh_op_linear_chain(device, type_a, wa.ctypes.data, _ptr(wu), _ptr(ba), k, n_a, x.ctypes.data, _ptr(nw), eps,
                                            _ptr(rs), xq_next, _ptr(nn), type_b, wb.ctypes.data, n_b, oa.ctypes.data, ob.ctypes.data,
                                            ob2.ctypes.data, C.byref(used)), "linear_chain")
    return oa, ob, ob2, bool(used.value)


def tp_shard(ggml_type: int, ne: Sequence[int], axis: int, rank: int, n_ranks: int, raw, dst: Optional[np.ndarray] = None):
    """lgh_tp_shard (host only): rank `rank`'s shard of a [ne[1] rows][ne[0] elements] GGUF payload, axis 0 = rows, 1 = k.
    -> the shard's bytes; with `dst` (a uint8 buffer) -> the number of bytes written into it."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    ne = list(ne)
    ne4 = (C.c_uint64 * 4)(*(ne + [0] * (4 - len(ne))))
    buf = np.empty(raw.size, np.uint8) if dst is None else dst
    written = C.c_size_t(0)
    _chk(load_library().lgh_tp_shard(ggml_type, ne4, axis, rank, n_ranks, raw.ctypes.data, raw.nbytes, buf.ctypes.data, buf.nbytes,
                                     C.byref(written)), "tp_shard")
    return buf[:written.value].copy() if dst is None else written.value


def kv_cache_layout(kv_cache_type: int, num_kv_heads: int, max_seq_len: int, head_dim: int, flags: int = 0) -> KvLayout:
    """lgh_kv_cache_layout (host only): the sizes of the KV cache a descriptor with these fields asks for."""
    d = ModelDesc()
    d.struct_size = C.sizeof(ModelDesc)
    d.kv_cache_type, d.num_kv_heads, d.max_seq_len, d.head_dim, d.flags = int(kv_cache_type), num_kv_heads, max_seq_len, head_dim, flags
    out = KvLayout()
    _chk(load_library().lgh_kv_cache_layout(C.byref(d), C.byref(out)), "kv_cache_layout")
    return out


def op_tp_reduce(partials, resid=None, norm_w=None, *, image: bool = False, ssq: bool = False, fill: int = 0, device: int = 0):
    """tp_reduce_kernel on its own: out = resid + (((p0 + p1) + p2) ...) over partials [n, H] in rank order.
    -> dict(out, image (uint8 or None), ssq (f32 or None)); every output buffer starts filled with the byte `fill`."""
    p = _f32(partials)
    n, H = p.shape
    rs, nw = (None if v is None else _f32(v) for v in (resid, norm_w))
    out = np.full(H * 4, fill, np.uint8).view(np.float32)
    img = np.full((H + 255) // 256 * 1280, fill, np.uint8) if image else None
    sq = np.full(max(H // 16, 1) * 4, fill, np.uint8).view(np.float32) if ssq else None
    _chk(load_library().lgh_op_tp_reduce(device, p.ctypes.data, n, _ptr(rs), _ptr(nw), H, out.ctypes.data, _ptr(img), _ptr(sq)), "tp_reduce")
    return {"out": out, "image": img, "ssq": sq}


def op_tp_pf_reduce(partials, resid, *, col0: int = 0, bias=None, norm_w=None, path: int = 0, fill: int = 0, device: int = 0):
    """The two row-wise launches of a tensor-parallel prompt block (path 0), or the single context's row epilogue on rank 0's partials
    (path 1, one rank only).  partials [n, S, 128, ncols], resid [m, H].  -> dict(hidden [128, H], xh (uint8 image), ssq [128, 8]);
    every output buffer starts filled with the byte `fill`, rows 0 .. m - 1 of hidden with resid."""
    p, rs = _f32(partials), _f32(resid)
    n, S, rows, ncols = p.shape
    if rows != 128:
        raise ValueError("partials are [n, S, 128, ncols]")
    m, H = rs.shape
    b, nw = (None if v is None else _f32(v) for v in (bias, norm_w))
    hid = np.full((128, H), 0, np.float32)
    hid.view(np.uint8)[...] = fill
    xh = np.full((H + 255) // 256 * 65536, fill, np.uint8)
    sq = np.full(128 * PF_SSQ_CHUNKS * 4, fill, np.uint8).view(np.float32).reshape(128, PF_SSQ_CHUNKS)
    _chk(load_library().lgh_op_tp_pf_reduce(device, path, p.ctypes.data, n, S, ncols, col0, _ptr(b), rs.ctypes.data, _ptr(nw), H, m,
                                            hid.ctypes.data, xh.ctypes.data, sq.ctypes.data), "tp_pf_reduce")
    return {"hidden": hid, "xh": xh, "ssq": sq}


def op_set_flags(flags: int) -> int:
    """Context flags (FLAG_*) of every later op_* / bench_* call of this process; returns the previous value."""
    return int(load_library().lgh_op_set_flags(int(flags)))


def static_launches() -> int:
    """Matrix-core mat-vec launches of this process that ran a static launch plan so far."""
    return int(load_library().lgh_debug_static_launches())


def mv_plan(k: int, n_rows: int, launch_rows: int = 0) -> dict:
    """lgh_debug_mv_plan (host only): the matrix-core mat-vec planner's geometry for a [n_rows, k] weight in a launch of launch_rows
    rows in all.  -> dict(T, G, nbw, rows_per_wg, n_wg, threads, red_floats)."""
    out = (C.c_uint32 * 7)()
    _chk(load_library().lgh_debug_mv_plan(k, n_rows, launch_rows, out), "mv_plan")
    return dict(zip(("T", "G", "nbw", "rows_per_wg", "n_wg", "threads", "red_floats"), (int(v) for v in out)))


def op_linear_image(ggml_type: int, w, k: int, n: int, x, *, w_up=None, bias=None, norm_w=None, eps: float = 1e-5, resid=None,
                    xq_next: int = 0, next_nw=None, want_argmax: bool = False, device: int = 0):
    """One launch as the engine assembles it (STORE / RESID + bias, or SwiGLU with w_up) and everything it leaves.
    -> dict(out, image (uint8 or None), ssq (f32 or None), token, parts, static = 1 if the launch ran a static launch plan)."""
    x = _f32(x)
    wa = np.ascontiguousarray(w, dtype=np.uint8)
    wu = None if w_up is None else np.ascontiguousarray(w_up, dtype=np.uint8)
    ba, nw, rs, nn = (None if v is None else _f32(v) for v in (bias, norm_w, resid, next_nw))
    out = np.empty(n, np.float32)
    img = np.zeros((n + 255) // 256 * 1280, np.uint8)
    ssq = np.zeros(max(n // 16, 1), np.float32)
    used, tok, parts, static = C.c_int(0), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _chk(load_library().lgh_op_linear_image(device, ggml_type, wa.ctypes.data, _ptr(wu), _ptr(ba), k, n, x.ctypes.data, _ptr(nw), eps, _ptr(rs),
                                            xq_next, _ptr(nn), int(want_argmax), out.ctypes.data, img.ctypes.data, ssq.ctypes.data,
                                            C.byref(used), C.byref(tok), C.byref(parts), C.byref(static)), "linear_image")
    return {"out": out, "image": img if used.value else None, "ssq": ssq if used.value and xq_next == 2 else None,
            "token": tok.value, "parts": parts.value, "static": static.value}


def op_moe_experts(type_gate_up: int, w_gate, w_up, type_down: int, w_down, n_experts: int, hidden: int, ffn: int, top_k: int, x,
                   norm_w, eps: float, *, router=None, sel=None, sel_w=None, device: int = 0):
    """ffn_forward's MoE half: x + sum_p w_p down_e(silu(gate_e x') up_e x'), with the device router (router [E, hidden] f32) or the
    given selection (sel int32 / sel_w f32, top_k each).  -> (out [hidden], sel used, weights used)."""
    x, nw = _f32(x), _f32(norm_w)
    wg, wu, wd = (np.ascontiguousarray(w, dtype=np.uint8) for w in (w_gate, w_up, w_down))
    r = None if router is None else _f32(router)
    s = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
    sw = None if sel_w is None else _f32(sel_w)
    out, so, swo = np.empty(hidden, np.float32), np.empty(top_k, np.int32), np.empty(top_k, np.float32)
    _chk(load_library().lgh_op_moe_experts(device, type_gate_up, wg.ctypes.data, wu.ctypes.data, type_down, wd.ctypes.data, n_experts,
                                           hidden, ffn, top_k, _ptr(r), _ptr(s), _ptr(sw), x.ctypes.data, nw.ctypes.data, eps,
                                           out.ctypes.data, so.ctypes.data, swo.ctypes.data), "moe_experts")
    return out, so, swo


# ---- the multi-sequence step's launches, one at a time (lgh_op_*_multi)
MAX_BATCH = 16                                       # kMaxBatch
MV_STRUCTURES = ("mvqb", "mvqb2 split", "mvqb2 seq")  # lgh_debug_mvqb_structures' order


def _structure(counts) -> str:
    """The one structure the launches of a call ran as ('mixed: ...' when they differ)."""
    ran = [MV_STRUCTURES[i] for i in range(3) if counts[i]]
    return ran[0] if len(ran) == 1 else "mixed: %s" % list(counts)


def _xq_bytes(n: int) -> int:
    return (n + 255) // 256 * 1280


def mvqb_structures():
    """Multi-sequence mat-vec launches of this process so far, per structure (MV_STRUCTURES' order)."""
    out = np.zeros(3, np.uint64)
    load_library().lgh_debug_mvqb_structures(out.ctypes.data)
    return [int(v) for v in out]


def op_linear_multi(ggml_type: int, w, k: int, n: int, x, *, max_batch: int = MAX_BATCH, w_up=None, bias=None, norm_w=None, eps: float = 1e-5,
                    resid=None, xq_next: int = 0, next_nw=None, device: int = 0):
    """One multi-sequence launch on x [n_seq, k] as the step assembles it: the SwiGLU pair (w_up), a residual launch (resid [n_seq, n], + bias)
    or a store.  -> dict(out [max_batch, n], pad (a store: the floats between row n and the next sequence's row 0), image [max_batch, bytes] / ssq [max_batch, n / 16] (None without image slots), used,
    structure, counts); rows of sequences >= n_seq come back as the scratch held them (the NaN pattern 0x7FC0BEEF)."""
    x = _f32(x)
    n_seq = x.shape[0]
    wa = np.ascontiguousarray(w, dtype=np.uint8)
    wu = None if w_up is None else np.ascontiguousarray(w_up, dtype=np.uint8)
    ba, nw, rs, nn = (None if v is None else _f32(v) for v in (bias, norm_w, resid, next_nw))
    slots = w_up is not None or resid is not None
    out = np.empty((max_batch, n if slots else (n + 15) // 16 * 16), np.float32)   # (a store's rows lie a whole number of tiles apart)
    img = np.zeros((max_batch, _xq_bytes(n)), np.uint8) if slots else None
    ssq = np.zeros((max_batch, n // 16 + 64), np.float32) if slots else None
    used, counts = C.c_int(0), np.zeros(3, np.int32)
    _chk(load_library().lgh_op_linear_multi(device, ggml_type, wa.ctypes.data, _ptr(wu), _ptr(ba), k, n, n_seq, max_batch, x.ctypes.data, _ptr(nw),
                                            eps, _ptr(rs), xq_next, _ptr(nn), out.ctypes.data, _ptr(img), _ptr(ssq), C.byref(used),
                                            counts.ctypes.data), "linear_multi")
    return {"out": out[:, :n], "pad": out[:, n:], "image": img, "ssq": None if ssq is None else ssq[:, :n // 16], "used": bool(used.value),
            "structure": _structure(counts), "counts": [int(v) for v in counts]}


def op_linear_chain_multi(type_a: int, w_a, k: int, n_a: int, x, type_b: int, w_b, n_b: int, *, max_batch: int = MAX_BATCH, w_a_up=None,
                          bias_a=None, norm_w=None, eps: float = 1e-5, resid=None, xq_next: int = 1, next_nw=None, device: int = 0):
    """op_linear_chain for x [n_seq, k]: A (SwiGLU pair or residual launch) leaves every sequence's image, B (store) runs from them and again
    after a fresh conversion.  -> (out_a [n_seq, n_a], out_b, out_b_requant [n_seq, n_b], image_used)."""
    x = _f32(x)
    n_seq = x.shape[0]
    wa, wb = np.ascontiguousarray(w_a, dtype=np.uint8), np.ascontiguousarray(w_b, dtype=np.uint8)
    wu = None if w_a_up is None else np.ascontiguousarray(w_a_up, dtype=np.uint8)
    ba, nw, rs, nn = (None if v is None else _f32(v) for v in (bias_a, norm_w, resid, next_nw))
    oa, ob, ob2 = np.empty((n_seq, n_a), np.float32), np.empty((n_seq, n_b), np.float32), np.empty((n_seq, n_b), np.float32)
    used = C.c_int(-1)
    _chk(load_library().lgh_op_linear_chain_multi(device, type_a, wa.ctypes.data, _ptr(wu), _ptr(ba), k, n_a, n_seq, max_batch, x.ctypes.data,
                                                  _ptr(nw), eps, _ptr(rs), xq_next, _ptr(nn), type_b, wb.ctypes.data, n_b, oa.ctypes.data,
                                                  ob.ctypes.data, ob2.ctypes.data, C.byref(used)), "linear_chain_multi")
    return oa, ob, ob2, bool(used.value)


def op_qkv_rope_multi(types, ws, biases, x, norm_w, eps: float, head_dim: int, n_heads: int, n_kv: int, max_seq: int, pos, slot,
                      rope_base: float, rope_scale: float, *, max_batch: int = MAX_BATCH, staged: bool = False, device: int = 0):
    """The step's QKV launch(es) on x [n_seq, hidden]: sequence s rotated at pos[s], its K / V rows into row pos[s] of cache slot slot[s].
    -> dict(q [max_batch, n_heads * head_dim], k / v [max_batch, n_kv, max_seq, head_dim] (f32 caches) or staged [max_batch, 2, n_kv *
    head_dim] (the quantized caches' variant), structure, counts)."""
    x, nw = _f32(x), _f32(norm_w)
    n_seq, hidden = x.shape
    ws = [np.ascontiguousarray(w, dtype=np.uint8) for w in ws]
    bs = [None if b is None else _f32(b) for b in biases]
    tarr = np.array(types, dtype=np.uint32)
    warr = (C.c_void_p * 3)(*[w.ctypes.data for w in ws])
    barr = (C.c_void_p * 3)(*[_ptr(b) for b in bs])
    p, s = np.ascontiguousarray(pos, dtype=np.int32), np.ascontiguousarray(slot, dtype=np.int32)
    q = np.empty((max_batch, n_heads * head_dim), np.float32)
    kc = vc = st = None
    if staged:
        st = np.empty((max_batch, 2, n_kv * head_dim), np.float32)
    else:
        kc, vc = np.empty((max_batch, n_kv, max_seq, head_dim), np.float32), np.empty((max_batch, n_kv, max_seq, head_dim), np.float32)
    counts = np.zeros(3, np.int32)
    _chk(load_library().lgh_op_qkv_rope_multi(device, tarr.ctypes.data, C.cast(warr, C.c_void_p), C.cast(barr, C.c_void_p), x.ctypes.data,
                                              nw.ctypes.data, eps, hidden, head_dim, n_heads, n_kv, max_seq, n_seq, max_batch, p.ctypes.data,
                                              s.ctypes.data, rope_base, rope_scale, int(staged), q.ctypes.data, _ptr(kc), _ptr(vc), _ptr(st),
                                              counts.ctypes.data), "qkv_rope_multi")
    return {"q": q, "k": kc, "v": vc, "staged": st, "structure": _structure(counts), "counts": [int(v) for v in counts]}


def op_moe_multi(type_gate_up: int, w_gate, w_up, type_down: int, w_down, n_experts: int, hidden: int, ffn: int, top_k: int, x, norm_w, next_nw,
                 eps: float, *, max_batch: int = MAX_BATCH, router=None, sel=None, sel_w=None, device: int = 0):
    """The grouped MoE half of a step on x [n_seq, hidden]: device router (router [E, hidden]) or the given sel / sel_w [n_seq, top_k].
    -> dict(out [max_batch, hidden], image / ssq as the combine launch left them, image_requant / ssq_requant as the engine's converter
    makes them from out, sel, sel_w [n_seq, top_k], cnt [64], idx [64, 16], counts)."""
    x, nw, nn = _f32(x), _f32(norm_w), _f32(next_nw)
    n_seq = x.shape[0]
    wg, wu, wd = (np.ascontiguousarray(w, dtype=np.uint8) for w in (w_gate, w_up, w_down))
    r = None if router is None else _f32(router)
    s = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
    sw = None if sel_w is None else _f32(sel_w)
    out = np.empty((max_batch, hidden), np.float32)
    img, img2 = (np.zeros((max_batch, _xq_bytes(hidden)), np.uint8) for _ in range(2))
    ssq, ssq2 = (np.zeros((max_batch, hidden // 16 + 64), np.float32) for _ in range(2))
    so, swo = np.empty((n_seq, top_k), np.int32), np.empty((n_seq, top_k), np.float32)
    cnt, idx, counts = np.empty(64, np.int32), np.empty((64, MAX_BATCH), np.int32), np.zeros(3, np.int32)
    _chk(load_library().lgh_op_moe_multi(device, type_gate_up, wg.ctypes.data, wu.ctypes.data, type_down, wd.ctypes.data, n_experts, hidden, ffn,
                                         top_k, n_seq, max_batch, _ptr(r), _ptr(s), _ptr(sw), x.ctypes.data, nw.ctypes.data, nn.ctypes.data, eps,
                                         out.ctypes.data, img.ctypes.data, ssq.ctypes.data, img2.ctypes.data, ssq2.ctypes.data, so.ctypes.data,
                                         swo.ctypes.data, cnt.ctypes.data, idx.ctypes.data, counts.ctypes.data), "moe_multi")
    h16 = hidden // 16
    return {"out": out, "image": img, "ssq": ssq[:, :h16], "image_requant": img2, "ssq_requant": ssq2[:, :h16], "sel": so, "sel_w": swo,
            "cnt": cnt, "idx": idx, "counts": [int(v) for v in counts]}


PF_SSQ_CHUNKS = 8      # kPfSsqChunks: sums of squares per token, one per 2048 columns
PF_TOKENS = 128        # kPfTokens
PF_MOE_ROWS = 384      # kPfMoeRows


def op_pf_qkv(types, ws, biases, hidden, norm_w, eps: float, head_dim: int, n_heads: int, n_kv: int, neox: bool, k_cache, v_cache, pos0: int,
              rope_base: float, rope_scale: float, device: int = 0):
    """The batched prompt path's QKV step on a block hidden [m, H]: XH(hidden * norm_w), the q|k|v GEMM, 1/rms, bias, RoPE at pos0 + t.
    -> (q [m, n_heads * head_dim], k_cache, v_cache) after the call (copies; caches [n_kv, max_seq, head_dim])."""
    h, nw = _f32(hidden), _f32(norm_w)
    m, H = h.shape
    kc, vc = np.array(k_cache, dtype=np.float32, copy=True), np.array(v_cache, dtype=np.float32, copy=True)
    ws = [np.ascontiguousarray(w, dtype=np.uint8) for w in ws]
    bs = [None if b is None else _f32(b) for b in biases]
    tarr = np.array(types, dtype=np.uint32)
    warr = (C.c_void_p * 3)(*[w.ctypes.data for w in ws])
    barr = (C.c_void_p * 3)(*[_ptr(b) for b in bs])
    q = np.empty((m, n_heads * head_dim), np.float32)
    _chk(load_library().lgh_op_pf_qkv(device, tarr.ctypes.data, C.cast(warr, C.c_void_p), C.cast(barr, C.c_void_p), h.ctypes.data, nw.ctypes.data,
                                      eps, H, head_dim, n_heads, n_kv, int(bool(neox)), kc.shape[1], pos0, m, rope_base, rope_scale,
                                      q.ctypes.data, kc.ctypes.data, vc.ctypes.data), "pf_qkv")
    return q, kc, vc


def _pf_outs(m: int, H: int):
    return np.empty((m, H), np.float32), np.full((m, H), np.nan, np.float32), np.full((m, PF_SSQ_CHUNKS), np.nan, np.float32)


def op_pf_linear(ggml_type: int, w, x, resid, next_nw, *, bias=None, device: int = 0):
    """The batched prompt path's wo step: resid [m, H] + W . x (+ bias), x [m, k].  -> (hidden [m, H], next XH [m, H] widened to f32,
    ssq [m, 8])."""
    w, x, r, nn = np.ascontiguousarray(w, dtype=np.uint8), _f32(x), _f32(resid), _f32(next_nw)
    b = None if bias is None else _f32(bias)
    (m, k), H = x.shape, r.shape[1]
    ho, xo, so = _pf_outs(m, H)
    _chk(load_library().lgh_op_pf_linear(device, ggml_type, w.ctypes.data, _ptr(b), x.ctypes.data, k, H, r.ctypes.data, nn.ctypes.data, m,
                                         ho.ctypes.data, xo.ctypes.data, so.ctypes.data), "pf_linear")
    return ho, xo, so


def op_pf_ffn(type_gate_up: int, w_gate, w_up, type_down: int, w_down, hidden, norm_w, ffn: int, *, next_nw=None, eps: float = 1e-5,
              want_act: bool = True, device: int = 0):
    """The batched prompt path's dense FFN step on hidden [m, H].  -> (hidden, next XH (NaN without next_nw), ssq, act [m, ffn] = the
    f16 SwiGLU output the down GEMM read, widened; None with want_act = False)."""
    wg, wu, wd = (np.ascontiguousarray(w, dtype=np.uint8) for w in (w_gate, w_up, w_down))
    h, nw = _f32(hidden), _f32(norm_w)
    nn = None if next_nw is None else _f32(next_nw)
    m, H = h.shape
    ho, xo, so = _pf_outs(m, H)
    act = np.empty((m, ffn), np.float32) if want_act else None
    _chk(load_library().lgh_op_pf_ffn(device, type_gate_up, wg.ctypes.data, wu.ctypes.data, type_down, wd.ctypes.data, h.ctypes.data,
                                      nw.ctypes.data, _ptr(nn), eps, H, ffn, m, ho.ctypes.data, xo.ctypes.data, so.ctypes.data,
                                      _ptr(act)), "pf_ffn")
    return ho, xo, so, act


def op_pf_moe(type_gate_up: int, w_gate, w_up, type_down: int, w_down, router, n_experts: int, top_k: int, hidden, norm_w, ffn: int, *,
              next_nw=None, eps: float = 1e-5, want_act: bool = True, device: int = 0):
    """The batched prompt path's MoE step on hidden [m, H].  -> dict: hidden, xh, ssq, sel / w / tokmap [m, top_k], counts / bases [E],
    lists [E, 128], rowmap [384], act [E, 128, ffn] (every expert's f16 SwiGLU rows as its down GEMM read them; left out with want_act = False)."""
    wg, wu, wd = (np.ascontiguousarray(w, dtype=np.uint8) for w in (w_gate, w_up, w_down))
    h, nw, r = _f32(hidden), _f32(norm_w), _f32(router)
    nn = None if next_nw is None else _f32(next_nw)
    m, H = h.shape
    ho, xo, so = _pf_outs(m, H)
    o = dict(hidden=ho, xh=xo, ssq=so, sel=np.empty((m, top_k), np.int32), w=np.empty((m, top_k), np.float32),
             counts=np.empty(n_experts, np.int32), bases=np.empty(n_experts, np.int32), lists=np.empty((n_experts, PF_TOKENS), np.int32),
             rowmap=np.empty(PF_MOE_ROWS, np.int32), tokmap=np.empty((m, top_k), np.int32))
    act = np.empty((n_experts, PF_TOKENS, ffn), np.float32) if want_act else None
    _chk(load_library().lgh_op_pf_moe(device, type_gate_up, wg.ctypes.data, wu.ctypes.data, type_down, wd.ctypes.data, r.ctypes.data, n_experts,
                                      top_k, h.ctypes.data, nw.ctypes.data, _ptr(nn), eps, H, ffn, m, ho.ctypes.data, xo.ctypes.data,
                                      so.ctypes.data, o["sel"].ctypes.data, o["w"].ctypes.data, o["counts"].ctypes.data, o["bases"].ctypes.data,
                                      o["lists"].ctypes.data, o["rowmap"].ctypes.data, o["tokmap"].ctypes.data, _ptr(act)), "pf_moe")
    if want_act:
        o["act"] = act
    return o


def op_attention_kv8(kv_cache_type: int, q, k_bytes, v_bytes, k_scale, v_scale, k_new, v_new, scale: float, pos: int, n_splits: int = 8,
                     device: int = 0, *, image: bool = False):
    """One decode step's attention over an int8 / FP8 cache (KV_INT8 / KV_FP8_E4M3 / KV_FP8_E5M2): bytes [nkv, max_seq, d] (uint8 or
    int8), scales [nkv, max_seq] (int8 only, else None); the launch stores k_new / v_new [nkv, d] at row `pos`.
    -> (out [nh, d], k_bytes, v_bytes, k_scale, v_scale) after the call (copies; the inputs are untouched); image: and the XQ image of
    out (op_attention_decode) as a last element."""
    q, kn, vn = _f32(q), _f32(k_new), _f32(v_new)
    kb, vb = np.array(k_bytes, dtype=np.uint8, copy=True), np.array(v_bytes, dtype=np.uint8, copy=True)
    i8 = kv_cache_type == KV_INT8
    ks = np.array(k_scale, dtype=np.float32, copy=True) if i8 else None
    vs = np.array(v_scale, dtype=np.float32, copy=True) if i8 else None
    out = np.empty_like(q)
    img = _attn_image(q) if image else None
    _chk(load_library().lgh_op_attention_kv8(device, kv_cache_type, q.ctypes.data, kb.ctypes.data, vb.ctypes.data,
                                             ks.ctypes.data if i8 else None, vs.ctypes.data if i8 else None, kn.ctypes.data, vn.ctypes.data,
                                             out.ctypes.data, q.shape[0], kb.shape[0], q.shape[1], kb.shape[1], scale, pos, n_splits, _ptr(img)),
         "attention_kv8")
    return (out, kb, vb, ks, vs, img) if image else (out, kb, vb, ks, vs)


def op_attention_kv8_multi(kv_cache_type: int, q, k_bytes, v_bytes, k_scale, v_scale, k_new, v_new, scale: float, pos, slot, n_splits: int = 8,
                           device: int = 0, *, image: bool = False):
    """The multi-sequence decode step's attention over int8 / FP8 cache slots: sequence s attends to rows 0..pos[s]-1 of slot slot[s]
    and to its own k_new[s] / v_new[s], which the launch stores at row pos[s] of that slot.  q [n_seq, nh, d]; bytes
    [n_slots, nkv, max_seq, d]; scales [n_slots, nkv, max_seq] (int8 only, else None); k_new / v_new [n_seq, nkv, d].
    -> (out [n_seq, nh, d], k_bytes, v_bytes, k_scale, v_scale) after the call (copies; the inputs are untouched); image: and the
    n_seq + 1 XQ images (op_attention_decode_multi) as a last element."""
    q, kn, vn = _f32(q), _f32(k_new), _f32(v_new)
    kb, vb = np.array(k_bytes, dtype=np.uint8, copy=True), np.array(v_bytes, dtype=np.uint8, copy=True)
    pos, slot = np.ascontiguousarray(pos, dtype=np.int32), np.ascontiguousarray(slot, dtype=np.int32)
    if not (len(pos) == len(slot) == q.shape[0] == kn.shape[0] == vn.shape[0]):
        raise ValueError("op_attention_kv8_multi: q, k_new, v_new, pos and slot must name the same number of sequences")
    i8 = kv_cache_type == KV_INT8
    ks = np.array(k_scale, dtype=np.float32, copy=True) if i8 else None
    vs = np.array(v_scale, dtype=np.float32, copy=True) if i8 else None
    out = np.empty_like(q)
    img = _attn_image(q, q.shape[0] + 1) if image else None
    _chk(load_library().lgh_op_attention_kv8_multi(device, kv_cache_type, q.ctypes.data, kb.ctypes.data, vb.ctypes.data, _ptr(ks), _ptr(vs),
                                                   kn.ctypes.data, vn.ctypes.data, out.ctypes.data, q.shape[1], kb.shape[1], q.shape[2],
                                                   kb.shape[2], kb.shape[0], len(pos), pos.ctypes.data, slot.ctypes.data, scale, n_splits,
                                                   _ptr(img)), "attention_kv8_multi")
    return (out, kb, vb, ks, vs, img) if image else (out, kb, vb, ks, vs)


def op_attention_tq(kv_cache_type: int, q, k_codes, v_codes, k_qjl, k_new, v_new, signs, qjl_matrices, scale: float, pos: int,
                    n_splits: int = 8, device: int = 0, *, image: bool = False):
    """One decode step's attention over a TurboQuant cache (KV_TQ2 / TQ3 / TQ2_QJL / TQ3_QJL): codes [nkv, max_seq, row bytes];
    k_qjl [nkv, max_seq, d / 32 + 1] uint32 words (QJL types, else None); signs [nkv, 2, d]; qjl_matrices [nkv, d, d] (QJL types).
    The launch compresses k_new / v_new [nkv, d] into row `pos`.  -> (out [nh, d], k_codes, v_codes, k_qjl) after the call (copies);
    image: and the XQ image of out (op_attention_decode) as a last element."""
    q, kn, vn, sg = _f32(q), _f32(k_new), _f32(v_new), _f32(signs)
    kc, vc = np.array(k_codes, dtype=np.uint8, copy=True), np.array(v_codes, dtype=np.uint8, copy=True)
    qjl = kv_cache_type in (KV_TQ2_QJL, KV_TQ3_QJL)
    kx = np.array(k_qjl, dtype=np.uint32, copy=True) if qjl else None
    S = _f32(qjl_matrices) if qjl else None
    out = np.empty_like(q)
    img = _attn_image(q) if image else None
    _chk(load_library().lgh_op_attention_tq(device, kv_cache_type, q.ctypes.data, kc.ctypes.data, vc.ctypes.data,
                                            kx.ctypes.data if qjl else None, kn.ctypes.data, vn.ctypes.data, sg.ctypes.data,
                                            S.ctypes.data if qjl else None, out.ctypes.data, q.shape[0], kc.shape[0], q.shape[1],
                                            kc.shape[1], scale, pos, n_splits, _ptr(img)), "attention_tq")
    return (out, kc, vc, kx, img) if image else (out, kc, vc, kx)


def op_attention_tq_multi(kv_cache_type: int, q, k_codes, v_codes, k_qjl, k_new, v_new, signs, qjl_matrices, scale: float, pos, slot,
                          n_splits: int = 8, device: int = 0, *, image: bool = False):
    """The multi-sequence decode step's attention over TurboQuant cache slots: sequence s attends to rows 0..pos[s]-1 of slot slot[s] and
    to its own k_new[s] / v_new[s], which the launch compresses into row pos[s] of that slot.  q [n_seq, nh, d]; codes
    [n_slots, nkv, max_seq, row bytes]; k_qjl [n_slots, nkv, max_seq, d / 32 + 1] uint32 words (QJL types, else None); k_new / v_new
    [n_seq, nkv, d]; signs [nkv, 2, d]; qjl_matrices [nkv, d, d] (QJL types).
    -> (out [n_seq, nh, d], k_codes, v_codes, k_qjl) after the call (copies; the inputs are untouched); image: and the n_seq + 1 XQ
    images (op_attention_decode_multi) as a last element."""
    q, kn, vn, sg = _f32(q), _f32(k_new), _f32(v_new), _f32(signs)
    kc, vc = np.array(k_codes, dtype=np.uint8, copy=True), np.array(v_codes, dtype=np.uint8, copy=True)
    pos, slot = np.ascontiguousarray(pos, dtype=np.int32), np.ascontiguousarray(slot, dtype=np.int32)
    if not (len(pos) == len(slot) == q.shape[0] == kn.shape[0] == vn.shape[0]):
        raise ValueError("op_attention_tq_multi: q, k_new, v_new, pos and slot must name the same number of sequences")
    qjl = kv_cache_type in (KV_TQ2_QJL, KV_TQ3_QJL)
    kx = np.array(k_qjl, dtype=np.uint32, copy=True) if qjl else None
    S = _f32(qjl_matrices) if qjl else None
    out = np.empty_like(q)
    img = _attn_image(q, q.shape[0] + 1) if image else None
    _chk(load_library().lgh_op_attention_tq_multi(device, kv_cache_type, q.ctypes.data, kc.ctypes.data, vc.ctypes.data, _ptr(kx), kn.ctypes.data,
                                                  vn.ctypes.data, sg.ctypes.data, _ptr(S), out.ctypes.data, q.shape[1], kc.shape[1], q.shape[2],
                                                  kc.shape[2], kc.shape[0], len(pos), pos.ctypes.data, slot.ctypes.data, scale, n_splits,
                                                  _ptr(img)), "attention_tq_multi")
    return (out, kc, vc, kx, img) if image else (out, kc, vc, kx)


def op_attention_prefill(q, k_cache, v_cache, scale: float, pos0: int, device: int = 0) -> np.ndarray:
    """Causal attention of a block of prompt tokens on the batched-prefill kernel: q [m, nh, d] at positions pos0..pos0+m-1; the
    caches [nkv, max_seq, d] hold rows 0..pos0+m-1.  -> [m, nh * d]: the kernel's f16 outputs widened to f32."""
    q, kc, vc = _f32(q), _f32(k_cache), _f32(v_cache)
    m, nh, d = q.shape
    out = np.empty((m, nh * d), dtype=np.float32)
    _chk(load_library().lgh_op_attention_prefill(device, q.ctypes.data, kc.ctypes.data, vc.ctypes.data, out.ctypes.data, nh, kc.shape[0], d,
                                                 kc.shape[1], scale, pos0, m), "attention_prefill")
    return out


def op_pf_tq_store(kv_cache_type: int, k_rows, v_rows, pos0: int, signs, k_codes, v_codes, device: int = 0):
    """The batched prefill's TurboQuant row store (KV_TQ2 / KV_TQ3): k_rows / v_rows [nkv, m, d] f32 are compressed into rows
    pos0..pos0+m-1 of the code caches [nkv, max_seq, row bytes]; signs [nkv, 2, d].  -> (k_codes, v_codes) after the call (copies)."""
    kr, vr, sg = _f32(k_rows), _f32(v_rows), _f32(signs)
    kc, vc = np.array(k_codes, dtype=np.uint8, copy=True), np.array(v_codes, dtype=np.uint8, copy=True)
    nkv, m, d = kr.shape
    _chk(load_library().lgh_op_pf_tq_store(device, kv_cache_type, kr.ctypes.data, vr.ctypes.data, m, nkv, d, kc.shape[1], pos0,
                                           sg.ctypes.data, kc.ctypes.data, vc.ctypes.data), "pf_tq_store")
    return kc, vc


def op_pf_kv8_store(kv_cache_type: int, k_rows, v_rows, pos0: int, k_bytes, v_bytes, k_scales=None, v_scales=None, device: int = 0):
    """The batched prefill's byte-cache row store (KV_INT8 / KV_FP8_E4M3 / KV_FP8_E5M2): k_rows / v_rows [nkv, m, d] f32 are quantized
    into rows pos0..pos0+m-1 of the byte caches [nkv, max_seq, d] and, int8, of the scales [nkv, max_seq] (ignored for FP8).
    -> (k_bytes, v_bytes, k_scales, v_scales) after the call (copies; the scales None where none were given)."""
    kr, vr = _f32(k_rows), _f32(v_rows)
    kb, vb = np.array(k_bytes, dtype=np.uint8, copy=True), np.array(v_bytes, dtype=np.uint8, copy=True)
    ks = None if k_scales is None else np.array(k_scales, dtype=np.float32, copy=True)
    vs = None if v_scales is None else np.array(v_scales, dtype=np.float32, copy=True)
    nkv, m, d = kr.shape
    _chk(load_library().lgh_op_pf_kv8_store(device, kv_cache_type, kr.ctypes.data, vr.ctypes.data, m, nkv, d, kb.shape[1], pos0, kb.ctypes.data,
                                            vb.ctypes.data, None if ks is None else ks.ctypes.data, None if vs is None else vs.ctypes.data),
         "pf_kv8_store")
    return kb, vb, ks, vs


def op_attention_prefill_kv8(kv_cache_type: int, q, k_bytes, v_bytes, k_scales, v_scales, scale: float, pos0: int, device: int = 0) -> np.ndarray:
    """Causal attention of a block of prompt tokens over a byte cache (KV_INT8 / KV_FP8_E4M3 / KV_FP8_E5M2) as the batched prefill runs
    it: q [m, nh, d] at positions pos0..pos0+m-1; the byte caches [nkv, max_seq, d] hold rows 0..pos0+m-1, the scales [nkv, max_seq]
    go with int8 (ignored, and may be None, for FP8).  -> [m, nh * d]: the kernel's f16 outputs widened to f32."""
    q = _f32(q)
    kb, vb = np.ascontiguousarray(k_bytes, dtype=np.uint8), np.ascontiguousarray(v_bytes, dtype=np.uint8)
    ks = None if k_scales is None else _f32(k_scales)
    vs = None if v_scales is None else _f32(v_scales)
    m, nh, d = q.shape
    out = np.empty((m, nh * d), dtype=np.float32)
    _chk(load_library().lgh_op_attention_prefill_kv8(device, kv_cache_type, q.ctypes.data, kb.ctypes.data, vb.ctypes.data,
                                                     None if ks is None else ks.ctypes.data, None if vs is None else vs.ctypes.data,
                                                     out.ctypes.data, nh, kb.shape[0], d, kb.shape[1], scale, pos0, m), "attention_prefill_kv8")
    return out


def op_kv_prefix_copy(kv_cache_type: int, caches, slot: int, n_rows: int, head_dim: int, packed=None, device: int = 0):
    """kv_prefix_copy_kernel over host arrays.  caches: per layer the five tensors (K, V, K scales, V scales, K QJL words) as uint8
    arrays [n_slots, nkv, max_seq, bytes per position], None where the format has none.  packed None: save -> the packed rows
    (uint8) of `slot`; else restore -> the caches after the launch (copies, same nesting)."""
    lay = [[None if t is None else np.array(t, dtype=np.uint8, copy=True) for t in layer] for layer in caches]
    first = next(t for t in lay[0] if t is not None)
    n_slots, nkv, max_seq = first.shape[:3]
    ptrs = (C.c_void_p * (5 * len(lay)))(*[None if t is None else t.ctypes.data for layer in lay for t in layer])
    per_pos = sum(t.shape[3] for t in lay[0] if t is not None)
    if packed is None:
        buf = np.zeros(len(lay) * nkv * n_rows * per_pos, dtype=np.uint8)
    else:
        buf = np.ascontiguousarray(packed, dtype=np.uint8)
        assert buf.size == len(lay) * nkv * n_rows * per_pos
    _chk(load_library().lgh_op_kv_prefix_copy(device, kv_cache_type, nkv, max_seq, head_dim, len(lay), n_slots, ptrs, slot, n_rows,
                                              buf.ctypes.data, 0 if packed is None else 1), "kv_prefix_copy")
    return buf if packed is None else lay


def op_attention_prefill_tq(kv_cache_type: int, q, k_codes, v_codes, signs, scale: float, pos0: int, device: int = 0) -> np.ndarray:
    """Causal attention of a block of prompt tokens over a TurboQuantMSE cache (KV_TQ2 / KV_TQ3) as the batched prefill runs it: q
    [m, nh, d] at positions pos0..pos0+m-1; the code caches [nkv, max_seq, row bytes] hold rows 0..pos0+m-1; signs [nkv, 2, d].
    -> [m, nh * d]: the kernel's f16 outputs widened to f32."""
    q, sg = _f32(q), _f32(signs)
    kc, vc = np.ascontiguousarray(k_codes, dtype=np.uint8), np.ascontiguousarray(v_codes, dtype=np.uint8)
    m, nh, d = q.shape
    out = np.empty((m, nh * d), dtype=np.float32)
    _chk(load_library().lgh_op_attention_prefill_tq(device, kv_cache_type, q.ctypes.data, kc.ctypes.data, vc.ctypes.data, sg.ctypes.data,
                                                    out.ctypes.data, nh, kc.shape[0], d, kc.shape[1], scale, pos0, m), "attention_prefill_tq")
    return out


def op_kv_roundtrip(kv_cache_type: int, row, device: int = 0):
    """One row through a KV cache format (KV_INT8 / KV_FP8_E4M3 / KV_FP8_E5M2) and back: (bytes, scale, values read back)."""
    x = _f32(row)
    b = np.zeros(x.size, dtype=np.uint8)
    back = np.empty_like(x)
    sc = C.c_float(1.0)
    _chk(load_library().lgh_op_kv_roundtrip(device, kv_cache_type, x.ctypes.data, x.size, b.ctypes.data, C.addressof(sc),
                                            back.ctypes.data), "kv_roundtrip")
    return b, float(sc.value), back


def op_tq_compress(x, bits: int, signs, device: int = 0) -> np.ndarray:
    """TurboQuantEngine::compress without QJL (src/model/turboquant/quant.rs:71-103) on the device: the row's packed codes."""
    x, sg = _f32(x), _f32(signs)
    out = np.zeros(x.size // 4 if bits == 2 else x.size // 8 * 3, dtype=np.uint8)
    _chk(load_library().lgh_op_tq_compress(device, bits, x.ctypes.data, x.size, sg.ctypes.data, out.ctypes.data), "tq_compress")
    return out


def op_tq_compress_qjl(x, bits: int, signs, qjl_matrix, device: int = 0):
    """TurboQuantEngine::compress with use_qjl (quant.rs:71-103) on the device -> (codes, qjl_bits uint64[dim / 64], residual_norm)."""
    x, sg, S = _f32(x), _f32(signs), _f32(qjl_matrix)
    assert S.size == x.size * x.size
    codes = np.zeros(x.size // 4 if bits == 2 else x.size // 8 * 3, dtype=np.uint8)
    qb = np.zeros(x.size // 64, dtype=np.uint64)
    norm = C.c_float(0.0)
    _chk(load_library().lgh_op_tq_compress_qjl(device, bits, x.ctypes.data, x.size, sg.ctypes.data, S.ctypes.data, codes.ctypes.data,
                                               qb.ctypes.data, C.addressof(norm)), "tq_compress_qjl")
    return codes, qb, float(norm.value)


def op_sample(logits, recent: Sequence[int] = (), counts=None, uniform: float = 0.0, device: int = 0, mu: Optional[float] = None,
              **cfg):
    """One Sampler::sample call on the device (lgh_op_sample); cfg: keyword arguments of `sampler_config`.  With min_p / mirostat /
    tau / eta among them it goes through lgh_op_sample_ex; under Mirostat `mu` is the sampler's mirostat_mu before the call
    (default 2 * tau, as Sampler::new sets it) and the result is (token, mu after the call)."""
    lg = _f32(logits)
    rc = np.ascontiguousarray(recent, dtype=np.uint32)
    cn = np.ascontiguousarray(counts, dtype=np.uint32) if counts is not None else None
    if cn is not None:
        assert cn.size == lg.size
    tok = C.c_uint32()
    if _is_ex(cfg) or mu is not None:
        ex = sampler_config_ex(**cfg)
        mu_in = float(mu) if mu is not None else 2.0 * ex.mirostat_tau
        mu_out = C.c_float()
        _chk(load_library().lgh_op_sample_ex(device, lg.ctypes.data, lg.size, C.byref(ex), rc.ctypes.data if rc.size else None, rc.size,
                                             cn.ctypes.data if cn is not None else None, float(uniform), mu_in, C.byref(tok),
                                             C.byref(mu_out)), "lgh_op_sample_ex")
        return (tok.value, mu_out.value) if ex.mirostat else tok.value
    _chk(load_library().lgh_op_sample(device, lg.ctypes.data, lg.size, C.byref(sampler_config(**cfg)),
                                      rc.ctypes.data if rc.size else None, rc.size, cn.ctypes.data if cn is not None else None,
                                      float(uniform), C.byref(tok)), "lgh_op_sample")
    return tok.value


def op_silu_mul(gate, up, device: int = 0) -> np.ndarray:
    g, u = _f32(gate), _f32(up)
    out = np.empty_like(g)
    _chk(load_library().lgh_op_silu_mul(device, g.ctypes.data, u.ctypes.data, out.ctypes.data, g.size), "silu_mul")
    return out


class HipBackend:
    """Mirror of the reference's per-op `Backend` trait (src/backend/mod.rs:29-265) over the C ABI: host tensors (numpy
    arrays) in and out, the same method names and argument meaning; what `select_gpu_backend` (src/engine.rs:738-812) would
    hold as `Box<dyn Backend>`.  `load_weight` + a `name=` on vec_mat_q is the CUDA backend's device-resident weight store
    (src/backend/cuda/mod.rs:121-146, 511-575).  No CPU fallback: every method runs a HIP kernel or raises."""

    def __init__(self, device: int = 0):
        self.device = device
        self._h = C.c_void_p()
        _chk(load_library().lgh_backend_create(device, C.byref(self._h)), "lgh_backend_create (is a HIP device visible?)")

    def close(self) -> None:
        if self._h:
            load_library().lgh_backend_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def name(self) -> str:
        return "hip"

    def is_available(self) -> bool:
        return device_count() > self.device

    # memory: host tensors are the currency of this surface (backend/mod.rs:40-49)
    def alloc(self, shape, dtype=np.float32) -> np.ndarray:
        return np.zeros(shape, dtype=dtype)

    def copy_to(self, tensor: np.ndarray) -> np.ndarray:
        return np.array(tensor, copy=True)

    def _ew(self, fn, what, *arrs, scalar=None):
        a = [_f32(x) for x in arrs]
        for b in a[1:]:
            if b.shape != a[0].shape:
                raise BackendError(2, f"{what}: shapes {a[0].shape} and {b.shape} differ")   # check_same_shape (ops.rs:1543)
        out = np.empty_like(a[0])
        args = [self.device] + [x.ctypes.data for x in a] + ([scalar] if scalar is not None else []) + [out.ctypes.data, out.size]
        _chk(fn(*args), what)
        return out

    def add(self, a, b) -> np.ndarray:
        return self._ew(load_library().lgh_op_add, "add", a, b)

    def mul(self, a, b) -> np.ndarray:
        return self._ew(load_library().lgh_op_mul, "mul", a, b)

    def scale(self, a, scalar: float) -> np.ndarray:
        return self._ew(load_library().lgh_op_scale, "scale", a, scalar=float(scalar))

    def silu(self, x) -> np.ndarray:
        return self._ew(load_library().lgh_op_silu, "silu", x)

    def gelu(self, x) -> np.ndarray:
        return self._ew(load_library().lgh_op_gelu, "gelu", x)

    def softmax(self, x) -> np.ndarray:
        x = _f32(x)
        out = np.empty_like(x)
        last = x.shape[-1] if x.ndim else 1
        _chk(load_library().lgh_op_softmax(self.device, x.ctypes.data, out.ctypes.data, x.size // max(last, 1), last), "softmax")
        return out

    def rms_norm(self, x, weight, eps: float) -> np.ndarray:
        return op_rms_norm(x, weight, eps, self.device)

    def matmul(self, a, b) -> np.ndarray:
        a, b = _f32(a), _f32(b)
        if a.ndim != 2 or b.ndim != 2:
            raise BackendError(6, "matmul requires 2D tensors")                                  # ops.rs:434-438
        if a.shape[1] != b.shape[0]:
            raise BackendError(2, f"matmul: [{a.shape}] @ [{b.shape}]")                            # ops.rs:443-448
        out = np.empty((a.shape[0], b.shape[1]), dtype=np.float32)
        _chk(load_library().lgh_op_matmul(self.device, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.shape[0], a.shape[1], b.shape[1]), "matmul")
        return out

    def matvec(self, a, b) -> np.ndarray:
        a, b = _f32(a), _f32(b)
        if a.ndim != 2 or b.ndim != 1:
            raise BackendError(6, "matvec requires 2D matrix and 1D vector")                     # ops.rs:536-540
        if b.shape[0] != a.shape[1]:
            raise BackendError(2, f"matvec: expected [{a.shape[1]}], got {b.shape}")
        out = np.empty(a.shape[0], dtype=np.float32)
        _chk(load_library().lgh_op_matvec(self.device, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.shape[0], a.shape[1]), "matvec")
        return out

    def vec_mat(self, a, b_f32, n: int) -> np.ndarray:
        """x [k] @ W [k, n] with W in GGUF order (element (i, j) at i + j*k, ops.rs:959-1002)."""
        return op_vec_mat(0, _f32(b_f32), a, n, self.device)

    def dequantize(self, ggml_type: int, raw: np.ndarray, n_elems: int) -> np.ndarray:
        return op_dequantize(ggml_type, raw, n_elems, self.device)

    def matvec_q(self, ggml_type: int, a_raw: np.ndarray, b, m: int) -> np.ndarray:
        a_raw, b = np.ascontiguousarray(a_raw), _f32(b)
        out = np.empty(m, dtype=np.float32)
        _chk(load_library().lgh_op_matvec_q(self.device, ggml_type, a_raw.ctypes.data, b.ctypes.data, out.ctypes.data, m, b.size), "matvec_q")
        return out

    def load_weight(self, name: str, ggml_type: int, raw: np.ndarray, k: int, n: int) -> None:
        raw = np.ascontiguousarray(raw)
        self._call(load_library().lgh_backend_load_weight(self._h, name.encode(), ggml_type, raw.ctypes.data, k, n))

    def has_weight(self, name: str) -> bool:
        return bool(load_library().lgh_backend_has_weight(self._h, name.encode()))

    def vec_mat_q(self, a, ggml_type: int = 0, b_raw: Optional[np.ndarray] = None, n: int = 0, name: Optional[str] = None) -> np.ndarray:
        """x [k] @ quantized W (n rows of k/bs blocks).  With `name` of a loaded weight nothing but x crosses PCIe."""
        a = _f32(a)
        if name is not None and self.has_weight(name):
            out = np.empty(n, dtype=np.float32)
            self._call(load_library().lgh_backend_vec_mat_q(self._h, name.encode(), a.ctypes.data, out.ctypes.data, a.size, n))
            return out
        if b_raw is None:
            raise BackendError(6, f"vec_mat_q: no device-resident weight named {name!r} and no host tensor given")
        return op_vec_mat(ggml_type, b_raw, a, n, self.device)

    def rope(self, q, k, pos: int, freq_base: float, freq_scale: float, use_neox: bool):
        return op_rope(q, k, pos, freq_base, freq_scale, use_neox, self.device)

    def attention(self, q, k, v, scale: float) -> np.ndarray:
        q, k, v = _f32(q), _f32(k), _f32(v)
        if q.ndim != 3 or k.ndim != 3 or v.ndim != 3:
            raise BackendError(6, "Attention requires 3D tensors")                               # ops.rs:1365-1369
        if k.shape[2] != q.shape[2] or v.shape != k.shape or q.shape[0] % k.shape[0]:
            raise BackendError(6, "Attention tensor dimension mismatch")                         # ops.rs:1381-1389
        out = np.empty_like(q)
        _chk(load_library().lgh_op_attention(self.device, q.ctypes.data, k.ctypes.data, v.ctypes.data, out.ctypes.data, q.shape[0],
                                             k.shape[0], q.shape[1], k.shape[1], q.shape[2], scale), "attention")
        return out

    def flash_attention(self, q, k, v, scale: float, causal: bool = True) -> np.ndarray:   # backend/mod.rs:159-171: defaults to attention
        return self.attention(q, k, v, scale)

    def attention_cached(self, q, k_cache, v_cache, scale: float, kv_len: int) -> np.ndarray:
        return op_attention_cached(q, k_cache, v_cache, scale, kv_len, device=self.device)

    def _call(self, status: int) -> None:
        if status != 0:
            raise BackendError(status, load_library().lgh_backend_last_error(self._h).decode())


def bench_vec_mat(ggml_type: int, w: np.ndarray, k: int, n: int, mode: int = 0, iters: int = 50,
                  w2: Optional[np.ndarray] = None, copies: int = 1, device: int = 0) -> float:
    """Mean device time (µs) of one fused mat-vec launch (hipEvents on the launch stream)."""
    w = np.ascontiguousarray(w)
    us = C.c_double()
    _chk(load_library().lgh_bench_vec_mat(device, ggml_type, w.ctypes.data, w2.ctypes.data if w2 is not None else None,
                                          k, n, mode, iters, copies, C.byref(us)), "bench_vec_mat")
    return us.value


def bench_hbm_read(nbytes: int = 1 << 30, iters: int = 10, device: int = 0) -> float:
    """Measured streaming-read rate of the device in GB/s (the practical ceiling next to the 8 TB/s spec peak)."""
    out = C.c_double(0.0)
    _chk(load_library().lgh_bench_hbm_read(device, nbytes, iters, C.byref(out)), "bench_hbm_read")
    return float(out.value)


def gguf_inspect(path: str) -> dict:
    """Header of a GGUF file as the loader sees it (no GPU needed): version, counts, architecture, model description."""
    info = GgufInfo()
    err = C.create_string_buffer(512)
    rc = load_library().lgh_gguf_inspect(path.encode(), C.byref(info), err, len(err))
    if rc:
        raise BackendError(rc, "lgh_gguf_inspect: " + err.value.decode(errors="replace"))
    return {"version": info.version, "alignment": info.alignment, "n_tensors": info.n_tensors, "n_kv": info.n_kv,
            "data_offset": info.data_offset, "file_bytes": info.file_bytes, "architecture": info.architecture.decode(),
            "has_model_config": info.desc.struct_size != 0, "note": err.value.decode(errors="replace"),
            "desc": {n: getattr(info.desc, n) for n, _ in ModelDesc._fields_}}


GGUF_VALUE_TYPES = ("u8", "i8", "u16", "i16", "u32", "i32", "f32", "bool", "string", "array", "u64", "i64", "f64")


def gguf_get(path: str, key: str):
    """One metadata value: (type name, python value) — GgufData::get_* (src/gguf/types.rs:71-104); None when absent."""
    v = GgufValue()
    err = C.create_string_buffer(512)
    rc = load_library().lgh_gguf_get(path.encode(), key.encode(), C.byref(v), err, len(err))
    if rc:
        msg = err.value.decode(errors="replace")
        if msg.startswith("no metadata key"):
            return None
        raise BackendError(rc, "lgh_gguf_get: " + msg)
    t = GGUF_VALUE_TYPES[v.type]
    if t in ("f32", "f64"):
        return t, float(v.f)
    if t == "string":
        return t, v.s.decode(errors="replace")
    if t == "array":
        return t, int(v.arr_len)
    if t == "bool":
        return t, bool(v.u)
    if t in ("i8", "i16", "i32", "i64"):
        return t, int(C.c_int64(v.u).value)
    return t, int(v.u)
