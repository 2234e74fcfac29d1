from pygpukit_amd.ops.nn.activation import gelu, quick_gelu, relu2, sigmoid, silu, tanh
from pygpukit_amd.ops.nn.alibi import sdpa_alibi, sdpa_alibi_fixed_cache, sdpa_alibi_fixed_cache_ptr, sdpa_alibi_strided
from pygpukit_amd.ops.nn.attention import (fa3_fp8_available, get_sm_version, quantize_fp8_per_head, sdpa_causal,
                                          sdpa_causal_fixed_cache, sdpa_causal_fixed_cache_ptr, sdpa_causal_fp8,
                                          sdpa_causal_fp8_strided, sdpa_causal_strided, sdpa_noncausal,
                                          sdpa_noncausal_strided)
from pygpukit_amd.ops.nn.fused import geglu, glu_packed, rmsnorm_residual, swiglu
from pygpukit_amd.ops.nn.llama4 import (irope_scale_q, l2norm, llama4_qk_norm_cache_write, llama4_qk_norm_cache_write_ptr,
                                        sdpa_irope, sdpa_irope_fixed_cache, sdpa_irope_fixed_cache_ptr, sdpa_irope_strided)
from pygpukit_amd.ops.nn.linear import (bias_add_inplace, embed_token_position_ptr, ln_linear, ln_linear_plan, ln_linear_qkv_cache_ptr,
                                        slice_rows_range_ptr, split_qkv_batch)
from pygpukit_amd.ops.nn.norm import group_norm, group_norm_plan, group_norm_silu, layernorm, rmsnorm
from pygpukit_amd.ops.nn.relpos import (relbias_plan, relpos_bias_table, relpos_bucket, relpos_compute_bias, sdpa_relbias,
                                        sdpa_relbias_strided)
from pygpukit_amd.ops.nn.recurrent import lstm_bidirectional, lstm_forward, lstm_plan
from pygpukit_amd.ops.nn.rope import (alibi_add_bias, alibi_compute_bias, alibi_init_slopes, pope_init_encoding, pope_inplace,
                                      rope_init_linear, rope_init_ntk_aware, rope_init_yarn, rope_inplace, rope_inplace_f32table)

__all__ = ["gelu", "silu", "sigmoid", "tanh", "relu2", "sdpa_causal", "sdpa_causal_fixed_cache",
           "sdpa_causal_fixed_cache_ptr", "sdpa_causal_strided", "sdpa_causal_fp8", "sdpa_causal_fp8_strided", "fa3_fp8_available",
           "get_sm_version", "quantize_fp8_per_head", "rmsnorm_residual", "swiglu", "geglu", "glu_packed",
           "bias_add_inplace", "split_qkv_batch", "slice_rows_range_ptr", "layernorm", "rmsnorm", "rope_inplace",
           "rope_inplace_f32table", "l2norm", "irope_scale_q", "sdpa_irope", "sdpa_irope_strided", "llama4_qk_norm_cache_write",
           "llama4_qk_norm_cache_write_ptr", "sdpa_irope_fixed_cache", "sdpa_irope_fixed_cache_ptr", "rope_init_ntk_aware",
           "rope_init_yarn", "rope_init_linear", "pope_init_encoding", "pope_inplace", "alibi_init_slopes", "alibi_compute_bias",
           "alibi_add_bias", "sdpa_alibi", "sdpa_alibi_strided", "sdpa_alibi_fixed_cache", "sdpa_alibi_fixed_cache_ptr",
           "lstm_forward", "lstm_bidirectional", "lstm_plan", "sdpa_noncausal", "sdpa_noncausal_strided", "ln_linear",
           "ln_linear_plan", "ln_linear_qkv_cache_ptr", "embed_token_position_ptr", "group_norm", "group_norm_silu", "group_norm_plan",
           "relpos_bucket", "relpos_bias_table", "relpos_compute_bias", "sdpa_relbias", "sdpa_relbias_strided", "relbias_plan", "quick_gelu"]
