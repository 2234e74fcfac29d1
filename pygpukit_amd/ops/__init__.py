"""pygpukit_amd.ops: operator surface mirroring pygpukit.ops on the LLM-inference hot path."""

from pygpukit_amd.ops.conv import conv1d, conv2d
from pygpukit_amd.ops.elementwise import add, add_inplace, clamp, copy_to, div, mul, mul_inplace, sub, where
from pygpukit_amd.ops.embedding import (embedding_lookup, embedding_lookup_batch, embedding_lookup_ptr,
                                       kv_cache_prefill, kv_cache_prefill_gqa, kv_cache_update, kv_cache_update_gqa, kv_cache_update_gqa_ptr)
from pygpukit_amd.ops.matmul import (batched_matmul, gemm_w8a16_init_lut, gemv_bf16, gemv_bf16_opt_available, gemv_fp8_bf16,
                                    gemv_fp8_bf16_batched, linear_bias_gelu, matmul, matmul_nt, transpose, w8a16_gemm,
                                    w8a16_gemm_nk, w8a16_gemm_sm120, matmul_fp8, matmul_fp8_sm120, gemm_fp8_fp8_blockwise_nt,
                                    quantize_fp8_rows, quantize_fp8_blocks, fp8_available, fp8_init_lut, matmul_fp8_fp8_sm120,
                                    gemm_fp8_fp8_sm120, matmul_fp8_fp8_blockwise_sm120, gemm_fp8_fp8_blockwise_sm120,
                                    fp8_fp8_get_scale_sizes, gemm_fp8_fp8_get_scale_sizes, fp8_get_sizes, fp8_fp8_sm120_available,
                                    gemm_fp8_fp8_sm120_available, grouped_gemm_bf16, grouped_gemm_fp8_bf16,
                                    grouped_gemm_fp8_bf16_sm120, grouped_gemm_init_lut, nvf4_get_sizes, gemv_nvf4_get_sizes,
                                    quantize_bf16_to_nvf4, matmul_nvf4_bf16_sm120, gemm_nvf4_bf16_sm120, gemv_nvf4_bf16,
                                    gemv_nvf4_bf16_sm120, nvf4_bf16_sm120_available, gemm_nvf4_bf16_sm120_available,
                                    gemv_nvf4_available, gemv_nvf4_bf16_sm120_available, nvf4_nk_get_sizes,
                                    quantize_bf16_to_nvf4_nk, quantize_nvf4_nk)
from pygpukit_amd.ops.moe import (moe_compute_permutation, moe_expand_expert_offsets, moe_gather, moe_scatter, moe_softmax_topk,
                                  moe_topk_softmax, moe_topk_with_indices)
from pygpukit_amd.ops.nn import (fa3_fp8_available, get_sm_version, quantize_fp8_per_head, sdpa_causal_fp8, sdpa_causal_fp8_strided,
                                bias_add_inplace, geglu, gelu, glu_packed, layernorm, lstm_bidirectional, lstm_forward, relu2, rmsnorm, rmsnorm_residual, rope_inplace,
                                rope_inplace_f32table, sdpa_causal, sdpa_causal_fixed_cache, sdpa_causal_fixed_cache_ptr,
                                sdpa_causal_strided, sdpa_noncausal, sdpa_noncausal_strided, sigmoid, silu, slice_rows_range_ptr, split_qkv_batch, swiglu, tanh,
                                embed_token_position_ptr, ln_linear, ln_linear_plan, ln_linear_qkv_cache_ptr, group_norm, group_norm_silu)
from pygpukit_amd.ops.nn import relbias_plan, relpos_bias_table, relpos_bucket, relpos_compute_bias, sdpa_relbias, sdpa_relbias_strided
from pygpukit_amd.ops.plan import BASE_PLAN_OPS, TENSOR_PLAN_OPS, base_op_grid, base_op_plan, tensor_op_grid, tensor_op_plan
from pygpukit_amd.ops.reduction import argmax, argmax_int, argmax_rows, max, mean, min, softmax, sum, sum_axis
from pygpukit_amd.ops.unary import abs, cos, exp, log, neg, relu, rsqrt, sin, sqrt
from pygpukit_amd.ops.paged import (allocate_kv_cache, argmax_sample, check_eos, compute_cumsum, copy_to_paged_cache, gather_embeddings,
                                    paged_attention_v1, prepare_batch_inputs, prepare_position_ids, reshape_and_cache,
                                    scatter_last_token_logits)
from pygpukit_amd.ops.sampling import (sample_greedy, sample_multinomial, sample_token_gpu, sample_topk, sample_topk_to_buf_ptr,
                                       sample_topp, set_sampling_seed)
from pygpukit_amd.ops.tensor import (cast_bf16_to_f32, cast_f16_to_f32, cast_f32_to_bf16, cast_f32_to_f16, concat_axis0,
                                    repeat_interleave_axis1, reshape_copy, transpose_3d_012, transpose_3d_021, transpose_4d_0132,
                                    transpose_4d_0213)
from pygpukit_amd.ops import audio

__all__ = [n for n in dir() if not n.startswith("_")]
