from pygpukit_amd.ops.matmul.fp8 import (fp8_available, fp8_fp8_get_scale_sizes, fp8_fp8_sm120_available, fp8_get_sizes,
                                         fp8_init_lut, gemm_fp8_fp8_blockwise_nt, gemm_fp8_fp8_blockwise_sm120,
                                         gemm_fp8_fp8_get_scale_sizes, gemm_fp8_fp8_sm120, gemm_fp8_fp8_sm120_available,
                                         matmul_fp8, matmul_fp8_fp8_blockwise_sm120, matmul_fp8_fp8_sm120, matmul_fp8_sm120,
                                         quantize_fp8_blocks, quantize_fp8_rows)
from pygpukit_amd.ops.matmul.grouped import (grouped_gemm_bf16, grouped_gemm_fp8_bf16, grouped_gemm_fp8_bf16_sm120,
                                             grouped_gemm_init_lut, grouped_gemm_sorted_splits)
from pygpukit_amd.ops.matmul.gemv import gemv_bf16, gemv_bf16_opt_available, gemv_fp8_bf16, gemv_fp8_bf16_batched
from pygpukit_amd.ops.matmul.nvf4 import (gemm_nvf4_bf16_sm120, gemm_nvf4_bf16_sm120_available, gemv_nvf4_available,
                                          gemv_nvf4_bf16, gemv_nvf4_bf16_sm120, gemv_nvf4_bf16_sm120_available, gemv_nvf4_get_sizes,
                                          matmul_nvf4_bf16_sm120, nvf4_bf16_sm120_available, nvf4_get_sizes, nvf4_nk_get_sizes,
                                          quantize_bf16_to_nvf4, quantize_bf16_to_nvf4_nk, quantize_nvf4_nk)
from pygpukit_amd.ops.matmul.generic import GEMM_PLAN_OPS, batched_matmul, gemm_plan, linear_bias_gelu, matmul, matmul_nt, transpose
from pygpukit_amd.ops.matmul.w8a16 import gemm_w8a16_init_lut, w8a16_gemm, w8a16_gemm_nk, w8a16_gemm_sm120

__all__ = ["matmul", "matmul_nt", "gemm_plan", "GEMM_PLAN_OPS", "transpose", "batched_matmul", "linear_bias_gelu", "gemv_bf16",
           "gemv_bf16_opt_available", "gemv_fp8_bf16", "gemv_fp8_bf16_batched", "w8a16_gemm_sm120", "w8a16_gemm", "w8a16_gemm_nk",
           "gemm_w8a16_init_lut", "matmul_fp8", "matmul_fp8_sm120", "gemm_fp8_fp8_blockwise_nt", "quantize_fp8_rows",
           "quantize_fp8_blocks", "fp8_available", "fp8_init_lut", "matmul_fp8_fp8_sm120", "gemm_fp8_fp8_sm120",
           "matmul_fp8_fp8_blockwise_sm120", "gemm_fp8_fp8_blockwise_sm120", "fp8_fp8_get_scale_sizes",
           "gemm_fp8_fp8_get_scale_sizes", "fp8_get_sizes", "fp8_fp8_sm120_available", "gemm_fp8_fp8_sm120_available",
           "grouped_gemm_init_lut", "grouped_gemm_fp8_bf16", "grouped_gemm_fp8_bf16_sm120", "grouped_gemm_bf16",
           "grouped_gemm_sorted_splits", "nvf4_get_sizes", "nvf4_nk_get_sizes", "quantize_bf16_to_nvf4_nk", "quantize_nvf4_nk", "gemv_nvf4_get_sizes", "quantize_bf16_to_nvf4",
           "matmul_nvf4_bf16_sm120", "gemm_nvf4_bf16_sm120", "gemv_nvf4_bf16", "gemv_nvf4_bf16_sm120", "nvf4_bf16_sm120_available",
           "gemm_nvf4_bf16_sm120_available", "gemv_nvf4_available", "gemv_nvf4_bf16_sm120_available"]
