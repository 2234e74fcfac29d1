"""pygpukit_amd - MI355X (gfx950) native implementation of PyGPUkit's LLM-inference hot path.

Same operator / model surface as the reference package `pygpukit` for that path (GPUArray, ops.*,
llm.CausalTransformerModel and the decode strategies); every op runs a hand-written HIP kernel
through the C ABI of libpgk_hip.so.  There is no CPU backend: importing works anywhere, using it
without the library or without a GPU raises.
"""

__version__ = "0.1.0"

from pygpukit_amd import core, ops  # noqa: F401
from pygpukit_amd.core import (CudaEvent, CudaGraph, DataType, GPUArray, Stream, bfloat16, device_synchronize, empty,  # noqa: F401
                              event_elapsed_ms, event_elapsed_us, float16, float32, float64, from_numpy, get_backend,
                              has_native_module, int4, int8, int16, int32, int64, ones, uint8, zeros)
from pygpukit_amd.core.device import (DeviceCapabilities, DeviceInfo, FallbackDeviceCapabilities, get_device_capabilities,  # noqa: F401,E402
                                      get_device_info, is_cuda_available)
from pygpukit_amd.core.stream import StreamManager, default_stream  # noqa: F401,E402
from pygpukit_amd.ops.basic import (abs, add, argmax, bias_add_inplace, clamp, cos, div, exp, gelu, layernorm,  # noqa: F401,E402,A004
                                    linear_bias_gelu, log, lstm_bidirectional, lstm_forward, matmul, max, mean, min, mul, neg, relu, rsqrt, sigmoid, sin, softmax,
                                    sqrt, sub, sum, sum_axis, tanh, transpose, where)
from pygpukit_amd.jit import (JITKernel, NvrtcError, NvrtcErrorCode, get_nvrtc_path, get_nvrtc_version, is_nvrtc_available,  # noqa: F401,E402
                              jit, warmup)
from pygpukit_amd.ops.nn.attention import (fa3_fp8_available, get_sm_version, sdpa_causal_fp8, sdpa_noncausal,  # noqa: F401,E402
                                          sdpa_noncausal_strided)
from pygpukit_amd.ops.nn.linear import embed_token_position_ptr, ln_linear, ln_linear_plan, ln_linear_qkv_cache_ptr  # noqa: F401,E402
from pygpukit_amd.ops.conv import conv1d, conv2d  # noqa: F401,E402
from pygpukit_amd.ops.nn.norm import group_norm, group_norm_silu  # noqa: F401,E402
from pygpukit_amd.ops.nn.relpos import (relbias_plan, relpos_bias_table, relpos_bucket, relpos_compute_bias, sdpa_relbias,  # noqa: F401,E402
                                        sdpa_relbias_strided)
from pygpukit_amd.ops.nn.window import (kv_cache_update_ring, kv_cache_update_ring_ptr, sdpa_sliding_window,  # noqa: F401,E402
                                        sdpa_sliding_window_fixed_cache, sdpa_sliding_window_fixed_cache_ptr, sdpa_sliding_window_strided,
                                        sdpa_window_plan)
from pygpukit_amd.ops.matmul.int8 import (gemm_int4_int8_sm120, gemm_int4_int32_available, gemm_int4_int32_sm120,  # noqa: F401,E402
                                          gemm_int8_int32_available, gemm_int8_int32_sm120, int4_gemm_available, int4_gemm_int8_sm120,
                                          int4_gemm_int32_sm120, int4_gemv_available, int4_gemv_int32_sm120, int8_native_gemm_available,
                                          int8_native_gemm_sm120, int_gemm_plan, matmul_int8_dequant)
from pygpukit_amd.ops.paged import paged_attention_prefill, paged_prefill_plan  # noqa: F401,E402
from pygpukit_amd.ops.paged import (copy_to_paged_cache_fp8, paged_attention_prefill_fp8, paged_attention_v1_fp8, paged_kv_fp8_plan,  # noqa: F401,E402
                                    reshape_and_cache_fp8)
from pygpukit_amd.ops.quantize import dequantize_int8, linear_int8, quantize_to_int8  # noqa: F401,E402
from pygpukit_amd.ops.nn.kvfp8 import (kv_cache_prefill_gqa_fp8, kv_cache_update_gqa_fp8, kv_cache_update_gqa_fp8_ptr, kv_fp8_scales, sdpa_causal_fixed_cache_fp8,  # noqa: F401,E402
                                       sdpa_causal_fixed_cache_fp8_ptr, sdpa_kv_fp8_plan)
from pygpukit_amd.ops.nn.mla import mla_cache_write, mla_cache_write_ptr, sdpa_mla_fixed_cache, sdpa_mla_fixed_cache_ptr, sdpa_mla_plan, sdpa_mla_prefill, sdpa_mla_prefill_plan, allocate_mla_cache, mla_reshape_and_cache, sdpa_mla_paged, sdpa_mla_paged_plan  # noqa: F401,E402
