/*
 * pgk_hip.h - C ABI of libpgk_hip.so, the MI355X (gfx950) native backend for the
 * PyGPUkit LLM-inference hot path.
 *
 * This is the drop-in boundary.  In the reference the same boundary is the pybind11
 * module `_pygpukit_native` (native/bindings/module.cpp:10-21) over the C++ operator
 * API native/ops/ops.cuh; here it is a plain C ABI (no C++ types, no exceptions, no
 * torch types) bound from Python with ctypes (pygpukit_amd/_hip.py).  Every entry
 * point names the reference interface it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - every function returns pgk_status (0 = OK); pgk_last_error() gives the message
 *     for the calling thread (reference: C++ exceptions -> Python RuntimeError,
 *     native/core/types.hpp:108-111).
 *   - pointers are DEVICE pointers unless the parameter name starts with `h_`.
 *   - arrays are dense, row-major, C-contiguous (reference: core/array.py:197-215).
 *   - `dt` is the element type of the floating operands (PGK_F32 / PGK_F16 / PGK_BF16);
 *     bf16 travels as raw 16-bit words (reference: core/dtypes.py:54).
 *   - `stream` may be NULL = the calling thread's current stream
 *     (pgk_stream_set_current; default: one library-owned stream per device).  Ops
 *     never synchronise; only D2H copies, pgk_stream_sync and pgk_device_sync do.
 *     (The reference syncs after every op, native/ops/common/error.cuh:28-37.)
 *   - ops never allocate; callers pass outputs and workspaces.  Safe to capture.
 */
#ifndef PGK_HIP_H
#define PGK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int pgk_status;
#define PGK_OK 0
#define PGK_ERR_INVALID 1   /* bad shape / dtype / argument (reference: std::runtime_error) */
#define PGK_ERR_HIP 2       /* HIP runtime failure (reference: CudaError) */
#define PGK_ERR_UNSUPPORTED 3
#define PGK_ERR_RCCL 4
#define PGK_ERR_JIT 5        /* runtime compilation / module load / launch of a user kernel (reference: NvrtcError) */

/* Same order as the reference's DataType enum (native/bindings/core_bindings.cpp:19-30). */
typedef enum {
    PGK_F64 = 0, PGK_F32 = 1, PGK_F16 = 2, PGK_BF16 = 3, PGK_I64 = 4,
    PGK_I32 = 5, PGK_I16 = 6, PGK_I8 = 7, PGK_U8 = 8, PGK_I4 = 9
} pgk_dtype;

typedef void* pgk_stream;
typedef void* pgk_event;
typedef void* pgk_graph;
typedef void* pgk_comm;
typedef void* pgk_engine;

/* ---------------------------------------------------------------- errors / device -- */
const char* pgk_last_error(void);
const char* pgk_version(void);
/* native/bindings/core_bindings.cpp:52-57 (get_device_count, set_device, get_current_device,
 * device_synchronize, get_device_properties) */
pgk_status pgk_device_count(int* n);
pgk_status pgk_device_set(int dev);
pgk_status pgk_device_get(int* dev);
pgk_status pgk_device_sync(void);
typedef struct {
    char name[128];
    char arch[32];
    size_t total_mem;
    int cu_count;
    int wavefront_size;
    int clock_khz;
    int lds_per_cu;
    int l2_bytes;
} pgk_device_props_t;
pgk_status pgk_device_props(int dev, pgk_device_props_t* out);
/* The current device's gfx target as a number: the decimal digits after "gfx" in its architecture name (950 on
 * MI355X).  Stands where the reference reports an SM version. */
pgk_status pgk_device_arch(int* gfx);
pgk_status pgk_mem_info(size_t* free_bytes, size_t* total_bytes);

/* ---------------------------------------------------------------------- memory ------ */
/* Pooled device allocator.  Replaces per-array cuMemAlloc/cuMemFree
 * (native/core/memory.cpp:127-133) and the size-class pool of rust/pygpukit-core
 * (memory/pool.rs:106-422): power-of-two-ish size classes, cached free lists, no
 * hipMalloc on a pool hit (so allocation is legal while a stream is capturing). */
pgk_status pgk_malloc(void** ptr, size_t nbytes);
pgk_status pgk_free(void* ptr);
typedef struct {
    size_t bytes_in_use, bytes_cached, bytes_reserved_peak;
    uint64_t n_alloc, n_pool_hit, n_device_malloc, n_free;
} pgk_pool_stats_t;
pgk_status pgk_pool_stats(pgk_pool_stats_t* out);
pgk_status pgk_pool_trim(void);               /* return cached blocks to the driver */
pgk_status pgk_host_alloc(void** h_ptr, size_t nbytes);   /* pinned host memory */
pgk_status pgk_host_free(void* h_ptr);
/* GPUArray::copy_from_host / copy_to_host / fill_zeros (native/core/memory.hpp:87-91) and
 * memcpy_device_to_device_async (core_bindings.cpp:317).  h2d/d2h return after the copy
 * has completed (ordered after prior work on `stream`); *_async need pinned host memory. */
pgk_status pgk_memcpy_h2d(void* dst, const void* h_src, size_t nbytes, pgk_stream stream);
pgk_status pgk_memcpy_d2h(void* h_dst, const void* src, size_t nbytes, pgk_stream stream);
pgk_status pgk_memcpy_h2d_async(void* dst, const void* h_src, size_t nbytes, pgk_stream stream);
pgk_status pgk_memcpy_d2h_async(void* h_dst, const void* src, size_t nbytes, pgk_stream stream);
pgk_status pgk_memcpy_d2d(void* dst, const void* src, size_t nbytes, pgk_stream stream);
pgk_status pgk_memset(void* dst, int value, size_t nbytes, pgk_stream stream);
pgk_status pgk_fill(void* dst, double value, size_t n, pgk_dtype dt, pgk_stream stream); /* ones() */

/* ------------------------------------------------------- streams / events / graphs -- */
/* Stream(priority) native/core/stream.hpp:21-35 */
pgk_status pgk_stream_create(pgk_stream* out, int high_priority);
pgk_status pgk_stream_destroy(pgk_stream s);
pgk_status pgk_stream_sync(pgk_stream s);
pgk_status pgk_stream_set_current(pgk_stream s);     /* NULL restores the default stream */
pgk_status pgk_stream_get_current(pgk_stream* out);
/* CudaEvent native/core/event.hpp:13-38, event_elapsed_ms core_bindings.cpp:259 */
pgk_status pgk_event_create(pgk_event* out);
pgk_status pgk_event_destroy(pgk_event e);
pgk_status pgk_event_record(pgk_event e, pgk_stream s);
pgk_status pgk_event_sync(pgk_event e);
/* cudaStreamWaitEvent: work queued on `s` (NULL: the current stream) after this call runs after `e` */
pgk_status pgk_stream_wait_event(pgk_stream s, pgk_event e);
pgk_status pgk_event_query(pgk_event e, int* done);
pgk_status pgk_event_elapsed_ms(pgk_event start, pgk_event stop, float* ms);
/* CudaGraph native/core/cuda_graph.hpp:31-88: begin_capture / end_capture / replay /
 * synchronize / reset / is_ready / num_nodes.  Capture is on `stream` (thread-local
 * capture in the reference, cuda_graph.cu:84-107).  Pool blocks allocated by the capturing thread between begin and end
 * are baked into the graph: freeing one only parks it until pgk_graph_destroy, so replays never find them recycled. */
pgk_status pgk_graph_begin_capture(pgk_stream s);
pgk_status pgk_graph_end_capture(pgk_stream s, pgk_graph* out);
pgk_status pgk_graph_launch(pgk_graph g, pgk_stream s);
pgk_status pgk_graph_num_nodes(pgk_graph g, size_t* n);
pgk_status pgk_graph_destroy(pgk_graph g);
pgk_status pgk_stream_is_capturing(pgk_stream s, int* yes);

/* ------------------------------------------------------------------ elementwise ----- */
/* ops.cuh:24-37 add/mul/sub/div (out-of-place, same shape); op: 0 add, 1 sub, 2 mul, 3 div */
pgk_status pgk_binary(const void* a, const void* b, void* c, size_t n, int op, pgk_dtype dt, pgk_stream s);
/* ops.cuh:413,416 add_inplace / mul_inplace: a (op)= b */
pgk_status pgk_binary_inplace(void* a, const void* b, size_t n, int op, pgk_dtype dt, pgk_stream s);
/* ops.cuh:139 bias_add_inplace: out[rows,features] += bias[features] */
pgk_status pgk_bias_add_inplace(void* out, const void* bias, int rows, int features, pgk_dtype dt, pgk_stream s);
/* ops.cuh:136 gelu (tanh form 0.7978845608/0.044715), :176-179 silu; act: 0 silu, 1 gelu, 2 sigmoid, 3 tanh, 4 relu2,
 * 14 quick_gelu = x * sigmoid(1.702 x) [build-defined: CLIP's hidden_act] */
pgk_status pgk_activation(const void* x, void* y, size_t n, int act, pgk_dtype dt, pgk_stream s);
/* ... and the unary family of ops.cuh:60-101 (src/pygpukit/ops/unary.py:16-260) through the same entry:
 * act 5 exp, 6 log, 7 relu, 8 sin, 9 cos, 10 sqrt, 11 rsqrt, 12 abs, 13 neg */
/* ops.cuh:92-131 (src/pygpukit/ops/reduction.py:16-130,227): whole-array reduction to one element of the input dtype;
 * op: 0 sum, 1 mean, 2 max, 3 min.  Fixed two-level tree in fp32: the same bits on every run. */
pgk_status pgk_reduce(const void* x, void* out, size_t n, int op, pgk_dtype dt, pgk_stream s);
/* reduction.py:133-224 softmax over the last axis of [rows, n] (max-subtracted, fp32 math) */
pgk_status pgk_softmax_rows(const void* x, void* y, int rows, int n, pgk_dtype dt, pgk_stream s);
/* reduction.py:271-300 sum_axis of a 2-D [m, n]: axis 0 -> out[n], axis 1 -> out[m] */
pgk_status pgk_sum_axis(const void* x, void* out, int m, int n, int axis, pgk_dtype dt, pgk_stream s);
/* ops/elementwise.py:254-276 clamp to [lo, hi]; :279-308 where(cond != 0 ? a : b), cond one byte per element */
pgk_status pgk_clamp(const void* x, void* y, size_t n, float lo, float hi, pgk_dtype dt, pgk_stream s);
pgk_status pgk_where(const uint8_t* cond, const void* a, const void* b, void* y, size_t n, pgk_dtype dt, pgk_stream s);
/* int32 -> int64 (the reference's ops.argmax returns an int64 [1] array, reduction.py:249-268) */
pgk_status pgk_widen_i32_i64(const int32_t* src, int64_t* dst, size_t n, pgk_stream s);
/* ops.cuh:206-212 swiglu / geglu: out = act(gate) * up ; act: 0 silu, 1 gelu */
pgk_status pgk_glu(const void* gate, const void* up, void* out, size_t n, int act, pgk_dtype dt, pgk_stream s);
/* Row-packed GLU: gate_up[rows, 2*inter] (gate columns then up columns, the fused gate_up projection of
 * src/pygpukit/llm/layers/mlp.py:84-86) -> out[rows, inter] = act(gate) * up.  Replaces the reference's
 * narrow + silu + mul_inplace sequence (models/causal.py:537-549), which is only exact for rows == 1. */
pgk_status pgk_glu_packed(const void* gate_up, void* out, int rows, int inter, int act, pgk_dtype dt, pgk_stream s);
/* ops.cuh:426-436 cast_f32_to_bf16 / f32_to_f16 / bf16_to_f32 / f16_to_f32 (RNE) */
pgk_status pgk_cast(const void* src, pgk_dtype src_dt, void* dst, pgk_dtype dst_dt, size_t n, pgk_stream s);

/* Host-only queries of the base op dispatch (csrc/base_plan.h; DESIGN.md "Base op dispatch leaves"): the kernel branch a call
 * takes and the number of blocks it launches, from the functions the launchers themselves call.  op: "binary", "activation",
 * "glu", "cast", "clamp", "where", "reduce" (n_or_rows = elements, features ignored), "glu_packed" (rows, inter), "bias_add",
 * "rmsnorm", "rmsnorm_residual", "layernorm" (rows, features), "rope" (seq * (Hq + Hk), D).  aligned: every pointer the
 * launcher tests is on a 16-byte boundary.  Leaves: ew_vec / ew_scalar, row_vec / row_scalar, norm_wave / norm_block,
 * cast_x4, rope_pairs, ew_stride, reduce_tree (the first level of pgk_reduce).  NULL / -1 and pgk_last_error for a call the entry point rejects.  No device is touched. */
const char* pgk_base_op_plan(const char* op, size_t rows, int features, pgk_dtype dt, int aligned);
int pgk_base_op_grid(const char* op, size_t n_or_rows, int features, pgk_dtype dt, int aligned);

/* Host-only queries of the byte movers' dispatch (csrc/tensor_plan.h; DESIGN.md "Byte-mover dispatch leaves"): the kernel
 * instantiation a call takes and the number of blocks it launches, from the functions the launchers themselves call.  The work
 * is batch * rows rows of row_bytes bytes.  op: "transpose_2d" (batch 1) / "transpose_batched" (batch <= 65535): matrices of
 * rows x row_bytes / itemsize -> "tile64"; "transpose_3d_021", "repeat_interleave", "slice_rows", "kv_cache_write" (seq * cache
 * heads rows), "embedding_lookup", "scatter_last_logits": output rows -> "vec16" .. "vec1"; "split_qkv": rows of q + k + v bytes,
 * low_bits also carrying q_bytes | k_bytes | v_bytes; "paged_cache_write": tokens * kv heads rows, whole 16-byte chunks ->
 * "vec16"; "argmax": rows of row_bytes / itemsize elements -> "block256" / "block1024".  low_bits: the OR of the addresses the
 * launcher tests (the low four bits count).  NULL / -1 and pgk_last_error for a call the entry point rejects, and for an empty one,
 * which launches nothing.  No device is touched. */
const char* pgk_tensor_op_plan(const char* op, size_t batch, size_t rows, size_t row_bytes, int itemsize, unsigned low_bits);
int pgk_tensor_op_grid(const char* op, size_t batch, size_t rows, size_t row_bytes, int itemsize, unsigned low_bits);

/* ------------------------------------------------------------------------ norms ----- */
/* ops.cuh:152-155 rmsnorm(input[rows,features], gamma[features]) -> out (may alias input) */
pgk_status pgk_rmsnorm(const void* x, const void* gamma, void* out, int rows, int features, float eps,
                       pgk_dtype dt, pgk_stream s);
/* ops.cuh:199-201 rmsnorm_residual: out = rmsnorm(x + residual) * gamma */
pgk_status pgk_rmsnorm_residual(const void* x, const void* residual, const void* gamma, void* out, int rows,
                                int features, float eps, pgk_dtype dt, pgk_stream s);
/* ops.cuh:143 layernorm (population variance) */
pgk_status pgk_layernorm(const void* x, const void* gamma, const void* beta, void* out, int rows, int features,
                         float eps, pgk_dtype dt, pgk_stream s);

/* ------------------------------------------------------------------------- rope ----- */
/* ops.cuh:218 rope_inplace (table in dt) and :224 rope_inplace_f32table (fp32 table):
 * q[S,Hq,D], k[S,Hk,D], cos/sin[S,D]; rotate-half, table column d < D/2. */
pgk_status pgk_rope_inplace(void* q, void* k, const void* cos, const void* sin, int seq, int hq, int hk, int d,
                            pgk_dtype dt, int f32_table, pgk_stream s);

/* ------------------------------------------------------------- layout shuffles ------ */
/* ops.cuh:132 transpose (2-D) */
pgk_status pgk_transpose_2d(const void* in, void* out, int rows, int cols, int itemsize, pgk_stream s);
/* ops.cuh:352-354 transpose_3d_021: [d0,d1,d2] -> [d1,d0,d2] */
pgk_status pgk_transpose_3d_021(const void* in, void* out, int d0, int d1, int d2, int itemsize, pgk_stream s);
/* src/pygpukit/ops/tensor.py:256-318 transpose_3d_012 ([d0,d1,d2] -> [d0,d2,d1]) and :320-380 transpose_4d_0132
 * ([d0,d1,d2,d3] -> [d0,d1,d3,d2]): `batch` independent [rows, cols] matrices, each transposed */
pgk_status pgk_transpose_batched(const void* in, void* out, int batch, int rows, int cols, int itemsize, pgk_stream s);
/* tensor.py:191-254 transpose_4d_0213: [d0,d1,d2,d3] -> [d0,d2,d1,d3] */
pgk_status pgk_transpose_4d_0213(const void* in, void* out, int d0, int d1, int d2, int d3, int itemsize, pgk_stream s);
/* ops.cuh:349 repeat_interleave_axis1: [d0,d1,d2] -> [d0,d1*r,d2] */
pgk_status pgk_repeat_interleave_axis1(const void* in, void* out, int d0, int d1, int d2, int repeats,
                                       int itemsize, pgk_stream s);
/* ops.cuh:271 split_qkv_batch: qkv[rows,q+k+v] -> q[rows,q], k[rows,k], v[rows,v] */
pgk_status pgk_split_qkv_batch(const void* qkv, void* q, void* k, void* v, int rows, int q_dim, int k_dim,
                               int v_dim, int itemsize, pgk_stream s);
/* (concat_axis0 ops.cuh:345, reshape_copy :375-377, copy_to :419 are pgk_memcpy_d2d.) */

/* ------------------------------------------------------ embedding / KV cache -------- */
/* ops.cuh:403-405 embedding_lookup / _ptr / _batch: out[i,:] = table[ids[i],:].
 * `ids` is a device int32 array when ids_on_device, else h_id is used for row 0. */
pgk_status pgk_embedding_lookup(const void* table, void* out, int hidden, int itemsize, int h_id,
                                const int32_t* ids, int n_ids, pgk_stream s);
/* ops.cuh:410 slice_rows_range_ptr: out[0:count,:] = table[start:start+count,:], start from device int32 */
pgk_status pgk_slice_rows_range_ptr(const void* table, void* out, const int32_t* start_buf, int count, int row_elems,
                                    int itemsize, pgk_stream s);
/* ops.cuh:397-399 kv_cache_update_gqa / _ptr / kv_cache_prefill_gqa: scatter new_kv[S,Hkv,D]
 * into cache[Hc,max_seq,D] rows pos..pos+S-1; cache head h reads kv head h/(Hc/Hkv).  Hc == Hq is
 * the reference's GQA-expanded layout; Hc == Hkv the un-expanded MI355X layout.  pos_buf (device
 * int32) overrides h_pos when non-NULL (graph replay). */
pgk_status pgk_kv_cache_write(const void* new_kv, void* cache, int seq, int hkv, int hc, int max_seq, int d,
                              int itemsize, int h_pos, const int32_t* pos_buf, pgk_stream s);

/* -------------------------------------------------------------------- sampling ------ */
/* ops.cuh:104 argmax, :572 sample_greedy: index of the max over n elements of each of `rows`
 * rows; ties resolve to the LOWEST index (np.argmax; src/pygpukit/llm/sampling.py:60-61).
 * out_idx: device int32[rows]. */
pgk_status pgk_argmax(const void* x, int rows, int n, pgk_dtype dt, int32_t* out_idx, pgk_stream s);

/* sample_multinomial / sample_topk / sample_topp / sample_topk_to_buf_ptr (src/pygpukit/ops/sampling.py:11-141,
 * native/ops/sampling/sampling.cu): one token per logits row, temperature > 0, top_k = 0 disables top-k,
 * top_p = 1 disables the nucleus; the uniform random number comes from `u` or, when `u_buf` is non-NULL, from device
 * memory (graph-replay compatible).  Deterministic function of its inputs, defined in csrc/ops_sampling.hip and
 * restated by oracle/cpu_ref.py sample_token_u.  Result: int32 per row in device memory. */
pgk_status pgk_sample_token(const void* logits, int rows, int vocab, pgk_dtype dt, float temperature, int top_k,
                            float top_p, float u, const float* u_buf, int32_t* out_tokens, pgk_stream s);

/* ------------------------------------------------------------------ safetensors reader ------ */
/* SafeTensorsFile (src/pygpukit/llm/safetensors.py:122-235 over rust/pygpukit-core/src/llm/tensor_loader.rs): the file
 * is mmap'ed read-only and its JSON header parsed once.  dtype ids are safetensors.py:28-43 (0 F32, 1 F16, 2 BF16, 3 F64,
 * 4 F8_E4M3, 5 F8_E5M2, 6 I32, 7 I64, 8 I16, 9 I8, 10 U8, 11 BOOL); `offset` is from the start of the file. */
pgk_status pgk_st_open(const char* path, void** handle);
void pgk_st_close(void* handle);
int pgk_st_num_tensors(void* handle);
uint64_t pgk_st_file_size(void* handle);
const char* pgk_st_tensor_name(void* handle, int i);
pgk_status pgk_st_tensor_info(void* handle, const char* name, int* dtype, int* ndim, int64_t* shape8, uint64_t* offset,
                              uint64_t* nbytes);
pgk_status pgk_st_tensor_data(void* handle, const char* name, const void** ptr, uint64_t* nbytes);
/* mapped file -> device without a host copy (loader.py:160-175 memcpy_ptr_to_device) */
pgk_status pgk_st_upload(void* handle, const char* name, void* dst_device, uint64_t dst_bytes, pgk_stream s);

/* ----------------------------------------------------------------- runtime compilation ------ */
/* native/jit/compiler.hpp + kernel.hpp (bound in native/bindings/jit_bindings.cpp:65-122): NVRTC -> PTX ->
 * cuModuleLoadData -> cuLaunchKernel becomes hiprtc -> gfx950 code object -> hipModuleLoadData ->
 * hipModuleLaunchKernel.  libhiprtc is dlopen'ed on first use (is_nvrtc_available's contract).  `rtc_code` outputs
 * are hiprtcResult values (numerically nvrtcResult's) or 1000 NotLoaded / 1001 load failed / 1002 function not found /
 * 1003 launch failed, as in src/pygpukit/jit/compiler.py:20-43. */
int pgk_jit_available(void);
const char* pgk_jit_library_path(void);
pgk_status pgk_jit_version(int* major, int* minor);
/* compile_to_ptx: NVRTC arch flags in `options` are dropped, --offload-arch=gfx950 is supplied; a program handle is
 * returned even on a compilation error so that its log can be read. */
pgk_status pgk_jit_compile(const char* source, const char* name, const char* const* options, int n_options,
                           void** program_out, int* rtc_code);
const char* pgk_jit_program_log(void* program);
pgk_status pgk_jit_program_code(void* program, const void** code, size_t* size);
void pgk_jit_program_destroy(void* program);
/* JITKernel: module + function handle for one extern "C" __global__ function of a compiled program */
pgk_status pgk_jit_kernel_create(void* program, const char* func_name, void** kernel_out, int* rtc_code);
void pgk_jit_kernel_destroy(void* kernel);
pgk_status pgk_jit_suggested_block_size(void* kernel, size_t dynamic_smem, int* block_size);
/* args[i] points at the value of kernel argument i (cuLaunchKernel's kernelParams convention) */
pgk_status pgk_jit_launch(void* kernel, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned by, unsigned bz,
                          unsigned shared_bytes, void** args, pgk_stream s);

/* ------------------------------------------------- paged KV cache / continuous batching ------ */
/* ops.cuh:466-478 paged_attention_v1 (native/ops/attention/paged_attention.cuh:46-200): single-query attention over a
 * paged cache.  Q/out [num_seqs, Hq, D]; K/V cache [num_blocks, Hkv, block_size, D]; block_tables [num_seqs,
 * max_blocks_per_seq] int32; context_lens [num_seqs] int32 (device).  scale <= 0 -> 1/sqrt(D).  max_context bounds the
 * context lengths (it sizes the KV split); contexts beyond 512 need `workspace` of
 * pgk_paged_attention_workspace_bytes bytes.  dt = PGK_BF16 / PGK_F16 (the reference is f16-only). */
size_t pgk_paged_attention_workspace_bytes(int num_seqs, int num_heads, int head_dim, int max_context);
pgk_status pgk_paged_attention_v1(const void* q, const void* k_cache, const void* v_cache, const int32_t* block_tables,
                                  const int32_t* context_lens, void* out, int num_seqs, int num_heads, int num_kv_heads,
                                  int head_dim, int block_size, int max_blocks_per_seq, int max_context, float scale,
                                  void* workspace, pgk_dtype dt, pgk_stream s);
/* ops.cuh:480-502 copy_to_paged_cache / reshape_and_cache (paged_attention.cuh:206-283): K_new/V_new
 * [n_tokens, Hkv, D] rows scattered to slot_mapping[token] = physical_block * block_size + offset (negative: skip). */
pgk_status pgk_paged_cache_write(const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                 const int32_t* slot_mapping, int n_tokens, int num_kv_heads, int block_size, int head_dim,
                                 int itemsize, pgk_stream s);
/* ops.cuh:520-528 scatter_last_token_logits (continuous_batching.cuh:103-133): out[b] = logits[seq_start[b] + seq_lens[b] - 1];
 * any vocabulary and alignment: 16-, 8-, 4-, 2- or 1-byte vectors by the row's byte size and the two addresses (tensor_plan.h) */
pgk_status pgk_scatter_last_token_logits(const void* logits, void* out, const int32_t* seq_start, const int32_t* seq_lens,
                                         int batch, int vocab, int itemsize, pgk_stream s);
/* ops.cuh:530-539 prepare_position_ids (continuous_batching.cuh:139-165) */
pgk_status pgk_prepare_position_ids(const int32_t* seq_start, const int32_t* seq_ctx, const int32_t* is_prefill,
                                    const int32_t* input_lens, int32_t* position_ids, int batch, pgk_stream s);
/* ops.cuh:550-553 check_eos (continuous_batching.cuh:231-241), :555-556 compute_cumsum (exclusive) */
pgk_status pgk_check_eos(const int32_t* tokens, int32_t* finished, int n, int eos_token_id, pgk_stream s);
pgk_status pgk_exclusive_cumsum_i32(const int32_t* in, int32_t* out, int n, pgk_stream s);

/* ---------------------------------------------------------------------- matmul ------ */
/* ops.cuh:119-124 matmul: C[M,N] = A[M,K] B[K,N]  (row-major, fp32 accumulate, dt out). */
pgk_status pgk_gemm_nn(const void* a, const void* b, void* c, int m, int n, int k, pgk_dtype dt, pgk_stream s);
/* LinearBF16 (src/pygpukit/llm/layers/linear.py:46-99): C[M,N] = A[M,K] W[N,K]^T (+bias[N]) on the
 * PyTorch-layout weight directly - no transposed copy of W is ever made (the reference keeps W and W^T). */
pgk_status pgk_gemm_nt(const void* a, const void* w, const void* bias, void* c, int m, int n, int k,
                       pgk_dtype dt, pgk_stream s);
/* pygpukit_gemv_bf16_opt_sm120 (native/ops/matmul/gemv/bf16_bf16/sm120/bf16_opt.cu:36-47):
 * C[N] = A[K] . B[N,K]^T.  dt = PGK_BF16 / PGK_F16 / PGK_F32 (all fp32 accumulate). */
pgk_status pgk_gemv(const void* a, const void* b_nk, void* c, int k, int n, pgk_dtype dt, pgk_stream s);
/* gemv_fp8_bf16_sm120 / _batched (native/ops/matmul/gemv/w8a16_bf16/sm120/fp8_opt_kernels.cu:27-64):
 * C[M,N] = A[M,K] . (E4M3[B[N,K]] * scale[N/128,K/128])^T ; A, scale, C bf16; M >= 1. */
pgk_status pgk_gemv_fp8_bf16(const void* a, const uint8_t* b_nk, const void* scale, void* c, int m, int k, int n,
                             pgk_stream s);
/* pygpukit_w8a16_gemm_sm120 (native/bindings/gemm/fp8xbf16_bf16.cpp:9-12):
 * C[M,N] = A[M,K] . dequant(B_fp8[K,N], scale[K/128,N/128]) ; note the [K,N] layout. */
pgk_status pgk_w8a16_gemm_kn(const void* a, const uint8_t* b_kn, const void* scale, void* c, int m, int n, int k,
                             pgk_stream s);
/* Same product on the PyTorch-layout weight W_fp8[N,K] with scale[N/128,K/128] (the layout LinearFP8 stores,
 * src/pygpukit/llm/layers/linear.py:149-160): avoids the transposed fp8 + scale copies the reference
 * makes for its M > 1 path (linear.py:173-179). */
pgk_status pgk_w8a16_gemm_nk(const void* a, const uint8_t* w_nk, const void* scale, void* c, int m, int n, int k,
                             pgk_stream s);
/* gemm_fp8_fp8_blockwise_sm120 (src/pygpukit/ops/matmul/fp8.py:288-343; its native side is CUTLASS and absent
 * from the checkout): fp8 x fp8 MFMA GEMM with 128-wide block scales,
 *   C[m][n] = sum_kb a_scale[m][kb] * w_scale[n/128][kb] * sum_{k in kb} E4M3(a[m][k]) * E4M3(w[n][k]).
 * a_fp8 [M,K] codes with a_scale [M, K/128] fp32 (one scale per row per 128 k); w_fp8_nk [N,K] codes with
 * w_scale [ceil(N/128), K/128] bf16 (the LinearFP8 layout, linear.py:149-160); C bf16 [M,N].  K % 128 == 0. */
pgk_status pgk_gemm_fp8_nt(const uint8_t* a_fp8, const float* a_scale, const uint8_t* w_fp8_nk, const void* w_scale,
                           void* c, int m, int n, int k, pgk_stream s);
/* [build-defined] The kernel that a call of the dense GEMM family takes, decided on the host (needs no device):
 * op = "nt" (pgk_gemm_nt), "nn" (pgk_gemm_nn), "w8a16_nk", "w8a16_kn", "gemv_fp8" (pgk_gemv_fp8_bf16) or "fp8_nt"
 * (pgk_gemm_fp8_nt); aligned = every operand on a 16-byte boundary.  Reads PGK_GEMM256 / PGK_GEMM256S per call, as the
 * dispatchers do, and is built from the decision functions they switch on (csrc/gemm_plan.h).  Returns a leaf name
 * ("GEMM dispatch leaves") in a thread-local buffer that the next call on the thread overwrites, or NULL
 * with pgk_last_error set for an op, dtype or shape that the entry point rejects. */
const char* pgk_gemm_plan(const char* op, int m, int n, int k, pgk_dtype dt, int aligned);
/* gemm_fp8_fp8_sm120 / gemm_fp8_fp8_blockwise_sm120 (src/pygpukit/ops/matmul/fp8.py:220-343, bindings
 * native/bindings/gemm/fp8xfp8_fp8.cpp): fp8 in, fp8 out,
 *   D[m][n] = E4M3( sum_kb scale_a[mb,kb] * scale_b[nb,kb] * sum_{k in kb} E4M3(a[m][k]) * E4M3(b[k][n]) ),
 * mb = m/128, nb = n/128, kb = k/128.  a_mk [M,K], b_kn [K,N], d_mn [M,N]: e4m3 codes, row-major as the shapes say
 * (the reference hands its [K,N] buffer to CUTLASS as column-major, i.e. N x K bytes; this entry follows the
 * declared shape, like pgk_w8a16_gemm_kn).  Output: RNE with satfinite (|x| > 448 -> +-448), NaN stays NaN.
 * scale_a / scale_b fp32, ceil(M/128)*ceil(K/128) and ceil(N/128)*ceil(K/128) elements, MN-major: (mb, kb) at
 * kb*ceil(M/128) + mb, (nb, kb) at kb*ceil(N/128) + nb.  That layout is the default of CUTLASS's
 * Sm1xxBlockwiseScaleConfig (fp8_cutlass.cu:84-86,261-268), taken from CUTLASS's defaults, not pinned by a
 * reference run.  Both scales NULL = unit scales; exactly one NULL is an error.
 * M >= 1; N, K multiples of 16 (K need not be a multiple of 128); operands 16-byte aligned. */
pgk_status pgk_gemm_fp8_fp8_nn(const uint8_t* a_mk, const uint8_t* b_kn, uint8_t* d_mn, const float* scale_a,
                               const float* scale_b, int m, int n, int k, pgk_stream s);
/* Activation quantiser for pgk_gemm_fp8_nt (the fp32-in "auto-quantise" half of matmul_fp8, fp8.py:20-83):
 * per (row, 128-k block) scale = absmax/448 (1 for an all-zero block), codes = RNE e4m3 of x/scale.
 * dt = PGK_BF16 / PGK_F16 / PGK_F32. */
pgk_status pgk_quantize_fp8_rows(const void* x, uint8_t* out_fp8, float* out_scale, int m, int k, pgk_dtype dt,
                                 pgk_stream s);
/* Weight quantiser: per 128x128 block scale = bf16(absmax/448), codes = RNE e4m3 of w/scale - the LinearFP8
 * storage format (loader.py:228-252 reads it from checkpoints; this builds it from bf16 weights on device). */
pgk_status pgk_quantize_fp8_blocks(const void* w_bf16, uint8_t* out_fp8, void* out_scale_bf16, int n, int k,
                                   pgk_stream s);

/* ----------------------------------------------------------------------- NVF4 ------ */
/* NVF4 (native/ops/matmul/gemv/w4a16_bf16/sm120/nvf4.cuh:36-110): a 4-bit code c has sign bit 3 and magnitude
 * {0, .5, 1, 1.5, 2, 3, 4, 6}[c & 7]; a byte holds k (even) in its low nibble, k+1 in its high nibble.  Weights:
 * data [K/2, N] (byte (k/2)*N + n), scale [ceil(K/32), N] (byte (k/32)*N + n) with a scale byte s worth
 * (1 + (s&7)/8) * 2^(((s>>3)&15) - 7); bit 7 is ignored. */
/* quantize_bf16_to_nvf4 (nvf4_kernels.cu:239-320): x_kn bf16 [K,N] -> data + scale, per (column, 32-row block):
 * scale = max|x|/6 (1 when max|x| <= 1e-8), encoded as above (exponent and mantissa clamped, never rounded up
 * past mantissa 7), codes = the threshold chain 0.25 .. 5.0 of x * (1 / decoded scale), ties away from zero,
 * NaN -> +6.  K even (the reference writes past the data for odd K). */
pgk_status pgk_quantize_nvf4(const void* x_kn, uint8_t* data, uint8_t* scale, int k, int n, pgk_stream s);
/* The engine's NK layout of the same format (this project's, not the reference's): x_nk bf16 [N,K] -> data [N, K/2]
 * (byte j of row n holds k = 2j in its low nibble, 2j+1 in its high nibble) and scale [N, K/32].  Its bytes are the
 * transpose of pgk_quantize_nvf4 on x_nk^T (same arithmetic per 32-k block).  K % 32 == 0; x_nk and data 16-byte aligned. */
pgk_status pgk_quantize_nvf4_nk(const void* x_nk, uint8_t* data, uint8_t* scale, int n, int k, pgk_stream s);
/* gemv_nvf4_bf16_sm120 (nvf4_kernels.cu:19-235): C[n] = bf16(alpha * sum_k a[k] * e2m1(k,n) * scale(k/32,n)),
 * fp32 accumulation in a fixed order (no atomics).  a bf16 [K], C bf16 [N]; K even, any K % 32.  workspace:
 * pgk_gemv_nvf4_workspace_bytes(k, n) bytes (0: may be NULL) for the partial sums of a K split. */
size_t pgk_gemv_nvf4_workspace_bytes(int k, int n);
pgk_status pgk_gemv_nvf4_bf16(const void* a, const uint8_t* data, const uint8_t* scale, void* c, void* workspace, int k,
                              int n, float alpha, pgk_stream s);
/* The operand packer of gemm_nvf4_bf16_sm120 (nvf4_cutlass.cu:157-317): unit-scale e2m1 of bf16 (thresholds
 * 0.25 .. 5.0 on |x|, ties away from zero, NaN -> +0, +-inf -> +-6) packed K-contiguous into out [rows, Kp/2],
 * Kp = k rounded up to a multiple of 128, zero nibbles past k.  transpose = 0: x is [rows, k] (A); transpose = 1:
 * x is [k, rows] (B [K,N], rows = N).  k % 32 == 0; out 16-byte aligned (x too when transpose = 0). */
pgk_status pgk_quantize_e2m1_unit(const void* x, uint8_t* out, int rows, int k, int transpose, pgk_stream s);
/* D[m][n] = bf16(sum_k e2m1(a[m][k]) * e2m1(b[n][k])) on operands packed by pgk_quantize_e2m1_unit, exact in fp32
 * for K < 116000 (v_mfma_scale_f32_16x16x128_f8f6f4, e2m1 operands, unit scales).  kp % 128 == 0; d bf16 [M,N]. */
pgk_status pgk_gemm_fp4_nt(const uint8_t* a_packed, const uint8_t* b_packed, void* d, int m, int n, int kp, pgk_stream s);
/* Bytes of the packed A and B of one gemm_nvf4_bf16_sm120 call: (m + n) * Kp/2 (A first, B at m * Kp/2). */
size_t pgk_gemm_nvf4_workspace_bytes(int m, int n, int k);

/* ------------------------------------------------------------------- attention ------ */
/* ops.cuh:287-290 sdpa_causal(Q[Hq,q,D], K[Hkv,kv,D], V, scale<=0 -> 1/sqrt(D)), mask
 * kv_pos < (kv_len - q_len) + q_pos + 1.  Strides are in elements so both the reference's
 * [H,S,D] layout and the projection's native [S,H,D] layout work without transposes; Hkv may be a
 * divisor of Hq (GQA without repeat_interleave). */
pgk_status pgk_sdpa_causal(const void* q, const void* k, const void* v, void* out, int hq, int hkv, int q_len,
                           int kv_len, int d, float scale, int64_t q_stride_h, int64_t q_stride_s,
                           int64_t kv_stride_h, int64_t kv_stride_s, int64_t o_stride_h, int64_t o_stride_s,
                           pgk_dtype dt, pgk_stream s);
/* [build-defined: the reference's encoders run batched_matmul -> softmax -> batched_matmul]  sdpa_noncausal:
 * out[h][i] = softmax_j(q[h][i] . k[h / rep][j] * scale, over ALL j < kv_len) . v[h / rep] - no mask, and no relation
 * between q_len and kv_len (cross-attention: few queries, many keys).  Arguments as pgk_sdpa_causal.  f16 / bf16 with
 * d 64 or 128, 16-byte aligned q / k / v, 8-byte aligned out, q / kv strides multiples of 8 and out strides multiples of 4
 * elements run the MFMA flash kernel (FlashFull policy, every q_len; V^T and split workspaces from the pool); anything
 * else - float32 included - and PYGPUKIT_FLASH_ATTENTION=0 run the one-workgroup-per-row fallback (kv_len <= 15360,
 * q_len <= 65535, PGK_ERR_UNSUPPORTED beyond). */
pgk_status pgk_sdpa_noncausal(const void* q, const void* k, const void* v, void* out, int hq, int hkv, int q_len,
                              int kv_len, int d, float scale, int64_t q_stride_h, int64_t q_stride_s,
                              int64_t kv_stride_h, int64_t kv_stride_s, int64_t o_stride_h, int64_t o_stride_s,
                              pgk_dtype dt, pgk_stream s);
/* sdpa_causal_fp8 (src/pygpukit/ops/nn/attention.py:238-347; flash_attention_3_fp8_sm120.cuh): the same op with the
 * first product in fp8.  Q (per query head) and K (per kv head) are quantised to e4m3 with one power-of-two scale
 * per head (pgk_quantize_fp8_per_head), s = scale * 2^(eq+ek) * sum_d q8 * k8 in fp32, softmax in fp32, P.V with
 * V unquantised in bf16, bf16 out.  Arguments as pgk_sdpa_causal; dt must be PGK_BF16 and d 128 (anything else is
 * PGK_ERR_INVALID with a message); pointers 16-byte aligned, strides multiples of 8 elements.  Workspaces come
 * from the pool (stream-ordered). */
pgk_status pgk_sdpa_causal_fp8(const void* q, const void* k, const void* v, void* out, int hq, int hkv, int q_len,
                               int kv_len, int d, float scale, int64_t q_stride_h, int64_t q_stride_s,
                               int64_t kv_stride_h, int64_t kv_stride_s, int64_t o_stride_h, int64_t o_stride_s,
                               pgk_dtype dt, pgk_stream s);
/* quantize_to_fp8_e4m3_per_head_kernel (flash_attention_3_fp8_sm120.cuh:475-547): x bf16 [heads, rows, 128] with
 * (head, row) strides in elements -> codes u8 [heads, rows, 128] (contiguous) and one UE8M0 byte per head.
 * a = max|x_h|; e = 0 when a == 0, else the smallest integer with 448 * 2^e >= a, clamped to [-127, 127];
 * scale byte = e + 127; code = RNE satfinite e4m3 of x * 2^-e (an exact multiply: bit-reproducible). */
pgk_status pgk_quantize_fp8_per_head(const void* x, uint8_t* codes, uint8_t* scale_bytes, int heads, int rows, int d,
                                     int64_t stride_h, int64_t stride_s, pgk_dtype dt, pgk_stream s);
/* ---- Llama-4 attention (src/pygpukit/ops/nn/llama4.py; native/ops/nn/llama4_kernels.cuh) ----
 * t(pos) = log1pf(floorf((float)(pos + 1) / floor_scale)) * attn_scale + 1, every step rounded to fp32 in that order
 * (log1pf correctly rounded, no FMA contraction).  `pos_dt` is the element type of `positions`: PGK_I64 (the
 * reference's) or PGK_I32.
 * l2norm: out = in * rsqrt(mean(in^2) + eps) over the last dimension, no gamma; f32 / f16 / bf16, fp32 sums, any
 * features >= 1; in == out allowed. */
pgk_status pgk_l2norm(const void* in, void* out, int rows, int features, float eps, pgk_dtype dt, pgk_stream s);
/* irope_scale_q: out[s][h][:] = q[s][h][:] * t(positions[s]); Q [seq_len, n_heads, head_dim] f16 / bf16 (fp32 multiply,
 * one RNE rounding). */
pgk_status pgk_irope_scale_q(const void* q, const void* positions, void* out, int seq_len, int n_heads, int head_dim,
                             float attn_scale, float floor_scale, pgk_dtype pos_dt, pgk_dtype dt, pgk_stream s);
/* sdpa_irope: softmax(Q.K^T * t(positions[i]) / sqrt(d) + mask) . V; query row i sees kv j exactly when
 * j <= i + causal_offset and j < kv_len (kv_len may be smaller or larger than q_len).  Strides in elements as in
 * pgk_sdpa_causal.  f16 / bf16, d 64 or 128, hq % hkv == 0, q_len >= 1, kv_len >= 1, causal_offset >= 0, pointers
 * 16-byte aligned and strides multiples of 8 elements: anything else is PGK_ERR_INVALID with a message (the
 * reference's kernel returns NaN rows for a negative offset).  Workspaces come from the pool (stream-ordered). */
pgk_status pgk_sdpa_irope(const void* q, const void* k, const void* v, const void* positions, void* out, int hq, int hkv,
                          int q_len, int kv_len, int d, float attn_scale, float floor_scale, int causal_offset,
                          int64_t q_stride_h, int64_t q_stride_s, int64_t kv_stride_h, int64_t kv_stride_s,
                          int64_t o_stride_h, int64_t o_stride_s, pgk_dtype pos_dt, pgk_dtype dt, pgk_stream s);
/* [build-defined: the reference has no cached Llama-4 path]  llama4_qk_norm_cache_write: one launch over the projection
 * buffers q [seq, hq*d], k / v [seq, hkv*d] (row-major) and the caches [hkv, max_seq, d] (pgk_kv_cache_write's
 * un-expanded layout): with qk_norm != 0 every Q head row is l2-normalised in place and every K head row is normalised
 * on its way to k_cache[h][pos0 + s] (k itself is not written); V goes to v_cache[h][pos0 + s].  The normalisation is
 * pgk_l2norm's, bit for bit.  pos0 = pos_buf[0] (device int32) when pos_buf is non-NULL, else h_pos.  Rows with
 * pos0 + s outside [0, max_seq) are not written; a host position with h_pos + seq > max_seq is PGK_ERR_INVALID.
 * f16 / bf16, d 64 or 128, 16-byte aligned pointers, seq >= 1.  No allocation, no sync. */
pgk_status pgk_llama4_qk_norm_cache_write(void* q, const void* k, const void* v, void* k_cache, void* v_cache, int seq, int hq,
                                          int hkv, int max_seq, int d, float eps, int qk_norm, int h_pos,
                                          const int32_t* pos_buf, pgk_dtype dt, pgk_stream s);
/* [build-defined] sdpa_irope_fixed_cache: split-KV flash-decoding of one query row Q [hq, 1, d] over rows 0 .. pos of the
 * caches [hkv, max_seq, d] = pgk_sdpa_irope(Q, cache[:, :pos+1], positions = [pos], causal_offset = pos); pos = pos_buf[0]
 * when pos_buf is non-NULL (clamped to the cache on the device), else h_pos (outside [0, max_seq): PGK_ERR_INVALID).
 * t(pos) / sqrt(d) multiplies the fp32 q values: Q * t is never rounded to 16 bits.  `workspace` must hold
 * pgk_sdpa_decode_workspace_bytes(hq, d, max_seq).  f16 / bf16, d 64 or 128, hq % hkv == 0.  No allocation, no sync. */
pgk_status pgk_sdpa_irope_fixed_cache(const void* q, const void* k_cache, const void* v_cache, void* out, int hq, int hkv,
                                      int max_seq, int d, float attn_scale, float floor_scale, int h_pos,
                                      const int32_t* pos_buf, void* workspace, pgk_dtype dt, pgk_stream s);
/* ---- positional encodings beside RoPE (reference: ops/nn/rope.py:386-653; the tables are built on the host) ----
 * pope_inplace: q [seq, hq, d] and k [seq, hk, d] (f32 / f16 / bf16, the same type) += encoding[start_pos + s][:], encoding
 * fp32 [max_seq, d]: one fp32 add, one RNE rounding.  start_pos < 0 or start_pos + seq > max_seq is PGK_ERR_INVALID. */
pgk_status pgk_pope_inplace(void* q, void* k, const void* encoding, int seq, int hq, int hk, int d, int start_pos, int max_seq,
                            pgk_dtype dt, pgk_stream s);
/* alibi_compute_bias: bias fp32 [num_heads, seq_len, seq_len] = -slopes[h] * (i - j) (one fp32 multiply; positive for
 * j > i), or -1e9 for j > i when `causal`.  slopes fp32 [num_heads]. */
pgk_status pgk_alibi_compute_bias(const void* slopes, void* bias, int seq_len, int num_heads, int causal, pgk_stream s);
/* alibi_add_bias: scores fp32 [batch, num_heads, q_len, kv_len] -= slopes[h] * (start_pos + i - j) for every j, product and
 * difference rounded separately (no FMA).  scores_dt / slopes_dt other than PGK_F32, or n_slopes != num_heads, is
 * PGK_ERR_INVALID. */
pgk_status pgk_alibi_add_bias(void* scores, const void* slopes, int batch, int num_heads, int q_len, int kv_len, int start_pos,
                              pgk_dtype scores_dt, pgk_dtype slopes_dt, int n_slopes, pgk_stream s);
/* [build-defined: the reference only materialises the bias]  sdpa_alibi: with off = kv_len - q_len,
 *   out[h][i] = softmax_j(q[h][i] . k[h / rep][j] * scale - slopes[h] * (off + i - j), over j <= off + i) . v[h / rep]
 * on the MFMA flash-prefill kernel; slopes fp32 [hq], one per QUERY head; scale <= 0 means 1 / sqrt(d).  Strides in elements
 * as in pgk_sdpa_causal.  f16 / bf16, d 64 or 128, hq % hkv == 0, kv_len >= q_len >= 1, pointers 16-byte aligned and strides
 * non-negative multiples of 8 elements: anything else is PGK_ERR_INVALID with a message.  Workspaces come from the pool. */
pgk_status pgk_sdpa_alibi(const void* q, const void* k, const void* v, const void* slopes, void* out, int hq, int hkv, int q_len,
                          int kv_len, int d, float scale, int64_t q_stride_h, int64_t q_stride_s, int64_t kv_stride_h,
                          int64_t kv_stride_s, int64_t o_stride_h, int64_t o_stride_s, pgk_dtype dt, pgk_stream s);
/* [build-defined] sdpa_alibi_fixed_cache: pgk_sdpa_fixed_cache's contract (Q [hq, q_len, d] over the first context_len rows of
 * the caches [hkv, max_seq, d]; ctx_buf, a device int32, overrides h_context_len when non-NULL) with the bias
 * -slopes[h] * (context_len - q_len + i - j).  q_len == 1: split-KV flash-decoding, `workspace` must hold
 * pgk_sdpa_decode_workspace_bytes(hq, d, max_seq), no allocation, no sync.  q_len > 1: ctx_buf must be NULL; pgk_sdpa_alibi
 * over the cache in place.  f16 / bf16, d 64 or 128, hq % hkv == 0, q_len <= context_len <= max_seq. */
pgk_status pgk_sdpa_alibi_fixed_cache(const void* q, const void* k_cache, const void* v_cache, const void* slopes, void* out, int hq,
                                      int hkv, int q_len, int max_seq, int d, float scale, int h_context_len, const int32_t* ctx_buf,
                                      void* workspace, pgk_dtype dt, pgk_stream s);
/* [build-defined: the reference's T5 encoder adds a dense [1, H, S, S] bias to materialised scores on the host]  sdpa_relbias:
 *   out[h][i] = softmax_j(q[h][i] . k[h / rep][j] * scale + table[h][clamp(j - i, -radius, radius) + radius], ALL j < kv_len) . v[h / rep]
 * - no mask, any q_len, kv_len >= 1; delta is KEY position minus QUERY position.  table: fp32 [hq][2 * radius + 1] on the device,
 * one row per QUERY head, finite entries, radius >= 0; scale <= 0 means 1 / sqrt(d).  Strides in elements as in pgk_sdpa_noncausal.
 * f16 / bf16 with d 64 or 128, radius <= 1024, 16-byte aligned q / k / v, 8-byte aligned out, q / kv strides multiples of 8 and
 * out strides multiples of 4 elements run the MFMA flash kernel (FlashRelBias policy: the head's row staged in LDS, the score
 * accumulators start from it; workspaces from the pool); anything else with d <= 256 - float32 included - and
 * PYGPUKIT_FLASH_ATTENTION=0 run one wave per (head, query row) in fp32 (hq <= 65535).  d > 256 there: PGK_ERR_UNSUPPORTED. */
pgk_status pgk_sdpa_relbias(const void* q, const void* k, const void* v, const void* table, void* out, int hq, int hkv, int q_len,
                            int kv_len, int d, int radius, float scale, int64_t q_stride_h, int64_t q_stride_s, int64_t kv_stride_h,
                            int64_t kv_stride_s, int64_t o_stride_h, int64_t o_stride_s, pgk_dtype dt, pgk_stream s);
/* Host-only: "relbias_flash" or "relbias_rows", the kernel pgk_sdpa_relbias takes for this head_dim, radius and dtype; aligned:
 * pointers and strides as the flash path needs them (a contiguous [H, S, D] call is).  NULL + pgk_last_error for head_dim outside
 * 1..256, a negative radius or a non-float dtype. */
const char* pgk_relbias_plan(int head_dim, int radius, pgk_dtype dt, int aligned);
/* ops.cuh:294-300 sdpa_causal_fixed_cache / _ptr: Q[Hq,q_len,D] over the first context_len rows of
 * cache[Hc,max_seq,D].  ctx_buf (device int32) overrides h_context_len when non-NULL.  q_len == 1
 * uses split-KV flash-decoding (replaces native/ops/nn/flash_decoding.cuh:75-377, fp16-only there);
 * `workspace` must hold pgk_sdpa_decode_workspace_bytes(). */
size_t pgk_sdpa_decode_workspace_bytes(int hq, int d, int max_seq);
pgk_status pgk_sdpa_fixed_cache(const void* q, const void* k_cache, const void* v_cache, void* out, int hq, int hc,
                                int q_len, int max_seq, int d, float scale, int h_context_len,
                                const int32_t* ctx_buf, void* workspace, pgk_dtype dt, pgk_stream s);

/* ---------------------------------------------------------------------- engine ------ */
/* Native decode/prefill launcher: one C call (or one hipGraph launch) per token step instead of
 * ~21 Python-dispatched launches per layer.  Replaces the device-dispatch half
 * of rust/pygpukit-core (dispatch/controller.rs:267-530) and the 2L+2 captured graphs of
 * src/pygpukit/llm/decode/m1_graph.py:248-589 with ONE whole-step graph whose token id, position
 * and context length live in device memory. */
typedef struct {
    int vocab_size, hidden_size, num_layers, num_heads, num_kv_heads, head_dim, intermediate_size;
    int max_seq_len;      /* KV-cache rows per sequence */
    int max_batch;        /* independent sequences resident on this GPU */
    float norm_eps, rope_theta;
    int weight_format;    /* 0 = bf16 linears, 1 = fp8-e4m3 linears with 128x128 bf16 block scales (w8a16),
                           * 2 = as 1, and prefill of > 128 tokens also quantises activations per row per 128 k
                           *     and runs the projections on the fp8 x fp8 MFMA GEMM (decode stays w8a16),
                           * 3 = NVF4 linears (w4a16) in the NK layout of pgk_quantize_nvf4_nk: w_* = uint8 codes
                           *     [N, K/2] (16-byte aligned), s_* = uint8 scale bytes [N, K/32] (required).  Decode
                           *     streams the codes (GEMV chunks of <= 8 sequences); prefill dequantises one layer at a
                           *     time into an engine scratch (counted by pgk_engine_bytes) and runs the bf16 GEMMs.
                           *     Formats 1-3 need hidden_size and intermediate_size multiples of 128. */
    int use_qk_norm;
} pgk_model_config_t;

typedef struct {
    const void* attn_norm;          /* [H] bf16 */
    const void* w_qkv;              /* [(Hq+2Hkv)*D, H] bf16 or u8 */
    const void* s_qkv;              /* fp8 block scales, NVF4 scale bytes [N, K/32] (format 3), or NULL */
    const void* q_norm; const void* k_norm;   /* [D] bf16 or NULL */
    const void* w_o;  const void* s_o;        /* [H, Hq*D] */
    const void* mlp_norm;           /* [H] */
    const void* w_gate_up; const void* s_gate_up;   /* [2I, H]: rows 0..I-1 gate, I..2I-1 up */
    const void* w_down; const void* s_down;         /* [H, I] */
} pgk_layer_weights_t;

pgk_status pgk_engine_create(const pgk_model_config_t* cfg, const void* embed, const void* lm_head,
                             const void* final_norm, const pgk_layer_weights_t* layers, pgk_engine* out);
pgk_status pgk_engine_destroy(pgk_engine e);
/* bytes the engine allocated from the pool (KV caches, activations, rope tables) */
pgk_status pgk_engine_bytes(pgk_engine e, size_t* kv_bytes, size_t* workspace_bytes);
/* Prefill `n` tokens of sequence slot `seq` starting at position start_pos; writes K/V rows, and if
 * h_logits_out != NULL copies the last row's logits (fp32 [V]) to host.  all_logits (device bf16
 * [n,V]) may be NULL. */
pgk_status pgk_engine_prefill(pgk_engine e, int seq, const int32_t* h_tokens, int n, int start_pos,
                              void* all_logits, float* h_last_logits, pgk_stream s);
/* Set the per-sequence decode state (token to feed, its position) for `batch` sequences. */
pgk_status pgk_engine_set_state(pgk_engine e, const int32_t* h_tokens, const int32_t* h_positions, int batch,
                                pgk_stream s);
/* Enqueue ONE decode step for the first `batch` sequences: embeds state tokens, runs all layers
 * (KV write at position, attention over position+1 rows), lm_head, greedy argmax; then
 * state.token = argmax, state.position += 1, and the token is appended to the engine's device
 * token log.  No host interaction: any number of steps can be queued back to back. */
pgk_status pgk_engine_decode_step(pgk_engine e, int batch, pgk_stream s);
/* Eager steps whose every launch carries its own start/stop hipEvent (hipExtLaunchKernelGGL: the dispatch's begin -> end
 * interval, what rocprofv3 --kernel-trace reports): per-kernel-class time sums (ms) and launch counts for the 8 classes
 * embed, norm_qkv, attn, oproj, gateup, down, lmhead, argmax (in that order).  Advances the decode state like n_iters
 * ordinary steps.  (Measurement only: the reference's counterpart is its KernelProfiler, native/core/profiler.hpp.) */
pgk_status pgk_engine_profile_step(pgk_engine e, int batch, int n_iters, float* h_ms_sum, int* h_count, pgk_stream s);
/* Timeline of ONE graph-replayed step (diagnostic): every workgroup of every kernel stamps the 100 MHz s_memrealtime
 * counter at its first and last instruction; per launch, in launch order,
 *   h_out[6 i .. 6 i + 5] = { kernel class, workgroups, first start, last start, first end, last end }
 * (times in 10 ns ticks from the step's first start).  `warm` replays precede the measured one; the state advances by
 * warm + 1 steps; the engine's own captured graph is untouched. */
pgk_status pgk_engine_timeline(pgk_engine e, int batch, int warm, uint64_t* h_out, int max_launches, int* n_launches, pgk_stream s);
/* Capture decode_step(batch) into hipGraphs owned by the engine / replay them.  A step has two launch sequences - the
 * short-context one (contexts <= 512, a single sequence <= 384: whole-context attention kernels, 4L+2 launches at batch 1)
 * and the split-KV one (5L+2), whose slices are cut for a context tier (1024, 2048, ... positions, the cache length) - all
 * correct at ANY context they cover; capture records the short sequence and one split-KV graph per tier the cache can hold,
 * and replay picks per step by the CONTEXT the step will see, from the positions last given to pgk_engine_set_state plus
 * the steps enqueued since (a host-side bound, a speed hint only).  The reference's fixed cache takes any max_seq_len with one code
 * path (src/pygpukit/llm/layers/attention.py:128-146, llm/decode/m1_graph.py:248-325). */
pgk_status pgk_engine_capture(pgk_engine e, int batch, pgk_stream s);
pgk_status pgk_engine_replay(pgk_engine e, int n_steps, pgk_stream s);
/* Read back: logits of the last step (device pointer, fp32 [batch,V]), token log (host copy). */
pgk_status pgk_engine_logits_ptr(pgk_engine e, void** logits_f32);
pgk_status pgk_engine_read_tokens(pgk_engine e, int32_t* h_out, int batch, int n_steps, pgk_stream s);
pgk_status pgk_engine_reset_log(pgk_engine e, pgk_stream s);
/* In-graph stochastic sampling (the graph-compatible sample_topk_to_buf_ptr of src/pygpukit/ops/sampling.py:40-71, for the
 * whole-step graph): each step draws one token per sequence from the step's fp32 logits with pgk_sample_token's
 * semantics; the uniform numbers are row (step counter % n_rows) of `h_uniforms` [n_rows][max_batch], copied to the device
 * here.  temperature <= 0 restores greedy argmax.  The sampling node's arguments are baked into a captured graph, so a
 * call that changes on/off, temperature, top_k, top_p or n_rows (or has to grow a buffer) DROPS the engine's captured
 * graph: pgk_engine_replay fails until pgk_engine_capture is called again.  A refill with identical parameters and
 * n_rows keeps the graph and only queues fresh uniforms. */
pgk_status pgk_engine_set_sampling(pgk_engine e, float temperature, int top_k, float top_p, const float* h_uniforms, int n_rows,
                                   pgk_stream s);
/* Diagnostic: per logged step, {s_memtime (shader clock ticks), s_memrealtime (100 MHz ticks)} stamped by the
 * step's last kernel: the in-kernel shader clock between two steps is d(memtime)/d(memrealtime) x 100 MHz
 * (MI355X_MICROARCH.md, DVFS give-back item 6).  h_out: uint64[2 * n_steps]. */
pgk_status pgk_engine_read_clock(pgk_engine e, uint64_t* h_out, int n_steps, pgk_stream s);
/* KV cache access for parity tests: pointers to layer `l`'s K and V caches [max_batch,Hkv,max_seq,D] bf16 */
pgk_status pgk_engine_kv_ptr(pgk_engine e, int layer, void** k, void** v);
/* device int32[max_batch] arrays holding each sequence's current token and position (the step's inputs and,
 * after it, its sampled tokens): what the data-parallel harness all-gathers over RCCL */
pgk_status pgk_engine_state_ptr(pgk_engine e, void** tokens, void** positions);
/* number of kernel launches one decode step enqueues (for reporting) */
pgk_status pgk_engine_launches_per_step(pgk_engine e, int* n);
/* Read-only: the attention launches of ONE decode step of `batch` sequences whose largest position is `max_position`
 * (what pgk_engine_set_state + pgk_engine_decode_step, or a replay of a capture of that batch, would run), computed by
 * the functions the launcher itself calls; no device work, no state change.  `out` receives one line per chunk:
 *   chunk b0=<first sequence> m=<sequences> form=gemv|batched|tiled|packed attn=<kernel> heads=<g[+g..]> nsplit=<slices>
 *         span=<rows the slices cover> out=f32|bf16 tail=none|merge|merge_oproj_bf16|merge_oproj_fp8
 * attn: attn_oproj_mfma / attn_oproj (fused with o_proj), attn_mfma_direct / attn_decode_direct (whole context, one
 * workgroup per sequence and kv head), attn_decode_split; heads: query heads per kv head of each launch (GQA head chunks).
 * One exception for replays: a SHORT step (largest position below 384 for one sequence, 512 for a batch) whose chunk has
 * no whole-context kernel - a single sequence with fp8 / NVF4 W_o or with a GQA group other than 1 / 2 / 4 - was captured
 * with the cache length as its span; the replay runs the kernels named here over more slices than nsplit / span say,
 * which report the eager step. */
pgk_status pgk_engine_attn_plan(pgk_engine e, int batch, int max_position, char* out, size_t n);
/* Read-only, no device: what wave `wave` (0..3) of the fused MFMA decode attention kernel requests for a context of c1 cached
 * rows, and its counted waits.  pre: W_o preloads of the form (4 fused with o_proj, 0 batch form); c0: start of a later chunk
 * (a positive multiple of 192).  out[5]: [0..2] requests allowed outstanding at the waits for the new token's inputs, chunk 0's
 * K rows, chunk 0's V rows; [3] tiles of 16 rows the wave stages at c0 (0 where c0 >= c1); [4] requests allowed outstanding at
 * the wait for their K rows.  A tile is 4 K and 4 V requests; chunk 0 is always 3 tiles per wave. */
pgk_status pgk_attn_mfma_plan(int c1, int c0, int wave, int pre, int32_t* out);
/* Read-only: the PROJECTION launches (w_qkv, w_o, w_gate_up, w_down, lm_head), computed by the functions the launchers
 * themselves call; no device work, no state change.
 * prefill_n == 0: one decode step of `batch` sequences whose largest position is `max_position`.  Per chunk one line
 *   chunk b0=<first sequence> m=<sequences> form=gemv|batched|tiled|packed act=f32|bf16 oproj=fused|merged|own
 *         carried=<0|1> normrows=<0|1> attn16=direct|normrows|none
 * (act: the activation type the chunk's projections read; oproj: inside the fused attention kernel, inside the split-KV
 * merge kernel, or a launch of its own; carried: o_proj / down_proj carry the next RMSNorm; normrows: norm_rows_bf16
 * launches in front of the consumers; attn16: who writes o_proj's bf16 input rows), followed by one line per projection:
 *   proj name=<p> kernel=fused_gemv m=<M> act=.. w=bf16|fp8|nvf4 pro=norm|plain|norm_sum r=<rows per wave> c=<preload
 *        depth, 0: the generic loop> grid=<workgroups> n=<outputs> k=<K>
 *   proj name=<p> kernel=batched_reg|batched_lds|batched_mt w=bf16|fp8 rows=<weight rows per workgroup> mp=<LDS image
 *        rows> tiles=<M tiles of 16 per workgroup> copy=<1: reads the fragment-major copy> grid=.. n=.. k=..
 *   proj name=<p> kernel=pkgemm|pkgemm_resid splits=<split-K slabs> n=.. k=..
 * (no `o` line where o_proj is fused or merged).
 * prefill_n > 0: one pgk_engine_prefill call of prefill_n tokens (batch / max_position ignored); one line
 *   prefill n=.. path=ws|pk|gemm|fp8act ws=.. pk=.. pk_heads=.. carried=.. pkd=.. nvf4=.. fp8act=.. fuse_heads=..
 *           fuse_heads8=.. fuse_sw16=.. fuse_sw8=.. s_qkv=.. s_o=.. s_gu=.. s_d=..
 * path: wsgemm_nt, pkgemm_nt, the 128- / 256-tile engine_gemm_* kernels, gemm_fp8_*; s_*: the split-K slabs of the
 * family that runs. */
pgk_status pgk_engine_linear_plan(pgk_engine e, int batch, int max_position, int prefill_n, char* out, size_t n);

/* ------------------------------------------------------------------ Mixture of Experts ------ */
/* Routing, permutation and grouped expert GEMMs (ops_moe.hip).  Restates native/ops/moe/topk_kernels.cuh,
 * permute_kernels.cuh, moe_kernels.cuh and native/ops/matmul/gemm/w8a16_bf16/sm120/grouped_gemm.cu.  Every entry is
 * stream-ordered; none synchronises the host or reads a device value back to size a launch.
 *
 * Top-k: logits [T,E] (bf16 or fp32, E <= 256, k <= 8) -> weights [T,k] (logits dtype), indices [T,k] int32.  The k
 * largest logits in descending order, the lowest expert index first among equal logits (the strict '>' scan of
 * topk_with_indices_kernel, topk_kernels.cuh:49-64); NaN logits rank as -inf; the k ids are distinct.  softmax != 0
 * replaces the values by softmax_topk over the k (fp32, topk_kernels.cuh:192-260), stored in the logits dtype.
 * pgk_moe_softmax_topk is that second step alone, in place. */
pgk_status pgk_moe_topk_softmax(const void* logits, void* weights, int32_t* indices, int T, int E, int k, int softmax,
                                pgk_dtype dt, pgk_stream s);
pgk_status pgk_moe_softmax_topk(void* weights, int T, int k, pgk_dtype dt, pgk_stream s);
/* Permutation of the T*k (token, slot) entries by expert (moe_kernels.cuh / permute_kernels.cuh):
 *   expert_counts [E], expert_offsets [E+1] (exclusive scan, offsets[E] = rows placed),
 *   permute_indices [T*k]: sorted row r holds flat index token*k + slot,  reverse_perm [T*k]: flat -> sorted row,
 *   tiles [pgk_moe_max_tiles(T,k,E)][2]: {expert, first sorted row} per 128-row piece of every non-empty expert
 *     segment, in expert order, then {-1, 0} to the end - the table pgk_grouped_gemm_sorted reads.
 * DETERMINISTIC, unlike the reference (whose order within an expert is whatever atomicAdd produced): within one expert the
 * rows are in ascending flat index (token-major, then slot) - a stable counting sort, no atomic decides an order.
 * Ids outside [0,E) are not placed (reverse_perm -1; permute_indices is -1 past offsets[E]).  workspace: pgk_moe_workspace_bytes(T,k,E) bytes of device memory. */
int pgk_moe_max_tiles(int T, int k, int E);
size_t pgk_moe_workspace_bytes(int T, int k, int E);
pgk_status pgk_moe_compute_permutation(const int32_t* indices, int T, int k, int E, int32_t* expert_counts,
                                       int32_t* expert_offsets, int32_t* permute_indices, int32_t* reverse_perm,
                                       int32_t* tiles, void* workspace, pgk_stream s);
/* gathered [T*k, H] = x[permute_indices[r] / k]; rows whose entry is outside [0, T*k) are zero (the permutation writes -1
 * past offsets[E]); bf16, f16 or fp32 */
pgk_status pgk_moe_gather(const void* x, const int32_t* permute_indices, void* gathered, int T, int k, int H, pgk_dtype dt,
                          pgk_stream s);
/* out [T,H] = sum over slot of weights[t,slot] * y[reverse_perm[t*k+slot]], summed in fp32 in slot order and rounded once
 * (scatter_with_reverse_perm_kernel).  weights and out are `dt`; y is `dt` [T*k,H] when splits == 0, or fp32 slabs
 * [splits][T*k][H] (pgk_grouped_gemm_sorted's split-K output) that are summed in slab order first. */
pgk_status pgk_moe_scatter(const void* y, int splits, const void* weights, const int32_t* reverse_perm, void* out, int T,
                           int k, int H, pgk_dtype dt, pgk_stream s);
/* row_expert_ids [nrows]: e with offsets[e] <= r < offsets[e+1], -1 past offsets[E] */
pgk_status pgk_moe_expand_expert_offsets(const int32_t* expert_offsets, int E, int32_t* row_expert_ids, int nrows, pgk_stream s);
/* Grouped expert GEMM, C[r,:] = A[r,:] . W[e_r]^T, bf16 A and C, W stacked [E,N,K]: bf16 (fp8 == 0; K, N % 8 == 0) or
 * fp8-e4m3 codes with bf16 128x128 block scales [E,N/128,K/128] (fp8 != 0; K, N % 128 == 0), the layout of
 * grouped_gemm_fp8_bf16.
 * _rows: any row order (the reference's contract, grouped_gemm.cu): fp32 dequantisation lut[code] * scale and fp32 sums;
 *   rows whose id is outside [0,E) are zero.
 * _sorted: rows grouped by expert (A = gathered [T*k,K], or x [T,K] read through a_map = permute_indices), driven by the
 *   tile table.  T*k/E <= 64: weight-streaming kernel, each active expert's weight read from HBM about once per call; else
 *   128x128 MFMA tiles.  The weight is rounded to bf16 after dequantisation (<= 2^-9 relative per weight).  splits == 0:
 *   C bf16 [T*k,N]; splits == pgk_grouped_gemm_sorted_splits(...): fp32 slabs [splits][T*k][N] for pgk_moe_scatter. */
pgk_status pgk_grouped_gemm_rows(const void* a, const void* w, const void* wscale, int fp8, void* c, const int32_t* row_expert_ids,
                                 int M, int N, int K, int E, pgk_stream s);
int pgk_grouped_gemm_sorted_splits(int T, int k, int E, int N, int K);
pgk_status pgk_grouped_gemm_sorted(const void* a, const int32_t* a_map, const void* w, const void* wscale, int fp8, void* c,
                                   int splits, const int32_t* expert_offsets, const int32_t* tiles, int T, int k, int E, int N,
                                   int K, pgk_stream s);

/* ------------------------------------------------------------------------ LSTM ------ */
/* LSTM forward over a whole sequence, one or two directions (ops_lstm.hip; reference: native/ops/nn/recurrent/lstm.inl).
 *   g = W_ih . x_t + b_ih + b_hh + W_hh . h_{t-1}  (gate order i, f, g, o);  c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g_g);
 *   h_t = sigmoid(o) tanh(c_t).
 * x [B,S,I]; per direction W_ih [4H,I], W_hh [4H,H], b_ih / b_hh [4H], h0 / c0 [B,H] or NULL for zeros.  bwd == NULL: one
 * direction, walked t = S-1..0 when reverse != 0, out [B,S,H], h_n / c_n [B,H].  bwd != NULL (reverse must be 0): the
 * backward direction runs in the same launches, out [B,S,2H] with forward in [..., :H] and backward in [..., H:] written
 * in place (leading dimension ndir * H, no concatenation pass), h_n / c_n [2,B,H].  out[:, t] is written at the position
 * processed, so h_n is out[:, S-1] walking forwards and out[:, 0] walking backwards.
 * dt: PGK_F32 (any I, H >= 1) or PGK_F16 / PGK_BF16 (I % 8 == 0, H % 8 == 0), shared by every tensor.  Gates, h and c are fp32
 * for the whole sequence in every dtype: only what is returned is rounded, once.
 * x, G (B*S*4H) and each weight must stay below 2^31 elements.
 * Workspaces (device, 16-byte aligned, fp32): ws_gates [ndir * B * S * 4H], ws_state [3 * ndir * B * H].  The library
 * allocates nothing, never synchronises the host and enqueues everything on `s`: 2 launches when pgk_lstm_plan says
 * resident (1), S + 2 when it says stepped (0).  PGK_LSTM_RESIDENT=0 (read per call) forces the stepped path. */
typedef struct {
    const void *w_ih, *w_hh, *b_ih, *b_hh, *h0, *c0;
} pgk_lstm_dir;
pgk_status pgk_lstm(const void* x, const pgk_lstm_dir* fwd, const pgk_lstm_dir* bwd, void* out, void* h_n, void* c_n, float* ws_gates,
                    float* ws_state, int B, int S, int I, int H, int reverse, pgk_dtype dt, pgk_stream s);
/* Host only, needs no device: 1 when a call of this size runs the resident recurrence (one workgroup per direction and
 * chunk of batch rows keeps W_hh in registers for all S steps), 0 when it runs one launch per timestep. */
int pgk_lstm_plan(int batch, int hidden, pgk_dtype dt);

/* ---------------------------------------------------------------------- conv1d ------ */
/* conv1d (ops_conv.hip; reference: src/pygpukit/ops/conv.py, native/ops/conv/conv1d_kernels.cuh):
 *   out[b][m][n] = bias[m] + sum_{c < C_in, t < K} weight[m][c][t] * x[b][c][n * stride + t - padding]   (zeros outside [0, L))
 * x [B,C_in,L], weight [C_out,C_in,K], bias [C_out] or NULL, L_out = (L + 2 * padding - K) / stride + 1 >= 1; any sizes.
 * [build-defined] epilogue, on the fp32 accumulator, in this order: + bias; act (0 none, 1 tanh GELU - the gelu op's device
 * function); layout [B,C_out,L_out] or, with channels_last, [B,L_out,C_out]; + add[L_out][C_out] (same dtype, may be NULL,
 * needs channels_last); one rounding to dt.
 * bf16 / f16 run an implicit GEMM on the 32x32x16 MFMA when pgk_conv1d_plan says 1; it reads the weight as the image
 * [K][C_out padded to 64][C_in padded to 32] that pgk_conv1d_pack_weight writes: packed_weight (16-byte aligned, of
 * pgk_conv1d_packed_elems elements) or, when NULL, packed per call into stream-ordered pool workspace.  float32, and 16-bit
 * calls with plan 0 or a misaligned packed_weight, run the tiled FMA kernel on `weight` itself.  One launch (+ the pack
 * pre-pass), never synchronises the host, everything on `s`.  B <= 65535, L + 2 * padding < 2^31. */
pgk_status pgk_conv1d(const void* x, const void* weight, const void* packed_weight, const void* bias, const void* add, void* out,
                      int B, int C_in, int C_out, int L, int K, int stride, int padding, int act, int channels_last, pgk_dtype dt,
                      pgk_stream s);
/* Host only, needs no device: 1 = MFMA kernel (16-bit dtype, (63 * stride + K + 64 * K) * 80 bytes of LDS <= 64 KiB,
 * PGK_CONV_MFMA != "0", read per call), 0 = FMA kernel, -1 = invalid shape or dtype. */
int pgk_conv1d_plan(int C_in, int C_out, int L, int K, int stride, int padding, pgk_dtype dt);
size_t pgk_conv1d_packed_elems(int C_in, int C_out, int K);
pgk_status pgk_conv1d_pack_weight(const void* weight, void* packed, int C_in, int C_out, int K, pgk_dtype dt, pgk_stream s);

/* [build-defined] ln_linear: the linear layer of a LayerNorm transformer's one-token step in one launch (ops_lnlinear.hip).
 *   out[m, n] = act( LN(x[m, :]; gamma, beta, eps) . w[n, :] + bias[n] ) + residual[m, n]
 * w is [n, k] (PyTorch layout), m = 1..8, every operand of dtype dt (f32 / f16 / bf16).  gamma == NULL: no norm (beta must then be
 * NULL too); bias and residual may be NULL; act 0 = none, 1 = the gelu op's tanh GELU.  residual may alias out; x may not
 * (PGK_ERR_INVALID).  LayerNorm uses the population variance, as pgk_layernorm.  Statistics, the normalised row, accumulation and
 * the epilogue are fp32 with ONE rounding at the store: in the 16-bit dtypes the normalised activations are never rounded to 16
 * bits when the m * k fp32 image fits in 64 KB of LDS; no-norm calls beyond that hold the rows in dt as pgk_gemv does; k % 8 != 0,
 * operands off 16-byte alignment and norm calls beyond the budget run a generic kernel (one wave per output).  No allocation, no
 * host synchronisation, capturable. */
pgk_status pgk_ln_linear(const void* x, const void* gamma, const void* beta, const void* w, const void* bias, const void* residual,
                         void* out, int m, int k, int n, float eps, int act, pgk_dtype dt, pgk_stream s);
/* Host only, needs no device: the kernel a pgk_ln_linear call takes.  0 = generic, 1 = fast path on an fp32 image, 2 = fast path on
 * a dt image (no norm, fp32 image over 64 KB), -1 = invalid shape or dtype.  `aligned`: x, w (and gamma, beta) are 16-byte aligned.
 * PGK_LN_LINEAR_GENERIC=1 (read per call) forces 0.  k is a runtime argument of every kernel: there is no k specialisation. */
int pgk_ln_linear_plan(int m, int k, int n, pgk_dtype dt, int norm, int aligned);
/* The same kernel at m = 1, n = 3 * heads * head_dim on the fused q | k | v weight, with a scatter epilogue: rows [0, d) go to
 * q_out[d], rows [d, 2d) to k_cache[h][pos][:] and rows [2d, 3d) to v_cache[h][pos][:] (d = heads * head_dim, caches
 * [heads, max_seq, head_dim]).  pos = pos_buf[0] when pos_buf != NULL, clamped to the cache on the device; else h_pos, which must
 * lie in [0, max_seq).  The stored values are bit-identical to pgk_ln_linear followed by two pgk_kv_cache_write calls. */
pgk_status pgk_ln_linear_qkv_cache(const void* x, const void* gamma, const void* beta, const void* w_qkv, const void* bias_qkv,
                                   void* q_out, void* k_cache, void* v_cache, int k, int heads, int head_dim, int max_seq, float eps,
                                   int h_pos, const int32_t* pos_buf, pgk_dtype dt, pgk_stream s);
/* out[hidden] = tok_table[state[0]][:] + pos_table[state[1]][:]: one fp32 add, one rounding.  state is a device int32[2]; both
 * indices are clamped on the device to [0, vocab) / [0, max_pos). */
pgk_status pgk_embed_token_position(const void* tok_table, const void* pos_table, void* out, int hidden, int vocab, int max_pos,
                                    const int32_t* state, pgk_dtype dt, pgk_stream s);

/* ------------------------------------------------------------------------ audio ------ */
/* ops.audio (pygpukit_amd/csrc/ops_audio.hip).  Everything is float32 up to the final cast.
 * pgk_audio_log_mel: samples [batch][n] -> log-mel in ONE launch: reflect centre padding by index arithmetic (center != 0, pad =
 * n_fft / 2), framing, window [n_fft], the DFT as an f32 MFMA GEMM against dft_table, re^2 + im^2, the filterbank mel_fb
 * [n_mels][n_fft / 2 + 1] over each row's span fb_span[2 m] .. fb_span[2 m + 1] (inclusive, first > last for an empty row), the
 * logarithm (log_mode 0: log10(max(m, eps)) with log_floor = log10(eps) rounded once by the caller; 1: ln(m + eps); 2: none), (x + offset) *
 * scale, the cast to out_dt.  dft_table is [2][n_fft][nbp] floats, nbp = n_fft / 2 + 1 rounded up to 32, zeros in the padding:
 * cos(2 pi k bin / n_fft) at [0][k][bin] and -sin at [1][k][bin].  out is [batch][n_mels][n_frames], or [batch][n_frames][n_mels]
 * when frames_last; n_frames may be less than the signal holds (drop_last_frame).  n_fft even in [16, 2048], 1 <= hop <= n_fft,
 * n_mels in [1, 256].  use_range: x = max(x, max over the whole call - range) before the affine; the kernel then stores float32,
 * folds the maximum into one device word and a second kernel finishes (one stream-ordered workspace allocation). */
pgk_status pgk_audio_log_mel(const float* samples, const float* window, const float* dft_table, const float* mel_fb, const int32_t* fb_span,
                             void* out, int batch, long long n, int n_fft, int hop, int center, int n_mels, int n_frames, int log_mode, float eps,
                             float log_floor, float offset, float scale, int use_range, float range, int frames_last, pgk_dtype out_dt,
                             pgk_stream s);
/* Host only: 1 = the workgroup's sample span sits in LDS, 0 = samples are read from global memory (the span, the window and the
 * power tile exceed the LDS budget, or PGK_AUDIO_LDS=0), -1 = invalid.  stage 0 = log-mel, 1 = stft. */
int pgk_audio_log_mel_plan(int n_fft, int hop, int stage);
/* The same kernel stopped after the DFT: out [n_frames][n_fft / 2 + 1][2] float32, re and im interleaved. */
pgk_status pgk_audio_stft(const float* samples, const float* window, const float* dft_table, float* out, long long n, int n_fft, int hop,
                          int center, pgk_stream s);
/* n outputs, one launch.  op 0: int16 -> x / 32768; 1: interleaved L R pairs -> (l + r) * 0.5; 2: (re, im) pairs -> re^2 + im^2;
 * 3: its square root; 4: ln(x + eps); 5: 10 log10(x + eps). */
pgk_status pgk_audio_map(const void* in, float* out, size_t n, int op, float eps, pgk_stream s);
/* In place, one launch (one workgroup).  mode 0: x / max|x| when max|x| > 1e-8; mode 1: x * target_rms / rms when rms > 1e-8. */
pgk_status pgk_audio_normalize(float* x, size_t n, int mode, double target_rms, pgk_stream s);
/* n_out = n * dst / src.  ratio >= 2 (src = ratio * dst): out[i] = sum_t taps[t] * x[i * ratio - n_taps / 2 + t], zeros outside the
 * signal.  ratio 0: linear interpolation at i * src / dst, position and fraction computed in 64-bit integers. */
pgk_status pgk_audio_resample(const float* x, float* out, const float* taps, long long n, long long n_out, int ratio, int n_taps, int src, int dst,
                              pgk_stream s);

/* ------------------------------------------------------------------- diffusion ------ */
/* ops_diffusion.hip: the row kernels of a diffusion transformer (DiT) block.  x, residual, sum_out, y are [batch, tokens,
 * features] in dt; for every token row r of batch element b
 *     mode 0:  s = residual ? residual[r] + g_b * x[r] : x[r];   sum_out[r] = round(s);
 *              y[r] = round((norm ? LN(s) : s) * (1 + scale_b) + shift_b)
 *     mode 1:  y[r] = round(residual[r] + g_b * (LN(x[r]) * (1 + scale_b) + shift_b))     (the reference's adaln_zero)
 * LN(s) = (s - mean) / sqrt(var + eps): population variance, no gamma / beta, on the unrounded fp32 s.  Each of gate / scale /
 * shift is tab[features] + vec[b * stride .. + features] in vec_dt (dt or PGK_F32); either part may be NULL (both NULL: g = 1,
 * scale = 0, shift = 0), stride 0 gives a batch-independent vector.  residual, sum_out and y may each be NULL in mode 0 (at
 * least one of sum_out / y is required; a gate needs a residual); mode 1 needs residual and y and always normalises.  sum_out
 * may alias residual and y may alias x.  A wave per row with the row in registers when features is a whole number of 16-byte
 * vectors within 64 * 8 of them and every pointer and vector row is 16-byte aligned, else a 256-thread block per row. */
pgk_status pgk_adaln_fused(const void* x, const void* residual, void* sum_out, void* y, const void* gate_tab, const void* gate_vec,
                           int64_t gate_stride, const void* scale_tab, const void* scale_vec, int64_t scale_stride,
                           const void* shift_tab, const void* shift_vec, int64_t shift_stride, int batch, int tokens, int features,
                           float eps, int norm, int mode, pgk_dtype dt, pgk_dtype vec_dt, pgk_stream s);
/* Host only: "adaln_wave" or "adaln_block" from the function the launcher calls; NULL and pgk_last_error when invalid.  aligned:
 * every pointer the launcher tests (rows, tables, vectors and their strides) is on a 16-byte boundary. */
const char* pgk_adaln_plan(int features, pgk_dtype dt, int aligned);
/* in [B, C, H, W] -> out [B * (H/p) * (W/p), C * p * p]: rows in row-major (h, w) patch order, columns (c, ph, pw).  A pure move
 * of 2- or 4-byte elements; H or W no multiple of p is PGK_ERR_INVALID. */
pgk_status pgk_patchify(const void* in, void* out, int B, int C, int H, int W, int p, pgk_dtype dt, pgk_stream s);
/* in [B * (H/p) * (W/p), p * p * Co] with columns (ph, pw, c) -> out [B, Co, H, W]. */
pgk_status pgk_unpatchify(const void* in, void* out, int B, int Co, int H, int W, int p, pgk_dtype dt, pgk_stream s);

/* ------------------------------------------------------------------ FLUX ------ */
/* (ops_flux.hip; reference: src/pygpukit/diffusion/models/flux/)
 * Per-head RMSNorm of Q and K with learned weights, then interleaved-pair RoPE, in place, one launch.  Row r = b * seq + p of Q
 * lies at q + r * row_stride + h * head_stride (elements of dt), K likewise from k; a fused [B * seq, 3 H D] projection has
 * row_stride = 3 H D, head_stride = D, k = q + H D.  Rows with p < split use wq_a / wk_a [head_dim], the others wq_b / wk_b (in
 * w_dt: dt or PGK_F32); a pair that no row uses may be NULL.  cos / sin are [seq, head_dim] fp32, indexed by p.  In fp32,
 * rounded once at the store:
 *     n[j] = x[j] / sqrt(mean_j(x^2) + eps) * w[j];   out[j] = n[j] * cos[p, j] + rot[j] * sin[p, j],
 *     rot[2i] = -n[2i+1], rot[2i+1] = n[2i].
 * head_dim 64 / 128 with every pointer and both strides on 16 bytes: the vector kernel (a head is 8 / 16 / 32 lanes of one
 * 16-byte vector); any other even head_dim <= 256 or any misalignment: a wave per head.  An odd head_dim is PGK_ERR_INVALID.
 * Nothing outside the head_dim columns of each Q and K head is read or written. */
pgk_status pgk_flux_qk_norm_rope(void* q, void* k, int64_t row_stride, int64_t head_stride, const void* wq_a, const void* wk_a,
                                 const void* wq_b, const void* wk_b, const float* cos, const float* sin, int batch, int seq, int split,
                                 int heads, int head_dim, float eps, pgk_dtype dt, pgk_dtype w_dt, pgk_stream s);
/* Host only: "flux_qk_norm_rope_vec" or "flux_qk_norm_rope_scalar"; NULL and pgk_last_error for an odd or oversized head_dim. */
const char* pgk_flux_qk_norm_rope_plan(int head_dim, pgk_dtype dt, int aligned);
/* out[r * out_stride + c] = gelu(x[r * cols + c]) (tanh form, the gelu op's device function: bit-identical to it); 16-byte
 * accesses when both pointers, cols and out_stride allow. */
pgk_status pgk_flux_gelu_pack(const void* x, void* out, int64_t rows, int cols, int64_t out_stride, pgk_dtype dt, pgk_stream s);
/* in [B, h * w, C * 4] with columns (c, ph, pw) -> out [B, C, 2h, 2w]; a pure move of 2- or 4-byte elements. */
pgk_status pgk_flux_unpack_latents(const void* in, void* out, int B, int C, int h, int w, pgk_dtype dt, pgk_stream s);
/* sample[i] = fma(dt_step, (float)v[i], sample[i]): the flow-matching Euler update; sample fp32, v in v_dt. */
pgk_status pgk_flow_euler_step(float* sample, const void* v, size_t n, float dt_step, pgk_dtype v_dt, pgk_stream s);

/* ------------------------------------------------------------------ VAE decoder ------ */
/* conv2d (ops_conv2d.hip; reference: src/pygpukit/ops/conv.py conv2d):
 *   out[n][m][oy][ox] = bias[m] + sum_{c, ky, kx} weight[m][c][ky][kx] * X[n][c][oy * sh + ky * dh - ph][ox * sw + kx * dw - pw]
 * with zeros outside X.  X is x itself, or with upsample == 2 its nearest-neighbour 2x: X[c][y][x] = x[c][y >> 1][x >> 1], of
 * size 2H x 2W, never materialised.  x is [N,C_in,H,W], or [N,H,W,C_in] with channels_last_in; out is [N,C_out,Ho,Wo], or
 * [N,Ho,Wo,C_out] with channels_last_out; add (or NULL) has out's shape and layout and is added in fp32 after the bias; one
 * rounding.  bf16 / f16 run an implicit GEMM on the 32x32x16 MFMA when pgk_conv2d_plan says 1; it reads the weight as the image
 * [KH * KW][C_out padded to 64][C_in padded to 32] that pgk_conv2d_pack_weight writes (packed_weight, 16-byte aligned, or NULL:
 * packed per call into pool workspace).  Everything else runs the tiled FMA kernel on `weight`.  One launch (+ the pack
 * pre-pass), never synchronises the host.  N <= 65535; H, W (after the upsample, with padding) < 2^30; global offsets are
 * size_t. */
pgk_status pgk_conv2d(const void* x, const void* weight, const void* packed_weight, const void* bias, const void* add, void* out,
                      int N, int C_in, int C_out, int H, int W, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w,
                      int dil_h, int dil_w, int upsample, int channels_last_in, int channels_last_out, pgk_dtype dt, pgk_stream s);
/* Host only: 1 = MFMA kernel (16-bit dtype, KH == KW in {1, 3}, stride_h == stride_w in {1, 2}, dilation 1, PGK_CONV_MFMA
 * not "0"), 0 = FMA kernel, -1 = invalid shape or dtype. */
int pgk_conv2d_plan(int C_in, int C_out, int H, int W, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                    int dil_w, int upsample, pgk_dtype dt);
size_t pgk_conv2d_packed_elems(int C_in, int C_out, int KH, int KW);
pgk_status pgk_conv2d_pack_weight(const void* weight, void* packed, int C_in, int C_out, int KH, int KW, pgk_dtype dt, pgk_stream s);
/* group_norm (ops_groupnorm.hip): x [N,C,HW] (or [N,HW,C] with channels_last), G groups of C / G consecutive channels;
 *   y = (x - mean_g) / sqrt(var_g + eps) * gamma[c] + beta[c], population variance over the group's (C / G) * HW elements;
 * act 1 applies SiLU to the fp32 value; one rounding.  Statistics are Welford (count, mean, M2) triples merged with Chan's
 * formula in a fixed order - no atomics, run-to-run identical.  Plan 0 ("block"): one workgroup per (image, group), one launch.
 * Plan 1 ("split"): launch 1 writes one partial per (image, pixel chunk, group) into pool workspace, launch 2 re-merges the
 * group's partials in chunk order in every workgroup and normalises its chunk.  PGK_GN_SPLIT=0/1 forces the plan. */
pgk_status pgk_group_norm(const void* x, const void* gamma, const void* beta, void* out, int N, int C, int HW, int G, float eps,
                          int act, int channels_last, pgk_dtype dt, pgk_stream s);
/* Host only: 0 = block, 1 = split, -1 = invalid. */
int pgk_group_norm_plan(int N, int C, int HW, int G, pgk_dtype dt, int channels_last);

/* ------------------------------------------------------------------------ RCCL ------ */
/* New functionality (the reference is single-GPU, docs/scheduler.md:358): data-parallel batch
 * decode over one 8xMI355X node.  One process per GPU; RCCL over xGMI only for the one-time weight
 * broadcast and the per-step gather of sampled tokens / logits. */
pgk_status pgk_comm_unique_id(char* h_id128);                       /* 128-byte ncclUniqueId */
pgk_status pgk_comm_init(pgk_comm* out, const char* h_id128, int rank, int world);
pgk_status pgk_comm_destroy(pgk_comm c);
pgk_status pgk_comm_broadcast(pgk_comm c, void* buf, size_t nbytes, int root, pgk_stream s);
pgk_status pgk_comm_all_gather(pgk_comm c, const void* send, void* recv, size_t nbytes_per_rank, pgk_stream s);
pgk_status pgk_comm_all_reduce_max_f64(pgk_comm c, double* buf, int n, pgk_stream s);
pgk_status pgk_comm_barrier(pgk_comm c, pgk_stream s);

#ifdef __cplusplus
}
#endif
#endif /* PGK_HIP_H */
