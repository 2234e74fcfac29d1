// Host-side decisions of the op-level attention family: pgk_sdpa_causal / _noncausal / _irope / _alibi / _causal_fp8 (ops_attention.hip,
// ops_flash.hip, ops_flash_fp8.hip, ops_llama4.hip, ops_posenc.hip), the fixed-cache decode entries and pgk_paged_attention_v1
// (ops_paged.hip).  Every split count, head grouping and kernel choice the launchers used to spell inline lives here as a pure
// function of the shape, the strides and "these pointers are aligned"; the launchers switch on what these functions return.  No
// device, stream or pointer is touched here.  The entry points one attention file offers the others are declared at the end.
#pragma once

#include "pgk_internal.h"

namespace pgk {

// element strides of Q [Hq][q_len][D], K / V [Hkv][kv_len][D] and the output (head, sequence position)
struct FlashStrides { long long qh, qs, kh, ks, oh, os; };

constexpr int FL_BQ = 128, FL_BKV = 64, FL_THREADS = 256;   // second-generation flash kernel: query rows / keys per tile, threads

// ---- split-KV decode over a fixed cache (decode_phase1_kernel, attn_core.hip.h) ------------------------------------------------
// chunks of the cache per kv head, fixed by max_seq (a captured graph keeps its grid while the context grows):
// ~256 positions per chunk at full context.  pgk_sdpa_decode_workspace_bytes sizes the records with it.
inline int decode_nsplit(int max_seq) {
    const int n = (max_seq + 255) / 256;
    return n < 1 ? 1 : (n > 64 ? 64 : n);
}

// Query heads served by one workgroup: every K / V row is read once per group of G heads of its kv head, so the largest of
// 4 / 2 / 1 that divides Hq / Hkv.  allow5 (pgk_sdpa_irope_fixed_cache, pgk_sdpa_alibi_fixed_cache): 5 serves Llama-4 Scout's
// Hq / Hkv = 40 / 8 in one pass, but only where its grid still has a workgroup per CU (256): with fewer the walk is
// latency-bound and G = 1's five times as many workgroups win (measured at 40 / 8 heads, D = 128: 8.4 against 13.7 us in a
// cache of 512 rows, 17.3 against 19.9 at 4096; 47.3 against 46.0 at 16384, 96.1 against 86.8 at 65536).
// pgk_sdpa_fixed_cache passes allow5 = false: nobody has measured it at G = 5, and its kernel is not instantiated there.
inline int decode_heads_per_group(int hq, int hkv, int nsplit, bool allow5) {
    const int rep = hq / hkv;
    const int G = rep % 4 == 0 ? 4 : rep % 2 == 0 ? 2 : 1;
    return allow5 && G == 1 && rep % 5 == 0 && (long long)nsplit * (hq / 5) >= 256 ? 5 : G;
}

// pgk_sdpa_fixed_cache: split-KV decode, or the general causal path over the cache prefix.  flash_decoding_off:
// PYGPUKIT_FLASH_DECODING=0, which only a host context length can honour (the general path cannot read a device one).
inline bool decode_fast(int q_len, int d, bool has_workspace, bool ptrs_aligned, bool flash_decoding_off, bool device_ctx) {
    return q_len == 1 && (d == 128 || d == 64) && has_workspace && ptrs_aligned && !(flash_decoding_off && !device_ctx);
}

// ---- pgk_paged_attention_v1: slices of ~512 positions per (sequence, kv head); 1 = no workspace, no combine launch ------------
inline int paged_nsplit(int max_context) {
    const int n = (max_context + 511) / 512;
    return n < 1 ? 1 : (n > 32 ? 32 : n);
}

// ---- prefill: which kernel takes an sdpa call ---------------------------------------------------------------------------------
// first-generation MFMA kernel (flash_prefill_kernel): 16-byte loads of Q, K and V rows.  in_aligned: q, k and v are 16-byte aligned
inline bool flash1_ok(int d, bool in_aligned, const FlashStrides& sd) {
    return (d == 64 || d == 128) && in_aligned && sd.qs % 8 == 0 && sd.ks % 8 == 0 && sd.qh % 8 == 0 && sd.kh % 8 == 0;
}
// second-generation kernel (flash_fwd_kernel) and the one-tile kernel: 8-byte stores of 4 output dims as well.  out_aligned8: out
// is 8-byte aligned.  (pgk_sdpa_irope / _alibi / _causal_fp8 have no other kernel and REQUIRE something stricter of their callers.)
inline bool flash2_ok(int d, bool in_aligned, bool out_aligned8, const FlashStrides& sd) {
    return flash1_ok(d, in_aligned, sd) && out_aligned8 && sd.os % 4 == 0 && sd.oh % 4 == 0;
}

enum SdpaKernel { SDPA_FLASH2 = 0, SDPA_ONE_TILE = 1, SDPA_FLASH1 = 2, SDPA_NAIVE = 3 };

// pgk_sdpa_causal (and pgk_sdpa_fixed_cache's general path).  half: f16 / bf16; flash_on: PYGPUKIT_FLASH_ATTENTION is not 0.
// The first-generation kernel keeps the prompts up to 128 rows, where its 64-row tiles give twice the workgroups; a bf16,
// D = 128 context of up to 128 keys is one tile (attn_short_kernel).
inline SdpaKernel sdpa_causal_pick(bool half, bool is_bf16, int d, int q_len, int kv_len, bool in_aligned, bool out_aligned8,
                                   const FlashStrides& sd, bool flash_on) {
    if (!half || !flash_on || !flash1_ok(d, in_aligned, sd)) return SDPA_NAIVE;
    const bool gen2 = flash2_ok(d, in_aligned, out_aligned8, sd);
    if (gen2 && q_len > 128) return SDPA_FLASH2;
    if (gen2 && is_bf16 && d == 128 && kv_len <= 128) return SDPA_ONE_TILE;
    return SDPA_FLASH1;
}
// pgk_sdpa_noncausal: the second-generation kernel at every q_len (the other two are causal-only), or the fallback
inline SdpaKernel sdpa_full_pick(bool half, int d, bool in_aligned, bool out_aligned8, const FlashStrides& sd, bool flash_on) {
    return half && flash_on && flash2_ok(d, in_aligned, out_aligned8, sd) ? SDPA_FLASH2 : SDPA_NAIVE;
}

// ---- pgk_sdpa_relbias: the flash kernel with the FlashRelBias policy, or the one-wave-per-row fp32 kernel (ops_relbias.hip) ----
// The staged table row is padded on both sides by the reach of a (wave, KV tile) pair - 64 keys + 32 query rows - so a tile that
// is not entirely saturated reads table entries with no per-element clamp.  The radius bound keeps the row within 9 KiB of LDS
// (64 KiB of K / V images at D = 128, two workgroups per CU in 160 KiB).
constexpr int FL_RELBIAS_PAD = FL_BKV + 32, FL_RELBIAS_MAX_RADIUS = 1024, RELBIAS_ROWS_MAX_D = 256;
inline size_t relbias_lds_bytes(int radius) { return (size_t)(2 * radius + 1 + 2 * FL_RELBIAS_PAD) * sizeof(float); }
inline SdpaKernel relbias_pick(bool half, int d, int radius, bool in_aligned, bool out_aligned8, const FlashStrides& sd, bool flash_on) {
    return half && flash_on && radius <= FL_RELBIAS_MAX_RADIUS && flash2_ok(d, in_aligned, out_aligned8, sd) ? SDPA_FLASH2 : SDPA_NAIVE;
}
// One wave's 32 query rows [qw0, qw0 + 32) against the 64 keys [kv0, kv0 + 64): delta = key - row spans
// [kv0 - qw0 - 31, kv0 - qw0 + 63].  Entirely at or below -radius (far left) or at or above +radius (far right) the bias is one
// value for the whole wave; anything else gathers from the padded row.
enum RelbiasTile { RELBIAS_FAR_LEFT = 0, RELBIAS_NEAR = 1, RELBIAS_FAR_RIGHT = 2 };
__host__ __device__ inline RelbiasTile relbias_tile_class(int kv0, int qw0, int radius) {
    const int rel = kv0 - qw0;
    return rel + FL_BKV - 1 <= -radius ? RELBIAS_FAR_LEFT : (rel - 31 >= radius ? RELBIAS_FAR_RIGHT : RELBIAS_NEAR);
}

// KV runs per query tile of the second-generation kernels: enough workgroups for two per CU (the kernels' occupancy), never more
// runs than the shortest useful run of two KV tiles allows for the heaviest query tile.  cus: device_cu_count()
inline int flash_nsplit(int nqt, int hq, int kv_len, int cus) {
    int nsplit = 1;
    const long long wgs = (long long)nqt * hq;
    while (nsplit < 4 && wgs * nsplit < 2LL * cus && ceil_div(kv_len, FL_BKV) >= 4 * (nsplit * 2)) nsplit *= 2;
    return nsplit;
}

// One launch of a second-generation kernel (16-bit tensors): its grid factors and its workspace, one stream-ordered allocation of
// `bytes` carved into V^T [Hkv][D][kv_pad] at 0 | partial O | (m, l) (both only when nsplit > 1) | extra_bytes of the caller's own,
// every region a multiple of 256 bytes.  kv_seen: the keys the heaviest query tile walks, which is what the split is sized by.
struct FlashPlan {
    int kv_pad, nqt, nsplit;
    size_t po_off, ml_off, extra_off, bytes;
};
inline FlashPlan flash_plan(int hq, int hkv, int q_len, int kv_len, int kv_seen, int d, int cus, size_t extra_bytes = 0) {
    auto up256 = [](size_t n) { return (n + 255) & ~(size_t)255; };
    FlashPlan p;
    p.kv_pad = ceil_div(kv_len, 64) * 64;
    p.nqt = ceil_div(q_len, FL_BQ);
    p.nsplit = flash_nsplit(p.nqt, hq, kv_seen, cus);
    p.po_off = up256((size_t)hkv * d * p.kv_pad * 2);
    p.ml_off = p.po_off + (p.nsplit > 1 ? up256((size_t)p.nsplit * q_len * hq * d * 2) : 0);
    p.extra_off = p.ml_off + (p.nsplit > 1 ? up256((size_t)p.nsplit * hq * q_len * 2 * sizeof(float)) : 0);
    p.bytes = p.extra_off + up256(extra_bytes);
    return p;
}

// ---- entry points across the family's translation units -----------------------------------------------------------------------
bool sdpa_flash_enabled();   // ops_attention.hip: PYGPUKIT_FLASH_ATTENTION, for the engine's direct use of flash_prefill_q8

// ops_flash.hip, flash_fwd_kernel with each policy; the callers have checked the arguments.  dt16: 0 = bf16, 1 = f16
pgk_status flash_prefill(const void* q, const void* k, const void* v, void* out, int hq, int hkv, int q_len, int kv_len, int d, float scale,
                         const FlashStrides& sd, int dt16, hipStream_t st);
pgk_status flash_prefill_full(const void* q, const void* k, const void* v, void* out, int hq, int hkv, int q_len, int kv_len, int d,
                              float scale, const FlashStrides& sd, int dt16, hipStream_t st);
pgk_status flash_prefill_irope(const void* q, const void* k, const void* v, const void* positions, void* out, int hq, int hkv, int q_len,
                               int kv_len, int d, float attn_scale, float floor_scale, int causal_offset, const FlashStrides& sd,
                               int pos_is_i64, int dt16, hipStream_t st);
pgk_status flash_prefill_alibi(const void* q, const void* k, const void* v, const float* slopes, void* out, int hq, int hkv, int q_len,
                               int kv_len, int d, float scale, const FlashStrides& sd, int dt16, hipStream_t st);
pgk_status flash_prefill_q8(const void* q, const void* k, const void* v, uint8_t* q8, float* q8s, int hq, int hkv, int q_len, int kv_len,
                            float scale, long long qh, long long qs, long long kh, long long ks, hipStream_t st);
// table: [hq][2 * radius + 1] fp32 on the device, 0 <= radius <= FL_RELBIAS_MAX_RADIUS; scale > 0; any q_len, kv_len >= 1
pgk_status flash_prefill_relbias(const void* q, const void* k, const void* v, const float* table, void* out, int hq, int hkv, int q_len,
                                 int kv_len, int d, int radius, float scale, const FlashStrides& sd, int dt16, hipStream_t st);

}  // namespace pgk
