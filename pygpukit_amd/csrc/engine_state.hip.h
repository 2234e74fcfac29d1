// The native engine's host state and the small pure helpers every engine translation unit shares.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "engine_common.hip.h"

namespace pgk {

constexpr int SHORT_CTX = 512;   // contexts up to here take the whole-context attention kernels (direct batch attention); one sequence: SHORT_CTX_B1
constexpr int SHORT_CTX_B1 = 384; // a single sequence's fused attention + o_proj kernel walks the context in chunks of 192 rows (AM_CHUNK) in EVERY one of its
                                  // 256 workgroups: two chunks still beat the split-KV sequence (context 300: 0.616 vs 0.625 ms per step), three do not (400: 0.678 vs 0.627)

struct Engine {
    pgk_model_config_t cfg;
    const bf16 *embed, *lm_head, *final_norm;
    std::vector<pgk_layer_weights_t> layers;
    int nsplit = 1, lm_blocks = 1, lm_cap = 1, log_cap = 4096;
    bool batched_mfma = true;   // chunks of 3 and 5..16 sequences use engine_batched.hip.h (PGK_BATCHED_MFMA=0: GEMV kernels only, =2: from 3 up)
    int batched_min = 5, batched_max = 64;   // PGK_BATCHED_MAX=16: chunks of at most 16 sequences (one weight pass per chunk), the A/B switch of the tiled kernels
    int cu_count = 256;
    bool short_path = true;     // contexts <= SHORT_CTX take the whole-context attention kernels (PGK_FUSED_ATTN=0: the split-KV sequence at every context)
    int pos_hi = -1;            // host-side upper bound of the largest position the next step sees (-1: unknown); selects the sequence, see step_is_short
    // in-graph stochastic sampling (pgk_engine_set_sampling): temperature <= 0 keeps greedy argmax
    float sample_temperature = 0.f, sample_top_p = 1.f;
    int sample_top_k = 0, u_cap = 0, u_alloc_rows = 0;   // u_cap: rows in use (ring length); u_alloc_rows: rows allocated
    float* u_ring = nullptr;       // [u_cap][max_batch] uniforms, row = step counter % u_cap
    void* sample_scratch = nullptr;   // top-k candidate keys (ops_sampling.hip), sized for max_batch rows
    size_t sample_scratch_cap = 0;
    int32_t* sampled = nullptr;    // [max_batch]
    bool fused_attn = false;   // one sequence at short context: attn + o_proj in one kernel (bf16 W_o, shapes that tile)
    bool attn_mfma = false;    // ... with Q.K^T and P.V on the matrix pipe from LDS-staged K/V (head_dim 128; PGK_ATTN_MFMA=0: the dot2 kernels); also the whole-context
                               // batch attention while its workgroups (96 KB of LDS: one per CU) fit one round - batch x Hkv <= CUs (beyond: attn_decode_kernel, batch 64 1.258 vs 1.316 ms)
    bool merged_oproj = false; // long contexts / fp8 W_o, one or two sequences: split-KV merge + o_proj in one kernel (PGK_MERGED_OPROJ=0: merge kernel + GEMV)
    int moproj_rows = 32;
    int oproj_rows = 32;       // W_o rows per workgroup on the fused path
    // device state
    bf16 *kcache = nullptr, *vcache = nullptr;
    float *rope_cos = nullptr, *rope_sin = nullptr, *cur_cos = nullptr, *cur_sin = nullptr;
    int32_t *tokens = nullptr, *positions = nullptr, *token_log = nullptr, *step_counter = nullptr;
    bf16 *act16 = nullptr, *attnv16 = nullptr;   // batched MFMA path: bf16 hand-off of SwiGLU output and attention output
    bf16* x16 = nullptr;                         // 17..64 sequences: the next RMSNorm's input rows in bf16 (layer 0: normalised by norm_rows_bf16; then un-normalised, written by o_proj / down)
    float* ss_part = nullptr;                    // ... and its statistic: per-workgroup sums of squares [64][1024]
    float *h = nullptr, *h2 = nullptr, *qkv = nullptr, *part = nullptr, *opart = nullptr, *attnv = nullptr, *act = nullptr, *logits = nullptr,
          *amax_val = nullptr;
    int* amax_idx = nullptr;
    unsigned long long* clk_log = nullptr;
    size_t kv_bytes = 0, ws_bytes = 0;
    // fragment-major copies of the layer weights for prompts of <= 128 tokens (ops_pkgemm.hip); PGK_PACKED_PREFILL=0: none
    struct PackedLayer { bf16 *qkv = nullptr, *o = nullptr, *gate_up = nullptr, *down = nullptr; };
    std::vector<PackedLayer> packed;
    bool packed_ok = false;     // the skinny-GEMM kernels of ops_pkgemm.hip can use the copy (their shape limits)
    bool packed_have = false;   // the copy exists (w8a16 engines: also for shapes beyond those kernels - the long-prompt GEMMs read it)
    size_t packed_bytes = 0;
    bool packed_resid = false;      // o_proj / down_proj without K split, carrying the next RMSNorm (pkgemm_resid_nt) where pkgemm_resid_ok takes both shapes; otherwise split-K slabs + norm launches
    float* pk_ss = nullptr;         // its sum-of-squares table [128][PK_SS_LD]
    bf16* packed_lm = nullptr;      // fragment-major lm_head for the batched (3..64 sequences) lm_head kernels (vocabularies of whole 16-row groups, max_batch >= 3)
    float* dec_slabs = nullptr;     // 17..64 sequences on the packed kernels: split-K slabs of o_proj / down_proj [splits][M][H] (PGK_PACKED_DECODE=0: engine_batched kernels)
    bool packed_decode = false;
    // NVF4 engines (weight_format 3): ONE layer's linears dequantised to row-major bf16 [qkv | o | gate_up | down], refilled
    // by the prefill in front of every layer's projections (never a copy of all layers)
    bf16* nv_deq = nullptr;
    // prefill workspace (grown on demand, outside capture)
    void* pf = nullptr;
    size_t pf_bytes = 0;
    int32_t* pf_tokens = nullptr;
    int pf_tokens_cap = 0;
    // captured steps: tier 0 = the short-context sequence (span 0); the others = the split-KV sequence with its slices cut for
    // contexts up to `span` positions (1024, 2048, ... and the cache length).  pgk_engine_replay picks per step (pick_tier).
    struct Tier { int span = 0; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; int launches = 0; };
    std::vector<Tier> tiers;
    int graph_batch = 0;
    int step_span = 0;          // the split-KV slicing of the step being enqueued (launch_attn); 0: the whole cache
    int launches_per_step = 0;
    std::vector<void*> allocs;

    size_t kv_layer_elems() const { return (size_t)cfg.max_batch * cfg.num_kv_heads * cfg.max_seq_len * cfg.head_dim; }
    int qkv_dim() const { return (cfg.num_heads + 2 * cfg.num_kv_heads) * cfg.head_dim; }
};

// a PGK_* switch that is on unless the environment sets it to 0
inline bool env_on(const char* name) {
    const char* v = getenv(name);
    return !(v && atoi(v) == 0);
}

inline pgk_status dev_alloc(Engine* e, void** p, size_t bytes, size_t* acct) {
    if (pgk_status r = pgk_malloc(p, bytes)) return r;
    e->allocs.push_back(*p);
    if (acct) *acct += bytes;
    return PGK_OK;
}

// Which launch sequence the NEXT step takes: the short-context one while the host-side bound on the step's largest
// position (set by pgk_engine_set_state, advanced by every step this library enqueues) stays below SHORT_CTX.  The bound
// is a speed hint only - both sequences are correct at any context - so a caller that rewrites the device-resident
// positions behind the library's back loses speed, never correctness; an unknown bound selects the long sequence.
inline int short_limit(int batch) { return batch == 1 ? SHORT_CTX_B1 : SHORT_CTX; }
inline bool step_is_short_at(const Engine* e, int batch, int pos_hi) { return e->short_path && pos_hi >= 0 && pos_hi + 1 <= short_limit(batch); }
inline bool step_is_short(const Engine* e, int batch) { return step_is_short_at(e, batch, e->pos_hi); }

// The split-KV slicing a step at the host-side position bound needs: the smallest of 1024, 2048, ... that covers the context, capped at
// the cache length (an unknown bound: the cache length).
inline int span_for_at(const Engine* e, int pos_hi) {
    const int cap = e->cfg.max_seq_len;
    if (pos_hi < 0) return cap;
    int span = 1024;
    while (span < pos_hi + 1 && span < cap) span *= 2;
    return span < cap ? span : cap;
}
inline int span_for(const Engine* e) { return span_for_at(e, e->pos_hi); }

// The captured step the next replay takes: the short-context sequence while the position bound allows it (and it was captured),
// otherwise the split-KV tier whose slices cover the context; both kinds are correct at any context they cover.
inline size_t pick_tier(const Engine* e) {
    const bool has_short = !e->tiers.empty() && e->tiers[0].span == 0;
    if (has_short && (e->tiers.size() == 1 || step_is_short(e, e->graph_batch))) return 0;
    const int want = span_for(e);
    for (size_t i = has_short ? 1 : 0; i < e->tiers.size(); ++i)
        if (e->tiers[i].span >= want) return i;
    return e->tiers.size() - 1;
}

// One decode chunk being enqueued: sequences [b0, b0 + M) of the step.  Every helper that enqueues adds to *launches at
// the point of its launch: `counted(n, launch(...))` (n == nullptr: the prefill, which keeps no count).
struct StepCtx { Engine* e; int b0, M; hipStream_t st; int* launches; bool short_ctx; };
inline pgk_status counted(int* launches, pgk_status r) {
    if (launches) ++*launches;
    return r;
}

// ---- the step's decisions as pure functions of the engine's host state: the launchers call them, and so does the read-only
// plan query (pgk_engine_attn_plan), which therefore names what a step would launch without restating any of it ----------

// How the step cuts its sequences into chunks: the next chunk of a step with `rem` sequences left.
enum ChunkForm { CF_GEMV = 0, CF_BATCHED, CF_TILED, CF_PACKED };
struct ChunkChoice { ChunkForm form; int m; };
inline ChunkChoice next_chunk(const Engine* e, int rem) {
    // the MFMA projections cost the same for 3 as for 16 sequences (~1.0-1.2 ms per step on Qwen3-0.6B); the GEMV
    // kernels exist for M = 1, 2, 4, 8 only, so 3 / 5 / 6 / 7 sequences would take two or three weight passes there
    // (measured: 7 sequences 2.46 ms against 1.05).  GEMV stays for exactly 1, 2 and 4 (0.70 / 0.93 / 0.82 ms).
    // NVF4 (w4a16): GEMV chunks of <= 8 sequences only, each re-reading the weights; batched_mfma is off for it
    const bool mfma_ok = e->cfg.weight_format != 3 && e->batched_mfma && (rem >= e->batched_min || (e->batched_min == 5 && rem == 3));
    if (mfma_ok) {
        const int m = rem > e->batched_max ? e->batched_max : rem;
        return {m > 16 ? (e->packed_decode ? CF_PACKED : CF_TILED) : CF_BATCHED, m};
    }
    return {CF_GEMV, rem >= 8 ? 8 : rem >= 4 ? 4 : rem >= 2 ? 2 : 1};
}

// Which attention launch sequence a chunk of M sequences takes.  `fused`: attention + o_proj partials in one kernel (one
// sequence at short context); `direct`: one workgroup per (sequence, kv head) walks the whole (short) context and writes the
// normalised output (`direct_bf16`: as bf16 rows for an MFMA o_proj) - no merge launch; otherwise split-KV slices, then
// `merged` (merge + o_proj partials in one launch) or the merge kernel.
struct AttnFlags { bool fused, direct, direct_bf16, merged; };
inline AttnFlags attn_flags(const Engine* e, ChunkForm form, int M, bool short_ctx) {
    if (form != CF_GEMV) return {false, short_ctx && M >= 3, true, false};
    // fused attention+o_proj recomputes a KV head's attention in every row-slice workgroup: right for one
    // sequence at short context, wasteful for a batch.
    // (two sequences ran the fused kernel too until round 3: its 96-KB workgroups are one per CU, so 2 x 256 of them took two
    // rounds - 9.4 us per layer against 3.7 + 2.4 for whole-context attention + an o_proj GEMV: 0.80 -> 0.66 ms per step)
    const bool fused = e->fused_attn && short_ctx && M == 1;
    const bool direct = !fused && short_ctx && M >= 2;
    // long contexts (or fp8 W_o): split-KV slices, then merge + o_proj partials in one launch; the gate/up prologue adds them
    const bool merged = !fused && !direct && M <= 2 && e->merged_oproj;
    return {fused, direct, false, merged};
}

// GQA groups other than the instantiated 1 / 2 / 4 query heads per kv head run as several launches over head chunks of
// 4, 2 and 1 heads: the size of the chunk that starts at head `off` of a group of G.
inline bool group_instantiated(int G) { return G == 1 || G == 2 || G == 4; }
inline int head_chunk(int G, int off) { return group_instantiated(G) ? G : ((G - off >= 4) ? 4 : ((G - off >= 2) ? 2 : 1)); }

// ---- the projections' decisions, shared by their launchers and the read-only plan query (pgk_engine_linear_plan) ----------

// fused_gemv_kernel (engine_gemv.hip.h).  Weight kinds: the k elements one lane loads per trip (WTraits<WT>::NW).
enum { GEMV_NW_BF16 = 8, GEMV_NW_FP8 = 16, GEMV_NW_NVF4 = 32 };
// Rows per wave R of a projection with n_out outputs (SwiGLU: pairs): enough workgroups to cover 256 CUs even for the
// N = hidden projections.
inline int gemv_rows(int nw, int M, bool swiglu, int n_out, int K) {
    // NVF4, 4 / 8 sequences: 4 rows per wave hold 2 x R x M partial sums besides the activation fragments - 190 to 256
    // VGPRs, one wave per SIMD; 2 rows per wave stay near the bf16 kernels' ~120
    if (nw == GEMV_NW_NVF4 && M >= 4) return 2;
    if (swiglu) {
        // One sequence, mid-sized gate/up (Qwen3-0.6B: 3072 pairs): 3 pairs per wave = 256 workgroups, one per CU.  Every
        // workgroup's prologue re-reads h and the 8 o_proj partial vectors (36 KB from L2); with 768 two-pair workgroups that
        // was 108 KB per CU through the texture addresser against 49 KB of weights (gate/up span 4.32 -> 3.69 us, step 0.607
        // -> 0.592 ms; 4 pairs per wave = 384 workgroups: 4.28 us).  Needs the 6 rows x C chunks to fit the preload budget.
        if (M == 1 && n_out >= 2048 && n_out < 4096 && K % (64 * nw) == 0 && K / (64 * nw) <= 2) return 6;
        return n_out >= 4096 ? 4 : 2;
    }
    return n_out >= 4096 ? 4 : (n_out >= 2048 ? 2 : 1);
}
// Preload depth C of a row of K elements at R rows per wave: K / (64 * NW) chunks (NVF4: K / 1024, (C + 1) / 2 chunks per lane)
// when the row is short enough to sit in registers (R * C * 4 preload VGPRs <= 48) and the depth is instantiated; 0: the generic loop.
inline int gemv_preload(int nw, int R, int K) {
    const bool nv4 = nw == GEMV_NW_NVF4;
    const int unit = nv4 ? 1024 : 64 * nw;
    const int c = (K % unit == 0) ? K / unit : 0;
    const bool inst = c == 1 || c == 2 || c == 3 || c == 4 || c == 6;
    return inst && (nv4 ? (c + 1) / 2 : c) <= 12 / R ? c : 0;
}
// workgroups of a GEMV projection: 4 waves of R rows (SwiGLU: R / 2 pairs), at most 1024 (the lm_head forces its own count)
inline int gemv_grid(int R, bool swiglu, int n_out, int force_grid) {
    const int grid = force_grid ? force_grid : (n_out + (swiglu ? R / 2 : R) * 4 - 1) / ((swiglu ? R / 2 : R) * 4);
    return grid > 1024 ? 1024 : grid;
}

// engine_batched.hip.h, 3..16 sequences: register-resident activation fragments at the instantiated widths K = 128 x
// {8, 16, 24, 32} (batched_reg_kernel); every other multiple of 128 streams through the LDS-image kernel (batched_mfma_kernel),
// which is therefore never launched at those four widths
inline bool batched_is_reg(int K) { const int s = K / 128; return s == 8 || s == 16 || s == 24 || s == 32; }
// ... weight rows per workgroup of batched_reg_kernel: enough workgroups to pull HBM bandwidth - fewer weight rows per
// workgroup when N / 16 would leave CUs idle (the LDS-image kernel: always 16)
inline int batched_reg_rows(int N, bool logits) { return (logits || (N + 15) / 16 >= 192) ? 16 : ((N + 7) / 8 >= 192 ? 8 : 4); }
// ... 17..64 sequences (batched_mt_kernel): rows per workgroup and M tiles of 16 per workgroup
// (Tried for the N = hidden projections at batch 64: 16 rows per workgroup - 64 workgroups, a quarter of the activation
// traffic: 17.2 / 12.1 us against 15.5 / 11.1; and the weights of 16 rows parked in LDS with one wave per 16-row batch tile,
// no cross-wave reduction: 16.4 us average.  A workgroup keeps at most ~64 KB of loads in flight, so 64 workgroups cannot
// pull the 6 MB of weights plus their activation rows faster than 256 four-row workgroups that each re-read the rows.)
inline int mt_rows_per_group(int N, bool logits) { return (logits || (N + 15) / 16 >= 192) ? 16 : 4; }
inline int mt_tiles(int M) { return M <= 32 ? 2 : 4; }
// ... both read the fragment-major copy only with bf16 weights and 16-row workgroups (whole 16-row groups; a ragged last group reads row-major)
inline bool batched_reads_copy(bool fp8, int rows_per_group, bool have_copy) { return !fp8 && rows_per_group == 16 && have_copy; }
// ... of the layer's QKV and gate / up matrices where the engine holds one (o_proj / down_proj: none); the lm_head: packed_lm
inline bool batched_layer_copy(const Engine* e, bool fp8) { return !fp8 && e->packed_ok; }
// argmax partial blocks per sequence of the batched lm_head
inline int batched_lm_blocks(int vocab) { const int g = (vocab + 15) / 16; return g < 2048 ? g : 2048; }

// pgk_engine_prefill's choices for a chunk of n tokens (engine_prefill.hip): which GEMM family each projection runs on, its
// split-K slabs and the fused epilogues.
struct PrefillChoice {
    bool ws;            // n <= 128: weight-streaming kernels (wsgemm_nt, or pkgemm_nt with `pk`)
    bool pk;            // ... on the fragment-major copy (ops_pkgemm.hip)
    bool pk_heads;      // ... with the QKV epilogue (head_dim 128)
    bool carried;       // ... o_proj / down_proj carry the next RMSNorm (pkgemm_resid_nt)
    bool pkd;           // n > 128, w8a16: the staged bf16 GEMMs read the dequantised fragment-major copy
    bool nv4, w16, gsplit, fp8, fp8act;
    bool fuse_epi, fuse_q, fuse_sw8, fuse_sw16, fuse_heads8, fuse_heads;
    int s_o, s_d, s_qkv, s_gu;   // wsgemm_nt split-K slabs
    int pk_so, pk_sd;            // pkgemm_nt split-K slabs of the N = hidden projections
    int g_so, g_sd;              // engine_gemm_nt_slabs split-K slabs of the N = hidden projections
};
PrefillChoice prefill_choice(const Engine* e, int n);

// Host entries the prefill and the decode step's packed path (one row per SEQUENCE) share; defined in engine_prefill.hip.
// h[r] += the *pending split-K slabs of the projection in front of this norm (then *pending = 0), x[r] = bf16(rmsnorm(h[r]) * gamma)
pgk_status rmsnorm_slabs(float* h, const bf16* gamma, bf16* x, int rows, int H, float eps, const float* slabs, int* pending, uint8_t* q8,
                         float* q8s, hipStream_t st, int* launches);
// packed path with carried norms, after attention: o_proj, gate_up, down_proj of `layer`
pgk_status packed_mlp_carried(Engine* e, int layer, int rows, const bf16* attn16, bf16* act16, float* h, bf16* x16, int* ss_n, hipStream_t st,
                              int* launches);

}  // namespace pgk
