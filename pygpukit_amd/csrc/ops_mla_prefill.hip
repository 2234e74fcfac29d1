// Multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi-K2), causal attention of a PROMPT CHUNK in the decompressed (non-absorbed)
// form: contraction 192 = 128 no-position + 64 rope dims, values 128 wide - (576 + 512) / (192 + 128) = 3.4 times less arithmetic
// per (query, key, head) than the absorbed form of ops_mla.hip, which is the decode tool.
//   pgk_sdpa_mla_prefill   out[i][h] = sum_j softmax_j(scale (<q_nope[i][h], kv[j][h][:128]> + <q_pe[i][h], cache[j][512:]>)) kv[j][h][128:]
//                          over j <= kv_len - q_len + i
// The operands are what the layer's GEMMs leave: q_nope [S][H][128], q_pe [S][H][64] (roped), kv [T][H][256] = kv_b_proj of the
// latent rows 0 .. T - 1 with k_nope and v interleaved per head as the HF weight has them, and the latent cache [max_seq][576], of
// which only the 64 rope columns of rows 0 .. T - 1 are read.  No pack, no concatenated K, no V^T pre-pass, no workspace.
//
// The kernel (mla_prefill_kernel).  One workgroup of 4 waves owns 128 query rows of one head, a wave 32 of them, a lane ONE row for
// the whole walk (the orientation of flash_fwd_kernel and paged_prefill_kernel):
//   S^T = K . Q^T           v_mfma_f32_32x32x16, 12 k-steps over 192, two 32-key halves of a 64-key tile; the B operand Q^T stays in 48
//                           VGPRs for the whole walk, premultiplied by scale * log2(e) (one more rounding to 16 bits, as the flash
//                           kernels), so the scores leave the MFMA in the exp2 domain;
//   online softmax          fp32, exp2 domain, deferred rescale (the reference point moves only when the maximum grew by more than 6);
//   O^T += V^T . P^T        4 k-steps of 16 keys x 4 tiles of 32 value dims (64 fp32 accumulators); the B operand is the probabilities
//                           packed to 16 bits straight from the score registers, the A operand V^T comes out of the ROW-MAJOR V
//                           image through ds_read_b64_tr_b16, as mla_decode_kernel reads C^T.
// K image of a tile: [64][192] 16-bit, columns 0 .. 127 from this head's kv rows (256 of the 512 bytes a head owns in a [T][H * 256]
// row), columns 128 .. 191 from the cache's rope columns - the same bytes for every head, so all but the first head's reads of them
// hit the L2.  Rows are 384 bytes = 24 sixteen-byte chunks, 1.5 sweeps of the 64 banks: chunk c of row r sits at chunk
// c ^ ((r >> 1) & 7), which keeps it in its group of 8 and puts the same chunk of 16 consecutive rows on 16 different bank quads
// (bit 3 of the slot alternates with the row's parity by the pitch alone, the low three bits by the XOR).  Padding the row to 400
// bytes would do the same and cost 1 KiB per image - with two images that is the difference between two workgroups per CU and one.
// V image: [64][128] row-major with paged_prefill_kernel's segment swizzle (segment g of row r at g ^ (r & 3)).
// Pipelining: both images are DOUBLE BUFFERED (2 x 40 KiB = 80 KiB, exactly two workgroups in a CU's 160 KiB) and the ten 16-byte
// chunks a thread stages of tile t + 1 are in flight in registers under the MFMAs of tile t: one barrier per tile.  The
// alternative, one image and the next tile in registers only (mla_decode_kernel), needs two more barriers per tile and gains no
// occupancy: the registers (Q 48 + O 64 + S 32 + staging 40) already bound the kernel to two waves per SIMD.
// Mask: the walk ends at the last tile the workgroup's last row sees; a wave skips a tile that lies above all of its rows; only a
// tile that some row's limit falls into (the diagonal, and the ragged last tile) takes the select branch.  Image rows at or beyond
// the walk's end (never past kv_len) are not loaded: zero in K AND in V - 0 x NaN inside an MFMA is NaN - and masked by select.
// Query rows past q_len compute a copy of the last row and are not stored; every row below q_len is stored.
// Workgroup ids are re-dealt head fastest, query tiles from the last down: the dispatcher deals consecutive ids to the 8 XCDs in
// turn, so with H a multiple of 8 a head's kv stream is served by one L2, and the heaviest tiles start first.
// No KV split: a chunk of a few rows over a long prefix is one workgroup's walk per head - sdpa_mla_fixed_cache is that tool.

#include "flash_common.hip.h"
#include "pgk_internal.h"

namespace pgk {

constexpr int MLAP_KROWB = MLAP_QK * 2;                      // 384 bytes per K image row
constexpr int MLAP_KIMG = MLAP_BKV * MLAP_KROWB;             // 24576
constexpr int MLAP_VIMG = MLAP_BKV * MLAP_V * 2;             // 16384
constexpr int MLAP_LDS = 2 * (MLAP_KIMG + MLAP_VIMG);        // K[2] | V[2]
constexpr int MLAP_KVROW = MLAP_NOPE + MLAP_V;               // elements of one head in a kv row
static_assert(MLAP_BQ == 128 && MLAP_BKV == 64 && MLAP_NOPE == 128 && MLAP_V == 128 && MLA_ROPE == 64, "mla prefill tile");

__device__ __forceinline__ int mlap_k_off(int r, int c) { return r * MLAP_KROWB + ((c ^ ((r >> 1) & 7)) << 4); }
__device__ __forceinline__ int mlap_v_off(int r, int c) { return r * (2 * MLAP_V) + (((c >> 2) ^ (r & 3)) << 6) + ((c & 3) << 4); }

typedef short mlap_v4s __attribute__((ext_vector_type(4)));

template <class T>
__global__ __launch_bounds__(256, 2) void mla_prefill_kernel(const T* q_nope, const T* q_pe, const T* kv, const T* cache, T* out, int heads,
                                                          int q_len, int kv_len, float scale_log2e) {
    constexpr int KS = MLAP_QK / 16, KSN = MLAP_NOPE / 16, DT = MLAP_V / 32;
    extern __shared__ __attribute__((aligned(16))) char mlap_smem[];
    const int wg = blockIdx.x + gridDim.x * blockIdx.y;
    const int head = wg % heads, row0 = ((int)gridDim.x - 1 - wg / heads) * MLAP_BQ;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, ql = lane & 31, h = lane >> 5;
    const int moff = kv_len - q_len;                         // query row i sees key j <= moff + i
    const int wrow0 = row0 + wid * 32, row_raw = wrow0 + ql, row = min(row_raw, q_len - 1);
    const int lim = moff + row;                              // last visible key of this lane's row (<= kv_len - 1)
    const int lim_first = moff + min(wrow0, q_len - 1), lim_last = moff + min(wrow0 + 31, q_len - 1);      // wave-uniform
    const bool wave_live = wrow0 < q_len;
    const int kv_end = moff + min(row0 + MLAP_BQ - 1, q_len - 1) + 1;      // keys the workgroup's last live row sees (1 .. kv_len)
    const int nt = (kv_end + MLAP_BKV - 1) / MLAP_BKV;

    // Q^T fragments (B operand): lane = query row, k-step ks covers depth 16 ks + 8 h .. + 7; steps 0 .. 7 q_nope, 8 .. 11 q_pe
    uint4 qf[KS];
    {
        const size_t rh = (size_t)row * heads + head;
        const T* qn = q_nope + rh * MLAP_NOPE + 8 * h;
        const T* qp = q_pe + rh * MLA_ROPE + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            Vec<T> v;
            v.load(ks < KSN ? qn + ks * 16 : qp + (ks - KSN) * 16);
            float f[8];
            v.to_float(f);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] *= scale_log2e;
            v.from_float(f);
            qf[ks] = v.raw;
        }
    }
    f32x16_fl o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // ---- staging: of a tile's 64 rows a thread takes chunk sc of k_nope and of v of rows sr + 16 i (i < 4) and chunk rc of the rope
    // key of rows rr + 32 i (i < 2).  Named registers, not arrays: an array of staged chunks tends to end up in scratch memory.
    const int sr = tid >> 4, sc = tid & 15, rr = tid >> 3, rc = tid & 7;
    const T* kv_head = kv + (size_t)head * MLAP_KVROW + sc * 8;
    const T* kpe = cache + MLA_LATENT + rc * 8;
    const size_t kv_pitch = (size_t)heads * MLAP_KVROW;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    uint4 kn0, kn1, kn2, kn3, vv0, vv1, vv2, vv3, kr0, kr1;
    auto kv_row = [&](int r, uint4& k, uint4& v) {
        k = zero4;
        v = zero4;
        if (r < kv_end) {
            const T* p = kv_head + (size_t)r * kv_pitch;
            k = *reinterpret_cast<const uint4*>(p);
            v = *reinterpret_cast<const uint4*>(p + MLAP_NOPE);
        }
    };
    auto pe_row = [&](int r, uint4& k) {
        k = zero4;
        if (r < kv_end) k = *reinterpret_cast<const uint4*>(kpe + (size_t)r * MLA_WIDTH);
    };
    auto load_tile = [&](int t) {
        const int r = t * MLAP_BKV + sr, p = t * MLAP_BKV + rr;
        kv_row(r, kn0, vv0);
        kv_row(r + 16, kn1, vv1);
        kv_row(r + 32, kn2, vv2);
        kv_row(r + 48, kn3, vv3);
        pe_row(p, kr0);
        pe_row(p + 32, kr1);
    };
    auto store_tile = [&](int buf) {
        char* kb = mlap_smem + buf * MLAP_KIMG;
        char* vb = mlap_smem + 2 * MLAP_KIMG + buf * MLAP_VIMG;
        *reinterpret_cast<uint4*>(kb + mlap_k_off(sr, sc)) = kn0;
        *reinterpret_cast<uint4*>(kb + mlap_k_off(sr + 16, sc)) = kn1;
        *reinterpret_cast<uint4*>(kb + mlap_k_off(sr + 32, sc)) = kn2;
        *reinterpret_cast<uint4*>(kb + mlap_k_off(sr + 48, sc)) = kn3;
        *reinterpret_cast<uint4*>(kb + mlap_k_off(rr, 16 + rc)) = kr0;
        *reinterpret_cast<uint4*>(kb + mlap_k_off(rr + 32, 16 + rc)) = kr1;
        *reinterpret_cast<uint4*>(vb + mlap_v_off(sr, sc)) = vv0;
        *reinterpret_cast<uint4*>(vb + mlap_v_off(sr + 16, sc)) = vv1;
        *reinterpret_cast<uint4*>(vb + mlap_v_off(sr + 32, sc)) = vv2;
        *reinterpret_cast<uint4*>(vb + mlap_v_off(sr + 48, sc)) = vv3;
    };
    // A operand of S^T: row ql (and 32 + ql, whose swizzle term is the same), chunk 2 ks + h.  The chunk's low three bits are
    // (2 ks & 7) ^ h ^ swizzle: four per-lane bases, the group of 8 a literal
    int koff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) koff[j] = ql * MLAP_KROWB + (((2 * j) ^ h ^ ((ql >> 1) & 7)) << 4);
    // V^T fragment of (k-step s, half u, dim tile i): paged_prefill_kernel's transposing read - the 16 lanes of a quarter-wave read
    // the 4 x 16 block of rows 16 s + 8 u + 4 h + (0..3), dims 32 i + 16 (ql >> 4) + (0..15)
    int voff[DT];
    {
        const int l15 = lane & 15, r = 4 * h + (l15 >> 2);
#pragma unroll
        for (int i = 0; i < DT; ++i) voff[i] = r * (2 * MLAP_V) + ((i ^ (r & 3)) << 6) + 32 * (ql >> 4) + 8 * (l15 & 3);
    }

    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1, kv0 = t * MLAP_BKV;
        if (t + 1 < nt) load_tile(t + 1);
        if (wave_live && kv0 <= lim_last) {                  // else the tile is above every row of this wave (wave-uniform)
            const char* kb = mlap_smem + buf * MLAP_KIMG;
            const char* vb = mlap_smem + 2 * MLAP_KIMG + buf * MLAP_VIMG;
            f32x16_fl s0, s1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int a = koff[ks & 3] + (ks >> 2) * 128;
                s0 = mfma32<T>(*reinterpret_cast<const uint4*>(kb + a), qf[ks], s0);
                s1 = mfma32<T>(*reinterpret_cast<const uint4*>(kb + a + 32 * MLAP_KROWB), qf[ks], s1);
            }
            // this lane holds keys (r & 3) + 8 (r >> 2) + 4 h of each 32-key half; masked by select, never by arithmetic
            if (kv0 + MLAP_BKV - 1 > lim_first) {            // some row's limit falls inside the tile (covers the ragged end)
                const int ll = lim - kv0 - 4 * h;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kvl = (r & 3) + 8 * (r >> 2);
                    s0[r] = kvl <= ll ? s0[r] : -INFINITY;
                    s1[r] = 32 + kvl <= ll ? s1[r] : -INFINITY;
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(fmaxf(s0[r], s1[r]), fmaxf(s0[r + 1], s1[r + 1])), mx);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = (mx > m_run + 6.0f || m_run == -INFINITY) ? fmaxf(m_run, mx) : m_run;       // so p <= 64
            const float m_use = m_new == -INFINITY ? 0.f : m_new;       // nothing visible so far: p = exp2(-inf) = 0
            const bool moved = __builtin_amdgcn_ballot_w64(m_new != m_run) != 0;
            const float alpha = moved ? __builtin_amdgcn_exp2f(m_run - m_use) : 1.0f;
            float ls = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s0[r] = __builtin_amdgcn_exp2f(s0[r] - m_use);
                s1[r] = __builtin_amdgcn_exp2f(s1[r] - m_use);
                ls += s0[r] + s1[r];
            }
            l_run = l_run * alpha + ls;
            m_run = m_new;
            if (moved) {
#pragma unroll
                for (int i = 0; i < DT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
            }
            // O^T += V^T . P^T: 4 k-steps of 16 keys; element j of the B operand is key 16 s + 8 (j >> 2) + 4 h + (j & 3)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const f32x16_fl& p = s < 2 ? s0 : s1;
                const int b = 8 * (s & 1);
                const uint4 pb = make_uint4(pack16x2<T>(p[b + 0], p[b + 1]), pack16x2<T>(p[b + 2], p[b + 3]),
                                            pack16x2<T>(p[b + 4], p[b + 5]), pack16x2<T>(p[b + 6], p[b + 7]));
#pragma unroll
                for (int i = 0; i < DT; ++i) {
                    const mlap_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) mlap_v4s*)(vb + voff[i] + (16 * s) * (2 * MLAP_V)));
                    const mlap_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) mlap_v4s*)(vb + voff[i] + (16 * s + 8) * (2 * MLAP_V)));
                    const uint2 u0 = __builtin_bit_cast(uint2, lo), u1 = __builtin_bit_cast(uint2, hi);
                    o[i] = mfma32<T>(make_uint4(u0.x, u0.y, u1.x, u1.y), pb, o[i]);
                }
            }
        }
        if (t + 1 < nt) store_tile(buf ^ 1);                 // the buffer every wave left before the barrier of tile t - 1
        __syncthreads();
    }

    // normalise and store: registers 4 g4 .. 4 g4 + 3 of tile i are value dims 32 i + 8 g4 + 4 h .. + 3 of this lane's row
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (row_raw >= q_len) return;
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    T* orow = out + ((size_t)row * heads + head) * MLAP_V + 4 * h;
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            uint2 x;
            x.x = pack16x2<T>(o[i][4 * g4] * inv, o[i][4 * g4 + 1] * inv);
            x.y = pack16x2<T>(o[i][4 * g4 + 2] * inv, o[i][4 * g4 + 3] * inv);
            *reinterpret_cast<uint2*>(orow + i * 32 + 8 * g4) = x;
        }
}

template <class T>
static pgk_status launch_mla_prefill(const void* q_nope, const void* q_pe, const void* kv, const void* cache, void* out, int heads, int q_len,
                                     int kv_len, float scale, hipStream_t st) {
    return launch_dyn_lds<mla_prefill_kernel<T>>(dim3(mla_prefill_tiles(q_len), heads), 256, MLAP_LDS, true, st, (const T*)q_nope, (const T*)q_pe,
                                                 (const T*)kv, (const T*)cache, (T*)out, heads, q_len, kv_len, scale * 1.4426950408889634f);
}

}  // namespace pgk

using namespace pgk;

extern "C" {

const char* pgk_sdpa_mla_prefill_plan(int num_heads, int q_len, int kv_len, pgk_dtype dt, int* grid) {
    if (const char* why = mla_prefill_refusal(num_heads, q_len, kv_len, dt == PGK_BF16 || dt == PGK_F16)) {
        set_error(PGK_ERR_INVALID, "pgk_sdpa_mla_prefill_plan: %s (heads %d, q_len %d, kv_len %d, dtype %d)", why, num_heads, q_len, kv_len, (int)dt);
        return nullptr;
    }
    if (grid) {
        grid[0] = mla_prefill_tiles(q_len);
        grid[1] = num_heads;
    }
    return "mla_prefill_mfma";
}

pgk_status pgk_sdpa_mla_prefill(const void* q_nope, const void* q_pe, const void* kv, const void* cache, void* out, int num_heads, int q_len,
                                int kv_len, int max_seq, float scale, pgk_dtype dt, pgk_stream s) {
    PGK_REQUIRE(q_nope && q_pe && kv && cache && out, "pgk_sdpa_mla_prefill: null pointer");
    const char* why = mla_prefill_refusal(num_heads, q_len, kv_len, dt == PGK_BF16 || dt == PGK_F16);
    PGK_REQUIRE(!why, "pgk_sdpa_mla_prefill: %s (heads %d, q_len %d, kv_len %d, dtype %d)", why, num_heads, q_len, kv_len, (int)dt);
    PGK_REQUIRE(kv_len <= max_seq, "pgk_sdpa_mla_prefill: kv_len %d beyond the cache of %d rows", kv_len, max_seq);
    PGK_REQUIRE(scale > 0.f, "pgk_sdpa_mla_prefill: scale must be positive (the model's mscale^2 / sqrt(192) has no default), got %g", (double)scale);
    PGK_REQUIRE(aligned16(q_nope) && aligned16(q_pe) && aligned16(kv) && aligned16(cache) && aligned16(out),
                "pgk_sdpa_mla_prefill: q_nope, q_pe, kv, cache and out must be 16-byte aligned");
    hipStream_t st = resolve_stream(s);
    if (dt == PGK_BF16) return launch_mla_prefill<bf16>(q_nope, q_pe, kv, cache, out, num_heads, q_len, kv_len, scale, st);
    return launch_mla_prefill<f16>(q_nope, q_pe, kv, cache, out, num_heads, q_len, kv_len, scale, st);
}

}  // extern "C"
