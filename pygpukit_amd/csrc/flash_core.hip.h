// The tile walk of the second-generation flash prefill kernels, written once: flash_fwd_kernel (ops_flash.hip, 16-bit first
// product, five mask / bias policies) and flash_fwd_fp8_kernel (ops_flash_fp8.hip, e4m3 first product) differ in how a tile's
// scores S^T = K . Q^T are formed - the K image, the Q fragments, the MFMA - and share everything else, which lives here:
// the work mapping, V^T staging, one tile's mask + online softmax + P.V, the loop around them, the row store, and on the host
// the launch sequence (the workspace plan is attn_plan.h's flash_plan).  Every function is forceinline and compiled under the
// including file's flags (ops_flash_fp8.o alone is built with -fno-honor-nans, see the Makefile).
//
// Orientation: the scores are computed TRANSPOSED, S^T[kv][q] on a 32x32 MFMA, so a lane owns one query column (q = lane & 31)
// and its 16 accumulator registers per 32-kv sub-tile are kv rows.  Consequences:
//   * the online softmax (max, exp2, sum) of a query row is lane-local arithmetic over registers plus ONE exchange
//     with lane ^ 32 (the other half of the rows) - no LDS, no 16-lane butterflies;
//   * the probabilities are already laid out as the B operand of the second product O^T[d][q] += V^T[d][kv] . P^T[kv][q]:
//     registers 8s..8s+7 of a sub-tile, packed pairwise to 16-bit, ARE the k-step-s fragment (k order permuted:
//     element j of lane half h is kv = 16s + 8(j>>2) + 4h + (j&3)); the V^T operand is read in the same permuted
//     order (two 8-byte LDS reads per fragment), so P never touches LDS;
//   * alpha (the running-max rescale) and 1/l are per-lane scalars for the O^T accumulators (q is again the lane).
// V arrives transposed: a small pre-pass writes V^T [Hkv][D][kv_pad] (zero padded to a multiple of 64 positions) so
// that both LDS images are filled with 16-byte row-contiguous chunks.
// Workgroup = 4 waves = 128 query rows of one head; KV tiles of 64 positions, K and V^T [D][64] double buffered in LDS (64 KiB
// with 16-bit K at D = 128: two workgroups per CU).
#pragma once

#include "flash_common.hip.h"

namespace pgk {

// What a workgroup (and this wave of it) works on.  Workgroup id -> (kv head, query head in its group, query tile, KV run): all
// query heads of a kv head share id % Hkv, i.e. an XCD when Hkv is a multiple of 8, so the K / V stream of a head is served by
// one L2.  Heavy tiles first (causal: late query tiles see more keys) - and, when the launch is one round of two workgroups
// per CU (KV split), the second half of the ids in ASCENDING weight: a CU's two residents are then a heavy and a light run
// (ids i and i + grid / 2 sit on the same CU when the dispatcher deals one workgroup to every CU before the second).
struct FlashWork {
    int kvh, head, split, qt;
    int qw0;          // first query row of this wave
    int mask_off;     // kv_pos <= mask_off + q_pos is visible
};
__device__ __forceinline__ FlashWork flash_work(int hq, int hkv, int q_len, int nsplit, int mask_off) {
    FlashWork w;
    const int rep = hq / hkv, nqt = (q_len + FL_BQ - 1) / FL_BQ;
    const int id = blockIdx.x;
    const int rest = id / hkv;
    w.kvh = id % hkv;
    w.head = w.kvh * rep + rest % rep;
    int order = rest / rep;
    const int nord = nqt * nsplit;
    if (nsplit > 1 && order >= nord / 2) order = nord / 2 + (nord - 1 - order);
    w.split = order % nsplit;
    w.qt = nqt - 1 - order / nsplit;
    w.qw0 = w.qt * FL_BQ + (threadIdx.x >> 6) * 32;
    w.mask_off = mask_off;
    return w;
}

// V^T staging of one tile: global loads into NAMED registers (an array here ends up in scratch memory at this register
// pressure, see ops_fp8_gemm.hip), then the swizzled 8-byte LDS stores.  Chunk i of this thread is row vd + 32 i, 16-byte
// chunk vc of the tile; VCH = D / 32 chunks per thread.  A whole tile addresses its rows as (wave-uniform tile base) +
// (per-lane element offset fixed for the kernel), so the per-tile address arithmetic is scalar.
template <class T, int VCH> struct FlashVStage {
    static_assert(VCH == 2 || VCH == 4, "staging is written for D = 64 / 128");
    uint4 r0, r1, r2, r3;
    uint32_t vo0, vo_step;
    int vd, vc;
    __device__ __forceinline__ FlashVStage(int tid, int kv_pad)
        : vo0((uint32_t)((tid >> 3) * kv_pad + (tid & 7) * 8)), vo_step((uint32_t)(32 * kv_pad)), vd(tid >> 3), vc(tid & 7) {}
    __device__ __forceinline__ void load(const T* vh, int t) {      // vh: this kv head's V^T [D][kv_pad]
        const T* vtile = vh + t * FL_BKV;
        r0 = *reinterpret_cast<const uint4*>(vtile + vo0);
        r1 = *reinterpret_cast<const uint4*>(vtile + vo0 + vo_step);
        if constexpr (VCH == 4) {
            r2 = *reinterpret_cast<const uint4*>(vtile + vo0 + 2 * vo_step);
            r3 = *reinterpret_cast<const uint4*>(vtile + vo0 + 3 * vo_step);
        }
    }
    __device__ __forceinline__ void put(char* vb, int d, const uint4& x) const {
        *reinterpret_cast<uint2*>(vb + fl_v_off(d, 2 * vc)) = make_uint2(x.x, x.y);
        *reinterpret_cast<uint2*>(vb + fl_v_off(d, 2 * vc + 1)) = make_uint2(x.z, x.w);
    }
    __device__ __forceinline__ void store(char* vb) const {         // vb: the V^T image of the buffer being filled
        put(vb, vd, r0);
        put(vb, vd + 32, r1);
        if constexpr (VCH == 4) {
            put(vb, vd + 64, r2);
            put(vb, vd + 96, r3);
        }
    }
};

typedef uint32_t fl_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const volatile fl_u32x2* fl_lds_cv64;     // volatile drops the inferred address space: say it

// One live KV tile after its first product: mask, online softmax, O^T += V^T . P^T.  sc0 / sc1: S^T of the two 32-kv
// sub-tiles - this lane holds query w.qw0 + ql and kv rows (r&3) + 8(r>>2) + 4h of each.  SCALED = false: the scores are in
// the exp2 domain already.  SCALED = true (fp8): they are raw sums and cf > 0 takes them there; the maximum is taken on the raw
// sums (the maximum of the raw sums is the maximum of the scores) and cf rides in the exp2 argument as an FMA that replaces
// the subtraction of the running maximum.  vb: the V^T image of this tile's buffer.
template <class T, int DT, bool SCALED>
__device__ __forceinline__ void flash_softmax_pv(const FlashWork& w, int kv0, int kv_len, int ql, int h, f32x16_fl& sc0, f32x16_fl& sc1,
                                                 f32x16_fl (&o)[DT], float& m_run, float& l_run, const char* vb, float cf) {
    const bool need_mask = kv0 + FL_BKV - 1 > w.mask_off + w.qw0 || kv0 + FL_BKV > kv_len;   // wave-uniform
    const int lim = min(w.mask_off + w.qw0 + ql, kv_len - 1) - kv0 - 4 * h;                  // local kv row <= lim is visible
    float mx = -INFINITY;
    if (need_mask) {   // diagonal / ragged tiles only: a real wave-uniform branch, not 32 predicated selects per tile
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kvl = (r & 3) + 8 * (r >> 2);
            sc0[r] = kvl <= lim ? sc0[r] : -INFINITY;
            sc1[r] = 32 + kvl <= lim ? sc1[r] : -INFINITY;
        }
    }
    // (without -fno-honor-nans every operand of a max is first canonicalised with a v_max_f32 x, x, x of its own - 60 vector
    // instructions for 32 scores where 16 v_max3_f32 do: ops_flash_fp8.hip is built with the flag, ops_flash.hip without)
#pragma unroll
    for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(fmaxf(sc0[r], sc1[r]), fmaxf(sc0[r + 1], sc1[r + 1])), mx);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if constexpr (SCALED) mx *= cf;
    // Deferred rescale: the reference point of a row only moves when its maximum grew by more than 6 (log2 domain), so
    // probabilities stay <= 64 (exact in fp32 sums, fine in 16-bit P) and on most tiles - for the whole wave - alpha is
    // exactly 1 and the 64-multiply rescale of O is skipped.
    const float m_new = (mx > m_run + 6.0f || m_run == -INFINITY) ? fmaxf(m_run, mx) : m_run;
    const float m_use = m_new == -INFINITY ? 0.f : m_new;        // a fully masked row so far: p = exp2(-inf) = 0
    const bool moved = __builtin_amdgcn_ballot_w64(m_new != m_run) != 0;   // wave-uniform
    const float alpha = moved ? __builtin_amdgcn_exp2f(m_run - m_use) : 1.0f;   // m_run = -inf -> 0 (accumulators are 0 anyway)
    float ls = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if constexpr (SCALED) {
            sc0[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc0[r], cf, -m_use));
            sc1[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc1[r], cf, -m_use));
        } else {
            sc0[r] = __builtin_amdgcn_exp2f(sc0[r] - m_use);
            sc1[r] = __builtin_amdgcn_exp2f(sc1[r] - m_use);
        }
        ls += sc0[r] + sc1[r];
    }
    l_run = l_run * alpha + ls;
    m_run = m_new;
    if (moved) {
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
    }
    // ---- O^T += V^T . P^T : 4 k-steps of 16 kv ----
    // V^T fragment addresses: row d = 32 i + ql, 8-byte chunk c8 = 4 s + 2 u + h at d * 128 + ((c8 ^ ((d >> 1) & 15)) << 3).
    // 32 i is a multiple of 32, so the swizzle term depends on the lane and on c8 only: ONE address register per
    // (s, u) for this tile's buffer and the tile row i as the instruction's immediate offset (4096 i).  The reads are
    // VOLATILE: left ordinary, hipcc pairs those of tiles i and i + 2 into ds_read2st64_b64, which is served 16 lanes
    // at a time on a 32-bank modulus (2-way conflicts, half the rate); the first version kept them apart by laundering
    // every address through an empty asm - a v_mov + v_add per read, 64 vector instructions per tile.
    const char* vrow = vb + ql * 128;
    const int vsw = (ql >> 1) & 15;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        uint4 pb;
        if (s < 2) {
            pb = make_uint4(pack16x2<T>(sc0[8 * s + 0], sc0[8 * s + 1]), pack16x2<T>(sc0[8 * s + 2], sc0[8 * s + 3]),
                            pack16x2<T>(sc0[8 * s + 4], sc0[8 * s + 5]), pack16x2<T>(sc0[8 * s + 6], sc0[8 * s + 7]));
        } else {
            pb = make_uint4(pack16x2<T>(sc1[8 * (s - 2) + 0], sc1[8 * (s - 2) + 1]), pack16x2<T>(sc1[8 * (s - 2) + 2], sc1[8 * (s - 2) + 3]),
                            pack16x2<T>(sc1[8 * (s - 2) + 4], sc1[8 * (s - 2) + 5]), pack16x2<T>(sc1[8 * (s - 2) + 6], sc1[8 * (s - 2) + 7]));
        }
#pragma unroll
        for (int i = 0; i < DT; ++i) {
            // each 8-byte read stays a ds_read_b64 (two 32-lane halves, 64-bank modulus: the layout is conflict-free for it)
            const fl_u32x2 lo = *(fl_lds_cv64)(vrow + (((4 * s + h) ^ vsw) << 3) + i * 4096);
            const fl_u32x2 hi = *(fl_lds_cv64)(vrow + (((4 * s + 2 + h) ^ vsw) << 3) + i * 4096);
            o[i] = mfma32<T>(make_uint4(lo.x, lo.y, hi.x, hi.y), pb, o[i]);
        }
    }
}

// The walk over this workgroup's run of KV tiles [t0, t1): the keys its query tile can see, cut into nsplit runs.  (The bounds
// are computed here and not with the mapping above: their two 64-bit divisions, expanded ahead of the Q loads, cost 17 of the
// 21 kernels a block of 8 SGPRs, profiles/flash_share_isa.txt.)  One tile per iteration: S = K . Q^T, softmax, O += V . P; the global loads of tile
// t + 1 are issued before the MFMAs of tile t and parked in the other LDS buffer after them: one barrier per tile.  (Tried in
// round 3: multiplying S(t + 1) under the softmax of S(t).  As two conditional blocks hipcc keeps them apart - QK block, 64
// register copies, softmax - and the kernel lost 2 %; it needs a branch-free, two-tile-unrolled body to interleave.)
// The first product is the caller's: load_k(t) issues tile t's K loads into its named registers, store_k(buf) parks them in
// K image buf, qk(buf, kv0, s0, s1) forms S^T of the tile in buf.  retire_q() pins the Q fragments with an empty asm BEFORE
// the loop: if the Q loads are still counted as pending at the loop header, hipcc's conservative vmcnt bookkeeping waits for
// them in every iteration - behind the tile prefetch issued at the top of the loop, i.e. it drains the prefetch before the
// first MFMA.  vst is the caller's object, constructed beside its K staging registers: constructed here instead, hipcc pairs the
// prologue's V^T stores of the fp8 kernel differently (profiles/flash_share_isa.txt).  vs0: V^T image 0; image 1 follows it
// D * 128 bytes on.
template <class T, int DT, bool SCALED, class LoadK, class StoreK, class RetireQ, class QK>
__device__ __forceinline__ void flash_walk(const FlashWork& w, FlashVStage<T, DT>& vst, const T* vh, int q_len, int kv_len, int nsplit, int ql, int h, char* vs0,
                                           f32x16_fl (&o)[DT], float& m_run, float& l_run, float cf, LoadK&& load_k, StoreK&& store_k,
                                           RetireQ&& retire_q, QK&& qk) {
    constexpr int V_BYTES = DT * 32 * 128;
    const int q_last = min(w.qt * FL_BQ + FL_BQ - 1, q_len - 1);
    const int kv_end = min(kv_len, w.mask_off + q_last + 1);
    const int nt_all = (kv_end + FL_BKV - 1) / FL_BKV;
    const int t0 = (int)((long long)nt_all * w.split / nsplit), t1 = (int)((long long)nt_all * (w.split + 1) / nsplit);
    f32x16_fl sc0, sc1;
    if (t0 < t1) {
        load_k(t0);
        vst.load(vh, t0);
        store_k(t0 & 1);
        vst.store(vs0 + (t0 & 1) * V_BYTES);
    }
    retire_q();
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const int buf = t & 1, kv0 = t * FL_BKV;
        if (t + 1 < t1) { load_k(t + 1); vst.load(vh, t + 1); }
        const bool cur = kv0 <= w.mask_off + w.qw0 + 31;    // tiles entirely above this wave's diagonal contribute nothing (wave-uniform)
        if (cur) qk(buf, kv0, sc0, sc1);
        if (cur) flash_softmax_pv<T, DT, SCALED>(w, kv0, kv_len, ql, h, sc0, sc1, o, m_run, l_run, vs0 + buf * V_BYTES, cf);
        if (t + 1 < t1) { store_k(buf ^ 1); vst.store(vs0 + (buf ^ 1) * V_BYTES); }
        __syncthreads();
    }
}

// The row's sum over both lane halves; inv = its reciprocal, 0 for a row that saw no key
__device__ __forceinline__ float flash_row_sum(float l_run, float& inv) {
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    return l_tot;
}

// Normalise and store: lane = query row, registers 4g..4g+3 of tile i are d = 32i + 8g + 4h .. +3.  With a KV split the row
// goes to this run's partial output and lane half 0 leaves the run's (m, l) for flash_merge_kernel.
template <class T, int DT>
__device__ __forceinline__ void flash_store_row(const FlashWork& w, const f32x16_fl (&o)[DT], float m_run, float l_tot, float inv, int ql, int h,
                                                T* out, int hq, int q_len, const FlashStrides& sd, const FlashSplit& sp) {
    constexpr int D = DT * 32;
    const int qrow = w.qw0 + ql;
    if (qrow < q_len) {
        T* orow = sp.nsplit > 1 ? reinterpret_cast<T*>(sp.o) + (((size_t)w.split * q_len + qrow) * hq + w.head) * D
                                : out + (size_t)w.head * sd.oh + (size_t)qrow * sd.os;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 x;
                x.x = pack16x2<T>(o[i][4 * g] * inv, o[i][4 * g + 1] * inv);
                x.y = pack16x2<T>(o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv);
                *reinterpret_cast<uint2*>(orow + i * 32 + 8 * g + 4 * h) = x;
            }
        if (sp.nsplit > 1 && h == 0) {
            float* ml = sp.ml + (((size_t)w.split * hq + w.head) * q_len + qrow) * 2;
            ml[0] = m_run;
            ml[1] = l_tot;
        }
    }
}

// ---- host side: one launch = V^T pre-pass, the main kernel, the merge when the KV runs are split (flash_plan: attn_plan.h) ------
// ws: the launch's workspace of p.bytes, V^T first
inline FlashSplit flash_split(const FlashPlan& p, void* ws, uint8_t* q8 = nullptr, float* q8s = nullptr) {
    FlashSplit sp{p.nsplit, nullptr, nullptr, q8, q8s};
    if (p.nsplit > 1) {
        sp.o = (char*)ws + p.po_off;
        sp.ml = (float*)((char*)ws + p.ml_off);
    }
    return sp;
}

// main(grid, vt) launches the caller's kernel; returns the first launch error
template <class T, int D, class Main>
static hipError_t flash_run(const FlashPlan& p, void* ws, const FlashSplit& sp, const T* v, T* out, int hq, int hkv, int q_len, int kv_len,
                            const FlashStrides& sd, hipStream_t st, Main&& main) {
    T* vt = (T*)ws;
    transpose_v_kernel<T, D><<<dim3(p.kv_pad / 64, hkv), 256, 0, st>>>(v, vt, kv_len, p.kv_pad, sd.kh, sd.ks);
    main(p.nqt * hq * p.nsplit, (const T*)vt);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && p.nsplit > 1) {
        const size_t work = (size_t)q_len * hq * (D / 8);
        flash_merge_kernel<T, D><<<(unsigned)((work + 255) / 256), 256, 0, st>>>(sp.ml, (const T*)sp.o, out, hq, q_len, p.nsplit, sd.oh, sd.os, sp.q8, sp.q8s);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace pgk
