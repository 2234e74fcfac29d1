// ops.audio for gfx950 (reference: native/ops/audio/audio.cu + audio_kernels.cuh - pad, frame, window, radix-2 FFT, copy,
// power, a HOST mel matmul, log: about 20 launches and a device -> host -> device round trip).
//
// audio_frames_kernel: samples -> normalised log-mel in ONE launch, nothing in global memory in between.  An STFT with a
// fixed small n_fft is a GEMM of windowed frames against a cos / -sin table; it runs on v_mfma_f32_32x32x2_f32, which is
// bit for bit an fmaf chain in k order (float32 in, float32 accumulate - no reduced-precision MFMA anywhere in this file).
//   * a workgroup (8 waves) owns 32 consecutive frames of one batch row;
//   * their sample span (31 * hop + n_fft floats) is loaded ONCE into LDS, reflect padding done by index arithmetic on the
//     way in (left src = pad - i, right src = n - 2 - off, both clamped to [0, n - 1]).  Sample s lives at s + (s >> 5):
//     32 lanes read 32 frames `hop` apart, and hop = 160 would put all of them on two banks;
//   * a wave takes bin groups of 32: A operand = the DFT table (lane -> bin, k-major so the 32 bins of a lane half are one
//     128-byte run, streamed from L2), B operand = sample * window formed from LDS (lane -> frame).  The cos and the -sin
//     tile of a bin group are two accumulators of the SAME wave with the same lane / register map, so re^2 + im^2 needs no
//     exchange;
//   * the power tile [bin][32 frames] goes to LDS; thread (mel row, frame) runs the filterbank row over its non-zero span
//     only (host-computed first / last bin), then log, affine, cast and the store in either layout.
// When span + window + power tile exceed the LDS budget (n_fft = 2048 with most hops) the samples are read from global
// memory with the same index arithmetic (audio_log_mel_plan: "lds" / "global").
// dynamic_range (OpenAI Whisper's max(x, x.max() - 8)): the kernel stores float32 log-mel and folds the maximum of the whole
// call into one device word with a vector atomic max on an order-preserving unsigned image of the float; audio_clamp_kernel
// then applies the clamp, the affine and the cast.  Without it the op is one launch.
// stft is the same kernel stopped after the DFT (re, im interleaved).  The small ops are one launch each.

#include <cstdlib>
#include <cstring>

#include "flash_common.hip.h"

namespace pgk {

constexpr int AU_FRAMES = 32, AU_THREADS = 512, AU_WAVES = AU_THREADS / 64;
constexpr size_t AU_LDS_MAX = 160 * 1024 - 256;     // dynamic part; the static word and alignment fit in the rest
constexpr int AU_MAX_NFFT = 2048, AU_MAX_MELS = 256;

struct AudioArgs {
    int n, n_fft, hop, pad, n_frames, n_freq, nbp, n_mels;     // pad = n_fft / 2 when centred, else 0; nbp = n_freq padded to 32
    int log_mode;                                              // 0: log10(max(m, eps)), 1: ln(m + eps), 2: m
    int frames_last;                                           // 1: out [B][n_frames][n_mels], 0: [B][n_mels][n_frames]
    int fold_max;                                              // 1: store raw float32 log-mel and fold the maximum
    float eps, log_floor, offset, scale;                       // log_floor = log10(eps), rounded once on the host
};

__device__ __forceinline__ int au_slot(int s) { return s + (s >> 5); }

// index into the padded signal -> index into the samples: the reference's pad_reflect_kernel, clamped (frames past the end of
// a partial tile read clamped addresses too; they are never stored)
__device__ __forceinline__ int au_src(long long i, int n, int pad) {
    long long s = i - pad;
    if (i < pad) s = pad - i;
    else if (s >= n) s = (long long)n - 2 - (s - n);
    return (int)(s < 0 ? 0 : (s > n - 1 ? n - 1 : s));
}

__device__ __forceinline__ unsigned au_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float au_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float au_log(float m, const AudioArgs& a) {
    if (a.log_mode == 0) return m > a.eps ? log10f(m) : a.log_floor;
    return a.log_mode == 1 ? logf(m + a.eps) : m;
}

// STAGE 0: log-mel (out: T, or float32 when a.fold_max); STAGE 1: stft (out: float32 [n_frames][n_freq][2], batch 1)
// dynamic LDS: [window n_fft][power nbp * 32 (STAGE 0)][span slots (LDS_SPAN)] floats
template <class T, int STAGE, bool LDS_SPAN>
__global__ __launch_bounds__(AU_THREADS) void audio_frames_kernel(const float* x, const float* window, const float* table, const float* fb,
                                                                  const int* fb_span, void* out, unsigned* max_word, AudioArgs a) {
    extern __shared__ __attribute__((aligned(16))) float au_smem[];
    __shared__ unsigned wg_max;
    float* win = au_smem;
    float* pw = win + a.n_fft;
    float* xs = pw + (STAGE == 0 ? a.nbp * AU_FRAMES : 0);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, ql = lane & 31, h = lane >> 5;
    const int f0 = blockIdx.x * AU_FRAMES, b = blockIdx.y;
    const float* xb = x + (size_t)b * a.n;
    const long long i0 = (long long)f0 * a.hop;                // padded-signal index of the span's first sample

    for (int i = tid; i < a.n_fft; i += AU_THREADS) win[i] = window[i];
    if (LDS_SPAN) {
        const int span = (AU_FRAMES - 1) * a.hop + a.n_fft;
        for (int s = tid; s < span; s += AU_THREADS) xs[au_slot(s)] = xb[au_src(i0 + s, a.n, a.pad)];
    }
    if (tid == 0) wg_max = 0u;
    __syncthreads();

    const int groups = a.nbp / 32;
    for (int g = wid; g < groups; g += AU_WAVES) {
        f32x16_fl re, im;
#pragma unroll
        for (int r = 0; r < 16; ++r) re[r] = 0.f, im[r] = 0.f;
        const float* tc = table + (size_t)h * a.nbp + g * 32 + ql;          // cos rows [k][nbp]; -sin rows follow at k + n_fft
        const float* ts = tc + (size_t)a.n_fft * a.nbp;
        const int sb = ql * a.hop + h;
        // one k pair: lane half h takes k0 + h.  Four pairs per trip so that the loads of the later ones are in flight under the
        // MFMAs of the earlier ones; n_fft is even, not necessarily a multiple of 8
        auto step = [&](int k0) {
            const float xv = LDS_SPAN ? xs[au_slot(sb + k0)] : xb[au_src(i0 + sb + k0, a.n, a.pad)];
            const float v = xv * win[k0 + h];
            const float c = tc[(size_t)k0 * a.nbp], s = ts[(size_t)k0 * a.nbp];
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(c, v, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_32x32x2f32(s, v, im, 0, 0, 0);
        };
        int k0 = 0;
        for (; k0 + 8 <= a.n_fft; k0 += 8) {
#pragma unroll
            for (int j = 0; j < 4; ++j) step(k0 + 2 * j);
        }
        for (; k0 < a.n_fft; k0 += 2) step(k0);
        // accumulator layout: column (frame) = lane & 31, rows (bins) (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int bin = g * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (STAGE == 0) {
                pw[bin * AU_FRAMES + ql] = fmaf(im[r], im[r], re[r] * re[r]);
            } else if (bin < a.n_freq && f0 + ql < a.n_frames) {
                float2* o = reinterpret_cast<float2*>(out) + (size_t)(f0 + ql) * a.n_freq + bin;
                *o = make_float2(re[r], im[r]);
            }
        }
    }
    if (STAGE != 0) return;
    __syncthreads();

    const int f = tid & 31, frame = f0 + f;
    unsigned key = 0u;
    for (int m = tid >> 5; m < a.n_mels; m += AU_THREADS / 32) {
        const int lo = max(fb_span[2 * m], 0), hi = min(fb_span[2 * m + 1], a.n_freq - 1);   // inclusive; an empty row has hi < lo
        const float* row = fb + (size_t)m * a.n_freq;
        float acc = 0.f;
        for (int k = lo; k <= hi; ++k) acc = fmaf(row[k], pw[k * AU_FRAMES + f], acc);
        float v = au_log(acc, a);
        if (frame >= a.n_frames) continue;
        const size_t o = a.frames_last ? ((size_t)b * a.n_frames + frame) * a.n_mels + m : ((size_t)b * a.n_mels + m) * a.n_frames + frame;
        if (a.fold_max) {
            reinterpret_cast<float*>(out)[o] = v;
            const unsigned kv = au_key(v);
            key = kv > key ? kv : key;
        } else {
            reinterpret_cast<T*>(out)[o] = from_f<T>((v + a.offset) * a.scale);
        }
    }
    if (a.fold_max) {
        if (key) atomicMax(&wg_max, key);
        __syncthreads();
        if (tid == 0 && wg_max) atomicMax(max_word, wg_max);
    }
}

template <class T>
__global__ __launch_bounds__(256) void audio_clamp_kernel(const float* x, T* out, const unsigned* max_word, size_t n, float range, float offset,
                                                          float scale) {
    const float floor_v = au_unkey(*max_word) - range;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = from_f<T>((fmaxf(x[i], floor_v) + offset) * scale);
}

enum { AU_PCM = 0, AU_MONO = 1, AU_POWER = 2, AU_MAGNITUDE = 3, AU_LN = 4, AU_DB = 5 };

template <int OP>
__global__ __launch_bounds__(256) void audio_map_kernel(const void* in, float* out, size_t n, float eps) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v;
        if (OP == AU_PCM) {
            v = (float)reinterpret_cast<const int16_t*>(in)[i] * (1.0f / 32768.0f);
        } else if (OP == AU_LN) {
            v = logf(reinterpret_cast<const float*>(in)[i] + eps);
        } else if (OP == AU_DB) {
            v = 10.0f * log10f(reinterpret_cast<const float*>(in)[i] + eps);
        } else {
            const float2 p = reinterpret_cast<const float2*>(in)[i];
            if (OP == AU_MONO) v = __fadd_rn(p.x, p.y) * 0.5f;
            else {
                v = fmaf(p.y, p.y, p.x * p.x);
                if (OP == AU_MAGNITUDE) v = sqrtf(v);
            }
        }
        out[i] = v;
    }
}

// One workgroup, in place: the scale needs the whole signal, and a second pass over <= a few MB reads it back from L2.
// mode 0: peak (scale = 1 / max|x| when max|x| > 1e-8), mode 1: rms (scale = target_rms / rms when rms > 1e-8; the sum of
// squares is accumulated in double, as the reference's host loop does).
__global__ __launch_bounds__(1024) void audio_normalize_kernel(float* x, size_t n, int mode, double target_rms) {
    __shared__ double red[1024];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (size_t i = tid; i < n; i += 1024) {
        const double v = (double)x[i];
        acc = mode == 0 ? fmax(acc, fabs(v)) : acc + v * v;
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) red[tid] = mode == 0 ? fmax(red[tid], red[tid + s]) : red[tid] + red[tid + s];
        __syncthreads();
    }
    float scale;
    if (mode == 0) {
        const float mx = (float)red[0];
        if (!(mx > 1e-8f)) return;
        scale = 1.0f / mx;
    } else {
        const double rms = sqrt(red[0] / (double)n);
        if (!(rms > 1e-8)) return;
        scale = (float)(target_rms / rms);
    }
    for (size_t i = tid; i < n; i += 1024) x[i] *= scale;
}

// ratio > 0: decimator, out[i] = sum_t taps[t] * x[i * ratio - n_taps / 2 + t], zeros outside the signal.
// ratio == 0: linear interpolation at i * src / dst, position and fraction from 64-bit integers.
__global__ __launch_bounds__(256) void audio_resample_kernel(const float* x, float* out, const float* taps, long long n, long long n_out, int ratio,
                                                             int n_taps, int src, int dst) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (long long)gridDim.x * 256) {
        if (ratio > 0) {
            const long long p0 = i * ratio - n_taps / 2;
            float acc = 0.f;
            for (int t = 0; t < n_taps; ++t) {
                const long long p = p0 + t;
                if (p >= 0 && p < n) acc = fmaf(x[p], taps[t], acc);
            }
            out[i] = acc;
        } else {
            const long long num = i * src, p = num / dst;
            const float frac = (float)(num - p * dst) / (float)dst;
            const float s0 = p < n ? x[p] : 0.f, s1 = p + 1 < n ? x[p + 1] : s0;
            out[i] = fmaf(frac, s1 - s0, s0);
        }
    }
}

static bool audio_lds_off() {
    const char* e = getenv("PGK_AUDIO_LDS");
    return e && strcmp(e, "0") == 0;
}
static inline int au_nbp(int n_fft) { return ceil_div(n_fft / 2 + 1, 32) * 32; }
static inline size_t au_span_slots(int n_fft, int hop) {
    const size_t span = (size_t)(AU_FRAMES - 1) * hop + n_fft;
    return span + (span >> 5) + 1;
}
static inline size_t au_lds_bytes(int n_fft, int hop, int stage, bool lds_span) {
    return 4 * ((size_t)n_fft + (stage == 0 ? (size_t)au_nbp(n_fft) * AU_FRAMES : 0) + (lds_span ? au_span_slots(n_fft, hop) : 0));
}
static bool au_shape_ok(long long n, int n_fft, int hop, int center) {
    return n >= 1 && n < (1LL << 31) - 2 * AU_MAX_NFFT && n_fft >= 16 && n_fft <= AU_MAX_NFFT && n_fft % 2 == 0 && hop >= 1 && hop <= n_fft &&
           (center || n >= n_fft);
}
static inline int au_frames(long long n, int n_fft, int hop, int center) { return (int)((n + (center ? 2 * (n_fft / 2) : 0) - n_fft) / hop + 1); }
// 1: the sample span sits in LDS; 0: samples are read from global memory
static int au_plan(int n_fft, int hop, int stage) { return !audio_lds_off() && au_lds_bytes(n_fft, hop, stage, true) <= AU_LDS_MAX ? 1 : 0; }

template <class T, int STAGE, bool LDS_SPAN>
static pgk_status au_launch(const float* x, const float* window, const float* table, const float* fb, const int* fb_span, void* out,
                            unsigned* max_word, const AudioArgs& a, int batch, hipStream_t st) {
    const size_t lds = au_lds_bytes(a.n_fft, a.hop, STAGE, LDS_SPAN);
    static bool attr_done = false;                             // per instantiation
    if (!attr_done) {
        PGK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&audio_frames_kernel<T, STAGE, LDS_SPAN>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)AU_LDS_MAX));
        attr_done = true;
    }
    audio_frames_kernel<T, STAGE, LDS_SPAN><<<dim3(ceil_div(a.n_frames, AU_FRAMES), batch), AU_THREADS, lds, st>>>(x, window, table, fb, fb_span, out,
                                                                                                                 max_word, a);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

template <class T>
static pgk_status au_log_mel(const float* x, const float* window, const float* table, const float* fb, const int* fb_span, void* out,
                             unsigned* max_word, const AudioArgs& a, int batch, hipStream_t st) {
    if (au_plan(a.n_fft, a.hop, 0)) return au_launch<T, 0, true>(x, window, table, fb, fb_span, out, max_word, a, batch, st);
    return au_launch<T, 0, false>(x, window, table, fb, fb_span, out, max_word, a, batch, st);
}

static inline unsigned au_grid(size_t n) {
    const size_t blocks = (n + 255) / 256;
    return (unsigned)(blocks > 4096 ? 4096 : (blocks ? blocks : 1));
}

}  // namespace pgk

using namespace pgk;

extern "C" {

int pgk_audio_log_mel_plan(int n_fft, int hop, int stage) {
    if (n_fft < 16 || n_fft > AU_MAX_NFFT || n_fft % 2 || hop < 1 || hop > n_fft || stage < 0 || stage > 1) return -1;
    return au_plan(n_fft, hop, stage);
}

pgk_status pgk_audio_log_mel(const float* samples, const float* window, const float* dft_table, const float* mel_fb, const int32_t* fb_span,
                             void* out, int batch, long long n, int n_fft, int hop, int center, int n_mels, int n_frames, int log_mode, float eps,
                             float log_floor, float offset, float scale, int use_range, float range, int frames_last, pgk_dtype out_dt,
                             pgk_stream s) {
    PGK_REQUIRE(samples && window && dft_table && mel_fb && fb_span && out, "pgk_audio_log_mel: null pointer");
    PGK_REQUIRE(au_shape_ok(n, n_fft, hop, center),
                "pgk_audio_log_mel: bad shape n=%lld n_fft=%d hop=%d center=%d (n_fft even in [16, %d], 1 <= hop <= n_fft, n >= n_fft uncentred)", n,
                n_fft, hop, center, AU_MAX_NFFT);
    PGK_REQUIRE(batch >= 1 && batch <= 65535, "pgk_audio_log_mel: batch %d outside [1, 65535]", batch);
    PGK_REQUIRE(n_mels >= 1 && n_mels <= AU_MAX_MELS, "pgk_audio_log_mel: n_mels %d outside [1, %d]", n_mels, AU_MAX_MELS);
    const int all_frames = au_frames(n, n_fft, hop, center);
    PGK_REQUIRE(n_frames >= 1 && n_frames <= all_frames, "pgk_audio_log_mel: n_frames %d outside [1, %d]", n_frames, all_frames);
    PGK_REQUIRE(log_mode >= 0 && log_mode <= 2, "pgk_audio_log_mel: log mode %d (0 = log10(max(m, eps)), 1 = ln(m + eps), 2 = none)", log_mode);
    PGK_REQUIRE(is_float_dtype(out_dt), "pgk_audio_log_mel: out dtype %d is not float32/float16/bfloat16", (int)out_dt);
    hipStream_t st = resolve_stream(s);
    AudioArgs a{(int)n, n_fft, hop, center ? n_fft / 2 : 0, n_frames, n_fft / 2 + 1, au_nbp(n_fft), n_mels, log_mode, frames_last ? 1 : 0,
                use_range ? 1 : 0, eps, log_floor, offset, scale};
    if (!use_range) {
        PGK_DISPATCH_FLOAT(out_dt, "pgk_audio_log_mel", return (au_log_mel<T>(samples, window, dft_table, mel_fb, fb_span, out, nullptr, a, batch, st)));
        return PGK_OK;
    }
    // float32 log-mel (in `out` itself when that is float32) + the maximum word, then the clamp pass
    const size_t total = (size_t)batch * n_mels * n_frames;
    void* ws = nullptr;
    if (pgk_status r = pgk_malloc(&ws, 16 + (out_dt == PGK_F32 ? 0 : total * 4))) return r;
    unsigned* word = reinterpret_cast<unsigned*>(ws);
    float* raw = out_dt == PGK_F32 ? reinterpret_cast<float*>(out) : reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + 16);
    hipError_t e = hipMemsetAsync(word, 0, 4, st);
    pgk_status r = PGK_OK;
    if (e == hipSuccess) r = au_log_mel<float>(samples, window, dft_table, mel_fb, fb_span, raw, word, a, batch, st);
    if (e == hipSuccess && r == PGK_OK) {
        switch (out_dt) {
            case PGK_F32: audio_clamp_kernel<float><<<au_grid(total), 256, 0, st>>>(raw, (float*)out, word, total, range, offset, scale); break;
            case PGK_F16: audio_clamp_kernel<f16><<<au_grid(total), 256, 0, st>>>(raw, (f16*)out, word, total, range, offset, scale); break;
            default: audio_clamp_kernel<bf16><<<au_grid(total), 256, 0, st>>>(raw, (bf16*)out, word, total, range, offset, scale); break;
        }
        e = hipGetLastError();
    }
    pgk_free(ws);   // stream-ordered reuse: later work on this stream runs after the kernels above
    if (r != PGK_OK) return r;
    PGK_CHECK_HIP(e);
    return PGK_OK;
}

pgk_status pgk_audio_stft(const float* samples, const float* window, const float* dft_table, float* out, long long n, int n_fft, int hop,
                          int center, pgk_stream s) {
    PGK_REQUIRE(samples && window && dft_table && out, "pgk_audio_stft: null pointer");
    PGK_REQUIRE(au_shape_ok(n, n_fft, hop, center),
                "pgk_audio_stft: bad shape n=%lld n_fft=%d hop=%d center=%d (n_fft even in [16, %d], 1 <= hop <= n_fft, n >= n_fft uncentred)", n, n_fft,
                hop, center, AU_MAX_NFFT);
    AudioArgs a{(int)n, n_fft, hop, center ? n_fft / 2 : 0, au_frames(n, n_fft, hop, center), n_fft / 2 + 1, au_nbp(n_fft), 0, 0, 0, 0, 0.f, 0.f, 0.f, 0.f};
    hipStream_t st = resolve_stream(s);
    if (au_plan(n_fft, hop, 1)) return au_launch<float, 1, true>(samples, window, dft_table, nullptr, nullptr, out, nullptr, a, 1, st);
    return au_launch<float, 1, false>(samples, window, dft_table, nullptr, nullptr, out, nullptr, a, 1, st);
}

pgk_status pgk_audio_map(const void* in, float* out, size_t n, int op, float eps, pgk_stream s) {
    PGK_REQUIRE(op >= AU_PCM && op <= AU_DB, "pgk_audio_map: op %d outside [0, 5]", op);
    if (n == 0) return PGK_OK;
    PGK_REQUIRE(in && out, "pgk_audio_map: null pointer");
    hipStream_t st = resolve_stream(s);
    switch (op) {
        case AU_PCM: audio_map_kernel<AU_PCM><<<au_grid(n), 256, 0, st>>>(in, out, n, eps); break;
        case AU_MONO: audio_map_kernel<AU_MONO><<<au_grid(n), 256, 0, st>>>(in, out, n, eps); break;
        case AU_POWER: audio_map_kernel<AU_POWER><<<au_grid(n), 256, 0, st>>>(in, out, n, eps); break;
        case AU_MAGNITUDE: audio_map_kernel<AU_MAGNITUDE><<<au_grid(n), 256, 0, st>>>(in, out, n, eps); break;
        case AU_LN: audio_map_kernel<AU_LN><<<au_grid(n), 256, 0, st>>>(in, out, n, eps); break;
        default: audio_map_kernel<AU_DB><<<au_grid(n), 256, 0, st>>>(in, out, n, eps); break;
    }
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_audio_normalize(float* x, size_t n, int mode, double target_rms, pgk_stream s) {
    PGK_REQUIRE(mode == 0 || mode == 1, "pgk_audio_normalize: mode %d (0 = peak, 1 = rms)", mode);
    if (n == 0) return PGK_OK;
    PGK_REQUIRE(x, "pgk_audio_normalize: null pointer");
    audio_normalize_kernel<<<1, 1024, 0, resolve_stream(s)>>>(x, n, mode, target_rms);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

pgk_status pgk_audio_resample(const float* x, float* out, const float* taps, long long n, long long n_out, int ratio, int n_taps, int src, int dst,
                              pgk_stream s) {
    PGK_REQUIRE(n >= 1 && src >= 1 && dst >= 1 && n_out == n * dst / src, "pgk_audio_resample: n=%lld n_out=%lld src=%d dst=%d (n_out = n * dst / src)",
                n, n_out, src, dst);
    PGK_REQUIRE(ratio == 0 || (ratio >= 2 && src == (long long)ratio * dst && taps && n_taps >= 2 && n_taps % 2 == 0),
                "pgk_audio_resample: ratio %d needs src = ratio * dst and an even number of taps (%d)", ratio, n_taps);
    if (n_out == 0) return PGK_OK;
    PGK_REQUIRE(x && out, "pgk_audio_resample: null pointer");
    audio_resample_kernel<<<au_grid((size_t)n_out), 256, 0, resolve_stream(s)>>>(x, out, taps, n, n_out, ratio, n_taps, src, dst);
    PGK_LAUNCH_CHECK();
    return PGK_OK;
}

}  // extern "C"
