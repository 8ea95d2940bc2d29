// k_stitch.h -- overlapped chunk outputs of a long file joined on the device (aero_amd/enhance.py: predict_signal(overlap > 0), write_device).
//
//   aero_overlap_stitch   out[c][t] = y_k[c][j]                                          outside a fade
//                                   = p + fade[j] (c - p),  p = y_{k-1}[c][hop + j], c = y_k[c][j]      k >= 1 and j < V
//                         k = min(t / hop, n - 1), j = t - k hop;  and the running peak max |out| as fp32 bits
//   aero_wav_finalize     wav[t][c] = out[c][t] / max(peak, 1)                            (the fp32 payload of the file, interleaved)
//
// Chunk k of the file covers the output samples [k hop, k hop + Ly); neighbouring chunks share V = Ly - hop samples, over which the output
// moves from the earlier chunk to the later one along the table `fade`.  One launch joins the g equal-length chunk outputs of ONE forward,
// global chunks k0 .. k0 + g - 1: it writes [k0 hop, (k0 + g) hop) of every channel, or to the end of its last chunk when that is the
// file's last.  The chunk in front of the group's first arrives as `prev` (the last rows of the previous launch's y).
//
// Gather form: a thread owns four consecutive OUTPUT samples and reads them from one or two chunk rows, so nothing but the peak word is
// written by more than one thread and the result does not depend on scheduling.  A thread's four samples are one 16-byte ALIGNED vector
// of `out` (the row's first sample sits anywhere in its vector, as in k_data.h): a vector inside the written range is one 16-byte store;
// its sources are 16-byte loads where the four samples come from one chunk, lie on one side of the fade's end and every source address
// is aligned (hop odd: never), single floats otherwise.  Vectors cut by either end of the range are handled sample by sample.
// The peak: |v| as uint bits (monotone for finite values) reduced over the block, one atomicMax per block -- max is order-independent.
#pragma once
#include "aero_common.h"

struct aero_stitch_args {
    const float* y;          // [g ch][Ly]
    const float* prev;       // [ch][Lprev] or null
    const float* fade;       // [V]
    float* out;              // [ch][N_out]
    unsigned int* peak_bits;
    int64_t N_out, t_begin;  // t_begin = k0 hop
    int Ly, Lprev, V, hop, g, ch, len;   // len: samples written per channel, from t_begin
};

// sample r (counted from t_begin) of channel c
static __device__ __forceinline__ float aero_stitch_one(const aero_stitch_args& a, int c, int r) {
    const int q = r / a.hop, k = q < a.g - 1 ? q : a.g - 1, j = r - k * a.hop;
    const float cur = a.y[((int64_t)k * a.ch + c) * a.Ly + j];
    if (j >= a.V || (k == 0 && !a.prev)) return cur;
    const float p = k == 0 ? a.prev[(int64_t)c * a.Lprev + a.hop + j] : a.y[((int64_t)(k - 1) * a.ch + c) * a.Ly + a.hop + j];
    return p + a.fade[j] * (cur - p);
}

static __device__ __forceinline__ unsigned int aero_block_max_u32(unsigned int m) {
    __shared__ unsigned int wave_max[4];
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned int o = __shfl_xor(m, s);
        m = o > m ? o : m;
    }
    if (aero_lane() == 0) wave_max[aero_wave()] = m;
    __syncthreads();
    m = wave_max[0];
    for (int w = 1; w < 4; ++w) m = wave_max[w] > m ? wave_max[w] : m;
    return m;
}

// grid (vectors of the written range / 256, ch); the range spans at most len / 4 + 2 vectors
__global__ __launch_bounds__(256) void aero_overlap_stitch_kernel(aero_stitch_args a) {
    const int c = blockIdx.y;
    float* row = a.out + (int64_t)c * a.N_out + a.t_begin;
    // this thread's first sample counted from t_begin (>= -3): its vector of `out` is 16-byte aligned
    const int r0 = -(int)(((uintptr_t)row >> 2) & 3) + (int)(blockIdx.x * 256 + threadIdx.x) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned int m = 0;
    if (r0 >= 0 && r0 + 4 <= a.len) {
        const int q = r0 / a.hop, k = q < a.g - 1 ? q : a.g - 1, j = r0 - k * a.hop;
        const bool one_chunk = k == a.g - 1 || j + 3 < a.hop;
        const bool blend = (k > 0 || a.prev) && j < a.V;
        const float* cp = a.y + ((int64_t)k * a.ch + c) * a.Ly + j;
        if (one_chunk && !blend && ((uintptr_t)cp & 15) == 0) {
            const f32x4 cv = *(const f32x4*)cp;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = cv[e];
        } else if (one_chunk && blend && j + 3 < a.V) {
            const float* pp = (k == 0 ? a.prev + (int64_t)c * a.Lprev : a.y + ((int64_t)(k - 1) * a.ch + c) * a.Ly) + a.hop + j;
            const float* fp = a.fade + j;
            if ((((uintptr_t)cp | (uintptr_t)pp | (uintptr_t)fp) & 15) == 0) {
                const f32x4 cv = *(const f32x4*)cp, pv = *(const f32x4*)pp, fv = *(const f32x4*)fp;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = pv[e] + fv[e] * (cv[e] - pv[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = pp[e] + fp[e] * (cp[e] - pp[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = aero_stitch_one(a, c, r0 + e);
        }
        *(f32x4*)(row + r0) = f32x4{v[0], v[1], v[2], v[3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned int u = __float_as_uint(fabsf(v[e]));
            m = u > m ? u : m;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = r0 + e;
            if (r >= 0 && r < a.len) {
                const float x = aero_stitch_one(a, c, r);
                row[r] = x;
                const unsigned int u = __float_as_uint(fabsf(x));
                m = u > m ? u : m;
            }
        }
    }
    m = aero_block_max_u32(m);
    if (threadIdx.x == 0 && m) atomicMax(a.peak_bits, m);
}

static int aero_overlap_stitch_launch(const float* y, int Ly, const float* prev, int Lprev, const float* fade, int V, int hop, int64_t k0,
                                      int g, int ch, int last, float* out, int64_t N_out, unsigned int* peak_bits, hipStream_t stream,
                                      const char** err) {
    if (!y || !fade || !out || !peak_bits) {
        *err = "aero_overlap_stitch: null y, fade, out or peak_bits";
        return AERO_ERR_ARG;
    }
    if (g < 1 || ch < 1 || ch > 65535 || Ly < 1 || hop < 1 || V < 0 || k0 < 0 || N_out < 1) {
        *err = "aero_overlap_stitch: g, Ly, hop, N_out >= 1, ch in 1 .. 65535, V >= 0 and k0 >= 0 are required";
        return AERO_ERR_ARG;
    }
    if (V > hop) {
        *err = "aero_overlap_stitch: the overlap V exceeds the hop (more than two chunks would meet in one sample)";
        return AERO_ERR_ARG;
    }
    if ((k0 == 0) != (prev == nullptr)) {
        *err = "aero_overlap_stitch: prev is the chunk in front of the group: null exactly when k0 = 0";
        return AERO_ERR_ARG;
    }
    if ((!last || g > 1) && Ly < hop + V) {
        *err = "aero_overlap_stitch: a chunk that is not the file's last needs Ly >= hop + V";
        return AERO_ERR_ARG;
    }
    if (prev && Lprev < hop + V) {
        *err = "aero_overlap_stitch: prev needs Lprev >= hop + V";
        return AERO_ERR_ARG;
    }
    if ((((uintptr_t)y | (uintptr_t)prev | (uintptr_t)fade | (uintptr_t)out | (uintptr_t)peak_bits)) & 3) {
        *err = "aero_overlap_stitch: y, prev, fade, out and peak_bits must be aligned to 4 bytes";
        return AERO_ERR_ARG;
    }
    const int64_t t_begin = k0 * (int64_t)hop;
    const int64_t len = last ? (int64_t)(g - 1) * hop + Ly : (int64_t)g * hop;
    if (t_begin + len > N_out || len > 0x7fff0000) {
        *err = "aero_overlap_stitch: the written range [k0 hop, k0 hop + len) must lie inside [0, N_out) and span fewer than 2^31 samples";
        return AERO_ERR_ARG;
    }
    aero_stitch_args a;
    a.y = y, a.prev = prev, a.fade = fade, a.out = out, a.peak_bits = peak_bits;
    a.N_out = N_out, a.t_begin = t_begin;
    a.Ly = Ly, a.Lprev = Lprev, a.V = V, a.hop = hop, a.g = g, a.ch = ch, a.len = (int)len;
    const dim3 grid((unsigned)((len / 4 + 2 + 255) / 256), (unsigned)ch);
    AERO_LAUNCH(aero_overlap_stitch_kernel, grid, dim3(256), stream, a);
    return AERO_OK;
}

// a thread owns one 16-byte aligned vector of `wav`: four consecutive elements e = t ch + c of the interleaved payload.
// x / d is the correctly rounded fp32 division (hipcc's default for `/`): bit-equal to the host's wav / max(peak, 1)
__global__ __launch_bounds__(256) void aero_wav_finalize_kernel(const float* out, const unsigned int* peak_bits, int ch, int64_t N_out,
                                                                float* wav) {
    const float d = fmaxf(__uint_as_float(*peak_bits), 1.0f);
    const int64_t total = N_out * ch;
    const int64_t e0 = -(int64_t)(((uintptr_t)wav >> 2) & 3) + ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= total) return;
    float v[4];
    const bool whole = e0 >= 0 && e0 + 4 <= total;
    if (whole && ch == 1 && ((uintptr_t)(out + e0) & 15) == 0) {
        const f32x4 r = *(const f32x4*)(out + e0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = r[e] / d;
    } else {
        const int64_t eb = e0 < 0 ? 0 : e0;
        int64_t t = eb / ch;
        int c = (int)(eb - t * ch);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t x = e0 + e;
            v[e] = 0.f;
            if (x >= 0 && x < total) {
                v[e] = out[(int64_t)c * N_out + t] / d;
                if (++c == ch) c = 0, ++t;
            }
        }
    }
    if (whole) {
        *(f32x4*)(wav + e0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e0 + e >= 0 && e0 + e < total) wav[e0 + e] = v[e];
    }
}

static int aero_wav_finalize_launch(const float* out, const unsigned int* peak_bits, int ch, int64_t N_out, float* wav, hipStream_t stream,
                                    const char** err) {
    if (!out || !peak_bits || !wav) {
        *err = "aero_wav_finalize: null out, peak_bits or wav";
        return AERO_ERR_ARG;
    }
    if (ch < 1 || N_out < 1 || N_out > ((int64_t)1 << 33) / ch) {
        *err = "aero_wav_finalize: ch >= 1 and 1 <= N_out <= 2^33 / ch are required";
        return AERO_ERR_ARG;
    }
    if (((uintptr_t)out | (uintptr_t)peak_bits | (uintptr_t)wav) & 3) {
        *err = "aero_wav_finalize: out, peak_bits and wav must be aligned to 4 bytes";
        return AERO_ERR_ARG;
    }
    const int64_t blocks = (N_out * ch / 4 + 2 + 255) / 256;
    AERO_LAUNCH(aero_wav_finalize_kernel, dim3((unsigned)blocks), dim3(256), stream, out, peak_bits, ch, N_out, wav);
    return AERO_OK;
}
