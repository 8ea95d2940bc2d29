// k_seanet.h -- the Seanet baseline generator (reference src/models/seanet.py), inference forward.
//
// Activations fp16 channels-last [B][T][C], fp32 accumulation, fp16 operands.  The waveform ends (C = 1) stay fp32.
//
//   aero_seanet_stats      per item: unbiased std of the waveform and 1 / (floor + std)                       (seanet.py:158-161)
//   aero_seanet_front      x / (floor + std), sinc resampling as a polyphase FIR, right zero pad -> fp32 [B][Tpad]   (seanet.py:161-168)
//   aero_seanet_conv_in    ReflectionPad1d(3) + Conv1d(1, C, 7) + tanh                                        (seanet.py:106-110)
//   aero_seanet_conv       the general MFMA conv: LeakyReLU on the INPUT, K taps (stride, dilation, zero or reflect padding), bias,
//                          optional tanh, optional add of a tensor of the output's shape (the decoder's skip), and an output scatter
//                          that turns "r phases x Cout channels per row" into r rows -- the transposed convs.  It is every strided /
//                          transposed / latent conv of the model and the layer-by-layer form of a ResnetBlock (AERO_SEANET_FUSE=0)
//   aero_seanet_resblock   ResnetBlock in ONE launch: y = Ws x + bs + W2 lrelu(W1 (*)_d reflect_d(lrelu(x)) + b1) + b2 (+ add)
//   aero_seanet_conv_out   LeakyReLU + ReflectionPad1d(3) + Conv1d(C, 1, 7) + tanh, + skip, trim, * std -> fp32 (seanet.py:113-119,176-179)
//
// MFMA operands (v_mfma_f32_16x16x32_f16): A = weights, rows = 16 output channels; B = activations, columns = 16 time steps; lane l
// holds k = 8 (l >> 4) .. + 7 of row / column l & 15 -- on channels-last rows 8 consecutive channels of one tap, one 16-byte read.  The
// weights are packed on the host in fragment order, image[m tile][k step][lane][8] (aero_amd/seanet.py: mfma_image), so a wave's A
// fragment is one contiguous 1 KiB read; M is padded to a multiple of 32 (a wave owns two m tiles x two n tiles), K to a multiple of 32.
// D: lane l holds rows 4 (l >> 4) .. + 3 of column l & 15: four consecutive channels of one time step, one 8-byte store.
#pragma once
#include "aero_common.h"

static __device__ __forceinline__ h16x8 aero_sn_lrelu8(h16x8 v, float slope) {
    h16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float f = (float)v[e];
        o[e] = (h16)(f > 0.f ? f : f * slope);
    }
    return o;
}

static __device__ __forceinline__ int aero_sn_reflect(int t, int T) {
    if (t < 0) t = -t;
    if (t >= T) t = 2 * (T - 1) - t;
    return t < 0 ? 0 : (t >= T ? T - 1 : t);                    // (only rows of masked outputs can still be outside)
}

// ---------------------------------------------------------------------------------------------------------------- front end
__global__ __launch_bounds__(256) void aero_seanet_stats_kernel(const float* x, int L, float floor_, float* stats) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const float* xb = x + (int64_t)blockIdx.x * L;
    double s = 0.0;
    for (int i = tid; i < L; i += 256) s += (double)xb[i];
    red[tid] = s;
    __syncthreads();
    for (int k = 128; k >= 1; k >>= 1) {
        if (tid < k) red[tid] += red[tid + k];
        __syncthreads();
    }
    const double mean = red[0] / (double)L;
    __syncthreads();
    s = 0.0;
    for (int i = tid; i < L; i += 256) {
        const double d = (double)xb[i] - mean;
        s += d * d;
    }
    red[tid] = s;
    __syncthreads();
    for (int k = 128; k >= 1; k >>= 1) {
        if (tid < k) red[tid] += red[tid + k];
        __syncthreads();
    }
    if (tid == 0) {
        const float sd = (float)sqrt(red[0] / (double)(L - 1));  // (L = 1: 0 / 0 = NaN, as torch.std)
        stats[2 * blockIdx.x] = sd;
        stats[2 * blockIdx.x + 1] = 1.0f / (floor_ + sd);
    }
}

static int aero_seanet_stats_launch(const float* x, int B, int L, float floor_, float* stats, hipStream_t stream, const char** err) {
    if (!x || !stats || B < 1 || L < 1) { *err = "seanet_stats: bad arguments"; return AERO_ERR_ARG; }
    AERO_LAUNCH(aero_seanet_stats_kernel, dim3((unsigned)B), dim3(256), stream, x, L, floor_, stats);
    return AERO_OK;
}

// y[b][t] = inv[b] * sum_k table[t % nw][k] x[b][(t / nw) og - width + k]  (t < Lup; 0 for Lup <= t < Tpad); table NULL: y = inv x
__global__ __launch_bounds__(256) void aero_seanet_front_kernel(const float* x, const float* stats, const float* table, float* y, int L, int Lup,
                                                                int Tpad, int og, int nw, int width, int64_t n) {
    const int KW = 2 * width + og;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / Tpad;
        const int t = (int)(idx - b * Tpad);
        const float* xb = x + b * L;
        float v = 0.f;
        if (t < Lup) {
            if (table) {
                const int i = t / nw, j = t - i * nw;
                const int base = i * og - width;
                const float* tj = table + (int64_t)j * KW;
                for (int k = 0; k < KW; ++k) {
                    const int s = base + k;
                    if (s >= 0 && s < L) v += tj[k] * xb[s];
                }
            } else {
                v = xb[t];
            }
            if (stats) v *= stats[2 * b + 1];
        }
        y[idx] = v;
    }
}

static int aero_seanet_front_launch(const float* x, const float* stats, const float* table, float* y, int B, int L, int Lup, int Tpad, int og, int nw,
                                    int width, hipStream_t stream, const char** err) {
    if (!x || !y || B < 1 || L < 1 || Lup < 1 || Tpad < Lup) { *err = "seanet_front: bad arguments"; return AERO_ERR_ARG; }
    if (table ? (og < 1 || nw < 1 || width < 0 || (int64_t)Lup > ((int64_t)L * nw + og - 1) / og) : Lup != L) {
        *err = "seanet_front: the resampled length must be ceil(L new / orig) at most (L without a table)";
        return AERO_ERR_ARG;
    }
    const int64_t n = (int64_t)B * Tpad;
    int64_t nb = (n + 255) / 256;
    if (nb > 16384) nb = 16384;
    AERO_LAUNCH(aero_seanet_front_kernel, dim3((unsigned)nb), dim3(256), stream, x, stats, table, y, L, Lup, Tpad, og, nw, width, n);
    return AERO_OK;
}

// y[b][t][c] = tanh(bias[c] + sum_k w[c][k] fp16(x[b][reflect(t + k - 3)]));  w fp32 [C][7] holding fp16 values
__global__ __launch_bounds__(256) void aero_seanet_conv_in_kernel(const float* x, const float* w, const float* bias, h16* y, int T, int C, int64_t n) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % C);
        const int64_t r = idx / C;
        const int64_t b = r / T;
        const int t = (int)(r - b * T);
        const float* xb = x + b * T;
        float v = bias[c];
#pragma unroll
        for (int k = 0; k < 7; ++k) v += w[c * 7 + k] * (float)(h16)xb[aero_sn_reflect(t + k - 3, T)];
        y[idx] = (h16)tanhf(v);
    }
}

static int aero_seanet_conv_in_launch(const float* x, const float* w, const float* bias, void* y, int B, int T, int C, hipStream_t stream,
                                      const char** err) {
    if (!x || !w || !bias || !y || B < 1 || C < 1) { *err = "seanet_conv_in: bad arguments"; return AERO_ERR_ARG; }
    if (T < 4) { *err = "seanet_conv_in: reflection padding 3 needs more than 3 samples"; return AERO_ERR_ARG; }
    const int64_t n = (int64_t)B * T * C;
    int64_t nb = (n + 255) / 256;
    if (nb > 32768) nb = 32768;
    AERO_LAUNCH(aero_seanet_conv_in_kernel, dim3((unsigned)nb), dim3(256), stream, x, w, bias, (h16*)y, T, C, n);
    return AERO_OK;
}

// y[b][t] = scale[b] * (tanh(bias + sum_{k, c} w[k][c] lrelu(x[b][reflect(t + k - 3)][c])) + skip[b][t]) for t < Tout;  skip fp32 [B][T]
__global__ __launch_bounds__(256) void aero_seanet_conv_out_kernel(const h16* x, const h16* w, const float* bias, const float* skip, const float* stats,
                                                                   float* y, int T, int C, int Tout, float slope, int64_t n) {
    const int cv = C >> 3;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / Tout;
        const int t = (int)(idx - b * Tout);
        const h16* xb = x + b * T * C;
        float v = bias[0];
        for (int k = 0; k < 7; ++k) {
            const h16* xr = xb + (int64_t)aero_sn_reflect(t + k - 3, T) * C;
            const h16* wk = w + k * C;
            for (int q = 0; q < cv; ++q) {
                const h16x8 a = aero_sn_lrelu8(*(const h16x8*)(xr + q * 8), slope);
                const h16x8 ww = *(const h16x8*)(wk + q * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) v += (float)ww[e] * (float)a[e];
            }
        }
        v = tanhf(v);
        if (skip) v += skip[b * T + t];
        if (stats) v *= stats[2 * b];
        y[idx] = v;
    }
}

static int aero_seanet_conv_out_launch(const void* x, const void* w, const float* bias, const float* skip, const float* stats, float* y, int B, int T,
                                       int C, int Tout, float slope, hipStream_t stream, const char** err) {
    if (!x || !w || !bias || !y || B < 1 || C < 8 || (C & 7) || Tout < 1 || Tout > T) { *err = "seanet_conv_out: bad arguments (C a multiple of 8)"; return AERO_ERR_ARG; }
    if (T < 4) { *err = "seanet_conv_out: reflection padding 3 needs more than 3 samples"; return AERO_ERR_ARG; }
    const int64_t n = (int64_t)B * Tout;
    int64_t nb = (n + 255) / 256;
    if (nb > 32768) nb = 32768;
    AERO_LAUNCH(aero_seanet_conv_out_kernel, dim3((unsigned)nb), dim3(256), stream, (const h16*)x, (const h16*)w, bias, skip, stats, y, T, C, Tout, slope, n);
    return AERO_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the general MFMA conv
// Row q of the product (q < Tq) has M = R Cout values: D[m][q] = bias[m] + sum_{k, c} W[m][k Cin + c] lrelu(x[q stride + k dil - pad][c]);
// value m = ph Cout + co is stored at time t = q R + ph - P, channel co, if 0 <= t < Tout.  A plain conv has R = 1, P = 0, Tq = Tout.
// Block = 128 rows x 32 values (four waves of 32 rows), grid (ceil(Tq / 128), Mpad / 32, B).  Operands straight from global memory / L2:
// no LDS, no barrier.
__global__ __launch_bounds__(256) void aero_seanet_conv_kernel(aero_seanet_conv_desc p) {
    const int lane = threadIdx.x & 63, wave = aero_uniform(threadIdx.x >> 6);
    const int g = lane >> 4, col = lane & 15;
    const int b = blockIdx.z;
    const int m0 = blockIdx.y * 32;
    const int q0 = blockIdx.x * 128 + wave * 32;
    if (q0 >= p.Tq) return;                                      // (wave-uniform; the kernel has no block barrier)
    const h16* xb = (const h16*)p.x + (int64_t)b * p.Tin * p.Cin;
    const int qn[2] = {q0 + col, q0 + 16 + col};
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[i][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int tap = (8 * g) / p.Cin, c = (8 * g) % p.Cin;
    const h16* wa = (const h16*)p.wimg + (int64_t)(m0 >> 4) * p.ksteps * 512 + lane * 8;
    for (int ks = 0; ks < p.ksteps; ++ks) {
        const h16x8 A0 = *(const h16x8*)(wa + (int64_t)ks * 512);
        const h16x8 A1 = *(const h16x8*)(wa + ((int64_t)p.ksteps + ks) * 512);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            h16x8 Bv = (h16x8){0, 0, 0, 0, 0, 0, 0, 0};
            if (tap < p.K && qn[n] < p.Tq) {
                int row = qn[n] * p.stride + tap * p.dil - p.pad;
                if (p.reflect) row = aero_sn_reflect(row, p.Tin);
                if (row >= 0 && row < p.Tin) Bv = aero_sn_lrelu8(*(const h16x8*)(xb + (int64_t)row * p.Cin + c), p.in_slope);
            }
            acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A0, Bv, acc[0][n], 0, 0, 0);
            acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A1, Bv, acc[1][n], 0, 0, 0);
        }
        c += 32;
        while (c >= p.Cin) { c -= p.Cin; ++tap; }
    }
    h16* y = (h16*)p.y;
    const h16* add = (const h16*)p.add;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + i * 16 + 4 * g;
        if (m >= p.M) continue;
        const int ph = m / p.Cout, co = m - ph * p.Cout;
        const f32x4 bias4 = *(const f32x4*)(p.bias + m);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int t = qn[n] * p.R + ph - p.P;
            if (qn[n] >= p.Tq || t < 0 || t >= p.Tout) continue;
            const int64_t o = ((int64_t)b * p.Tout + t) * p.Cout + co;
            h16x4 a4 = (h16x4){0, 0, 0, 0};
            if (add) a4 = *(const h16x4*)(add + o);
            h16x4 out;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[i][n][e] + bias4[e];
                if (p.act == 1) v = tanhf(v);
                out[e] = (h16)(v + (float)a4[e]);
            }
            *(h16x4*)(y + o) = out;
        }
    }
}

static int aero_seanet_conv_launch(const aero_seanet_conv_desc* d, hipStream_t stream, const char** err) {
    if (!d || !d->x || !d->wimg || !d->bias || !d->y || d->B < 1 || d->Tin < 1 || d->Tq < 1 || d->Tout < 1 || d->K < 1 || d->stride < 1 || d->dil < 1 ||
        d->pad < 0 || d->R < 1 || d->P < 0 || d->act < 0 || d->act > 1) {
        *err = "seanet_conv: bad arguments";
        return AERO_ERR_ARG;
    }
    if (d->Cin < 8 || (d->Cin & 7) || d->Cout < 8 || (d->Cout & 7) || d->M != d->R * d->Cout) {
        *err = "seanet_conv: channel counts must be multiples of 8 and M = R Cout";
        return AERO_ERR_ARG;
    }
    if (d->ksteps != (d->K * d->Cin + 31) / 32) { *err = "seanet_conv: ksteps must be ceil(K Cin / 32)"; return AERO_ERR_ARG; }
    if (d->reflect && d->pad >= d->Tin) { *err = "seanet_conv: reflection padding must be smaller than the input length"; return AERO_ERR_ARG; }
    // every row the kernel reads lies inside [0, Tin) or is masked (zero padding) / clamped (reflect); every store is masked by Tq, Tout, M
    const int mtiles = (d->M + 31) / 32;
    if (mtiles > 65535 || d->B > 65535) { *err = "seanet_conv: grid too large"; return AERO_ERR_ARG; }
    AERO_LAUNCH(aero_seanet_conv_kernel, dim3((unsigned)((d->Tq + 127) / 128), (unsigned)mtiles, (unsigned)d->B), dim3(256), stream, *d);
    return AERO_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the fused ResnetBlock
// Block = 128 time steps of one item (four waves of 32), every channel.  LDS: xs = the raw x tile with a halo of d rows on each side
// (reflected at the clip's ends), [128 + 2 d][C + 8]; hs = the hidden activation lrelu(fp16(W1 ... + b1)) as fp16, [128][C + 8], each
// wave reading back only the 32 rows it wrote (a wave-level rendezvous, no block barrier after the staging one).  The row pitch C + 8
// halves = an odd number of 16-byte slots, so the 16 rows of a fragment read fall on distinct bank groups.
//   GEMM 1 (K = 3 C):  B fragment = lrelu(xs[tl + tap d][c ..]),  tap = 0, 1, 2  <->  time offsets -d, 0, +d
//   GEMM 2 (K = 2 C):  B fragment = hs[tl][k ..] for k < C, the RAW xs[tl + d][k - C ..] for C <= k < 2 C: [W2 | Ws] in one product
#define AERO_SN_TT 128
__global__ __launch_bounds__(256) void aero_seanet_resblock_kernel(aero_seanet_res_desc p) {
    h16* xs = (h16*)AERO_DYN_SMEM;
    const int C = p.C, d = p.d, XS = C + 8, NR = AERO_SN_TT + 2 * d;
    h16* hs = xs + NR * XS;
    const int tid = threadIdx.x, lane = tid & 63, wave = aero_uniform(tid >> 6);
    const int g = lane >> 4, col = lane & 15;
    const int b = blockIdx.y, t0 = blockIdx.x * AERO_SN_TT;
    const h16* xb = (const h16*)p.x + (int64_t)b * p.T * C;
    const int cv = C >> 3;
    for (int idx = tid; idx < NR * cv; idx += 256) {
        const int r = idx / cv, v = idx - r * cv;
        const int t = aero_sn_reflect(t0 - d + r, p.T);
        *(h16x8*)(xs + r * XS + v * 8) = *(const h16x8*)(xb + (int64_t)t * C + v * 8);
    }
    __syncthreads();
    if (t0 + wave * 32 >= p.T) return;                           // (wave-uniform; no block barrier below)
    const int tl[2] = {wave * 32 + col, wave * 32 + 16 + col};
    const int mt2 = (C + 31) >> 5;                               // pairs of m tiles
    const h16* w1 = (const h16*)p.w1 + lane * 8;
    for (int mp = 0; mp < mt2; ++mp) {
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[i][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        int tap = (8 * g) / C, c = (8 * g) % C;
        const h16* wa = w1 + (int64_t)(2 * mp) * p.ks1 * 512;
        for (int ks = 0; ks < p.ks1; ++ks) {
            const h16x8 A0 = *(const h16x8*)(wa + (int64_t)ks * 512);
            const h16x8 A1 = *(const h16x8*)(wa + ((int64_t)p.ks1 + ks) * 512);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                h16x8 Bv = (h16x8){0, 0, 0, 0, 0, 0, 0, 0};
                if (tap < 3) Bv = aero_sn_lrelu8(*(const h16x8*)(xs + (tl[n] + tap * d) * XS + c), p.slope);
                acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A0, Bv, acc[0][n], 0, 0, 0);
                acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A1, Bv, acc[1][n], 0, 0, 0);
            }
            c += 32;
            while (c >= C) { c -= C; ++tap; }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = mp * 32 + i * 16 + 4 * g;
            if (m >= C) continue;
            const f32x4 b4 = *(const f32x4*)(p.b1 + m);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                h16x4 out;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float f = (float)(h16)(acc[i][n][e] + b4[e]);          // the hidden activation as the layer-by-layer form stores it
                    out[e] = (h16)(f > 0.f ? f : f * p.slope);
                }
                *(h16x4*)(hs + tl[n] * XS + m) = out;
            }
        }
    }
    aero_wave_sync();
    h16* y = (h16*)p.y;
    const h16* add = (const h16*)p.add;
    const h16* w2 = (const h16*)p.w2s + lane * 8;
    for (int mp = 0; mp < mt2; ++mp) {
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[i][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const h16* wa = w2 + (int64_t)(2 * mp) * p.ks2 * 512;
        for (int ks = 0; ks < p.ks2; ++ks) {
            const h16x8 A0 = *(const h16x8*)(wa + (int64_t)ks * 512);
            const h16x8 A1 = *(const h16x8*)(wa + ((int64_t)p.ks2 + ks) * 512);
            const int k = ks * 32 + 8 * g;
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                h16x8 Bv = (h16x8){0, 0, 0, 0, 0, 0, 0, 0};
                if (k < C) Bv = *(const h16x8*)(hs + tl[n] * XS + k);
                else if (k < 2 * C) Bv = *(const h16x8*)(xs + (tl[n] + d) * XS + (k - C));
                acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A0, Bv, acc[0][n], 0, 0, 0);
                acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A1, Bv, acc[1][n], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = mp * 32 + i * 16 + 4 * g;
            if (m >= C) continue;
            const f32x4 b4 = *(const f32x4*)(p.b2s + m);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int t = t0 + tl[n];
                if (t >= p.T) continue;
                const int64_t o = ((int64_t)b * p.T + t) * C + m;
                h16x4 a4 = (h16x4){0, 0, 0, 0};
                if (add) a4 = *(const h16x4*)(add + o);
                h16x4 out;
#pragma unroll
                for (int e = 0; e < 4; ++e) out[e] = (h16)(acc[i][n][e] + b4[e] + (float)a4[e]);
                *(h16x4*)(y + o) = out;
            }
        }
    }
}

static int64_t aero_seanet_resblock_lds(int C, int d) { return (int64_t)(2 * AERO_SN_TT + 2 * d) * (C + 8) * 2; }

static int aero_seanet_resblock_launch(const aero_seanet_res_desc* p, hipStream_t stream, const char** err) {
    if (!p || !p->x || !p->w1 || !p->w2s || !p->b1 || !p->b2s || !p->y || p->B < 1 || p->T < 1 || p->d < 1) {
        *err = "seanet_resblock: bad arguments";
        return AERO_ERR_ARG;
    }
    if (p->C < 8 || (p->C & 7)) { *err = "seanet_resblock: C must be a multiple of 8"; return AERO_ERR_ARG; }
    if (p->ks1 != (3 * p->C + 31) / 32 || p->ks2 != (2 * p->C + 31) / 32) { *err = "seanet_resblock: ks1 / ks2 must be ceil(3 C / 32), ceil(2 C / 32)"; return AERO_ERR_ARG; }
    if (p->d >= p->T) { *err = "seanet_resblock: reflection padding (the dilation) must be smaller than the input length"; return AERO_ERR_ARG; }
    if (p->x == p->y) { *err = "seanet_resblock: not in place (neighbouring tiles read the halo)"; return AERO_ERR_ARG; }
    const int64_t lds = aero_seanet_resblock_lds(p->C, p->d);
    if (lds > 160 * 1024) { *err = "seanet_resblock: tile does not fit the 160 KiB LDS (C <= 256 at d <= 9)"; return AERO_ERR_UNSUPPORTED; }
    if (p->B > 65535) { *err = "seanet_resblock: grid too large"; return AERO_ERR_ARG; }
    AERO_LAUNCH_DYN(aero_seanet_resblock_kernel, dim3((unsigned)((p->T + AERO_SN_TT - 1) / AERO_SN_TT), (unsigned)p->B), dim3(256), (size_t)lds, stream, *p);
    return AERO_OK;
}
