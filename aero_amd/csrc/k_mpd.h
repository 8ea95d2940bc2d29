// k_mpd.h -- the edge pieces of the HiFi-GAN multi-period critic `mpd` (reference src/models/discriminators.py:89-147,
// DiscriminatorP / MultiPeriodDiscriminator); its dense layers (convs 1-4, 98 % of the FLOPs) run on aero_conv_fwd / aero_conv_wgrad
// and its 1-channel output conv on aero_gconv1d_fwd / _bwd (aero_amd/mpd.py).
//
// Layout: column j of clip b of the period-p view [B, 1, H, p] (discriminators.py:109-115) is batch item n = b p + j of a channels-last
// row signal [N = B p][rows][C] -- the (5, 1) Conv2d over H is then a Conv1d over the rows.  A stride-3 layer reads its input as
// [N][rows / 3][3 C] (same memory), so its producer stores `pitch` = 3 ceil(H / 3) rows per item with rows H .. pitch - 1 ZERO.
//
//   aero_mpd_fold          reflect pad on the right to a multiple of p (discriminators.py:110-113), fold into columns, cast to fp16
//   aero_mpd_unfold_add    its adjoint: the column gradients ADDED to the fp32 waveform gradient, the reflected tail folded back
//   aero_mpd_conv0_fwd     Conv2d(1, C, (5, 1), (3, 1), padding (2, 0)) + bias + LeakyReLU, rows stored at a pitch with a zero tail
//   aero_mpd_conv0_bwd     its data gradient (fp32, scaled) and deterministic weight / bias gradient (chunk slabs added in order)
//   aero_mpd_act           LeakyReLU in place on rows < H of a pitched buffer, rows H .. pitch - 1 zeroed (behind aero_conv_fwd)
#pragma once
#include "aero_common.h"

__global__ __launch_bounds__(256) void aero_mpd_fold_kernel(const float* x, h16* y, int L, int p, int H, int64_t n) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int64_t col = idx / H;                             // b p + j
        const int h = (int)(idx - col * H);
        const int64_t b = col / p;
        const int j = (int)(col - b * p);
        int i = h * p + j;
        if (i >= L) i = 2 * (L - 1) - i;                         // F.pad(..., 'reflect') on the right
        y[idx] = (h16)x[b * L + i];
    }
}

static int aero_mpd_fold_launch(const float* x, int B, int L, int p, void* y, hipStream_t stream, const char** err) {
    if (!x || !y || B < 1 || p < 1 || L < p) { *err = "mpd_fold: bad arguments (reflect padding needs L >= p)"; return AERO_ERR_ARG; }
    const int H = (L + p - 1) / p;
    const int64_t n = (int64_t)B * p * H;
    int64_t nb = (n + 255) / 256;
    if (nb > 8192) nb = 8192;
    AERO_LAUNCH(aero_mpd_fold_kernel, dim3((unsigned)nb), dim3(256), stream, x, (h16*)y, L, p, H, n);
    return AERO_OK;
}

// dx[b][i] += g[b p + i % p][i / p] (+ the same for the mirrored position i' = 2 (L - 1) - i when that lies in the padded tail)
__global__ __launch_bounds__(256) void aero_mpd_unfold_add_kernel(const float* g, float* dx, int L, int p, int H, int64_t n) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / L;
        const int i = (int)(idx - b * L);
        const float* gb = g + b * p * H;
        float v = gb[(int64_t)(i % p) * H + i / p];
        const int m = 2 * (L - 1) - i;
        if (m >= L && m < H * p) v += gb[(int64_t)(m % p) * H + m / p];
        dx[idx] += v;
    }
}

static int aero_mpd_unfold_add_launch(const float* g, int B, int L, int p, float* dx, hipStream_t stream, const char** err) {
    if (!g || !dx || B < 1 || p < 1 || L < p) { *err = "mpd_unfold_add: bad arguments"; return AERO_ERR_ARG; }
    const int H = (L + p - 1) / p;
    const int64_t n = (int64_t)B * L;
    int64_t nb = (n + 255) / 256;
    if (nb > 8192) nb = 8192;
    AERO_LAUNCH(aero_mpd_unfold_add_kernel, dim3((unsigned)nb), dim3(256), stream, g, dx, L, p, H, n);
    return AERO_OK;
}

// y[n][o][c] = lrelu(bias[c] + sum_k w[c][k] x[n][3 o + k - 2]) for o < Ho, 0 for Ho <= o < pitch;  w fp32 [C][5] (weight norm applied)
__global__ __launch_bounds__(256) void aero_mpd_conv0_fwd_kernel(const h16* x, const float* w, const float* bias, h16* y, int H, int C, int Ho, int pitch,
                                                                 float slope, int64_t n) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % C);
        const int64_t r = idx / C;
        const int64_t item = r / pitch;
        const int o = (int)(r - item * pitch);
        float v = 0.f;
        if (o < Ho) {
            const h16* xr = x + item * H;
            v = bias ? bias[c] : 0.f;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int t = 3 * o + k - 2;
                if (t >= 0 && t < H) v += w[c * 5 + k] * (float)xr[t];
            }
            v = v > 0.f ? v : v * slope;
        }
        y[idx] = (h16)v;
    }
}

static int aero_mpd_conv0_fwd_launch(const void* x, const float* w, const float* bias, void* y, int N, int H, int C, int pitch, float slope,
                                     hipStream_t stream, const char** err) {
    const int Ho = (H + 2) / 3;                                  // (H + 4 - 5) / 3 + 1
    if (!x || !w || !y || N < 1 || H < 1 || C < 1 || pitch < Ho) { *err = "mpd_conv0_fwd: bad arguments"; return AERO_ERR_ARG; }
    const int64_t n = (int64_t)N * pitch * C;
    int64_t nb = (n + 255) / 256;
    if (nb > 16384) nb = 16384;
    AERO_LAUNCH(aero_mpd_conv0_fwd_kernel, dim3((unsigned)nb), dim3(256), stream, (const h16*)x, w, bias, (h16*)y, H, C, Ho, pitch, slope, n);
    return AERO_OK;
}

// data gradient: dx[n][i] = inv_scale[0] * sum_{k, o : 3 o + k - 2 = i} sum_c w[c][k] dyp[n][o][c]    (dyp: gradient of the PRE-activation)
__global__ __launch_bounds__(256) void aero_mpd_conv0_dgrad_kernel(const h16* dyp, const float* w, const float* inv_scale, float* dx, int H, int C, int Ho,
                                                                   int pitch, int64_t n) {
    const float a = inv_scale ? inv_scale[0] : 1.f;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int64_t item = idx / H;
        const int i = (int)(idx - item * H);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int q = i + 2 - k;
            if (q < 0 || q % 3) continue;
            const int o = q / 3;
            if (o >= Ho) continue;
            const h16* dr = dyp + (item * pitch + o) * C;
            for (int c = 0; c < C; ++c) s += w[c * 5 + k] * (float)dr[c];
        }
        dx[idx] = a * s;
    }
}

// weight / bias gradient, chunk `blockIdx.x` of the N * Ho positions: slab[chunk][c][0..4] = sum dyp[n][o][c] x[n][3 o + k - 2],
// slab[chunk][c][5] = sum dyp[n][o][c].  Thread (c = tid % C, lane q = tid / C) takes every Q-th position; lanes added in order.
#define AERO_MPD_WG_PER 2048                                    /* positions per chunk (at least) */
__global__ __launch_bounds__(256) void aero_mpd_conv0_wgrad_kernel(const h16* dyp, const h16* x, float* slabs, int H, int C, int Ho, int pitch,
                                                                   int64_t P, int64_t per) {
    __shared__ float red[256 * 6];
    const int tid = threadIdx.x;
    const int Q = 256 / C;
    const int c = tid % C, q = tid / C;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int64_t p0 = (int64_t)blockIdx.x * per;
    const int64_t p1 = p0 + per < P ? p0 + per : P;
    if (q < Q) {
        for (int64_t pos = p0 + q; pos < p1; pos += Q) {
            const int64_t item = pos / Ho;
            const int o = (int)(pos - item * Ho);
            const float d = (float)dyp[(item * pitch + o) * C + c];
            const h16* xr = x + item * H;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int t = 3 * o + k - 2;
                if (t >= 0 && t < H) acc[k] += d * (float)xr[t];
            }
            acc[5] += d;
        }
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) red[tid * 6 + e] = acc[e];
    __syncthreads();
    for (int u = tid; u < C * 6; u += 256) {
        const int cc = u / 6, e = u - cc * 6;
        float s = 0.f;
        for (int qq = 0; qq < Q; ++qq) s += red[(qq * C + cc) * 6 + e];
        slabs[(int64_t)blockIdx.x * C * 6 + u] = s;
    }
}

__global__ __launch_bounds__(256) void aero_mpd_conv0_wgrad_finish_kernel(const float* slabs, int nchunk, int C, float* dw, float* db) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= C * 6) return;
    float s = 0.f;
    for (int k = 0; k < nchunk; ++k) s += slabs[(int64_t)k * C * 6 + u];
    const int c = u / 6, e = u - c * 6;
    if (e < 5) dw[c * 5 + e] = s;
    else if (db) db[c] = s;
}

static int64_t aero_mpd_conv0_chunks(int N, int H, int64_t* per) {
    const int Ho = (H + 2) / 3;
    const int64_t P = (int64_t)N * Ho;
    int64_t nc = (P + AERO_MPD_WG_PER - 1) / AERO_MPD_WG_PER;
    if (nc > 512) nc = 512;
    if (nc < 1) nc = 1;
    if (per) *per = (P + nc - 1) / nc;
    return nc;
}

static int aero_mpd_conv0_bwd_launch(const void* dyp, const void* x, const float* w, const float* inv_scale, float* dx, float* slabs, int nslab,
                                     float* dw, float* db, int N, int H, int C, int pitch, hipStream_t stream, const char** err) {
    const int Ho = (H + 2) / 3;
    if (!dyp || N < 1 || H < 1 || C < 1 || C > 256 || pitch < Ho) { *err = "mpd_conv0_bwd: bad arguments (C <= 256)"; return AERO_ERR_ARG; }
    if (dx) {
        if (!w) { *err = "mpd_conv0_bwd: the data gradient needs w"; return AERO_ERR_ARG; }
        const int64_t n = (int64_t)N * H;
        int64_t nb = (n + 255) / 256;
        if (nb > 16384) nb = 16384;
        AERO_LAUNCH(aero_mpd_conv0_dgrad_kernel, dim3((unsigned)nb), dim3(256), stream, (const h16*)dyp, w, inv_scale, dx, H, C, Ho, pitch, n);
    }
    if (dw) {
        int64_t per = 0;
        const int64_t nc = aero_mpd_conv0_chunks(N, H, &per);
        if (!x || !slabs || nslab < nc) { *err = "mpd_conv0_bwd: the weight gradient needs x and aero_mpd_conv0_slabs() slabs"; return AERO_ERR_ARG; }
        AERO_LAUNCH(aero_mpd_conv0_wgrad_kernel, dim3((unsigned)nc), dim3(256), stream, (const h16*)dyp, (const h16*)x, slabs, H, C, Ho, pitch,
                    (int64_t)N * Ho, per);
        AERO_LAUNCH(aero_mpd_conv0_wgrad_finish_kernel, dim3((unsigned)((C * 6 + 255) / 256)), dim3(256), stream, (const float*)slabs, (int)nc, C, dw, db);
    }
    return AERO_OK;
}

__global__ __launch_bounds__(256) void aero_mpd_act_kernel(h16* y, int H, int pitch, int C, float slope, int64_t n) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int row = (int)((idx / C) % pitch);
        float v = 0.f;
        if (row < H) {
            v = (float)y[idx];
            v = v > 0.f ? v : v * slope;
        }
        y[idx] = (h16)v;
    }
}

static int aero_mpd_act_launch(void* y, int N, int H, int pitch, int C, float slope, hipStream_t stream, const char** err) {
    if (!y || N < 1 || H < 1 || pitch < H || C < 1) { *err = "mpd_act: bad arguments"; return AERO_ERR_ARG; }
    const int64_t n = (int64_t)N * pitch * C;
    int64_t nb = (n + 255) / 256;
    if (nb > 8192) nb = 8192;
    AERO_LAUNCH(aero_mpd_act_kernel, dim3((unsigned)nb), dim3(256), stream, (h16*)y, H, pitch, C, slope, n);
    return AERO_OK;
}
