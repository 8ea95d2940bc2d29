// k_data.h -- training batches cut out of a device-resident sample arena (aero_amd/data.py: DeviceLrHrStore).
//
//   aero_segment_gather    out[b][t] = 0 <= start_b + t < len_f ? arena[off_f + start_b + t] (/ 32768 for int16) : 0,  f = item_file[b]
//
// The arena holds the decoded samples of every file of one side (lr or hr) back to back, int16 (PCM16 as stored) or fp32; a batch is B
// segments of L samples, each a window [start, start + L) of one file, zero padded behind the file's end (reference Audioset.__getitem__:
// a partial read, then F.pad).  int16 / 32768 is exact in fp32, so the result is bit-equal to the host reader's.
//
// A thread owns one 16-byte ALIGNED vector of the arena (8 int16 or 4 fp32): the window's first sample sits anywhere in its vector, so the
// thread's outputs start at t0 = vector start - window start, which is negative for the first vector of an unaligned window.  A vector
// that lies wholly inside its file is one 16-byte load (it may cover samples of the file outside the window: read, not stored); a vector
// cut by either end of the file is read sample by sample, in-range samples only -- nothing outside [off, off + len) is ever read, whatever
// follows the file in the arena.  The stores are two / one float4 where the output address of the thread's run is 16-byte aligned and the
// run lies inside the row (a per-item property: (b L - misalignment) mod 4), single floats otherwise.
#pragma once
#include "aero_common.h"

typedef short aero_s16x8 __attribute__((ext_vector_type(8)));

template <typename T>
struct aero_gather_vec;
template <>
struct aero_gather_vec<int16_t> {
    static constexpr int EV = 8;
    static __device__ __forceinline__ void load(const int16_t* p, float* v) {
        const aero_s16x8 r = *(const aero_s16x8*)p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)r[e] * (1.0f / 32768.0f);
    }
    static __device__ __forceinline__ float one(int16_t x) { return (float)x * (1.0f / 32768.0f); }
};
template <>
struct aero_gather_vec<float> {
    static constexpr int EV = 4;
    static __device__ __forceinline__ void load(const float* p, float* v) {
        const f32x4 r = *(const f32x4*)p;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = r[e];
    }
    static __device__ __forceinline__ float one(float x) { return x; }
};

// grid (vectors of a window / 256, B); a window spans at most L / EV + 2 vectors
template <typename T>
__global__ __launch_bounds__(256) void aero_segment_gather_kernel(const T* arena, const int64_t* file_off, const int64_t* file_len,
                                                                  const int32_t* item_file, const int64_t* item_start, int n_files, int L,
                                                                  float* out) {
    constexpr int EV = aero_gather_vec<T>::EV;
    const int b = blockIdx.y;
    const int f = item_file[b];
    int64_t off = 0, len = 0;                                    // (a file index outside the table: an all-zero row, no read)
    if (f >= 0 && f < n_files) {
        off = file_off[f];
        len = file_len[f];
    }
    const int64_t start = item_start[b];
    // element index of the window's first sample counted from address 0, and of the aligned vector that holds it
    const int64_t p0 = (int64_t)((uintptr_t)arena / sizeof(T)) + off + start;
    const int64_t v0 = p0 & ~(int64_t)(EV - 1);
    const int64_t t0 = (v0 - p0) + ((int64_t)blockIdx.x * 256 + threadIdx.x) * EV;     // output index of this thread's first sample (>= -(EV - 1))
    if (t0 >= L) return;
    const int64_t s0 = start + t0;                               // its position in the file
    float v[EV];
    if (s0 >= 0 && s0 + EV <= len) {
        aero_gather_vec<T>::load(arena + off + s0, v);
    } else {
#pragma unroll
        for (int e = 0; e < EV; ++e) {
            const int64_t s = s0 + e, t = t0 + e;
            v[e] = (s >= 0 && s < len && t >= 0 && t < L) ? aero_gather_vec<T>::one(arena[off + s]) : 0.f;
        }
    }
    float* o = out + (int64_t)b * L + t0;
    if (t0 >= 0 && t0 + EV <= L && ((uintptr_t)o & 15) == 0) {
#pragma unroll
        for (int e = 0; e < EV; e += 4) *(f32x4*)(o + e) = f32x4{v[e], v[e + 1], v[e + 2], v[e + 3]};
    } else {
#pragma unroll
        for (int e = 0; e < EV; ++e)
            if (t0 + e >= 0 && t0 + e < L) o[e] = v[e];
    }
}

static int aero_segment_gather_launch(const void* arena, int is_f32, const int64_t* file_off, const int64_t* file_len, int n_files,
                                      const int32_t* item_file, const int64_t* item_start, int B, int L, float* out, hipStream_t stream,
                                      const char** err) {
    if (!arena || !file_off || !file_len || !item_file || !item_start || !out) {
        *err = "aero_segment_gather: null arena, table or output";
        return AERO_ERR_ARG;
    }
    if (B < 1 || B > 65535 || L < 1 || n_files < 1) {
        *err = "aero_segment_gather: B in 1 .. 65535, L >= 1 and n_files >= 1 are required";
        return AERO_ERR_ARG;
    }
    if (((uintptr_t)arena & (is_f32 ? 3 : 1)) || ((uintptr_t)out & 3)) {
        *err = "aero_segment_gather: the arena must be aligned to its sample type and the output to 4 bytes";
        return AERO_ERR_ARG;
    }
    const int ev = is_f32 ? 4 : 8;
    const dim3 grid((unsigned)((L / ev + 2 + 255) / 256), (unsigned)B);
    if (is_f32)
        AERO_LAUNCH(aero_segment_gather_kernel<float>, grid, dim3(256), stream, (const float*)arena, file_off, file_len, item_file, item_start,
                    n_files, L, out);
    else
        AERO_LAUNCH(aero_segment_gather_kernel<int16_t>, grid, dim3(256), stream, (const int16_t*)arena, file_off, file_len, item_file,
                    item_start, n_files, L, out);
    return AERO_OK;
}
