// posenn_se.h — the feature-attention variant (`-se_insert'): an SE block on cnv5 in front of each head's cnv6.
//
// Reference: nets/posenn.py:219-246 (the loop over `rotation', `translation' re-binds cnv5: the translation head's block runs
// on the tensor the rotation head's block has already scaled), nets/attention_module.py:9-52 (se_block: mean over (h, w),
// dense 256 -> 32 ReLU, dense 32 -> 256 sigmoid, x * s; the call passes no activation, so ReLU whatever `-fc_*' says),
// davo.py:1010-1011.  With x = cnv5 of one pair image, d = mean_{h,w}(x):
//     s_r = sigmoid(relu(d W1r + b1r) W2r + b2r)              rotation/cnv6 reads x * s_r
//     s_t = sigmoid(relu((s_r d) W1t + b1t) W2t + b2t)        translation/cnv6 reads x * s_r * s_t
// mean(x * s_r) = s_r * mean(x) (s_r is constant over the image), so one reduction of cnv5 serves both blocks.
//
// Three launches: se5_squeeze (per image and chunk of pixels: 256 channel sums), se5_excite (per image: both blocks, float32),
// se5_scale (cnv5 read once -> the 512-channel tensor [x s_r | x s_r s_t] cnv6 reads as a two-group layer).  H3 = the f16x3
// storage (per pixel and 32 channels: 32 hi halves | 32 lo halves, carrying 2^act_shift), else plain float32 NHWC.
// Fixed chunking, fixed reduction order, no floating-point atomics: bitwise reproducible run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "params.h"

namespace davo {

typedef _Float16 se5_h8 __attribute__((ext_vector_type(8)));

// partial[n][chunk][c] = sum over the chunk's pixels of image n of cnv5[n][pixel][c] (in stored units).
// grid (SE5_CHUNKS, NB), 256 threads.  A chunk is ceil(P / SE5_CHUNKS) pixels of ONE image (P = pixels per image: any number,
// chunks past the image's end write zeros), so no sum crosses an image boundary.  H3: 32 threads per pixel (8 channels each:
// one 16-byte unit of hi halves, one of lo halves), 8 pixels per pass; float32: 64 threads per pixel (one float4), 4 pixels.
template <bool H3>
__global__ __launch_bounds__(256) void se5_squeeze(const uint8_t* __restrict__ x, int P, float* __restrict__ partial) {
    constexpr int TPP = H3 ? 32 : 64;          // threads per pixel
    constexpr int PL = 256 / TPP;              // pixels per pass
    constexpr int CPT = SE5_C / TPP;           // channels per thread
    const int chunk = blockIdx.x, n = blockIdx.y;
    const int per = (P + SE5_CHUNKS - 1) / SE5_CHUNKS;
    const int beg = min(chunk * per, P), end = min(beg + per, P);
    const int cg = threadIdx.x % TPP, pl = threadIdx.x / TPP;
    const uint8_t* img = x + (size_t)n * P * (SE5_C * 4);
    float acc[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) acc[k] = 0.f;
    for (int i = beg + pl; i < end; i += PL) {
        const uint8_t* px = img + (size_t)i * (SE5_C * 4);
        if (H3) {
            const uint8_t* u = px + (cg >> 2) * 128 + (cg & 3) * 16;
            const se5_h8 hi = *reinterpret_cast<const se5_h8*>(u), lo = *reinterpret_cast<const se5_h8*>(u + 64);
#pragma unroll
            for (int k = 0; k < CPT; ++k) acc[k] += (float)hi[k % 8] + (float)lo[k % 8];
        } else {
            const float4 v = *reinterpret_cast<const float4*>(px + cg * 16);
            acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
        }
    }
    __shared__ float red[PL][SE5_C];
#pragma unroll
    for (int k = 0; k < CPT; ++k) red[pl][cg * CPT + k] = acc[k];
    __syncthreads();
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < PL; ++q) s += red[q][threadIdx.x];
    partial[((size_t)n * SE5_CHUNKS + chunk) * SE5_C + threadIdx.x] = s;
}

// one SE block on a descriptor held in LDS (d[256]) -> this thread's channel of sigmoid(relu(d W1 + b1) W2 + b2).
// 256 threads; W1 [256][32], W2 [32][256] in the reference's [in, out] layout.  tmp: [8][32] + [32] floats of LDS.
__device__ __forceinline__ float se5_block(const float* __restrict__ d, const float* __restrict__ w1, const float* __restrict__ b1,
                                           const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ tmp) {
    const int t = threadIdx.x, j = t & (SE5_HID - 1), part = t >> 5;      // eight parts of 32 input channels per unit
    float z = 0.f;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
        const int c = part * 32 + k;
        z = fmaf(d[c], w1[c * SE5_HID + j], z);
    }
    tmp[part * SE5_HID + j] = z;
    __syncthreads();
    if (t < SE5_HID) {
        float e = b1[t];
#pragma unroll
        for (int q = 0; q < 8; ++q) e += tmp[q * SE5_HID + t];
        tmp[8 * SE5_HID + t] = fmaxf(e, 0.f);
    }
    __syncthreads();
    float y = b2[t];
#pragma unroll 8
    for (int k = 0; k < SE5_HID; ++k) y = fmaf(tmp[8 * SE5_HID + k], w2[k * SE5_C + t], y);
    __syncthreads();                           // tmp is reused by the next block
    return 1.0f / (1.0f + expf(-y));
}

// scale[n][0][c] = s_r, scale[n][1][c] = s_r * s_t.  grid NB, 256 threads (one per channel).  unscale = 2^-act_shift of cnv5
// (1 in float32 mode): the sums are in stored units.  w: the eight dense tensors, rotation's four then translation's.
struct Se5Weights { const float *w1r, *b1r, *w2r, *b2r, *w1t, *b1t, *w2t, *b2t; };
__global__ __launch_bounds__(256) void se5_excite(const float* __restrict__ partial, int P, float unscale, Se5Weights w,
                                                  float* __restrict__ scale) {
    __shared__ float d[SE5_C];
    __shared__ float tmp[9 * SE5_HID];
    const int n = blockIdx.x, c = threadIdx.x;
    const float* p = partial + (size_t)n * SE5_CHUNKS * SE5_C + c;
    float sum = 0.f;
#pragma unroll 8
    for (int q = 0; q < SE5_CHUNKS; ++q) sum += p[q * SE5_C];
    const float dc = (sum * unscale) / (float)P;
    d[c] = dc;
    __syncthreads();
    const float sr = se5_block(d, w.w1r, w.b1r, w.w2r, w.b2r, tmp);
    d[c] = sr * dc;                            // the mean of the scaled tensor (the loop re-binds cnv5)
    __syncthreads();
    const float st = se5_block(d, w.w1t, w.b1t, w.w2t, w.b2t, tmp);
    scale[((size_t)n * 2 + 0) * SE5_C + c] = sr;
    scale[((size_t)n * 2 + 1) * SE5_C + c] = sr * st;
}

// y[n][pixel] = [x * s_r (256 channels) | x * (s_r s_t) (256 channels)] in x's storage; one thread per 16-byte unit pair (H3: 8 channels)
// or float4 (float32: 4 channels).  H3: decode each pair, multiply in float32, re-split; the values keep cnv5's storage scale, and
// every factor is below 1, so nothing can clamp.  range: the record word of the scaled tensor (or null) receives the largest
// stored magnitude of the translation half - element by element the smaller of the two halves, so a half that sinks below
// the storage floor is seen even when the other does not.
// grid (ceil(P * threads per pixel / 256), NB): a workgroup stays inside one image.
template <bool H3>
__global__ __launch_bounds__(256) void se5_scale(const uint8_t* __restrict__ x, const float* __restrict__ scale, int P,
                                                 uint8_t* __restrict__ y, unsigned* __restrict__ range) {
    constexpr int TPP = H3 ? 32 : 64;
    const int n = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;              // (pixel of the image, channel group)
    float vmax = 0.f;
    if (idx < P * TPP) {
        const size_t pix = (size_t)n * P + idx / TPP;
        const int cg = idx % TPP;
        const float* sn = scale + (size_t)n * 2 * SE5_C;
        const uint8_t* px = x + (size_t)pix * (SE5_C * 4);
        uint8_t* py = y + (size_t)pix * (2 * SE5_C * 4);
        if (H3) {
            const int off = (cg >> 2) * 128 + (cg & 3) * 16;
            const se5_h8 hi = *reinterpret_cast<const se5_h8*>(px + off), lo = *reinterpret_cast<const se5_h8*>(px + off + 64);
            const float4 r0 = *reinterpret_cast<const float4*>(sn + cg * 8), r1 = *reinterpret_cast<const float4*>(sn + cg * 8 + 4);
            const float4 t0 = *reinterpret_cast<const float4*>(sn + SE5_C + cg * 8), t1 = *reinterpret_cast<const float4*>(sn + SE5_C + cg * 8 + 4);
            const float sr[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
            const float st[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
            se5_h8 ah, al, bh, bl;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float v = (float)hi[k] + (float)lo[k];
                // the clamp is the fp16 range every storing epilogue applies (no factor exceeds 1: it never binds).  It also stands
                // between the product and the conversions: left to fuse them (v_fma_mix), the compiler rounded the stored hi half from
                // the float32 product and the lo half against a hi rounded from the exact one - one fp16 ulp apart in 2^-15 of the values
                const float a = fminf(v * sr[k], 65504.f), b = fminf(v * st[k], 65504.f);
                vmax = fmaxf(vmax, fabsf(b));
                ah[k] = (_Float16)a; al[k] = (_Float16)(a - (float)ah[k]);
                bh[k] = (_Float16)b; bl[k] = (_Float16)(b - (float)bh[k]);
            }
            *reinterpret_cast<se5_h8*>(py + off) = ah;
            *reinterpret_cast<se5_h8*>(py + off + 64) = al;
            *reinterpret_cast<se5_h8*>(py + SE5_C * 4 + off) = bh;
            *reinterpret_cast<se5_h8*>(py + SE5_C * 4 + off + 64) = bl;
        } else {
            const float4 v = *reinterpret_cast<const float4*>(px + cg * 16);
            const float4 r = *reinterpret_cast<const float4*>(sn + cg * 4), t = *reinterpret_cast<const float4*>(sn + SE5_C + cg * 4);
            *reinterpret_cast<float4*>(py + cg * 16) = make_float4(v.x * r.x, v.y * r.y, v.z * r.z, v.w * r.w);
            *reinterpret_cast<float4*>(py + SE5_C * 4 + cg * 16) = make_float4(v.x * t.x, v.y * t.y, v.z * t.z, v.w * t.w);
        }
    }
    if (H3 && range) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
        range_note(range, vmax, (threadIdx.x & 63) == 0);
    }
}

}  // namespace davo
