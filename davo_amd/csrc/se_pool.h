// se_pool.h — squeeze and excitation of the pooled flow-attention variants (att_source 14..17, params.h): the SE descriptor is a
// grid of window means of the SE-transformed flow (pool_plan.h) instead of one global mean.
//
// Reference: nets/attention_module.py:68-77 (gp2x2), :79-86, 137-167 (spp: tf.pad, avg_pool SAME), :89-101 (the two dense
// layers), davo.py:1088-1102 (transform, applied per pixel before pooling), :1181-1210 (the branches), :1404-1412 (scope se_flow:
// the target's map is ones).
//
//   se_pool_squeeze   one workgroup per work item (a cell, or a row slab of a large cell): partial[b][s][item][2] = the sum of
//                     t(flow[b][s]) over the item's pixels.  Only pixels inside a window are read.
//   se_pool_excite    one wave per (window, frame): adds each cell's items in item order, multiplies by the cell's reciprocal
//                     divisor, runs dense D -> NH -> 19 and writes the class table; the descriptor goes to a debug tensor too.
// Every order of addition is fixed by the plan and the thread count: the same bits run after run, whatever the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "input_decode.h"
#include "params.h"
#include "prologue.h"

namespace davo {

// grid (items, selected sources, B), 256 threads.  A row of an item is cut into units: one pixel where the row's first column
// is odd, then pairs of pixels on even columns (one widen_fetch4: W is a multiple of 4, so an even column is a 16-byte boundary of a
// float32 plane, an 8-byte one of a binary16 plane), then one pixel where a column is left over - a pair never straddles a cell
// edge.  Unit u of the item goes to thread u % 256; a thread adds its units in order, then se_squeeze_partial's fixed tree.
template <typename FT>
__global__ __launch_bounds__(256) void se_pool_squeeze(const FT* __restrict__ flow, int H, int W, Variant v, int sel, PoolDev pd,
                                                       float* __restrict__ partial) {
    const int item = blockIdx.x, s = pair_source(blockIdx.y, sel), b = blockIdx.z;
    const int4 r = reinterpret_cast<const int4*>(pd.items)[item];            // y0, y1, x0, x1: inside [0, H) x [0, W) (pool_plan.h)
    const FT* f = flow + ((size_t)b * 4 + s) * (size_t)H * W * 2;
    const int x0 = r.z, x1 = r.w;
    const int head = x0 & 1, xa = x0 + head;
    const int npair = (x1 - xa) >> 1, tail = (x1 - xa) & 1;
    const int nu = head + npair + tail;
    const int total = (r.y - r.x) * nu;
    float sx = 0.f, sy = 0.f;
    for (int u = threadIdx.x; u < total; u += 256) {
        const int row = u / nu, k = u - row * nu;
        const size_t rowoff = (size_t)(r.x + row) * W;
        if (k >= head && k < head + npair) {
            const float4 q = widen_fetch4(f + (rowoff + xa + 2 * (k - head)) * 2);
            sx += se_flow_transform(q.x, 0, v) + se_flow_transform(q.z, 0, v);
            sy += se_flow_transform(q.y, 1, v) + se_flow_transform(q.w, 1, v);
        } else {
            const float2 q = flow_fetch1(f + (rowoff + (k < head ? x0 : x1 - 1)) * 2);
            sx += se_flow_transform(q.x, 0, v);
            sy += se_flow_transform(q.y, 1, v);
        }
    }
    __shared__ float red[2][4];
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[0][wid] = sx; red[1][wid] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = partial + (((size_t)b * 2 + s) * pd.n_items + item) * 2;
        o[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        o[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// grid (B, 3 frames), 64 threads; NH = the bottleneck width (8, or 19 for gp2x2's `_nobottle').  Descriptor entry i = lane + 64 q
// (q < POOL_MAX_D / 64) is the lane's: entry 2 c + k is component k of cell c.  Dense [D, NH]: every lane's products over its own
// entries in q order, closed by a fixed butterfly over the lanes, so every lane holds every bottleneck unit; dense [NH, 19]: lane
// c < 19 evaluates class c, as se_excite_wave does.  All of a lane's weights are requested ahead of the first use.
// desc [B][2][D]: the descriptor as the dense layer reads it ("se_desc", davo_debug_read).
template <int NH>
__global__ __launch_bounds__(64) void se_pool_excite(const float* __restrict__ partial, PoolDev pd, Variant v,
                                                     const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, const float* __restrict__ b2,
                                                     float* __restrict__ tab, float* __restrict__ desc,
                                                     unsigned* __restrict__ range_reset, int sel) {
    if (range_reset && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) range_reset[RANGE_SNAP] = 0u;      // as se_excite
    const int b = blockIdx.x, frame = blockIdx.y, lane = threadIdx.x;
    if (!pair_reads_frame(frame, sel)) return;
    float* t = tab + ((size_t)b * 3 + frame) * NCLS;
    if (frame == 0) {                                          // davo.py:1408-1412
        if (lane < NCLS) t[lane] = 1.0f;
        return;
    }
    constexpr int Q = POOL_MAX_D / 64;
    const int D = 2 * pd.n_cells, s = frame - 1;
    float w1c[Q][NH], w2c[NH], b1c[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) b1c[j] = b1[j];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = min(lane + 64 * q, D - 1);
#pragma unroll
        for (int j = 0; j < NH; ++j) w1c[q][j] = w1[i * NH + j];
    }
    const int k = min(lane, NCLS - 1);
#pragma unroll
    for (int j = 0; j < NH; ++j) w2c[j] = w2[j * NCLS + k];
    const float b2k = b2[k];
    const float* pp = partial + ((size_t)b * 2 + s) * pd.n_items * 2;
    float acc[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) acc[j] = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = lane + 64 * q;
        if (i < D) {
            const int cell = i >> 1, c = i & 1;
            const int first = pd.cell_first[cell], last = pd.cell_first[cell + 1];
            float sum = 0.f;
            for (int it = first; it < last; ++it) sum += pp[it * 2 + c];
            const float d = sum * pd.inv_div[cell];
            desc[((size_t)b * 2 + s) * D + i] = d;
#pragma unroll
            for (int j = 0; j < NH; ++j) acc[j] += d * w1c[q][j];
        }
    }
    float e[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) {
        float z = acc[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        z += b1c[j];
        e[j] = v.se_act == 1 ? tanhf(z) : v.se_act == 2 ? (z > 0.f ? z : 0.2f * z) : fmaxf(z, 0.f);
    }
    if (lane < NCLS) {
        float y = b2k;
#pragma unroll
        for (int j = 0; j < NH; ++j) y += e[j] * w2c[j];
        t[lane] = 1.0f / (1.0f + expf(-y));
    }
}

}  // namespace davo
