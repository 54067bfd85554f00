// prologue.h — the HBM-bound front of the pose path: SE squeeze, the 2->8->19 excitation
// MLP (se_flow; twice, near and far, for the depth-split flow attention), the class-table squeeze / excitation of the segmentation, rgb, seg+flow and
// depth sources, and the mask + pack pass that builds the PoseNN input.
//
// Reference (all under /root/reference): davo.py:1519-1522 (u8 -> f32 * (1/255) * 2 - 1),
// data_loader.py:537-557 (strip = src0 | tgt | src1), davo.py:978-982 / 998-1004 (flow planes
// 0,1; seg file planes src0,tgt,src1), davo.py:1088-1102 (SE input transform),
// nets/attention_module.py:9-52 (se_block), :54-103 (se, mode 'gp'), davo.py:1274-1374
// (class-table sources), davo.py:1115,1178 (one_hot . weights ==
// 19-entry LUT gather, out-of-range id -> 0), nets/posenn.py:380-394 (static weights),
// davo.py:1404-1442 (masking, concat).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "input_decode.h"
#include "params.h"
#include "pose_tail.h"

namespace davo {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// SE squeeze, pass 1: partial[b][s][chunk][2] = sum over the chunk's pixels of t(flow[b][s]).
// grid (SQ_CHUNKS, selected sources, B), 256 threads; float4 = two pixels x (fx, fy).  Fixed chunking and a
// fixed reduction tree -> bitwise reproducible run to run.  With one pair selected (sel, params.h) only that source's plane is read.
// FT: the flow element, float or in_f16 (input_decode.h); a thread's unit comes from one widen_fetch4.
template <typename FT>
__global__ __launch_bounds__(256) void se_squeeze_partial(const FT* __restrict__ flow, int HW,
                                                          int norm_flow, int abs_mode, int sel,
                                                          float* __restrict__ partial) {
    const int chunk = blockIdx.x, s = pair_source(blockIdx.y, sel), b = blockIdx.z;
    const FT* f = flow + ((size_t)b * 4 + s) * HW * 2;
    const int nvec = HW / 2;                                   // HW is a multiple of 16
    const int per = (nvec + SQ_CHUNKS - 1) / SQ_CHUNKS;
    const int beg = chunk * per, end = min(beg + per, nvec);
    float sx = 0.f, sy = 0.f;
    for (int i = beg + threadIdx.x; i < end; i += 256) {
        float4 v = widen_fetch4(f + (size_t)i * 4);
        if (norm_flow) {
            v.x = (v.x - 0.32140523f) / 15.384229f; v.y = (v.y - 0.32140523f) / 15.384229f;
            v.z = (v.z - 0.32140523f) / 15.384229f; v.w = (v.w - 0.32140523f) / 15.384229f;
        }
        if (abs_mode & 1) { v.x = fabsf(v.x); v.z = fabsf(v.z); }
        if (abs_mode & 2) { v.y = fabsf(v.y); v.w = fabsf(v.w); }
        sx += v.x + v.z;
        sy += v.y + v.w;
    }
    __shared__ float red[2][4];
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[0][wid] = sx; red[1][wid] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = partial + (((size_t)b * 2 + s) * SQ_CHUNKS + chunk) * 2;
        o[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        o[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

__device__ __forceinline__ unsigned agent_load_u32(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The SE flow transform of one component (davo.py:1088-1102): c = 0 horizontal, 1 vertical.
__device__ __forceinline__ float se_flow_transform(float f, int c, const Variant& v) {
    if (v.norm_flow) f = (f - 0.32140523f) / 15.384229f;
    return (v.abs_mode & (1 << c)) ? fabsf(f) : f;
}

// Class-table excitation (att_source 4..12), one wave: tab[b][frame][19].  The descriptor's element c is lane c's: the sum of word c
// of the frame's SQ_CHUNKS squeeze records in chunk order (integers for the histogram and the rgb sums, so their order does not
// matter at all; the flow sums in a fixed order), turned into the mean once.  Then one lane per bottleneck unit, its inputs
// broadcast by shuffles, then one lane per class.  A `_wo_tgt' source's target table is ones (davo.py:1283,1310,1349,1366,1219).
// Depth sources (11, 12): the one input is the mean of depth_frame + depth_tgt (davo.py:1109: `list + tensor' broadcasts the
// target's depth onto every frame).  se_depth_squeeze sums each plane once; lane 0 adds the frame's SQ_CHUNKS records in chunk
// order, lane 1 the target's, their sum is divided by H*W once.
template <bool AGENT>
__device__ __forceinline__ void se_class_excite_wave(const unsigned* __restrict__ partial, int HW, const Variant& v, int b, int frame,
                                                     int lane, const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ tab) {
    float* t = tab + ((size_t)b * 3 + frame) * NCLS;
    const int a = v.att_source;
    if (frame == 0 && !att_tgt_attended(a)) {
        if (lane < NCLS) t[lane] = 1.0f;
        return;
    }
    const int nin = att_se_in(a), nh = att_se_hidden(a);
    // the lane's weights first, in fixed-length loops: all of them in flight at once, ahead of the descriptor's loads (a loop over
    // nin dependent round trips took 15 us at B = 32)
    constexpr int MAX_IN = NCLS + 2;
    const int j = min(lane, nh - 1), k = min(lane, NCLS - 1);
    float w1c[MAX_IN], w2c[NCLS];
#pragma unroll
    for (int c = 0; c < MAX_IN; ++c) w1c[c] = w1[min(c, nin - 1) * nh + j];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) w2c[c] = w2[min(c, nh - 1) * NCLS + k];
    const float b1j = b1[j], b2k = b2[k];
    const unsigned* rec = partial + ((size_t)b * 3 + frame) * SQ_CHUNKS * SQ_REC;
    float d = 0.f;
    if (att_desc_depth(a)) {
        float sum = 0.f;
        if (lane < 2) {
            const unsigned* q = partial + ((size_t)b * 3 + (lane == 0 ? frame : 0)) * SQ_CHUNKS * SQ_REC;
            for (int ch = 0; ch < SQ_CHUNKS; ++ch) sum += __uint_as_float(AGENT ? agent_load_u32(q + ch * SQ_REC) : q[ch * SQ_REC]);
        }
        d = (__shfl(sum, 0, 64) + __shfl(sum, 1, 64)) * (1.0f / (float)HW);
    } else if (lane < nin) {
        if (att_desc_flow(a) && lane >= NCLS) {
            const int c = lane - NCLS;
            if (frame == 0) {
                d = se_flow_transform(0.f, c, v);               // the target's flow is zeros_like (davo.py:978)
            } else {
                float sum = 0.f;
                for (int ch = 0; ch < SQ_CHUNKS; ++ch) {
                    const unsigned* q = rec + ch * SQ_REC + lane;
                    sum += __uint_as_float(AGENT ? agent_load_u32(q) : *q);
                }
                d = sum * (1.0f / (float)HW);
            }
        } else {
            unsigned long long sum = 0;
            for (int ch = 0; ch < SQ_CHUNKS; ++ch) {
                const unsigned* q = rec + ch * SQ_REC + lane;
                sum += AGENT ? agent_load_u32(q) : *q;
            }
            // histogram: mean of one_hot = count / HW; rgb: mean of u8 * (1/255) * 2 - 1 over the frame (davo.py:1521-1522)
            d = att_desc_rgb(a) ? (float)((double)sum / ((double)HW * 255.0) * 2.0 - 1.0) : (float)((double)sum / (double)HW);
        }
    }
    float z = b1j;
#pragma unroll
    for (int c = 0; c < MAX_IN; ++c) {                                                  // dense [nin, nh]
        const float dc = __shfl(d, c, 64);
        if (c < nin) z += dc * w1c[c];
    }
    const float e = v.se_act == 1 ? tanhf(z) : v.se_act == 2 ? (z > 0.f ? z : 0.2f * z) : fmaxf(z, 0.f);
    float y = b2k;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {                                                    // dense [nh, 19]
        const float ec = __shfl(e, c, 64);
        if (c < nh) y += ec * w2c[c];
    }
    // the static table's expression: zero kernels and recover_fc/bias = the static weights give its table to the bit
    if (lane < NCLS) t[lane] = 1.0f / (1.0f + expf(-y));
}

// One wave's share of the excitation: tab[b][frame][19] for frame = (tgt, src0, src1).
// Lanes 0..31 fetch the squeeze partials (fixed butterfly: bitwise reproducible), every lane evaluates the 8 bottleneck
// units, lane c < 19 the class c of the recovery layer — the three dependent steps of the MLP cost three memory round
// trips instead of the ~200 a single lane needed.  AGENT: the partials were written by other workgroups of the SAME
// launch (se_squeeze_excite's last workgroup): read them past the non-coherent caches.
template <bool AGENT>
__device__ __forceinline__ void se_excite_wave(const float* __restrict__ partial, int HW, const Variant& v, int b, int frame, int lane,
                                               const float* __restrict__ w1, const float* __restrict__ b1,
                                               const float* __restrict__ w2, const float* __restrict__ b2,
                                               const float* __restrict__ wstatic, float* __restrict__ tab) {
    if (att_class_table(v.att_source)) {
        se_class_excite_wave<AGENT>(reinterpret_cast<const unsigned*>(partial), HW, v, b, frame, lane, w1, b1, w2, b2, tab);
        return;
    }
    float* t = tab + ((size_t)b * 3 + frame) * NCLS;
    if (att_flow_squeeze(v.att_source) && frame >= 1) {        // se_flow, and each of the depth-split source's two MLPs
        const float* pp = partial + ((size_t)b * 2 + (frame - 1)) * SQ_CHUNKS * 2;
        static_assert(SQ_CHUNKS == 32, "one partial pair per lane of the lower half-wave");
        float sx = 0.f, sy = 0.f;
        if (lane < SQ_CHUNKS) {
            sx = AGENT ? agent_load(pp + 2 * lane) : pp[2 * lane];
            sy = AGENT ? agent_load(pp + 2 * lane + 1) : pp[2 * lane + 1];
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); }
        const float inv = 1.0f / (float)HW;
        sx *= inv; sy *= inv;                                  // tf.reduce_mean(axis=[1,2])
        float e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float z = sx * w1[j] + sy * w1[8 + j] + b1[j];     // dense [2,8]
            e[j] = v.se_act == 1 ? tanhf(z) : v.se_act == 2 ? (z > 0.f ? z : 0.2f * z) : fmaxf(z, 0.f);
        }
        if (lane < NCLS) {
            float z = b2[lane];
#pragma unroll
            for (int j = 0; j < 8; ++j) z += e[j] * w2[j * NCLS + lane];   // dense [8,19]
            t[lane] = 1.0f / (1.0f + expf(-z));
        }
    } else if (lane < NCLS) {
        if ((v.att_source == 2 && frame >= 1) || v.att_source == 3) t[lane] = 1.0f / (1.0f + expf(-wstatic[lane]));
        else t[lane] = 1.0f;                                   // davo.py:1408-1412 / 1385-1389
    }
}

// SE pass 2 + excitation as a launch of its own: one 64-lane wave per (triplet, frame).  Used by the variants without a
// squeeze (static / no attention) and with davo_set_option "fold_tails" 0.
__global__ __launch_bounds__(64) void se_excite(const float* __restrict__ partial, int HW, Variant v,
                                                const float* __restrict__ w1, const float* __restrict__ b1,
                                                const float* __restrict__ w2, const float* __restrict__ b2,
                                                const float* __restrict__ wstatic,
                                                float* __restrict__ tab, unsigned* __restrict__ range_reset, int sel) {
    // a ticketed device-path batch starts its own f16x3 range record (range_guard.hip: ticket_begin): first kernel of the forward, so in stream
    // order before any storing epilogue; a null pointer = the record is the caller's business
    if (range_reset && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) range_reset[RANGE_SNAP] = 0u;   // the per-batch word (params.h)
    if (!pair_reads_frame(blockIdx.y, sel)) return;           // an unselected source frame has no squeeze record and no reader of its table
    se_excite_wave<false>(partial, HW, v, blockIdx.x, blockIdx.y, threadIdx.x, w1, b1, w2, b2, wstatic, tab);
}

// Squeeze and excitation in ONE launch (attention_module.py:64-67 then :89-101): se_squeeze_partial's body, and the
// workgroup that delivers the LAST of a triplet's 2 x SQ_CHUNKS partial sums evaluates that triplet's three tables
// (pose_tail.h: ticket counter per triplet, agent-scope fences).  Same sums in the same order as the two launches.
// The second excitation of the depth-split source (att_source 13): the far MLP's tensors and the far table [B][3][19].  The far
// tables are evaluated from the same partial sums, in the same order, by the same code as the near ones: equal MLPs give equal bits.
struct SeFar {
    const float *w1, *b1, *w2, *b2;
    float* tab;
};

template <bool SPLIT, typename FT>
__device__ __forceinline__ void se_squeeze_excite_body(const FT* __restrict__ flow, int HW, const Variant& v,
                                                       float* __restrict__ partial, unsigned* __restrict__ counters,
                                                       const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const float* __restrict__ b2,
                                                       const float* __restrict__ wstatic, float* __restrict__ tab,
                                                       unsigned* __restrict__ range_reset, int sel, const SeFar& far) {
    const int chunk = blockIdx.x, s = pair_source(blockIdx.y, sel), b = blockIdx.z;
    if (range_reset && chunk == 0 && blockIdx.y == 0 && b == 0 && threadIdx.x == 0) range_reset[RANGE_SNAP] = 0u;      // as se_excite
    const FT* f = flow + ((size_t)b * 4 + s) * HW * 2;
    const int nvec = HW / 2;                                   // HW is a multiple of 16
    const int per = (nvec + SQ_CHUNKS - 1) / SQ_CHUNKS;
    const int beg = chunk * per, end = min(beg + per, nvec);
    float sx = 0.f, sy = 0.f;
    for (int i = beg + threadIdx.x; i < end; i += 256) {
        float4 q = widen_fetch4(f + (size_t)i * 4);
        if (v.norm_flow) {
            q.x = (q.x - 0.32140523f) / 15.384229f; q.y = (q.y - 0.32140523f) / 15.384229f;
            q.z = (q.z - 0.32140523f) / 15.384229f; q.w = (q.w - 0.32140523f) / 15.384229f;
        }
        if (v.abs_mode & 1) { q.x = fabsf(q.x); q.z = fabsf(q.z); }
        if (v.abs_mode & 2) { q.y = fabsf(q.y); q.w = fabsf(q.w); }
        sx += q.x + q.z;
        sy += q.y + q.w;
    }
    __shared__ float red[2][4];
    __shared__ unsigned ticket;
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[0][wid] = sx; red[1][wid] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = partial + (((size_t)b * 2 + s) * SQ_CHUNKS + chunk) * 2;
        agent_store(o, (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
        agent_store(o + 1, (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
        agent_stores_done();
    }
    if (!last_workgroup(counters + b, (unsigned)(pairs_per_window(sel) * SQ_CHUNKS), &ticket)) return;
    if (wid < 3 && pair_reads_frame(wid, sel)) {
        se_excite_wave<true>(partial, HW, v, b, wid, lane, w1, b1, w2, b2, wstatic, tab);
        if (SPLIT) se_excite_wave<true>(partial, HW, v, b, wid, lane, far.w1, far.b1, far.w2, far.b2, wstatic, far.tab);
    }
    if (threadIdx.x == 0) __hip_atomic_store(counters + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename FT>
__global__ __launch_bounds__(256) void se_squeeze_excite(const FT* __restrict__ flow, int HW, Variant v,
                                                         float* __restrict__ partial, unsigned* __restrict__ counters,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ b2,
                                                         const float* __restrict__ wstatic, float* __restrict__ tab,
                                                         unsigned* __restrict__ range_reset, int sel) {
    se_squeeze_excite_body<false>(flow, HW, v, partial, counters, w1, b1, w2, b2, wstatic, tab, range_reset, sel, SeFar{});
}

// ... of the depth-split source: the triplet's last workgroup evaluates the near tables, then the far ones
template <typename FT>
__global__ __launch_bounds__(256) void se_squeeze_excite_split(const FT* __restrict__ flow, int HW, Variant v,
                                                               float* __restrict__ partial, unsigned* __restrict__ counters,
                                                               const float* __restrict__ w1, const float* __restrict__ b1,
                                                               const float* __restrict__ w2, const float* __restrict__ b2,
                                                               float* __restrict__ tab, unsigned* __restrict__ range_reset, int sel, SeFar far) {
    se_squeeze_excite_body<true>(flow, HW, v, partial, counters, w1, b1, w2, b2, nullptr, tab, range_reset, sel, far);
}

// Class-table SE squeeze (att_source 4..10): one workgroup per (chunk, frame, triplet), grid (SQ_CHUNKS, att_se_frames, B); frame =
// blockIdx.y + 3 - att_se_frames (the `_wo_tgt' sources skip the target).  It writes partial[b][frame][chunk][SQ_REC] words:
//   histogram sources: [0, 19) label counts of the chunk (the att_lookup rule: finite values in (-1, 19), truncated; anything else
//                      counts in no bin but in the HW denominator, davo.py:1115), SegFlow: [19, 21) float sums of the SE-transformed
//                      flow (src frames; the target's flow is zeros and has no sums);
//   rgb sources:       [0, 3) sums of the frame's u8 channel bytes.
// A thread takes 4 horizontally adjacent pixels per step (one label_fetch4 - a float4 of labels, or four bytes in the byte
// format LT = uint8_t, input_decode.h - 12 strip bytes, one flow_fetch4 of flow in the flow format FT).  Label counts:
// per class one 64-bit ballot per pixel slot and a scalar popcount - wave-uniform sums with no LDS atomics on a hot bin (the labels
// come in 8x8 blocks of one class).  The loop's trip count is uniform, so every lane sees every ballot.  The counts and byte sums
// are exact integers and the flow sums use a fixed tree: bitwise reproducible.  FOLD: the workgroup that delivers the triplet's
// last record evaluates its three tables (se_squeeze_excite's protocol, pose_tail.h).
template <bool FOLD, typename LT, typename FT>
__global__ __launch_bounds__(256) void se_class_squeeze(const uint8_t* __restrict__ img, const FT* __restrict__ flow,
                                                        const LT* __restrict__ seg, int H, int W, Variant v,
                                                        unsigned* __restrict__ partial, unsigned* __restrict__ counters,
                                                        const float* __restrict__ w1, const float* __restrict__ b1,
                                                        const float* __restrict__ w2, const float* __restrict__ b2,
                                                        float* __restrict__ tab, unsigned* __restrict__ range_reset, int sel) {
    const int a = v.att_source, nf = att_se_frames(a);
    // one pair selected (params.h): grid y is nf - 1 - the target where the source covers it, then the selected source frame
    const int chunk = blockIdx.x, b = blockIdx.z;
    const int frame = sel == PAIRS_BOTH ? (int)blockIdx.y + 3 - nf : ((nf == 3 && blockIdx.y == 0) ? 0 : 1 + (sel >> 1));
    if (FOLD && range_reset && chunk == 0 && blockIdx.y == 0 && b == 0 && threadIdx.x == 0) range_reset[RANGE_SNAP] = 0u;   // as se_excite
    const int HW = H * W;
    const int nunits = HW >> 2;                                // 4-pixel units; W is a multiple of 4, so a unit never wraps a row
    const int per = (nunits + SQ_CHUNKS - 1) / SQ_CHUNKS;
    const int beg = chunk * per, end = min(beg + per, nunits);
    const bool hist = att_desc_hist(a), rgb = att_desc_rgb(a), fl = att_desc_flow(a) && frame >= 1;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // strip slot / seg file plane of the frame: (tgt, src0, src1) -> strip src0|tgt|src1 (data_loader.py:537-557), seg file
    // order src0, tgt, src1 (davo.py:998-1004)
    const int slot = frame == 0 ? 1 : frame == 1 ? 0 : 2;
    const LT* lab = seg + ((size_t)b * 3 + slot) * HW;         // LT: the label format, float32 or bytes (input_decode.h)
    const FT* fv = flow + ((size_t)b * 4 + (frame >= 1 ? frame - 1 : 0)) * HW * 2;      // FT: the flow format (input_decode.h)
    unsigned cnt[NCLS];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) cnt[c] = 0u;
    unsigned sr = 0u, sg = 0u, sb = 0u;
    float sx = 0.f, sy = 0.f;
    for (int base = beg; base < end; base += 256) {            // uniform trip count
        const int i = base + threadIdx.x;
        const bool ok = i < end;
        if (hist) {
            const LabelIds4 q = ok ? label_fetch4(lab, (size_t)i << 2) : LabelIds4{{-1, -1, -1, -1}};
            const int* id = q.id;
#pragma unroll
            for (int c = 0; c < NCLS; ++c)
                cnt[c] += (unsigned)(__popcll(__ballot(id[0] == c)) + __popcll(__ballot(id[1] == c)) +
                                     __popcll(__ballot(id[2] == c)) + __popcll(__ballot(id[3] == c)));
        }
        if (rgb && ok) {
            const int p = i << 2, y = p / W, x = p - y * W;
            const uint32_t* q = reinterpret_cast<const uint32_t*>(img + ((size_t)b * H + y) * (size_t)(9 * W) + (size_t)(slot * W + x) * 3);
            const uint32_t q0 = q[0], q1 = q[1], q2 = q[2];         // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            sr += (q0 & 255u) + (q0 >> 24) + ((q1 >> 16) & 255u) + ((q2 >> 8) & 255u);
            sg += ((q0 >> 8) & 255u) + (q1 & 255u) + (q1 >> 24) + ((q2 >> 16) & 255u);
            sb += ((q0 >> 16) & 255u) + ((q1 >> 8) & 255u) + (q2 & 255u) + (q2 >> 24);
        }
        if (fl && ok) {
            const Flow4 f = flow_fetch4(fv + (size_t)(2 * i) * 4);
            sx += (se_flow_transform(f.v[0], 0, v) + se_flow_transform(f.v[2], 0, v)) + (se_flow_transform(f.v[4], 0, v) + se_flow_transform(f.v[6], 0, v));
            sy += (se_flow_transform(f.v[1], 1, v) + se_flow_transform(f.v[3], 1, v)) + (se_flow_transform(f.v[5], 1, v) + se_flow_transform(f.v[7], 1, v));
        }
    }
    __shared__ unsigned red_u[4][NCLS];
    __shared__ float red_f[2][4];
    __shared__ unsigned ticket;
    if (hist && lane == 0) {
#pragma unroll
        for (int c = 0; c < NCLS; ++c) red_u[wid][c] = cnt[c];     // wave-uniform
    }
    if (rgb) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sr += __shfl_xor(sr, o, 64); sg += __shfl_xor(sg, o, 64); sb += __shfl_xor(sb, o, 64);
        }
        if (lane == 0) { red_u[wid][0] = sr; red_u[wid][1] = sg; red_u[wid][2] = sb; }
    }
    if (fl) {
        sx = wave_sum(sx);
        sy = wave_sum(sy);
        if (lane == 0) { red_f[0][wid] = sx; red_f[1][wid] = sy; }
    }
    __syncthreads();
    if (wid == 0) {
        unsigned* o = partial + (((size_t)b * 3 + frame) * SQ_CHUNKS + chunk) * SQ_REC;
        const int nu = hist ? NCLS : rgb ? 3 : 0;
        unsigned w = 0u;
        bool store = false;
        if (lane < nu) {
            w = (red_u[0][lane] + red_u[1][lane]) + (red_u[2][lane] + red_u[3][lane]);
            store = true;
        } else if (fl && (lane == NCLS || lane == NCLS + 1)) {
            const int c = lane - NCLS;
            w = __float_as_uint((red_f[c][0] + red_f[c][1]) + (red_f[c][2] + red_f[c][3]));
            store = true;
        }
        if (store) {
            if (FOLD) __hip_atomic_store(o + lane, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else o[lane] = w;
        }
        if (FOLD) agent_stores_done();
    }
    if (!FOLD) return;
    if (!last_workgroup(counters + b, (unsigned)((nf - (sel == PAIRS_BOTH ? 0 : 1)) * SQ_CHUNKS), &ticket)) return;
    if (wid < 3 && pair_reads_frame(wid, sel)) se_class_excite_wave<true>(partial, HW, v, b, wid, lane, w1, b1, w2, b2, tab);
    if (threadIdx.x == 0) __hip_atomic_store(counters + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Depth-source SE squeeze (att_source 11, 12; davo.py:1109, 1211-1227): grid (SQ_CHUNKS, 3 frames, B), one workgroup per (chunk,
// frame, triplet).  The SUMMED-PLANES form: each of the three depth planes is summed once (12 B per pixel and triplet) and the
// excitation adds S_frame + S_tgt (se_class_excite_wave), instead of summing depth_frame + depth_tgt per pixel; the two differ by
// float32 rounding only.  A thread takes four horizontally adjacent pixels (one 16-byte load) per step and adds them as
// (x + y) + (z + w); then the fixed wave butterfly and a fixed tree over the four waves: one float32 word per record
// (partial[b][frame][chunk][0]), bitwise the same run after run, no atomics on the sums.  depth is [B][3 file planes: src0, tgt,
// src1][H][W] in the depth format DT (float or in_f16, input_decode.h), 16-byte aligned; H*W is a multiple of 16.  A unit comes
// from one widen_fetch4, so the chunking, the sum's order and every bit are the float32 format's.  FOLD: the workgroup that
// delivers the triplet's last record evaluates its three tables (se_squeeze_excite's protocol, pose_tail.h).
template <bool FOLD, typename DT>
__global__ __launch_bounds__(256) void se_depth_squeeze(const DT* __restrict__ depth, int HW, Variant v,
                                                        unsigned* __restrict__ partial, unsigned* __restrict__ counters,
                                                        const float* __restrict__ w1, const float* __restrict__ b1,
                                                        const float* __restrict__ w2, const float* __restrict__ b2,
                                                        float* __restrict__ tab, unsigned* __restrict__ range_reset, int sel) {
    // one pair selected (params.h): grid y is 2 - the target, whose sum enters every descriptor, and the selected source frame
    const int chunk = blockIdx.x, b = blockIdx.z;
    const int frame = (sel == PAIRS_BOTH || blockIdx.y == 0) ? (int)blockIdx.y : 1 + (sel >> 1);
    if (FOLD && range_reset && chunk == 0 && frame == 0 && b == 0 && threadIdx.x == 0) range_reset[RANGE_SNAP] = 0u;   // as se_excite
    const int plane = frame == 0 ? 1 : frame == 1 ? 0 : 2;     // (tgt, src0, src1) -> file order src0, tgt, src1 (davo.py:991-996)
    const DT* dp = depth + ((size_t)b * 3 + plane) * HW;
    const int nunits = HW >> 2;
    const int per = (nunits + SQ_CHUNKS - 1) / SQ_CHUNKS;
    const int beg = chunk * per, end = min(beg + per, nunits);
    float sum = 0.f;
    for (int i = beg + threadIdx.x; i < end; i += 256) {
        const float4 q = widen_fetch4(dp + (size_t)i * 4);
        sum += (q.x + q.y) + (q.z + q.w);
    }
    __shared__ float red[4];
    __shared__ unsigned ticket;
    sum = wave_sum(sum);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned* o = partial + (((size_t)b * 3 + frame) * SQ_CHUNKS + chunk) * SQ_REC;
        const unsigned w = __float_as_uint((red[0] + red[1]) + (red[2] + red[3]));
        if (FOLD) {
            __hip_atomic_store(o, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            agent_stores_done();
        } else {
            o[0] = w;
        }
    }
    if (!FOLD) return;
    if (!last_workgroup(counters + b, (unsigned)((1 + pairs_per_window(sel)) * SQ_CHUNKS), &ticket)) return;
    if (wid < 3 && pair_reads_frame(wid, sel)) se_class_excite_wave<true>(partial, HW, v, b, wid, lane, w1, b1, w2, b2, tab);
    if (threadIdx.x == 0) __hip_atomic_store(counters + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Mask + pack: one thread per 4 horizontally adjacent pixels of one pair image.
// out[n][y][x][0..LD), n = the pair image of (window b, source s) under the batch's pair selection (params.h):
//                            LD = 8 : tgt rgb | src rgb*att | flow*att      (product layout; the
//                                      two identically-zero tgt-flow channels are dropped)
//                            LD = 10: tgt rgb | 0 0 | src rgb*att | flow*att (reference layout)
// v0 variants (rgb only) leave the flow slots zero.
// LT: the label format, float32 or bytes; a thread's four labels of a plane come from one label_fetch4 (input_decode.h).
// FT: the flow format, float32 or binary16; a thread's four pixels of flow come from one flow_fetch4 (input_decode.h).
// DSPLIT (att_source 13, the depth-split flow attention): per 4-pixel group one more widen_fetch4 (DT: the depth format, float32 or
// binary16, input_decode.h), of the depth plane of the source frame the label map belongs to (file plane 0 or 2), and each pixel's class is looked up in the near table `tab' or the far table
// `ds.tab_far' by att_lookup_split (input_decode.h, with DepthSplit); everything else is the same code.  The target's map is ones.
template <int LD, bool DSPLIT, typename LT, typename FT, typename DT>
__device__ __forceinline__ void mask_pack_body(const uint8_t* __restrict__ img, const FT* __restrict__ flow,
                                               const LT* __restrict__ seg, const float* __restrict__ tab,
                                               const Variant& v, int B, int sel, int H, int W, float* __restrict__ out, const DepthSplitOf<DT>& ds) {
    const int W4 = W >> 2;
    const long total = (long)B * pairs_per_window(sel) * H * W4;
    const long gid_raw = (long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = gid_raw < total;
    constexpr bool STAGED = LD == 16 || LD == 8;               // 32 B per pixel: the stores leave through LDS (below)
    if (!STAGED && !valid) return;
    const long gid = valid ? gid_raw : total - 1;             // staged: every thread reaches the barrier below
    const int x4 = (int)(gid % W4);
    long t = gid / W4;
    const int y = (int)(t % H); t /= H;
    const int n = (int)t, s = pair_source(n, sel), b = pair_window(n, sel);
    const int x = x4 * 4;

    const uint8_t* row = img + ((size_t)b * H + y) * (size_t)(9 * W);
    const uint32_t* pt = reinterpret_cast<const uint32_t*>(row + (size_t)(W + x) * 3);
    const uint32_t* ps = reinterpret_cast<const uint32_t*>(row + (size_t)((s ? 2 * W : 0) + x) * 3);
    const uint32_t t0 = pt[0], t1 = pt[1], t2 = pt[2];
    const uint32_t s0 = ps[0], s1 = ps[1], s2 = ps[2];
    const uint8_t tb[12] = {(uint8_t)t0, (uint8_t)(t0 >> 8), (uint8_t)(t0 >> 16), (uint8_t)(t0 >> 24),
                            (uint8_t)t1, (uint8_t)(t1 >> 8), (uint8_t)(t1 >> 16), (uint8_t)(t1 >> 24),
                            (uint8_t)t2, (uint8_t)(t2 >> 8), (uint8_t)(t2 >> 16), (uint8_t)(t2 >> 24)};
    const uint8_t sb[12] = {(uint8_t)s0, (uint8_t)(s0 >> 8), (uint8_t)(s0 >> 16), (uint8_t)(s0 >> 24),
                            (uint8_t)s1, (uint8_t)(s1 >> 8), (uint8_t)(s1 >> 16), (uint8_t)(s1 >> 24),
                            (uint8_t)s2, (uint8_t)(s2 >> 8), (uint8_t)(s2 >> 16), (uint8_t)(s2 >> 24)};

    const size_t pix = (size_t)y * W + x;
    const LabelIds4 sg = label_fetch4(seg + ((size_t)b * 3 + (s ? 2 : 0)) * H * W, pix);
    const float* tab_s = tab + ((size_t)b * 3 + 1 + s) * NCLS;
    // tf.ones_like overrides are ones everywhere, ignore-label pixels included: every frame for
    // -no_segmask (davo.py:1387), the tgt frame unless static_all (davo.py:1394,1411).
    float as[4] = {1.f, 1.f, 1.f, 1.f};
    if (DSPLIT) {
        const float4 dp = widen_fetch4(ds.depth + ((size_t)b * 3 + (s ? 2 : 0)) * H * W + pix);
        const float* far_s = ds.tab_far + ((size_t)b * 3 + 1 + s) * NCLS;
        as[0] = att_lookup_split(tab_s, far_s, ds.thr, dp.x, sg.id[0]); as[1] = att_lookup_split(tab_s, far_s, ds.thr, dp.y, sg.id[1]);
        as[2] = att_lookup_split(tab_s, far_s, ds.thr, dp.z, sg.id[2]); as[3] = att_lookup_split(tab_s, far_s, ds.thr, dp.w, sg.id[3]);
    } else if (v.att_source != 0) {
        as[0] = att_lookup_id(tab_s, sg.id[0]); as[1] = att_lookup_id(tab_s, sg.id[1]);
        as[2] = att_lookup_id(tab_s, sg.id[2]); as[3] = att_lookup_id(tab_s, sg.id[3]);
    }
    float at[4] = {1.f, 1.f, 1.f, 1.f};
    if (!DSPLIT && att_tgt_attended(v.att_source)) {                     // static_all / a with-target class table: tgt frame is masked too
        const LabelIds4 tg = label_fetch4(seg + ((size_t)b * 3 + 1) * H * W, pix);
        const float* tab_t = tab + (size_t)b * 3 * NCLS;
        at[0] = att_lookup_id(tab_t, tg.id[0]); at[1] = att_lookup_id(tab_t, tg.id[1]);
        at[2] = att_lookup_id(tab_t, tg.id[2]); at[3] = att_lookup_id(tab_t, tg.id[3]);
    }
    float fl[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (v.cin_per_frame == 5) {
        const Flow4 f = flow_fetch4(flow + (((size_t)b * 4 + s) * H * W + pix) * 2);
#pragma unroll
        for (int k = 0; k < 8; ++k) fl[k] = f.v[k];
    }
    constexpr int OUT_FLOATS = LD == 16 ? 8 : LD;          // LD 16 = split-fp16 layout, 8 floats' worth per pixel
    float* o = out + (((size_t)n * H + y) * W + x) * OUT_FLOATS;
    // LD 16 / 8: a thread's 4 pixels are 8 x 16 B, 128 B apart from its neighbour's - stored directly, every store
    // instruction would touch 64 separate lines.  The workgroup's 32 KB (contiguous: output offset = gid * 128 B)
    // go through LDS instead and leave as 1 KiB per wave instruction.  Unit t*8 + (k ^ (t&7)): 2-way bank conflicts
    // on the way in, none on the way out.  (Round 4: the float32 layout too - mask_pack<8> stored directly until then:
    // 46 us against mask_pack<16>'s 31 for the same bytes.)
    __shared__ float4 stage[STAGED ? 256 * 8 : 1];
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        const float mt = v.mask_rgb ? at[px] : 1.f, ms = v.mask_rgb ? as[px] : 1.f;
        const float mi = v.mask_info ? as[px] : 1.f;
        float r[10];
        r[0] = u8_to_unit(tb[3 * px]); r[1] = u8_to_unit(tb[3 * px + 1]); r[2] = u8_to_unit(tb[3 * px + 2]);
        r[3] = u8_to_unit(sb[3 * px]); r[4] = u8_to_unit(sb[3 * px + 1]); r[5] = u8_to_unit(sb[3 * px + 2]);
        if (v.mask_rgb) {
            r[0] *= mt; r[1] *= mt; r[2] *= mt;
            r[3] *= ms; r[4] *= ms; r[5] *= ms;
        }
        r[6] = v.mask_info ? fl[2 * px] * mi : fl[2 * px];
        r[7] = v.mask_info ? fl[2 * px + 1] * mi : fl[2 * px + 1];
        if (LD == 16) {
            // split-fp16 form for the f16x3 convolutions: per pixel [8 hi halves | 8 lo halves]
            // (32 bytes, the same as 8 floats): x = hi + lo
            _Float16 hl[16];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const _Float16 h = (_Float16)r[k];
                hl[k] = h;
                hl[8 + k] = (_Float16)(r[k] - (float)h);
            }
            const int t8 = threadIdx.x * 8, sw = threadIdx.x & 7;
            stage[t8 + ((2 * px) ^ sw)] = *reinterpret_cast<const float4*>(&hl[0]);
            stage[t8 + ((2 * px + 1) ^ sw)] = *reinterpret_cast<const float4*>(&hl[8]);
        } else if (LD == 8) {
            const int t8 = threadIdx.x * 8, sw = threadIdx.x & 7;
            stage[t8 + ((2 * px) ^ sw)] = make_float4(r[0], r[1], r[2], r[3]);
            stage[t8 + ((2 * px + 1) ^ sw)] = make_float4(r[4], r[5], r[6], r[7]);
        } else {
            float* q = o + px * 10;
            q[0] = r[0]; q[1] = r[1]; q[2] = r[2]; q[3] = 0.f; q[4] = 0.f;
            q[5] = r[3]; q[6] = r[4]; q[7] = r[5]; q[8] = r[6]; q[9] = r[7];
        }
    }
    if (STAGED) {
        __syncthreads();
        float4* og = reinterpret_cast<float4*>(out) + (size_t)blockIdx.x * (256 * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = i * 256 + threadIdx.x;              // physical unit; owner thread t = j >> 3
            const int k = (j & 7) ^ ((j >> 3) & 7);           // its logical 16-byte piece
            if ((long)blockIdx.x * 256 + (j >> 3) < total) og[(j & ~7) + k] = stage[j];
        }
    }
}

template <int LD, typename LT, typename FT>
__global__ __launch_bounds__(256) void mask_pack(const uint8_t* __restrict__ img, const FT* __restrict__ flow,
                                                 const LT* __restrict__ seg, const float* __restrict__ tab,
                                                 Variant v, int B, int sel, int H, int W, float* __restrict__ out) {
    mask_pack_body<LD, false>(img, flow, seg, tab, v, B, sel, H, W, out, DepthSplit{});
}

template <int LD, typename LT, typename FT, typename DT>
__global__ __launch_bounds__(256) void mask_pack_depthsplit(const uint8_t* __restrict__ img, const FT* __restrict__ flow,
                                                            const LT* __restrict__ seg, const float* __restrict__ tab,
                                                            Variant v, int B, int sel, int H, int W, float* __restrict__ out, DepthSplitOf<DT> ds) {
    mask_pack_body<LD, true>(img, flow, seg, tab, v, B, sel, H, W, out, ds);
}

// Mask + pack of the three-frame PoseNN (davo_set_posenn_topology; nets/posenn.py:78, davo.py:1460): one thread per 4 horizontally
// adjacent pixels of one WINDOW, out[b][y][x][0..16):
//   tgt rgb*att_t (3) | src0 rgb*att_0 (3) | flow0*att_0 (2) | src1 rgb*att_1 (3) | flow1*att_1 (2) | 0 0 0
// (the target's two identically-zero info channels are dropped, as the 8-channel layout drops them; v0 leaves the flow slots zero).
// H3 false: 16 floats per pixel; true: the split-fp16 form [16 hi | 16 lo] halves, the blocked layout of a 16-channel f16x3
// tensor.  64 B per pixel either way.  Each of the three label maps and two flow planes of the group is fetched once
// (label_fetch4 / flow_fetch4); the products are mask_pack's, in mask_pack's order.  The stores leave through LDS like
// mask_pack's STAGED path: a thread's 256 B are 16 units of 16 B, unit t*16 + (k ^ (t & 15)), the workgroup's 32 KB are contiguous
// in the output (offset = gid * 256 B) and leave as 1 KiB per wave instruction.
constexpr int PACK3_THREADS = 128;
template <bool H3, typename LT, typename FT>
__global__ __launch_bounds__(PACK3_THREADS) void mask_pack3(const uint8_t* __restrict__ img, const FT* __restrict__ flow,
                                                           const LT* __restrict__ seg, const float* __restrict__ tab,
                                                           Variant v, int B, int H, int W, float* __restrict__ out) {
    const int W4 = W >> 2;
    const long total = (long)B * H * W4;
    const long gid_raw = (long)blockIdx.x * PACK3_THREADS + threadIdx.x;
    const long gid = gid_raw < total ? gid_raw : total - 1;     // every thread reaches the barrier below
    const int x4 = (int)(gid % W4);
    long t = gid / W4;
    const int y = (int)(t % H);
    const int b = (int)(t / H);
    const int x = x4 * 4;
    const size_t HW = (size_t)H * W, pix = (size_t)y * W + x;

    // strip slots src0 | tgt | src1 (data_loader.py:537-557); frame f = 0 tgt, 1 src0, 2 src1
    const uint8_t* row = img + ((size_t)b * H + y) * (size_t)(9 * W);
    uint8_t px8[3][12];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        const int slot = f == 0 ? 1 : f == 1 ? 0 : 2;
        const uint32_t* q = reinterpret_cast<const uint32_t*>(row + (size_t)(slot * W + x) * 3);
        const uint32_t q0 = q[0], q1 = q[1], q2 = q[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px8[f][k] = (uint8_t)(q0 >> (8 * k)); px8[f][4 + k] = (uint8_t)(q1 >> (8 * k)); px8[f][8 + k] = (uint8_t)(q2 >> (8 * k));
        }
    }
    // attention per frame and pixel: ones unless the variant looks the pixel's class up (mask_pack's rules); seg file planes
    // src0, tgt, src1 (davo.py:998-1004)
    float att[3][4];
#pragma unroll
    for (int f = 0; f < 3; ++f)
#pragma unroll
        for (int k = 0; k < 4; ++k) att[f][k] = 1.f;
    if (v.att_source != 0) {
#pragma unroll
        for (int f = 1; f < 3; ++f) {
            const LabelIds4 sg = label_fetch4(seg + ((size_t)b * 3 + (f == 1 ? 0 : 2)) * HW, pix);
            const float* tab_f = tab + ((size_t)b * 3 + f) * NCLS;
#pragma unroll
            for (int k = 0; k < 4; ++k) att[f][k] = att_lookup_id(tab_f, sg.id[k]);
        }
    }
    if (att_tgt_attended(v.att_source)) {
        const LabelIds4 tg = label_fetch4(seg + ((size_t)b * 3 + 1) * HW, pix);
        const float* tab_t = tab + (size_t)b * 3 * NCLS;
#pragma unroll
        for (int k = 0; k < 4; ++k) att[0][k] = att_lookup_id(tab_t, tg.id[k]);
    }
    float fl[2][8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int k = 0; k < 8; ++k) fl[s][k] = 0.f;
    if (v.cin_per_frame == 5) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const Flow4 f = flow_fetch4(flow + (((size_t)b * 4 + s) * HW + pix) * 2);
#pragma unroll
            for (int k = 0; k < 8; ++k) fl[s][k] = f.v[k];
        }
    }
    __shared__ float4 stage[PACK3_THREADS * 16];
    const int t16 = threadIdx.x * 16, sw = threadIdx.x & 15;
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        float r[16];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r[k] = u8_to_unit(px8[0][3 * px + k]);
            r[3 + k] = u8_to_unit(px8[1][3 * px + k]);
            r[8 + k] = u8_to_unit(px8[2][3 * px + k]);
            if (v.mask_rgb) { r[k] *= att[0][px]; r[3 + k] *= att[1][px]; r[8 + k] *= att[2][px]; }
        }
        r[6] = v.mask_info ? fl[0][2 * px] * att[1][px] : fl[0][2 * px];
        r[7] = v.mask_info ? fl[0][2 * px + 1] * att[1][px] : fl[0][2 * px + 1];
        r[11] = v.mask_info ? fl[1][2 * px] * att[2][px] : fl[1][2 * px];
        r[12] = v.mask_info ? fl[1][2 * px + 1] * att[2][px] : fl[1][2 * px + 1];
        r[13] = 0.f; r[14] = 0.f; r[15] = 0.f;
        if (H3) {
            _Float16 hl[32];                       // [16 hi | 16 lo]: x = hi + lo
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const _Float16 h = (_Float16)r[k];
                hl[k] = h;
                hl[16 + k] = (_Float16)(r[k] - (float)h);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) stage[t16 + ((4 * px + u) ^ sw)] = *reinterpret_cast<const float4*>(&hl[8 * u]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) stage[t16 + ((4 * px + u) ^ sw)] = make_float4(r[4 * u], r[4 * u + 1], r[4 * u + 2], r[4 * u + 3]);
        }
    }
    __syncthreads();
    float4* og = reinterpret_cast<float4*>(out) + (size_t)blockIdx.x * (PACK3_THREADS * 16);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = i * PACK3_THREADS + threadIdx.x;    // physical unit; owner thread j >> 4
        const int k = (j & 15) ^ ((j >> 4) & 15);         // its logical 16-byte piece
        if ((long)blockIdx.x * PACK3_THREADS + (j >> 4) < total) og[(j & ~15) + k] = stage[j];
    }
}

// Pose head tail: pred (1x1, 256 -> 3, linear) + mean over H3 x W3 + 0.01 scale
// (nets/posenn.py:240-241,248-250).  pred and the mean are both linear, so
//   pose[n][head*3+j] = 0.01 * ( b[j] + (1/P) * sum_c ( sum_p cnv7[n][p][head][c] ) * Wp[c][j] ).
// Pass 1: grid (PH_SPLIT, 2B images, 2 heads), 256 threads = one per cnv7 channel (coalesced rows);
// block s sums its slice of the P pixels and writes 3 partial dot products.  Pass 2 (pose_finish)
// adds the PH_SPLIT partials in a fixed order -> bitwise reproducible.

// NC: columns of a head's pred: 3 (one pose per pair image) or 6 (the three-frame PoseNN: both poses of a window from one image,
// nets/posenn.py:120; the coupled network: all six components from its one head, nets/posenn.py:176-179), wpred [HEADS][256][NC],
// partial [images][HEADS][PH_SPLIT][NC]; the sums of a column are the same in either form.
// HEADS: heads side by side in a cnv7 pixel, 256 channels each: 2 (rotation | translation, grid z) or 1 (the coupled network).
template <int NC, int HEADS = 2>
__global__ __launch_bounds__(256) void pose_head_partial(const float* __restrict__ c7, int P,
                                                         const float* __restrict__ wpred /*[HEADS][256][NC]*/,
                                                         float* __restrict__ partial /*[images][HEADS][PH_SPLIT][NC]*/) {
    constexpr int LD = HEADS * 256;        // floats per cnv7 pixel
    const int sp = blockIdx.x, n = blockIdx.y, head = blockIdx.z, c = threadIdx.x;
    const int per = (P + PH_SPLIT - 1) / PH_SPLIT;
    const int p0 = sp * per, p1 = min(p0 + per, P);
    const float* src = c7 + (size_t)n * P * LD + head * 256 + c;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = p0;
    for (; p + 4 <= p1; p += 4) {
        s0 += src[(size_t)p * LD]; s1 += src[(size_t)(p + 1) * LD];
        s2 += src[(size_t)(p + 2) * LD]; s3 += src[(size_t)(p + 3) * LD];
    }
    for (; p < p1; ++p) s0 += src[(size_t)p * LD];
    const float sc = (s0 + s1) + (s2 + s3);
    const float* wp = wpred + ((size_t)head * 256 + c) * NC;
    float v[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) v[j] = sc * wp[j];
    __shared__ float red[NC][4];
    const int lane = c & 63, wid = c >> 6;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        v[j] = wave_sum(v[j]);
        if (lane == 0) red[j][wid] = v[j];
    }
    __syncthreads();
    if (c < NC)
        partial[(((size_t)n * HEADS + head) * PH_SPLIT + sp) * NC + c] = (red[c][0] + red[c][1]) + (red[c][2] + red[c][3]);
}

__global__ __launch_bounds__(64) void pose_finish(const float* __restrict__ partial, int NB, int P,
                                                  const float* __restrict__ bpred /*[2][3]*/,
                                                  float* __restrict__ pose /*[B][2][6]*/, int sel) {
    const int i = blockIdx.x * 64 + threadIdx.x;           // (n, head, j)
    if (i >= NB * 6) return;
    const int n = i / 6, hj = i - n * 6, head = hj / 3, j = hj - head * 3;
    const float* pp = partial + ((size_t)n * 2 + head) * PH_SPLIT * 3 + j;
    float tot = 0.f;
#pragma unroll
    for (int s = 0; s < PH_SPLIT; ++s) tot += pp[s * 3];
    pose_store(pose, n, hj, sel, 0.01f * (tot / (float)P + bpred[hj]));
}

// ... of the three-frame PoseNN: avg [B][6] per head, reshaped [-1, 2, 3] (nets/posenn.py:121-127):
// pose[b][s][3 head + k] = 0.01 * avg_head[b][3 s + k]; the PH_SPLIT partials in the same fixed order
__global__ __launch_bounds__(64) void pose_finish6(const float* __restrict__ partial /*[B][2][PH_SPLIT][6]*/, int B, int P,
                                                   const float* __restrict__ bpred /*[2][6]*/,
                                                   float* __restrict__ pose /*[B][2][6]*/) {
    const int i = blockIdx.x * 64 + threadIdx.x;           // (b, s, head, k): the index of the pose array itself
    if (i >= B * 12) return;
    const int b = i / 12, r = i - b * 12, s = r / 6, hk = r - s * 6, head = hk / 3, k = hk - head * 3;
    const int col = 3 * s + k;
    const float* pp = partial + ((size_t)b * 2 + head) * PH_SPLIT * 6 + col;
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < PH_SPLIT; ++q) tot += pp[q * 6];
    pose[i] = 0.01f * (tot / (float)P + bpred[head * 6 + col]);
}

// ... of the coupled network (nets/posenn.py:176-179): pred's six columns ARE the pose of pair image n, unpermuted:
// pose[pair_pose_row(n, sel)][k] = 0.01 * avg[n][k]; the PH_SPLIT partials in the same fixed order, stored through pose_store (one
// selected pair: +0.0 into the window's other row)
__global__ __launch_bounds__(64) void pose_finish_coupled(const float* __restrict__ partial /*[NB][PH_SPLIT][6]*/, int NB, int P,
                                                          const float* __restrict__ bpred /*[6]*/,
                                                          float* __restrict__ pose /*[B][2][6]*/, int sel) {
    const int i = blockIdx.x * 64 + threadIdx.x;           // (n, k)
    if (i >= NB * 6) return;
    const int n = i / 6, k = i - n * 6;
    const float* pp = partial + (size_t)n * PH_SPLIT * 6 + k;
    float tot = 0.f;
#pragma unroll
    for (int s = 0; s < PH_SPLIT; ++s) tot += pp[s * 6];
    pose_store(pose, n, k, sel, 0.01f * (tot / (float)P + bpred[k]));
}

// Pose from the per-tile partial sums cnv7's fused epilogue wrote (conv_igemm_h3.h, y_mode 2):
// partial[head][mtile][ntile][slot][k], slot 0 = the tile's first image, slot 1 = the next one.  One 64-lane wave per
// output (n, head, k): the tiles' terms are spread over the lanes and added by a fixed butterfly (pose_tail.h) — a
// single thread walking 56 dependent loads (128x32 tiles at batch 1) took 12 us.
// Range guard, device side (range_guard.hip: tickets).  The batch's range record is complete when its last kernel runs (stream order), so
// that kernel can see the verdict the host will reach later: if a layer left the fp16-pair range the batch will be re-issued,
// and the inputs it was issued on are copied into the context's ring slot NOW - behind the kernels that read them, ahead of
// anything the caller orders behind the batch (e.g. the H2D of the next batch into the same buffers).  A batch in range -
// every batch of a well-ranged checkpoint - costs six loads per thread and no copy.  Only flow planes 0 and 1 are read by the
// path (davo.py:978-982): the first half of every window's block.
// phase 1 (top of the kernel, so that the memory-side round trips pass behind the kernel's own work): the maxima, and the first half of the mirror
struct RangePeek { unsigned w[6]; bool fails; };       // (the feature-attention word is judged and mirrored at once: no copy kept)
__device__ __forceinline__ RangePeek range_peek(const SnapArgs& a, unsigned worker) {
    RangePeek r{};
    if (!a.record) return r;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        r.w[i] = __atomic_load_n(a.record + i, __ATOMIC_RELAXED);
        r.fails |= range_value_fails(__uint_as_float(r.w[i]));
    }
    unsigned se = 0u;
    if (a.se) {                                    // the scaled cnv5 of the feature-attention variant (posenn_se.h)
        se = __atomic_load_n(a.record + RANGE_SE, __ATOMIC_RELAXED);
        r.fails |= range_value_fails(__uint_as_float(se));
    }
    if (worker == 0) {
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store((v4u){r.w[0], r.w[1], r.w[2], r.w[3]}, reinterpret_cast<v4u*>(a.host_mirror));
        if (a.se) __builtin_nontemporal_store(se, a.host_mirror + RANGE_SE);      // acknowledged, like the quad above, before phase 2 stores the sequence number
    }
    return r;
}
// phase 2 (end of the kernel)
__device__ __forceinline__ void snapshot_inputs_if_range_fails(const SnapArgs& a, const RangePeek& r, unsigned worker, unsigned nworkers) {
    if (!a.record) return;
    const bool copy = r.fails && a.s_img != nullptr;
    if (worker == 0) {
        // The host's verdict reads this mirror: no device-to-host copy, no event, no stream to wait for (a synchronous read per
        // batch made batch 1 host-bound, 0.124 -> 0.36 ms per window; an event per batch costs a marker on the GPU's queue).  Two
        // 16-byte stores to coherent host memory; the second carries the sequence number and is issued after the first has been
        // acknowledged, so a host that sees this batch's number sees this batch's maxima.
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_nontemporal_store((v4u){r.w[4], r.w[5], copy ? 1u : 0u, a.seq}, reinterpret_cast<v4u*>(a.host_mirror) + 1);
        if (copy) a.record[RANGE_SNAP] = 1u;
    }
    if (!copy) return;
    const uint4* si = reinterpret_cast<const uint4*>(a.img);
    const uint4* sf = reinterpret_cast<const uint4*>(a.flow);
    const uint4* ss = reinterpret_cast<const uint4*>(a.seg);
    uint4* di = reinterpret_cast<uint4*>(a.s_img);
    uint4* df = reinterpret_cast<uint4*>(a.s_flow);
    uint4* ds = reinterpret_cast<uint4*>(a.s_seg);
    const size_t n_img = (size_t)a.img_vec * a.B, n_seg = (size_t)a.seg_vec * a.B, n_flow = (size_t)a.flow_vec_half * a.B;
    for (size_t i = worker; i < n_img; i += nworkers) di[i] = si[i];
    for (size_t i = worker; i < n_seg; i += nworkers) ds[i] = ss[i];
    if (a.s_depth) {                                           // depth sources: depth_vec 16-byte vectors of the depth format's planes, whatever the label format
        const uint4* sd = reinterpret_cast<const uint4*>(a.depth);
        uint4* dd = reinterpret_cast<uint4*>(a.s_depth);
        const size_t n_depth = (size_t)a.depth_vec * a.B;
        for (size_t i = worker; i < n_depth; i += nworkers) dd[i] = sd[i];
    }
    for (size_t i = worker; i < n_flow; i += nworkers) {
        const size_t b = i / a.flow_vec_half, o = i - b * a.flow_vec_half;
        df[b * a.flow_vec + o] = sf[b * a.flow_vec + o];
    }
}

__global__ __launch_bounds__(64) void pose_from_tiles(const float* __restrict__ partial, int NB, int P, int bm,
                                                      int mtiles, int ntiles_n, const float* __restrict__ bpred,
                                                      float* __restrict__ pose /*[B][2][6]*/, int sel, SnapArgs snap) {
    const int i = blockIdx.x;                              // (n, head, k)
    const int n = i / 6, hk = i - n * 6;
    const RangePeek peek = range_peek(snap, blockIdx.x * 64 + threadIdx.x);
    const float tot = pose_tile_sum<false>(partial, n, hk, P, bm, mtiles, ntiles_n, threadIdx.x);
    if (threadIdx.x == 0) pose_store(pose, n, hk, sel, 0.01f * (tot / (float)P + bpred[hk]));
    snapshot_inputs_if_range_fails(snap, peek, blockIdx.x * 64 + threadIdx.x, gridDim.x * 64);
}

// the same guard as a launch of its own, behind the pose heads that are not pose_from_tiles ("fuse_pose" 0, "fold_tails" 1, tiny maps)
__global__ __launch_bounds__(256) void range_guard_snapshot(SnapArgs snap) {
    const RangePeek peek = range_peek(snap, blockIdx.x * 256 + threadIdx.x);
    snapshot_inputs_if_range_fails(snap, peek, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// Split-K fix-up (forward.hip: small batches): out[m][n] = stored(relu(part[m][0][n] + part[m][1][n] + ...)) in the f16x3
// activation layout (per pixel, per 32 channels: 32 hi halves | 32 lo halves).  The partial sums carry the layer's
// out_scale already; fixed order of the S terms.  One thread per channel pair; N a multiple of 32.
__global__ __launch_bounds__(256) void splitk_fixup(const float* __restrict__ part, long total_pairs, int N, int S, int relu,
                                                    uint8_t* __restrict__ y, unsigned* __restrict__ range) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    float vmax = 0.f;
    if (idx < total_pairs) {
        const int half_n = N >> 1;
        const long m = idx / half_n;
        const int n = (int)(idx - m * half_n) * 2;
        const float2* src = reinterpret_cast<const float2*>(part + (m * S) * N + n);
        float2 v = src[0];
        for (int s = 1; s < S; ++s) {
            const float2 t = src[(long)s * half_n];
            v.x += t.x; v.y += t.y;
        }
        const float lo_clamp = relu ? 0.f : -65504.f;
        v.x = fmaxf(v.x, lo_clamp); v.y = fmaxf(v.y, lo_clamp);
        vmax = fmaxf(fabsf(v.x), fabsf(v.y));
        v.x = fminf(v.x, 65504.f); v.y = fminf(v.y, 65504.f);
        const _Float16 h0 = (_Float16)v.x, h1 = (_Float16)v.y;
        const _Float16 l0 = (_Float16)(v.x - (float)h0), l1 = (_Float16)(v.y - (float)h1);
        uint8_t* o = y + m * (long)N * 4 + (n >> 5) * 128 + (n & 31) * 2;
        *reinterpret_cast<unsigned*>(o) = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
        *reinterpret_cast<unsigned*>(o + 64) = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
    }
    if (range) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
        range_note(range, vmax, (threadIdx.x & 63) == 0);
    }
}

// ---- on-device cross-check (impl 1): one thread per output element, reference layouts ----
__global__ __launch_bounds__(256) void conv_direct(const float* __restrict__ x, int N, int Hin, int Win, int Cin,
                                                   int x_ld, int x_coff,
                                                   const float* __restrict__ w /*HWIO*/, int KS, int Cout,
                                                   const float* __restrict__ bias, int stride, int rate,
                                                   int pad_t, int pad_l, int Hout, int Wout, int relu,
                                                   float* __restrict__ y, int y_ld, int y_coff) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)N * Hout * Wout * Cout;
    if (gid >= total) return;
    const int co = (int)(gid % Cout);
    long m = gid / Cout;
    const int ox = (int)(m % Wout); long t = m / Wout;
    const int oy = (int)(t % Hout); const int n = (int)(t / Hout);
    float acc = 0.f;
    for (int ky = 0; ky < KS; ++ky) {
        const int iy = oy * stride - pad_t + ky * rate;
        if ((unsigned)iy >= (unsigned)Hin) continue;
        for (int kx = 0; kx < KS; ++kx) {
            const int ix = ox * stride - pad_l + kx * rate;
            if ((unsigned)ix >= (unsigned)Win) continue;
            const float* xp = x + ((size_t)(n * Hin + iy) * Win + ix) * x_ld + x_coff;
            const float* wp = w + ((size_t)(ky * KS + kx) * Cin) * Cout + co;
            for (int ci = 0; ci < Cin; ++ci) acc += xp[ci] * wp[(size_t)ci * Cout];
        }
    }
    acc += bias[co];
    if (relu) acc = fmaxf(acc, 0.f);
    y[m * y_ld + y_coff + co] = acc;
}

}  // namespace davo
