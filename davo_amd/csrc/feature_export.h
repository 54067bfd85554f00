// feature_export.h — the export kernels behind davo_forward_features (include/davo_hip.h): what
// DAVO.inference(sess, mode='feature') fetches beside the poses (reference davo.py:1553-1569), computed from what a forward
// leaves on the device - the attention tables, the inputs, and cnv6 in either storage form.  Nothing of the pose path runs here.
//
//   feature_maps         per frame (tgt, src0, src1): the attention map that was multiplied in (davo.py:1387,1394,1218,1405-1414,
//                        1468), the masked rgb (davo.py:1419-1421,1447-1449,1471-1475), the plain preprocessed rgb
//                        (davo.py:967-971, 1519-1522), and the 19-entry rows the maps are gathers of
//   feature_resize_cnv6  tf.image.resize_bilinear(cnv6 of the tgt->src1 call, (H, W)) of each head (davo.py:1457,1463-1465)
// and behind davo_forward_heat, what generate_feature_map.py:204-265 reduces those maps to, computed where cnv6 lies:
//   feature_heat_cnv6    per head and window the channel sum of the stored cnv6 [H/4][W/4] and the maximum of the whole block
//   feature_resize_plane the same resize of that one-channel sum plane to [H][W]
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "input_decode.h"
#include "params.h"

namespace davo {

// Which frames' maps are class-table gathers; the others are the reference's tf.ones_like overrides: 1.0 on every pixel, ignore
// labels included.  The same two tests mask_pack applies (prologue.h).
__host__ __device__ inline bool feature_frame_looked_up(int att_source, int frame) {
    return frame == 0 ? att_tgt_attended(att_source) : att_source != 0;
}

struct FeatureMapsOut {          // device pointers of one piece of nw windows; null = not wanted
    float* att_19;               // [3][nw][19]
    float* attention;            // [3][nw][H][W]
    float* masked;               // [3][nw][H][W][3]
    float* image;                // [3][nw][H][W][3]
};

// One thread per 4 horizontally adjacent pixels of one window, all three frames (mask_pack's unit).  img / seg / tab point at the
// first window of the piece.  The masked rgb is mask_pack's float32 expression - u8_to_unit, then one multiply by the frame's map
// where the variant masks rgb - so it equals the packed tensor's rgb channels to the bit.  The first 3 * nw * 19 threads also write
// the att_19 rows: the table row the forward used for a looked-up frame, 19 ones for an overridden one, whatever d_tab holds there.
// DSPLIT (att_source 13): a source frame's map is mask_pack_depthsplit's select - the frame's own depth plane against the threshold
// chooses the near table `tab' or the far table `ds.tab_far' per pixel (input_decode.h); depth points at the piece's first window
// like img and seg.  No single 19-row table was applied there (the reference sets no att_19s, davo.py:1470): o.att_19 is null.
// LT: the label format, float32 or bytes; DT (DSPLIT only): the depth format, float32 or binary16, read through widen_fetch4
// (input_decode.h).
template <bool DSPLIT, typename LT, typename DT>
__device__ __forceinline__ void feature_maps_body(const uint8_t* __restrict__ img, const LT* __restrict__ seg,
                                                  const float* __restrict__ tab, const Variant& v, int nw, int H, int W, const FeatureMapsOut& o,
                                                  const DepthSplitOf<DT>& ds) {
    const int W4 = W >> 2;
    const long total = (long)nw * H * W4;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (o.att_19 && gid < (long)nw * 3 * NCLS) {                 // (b, frame, class) -> [frame][b][class]
        const int cls = (int)(gid % NCLS), bf = (int)(gid / NCLS), frame = bf % 3, b = bf / 3;
        o.att_19[((size_t)frame * nw + b) * NCLS + cls] = feature_frame_looked_up(v.att_source, frame) ? tab[((size_t)b * 3 + frame) * NCLS + cls] : 1.0f;
    }
    if (gid >= total) return;
    const int x4 = (int)(gid % W4);
    long t = gid / W4;
    const int y = (int)(t % H), b = (int)(t / H);
    const int x = x4 * 4;
    const size_t HW = (size_t)H * W, pix = (size_t)y * W + x;
    const uint8_t* row = img + ((size_t)b * H + y) * (size_t)(9 * W);
#pragma unroll
    for (int frame = 0; frame < 3; ++frame) {
        // (tgt, src0, src1) -> strip slot src0 | tgt | src1 (data_loader.py:537-557) and seg file plane src0, tgt, src1 (davo.py:998-1004)
        const int slot = frame == 0 ? 1 : frame == 1 ? 0 : 2;
        float a[4] = {1.f, 1.f, 1.f, 1.f};
        if (feature_frame_looked_up(v.att_source, frame)) {
            const LabelIds4 sg = label_fetch4(seg + ((size_t)b * 3 + slot) * HW, pix);
            const float* tab_f = tab + ((size_t)b * 3 + frame) * NCLS;
            if (DSPLIT) {
                const float4 dp = widen_fetch4(ds.depth + ((size_t)b * 3 + slot) * HW + pix);
                const float* far_f = ds.tab_far + ((size_t)b * 3 + frame) * NCLS;
                a[0] = att_lookup_split(tab_f, far_f, ds.thr, dp.x, sg.id[0]); a[1] = att_lookup_split(tab_f, far_f, ds.thr, dp.y, sg.id[1]);
                a[2] = att_lookup_split(tab_f, far_f, ds.thr, dp.z, sg.id[2]); a[3] = att_lookup_split(tab_f, far_f, ds.thr, dp.w, sg.id[3]);
            } else {
                a[0] = att_lookup_id(tab_f, sg.id[0]); a[1] = att_lookup_id(tab_f, sg.id[1]);
                a[2] = att_lookup_id(tab_f, sg.id[2]); a[3] = att_lookup_id(tab_f, sg.id[3]);
            }
        }
        const size_t at = ((size_t)frame * nw + b) * HW + pix;
        if (o.attention) *reinterpret_cast<float4*>(o.attention + at) = make_float4(a[0], a[1], a[2], a[3]);
        if (!o.masked && !o.image) continue;
        const uint32_t* ps = reinterpret_cast<const uint32_t*>(row + (size_t)(slot * W + x) * 3);
        const uint32_t q0 = ps[0], q1 = ps[1], q2 = ps[2];
        const uint8_t bytes[12] = {(uint8_t)q0, (uint8_t)(q0 >> 8), (uint8_t)(q0 >> 16), (uint8_t)(q0 >> 24),
                                   (uint8_t)q1, (uint8_t)(q1 >> 8), (uint8_t)(q1 >> 16), (uint8_t)(q1 >> 24),
                                   (uint8_t)q2, (uint8_t)(q2 >> 8), (uint8_t)(q2 >> 16), (uint8_t)(q2 >> 24)};
        float plain[12], masked[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            float r = u8_to_unit(bytes[k]);
            plain[k] = r;
            if (v.mask_rgb) r *= a[k / 3];
            masked[k] = r;
        }
        float4* om = o.masked ? reinterpret_cast<float4*>(o.masked + at * 3) : nullptr;
        float4* oi = o.image ? reinterpret_cast<float4*>(o.image + at * 3) : nullptr;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (om) om[k] = make_float4(masked[4 * k], masked[4 * k + 1], masked[4 * k + 2], masked[4 * k + 3]);
            if (oi) oi[k] = make_float4(plain[4 * k], plain[4 * k + 1], plain[4 * k + 2], plain[4 * k + 3]);
        }
    }
}

template <typename LT>
__global__ __launch_bounds__(256) void feature_maps(const uint8_t* __restrict__ img, const LT* __restrict__ seg,
                                                    const float* __restrict__ tab, Variant v, int nw, int H, int W, FeatureMapsOut o) {
    feature_maps_body<false>(img, seg, tab, v, nw, H, W, o, DepthSplit{});
}

template <typename LT, typename DT>
__global__ __launch_bounds__(256) void feature_maps_depthsplit(const uint8_t* __restrict__ img, const LT* __restrict__ seg,
                                                               const float* __restrict__ tab, Variant v, int nw, int H, int W, FeatureMapsOut o,
                                                               DepthSplitOf<DT> ds) {
    feature_maps_body<true>(img, seg, tab, v, nw, H, W, o, ds);
}

// TF 1.13's resize_bilinear (align_corners=False, no half-pixel centres) at the one scale the library has: cnv6 is [H/4, W/4], so
// in = out / 4 exactly, lo = out >> 2, lerp = (out & 3) / 4, hi = min(lo + 1, last).  TF's order per value, float32, no contraction:
// top = tl + (tr - tl) * xl; bot = bl + (br - bl) * xl; out = top + (bot - top) * yl.
struct ResizeParams {
    const uint8_t* x;            // cnv6 of the forward, pair image 0: float32 NHWC [2B][H2][W2][2 c6], or the f16x3 blocked form (per
                                 // pixel and block of 32 channels [32 hi | 32 lo] halves, scaled by 2^act_shift)
    float* out[2];               // rotation, translation: [nw][4 H2][4 W2][c6] float32 of the piece; null = head not wanted
    int w0, nw;                  // windows [w0, w0 + nw) of that forward; window b's features are pair image 2 b + 1 (tgt->src1)
    int H2, W2, c6, cq_log2;     // cq = c6 / 4 channel quads per pixel
    int head0;                   // head of blockIdx.y == 0
    float unscale;               // 2^-act_shift[cnv6] (f16x3), exact
};

// four channels of one input pixel, decoded with davo_debug_read's expression (hooks.hip): (float)hi + (float)lo, times 2^-shift
template <bool H3, class Params>
__device__ __forceinline__ void resize_load4(const Params& p, size_t pixel, int ch, float v[4]) {
#pragma clang fp contract(off)
    if (H3) {
        const uint8_t* q = p.x + pixel * ((size_t)p.c6 * 8) + (size_t)(ch >> 5) * 128 + (size_t)(ch & 31) * 2;
        const uint2 hi = *reinterpret_cast<const uint2*>(q), lo = *reinterpret_cast<const uint2*>(q + 64);
        _Float16 h[4], l[4];
        __builtin_memcpy(h, &hi, 8);
        __builtin_memcpy(l, &lo, 8);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ((float)h[k] + (float)l[k]) * p.unscale;
    } else {
        const float4 f = *reinterpret_cast<const float4*>(p.x + (pixel * ((size_t)p.c6 * 2) + ch) * sizeof(float));
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
}

// A thread takes four channels of one output column and one (top, bottom) input row pair: one read of the two rows' corner pixels,
// the two horizontal lerps once, then the four output rows 4 iy .. 4 iy + 3 that share the pair.  Lanes run along the channel quads
// of consecutive columns, so each of a wave's four store instructions writes 1 KiB of contiguous output, 16 bytes per lane.  grid
// (ceil(nw H2 W cq / 256), heads wanted); all offsets 64-bit (B H W c6 passes 2^31 at B = 32 of the flagship shape).
template <bool H3>
__global__ __launch_bounds__(256) void feature_resize_cnv6(ResizeParams p) {
#pragma clang fp contract(off)
    const int W = p.W2 * 4, H = p.H2 * 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int cq = (int)(g & ((1 << p.cq_log2) - 1));
    long t = g >> p.cq_log2;
    const int x = (int)(t % W); t /= W;
    const int iy = (int)(t % p.H2);
    const long b = t / p.H2;
    if (b >= p.nw) return;
    const int head = p.head0 + blockIdx.y;
    const int ix = x >> 2, ix1 = min(ix + 1, p.W2 - 1), iy1 = min(iy + 1, p.H2 - 1);
    const float xl = (float)(x & 3) * 0.25f;
    const size_t n = 2 * (size_t)(p.w0 + b) + 1;
    const size_t r0 = (n * p.H2 + iy) * p.W2, r1 = (n * p.H2 + iy1) * p.W2;
    const int ch = head * p.c6 + 4 * cq;
    float tl[4], tr[4], bl[4], br[4];
    resize_load4<H3>(p, r0 + ix, ch, tl);
    resize_load4<H3>(p, r0 + ix1, ch, tr);
    resize_load4<H3>(p, r1 + ix, ch, bl);
    resize_load4<H3>(p, r1 + ix1, ch, br);
    float top[4], dv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        top[k] = tl[k] + (tr[k] - tl[k]) * xl;
        const float bot = bl[k] + (br[k] - bl[k]) * xl;
        dv[k] = bot - top[k];
    }
    float* o = p.out[head] + ((((size_t)b * H + 4 * (size_t)iy) * W + x) * p.c6 + 4 * cq);
    const size_t row = (size_t)W * p.c6;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float yl = (float)r * 0.25f;
        *reinterpret_cast<float4*>(o + r * row) = make_float4(top[0] + dv[0] * yl, top[1] + dv[1] * yl, top[2] + dv[2] * yl, top[3] + dv[3] * yl);
    }
}

// ---- the heat export: channel sum and maximum of cnv6, reduced on the device (davo_forward_heat) ------------------------------
// generate_feature_map.py:204-265 keeps of resize_bilinear(cnv6) only np.sum / np.mean over the channels and the block's maximum.
// The resize is linear, so the channel sum of the resized map is the resize of the channel sum; every stored value reappears at
// out[4i][4j] and every other output lies between its corners, so the maximum of the resized map is the maximum of the stored one.
struct HeatParams {
    const uint8_t* x;            // cnv6 as ResizeParams::x
    float* sum[2];               // rotation, translation: [nw][H2][W2] float32 of the piece; null = head not wanted
    unsigned* max[2];            // [nw] words, zeroed before the launch: the bit pattern of the head's largest value (cnv6 is post-ReLU)
    int w0, nw;                  // as ResizeParams
    int H2, W2, c6, cq_log2;
    int head0;
    float unscale;
};

// Lanes run along the channel quads of consecutive pixels: a lane adds its four channels as (c0 + c1) + (c2 + c3), then the cq
// lanes of a pixel add along a butterfly (lane ^ 1, ^ 2, ...): float32 addition commutes, so both partners hold the same bits and
// the sum is one fixed tree, 2 + log2(cq) <= 8 roundings deep, whatever the launch.  The maximum rides the same butterfly; where a
// wave lies inside one window it goes on to the wave's 64 lanes and one lane raises the window's word, else one lane per pixel does.
// Values that are not above zero (cnv6 is post-ReLU: zeros of either sign) count as +0, so the unsigned order is the float order.
// grid (ceil(nw H2 W2 cq / 256), heads wanted).
template <bool H3>
__global__ __launch_bounds__(256) void feature_heat_cnv6(HeatParams p) {
#pragma clang fp contract(off)
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int ncq = 1 << p.cq_log2;
    const int cq = (int)(g & (ncq - 1));
    const long HW2 = (long)p.H2 * p.W2, npix = (long)p.nw * HW2;
    const long pix = g >> p.cq_log2;
    const bool live = pix < npix;
    const long pc = live ? pix : npix - 1;             // a lane past the end repeats the last pixel: it takes part in the butterfly
    const int b = (int)(pc / HW2);
    const int head = p.head0 + blockIdx.y;
    const size_t n = 2 * (size_t)(p.w0 + b) + 1;
    float v[4];
    resize_load4<H3>(p, n * (size_t)HW2 + (size_t)(pc - (long)b * HW2), head * p.c6 + 4 * cq, v);
    float s = (v[0] + v[1]) + (v[2] + v[3]);
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) m = v[k] > m ? v[k] : m;
    for (int d = 1; d < ncq; d <<= 1) {
        s += __shfl_xor(s, d);
        const float o = __shfl_xor(m, d);
        m = o > m ? o : m;
    }
    if (live && cq == 0) p.sum[head][pix] = s;
    const bool one_window = __shfl(b, 0) == __shfl(b, 63);
    if (one_window) {
        for (int d = ncq; d < 64; d <<= 1) {
            const float o = __shfl_xor(m, d);
            m = o > m ? o : m;
        }
        if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(p.max[head] + b, __float_as_uint(m));
    } else if (live && cq == 0 && m > 0.0f) {
        atomicMax(p.max[head] + b, __float_as_uint(m));
    }
}

struct PlaneParams {
    const float* sum[2];         // [nw][H2][W2], feature_heat_cnv6's
    float* out[2];               // [nw][4 H2][4 W2]; null = head not wanted
    int nw, H2, W2;
    int head0;
};

// feature_resize_cnv6's index rule and float32 order on the one-channel plane: a thread takes one input pixel's 4 x 4 outputs - the
// four corners once, the four horizontal lerps once, then four rows of one float4 each; lanes run along the input row, so a wave's
// store is contiguous.  out[4i][4j] is sum[i][j] to the bit (both lerp weights are 0).  grid (ceil(nw H2 W2 / 256), heads wanted).
__global__ __launch_bounds__(256) void feature_resize_plane(PlaneParams p) {
#pragma clang fp contract(off)
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long HW2 = (long)p.H2 * p.W2;
    if (g >= (long)p.nw * HW2) return;
    const int ix = (int)(g % p.W2);
    long t = g / p.W2;
    const int iy = (int)(t % p.H2);
    const long b = t / p.H2;
    const int head = p.head0 + blockIdx.y;
    const int ix1 = min(ix + 1, p.W2 - 1), iy1 = min(iy + 1, p.H2 - 1);
    const float* src = p.sum[head] + b * HW2;
    const float tl = src[(long)iy * p.W2 + ix], tr = src[(long)iy * p.W2 + ix1];
    const float bl = src[(long)iy1 * p.W2 + ix], br = src[(long)iy1 * p.W2 + ix1];
    float top[4], dv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float xl = (float)k * 0.25f;
        top[k] = tl + (tr - tl) * xl;
        const float bot = bl + (br - bl) * xl;
        dv[k] = bot - top[k];
    }
    const size_t W = 4 * (size_t)p.W2, H = 4 * (size_t)p.H2;
    float* o = p.out[head] + (((size_t)b * H + 4 * (size_t)iy) * W + 4 * (size_t)ix);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float yl = (float)r * 0.25f;
        *reinterpret_cast<float4*>(o + r * W) = make_float4(top[0] + dv[0] * yl, top[1] + dv[1] * yl, top[2] + dv[2] * yl, top[3] + dv[3] * yl);
    }
}

}  // namespace davo
