// input_decode.h — the per-value decodes of the network's inputs that more than one translation unit evaluates: the class-table
// gather behind every attention map, its depth-split form (two tables, chosen per pixel by depth) and the u8 -> [-1, 1] preprocessing.  mask_pack and the fused cnv1 patch fill (prologue.h,
// conv_patch_h3.h) and the feature export (feature_export.h) must agree on them to the bit, so there is one definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "params.h"

namespace davo {

// A label is a class id per pixel, in one of the two formats of davo_set_label_format (include/davo_hip.h): the reference's float32
// or a byte.  label_id: the class a label selects, -1 for "no class".
//   float32: tf.cast(float -> int32) truncates toward zero; one_hot of an out-of-range id is a zero row.  NaN / inf /
//            beyond-int32 labels are platform-defined in the cast (x86: INT_MIN, GPUs: 0 or saturation) and pinned to
//            "no class" here: only finite values in (-1, 19) select a row (the comparison is false for NaN).
//   byte:    that rule folded into a byte by the host (davo_amd.labels_to_u8): L < 19 selects row L, 19..255 none (Cityscapes' 255
//            among them).
__device__ __forceinline__ int label_id(float seg) { return (seg > -1.0f && seg < (float)NCLS) ? (int)seg : -1; }
__device__ __forceinline__ int label_id(uint8_t L) { return L < NCLS ? (int)L : -1; }

__device__ __forceinline__ float att_lookup_id(const float* tab19, int id) { return id >= 0 ? tab19[id] : 0.f; }
template <typename LT>
__device__ __forceinline__ float att_lookup(const float* tab19, LT label) { return att_lookup_id(tab19, label_id(label)); }

// The label fetch of a 4-pixel unit (mask_pack, se_class_squeeze, feature_maps: a thread's four horizontally adjacent pixels): the
// class ids of pixels pix .. pix + 3 of one label plane.  float32: one 16-byte load; bytes: one 32-bit load.  `plane' is the
// frame's [H][W] plane and pix a multiple of 4, so the load is naturally aligned wherever the labels' base is 16-byte aligned: a
// byte plane holds H W bytes, W a multiple of 4 and H W a multiple of 16 (davo_create), float32 planes four times that.
struct LabelIds4 { int id[4]; };
__device__ __forceinline__ LabelIds4 label_fetch4(const float* __restrict__ plane, size_t pix) {
    const float4 q = *reinterpret_cast<const float4*>(plane + pix);
    return LabelIds4{{label_id(q.x), label_id(q.y), label_id(q.z), label_id(q.w)}};
}
__device__ __forceinline__ LabelIds4 label_fetch4(const uint8_t* __restrict__ plane, size_t pix) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(plane + pix);
    return LabelIds4{{label_id((uint8_t)q), label_id((uint8_t)(q >> 8)), label_id((uint8_t)(q >> 16)), label_id((uint8_t)(q >> 24))}};
}

// The optical flow and the depth planes each come in one of two formats (davo_set_flow_format, davo_set_depth_format;
// include/davo_hip.h): float32, or IEEE binary16 in the same layout - flow [B][4][H][W][2], (fx, fy) per pixel; depth [B][3 file
// planes: src0, tgt, src1][H][W], one value per pixel.  FT / DT is the element, float or in_f16.  A reader takes its values
// through one of the fetches below and computes in float32 from there on, so both formats run the same expressions in the same
// order: a binary16 input h gives the bits of the float32 input (float)h.  The widening is v_cvt_f32_f16 per value (two per
// instruction where the compiler pairs them): exact for every binary16 value - subnormals too (the code objects run with f16/f64
// denormals on, the amdgcn default; a half subnormal is a normal float32, so the float32 flush mode does not enter), signed zeros
// and infinities; a NaN stays a NaN (a signalling one comes out quiet, as from any float conversion).
// Each fetch takes the address of its unit's first element; the callers form it in element arithmetic, the same expression
// for both formats (a flow pixel is two elements, a depth pixel one).
//   flow_fetch4   a 4-pixel unit of flow (mask_pack, se_class_squeeze): pixels pix .. pix + 3 of one flow plane, pix a multiple of
//                 4.  float32: two 16-byte loads; binary16: ONE 16-byte load and eight widenings.  Aligned wherever the flow's base
//                 is 16-byte aligned: a plane holds 2 H W elements, H W a multiple of 16.
//   widen_fetch4  four consecutive elements: one 16-byte load, or one 8-byte load and four widenings.  Of flow a 2-pixel unit, the
//                 step of the SE squeeze's fixed chunking (se_squeeze_partial / se_squeeze_excite: unit i of the plane, thread and
//                 chunk boundaries fall on units; the squeeze keeps its units, so its summation order is the float32 format's) and
//                 of se_pool_squeeze.  Of depth pixels pix .. pix + 3 of one plane, pix a multiple of 4 - every reader of raw depth
//                 goes through it; aligned wherever the planes' base is 16-byte aligned: a plane holds H W elements.
//   flow_fetch1   one pixel of flow (the fused cnv1 patch fill): one 8-byte load, or one 4-byte load and two widenings.
typedef _Float16 in_f16;
struct Flow4 { float v[8]; };                                  // x0 y0 x1 y1 x2 y2 x3 y3
__device__ __forceinline__ Flow4 flow_fetch4(const float* __restrict__ unit) {
    const float4* p = reinterpret_cast<const float4*>(unit);
    const float4 a = p[0], b = p[1];
    return Flow4{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ Flow4 flow_fetch4(const in_f16* __restrict__ unit) {
    typedef _Float16 in_h8 __attribute__((ext_vector_type(8)));
    const in_h8 h = *reinterpret_cast<const in_h8*>(unit);
    return Flow4{{(float)h[0], (float)h[1], (float)h[2], (float)h[3], (float)h[4], (float)h[5], (float)h[6], (float)h[7]}};
}
__device__ __forceinline__ float4 widen_fetch4(const float* __restrict__ unit) {
    return *reinterpret_cast<const float4*>(unit);
}
__device__ __forceinline__ float4 widen_fetch4(const in_f16* __restrict__ unit) {
    typedef _Float16 in_h4 __attribute__((ext_vector_type(4)));
    const in_h4 h = *reinterpret_cast<const in_h4*>(unit);
    return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}
__device__ __forceinline__ float2 flow_fetch1(const float* __restrict__ px) {
    return *reinterpret_cast<const float2*>(px);
}
__device__ __forceinline__ float2 flow_fetch1(const in_f16* __restrict__ px) {
    typedef _Float16 in_h2 __attribute__((ext_vector_type(2)));
    const in_h2 h = *reinterpret_cast<const in_h2*>(px);
    return make_float2((float)h[0], (float)h[1]);
}

// Depth-split attention (att_source 13, davo.py:1143-1155): near = depth < thr in float32, strict; tf.where sends a NaN depth (the
// comparison is false) to the far side.  The pixel's class is looked up in the chosen table by att_lookup's rule.
__device__ __forceinline__ float att_lookup_split(const float* near19, const float* far19, float thr, float depth, int id) {
    return att_lookup_id(depth < thr ? near19 : far19, id);
}

// what the depth-split forms of mask_pack (prologue.h) and feature_maps (feature_export.h) take beside the near tables
// (DT: the depth element, float or in_f16 - the pointer keeps its element type all the way into the kernel)
template <typename DT>
struct DepthSplitOf {
    const DT* depth;             // [B][3 file planes: src0, tgt, src1][H][W] in the depth format DT, 16-byte aligned
    const float* tab_far;        // [B][3][19]
    float thr;                   // depth_threshold, the host's copy of the loaded scalar
};
using DepthSplit = DepthSplitOf<float>;
// The label maps have the same planes in the context's label format, [B][3 file planes: src0, tgt, src1][H][W] float32 or uint8,
// and the same requirement: a 16-byte aligned base (then every unit's load above is aligned, in either format).

__device__ __forceinline__ float u8_to_unit(uint32_t byte) {
    return (float)byte * (1.0f / 255.0f) * 2.0f - 1.0f;        // davo.py:1521-1522
}

}  // namespace davo
