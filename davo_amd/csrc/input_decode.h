// input_decode.h — the per-value decodes of the network's inputs that more than one translation unit evaluates: the class-table
// gather behind every attention map, its depth-split form (two tables, chosen per pixel by depth) and the u8 -> [-1, 1] preprocessing.  mask_pack and the fused cnv1 patch fill (prologue.h,
// conv_patch_h3.h) and the feature export (feature_export.h) must agree on them to the bit, so there is one definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "params.h"

namespace davo {

__device__ __forceinline__ float att_lookup(const float* tab19, float seg) {
    // tf.cast(float -> int32) truncates toward zero; one_hot of an out-of-range id is a zero row.  NaN / inf /
    // beyond-int32 labels are platform-defined in the cast (x86: INT_MIN, GPUs: 0 or saturation) and pinned to
    // "no class" here: only finite values in (-1, 19) select a row (the comparison is false for NaN).
    return (seg > -1.0f && seg < (float)NCLS) ? tab19[(int)seg] : 0.f;
}

// Depth-split attention (att_source 13, davo.py:1143-1155): near = depth < thr in float32, strict; tf.where sends a NaN depth (the
// comparison is false) to the far side.  The pixel's class is looked up in the chosen table by att_lookup's rule.
__device__ __forceinline__ float att_lookup_split(const float* near19, const float* far19, float thr, float depth, float seg) {
    return att_lookup(depth < thr ? near19 : far19, seg);
}

// what the depth-split forms of mask_pack (prologue.h) and feature_maps (feature_export.h) take beside the near tables
struct DepthSplit {
    const float* depth;          // [B][3 file planes: src0, tgt, src1][H][W] float32, 16-byte aligned
    const float* tab_far;        // [B][3][19]
    float thr;                   // depth_threshold, the host's copy of the loaded scalar
};

__device__ __forceinline__ float u8_to_unit(uint32_t byte) {
    return (float)byte * (1.0f / 255.0f) * 2.0f - 1.0f;        // davo.py:1521-1522
}

}  // namespace davo
