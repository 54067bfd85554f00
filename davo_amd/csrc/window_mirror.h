// window_mirror.h — the left-right mirror of a batch's inputs (include/davo_hip.h: davo_set_flip), on the device.
// The rule is the training loader's (data_loader.py:142-169, npy_flip / img_flip per frame): every frame is mirrored inside its own
// third of the strip, every flow plane, label map and depth plane on its own; no value changes (the horizontal flow component is
// NOT negated), plane and frame order stay.  The mirror happens once, where a batch becomes the staging set its forward reads
// (entry.hip: stage_windows); nothing downstream of the set knows.
//   window_mirror<LT, FT, DT, false>   window layout: sources and destinations are both window-major.  In place (the host entry points:
//                                      the staging set after its copies) or from the caller's device buffers into the set.
//   window_mirror<LT, FT, DT, true>    frame layout: window_gather with mirrored stores - frame-major sources (window_gather.h), the
//                                      same grid, no launch more than a gather; a flow that is in the set already is mirrored in place.
// A grid of (pieces, window, job), the jobs window_gather's: one third of the strip rows, one label or depth plane, one flow plane.
// Only what the pair selection and the variant read is touched (frame_plan's / stage_inputs' rule).
// A row is cut into units of a whole number of pixels; a lane holds unit p of a row and its partner U - 1 - p, reverses the pixels
// inside each and stores them swapped - so the same code runs in place.  The middle unit of a row with an odd number of them is its
// own partner: loaded twice, reversed and stored once.  Units are 16-byte multiples wherever the rows allow:
//   strip thirds   3-byte pixels: 16 pixels = 48 bytes (W % 16 == 0), else 4 pixels = three dwords (rows of 3W bytes are dword-aligned)
//   flow           8-byte pixels: 4 pixels = 32 bytes;  binary16: 4-byte pixels, 4 pixels = 16 bytes
//   labels         float32: 4 pixels = 16 bytes;  u8: 16 pixels = 16 bytes (W % 16 == 0), else 4 pixels = one dword
//   depth          float32: 4 pixels = 16 bytes;  binary16: 8 pixels = 16 bytes (W % 8 == 0), else 4 pixels = 8 bytes (rows of 2W
//                  bytes are 8-byte aligned, W being a multiple of 4)
// Four pixels of three bytes are three dwords; their mirror is three byte permutes (v_perm_b32) and one more for the middle dword.
// Pure streaming, two pairs of units in flight per lane, all loads of a round ahead of its first store; 64-bit offsets.  No
// floating-point arithmetic at all.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "window_gather.h"

namespace davo {

constexpr int MIRROR_PIECE = 512;                          // unit pairs per workgroup and round: 256 lanes x 2 pairs in flight

// bytes of {hi, lo} picked by the four selectors of sel (0..3: lo's bytes, 4..7: hi's), v_perm_b32's rule
__host__ __device__ __forceinline__ uint32_t mirror_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= (uint32_t)((both >> (8 * ((sel >> (8 * i)) & 7))) & 0xff) << (8 * i);
    return r;
#endif
}

// The pixels of one unit in reverse order.  PX: bytes per pixel (1, 2, 3, 4, 8); K: dwords per unit.
template <int PX, int K>
__host__ __device__ __forceinline__ void mirror_unit(const uint32_t (&in)[K], uint32_t (&out)[K]) {
    static_assert(PX == 1 || PX == 2 || PX == 3 || PX == 4 || PX == 8, "pixel sizes of the input planes");
    static_assert((K * 4) % PX == 0 && (PX != 3 || K % 3 == 0) && (PX != 8 || K % 2 == 0), "a unit is a whole number of pixels");
    if constexpr (PX == 4) {
#pragma unroll
        for (int i = 0; i < K; ++i) out[i] = in[K - 1 - i];
    } else if constexpr (PX == 8) {
#pragma unroll
        for (int i = 0; i < K; i += 2) { out[i] = in[K - 2 - i]; out[i + 1] = in[K - 1 - i]; }
    } else if constexpr (PX == 1) {
#pragma unroll
        for (int i = 0; i < K; ++i) out[i] = mirror_perm(0u, in[K - 1 - i], 0x00010203u);
    } else if constexpr (PX == 2) {
        // two halves b0 b1 | b2 b3 in a dword -> b2 b3 | b0 b1: one byte permute; dwords in reverse order
#pragma unroll
        for (int i = 0; i < K; ++i) out[i] = mirror_perm(0u, in[K - 1 - i], 0x01000302u);
    } else {
        // four pixels b0..b11 in (d0, d1, d2) -> b9 b10 b11 b6 | b7 b8 b3 b4 | b5 b0 b1 b2; groups of four pixels in reverse order
#pragma unroll
        for (int g = 0; g < K / 3; ++g) {
            const uint32_t d0 = in[3 * g], d1 = in[3 * g + 1], d2 = in[3 * g + 2];
            uint32_t* o = out + (K - 3 - 3 * g);
            o[0] = mirror_perm(d2, d1, 0x02070605u);
            o[1] = mirror_perm(d0, mirror_perm(d2, d1, 0x00000403u), 0x03070100u);
            o[2] = mirror_perm(d1, d0, 0x02010005u);
        }
    }
}

template <int K>
__device__ __forceinline__ void mirror_load(const uint8_t* p, uint32_t (&v)[K]) {
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int i = 0; i < K / 4; ++i) {
            const gather_vec4 q = reinterpret_cast<const gather_vec4*>(p)[i];
            v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
        }
    } else if constexpr (K == 2) {                          // one 8-byte load (binary16 depth rows with W % 8 == 4)
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        v[0] = q.x; v[1] = q.y;
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) v[i] = reinterpret_cast<const uint32_t*>(p)[i];
    }
}

template <int K>
__device__ __forceinline__ void mirror_store(uint8_t* p, const uint32_t (&v)[K]) {
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int i = 0; i < K / 4; ++i) {
            gather_vec4 q;
            q.x = v[4 * i]; q.y = v[4 * i + 1]; q.z = v[4 * i + 2]; q.w = v[4 * i + 3];
            reinterpret_cast<gather_vec4*>(p)[i] = q;
        }
    } else if constexpr (K == 2) {
        *reinterpret_cast<uint2*>(p) = make_uint2(v[0], v[1]);
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) reinterpret_cast<uint32_t*>(p)[i] = v[i];
    }
}

// `rows' rows of U units each, src_pitch / dst_pitch bytes apart, mirrored from src to dst; src may BE dst (no __restrict__: every
// load of a round stays ahead of its stores, and a unit is read and written by one lane only)
template <int PX, int K>
__device__ __forceinline__ void mirror_rows(const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch, unsigned rows, unsigned U) {
    const unsigned P = (U + 1) / 2, total = rows * P;      // pairs per row: unit p with unit U - 1 - p
    const unsigned step = gridDim.x * MIRROR_PIECE;
    for (unsigned base = blockIdx.x * MIRROR_PIECE + threadIdx.x; base < total; base += step) {
        // unconditional loads (a lane past the end re-reads the last pair and stores nothing)
        uint32_t lo[2][K], hi[2][K];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const unsigned i = min(base + u * 256, total - 1);
            const unsigned row = i / P, p = i - row * P;
            const uint8_t* r = src + (size_t)row * src_pitch;
            mirror_load<K>(r + (size_t)p * (K * 4), lo[u]);
            mirror_load<K>(r + (size_t)(U - 1 - p) * (K * 4), hi[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const unsigned i = base + u * 256;
            if (i >= total) continue;
            const unsigned row = i / P, p = i - row * P, q = U - 1 - p;
            uint8_t* r = dst + (size_t)row * dst_pitch;
            uint32_t m[K];
            mirror_unit<PX, K>(lo[u], m);
            mirror_store<K>(r + (size_t)q * (K * 4), m);
            if (q == p) continue;                           // the middle unit is its own partner: reversed once
            mirror_unit<PX, K>(hi[u], m);
            mirror_store<K>(r + (size_t)p * (K * 4), m);
        }
    }
}

// a plane of H rows of W pixels of PX bytes, contiguous on both sides
template <int PX>
__device__ __forceinline__ void mirror_plane(const uint8_t* src, uint8_t* dst, int H, int W) {
    const size_t pitch = (size_t)W * PX;
    if constexpr (PX == 1) {
        if (W % 16 == 0) mirror_rows<1, 4>(src, pitch, dst, pitch, H, W / 16);
        else mirror_rows<1, 1>(src, pitch, dst, pitch, H, W / 4);
    } else if constexpr (PX == 2) {
        if (W % 8 == 0) mirror_rows<2, 4>(src, pitch, dst, pitch, H, W / 8);
        else mirror_rows<2, 2>(src, pitch, dst, pitch, H, W / 4);
    } else {
        mirror_rows<PX, PX>(src, pitch, dst, pitch, H, W / 4);      // four pixels: PX dwords
    }
}

// GatherArgs (window_gather.h) serves both forms: f_* the sources - frame-major (FRAMES) or window-major like the destinations -,
// w_* the destinations.  FRAMES: f_flow null = the flow is in the set already, mirrored there in place.  seg_tgt: the variant
// attends the target, so its label map is read - whatever the selection; where it does not, no kernel reads that map (davo_submit's
// staging does not even copy it) and the mirror leaves it alone.  depth_tgt: a ONE-pair batch reads the target's depth plane
// (both pairs: every plane, stage_inputs copies them whole).
template <typename LT, typename FT, typename DT, bool FRAMES>
__global__ __launch_bounds__(256) void window_mirror(GatherArgs a) {
    const size_t n = blockIdx.y, HW = (size_t)a.H * a.W;
    const int job = blockIdx.z;
    const bool both = a.sel == PAIRS_BOTH;
    if (job < 3) {                                        // strip third k of every row
        const int k = job;
        if (k != 1 && !(a.sel & (k == 0 ? PAIRS_SRC0 : PAIRS_SRC1))) return;
        const size_t third = (size_t)a.W * 3;
        const uint8_t* src = FRAMES ? a.f_img + a.frame(n, k) * HW * 3 : a.f_img + n * HW * 9 + k * third;
        const size_t src_pitch = FRAMES ? third : third * 3;
        uint8_t* dst = a.w_img + n * HW * 9 + k * third;
        if (a.W % 16 == 0) mirror_rows<3, 12>(src, src_pitch, dst, third * 3, a.H, a.W / 16);
        else mirror_rows<3, 3>(src, src_pitch, dst, third * 3, a.H, a.W / 4);
    } else if (job < 9) {                                 // plane k of the label maps (3..5) or the depth planes (6..8)
        const bool depth = job >= 6;
        const int k = (job - 3) % 3;
        if (depth && !a.f_depth) return;
        if (k == 1 ? !(depth ? (both || a.depth_tgt) : a.seg_tgt) : !(a.sel & (k == 0 ? PAIRS_SRC0 : PAIRS_SRC1))) return;
        const size_t pb = HW * (depth ? sizeof(DT) : sizeof(LT));
        const uint8_t* src = (depth ? a.f_depth : a.f_seg) + (FRAMES ? a.frame(n, k) : n * 3 + k) * pb;
        uint8_t* dst = (depth ? a.w_depth : a.w_seg) + (n * 3 + k) * pb;
        if (depth) mirror_plane<(int)sizeof(DT)>(src, dst, a.H, a.W);
        else mirror_plane<(int)sizeof(LT)>(src, dst, a.H, a.W);
    } else {                                              // flow plane p of planes 0, 1 of [B][4]
        const int p = job - 9;
        if (!(a.sel & (p == 0 ? PAIRS_SRC0 : PAIRS_SRC1))) return;
        const size_t pb = HW * 2 * sizeof(FT);
        uint8_t* dst = a.w_flow + (n * 4 + p) * pb;
        const uint8_t* src = !a.f_flow ? dst : a.f_flow + (FRAMES ? n * 2 + p : n * 4 + p) * pb;
        mirror_plane<2 * (int)sizeof(FT)>(src, dst, a.H, a.W);
    }
}

}  // namespace davo
