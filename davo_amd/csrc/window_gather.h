// window_gather.h — the frame layout of a batch (include/davo_hip.h: "Frame sequences") and the kernel that expands it.
// A caller that holds a video hands over every frame once: frames [N+2][H][W][3] bytes, label maps and depth planes
// [N+2][H][W], flow [N][2][H][W][2]; window n is (src0, tgt, src1) = frames (n, n+1, n+2).  Every kernel of the path reads the
// reference's window layout (strip [B][H][3W][3], planes [B][3][H][W], flow [B][4][H][W][2]), so one launch of window_gather
// per batch writes the windows into the slot's staging set ahead of the forward: nothing downstream knows the difference.
//   frame_plan      pure host logic: which frames and flow planes a batch of N windows reads under a pair selection - what the
//                   host entry points copy and what the kernel gathers (davo_frames_plan exports it)
//   track_step      pure host logic: the ring of a tracking session - where a push puts its frames, which places its windows read
//                   and what orders the two (davo_track_ring exports it).  The kernel reads a ring through GatherArgs' frame
//                   bases: the same body, no second kernel
//   window_gather   the kernel: a grid of (pieces, window, job); a job is one third of the strip rows, one label or depth plane
//                   or one flow plane of its window.  Pure streaming: 16 bytes per lane, four loads in flight per lane,
//                   consecutive lanes on consecutive addresses on both sides; strip rows of 3W bytes that are no multiple of
//                   16 (W % 16 != 0) move as dwords (3W % 4 == 0 always).  64-bit offsets throughout.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "params.h"

namespace davo {

// Frame ranges [lo, hi) of each plane kind, and flow planes [lo, hi), that a batch of N windows reads (frame f of the batch is
// frame f of the caller's arrays).  tgt->src0 reads frames (n + 1, n), tgt->src1 frames (n + 1, n + 2); the label map of the
// target only where the variant attends it; the depth sources 11, 12 the target's and the source's depth plane, the depth-split
// attention (13) the source's alone - stage_inputs' rules (entry.hip), frame-major.
struct FramePlan {
    int img[2], seg[2], depth[2], flow[2];
    bool seg_tgt, depth_tgt;               // a one-pair batch reads the target's label map / depth plane too
};
inline FramePlan frame_plan(int N, int sel, int att_source) {
    FramePlan p{};
    const bool s0 = sel & PAIRS_SRC0, s1 = sel & PAIRS_SRC1, both = sel == PAIRS_BOTH;
    p.seg_tgt = att_tgt_attended(att_source);
    p.depth_tgt = att_desc_depth(att_source);
    auto range = [&](int* r, bool tgt) {      // the source frames, widened by the target's where it is read
        r[0] = both ? 0 : s0 ? 0 : (tgt ? 1 : 2);
        r[1] = both ? N + 2 : s1 ? N + 2 : (tgt ? N + 1 : N);
    };
    range(p.img, true);
    range(p.seg, p.seg_tgt);
    if (att_reads_depth(att_source)) range(p.depth, p.depth_tgt);
    p.flow[0] = s0 ? 0 : 1;
    p.flow[1] = s1 ? 2 : 1;
    return p;
}
// bytes that cross the link for such a batch (e: the element sizes of the batch's input format, params.h)
inline long long frame_plan_bytes(const FramePlan& p, int N, int H, int W, const ElemBytes& e) {
    const long long HW = (long long)H * W;
    return (p.img[1] - p.img[0]) * HW * 3 + (long long)N * (p.flow[1] - p.flow[0]) * HW * 2 * e.flow +
           (p.seg[1] - p.seg[0]) * HW * e.label + (p.depth[1] - p.depth[0]) * HW * e.depth;
}

// ---- the ring of a tracking session (include/davo_hip.h: "Online tracking"), pure host logic ---------------------------------
// A session of S lanes keeps the frames of the last pushes on the device in a ring of R places, a place = S frames of one plane
// kind.  Push t (t = 0, 1, ...) uploads its frames into place t mod R and - from t = 2 on - gathers window (t - 2, t - 1, t) of
// every lane from places (t - 2 + k) mod R.  Place t mod R last held the frames of push t - R, which the gathers of pushes t - R,
// t - R + 1 and t - R + 2 read: the upload of push t is ordered behind those three gathers, and the gather of push t behind the
// uploads of pushes t - 2 and t - 1 (events, where the streams differ: entry.hip).  R = slots in flight + 2: the youngest gather
// an upload waits for then is that of push t - slots, which ran on the same stream - so an upload never waits for the kernels of
// a push that another slot is still running, and the copies of push t + 1 go under the kernels of push t.
constexpr int TRACK_RING_MIN = 3, TRACK_RING_MAX = 6;     // davo_set_inflight 1..4
struct TrackStep {
    int R;
    int upload_place;                                     // where the frames of push t go
    int place[3];                                         // the places window (src0, tgt, src1) of push t reads (t >= 2)
    long long upload_after[3];                            // pushes whose gather the upload is ordered behind; -1: none (they gathered nothing)
    long long gather_after[2];                            // pushes whose upload the gather is ordered behind (t >= 2)
};
inline int track_ring_places(int inflight) { return inflight + 2; }
inline TrackStep track_step(long long t, int R) {
    TrackStep s{};
    s.R = R;
    s.upload_place = (int)(t % R);
    for (int k = 0; k < 3; ++k) {
        s.place[k] = t >= 2 ? (int)((t - 2 + k) % R) : -1;
        const long long u = t - R + k;
        s.upload_after[k] = u >= 2 ? u : -1;
    }
    s.gather_after[0] = t - 2;
    s.gather_after[1] = t - 1;
    return s;
}
// bytes one push of S lanes copies across the link: a frame, a label map and (where the variant reads depth) a depth plane per
// lane, and the flow planes of the selection - davo_frames_plan's figure for N = 1 less the two frames it sends again
inline long long track_push_bytes(int S, int sel, int att_source, int H, int W, const ElemBytes& e) {
    const long long HW = (long long)H * W;
    return S * (HW * 3 + pairs_per_window(sel) * HW * 2 * e.flow + HW * e.label + (att_reads_depth(att_source) ? HW * e.depth : 0));
}

struct GatherArgs {
    const uint8_t *f_img, *f_seg, *f_depth, *f_flow;      // frame-major sources; f_depth null: the variant reads none; f_flow null: the flow is in place already
    uint8_t *w_img, *w_seg, *w_depth, *w_flow;            // window-major destinations (window 0 of the batch)
    int H, W;
    int sel;                                              // pair selection (PAIRS_*): what no selected pair reads is not gathered
    int seg_tgt, depth_tgt;                               // FramePlan's
    // frame-major sources: window n takes strip third / plane k from frame base_k + n * stride of f_img, f_seg and f_depth.  A batch
    // of consecutive frames is (0, 1, 2), stride 1 - the defaults; a push of S lanes out of a ring whose places hold S frames each
    // is (place[0] S, place[1] S, place[2] S), stride 1 (track_ring below).  The flow planes are window-major on both sides
    int base0 = 0, base1 = 1, base2 = 2, stride = 1;
    __host__ __device__ size_t frame(size_t n, int k) const { return (size_t)(k == 0 ? base0 : k == 1 ? base1 : base2) + n * (size_t)stride; }
};
constexpr int GATHER_JOBS = 11;                           // 0..2 strip thirds | 3..5 label planes | 6..8 depth planes | 9, 10 flow planes
typedef unsigned gather_vec4 __attribute__((ext_vector_type(4)));      // 16 bytes per lane, a type an asm operand can hold
constexpr int GATHER_PIECE = 1024;                        // vectors per workgroup and round: 256 lanes x 4 loads in flight

// nvec vectors from src (contiguous) to dst: rows of row_vecs vectors, dst_pitch bytes apart (one row: a flat copy)
template <typename V>
__device__ __forceinline__ void gather_copy(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, unsigned nvec,
                                            unsigned row_vecs, size_t dst_pitch) {
    const unsigned step = gridDim.x * GATHER_PIECE;
    for (unsigned base = blockIdx.x * GATHER_PIECE + threadIdx.x; base < nvec; base += step) {
        // four unconditional loads (a lane past the end re-reads the last vector and stores nothing): all in flight before the
        // first store waits
        V v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned i = min(base + u * 256, nvec - 1);
            v[u] = *reinterpret_cast<const V*>(src + (size_t)i * sizeof(V));
        }
        // the four values pass through an empty asm: the loads stay ahead of it and in flight together (left alone the compiler
        // sinks each load into its store's branch and waits for them one by one)
        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned i = base + u * 256;
            if (i >= nvec) continue;
            const unsigned row = dst_pitch ? i / row_vecs : 0u, col = i - row * row_vecs;
            *reinterpret_cast<V*>(dst + (size_t)row * dst_pitch + (size_t)col * sizeof(V)) = v[u];
        }
    }
}

// LT: the label element (float or uint8_t, davo_set_label_format); FT: the flow element (float or in_f16, davo_set_flow_format) -
// a flow plane is 2 H W of them, a whole number of 16-byte vectors in either format (H W is a multiple of 16); DT: the depth
// element (float or in_f16, davo_set_depth_format) - a depth plane is H W of them, a whole number of vectors too
template <typename LT, typename FT, typename DT>
__global__ __launch_bounds__(256) void window_gather(GatherArgs a) {
    const size_t n = blockIdx.y, HW = (size_t)a.H * a.W;
    const int job = blockIdx.z;
    const bool both = a.sel == PAIRS_BOTH;
    if (job < 3) {                                        // strip third k of every row: frame a.frame(n, k)
        const int k = job;
        if (k != 1 && !(a.sel & (k == 0 ? PAIRS_SRC0 : PAIRS_SRC1))) return;
        const size_t third = (size_t)a.W * 3;
        const uint8_t* src = a.f_img + a.frame(n, k) * HW * 3;
        uint8_t* dst = a.w_img + n * HW * 9 + k * third;
        if (a.W % 16 == 0) gather_copy<gather_vec4>(src, dst, (unsigned)(HW * 3 / 16), (unsigned)(third / 16), third * 3);
        else gather_copy<uint32_t>(src, dst, (unsigned)(HW * 3 / 4), (unsigned)(third / 4), third * 3);
    } else if (job < 9) {                                 // plane k of the label maps (3..5) or the depth planes (6..8)
        const bool depth = job >= 6;
        const int k = (job - 3) % 3;
        if (depth && !a.f_depth) return;
        if (k == 1 ? !(both || (depth ? a.depth_tgt : a.seg_tgt)) : !(a.sel & (k == 0 ? PAIRS_SRC0 : PAIRS_SRC1))) return;
        const size_t pb = HW * (depth ? sizeof(DT) : sizeof(LT));
        const unsigned nvec = (unsigned)(pb / 16);
        gather_copy<gather_vec4>((depth ? a.f_depth : a.f_seg) + a.frame(n, k) * pb, (depth ? a.w_depth : a.w_seg) + (n * 3 + k) * pb, nvec, nvec, 0);
    } else {                                              // flow plane p: [N][2] -> planes 0, 1 of [B][4]
        const int p = job - 9;
        if (!a.f_flow || !(a.sel & (p == 0 ? PAIRS_SRC0 : PAIRS_SRC1))) return;
        const size_t pb = HW * 2 * sizeof(FT);
        const unsigned nvec = (unsigned)(pb / 16);
        gather_copy<gather_vec4>(a.f_flow + (n * 2 + p) * pb, a.w_flow + (n * 4 + p) * pb, nvec, nvec, 0);
    }
}

}  // namespace davo
