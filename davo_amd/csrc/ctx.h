// ctx.h — host-side state of one davo_ctx (include/davo_hip.h) and the small helpers every
// translation unit of libdavo_hip.so shares.  Host code only; the kernels live in conv_igemm.h,
// conv_igemm_h3.h, conv_igemm_h3s.h, conv_patch_h3.h, prologue.h and se_pool.h and are launched through launch.h.
//
// Translation units (built in parallel by davo_amd/_lib.py, linked into one shared library):
//   api.hip         extern "C": context life cycle, weights, settings and the option table, range-state calls, davo_synchronize
//   entry.hip       extern "C": the calls that take a batch (device, streaming and host forward families, both layouts), delivery
//   export.hip      extern "C": the feature and heat exports (davo_set_*_export, davo_forward_features, davo_forward_heat)
//   hooks.hip       extern "C": measurement and test hooks (davo_debug_read, davo_conv2d_same, plan and profile calls, memory helpers)
//   forward.hip     the forward of the pose path, issued: validate, ensure weights, decide_forward (plan.hip), then run_front / run_layers / run_head
//   range_guard.hip the f16x3 range guard: records, verdicts, calibration, re-issues, tickets (its bookkeeping: range_book.h)
//   plan.hip        launch planning: tile shapes, whole-round launch splits, every launch decision of a conv layer and the launch sequence of a
//                   whole forward (decide_forward: front, packer, layer records, head) - pure host logic
//   weights.hip     weight re-layout: HWIO float32 -> packed f32 / split-fp16 operands
//   launch_f32.hip  conv_igemm_f32 instantiations + dispatch
//   launch_h3.hip   conv_igemm_h3 instantiations + dispatch (the f16x3 path, the long compile)
//   launch_h3s.hip  conv_igemm_h3s instantiations (208x256 tile); launch_h3_generic.hip: davo_conv2d_same's shapes
//   launch_misc.hip prologue / pooled squeeze and excite (se_pool.h) / pose head / cnv1..cnv3 patch / feature-attention (posenn_se.h) / window gather and mirror (window_gather.h, window_mirror.h) / direct-convolution kernels + dispatch
//   launch_feature.hip  the feature export kernels (feature_export.h) + dispatch
//   comm.hip        RCCL communicator behind the C ABI (pose gather of the window-sharded driver)
// owned.h holds the owner types (device / page-locked memory, streams, events): everything a context allocates is a member of
// one of them, so `delete ctx' is the whole teardown.  What is built lazily is a named group (HostStaging, PoseRing, RangeRing,
// Snapshots, FxBlock, SeWorkspace, TrackState, a Slot), built into a local and moved in complete: a group exists whole or not at all.
//
// A forward's inputs.  forward_device(c, run, B, in, d_pose, &res) reads the context for what lasts (geometry, weights, options,
// storage scales, the slots' workspaces); what belongs to the batch travels in one argument, `run' (struct Run below): its slot and
// stream, its range record, its snapshot arguments, its pair selection and its arithmetic mode.  The entry point builds it on its
// stack, so nothing is set on the context before a forward or put back after it; `res' says what really ran, and what the context
// keeps of a forward is reported state (last_*), which no forward reads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <map>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/davo_hip.h"
#include "owned.h"
#include "params.h"
#include "plan.h"
#include "range_book.h"

namespace davo {

static_assert(RECORD_WORDS == RANGE_WORDS, "range_book.h sizes a ticket's copy of its record");

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
    DevMem<float> dev;             // raw copy in the reference layout (impl 1, pose_head, SE)
};

struct ConvLayer : LayerGeom {     // plan.h: the host fields, all that the launch decisions read
    const char* label = nullptr;
    DevMem<float> d_w;             // [groups][npad][kpad]
    DevMem<float> d_b;             // [groups][npad]
    DevMem<uint8_t> d_wh;          // f16x3: [groups][npad_h][nchunks_h][32 hi | 32 lo] halves
    DevMem<float> d_bh;            // [groups][npad_h]
};

struct ProfEntry {
    std::string name;
    int launches = 0;
    double total_ms = 0.0;
    std::vector<std::pair<EventOwner, EventOwner>> pending;
    // per-launch record since the last reset (davo_profile_samples; at most PROF_SAMPLES_CAP kept): the launch's own duration
    // and the time from the previous bracketed launch's start to this one's (-1 when the previous start is not known)
    std::vector<float> dur_ms, period_ms;
};
constexpr size_t PROF_SAMPLES_CAP = 8192;

// One in-flight batch: its own HIP stream and activation workspace.  Weights are shared.
constexpr int MAX_INFLIGHT = 4;                  // slots a context rotates through at most (davo_set_inflight; the per-slot scratch and staging sets are sized by it)
struct SeWorkspace {                             // feature attention (posenn_se.h): [NB][P2][512] scaled cnv5, [NB][2][256] scales, [NB][SE5_CHUNKS][256] sums
    DevMem<float> d_se, d_se_scale, d_se_partial;
};
struct Slot {
    StreamOwner stream;
    DevMem<float> d_partial, d_tab, d_packed, d_pose_partial;
    DevMem<float> d_tab_far;                     // depth-split flow attention (att_source 13): the far MLP's tables [B][3][19] (d_tab holds the near ones); null in every other variant
    DevMem<float> d_desc;                        // pooled flow attention (att_source 14..17): the SE descriptors [B][2][D] ("se_desc"); null in every other variant
    DevMem<float> d_act[7];
    std::optional<SeWorkspace> se;              // absent with the feature-attention mode off
    DevMem<unsigned> d_counters;                 // "last workgroup" tickets (pose_tail.h): [0] cnv7's pose tail, [1 + b] triplet b's squeeze, [1 + max_batch + t] tile t of a split-K launch
};
static_assert(std::is_nothrow_move_constructible<Slot>::value, "davo_ctx::slots is a std::vector");

// Device room of the context for max_batch windows of every plane the variant reads (api.hip: alloc_input_set builds one whole);
// depth stays null unless the variant reads it, so a set's view says by itself whether there are depth planes to carry along.
// A set is only ever assigned whole, so it is either empty or built.
struct InputSet {
    DevMem<void> img, flow, seg, depth;
    bool built() const { return static_cast<bool>(img); }
    Inputs view() const { return Inputs{img.get(), flow.get(), seg.get(), depth.get()}; }
};

// A slot's frame buffer (window_gather.h): the frames of a frame-layout batch as the host entry points copy them, max_batch + 2
// frames per plane, before window_gather expands them into the slot's staging set.  No flow (it is copied straight into the
// staging set); depth only where the variant reads it.  Built whole by the slot's first `_frames' call (entry.hip: acquire_stager).
struct FrameSet {
    DevMem<void> img, seg, depth;
    bool built() const { return static_cast<bool>(img); }
};

// A batch davo_submit has issued whose poses have not been delivered to the caller's array yet (entry.hip: streaming entry point).
// Its inputs live in the staging set of its in-flight slot (at most MAX_INFLIGHT slots), its poses in entry `pr` of a ring of STREAM_POSES device
// buffers with page-locked host twins, so neither a re-issue nor the caller's buffer recycling can touch another batch's data.
constexpr int STREAM_POSES = 8;
struct StreamJob {
    int B;
    float* pose_out;                           // the caller's [B,2,6] (pageable is fine: written by the host at delivery)
    int pr;                                    // pose ring entry
    bool ticketed;                             // has a range ticket (f16x3) that must be judged before delivery
    unsigned seq;                              // ... its sequence number
};

// How one batch runs.  The entry point (entry.hip) fills one on its stack and forward_device hands it down to every layer runner:
// the forward is a function of (context, Run, batch), and no entry point leaves anything behind on the context for it.
struct Run {
    int slot = 0;                              // the in-flight slot: its workspace is c->slots[slot], its per-slot scratch region `slot`
    hipStream_t stream = nullptr;              // slot_stream(c, slot): every launch, memset and copy of the batch goes here
    unsigned* range = nullptr;                 // f16x3: the range record the storing epilogues raise (d_range_base or one of the ring's)
    bool zero_record = false;                  // ... and whether the forward's first kernel zeroes it (ticketed device-path batches)
    SnapArgs snap{};                           // ticketed batches: the last kernel copies the inputs if the record fails (prologue.h)
    int pairs = PAIRS_BOTH;                    // pair selection (params.h): the context's for a new batch, the ticket's for a re-issue
    int precision = 1, impl = 0;               // the arithmetic of THIS run (calibration and the float32 re-issue differ from the context's)
};
// What forward_device reports back: the arithmetic it really ran
struct RunResult {
    bool h3 = false;                           // f16x3 kernels: the record holds this batch's maxima
    bool f32_fallback = false;                 // float32 kernels because of the weight guard (counted once per API call by the caller)
};

// device tables of a layer whose GEMM rows are sorted by padding class (pad_classes.h), and the host copy of the per-tile tap masks
// (what a tile costs: tile_order_pc, forward.hip)
struct PadTables {
    DevMem<int> row_pixel;
    DevMem<unsigned short> tile_taps;
    std::vector<uint16_t> host_taps;
};

// ---- what the context builds at a first use, each whole or not at all ------------------------------------------------------------
// davo_forward's staging (its first call): the input set, the poses on the device and their page-locked bounce buffer, the stream
// the H2D of the next sub-batch runs on while the previous one computes, and one event per sub-batch (the only part that grows)
struct HostStaging {
    InputSet set;
    DevMem<float> d_pose;
    PinnedMem<float> h_pose;
    StreamOwner copy_stream;
    std::vector<EventOwner> copy_done;
};
// davo_submit's pose ring (its first call): entry k holds a batch's poses on the device, their page-locked twin, "the poses are in
// the twin" and "the H2D copies of the batch are done" (recorded only for hold < STREAM_POSES: copy_tracked)
struct PoseRing {
    struct Entry {
        DevMem<float> dev;
        PinnedMem<float> host;
        EventOwner pose_done, copied;
        bool copy_tracked = false;
    } e[STREAM_POSES];
};
// the range guard's ring, stage one (the first f16x3 batch): the stream that reads records and their page-locked mirrors -
// [0] landing pad of a record read, [1 + r] the mirror ring slot r's last kernel writes; h_range_dev is h_range as the device sees it
struct RangeRing {
    StreamOwner read_stream;
    PinnedMem<unsigned> h_range;
    unsigned* h_range_dev = nullptr;
};
// ... stage two (the first ticket that wants a copy of its inputs): the ring slots' input snapshots
struct Snapshots { InputSet sets[RANGE_RING]; };
// the feature export's device block for `cap' windows of every export tensor (davo_set_feature_export)
struct FxBlock {
    DevMem<float> d;
    int cap = 0;
};
// the heat export's device block (davo_set_heat_export): for `cap' windows and both heads the resized sum planes [2][cap][H][W], the
// channel sums they are resized from [2][cap][H/4][W/4] and the maxima [2][cap]; last_np = windows of the piece it holds
struct HeatBlock {
    DevMem<float> d;
    int cap = 0;
    int last_np = 0;
};

// A tracking session (davo_track_begin .. davo_track_end, entry.hip): `lanes' video streams in lockstep, one new frame each per
// push.  The ring keeps the frames, label maps and (depth variants) depth planes of the last pushes on the device as they were
// pushed - never mirrored -, R places of `lanes' frames each, in the context's label and depth element types (window_gather.h:
// track_step says which place a push writes and reads).  Per push index mod R: `uploaded' = its frames are in their place,
// `gathered' = its windows have been read out of the ring; up_stream / ga_stream the stream each was recorded on.
struct TrackState {
    int lanes = 0, policy = 0, R = 0;
    long long pushed = 0;                        // frames per lane so far
    DevMem<void> img, seg, depth;                // [R][lanes] frames of each plane kind
    struct Place {
        EventOwner uploaded, gathered;
        hipStream_t up_stream = nullptr, ga_stream = nullptr;
        bool up = false, ga = false;             // the event has been recorded at all
    };
    std::vector<Place> places;                   // R of them
};

struct Comm;                                     // comm.hip: RCCL communicator state

}  // namespace davo

struct davo_ctx {
    int device = 0, H = 0, W = 0, max_batch = 0;
    std::vector<davo::Slot> slots;             // slots[0] is created by davo_create
    int inflight = 1, next_slot = 0;
    int dev_cus = 256;                         // compute units of the device (hipDeviceProp_t::multiProcessorCount, read by davo_create)
    int ncu = 256;                             // compute units a launch of this context may use (CU-masked slot streams: dev_cus / slots)
    bool cu_partition = false;                 // davo_set_option "cu_partition": slot i's stream is masked to its own share of every XCD's CUs
    hipStream_t user_stream = nullptr;         // davo_set_stream: the caller's stream, which slot 0 then runs on (null: the slot's own)
    davo::LaunchOptions opt;                   // the launch options as davo_set_option stored them (options.h: every field, default and rule)
    std::map<std::vector<int>, davo::DevMem<int>> tile_orders;   // device tables of those launches, by (layer, tile rows, tiles, ...); nullptr = uniform
    std::map<std::vector<int>, davo::PadTables> pad_tables;   // their device tables, by (layer, pair images, map, padding, rate)
    int xcd_rr = -1;                           // workgroups (x, y) of a grid whose x extent is a multiple of 8 share an XCD for every y: -1 not probed yet | 0 no | 1 yes
    davo::GrowBuf d_splitk;                    // split-K partial sums [MAX_INFLIGHT slots][M][2][N] float32
    size_t splitk_floats = 0;                  // ... per slot
    davo::GrowBuf d_pose_tiles;                // per-tile partial sums of the fused pose head, one region per slot likewise
    size_t pose_tiles_floats = 0;
    bool cnv7_valid = true;
    davo::Variant v{};
    float depth_thr = 0.f;                     // att_source 13: pose_exp_net/se_flow/depth_threshold as davo_load_weight received it (the kernels take it as an argument)
    // att_source 14..17: the pool plan of (H, W, att_source) on the device (pool_plan.h; davo_create builds it once), empty in every other variant
    davo::DevMem<int> d_pool_items, d_pool_cell_first;
    davo::DevMem<float> d_pool_inv_div;
    davo::PoolDev pool{};
    int posenn_se = 0;                         // davo_set_posenn_se: 0 none | 1 insert - an SE block on cnv5 ahead of each head's cnv6 (posenn_se.h); cnv6 is then a two-group layer
    int topology = DAVO_POSENN_PAIRS;          // davo_set_posenn_topology: DAVO_POSENN_TRIPLET = one (tgt, src0, src1) image per window through cnv1..cnv7 (cnv1 at 16 packed
                                               // channels, B images a batch), pred six columns wide, the unfused two-pass pose head (forward.hip)
    int heads = DAVO_POSENN_HEADS_DECOUPLED;   // davo_set_posenn_heads: DAVO_POSENN_HEADS_COUPLED = couple_sharednet_v0_dilation - one cnv6 (256 -> c6, one group), one cnv7
                                               // (c6 -> 256, one group, reads all of cnv6), pred six columns wide: fused into cnv7's f16x3 epilogue (NC = 6), else the
                                               // two-pass pose head on a stored cnv7 (forward.hip)
    bool forward_seen = false;                 // a forward has been issued (davo_set_posenn_se, davo_set_posenn_topology and davo_set_posenn_heads are refused from then on)
    davo::InputFormat fmt;                     // davo_set_{label,flow,depth}_format: what every `seg' / `flow' / `depth' argument points at, and what plane_bytes() sizes
    bool inputs_seen = false;                  // an entry point has taken inputs (davo_set_label_format, davo_set_flow_format and davo_set_depth_format are refused from then on)
    int impl = 0;
    int precision = 1;                         // 0 = FP32 MFMA (bit-exact fmaf chains), 1 = f16x3 split (default)
    bool packed_h_ready = false;
    int weight_channel_spread_log2 = 0;        // largest log2 spread of the per-input-channel weight norms over cnv2..cnv7 (weights.hip)
    std::string weight_channel_spread_layer;   // ... and the tensor that has it
    std::string err;
    std::map<std::string, davo::HostTensor> weights;
    std::vector<std::string> needed;
    bool packed_ready = false;                 // float32 convolution weights packed (built at the first float32 forward)
    bool pred_ready = false;                   // pose head kernels on the device (every mode)
    davo::ConvLayer L[7];                      // cnv1..cnv5, cnv6 (fused), cnv7 (grouped)
    davo::DevMem<float> d_wpred, d_bpred;
    davo::DevMem<float> d_wpred_halves;        // coupled PoseNN: pred as [2][256][3], columns 0..2 then 3..5 - what cnv7's six-column fused epilogue reads (null otherwise)
    davo::DevMem<uint8_t> d_w1patch;           // cnv1 B fragments for conv_patch_cnv1_h3 (three-frame PoseNN: for conv_patch_cnv1t_h3)
    davo::DevMem<uint8_t> d_w2patch;           // cnv2 B fragments for conv_patch_cnv2_h3
    davo::DevMem<float> d_w1patch_f32, d_w2patch_f32, d_w3patch_f32;      // float32 mode: cnv1 / cnv2 / cnv3 weights in the patch kernels' register order (conv_patch_f32.h)
    davo::DevMem<uint8_t> d_w3patch;           // cnv3 B fragments for conv_patch_cnv3_h3
    // geometry
    int H1, W1, H2, W2, H3, W3;
    davo::DevMem<float> d_zeros;
    size_t act_floats_per_img[7];              // the activations as the network stores them (davo_debug_read sizes by these; davo_set_posenn_heads changes [5] and [6])
    size_t slot_floats_per_img[7];             // what every slot's d_act buffers hold per image: the decoupled widths, fixed by davo_create, so that a slot built
                                               // at any time (davo_set_inflight) fits whichever heads the context ends up with
    int act_ch[7];
    int pairs = davo::PAIRS_BOTH;              // davo_set_pairs: the pairs of every window the batches issued from now on run
    bool flip = false;                         // davo_set_flip: the batches issued from now on are mirrored left-right where they are staged (window_mirror.h); a batch in
                                               // flight is past that step and its re-issues read the mirrored staging set or snapshot, so neither mirrors again
    // The last forward, as reported: written by forward_device, read by davo_debug_read / davo_last_plan / the feature export
    // alone (last_slot also by last_stream() below) - never an input of a forward
    int last_slot = 0;                         // its slot; 0 again after davo_create, davo_set_posenn_se, davo_set_stream and a rebuild of the slot streams
    int last_B = 0;
    int last_pairs = davo::PAIRS_BOTH;         // davo_debug_read sizes its tensors by last_B windows of that many pair images
    int last_precision = 0;
    int packed_ld = 8;
    bool packed_valid = true;                  // false when cnv1 consumed the raw inputs directly (fused)
    davo::Inputs last_in{};                    // the last forward's inputs: davo_debug_read("packed") re-packs from them after a fused cnv1
    int last_plan[7][2] = {};                  // per layer, per launch: 128-row M tiles * 1000 + tile id / BN (reported by the bench)
    int last_split[7] = {};                    // per layer: split-K parts of the last forward's launch (1: one K chain; davo_last_split)
    std::optional<davo::HostStaging> host;     // davo_forward's staging (built by its first call)
    // f16x3 range management: activations are stored as fp16 pairs scaled by 2^act_shift[layer] (davo_calibrate);
    // every storing epilogue atomicMax-es the largest stored magnitude into word `layer' of the run's record (Run::range)
    int act_shift[7] = {0, 0, 0, 0, 0, 0, 0};
    davo::DevMem<unsigned> d_range_base;       // [1 + RANGE_RING][RANGE_WORDS] (params.h): record 0 serves the host path, calibration and re-issues; 1.. the ring
    // Range recovery (davo_set_option "auto_range", default on): every device-path batch is judged on a record of its own, at the
    // latest when its ring slot is needed again (RANGE_RING batches later) or at davo_synchronize; a failed verdict re-issues that
    // batch from the context's own copy of its inputs - recalibrated, or on the float32 kernels (range_guard.hip)
    bool opt_auto_range = true;
    bool opt_stable_inputs = false;            // "stable_inputs": the caller keeps inputs unchanged until the verdict, no copies are taken
    davo::RangeBook book;                      // the guard's bookkeeping: ring cursor, tickets, pose spans, deferred verdict (range_book.h)
    std::optional<davo::RangeRing> ring;       // the records' host mirrors and the stream that reads them (range_guard.hip: ensure_ring)
    std::optional<davo::Snapshots> snaps;      // the ring slots' input snapshots (built for the first ticket that wants one)
    float range_seen[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // largest true |activation| judged since the last reset
    std::string range_report;                  // what the range management last did, in words (davo_range_report)
    long long n_recalibrations = 0, n_f32_batches = 0, n_reissued = 0;
    int host_chunk = 8;                        // davo_forward: windows per sub-batch (davo_set_option "host_chunk"; 0 = whole batch)
    // feature export (davo_set_feature_export / davo_forward_features, export.hip): one device block for fx->cap windows of every
    // export tensor, absent with the export off
    bool fx_on = false;
    std::optional<davo::FxBlock> fx;
    // heat export (davo_set_heat_export / davo_forward_heat, export.hip): a block of its own, absent with the export off
    std::optional<davo::HeatBlock> heat;
    // streaming host entry (davo_submit / davo_wait): staging input sets, pose ring, undelivered batches in issue order
    davo::InputSet stream_sets[davo::MAX_INFLIGHT];     // one staging set per in-flight slot (built by the slot's first davo_submit, davo_submit_frames or davo_forward_device_frames)
    std::optional<davo::PoseRing> pose_ring;   // built by the first davo_submit
    davo::FrameSet frame_sets[davo::MAX_INFLIGHT];      // frame layout: one frame buffer per in-flight slot (built by the slot's first davo_submit_frames; [0] also by davo_forward_frames)
    std::optional<davo::TrackState> track;     // online tracking: the session's ring and events (davo_track_begin builds it whole, davo_track_end and davo_destroy free it)
    std::deque<davo::StreamJob> jobs;
    unsigned long long n_submitted = 0;
    davo::DevMem<float> d_reissue_pose;        // a re-issued batch writes here first; copied to its own pose buffer unless a later batch has taken that
    // profiling
    bool prof = false;
    bool prof_dominant_only = false;           // profile mode 2: bracket only the main cnv6 launch
    int prof_stride = 1, prof_tick = 0;        // ... of every prof_stride-th batch (davo_set_option "profile_stride"): an event pair
                                               // costs two ~6 us bubbles around the launch it brackets
    std::vector<davo::ProfEntry> prof_entries;
    std::vector<davo::EventOwner> event_pool;
    // multi-GPU (comm.hip)
    davo::Comm* comm = nullptr;                // owned through comm_release (the type is comm.hip's)
};

namespace davo {

inline int fail(davo_ctx* c, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIP_TRY(c, expr)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return ::davo::fail(c, DAVO_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                           \
    } while (0)

// bytes of one window of each input plane
struct PlaneBytes { size_t img, flow, seg, depth; };
inline PlaneBytes plane_bytes(const davo_ctx* c) {
    const size_t HW = (size_t)c->H * c->W;
    // seg: [3,H,W,1] in the context's label format, float32 or bytes; depth: [3,H,W,1] in the context's depth format, float32 or binary16 (davo.py:991-996).  H W is a
    // multiple of 16, so every window of every plane starts 16-byte aligned where the block does, in either format.  flow: [4,H,W,2] in
    // the context's flow format, float32 or binary16: a plane of 2 H W halves is still a multiple of 64 bytes
    const ElemBytes e = element_bytes(c->fmt);
    return PlaneBytes{HW * 9, HW * 8 * e.flow, HW * 3 * e.label, HW * 3 * e.depth};
}
inline bool needs_depth(const davo_ctx* c) { return att_reads_depth(c->v.att_source); }
// the calls a tracking session refuses (davo_set_inflight, the export switches, davo_calibrate): DAVO_OK outside a session
inline int refuse_while_tracking(davo_ctx* c, const char* fn) {
    return c->track ? fail(c, DAVO_ERR_INVALID, "%s: a tracking session is open (davo_track_begin): call davo_track_end first", fn) : DAVO_OK;
}
inline bool triplet(const davo_ctx* c) { return c->topology == DAVO_POSENN_TRIPLET; }
// images a batch of B windows sends through cnv1..cnv7: one per selected pair, or one per window in the three-frame PoseNN
inline int batch_images(const davo_ctx* c, int B, int sel) { return triplet(c) ? B : pairs_per_window(sel) * B; }
// columns of a head's pred, and TF input channels of cnv1 (nets/posenn.py:78,120)
inline bool coupled(const davo_ctx* c) { return c->heads == DAVO_POSENN_HEADS_COUPLED; }
inline int pred_cols(const davo_ctx* c) { return (triplet(c) || coupled(c)) ? 6 : 3; }
inline int cnv1_cin_tf(const davo_ctx* c) { return (triplet(c) ? 3 : 2) * c->v.cin_per_frame; }

// the stream slot i runs on: its own, or the caller's for slot 0 (davo_set_stream)
inline hipStream_t slot_stream(const davo_ctx* c, int i) { return (c->user_stream && i == 0) ? c->user_stream : c->slots[i].stream.get(); }
// a batch in slot i as the context's settings of the moment say, on the base record (range_guard.hip: ticket_begin moves it to a record of its own)
inline Run make_run(const davo_ctx* c, int i) {
    return Run{i, slot_stream(c, i), c->d_range_base.get(), false, SnapArgs{}, c->pairs, c->precision, c->impl};
}
// outside a forward (davo_memcpy_*, davo_debug_read, the feature export): the stream and workspace of the most recently issued batch
inline hipStream_t last_stream(const davo_ctx* c) { return slot_stream(c, c->last_slot); }
inline const Slot& last_workspace(const davo_ctx* c) { return c->slots[c->last_slot]; }

// ---- profiling: HIP events around a launch on stream s ---------------------------------------
struct ProfScope {
    davo_ctx* c;
    hipStream_t s;
    ProfEntry* e = nullptr;
    EventOwner a, b;                           // out of the context's pool, back into it (or into e->pending) at the end
    ProfScope(davo_ctx* ctx, hipStream_t stream, const char* name);
    ~ProfScope();
};
int prof_collect(davo_ctx* c);
int sync_all_slots(davo_ctx* c);

// ---- weights.hip ----------------------------------------------------------------------------
void init_layer(ConvLayer& L, const char* label, int KS, int stride, int rate, int cin, int cout, int groups);
void init_posenn_layers(ConvLayer (&L)[7], int c6);
void init_coupled_head(ConvLayer (&L)[7], int c6);      // cnv6 and cnv7 of the coupled network, one group each
std::vector<std::string> needed_names(const Variant& v, int posenn_se = 0, bool coupled = false);
// TF name of an SE dense tensor of the variant's scope (k: 0 bottleneck_fc/kernel, 1 its bias, 2 recover_fc/kernel, 3 its bias);
// the se_flow scope's for the variants without SE layers (the kernels do not read them there)
const char* se_weight_name(int att_source, int k);
// att_source 13: the se_flow_near tensors are se_weight_name(13, k), the se_flow_far ones se_far_weight_name(k); the scalar threshold:
const char* se_far_weight_name(int k);
constexpr const char* DEPTH_THRESHOLD_NAME = "pose_exp_net/se_flow/depth_threshold";
// the SE layers' scope is a dense tensor the kernels read in the reference's [in,out] layout (not re-laid-out like a convolution)
bool is_dense_weight(const std::string& name);
bool expected_shape(const davo_ctx* c, const std::string& name, std::vector<int64_t>* sh);
int upload(davo_ctx* c, const std::vector<float>& host, DevMem<float>* dev);      // frees what *dev held first
int build_packed_weights(davo_ctx* c);
int build_pred_weights(davo_ctx* c);
int build_packed_weights_h3(davo_ctx* c);
int missing_weights(davo_ctx* c, std::string* names);
float weight_prescale(const float* w, size_t n);
void pack_conv_weights(const float* w_tf, int KS, int cin_tf, int cout, const int* chmap, int cin_packed,
                       int npad, int kpad, float* out);
void pack_conv_weights_h3(const float* w_tf, int KS, int cin_tf, int cout, const int* chmap, int cin_packed,
                          int cb_log2, int tpc_log2, int cpb, int nchunks, float scale, _Float16* out);
inline void split_f16(float v, _Float16* hi, _Float16* lo) {
    const _Float16 h = (_Float16)v;
    *hi = h;
    *lo = (_Float16)(v - (float)h);
}

// ---- forward.hip ----------------------------------------------------------------------------
// B windows of `in' -> d_pose, run as `run' says; *res (if not null) receives what really ran
int forward_device(davo_ctx* c, const Run& run, int B, const Inputs& in, void* d_pose, RunResult* res = nullptr);

// ---- api.hip --------------------------------------------------------------------------------
int zero_now(davo_ctx* c, void* p, size_t bytes);                              // hipMemset that returns when the bytes ARE zero
int alloc_input_set(davo_ctx* c, InputSet* s, bool zero_unread);               // *s is assigned whole, or left as it was

// ---- export.hip -----------------------------------------------------------------------------
// what a davo_forward_features / davo_forward_heat call wants beside the poses; null = nothing of that kind
struct Exports {
    const davo_feature_out* fx = nullptr;
    const davo_heat_out* heat = nullptr;
    explicit operator bool() const { return fx || heat; }
};
int export_all(davo_ctx* c, const Exports& ex, const Inputs& in, int w0, int nw, int b0, int B);

// ---- entry.hip ------------------------------------------------------------------------------
// A batch as the caller handed it to an entry point: the layout, the four pointers under the names the layout gives them (the two
// structs share one shape: what treats all layouts alike reads `win'), where they point, the entry point's family name for
// messages (the window forms append `_depth' themselves) and whether its signature has a depth parameter at all.
// Windows: img [B,H,3W,3], flow [B,4,H,W,2], seg and depth [B,3,H,W,1]; frames: frames [N+2,H,W,3], flow2 [N,2,H,W,2], seg and depth [N+2,H,W,1]
enum class Layout { Windows, Frames };
struct FrameInputs { const void *frames, *flow2, *seg, *depth; };
struct Batch {
    Layout layout;
    union { Inputs win; FrameInputs fr; };
    bool on_device;
    const char* fn;
    bool depth_param;
};
inline Batch window_batch(const char* fn, bool on_device, bool depth_param, const void* img, const void* flow, const void* seg, const void* depth) {
    return Batch{Layout::Windows, {Inputs{img, flow, seg, depth}}, on_device, fn, depth_param};
}
inline Batch frame_batch(const char* fn, bool on_device, const void* frames, const void* flow2, const void* seg, const void* depth) {
    Batch b{Layout::Frames, {}, on_device, fn, true};
    b.fr = FrameInputs{frames, flow2, seg, depth};
    return b;
}
int check_batch(davo_ctx* c, Batch* b, int B, bool out_given, int hold = 0);   // the one argument check; clears a depth pointer the variant does not read
Inputs from_window(const davo_ctx* c, const Inputs& in, int b0);               // windows b0.. of a batch's planes
int forward_entry(davo_ctx* c, int B, Batch b, float* pose_out, Exports ex = Exports{});      // davo_forward's body, with the exports wanted
int deliver_all(davo_ctx* c);                                                  // every davo_submit batch still under way, in issue order
void drain_own_streams(davo_ctx* c);
int mirror_device_batch(davo_ctx* c, const Inputs& in, int B, Inputs* out);    // davo_calibrate with flip on: the batch mirrored into slot 0's staging set

// ---- range_guard.hip: what the entry points need of the f16x3 range guard --------------------
int ensure_ring(davo_ctx* c, bool snapshots);                                  // the records' host mirrors (and the ring's input snapshots)
// the record of sequence number seq is final in mirror m (its last kernel ran on stream s) -> raw; at once where s is idle
int wait_record(davo_ctx* c, const unsigned* m, unsigned seq, hipStream_t s, unsigned raw[RANGE_WORDS]);
int judge_record(davo_ctx* c, const unsigned* raw /*[RANGE_WORDS]*/, const int* shifts);      // the verdict: DAVO_ERR_RANGE names the layer
int recover_batch(davo_ctx* c, const Reissue& b);                              // a failed verdict: re-issue (as is, recalibrated, float32)
int judge_front(davo_ctx* c);                                                  // verdict (and re-issue) of the oldest pending ticket
int judge_all(davo_ctx* c);                                                    // ... of every one; returns the deferred verdict, if any
int freeze_pending_and_reset_ring(davo_ctx* c);                                // every stream idle, the scales are about to change
int calibrate_on(davo_ctx* c, int B, const Inputs& in, void* d_pose, int sel);
// a ticketed batch: the ring slot is free / *run records into it, *t says what a re-issue would read / the batch is out
int ticket_reserve(davo_ctx* c);
int ticket_begin(davo_ctx* c, Run* run, int B, const Inputs& in, Ticket* t, bool own_inputs = false);
int ticket_end(davo_ctx* c, int rc, const RunResult& res, Ticket t, void* d_pose, float* h_pose = nullptr);

// ---- comm.hip -------------------------------------------------------------------------------
void comm_release(davo_ctx* c);

}  // namespace davo
