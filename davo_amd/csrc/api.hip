// api.hip — the extern "C" entry points of libdavo_hip.so (include/davo_hip.h): context life
// cycle, weight loading, the host- and device-buffer forward calls, the streaming state,
// measurement and test hooks.  The forward plan itself is forward.hip; the f16x3 range guard
// around it is range_guard.hip (bookkeeping: range_book.h); kernels are reached through
// launch.h; the RCCL communicator is comm.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <cstring>

#include "ctx.h"
#include "launch.h"
#include "pad_classes.h"
#include "plan.h"
#include "window_gather.h"

using namespace davo;

namespace davo {

// hipMemset runs on the null stream and may return before the fill has run; the context's streams are non-blocking, so nothing
// orders them behind it.  (Found as one wrong batch in twenty streamed runs: the zero fill of a slot's new staging set landed on
// top of the first batch's freshly copied flow planes, profiles/r05f_stream_flake.log.)  Returns when the bytes ARE zero.
int zero_now(davo_ctx* c, void* p, size_t bytes) {
    HIP_TRY(c, hipMemset(p, 0, bytes));
    HIP_TRY(c, hipStreamSynchronize(nullptr));
    return DAVO_OK;
}

// Room for max_batch windows of every plane the variant reads.  zero_unread: the flow and label planes start out zero - what the path
// never reads (flow planes 2,3; the target frame's label map) is never copied into a davo_submit staging set: defined contents all the same
int alloc_input_set(davo_ctx* c, InputSet* out, bool zero_unread) {
    const PlaneBytes nb = plane_bytes(c);
    const size_t n = (size_t)c->max_batch;
    InputSet s;
    HIP_TRY(c, dev_alloc(&s.img, nb.img * n));
    HIP_TRY(c, dev_alloc(&s.flow, nb.flow * n));
    HIP_TRY(c, dev_alloc(&s.seg, nb.seg * n));
    if (needs_depth(c)) HIP_TRY(c, dev_alloc(&s.depth, nb.depth * n));      // always copied whole
    if (zero_unread) {
        { int rc = zero_now(c, s.flow.get(), nb.flow * n); if (rc) return rc; }
        { int rc = zero_now(c, s.seg.get(), nb.seg * n); if (rc) return rc; }
    }
    *out = std::move(s);
    return DAVO_OK;
}

}  // namespace davo

namespace {

// the feature-attention variant's room in one slot (posenn_se.h): the 512-channel scaled tensor of cnv5's geometry (2,048 bytes per
// pixel in either arithmetic mode), the scale table and the squeeze's partial sums.  Nothing of it exists with the mode off.
int alloc_se_workspace(davo_ctx* c, Slot* s) {
    const size_t NB = 2 * (size_t)c->max_batch;
    s->se.reset();
    SeWorkspace w;
    HIP_TRY(c, dev_alloc(&w.d_se, NB * c->H2 * c->W2 * 512));
    HIP_TRY(c, dev_alloc(&w.d_se_scale, NB * 2 * 256));
    HIP_TRY(c, dev_alloc(&w.d_se_partial, NB * SE5_CHUNKS * 256));
    s->se = std::move(w);
    return DAVO_OK;
}

// one more in-flight slot (stream + activation workspace for max_batch triplets): appended once it is complete
int add_slot(davo_ctx* c) {
    const size_t NB = 2 * (size_t)c->max_batch;
    Slot s;
    HIP_TRY(c, stream_create(&s.stream));
    for (int i = 0; i < 7; ++i) HIP_TRY(c, dev_alloc(&s.d_act[i], NB * c->act_floats_per_img[i]));
    HIP_TRY(c, dev_alloc(&s.d_packed, NB * (size_t)c->H * c->W * 10));
    // squeeze partials: se_flow [B][2 sources][SQ_CHUNKS][2] floats, the class-table sources [B][3 frames][SQ_CHUNKS][SQ_REC] words
    const size_t partial_floats = (size_t)c->max_batch * SQ_CHUNKS * (att_class_table(c->v.att_source) ? 3 * SQ_REC : 2 * 2);
    HIP_TRY(c, dev_alloc(&s.d_partial, partial_floats));
    HIP_TRY(c, dev_alloc(&s.d_tab, (size_t)c->max_batch * 3 * NCLS));
    if (c->v.att_source == ATT_DEPTH_SPLIT) HIP_TRY(c, dev_alloc(&s.d_tab_far, (size_t)c->max_batch * 3 * NCLS));      // the far MLP's tables: this source only
    HIP_TRY(c, dev_alloc(&s.d_pose_partial, NB * 2 * PH_SPLIT * 3));
    { int rc = zero_now(c, s.d_partial.get(), partial_floats * sizeof(float)); if (rc) return rc; }
    const size_t counters = (size_t)c->max_batch + 1 + SK_TILE_COUNTERS;
    HIP_TRY(c, dev_alloc(&s.d_counters, counters));
    { int rc = zero_now(c, s.d_counters.get(), counters * sizeof(unsigned)); if (rc) return rc; }
    if (c->posenn_se) { int rc = alloc_se_workspace(c, &s); if (rc) return rc; }
    c->slots.push_back(std::move(s));
    return DAVO_OK;
}

}  // namespace

// ============================================================================================
extern "C" {

int davo_create(davo_ctx** out, int device, int H, int W, int max_batch, const davo_variant* v) {
    if (!out || !v) return DAVO_ERR_INVALID;
    *out = nullptr;
    davo_ctx* c = new davo_ctx();
    *out = c;                                   // returned even on failure so the message is readable
    c->device = device; c->H = H; c->W = W; c->max_batch = max_batch;
    c->v = Variant{v->cin_per_frame, v->cnv6_out, v->se_act, v->norm_flow, v->abs_mode, v->att_source,
                   v->mask_rgb, v->mask_info};
    if (H < 16 || W < 16 || H % 4 || W % 4) return fail(c, DAVO_ERR_INVALID, "H and W must be multiples of 4 and >= 16 (got %dx%d)", H, W);
    if (max_batch < 1) return fail(c, DAVO_ERR_INVALID, "max_batch must be >= 1");
    if (v->cin_per_frame != 5 && v->cin_per_frame != 3) return fail(c, DAVO_ERR_INVALID, "cin_per_frame must be 3 or 5");
    if (ilog2_exact(v->cnv6_out) < 5 || v->cnv6_out > 256) return fail(c, DAVO_ERR_INVALID, "cnv6_out must be 32, 64, 128 or 256");
    if (v->se_act < 0 || v->se_act > 2 || v->abs_mode < 0 || v->abs_mode > 3 || v->att_source < 0 || v->att_source > ATT_DEPTH_SPLIT)
        return fail(c, DAVO_ERR_INVALID, "variant field out of range");
    int ndev = 0;
    HIP_TRY(c, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(c, DAVO_ERR_INVALID, "device %d not present (%d visible)", device, ndev);
    HIP_TRY(c, hipSetDevice(device));
    {   // the launch planner sizes whole rounds for the CUs this device really has (a partitioned MI355X exposes fewer than 256)
        hipDeviceProp_t prop;
        HIP_TRY(c, hipGetDeviceProperties(&prop, device));
        c->dev_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        c->ncu = c->dev_cus;
    }
    c->needed = needed_names(c->v);

    c->H1 = (H + 1) / 2; c->W1 = (W + 1) / 2;
    c->H2 = (c->H1 + 1) / 2; c->W2 = (c->W1 + 1) / 2;
    c->H3 = (c->H2 + 1) / 2; c->W3 = (c->W2 + 1) / 2;
    const int c6 = c->v.cnv6_out;
    init_layer(c->L[0], "cnv1", 7, 2, 1, 8, 16, 1);
    init_layer(c->L[1], "cnv2", 5, 2, 1, 16, 32, 1);
    init_layer(c->L[2], "cnv3", 3, 1, 2, 32, 64, 1);
    init_layer(c->L[3], "cnv4", 3, 1, 4, 64, 128, 1);
    init_layer(c->L[4], "cnv5", 3, 1, 8, 128, 256, 1);
    init_layer(c->L[5], "cnv6", 3, 1, 2, 256, 2 * c6, 1);
    init_layer(c->L[6], "cnv7", 3, 2, 1, c6, 256, 2);

    const int ch[7] = {16, 32, 64, 128, 256, 2 * c6, 512};
    const size_t px[7] = {(size_t)c->H1 * c->W1, (size_t)c->H2 * c->W2, (size_t)c->H2 * c->W2, (size_t)c->H2 * c->W2,
                          (size_t)c->H2 * c->W2, (size_t)c->H2 * c->W2, (size_t)c->H3 * c->W3};
    for (int i = 0; i < 7; ++i) {
        c->act_ch[i] = ch[i];
        c->act_floats_per_img[i] = px[i] * ch[i];
    }
    { int rc = add_slot(c); if (rc) return rc; }
    HIP_TRY(c, dev_alloc(&c->d_zeros, 256 / sizeof(float)));
    { int rc = zero_now(c, c->d_zeros.get(), 256); if (rc) return rc; }
    HIP_TRY(c, dev_alloc(&c->d_range_base, (1 + RANGE_RING) * RANGE_WORDS));
    { int rc = zero_now(c, c->d_range_base.get(), (1 + RANGE_RING) * RANGE_WORDS * sizeof(unsigned)); if (rc) return rc; }
    return DAVO_OK;
}

int davo_set_posenn_se(davo_ctx* c, int mode) {
    if (!c) return DAVO_ERR_INVALID;
    if (mode != 0 && mode != 1) return fail(c, DAVO_ERR_INVALID, "posenn_se mode must be 0 (none) or 1 (insert)");
    if (!c->weights.empty() || c->forward_seen)
        return fail(c, DAVO_ERR_INVALID, "davo_set_posenn_se must be called before the first davo_load_weight and the first forward "
                    "(it changes the variant's variables and cnv6's layout)");
    if (mode && c->v.att_source != 0)
        return fail(c, DAVO_ERR_INVALID, "the feature-attention PoseNN (`-se_insert') runs with att_source 0 (`-no_segmask') only, got %d", c->v.att_source);
    HIP_TRY(c, hipSetDevice(c->device));
    c->posenn_se = mode;
    // the heads read different inputs now: cnv6 becomes one group per head, the grouped path cnv7 runs on (forward.hip)
    const int c6 = c->v.cnv6_out;
    if (mode) init_layer(c->L[5], "cnv6", 3, 1, 2, 256, c6, 2);
    else init_layer(c->L[5], "cnv6", 3, 1, 2, 256, 2 * c6, 1);
    c->needed = needed_names(c->v, mode);
    for (Slot& s : c->slots) {
        if (mode) { int rc = alloc_se_workspace(c, &s); if (rc) return rc; }
        else s.se.reset();
    }
    c->last_slot = 0;
    return DAVO_OK;
}

int davo_set_label_format(davo_ctx* c, int fmt) {
    if (!c) return DAVO_ERR_INVALID;
    if (fmt != DAVO_LABELS_F32 && fmt != DAVO_LABELS_U8)
        return fail(c, DAVO_ERR_INVALID, "label format must be DAVO_LABELS_F32 (0) or DAVO_LABELS_U8 (1), got %d", fmt);
    // everything sized by plane_bytes() follows the format: it is fixed once inputs were taken or a set of them was allocated
    bool sets = static_cast<bool>(c->host) || static_cast<bool>(c->snaps);
    for (const InputSet& s : c->stream_sets) sets = sets || s.built();
    for (const FrameSet& s : c->frame_sets) sets = sets || s.built();
    if (c->inputs_seen || c->forward_seen || sets)
        return fail(c, DAVO_ERR_INVALID, "davo_set_label_format must be called before the first call that takes inputs "
                    "(the staging sets, the range guard's snapshots and every copy are sized by it)");
    c->label_fmt = fmt;
    return DAVO_OK;
}

int davo_get_label_format(const davo_ctx* c) { return c ? c->label_fmt : DAVO_ERR_INVALID; }

int davo_load_weight(davo_ctx* c, const char* tf_name, const float* data, const int64_t* shape, int ndim) {
    // ndim 0: a scalar variable (the depth threshold); shape may then be null
    if (!c || !tf_name || !data || ndim < 0 || ndim > 4 || (!shape && ndim > 0)) return fail(c, DAVO_ERR_INVALID, "bad argument to davo_load_weight");
    std::vector<int64_t> want;
    if (!expected_shape(c, tf_name, &want)) return fail(c, DAVO_ERR_INVALID, "unknown variable `%s'", tf_name);
    bool listed = false;
    for (auto& n : c->needed) listed |= (n == tf_name);
    if (!listed) return fail(c, DAVO_ERR_INVALID, "variable `%s' is not part of this variant", tf_name);
    std::vector<int64_t> got;
    if (ndim > 0) got.assign(shape, shape + ndim);
    if (got != want) {
        std::string g, w;
        for (auto d : got) g += std::to_string(d) + ",";
        for (auto d : want) w += std::to_string(d) + ",";
        return fail(c, DAVO_ERR_INVALID, "`%s': shape [%s] does not match expected [%s]", tf_name, g.c_str(), w.c_str());
    }
    size_t n = 1;
    for (auto d : got) n *= (size_t)d;
    HostTensor& t = c->weights[tf_name];
    t.shape = got;
    t.data.assign(data, data + n);
    if (strcmp(tf_name, DEPTH_THRESHOLD_NAME) == 0) c->depth_thr = data[0];      // the kernels take it as an argument from this host copy
    HIP_TRY(c, hipSetDevice(c->device));
    // the kernels read the small dense tensors (SE fully-connected layers, static channel weights) in the reference's own layout;
    // the convolution tensors are re-laid-out at the first forward (weights.hip) and their raw device copy is only the test hook's
    // (impl 1: uploaded on demand, forward.hip) - 20 hipMalloc + copies less in front of a rank's first batch
    const std::string nm = tf_name;
    const bool dense = is_dense_weight(nm);
    t.dev.reset();
    if (dense) { int rc = upload(c, t.data, &t.dev); if (rc) return rc; }
    c->packed_ready = false;
    c->packed_h_ready = false;
    c->pred_ready = false;
    return DAVO_OK;
}

int davo_weights_missing(davo_ctx* c) {
    if (!c) return DAVO_ERR_INVALID;
    std::string names;
    const int n = missing_weights(c, &names);
    if (n) c->err = "weights not loaded: " + names;
    return n;
}

// ---- the forward entry points ----------------------------------------------------------------------------
// The f16x3 batches they issue are judged by the range guard (range_guard.hip, reached through ctx.h; bookkeeping: c->book).
namespace {

// The depth argument of an entry point.  A variant that reads depth planes (att_source 11, 12, 13) must be called through the `_depth' form with
// the planes; every other variant reads no depth: the `_depth' forms accept a pointer (or null) and ignore it.
int resolve_depth(davo_ctx* c, const char* fn, bool depth_form, const void** depth) {
    if (!needs_depth(c)) { *depth = nullptr; return DAVO_OK; }
    if (!depth_form) return fail(c, DAVO_ERR_INVALID, "%s: this variant reads depth planes (att_source %d): call %s_depth", fn, c->v.att_source, fn);
    if (!*depth) return fail(c, DAVO_ERR_INVALID, "%s_depth: null depth pointer", fn);
    return DAVO_OK;
}

// frame layout (defined with the streaming entry point below)
// A frame-layout batch as the caller handed it: frames [N+2,H,W,3], flow2 [N,2,H,W,2], seg and depth [N+2,H,W,1]
struct FrameInputs { const void *frames, *flow2, *seg, *depth; };
int resolve_frames_depth(davo_ctx* c, const char* fn, const void** depth);
int gather_windows(davo_ctx* c, const InputSet& set, const FrameInputs& fr, int b0, int nb, int sel, hipStream_t s);

}  // namespace

// the body of davo_forward_device / davo_forward_device_depth (depth_form) and of davo_forward_device_frames (frames: d_img, d_flow,
// d_seg, d_depth are the frame layout's d_frames, d_flow2, d_seg, d_depth; the batch runs on the slot's staging set, gathered from them)
static int forward_device_entry(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg, const void* d_depth,
                                void* d_pose, float* elapsed_ms, bool depth_form, bool frames = false) {
    if (!c) return DAVO_ERR_INVALID;
    if (B < 1 || B > c->max_batch) return fail(c, DAVO_ERR_INVALID, "batch %d outside [1,%d]", B, c->max_batch);
    if (!d_img || !d_flow || !d_seg || !d_pose) return fail(c, DAVO_ERR_INVALID, "null device pointer");
    { int rc = frames ? resolve_frames_depth(c, "davo_forward_device_frames", &d_depth) : resolve_depth(c, "davo_forward_device", depth_form, &d_depth); if (rc) return rc; }
    if (frames && (((uintptr_t)d_img | (uintptr_t)d_flow | (uintptr_t)d_seg | (uintptr_t)d_depth) & 15))
        return fail(c, DAVO_ERR_INVALID, "davo_forward_device_frames: device input buffers must be 16-byte aligned");
    c->inputs_seen = true;
    HIP_TRY(c, hipSetDevice(c->device));
    if (frames && !c->stream_sets[c->next_slot].built()) { int rc = alloc_input_set(c, &c->stream_sets[c->next_slot], true); if (rc) return rc; }
    const Inputs in = frames ? c->stream_sets[c->next_slot].view() : Inputs{d_img, d_flow, d_seg, d_depth};
    const bool ticketed = c->impl == 0 && c->precision == 1;      // f16x3: the batch gets a record (and a copy of its inputs) of its own
    if (ticketed) { int rc = ticket_reserve(c); if (rc) return rc; }
    // rotate through the in-flight slots: this batch runs on its own stream and workspace
    Run run = make_run(c, c->next_slot);
    const int slot = c->next_slot;
    c->next_slot = (c->next_slot + 1) % c->inflight;
    EventOwner e0, e1;
    if (frames) {
        // the windows into the slot's staging set, in stream order behind the forward that last read it and ahead of the ticket: the
        // caller's buffers are free once this launch has run, and the batch is the library's own from here on (own_inputs below).
        // The timed form brackets the gather too: elapsed_ms is what the layout costs on resident inputs
        if (elapsed_ms) {
            HIP_TRY(c, event_create(&e0));
            HIP_TRY(c, hipEventRecord(e0.get(), run.stream));
        }
        int rc = gather_windows(c, c->stream_sets[slot], FrameInputs{d_img, d_flow, d_seg, d_depth}, 0, B, run.pairs, run.stream);
        if (rc) return rc;
    }
    Ticket t{};
    if (ticketed) { int rc = ticket_begin(c, &run, B, in, &t, frames); if (rc) return rc; }
    if (!ticketed && c->book.spans_full()) {               // float32 batches behind pending f16x3 tickets: bounded
        const int rc = judge_all(c);
        if (rc == DAVO_ERR_RANGE) c->book.defer(rc, c->err);       // "auto_range" 0: reported by the next davo_synchronize (judge_all has just emptied the store)
        else if (rc) return rc;
    }
    c->book.note_issue(d_pose, B);
    RunResult res;
    if (!elapsed_ms) {
        int rc = forward_device(c, run, B, in, d_pose, &res);
        return ticketed ? ticket_end(c, rc, res, t, d_pose) : rc;      // (only a ticketed batch starts as f16x3, so only it can fall back)
    }
    int rc = DAVO_OK;
    auto hip_ok = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == DAVO_OK) rc = fail(c, DAVO_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
        return e == hipSuccess;
    };
    if (hip_ok(event_create(&e1), "hipEventCreate") &&
        (e0 || (hip_ok(event_create(&e0), "hipEventCreate") && hip_ok(hipEventRecord(e0.get(), run.stream), "hipEventRecord")))) {
        rc = forward_device(c, run, B, in, d_pose, &res);
        if (rc == DAVO_OK && hip_ok(hipEventRecord(e1.get(), run.stream), "hipEventRecord") &&
            hip_ok(hipEventSynchronize(e1.get()), "hipEventSynchronize"))
            hip_ok(hipEventElapsedTime(elapsed_ms, e0.get(), e1.get()), "hipEventElapsedTime");
    }
    if (ticketed) rc = ticket_end(c, rc, res, t, d_pose);
    // the timed form is synchronous, so it can judge (and, if need be, re-issue) its own batch; elapsed_ms is the first issue's
    if (rc == DAVO_OK && c->inflight == 1) rc = judge_all(c);
    return rc;
}

int davo_forward_device(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg,
                        void* d_pose, float* elapsed_ms) {
    return forward_device_entry(c, B, d_img, d_flow, d_seg, nullptr, d_pose, elapsed_ms, false);
}

int davo_forward_device_depth(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg, const void* d_depth,
                              void* d_pose, float* elapsed_ms) {
    return forward_device_entry(c, B, d_img, d_flow, d_seg, d_depth, d_pose, elapsed_ms, true);
}

int davo_forward_device_frames(davo_ctx* c, int N, const void* d_frames, const void* d_flow2, const void* d_seg, const void* d_depth,
                               void* d_pose, float* elapsed_ms) {
    return forward_device_entry(c, N, d_frames, d_flow2, d_seg, d_depth, d_pose, elapsed_ms, true, true);
}

int davo_frames_plan(int H, int W, int N, int pairs, int att_source, int label_fmt, int* ranges, long long* link_bytes) {
    if (H < 1 || W < 1 || N < 1 || (pairs != PAIRS_SRC0 && pairs != PAIRS_SRC1 && pairs != PAIRS_BOTH) || att_source < 0 || att_source > ATT_DEPTH_SPLIT ||
        (label_fmt != LABELS_F32 && label_fmt != LABELS_U8))
        return DAVO_ERR_INVALID;
    const FramePlan p = frame_plan(N, pairs, att_source);
    if (ranges) {
        const int r[8] = {p.img[0], p.img[1], p.seg[0], p.seg[1], p.depth[0], p.depth[1], p.flow[0], p.flow[1]};
        memcpy(ranges, r, sizeof r);
    }
    if (link_bytes) *link_bytes = frame_plan_bytes(p, N, H, W, label_fmt == LABELS_U8 ? 1 : 4);
    return DAVO_OK;
}


// ---- streaming host entry: davo_submit / davo_wait ----------------------------------------------------------------
// The reference's driver pulls batches through tf.data's prefetch(8B) while the session runs (test_kitti_pose.py:133-145,
// data_loader.py:321-324): input transfer, compute and result delivery of neighbouring batches overlap.  davo_forward cannot (it
// returns poses), so the sequence driver uses this pair.  davo_submit rotates through the in-flight slots like
// davo_forward_device; on the slot's OWN stream it queues the H2D copies of the batch into the slot's staging set, the forward,
// and the D2H of the poses into a page-locked ring entry.  A stream runs in order, so the staging set is safe to refill without an
// event, and with two or more slots the copies of batch n+1 run under the kernels of batch n.  (First built with a copy stream
// and events between it and the slots: each hipEventRecord costs 6 us of host time and a marker on the queue,
// profiles/r05a_hip_call_cost.log, and the batch-1 loop ran at 134-168 us per window.)  davo_wait / davo_synchronize judge the
// batch's range ticket (re-issuing it if need be) and only then write the poses into the caller's array.  Inputs, poses and range
// snapshots of a batch all live in context-owned memory.
namespace {

int ensure_stream_state(davo_ctx* c, int slot) {
    if (!c->pose_ring) {
        PoseRing ring;
        for (PoseRing::Entry& e : ring.e) {
            HIP_TRY(c, dev_alloc(&e.dev, (size_t)c->max_batch * 12));
            HIP_TRY(c, pinned_alloc(&e.host, (size_t)c->max_batch * 12, hipHostMallocDefault));
            HIP_TRY(c, event_create(&e.pose_done, hipEventDisableTiming));
            HIP_TRY(c, event_create(&e.copied, hipEventDisableTiming));
        }
        c->pose_ring = std::move(ring);
    }
    if (!c->stream_sets[slot].built()) { int rc = alloc_input_set(c, &c->stream_sets[slot], true); if (rc) return rc; }
    return DAVO_OK;
}

// windows b0.. of a batch's planes
Inputs from_window(const davo_ctx* c, const Inputs& in, int b0) {
    const PlaneBytes nb = plane_bytes(c);
    auto at = [b0](const void* q, size_t bytes) -> const void* { return q ? static_cast<const uint8_t*>(q) + bytes * b0 : nullptr; };
    return Inputs{at(in.img, nb.img), at(in.flow, nb.flow), at(in.seg, nb.seg), at(in.depth, nb.depth)};
}

// Host -> device, on stream s: windows [b0, b0 + nb) of the caller's arrays into the same windows of a staging set.  Only what the path
// reads crosses PCIe: flow planes 0,1 (davo.py:978-982); the label maps; for the depth sources all three depth planes (the target's
// depth enters every frame's descriptor, davo.py:1109).  sources_only_seg: unless the variant reads the target frame's label map too
// (-segmask_all-static, the with-target class-table sources), only the two source frames' maps go (davo.py:998-1004, 1408-1412), in
// batches of four windows and more.
// One pair selected (sel, params.h): only what that pair reads is copied, each plane to its usual place - of every strip row the
// byte range of (tgt, selected source), the source's flow plane, its label map (and the target's where the variant attends it),
// for the depth sources the target's and the source's depth plane.  The regions skipped keep whatever they held; no kernel of a
// one-pair batch reads them.  At 128x416: 319,488 + 425,984 + 212,992 = 958,464 B per window instead of 1,757,184.
int stage_inputs(davo_ctx* c, const InputSet& set, const Inputs& host, int b0, int nb, bool sources_only_seg, int sel, hipStream_t s) {
    const PlaneBytes n = plane_bytes(c);
    const Inputs src = from_window(c, host, b0);
    auto dst = [b0](const DevMem<void>& q, size_t bytes) { return static_cast<uint8_t*>(q.get()) + bytes * b0; };
    if (sel != PAIRS_BOTH) {
        const int src1 = sel == PAIRS_SRC1;
        auto copy2d = [&](uint8_t* d, const void* h, size_t pitch, size_t off, size_t width, size_t rows) {
            return hipMemcpy2DAsync(d + off, pitch, static_cast<const uint8_t*>(h) + off, pitch, width, rows, hipMemcpyHostToDevice, s);
        };
        const size_t row = (size_t)c->W * 9, third = row / 3;       // strip row: src0 | tgt | src1 (data_loader.py:537-557)
        HIP_TRY(c, copy2d(dst(set.img, n.img), src.img, row, src1 ? third : 0, 2 * third, (size_t)nb * c->H));
        HIP_TRY(c, copy2d(dst(set.flow, n.flow), src.flow, n.flow, src1 ? n.flow / 4 : 0, n.flow / 4, nb));
        // planes in file order src0, tgt, src1 (davo.py:991-1004): with the target, two neighbouring planes
        const size_t plane = n.seg / 3;
        if (att_tgt_attended(c->v.att_source)) HIP_TRY(c, copy2d(dst(set.seg, n.seg), src.seg, n.seg, src1 ? plane : 0, 2 * plane, nb));
        else HIP_TRY(c, copy2d(dst(set.seg, n.seg), src.seg, n.seg, src1 ? 2 * plane : 0, plane, nb));
        // depth sources: the target's plane and the source's; the depth-split attention reads the source frame's plane alone
        const size_t dplane = n.depth / 3;                     // (float32 whatever the label format)
        if (src.depth && c->v.att_source == ATT_DEPTH_SPLIT) HIP_TRY(c, copy2d(dst(set.depth, n.depth), src.depth, n.depth, src1 ? 2 * dplane : 0, dplane, nb));
        else if (src.depth) HIP_TRY(c, copy2d(dst(set.depth, n.depth), src.depth, n.depth, src1 ? dplane : 0, 2 * dplane, nb));
        return DAVO_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(dst(set.img, n.img), src.img, n.img * nb, hipMemcpyHostToDevice, s));
    if (nb == 1) HIP_TRY(c, hipMemcpyAsync(dst(set.flow, n.flow), src.flow, n.flow / 2, hipMemcpyHostToDevice, s));
    else HIP_TRY(c, hipMemcpy2DAsync(dst(set.flow, n.flow), n.flow, src.flow, n.flow, n.flow / 2, nb, hipMemcpyHostToDevice, s));
    if (!sources_only_seg || att_tgt_attended(c->v.att_source) || nb < 4) HIP_TRY(c, hipMemcpyAsync(dst(set.seg, n.seg), src.seg, n.seg * nb, hipMemcpyHostToDevice, s));
    else
        for (int plane = 0; plane < 3; plane += 2)
            HIP_TRY(c, hipMemcpy2DAsync(dst(set.seg, n.seg) + plane * (n.seg / 3), n.seg, (const uint8_t*)src.seg + plane * (n.seg / 3), n.seg,
                                        n.seg / 3, nb, hipMemcpyHostToDevice, s));
    if (src.depth) HIP_TRY(c, hipMemcpyAsync(dst(set.depth, n.depth), src.depth, n.depth * nb, hipMemcpyHostToDevice, s));
    return DAVO_OK;
}

// ---- frame layout (window_gather.h; include/davo_hip.h "Frame sequences") ---------------------------------------
// bytes of one frame of each plane kind (flow2: of one window)
PlaneBytes frame_bytes(const davo_ctx* c) {
    const PlaneBytes n = plane_bytes(c);
    return PlaneBytes{n.img / 3, n.flow / 2, n.seg / 3, n.depth / 3};
}
// the depth argument of a `_frames' entry point: in the signature, NULL where the variant reads none
int resolve_frames_depth(davo_ctx* c, const char* fn, const void** depth) {
    if (!needs_depth(c)) { *depth = nullptr; return DAVO_OK; }
    if (!*depth) return fail(c, DAVO_ERR_INVALID, "%s: this variant reads depth planes (att_source %d): depth must not be NULL", fn, c->v.att_source);
    return DAVO_OK;
}

int ensure_frame_set(davo_ctx* c, int slot) {
    if (c->frame_sets[slot].built()) return DAVO_OK;
    const PlaneBytes f = frame_bytes(c);
    const size_t n = (size_t)c->max_batch + 2;
    FrameSet s;
    HIP_TRY(c, dev_alloc(&s.img, f.img * n));
    HIP_TRY(c, dev_alloc(&s.seg, f.seg * n));
    if (needs_depth(c)) HIP_TRY(c, dev_alloc(&s.depth, f.depth * n));
    c->frame_sets[slot] = std::move(s);
    return DAVO_OK;
}

// frames copied so far of each plane kind by the sub-batches of one call (a frame crosses the link once per call)
struct FrameCursor { int img = 0, seg = 0, depth = 0; };

// Host -> device, on stream s, for windows [b0, b0 + nb) of a frame-layout call: the frames frame_plan says they read and no
// earlier sub-batch of the call has brought (*cur) into the slot's frame buffer, frame f to place f; the flow planes of the
// selection straight into planes 0, 1 of the same windows of the staging set, as stage_inputs puts them.
int stage_frames(davo_ctx* c, const FrameSet& fs, const InputSet& set, const FrameInputs& host, int b0, int nb, int sel, FrameCursor* cur, hipStream_t s) {
    const PlaneBytes f = frame_bytes(c), n = plane_bytes(c);
    const FramePlan p = frame_plan(nb, sel, c->v.att_source);
    auto copy = [&](const DevMem<void>& d, const void* h, size_t per, const int r[2], int* done) -> int {
        const int lo = std::max(b0 + r[0], *done), hi = b0 + r[1];
        if (hi > lo) HIP_TRY(c, hipMemcpyAsync(static_cast<uint8_t*>(d.get()) + per * lo, static_cast<const uint8_t*>(h) + per * lo, per * (hi - lo), hipMemcpyHostToDevice, s));
        *done = std::max(*done, hi);
        return DAVO_OK;
    };
    { int rc = copy(fs.img, host.frames, f.img, p.img, &cur->img); if (rc) return rc; }
    { int rc = copy(fs.seg, host.seg, f.seg, p.seg, &cur->seg); if (rc) return rc; }
    if (host.depth) { int rc = copy(fs.depth, host.depth, f.depth, p.depth, &cur->depth); if (rc) return rc; }
    const size_t plane = n.flow / 4, off = plane * p.flow[0], width = plane * (p.flow[1] - p.flow[0]);
    uint8_t* const d = static_cast<uint8_t*>(set.flow.get()) + n.flow * b0 + off;
    const uint8_t* const h = static_cast<const uint8_t*>(host.flow2) + f.flow * b0 + off;
    if (nb == 1) HIP_TRY(c, hipMemcpyAsync(d, h, width, hipMemcpyHostToDevice, s));
    else HIP_TRY(c, hipMemcpy2DAsync(d, n.flow, h, f.flow, width, nb, hipMemcpyHostToDevice, s));
    return DAVO_OK;
}

// window_gather on stream s: windows [b0, b0 + nb) of `set' from frames [b0, b0 + nb + 2) of `fr' (device pointers, frame 0 of the
// call); fr.flow2 null: the flow is in the set already
int gather_windows(davo_ctx* c, const InputSet& set, const FrameInputs& fr, int b0, int nb, int sel, hipStream_t s) {
    const PlaneBytes f = frame_bytes(c), n = plane_bytes(c);
    const FramePlan p = frame_plan(nb, sel, c->v.att_source);
    auto src = [b0](const void* q, size_t per) { return q ? static_cast<const uint8_t*>(q) + per * b0 : nullptr; };
    auto dst = [b0](const DevMem<void>& q, size_t per) { return q ? static_cast<uint8_t*>(q.get()) + per * b0 : nullptr; };
    const GatherArgs a{src(fr.frames, f.img), src(fr.seg, f.seg), src(fr.depth, f.depth), src(fr.flow2, f.flow),
                       dst(set.img, n.img), dst(set.seg, n.seg), dst(set.depth, n.depth), dst(set.flow, n.flow),
                       c->H, c->W, sel, p.seg_tgt, p.depth_tgt};
    ProfScope ps(c, s, "window_gather");
    HIP_TRY(c, launch_window_gather(a, nb, c->label_fmt, s));
    return DAVO_OK;
}

// the oldest undelivered batch: verdict (and re-issue) first, then its poses go to the caller's array
int deliver_front(davo_ctx* c) {
    const StreamJob j = c->jobs.front();
    c->jobs.pop_front();
    while (j.ticketed && c->book.pending(j.seq)) {
        const int rc = judge_front(c);
        if (rc == DAVO_ERR_RANGE && !c->opt_auto_range) c->book.defer(rc, c->err);      // reported by the next davo_synchronize; the poses are delivered as they are
        else if (rc) return rc;
    }
    const PoseRing::Entry& e = c->pose_ring->e[j.pr];           // (a job exists, so the ring does)
    HIP_TRY(c, hipEventSynchronize(e.pose_done.get()));
    memcpy(j.pose_out, e.host.get(), (size_t)j.B * 12 * sizeof(float));
    return DAVO_OK;
}

// every stream the context runs work on is idle: the slots' (and the caller's), the host path's copy stream, the guard's read stream
void drain_own_streams(davo_ctx* c) {
    (void)sync_all_slots(c);
    if (c->host) (void)hipStreamSynchronize(c->host->copy_stream.get());
    if (c->ring) (void)hipStreamSynchronize(c->ring->read_stream.get());
}

int deliver_all(davo_ctx* c) {
    while (!c->jobs.empty()) { const int rc = deliver_front(c); if (rc) { c->jobs.clear(); return rc; } }
    return DAVO_OK;
}

}  // namespace

// the body of davo_submit / davo_submit_depth (depth_form) and of davo_submit_frames (frames: img, flow, seg, depth_in are the frame
// layout's frames, flow2, seg, depth)
static int submit_entry(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth_in, float* pose_out,
                        int hold, bool depth_form, bool frames = false) {
    if (!c) return DAVO_ERR_INVALID;
    if (!img || !flow || !seg || !pose_out) return fail(c, DAVO_ERR_INVALID, "null host pointer");
    const void* depth = depth_in;
    { int rc = frames ? resolve_frames_depth(c, "davo_submit_frames", &depth) : resolve_depth(c, "davo_submit", depth_form, &depth); if (rc) return rc; }
    if (B < 1 || B > c->max_batch) return fail(c, DAVO_ERR_INVALID, "batch %d outside [1,%d]", B, c->max_batch);
    if (hold < 0) return fail(c, DAVO_ERR_INVALID, "hold must be >= 0");
    c->inputs_seen = true;
    HIP_TRY(c, hipSetDevice(c->device));
    // deliver what has finished (never blocks), and make room in the pose ring (blocks on the oldest batch only when the ring is full)
    while (!c->jobs.empty() && ((int)c->jobs.size() >= STREAM_POSES || hipEventQuery(c->pose_ring->e[c->jobs.front().pr].pose_done.get()) == hipSuccess)) {
        const int rc = deliver_front(c);
        if (rc) return rc;
    }
    const bool ticketed = c->impl == 0 && c->precision == 1;
    if (ticketed) { int rc = ticket_reserve(c); if (rc) return rc; }          // may judge - and re-issue - an older batch: before the slot rotation
    const int slot = c->next_slot, pr = (int)(c->n_submitted % STREAM_POSES);
    { int rc = ensure_stream_state(c, slot); if (rc) return rc; }
    if (frames) { int rc = ensure_frame_set(c, slot); if (rc) return rc; }
    Run run = make_run(c, slot);
    c->next_slot = (c->next_slot + 1) % c->inflight;
    hipStream_t s = run.stream;
    // H2D on the slot's stream, in order behind the forward that last read this staging set
    const InputSet& set = c->stream_sets[slot];
    PoseRing::Entry& e = c->pose_ring->e[pr];
    if (frames) {      // the frames into the slot's frame buffer (behind the gather that last read it), the flow into the set
        FrameCursor cur;
        { int rc = stage_frames(c, c->frame_sets[slot], set, FrameInputs{img, flow, seg, depth}, 0, B, c->pairs, &cur, s); if (rc) return rc; }
    } else { int rc = stage_inputs(c, set, Inputs{img, flow, seg, depth}, 0, B, true, c->pairs, s); if (rc) return rc; }
    // the caller keeps a batch's inputs unchanged for `hold` more submits.  With hold >= STREAM_POSES the pose ring already implies it
    // (a batch is delivered - so its copies are long done - before the eighth submit after it returns): no event then
    const bool track_copy = hold < STREAM_POSES;
    if (track_copy) HIP_TRY(c, hipEventRecord(e.copied.get(), s));
    if (frames) {      // the windows, from the device's copy of the frames: the staging set is an ordinary window batch from here on
        const FrameSet& fs = c->frame_sets[slot];
        int rc = gather_windows(c, set, FrameInputs{fs.img.get(), nullptr, fs.seg.get(), fs.depth.get()}, 0, B, c->pairs, s);
        if (rc) return rc;
    }

    Ticket t{};
    if (ticketed) { int rc = ticket_begin(c, &run, B, set.view(), &t, true); if (rc) return rc; }
    c->book.note_issue();             // (no pose span: a pose ring entry is not reused before its batch has been delivered)
    RunResult res;
    int rc = forward_device(c, run, B, set.view(), e.dev.get(), &res);
    if (ticketed) rc = ticket_end(c, rc, res, t, e.dev.get(), e.host.get());
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(e.host.get(), e.dev.get(), (size_t)B * 12 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(e.pose_done.get(), s));
    c->jobs.push_back(StreamJob{B, pose_out, pr, ticketed && res.h3, t.seq});      // (the weight guard's float32 batches get no ticket)
    e.copy_tracked = track_copy;
    ++c->n_submitted;
    if (track_copy && (unsigned long long)hold < c->n_submitted) {
        const int q = (int)((c->n_submitted - 1 - hold) % STREAM_POSES);
        if (c->pose_ring->e[q].copy_tracked) HIP_TRY(c, hipEventSynchronize(c->pose_ring->e[q].copied.get()));
        // (a batch submitted with hold >= 8 recorded no event: it has been delivered by now if it is 8 or more submits back, and a
        // caller that lowers `hold` from one call to the next keeps the larger promise for the batches it made it for)
    }
    return DAVO_OK;
}

int davo_submit(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, float* pose_out, int hold) {
    return submit_entry(c, B, img, flow, seg, nullptr, pose_out, hold, false);
}

int davo_submit_depth(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth, float* pose_out, int hold) {
    return submit_entry(c, B, img, flow, seg, depth, pose_out, hold, true);
}

int davo_submit_frames(davo_ctx* c, int N, const uint8_t* frames, const float* flow2, const float* seg, const float* depth, float* pose_out, int hold) {
    return submit_entry(c, N, frames, flow2, seg, depth, pose_out, hold, true, true);
}

int davo_wait(davo_ctx* c, int leave_pending) {
    if (!c) return DAVO_ERR_INVALID;
    if (leave_pending < 0) return fail(c, DAVO_ERR_INVALID, "leave_pending must be >= 0");
    HIP_TRY(c, hipSetDevice(c->device));
    while ((int)c->jobs.size() > leave_pending) { const int rc = deliver_front(c); if (rc) return rc; }
    return DAVO_OK;
}

int davo_pending(davo_ctx* c) { return c ? (int)c->jobs.size() : DAVO_ERR_INVALID; }

// ---- feature export: davo_set_feature_export / davo_forward_features ----------------------------------------------
// What DAVO.inference(sess, mode='feature') fetches beside the poses (davo.py:1553-1569; generate_feature_map.py:183-260 is its
// reader): everything is computed from what a forward leaves on the device - the class tables (d_tab), the staged inputs and cnv6
// in the storage form the forward ran in - by the two kernels of feature_export.h, into one workspace block of the context, and
// copied to the caller's arrays piece by piece.  The block holds fx_cap windows of every export tensor: the largest sub-batch
// davo_forward issues under the host_chunk of the moment the export was switched on; a larger run of windows (a re-issued batch,
// a host_chunk raised since) goes out in pieces of fx_cap.  With the export off nothing here is allocated or launched.
namespace {

struct FxLayout { size_t rot, trans, masked, image, attention, att_19, total; };      // float offsets into d_fx for `cap' windows
FxLayout fx_layout(const davo_ctx* c, int cap) {
    const size_t HW = (size_t)c->H * c->W, n = (size_t)cap, c6 = (size_t)c->v.cnv6_out;
    FxLayout l{};
    l.rot = 0;
    l.trans = l.rot + n * HW * c6;
    l.masked = l.trans + n * HW * c6;
    l.image = l.masked + n * HW * 9;
    l.attention = l.image + n * HW * 9;
    l.att_19 = l.attention + n * HW * 3;              // last: the only section that is no multiple of 16 bytes
    l.total = l.att_19 + n * 3 * NCLS;
    return l;
}

bool fx_wanted(const davo_feature_out* o) {
    return o && (o->att_19 || o->attention || o->masked_image || o->image || o->feat_rot || o->feat_trans);
}

// Windows [w0, w0 + nw) of the last forward - `in' are that forward's device inputs, window 0 - go to windows
// [b0, b0 + nw) of the caller's arrays of B windows.  Reads d_tab, the inputs and d_act[5] as that forward left them, in the
// precision it ran (last_precision) and under the storage scale it stored cnv6 with.  Returns with the copies done.
int export_features(davo_ctx* c, const Inputs& in, int w0, int nw, int b0, int B, const davo_feature_out& out) {
    if (!c->fx || c->fx->cap < 1) return fail(c, DAVO_ERR_INVALID, "internal: no feature export workspace");
    float* const d_fx = c->fx->d.get();
    const int fx_cap = c->fx->cap;
    if (c->last_pairs != PAIRS_BOTH || w0 < 0 || w0 + nw > c->last_B) return fail(c, DAVO_ERR_INVALID, "internal: feature export of windows the last forward did not run");
    const size_t HW = (size_t)c->H * c->W, c6 = (size_t)c->v.cnv6_out;
    const bool h3 = c->last_precision == 1;
    const FxLayout l = fx_layout(c, fx_cap);
    const Slot& ws = last_workspace(c);
    hipStream_t s = last_stream(c);
    for (int p0 = 0; p0 < nw; p0 += fx_cap) {
        const int np = std::min(fx_cap, nw - p0);
        const Inputs win = from_window(c, in, w0 + p0);
        float* const w_att19 = out.att_19 ? d_fx + l.att_19 : nullptr;
        float* const w_att = out.attention ? d_fx + l.attention : nullptr;
        float* const w_masked = out.masked_image ? d_fx + l.masked : nullptr;
        float* const w_image = out.image ? d_fx + l.image : nullptr;
        float* const w_rot = out.feat_rot ? d_fx + l.rot : nullptr;
        float* const w_trans = out.feat_trans ? d_fx + l.trans : nullptr;
        if (w_att19 || w_att || w_masked || w_image) {
            ProfScope ps(c, s, "feature_maps");
            HIP_TRY(c, launch_feature_maps(static_cast<const uint8_t*>(win.img), win.seg, c->label_fmt,
                                           ws.d_tab.get() + (size_t)(w0 + p0) * 3 * NCLS, c->v, np, c->H, c->W, w_att19, w_att, w_masked, w_image, s,
                                           static_cast<const float*>(win.depth), ws.d_tab_far ? ws.d_tab_far.get() + (size_t)(w0 + p0) * 3 * NCLS : nullptr, c->depth_thr));
        }
        if (w_rot || w_trans) {
            ProfScope ps(c, s, "feature_resize_cnv6");
            HIP_TRY(c, launch_feature_resize_cnv6(h3, ws.d_act[5].get(), w0 + p0, np, c->H2, c->W2, (int)c6, h3 ? ldexpf(1.0f, -c->act_shift[5]) : 1.0f,
                                                  w_rot, w_trans, s));
        }
        // the caller's per-frame arrays are [3][B][...], the workspace's [3][np][...]: one copy per frame
        const size_t first = (size_t)(b0 + p0);
        auto frames = [&](float* host, const float* dev, size_t per_window) -> int {
            if (!host) return DAVO_OK;
            for (int f = 0; f < 3; ++f)
                HIP_TRY(c, hipMemcpyAsync(host + ((size_t)f * B + first) * per_window, dev + (size_t)f * np * per_window,
                                          (size_t)np * per_window * sizeof(float), hipMemcpyDeviceToHost, s));
            return DAVO_OK;
        };
        { int rc = frames(out.att_19, w_att19, NCLS); if (rc) return rc; }
        { int rc = frames(out.attention, w_att, HW); if (rc) return rc; }
        { int rc = frames(out.masked_image, w_masked, HW * 3); if (rc) return rc; }
        { int rc = frames(out.image, w_image, HW * 3); if (rc) return rc; }
        if (w_rot) HIP_TRY(c, hipMemcpyAsync(out.feat_rot + first * HW * c6, w_rot, (size_t)np * HW * c6 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (w_trans) HIP_TRY(c, hipMemcpyAsync(out.feat_trans + first * HW * c6, w_trans, (size_t)np * HW * c6 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));              // the next piece reuses the workspace
    }
    return DAVO_OK;
}

// ---- heat export: davo_set_heat_export / davo_forward_heat ------------------------------------------------------
// What generate_feature_map.py:204-265 keeps of the two feature maps: per head and window the channel sum of the resized cnv6 and
// the block's maximum, reduced where cnv6 lies (feature_export.h: feature_heat_cnv6, feature_resize_plane) into a block of the
// context's own - 2 (H/4 W/4 + H W + 1) floats per window - and copied out piece by piece like the full export.
struct HeatLayout { size_t plane, sum, max, total; };      // float offsets into the block for `cap' windows; head h at + h * cap * per-window
HeatLayout heat_layout(const davo_ctx* c, int cap) {
    const size_t HW = (size_t)c->H * c->W, HW2 = (size_t)c->H2 * c->W2, n = (size_t)cap;
    HeatLayout l{};
    l.plane = 0;                                       // first: written as float4, H W is a multiple of 16
    l.sum = l.plane + 2 * n * HW;
    l.max = l.sum + 2 * n * HW2;
    l.total = l.max + 2 * n;
    return l;
}

bool heat_wanted(const davo_heat_out* o) { return o && (o->rot_sum || o->trans_sum || o->rot_max || o->trans_max); }

// export_features' contract for the heat members: windows [w0, w0 + nw) of the last forward -> windows [b0, b0 + nw) of the caller's
int export_heat(davo_ctx* c, int w0, int nw, int b0, const davo_heat_out& out) {
    if (!c->heat || c->heat->cap < 1) return fail(c, DAVO_ERR_INVALID, "internal: no heat export workspace");
    float* const d = c->heat->d.get();
    const int cap = c->heat->cap;
    if (c->last_pairs != PAIRS_BOTH || w0 < 0 || w0 + nw > c->last_B) return fail(c, DAVO_ERR_INVALID, "internal: heat export of windows the last forward did not run");
    const size_t HW = (size_t)c->H * c->W, HW2 = (size_t)c->H2 * c->W2;
    const bool h3 = c->last_precision == 1;
    const HeatLayout l = heat_layout(c, cap);
    const Slot& ws = last_workspace(c);
    hipStream_t s = last_stream(c);
    const bool rot = out.rot_sum || out.rot_max, trans = out.trans_sum || out.trans_max;
    for (int p0 = 0; p0 < nw; p0 += cap) {
        const int np = std::min(cap, nw - p0);
        float* const w_plane[2] = {out.rot_sum ? d + l.plane : nullptr, out.trans_sum ? d + l.plane + (size_t)cap * HW : nullptr};
        float* const w_sum[2] = {rot ? d + l.sum : nullptr, trans ? d + l.sum + (size_t)cap * HW2 : nullptr};
        float* const w_max[2] = {rot ? d + l.max : nullptr, trans ? d + l.max + cap : nullptr};
        {
            ProfScope ps(c, s, "feature_heat_cnv6");
            HIP_TRY(c, launch_feature_heat(h3, ws.d_act[5].get(), w0 + p0, np, c->H2, c->W2, c->v.cnv6_out, h3 ? ldexpf(1.0f, -c->act_shift[5]) : 1.0f,
                                           w_sum[0], w_sum[1], w_max[0], w_max[1], w_plane[0], w_plane[1], s));
        }
        c->heat->last_np = np;
        const size_t first = (size_t)(b0 + p0);
        if (out.rot_sum) HIP_TRY(c, hipMemcpyAsync(out.rot_sum + first * HW, w_plane[0], (size_t)np * HW * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.trans_sum) HIP_TRY(c, hipMemcpyAsync(out.trans_sum + first * HW, w_plane[1], (size_t)np * HW * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.rot_max) HIP_TRY(c, hipMemcpyAsync(out.rot_max + first, w_max[0], (size_t)np * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.trans_max) HIP_TRY(c, hipMemcpyAsync(out.trans_max + first, w_max[1], (size_t)np * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));              // the next piece reuses the workspace
    }
    return DAVO_OK;
}

// The depth-split flow attention applies two tables per frame, chosen per pixel: there is no 19-row table an `att_19' member could
// hold (the reference sets no att_19s for the branch either, davo.py:1470).  Refused before anything runs; the context stays usable.
int refuse_att_19(davo_ctx* c, const char* fn, const davo_feature_out* out) {
    if (c->v.att_source != ATT_DEPTH_SPLIT || !out || !out->att_19) return DAVO_OK;
    return fail(c, DAVO_ERR_INVALID, "%s: `att_19' does not exist for the depth-split flow attention (att_source %d): every source pixel takes its "
                "weight from the near or the far table by its depth, no single 19-row table was applied - pass att_19 = NULL", fn, ATT_DEPTH_SPLIT);
}

// what a davo_forward_features / davo_forward_heat call wants beside the poses; null = nothing of that kind
struct Exports {
    const davo_feature_out* fx = nullptr;
    const davo_heat_out* heat = nullptr;
    explicit operator bool() const { return fx || heat; }
};
int export_all(davo_ctx* c, const Exports& ex, const Inputs& in, int w0, int nw, int b0, int B) {
    if (ex.fx) { int rc = export_features(c, in, w0, nw, b0, B, *ex.fx); if (rc) return rc; }
    if (ex.heat) { int rc = export_heat(c, w0, nw, b0, *ex.heat); if (rc) return rc; }
    return DAVO_OK;
}

}  // namespace

// the body of davo_forward / davo_forward_depth (depth_form) and of davo_forward_features / davo_forward_heat (ex: the exports wanted)
// ... and of davo_forward_frames (frames: img, flow, seg, depth_in are the frame layout's frames, flow2, seg, depth)
static int forward_entry(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth_in, float* pose_out,
                         bool depth_form, const Exports ex = Exports{}, bool frames = false) {
    if (!c) return DAVO_ERR_INVALID;
    if (!img || !flow || !seg || !pose_out) return fail(c, DAVO_ERR_INVALID, "null host pointer");
    const void* depth = depth_in;
    { int rc = frames ? resolve_frames_depth(c, "davo_forward_frames", &depth) : resolve_depth(c, "davo_forward", depth_form, &depth); if (rc) return rc; }
    if (B < 1 || B > c->max_batch) return fail(c, DAVO_ERR_INVALID, "batch %d outside [1,%d]", B, c->max_batch);
    c->inputs_seen = true;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = deliver_all(c); if (rc) return rc; }          // davo_submit batches still under way: delivered first
    { int rc = sync_all_slots(c); if (rc) return rc; }       // the host path owns the single staging buffer set
    if (!c->host) {
        HostStaging h;
        { int rc = alloc_input_set(c, &h.set, false); if (rc) return rc; }
        HIP_TRY(c, dev_alloc(&h.d_pose, (size_t)c->max_batch * 12));
        HIP_TRY(c, stream_create(&h.copy_stream));
        HIP_TRY(c, pinned_alloc(&h.h_pose, (size_t)c->max_batch * 12, hipHostMallocDefault));
        c->host = std::move(h);
    }
    HostStaging& hs = *c->host;
    if (frames) { int rc = ensure_frame_set(c, 0); if (rc) return rc; }      // slot 0's: every slot is idle
    FrameCursor cur;
    { int rc = judge_all(c); if (rc) return rc; }               // device-path batches issued before this call
    Run run = make_run(c, 0);                                   // slot 0, the base record
    // The base record holds RUNNING maxima like the ring's records (params.h): a record that starts at zero is raised by every wave of
    // every kernel's first round, and at batch 1 - the reference's operating point - those serialised atomics were 200 us of this
    // call's 417.  "Clamped" stays exact per call (the call that pushes a maximum past 65504 fails, and every recovery path zeroes
    // the record); "too small" is judged on what has been stored since the record was last zeroed: by a recovery, a change of scales,
    // and every FRESH_EVERY-th call.
    if (c->book.host_record_due()) {
        HIP_TRY(c, hipMemsetAsync(c->d_range_base.get(), 0, RANGE_WORDS * sizeof(unsigned), run.stream));
    }
    // Sub-batches: the copy of chunk i+1 (copy_stream) overlaps the kernels of chunk i (compute stream).
    // Results do not depend on the split (windows are independent; tests/test_hip_parity.py batch invariance).
    // Only flow planes 0 and 1 are read by the path (davo.py:978-982), so only those cross PCIe.
    const int chunk = (c->host_chunk > 0 && B >= 2 * c->host_chunk) ? c->host_chunk : B;
    const int nchunks = (B + chunk - 1) / chunk;
    while ((int)hs.copy_done.size() < nchunks) {
        EventOwner e;
        HIP_TRY(c, event_create(&e, hipEventDisableTiming));
        hs.copy_done.push_back(std::move(e));
    }
    bool f32_fallback = false;
    RunResult res;
    // Batch 1 is the reference's own operating point (run_inference.sh:44-51), and there this call was 474 us around 129 us of kernels
    // (round 5).  What went: the copy stream and its event for a call that is a single sub-batch (the copies go on the compute
    // stream itself); the read-back of the range record on a stream of its own behind the synchronise (the call's last kernel mirrors
    // the record into page-locked host memory like a ticketed batch's, prologue.h); the pose copy into pageable memory (a page-locked
    // bounce buffer, then memcpy).
    const bool h3_call = c->impl == 0 && c->precision == 1;
    if (h3_call) { int rc = ensure_ring(c, false); if (rc) return rc; }
    unsigned seq = 0;
    for (int i = 0; i < nchunks; ++i) {
        const int b0 = i * chunk, nb = std::min(chunk, B - b0);
        hipStream_t cs = nchunks == 1 ? run.stream : hs.copy_stream.get();
        if (frames) {      // windows [b0, b0 + nb) take frames [b0, b0 + nb + 2): the two it shares with the sub-batch before are on the device already
            const FrameSet& fs = c->frame_sets[0];
            { int rc = stage_frames(c, fs, hs.set, FrameInputs{img, flow, seg, depth}, b0, nb, c->pairs, &cur, cs); if (rc) return rc; }
            { int rc = gather_windows(c, hs.set, FrameInputs{fs.img.get(), nullptr, fs.seg.get(), fs.depth.get()}, b0, nb, c->pairs, cs); if (rc) return rc; }
        } else { int rc = stage_inputs(c, hs.set, Inputs{img, flow, seg, depth}, b0, nb, false, c->pairs, cs); if (rc) return rc; }      // both pairs: the label maps whole
        if (nchunks > 1) {
            HIP_TRY(c, hipEventRecord(hs.copy_done[i].get(), cs));
            HIP_TRY(c, hipStreamWaitEvent(run.stream, hs.copy_done[i].get(), 0));
        }
        if (h3_call && i == nchunks - 1) {       // the call's last kernel mirrors the finished record (all sub-batches) to the host
            seq = c->book.next_seq();
            run.snap.record = c->d_range_base.get(); run.snap.host_mirror = c->ring->h_range_dev; run.snap.seq = seq; run.snap.B = nb; run.snap.se = c->posenn_se;
        }
        int rc = forward_device(c, run, nb, from_window(c, hs.set.view(), b0), hs.d_pose.get() + (size_t)b0 * 12, &res);
        if (rc) return rc;
        f32_fallback |= res.f32_fallback;
        // feature export: the context holds one sub-batch's activations, so every sub-batch but the last is exported before the next
        // one runs; the last one waits for the verdict below
        if (ex && i < nchunks - 1 && (rc = export_all(c, ex, from_window(c, hs.set.view(), b0), 0, nb, b0, B))) return rc;
    }
    const int last_b0 = (nchunks - 1) * chunk;
    auto export_last = [&]() { return !ex ? DAVO_OK : export_all(c, ex, from_window(c, hs.set.view(), last_b0), 0, B - last_b0, last_b0, B); };
    if (f32_fallback) ++c->n_f32_batches;                      // once per call, not per sub-batch
    HIP_TRY(c, hipMemcpyAsync(hs.h_pose.get(), hs.d_pose.get(), (size_t)B * 12 * sizeof(float), hipMemcpyDeviceToHost, run.stream));
    HIP_TRY(c, hipStreamSynchronize(run.stream));
    memcpy(pose_out, hs.h_pose.get(), (size_t)B * 12 * sizeof(float));
    if (!res.h3) return export_last();
    // The call ran f16x3 (res is the last sub-batch's), so that sub-batch carried run.snap - h3_call reads the same impl and precision
    // run does - and its last kernel, pose_from_tiles or range_guard_snapshot (forward.hip), has stored the record and seq in the
    // mirror; the stream is idle, so the wait returns at once
    unsigned raw[RANGE_WORDS];
    int rc = wait_record(c, c->ring->h_range.get(), seq, run.stream, raw);
    if (rc) return rc;
    rc = judge_record(c, raw, c->act_shift);
    if (rc == DAVO_ERR_RANGE && c->opt_auto_range) {
        // the staged copy of the batch is still in HBM: re-issue it whole (recalibrated, or on the float32 kernels); nothing has
        // been issued since, so its pose buffer is its own
        rc = recover_batch(c, Reissue{B, c->pairs, hs.set.view(), hs.d_pose.get(), false, 0});
        if (rc == DAVO_OK) HIP_TRY(c, hipMemcpy(pose_out, hs.d_pose.get(), (size_t)B * 12 * sizeof(float), hipMemcpyDeviceToHost));
        // the re-issue ran the whole batch as one forward and produced the poses returned: every window's exports come from it, in
        // the precision and under the scales it ran with (what the sub-batches exported above is overwritten)
        if (rc == DAVO_OK && ex) rc = export_all(c, ex, hs.set.view(), 0, B, 0, B);
        return rc;
    }
    return rc == DAVO_OK ? export_last() : rc;
}

int davo_forward(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, float* pose_out) {
    return forward_entry(c, B, img, flow, seg, nullptr, pose_out, false);
}

int davo_forward_depth(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth, float* pose_out) {
    return forward_entry(c, B, img, flow, seg, depth, pose_out, true);
}

int davo_forward_frames(davo_ctx* c, int N, const uint8_t* frames, const float* flow2, const float* seg, const float* depth, float* pose_out) {
    return forward_entry(c, N, frames, flow2, seg, depth, pose_out, true, Exports{}, true);
}

int davo_set_feature_export(davo_ctx* c, int on) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = sync_all_slots(c); if (rc) return rc; }
    if (!on) { c->fx.reset(); c->fx_on = false; return DAVO_OK; }
    if (!c->fx) {
        FxBlock fx;
        fx.cap = c->host_chunk > 0 ? std::min(c->max_batch, 2 * c->host_chunk - 1) : c->max_batch;      // davo_forward's largest sub-batch
        HIP_TRY(c, dev_alloc(&fx.d, fx_layout(c, fx.cap).total));
        c->fx = std::move(fx);
    }
    c->fx_on = true;
    return DAVO_OK;
}

int davo_forward_features(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth, float* pose_out,
                          const davo_feature_out* out) {
    if (!c) return DAVO_ERR_INVALID;
    if (!c->fx_on) return fail(c, DAVO_ERR_NOT_READY, "davo_forward_features: the feature export is off - call davo_set_feature_export(ctx, 1) first");
    if (c->pairs != PAIRS_BOTH)
        return fail(c, DAVO_ERR_INVALID, "davo_forward_features runs both pairs of every window, the reference's semantics (davo.py:1456-1457): "
                    "davo_set_pairs(ctx, DAVO_PAIRS_BOTH) first (the selection is %d)", c->pairs);
    { int rc = refuse_att_19(c, "davo_forward_features", out); if (rc) return rc; }
    return forward_entry(c, B, img, flow, seg, depth, pose_out, true, Exports{fx_wanted(out) ? out : nullptr, nullptr});
}

int davo_set_heat_export(davo_ctx* c, int on) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = sync_all_slots(c); if (rc) return rc; }
    if (!on) { c->heat.reset(); return DAVO_OK; }
    if (!c->heat) {
        HeatBlock h;
        h.cap = c->host_chunk > 0 ? std::min(c->max_batch, 2 * c->host_chunk - 1) : c->max_batch;      // davo_forward's largest sub-batch
        HIP_TRY(c, dev_alloc(&h.d, heat_layout(c, h.cap).total));
        c->heat = std::move(h);
    }
    return DAVO_OK;
}

int davo_forward_heat(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth, float* pose_out,
                      const davo_feature_out* out, const davo_heat_out* heat) {
    if (!c) return DAVO_ERR_INVALID;
    const bool want_fx = fx_wanted(out), want_heat = heat_wanted(heat);
    if (want_fx && !c->fx_on) return fail(c, DAVO_ERR_NOT_READY, "davo_forward_heat: a member of `out' is wanted and the feature export is off - call davo_set_feature_export(ctx, 1) first");
    if (want_heat && !c->heat) return fail(c, DAVO_ERR_NOT_READY, "davo_forward_heat: a member of `heat' is wanted and the heat export is off - call davo_set_heat_export(ctx, 1) first");
    if (c->pairs != PAIRS_BOTH)
        return fail(c, DAVO_ERR_INVALID, "davo_forward_heat runs both pairs of every window, the reference's semantics (davo.py:1456-1457): "
                    "davo_set_pairs(ctx, DAVO_PAIRS_BOTH) first (the selection is %d)", c->pairs);
    { int rc = refuse_att_19(c, "davo_forward_heat", out); if (rc) return rc; }
    return forward_entry(c, B, img, flow, seg, depth, pose_out, true, Exports{want_fx ? out : nullptr, want_heat ? heat : nullptr});
}

int davo_range_stats(davo_ctx* c, long long* recalibrations, long long* f32_batches, long long* reissued) {
    if (!c) return DAVO_ERR_INVALID;
    if (recalibrations) *recalibrations = c->n_recalibrations;
    if (f32_batches) *f32_batches = c->n_f32_batches;
    if (reissued) *reissued = c->n_reissued;
    return DAVO_OK;
}

int davo_activation_range(davo_ctx* c, float* max_abs, int* shifts, int reset) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = judge_all(c); if (rc && rc != DAVO_ERR_RANGE) return rc; }      // every issued batch's record is in range_seen now
    for (int i = 0; i < 6; ++i) {
        if (max_abs) max_abs[i] = c->range_seen[i];
        if (shifts) shifts[i] = c->act_shift[i];
    }
    if (reset) for (int i = 0; i < 6; ++i) c->range_seen[i] = 0.f;
    return DAVO_OK;
}

const char* davo_range_report(const davo_ctx* c) { return c ? c->range_report.c_str() : ""; }

int davo_set_activation_shifts(davo_ctx* c, const int* shifts) {
    if (!c) return DAVO_ERR_INVALID;
    { int rc = judge_all(c); if (rc) return rc; }             // batches issued under the old scales get their verdict first
    { int rc = freeze_pending_and_reset_ring(c); if (rc) return rc; }      // maxima stored under the old scales say nothing about the new
    c->book.host_record_stale();                                             // ... the host path's record included: its next call starts afresh
    for (int i = 0; i < 6; ++i) {
        const int s = shifts ? shifts[i] : 0;
        if (s < -60 || s > 60) return fail(c, DAVO_ERR_INVALID, "activation shift %d outside [-60,60]", s);
        c->act_shift[i] = s;
    }
    return DAVO_OK;
}

int davo_reset_range_state(davo_ctx* c) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    // batches issued so far get their verdict - and their recovery - under the scales they ran with; with "auto_range" 0 a failed
    // verdict is this call's result, after the state has been reset all the same
    const int verdict = judge_all(c);
    if (verdict && verdict != DAVO_ERR_RANGE) return verdict;
    const std::string verdict_err = c->err;
    { int rc = freeze_pending_and_reset_ring(c); if (rc) return rc; }       // no ticket is pending: this zeroes the ring's records
    { int rc = zero_now(c, c->d_range_base.get(), RANGE_WORDS * sizeof(unsigned)); if (rc) return rc; }
    for (int i = 0; i < 7; ++i) c->act_shift[i] = 0;
    for (int i = 0; i < 6; ++i) c->range_seen[i] = 0.f;
    c->book.reset();                                                         // the counters' and the cursor's initial values, no deferred verdict
    c->range_report.clear();
    if (verdict) { c->err = verdict_err; return verdict; }
    return DAVO_OK;
}

// the body of davo_calibrate / davo_calibrate_depth (depth_form)
static int calibrate_entry(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg, const void* d_depth, int* shifts_out,
                           bool depth_form) {
    if (!c) return DAVO_ERR_INVALID;
    if (B < 1 || B > c->max_batch) return fail(c, DAVO_ERR_INVALID, "batch %d outside [1,%d]", B, c->max_batch);
    if (!d_img || !d_flow || !d_seg) return fail(c, DAVO_ERR_INVALID, "null device pointer");
    { int rc = resolve_depth(c, "davo_calibrate", depth_form, &d_depth); if (rc) return rc; }
    c->inputs_seen = true;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = judge_all(c); if (rc) return rc; }             // batches issued under the old scales get their verdict first
    { int rc = freeze_pending_and_reset_ring(c); if (rc) return rc; }
    DevMem<float> d_pose;
    HIP_TRY(c, dev_alloc(&d_pose, (size_t)B * 12));
    const int rc = calibrate_on(c, B, Inputs{d_img, d_flow, d_seg, d_depth}, d_pose.get(), PAIRS_BOTH);
    if (rc == DAVO_OK && shifts_out) for (int i = 0; i < 6; ++i) shifts_out[i] = c->act_shift[i];
    return rc;
}

int davo_calibrate(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg, int* shifts_out) {
    return calibrate_entry(c, B, d_img, d_flow, d_seg, nullptr, shifts_out, false);
}

int davo_calibrate_depth(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg, const void* d_depth, int* shifts_out) {
    return calibrate_entry(c, B, d_img, d_flow, d_seg, d_depth, shifts_out, true);
}

const char* davo_last_error(const davo_ctx* c) { return c ? c->err.c_str() : "null context"; }

// Every member of the context frees what it owns (owned.h), in any order: the streams are drained first so that nothing on the
// device still reads what goes.
void davo_destroy(davo_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    drain_own_streams(c);
    comm_release(c);
    delete c;
}

int davo_host_alloc(int device, size_t bytes, void** out) {
    if (!out || bytes == 0) return DAVO_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return DAVO_ERR_HIP;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? DAVO_OK : DAVO_ERR_HIP;
}
int davo_host_free(void* p) { return hipHostFree(p) == hipSuccess ? DAVO_OK : DAVO_ERR_HIP; }
int davo_host_register(int device, void* p, size_t bytes) {
    if (!p || bytes == 0) return DAVO_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return DAVO_ERR_HIP;
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? DAVO_OK : DAVO_ERR_HIP;
}
int davo_host_unregister(void* p) { return hipHostUnregister(p) == hipSuccess ? DAVO_OK : DAVO_ERR_HIP; }

int davo_device_malloc(davo_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMalloc(out, bytes));
    return DAVO_OK;
}
int davo_device_free(davo_ctx* c, void* p) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipFree(p));
    return DAVO_OK;
}
int davo_memcpy_h2d(davo_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, last_stream(c)));
    HIP_TRY(c, hipStreamSynchronize(last_stream(c)));
    return DAVO_OK;
}
int davo_memcpy_d2h(davo_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, last_stream(c)));
    HIP_TRY(c, hipStreamSynchronize(last_stream(c)));
    return DAVO_OK;
}
int davo_synchronize(davo_ctx* c) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    // f16x3: the batches davo_forward_device issued since the last synchronize are judged here (the asynchronous
    // entry point cannot know its own result).  A failed verdict re-issues that batch (recover_batch); with "auto_range" 0
    // it is returned as DAVO_ERR_RANGE = some layer left the fp16-pair storage range.  davo_submit batches are delivered first.
    { int rc = deliver_all(c); if (rc) return rc; }
    return judge_all(c);
}
int davo_set_stream(davo_ctx* c, void* hip_stream) {
    if (!c) return DAVO_ERR_INVALID;
    if (hip_stream && c->inflight > 1) return fail(c, DAVO_ERR_INVALID, "a caller-owned stream needs davo_set_inflight(ctx, 1)");
    // batches issued on the stream the context is about to leave get their verdict (and any re-issue) while that stream is still
    // the one the context synchronises; the caller may destroy it afterwards
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = deliver_all(c); if (rc) return rc; }
    { int rc = judge_all(c); if (rc) return rc; }
    c->user_stream = static_cast<hipStream_t>(hip_stream);
    c->last_slot = 0;
    return DAVO_OK;
}

int davo_profile_enable(davo_ctx* c, int on) {
    if (!c) return DAVO_ERR_INVALID;
    if (!on && c->prof) { int rc = prof_collect(c); if (rc) return rc; }
    c->prof = on != 0;
    c->prof_dominant_only = on == 2;
    return DAVO_OK;
}
int davo_profile_reset(davo_ctx* c) {
    if (!c) return DAVO_ERR_INVALID;
    int rc = prof_collect(c);
    if (rc) return rc;
    for (auto& pe : c->prof_entries) { pe.launches = 0; pe.total_ms = 0.0; pe.dur_ms.clear(); pe.period_ms.clear(); }
    return DAVO_OK;
}
int davo_profile_samples(davo_ctx* c, const char* name, int which, float* out, int cap) {
    if (!c || !name || which < 0 || which > 1 || cap < 0 || (cap > 0 && !out)) return DAVO_ERR_INVALID;
    int rc = prof_collect(c);
    if (rc) return rc;
    for (const auto& pe : c->prof_entries)
        if (pe.name == name) {
            const std::vector<float>& v = which == 0 ? pe.dur_ms : pe.period_ms;
            const int n = (int)std::min(v.size(), (size_t)cap);
            for (int i = 0; i < n; ++i) out[i] = v[i];
            return (int)v.size();
        }
    return 0;
}
int davo_profile_entry(davo_ctx* c, int i, char* name, int name_len, int* launches, double* total_ms) {
    if (!c) return DAVO_ERR_INVALID;
    int rc = prof_collect(c);
    if (rc) return rc;
    if (i < 0 || i >= (int)c->prof_entries.size()) return DAVO_ERR_INVALID;
    const ProfEntry& pe = c->prof_entries[i];
    if (name && name_len > 0) { strncpy(name, pe.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    if (launches) *launches = pe.launches;
    if (total_ms) *total_ms = pe.total_ms;
    return DAVO_OK;
}

int davo_last_plan(davo_ctx* c, int layer, int launch, int* mtiles, int* bn) {
    if (!c || layer < 0 || layer > 6 || launch < 0 || launch > 1) return DAVO_ERR_INVALID;
    const int v = c->last_plan[layer][launch];
    if (mtiles) *mtiles = v / 1000;
    if (bn) *bn = v % 1000;
    return DAVO_OK;
}

int davo_last_split(davo_ctx* c, int layer, int* parts) {
    if (!c || layer < 0 || layer > 6) return DAVO_ERR_INVALID;
    if (parts) *parts = c->last_split[layer];
    return DAVO_OK;
}

// (Re)create the slots' streams.  With cu_partition on, slot i of n gets the CUs [i*32/n, (i+1)*32/n) of EVERY XCD
// (hipExtStreamCreateWithCUMask; mask bit b = CU b/8 of XCD b%8, and a mask must leave no XCD empty — probed with
// tools/exp/cumask_probe.hip), so batches in different slots run side by side on disjoint CUs and the write bursts of
// one overlap the matrix phases of the other.  The launch planner then sizes rounds for 256/n CUs.
static int rebuild_slot_streams(davo_ctx* c, int n) {
    for (int i = 0; i < (int)c->slots.size(); ++i) {
        Slot& s = c->slots[i];
        StreamOwner fresh;                                                     // the slot keeps a live stream whatever fails here
        if (c->cu_partition && n > 1 && i < n && c->dev_cus == 256) {          // the mask layout below is the 8 XCD x 32 CU part's
            uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const int lo = i * 32 / n, hi = (i + 1) * 32 / n;                 // CU indices inside an XCD
            for (int b = 0; b < 256; ++b)
                if (b / 8 >= lo && b / 8 < hi) mask[b / 32] |= 1u << (b % 32);
            HIP_TRY(c, stream_create(&fresh, 8, mask));
        } else {
            HIP_TRY(c, stream_create(&fresh));
        }
        std::swap(s.stream, fresh);
        if (fresh) HIP_TRY(c, hipStreamDestroy(fresh.release()));              // the old one: a failure is reported
    }
    c->ncu = (c->cu_partition && n > 1 && c->dev_cus == 256) ? 256 / n : c->dev_cus;
    c->last_slot = 0;
    return DAVO_OK;
}

int davo_set_inflight(davo_ctx* c, int n) {
    if (!c || n < 1 || n > MAX_INFLIGHT) return fail(c, DAVO_ERR_INVALID, "inflight must be 1..4");
    if (n > 1 && c->user_stream) return fail(c, DAVO_ERR_INVALID, "in-flight slots use the context's own streams: clear davo_set_stream first");
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = deliver_all(c); if (rc) return rc; }
    { int rc = sync_all_slots(c); if (rc) return rc; }
    while ((int)c->slots.size() < n) { int rc = add_slot(c); if (rc) return rc; }      // a slot that could not be built whole is not appended
    c->inflight = n;
    c->next_slot = 0;
    if (c->cu_partition || c->ncu != c->dev_cus) { int rc = rebuild_slot_streams(c, n); if (rc) return rc; }
    return DAVO_OK;
}

int davo_set_option(davo_ctx* c, const char* key, int value) {
    if (!c || !key) return DAVO_ERR_INVALID;
    const std::string k = key;
    if (k == "fuse_pose") c->opt_fuse_pose = value != 0;
    else if (k == "fuse_pack") c->opt_fuse_pack = value < 0 ? -1 : (value != 0);
    else if (k == "share_taps") c->opt_share_taps = value != 0;
    else if (k == "merge_rem") c->opt_merge_rem = value != 0;
    else if (k == "merge_cnv4") c->opt_merge_cnv4 = value != 0;
    else if (k == "tile_208x128") c->opt_tile_208x128 = value != 0;
    else if (k == "merge_order") c->opt_merge_order = value < 0 ? -1 : (value > 2 ? 0 : value);
    else if (k == "skip_order") c->opt_skip_order = value < 0 ? 0 : (value > 2 ? 2 : value);
    else if (k == "pad_classes") {
        // 0 off | 1 the default layers | 8 + mask: the layers of the mask (1 cnv4, 2 cnv5, 4 cnv6)
        if (value == 0 || value == 1) c->opt_pad_classes = value ? PAD_CLASS_LAYERS : 0;
        else if (value >= 8 && value <= 15) c->opt_pad_classes = value & 7;
        else return fail(c, DAVO_ERR_INVALID, "pad_classes must be 0, 1 or 8 + a layer mask (8..15), got %d", value);
    }
    else if (k == "patch_cnv2") c->opt_patch_cnv2 = value != 0;
    else if (k == "patch_cnv3") c->opt_patch_cnv3 = value != 0;
    else if (k == "fold_tails") c->opt_fold_tails = value < 0 ? -1 : (value > 2 ? 1 : value);
    else if (k == "deep_ring") c->opt_deep_ring = value != 0;
    else if (k == "wave128") c->opt_wave128 = value < 0 ? 0 : (value > 3 ? 3 : value);      // 3: cnv4 on conv_igemm_h3w128 whatever the round count (test hook)
    else if (k == "split_k") c->opt_split_k = value != 0;
    else if (k == "fold_fixup") c->opt_fold_fixup = value != 0;
    else if (k == "f32_n16") c->opt_f32_n16 = value != 0;
    else if (k == "f32_n256") c->opt_f32_n256 = value != 0;
    else if (k == "merge_rem_f32") c->opt_merge_rem_f32 = value < 0 ? 0 : (value > 2 ? 2 : value);
    else if (k == "patch_f32") c->opt_patch_f32 = value != 0;
    else if (k == "auto_range") { int rc = judge_all(c); if (rc) return rc; c->opt_auto_range = value != 0; }
    else if (k == "stable_inputs") { int rc = judge_all(c); if (rc) return rc; c->opt_stable_inputs = value != 0; }
    else if (k == "force_tile") {
        // test hook: every f16x3 layer the tile fits runs as ONE launch of that tile shape (plan.h tile ids; -1 = planner)
        if (value < -1 || value >= NUM_TILES) return fail(c, DAVO_ERR_INVALID, "force_tile must be -1..%d", NUM_TILES - 1);
        for (auto& L : c->L) L.tile_h = (value >= 0 && L.cout >= tile_shape(value).bn) ? value : -1;
    }
    else if (k == "cu_partition") {
        if (c->user_stream) return fail(c, DAVO_ERR_INVALID, "cu_partition uses the context's own streams: clear davo_set_stream first");
        HIP_TRY(c, hipSetDevice(c->device));
        { int rc = sync_all_slots(c); if (rc) return rc; }
        c->cu_partition = value != 0;
        int rc = rebuild_slot_streams(c, c->inflight);
        if (rc) return rc;
    }
    else if (k == "profile_stride") { if (value < 1) return fail(c, DAVO_ERR_INVALID, "profile_stride must be >= 1"); c->prof_stride = value; c->prof_tick = 0; }
    else if (k == "host_chunk") { if (value < 0) return fail(c, DAVO_ERR_INVALID, "host_chunk must be >= 0"); c->host_chunk = value; }
    else return fail(c, DAVO_ERR_INVALID, "unknown option `%s'", key);
    return DAVO_OK;
}

int davo_set_precision(davo_ctx* c, int precision) {
    if (!c || (precision != 0 && precision != 1)) return fail(c, DAVO_ERR_INVALID, "precision must be 0 (f32) or 1 (f16x3)");
    c->precision = precision;
    return DAVO_OK;
}

int davo_set_pairs(davo_ctx* c, int pairs) {
    if (!c) return DAVO_ERR_INVALID;
    if (pairs != DAVO_PAIRS_SRC0 && pairs != DAVO_PAIRS_SRC1 && pairs != DAVO_PAIRS_BOTH)
        return fail(c, DAVO_ERR_INVALID, "pairs must be DAVO_PAIRS_SRC0 (1), DAVO_PAIRS_SRC1 (2) or DAVO_PAIRS_BOTH (3), got %d", pairs);
    c->pairs = pairs;              // batches in flight and their re-issues keep theirs (Ticket::pairs)
    return DAVO_OK;
}

int davo_get_pairs(const davo_ctx* c) { return c ? c->pairs : DAVO_ERR_INVALID; }

int davo_set_impl(davo_ctx* c, int impl) {
    if (!c || (impl != 0 && impl != 1)) return fail(c, DAVO_ERR_INVALID, "impl must be 0 (mfma) or 1 (direct)");
    c->impl = impl;
    return DAVO_OK;
}

int davo_debug_read(davo_ctx* c, const char* tensor, float* host_out, size_t n_floats) {
    if (!c || !tensor || !host_out) return DAVO_ERR_INVALID;
    if (c->last_B < 1) return fail(c, DAVO_ERR_NOT_READY, "no forward has run yet");
    const size_t NB = (size_t)pairs_per_window(c->last_pairs) * c->last_B;      // pair images of the last forward
    const float* src = nullptr;
    size_t n = 0;
    const std::string t = tensor;
    const Slot& ws = last_workspace(c);
    if (t == "att_table") { src = ws.d_tab.get(); n = (size_t)c->last_B * 3 * NCLS; }       // att_source 13: the near MLP's tables
    else if (t == "att_table_far") {                         // ... and the far MLP's; the target's rows are ones in both
        if (!ws.d_tab_far) return fail(c, DAVO_ERR_INVALID, "`att_table_far' exists for the depth-split flow attention only (att_source %d, got %d)", ATT_DEPTH_SPLIT, c->v.att_source);
        src = ws.d_tab_far.get(); n = (size_t)c->last_B * 3 * NCLS;
    }
    else if (t == "cnv5_se_scale" || t == "cnv5_se") {      // feature attention (posenn_se.h): [2B][2][256] s_r | s_r s_t; [2B][H2][W2][512] rotation | translation input of cnv6
        if (!c->posenn_se || !ws.se) return fail(c, DAVO_ERR_NOT_READY, "`%s' exists in the feature-attention variant only (davo_set_posenn_se)", tensor);
        if (t == "cnv5_se") { src = ws.se->d_se.get(); n = NB * c->H2 * c->W2 * 512; }
        else { src = ws.se->d_se_scale.get(); n = NB * 2 * 256; }
    }
    else if (t == "packed") {
        if (!c->packed_valid) {          // fused path: materialise the packed tensor on demand from the last inputs
            HIP_TRY(c, launch_mask_pack(16, static_cast<const uint8_t*>(c->last_in.img), static_cast<const float*>(c->last_in.flow),
                                        c->last_in.seg, c->label_fmt, ws.d_tab.get(), c->v, c->last_B, c->H, c->W, ws.d_packed.get(), c->last_pairs, last_stream(c)));
            c->packed_valid = true;
        }
        src = ws.d_packed.get(); n = NB * c->H * c->W * c->packed_ld;
    }
    else {
        const char* names[7] = {"cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6", "cnv7"};
        for (int i = 0; i < 7; ++i)
            if (t == names[i]) { src = ws.d_act[i].get(); n = NB * c->act_floats_per_img[i]; }
    }
    if (t == "heat_sum") {            // the heat export's channel sums of the piece it exported last: [2][np][H2][W2], rotation | translation
        if (!c->heat || c->heat->last_np < 1) return fail(c, DAVO_ERR_NOT_READY, "`heat_sum' exists after a davo_forward_heat with the heat export on");
        const size_t per = (size_t)c->H2 * c->W2, np = (size_t)c->heat->last_np;
        if (n_floats != 2 * np * per) return fail(c, DAVO_ERR_INVALID, "`heat_sum' holds %zu floats, caller asked for %zu", 2 * np * per, n_floats);
        const size_t at = (size_t)2 * c->heat->cap * c->H * c->W;
        for (int h = 0; h < 2; ++h) {
            int rc = davo_memcpy_d2h(c, host_out + h * np * per, c->heat->d.get() + at + (size_t)h * c->heat->cap * per, np * per * sizeof(float));
            if (rc) return rc;
        }
        return DAVO_OK;
    }
    if (t == "pose_tiles") {          // the fused pose head's per-tile partial sums of the last batch (slot 0's region)
        if (c->cnv7_valid || !c->d_pose_tiles.get()) return fail(c, DAVO_ERR_NOT_READY, "the pose head did not run fused");
#ifndef DAVO_POSE_DEBUG
        if (n_floats > c->pose_tiles_floats) return fail(c, DAVO_ERR_INVALID, "pose_tiles holds %zu floats", c->pose_tiles_floats);
#endif
        return davo_memcpy_d2h(c, host_out, c->d_pose_tiles.get(), n_floats * sizeof(float));
    }
    if (t == "cnv7" && !c->cnv7_valid)
        return fail(c, DAVO_ERR_NOT_READY, "cnv7 was not materialised: the pose head ran fused (davo_set_option(ctx, \"fuse_pose\", 0))");
    if (!src) return fail(c, DAVO_ERR_INVALID, "unknown tensor `%s'", tensor);
    if (n != n_floats) return fail(c, DAVO_ERR_INVALID, "`%s' holds %zu floats, caller asked for %zu", tensor, n, n_floats);
    int rc = davo_memcpy_d2h(c, host_out, src, n * sizeof(float));
    if (rc) return rc;
    const bool split = c->last_precision == 1 && t != "att_table" && t != "att_table_far" && t != "cnv7" && t != "cnv5_se_scale";
    if (split) {       // split-fp16 blocked -> plain float32 NHWC
        int ch = 8;
        const char* names[6] = {"cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6"};
        for (int i = 0; i < 6; ++i) if (t == names[i]) ch = c->act_ch[i];
        if (t == "cnv5_se") ch = 512;                // cnv5's storage ...
        const int cb = ch < 32 ? ch : 32;
        int shift = t == "cnv5_se" ? c->act_shift[4] : 0;       // ... and its scale
        for (int i = 0; i < 6; ++i) if (t == names[i]) shift = c->act_shift[i];
        std::vector<float> tmp(ch);
        const size_t npix = n / ch;
        for (size_t px = 0; px < npix; ++px) {
            const _Float16* raw = reinterpret_cast<const _Float16*>(host_out + px * ch);
            for (int k = 0; k < ch; ++k) {
                const _Float16* blk = raw + (size_t)(k / cb) * cb * 2;
                tmp[k] = ldexpf((float)blk[k % cb] + (float)blk[cb + k % cb], -shift);
            }
            memcpy(host_out + px * ch, tmp.data(), ch * sizeof(float));
        }
    }
    return DAVO_OK;
}

int davo_tile_filter_rows(int m0, int m1, int Hout, int Wout, int Hin, int stride, int pad_t, int rate,
                          int* ky0, int* nky, int nblocks, int* chunk_map) {
    if (!ky0 || !nky || Hout < 1 || Wout < 1 || Hin < 1 || stride < 1 || rate < 1 || m0 < 0 || nblocks < 0) return DAVO_ERR_INVALID;
    const FilterRows fr = valid_filter_rows(m0, m1, Hout, Wout, Hin, stride, pad_t, rate);
    *ky0 = fr.ky0;
    *nky = fr.nky;
    if (chunk_map)
        for (int v = 0; v < 3 * fr.nky * nblocks; ++v) chunk_map[v] = h3_real_chunk(v, fr.ky0, fr.nky);
    return DAVO_OK;
}

int davo_pad_class_tables(int NB, int Hout, int Wout, int Hin, int Win, int pad_t, int pad_l, int rate, int* row_pixel, unsigned short* tile_taps) {
    if (!row_pixel || !tile_taps || NB < 1 || Hout < 1 || Wout < 1 || Hin < 1 || Win < 1 || rate < 1 || (long)NB * Hout * Wout > 0x7fffff00L) return DAVO_ERR_INVALID;
    std::vector<int32_t> rows;
    std::vector<uint16_t> taps;
    const bool sorted = pad_class_tables(NB, Hout, Wout, Hin, Win, pad_t, pad_l, rate, BM, &rows, &taps);
    memcpy(row_pixel, rows.data(), rows.size() * sizeof(int32_t));
    memcpy(tile_taps, taps.data(), taps.size() * sizeof(uint16_t));
    return sorted ? 1 : 0;
}

int davo_pad_class_tile_order(const unsigned short* tile_taps, int mtile0, int mtiles, int ntiles_n, int* order) {
    if (!tile_taps || !order || mtile0 < 0 || mtiles < 1 || ntiles_n < 1) return DAVO_ERR_INVALID;
    std::vector<int> o;
    pad_class_tile_order(tile_taps, mtile0, mtiles, ntiles_n, &o);
    memcpy(order, o.data(), o.size() * sizeof(int));
    return DAVO_OK;
}

int davo_plan_layer_f32(int mtiles, int npad, int groups, int ncu, int* mtile0, int* launch_mtiles, int* tile_bn) {
    if (mtiles < 1 || npad < 32 || npad % 32 || groups < 1 || ncu < 1 || !mtile0 || !launch_mtiles || !tile_bn) return DAVO_ERR_INVALID;
    const std::vector<Launch> plan = plan_layer(mtiles, npad, groups, ncu);
    if (plan.empty() || plan.size() > 2) return DAVO_ERR_INVALID;
    for (size_t i = 0; i < plan.size(); ++i) { mtile0[i] = plan[i].mtile0; launch_mtiles[i] = plan[i].mtiles; tile_bn[i] = plan[i].BN; }
    return (int)plan.size();
}

int davo_plan_layer(int M, int npad, int groups, int* rows, int* tile_bm, int* tile_bn) {
    if (M < 1 || npad < 32 || npad % 32 || groups < 1 || !rows || !tile_bm || !tile_bn) return DAVO_ERR_INVALID;
    const std::vector<LaunchH> plan = plan_layer_h3(M, npad, groups, -1, npad == 256);
    if (plan.empty() || plan.size() > 2) return DAVO_ERR_INVALID;
    for (size_t i = 0; i < plan.size(); ++i) {
        const TileShape ts = tile_shape(plan[i].tile);
        rows[i] = plan[i].rows; tile_bm[i] = ts.bm; tile_bn[i] = ts.bn;
    }
    return (int)plan.size();
}

int davo_conv2d_same(int device, const float* x, int N, int H, int W, int Cin, const float* w, int k, int Cout,
                     const float* bias, int stride, int rate, int relu, int precision, float* y, char* err, int err_len) {
    auto bad = [&](const char* m, int code) {
        if (err && err_len > 0) { strncpy(err, m, err_len - 1); err[err_len - 1] = 0; }
        return code;
    };
    const int cl = ilog2_exact(Cin);
    if (!x || !w || !bias || !y) return bad("null pointer", DAVO_ERR_INVALID);
    if (cl < 2) return bad("Cin must be a power of two >= 4", DAVO_ERR_INVALID);
    if (precision == 1 && cl < 3) return bad("f16x3 needs Cin >= 8", DAVO_ERR_INVALID);
    if (!(k == 1 || k == 3 || k == 5 || k == 7) || !(stride == 1 || stride == 2) || rate < 1)
        return bad("k in {1,3,5,7}, stride in {1,2}, rate >= 1", DAVO_ERR_INVALID);
    if (hipSetDevice(device) != hipSuccess) return bad("hipSetDevice failed", DAVO_ERR_HIP);
    ConvLayer L;
    init_layer(L, "conv", k, stride, rate, Cin, Cout, 1);
    int Ho, Wo, pt, pl;
    same_pad(H, k, stride, rate, &Ho, &pt);
    same_pad(W, k, stride, rate, &Wo, &pl);
    const size_t nx = (size_t)N * H * W * Cin, ny = (size_t)N * Ho * Wo * Cout;
    std::vector<float> bp(precision == 1 ? L.npad_h : L.npad, 0.f);
    memcpy(bp.data(), bias, Cout * sizeof(float));
    std::vector<float> wp;
    std::vector<_Float16> wph, xh;
    const void *hx = x, *hw = nullptr;
    size_t wbytes = 0;
    if (precision == 1) {
        wph.assign((size_t)L.npad_h * L.nchunks_h * 64, (_Float16)0.0f);
        L.wscale = weight_prescale(w, (size_t)k * k * Cin * Cout);
        pack_conv_weights_h3(w, k, Cin, Cout, nullptr, Cin, L.cb_log2, L.tpc_log2, L.cpb, L.nchunks_h, L.wscale, wph.data());
        hw = wph.data(); wbytes = wph.size() * sizeof(_Float16);
        const int cb = 1 << L.cb_log2;                       // float32 NHWC -> split-fp16 blocked
        xh.resize(nx * 2);
        for (size_t px = 0; px < nx / Cin; ++px)
            for (int ch = 0; ch < Cin; ++ch) {
                _Float16* blk = xh.data() + px * Cin * 2 + (size_t)(ch / cb) * cb * 2;
                split_f16(x[px * Cin + ch], blk + ch % cb, blk + cb + ch % cb);
            }
        hx = xh.data();
    } else {
        wp.assign((size_t)L.npad * L.kpad, 0.f);
        pack_conv_weights(w, k, Cin, Cout, nullptr, Cin, L.npad, L.kpad, wp.data());
        hw = wp.data(); wbytes = wp.size() * sizeof(float);
    }
    DevMem<void> dx, dw, db, dy, dz;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    chk(dev_alloc(&dx, nx * 4)); chk(dev_alloc(&dw, wbytes));
    chk(dev_alloc(&db, bp.size() * 4)); chk(dev_alloc(&dy, ny * 4));
    chk(dev_alloc(&dz, 256));
    if (e == hipSuccess) {
        chk(hipMemset(dz.get(), 0, 256));
        chk(hipMemcpy(dx.get(), hx, nx * 4, hipMemcpyHostToDevice));
        chk(hipMemcpy(dw.get(), hw, wbytes, hipMemcpyHostToDevice));
        chk(hipMemcpy(db.get(), bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
        if (precision == 1) {
            const int tile = Cout <= 32 ? TILE_128x32 : Cout <= 64 ? TILE_256x64 : Cout <= 128 ? TILE_256x128 : TILE_128x256;
            const TileShape ts = tile_shape(tile);
            ConvParamsH p{};
            p.x = static_cast<const uint8_t*>(dx.get()); p.w = static_cast<const uint8_t*>(dw.get());
            p.bias = static_cast<const float*>(db.get()); p.y = static_cast<uint8_t*>(dy.get());
            p.zeros = static_cast<const uint8_t*>(dz.get());
            p.Hin = H; p.Win = W; p.Hout = Ho; p.Wout = Wo; p.x_pix_bytes = (long)Cin * 4; p.x_pix_log2 = -1;
            p.cb_log2 = L.cb_log2; p.tpc_log2 = L.tpc_log2; p.cpb = L.cpb; p.nchunks = L.nchunks_h;
            p.w_row_bytes = (long)L.nchunks_h * 128; p.y_mode = 0; p.y_ld = Cout; p.Cout = Cout;
            p.pad_t = pt; p.pad_l = pl; p.rate = rate; p.M = N * Ho * Wo; p.ntaps = k * k;
            p.Mtot = p.M; p.xs = 0; p.ntiles_n = L.npad_h / ts.bn; p.relu = relu; p.out_scale = 1.0f / L.wscale; p.bias_scale = L.wscale; p.range = nullptr;
            dim3 grid((p.M + ts.bm - 1) / ts.bm * p.ntiles_n, 1);
            const hipError_t le = launch_h3_generic(k, stride, tile, p, grid, nullptr);
            chk(le);
        } else {
            ConvParams p{};
            p.x = static_cast<const float*>(dx.get()); p.w = static_cast<const float*>(dw.get());
            p.bias = static_cast<const float*>(db.get()); p.y = static_cast<float*>(dy.get());
            p.zeros = static_cast<const float*>(dz.get());
            p.Hin = H; p.Win = W; p.Hout = Ho; p.Wout = Wo; p.cin_log2 = cl; p.x_ld = Cin; p.y_ld = Cout;
            p.Cout = Cout; p.pad_t = pt; p.pad_l = pl; p.rate = rate; p.M = N * Ho * Wo;
            p.nchunks = L.nchunks; p.Kpad = L.kpad; p.ntaps = k * k; p.ntiles_n = L.npad / L.BN; p.relu = relu;
            dim3 grid((p.M + BM - 1) / BM * p.ntiles_n, 1);
            chk(launch_conv(k, stride, L.BN, p, grid, nullptr));
        }
        chk(hipDeviceSynchronize());
        chk(hipMemcpy(y, dy.get(), ny * 4, hipMemcpyDeviceToHost));
    }
    if (e != hipSuccess) return bad(hipGetErrorString(e), DAVO_ERR_HIP);
    return DAVO_OK;
}

}  // extern "C"
