// entry.hip — the entry points of libdavo_hip.so that take a batch (include/davo_hip.h): the device-buffer, the streaming and the
// host-buffer forward family, each in the window and the frame layout, with davo_wait / davo_pending and the delivery of streamed
// batches.  A wrapper describes the batch as the caller handed it (ctx.h: Batch), one check serves them all, and a Stager brings
// the batch's windows into the staging set the forward reads, whatever the layout.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "ctx.h"
#include "launch.h"
#include "pool_plan.h"
#include "window_gather.h"
#include "window_mirror.h"

using namespace davo;

// ---- the forward entry points ----------------------------------------------------------------------------
// The f16x3 batches they issue are judged by the range guard (range_guard.hip, reached through ctx.h; bookkeeping: c->book).

// The one argument check, in this order: null pointers, the depth argument, the batch range, hold, alignment.
// Depth: a variant that reads depth planes (att_source 11, 12, 13) must be called with the planes - the window layout through the
// `_depth' form, the frame layout with a non-null `depth'; every other variant reads no depth: a pointer (or null) is accepted and ignored.
int davo::check_batch(davo_ctx* c, Batch* b, int B, bool out_given, int hold) {
    if (!c) return DAVO_ERR_INVALID;
    if (!b->win.img || !b->win.flow || !b->win.seg || !out_given) return fail(c, DAVO_ERR_INVALID, "null %s pointer", b->on_device ? "device" : "host");
    if (!needs_depth(c)) b->win.depth = nullptr;
    else if (b->layout == Layout::Frames) {
        if (!b->fr.depth) return fail(c, DAVO_ERR_INVALID, "%s: this variant reads depth planes (att_source %d): depth must not be NULL", b->fn, c->v.att_source);
    } else {
        if (!b->depth_param) return fail(c, DAVO_ERR_INVALID, "%s: this variant reads depth planes (att_source %d): call %s_depth", b->fn, c->v.att_source, b->fn);
        if (!b->win.depth) return fail(c, DAVO_ERR_INVALID, "%s_depth: null depth pointer", b->fn);
    }
    if (B < 1 || B > c->max_batch) return fail(c, DAVO_ERR_INVALID, "batch %d outside [1,%d]", B, c->max_batch);
    if (hold < 0) return fail(c, DAVO_ERR_INVALID, "hold must be >= 0");
    // a binary16 flow is read in 16-byte units of four pixels (input_decode.h: flow_fetch4): on the device its base is 16-byte aligned
    if (c->fmt.flow == FLOW_F16 && b->on_device && b->layout == Layout::Windows && ((uintptr_t)b->win.flow & 15))
        return fail(c, DAVO_ERR_INVALID, "%s: a binary16 device flow buffer (davo_set_flow_format) must be 16-byte aligned", b->fn);
    // flip on: window_mirror reads the caller's device buffers in 16-byte units
    if (c->flip && b->on_device && b->layout == Layout::Windows && (((uintptr_t)b->win.img | (uintptr_t)b->win.flow | (uintptr_t)b->win.seg | (uintptr_t)b->win.depth) & 15))
        return fail(c, DAVO_ERR_INVALID, "%s: with davo_set_flip on, device input buffers must be 16-byte aligned", b->fn);
    if (b->layout == Layout::Frames && b->on_device && (((uintptr_t)b->fr.frames | (uintptr_t)b->fr.flow2 | (uintptr_t)b->fr.seg | (uintptr_t)b->fr.depth) & 15))
        return fail(c, DAVO_ERR_INVALID, "%s: device input buffers must be 16-byte aligned", b->fn);
    return DAVO_OK;
}

// windows b0.. of a batch's planes
Inputs davo::from_window(const davo_ctx* c, const Inputs& in, int b0) {
    const PlaneBytes nb = plane_bytes(c);
    auto at = [b0](const void* q, size_t bytes) -> const void* { return q ? static_cast<const uint8_t*>(q) + bytes * b0 : nullptr; };
    return Inputs{at(in.img, nb.img), at(in.flow, nb.flow), at(in.seg, nb.seg), at(in.depth, nb.depth)};
}

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
        const size_t dplane = n.depth / 3;                     // (the depth format's, whatever the label format)
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
// call); fr.flow2 null: the flow is in the set already.  flip: the same launch stores every row mirrored (window_mirror.h)
int gather_windows(davo_ctx* c, const InputSet& set, const FrameInputs& fr, int b0, int nb, int sel, bool flip, hipStream_t s) {
    const PlaneBytes f = frame_bytes(c), n = plane_bytes(c);
    const FramePlan p = frame_plan(nb, sel, c->v.att_source);
    auto src = [b0](const void* q, size_t per) { return q ? static_cast<const uint8_t*>(q) + per * b0 : nullptr; };
    auto dst = [b0](const DevMem<void>& q, size_t per) { return q ? static_cast<uint8_t*>(q.get()) + per * b0 : nullptr; };
    const GatherArgs a{src(fr.frames, f.img), src(fr.seg, f.seg), src(fr.depth, f.depth), src(fr.flow2, f.flow),
                       dst(set.img, n.img), dst(set.seg, n.seg), dst(set.depth, n.depth), dst(set.flow, n.flow),
                       c->H, c->W, sel, p.seg_tgt, p.depth_tgt};
    ProfScope ps(c, s, "window_gather");
    // (the mirrored form leaves out the target's label map where the variant does not attend it: no kernel reads it)
    if (flip) HIP_TRY(c, launch_window_mirror(a, nb, true, c->fmt, s));
    else HIP_TRY(c, launch_window_gather(a, nb, c->fmt, s));
    return DAVO_OK;
}

// window_mirror on stream s: windows [b0, b0 + nb) of `set' mirrored left-right - in place (from null: the copies of stage_inputs
// are there), or from the caller's device buffers `from' (window 0 of the batch), which are only read.  seg_tgt: the target's label
// map is among what the set holds and the batch reads.  Only what the selection and the variant read is touched.
int mirror_windows(davo_ctx* c, const InputSet& set, const Inputs* from, int b0, int nb, int sel, bool seg_tgt, hipStream_t s) {
    const Inputs dst = from_window(c, set.view(), b0), src = from ? from_window(c, *from, b0) : dst;
    auto rd = [](const void* q) { return static_cast<const uint8_t*>(q); };
    auto wr = [](const void* q) { return const_cast<uint8_t*>(static_cast<const uint8_t*>(q)); };
    const GatherArgs a{rd(src.img), rd(src.seg), dst.depth ? rd(src.depth) : nullptr, rd(src.flow), wr(dst.img), wr(dst.seg), wr(dst.depth), wr(dst.flow),
                       c->H, c->W, sel, seg_tgt, att_desc_depth(c->v.att_source)};
    ProfScope ps(c, s, "window_mirror");
    HIP_TRY(c, launch_window_mirror(a, nb, false, c->fmt, s));
    return DAVO_OK;
}

// ---- tracking: the session's ring (ctx.h: TrackState; window_gather.h: track_step) ---------------------------------------------
// Both steps of a push run on the stream given, its slot's.  The ring is shared by every slot, so what stream order does for a
// slot's own staging set events do here, stream to stream and never through the host: the upload waits for the three gathers
// that read its place, the gather for the two uploads of the earlier places it reads.  An event recorded on the stream that
// would wait for it is skipped (stream order holds it already): with one slot in flight no wait is issued at all.

// The frames of push t into place t mod R - from the host, or from the caller's device buffers - and, from the host, the flow
// planes of the selection straight into planes 0, 1 of windows [0, lanes) of `set', as stage_frames puts them (set null: a push
// that issues no window)
int track_upload(davo_ctx* c, const FrameInputs& fr, bool on_device, long long t, const InputSet* set, int sel, hipStream_t s) {
    TrackState& tr = *c->track;
    const TrackStep st = track_step(t, tr.R);
    const PlaneBytes f = frame_bytes(c), n = plane_bytes(c);
    for (const long long u : st.upload_after) {
        if (u < 0) continue;
        const TrackState::Place& q = tr.places[u % tr.R];
        if (q.ga && q.ga_stream != s) HIP_TRY(c, hipStreamWaitEvent(s, q.gathered.get(), 0));
    }
    const size_t S = (size_t)tr.lanes, at = (size_t)st.upload_place * S;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    auto put = [&](const DevMem<void>& d, const void* src, size_t per) {
        return hipMemcpyAsync(static_cast<uint8_t*>(d.get()) + per * at, src, per * S, kind, s);
    };
    HIP_TRY(c, put(tr.img, fr.frames, f.img));
    HIP_TRY(c, put(tr.seg, fr.seg, f.seg));
    if (tr.depth) HIP_TRY(c, put(tr.depth, fr.depth, f.depth));
    if (set && !on_device) {
        const FramePlan p = frame_plan(1, sel, c->v.att_source);
        const size_t plane = n.flow / 4, off = plane * p.flow[0], width = plane * (p.flow[1] - p.flow[0]);
        uint8_t* const d = static_cast<uint8_t*>(set->flow.get()) + off;
        const uint8_t* const h = static_cast<const uint8_t*>(fr.flow2) + off;
        if (S == 1) HIP_TRY(c, hipMemcpyAsync(d, h, width, hipMemcpyHostToDevice, s));
        else HIP_TRY(c, hipMemcpy2DAsync(d, n.flow, h, f.flow, width, S, hipMemcpyHostToDevice, s));
    }
    TrackState::Place& me = tr.places[st.upload_place];
    HIP_TRY(c, hipEventRecord(me.uploaded.get(), s));
    me.up = true; me.up_stream = s;
    return DAVO_OK;
}

// The windows of push t (t >= 2) out of the ring into windows [0, lanes) of `set': the gather launch of the frame layout with the
// ring's places as frame bases.  d_flow2: the caller's device flow [lanes][2] (null: the flow is in the set already)
int track_gather(davo_ctx* c, const InputSet& set, const void* d_flow2, long long t, int sel, bool flip, hipStream_t s) {
    TrackState& tr = *c->track;
    const TrackStep st = track_step(t, tr.R);
    for (const long long u : st.gather_after) {
        const TrackState::Place& q = tr.places[u % tr.R];
        if (q.up && q.up_stream != s) HIP_TRY(c, hipStreamWaitEvent(s, q.uploaded.get(), 0));
    }
    const FramePlan p = frame_plan(tr.lanes, sel, c->v.att_source);
    auto rd = [](const void* q) { return static_cast<const uint8_t*>(q); };
    auto wr = [](const DevMem<void>& q) { return static_cast<uint8_t*>(q.get()); };
    const GatherArgs a{rd(tr.img.get()), rd(tr.seg.get()), rd(tr.depth.get()), rd(d_flow2), wr(set.img), wr(set.seg), wr(set.depth), wr(set.flow),
                       c->H, c->W, sel, p.seg_tgt, p.depth_tgt,
                       st.place[0] * tr.lanes, st.place[1] * tr.lanes, st.place[2] * tr.lanes, 1};
    {
        ProfScope ps(c, s, "window_gather");
        if (flip) HIP_TRY(c, launch_window_mirror(a, tr.lanes, true, c->fmt, s));
        else HIP_TRY(c, launch_window_gather(a, tr.lanes, c->fmt, s));
    }
    TrackState::Place& me = tr.places[st.upload_place];
    HIP_TRY(c, hipEventRecord(me.gathered.get(), s));
    me.ga = true; me.ga_stream = s;
    return DAVO_OK;
}

// ---- the stager: a batch's windows into the staging set its forward reads, a run of windows [b0, b0 + nb) at a time ----------
// Two steps per run, both on the stream given: stage_upload brings what the windows read onto the device, stage_windows makes the
// set hold them as windows.  Window layout: stage_inputs, then nothing.  Frame layout: stage_frames into the slot's frame buffer
// (a frame crosses the link once per call: cur), then gather_windows from it - or, for a batch on the device, nothing and then
// gather_windows from the caller's buffers.  A window batch on the device has no set: its forward reads the caller's buffers.
// With flip on (davo_set_flip, as it stood when the batch was issued) the second step also mirrors: the frame layout inside its one
// gather launch; the window layout from the host with one window_mirror launch on the set, in place; a window batch on the device
// gets the slot's staging set after all and is mirrored into it from the caller's buffers, which are never written.
enum class Path { Device, Submit, Forward };
// a push of a tracking session (davo_track_push[_device]): a frame-layout batch of `lanes' windows whose frames pass through the
// session's ring.  t: its index (frames pushed before it); sel: the pair selection the policy gives it
struct Push { long long t; int sel; };
struct Stager {
    davo_ctx* c;
    Batch b;
    bool flip = false;                         // the context's setting when the batch was issued
    int sel = PAIRS_BOTH;                      // the batch's pair selection: the context's, or the push's
    const Push* push = nullptr;                // a push: b.fr holds ONE new frame per lane, the windows come out of the ring
    const InputSet* set = nullptr;             // the path's staging set of the slot (null: none, see above)
    const FrameSet* fs = nullptr;              // frame layout from the host: the slot's frame buffer
    bool sources_only_seg = false;             // stage_inputs': davo_submit's batches
    FrameCursor cur;
    Inputs inputs() const { return set ? set->view() : b.win; }      // what the forward reads
};

// The stager of batch b in `slot'; builds what the path keeps per slot at its first use, each group whole: davo_forward's staging
// (slot 0), davo_submit's pose ring and the slot's staging set, the slot's frame buffer for frames that come from the host.
int acquire_stager(davo_ctx* c, const Batch& b, Path path, int slot, Stager* st, const Push* push = nullptr) {
    *st = Stager{c, b, c->flip, push ? push->sel : c->pairs, push};
    if (path == Path::Forward) {
        if (!c->host) {
            HostStaging h;
            { int rc = alloc_input_set(c, &h.set, false); if (rc) return rc; }
            HIP_TRY(c, dev_alloc(&h.d_pose, (size_t)c->max_batch * 12));
            HIP_TRY(c, stream_create(&h.copy_stream));
            HIP_TRY(c, pinned_alloc(&h.h_pose, (size_t)c->max_batch * 12, hipHostMallocDefault));
            c->host = std::move(h);
        }
        st->set = &c->host->set;
    } else if (path == Path::Submit) {
        { int rc = ensure_stream_state(c, slot); if (rc) return rc; }
        st->set = &c->stream_sets[slot];
        st->sources_only_seg = true;
    } else if (b.layout == Layout::Frames || st->flip) {
        if (!c->stream_sets[slot].built()) { int rc = alloc_input_set(c, &c->stream_sets[slot], true); if (rc) return rc; }
        st->set = &c->stream_sets[slot];
    }
    if (b.layout == Layout::Frames && !b.on_device && !push) {      // (a push's frames go into the session's ring)
        { int rc = ensure_frame_set(c, slot); if (rc) return rc; }
        st->fs = &c->frame_sets[slot];
    }
    return DAVO_OK;
}

int stage_upload(Stager* st, int b0, int nb, hipStream_t s) {
    if (st->push) return track_upload(st->c, st->b.fr, st->b.on_device, st->push->t, st->set, st->sel, s);
    if (st->b.on_device) return DAVO_OK;
    if (st->fs) return stage_frames(st->c, *st->fs, *st->set, st->b.fr, b0, nb, st->sel, &st->cur, s);
    return stage_inputs(st->c, *st->set, st->b.win, b0, nb, st->sources_only_seg, st->sel, s);
}

int stage_windows(Stager* st, int b0, int nb, hipStream_t s) {
    davo_ctx* c = st->c;
    if (st->b.layout != Layout::Frames) {
        if (!st->flip) return DAVO_OK;
        // the target's label map is read only where the variant attends it (davo_submit's staging does not even copy it otherwise)
        return mirror_windows(c, *st->set, st->b.on_device ? &st->b.win : nullptr, b0, nb, st->sel, att_tgt_attended(c->v.att_source), s);
    }
    if (st->push) return track_gather(c, *st->set, st->b.on_device ? st->b.fr.flow2 : nullptr, st->push->t, st->sel, st->flip, s);
    const FrameInputs dev = st->fs ? FrameInputs{st->fs->img.get(), nullptr, st->fs->seg.get(), st->fs->depth.get()} : st->b.fr;
    return gather_windows(c, *st->set, dev, b0, nb, st->sel, st->flip, s);
}

}  // namespace

// davo_calibrate's batch with flip on: B windows of the caller's device buffers mirrored into slot 0's staging set on its stream
// (every stream is idle); *out = what the calibration passes read
int davo::mirror_device_batch(davo_ctx* c, const Inputs& in, int B, Inputs* out) {
    if (!c->stream_sets[0].built()) { int rc = alloc_input_set(c, &c->stream_sets[0], true); if (rc) return rc; }
    *out = c->stream_sets[0].view();
    return mirror_windows(c, c->stream_sets[0], &in, 0, B, PAIRS_BOTH, att_tgt_attended(c->v.att_source), slot_stream(c, 0));
}

namespace {

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

}  // namespace

// every stream the context runs work on is idle: the slots' (and the caller's), the host path's copy stream, the guard's read stream
void davo::drain_own_streams(davo_ctx* c) {
    (void)sync_all_slots(c);
    if (c->host) (void)hipStreamSynchronize(c->host->copy_stream.get());
    if (c->ring) (void)hipStreamSynchronize(c->ring->read_stream.get());
}

int davo::deliver_all(davo_ctx* c) {
    while (!c->jobs.empty()) { const int rc = deliver_front(c); if (rc) { c->jobs.clear(); return rc; } }
    return DAVO_OK;
}

// the body of davo_forward_device, davo_forward_device_depth and davo_forward_device_frames: b's pointers are device pointers.  A
// frame batch runs on the slot's staging set, gathered from them
static int forward_device_entry(davo_ctx* c, int B, Batch b, void* d_pose, float* elapsed_ms, const Push* push = nullptr) {
    { int rc = check_batch(c, &b, B, d_pose != nullptr); if (rc) return rc; }
    c->inputs_seen = true;
    HIP_TRY(c, hipSetDevice(c->device));
    Stager st;
    { int rc = acquire_stager(c, b, Path::Device, c->next_slot, &st, push); if (rc) return rc; }
    const Inputs in = st.inputs();
    const bool ticketed = c->impl == 0 && c->precision == 1;      // f16x3: the batch gets a record (and a copy of its inputs) of its own
    if (ticketed) { int rc = ticket_reserve(c); if (rc) return rc; }
    // rotate through the in-flight slots: this batch runs on its own stream and workspace
    Run run = make_run(c, c->next_slot);
    run.pairs = st.sel;
    c->next_slot = (c->next_slot + 1) % c->inflight;
    EventOwner e0, e1;
    // the windows into the slot's staging set, in stream order behind the forward that last read it and ahead of the ticket: the
    // caller's buffers are free once this launch has run, and the batch is the library's own from here on (own_inputs below).
    // The timed form brackets the gather too: elapsed_ms is what the layout costs on resident inputs
    if (elapsed_ms && st.set) {
        HIP_TRY(c, event_create(&e0));
        HIP_TRY(c, hipEventRecord(e0.get(), run.stream));
    }
    { int rc = stage_upload(&st, 0, B, run.stream); if (rc) return rc; }       // (a push: its frames into the ring; else nothing, the batch is on the device)
    { int rc = stage_windows(&st, 0, B, run.stream); if (rc) return rc; }
    Ticket t{};
    if (ticketed) { int rc = ticket_begin(c, &run, B, in, &t, st.set != nullptr); if (rc) return rc; }
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

extern "C" {

int davo_forward_device(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg,
                        void* d_pose, float* elapsed_ms) {
    return forward_device_entry(c, B, window_batch("davo_forward_device", true, false, d_img, d_flow, d_seg, nullptr), d_pose, elapsed_ms);
}

int davo_forward_device_depth(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg, const void* d_depth,
                              void* d_pose, float* elapsed_ms) {
    return forward_device_entry(c, B, window_batch("davo_forward_device", true, true, d_img, d_flow, d_seg, d_depth), d_pose, elapsed_ms);
}

int davo_forward_device_frames(davo_ctx* c, int N, const void* d_frames, const void* d_flow2, const void* d_seg, const void* d_depth,
                               void* d_pose, float* elapsed_ms) {
    return forward_device_entry(c, N, frame_batch("davo_forward_device_frames", true, d_frames, d_flow2, d_seg, d_depth), d_pose, elapsed_ms);
}

int davo_frames_plan_fmt2(int H, int W, int N, int pairs, int att_source, int label_fmt, int flow_fmt, int depth_fmt, int* ranges, long long* link_bytes) {
    const InputFormat fmt{label_fmt, flow_fmt, depth_fmt};
    if (H < 1 || W < 1 || N < 1 || (pairs != PAIRS_SRC0 && pairs != PAIRS_SRC1 && pairs != PAIRS_BOTH) || att_source < 0 || att_source > ATT_MAX || !valid(fmt))
        return DAVO_ERR_INVALID;
    const FramePlan p = frame_plan(N, pairs, att_source);
    if (ranges) {
        const int r[8] = {p.img[0], p.img[1], p.seg[0], p.seg[1], p.depth[0], p.depth[1], p.flow[0], p.flow[1]};
        memcpy(ranges, r, sizeof r);
    }
    if (link_bytes) *link_bytes = frame_plan_bytes(p, N, H, W, element_bytes(fmt));
    return DAVO_OK;
}

int davo_frames_plan_fmt(int H, int W, int N, int pairs, int att_source, int label_fmt, int flow_fmt, int* ranges, long long* link_bytes) {
    return davo_frames_plan_fmt2(H, W, N, pairs, att_source, label_fmt, flow_fmt, DEPTH_F32, ranges, link_bytes);
}

int davo_frames_plan(int H, int W, int N, int pairs, int att_source, int label_fmt, int* ranges, long long* link_bytes) {
    // the range this form was published with (tests/test_frames.py pins 14 as refused): the pooled sources go through davo_frames_plan_fmt
    if (att_source > ATT_DEPTH_SPLIT) return DAVO_ERR_INVALID;
    return davo_frames_plan_fmt(H, W, N, pairs, att_source, label_fmt, FLOW_F32, ranges, link_bytes);
}

int davo_pool_plan(int H, int W, int att_source, int* n_cells, int* rects, float* inv_div) {
    if (H < 1 || W < 1 || att_source < 0 || att_source > ATT_MAX || !n_cells) return DAVO_ERR_INVALID;
    const PoolPlan p = pool_plan(H, W, att_source);
    *n_cells = (int)p.cells.size();
    for (size_t i = 0; i < p.cells.size(); ++i) {
        const PoolCell& c = p.cells[i];
        if (rects) { rects[4 * i] = c.y0; rects[4 * i + 1] = c.y1; rects[4 * i + 2] = c.x0; rects[4 * i + 3] = c.x1; }
        if (inv_div) inv_div[i] = c.inv_div;
    }
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

// the body of davo_submit, davo_submit_depth and davo_submit_frames: b's pointers are host pointers
static int submit_entry(davo_ctx* c, int B, Batch b, float* pose_out, int hold, const Push* push = nullptr) {
    { int rc = check_batch(c, &b, B, pose_out != nullptr, hold); if (rc) return rc; }
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
    Stager st;
    { int rc = acquire_stager(c, b, Path::Submit, slot, &st, push); if (rc) return rc; }
    Run run = make_run(c, slot);
    run.pairs = st.sel;
    c->next_slot = (c->next_slot + 1) % c->inflight;
    hipStream_t s = run.stream;
    // H2D on the slot's stream, in order behind the forward that last read this staging set (and, the frame layout, behind the
    // gather that last read the slot's frame buffer)
    const InputSet& set = *st.set;
    PoseRing::Entry& e = c->pose_ring->e[pr];
    { int rc = stage_upload(&st, 0, B, s); if (rc) return rc; }
    // the caller keeps a batch's inputs unchanged for `hold` more submits.  With hold >= STREAM_POSES the pose ring already implies it
    // (a batch is delivered - so its copies are long done - before the eighth submit after it returns): no event then
    const bool track_copy = hold < STREAM_POSES;
    if (track_copy) HIP_TRY(c, hipEventRecord(e.copied.get(), s));
    { int rc = stage_windows(&st, 0, B, s); if (rc) return rc; }      // the staging set is an ordinary window batch from here on

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
    return submit_entry(c, B, window_batch("davo_submit", false, false, img, flow, seg, nullptr), pose_out, hold);
}

int davo_submit_depth(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth, float* pose_out, int hold) {
    return submit_entry(c, B, window_batch("davo_submit", false, true, img, flow, seg, depth), pose_out, hold);
}

int davo_submit_frames(davo_ctx* c, int N, const uint8_t* frames, const float* flow2, const float* seg, const float* depth, float* pose_out, int hold) {
    return submit_entry(c, N, frame_batch("davo_submit_frames", false, frames, flow2, seg, depth), pose_out, hold);
}

int davo_wait(davo_ctx* c, int leave_pending) {
    if (!c) return DAVO_ERR_INVALID;
    if (leave_pending < 0) return fail(c, DAVO_ERR_INVALID, "leave_pending must be >= 0");
    HIP_TRY(c, hipSetDevice(c->device));
    while ((int)c->jobs.size() > leave_pending) { const int rc = deliver_front(c); if (rc) return rc; }
    return DAVO_OK;
}

int davo_pending(davo_ctx* c) { return c ? (int)c->jobs.size() : DAVO_ERR_INVALID; }

// ---- online tracking: davo_track_begin / davo_track_push[_device] / davo_track_end ---------------------------------------------
// A push is a frame-layout batch of `lanes' windows through submit_entry / forward_device_entry above: the same slots, tickets,
// pose ring, delivery and `hold'.  What differs is where its frames come from (the Stager's two steps: track_upload, track_gather)
// and who picks its pair selection (the session's policy).  The range guard's copy of a push is of the staging set: a re-issue
// never reads the ring.

int davo_track_begin(davo_ctx* c, int lanes, int policy) {
    if (!c) return DAVO_ERR_INVALID;
    if (c->track) return fail(c, DAVO_ERR_INVALID, "davo_track_begin: a tracking session is open already: call davo_track_end first");
    if (lanes < 1 || lanes > c->max_batch) return fail(c, DAVO_ERR_INVALID, "davo_track_begin: lanes %d outside [1,%d] (max_batch)", lanes, c->max_batch);
    if (policy != DAVO_TRACK_TRAJECTORY && policy != DAVO_TRACK_AS_SET)
        return fail(c, DAVO_ERR_INVALID, "davo_track_begin: policy must be DAVO_TRACK_TRAJECTORY (0) or DAVO_TRACK_AS_SET (1), got %d", policy);
    if (c->fx_on || c->heat) return fail(c, DAVO_ERR_INVALID, "davo_track_begin: there are no exports under tracking: switch the feature and heat exports off first");
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = deliver_all(c); if (rc) return rc; }
    TrackState tr;
    tr.lanes = lanes; tr.policy = policy; tr.R = track_ring_places(c->inflight);
    const PlaneBytes f = frame_bytes(c);
    const size_t n = (size_t)tr.R * lanes;
    HIP_TRY(c, dev_alloc(&tr.img, f.img * n));
    HIP_TRY(c, dev_alloc(&tr.seg, f.seg * n));
    if (needs_depth(c)) HIP_TRY(c, dev_alloc(&tr.depth, f.depth * n));
    tr.places.resize(tr.R);
    for (TrackState::Place& p : tr.places) {
        HIP_TRY(c, event_create(&p.uploaded, hipEventDisableTiming));
        HIP_TRY(c, event_create(&p.gathered, hipEventDisableTiming));
    }
    c->track = std::move(tr);
    return DAVO_OK;
}

// the selection of the push about to be issued: the three-frame network runs whole windows whatever the policy
static int push_selection(const davo_ctx* c) {
    const TrackState& tr = *c->track;
    if (triplet(c)) return PAIRS_BOTH;
    if (tr.policy == DAVO_TRACK_AS_SET) return c->pairs;
    return tr.pushed == 2 ? PAIRS_BOTH : PAIRS_SRC1;       // the session's first window, then tgt->src1 alone
}

// the body of davo_track_push and davo_track_push_device -> windows issued (0 or lanes) or a negative status
static int track_push_entry(davo_ctx* c, Batch b, void* pose, int hold, float* elapsed_ms) {
    if (!c) return DAVO_ERR_INVALID;
    if (!c->track) return fail(c, DAVO_ERR_INVALID, "%s: no tracking session is open: call davo_track_begin first", b.fn);
    TrackState& tr = *c->track;
    const Push push{tr.pushed, push_selection(c)};
    if (push.t >= 2) {
        const int rc = b.on_device ? forward_device_entry(c, tr.lanes, b, pose, elapsed_ms, &push)
                                   : submit_entry(c, tr.lanes, b, static_cast<float*>(pose), hold, &push);
        if (rc) return rc;
        ++tr.pushed;
        return tr.lanes;
    }
    // fewer than two earlier frames: the frame goes into the ring and nothing is issued (flow2 and the poses are not read: either may be NULL)
    if (!b.fr.flow2) b.fr.flow2 = b.fr.frames;
    { int rc = check_batch(c, &b, tr.lanes, true, hold); if (rc) return rc; }
    c->inputs_seen = true;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = track_upload(c, b.fr, b.on_device, push.t, nullptr, push.sel, slot_stream(c, c->next_slot)); if (rc) return rc; }
    // from the host: the caller's arrays are free on return, whatever `hold' (no submit is counted that a later `hold' could refer to)
    if (!b.on_device) HIP_TRY(c, hipEventSynchronize(tr.places[push.t % tr.R].uploaded.get()));
    if (elapsed_ms) *elapsed_ms = 0.f;
    ++tr.pushed;
    return 0;
}

int davo_track_push(davo_ctx* c, const uint8_t* frames, const float* flow2, const float* seg, const float* depth, float* pose_out, int hold) {
    return track_push_entry(c, frame_batch("davo_track_push", false, frames, flow2, seg, depth), pose_out, hold, nullptr);
}

int davo_track_push_device(davo_ctx* c, const void* d_frames, const void* d_flow2, const void* d_seg, const void* d_depth, void* d_pose, float* elapsed_ms) {
    return track_push_entry(c, frame_batch("davo_track_push_device", true, d_frames, d_flow2, d_seg, d_depth), d_pose, 0, elapsed_ms);
}

int davo_track_frames(const davo_ctx* c) { return c && c->track ? (int)c->track->pushed : DAVO_ERR_INVALID; }

int davo_track_end(davo_ctx* c) {
    if (!c) return DAVO_ERR_INVALID;
    if (!c->track) return fail(c, DAVO_ERR_INVALID, "davo_track_end: no tracking session is open");
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = deliver_all(c);
    // nothing on the device may still touch the ring: every copy into it and every gather out of it has an event
    for (const TrackState::Place& p : c->track->places) {
        if (p.up) (void)hipEventSynchronize(p.uploaded.get());
        if (p.ga) (void)hipEventSynchronize(p.gathered.get());
    }
    c->track.reset();
    return rc;
}

// test hook: every byte of ring place `place' (its frames, label maps and depth planes) becomes `byte', once nothing in flight
// touches the ring
int davo_track_debug_fill(davo_ctx* c, int place, int byte) {
    if (!c) return DAVO_ERR_INVALID;
    if (!c->track || place < 0 || place >= c->track->R) return fail(c, DAVO_ERR_INVALID, "davo_track_debug_fill: no session, or place outside [0,R)");
    HIP_TRY(c, hipSetDevice(c->device));
    TrackState& tr = *c->track;
    for (const TrackState::Place& p : tr.places) {
        if (p.up) HIP_TRY(c, hipEventSynchronize(p.uploaded.get()));
        if (p.ga) HIP_TRY(c, hipEventSynchronize(p.gathered.get()));
    }
    const PlaneBytes f = frame_bytes(c);
    const size_t S = (size_t)tr.lanes;
    auto fill = [&](const DevMem<void>& d, size_t per) { return hipMemset(static_cast<uint8_t*>(d.get()) + per * S * place, byte, per * S); };
    HIP_TRY(c, fill(tr.img, f.img));
    HIP_TRY(c, fill(tr.seg, f.seg));
    if (tr.depth) HIP_TRY(c, fill(tr.depth, f.depth));
    HIP_TRY(c, hipStreamSynchronize(nullptr));               // (api.hip: zero_now)
    return DAVO_OK;
}

int davo_track_plan(int H, int W, int lanes, int pairs, int att_source, int label_fmt, int flow_fmt, int depth_fmt, long long* link_bytes) {
    const InputFormat fmt{label_fmt, flow_fmt, depth_fmt};
    if (H < 1 || W < 1 || lanes < 1 || (pairs != PAIRS_SRC0 && pairs != PAIRS_SRC1 && pairs != PAIRS_BOTH) || att_source < 0 || att_source > ATT_MAX || !valid(fmt))
        return DAVO_ERR_INVALID;
    if (link_bytes) *link_bytes = track_push_bytes(lanes, pairs, att_source, H, W, element_bytes(fmt));
    return DAVO_OK;
}

int davo_track_ring(int inflight, long long t, int* places, long long* after) {
    if (inflight < 1 || inflight > MAX_INFLIGHT || t < 0) return DAVO_ERR_INVALID;
    const TrackStep s = track_step(t, track_ring_places(inflight));
    if (places) { places[0] = s.upload_place; for (int k = 0; k < 3; ++k) places[1 + k] = s.place[k]; }
    if (after) { for (int k = 0; k < 3; ++k) after[k] = s.upload_after[k]; after[3] = s.gather_after[0]; after[4] = s.gather_after[1]; }
    return s.R;
}

}  // extern "C"

// the body of davo_forward, davo_forward_depth and davo_forward_frames, and of davo_forward_features / davo_forward_heat (export.hip;
// ex: the exports wanted): b's pointers are host pointers
int davo::forward_entry(davo_ctx* c, int B, Batch b, float* pose_out, const Exports ex) {
    { int rc = check_batch(c, &b, B, pose_out != nullptr); if (rc) return rc; }
    c->inputs_seen = true;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = deliver_all(c); if (rc) return rc; }          // davo_submit batches still under way: delivered first
    { int rc = sync_all_slots(c); if (rc) return rc; }       // the host path owns the single staging buffer set
    Stager st;
    { int rc = acquire_stager(c, b, Path::Forward, 0, &st); if (rc) return rc; }      // slot 0's: every slot is idle
    HostStaging& hs = *c->host;
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
        // (frame layout: windows [b0, b0 + nb) take frames [b0, b0 + nb + 2), the two it shares with the sub-batch before are on the
        // device already; window layout, both pairs: the label maps whole)
        { int rc = stage_upload(&st, b0, nb, cs); if (rc) return rc; }
        { int rc = stage_windows(&st, b0, nb, cs); if (rc) return rc; }
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

extern "C" {

int davo_forward(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, float* pose_out) {
    return forward_entry(c, B, window_batch("davo_forward", false, false, img, flow, seg, nullptr), pose_out);
}

int davo_forward_depth(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth, float* pose_out) {
    return forward_entry(c, B, window_batch("davo_forward", false, true, img, flow, seg, depth), pose_out);
}

int davo_forward_frames(davo_ctx* c, int N, const uint8_t* frames, const float* flow2, const float* seg, const float* depth, float* pose_out) {
    return forward_entry(c, N, frame_batch("davo_forward_frames", false, frames, flow2, seg, depth), pose_out);
}

}  // extern "C"
