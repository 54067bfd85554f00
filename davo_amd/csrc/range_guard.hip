// range_guard.hip — the f16x3 range guard's device-touching half: the ring's records and snapshots, the verdict on a record,
// calibration, the re-issue of a batch that failed, and the tickets of the batches that wait for their verdict.  Its bookkeeping
// is range_book.h (davo_ctx::book); the entry points that issue, deliver and synchronise are api.hip.
//
// The reference's float32 graph (nets/posenn.py:205-215, davo.py:1553-1569) never fails on a finite network, so the
// default f16x3 arithmetic must not either: a batch whose range record fails the verdict is re-issued here - first
// with the storage scales re-calibrated on that very batch, and if it still leaves the fp16-pair range, on the
// library's own float32 kernels (davo_set_precision(ctx, 0) for that batch only).  "auto_range" 0 restores the plain
// DAVO_ERR_RANGE verdict.
//
// Device path (round 4).  Every batch davo_forward_device issues owns one slot of a ring of RANGE_RING: a record of its own
// (zeroed by the forward's first kernel) and, unless the caller declared "stable_inputs", room for a copy of its inputs.  The
// batch's LAST kernel reads the finished record and, if a layer left the range, copies the inputs it was issued on into the
// slot (prologue.h: snapshot_inputs_if_range_fails) - in stream order behind the kernels that read them and ahead of anything
// the caller orders behind the batch, e.g. the next H2D into the same buffers.  A batch in range costs six loads per thread and
// no copy.  A batch is judged when its slot is needed again, at davo_synchronize, or before anything that changes the scales;
// a failed verdict re-issues THAT batch from the slot's copy, so a streaming caller that recycles its input buffers still gets
// float32-grade poses for every batch.  (First built with an unconditional side-stream copy: +1.6 % of the step at B = 32,
// profiles/r04_snapshot_ab.log.)
//
// One of each: ONE wait for a batch's record (wait_record), ONE verdict (judge_record), ONE place a verdict waits for
// davo_synchronize (RangeBook::defer / take_deferred).
#include <cmath>
#include <cstring>

#include "ctx.h"

namespace davo {

int ensure_ring(davo_ctx* c, bool snapshots) {
    if (!c->ring) {
        constexpr size_t words = (1 + RANGE_RING) * RANGE_WORDS;
        RangeRing r;
        HIP_TRY(c, stream_create(&r.read_stream));
        HIP_TRY(c, pinned_alloc(&r.h_range, words, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&r.h_range_dev), r.h_range.get(), 0));
        memset(r.h_range.get(), 0, words * sizeof(unsigned));
        c->ring = std::move(r);
    }
    if (snapshots && !c->snaps) {
        Snapshots sn;
        for (InputSet& set : sn.sets) { int rc = alloc_input_set(c, &set, false); if (rc) return rc; }
        c->snaps = std::move(sn);
    }
    return DAVO_OK;
}

namespace {

// a record -> host, on a stream of its own (never behind queued batches, never through the null stream)
int read_record(davo_ctx* c, const unsigned* d_rec, unsigned raw[RANGE_WORDS]) {
    { int rc = ensure_ring(c, false); if (rc) return rc; }
    const RangeRing& r = *c->ring;
    HIP_TRY(c, hipMemcpyAsync(r.h_range.get(), d_rec, RANGE_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, r.read_stream.get()));
    HIP_TRY(c, hipStreamSynchronize(r.read_stream.get()));
    memcpy(raw, r.h_range.get(), RANGE_WORDS * sizeof(unsigned));
    return DAVO_OK;
}

unsigned* ring_record(davo_ctx* c, int r) { return c->d_range_base.get() + RANGE_WORDS * (1 + r); }
const unsigned* ring_mirror(const davo_ctx* c, int r) { return c->ring->h_range.get() + RANGE_WORDS * (1 + r); }      // (a ticket exists, so the ring does)

int zero_base_record(davo_ctx* c, hipStream_t s) {
    HIP_TRY(c, hipMemsetAsync(c->d_range_base.get(), 0, RANGE_WORDS * sizeof(unsigned), s));
    return DAVO_OK;
}

}  // namespace

// The record of sequence number `seq' is final in mirror m -> raw.  The batch's last kernel, on stream s, writes its sequence
// number into the mirror behind the maxima (prologue.h): poll that, with the stream's own state as the way out if the device has
// failed.  Returns at once when the mirror already carries seq - always so where s is idle.
int wait_record(davo_ctx* c, const unsigned* mirror, unsigned seq, hipStream_t s, unsigned raw[RANGE_WORDS]) {
    volatile const unsigned* m = mirror;
    for (unsigned spin = 0; m[RANGE_SEQ] != seq; ++spin) {
        if ((spin & 1023u) == 1023u) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) {                                    // the stream is idle: the store is on its way or the kernel never ran
                if (m[RANGE_SEQ] == seq) break;
                HIP_TRY(c, hipStreamSynchronize(s));
                if (m[RANGE_SEQ] != seq) return fail(c, DAVO_ERR_HIP, "a batch finished without reporting its range record");
                break;
            }
            if (q != hipErrorNotReady) return fail(c, DAVO_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(q));
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    for (int i = 0; i < RANGE_WORDS; ++i) raw[i] = m[i];
    return DAVO_OK;
}

// f16x3 only.  Stored activations (fp16 hi/lo pairs) are float32-grade while the layer's largest stored value is
// below the fp16 maximum (above it values were clamped) and not so small that the pairs lose their low bits
// (tools/exp_activation_scale.py: with ONE layer off its scale the 1e-4 bar holds down to ~2^-16 of O(1) activations; with
// all six stored layers at the floor the errors add up, so the guard is 2^-6: docs/F16X3_NUMERICS.md, "The guard's floor").
// The verdict on the record of a batch issued under the scales `shifts': DAVO_ERR_RANGE (the message names the layer), or DAVO_OK -
// and then the batch's true magnitudes enter range_seen (davo_activation_range)
int judge_record(davo_ctx* c, const unsigned* raw, const int* shifts) {
    static const char* names[6] = {"cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6"};
    for (int i = 0; i < 6; ++i) {
        float v;
        if (i == 5 && c->posenn_se) {                // in the order of the forward: between cnv5 and cnv6
            // the scaled cnv5 of the feature-attention variant is a stored activation of its own.  It shares cnv5's scale and every
            // factor is a sigmoid, so it cannot clamp where cnv5 did not, but it can sink below the floor - and no calibration moves
            // it there without moving cnv5: such a batch ends on the float32 kernels (recover_batch)
            memcpy(&v, &raw[RANGE_SE], sizeof v);
            if (range_value_fails(v))
                return fail(c, DAVO_ERR_RANGE, "cnv5_se activations (cnv5 times its feature-attention scales) are at most %.4g: %s for the fp16-pair "
                            "storage at cnv5's scale 2^%d - davo_set_precision(ctx, 0)", (double)ldexpf(v, -shifts[4]),
                            v < 65504.f ? "too small" : "outside the range", shifts[4]);
        }
        memcpy(&v, &raw[i], sizeof v);
        if (!range_value_fails(v)) continue;         // params.h: the test the batch's last kernel applies too
        const float actual = ldexpf(v, -shifts[i]);
        if (!(v < 65504.f))
            return fail(c, DAVO_ERR_RANGE, "%s activations reach %.4g: outside the fp16-pair storage range at scale 2^%d "
                        "(values were clamped) - run davo_calibrate() or davo_set_precision(ctx, 0)", names[i], (double)actual, shifts[i]);
        return fail(c, DAVO_ERR_RANGE, "%s activations are at most %.4g: too small for the fp16-pair storage at scale 2^%d "
                        "- run davo_calibrate() or davo_set_precision(ctx, 0)", names[i], (double)actual, shifts[i]);
    }
    for (int i = 0; i < 6; ++i) {                    // in range: what davo_activation_range reports
        float v;
        memcpy(&v, &raw[i], sizeof v);
        const float t = ldexpf(v, -shifts[i]);
        if (!(t <= c->range_seen[i])) c->range_seen[i] = t;          // NaN / inf records stay visible
    }
    return DAVO_OK;
}

// Every stream idle.  The ring's running maxima (params.h) are about to lose their meaning - a failed verdict, or the scales are
// going to change: read the record of every batch that is still waiting for its verdict into its ticket first, then reset the ring.
int freeze_pending_and_reset_ring(davo_ctx* c) {
    for (Ticket& t : c->book.tickets)
        if (!t.frozen) {
            // every stream the context knows is idle, so the mirrors are final - unless the batch went out on a caller's stream the
            // context no longer runs on (davo_set_stream judges its tickets before a switch; this is the belt to those braces)
            { int rc = wait_record(c, ring_mirror(c, t.ring), t.seq, t.stream, t.raw); if (rc) return rc; }
            t.frozen = true;
        }
    { int rc = zero_now(c, c->d_range_base.get() + RANGE_WORDS, RANGE_RING * RANGE_WORDS * sizeof(unsigned)); if (rc) return rc; }
    return DAVO_OK;
}

// power-of-two storage scales from a sample batch: each pass runs the path and moves every layer's largest stored
// value into [512, 1024).  A layer computed from badly ranged inputs still has about the right magnitude, so each
// pass fixes at least the first badly ranged layer exactly and the later ones to within a few powers of two.
// Runs on the base record; every stream must be idle.  sel: davo_calibrate runs both pairs of the batch it is handed; a re-issue
// calibrates on the pairs the batch ran (an unselected frame's planes may never have been copied: stale bytes).
int calibrate_on(davo_ctx* c, int B, const Inputs& in, void* d_pose, int sel) {
    int rc = DAVO_OK;
    Run run = make_run(c, 0);
    run.pairs = sel; run.precision = 1; run.impl = 0;
    for (int pass = 0; pass < 8 && rc == DAVO_OK; ++pass) {
        if ((rc = zero_base_record(c, run.stream))) break;
        rc = forward_device(c, run, B, in, d_pose);
        if (rc) break;
        if (hipStreamSynchronize(run.stream) != hipSuccess) { rc = fail(c, DAVO_ERR_HIP, "hipStreamSynchronize failed"); break; }
        unsigned raw[RANGE_WORDS];
        if ((rc = read_record(c, c->d_range_base.get(), raw))) break;
        bool changed = false;
        for (int i = 0; i < 6; ++i) {
            float v;
            memcpy(&v, &raw[i], sizeof v);
            int delta = 0;
            if (!std::isfinite(v)) delta = -32;
            else if (v > 0.f) { int e; (void)frexpf(v, &e); delta = 10 - e; }        // stored max -> [2^9, 2^10): 64x headroom
            int ns = c->act_shift[i] + delta;
            ns = ns < -60 ? -60 : (ns > 60 ? 60 : ns);
            if (ns != c->act_shift[i]) { c->act_shift[i] = ns; changed = true; }
        }
        if (!changed) break;
    }
    (void)zero_base_record(c, run.stream);
    return rc;
}

namespace {

// one batch, synchronously, on the base record; -> DAVO_OK, DAVO_ERR_RANGE (the verdict) or a hard error
int run_judged(davo_ctx* c, const Run& run, const Reissue& b) {
    { int rc = zero_base_record(c, run.stream); if (rc) return rc; }
    RunResult res;
    int rc = forward_device(c, run, b.B, b.in, b.pose, &res);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(run.stream));
    if (!res.h3) return DAVO_OK;
    unsigned raw[RANGE_WORDS];
    if ((rc = read_record(c, c->d_range_base.get(), raw))) return rc;
    return judge_record(c, raw, c->act_shift);
}

}  // namespace

// A failed verdict: re-issue the batch, with the pair selection it was issued with - as issued if the scales have moved since and now hold it, re-calibrated on itself if
// not, on the float32 kernels if even that leaves the range (per-layer scales cannot cover e.g. an inf / NaN producing net).
// Drains every stream first: the re-issue uses slot 0's workspace and the base record.
// A caller may have handed the batch's pose buffer to a LATER batch since (two alternating buffers, one buffer overwritten every
// step): the re-issue therefore writes into a pose buffer of the context and is copied to the caller's only if no batch
// issued after this one targets an overlapping range - the newest writer of a buffer always wins (RangeBook::superseded).
int recover_batch(davo_ctx* c, const Reissue& orig) {
    { int rc = sync_all_slots(c); if (rc) return rc; }
    const std::string verdict = c->err;
    { int rc = freeze_pending_and_reset_ring(c); if (rc) return rc; }       // the failed slot's maximum must go; the scales may move
    if (!c->d_reissue_pose) HIP_TRY(c, dev_alloc(&c->d_reissue_pose, (size_t)c->max_batch * 12));
    Reissue b = orig;
    b.pose = c->d_reissue_pose.get();
    Run run = make_run(c, 0);
    run.pairs = b.pairs;
    int rc = run_judged(c, run, b);
    if (rc == DAVO_ERR_RANGE) {
        if ((rc = calibrate_on(c, b.B, b.in, b.pose, b.pairs))) return rc;
        ++c->n_recalibrations;
        rc = run_judged(c, run, b);
        c->range_report = "re-calibrated: " + verdict;
    }
    if (rc == DAVO_ERR_RANGE) {
        run.precision = 0;
        rc = forward_device(c, run, b.B, b.in, b.pose);
        if (rc == DAVO_OK && hipStreamSynchronize(run.stream) != hipSuccess) rc = fail(c, DAVO_ERR_HIP, "hipStreamSynchronize failed");
        ++c->n_f32_batches;
        c->range_report = "float32 kernels for one batch: " + verdict;
    }
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(run.stream));
    if (!c->book.superseded(orig))
        HIP_TRY(c, hipMemcpy(orig.pose, c->d_reissue_pose.get(), (size_t)orig.B * 12 * sizeof(float), hipMemcpyDeviceToDevice));
    ++c->n_reissued;
    c->err.clear();
    return DAVO_OK;
}

// verdict on the oldest unjudged device-path batch (waits for that batch only)
int judge_front(davo_ctx* c) {
    const Ticket t = c->book.take_front();
    unsigned raw[RANGE_WORDS];
    if (t.frozen) memcpy(raw, t.raw, sizeof raw);        // read when the ring was reset (every stream was idle then)
    else { int rc = wait_record(c, ring_mirror(c, t.ring), t.seq, t.stream, raw); if (rc) return rc; }
    int rc = judge_record(c, raw, t.shifts);
    if (rc == DAVO_ERR_RANGE && c->opt_auto_range) {
        // the batch's last kernel reached the same verdict on the same record and kept the inputs (prologue.h)
        if (t.snap && raw[RANGE_SNAP] != 1u) rc = fail(c, DAVO_ERR_INVALID, "internal: a batch failed its range verdict but its inputs were not kept");
        else {
            rc = recover_batch(c, t.reissue());
            // a davo_submit batch: the re-issue rewrote the pose ring entry, its page-locked twin follows (every stream is idle)
            if (rc == DAVO_OK && t.h_pose && hipMemcpy(t.h_pose, t.pose, (size_t)t.B * 12 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                rc = fail(c, DAVO_ERR_HIP, "copying re-issued poses to the host failed");
        }
    } else if (rc == DAVO_ERR_RANGE && !t.frozen) {
        // no recovery ("auto_range" 0): the slot's running maximum has served its verdict - the next batch starts afresh
        const std::string keep = c->err;
        if (hipMemsetAsync(ring_record(c, t.ring), 0, RANGE_WORDS * sizeof(unsigned), c->ring->read_stream.get()) != hipSuccess ||
            hipStreamSynchronize(c->ring->read_stream.get()) != hipSuccess) rc = fail(c, DAVO_ERR_HIP, "resetting a range record failed");
        else c->err = keep;
    }
    c->book.release(t.ring);              // after the re-issue: it read the slot's copy of the inputs
    return rc;
}

// every unjudged batch; a failed verdict with "auto_range" 0 does not stop the others from being judged: it joins the deferred
// one (the first wins), and the store is empty again when this returns
int judge_all(davo_ctx* c) {
    while (!c->book.tickets.empty()) {
        const int rc = judge_front(c);
        if (rc == DAVO_ERR_RANGE) c->book.defer(rc, c->err);
        else if (rc) { c->book.drop_all(); (void)c->book.take_deferred(); return rc; }
    }
    const Verdict first = c->book.take_deferred();
    { int rc = sync_all_slots(c); if (rc) return rc; }
    if (first.rc) { c->err = first.err; return first.rc; }
    return DAVO_OK;
}

// the batch about to be issued takes the ring slot at the cursor: judge what still holds it (may re-issue: before the slot rotation)
int ticket_reserve(davo_ctx* c) {
    while (c->book.cursor_held()) {
        const int rc = judge_front(c);
        if (rc == DAVO_ERR_RANGE && !c->opt_auto_range) c->book.defer(rc, c->err);      // reported by the next davo_synchronize; this batch is issued all the same
        else if (rc) return rc;
    }
    return DAVO_OK;
}

// ... the batch's kernels record into the slot's record; its last kernel keeps the inputs there if the record fails: *run is told so.
// *t receives what is known of the batch's ticket now: above all what a re-issue would read
int ticket_begin(davo_ctx* c, Run* run, int B, const Inputs& in, Ticket* t, bool own_inputs) {
    const int r = c->book.ring_next;
    *t = Ticket{};
    t->B = B; t->ring = r; t->pairs = run->pairs; t->stream = run->stream;
    // own_inputs: the batch reads a staging set of the context (davo_submit), which the next batches overwrite whatever the caller declared
    t->snap = c->opt_auto_range && (!c->opt_stable_inputs || own_inputs);
    if (t->snap && (((uintptr_t)in.img | (uintptr_t)in.flow | (uintptr_t)in.seg | (uintptr_t)in.depth) & 15)) return fail(c, DAVO_ERR_INVALID, "device input buffers must be 16-byte aligned");
    { int rc = ensure_ring(c, t->snap); if (rc) return rc; }
    run->range = ring_record(c, r);
    run->zero_record = true;
    // The records hold RUNNING maxima (params.h): "clamped" is exact per batch, "too small" is judged on everything a slot has stored
    // since its record was last zeroed.  So that a long stream that never synchronises still notices activations that collapse,
    // every FRESH_EVERY-th batch starts from a zeroed record (a memset in stream order ahead of the batch's kernels; that batch pays
    // its first round's atomics, ~0.2 ms, once in FRESH_EVERY batches).
    if (c->book.ring_record_due()) {
        HIP_TRY(c, hipMemsetAsync(run->range, 0, 6 * sizeof(unsigned), run->stream));
        if (c->posenn_se) HIP_TRY(c, hipMemsetAsync(run->range + RANGE_SE, 0, sizeof(unsigned), run->stream));
    }
    t->seq = c->book.next_seq();
    const InputSet none;
    const InputSet& keep = t->snap ? c->snaps->sets[r] : none;        // no snapshot: no destination, and the ticket remembers the caller's buffers
    t->in = t->snap ? keep.view() : in;
    const PlaneBytes nb = plane_bytes(c);
    auto src = [](const void* q) { return static_cast<const uint8_t*>(q); };
    auto dst = [](const DevMem<void>& q) { return static_cast<uint8_t*>(q.get()); };
    run->snap = SnapArgs{run->range, c->ring->h_range_dev + RANGE_WORDS * (1 + r), t->seq,
                       src(in.img), src(in.flow), src(in.seg), dst(keep.img), dst(keep.flow), dst(keep.seg),
                       (unsigned)(nb.img / 16), (unsigned)(nb.flow / 32), (unsigned)(nb.flow / 16), (unsigned)(nb.seg / 16), B,
                       src(in.depth), dst(keep.depth), c->posenn_se, (unsigned)(nb.depth / 16)};
    return DAVO_OK;
}

// the batch is out (rc, res: forward_device's): its ticket is filed
int ticket_end(davo_ctx* c, int rc, const RunResult& res, Ticket t, void* d_pose, float* h_pose) {
    if (rc) return rc;
    if (res.f32_fallback) ++c->n_f32_batches;
    t.pose = d_pose; t.h_pose = h_pose;
    for (int i = 0; i < 6; ++i) t.shifts[i] = c->act_shift[i];
    c->book.file(t, res.h3);                                                     // float32 kernels (weight guard): no record, no verdict
    return DAVO_OK;
}

}  // namespace davo
