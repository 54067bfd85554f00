// range_book.h — the bookkeeping of the f16x3 range guard as one plain type: which ring slot the next batch takes, which
// batches still wait for their verdict, whose pose buffer a later batch has taken, the sequence numbers the batches' last
// kernels report with, the verdict an entry point could not return itself, and the cadence of the fresh records.  Host C++
// with no HIP call in it and no include beyond the standard library, so it is tested without a GPU (tests/test_range_book.py);
// everything that touches the device is range_guard.hip.
#pragma once
#include <cstddef>
#include <cstdint>
#include <deque>
#include <string>
#include <utility>

typedef struct ihipStream_t* hipStream_t;      // as the HIP API header declares it (a ticket remembers its stream; nothing here calls HIP)

namespace davo {

constexpr int RANGE_RING = 8;                  // ring slots: batches that may wait for their verdict at one time
constexpr int RECORD_WORDS = 12;               // words of a range record (params.h: RANGE_WORDS; ctx.h asserts they agree)
constexpr int FRESH_EVERY = 256;               // every FRESH_EVERY-th batch starts from a zeroed record (range_guard.hip: ticket_begin)
constexpr size_t MAX_POSE_SPANS = 64;          // float32 batches noted behind pending tickets before the tickets are judged

// The planes of one batch, as every host function hands them on: img [B][H][W][9] bytes, flow [B][8][H][W], seg [B][3][H][W] and
// depth [B][3][H][W] float32 in file order (src0, tgt, src1).  depth is read by the depth sources only (att_source 11, 12) and is
// null for every other variant.
struct Inputs { const void *img, *flow, *seg, *depth; };

// What a re-issue reads, and whether the newest-writer-wins rule applies to its pose buffer: a device-path batch may have lost
// the buffer to a batch issued after it; davo_forward's batch cannot (the call returns before anything else is issued).
struct Reissue {
    int B;
    int pairs;                                 // the pair selection the batch was issued with
    Inputs in;
    void* pose;
    bool device_path;
    unsigned long long issue;                  // device path: the batch's issue number
};

// A batch davo_forward_device has issued whose f16x3 range record has not been judged yet.  Every such batch owns one slot of a
// small ring: a range record of its own and - unless the caller declared its inputs stable - room for a context-owned copy of
// its inputs, which the batch's last kernel fills if (and only if) the record will fail the verdict, so that the re-issue reads
// exactly what was issued whatever the caller has done to its buffers since (range_guard.hip, prologue.h).
struct Ticket {
    int B;
    int pairs;                                 // the pair selection the batch was issued with: every re-issue runs the same pairs, whatever davo_set_pairs said since
    Inputs in;                                 // what a re-issue reads: the ring slot's snapshot, or the caller's buffers ("stable_inputs")
    void* pose;
    int ring;
    bool snap;                                 // `in` is the ring slot's copy
    bool frozen;                               // raw holds the batch's record (read before the ring's records were reset)
    unsigned raw[RECORD_WORDS];
    unsigned seq;                              // the batch's sequence number: its last kernel writes it into the slot's host mirror
    hipStream_t stream;                        // the stream it was issued on
    int shifts[6];                             // storage scales the batch was issued under (davo_activation_range reports true magnitudes)
    unsigned long long issue;                  // issue number of the batch (RangeBook::superseded)
    float* h_pose;                             // davo_submit batches: page-locked host copy of `pose`, refreshed after a re-issue (else null)
    Reissue reissue() const { return Reissue{B, pairs, in, pose, true, issue}; }
};

struct PoseSpan { uintptr_t lo, hi; unsigned long long issue; };      // the pose buffer range of an issued batch

struct Verdict { int rc = 0; std::string err; };

struct RangeBook {
    std::deque<Ticket> tickets;                // issued, not judged yet, oldest first
    bool ring_busy[RANGE_RING] = {};           // the slot's record and snapshot belong to a ticket (until its verdict AND its re-issue)
    int ring_next = 0;                         // the cursor: the slot the next ticketed batch takes
    std::deque<PoseSpan> pose_spans;           // pose buffer ranges of the batches issued since the oldest pending ticket
    unsigned long long n_issued = 0;
    unsigned batch_seq = 0;                    // sequence number of the last batch that reports through a mirror (never 0 for a batch)
    int since_fresh_record = 0;                // ticketed batches since one last started from a zeroed range record
    int host_since_fresh = 1 << 30;            // davo_forward calls since the base record was last zeroed; the first call starts afresh
    Verdict deferred;                          // "auto_range" 0: a failed verdict met while issuing or delivering, reported by the next davo_synchronize

    unsigned next_seq() { if (++batch_seq == 0) batch_seq = 1; return batch_seq; }

    // ---- the ring ----
    bool cursor_held() const { return ring_busy[ring_next]; }       // the front ticket must be judged before the next batch is issued
    // the batch that took the slot at the cursor is out: its ticket is filed and the cursor moves on.  A batch that ran on the
    // float32 kernels (the weight guard) left no record: nothing to judge, and the next batch takes the same slot
    void file(Ticket t, bool ran_f16x3) {
        if (!ran_f16x3) return;
        t.issue = n_issued;
        tickets.push_back(t);
        ring_busy[t.ring] = true;
        ring_next = (t.ring + 1) % RANGE_RING;
    }
    Ticket take_front() { const Ticket t = tickets.front(); tickets.pop_front(); return t; }      // its slot stays held until release()
    void release(int ring) { ring_busy[ring] = false; }
    void drop_all() { for (const Ticket& t : tickets) ring_busy[t.ring] = false; tickets.clear(); }
    bool pending(unsigned seq) const {
        for (const Ticket& t : tickets) if (t.seq == seq) return true;
        return false;
    }

    // ---- the newest writer of a pose buffer wins ----
    // every batch davo_forward_device issues leaves the range of its pose buffer here - while a ticket is pending: only then can a
    // re-issue come later; entries no pending ticket can be older than are dropped
    void note_issue(const void* d_pose, int B) {
        ++n_issued;
        const unsigned long long oldest = tickets.empty() ? n_issued : tickets.front().issue;
        while (!pose_spans.empty() && pose_spans.front().issue <= oldest) pose_spans.pop_front();
        if (!tickets.empty()) pose_spans.push_back(PoseSpan{(uintptr_t)d_pose, (uintptr_t)d_pose + (size_t)B * 12 * sizeof(float), n_issued});
    }
    void note_issue() { ++n_issued; }          // davo_submit: no span (a pose ring entry is not reused before its batch has been delivered)
    bool spans_full() const { return pose_spans.size() > MAX_POSE_SPANS; }
    // a batch issued after this one targets an overlapping range of its pose buffer
    bool superseded(const Reissue& b) const {
        if (!b.device_path) return false;
        const uintptr_t lo = (uintptr_t)b.pose, hi = lo + (size_t)b.B * 12 * sizeof(float);
        for (const PoseSpan& sp : pose_spans)
            if (sp.issue > b.issue && sp.lo < hi && lo < sp.hi) return true;
        return false;
    }

    // ---- the deferred verdict: the first one wins; taking it clears it ----
    void defer(int rc, const std::string& err) { if (!deferred.rc) deferred = Verdict{rc, err}; }
    Verdict take_deferred() { Verdict v; std::swap(v, deferred); return v; }

    // ---- fresh records: -> this batch / call starts from a zeroed record ----
    bool ring_record_due() { if (++since_fresh_record < FRESH_EVERY) return false; since_fresh_record = 0; return true; }
    bool host_record_due() { if (++host_since_fresh < FRESH_EVERY) return false; host_since_fresh = 0; return true; }
    void host_record_stale() { host_since_fresh = FRESH_EVERY; }        // the scales changed: davo_forward's next call starts afresh

    // davo_reset_range_state, no ticket pending: cursor, counters and the deferred verdict as in a new book.  Sequence and issue
    // numbers keep counting: a mirror may still hold an old batch's number, and spans are told apart by theirs
    void reset() {
        host_since_fresh = 1 << 30;
        since_fresh_record = 0;
        ring_next = 0;
        deferred = Verdict{};
    }
};

}  // namespace davo
