// Stand-alone check of davo_amd/csrc/range_book.h (tests/test_range_book.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it): the range guard's bookkeeping, with no GPU and no HIP.
#include <cstdio>
#include <cstdlib>

#include "range_book.h"

using namespace davo;

#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } \
    } while (0)

// what ticket_begin / ticket_end know of a batch when it is filed
static Ticket ticket(const RangeBook& b, void* pose, int B) {
    Ticket t{};
    t.B = B; t.pose = pose; t.ring = b.ring_next;
    return t;
}

// one f16x3 davo_forward_device: span noted, then the ticket filed
static void issue(RangeBook& b, void* pose, int B, bool ran_f16x3 = true) {
    Ticket t = ticket(b, pose, B);
    t.seq = b.next_seq();
    b.note_issue(pose, B);
    b.file(t, ran_f16x3);
}

static void sequence_numbers() {
    RangeBook b;
    CHECK(b.next_seq() == 1 && b.next_seq() == 2);
    b.batch_seq = 0xfffffffeu;
    CHECK(b.next_seq() == 0xffffffffu);
    CHECK(b.next_seq() == 1);                      // never 0: a zeroed mirror must not look like a batch's report
}

static void ring_rotation() {
    RangeBook b;
    float pose[8][24];
    for (int k = 0; k < RANGE_RING; ++k) {
        CHECK(b.ring_next == k && !b.cursor_held());       // the cursor walks 0..7
        issue(b, pose[k], 2);
    }
    CHECK(b.ring_next == 0 && b.cursor_held());            // ... and then 0: held, the front must be judged first
    CHECK(b.tickets.size() == (size_t)RANGE_RING && b.tickets.front().ring == 0);
    const Ticket front = b.take_front();
    CHECK(front.ring == 0 && front.seq == 1 && b.cursor_held());       // held until the verdict AND the re-issue are done
    CHECK(b.pending(2) && !b.pending(1));
    b.release(front.ring);
    CHECK(!b.cursor_held() && b.ring_busy[1]);
    issue(b, pose[0], 2);
    CHECK(b.ring_next == 1 && b.cursor_held() && b.tickets.back().ring == 0);
    // a batch that ran on the float32 kernels files nothing and leaves the cursor where it was
    b.release(b.take_front().ring);
    const size_t n = b.tickets.size();
    issue(b, pose[1], 2, false);
    CHECK(b.ring_next == 1 && !b.cursor_held() && b.tickets.size() == n);
    b.drop_all();
    CHECK(b.tickets.empty());
    for (int r = 0; r < RANGE_RING; ++r) CHECK(!b.ring_busy[r]);
}

static void supersede_rule_and_spans() {
    RangeBook b;
    static float buf[3 * 24];                              // three pose buffers of B = 2, back to back
    float *p0 = buf, *p1 = buf + 24, *p2 = buf + 48;
    // spans are recorded only while a ticket is pending
    b.note_issue(p1, 2);                                   // a float32 batch, nothing pending
    CHECK(b.pose_spans.empty());
    issue(b, p1, 2);                                       // batch 2 (its own span is not kept: nothing was pending when it was noted)
    CHECK(b.pose_spans.empty() && b.tickets.size() == 1);
    const Reissue first = b.tickets.front().reissue();
    CHECK(first.device_path && first.issue == 2 && first.pose == p1 && first.B == 2);
    CHECK(!b.superseded(first));
    // an adjacent half-open range [hi, ...) does not supersede, nor does the one that ends at lo
    issue(b, p2, 2);
    issue(b, p0, 2);
    CHECK(b.pose_spans.size() == 2 && !b.superseded(first));
    // a later batch whose pose range overlaps does - by one float at either end
    issue(b, p0 + 1, 2);
    CHECK(b.superseded(first));
    const Reissue third = b.tickets[2].reissue();          // the batch into p0: superseded by p0 + 1 as well
    CHECK(third.issue == 4 && b.superseded(third));
    // an earlier batch's span does not: the batch into p0 + 1 is the newest writer of its range
    const Reissue last = b.tickets.back().reissue();
    CHECK(last.issue == 5 && !b.superseded(last));
    const Reissue second = b.tickets[1].reissue();         // p2: [p2, p2 + 24) touches nothing issued later
    CHECK(!b.superseded(second));
    // the host path's re-issue is never superseded, whatever the spans say
    CHECK(!b.superseded(Reissue{2, 3, Inputs{}, p1, false, 0}));
    CHECK(!b.superseded(Reissue{2, 3, Inputs{}, p0, false, 0}));
    // davo_submit counts the issue and leaves no span
    const size_t spans = b.pose_spans.size();
    b.note_issue();
    CHECK(b.n_issued == 6 && b.pose_spans.size() == spans);
    // pruned once no pending ticket is older: judging the first two leaves the ticket of issue 4 in front
    b.release(b.take_front().ring);
    b.release(b.take_front().ring);
    b.note_issue(p2, 2);
    CHECK(b.tickets.front().issue == 4);
    for (const PoseSpan& sp : b.pose_spans) CHECK(sp.issue > 4);
    CHECK(b.pose_spans.size() == 2);                       // issues 5 and 7
    b.drop_all();
    b.note_issue(p2, 2);
    CHECK(b.pose_spans.empty());
    // the bound on spans behind a pending ticket
    issue(b, p0, 2);
    for (size_t k = 0; k < MAX_POSE_SPANS; ++k) b.note_issue(p2, 2);
    CHECK(!b.spans_full());
    b.note_issue(p2, 2);
    CHECK(b.spans_full());
}

static void deferred_verdict() {
    RangeBook b;
    CHECK(b.take_deferred().rc == 0);
    b.defer(-5, "cnv3 first");
    b.defer(-5, "cnv4 second");                            // the first one wins
    Verdict v = b.take_deferred();
    CHECK(v.rc == -5 && v.err == "cnv3 first");
    v = b.take_deferred();                                 // taking it cleared it
    CHECK(v.rc == 0 && v.err.empty());
    b.defer(-5, "cnv4 second");                            // ... so the next one is kept
    CHECK(b.deferred.rc == -5 && b.deferred.err == "cnv4 second");
    b.reset();                                             // reset clears it
    CHECK(b.take_deferred().rc == 0);
}

static void fresh_records_and_reset() {
    RangeBook b;
    CHECK(b.host_record_due());                            // davo_forward's first call starts afresh
    int due = 0;
    for (int k = 0; k < 2 * FRESH_EVERY; ++k) due += b.host_record_due();
    CHECK(due == 2 && b.host_since_fresh == 0);
    b.host_record_stale();
    CHECK(b.host_record_due() && !b.host_record_due());
    due = 0;
    for (int k = 1; k <= 2 * FRESH_EVERY; ++k)
        if (b.ring_record_due()) { ++due; CHECK(k % FRESH_EVERY == 0); }
    CHECK(due == 2);
    // reset: cursor, counters and the deferred verdict as in a new book; sequence and issue numbers keep counting
    float pose[24];
    issue(b, pose, 2);
    b.release(b.take_front().ring);
    (void)b.ring_record_due();
    b.defer(-5, "x");
    const unsigned seq = b.batch_seq;
    const unsigned long long n = b.n_issued;
    b.reset();
    const RangeBook fresh;
    CHECK(b.ring_next == fresh.ring_next && b.since_fresh_record == fresh.since_fresh_record &&
          b.host_since_fresh == fresh.host_since_fresh && b.deferred.rc == 0 && b.deferred.err.empty());
    CHECK(b.batch_seq == seq && b.n_issued == n && b.host_record_due());
}

int main() {
    sequence_numbers();
    ring_rotation();
    supersede_rule_and_spans();
    deferred_verdict();
    fresh_records_and_reset();
    puts("range book ok");
    return 0;
}
