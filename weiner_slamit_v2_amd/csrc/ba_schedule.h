// ba_schedule.h — the chunk schedule of one LM stage of the local BA (Optimizer.cc:659-707), as a state machine without a device.
// Plain C++ (no HIP): the solve (ba_api.hip) drives the device by it, tests/test_ba_schedule.py a fake one.
//
// LM trial slots are queued in chunks; the windows' states come back through two pinned host buffers one chunk LATE (the next chunk
// is already queued when the host looks at the previous one: no bubble between chunks).  Slots of a finished stage return at once,
// but a slot queued in vain still costs its launches (~30 us): the first chunk of a stage is the number of trials the stage cannot do
// without (one per iteration in the robust stage; three in the final one, whose "no progress three times" rule can end it that
// early; four at the most), the chunks after it are single slots.  (Chunks of two throughout queued 20 slots for the 14 trials of a
// window-8 solve.)  A stage queues at most 10 its + 1 slots (ten LM trials per iteration), and at least one: its == 0 still queues a
// slot, which the kernels return from at once.
//
// The schedule is the trace it produces:
//   Q(n, buf, first)  n slots queued, the first of them flagged as the stage's first slot when `first`, then the states copied to
//                     host buffer `buf` and event `buf` recorded;
//   W(buf)            event `buf` waited for and the `done` flags of buffer `buf` read.
// One step of the driver is: poll the caller's stop flag; next(); Q if nslots; W if wbuf >= 0; finished(all windows done in W).
// Within a step Q comes before W, and W reads the buffer of the step before: a buffer is never queued into again before its W.
#ifndef SLAMIT_BA_SCHEDULE_H
#define SLAMIT_BA_SCHEDULE_H

#include <algorithm>

struct BaChunk {
    int nslots;   // slots to queue now (0: the budget is spent, nothing more is queued)
    int qbuf;     // the buffer their read-back goes to
    bool first;   // the first of them is the stage's first slot
    int wbuf;     // the buffer to wait for and inspect after queueing (-1: none yet)
};

class BaStageSchedule {
public:
    BaStageSchedule(int stage, int its)
        : budget_(its * 10 + 1), first_chunk_(std::max(1, std::min(stage == 0 ? its : 3, std::min(its, 4)))) {}

    BaChunk next() {
        BaChunk c{0, cur_, first_, pending_};
        if (budget_ > 0) {
            c.nslots = std::min(first_ ? first_chunk_ : 1, budget_);
            first_ = false;
            budget_ -= c.nslots;
        }
        return c;
    }

    // `all_done`: every window's `done` in the buffer just inspected (false when there was none).  True: the stage is over.
    bool finished(bool all_done) {
        if (all_done || (budget_ <= 0 && pending_ == cur_)) return true;   // (the latter: nothing new was queued, the last read-back has been looked at)
        pending_ = cur_;
        if (budget_ > 0) cur_ ^= 1;
        return false;
    }

private:
    int budget_, first_chunk_;
    int cur_ = 0, pending_ = -1;
    bool first_ = true;
};

#endif
