// pt_stream_sched.hpp — the host side of the frame stream: which batch joins the running stream, how long the next group of iterations is, what a
// look at the device's scheduler words means, which batches retire.  Plain C++: no HIP runtime call and no context.  Everything that touches the
// device goes through the `Dev` the caller hands in: pt_stream_dev.hpp supplies the launches (StreamDev), tests/c/stream_sched_check.cpp a model of the
// device, so every decision below can be single-stepped on a CPU.
//
// A batch is SUBMITTED (its jobs are appended to the running stream, or a new stream starts) and later RETIRED (all its pixel-frame jobs done: its
// frames are added to the FRAME image, in u_frameCount order).  Between the two the host only PUMPS: it launches iterations (intersect + shade) in
// groups and looks at the scheduler words after each group.
//   pt_render_batch        = submit + pump until the batch is retired
//   pt_render_batch_async  = submit + pump until most of its jobs have been handed out; the rest, and the jobs still in flight, are finished
//                            underneath the next batch (or by pt_finish_image / any synchronous entry point)
// The host looks once per GROUP of iterations: a group = its launches + (a scan of the oldest batches) + a snapshot of Control, which lands in pinned
// memory behind the group's sequence number.  Up to two groups are in flight: the host looks at a snapshot when it has landed, so the stream always
// holds the next group's launches while one runs, and an asynchronous submission never waits for the iterations it started.
//
// What Dev provides (every int is 0 or a PT_ERR_* code unless said otherwise):
//   int launchIterations(int n, unsigned launched, int iter)   n iterations from number `iter` on, each over at most `launched` slots
//   int launchScan(const SchedScan& ends)                      which of the oldest batches does a live slot still work on (Control::busy)
//   int launchSnapshot(int slot, unsigned seq)                 Control into the snapshot `slot` (0 or 1), then seq as its stamp
//   int landed(int slot, unsigned seq, bool wait, ControlView& v)   1: the snapshot has landed, v is its view; 0: not yet (wait = false only); < 0: error
//   int retire(const StreamEntry& e)                           accumulate the batch
//   int sceneReady() / int openStream(int pool)                a new stream: the scene built, or its refusal; then everything a stream of `pool`
//                                                              slots needs, Control initialised, every slot dead
//   int growPool(int from, int to)                             the slots [from, to) are dead
//   int appendJobs(unsigned f0, int nFrames, unsigned nJobs, int mode, int pool)   the seeds of frames f0..., k_submit(nJobs, mode, pool), revive
//   uint64_t itersPerJob()                                     iterations within which every job of the running stream retires
//   int didNotDrain()                                          the error of a pump beyond its bound
#pragma once
#include <algorithm>
#include <cstdint>
#include <deque>
#include "pt_launch_plan.hpp"

// iterations of a group while jobs remain (the test builds the scheduler once with another value)
#ifndef PT_SCHED_GROUP
#define PT_SCHED_GROUP 24
#endif

namespace ptp {

// PUMP_IDLE: every batch retired.  PUMP_ISSUED: the jobs not yet handed out fit into roughly one more group of iterations (never waits for the pool
// to run dry, and never for the group it starts).  PUMP_IMAGE: no unretired batch targets image `arg`.  PUMP_RING: at most `arg` ring rows are still
// owned by unretired batches.
enum PumpUntil { PUMP_IDLE, PUMP_ISSUED, PUMP_IMAGE, PUMP_RING };

struct ControlView {               // what the host reads of a snapshot of Control
    unsigned nextJob = 0, exhausted[4] = {0, 0, 0, 0}, qCount0 = 0, qCount32 = 0, busy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
struct SchedScan { unsigned f[8]; int n; };      // ends.f[k] = first stream frame BEHIND the k-th oldest unretired batch (k_scan_inflight)
struct StreamEntry { unsigned jobEnd, f0; int nFrames, firstFrame, image; };      // a submitted, not yet accumulated batch

// a submission as submitBatch hands it over: the batch, and what decides whether the running stream can take it
struct SubmitReq {
    int firstFrame = 0, nFrames = 1, image = 0; uint64_t nJobs = 0; bool async = false;
    bool sceneDirty = false, sameInputs = true, sameContract = true;      // against what the running stream was started with
    int ringFrames = 0, wantRing = 0;                  // rows of the frame ring as allocated / as this batch wants them (ringRows)
    int poolSlots = 0, allocSlots = 0;                 // pt_set_option 0 (0 = automatic); slots allocated
};

// the decisions a scheduler has taken so far, one bit each (tests/test_stream_sched.py requires every one of them of its scripts)
enum SchedBranch {
    BR_NEW_STREAM, BR_JOIN, BR_REFUSE_DIRTY, BR_REFUSE_INPUTS, BR_REFUSE_RING, BR_REFUSE_CONTRACT, BR_REFUSE_JOBS, BR_RING_WAIT, BR_RING_RESTART,
    BR_POOL_GROWN, BR_POOL_KEPT, BR_KICK_FIRST, BR_ISSUED_LEFT, BR_ISSUED_KICK, BR_TAIL_GROUP, BR_STALE_EPOCH, BR_ALL_DEAD, BR_SCAN_PARTIAL,
    BR_SCAN_EIGHT, BR_SCAN_MOVED, BR_DISCARDED, BR_UNTIL_IMAGE, BR_UNTIL_RING, BR_DROPPED, BR_DID_NOT_DRAIN, BR_COUNT
};

struct StreamSched {
    std::deque<StreamEntry> pending;
    unsigned streamFrames = 0, streamJobs = 0;         // frames and jobs submitted to the running stream
    unsigned lastNextJob = 0, lastDelta = 0; int lastCheck = PT_SCHED_GROUP;      // Control::nextJob at the last look, what it had grown by, over how many iterations
    unsigned launched = 0; int iter = 0; bool draining = false;      // the host's upper bound on the slots an iteration visits; the next iteration's number; the tail has begun
    uint64_t lastSubmitJobs = 0, jobsThisImage = 0, jobsPerImage = 0;      // what the last submission added; jobs submitted for the current / the previous FRAME image
    int poolActive = 0;                                // slots of the running stream's pool
    // host words of the (up to two) groups in flight; their snapshots and stamps are the caller's, by slot
    struct Group { unsigned seq = 0; int check = 0, iterEnd = 0, nScan = 0; unsigned scanF0 = 0, epoch = 0; int64_t predicted = 0; };
    Group grp[2]; int grpHead = 0, grpCount = 0; bool scanInFlight = false; unsigned submitEpoch = 0, groupSeq = 0;
    int64_t inflightPredicted = 0;  // jobs the groups in flight are expected to hand out (iterations x the rate of the last look): lastNextJob is as old as the oldest of them
    uint64_t reached = 0;           // SchedBranch bits

    void note(SchedBranch b) { reached |= 1ull << b; }
    bool idle() const { return pending.empty(); }
    // pt_next_image: the jobs of the image just left are what an image takes (grownPool)
    void imageTurned() { if (jobsThisImage) jobsPerImage = jobsThisImage; jobsThisImage = 0; }
    // a failed stream's batches must not be retired later
    void dropPending() { if (!pending.empty()) note(BR_DROPPED); pending.clear(); }

    // ---------------------------------------------------------------------------------------------- looks
    int oldestSlot() const { return (grpHead + 2 - grpCount) % 2; }
    // What the oldest group's snapshot says: the stream's rate, whether the tail has begun and how many slots it holds, and how many of the front
    // batches retire (in u_frameCount order, oldest first).
    int take(const Group& g, const ControlView& h) {
        lastDelta = h.nextJob >= lastNextJob ? h.nextJob - lastNextJob : 0; lastCheck = g.check;
        lastNextJob = h.nextJob;
        bool allDead = false;
        if (g.epoch == submitEpoch) {                              // nothing was submitted since the group was launched: its view of the tail is the stream's
            if (h.exhausted[(g.iterEnd + 3) & 3]) {                // the iteration after the group reads the queue: its count is exact (and only falls from there)
                draining = true;
                launched = (g.iterEnd & 1) ? h.qCount32 : h.qCount0;
                allDead = launched == 0;
            } else if (h.nextJob >= streamJobs) {
                draining = true;                                   // jobs just ran out; the queue starts within two iterations
            }
        } else note(BR_STALE_EPOCH);
        if (allDead) { note(BR_ALL_DEAD); return (int)pending.size(); }
        if (!g.nScan || pending.empty()) return 0;
        if (pending.front().f0 != g.scanF0) { note(BR_SCAN_MOVED); return 0; }      // the scan saw batches that have retired since
        int n = 0;
        while (n < g.nScan && n < (int)pending.size() && !h.busy[n]) n++;
        if (n > 0 && n < g.nScan) note(BR_SCAN_PARTIAL);
        return n;
    }
    // The oldest group in flight, once its snapshot has landed (wait = false: only if it already has).  1 = looked at, 0 = not ready yet, < 0 = PT_ERR_*.
    // discard: nothing to learn from it (it ran over a dead pool, or for a stream that has ended)
    template <class Dev> int lookAtOldest(Dev& dev, bool wait, bool discard) {
        const Group g = grp[oldestSlot()];
        ControlView h;
        const int r = dev.landed(oldestSlot(), g.seq, wait, h);
        if (r <= 0) return r;
        grpCount--;
        if (g.nScan) scanInFlight = false;
        inflightPredicted = std::max<int64_t>(0, inflightPredicted - g.predicted);
        if (discard) { note(BR_DISCARDED); return 1; }
        for (int n = take(g, h); n > 0; n--) {
            const StreamEntry e = pending.front();
            pending.pop_front();
            if (const int rc = dev.retire(e)) return rc;
        }
        return 1;
    }
    template <class Dev> int drainGroups(Dev& dev, bool discard) {
        while (grpCount > 0) { const int r = lookAtOldest(dev, true, discard); if (r < 0) return r; }
        return 0;
    }

    // ---------------------------------------------------------------------------------------------- groups
    int64_t backlog() const { return (int64_t)streamJobs - (int64_t)lastNextJob - inflightPredicted; }      // jobs not handed out as of the last look, less what the groups in flight take
    bool satisfied(PumpUntil until, int arg) const {
        if (pending.empty()) return true;
        switch (until) {
            case PUMP_IDLE: return false;
            case PUMP_ISSUED: return draining || backlog() <= std::max<int64_t>((int64_t)lastDelta, (int64_t)arg);
            case PUMP_IMAGE: for (const auto& e : pending) if (e.image == arg) return false; return true;
            case PUMP_RING: return (int)(streamFrames - pending.front().f0) <= arg;
        }
        return true;
    }
    // The device runs the schedule by itself: slots pull jobs while there are any; from the iteration after the first empty pull on, every shading
    // launch packs the surviving slots into a dense queue for the next iteration (Control::exhausted).  The host only looks: while jobs remain the
    // end is at least one whole job (>= SAMPLE_RES iterations) away, so a group is 24 iterations, in the tail 8; each look shrinks the launch grids
    // to the live count.
    struct GroupPlan { int n; int64_t predicted; };      // iterations, and the jobs they are expected to hand out
    GroupPlan nextGroup(bool kick, PumpUntil until, int arg) {
        int CHECK = draining ? 8 : PT_SCHED_GROUP;
        if (draining) note(BR_TAIL_GROUP);
        if (kick && lastDelta == 0) { CHECK = 4; note(BR_KICK_FIRST); }      // the first looks of a stream fed in small submissions come early: the pool grows with the backlog they report
        const int64_t perIter = std::max<int64_t>(1, (int64_t)lastDelta / std::max(1, lastCheck));      // jobs handed out per iteration at the last look
        if (until == PUMP_ISSUED && lastDelta > 0) {              // approach the end of the job supply without running into it
            const int64_t left0 = std::max<int64_t>(0, backlog());
            const int64_t left = left0 - (int64_t)lastDelta / 2 - (int64_t)arg;
            if (left > 0) { CHECK = (int)std::max<int64_t>(1, std::min<int64_t>(CHECK, left / perIter)); note(BR_ISSUED_LEFT); }
            // (two iterations' worth stay behind: later submissions sit BEHIND this group in the stream, and a pull that comes back empty sends the pool into its tail)
            else if (kick) { CHECK = (int)std::max<int64_t>(1, std::min<int64_t>(CHECK, std::max<int64_t>(left0, (int64_t)lastSubmitJobs) / perIter - 2)); note(BR_ISSUED_KICK); }
        }
        return GroupPlan{CHECK, lastDelta > 0 ? (int64_t)CHECK * perIter : 0};
    }
    // the oldest batches that have been handed out completely (as of the last look): which of them are still in flight?  n = 0: none to ask about
    SchedScan scanEnds() const {
        SchedScan ends{};
        for (const auto& e : pending) {
            if (ends.n == 8 || lastNextJob < e.jobEnd) break;
            ends.f[ends.n++] = e.f0 + (unsigned)e.nFrames;
        }
        return ends;
    }
    // One group: its iterations, a scan once the oldest batches have been handed out completely (one scan in flight at a time), the snapshot
    template <class Dev> int launchGroup(Dev& dev, const GroupPlan& p) {
        if (const int rc = dev.launchIterations(p.n, launched, iter)) return rc;
        iter = (int)(((unsigned)iter + (unsigned)p.n) & 0x3fffffffu);
        Group& g = grp[grpHead];
        g.check = p.n; g.iterEnd = iter; g.epoch = submitEpoch; g.nScan = 0;
        g.predicted = p.predicted; inflightPredicted += p.predicted;
        if (!scanInFlight) {
            const SchedScan ends = scanEnds();
            if (ends.n) {
                if (const int rc = dev.launchScan(ends)) return rc;
                g.nScan = ends.n; g.scanF0 = pending.front().f0; scanInFlight = true;
                if (ends.n == 8) note(BR_SCAN_EIGHT);
            }
        }
        if (++groupSeq == 0) groupSeq = 1;                         // (0 = "nothing has arrived")
        g.seq = groupSeq;
        if (const int rc = dev.launchSnapshot(grpHead, g.seq)) return rc;
        grpHead = (grpHead + 1) % 2; grpCount++;
        return 0;
    }
    // every job retires within itersPerJob iterations of being started, and a slot runs at most ceil(jobs / slots) jobs back to back: a pump that
    // exceeds this bound (x2) is a scheduler bug, not work
    uint64_t iterationBound(uint64_t itersPerJob) const {
        const uint64_t N = (uint64_t)poolActive;
        const uint64_t outstanding = (uint64_t)streamJobs - std::min<uint64_t>(lastNextJob, streamJobs) + N;
        return 2 * ((outstanding + N - 1) / N + 1) * itersPerJob + 64 + 48;
    }
    // *iters: the iterations launched, when the pump succeeds
    template <class Dev> int pump(Dev& dev, PumpUntil until, int arg, uint64_t* iters = nullptr) {
        if (pending.empty()) return drainGroups(dev, true);        // (groups launched before the last batch retired ran over a dead pool: nothing to learn from them)
        if (until == PUMP_IMAGE) note(BR_UNTIL_IMAGE);
        if (until == PUMP_RING) note(BR_UNTIL_RING);
        const uint64_t maxIters = iterationBound(dev.itersPerJob());
        uint64_t done = 0;
        int rc;
        bool kick = until == PUMP_ISSUED;                         // a submission always gets the GPU going: about as many iterations as consume what it added
        while (grpCount > 0 && (rc = lookAtOldest(dev, false, false)) != 0) if (rc < 0) return rc;      // whatever has finished since the last call
        for (;;) {
            const bool want = kick || !satisfied(until, arg);
            if (!want) break;
            if (done > maxIters) { note(BR_DID_NOT_DRAIN); return dev.didNotDrain(); }
            const int room = draining ? 1 : 2;                     // the tail is run look by look: every look shrinks the grids
            if (grpCount < room) {
                const GroupPlan p = nextGroup(kick, until, arg);
                if ((rc = launchGroup(dev, p))) return rc;
                done += (uint64_t)p.n; kick = false; continue;
            }
            if (kick) { kick = false; continue; }                 // two groups are on their way already: the submission rides behind them
            if ((rc = lookAtOldest(dev, true, false)) < 0) return rc;
        }
        if (iters) *iters += done;
        if (until != PUMP_ISSUED) return drainGroups(dev, pending.empty());      // synchronous callers leave nothing behind them
        return 0;
    }
    template <class Dev> int flush(Dev& dev, uint64_t* iters = nullptr) { return pending.empty() ? 0 : pump(dev, PUMP_IDLE, 0, iters); }

    // ---------------------------------------------------------------------------------------------- submission
    // the running stream can take the batch if nothing the kernels were launched with changes
    bool canJoin(const SubmitReq& q) {
        if (pending.empty()) return false;
        const SchedBranch why = q.sceneDirty ? BR_REFUSE_DIRTY : !q.sameInputs ? BR_REFUSE_INPUTS : q.ringFrames < q.wantRing ? BR_REFUSE_RING :
                                !q.sameContract ? BR_REFUSE_CONTRACT : (uint64_t)streamJobs + q.nJobs >= (1ull << 31) ? BR_REFUSE_JOBS : BR_JOIN;
        note(why);
        return why == BR_JOIN;
    }
    template <class Dev> int submit(Dev& dev, const SubmitReq& q, uint64_t* iters = nullptr) {
        int rc;
        bool join = canJoin(q);
        if (join && (int)(streamFrames - pending.front().f0) + q.nFrames > q.ringFrames) {
            if ((rc = pump(dev, PUMP_RING, q.ringFrames - q.nFrames, iters))) return rc;      // wait for ring rows
            join = !pending.empty();                               // the stream ended meanwhile: start over
            note(join ? BR_RING_WAIT : BR_RING_RESTART);
        } else if (!join) {
            if ((rc = flush(dev, iters))) return rc;
        }
        if (!join) {                                               // ---- a new stream
            note(BR_NEW_STREAM);
            if ((rc = dev.sceneReady())) return rc;
            poolActive = newStreamPool(q.nJobs, q.async, q.poolSlots);
            if ((rc = dev.openStream(poolActive)) || (rc = drainGroups(dev, true))) return rc;
            inflightPredicted = 0;
            streamFrames = 0; streamJobs = 0; lastNextJob = 0; lastDelta = 0; lastCheck = PT_SCHED_GROUP; iter = 0;
        }
        // a stream fed in small batches (the reference draws ONE frame per call) started with a small pool: let it grow with the backlog
        bool grown = false;
        if (join && q.async && q.poolSlots == 0) {
            const uint64_t outstanding = (uint64_t)std::max<int64_t>(0, (int64_t)streamJobs - (int64_t)std::min<uint64_t>(lastNextJob, streamJobs) - inflightPredicted) + q.nJobs;
            if (const size_t target = grownPool(outstanding, jobsPerImage, q.allocSlots, poolActive)) {
                if ((rc = dev.growPool(poolActive, (int)target))) return rc;
                poolActive = (int)target;
                grown = true;
            }
            note(grown ? BR_POOL_GROWN : BR_POOL_KEPT);
        }
        // ---- append
        const unsigned f0 = streamFrames;
        if ((rc = dev.appendJobs(f0, q.nFrames, (unsigned)q.nJobs, join ? (grown ? 2 : 0) : 1, poolActive))) return rc;
        streamFrames += (unsigned)q.nFrames; streamJobs += (unsigned)q.nJobs;
        lastSubmitJobs = q.nJobs; jobsThisImage += q.nJobs;
        pending.push_back(StreamEntry{streamJobs, f0, q.nFrames, q.firstFrame, q.image});
        draining = false; launched = (unsigned)poolActive;        // (if the pool had run dry, k_submit dropped the tail queue)
        submitEpoch++;                                            // the groups in flight were launched for another tail: their view of it no longer counts
        // asynchronous: come back while the backlog of jobs not yet handed out is below what keeps the largest pool fed (2^23 * 8/5)
        if (q.async) return pump(dev, PUMP_ISSUED, q.poolSlots == 0 ? 14000000 : 0, iters);
        return pump(dev, PUMP_IDLE, 0, iters);
    }
};

}  // namespace ptp
