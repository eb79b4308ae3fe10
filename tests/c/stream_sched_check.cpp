// stream_sched_check.cpp — the frame-stream scheduler (csrc/hip/pt_stream_sched.hpp) on the CPU: a stand-alone program that runs scripts of
// submissions against a deterministic model of the device and prints every action the scheduler asks of it (tests/test_stream_sched.py).
//
//   stream_sched_check SCRIPTS        one trace per script on stdout, nothing on stderr, exit 0
//
// THE MODEL DEVICE keeps the words of Control the host reads (nextJob, jobEnd, needRevive, exhausted[4], the two queue counts, busy[8]) and the pool
// as COHORTS: a cohort is a run of job ids [lo, hi) that were started in the same launch, on hi - lo slots, `age` iterations ago.  Slots have no
// identity beyond that: the pool of N slots holds the cohorts' slots and N - live dead ones.  Launches take effect in the order they are made, at once
// (the stream is in order, so what a snapshot holds does not depend on when the host gets to see it):
//   init                 k_init_control: every word 0, needRevive 1; the pool's memset: no cohort (every slot dead)
//   submit(add, mode, n) k_submit, word for word: the flags cleared (dry if one was up), nextJob pulled back to jobEnd if it had overshot (dry),
//                        jobEnd += add, needRevive = dry or mode 2; mode 1: needRevive = 2 and nextJob = min(n, add); both queue counts 0
//   revive(n)            k_revive: needRevive 0: nothing.  2: jobs [0, min(n, jobEnd)) start.  1: every dead slot of the n asks, nextJob += their number
//                        (it may overshoot jobEnd), the ids below jobEnd start
//   iteration(j, bound)  intersect + shade of iteration j: it reads its slots through queue j&1 iff exhausted[(j+3)&3], over at most `bound` slots (a
//                        bound below what is alive would lose slots: the model prints "lost"); the other queue's count is zeroed; with exhausted[j&3]
//                        up it raises exhausted[(j+1)&3] and writes the survivors' number as the other queue's count.  Every cohort ages by one; a job
//                        lives D iterations (never ends under "never 1"); the slots of finished jobs pull together: nextJob += their number, the ids
//                        below jobEnd start as a new cohort, the rest die, and an empty pull raises exhausted[(j+1)&3].  With exhausted[j&3] up nobody
//                        pulls (k_shade knows the supply is dry)
//   scan(ends)           the busy words zeroed, then k_scan_inflight: busy[k] = a live job's frame (job / pixels per frame) lies below ends.f[k] and
//                        not below ends.f[k-1]
//   snapshot(seq)        the words as they are now.  "eager": it has landed whenever the host asks.  "lazy": it lands only when the host waits for it
//                        (snapshots land in the order of their launches)
//
// A SCRIPT is a block of lines (the host side of each is what pt_stream_dev.hpp does around the scheduler: Host below):
//   script NAME
//   create PIXELS POOLSLOTS D eager|lazy IMAGES SEQ0      pixels per frame, pt_set_option 0 (0 = automatic), a job's life, landing, ring images, the
//                                                         group sequence number the context starts from
//   submit FIRSTFRAME NFRAMES ASYNC INPUTS DIRTY FAST     pt_render_batch(_async) under frame inputs number INPUTS, after a scene upload (DIRTY), under the
//                                                         relaxed contract (FAST)
//   next_image | finish_image AGE | flush
//   adaptive FIRSTFRAME NFRAMES N                         renderSelected over N list entries: flush, a synchronous submission, the queue dropped if it fails
//   never 0|1 | moments 0|1                               jobs started from here on never end; pt_guided's moments are recorded
//   seek_iter V                                           the iteration counter jumps to V (kept congruent mod 4: the queue parity and the flag words go on)
//   stale_scan                                            the scan in flight is made one about another front batch (its scanF0 + 1).  No sequence of calls
//                                                         gets there: between a scan's launch and its look only an older group without a scan is looked
//                                                         at, which retires nothing or, the pool dead, everything — and then the queue is empty until a new
//                                                         stream discards the groups in flight.  The guard is kept as the parent has it, and reached this way
// THE TRACE: "group" (its iterations, the bound, the first iteration's number, the jobs it is predicted to hand out), "scan", "snapshot" (sequence
// number, groups in flight before it, the tail flag, the scan's batch count and first frame), "look" (a snapshot the host has taken), "retire", "init",
// "submit" (k_submit's arguments: mode 1 new stream, 0 joined, 2 joined and the pool grown), and per script line "rc" with the ring rows waited for and
// the error.  After a script: "branches" — the decisions its scheduler took (SchedBranch bits).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include "../../pathtracer-0_amd/csrc/hip/pt_stream_sched.hpp"

using ptp::ControlView;

struct Model {
    unsigned ppf = 1; int D = 1; bool never = false, lazy = false;
    unsigned nextJob = 0, jobEnd = 0, needRevive = 0, exhausted[4] = {0, 0, 0, 0}, qCount[2] = {0, 0}, busy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    struct Cohort { unsigned lo, hi; int age; bool never; };
    std::vector<Cohort> pool;
    // the group being launched (printed with the host's words for it once its iterations are out), the snapshots not yet landed
    int grpLen = 0, grpIter = 0; unsigned grpBound = 0;
    struct HostGroup { int64_t predicted; int inflight; bool tail; int nScan; unsigned scanF0; };
    std::function<HostGroup()> hostGroup;
    std::deque<std::function<void()>> notLanded;

    unsigned live() const { unsigned n = 0; for (const auto& c : pool) n += c.hi - c.lo; return n; }
    void start(unsigned base, unsigned want) {                   // ids [base, base + want) are asked for: those below jobEnd start
        const unsigned got = base >= jobEnd ? 0u : std::min(want, jobEnd - base);
        if (got) pool.push_back(Cohort{base, base + got, 0, never});
    }
    void init(unsigned pixelsPerFrame) {
        ppf = pixelsPerFrame; nextJob = jobEnd = 0; needRevive = 1; qCount[0] = qCount[1] = 0; pool.clear();
        for (auto& e : exhausted) e = 0;
        for (auto& b : busy) b = 0;
        std::printf("init\n");
    }
    void submit(unsigned add, int mode, unsigned nSlots) {
        bool dry = false;
        for (auto& e : exhausted) { dry = dry || e != 0; e = 0; }
        if (nextJob > jobEnd) { nextJob = jobEnd; dry = true; }
        jobEnd += add;
        needRevive = (dry || mode == 2) ? 1u : 0u;
        if (mode == 1) { needRevive = 2u; nextJob = std::min(nSlots, add); }
        qCount[0] = qCount[1] = 0;
        std::printf("submit mode=%d jobs=%u slots=%u\n", mode, add, nSlots);
    }
    void revive(unsigned nSlots) {
        if (needRevive == 2u) start(0, nSlots);
        else if (needRevive == 1u) { const unsigned dead = nSlots - live(), base = nextJob; nextJob += dead; start(base, dead); }
    }
    void iteration(int j, unsigned bound) {
        if (grpLen++ == 0) { grpIter = j; grpBound = bound; }
        const bool queueIn = exhausted[(j + 3) & 3] != 0, writeQueue = exhausted[j & 3] != 0;
        if (live() > (queueIn ? std::min(qCount[j & 1], bound) : bound)) std::printf("lost iter=%d bound=%u live=%u\n", j, bound, live());
        qCount[(j + 1) & 1] = 0;
        if (writeQueue) exhausted[(j + 1) & 3] = 1;
        unsigned done = 0;
        std::vector<Cohort> keep;
        for (auto c : pool) {
            c.age++;
            if (!c.never && c.age >= D) done += c.hi - c.lo; else keep.push_back(c);
        }
        pool.swap(keep);
        if (done && !writeQueue) {
            const unsigned base = nextJob;
            nextJob += done;
            if (base + done > jobEnd) exhausted[(j + 1) & 3] = 1;
            start(base, done);
        }
        if (writeQueue) qCount[(j + 1) & 1] = live();
    }
    void flushGroup(const HostGroup& h) {
        if (grpLen) std::printf("group n=%d launched=%u iter=%d predicted=%" PRId64 "\n", grpLen, grpBound, grpIter, h.predicted);
        grpLen = 0;
    }
    void scan(const unsigned* f, int n) {
        flushGroup(hostGroup());
        for (auto& b : busy) b = 0;
        for (const auto& c : pool) {
            const unsigned fLo = c.lo / ppf, fHi = (c.hi - 1) / ppf;
            for (int k = 0; k < n; k++) if (fLo < f[k] && (k == 0 || fHi >= f[k - 1])) busy[k] = 1;
        }
        std::printf("scan n=%d ends=", n);
        for (int k = 0; k < n; k++) std::printf("%s%u", k ? "," : "", f[k]);
        std::printf("\n");
    }
    // deliver: the host's copy of the words, then the stamp
    void snapshot(unsigned seq, const std::function<void(const ControlView&)>& deliver) {
        const HostGroup h = hostGroup();
        flushGroup(h);
        ControlView v;
        v.nextJob = nextJob; v.qCount0 = qCount[0]; v.qCount32 = qCount[1];
        for (int k = 0; k < 4; k++) v.exhausted[k] = exhausted[k];
        for (int k = 0; k < 8; k++) v.busy[k] = busy[k];
        if (h.nScan) std::printf("snapshot seq=%u inflight=%d tail=%d scan=%d@%u\n", seq, h.inflight, (int)h.tail, h.nScan, h.scanF0);
        else std::printf("snapshot seq=%u inflight=%d tail=%d\n", seq, h.inflight, (int)h.tail);
        if (lazy) notLanded.push_back([deliver, v] { deliver(v); }); else deliver(v);
    }
    void waited() { if (!notLanded.empty()) { notLanded.front()(); notLanded.pop_front(); } }
    void looked(unsigned seq) { std::printf("look seq=%u\n", seq); }
    void retired(unsigned f0, int nFrames, int firstFrame, int image, const char* kind) {
        std::printf("retire f0=%u frames=%d first=%d image=%d %s\n", f0, nFrames, firstFrame, image, kind);
    }
};

// What a script needs of a context; Host below is the one over the scheduler of pt_stream_sched.hpp
struct Create { unsigned ppf; int poolSlots, D; bool lazy; int images; unsigned seq0; };

struct Host {
    Model m; ptp::StreamSched sched;
    int images, curImage = 0, ringFrames = 0, allocSlots = 0, poolSlots;
    unsigned nLocal; bool sceneDirty = true, fastContract = false, streamFast = false, recordMoments = false, adaptOn = false;
    int inputs = 0, streamInputs = -1, adaptN = 0;
    int ringWaited = -1; std::string error;

    // the device side of the scheduler: the model
    struct Dev {
        Host& h; int wantRing = 0, capacity = 0;
        ControlView view[2]; unsigned stamp[2] = {0, 0};
        explicit Dev(Host& host) : h(host) {}
        int launchIterations(int n, unsigned launched, int iter) { for (int k = 0; k < n; k++) h.m.iteration((iter + k) & 0x3fffffff, launched); return 0; }
        int launchScan(const ptp::SchedScan& e) { h.m.scan(e.f, e.n); return 0; }
        int launchSnapshot(int slot, unsigned seq) {
            stamp[slot] = 0;
            h.m.snapshot(seq, [this, slot, seq](const ControlView& v) { view[slot] = v; stamp[slot] = seq; });
            return 0;
        }
        int landed(int slot, unsigned seq, bool wait, ControlView& v) {
            if (stamp[slot] != seq) {
                if (!wait) return 0;
                h.m.waited();
                if (stamp[slot] != seq) { h.error = "a snapshot never arrived"; return -3; }
            }
            h.m.looked(seq);
            v = view[slot];
            return 1;
        }
        int retire(const ptp::StreamEntry& e) {
            h.m.retired(e.f0, e.nFrames, e.firstFrame, e.image, h.adaptOn ? "adaptive" : h.recordMoments && e.image == h.curImage ? "moments" : "plain");
            return 0;
        }
        uint64_t itersPerJob() const { return (uint64_t)h.m.D + 1; }
        int didNotDrain() { h.error = "did not drain"; return -3; }
        int sceneReady() { h.sceneDirty = false; return 0; }
        int openStream(int pool) {
            h.allocSlots = std::max(h.allocSlots, std::max(capacity, pool));
            h.ringFrames = std::max(h.ringFrames, wantRing);
            h.streamInputs = h.inputs; h.streamFast = h.fastContract;
            h.m.init(h.adaptOn ? (unsigned)h.adaptN : h.nLocal);
            return 0;
        }
        int growPool(int, int) { return 0; }
        int appendJobs(unsigned, int, unsigned nJobs, int mode, int pool) { h.m.submit(nJobs, mode, (unsigned)pool); h.m.revive((unsigned)pool); return 0; }
    };
    Dev dev{*this};

    explicit Host(const Create& c) : images(c.images), poolSlots(c.poolSlots), nLocal(c.ppf) {
        m.D = c.D; m.lazy = c.lazy; sched.groupSeq = c.seq0;
        m.hostGroup = [this] {
            const ptp::StreamSched::Group& g = sched.grp[sched.grpHead];
            return Model::HostGroup{g.predicted, sched.grpCount, sched.draining, g.nScan, g.scanF0};
        };
    }
    int pump(ptp::PumpUntil until, int arg) { return sched.pump(dev, until, arg); }
    int flush() { return sched.flush(dev); }
    int submit(int firstFrame, int nFrames, bool async, int in, bool dirty, bool fast) {      // submitBatch
        inputs = in; sceneDirty = sceneDirty || dirty; fastContract = fast;
        const uint64_t nJobs = (uint64_t)(adaptOn ? (unsigned)adaptN : nLocal) * (uint64_t)nFrames;
        if (nJobs >= (1ull << 31)) { error = "batch too large"; return -1; }
        ptp::SubmitReq q;
        q.firstFrame = firstFrame; q.nFrames = nFrames; q.image = curImage; q.nJobs = nJobs; q.async = async;
        q.sceneDirty = sceneDirty; q.sameInputs = inputs == streamInputs; q.sameContract = streamFast == fastContract;
        q.ringFrames = ringFrames; q.wantRing = ptp::ringRows(nFrames, async, (size_t)nLocal * 16, images);
        q.poolSlots = poolSlots; q.allocSlots = allocSlots;
        dev.wantRing = q.wantRing; dev.capacity = ptp::newStreamCapacity(async, poolSlots);
        const uint64_t ring = (1ull << ptp::BR_RING_WAIT) | (1ull << ptp::BR_RING_RESTART), before = sched.reached;
        sched.reached &= ~ring;
        const int rc = sched.submit(dev, q);
        if (sched.reached & ring) ringWaited = q.ringFrames - nFrames;
        sched.reached |= before;
        return rc;
    }
    int nextImage() {                                            // pt_next_image
        const int next = (curImage + 1) % images;
        if (const int rc = pump(ptp::PUMP_IMAGE, next)) return rc;
        curImage = next;
        sched.imageTurned();
        return 0;
    }
    int finishImage(int age) { return pump(ptp::PUMP_IMAGE, (curImage + images - age) % images); }
    int adaptive(int firstFrame, int nFrames, int n) {           // renderSelected
        if (const int rc = flush()) return rc;
        adaptOn = true; adaptN = n;
        const int rc = submit(firstFrame, nFrames, false, inputs, false, fastContract);
        if (rc) sched.dropPending();
        adaptOn = false; adaptN = 0;
        return rc;
    }
    void seekIter(int v) { sched.iter = (v & ~3) | (sched.iter & 3); }
    void staleScan() { for (auto& g : sched.grp) if (g.nScan) g.scanF0++; }
    uint64_t reached() const { return sched.reached; }
};

template <class H> int runScripts(const char* path) {
    std::ifstream in(path);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    H* h = nullptr;
    auto endScript = [&] { if (h) { std::printf("branches %" PRIx64 "\n", (uint64_t)h->reached()); delete h; h = nullptr; } };
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string op, s;
        if (!(ss >> op)) continue;
        long long a[6] = {0, 0, 0, 0, 0, 0};
        if (op == "script") { endScript(); ss >> s; std::printf("== %s\n", s.c_str()); continue; }
        if (op == "create") {
            ss >> a[0] >> a[1] >> a[2] >> s >> a[3] >> a[4];
            h = new H(Create{(unsigned)a[0], (int)a[1], (int)a[2], s == "lazy", (int)a[3], (unsigned)a[4]});
            continue;
        }
        if (!h) { std::fprintf(stderr, "%s before create\n", op.c_str()); return 2; }
        for (auto& v : a) ss >> v;
        h->ringWaited = -1; h->error.clear();
        int rc = 0;
        if (op == "submit") rc = h->submit((int)a[0], (int)a[1], a[2] != 0, (int)a[3], a[4] != 0, a[5] != 0);
        else if (op == "next_image") rc = h->nextImage();
        else if (op == "finish_image") rc = h->finishImage((int)a[0]);
        else if (op == "flush") rc = h->flush();
        else if (op == "adaptive") rc = h->adaptive((int)a[0], (int)a[1], (int)a[2]);
        else if (op == "never") { h->m.never = a[0] != 0; continue; }
        else if (op == "moments") { h->recordMoments = a[0] != 0; continue; }
        else if (op == "seek_iter") { h->seekIter((int)a[0]); continue; }
        else if (op == "stale_scan") { h->staleScan(); continue; }
        else { std::fprintf(stderr, "unknown line: %s\n", line.c_str()); return 2; }
        std::printf("rc=%d", rc);
        if (h->ringWaited >= 0) std::printf(" ringwait=%d", h->ringWaited);
        if (!h->error.empty()) std::printf(" error=%s", h->error.c_str());
        std::printf("\n");
    }
    endScript();
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s SCRIPTS\n", argv[0]); return 2; }
    return runScripts<Host>(argv[1]);
}
