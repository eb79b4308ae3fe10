// group_plan_check.cpp — csrc/hip/pt_group_plan.hpp on the CPU (tests/test_group_plan.py builds this twice with g++: plain and under the address /
// undefined-behaviour sanitizers).
//   group_plan_check shard <dir> <W> <H> <total> <first> <count> <extra> ...    per group of six numbers: the maps of shards first .. first+count-1 of total,
//                                      shardSlots + extra slots each, as int32 into <dir>/<k>.bin, and one line "maps <k> slots=<n>"
//   group_plan_check shapes            every refusal of the header provoked, and the accepted shapes: "refusal <name> rc=<code> <text>", and for an
//                                      accepted one "shape <name> runs=<device>:<first>:<count>,... rccl= virtual= sod=<per stream>,... warn="
//   group_plan_check gather            the gather of every accepted shape, in every transport it allows, at 256 and 768 slots per shard, executed on
//                                      host arrays: one line "gather <name> mode= slots= ..." each, then "<n> failures"
#include "../../pathtracer-0_amd/csrc/hip/pt_group_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

int failures = 0;
void require(bool ok, const char* what) { if (!ok) { std::printf("FAILED %s\n", what); failures++; } }

int shard(int argc, char** argv) {
    const std::string dir = argv[2];
    for (int a = 3, k = 0; a + 6 <= argc; a += 6, k++) {
        const int W = std::atoi(argv[a]), H = std::atoi(argv[a + 1]), total = std::atoi(argv[a + 2]), first = std::atoi(argv[a + 3]), count = std::atoi(argv[a + 4]);
        const size_t nSlots = ptp::shardSlots(W, H, total) + (size_t)std::atoi(argv[a + 5]);
        std::vector<int32_t> maps;
        const ptp::Refused no = ptp::shardMaps(W, H, first, count, total, nSlots, maps);
        if (no.code) { std::printf("refused rc=%d %s\n", no.code, no.msg.c_str()); return 1; }
        std::FILE* f = std::fopen((dir + "/" + std::to_string(k) + ".bin").c_str(), "wb");
        if (!f) { std::printf("cannot write into %s\n", dir.c_str()); return 1; }
        const bool ok = maps.empty() || std::fwrite(maps.data(), 4, maps.size(), f) == maps.size();
        if (std::fclose(f) != 0 || !ok) { std::printf("short write into %s\n", dir.c_str()); return 1; }
        std::printf("maps %d slots=%zu\n", k, nSlots);
    }
    return 0;
}

// a call of pt_create_multi_part as the plan sees it
struct Call {
    const char* name; std::vector<int> devices; int nDev; int k; bool force;      // k: PT_MULTI_VIRTUAL_DEVICES
    int first = 0, total = -1;                                                    // total -1: the whole image (pt_create_multi)
    bool hwQueues = true, out = true, nullDevices = false; int n = -1, W = 64, H = 48;      // n -1: devices.size()
    int rc = 0; const char* text = "";
};
std::vector<int> zeros(int n) { return std::vector<int>((size_t)n, 0); }

std::vector<Call> calls() {
    const char* const ARG = "pt_create_multi: bad argument";
    const char* const ADJACENT = "pt_create_multi: the entries of one device must be adjacent ({0,0,1,1}, not {0,1,0,1})";
    const char* const EQUAL = "pt_create_multi: every device must be listed the same number of times";
    const char* const RANGE = "pt_create_multi: HIP device index out of range";
    const char* const VIRTUAL = "PT_MULTI_VIRTUAL_DEVICES=k needs ONE device listed a multiple of k times";
    std::vector<Call> c = {
        {"one", {0}, 1, 0, false},
        {"two", {0, 0}, 1, 0, false},
        {"three", {0, 0, 0}, 1, 0, false},
        {"devices3", {0, 1, 2}, 8, 0, false},
        {"pairs", {0, 0, 1, 1}, 8, 0, false},
        {"virtual4k2", zeros(4), 1, 2, false},
        {"virtual16k8", zeros(16), 1, 8, false},
        {"forced", {0}, 1, 0, true},
        {"interleaved", {0, 1, 0, 1}, 8, 0, false},
        {"uneven", {0, 0, 1}, 8, 0, false},
        {"virtual3k2", zeros(3), 1, 2, false},
        {"virtual_two_devices", {0, 1}, 8, 2, false},
        {"device_beyond", {0, 99}, 1, 0, false},
        {"device_negative", {-1}, 1, 0, false},
        {"part_beyond", {0, 0}, 1, 0, false},
        // beyond the issue's list: the other terms of the argument check, what is NOT refused, and the warning
        {"null_out", {0}, 1, 0, false}, {"null_devices", {0}, 1, 0, false}, {"none", {0}, 1, 0, false}, {"too_many", zeros(65), 1, 0, false},
        {"width", {0}, 1, 0, false}, {"height", {0}, 1, 0, false}, {"first_negative", {0}, 1, 0, false}, {"total_short", {0, 0}, 1, 0, false},
        {"part", {0, 0}, 1, 0, false}, {"virtual_k1", {0, 0}, 1, 1, false}, {"virtual_negative", {0, 0}, 1, -3, false},
        {"two_no_queues", {0, 0}, 1, 0, false}, {"devices3_no_queues", {0, 1, 2}, 8, 0, false}, {"sixtyfour", zeros(64), 1, 0, false},
    };
    auto at = [&](const char* name) -> Call& { for (Call& x : c) if (!std::strcmp(x.name, name)) return x; std::abort(); };
    auto refuse = [&](const char* name, int rc, const char* text) { at(name).rc = rc; at(name).text = text; };
    refuse("interleaved", PT_ERR_ARG, ADJACENT); refuse("uneven", PT_ERR_ARG, EQUAL);
    refuse("virtual3k2", PT_ERR_ARG, VIRTUAL); refuse("virtual_two_devices", PT_ERR_ARG, VIRTUAL);
    refuse("device_beyond", PT_ERR_NO_DEVICE, RANGE); refuse("device_negative", PT_ERR_NO_DEVICE, RANGE);
    at("part_beyond").first = 3; at("part_beyond").total = 4; refuse("part_beyond", PT_ERR_ARG, ARG);
    at("null_out").out = false; at("null_devices").nullDevices = true; at("none").n = 0; at("width").W = 0; at("height").H = 0; at("first_negative").first = -1;
    at("first_negative").total = 4; at("total_short").total = 1;
    for (const char* n : {"null_out", "null_devices", "none", "too_many", "width", "height", "first_negative", "total_short"}) refuse(n, PT_ERR_ARG, ARG);
    at("part").first = 2; at("part").total = 4;
    at("two_no_queues").hwQueues = false; at("devices3_no_queues").hwQueues = false;
    return c;
}

// the call through the two halves of the plan, in the entry point's order (the question for a HIP device lies between them)
ptp::Refused plan(const Call& c, ptp::GroupShape& g) {
    const int n = c.n >= 0 ? c.n : (int)c.devices.size();
    const int* devices = c.nullDevices ? nullptr : c.devices.data();
    const ptp::Refused no = ptp::checkGroupArgs(c.out, devices, n, c.W, c.H, c.first, c.total >= 0 ? c.total : n);
    if (no.code) return no;
    ptp::GroupEnv env; env.virtualDevices = c.k; env.forceRccl = c.force; env.hwQueuesSet = c.hwQueues;
    return ptp::planGroup(devices, n, c.nDev, env, g);
}

int shapes() {
    for (const Call& c : calls()) {
        ptp::GroupShape g;
        const ptp::Refused no = plan(c, g);
        std::printf("refusal %s rc=%d %s\n", c.name, no.code, no.msg.c_str());
        require(no.code == c.rc && no.msg == c.text, c.name);
        if (no.code) continue;
        std::printf("shape %s runs=", c.name);
        for (size_t r = 0; r < g.runs.size(); r++) std::printf("%s%d:%d:%d", r ? "," : "", g.runs[r].device, g.runs[r].first, g.runs[r].count);
        std::printf(" rccl=%d virtual=%d sod=", (int)g.useRccl, (int)g.virtualDevices);
        for (size_t i = 0; i < g.streamsOnDevice.size(); i++) std::printf("%s%d", i ? "," : "", g.streamsOnDevice[i]);
        std::printf(" warn=%d\n", (int)g.warnHwQueues);
        // the runs cover the streams in order, each on one device
        int next = 0;
        for (const ptp::GroupRun& r : g.runs) {
            require(r.first == next && r.count >= 1, "the runs follow each other");
            for (int j = 0; j < r.count; j++) require(c.devices[(size_t)(r.first + j)] == r.device, "a run's streams are on its device");
            next += r.count;
        }
        require(next == (int)c.devices.size() && g.streamsOnDevice.size() == c.devices.size(), "the runs cover every stream");
    }
    // a map that does not fit: 100 x 37 in three shards, shard 0 holds seven tiles
    int32_t small[256];
    const ptp::Refused no = ptp::shardMap(100, 37, 0, 3, small, 256);
    std::printf("refusal map_too_small rc=%d %s\n", no.code, no.msg.c_str());
    require(no.code == PT_ERR_ARG, "map_too_small");
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}

// ---- the gather, executed.  A buffer is floats, four per accumulator slot; shard i's image holds the tag i * TAG + f in float f (exact in a float)
constexpr int TAG = 4096;
enum Transport { T_COPIES, T_RCCL, T_VIRTUAL };

void gatherOne(const Call& c, const ptp::GroupShape& g, Transport mode, size_t nSlots) {
    const int n = (int)c.devices.size(), total = c.total >= 0 ? c.total : n;
    const bool useRccl = mode != T_COPIES;
    const ptp::GatherPlan p = ptp::planGather(g.runs, n, total, nSlots, useRccl, mode == T_VIRTUAL);
    std::vector<std::vector<float>> img((size_t)n), staging(g.runs.size());
    for (int i = 0; i < n; i++) { img[(size_t)i].resize(nSlots * 4); for (size_t f = 0; f < nSlots * 4; f++) img[(size_t)i][f] = (float)(i * TAG + (int)f); }
    std::vector<float> gathered(p.totalSlots * 4, -1.0f);
    require(p.totalSlots == nSlots * (size_t)n && p.untile == (total == n), "total slots, and un-tiled exactly when the group holds the whole image");
    require(p.stagingBytes.size() == g.runs.size(), "one staging size per run");
    for (size_t r = 0; r < g.runs.size(); r++) {
        require(p.stagingBytes[r] == (useRccl && g.runs[r].count > 1 ? (size_t)g.runs[r].count * nSlots * 16 : 0), "staging: only a run of several streams, only under the collective");
        staging[r].assign(p.stagingBytes[r] / 4, -1.0f);
    }
    // the copies, each run's release behind them
    auto runOf = [&](int shard) { for (size_t r = 0; r < g.runs.size(); r++) if (shard >= g.runs[r].first && shard < g.runs[r].first + g.runs[r].count) return (int)r; return -1; };
    size_t ci = 0, li = 0; int waits = 0;
    for (size_t r = 0; r < g.runs.size(); r++) {
        const ptp::GroupRun& run = g.runs[r];
        int copied = 0;
        for (; ci < p.copies.size() && p.copies[ci].run == (int)r; ci++, copied++) {
            const ptp::GatherCopy& k = p.copies[ci];
            require(k.shard >= 0 && k.shard < n && runOf(k.shard) == (int)r && k.lead == run.first, "a copy stays in its run and goes on the run's lead stream");
            require(k.waitFor == (k.shard == k.lead ? -1 : k.shard), "a copy from another stream's shard waits for that shard's event, the lead's own for none");
            require(k.toStaging == useRccl, "the destination is the staging block exactly under the collective");
            waits += k.waitFor >= 0;
            std::vector<float>& dst = k.toStaging ? staging[r] : gathered;
            const bool fits = (k.dstSlot + nSlots) * 4 <= dst.size();
            require(fits, "a copy stays inside its destination");
            if (fits && k.shard >= 0 && k.shard < n) std::memcpy(dst.data() + k.dstSlot * 4, img[(size_t)k.shard].data(), nSlots * 16);
        }
        require(copied == (useRccl && run.count == 1 ? 0 : run.count), "every shard of a run is copied once; a one-stream run under the collective not at all");
        const bool released = li < p.releases.size() && p.releases[li].run == (int)r;
        require(released == (copied > 0 && run.count > 1), "a run of several streams has one release behind its copies");
        if (released) {
            const ptp::GatherRelease& rel = p.releases[li++];
            require(rel.lead == run.first && rel.firstWaiter == run.first + 1 && rel.waiters == run.count - 1, "the lead records, every other stream of the run waits");
        }
    }
    require(ci == p.copies.size() && li == p.releases.size(), "no copy or release outside the runs' order");
    // the sends, by the contract of ncclGather as pt_multi.hpp states it: rank r's `count` elements land at r * count of the root's receive buffer,
    // no other rank's receive buffer is written; or, on virtual devices, as copies to the offsets the plan states
    require(p.sends.size() == (useRccl ? g.runs.size() : 0), "one send per run under the collective, none without");
    if (!useRccl) require(g.runs.size() == 1, "without the collective there is one run");
    int fromImage = 0;
    for (size_t r = 0; r < p.sends.size(); r++) {
        const ptp::GatherSend& s = p.sends[r];
        const ptp::GroupRun& run = g.runs[r];
        require(s.run == (int)r && s.shard == run.first, "rank r is run r, on its lead stream");
        require(s.fromImage == (run.count == 1) && (s.fromImage || p.stagingBytes[r] > 0), "a one-stream run sends its image, the others their staging block");
        require(s.floats == (size_t)run.count * nSlots * 4 && s.floats == p.sends[0].floats, "every rank sends the same count: its run's floats");
        require(s.recvIsGathered == (r == 0), "the receive side is the gathered buffer on the root, the send buffer elsewhere");
        require(s.rootWaits == (mode == T_VIRTUAL && r > 0), "the root waits for the other runs' blocks when they come by device copies");
        fromImage += s.fromImage;
        const std::vector<float>& send = s.fromImage ? img[(size_t)s.shard] : staging[r];
        const size_t at = mode == T_VIRTUAL ? s.rootOffset : r * s.floats;
        const bool fits = s.floats <= send.size() && at + s.floats <= gathered.size();
        require(fits, "a send stays inside its buffers");
        if (fits) std::memcpy(gathered.data() + at, send.data(), s.floats * 4);
    }
    // the gathered buffer: the images, shard-major
    bool concat = true;
    for (int i = 0; i < n; i++) concat = concat && !std::memcmp(gathered.data() + (size_t)i * nSlots * 4, img[(size_t)i].data(), nSlots * 16);
    require(concat, "the gathered buffer is the shard-major concatenation of the images");
    for (const auto& b : img) for (size_t f = 0; f < b.size(); f += 997) require(b[f] == (float)((&b - img.data()) * TAG + (int)f), "the images are only read");
    // un-tiled through the maps: pixel p holds the tag of p's owner.  An image of one tile row of `total` tiles per 256 slots, with odd edges
    const int W = 32 * total - 5, H = (int)(nSlots / 256) * 8 - 1, ntx = (W + 31) / 32;
    std::vector<int32_t> maps;
    require(ptp::shardMaps(W, H, c.first, n, total, nSlots, maps).code == 0, "the maps fit the slots");
    std::vector<float> full((size_t)W * H, -1.0f);
    for (size_t k = 0; k < maps.size(); k++) if (maps[k] >= 0) { require(full[(size_t)maps[k]] == -1.0f, "a pixel is written once"); full[(size_t)maps[k]] = gathered[4 * k]; }
    bool owners = true;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const int owner = ((y / 8) * ntx + x / 32) % total, i = owner - c.first;
            const float v = full[(size_t)y * W + x];
            owners = owners && (i >= 0 && i < n ? (int)v / TAG == i && (int)v % 4 == 0 : v == -1.0f);
        }
    require(owners, "un-tiled, every pixel of the group holds its owner's tag and no other pixel is written");
    std::printf("gather %s mode=%s slots=%zu runs=%zu staging=", c.name, mode == T_COPIES ? "copies" : mode == T_RCCL ? "rccl" : "virtual", nSlots, g.runs.size());
    for (size_t r = 0; r < p.stagingBytes.size(); r++) std::printf("%s%zu", r ? "," : "", p.stagingBytes[r]);
    std::printf(" copies=%zu waits=%d releases=%zu sends=%zu fromImage=%d total=%zu untile=%d\n", p.copies.size(), waits, p.releases.size(), p.sends.size(), fromImage,
                p.totalSlots, (int)p.untile);
}

int gather() {
    for (const Call& c : calls()) {
        ptp::GroupShape g;
        if (c.rc || plan(c, g).code) continue;
        for (size_t nSlots : {(size_t)256, (size_t)768}) {
            // one run: device copies alone, or the collective forced onto it; several: the collective, by RCCL or (virtual devices) by copies
            if (g.runs.size() == 1) { gatherOne(c, g, T_COPIES, nSlots); gatherOne(c, g, T_RCCL, nSlots); }
            else { gatherOne(c, g, T_RCCL, nSlots); if (g.virtualDevices) gatherOne(c, g, T_VIRTUAL, nSlots); }
            require(g.runs.size() == 1 ? g.useRccl == c.force : g.useRccl, "the shape asks for the collective exactly with several runs, or forced");
        }
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 9 && !std::strcmp(argv[1], "shard") && (argc - 3) % 6 == 0) return shard(argc, argv);
    if (argc == 2 && !std::strcmp(argv[1], "shapes")) return shapes();
    if (argc == 2 && !std::strcmp(argv[1], "gather")) return gather();
    std::printf("usage: group_plan_check shard <dir> (<W> <H> <total> <first> <count> <extra>)... | shapes | gather\n");
    return 2;
}
