// launch_plan_check.cpp — runs the launch planning of csrc/hip/pt_launch_plan.hpp on the CPU over a file of cases and prints every field of what it
// decided, one line per case (tests/test_launch_plan.py builds it with g++, once plain and once under the host sanitizers).
//
// A case is one line: a letter and integers.
//   E  nNodes nTriRecs numObj stackDepth stackMode asmNodeStride ellipMaps asmEligible ldsNodes ldsTris        (the scene as built)
//      extendMode extendTpb extendCacheBytes extendCacheSet extendMaxBlocksPerCU asmTpb asmLoop noneMin noneMinSet countStats      (the options)
//      numCUs streamsOnDevice part partEighths                                                                  (the device)
//      launched probes fast                                                                                     (the call)          -> planExtend
//   N  nJobs async poolSlots                              -> newStreamPool, newStreamCapacity
//   G  outstanding jobsPerImage allocSlots poolActive     -> grownPool
//   R  nFrames async rowBytes images                      -> ringRows
//   M  d                                                  -> magicDiv
#include "../../pathtracer-0_amd/csrc/hip/pt_launch_plan.hpp"

#include <cstdio>
#include <cstdlib>

namespace {

using namespace ptp;

void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "case file: %s\n", what); std::exit(2); } }
long long rd(FILE* f) { long long v; need(std::fscanf(f, "%lld", &v) == 1, "truncated case"); return v; }

}  // namespace

int main(int argc, char** argv) {
    need(argc == 2, "usage: launch_plan_check FILE");
    FILE* f = std::fopen(argv[1], "r");
    need(f != nullptr, "cannot open");
    char kind;
    while (std::fscanf(f, " %c", &kind) == 1) {
        if (kind == 'E') {
            PlanScene s; PlanOptions o; PlanDevice dv; PlanCall call;
            s.nNodes = (int)rd(f); s.nTriRecs = (int)rd(f); s.numObj = (int)rd(f); s.stackDepth = (int)rd(f); s.stackMode = (int)rd(f); s.asmNodeStride = (int)rd(f);
            s.ellipMaps = rd(f) != 0; s.asmEligible = rd(f) != 0; s.ldsNodes = (int)rd(f); s.ldsTris = (int)rd(f);
            o.extendMode = (int)rd(f); o.extendTpb = (int)rd(f); o.extendCacheBytes = (int)rd(f); o.extendCacheSet = rd(f) != 0; o.extendMaxBlocksPerCU = (int)rd(f);
            o.asmTpb = (int)rd(f); o.asmLoop = (int)rd(f); o.noneMin = (int)rd(f); o.noneMinSet = rd(f) != 0; o.countStats = rd(f) != 0;
            dv.numCUs = (int)rd(f); dv.streamsOnDevice = (int)rd(f); dv.part = rd(f) != 0; dv.partEighths = (int)rd(f);
            call.launched = (unsigned)rd(f); call.probes = rd(f) != 0; call.fast = rd(f) != 0;
            const ExtendPlan p = planExtend(s, o, dv, call);
            std::printf("kernel=%d tpb=%d grid=%d lds=%zu ldsNodes=%d ldsTris=%d noneMin=%d variant=%d mode=%u nWaves=%u divM=%u divS=%u rare=%d nObjLds=%d perCU=%d\n", p.kernel, p.tpb,
                        p.grid, p.lds, p.ldsNodes, p.ldsTris, p.noneMin, p.variant, p.mode, p.nWaves, p.divM, p.divS, (int)p.rare, p.nObjLds, p.perCU);
        } else if (kind == 'N') {
            const size_t nJobs = (size_t)rd(f); const bool async = rd(f) != 0; const int poolSlots = (int)rd(f);
            std::printf("pool=%d capacity=%d\n", newStreamPool(nJobs, async, poolSlots), newStreamCapacity(async, poolSlots));
        } else if (kind == 'G') {
            const uint64_t outstanding = (uint64_t)rd(f), jobsPerImage = (uint64_t)rd(f); const int allocSlots = (int)rd(f), poolActive = (int)rd(f);
            std::printf("grown=%zu\n", grownPool(outstanding, jobsPerImage, allocSlots, poolActive));
        } else if (kind == 'R') {
            const int nFrames = (int)rd(f); const bool async = rd(f) != 0; const size_t rowBytes = (size_t)rd(f); const int images = (int)rd(f);
            std::printf("ring=%d\n", ringRows(nFrames, async, rowBytes, images));
        } else if (kind == 'M') {
            const MagicDiv m = magicDiv((unsigned)rd(f));
            std::printf("m=%u s=%u\n", m.m, m.s);
        } else need(false, "unknown case letter");
    }
    std::fclose(f);
    return 0;
}
