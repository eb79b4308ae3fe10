// pt_options.hpp — the tuning options of pt_set_option (include/pt_debug.h): every settable value once (Options), and ONE table that says, per option
// number, its name, what it accepts, how it refuses, whether the scene has to be laid out again and where the value goes.  Plain C++: no HIP and no
// context.  pt_set_option (pt_hip.hip) calls Options::set and answers the two queries; the layout step (pt_scene_layout.hpp) and the launch planner
// (pt_launch_plan.hpp) read the struct itself; tests/c/options_check.cpp runs the table on the CPU.
#pragma once
#include "../../../include/pt_api.h"

#include <cstdint>

// the largest LDS budget option 2 takes: one CU's LDS (the test builds the table once with another value)
#ifndef PT_OPT_LDS_BUDGET_MAX
#define PT_OPT_LDS_BUDGET_MAX (160 * 1024)
#endif

// a BVH whose inner-node records exceed this many bytes (in the 80-B form) makes the hand-written intersect kernel use the 64-B form: what an XCD's 4 MB
// L2 holds beside the triangles and the path state streaming through it (measured: profiles/r04_d_node_record_layout.txt)
#ifndef ASM_NODES_80B_LIMIT
#define ASM_NODES_80B_LIMIT (2 << 20)
#endif

namespace ptp {

constexpr int POOL_SLOT_STEP = 256;      // path slots come in blocks of the pool kernels (PLAN_BLOCK, pt_launch_plan.hpp)

struct SetResult {
    int code;              // PT_OK, or PT_ERR_ARG: nothing was stored
    const char* msg;       // the refusal, for pt_last_error ("" with PT_OK)
    bool dirty;            // the value was stored and the scene has to be laid out again
    bool query;            // the option is a query: it stores nothing, the context answers it
};

// Every settable value, with its default.  What a member means: its row of OPTION_TABLE.
struct Options {
    int poolSlots = 0;
    bool countStats = false;
    int ldsBudget = 20 * 1024;
    int noneMin = 8; bool noneMinSet = false;                            // Set: option 3 was used
    int extendMode = 2, extendTpb = 256;
    int extendCacheBytes = 8 * 1024; bool extendCacheSet = false;       // Set: option 6 was used, the tile size is the caller's
    int refillMin = 24, extendMaxBlocksPerCU = 0, innerKeepEighths = 6;
    int bfsNodes = 0x7fffffff, stackModeForce = -1;
    int asmLoop = -1, asmTpb = 0;
    bool fastContract = false;
    int forceNiBits8 = 0, asmNodeLayout = -1;
    bool asmNoRootCull = false;
    int cuPartition = 0;
    int asmNodes80Limit = ASM_NODES_80B_LIMIT;      // no option: no row of the table reaches it.  The layout step's test sets it to get 64-B records from a small scene

    // pt_set_option without its context: checks `value` against the option's row and stores it.  A refused call, an unknown number and a query
    // leave every member as it was.
    inline SetResult set(int option, int64_t value);
};

enum OptionKind { OPT_VALUE, OPT_QUERY };
enum OptionStore {
    STORE_INT,           // the value itself
    STORE_NONZERO,       // value != 0
    STORE_IS_ZERO,       // value == 0: the member is the option's opposite
    STORE_POOL_SLOTS     // rounded up to whole blocks of POOL_SLOT_STEP; 0 (automatic) is accepted beside the range
};

struct OptionRow {
    int number; const char* name;        // the name as renderer.OPTIONS spells it
    OptionKind kind;
    int64_t lo, hi;                      // accepted: lo <= value <= hi ...
    int nList; int64_t list[5];          // ... or, with nList > 0, exactly these values
    const char* refusal;
    bool rebuilds;                       // an accepted set marks the scene for a rebuild: the layout step reads the member
    OptionStore store;
    int Options::* i; bool Options::* b; // the member it writes (one of the two)
    bool Options::* wasSet;              // raised by an accepted set, or null

    bool accepts(int64_t v) const {
        if (nList) { for (int k = 0; k < nList; k++) if (list[k] == v) return true; return false; }
        return (v >= lo && v <= hi) || (store == STORE_POOL_SLOTS && v == 0);
    }
    // the option value that leaves a fresh Options as it is
    int64_t defaultValue() const {
        const Options d;
        return i ? d.*i : store == STORE_IS_ZERO ? !(d.*b) : (d.*b ? 1 : 0);
    }
};

#define PT_OPT_I(m) STORE_INT, &Options::m, nullptr
constexpr int64_t OPT_ANY_LO = INT64_MIN, OPT_ANY_HI = INT64_MAX;

// One row per option number (15 is unassigned).  This table is the definition of the options; include/pt_debug.h describes them for callers.
const OptionRow OPTION_TABLE[] = {
    // path slots in flight; 0 = automatic (newStreamPool, pt_launch_plan.hpp).  Read when a frame stream starts
    {0, "path_slots", OPT_VALUE, POOL_SLOT_STEP, 1 << 26, 0, {}, "path slots must be 0 (automatic) or in [256, 2^26]", false, STORE_POOL_SLOTS, &Options::poolSlots, nullptr, nullptr},
    // count traversal statistics (PT_CNT_*): the counting instances of the compiled kernels; the hand-written kernel then takes no launch
    {1, "count_stats", OPT_VALUE, OPT_ANY_LO, OPT_ANY_HI, 0, {}, "", false, STORE_NONZERO, nullptr, &Options::countStats, nullptr},
    // LDS bytes per block of k_extend: its node / triangle tile beside one traversal stack per lane (the layout's ldsNodes, ldsTris)
    {2, "lds_budget", OPT_VALUE, 0, PT_OPT_LDS_BUDGET_MAX, 0, {}, "LDS budget out of range", true, PT_OPT_I(ldsBudget), nullptr},
    // lanes of a wave waiting for their next object / retirement that make that phase worth a trip; unless set, the fused loop of the hand-written
    // kernel gets 2 (planExtendAsm)
    {3, "none_min", OPT_VALUE, 1, 64, 0, {}, "next-object threshold must be in [1,64]", false, PT_OPT_I(noneMin), &Options::noneMinSet},
    // the intersect kernel: 0 one block per 256 lanes (k_extend), 1 persistent blocks (k_extend_persist), 2 the hand-written form of 1
    // (pt_extend_gfx950.s) for the launches it takes, 1 for the others (planExtend)
    {4, "extend_mode", OPT_VALUE, 0, 2, 0, {}, "extend mode must be 0, 1 or 2", false, PT_OPT_I(extendMode), nullptr},
    // threads per block of k_extend_persist; any other than 256 keeps the hand-written kernel out
    {5, "extend_tpb", OPT_VALUE, 0, 0, 5, {64, 128, 256, 512, 1024}, "extend block size must be 64, 128, 256, 512 or 1024", false, PT_OPT_I(extendTpb), nullptr},
    // bytes of the persistent kernels' LDS tile (node records, then triangle records).  The compiled kernel always sizes its tile by it, the
    // hand-written one only once the caller has set it; the layout step sizes pLdsNodes / pLdsTris by it
    {6, "extend_cache_bytes", OPT_VALUE, 0, 150 * 1024, 0, {}, "extend LDS cache bytes out of range", true, PT_OPT_I(extendCacheBytes), &Options::extendCacheSet},
    // idle lanes of a wave that trigger a ray refill (both persistent kernels)
    {7, "refill_min", OPT_VALUE, 1, 64, 0, {}, "refill threshold must be in [1,64]", false, PT_OPT_I(refillMin), nullptr},
    // cap on the blocks per CU of the persistent grid; 0 = as many as are resident at once
    {8, "extend_blocks_per_cu", OPT_VALUE, 0, 32, 0, {}, "blocks per CU must be in [0,32]", false, PT_OPT_I(extendMaxBlocksPerCU), nullptr},
    // the inner-node phase repeats while more than this many eighths of its starting lanes still sit on inner nodes
    {9, "inner_keep_eighths", OPT_VALUE, 0, 8, 0, {}, "inner-phase persistence must be in [0,8] eighths", false, PT_OPT_I(innerKeepEighths), nullptr},
    // inner-node records kept in breadth-first order (whole levels); the rest follow depth-first (LayoutRun::treeOrder)
    {10, "bfs_nodes", OPT_VALUE, 0, 0x7fffffff, 0, {}, "breadth-first node count out of range", true, PT_OPT_I(bfsNodes), nullptr},
    // traversal-stack entries at least this wide: -1 automatic, 0 short, 1 Packed18, 2 int / 24-bit (k_extend_persist; only ever towards wider entries)
    {11, "stack_mode", OPT_VALUE, -1, 2, 0, {}, "stack mode must be -1 (automatic), 0, 1 or 2", true, PT_OPT_I(stackModeForce), nullptr},
    // does the current scene run on the hand-written kernel?  (answered by pt_set_option: it may have to build the scene)
    {12, "query_asm_eligible", OPT_QUERY, OPT_ANY_LO, OPT_ANY_HI, 0, {}, "", false, STORE_INT, nullptr, nullptr, nullptr},
    // has the hand-written kernel been launched more than `value` times?  (answered by pt_set_option)
    {13, "query_asm_launches_above", OPT_QUERY, OPT_ANY_LO, OPT_ANY_HI, 0, {}, "", false, STORE_INT, nullptr, nullptr, nullptr},
    // main loop of the hand-written kernel: -1 automatic (planExtendAsm), 0 phase-voting, 1 fused trip
    {14, "asm_loop", OPT_VALUE, -1, 1, 0, {}, "main loop of the hand-written kernel: -1 automatic, 0 phase-voting, 1 fused trip", false, PT_OPT_I(asmLoop), nullptr},
    // the relaxed numeric contract, as set: a frame stream runs under the one it was started with
    {16, "numeric_contract", OPT_VALUE, 0, 1, 0, {}, "numeric contract: 0 exact (bit-identical to the oracle), 1 relaxed (hardware rcp/rsq/sqrt/log/cos; RMSE <= 1e-3)", false, STORE_NONZERO, nullptr,
     &Options::fastContract, nullptr},
    // threads per block of the hand-written kernel: 0 automatic (planExtendAsm)
    {17, "asm_tpb", OPT_VALUE, 0, 0, 4, {0, 256, 512, 1024}, "block size of the hand-written kernel: 0 automatic, 256, 512 or 1024", false, PT_OPT_I(asmTpb), nullptr},
    // index-stack encoding of the path state (tests): 1 = 8-bit codes even when the scene's dictionary fits 3 bits, 2 = the float stack
    {18, "index_stack_8bit", OPT_VALUE, 0, 2, 0, {}, "index-stack encoding: 0 automatic, 1 at least 8-bit codes, 2 the floats themselves", true, PT_OPT_I(forceNiBits8), nullptr},
    // node records of the hand-written kernel: -1 automatic (by the trees' size, LayoutRun::nodeRecords), 0 80-B, 1 64-B
    {19, "asm_node_layout", OPT_VALUE, -1, 1, 0, {}, "node records of the hand-written kernel: -1 automatic, 0 80-B sign-ordered, 1 64-B", true, PT_OPT_I(asmNodeLayout), nullptr},
    // more than 8 BVHs: the per-ray cull of the object loop; 0 switches it off (every group box infinite, LayoutRun::rootsAndCullGroups)
    {20, "asm_root_cull", OPT_VALUE, 0, 1, 0, {}, "per-ray cull of the object loop (more than 8 BVHs): 0 off, 1 on", true, STORE_IS_ZERO, nullptr, &Options::asmNoRootCull, nullptr},
    // spatial partition (an experiment: profiles/r06_c_cu_partition.txt): the intersect launches go to a stream whose CU mask holds this many eighths of
    // every XCD's CUs, the shading launches to the complement; built when the next batch is submitted
    {21, "cu_partition", OPT_VALUE, 0, 7, 0, {}, "spatial partition: eighths of every XCD's CUs for the intersect kernel (0 = off: both kernels on all CUs)", false, PT_OPT_I(cuPartition), nullptr},
};
#undef PT_OPT_I
constexpr int OPTION_ROWS = (int)(sizeof(OPTION_TABLE) / sizeof(OPTION_TABLE[0]));

inline const OptionRow* optionRow(int option) {
    for (const OptionRow& r : OPTION_TABLE) if (r.number == option) return &r;
    return nullptr;
}

inline SetResult Options::set(int option, int64_t value) {
    const OptionRow* r = optionRow(option);
    if (!r) return SetResult{PT_ERR_ARG, "unknown option", false, false};
    if (r->kind == OPT_QUERY) return SetResult{PT_OK, "", false, true};
    if (!r->accepts(value)) return SetResult{PT_ERR_ARG, r->refusal, false, false};
    switch (r->store) {
        case STORE_INT: this->*(r->i) = (int)value; break;
        case STORE_NONZERO: this->*(r->b) = value != 0; break;
        case STORE_IS_ZERO: this->*(r->b) = value == 0; break;
        case STORE_POOL_SLOTS: this->*(r->i) = (int)((value + POOL_SLOT_STEP - 1) / POOL_SLOT_STEP * POOL_SLOT_STEP); break;
    }
    if (r->wasSet) this->*(r->wasSet) = true;
    return SetResult{PT_OK, "", r->rebuilds, false};
}

}  // namespace ptp
