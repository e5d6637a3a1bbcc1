// The environment knobs of libkmcfield: one table, one accessor.  None is needed in production; INTEGRATION.md lists
// the same knobs (tests/test_knobs.py checks that the two lists agree and that kmcf_knob is the only reader).
//
// Every knob is read when the call that uses it runs -- once per plan, solve, wait or set-up, never inside an
// iteration or per launch -- so a process that changes its environment between two calls (bench.py, the tests) gets
// the new value at the next call.  The one exception is KMCF_DEVICE_SHARE: it describes the process (how many ranks
// share the GPU), every chip-filling grid of every plan is sized by it, and plans made under two different values
// would wait for each other on the device with the wrong residency; kmcf_device_share reads it once.
#pragma once
#include <cstdlib>

enum kmcf_knob_id {
    KNOB_BRICK, KNOB_SPMV_KIND, KNOB_SPMV_CODED, KNOB_SPMV_SELL, KNOB_SPMV_SELLV, KNOB_SPMV_SELL_ROWS,
    KNOB_SPMV_SELL_SORT, KNOB_SPMV_NT, KNOB_SELL_NT, KNOB_LONG_ROW, KNOB_CB_SCALED, KNOB_SUB_DENSE, KNOB_SUB_STRIP,
    KNOB_EVENTS_PERSISTENT, KNOB_EVENTS_FULLSCAN, KNOB_EVENTS_PARTITIONED, KNOB_EV_TREL, KNOB_CG_VARIANT,
    KNOB_CG_RESIDENT, KNOB_CGR_TPB, KNOB_CGR_G1, KNOB_CGR_DELAY, KNOB_CGR_RDELAY, KNOB_CGR_ADAPT, KNOB_CGR_TIMEOUT_MS,
    KNOB_CGR_CLASSIC_TILES, KNOB_TRANSPORT, KNOB_P2P_WINDOW_MB, KNOB_P2P_TIMEOUT_MS, KNOB_P2P_DIRECT, KNOB_P2P_AR,
    KNOB_FORCE_COMM, KNOB_LOOPBACK_TIMEOUT_S, KNOB_DEVICE_SHARE, KNOB_ENTER_ALWAYS, KNOB_TRACE, KNOB_COUNT
};

struct kmcf_knob_def {
    kmcf_knob_id id;
    const char *name, *dflt, *values, *what;
};

// ("set": the knob acts when it is present in the environment, whatever its value)
inline constexpr kmcf_knob_def kmcf_knobs[] = {
    {KNOB_BRICK, "KMCF_BRICK", "7.7", "edge in Å", "brick edge of the internal row order of K and T; 0 = the caller's row order"},
    {KNOB_SPMV_KIND, "KMCF_SPMV_KIND", "window, else stream, else vec", "0 vec / 1 stream / 2 window", "SpMV kernel family (forced: the window plan is not judged)"},
    {KNOB_SPMV_CODED, "KMCF_SPMV_CODED", "1", "0 / 1", "0: f64 values streamed even where they could be coded"},
    {KNOB_SPMV_SELL, "KMCF_SPMV_SELL", "1", "0 / 1", "0: the coded window kernel instead of the row-per-lane kernel"},
    {KNOB_SPMV_SELLV, "KMCF_SPMV_SELLV", "1", "0 / 1", "0: f64 matrices on the window kernel instead of the row-per-lane one"},
    {KNOB_SPMV_SELL_ROWS, "KMCF_SPMV_SELL_ROWS", "by size: 64 … 256", "64 … 256 (multiples of 64)", "rows per row-per-lane tile"},
    {KNOB_SPMV_SELL_SORT, "KMCF_SPMV_SELL_SORT", "1", "0 / 1", "0: the rows of a tile are not sorted into the internal row order"},
    {KNOB_SPMV_NT, "KMCF_SPMV_NT", "matrices beyond the caches", "0 / 1", "nontemporal matrix loads in the f64-value SpMV kernels"},
    {KNOB_SELL_NT, "KMCF_SELL_NT", "beyond the Infinity Cache", "0 / 1", "nontemporal loads of the coded entry stream"},
    {KNOB_LONG_ROW, "KMCF_LONG_ROW", "384", "entries; <= 0: none", "rows longer than this go to the long-row kernel"},
    {KNOB_CB_SCALED, "KMCF_CB_SCALED", "0", "0 / 1", "1: the CB-edge solve in the literal scaled form"},
    {KNOB_SUB_DENSE, "KMCF_SUB_DENSE", "dense from a quarter full", "0 bitmap / 1 dense / 2 jagged",
     "tunnel block as bitmap / dense symmetric tiles / jagged tiles (one rank); all ranks of a group must agree"},
    {KNOB_SUB_STRIP, "KMCF_SUB_STRIP", "16", ">= 1", "tunnel-block tiles per strip"},
    {KNOB_EVENTS_PERSISTENT, "KMCF_EVENTS_PERSISTENT", "1", "0 / 1", "0: three launches per event instead of one persistent block per batch"},
    {KNOB_EVENTS_FULLSCAN, "KMCF_EVENTS_FULLSCAN", "unset", "set", "the reference-style zero-out pass over the event list"},
    {KNOB_EVENTS_PARTITIONED, "KMCF_EVENTS_PARTITIONED", "unset", "set", "the reference's partitioned multi-rank event step instead of the replicated one"},
    {KNOB_EV_TREL, "KMCF_EV_TREL", "2048", "1 … 2048", "tests: claim range of the event batch kernel"},
    {KNOB_CG_VARIANT, "KMCF_CG_VARIANT", "classic on one rank, cg1r in a group", "classic / cg1r (any value starting with cg)", "CG recurrence"},
    {KNOB_CG_RESIDENT, "KMCF_CG_RESIDENT", "1", "0 / 1", "0: no register-resident launch"},
    {KNOB_CGR_TPB, "KMCF_CGR_TPB", "smallest that fits", "1 / 2 / 4", "resident launch: tiles per block"},
    {KNOB_CGR_G1, "KMCF_CGR_G1", "flat up to 256 blocks, else 16", "2 … 64", "resident launch: blocks per reduction group"},
    {KNOB_CGR_DELAY, "KMCF_CGR_DELAY", "6", "units of ≈ 0.1 µs", "resident launch: sleep before the first poll of a gather"},
    {KNOB_CGR_RDELAY, "KMCF_CGR_RDELAY", "6", "units of ≈ 0.1 µs", "resident launch: sleep before the first poll of a reduction's collection"},
    {KNOB_CGR_ADAPT, "KMCF_CGR_ADAPT", "16", "polls; 0 = fixed delays", "resident launch: streak of successful first polls after which a wavefront sleeps one unit less"},
    {KNOB_CGR_TIMEOUT_MS, "KMCF_CGR_TIMEOUT_MS", "4000 (a p2p group: KMCF_P2P_TIMEOUT_MS)", "ms", "resident launch: bound of its device-side waits"},
    {KNOB_CGR_CLASSIC_TILES, "KMCF_CGR_CLASSIC_TILES", "1024", "tiles", "largest matrix whose classic recurrence runs as a resident launch"},
    {KNOB_TRANSPORT, "KMCF_TRANSPORT", "rccl", "rccl / p2p / auto", "transport of a rank group's exchanges (auto: p2p if its self-test passes)"},
    {KNOB_P2P_WINDOW_MB, "KMCF_P2P_WINDOW_MB", "96", ">= 8", "size of a rank's peer-to-peer window"},
    {KNOB_P2P_TIMEOUT_MS, "KMCF_P2P_TIMEOUT_MS", "10000", "ms", "bound of every device-side wait of the p2p transport"},
    {KNOB_P2P_DIRECT, "KMCF_P2P_DIRECT", "1", "0 / 1", "0: staged halo protocol (put / wait-copy kernels on the comm stream)"},
    {KNOB_P2P_AR, "KMCF_P2P_AR", "inside the update kernel", "split", "split: the fused iteration's all-reduce in a 1-block kernel of its own"},
    {KNOB_FORCE_COMM, "KMCF_FORCE_COMM", "unset", "set", "tests: a 1-rank group runs the RCCL collectives"},
    {KNOB_LOOPBACK_TIMEOUT_S, "KMCF_LOOPBACK_TIMEOUT_S", "120", "s", "in-process test groups: how long a rank waits for its peers at a collective"},
    {KNOB_DEVICE_SHARE, "KMCF_DEVICE_SHARE", "1", ">= 1", "read once: s ranks share one GPU, chip-filling grids take 1/s (rehearsals)"},
    {KNOB_ENTER_ALWAYS, "KMCF_ENTER_ALWAYS", "unset", "set", "every entry point orders itself behind an event on the caller's stream"},
    {KNOB_TRACE, "KMCF_TRACE", "unset", "set", "host-side diagnostics on stderr: SpMV, resident and p2p plans, timing of kmcf_pcg_jacobi"},
};

constexpr bool kmcf_knobs_in_order(int k = 0)
{
    return k == KNOB_COUNT || (kmcf_knobs[k].id == k && kmcf_knobs_in_order(k + 1));
}
static_assert(sizeof(kmcf_knobs) / sizeof(kmcf_knobs[0]) == KNOB_COUNT && kmcf_knobs_in_order(), "kmcf_knobs: one entry per kmcf_knob_id, in the enum's order");

// The knob's value in the environment, or nullptr: the library's only reader of the environment.
inline const char *kmcf_knob(kmcf_knob_id k) { return getenv(kmcf_knobs[k].name); }
inline int kmcf_knob_int(kmcf_knob_id k, int dflt)
{
    const char *e = kmcf_knob(k);
    return e ? atoi(e) : dflt;
}
inline double kmcf_knob_f64(kmcf_knob_id k, double dflt)
{
    const char *e = kmcf_knob(k);
    return e ? atof(e) : dflt;
}
inline bool kmcf_trace() { return kmcf_knob(KNOB_TRACE) != nullptr; }
