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
#include <string>

enum kmcf_knob_id {
    KNOB_BRICK, KNOB_SPMV_KIND, KNOB_SPMV_CODED, KNOB_SPMV_SELL, KNOB_SPMV_SELLV, KNOB_SPMV_SELL_ROWS,
    KNOB_SPMV_SELL_SORT, KNOB_SPMV_NT, KNOB_SELL_NT, KNOB_SELL_PACK, KNOB_LONG_ROW, KNOB_CB_SCALED, KNOB_SUB_DENSE, KNOB_SUB_STRIP,
    KNOB_EVENTS_PERSISTENT, KNOB_EVENTS_FULLSCAN, KNOB_EVENTS_PARTITIONED, KNOB_EV_TREL, KNOB_CG_VARIANT,
    KNOB_CG_XBATCH, KNOB_CG_RESIDENT, KNOB_CGR_TPB, KNOB_CGR_G1, KNOB_CGR_DELAY, KNOB_CGR_RDELAY, KNOB_CGR_ADAPT, KNOB_CGR_TIMEOUT_MS,
    KNOB_CGR_CLASSIC_TILES, KNOB_TRANSPORT, KNOB_P2P_WINDOW_MB, KNOB_P2P_TIMEOUT_MS, KNOB_P2P_DIRECT, KNOB_P2P_AR,
    KNOB_FORCE_COMM, KNOB_LOOPBACK_TIMEOUT_S, KNOB_DEVICE_SHARE, KNOB_ENTER_ALWAYS, KNOB_TRACE, KNOB_COUNT
};

// Where a knob can be set per communicator (kmcf_set_option).  COMM: read at the next plan, solve, wait or set-up on the
// communicator, like the environment.  CONNECT: read while the communicator is created or connected; settable only
// before kmcf_comm_connect / kmcf_comm_p2p_export.  PROCESS: the environment only (KMCF_DEVICE_SHARE).
enum kmcf_knob_scope { KNOB_SCOPE_NONE, KNOB_COMM, KNOB_CONNECT, KNOB_PROCESS };

// The values kmcf_set_option accepts.  ENUM: one of the '|'-separated words of `words`; INT / F64: a number in
// [lo, hi], the whole string; FLAG: "1" sets the flag, "0" masks an environment setting.
enum kmcf_knob_kind { KNOB_SPEC_NONE, KNOB_ENUM, KNOB_INT, KNOB_F64, KNOB_FLAG };
struct kmcf_knob_spec {
    kmcf_knob_kind kind;
    const char *words;
    double lo, hi;
};
constexpr kmcf_knob_spec kv_enum(const char *words) { return {KNOB_ENUM, words, 0, 0}; }
constexpr kmcf_knob_spec kv_int(double lo, double hi) { return {KNOB_INT, nullptr, lo, hi}; }
constexpr kmcf_knob_spec kv_f64(double lo, double hi) { return {KNOB_F64, nullptr, lo, hi}; }
constexpr kmcf_knob_spec kv_flag() { return {KNOB_FLAG, "0|1", 0, 0}; }

struct kmcf_knob_def {
    kmcf_knob_id id;
    const char *name, *dflt, *values, *what;
    kmcf_knob_scope scope;
    bool group;     // every rank of a group must see the same value: it chooses collectives or the device-side protocol
    kmcf_knob_spec spec;
};

// ("set": the knob acts when it is present in the environment, whatever its value)
inline constexpr kmcf_knob_def kmcf_knobs[] = {
    {KNOB_BRICK, "KMCF_BRICK", "7.7", "edge in Å", "brick edge of the internal row order of K and T; 0 = the caller's row order",
     KNOB_COMM, true, kv_f64(0, 1000)},
    {KNOB_SPMV_KIND, "KMCF_SPMV_KIND", "window, else stream, else vec", "0 vec / 1 stream / 2 window", "SpMV kernel family (forced: the window plan is not judged)",
     KNOB_COMM, false, kv_enum("0|1|2")},
    {KNOB_SPMV_CODED, "KMCF_SPMV_CODED", "1", "0 / 1", "0: f64 values streamed even where they could be coded",
     KNOB_COMM, false, kv_enum("0|1")},
    {KNOB_SPMV_SELL, "KMCF_SPMV_SELL", "1", "0 / 1", "0: the coded window kernel instead of the row-per-lane kernel",
     KNOB_COMM, false, kv_enum("0|1")},
    {KNOB_SPMV_SELLV, "KMCF_SPMV_SELLV", "1", "0 / 1", "0: f64 matrices on the window kernel instead of the row-per-lane one",
     KNOB_COMM, false, kv_enum("0|1")},
    {KNOB_SPMV_SELL_ROWS, "KMCF_SPMV_SELL_ROWS", "by size: 64 … 256", "64 … 256 (multiples of 64)", "rows per row-per-lane tile",
     KNOB_COMM, false, kv_enum("64|128|192|256")},
    {KNOB_SPMV_SELL_SORT, "KMCF_SPMV_SELL_SORT", "1", "0 / 1", "0: the rows of a tile are not sorted into the internal row order",
     KNOB_COMM, false, kv_enum("0|1")},
    {KNOB_SPMV_NT, "KMCF_SPMV_NT", "matrices beyond the caches", "0 / 1", "nontemporal matrix loads in the f64-value SpMV kernels",
     KNOB_COMM, false, kv_enum("0|1")},
    {KNOB_SELL_NT, "KMCF_SELL_NT", "beyond the Infinity Cache", "0 / 1", "nontemporal loads of the coded entry stream",
     KNOB_COMM, false, kv_enum("0|1")},
    {KNOB_SELL_PACK, "KMCF_SELL_PACK", "1", "0 / 1", "0: the coded entry stream as 16-bit entries, four per 8-byte word, instead of five 12-bit fields",
     KNOB_COMM, false, kv_enum("0|1")},
    {KNOB_LONG_ROW, "KMCF_LONG_ROW", "384", "entries; <= 0: none", "rows longer than this go to the long-row kernel",
     KNOB_COMM, false, kv_int(-1000000000, 1000000000)},
    {KNOB_CB_SCALED, "KMCF_CB_SCALED", "0", "0 / 1", "1: the CB-edge solve in the literal scaled form (a group: one more halo exchange)",
     KNOB_COMM, true, kv_enum("0|1")},
    {KNOB_SUB_DENSE, "KMCF_SUB_DENSE", "dense from a quarter full", "0 bitmap / 1 dense / 2 jagged",
     "tunnel block as bitmap / dense symmetric tiles / jagged tiles (one rank); all ranks of a group must agree",
     KNOB_COMM, true, kv_enum("0|1|2")},
    {KNOB_SUB_STRIP, "KMCF_SUB_STRIP", "16", ">= 1", "tunnel-block tiles per strip",
     KNOB_COMM, true, kv_int(1, 1000000)},
    {KNOB_EVENTS_PERSISTENT, "KMCF_EVENTS_PERSISTENT", "1", "0 / 1", "0: three launches per event instead of one persistent block per batch",
     KNOB_COMM, true, kv_enum("0|1")},
    {KNOB_EVENTS_FULLSCAN, "KMCF_EVENTS_FULLSCAN", "unset", "set", "the reference-style zero-out pass over the event list",
     KNOB_COMM, false, kv_flag()},
    {KNOB_EVENTS_PARTITIONED, "KMCF_EVENTS_PARTITIONED", "unset", "set", "the reference's partitioned multi-rank event step instead of the replicated one",
     KNOB_COMM, true, kv_flag()},
    {KNOB_EV_TREL, "KMCF_EV_TREL", "2048", "1 … 2048", "tests: claim range of the event batch kernel",
     KNOB_COMM, false, kv_int(1, 2048)},
    {KNOB_CG_VARIANT, "KMCF_CG_VARIANT", "classic on one rank, cg1r in a group", "classic / cg1r (any value starting with cg)", "CG recurrence",
     KNOB_COMM, true, kv_enum("classic|cg1r")},
    {KNOB_CG_XBATCH, "KMCF_CG_XBATCH", "4", "1 / 2 / 3 / 4", "classic kernel loop of one rank: x += alpha p applied once in this many iterations, from a ring of p buffers",
     KNOB_COMM, false, kv_enum("1|2|3|4")},
    {KNOB_CG_RESIDENT, "KMCF_CG_RESIDENT", "1", "0 / 1", "0: no register-resident launch",
     KNOB_COMM, true, kv_enum("0|1")},
    {KNOB_CGR_TPB, "KMCF_CGR_TPB", "smallest that fits", "1 / 2 / 4", "resident launch: tiles per block",
     KNOB_COMM, true, kv_enum("1|2|4")},
    {KNOB_CGR_G1, "KMCF_CGR_G1", "flat up to 256 blocks, else 16", "2 … 64", "resident launch: blocks per reduction group",
     KNOB_COMM, true, kv_int(2, 64)},
    {KNOB_CGR_DELAY, "KMCF_CGR_DELAY", "6", "units of ≈ 0.1 µs", "resident launch: sleep before the first poll of a gather",
     KNOB_COMM, false, kv_int(0, 1000000)},
    {KNOB_CGR_RDELAY, "KMCF_CGR_RDELAY", "6", "units of ≈ 0.1 µs", "resident launch: sleep before the first poll of a reduction's collection",
     KNOB_COMM, false, kv_int(0, 1000000)},
    {KNOB_CGR_ADAPT, "KMCF_CGR_ADAPT", "16", "polls; 0 = fixed delays", "resident launch: streak of successful first polls after which a wavefront sleeps one unit less",
     KNOB_COMM, false, kv_int(0, 1000000)},
    {KNOB_CGR_TIMEOUT_MS, "KMCF_CGR_TIMEOUT_MS", "4000 (a p2p group: KMCF_P2P_TIMEOUT_MS)", "ms", "resident launch: bound of its device-side waits",
     KNOB_COMM, false, kv_int(1, 2000000000)},
    {KNOB_CGR_CLASSIC_TILES, "KMCF_CGR_CLASSIC_TILES", "1024", "tiles", "largest matrix whose classic recurrence runs as a resident launch",
     KNOB_COMM, false, kv_int(0, 2000000000)},
    {KNOB_TRANSPORT, "KMCF_TRANSPORT", "rccl", "rccl / p2p / auto", "transport of a rank group's exchanges (auto: p2p if its self-test passes)",
     KNOB_CONNECT, true, kv_enum("rccl|p2p|auto")},
    {KNOB_P2P_WINDOW_MB, "KMCF_P2P_WINDOW_MB", "96", ">= 8", "size of a rank's peer-to-peer window",
     KNOB_CONNECT, false, kv_int(8, 1000000)},
    {KNOB_P2P_TIMEOUT_MS, "KMCF_P2P_TIMEOUT_MS", "10000", "ms", "bound of every device-side wait of the p2p transport",
     KNOB_CONNECT, false, kv_f64(1, 1e9)},
    {KNOB_P2P_DIRECT, "KMCF_P2P_DIRECT", "1", "0 / 1", "0: staged halo protocol (put / wait-copy kernels on the comm stream)",
     KNOB_COMM, true, kv_enum("0|1")},
    {KNOB_P2P_AR, "KMCF_P2P_AR", "inside the update kernel", "split", "split: the fused iteration's all-reduce in a 1-block kernel of its own",
     KNOB_COMM, true, kv_enum("split|inside")},
    {KNOB_FORCE_COMM, "KMCF_FORCE_COMM", "unset", "set", "tests: a 1-rank group runs the RCCL collectives",
     KNOB_CONNECT, false, kv_flag()},
    {KNOB_LOOPBACK_TIMEOUT_S, "KMCF_LOOPBACK_TIMEOUT_S", "120", "s", "in-process test groups: how long a rank waits for its peers at a collective",
     KNOB_CONNECT, false, kv_int(1, 1000000)},
    {KNOB_DEVICE_SHARE, "KMCF_DEVICE_SHARE", "1", ">= 1", "read once: s ranks share one GPU, chip-filling grids take 1/s (rehearsals)",
     KNOB_PROCESS, false, kv_int(1, 64)},
    {KNOB_ENTER_ALWAYS, "KMCF_ENTER_ALWAYS", "unset", "set", "every entry point orders itself behind an event on the caller's stream",
     KNOB_COMM, false, kv_flag()},
    {KNOB_TRACE, "KMCF_TRACE", "unset", "set", "host-side diagnostics on stderr: SpMV, resident and p2p plans, timing of kmcf_pcg_jacobi",
     KNOB_COMM, false, kv_flag()},
};

constexpr bool kmcf_knobs_in_order(int k = 0)
{
    return k == KNOB_COUNT || (kmcf_knobs[k].id == k && kmcf_knobs_in_order(k + 1));
}
static_assert(sizeof(kmcf_knobs) / sizeof(kmcf_knobs[0]) == KNOB_COUNT && kmcf_knobs_in_order(), "kmcf_knobs: one entry per kmcf_knob_id, in the enum's order");
constexpr bool kmcf_knobs_specified(int k = 0)
{
    return k == KNOB_COUNT || (kmcf_knobs[k].scope != KNOB_SCOPE_NONE && kmcf_knobs[k].spec.kind != KNOB_SPEC_NONE &&
                               kmcf_knobs_specified(k + 1));
}
static_assert(kmcf_knobs_specified(), "kmcf_knobs: every entry has a scope and a value spec");

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

// Per-communicator overrides (kmcf_set_option): a validated string per knob, or nothing.  The effective value of a knob
// is the override if there is one, else the environment; a flag's override "0" reads as absent.
struct kmcf_knob_overrides {
    std::string val[KNOB_COUNT];
    bool set[KNOB_COUNT] = {};
};
inline const char *kmcf_knob_effective(const kmcf_knob_overrides &o, kmcf_knob_id k)
{
    if (!o.set[k]) return kmcf_knob(k);
    return kmcf_knobs[k].spec.kind == KNOB_FLAG && o.val[k] == "0" ? nullptr : o.val[k].c_str();
}
// where the effective value comes from: 0 nowhere (the library decides), 1 the environment, 2 the override
inline int kmcf_knob_source(const kmcf_knob_overrides &o, kmcf_knob_id k) { return o.set[k] ? 2 : kmcf_knob(k) ? 1 : 0; }
