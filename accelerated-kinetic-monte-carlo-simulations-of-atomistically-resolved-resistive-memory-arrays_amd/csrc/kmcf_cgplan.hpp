// Host decisions of the CG solver (kmcf_cg.hip): which of its four paths a solve takes, how many iterations the loop
// enqueues between two looks at the stop flag, and what the peer-to-peer sequence numbers are after a loop.  Pure
// functions: plain C++, no HIP header -- tests/cgplan_check.cpp calls them stand-alone.
#pragma once
#include <algorithm>

// ---------------------------------------------------------------- the path
// classic = the reference's recurrence and operation order (default for one rank); cg1r = the single-reduction
// recurrence (default for groups); LOOP = a loop of kernels, RESIDENT = ONE register-resident launch (kmcf_cgr.hip).
enum kmcf_cg_path { KMCF_CG_LOOP_CLASSIC, KMCF_CG_LOOP_CG1R, KMCF_CG_RESIDENT_CLASSIC, KMCF_CG_RESIDENT_CG1R };

// The kind of call: stopping rule, and whether the resident launch may serve it.
enum kmcf_cg_call {
    KMCF_CG_CALL_RESIDENT_OK,   // relative rule r.z / b.b; the system is the one a resident plan of the matrix is made for (K, T)
    KMCF_CG_CALL_LOOP_ONLY,     // relative rule, another system in the same matrix (heat solve): never resident
    KMCF_CG_CALL_ABSOLUTE,      // absolute rule of solve_sparse_CG_Jacobi (band-edge solve): never resident
};

inline bool kmcf_cg_is_resident(kmcf_cg_path p) { return p == KMCF_CG_RESIDENT_CLASSIC || p == KMCF_CG_RESIDENT_CG1R; }

//   call         recurrence                           resident_usable() called                      result
//   RESIDENT_OK  cg1r                                 always, once (also without a limit)           usable and has_limit: RESIDENT_CG1R, else LOOP_CG1R
//   RESIDENT_OK  classic                              once, only if classic_applies && has_limit    true: RESIDENT_CLASSIC, else LOOP_CLASSIC
//   LOOP_ONLY    by single_reduction, any rank count  never                                         LOOP_CG1R / LOOP_CLASSIC
//   ABSOLUTE     !multi: classic whatever             never                                         LOOP_CLASSIC
//                single_reduction says (the one-rank
//                band-edge solve is what it always was)
//   ABSOLUTE     multi: by single_reduction           never                                         LOOP_CG1R / LOOP_CLASSIC
// multi = nranks > 1 || force_collectives; single_reduction = kmcf_cg_single_reduction; classic_applies =
// kmcf_cgr_classic_applies; has_limit = fixed_iters > 0 || max_it > 0.  resident_usable (kmcf_cgr_usable) enters a
// collective the first time on a group: WHEN it is called is behaviour -- every rank calls it or none, whatever its
// limit, hence the cg1r row asks before it looks at has_limit.
template <class F>
kmcf_cg_path kmcf_cg_choose_path(kmcf_cg_call call, bool multi, bool single_reduction, bool classic_applies, bool has_limit,
                                 F &&resident_usable)
{
    if (call == KMCF_CG_CALL_RESIDENT_OK) {
        if (single_reduction) return resident_usable() && has_limit ? KMCF_CG_RESIDENT_CG1R : KMCF_CG_LOOP_CG1R;
        return classic_applies && has_limit && resident_usable() ? KMCF_CG_RESIDENT_CLASSIC : KMCF_CG_LOOP_CLASSIC;
    }
    if (call == KMCF_CG_CALL_ABSOLUTE && !multi) return KMCF_CG_LOOP_CLASSIC;
    return single_reduction ? KMCF_CG_LOOP_CG1R : KMCF_CG_LOOP_CLASSIC;
}

// "The next RESIDENT_OK solve runs resident", asked by a caller that passes a constant limit of its own (the K solve,
// which then hands the launch its vectors where they lie): the table with has_limit = true.
template <class F>
bool kmcf_cg_resident_applies(bool multi, bool single_reduction, bool classic_applies, F &&resident_usable)
{
    return kmcf_cg_is_resident(kmcf_cg_choose_path(KMCF_CG_CALL_RESIDENT_OK, multi, single_reduction, classic_applies, true, resident_usable));
}

// The classic loop of one rank leaves the r.z of the loop condition's last evaluation to the output kernel of a caller
// that collects the result itself (kmcf_pcg_jacobi); every other path has formed it.
inline bool kmcf_cg_tail_in_output(kmcf_cg_path path, bool multi, int n) { return path == KMCF_CG_LOOP_CLASSIC && !multi && n > 0; }

// ---------------------------------------------------------------- the chunk schedule
// Iterations are enqueued in chunks, the stop flag is read back once per chunk.  Under a stopping rule the chunks grow
// 2, 4, 8 ... KMCF_CG_CHUNK_MAX: a warm-started solve (every KMC step but the first) stops within a few iterations, and
// every iteration enqueued behind the stop is empty launches.  A fixed iteration count takes the largest chunk at once.
constexpr int KMCF_CG_CHUNK_MAX = 32;            // = KMCF_CHUNK_ITERS (kmcf_internal.hpp; asserted in kmcf_cg.hip)

inline int kmcf_cg_first_chunk_cap(bool stopping_rule) { return stopping_rule ? 2 : KMCF_CG_CHUNK_MAX; }
// the next chunk of a loop with `left` (> 0) iterations to go; the cap grows for the chunk after
inline int kmcf_cg_next_chunk(int &cap, int left)
{
    const int chunk = std::min(left, cap);
    cap = std::min(2 * cap, KMCF_CG_CHUNK_MAX);
    return chunk;
}

// ---------------------------------------------------------------- sequence numbers after a loop
// The peer-to-peer protocols number their exchanges densely: parities and acknowledgement windows hang on it, and a
// group whose ranks are one number apart waits until its bounded wait expires.  Inside the loop the host counts per
// LAUNCH; kernels behind the stop return at once (on every rank alike) without an exchange, so after the loop the
// numbers are set back to what really ran.
struct kmcf_cg_loop_end {
    bool done;       // the stopping rule fired
    int iters;       // iterations that went on, as the device reports them at the stop (read only if done)
    int launched;    // iterations enqueued
};
typedef unsigned long long kmcf_seq;

// classic loop, direct halo protocol: one SpMV (put, consumption, acknowledgement) per iteration that went on; both
// halo numbers (consumed, put) get this value
inline kmcf_seq kmcf_cg_classic_halo_seq(kmcf_seq halo0, const kmcf_cg_loop_end &e)
{
    return halo0 + (kmcf_seq)(e.done ? e.iters : e.launched);
}

// cg1r, reductions over peer-to-peer, not fused: one all-reduce per update kernel that ran -- the iterations that went
// on and the one that stopped
inline kmcf_seq kmcf_cg1_red_seq(kmcf_seq red0, const kmcf_cg_loop_end &e)
{
    return red0 + (kmcf_seq)(e.done ? e.iters + 1 : e.launched);
}

// cg1r fused (halo put and acknowledgement ride in the update kernel): one all-reduce, one consumed halo and one
// acknowledgement per executed update kernel; a put by every update that went on.  A loop that ended on its limit has
// put a last halo no SpMV will read: it counts as consumed, and the caller owes ONE acknowledgement with that number
// (every rank does the same), so that the sequence stays dense.
struct kmcf_cg1_fused_seq { kmcf_seq red, halo_consumed, halo_put; bool ack_owed; };
inline kmcf_cg1_fused_seq kmcf_cg1_fused_seq_after(kmcf_seq red0, kmcf_seq halo0, const kmcf_cg_loop_end &e)
{
    const kmcf_seq executed = (kmcf_seq)(e.done ? e.iters + 1 : e.launched);
    kmcf_cg1_fused_seq s{red0 + executed, halo0 + executed, halo0 + executed, !e.done};
    if (s.ack_owed) { ++s.halo_put; ++s.halo_consumed; }
    return s;
}
