// Stand-alone check of csrc/kmcf_cgplan.hpp (tests/test_cgplan_cpu.py builds it with -fsanitize=address,undefined and
// runs it): the path of a solve over every combination of its inputs and how often the resident plan is asked; the
// chunk schedule; the peer-to-peer sequence numbers after a loop, against numbers written out by hand.
#include <cstdio>
#include <vector>

#include "kmcf_cgplan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            ++failures;                                       \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);                \
            std::fprintf(stderr, "\n");                       \
        }                                                     \
    } while (0)

// kmcf_cgr_usable as the decision sees it: an answer, and a count of the calls (the first one on a group is a collective)
struct fake_usable {
    bool answer;
    int calls = 0;
    bool operator()() { ++calls; return answer; }
};

// One row of the table written out: inputs, the answer of the resident plan, and what must come of it.
struct path_row {
    kmcf_cg_call call;
    bool multi, single_reduction, classic_applies, has_limit, usable;
    kmcf_cg_path path;
    int calls;
};

static void path_rows_by_hand()
{
    const kmcf_cg_call OK = KMCF_CG_CALL_RESIDENT_OK, LOOP = KMCF_CG_CALL_LOOP_ONLY, ABS = KMCF_CG_CALL_ABSOLUTE;
    const path_row rows[] = {
        // call multi  sr     ca     limit  usable  path                      calls
        {OK,   true,  true,  false, true,  true,  KMCF_CG_RESIDENT_CG1R,    1},   // a group's K solve
        {OK,   true,  true,  false, false, true,  KMCF_CG_LOOP_CG1R,        1},   // cg1r without a limit: asked all the same
        {OK,   true,  true,  false, true,  false, KMCF_CG_LOOP_CG1R,        1},
        {OK,   false, true,  true,  true,  true,  KMCF_CG_RESIDENT_CG1R,    1},   // one rank, KMCF_CG_VARIANT=cg1r
        {OK,   false, false, true,  true,  true,  KMCF_CG_RESIDENT_CLASSIC, 1},   // one rank, small matrix
        {OK,   false, false, true,  true,  false, KMCF_CG_LOOP_CLASSIC,     1},
        {OK,   false, false, false, true,  true,  KMCF_CG_LOOP_CLASSIC,     0},   // too many tiles: not asked
        {OK,   false, false, true,  false, true,  KMCF_CG_LOOP_CLASSIC,     0},   // classic without a limit: not asked
        {OK,   true,  false, false, true,  true,  KMCF_CG_LOOP_CLASSIC,     0},   // a group forced to classic
        {LOOP, false, false, true,  true,  true,  KMCF_CG_LOOP_CLASSIC,     0},   // heat solve, one rank
        {LOOP, false, true,  true,  true,  true,  KMCF_CG_LOOP_CG1R,        0},   // ... obeys KMCF_CG_VARIANT on one rank
        {LOOP, true,  true,  false, true,  true,  KMCF_CG_LOOP_CG1R,        0},
        {ABS,  false, true,  true,  true,  true,  KMCF_CG_LOOP_CLASSIC,     0},   // one-rank band-edge solve ignores KMCF_CG_VARIANT
        {ABS,  false, false, true,  true,  true,  KMCF_CG_LOOP_CLASSIC,     0},
        {ABS,  true,  true,  false, true,  true,  KMCF_CG_LOOP_CG1R,        0},
        {ABS,  true,  false, false, true,  true,  KMCF_CG_LOOP_CLASSIC,     0},
    };
    int i = 0;
    for (const path_row &r : rows) {
        fake_usable u{r.usable};
        const kmcf_cg_path p = kmcf_cg_choose_path(r.call, r.multi, r.single_reduction, r.classic_applies, r.has_limit, u);
        CHECK(p == r.path && u.calls == r.calls, "row %d: path %d (want %d), %d calls (want %d)", i, (int)p, (int)r.path, u.calls, r.calls);
        ++i;
    }
    // kmcf_pcg_resident_applies: no has_limit in it
    fake_usable yes{true}, no{false}, unasked{true};
    CHECK(kmcf_cg_resident_applies(true, true, false, yes) && yes.calls == 1, "resident_applies: a group, usable");
    CHECK(!kmcf_cg_resident_applies(false, true, true, no) && no.calls == 1, "resident_applies: cg1r, not usable");
    CHECK(!kmcf_cg_resident_applies(false, false, false, unasked) && unasked.calls == 0, "resident_applies: classic, too many tiles");
}

static void path_table()
{
    for (int bits = 0; bits < 32; ++bits) {
        const bool multi = bits & 1, sr = bits & 2, ca = bits & 4, lim = bits & 8, us = bits & 16;
        // relative rule, resident allowed
        {
            fake_usable u{us};
            const kmcf_cg_path p = kmcf_cg_choose_path(KMCF_CG_CALL_RESIDENT_OK, multi, sr, ca, lim, u);
            kmcf_cg_path want;
            int calls;
            if (sr) {                              // cg1r: asked always, once -- also without a limit
                calls = 1;
                want = us && lim ? KMCF_CG_RESIDENT_CG1R : KMCF_CG_LOOP_CG1R;
            } else {                               // classic: asked once, only where the answer decides
                calls = ca && lim ? 1 : 0;
                want = ca && lim && us ? KMCF_CG_RESIDENT_CLASSIC : KMCF_CG_LOOP_CLASSIC;
            }
            CHECK(p == want && u.calls == calls, "resident ok, bits %d: path %d (want %d), %d calls (want %d)", bits, (int)p, (int)want, u.calls, calls);
            CHECK(kmcf_cg_is_resident(p) == (p == KMCF_CG_RESIDENT_CLASSIC || p == KMCF_CG_RESIDENT_CG1R), "is_resident, bits %d", bits);
        }
        // relative rule as a loop only (heat solve): the recurrence by single_reduction on any number of ranks
        {
            fake_usable u{us};
            const kmcf_cg_path p = kmcf_cg_choose_path(KMCF_CG_CALL_LOOP_ONLY, multi, sr, ca, lim, u);
            CHECK(p == (sr ? KMCF_CG_LOOP_CG1R : KMCF_CG_LOOP_CLASSIC) && u.calls == 0, "loop only, bits %d: path %d, %d calls", bits, (int)p, u.calls);
        }
        // absolute rule: one rank classic whatever single_reduction says, a group by single_reduction
        {
            fake_usable u{us};
            const kmcf_cg_path p = kmcf_cg_choose_path(KMCF_CG_CALL_ABSOLUTE, multi, sr, ca, lim, u);
            CHECK(p == (multi && sr ? KMCF_CG_LOOP_CG1R : KMCF_CG_LOOP_CLASSIC) && u.calls == 0, "absolute, bits %d: path %d, %d calls", bits, (int)p, u.calls);
        }
        // kmcf_pcg_resident_applies: cg1r -> usable; classic -> classic_applies && usable (asked only then); no has_limit in it
        if (!lim) {
            fake_usable u{us};
            const bool a = kmcf_cg_resident_applies(multi, sr, ca, u);
            CHECK(a == (sr ? us : ca && us) && u.calls == (sr || ca ? 1 : 0), "resident_applies, bits %d: %d, %d calls", bits, (int)a, u.calls);
        }
    }
    // tail_here: the output kernel forms the last r.z only behind the classic loop of one rank with rows
    const kmcf_cg_path all[] = {KMCF_CG_LOOP_CLASSIC, KMCF_CG_LOOP_CG1R, KMCF_CG_RESIDENT_CLASSIC, KMCF_CG_RESIDENT_CG1R};
    for (kmcf_cg_path p : all)
        for (int multi = 0; multi < 2; ++multi)
            for (int n : {0, 1, 6000})
                CHECK(kmcf_cg_tail_in_output(p, multi != 0, n) == (p == KMCF_CG_LOOP_CLASSIC && !multi && n > 0), "tail_here path %d multi %d n %d", (int)p, multi, n);
    CHECK(kmcf_cg_tail_in_output(KMCF_CG_LOOP_CLASSIC, false, 1) && !kmcf_cg_tail_in_output(KMCF_CG_LOOP_CLASSIC, false, 0) &&
              !kmcf_cg_tail_in_output(KMCF_CG_LOOP_CLASSIC, true, 1) && !kmcf_cg_tail_in_output(KMCF_CG_RESIDENT_CLASSIC, false, 1),
          "tail_here, explicit");
}

static std::vector<int> chunks_of(bool stopping_rule, int limit)
{
    std::vector<int> out;
    int cap = kmcf_cg_first_chunk_cap(stopping_rule), launched = 0;
    while (launched < limit) {
        out.push_back(kmcf_cg_next_chunk(cap, limit - launched));
        launched += out.back();
        if (out.size() > 1000) break;
    }
    return out;
}

static void chunk_schedule()
{
    struct { int limit; std::vector<int> rule, fixed; } want[] = {
        {0, {}, {}},
        {1, {1}, {1}},
        {2, {2}, {2}},
        {3, {2, 1}, {3}},
        {6, {2, 4}, {6}},
        {7, {2, 4, 1}, {7}},
        {62, {2, 4, 8, 16, 32}, {32, 30}},
        {63, {2, 4, 8, 16, 32, 1}, {32, 31}},
        {100, {2, 4, 8, 16, 32, 32, 6}, {32, 32, 32, 4}},
    };
    for (const auto &w : want) {
        const std::vector<int> r = chunks_of(true, w.limit), f = chunks_of(false, w.limit);
        CHECK(r == w.rule, "chunks under a stopping rule, limit %d", w.limit);
        CHECK(f == w.fixed, "chunks of a fixed-iteration solve, limit %d", w.limit);
        int sr = 0, sf = 0;
        for (int c : r) sr += c;
        for (int c : f) sf += c;
        CHECK(sr == w.limit && sf == w.limit, "limit %d: chunks sum to %d / %d", w.limit, sr, sf);
    }
}

// Loop ends of a solve with limit 5 under a stopping rule (chunks 2, 3): the stop found by the first check with no
// iteration gone on (the FIRST iteration's kernel stopped: the device reports 0); the stop in the last iteration
// launched (4 went on, the 5th stopped); the end on the limit.  And a fixed-iteration solve of 5.
static const kmcf_cg_loop_end STOP_FIRST{true, 0, 2}, STOP_LAST{true, 4, 5}, ON_LIMIT{false, 0, 5}, FIXED5{false, 0, 5};

static void sequence_numbers()
{
    // classic loop, direct protocol: both halo numbers = halo0 + (done ? iters : launched)
    CHECK(kmcf_cg_classic_halo_seq(10, STOP_FIRST) == 10, "classic, stop in the first iteration");
    CHECK(kmcf_cg_classic_halo_seq(10, STOP_LAST) == 14, "classic, stop in the last iteration launched");
    CHECK(kmcf_cg_classic_halo_seq(10, ON_LIMIT) == 15, "classic, end on the limit");
    // cg1r, peer-to-peer reductions, not fused: red0 + (done ? iters + 1 : launched)
    CHECK(kmcf_cg1_red_seq(7, STOP_FIRST) == 8, "cg1r separate, stop in the first iteration");
    CHECK(kmcf_cg1_red_seq(7, STOP_LAST) == 12, "cg1r separate, stop in the last iteration launched");
    CHECK(kmcf_cg1_red_seq(7, ON_LIMIT) == 12, "cg1r separate, end on the limit");
    // cg1r fused: executed = done ? iters + 1 : launched; reduction and consumed halo + executed; put the same if done,
    // else one more -- and then the consumed number goes one further and an acknowledgement with it is owed
    kmcf_cg1_fused_seq s = kmcf_cg1_fused_seq_after(7, 20, STOP_FIRST);
    CHECK(s.red == 8 && s.halo_consumed == 21 && s.halo_put == 21 && !s.ack_owed, "fused, stop in the first iteration: %llu %llu %llu %d", s.red,
          s.halo_consumed, s.halo_put, (int)s.ack_owed);
    s = kmcf_cg1_fused_seq_after(7, 20, STOP_LAST);
    CHECK(s.red == 12 && s.halo_consumed == 25 && s.halo_put == 25 && !s.ack_owed, "fused, stop in the last iteration launched: %llu %llu %llu %d",
          s.red, s.halo_consumed, s.halo_put, (int)s.ack_owed);
    s = kmcf_cg1_fused_seq_after(7, 20, ON_LIMIT);
    CHECK(s.red == 12 && s.halo_consumed == 26 && s.halo_put == 26 && s.ack_owed, "fused, end on the limit: %llu %llu %llu %d", s.red,
          s.halo_consumed, s.halo_put, (int)s.ack_owed);

    // two solves in a row stay dense: the second starts where the first ended (5 fixed iterations, then a stop after 4)
    const kmcf_seq h1 = kmcf_cg_classic_halo_seq(0, FIXED5);
    CHECK(h1 == 5 && kmcf_cg_classic_halo_seq(h1, STOP_LAST) == 9, "classic, two solves");
    const kmcf_seq r1 = kmcf_cg1_red_seq(0, FIXED5);
    CHECK(r1 == 5 && kmcf_cg1_red_seq(r1, STOP_LAST) == 10, "cg1r separate, two solves");
    const kmcf_cg1_fused_seq f1 = kmcf_cg1_fused_seq_after(0, 0, FIXED5);
    CHECK(f1.red == 5 && f1.halo_consumed == 6 && f1.halo_put == 6 && f1.ack_owed, "fused, first of two solves");
    // (halo 6 was put and acknowledged unread; the second solve's first SpMV puts and consumes 7)
    const kmcf_cg1_fused_seq f2 = kmcf_cg1_fused_seq_after(f1.red, f1.halo_consumed, STOP_LAST);
    CHECK(f2.red == 10 && f2.halo_consumed == 11 && f2.halo_put == 11 && !f2.ack_owed, "fused, second of two solves");
    CHECK(f1.halo_consumed == f1.halo_put && f2.halo_consumed == f2.halo_put, "fused: nothing put stays unconsumed between solves");
}

int main()
{
    path_rows_by_hand();
    path_table();
    chunk_schedule();
    sequence_numbers();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("cgplan ok\n");
    return 0;
}
