// Stand-alone check of csrc/kmcf_subplan.hpp (tests/test_subplan_cpu.py builds it with -fsanitize=address,undefined and
// runs it): the strip deal of the tiled tunnel block on worked examples and its properties over nb 1 ... 69; the
// storage rule of one rank and of a group with a synthetic amount of free memory, and when that amount is asked for.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kmcf_subplan.hpp"

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

// free device memory as the rule sees it: `bytes` (ok) or unreadable (!ok); counts the calls
struct fake_free {
    size_t bytes;
    bool ok;
    int calls = 0;
    bool operator()(size_t *out) { ++calls; *out = bytes; return ok; }
};

static bool strips_are(const kmcf_strip_deal &d, const std::vector<kmcf_strip> &want)
{
    if (d.strips.size() != want.size()) return false;
    for (size_t k = 0; k < want.size(); ++k)
        if (d.strips[k].I != want[k].I || d.strips[k].J0 != want[k].J0 || d.strips[k].len != want[k].len || d.strips[k].first != want[k].first)
            return false;
    return true;
}

static void deal_explicit()
{
    static_assert(sizeof(kmcf_strip) == 16, "a strip is four ints");
    const kmcf_strip_deal one = kmcf_deal_strips(3, 2, 1, 0, false);
    CHECK(strips_are(one, {{0, 0, 2, 0}, {0, 2, 1, 2}, {1, 1, 2, 3}, {2, 2, 1, 5}}), "P = 1: strips");
    CHECK((one.first == std::vector<int>{0, 2, 3, 4}), "P = 1: first");
    CHECK(one.n_tiles == 6 && one.tile_local.empty(), "P = 1: %lld tiles", one.n_tiles);
    const kmcf_strip_deal r0 = kmcf_deal_strips(3, 2, 2, 0, true), r1 = kmcf_deal_strips(3, 2, 2, 1, true);
    CHECK(strips_are(r0, {{0, 0, 2, 0}, {2, 2, 1, 2}}), "P = 2, rank 0: strips");
    CHECK((r0.first == std::vector<int>{0, 1, 1, 2}), "P = 2, rank 0: first");
    CHECK((r0.tile_local == std::vector<int>{0, 1, -1, -1, -1, 2}), "P = 2, rank 0: tile_local");
    CHECK(strips_are(r1, {{0, 2, 1, 0}, {1, 1, 2, 1}}), "P = 2, rank 1: strips");
    CHECK((r1.first == std::vector<int>{0, 1, 2, 2}), "P = 2, rank 1: first");
    CHECK((r1.tile_local == std::vector<int>{-1, -1, 0, 1, 2, -1}), "P = 2, rank 1: tile_local");
    CHECK(r0.n_tiles == 3 && r1.n_tiles == 3, "P = 2: %lld / %lld tiles", r0.n_tiles, r1.n_tiles);
    // the figures of DESIGN.md, nb = 30 in strips of 16
    CHECK(kmcf_deal_strips(30, 16, 2, 0, true).n_tiles == 233 && kmcf_deal_strips(30, 16, 2, 1, true).n_tiles == 232, "nb = 30 over two ranks");
    for (int r = 0; r < 3; ++r) CHECK(kmcf_deal_strips(30, 16, 3, r, true).n_tiles == 155, "nb = 30 over three ranks, rank %d", r);
}

static void deal_properties()
{
    const int lens[] = {1, 2, 3, 16}, ranks[] = {1, 2, 3, 4, 5, 8};
    for (int nb = 1; nb <= 69; ++nb)
        for (int strip_len : lens)
            for (int P : ranks) {
                const long long all = (long long)nb * (nb + 1) / 2;
                std::vector<int> holders((size_t)all, 0);
                long long sum = 0, lo = all, hi = 0;
                for (int r = 0; r < P; ++r) {
                    const kmcf_strip_deal d = kmcf_deal_strips(nb, strip_len, P, r, true);
                    long long mine = 0;
                    for (size_t k = 0; k < d.strips.size(); ++k) {
                        const kmcf_strip &s = d.strips[k];
                        CHECK(s.first == mine && s.len >= 1 && s.len <= strip_len && s.J0 >= s.I && s.J0 + s.len <= nb,
                              "nb %d len %d P %d rank %d: strip %zu", nb, strip_len, P, r, k);
                        CHECK(d.first[s.I] <= (int)k && (int)k < d.first[s.I + 1], "nb %d len %d P %d rank %d: strip %zu outside its block row's range", nb, strip_len, P, r, k);
                        for (int q = 0; q < s.len; ++q) {
                            const long long g = symm_tile_index(nb, s.I, s.J0 + q);
                            CHECK(g >= 0 && g < all && d.tile_local[(size_t)g] == mine + q, "nb %d len %d P %d rank %d: tile_local", nb, strip_len, P, r);
                            if (g >= 0 && g < all) ++holders[(size_t)g];
                        }
                        mine += s.len;
                    }
                    CHECK(mine == d.n_tiles && d.first[0] == 0 && d.first[nb] == (int)d.strips.size(), "nb %d len %d P %d rank %d: counts", nb, strip_len, P, r);
                    long long local = 0;
                    for (int v : d.tile_local) local += v >= 0;
                    CHECK(local == d.n_tiles, "nb %d len %d P %d rank %d: %lld tiles in tile_local, %lld held", nb, strip_len, P, r, local, d.n_tiles);
                    sum += d.n_tiles;
                    lo = std::min(lo, d.n_tiles);
                    hi = std::max(hi, d.n_tiles);
                }
                for (long long g = 0; g < all; ++g) CHECK(holders[(size_t)g] == 1, "nb %d len %d P %d: tile %lld held %d times", nb, strip_len, P, g, holders[(size_t)g]);
                CHECK(sum == all, "nb %d len %d P %d: %lld tiles dealt of %lld", nb, strip_len, P, sum, all);
                CHECK(hi - lo <= strip_len, "nb %d len %d P %d: %lld ... %lld tiles a rank", nb, strip_len, P, lo, hi);
            }
}

static bool is(const kmcf_sub_form &f, bool dense, bool jagged) { return f.dense == dense && f.jagged == jagged; }

static void rule_one_rank()
{
    const size_t plenty = (size_t)1 << 40, tight = 28000000;      // tight: the tiles of 2048 points need 17 301 504 > 0.6 x 28 000 000
    const int A = KMCF_SUB_AUTO;
    {   // below 2048 points: bitmap however full, and nobody asks for the free memory
        fake_free fr{plenty, true};
        CHECK(is(kmcf_sub_form_one_rank(2047, 2047LL * 2047, 0, 0, A, fr), false, false) && fr.calls == 0, "2047 points, full");
    }
    {   // a quarter full exactly: bitmap
        fake_free fr{plenty, true};
        CHECK(is(kmcf_sub_form_one_rank(2048, 1048576, 0, 0, A, fr), false, false) && fr.calls == 0, "2048 points, a quarter full");
    }
    {   // one entry more: dense, the free memory read once
        fake_free fr{plenty, true};
        CHECK(is(kmcf_sub_form_one_rank(2048, 1048577, 0, 0, A, fr), true, false) && fr.calls == 1, "2048 points, above a quarter (%d calls)", fr.calls);
    }
    {   // ... not read when the tiles' buffer is large enough already
        fake_free fr{tight, true};
        CHECK(is(kmcf_sub_form_one_rank(2048, 1048577, (size_t)528 * 4096, 0, A, fr), true, false) && fr.calls == 0, "capacity suffices");
        fake_free fr2{tight, true};
        CHECK(is(kmcf_sub_form_one_rank(2048, 1048577, (size_t)528 * 4096 - 1, 0, A, fr2), true, true) && fr2.calls == 1, "capacity one short");
    }
    {   // ... unreadable: dense
        fake_free fr{0, false};
        CHECK(is(kmcf_sub_form_one_rank(2048, 1048577, 0, 0, A, fr), true, false) && fr.calls == 1, "free memory unreadable");
    }
    {   // short of memory: jagged when that fits, else bitmap; what the jagged values hold already counts
        fake_free a{tight, true}, b{tight, true}, c{tight, true}, d{tight, true};
        CHECK(is(kmcf_sub_form_one_rank(2048, 1048577, 0, 0, A, a), true, true) && a.calls == 1, "shortage, a quarter full -> jagged");
        CHECK(is(kmcf_sub_form_one_rank(2048, 4194304, 0, 0, A, b), false, false) && b.calls == 1, "shortage, full -> bitmap");
        CHECK(is(kmcf_sub_form_one_rank(2048, 4194304, 0, 95968, A, c), true, true) && c.calls == 1, "shortage, full, jagged capacity -> jagged");
        CHECK(is(kmcf_sub_form_one_rank(2048, 4194304, 0, 95967, A, d), false, false), "shortage, full, jagged capacity one short -> bitmap");
    }
    {   // the knob
        fake_free fr{plenty, true};
        CHECK(is(kmcf_sub_form_one_rank(100, 5000, 0, 0, 0, fr), false, false), "knob 0");
        CHECK(is(kmcf_sub_form_one_rank(100, 5000, 0, 0, 1, fr), true, false), "knob 1");
        CHECK(is(kmcf_sub_form_one_rank(100, 5000, 0, 0, 2, fr), true, true), "knob 2");
        CHECK(fr.calls == 0, "100 points: the rule says bitmap, %d calls", fr.calls);
        CHECK(is(kmcf_sub_form_one_rank(2048, 4194304, 0, 0, 0, fr), false, false), "knob 0 on a full block");
        fake_free sh{tight, true};
        CHECK(is(kmcf_sub_form_one_rank(2048, 1048577, 0, 0, 1, sh), true, false) && sh.calls == 1, "knob 1 under the shortage");
        CHECK(is(kmcf_sub_form_one_rank(131073, 131073LL * 131073, 0, 0, 1, fr), false, false), "knob 1 beyond KMCF_MAX_PARTIALS block rows");
        CHECK(is(kmcf_sub_form_one_rank(131072, 131072LL * 131072, (size_t)1 << 62, 0, 1, fr), true, false), "knob 1 at KMCF_MAX_PARTIALS block rows");
    }
}

static void rule_group()
{
    const int A = KMCF_SUB_AUTO, P = 3, n_t = 2048;
    // a rank's share: (528 / 3 + 32) tiles and their parts, 33 792 bytes each
    const double share = (528.0 / 3 + 32) * 33792.0;
    {
        fake_free fr{(size_t)1 << 40, true};
        CHECK(kmcf_sub_group_vote(n_t, P, 0, 0, fr) == KMCF_SUB_NO_VOTE && fr.calls == 0, "knob 0: no vote");
    }
    {   // fits through the capacity held (doubles), free memory not read
        fake_free fr{0, true};
        CHECK(kmcf_sub_group_vote(n_t, P, (size_t)(share / 8), A, fr) == KMCF_SUB_FITS && fr.calls == 0, "fits by capacity");
        CHECK(kmcf_sub_group_vote(n_t, P, (size_t)(share / 8) - 1, A, fr) == KMCF_SUB_NO_FIT && fr.calls == 1, "capacity one short, nothing free");
    }
    {   // fits through share <= 0.6 free
        fake_free a{(size_t)(share / 0.6) + 16, true}, b{(size_t)(share / 0.6) - 16, true}, c{(size_t)1 << 40, false};
        CHECK(kmcf_sub_group_vote(n_t, P, 0, A, a) == KMCF_SUB_FITS && a.calls == 1, "fits by free memory");
        CHECK(kmcf_sub_group_vote(n_t, P, 0, A, b) == KMCF_SUB_NO_FIT && b.calls == 1, "does not fit");
        CHECK(kmcf_sub_group_vote(n_t, P, 0, 1, c) == KMCF_SUB_NO_FIT && c.calls == 1, "free memory unreadable: does not fit");
    }
    CHECK(!kmcf_sub_group_spread(n_t, 700, 4194304.0, false, A), "one rank does not fit: bitmap for all");
    CHECK(!kmcf_sub_group_spread(n_t, 700, 4194304.0, false, 1), "one rank does not fit: bitmap for all, whatever the knob");
    CHECK(kmcf_sub_group_spread(100, 30, 5000.0, true, 2), "knob 2: dense tiles, spread (a group has no jagged form)");
    CHECK(kmcf_sub_group_spread(100, 30, 5000.0, true, 1), "knob 1");
    CHECK(kmcf_sub_group_spread(n_t, 700, 1048577.0, true, A), "2048 points above a quarter: spread");
    CHECK(!kmcf_sub_group_spread(n_t, 700, 1048576.0, true, A), "2048 points, a quarter: bitmap");
    CHECK(!kmcf_sub_group_spread(2047, 700, 2047.0 * 2047, true, A), "2047 points: bitmap");
    CHECK(kmcf_sub_group_spread(1 << 20, 2048 * 256, 1e12, true, A), "own points: 2048 partials");
    CHECK(!kmcf_sub_group_spread(1 << 20, 2048 * 256 + 1, 1e12, true, A), "own points beyond 2048 partials: bitmap");
}

int main()
{
    deal_explicit();
    deal_properties();
    rule_one_rank();
    rule_group();
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::printf("subplan ok\n");
    return 0;
}
