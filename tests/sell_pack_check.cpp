// Stand-alone check of csrc/kmcf_sell_pack.hpp (tests/test_sell_pack_cpu.py builds it with
// -fsanitize=address,undefined and runs it): rows of every length 0 ... 64 through pack and unpack in the stream's
// lane stride, the extreme field values in every field position with the neighbouring fields and bits 60 ... 63
// untouched, the code-only update of the refresh kernel, the kernel's decode from the two dwords, the step count.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kmcf_sell_pack.hpp"

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

static const uint32_t EXTREMES[] = {0x000, 0xFFF, 0xBFF, 0x555, 0xAAA};     // 0xBFF: slot 1023, code 2

static uint32_t rng_state = 12345u;
static uint32_t rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

int main()
{
    static_assert(KMCF_PACK_FIELDS * KMCF_PACK_BITS == 60, "five 12-bit fields, four spare bits");
    // ---- step count
    for (int len = 0; len <= 64; ++len) {
        int want = 0;
        while (want * 5 < len) ++want;                                   // ceil(len / 5)
        CHECK(kmcf_pack_steps(len) == want, "steps(%d) = %d, want %d", len, kmcf_pack_steps(len), want);
    }
    CHECK(kmcf_pack_steps(52) == 11 && kmcf_pack_steps(53) == 11 && kmcf_pack_steps(64) == 13, "K: 11 steps, row limit: 13");

    // ---- extreme values in every field position, over several backgrounds: neighbours and bits 60 ... 63 untouched
    const uint64_t backgrounds[] = {0ull, 0x0FFFFFFFFFFFFFFFull, 0x0555555555555555ull, 0x0AAAAAAAAAAAAAAAull,
                                    kmcf_pack_fill(0x3FF), 0xF000000000000000ull, 0xFFFFFFFFFFFFFFFFull};
    for (uint64_t bg : backgrounds)
        for (int f = 0; f < KMCF_PACK_FIELDS; ++f)
            for (uint32_t v : EXTREMES) {
                const uint64_t w = kmcf_pack_put(bg, f, v);
                CHECK(kmcf_pack_get(w, f) == v, "put/get field %d value %03x", f, v);
                for (int g = 0; g < KMCF_PACK_FIELDS; ++g)
                    if (g != f) CHECK(kmcf_pack_get(w, g) == kmcf_pack_get(bg, g), "field %d changed by a put into %d", g, f);
                CHECK((w >> 60) == (bg >> 60), "bits 60-63 changed by a put into field %d", f);
                const uint64_t field_mask = (uint64_t)KMCF_PACK_MASK << (12 * f);
                CHECK(((w ^ bg) & ~field_mask) == 0, "bits outside field %d changed", f);
                // the code-only update: the slot bits of the field, and everything else, stay
                for (uint32_t code = 0; code < 4; ++code) {
                    const uint64_t c = kmcf_pack_put_code(w, f, code);
                    CHECK(kmcf_pack_get(c, f) == ((code << 10) | (v & 0x3FF)), "put_code field %d value %03x code %u", f, v, code);
                    CHECK(((c ^ w) & ~((uint64_t)0xC00 << (12 * f))) == 0, "put_code touched bits outside the code of field %d", f);
                }
                // the kernel's decode from the two dwords
                uint32_t off[KMCF_PACK_FIELDS];
                kmcf_pack_offsets((uint32_t)w, (uint32_t)(w >> 32), off);
                for (int g = 0; g < KMCF_PACK_FIELDS; ++g)
                    CHECK(off[g] == 8 * kmcf_pack_get(w, g), "offset of field %d: %u, want %u", g, off[g], 8 * kmcf_pack_get(w, g));
            }
    CHECK(kmcf_pack_fill(0x3FF) == 0x03FF3FF3FF3FF3FFull, "padding word");
    CHECK(kmcf_pack_field(2, 1023) == 0xBFF && kmcf_pack_field(1, 0x155) == 0x555, "field = (code << 10) | slot");

    // ---- rows of every length through pack / unpack, in the stream's layout (64 lanes side by side)
    const long stride = 64;
    for (int len = 0; len <= 64; ++len)
        for (int variant = 0; variant < 7; ++variant) {
            const int steps = kmcf_pack_steps(len);
            // exactly as many words as the row's steps (the sanitizer sees one word too far), lanes 0, 1 and 63 used
            std::vector<uint64_t> words((size_t)(steps > 0 ? (steps - 1) * stride + 64 : 0), kmcf_pack_fill(0x3FF));
            const std::vector<uint64_t> before = words;
            std::vector<uint16_t> in((size_t)len), out((size_t)len, 0xFFFF);
            for (int k = 0; k < len; ++k)
                in[k] = (uint16_t)(variant < 5 ? EXTREMES[(k + variant) % 5] : variant == 5 ? ((k & 1) ? 0xAAA : 0x555) : rnd() & 0xFFF);
            for (int lane : {0, 1, 63}) {
                if (steps == 0) break;
                kmcf_pack_row(in.data(), len, words.data() + lane, stride);
                kmcf_unpack_row(words.data() + lane, stride, len, out.data());
                for (int k = 0; k < len; ++k) CHECK(out[k] == in[k], "len %d lane %d entry %d: %03x, want %03x", len, lane, k, out[k], in[k]);
                // the fields past the row's end still hold the padding; bits 60 ... 63 are zero
                for (int k = len; k < 5 * steps; ++k)
                    CHECK(kmcf_pack_get(words[(size_t)lane + (size_t)(k / 5) * stride], k % 5) == 0x3FF, "len %d: padding field %d", len, k);
                for (int s = 0; s < steps; ++s) CHECK((words[(size_t)lane + (size_t)s * stride] >> 60) == 0, "len %d: bits 60-63 of step %d", len, s);
            }
            // no other lane's word was written
            for (size_t i = 0; i < words.size(); ++i)
                if (i % 64 != 0 && i % 64 != 1 && i % 64 != 63) CHECK(words[i] == before[i], "len %d: word %zu of another lane changed", len, i);
        }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("sell pack ok\n");
    return 0;
}
