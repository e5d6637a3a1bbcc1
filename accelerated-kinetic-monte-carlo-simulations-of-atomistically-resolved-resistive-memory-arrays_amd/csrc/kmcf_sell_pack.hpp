// Packed entry stream of the coded row-per-lane kernel: five 12-bit fields per 8-byte word.
//
// A field is (code << 10) | slot: the 10-bit window slot and the value code (dictionaries of <= 3 values: 2 bits).
// Field f of a word sits at bits 12 f ... 12 f + 11; bits 60 ... 63 are zero.  Entry k of a row goes to step k / 5,
// field k % 5; a row of len entries takes ceil(len / 5) steps.  Times 8, a field is the LDS byte offset of the entry's
// product (the 16-bit stream stores that offset itself: four entries per word).
//
// One definition for the planner, the refresh kernel, the SpMV kernel and the stand-alone test program: plain C++,
// no HIP header needed (the functions are host + device when a HIP compiler reads them).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMCF_PACK_HD __host__ __device__ inline
#else
#define KMCF_PACK_HD inline
#endif

constexpr int KMCF_PACK_FIELDS = 5;        // fields per word
constexpr int KMCF_PACK_BITS = 12;         // bits per field
constexpr int KMCF_PACK_SLOT_BITS = 10;    // of which the window slot
constexpr uint32_t KMCF_PACK_MASK = (1u << KMCF_PACK_BITS) - 1;

// steps (words) of a row of len entries
KMCF_PACK_HD int kmcf_pack_steps(int len) { return (len + KMCF_PACK_FIELDS - 1) / KMCF_PACK_FIELDS; }

KMCF_PACK_HD uint32_t kmcf_pack_field(uint32_t code, uint32_t slot) { return (code << KMCF_PACK_SLOT_BITS) | slot; }

// field f of a word
KMCF_PACK_HD uint32_t kmcf_pack_get(uint64_t w, int f) { return (uint32_t)(w >> (KMCF_PACK_BITS * f)) & KMCF_PACK_MASK; }

// the word with field f replaced (the other fields and bits 60 ... 63 as they were)
KMCF_PACK_HD uint64_t kmcf_pack_put(uint64_t w, int f, uint32_t field)
{
    const int sh = KMCF_PACK_BITS * f;
    return (w & ~((uint64_t)KMCF_PACK_MASK << sh)) | ((uint64_t)(field & KMCF_PACK_MASK) << sh);
}

// the word with the value code of field f replaced (its slot, the other fields and bits 60 ... 63 as they were)
KMCF_PACK_HD uint64_t kmcf_pack_put_code(uint64_t w, int f, uint32_t code)
{
    const int sh = KMCF_PACK_BITS * f + KMCF_PACK_SLOT_BITS;
    constexpr uint64_t cmask = (1u << (KMCF_PACK_BITS - KMCF_PACK_SLOT_BITS)) - 1;
    return (w & ~(cmask << sh)) | (((uint64_t)code & cmask) << sh);
}

// a word whose five fields are all `field` (the padding word: the slot that carries 0.0)
KMCF_PACK_HD uint64_t kmcf_pack_fill(uint32_t field)
{
    uint64_t w = 0;
    for (int f = 0; f < KMCF_PACK_FIELDS; ++f) w = kmcf_pack_put(w, f, field);
    return w;
}

// The five LDS byte offsets (field * 8) of a word given as its two dwords, as the kernel decodes them: the third
// field straddles the dwords (one alignbit).
KMCF_PACK_HD void kmcf_pack_offsets(uint32_t lo, uint32_t hi, uint32_t (&off)[KMCF_PACK_FIELDS])
{
    off[0] = (lo & KMCF_PACK_MASK) << 3;
    off[1] = ((lo >> 12) & KMCF_PACK_MASK) << 3;
    off[2] = (((hi << 8) | (lo >> 24)) & KMCF_PACK_MASK) << 3;
    off[3] = ((hi >> 4) & KMCF_PACK_MASK) << 3;
    off[4] = ((hi >> 16) & KMCF_PACK_MASK) << 3;
}

// Row of len fields into its words: entry k -> word (k / 5) * stride, field k % 5.  The words must hold the padding
// (or anything else whose other fields are to be kept) beforehand.
KMCF_PACK_HD void kmcf_pack_row(const uint16_t *fields, int len, uint64_t *words, long stride)
{
    for (int k = 0; k < len; ++k) {
        uint64_t &w = words[(long)(k / KMCF_PACK_FIELDS) * stride];
        w = kmcf_pack_put(w, k % KMCF_PACK_FIELDS, fields[k]);
    }
}

KMCF_PACK_HD void kmcf_unpack_row(const uint64_t *words, long stride, int len, uint16_t *fields)
{
    for (int k = 0; k < len; ++k)
        fields[k] = (uint16_t)kmcf_pack_get(words[(long)(k / KMCF_PACK_FIELDS) * stride], k % KMCF_PACK_FIELDS);
}
