// mcq_device.hpp -- per-lane arithmetic of the equity kernels: RNG front ends, search-free dealing from the
// ordered deck, the branch-free 7-card ranking key, and one Monte-Carlo iteration.
//
// Everything here is written against a few tiny primitives (popcount, count-leading-zeros, 32x32 high
// multiply, byte splat) so that the very same source is compiled for gfx950 by hipcc (the product) and, by
// tests/hostsim only, for the host compiler to unit-test the lane arithmetic where no GPU exists.
//
// What it reproduces (reference paths relative to /root/reference):
//   tools/montecarlo_python.py:121-189  dealing order and index semantics (see mcq_iteration)
//   tools/hand_evaluator.py:27-119      _calc_score ordering incl. its quirks (see mcq_eval_key)
//   tools/hand_evaluator.py:20-24       ties go to the first hand = hero
//
// Cost model, measured on gfx950 with tools/ubench (profiles/r01_ubench*.txt): in any instruction stream that
// contains even one non-trivial VALU op per 64 (shift-left, compare, select, popcount, multiply, any 3-operand
// form ...) EVERY wave64 VALU instruction issues in ~4.0-4.3 cycles; the 2.3-cycle rate exists only for pure
// add/and/or/xor/lshr streams.  A random LDS lookup costs ~8.5 cycles of the separate LDS pipe.  So the kernel
// is tuned for INSTRUCTION COUNT: fused 3-operand forms (and_or, or3, bitop3, lshl_or, add3, max3, sad_u8),
// selects where they are shorter than mask arithmetic, and LDS tables (indexed by byte offset, masks kept in
// the pre-shifted "x4 domain") wherever a lookup replaces more than one instruction.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/mcq.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MCQ_HD __host__ __device__ __forceinline__
#define MCQ_HDM __host__ __device__ __forceinline__ /* member functions */
#else
#define MCQ_HD static inline
#define MCQ_HDM inline
#endif

#define MCQ_STREAM_ITERS 16u /* iterations per RNG stream (MCQ-CTR v5) */
#define MCQ_WAVE 64u
#define MCQ_TASK_ITERS (MCQ_STREAM_ITERS * MCQ_WAVE) /* iterations per wave task */
#define MCQ_MAX_OPP 9

// ------------------------------------------------------------------------------------------ primitives
MCQ_HD uint32_t mcq_popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}
MCQ_HD uint32_t mcq_clz(uint32_t x) { /* x != 0 for a meaningful result */
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__clz((int)x);
#else
    return x ? (uint32_t)__builtin_clz(x) : 32u;
#endif
}
MCQ_HD uint32_t mcq_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
// mulhi32(a, b) + 128: draw indices travel as r | 0x80 (r < 64), the form the byte-SWAR hole scan wants, so the
// bias comes for free with the multiply (one v_mad_u64_u32)
MCQ_HD uint32_t mcq_mulhi_p128(uint32_t a, uint32_t b, uint64_t bias /* 128 << 32, see mcq_p128_bias */) {
    return (uint32_t)(((uint64_t)a * b + bias) >> 32);
}
// Both halves of the same product: the high word (biased as above) is returned, the low word -- the fraction that
// feeds the next draw -- goes to `lo`.  The product is made opaque as ONE 64-bit value: otherwise the compiler
// computes the low word a second time (v_mul_lo_u32 beside the v_mad_u64_u32; 32-bit multiplies issue at a quarter
// of the plain VALU rate).
MCQ_HD uint32_t mcq_mulhilo_p128(uint32_t a, uint32_t b, uint64_t bias, uint32_t &lo) {
    uint64_t p = (uint64_t)a * b + bias;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(p));
#endif
    lo = (uint32_t)p;
    uint32_t hi = (uint32_t)(p >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(hi)); /* a 32-bit value from here on: else comparing two of them becomes a 64-bit compare + moves */
#endif
    return hi;
}
// The bias as a value the optimiser cannot see through (device: pinned in a VGPR pair): left to itself the
// compiler re-creates the constant with a v_mov_b64 in front of every multiply (fifteen per 6-max iteration).
MCQ_HD uint64_t mcq_p128_bias() {
    uint64_t x = 128ull << 32;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#endif
    return x;
}
MCQ_HD bool mcq_any(bool pred) { /* true if the predicate holds in any active lane of the wave */
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(pred) != 0;
#else
    return pred;
#endif
}
MCQ_HD uint32_t mcq_rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
// Hide a value from the optimiser (device: pins it in a VGPR): keeps the compiler from re-associating a sum into
// separately shifted parts, so that a table address stays ONE shift-add.
MCQ_HD uint32_t mcq_opaque(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#endif
    return x;
}
// The same for a wave-uniform value (device: pins it in an SGPR).  A condition computed from it is evaluated
// where it is used (one scalar compare) instead of being carried across blocks as a lane mask, which the
// compiler rebuilds with VALU instructions.
MCQ_HD uint32_t mcq_opaque_uniform(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(x));
#endif
    return x;
}
MCQ_HD uint32_t mcq_bfe(uint32_t x, uint32_t off, uint32_t width) { /* (x >> off) & ((1 << width) - 1), off + width <= 32 */
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ubfe(x, off, width);
#else
    return (x >> off) & (width >= 32 ? 0xFFFFFFFFu : ((1u << width) - 1u));
#endif
}
MCQ_HD uint32_t mcq_mul24(uint32_t a, uint32_t b) { /* a, b < 2^24: one v_mul_u32_u24 */
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}
MCQ_HD uint32_t mcq_mad24(uint32_t a, uint32_t b, uint32_t c) { return mcq_mul24(a, b) + c; } /* one v_mad_u32_u24 */
MCQ_HD uint32_t mcq_sad_u8(uint32_t bytes, uint32_t acc) { /* acc + sum of the four bytes */
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(bytes, 0u, acc);
#else
    return acc + (bytes & 0xFFu) + ((bytes >> 8) & 0xFFu) + ((bytes >> 16) & 0xFFu) + (bytes >> 24);
#endif
}
MCQ_HD uint32_t mcq_perm(uint32_t hi, uint32_t lo, uint32_t sel) { /* v_perm_b32: result byte i = byte sel_i of hi:lo
                                                                      (0-3 lo, 4-7 hi), 0 for sel_i = 0x0C */
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t k = (sel >> (8u * i)) & 0xFFu;
        if (k < 8u) r |= (uint32_t)((v >> (8u * k)) & 0xFFu) << (8u * i);
    }
    return r;
#endif
}
MCQ_HD uint32_t mcq_bfi(uint32_t mask, uint32_t a, uint32_t b) { /* (mask & a) | (~mask & b): one v_bfi_b32 */
    return (mask & a) | (~mask & b);
}
MCQ_HD uint32_t mcq_max3(uint32_t a, uint32_t b, uint32_t c) { /* one v_max3_u32 */
    const uint32_t m = a > b ? a : b;
    return m > c ? m : c;
}
MCQ_HD uint32_t mcq_splat_byte(uint32_t x) { /* x < 256 -> x in all four bytes */
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, x, 0u); /* v_perm_b32: every selector byte 0 = byte 0 of x */
#else
    return x * 0x01010101u;
#endif
}

// ------------------------------------------------------------------------------------------ ranking keys
// Internal key = code << 28 | field, unsigned order == Python's order of _calc_score's (score, card_ranks).
// Codes leave a gap at 5; by_type index = code - (code >= 6).  Rank masks live in the "x4 domain" (bit r+2 =
// rank r) so that they are byte offsets into 32-bit LDS tables without a (slow) left shift; a field is
// [13-bit mask << 15][13-bit mask << 2].
#define MCQ_KEY_SHIFT 28
enum { MCQ_C_HIGH = 0, MCQ_C_PAIR = 1, MCQ_C_TWOPAIR = 2, MCQ_C_TRIPS = 3, MCQ_C_STRAIGHT = 4, MCQ_C_FLUSH = 6,
       MCQ_C_FULL = 7, MCQ_C_QUADS = 8, MCQ_C_SF = 9, MCQ_N_CODES = 10 };
MCQ_HD uint32_t mcq_code_to_type(uint32_t code) { return code - (code >= 6u ? 1u : 0u); } /* by_type index */
MCQ_HD uint32_t mcq_key_type(uint32_t key) { return mcq_code_to_type(key >> MCQ_KEY_SHIFT); }

// bit i of the result set <=> ranks i-1 .. i+3 all present (rank -1 = ace playing low)
MCQ_HD uint32_t mcq_straight_runs(uint32_t m) {
    uint32_t m2 = (m << 1) | (m >> 12);
    uint32_t r1 = m2 & (m2 >> 1);
    uint32_t r2 = r1 & (r1 >> 2);
    return r2 & (m2 >> 4);
}

// ------------------------------------------------------------------------------------------ rank-sum hash
// The key of a hand without a flush depends on the MULTISET of its seven ranks only, and a multiset is additive over
// cards: every rank has an integer weight such that all 49 205 multisets (seven cards, at most four of a rank) have
// distinct sums (tools/sum_hash.py chooses and checks them).  The table cards are then one running sum, a hand is
// board sum + hole sum, and the hand's rank comes out of a two-level row-displacement perfect hash,
//     id = hrank[hoff[s & MCQ_SUM_MASK] + (s >> MCQ_SUM_SHIFT)]
// (rows packed first-fit-decreasing by mcq_fill_tables).  The LOW bits of the sum choose the row: the weights grow
// about fourfold from rank to rank, so the high parts of all rows are translates of one self-similar pattern, and
// such rows do not interlock (rows by high bits: the packing stops at load factor 0.26); rows by the low 13 bits hold
// about six entries each, spread over 956 columns, and pack to 0.987.  An id is 16 bits, code << 12 | index: the index numbers the
// keys of one hand type in rising order from 1 (at most 2860 of a type: a pair with three kickers), so ids compare
// exactly as the 32-bit keys of mcq_eval_key do, an id is never 0, and a hand's type code is id >> 12.
#ifndef MCQ_SUM_SHIFT
#define MCQ_SUM_SHIFT 13u
#define MCQ_SUM_ROWS 8192u       /* 1 << MCQ_SUM_SHIFT */
#define MCQ_SUM_SLOTS 50176u     /* the packing ends at slot 49 857: load factor 0.987; hoff + hrank = 114 KB of LDS */
#endif
#define MCQ_SUM_MASK ((1u << MCQ_SUM_SHIFT) - 1u)
#define MCQ_SUM_ROW(s) ((s) & MCQ_SUM_MASK)
#define MCQ_SUM_COL(s) ((s) >> MCQ_SUM_SHIFT)
#define MCQ_SUM_MULTISETS 49205u
#define MCQ_ID_SHIFT 12
MCQ_HD uint32_t mcq_rank_weight(uint32_t rank) { /* rank < 13 */
    constexpr uint32_t kWeight[13] = {0u, 1u, 5u, 22u, 98u, 453u, 2031u, 8698u, 22854u, 83661u, 262349u, 636345u, 1479181u};
    return kWeight[rank];
}

struct McqSumImage { /* one piece, so that it travels global -> LDS as it lies */
    uint16_t hoff[MCQ_SUM_ROWS];   /* row displacement of the rank-sum hash */
    uint16_t hrank[MCQ_SUM_SLOTS]; /* id of the rank multiset whose sum hashes here, 0 in an empty slot */
    uint32_t sel8[256];            /* a copy of McqTables::sel8 */
};
static_assert(sizeof(McqSumImage) % 1024u == 0, "the one-launch kernel sends the image in 1 KB pieces");

// ------------------------------------------------------------------------------------------ lookup tables (LDS)
// sel8: only for laying out the per-query base deck (once per wave task).
// All mask-indexed tables are addressed with x4-domain masks (m4 = m << 2):
//   tops[m] (u32, byte offset m4):  the two-pair / full-house family (F2 in mcq_eval_key) reads it twice.  Bits 2..14:
//           the top set bit of m (x4 domain) -- the family's kicker when m is what the pairs leave over.  Bits 15..30:
//           the upper half of a finished TwoPair key when m is the mask of the ranks held at least twice: the top two
//           set bits of m << 15 | MCQ_C_TWOPAIR << 28; with fewer than two bits in m these are 0 and bit 31 is set
//           instead (never part of a key: it only makes the entry compare above every entry of the trips table below)
//   sd[m]   (u32, byte offset m4):  (straight ? 0x80 | top position 1..10 : 0) << 23, i.e. the complete
//           Straight key (0 without a straight); masks of at most four ranks cannot hold a straight and carry the
//           FourOfAKind key's field instead: the top two set bits of m (x4 domain, 0 if fewer than two) -- below every
//           key such a hand can have (at most four ranks in seven cards: two pairs at least) until the quads bit joins it
//   sd[8192 + m] ("kc", byte offset 32768 + m4, folded into the read instruction's offset field): the low part of
//           the HighCard / Pair / ThreeOfAKind key when m is the mask of the ranks held exactly once: m without
//           its two lowest set bits (the kickers that count) | the type code << 28, which the number of kickers
//           gives away for seven cards: 7 -> HighCard, 5 -> Pair, 4 -> ThreeOfAKind; any other count belongs to a
//           higher type whose own candidate key wins (code 0 here)
//   tf[m]   (u32, byte offset m4):  complete key of the SUIT mask m: StraightFlush (all ranks of the suit
//           plus the -1 slot when it holds the ace, hand_evaluator.py:71-80,93), Flush (top five, :98-100), or 0
//           when popcount(m) < 5
struct McqTables { /* order matters on the device: the first 64 KB are reachable through the 16-bit offset field of
                     the LDS read, i.e. the lookups whose index comes straight out of a logic instruction (tops,
                     sd); the index of kc is formed by an xor that takes the table base along.  The kernels of
                     the mask form (extended, exact, showdown) keep tops, sd | kc (the first 96 KB) and sel8 in LDS and read tf from GLOBAL memory
                     through the vector L1: the LDS pipe is their co-limiter and the flush lookup, whose index is
                     the sparsest, is the one that costs least there (measured) */
    uint32_t tops[8192];
    uint32_t sd[16384]; /* [0, 8192) sd, [8192, 16384) kc */
    uint32_t tf[16384]; /* [0, 8192) tf, [8192, 16384) the trips table, read through global memory with tf: for the mask
                           m of the ranks held at least three times the upper half of a finished FullHouse key, top
                           set bit of m << 15 | MCQ_C_FULL << 28, and 0 for m = 0 (see mcq_eval_key) */
    uint32_t sel8[256];
    /* the sum form (see "rank-sum hash" below): what the plain evaluation kernels read instead of tops / sd / tf */
    uint32_t tfid[8192]; /* tf[] as ids: the id of the suit mask's key, 0 when popcount(m) < 5; read from global memory */
    McqSumImage sum;     /* what those kernels keep in LDS */
};
#define MCQ_KC_BYTE_OFFSET 32768u /* kc relative to sd */
#define MCQ_TF_BYTE_OFFSET 98304u /* tf relative to tops = size of the part the evaluation kernels keep in LDS */
static_assert(__builtin_offsetof(McqTables, tops) == 0 && __builtin_offsetof(McqTables, tf) == MCQ_TF_BYTE_OFFSET,
              "McqTables layout");

static inline void mcq_fill_sum_tables(McqTables *t); /* tfid, hoff, hrank: behind the evaluator it restates */
static inline void mcq_fill_tables(McqTables *t) {
    for (uint32_t v = 0; v < 256; v++) {
        uint32_t e = 0, j = 0;
        for (uint32_t b = 0; b < 8; b++)
            if (v >> b & 1) e |= b << (3 * j++);
        t->sel8[v] = e;
    }
    for (uint32_t m = 0; m < 8192; m++) {
        uint32_t runs = mcq_straight_runs(m);
        uint32_t st = runs ? (0x80u | (32u - (uint32_t)__builtin_clz(runs))) : 0;
        uint32_t n = (uint32_t)__builtin_popcount(m);
        uint32_t d2 = m & (m - 1);
        d2 &= d2 - 1; /* m == 0 stays 0 */
        uint32_t hi1 = m ? 0x80000000u >> __builtin_clz(m) : 0, hi2 = 0;
        if (n >= 2) hi2 = hi1 | (0x80000000u >> __builtin_clz(m ^ hi1));
        t->sd[m] = n <= 4 ? hi2 << 2 : st << 23;
        t->sd[8192 + m] = (d2 << 2) | ((n == 5 ? (uint32_t)MCQ_C_PAIR : n == 4 ? (uint32_t)MCQ_C_TRIPS : 0u) << MCQ_KEY_SHIFT);
        t->tops[m] = (hi1 << 2) | (n >= 2 ? (hi2 << 15) | ((uint32_t)MCQ_C_TWOPAIR << MCQ_KEY_SHIFT) : 0x80000000u);
        t->tf[8192 + m] = m ? (hi1 << 15) | ((uint32_t)MCQ_C_FULL << MCQ_KEY_SHIFT) : 0u;
        uint32_t key = 0;
        if (n >= 5) {
            if (runs) {
                key = ((uint32_t)MCQ_C_SF << MCQ_KEY_SHIFT) | (m << 1) | (m >> 12);
            } else {
                uint32_t f = m;
                for (uint32_t k = n; k > 5; k--) f &= f - 1;
                key = ((uint32_t)MCQ_C_FLUSH << MCQ_KEY_SHIFT) | f;
            }
        }
        t->tf[m] = key;
    }
    mcq_fill_sum_tables(t);
}

// ------------------------------------------------------------------------------------------ RNG: MCQ-CTR v5
MCQ_HD void mcq_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                              uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint32_t l0, l1; /* both halves of a product from ONE v_mad_u64_u32 (not v_mul_hi_u32 + v_mul_lo_u32) */
        const uint32_t h0 = mcq_mulhilo_p128(0xD2511F53u, c0, 0ull, l0);
        const uint32_t h1 = mcq_mulhilo_p128(0xCD9E8D57u, c2, 0ull, l1);
        uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct McqXoshiro { /* xoshiro128++ (Blackman & Vigna): the table driver's per-table generator (mcq_tables.cpp) */
    uint32_t s0, s1, s2, s3;
    MCQ_HDM void seed(uint64_t seed, uint64_t qid, uint32_t stream) {
        uint32_t o[4];
        mcq_philox4x32_10((uint32_t)qid, (uint32_t)(qid >> 32), stream, 0x4D435131u, (uint32_t)seed,
                          (uint32_t)(seed >> 32), o);
        s0 = o[0]; s1 = o[1]; s2 = o[2]; s3 = o[3];
        if ((s0 | s1 | s2 | s3) == 0) s0 = 1;
    }
    MCQ_HDM uint32_t next() {
#ifdef MCQ_ABLATE_RNG /* diagnostic timing build: wrong results */
        s0 += 0x9E3779B9u;
        return s0;
#endif
        uint32_t result = mcq_rotl(s0 + s3, 7) + s0;
        uint32_t t = s1 << 9;
        s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3;
        s2 ^= t;
        s3 = mcq_rotl(s3, 11);
        return result;
    }
};

// The production mode's per-stream generator (MCQ-CTR v5): MWC64X -- David B. Thomas' multiply-with-carry generator
// for GPUs: (x, c) -> (lo, hi) of A * x + c, A = 4294883355, output x ^ c, period ~2^63, passes TestU01 BigCrush.
// ONE v_mad_u64_u32, a move of the carry into the addend pair and the output xor: three instructions per word against
// seven of v4's jsf32 (measured on the headline workload: 548 -> 516 VALU instructions per wave-iteration, 6.01 ->
// 5.73 ms).  Its two state words come from the Philox block of (seed, query id, stream).
struct McqMwc64x {
    uint32_t x, c;
    MCQ_HDM void seed(uint64_t seed, uint64_t qid, uint32_t stream) {
        uint32_t o[4];
        mcq_philox4x32_10((uint32_t)qid, (uint32_t)(qid >> 32), stream, 0x4D435131u, (uint32_t)seed,
                          (uint32_t)(seed >> 32), o);
        x = o[0];
        c = o[1] >> 1; /* carry < A; (2^32 - 1, A - 1), the other fixed point, cannot be seeded */
        if ((x | c) == 0) x = 0xf1ea5eedu; /* (0, 0) is a fixed point */
    }
    MCQ_HDM uint32_t next() {
#ifdef MCQ_ABLATE_RNG /* diagnostic timing build: wrong results */
        x += 0x9E3779B9u;
        return x;
#endif
        const uint32_t r = x ^ c;
        const uint64_t t = (uint64_t)4294883355u * x + c;
        x = (uint32_t)t;
        c = (uint32_t)(t >> 32);
        return r;
    }
};
typedef McqMwc64x McqStreamRng;

// Draw policy of the production mode, "MCQ-CTR v5": the reference's dealing law without its re-draw loop.
//   Opponent pair on a deck of length L from ONE word u, d = L - 1:  a = mulhi32(u, d), c = mulhi32(u * d mod 2^32, d)
//   -- (a, c) is uniform on [0, d)^2 up to d^2 / 2^32 -- and (r1, r2) = (a, c) if a != c else (d, a).  That is a
//   bijection from [0, d)^2 onto the pairs the reference accepts (r1 in [0,L), r2 in [0,L-1), r1 != r2;
//   montecarlo_python.py:167-176), so every accepted pair is as likely as after the reference's rejection loop,
//   with no divergent loop on the GPU.  No attempt is ever rejected, hence `passes` = one per opponent per
//   iteration (added by the caller).
//   Table cards, two per word: even draw: u = next(), idx = mulhi32(u, n), w = u * n; odd draw: idx = mulhi32(w, n)
//   (n = deck length - 1: never the last card, montecarlo_python.py:188).  Bias of either <= 2401 / 2^32.
// UNIFORM = true is the opt-in unbiased law (what montecarlo_cython.pyx:188 and
// Montecarlo.cpp:296-312 intend): a = mulhi32(u, L), c = mulhi32(u * L, d), (r1, r2) = (a, c) -- every ordered pair of
// distinct cards -- and table draws over all n = deck length cards.
// All draws are returned as r | 0x80 (see mcq_mulhi_p128).
template <bool UNIFORM>
struct McqCtrDrawsT {
    static constexpr uint32_t kTableShort = UNIFORM ? 0u : 1u; /* table draw range = deck length - kTableShort */
    McqStreamRng rng;
    uint32_t w;
    uint64_t bias; /* mcq_p128_bias(), set once per stream (start) */
    MCQ_HDM void start(uint64_t seed, uint64_t qid, uint32_t stream) {
        w = 0;
        bias = mcq_p128_bias();
        rng.seed(seed, qid, stream);
    }
    template <int P>
    MCQ_HDM void pair(uint32_t L, uint32_t &r1, uint32_t &r2) {
        const uint32_t dd = L - 1u, m1 = UNIFORM ? L : dd;
        const uint32_t u = rng.next();
        uint32_t frac; /* u * m1 mod 2^32 */
        const uint32_t a = mcq_mulhilo_p128(u, m1, bias, frac); /* (opaque: else a == c becomes a 64-bit compare + moves) */
        const uint32_t c = mcq_mulhi_p128(frac, dd, bias);
        r1 = (!UNIFORM && a == c) ? dd + 128u : a;
        r2 = c;
    }
    template <int K>
    MCQ_HDM uint32_t table(uint32_t n) {
        if ((K & 1) == 0) {
            const uint32_t u = rng.next();
            return mcq_mulhilo_p128(u, n, bias, w); /* w = u * n mod 2^32 */
        }
        return mcq_mulhi_p128(w, n, bias);
    }
};
typedef McqCtrDrawsT<false> McqCtrDraws;
typedef McqCtrDrawsT<true> McqCtrDrawsUniform;

// Draw policy of the parity mode: the stream walk (mcq_mt.hpp on the device, mcq_replay.hpp on the host) has already
// turned the MT19937 stream into the accepted draw values (one byte each, r | 0x80, draw-major:
// draws[d * stride + iteration]); rejected pairs only count in `passes`, which the walk supplies.
struct McqReplayDraws { /* one iteration, byte by byte */
    static constexpr uint32_t kTableShort = 1u;
    const uint8_t *p; /* &draws[iteration] */
    uint64_t stride;
    template <int P>
    MCQ_HDM void pair(uint32_t, uint32_t &r1, uint32_t &r2) {
        r1 = p[0];
        r2 = p[stride];
        p += 2 * stride;
    }
    template <int K>
    MCQ_HDM uint32_t table(uint32_t) {
        uint32_t v = p[0];
        p += stride;
        return v;
    }
};
// The same for FOUR consecutive iterations of a lane: one 32-bit load per draw row brings the four iterations' bytes
// (a wave reads 256 contiguous bytes per row instead of 64: a quarter of the vector-memory instructions and no
// 64-bit address arithmetic per byte); iteration `k` of the four takes byte k of every word.
MCQ_HD uint32_t mcq_ld32_bytes(const uint8_t *p) { /* device: p is 4-aligned (rows start at multiples of 64) */
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t *>(p);
#else
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
#endif
}
struct McqReplayDraws4 {
    static constexpr uint32_t kTableShort = 1u;
    uint32_t ow[2 * MCQ_MAX_OPP], tw[5];
    uint32_t sh; /* 8 * k */
    MCQ_HDM void load(const uint8_t *first /* &draws[4-aligned iteration] */, uint64_t stride, uint32_t n_opp, uint32_t n_deal) {
#pragma unroll
        for (int P = 0; P < MCQ_MAX_OPP; P++)
            if ((uint32_t)P < n_opp) {
                ow[2 * P] = mcq_ld32_bytes(first + (uint64_t)(2 * P) * stride);
                ow[2 * P + 1] = mcq_ld32_bytes(first + (uint64_t)(2 * P + 1) * stride);
            }
        const uint8_t *t = first + (uint64_t)(2u * n_opp) * stride;
#pragma unroll
        for (int K = 0; K < 5; K++)
            if ((uint32_t)K < n_deal) tw[K] = mcq_ld32_bytes(t + (uint64_t)K * stride);
    }
    template <int P>
    MCQ_HDM void pair(uint32_t, uint32_t &r1, uint32_t &r2) {
        r1 = mcq_bfe(ow[2 * P], sh, 8);
        r2 = mcq_bfe(ow[2 * P + 1], sh, 8);
    }
    template <int K>
    MCQ_HDM uint32_t table(uint32_t) { return mcq_bfe(tw[K], sh, 8); }
};

// ------------------------------------------------------------------------------------------ base deck
// k-th set bit of the 52-bit deck mask (card-id order = the reference's list order), cleared afterwards.
// Only used to lay out the per-query base deck once per wave task; the per-draw work is search-free (below).
MCQ_HD uint32_t mcq_select_pop(uint32_t &dlo, uint32_t &dhi, uint32_t k, const uint32_t *sel8) {
    uint32_t c = mcq_popc(dlo);
    bool up = k >= c;
    uint32_t w = up ? dhi : dlo;
    k = up ? k - c : k;
    uint32_t base = up ? 32u : 0u;
    c = mcq_popc(w & 0xFFFFu);
    bool u = k >= c;
    w = u ? w >> 16 : w;
    k = u ? k - c : k;
    base += u ? 16u : 0u;
    c = mcq_popc(w & 0xFFu);
    u = k >= c;
    w = u ? w >> 8 : w;
    k = u ? k - c : k;
    base += u ? 8u : 0u;
    uint32_t e = sel8[w & 0xFFu];
    uint32_t pos = base + ((e >> (3 * (k & 7u))) & 7u);
    uint32_t bit = 1u << (pos & 31u);
    dlo &= up ? 0xFFFFFFFFu : ~bit;
    dhi &= up ? ~bit : 0xFFFFFFFFu;
    return pos;
}

// One card as the evaluator wants it (16 bytes: one ds_read_b128 per dealt card).
struct __attribute__((aligned(16))) McqCard {
    uint32_t rb;  /* 4 << rank (x4 domain) */
    uint32_t cnt; /* 1 << 4*suit: packed per-suit counters */
    uint32_t los; /* suit-major bit, pre-shifted left by 2 (tf[] byte offset): clubs bits 2..14, diamonds 18..30 */
    uint32_t his; /* hearts bits 2..14, spades bits 18..30 */
};

MCQ_HD McqCard mcq_card(uint32_t c) { /* c < 52 */
    const uint32_t rank = c >> 2, suit = c & 3u;
    McqCard e;
    e.rb = 4u << rank;
    e.cnt = 1u << (4u * suit);
    const uint32_t bit = 4u << (rank + 16u * (suit & 1u));
    e.los = suit < 2 ? bit : 0u;
    e.his = suit < 2 ? 0u : bit;
    return e;
}

// ------------------------------------------------------------------------------------------ evaluator
// A hand is (table cards) + (two hole cards).  The table part is accumulated once per iteration:
//   any/ge2/ge3/eq4: ranks present at least once / twice / three times / four times; cnt: packed suit counters;
//   los/his: suit-major masks (pre-shifted).  Adding a card with rank bit r: eq4 |= ge3 & r; ge3 |= ge2 & r; ...
struct McqBoard {
    uint32_t any, ge2, ge3, eq4, cnt, los, his;
    MCQ_HDM void clear() { any = ge2 = ge3 = eq4 = cnt = los = his = 0; }
    MCQ_HDM void add(const McqCard &c) {
        eq4 |= ge3 & c.rb;
        ge3 |= ge2 & c.rb;
        ge2 |= any & c.rb;
        any |= c.rb;
        cnt += c.cnt;
        los |= c.los;
        his |= c.his;
    }
};

struct McqHole { /* two hole cards: B = r1 | r2, P = r1 & r2 (pocket pair) */
    uint32_t B, P, los, his;
    MCQ_HDM void set(const McqCard &a, const McqCard &b) {
        B = a.rb | b.rb;
        P = a.rb & b.rb;
        los = a.los | b.los;
        his = a.his | b.his;
    }
};

// Only a suit with at least three table cards can make a flush, and five table cards hold at most one such
// suit.  psel is the byte selector (mcq_perm) that takes that suit's 16-bit field out of a (his, los) pair -- clubs
// bytes 0-1 of los, diamonds 2-3, hearts bytes 0-1 of his, spades 2-3 -- in ONE instruction per hand; bfl4 is the
// table's mask in it.  Without such a suit the field of clubs is taken: table + hole then hold fewer than five bits
// and tf[] = 0.
MCQ_HD uint32_t mcq_suit_psel(uint32_t s) { /* s = 0..3: clubs, diamonds, hearts, spades */
    return mcq_mad24(s, 0x0202u, 0x0C0C0100u); /* + 0x0404: hearts or spades, his; + 0x0202: diamonds or spades, upper half-word */
}
struct McqFlushSel {
    uint32_t psel, bfl4;
    /* the same, and the suit itself (0 without one): what an opponent's card is read by (hole_by_suit of the deck accessors) */
    template <class Board>
    MCQ_HDM uint32_t from_board_suit(const Board &b) {
        const uint32_t f = (b.cnt + 0x5555u) & 0x8888u; /* bit 4s+3 <=> suit s has >= 3 table cards: one bit at most */
        /* f * 0x0123 = 0x0123 << (4s + 3): its bits 15-16 are nibble 3 - s of the constant = s, and 0 for f = 0.  No compare,
         * no select (those went through VCC and its wait states): and, 24-bit multiply, bit-field extract, multiply-add */
        const uint32_t s = mcq_bfe(mcq_mul24(f, 0x0123u), 15u, 2u);
        psel = mcq_suit_psel(s);
        bfl4 = mcq_perm(b.his, b.los, psel);
        return s;
    }
    template <class Board>
    MCQ_HDM void from_board(const Board &b) { (void)from_board_suit(b); }
};

// Table lookups by BYTE offset (x4-domain masks; never shifted left here).
MCQ_HD uint32_t mcq_ld_u32(const uint32_t *t, uint32_t byte_off) {
    return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(t) + byte_off);
}
MCQ_HD uint32_t mcq_ld_lo16(const uint32_t *t, uint32_t byte_off) { /* the entry's low half-word, zero-extended */
    /* (opaque: told that the upper half is zero, the compiler narrows the masks of the bit-field insert that takes
     * this value and emits three instructions for it) */
    return mcq_opaque(*reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(t) + byte_off));
}

// Key of table + hole = the maximum of four candidate keys (mcq_eval_cands).  Branch-free: every family of hand
// types yields a candidate that is the hand's key when the family applies and a smaller number when it does not:
//   F1  HighCard / Pair / ThreeOfAKind: (pair or trips rank) then the kickers = all other ranks minus the two
//       lowest (hand_evaluator.py:104-106, 110-115)
//   F2  TwoPair (two best pairs, kicker = best of the rest incl. a third pair, :39-42, 107-109) and
//       FullHouse (trips, best remaining pair or second trips, :36-38)
//   flush / straight flush (table tf)
//   straight (top rank decides, wheel lowest, :52-58) and FourOfAKind = the two highest distinct ranks of all
//       seven cards (:43-46): one candidate, because seven cards with quads hold four ranks at most and no straight.
// No condition is tested that a table entry already decides (see McqTables): F2 has one compare, between the entries
// of its two first lookups, and no candidate is cleared -- what a family leaves when it does not apply stays below
// 2^15, under every key of seven cards, or carries a code below the hand's true one.
// All masks below are x4-domain.
MCQ_HD void mcq_eval_cands(const McqBoard &b, const McqFlushSel &fs, const McqHole &h, const uint32_t *tf,
                           const uint32_t *tops, const uint32_t *sd, uint32_t (&cand)[4]) {
#ifdef MCQ_ABLATE_EVAL /* diagnostic timing build: wrong results */
    cand[0] = (b.any ^ h.B ^ (h.los >> 3)) | (1u << MCQ_KEY_SHIFT);
    cand[1] = cand[2] = cand[3] = 0u;
    return;
#endif
    const uint32_t any = b.any | h.B;
    const uint32_t ge2 = b.ge2 | (b.any & h.B) | h.P;
    const uint32_t ge3 = b.ge3 | (b.ge2 & h.B) | (b.any & h.P);
    const uint32_t eq4 = b.eq4 | (b.ge3 & h.B) | (b.ge2 & h.P);

    /* lookups first: their latency overlaps the arithmetic below */
    const uint32_t e_ge2 = mcq_ld_u32(tops, ge2);
    /* the trips table lies behind tf: in the kernels tf is the GLOBAL image, and the vector-memory path takes this
     * second sparse lookup off the LDS pipe as well (ge3 is zero for 19 hands in 20: one cache line); measured
     * 7.17 -> 7.04 ms, a third lookup there loses */
    const uint32_t e_ge3 = mcq_ld_u32(tf + 8192, ge3);
    const uint32_t d_any = mcq_ld_u32(sd, any);
    const uint32_t d_kick = mcq_ld_u32(sd, (any ^ ge2) + MCQ_KC_BYTE_OFFSET); /* kickers | type code of family F1 */
    cand[2] = mcq_ld_u32(tf, fs.bfl4 | mcq_perm(h.his, h.los, fs.psel)); /* tf: LDS or global */

    cand[0] = (ge2 << 13) | d_kick;

    /* F2.  e_ge3 > e_ge2 <=> trips AND a second rank held twice (0 < TwoPair entries < FullHouse entries < entries
     * of fewer than two ranks): the full house.  Either entry's bits 15..30 are the key's upper half and its first
     * field H; the kicker is the top of what H leaves of the ranks held twice (full house) or at all (two pairs).
     * Neither: e_ge2 has no upper half, and the candidate is one rank bit in the lower field. */
    const bool fh = e_ge3 > e_ge2;
    const uint32_t e_H = fh ? e_ge3 : e_ge2;
    const uint32_t R = (fh ? ge2 : any) ^ ((e_H >> 13) & 0x7FFCu);
    cand[1] = mcq_bfi(0x7FFF8000u, e_H, mcq_ld_lo16(tops, R)); /* (a 16-bit read: bit 31 of that entry stays out) */

    /* quads (0.17 % of hands) cost two instructions and no lookup of their own: bit 31 = MCQ_C_QUADS << 28 is the
     * sign of -eq4, and sd[any] is the rest of that key whenever eq4 != 0 */
    cand[3] = ((0u - eq4) & ((uint32_t)MCQ_C_QUADS << MCQ_KEY_SHIFT)) | d_any;
}

MCQ_HD uint32_t mcq_eval_key(const McqBoard &b, const McqFlushSel &fs, const McqHole &h, const uint32_t *tf,
                             const uint32_t *tops, const uint32_t *sd) {
    uint32_t c[4];
    mcq_eval_cands(b, fs, h, tf, tops, sd, c);
    const uint32_t k = mcq_max3(c[0], c[1], c[2]);
    return k > c[3] ? k : c[3];
}

// ------------------------------------------------------------------------------------------ evaluator, sum form
// What the plain path (mcq_iteration) runs.  A card is the same 16 bytes with the rank's WEIGHT in place of its bit
// (McqCard::rb), so the table is one add per card and a hand one add and two dependent 16-bit LDS reads.
MCQ_HD McqCard mcq_card_sum(uint32_t c) { /* c < 52 */
    McqCard e = mcq_card(c);
    e.rb = 2u * mcq_rank_weight(c >> 2); /* doubled: the sum's low bits are the byte offset of a 16-bit hoff entry as they are */
    return e;
}
struct McqSumBoard {
    uint32_t sum, cnt, los, his;
    MCQ_HDM void clear() { sum = cnt = los = his = 0; }
    MCQ_HDM void add(const McqCard &c) {
        sum += c.rb;
        cnt += c.cnt;
        los |= c.los;
        his |= c.his;
    }
};
struct McqSumHole {
    uint32_t ksum, los, his;
    MCQ_HDM void set(const McqCard &a, const McqCard &b) {
        ksum = a.rb + b.rb;
        los = a.los | b.los;
        his = a.his | b.his;
    }
};
struct McqSumTabs {
    const uint16_t *hoff, *hrank; /* LDS in the kernels */
    const uint32_t *tfid;         /* global memory, as tf is for the mask form */
};
/* the sum-form tables of the McqTables object whose tf member `tf` points at (host builds of the lane code) */
MCQ_HD McqSumTabs mcq_sum_tabs_of(const uint32_t *tf) {
    const McqTables *t = reinterpret_cast<const McqTables *>(reinterpret_cast<const char *>(tf) - MCQ_TF_BYTE_OFFSET);
    const McqSumTabs s = {t->sum.hoff, t->sum.hrank, t->tfid};
    return s;
}
MCQ_HD uint32_t mcq_ld_u16(const uint16_t *t, uint32_t byte_off) {
    return *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(t) + byte_off);
}
// The two ids of table + hole: of the rank multiset (never 0) and of the flush suit (0 without a flush); the hand's
// id is the greater one.  In two steps, so that a caller with several hands can send every hand's first reads before any
// second one (mcq_iteration_sum): mcq_sum_first sends the flush lookup and the row's displacement, mcq_sum_rank the
// slot's id.
MCQ_HD void mcq_sum_first(const McqSumBoard &b, const McqFlushSel &fs, const McqSumHole &h, const McqSumTabs &t,
                          uint32_t &s, uint32_t &d, uint32_t &flush_id) {
    s = b.sum + h.ksum; /* twice the multiset's sum (mcq_card_sum) */
    flush_id = mcq_ld_u32(t.tfid, fs.bfl4 | mcq_perm(h.his, h.los, fs.psel));
    d = mcq_ld_u16(t.hoff, s & (MCQ_SUM_MASK << 1));
}
MCQ_HD uint32_t mcq_sum_rank(const McqSumTabs &t, uint32_t s, uint32_t d) {
    return mcq_ld_u16(t.hrank, (d + (s >> (MCQ_SUM_SHIFT + 1u))) << 1);
}
MCQ_HD void mcq_sum_ids(const McqSumBoard &b, const McqFlushSel &fs, const McqSumHole &h, const McqSumTabs &t,
                        uint32_t &rank_id, uint32_t &flush_id) {
#ifdef MCQ_ABLATE_EVAL /* diagnostic timing build: wrong results */
    rank_id = ((b.sum ^ h.ksum ^ (h.los >> 3)) & 0xFFFu) | (1u << MCQ_ID_SHIFT);
    flush_id = 0u;
    return;
#endif
    uint32_t s, d;
    mcq_sum_first(b, fs, h, t, s, d, flush_id);
    rank_id = mcq_sum_rank(t, s, d);
}
MCQ_HD uint32_t mcq_sum_key(const McqSumBoard &b, const McqFlushSel &fs, const McqSumHole &h, const McqSumTabs &t) {
    uint32_t r, f;
    mcq_sum_ids(b, fs, h, t, r, f);
    return r > f ? r : f;
}
MCQ_HD uint32_t mcq_id_type(uint32_t id) { return mcq_code_to_type(id >> MCQ_ID_SHIFT); }

// ------------------------------------------------------------------------------------------ sum-form tables
// Host only, deterministic: mcq_eval_key (without a flush) over every rank multiset and every non-zero tf[] entry give
// the set of keys; sorted and numbered per type code they are the ids.  The rows of the hash are packed
// first-fit-decreasing (most entries first, ties by row number; every row at the lowest displacement that fits).
// Returns false if the tables do not fit their sizes (never, for the constants above: tests/test_sum_hash_host.py).
static inline bool mcq_fill_sum_tables_checked(McqTables *t, uint32_t *n_ids_by_code /* MCQ_N_CODES, or null */) {
    struct Entry { uint32_t sum, key; };
    std::vector<Entry> ms;
    ms.reserve(MCQ_SUM_MULTISETS);
    /* all multisets: a count per rank, at most four, seven in all (ranks in rising order, depth first) */
    uint32_t cnt[13] = {0}, left = 7u;
    for (int r = 0;;) {
        if (r == 13 || left == 0u) {
            if (left == 0u) {
                McqCard c[7];
                uint32_t k = 0, sum = 0;
                for (uint32_t q = 0; q < 13; q++)
                    for (uint32_t j = 0; j < cnt[q]; j++) {
                        c[k].rb = 4u << q;
                        c[k].cnt = c[k].los = c[k].his = 0u; /* no suits: tf[0] = 0, the flush candidate stays out */
                        k++;
                        sum += mcq_rank_weight(q);
                    }
                McqBoard b;
                b.clear();
                for (int i = 0; i < 5; i++) b.add(c[i]);
                McqFlushSel fs;
                fs.from_board(b);
                McqHole h;
                h.set(c[5], c[6]);
                const Entry e = {sum, mcq_eval_key(b, fs, h, t->tf, t->tops, t->sd)};
                ms.push_back(e);
            }
            /* back to the last rank whose count can still grow */
            for (r--; r >= 0 && (cnt[r] == 4u || left == 0u); r--) {
                left += cnt[r];
                cnt[r] = 0u;
            }
            if (r < 0) break;
            cnt[r]++;
            left--;
            r++;
        } else {
            r++; /* count 0 of this rank first */
        }
    }
    bool ok = ms.size() == MCQ_SUM_MULTISETS;

    std::vector<uint32_t> keys;
    keys.reserve(ms.size() + 8192u);
    for (const Entry &e : ms) keys.push_back(e.key);
    for (uint32_t m = 0; m < 8192u; m++)
        if (t->tf[m]) keys.push_back(t->tf[m]);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    uint32_t first[MCQ_N_CODES + 1]; /* position of a code's first key */
    for (uint32_t c = 0; c <= MCQ_N_CODES; c++)
        first[c] = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), c << MCQ_KEY_SHIFT) - keys.begin());
    first[MCQ_N_CODES] = (uint32_t)keys.size();
    for (uint32_t c = 0; c < MCQ_N_CODES; c++) {
        const uint32_t n = first[c + 1] - first[c];
        if (n_ids_by_code) n_ids_by_code[c] = n;
        ok = ok && n < (1u << MCQ_ID_SHIFT); /* index 1..n */
    }
    auto id_of = [&](uint32_t key) -> uint32_t {
        const uint32_t pos = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), key) - keys.begin());
        const uint32_t code = key >> MCQ_KEY_SHIFT;
        return (code << MCQ_ID_SHIFT) | (pos - first[code] + 1u);
    };
    for (uint32_t m = 0; m < 8192u; m++) t->tfid[m] = t->tf[m] ? id_of(t->tf[m]) : 0u;

    /* rows of the hash, by number of entries */
    std::sort(ms.begin(), ms.end(), [](const Entry &a, const Entry &b) {
        return MCQ_SUM_ROW(a.sum) != MCQ_SUM_ROW(b.sum) ? MCQ_SUM_ROW(a.sum) < MCQ_SUM_ROW(b.sum) : a.sum < b.sum;
    });
    for (size_t i = 1; i < ms.size(); i++) ok = ok && ms[i].sum != ms[i - 1].sum;
    std::vector<uint32_t> row_lo(MCQ_SUM_ROWS + 1u, 0u); /* entries of row r: ms[row_lo[r] .. row_lo[r + 1]), columns rising */
    for (const Entry &e : ms) row_lo[MCQ_SUM_ROW(e.sum) + 1u]++;
    for (uint32_t r = 0; r < MCQ_SUM_ROWS; r++) row_lo[r + 1u] += row_lo[r];
    std::vector<uint32_t> order(MCQ_SUM_ROWS);
    for (uint32_t r = 0; r < MCQ_SUM_ROWS; r++) order[r] = r;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return row_lo[a + 1u] - row_lo[a] > row_lo[b + 1u] - row_lo[b];
    });
    /* nxt[i]: a slot >= i below which, from i on, nothing is free (followed and shortened as in a union-find): the
     * search for a row's place only visits displacements that put the row's first entry on a free slot */
    std::vector<uint32_t> nxt(MCQ_SUM_SLOTS + 1u);
    for (uint32_t i = 0; i <= MCQ_SUM_SLOTS; i++) nxt[i] = i;
    auto next_free = [&](uint32_t i) -> uint32_t {
        while (nxt[i] != i) {
            nxt[i] = nxt[nxt[i]];
            i = nxt[i];
        }
        return i;
    };
    for (uint32_t i = 0; i < 256u; i++) t->sum.sel8[i] = t->sel8[i];
    for (uint32_t i = 0; i < MCQ_SUM_ROWS; i++) t->sum.hoff[i] = 0;
    for (uint32_t i = 0; i < MCQ_SUM_SLOTS; i++) t->sum.hrank[i] = 0;
    for (uint32_t oi = 0; oi < MCQ_SUM_ROWS && ok; oi++) {
        const uint32_t r = order[oi], lo = row_lo[r], hi = row_lo[r + 1u];
        if (lo == hi) break; /* empty rows: displacement 0, never read */
        const uint32_t col0 = MCQ_SUM_COL(ms[lo].sum), col1 = MCQ_SUM_COL(ms[hi - 1u].sum);
        uint32_t d = 0;
        for (;; d++) {
            const uint32_t at = next_free(d + col0 < MCQ_SUM_SLOTS ? d + col0 : MCQ_SUM_SLOTS);
            d = at - col0;
            if (d + col1 >= MCQ_SUM_SLOTS || d > 0xFFFFu) { ok = false; break; }
            bool fits = true;
            for (uint32_t k = lo + 1u; k < hi && fits; k++) fits = t->sum.hrank[d + MCQ_SUM_COL(ms[k].sum)] == 0u;
            if (fits) break;
        }
        if (!ok) break;
        t->sum.hoff[r] = (uint16_t)d;
        for (uint32_t k = lo; k < hi; k++) {
            const uint32_t slot = d + MCQ_SUM_COL(ms[k].sum);
            nxt[slot] = slot + 1u;
            t->sum.hrank[slot] = (uint16_t)id_of(ms[k].key); /* never 0 */
        }
    }
    return ok;
}
static inline void mcq_fill_sum_tables(McqTables *t) { (void)mcq_fill_sum_tables_checked(t, nullptr); }

// ------------------------------------------------------------------------------------------ one query, one lane
struct McqQueryCtx { /* wave-uniform */
    uint32_t deck_lo, deck_hi; /* remaining deck after removing the known table cards and hero (l.126-161) */
    uint32_t L0;               /* its length: 50 - n_board */
    uint32_t n_opp;            /* n_players - 1 */
    uint32_t n_deal;           /* 5 - n_board table cards still to come */
    uint32_t runs;
    McqHole hero;
    McqBoard board; /* the known table cards */
    McqSumHole hero_s; /* the same two in the sum form (what mcq_iteration reads) */
    McqSumBoard board_s;
};

// The 16-byte query record as four little-endian words (kept in SGPRs by the kernels): bytes 0-1 hole,
// 2-6 board, 7 n_board, 8 n_players, 9-11 reserved, 12-15 runs.  Register-only access: no byte arrays that
// would be indexed at run time (those go to scratch).
struct McqQueryWords {
    uint32_t w0, w1, w2, w3;
    MCQ_HDM uint32_t card(uint32_t k) const { /* k = 0,1: hole; 2..6: board */
        uint64_t v = ((uint64_t)w1 << 32) | w0;
        return (uint32_t)(v >> (8u * k)) & 0xFFu;
    }
    MCQ_HDM uint32_t n_board() const { return w1 >> 24; }
    MCQ_HDM uint32_t n_players() const { return w2 & 0xFFu; }
    MCQ_HDM uint32_t reserved() const { return w2 >> 8; }
    MCQ_HDM uint32_t runs() const { return w3; }
};

MCQ_HD bool mcq_query_valid(const McqQueryWords &q) {
    if (q.n_board() > 5 || q.n_players() < 1 || q.n_players() > 10 || q.reserved() != 0) return false;
    uint64_t seen = 0;
    bool ok = true;
    for (uint32_t i = 0; i < 2u + q.n_board(); i++) {
        uint32_t c = q.card(i);
        ok = ok && c < 52 && !((seen >> (c & 63u)) & 1);
        seen |= 1ull << (c & 63u);
    }
    return ok;
}

MCQ_HD void mcq_query_ctx(const McqQueryWords &q, McqQueryCtx &c) {
    uint64_t deck = (1ull << 52) - 1;
    c.board.clear();
    c.board_s.clear();
    for (uint32_t i = 0; i < q.n_board(); i++) {
        const uint32_t cd = q.card(2u + i);
        deck &= ~(1ull << cd);
        c.board.add(mcq_card(cd));
        c.board_s.add(mcq_card_sum(cd));
    }
    const uint32_t h0 = q.card(0), h1 = q.card(1);
    deck &= ~(1ull << h0);
    deck &= ~(1ull << h1);
    c.hero.set(mcq_card(h0), mcq_card(h1));
    c.hero_s.set(mcq_card_sum(h0), mcq_card_sum(h1));
    c.deck_lo = (uint32_t)deck;
    c.deck_hi = (uint32_t)(deck >> 32);
    c.L0 = 50u - q.n_board();
    c.n_opp = q.n_players() - 1u;
    c.n_deal = 5u - q.n_board();
    c.runs = q.runs();
}

// Scheduling weight of one wave task of a query, in units of 0.01 ns of measured kernel time per task
// (tools/weights_probe.py on MI355X: fit within 6 % over n_players 1..10, n_board 0/3/4/5).  Used only to cut the
// task list into equally expensive contiguous slices, never for results.
MCQ_HD uint32_t mcq_task_weight(const McqQueryWords &q) {
    const uint32_t n = q.n_players(), deal = 5u - q.n_board();
    return 160u + 200u * n + 10u * n * n + deal * (162u - 9u * n);
}
MCQ_HD uint32_t mcq_task_count(const McqQueryWords &q) { /* no overflow for runs up to 2^32 - 1 */
    return q.runs() / MCQ_TASK_ITERS + (q.runs() % MCQ_TASK_ITERS != 0u ? 1u : 0u);
}

// Share `part` of `n_parts` of a query: tasks [t_lo, t_hi) of its `tasks` tasks and the iterations they hold.
// The shares of all parts tile the query, so their tallies add up to the unsplit result (mcq_eval_batch_part).
struct McqPart {
    uint32_t t_lo, t_hi, runs;
};
MCQ_HD McqPart mcq_part(uint32_t tasks, uint32_t runs, uint32_t part, uint32_t n_parts) {
    McqPart p;
    p.t_lo = (uint32_t)((uint64_t)tasks * part / n_parts);
    p.t_hi = (uint32_t)((uint64_t)tasks * (part + 1u) / n_parts);
    const uint64_t a = (uint64_t)p.t_lo * MCQ_TASK_ITERS, b = (uint64_t)p.t_hi * MCQ_TASK_ITERS;
    p.runs = (uint32_t)((b < runs ? b : runs) - (a < runs ? a : runs));
    return p;
}

// Small batches: how finely the 1024-iteration tasks are cut (2^split sub-tasks each).  A lone wave per SIMD is bound
// by the latency of its dependent LDS lookups, so tasks are cut while that leaves at most two waves per SIMD -- and
// at most 512 waves on one query: every (wave, query) pair ends in twelve atomics on the query's result row, and
// atomics on one address serialise (100k runs: 31 us uncut, 18 us in 392 pieces, 29 us in 1568).  The tallies do not
// depend on the cut.  Decided on the host when it sees the queries, by the prep kernel when they live in HBM.
#define MCQ_SPLIT_FROM_PREP 0xFFFFFFFFu /* evaluation kernel argument: read the cut the prep kernel chose */
MCQ_HD uint32_t mcq_pick_split(uint64_t total_tasks, uint64_t max_tasks, uint32_t n_cu, uint32_t split_max) {
    const uint64_t want = 8ull * n_cu;
    uint32_t s = 0;
    while (s < split_max && (total_tasks << (s + 1u)) <= want && (max_tasks << (s + 1u)) <= 512u) s++;
    return s;
}

static inline McqQueryWords mcq_query_words(const mcq_query &q) { /* host side */
    McqQueryWords w;
    __builtin_memcpy(&w, &q, 16);
    return w;
}

// entry l of the base deck = the l-th card of the ordered remaining deck (device: lane l computes entry l), sum form
MCQ_HD McqCard mcq_base_entry(const McqQueryCtx &qc, uint32_t l, const uint32_t *sel8) {
    uint32_t dlo = qc.deck_lo, dhi = qc.deck_hi;
    uint32_t c = mcq_select_pop(dlo, dhi, l, sel8);
    return mcq_card_sum(c < 52u ? c : 0u); /* lanes beyond the deck length write an entry nobody reads */
}

// How an iteration reads the base deck.  `at` = base position + 128, as mcq_draw_opp / mcq_draw_table return it (the bias
// is folded into the pointer).  card(): a table card, all four fields; hole_card(): an opponent's card, whose suit counter
// nobody reads.
// hole_by_suit(): an opponent's card as the straight forms of mcq_iteration_sum read it, AFTER the table is dealt and by the
// one suit s that can still make a flush (McqFlushSel::from_board_suit): {a = the rank's doubled weight (McqCard::rb of the
// sum form), b = the card's tfid byte-offset bit if its suit is s, else 0} -- what McqSumHole::set and the v_perm of
// mcq_sum_first extract from the card's four words, the three suits nobody asks for never loaded.  suit_key(s) is how the
// accessor wants the suit named in the reads that follow (a table's byte offset, or s itself).
struct __attribute__((aligned(8))) McqPair {
    uint32_t a, b;
};
MCQ_HD McqPair mcq_hole_entry(const McqCard &c, uint32_t s) { /* from the card's fields: the definition */
    const McqPair e = {c.rb, mcq_perm(c.his, c.los, mcq_suit_psel(s))};
    return e;
}
struct McqDeckAoS { /* 64 entries of 16 bytes (host builds of the lane code) */
    const McqCard *base128;
    MCQ_HDM McqCard card(uint32_t at) const { return base128[at]; }
    MCQ_HDM McqCard hole_card(uint32_t at) const { return base128[at]; }
    MCQ_HDM uint32_t suit_key(uint32_t s) const { return s; }
    MCQ_HDM McqPair hole_by_suit(uint32_t at, uint32_t key) const { return mcq_hole_entry(base128[at], key); }
};
// The kernels' form: two arrays of 8-byte entries, X[e] = (rb, cnt) and Y[e] = (los, his) YOFF entries behind it.  A card
// is two 8-byte reads from ONE address register (Y at an immediate offset).  8-byte reads bank by (address / 4) mod 64 in
// groups of 32 lanes, so 8-byte entries spread over 32 slots and a deck of at most 50 cards puts at most two entries
// (e, e + 32) on a slot: a lane group is never worse than 2-way.  (16-byte entries read whole have 16 slots for 16 lanes
// and about three distinct entries on the fullest.)
// YOFF is the caller's layout.  Where 8 * YOFF is below 2048 or a multiple of 512, the compiler pairs the two reads of a
// table card into ONE two-address instruction (ds_read2_b64 / ds_read2st64_b64), which banks by (address / 4) mod 32 in
// groups of 16 lanes at twice the cycles: the kernels keep YOFF out of that set.
template <uint32_t YOFF>
struct McqDeckSplit {
    const McqPair *x128; /* X - 128 entries */
    MCQ_HDM McqCard card(uint32_t at) const {
        const McqPair x = x128[at], y = x128[at + YOFF];
        const McqCard c = {x.a, x.b, y.a, y.b};
        return c;
    }
    /* rb alone, a 4-byte read at the same address: with cnt loaded and dropped (an 8-byte read for both cards of a pair)
     * the 6-max iteration spills registers */
    MCQ_HDM McqCard hole_card(uint32_t at) const {
        const uint32_t rb = x128[at].a;
        const McqPair y = x128[at + YOFF];
        const McqCard c = {rb, 0u, y.a, y.b};
        return c;
    }
    /* (without a table by suit: from the card's fields) */
    MCQ_HDM uint32_t suit_key(uint32_t s) const { return s; }
    MCQ_HDM McqPair hole_by_suit(uint32_t at, uint32_t key) const { return mcq_hole_entry(hole_card(at), key); }
    /* entry e of both arrays (device: lane e writes it) */
    static MCQ_HDM void put(McqPair *x, uint32_t e, const McqCard &c) {
        const McqPair px = {c.rb, c.cnt}, py = {c.los, c.his};
        x[e] = px;
        x[e + YOFF] = py;
    }
};
// The bulk kernel's form: beside the two arrays a per-wave HOLE TABLE of 8-byte entries mcq_hole_entry(card at position p,
// suit s), p = 0..49, s = 0..3, at byte (p << POS_SHIFT) + s * SUIT_STRIDE: 1600 bytes a wave.  hole_by_suit() is one
// ds_read_b64 whose address is one shift-add of the position and the key; the key is formed once per iteration (a
// multiply-add of the suit: the table's LDS address, the -128 entries of `at` included).
//   position-major  POS_SHIFT 5, SUIT_STRIDE 8:   an entry's bank slot (8-byte reads: 32 slots) is 4 (p mod 8) + s
//   suit-major      POS_SHIFT 3, SUIT_STRIDE 400: four sub-tables of 50 entries back to back, slot (p + 18 s) mod 32
// About 63 % of the lanes read suit 0 (no flush possible, or clubs).  Position-major gives those lanes EIGHT slots for 50
// positions; suit-major all 32, at most two positions on a slot, and the sub-table of the next suit starts on slot 18,
// where the slots that suit 0 fills twice (0..17) end.  Measured: DESIGN.md, section 7, r19.
#define MCQ_HOLE_POSITIONS 50u
#define MCQ_HOLE_WAVE_BYTES (MCQ_HOLE_POSITIONS * 4u * 8u)
template <uint32_t YOFF, uint32_t POS_SHIFT, uint32_t SUIT_STRIDE>
struct McqDeckBySuit : McqDeckSplit<YOFF> {
    static_assert((POS_SHIFT == 5u && SUIT_STRIDE == 8u) || (POS_SHIFT == 3u && SUIT_STRIDE == 8u * MCQ_HOLE_POSITIONS),
                  "position-major or suit-major: either fills the wave's 1600 bytes exactly");
    const char *h128; /* the wave's hole table - (128 << POS_SHIFT) bytes */
    MCQ_HDM uint32_t suit_key(uint32_t s) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return mcq_mad24(s, SUIT_STRIDE, (uint32_t)(uintptr_t)h128); /* an LDS address: the low word of the generic one */
#else
        return s * SUIT_STRIDE;
#endif
    }
    MCQ_HDM McqPair hole_by_suit(uint32_t at, uint32_t key) const {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(3))) const McqPair *LdsPair;
        return *(LdsPair)(uintptr_t)((at << POS_SHIFT) + key);
#else
        return *reinterpret_cast<const McqPair *>(h128 + ((at << POS_SHIFT) + key));
#endif
    }
    /* position e, all four suits (device: lane e < MCQ_HOLE_POSITIONS writes them); h = the wave's hole table */
    static MCQ_HDM void put_holes(char *h, uint32_t e, const McqCard &c) {
#pragma unroll
        for (uint32_t s = 0; s < 4u; s++)
            *reinterpret_cast<McqPair *>(h + (e << POS_SHIFT) + s * SUIT_STRIDE) = mcq_hole_entry(c, s);
    }
};

struct McqLaneAcc {
    static constexpr bool kWays = false, kSeats = false;
    uint64_t types; /* MCQ_N_CODES fields of 6 bits: hero's winning hand codes (<= 16 per lane per task) */
    uint32_t tie;
    uint32_t passes;
};
// The accumulator type is the compile-time switch of mcq_iteration / mcq_iterations: with this one every opponent's
// key is materialised and the iterations hero does not lose are split by how many hands share the pot
// (mcq_result_ways).  Packed as `types` is: field e (6 bits, <= 16 per lane per task) counts the iterations in which
// hero is best together with e opponents, e = 0..9; field 0 repeats the strict wins and is not stored.
#define MCQ_N_WAYS 9u /* tie_ways[k - 2], k = 2..10 hands sharing the pot */
// (No `tie` here: it is the sum of fields 1..9, taken when the lanes are added up -- a register the iteration keeps.)
struct McqLaneAccWays {
    static constexpr bool kWays = true, kSeats = false;
    uint64_t types;
    uint32_t passes;
    uint64_t ways;
};
// The per-seat form (mcq_result_seats; extended queries, mcq_iteration_ext only): every hand's key is compared with the
// best of ALL hands, and each of the k seats holding it is credited.  One word per seat, three fields: share (16 bits:
// at most 16 iterations x 2520 per lane per task), win and tie (5 bits each, <= 16).  The word an iteration adds to each
// level seat depends on k alone: 2520 / k from a table (never a division), plus the win field's unit for k == 1, the tie
// field's otherwise.
#define MCQ_MAX_SEATS 10u
#define MCQ_SEAT_WIN_SHIFT 16u
#define MCQ_SEAT_TIE_SHIFT 21u
struct McqLaneAccSeats {
    static constexpr bool kWays = false, kSeats = true;
    uint32_t passes;
    uint32_t seat[MCQ_MAX_SEATS];
    /* what mcq_iteration_ranges has at the end of an accepted iteration (the seats' hands as card ids, the seats level with
     * the best, their increment): nothing to do here; the per-hand accumulator (mcq_hands.hpp) counts the watched seat's hand */
    MCQ_HDM void dealt(const uint16_t *, uint32_t, uint32_t, uint32_t) {}
};
static_assert(MCQ_STREAM_ITERS * MCQ_SHARE_UNIT < (1u << MCQ_SEAT_WIN_SHIFT) && MCQ_STREAM_ITERS < 32u, "fields of McqLaneAccSeats");
MCQ_HD uint32_t mcq_seat_increment(uint32_t k) { /* k = 1..10 hands share the pot */
    static constexpr uint32_t kInc[MCQ_MAX_SEATS] = {
        2520u | (1u << MCQ_SEAT_WIN_SHIFT), 1260u | (1u << MCQ_SEAT_TIE_SHIFT), 840u | (1u << MCQ_SEAT_TIE_SHIFT),
        630u | (1u << MCQ_SEAT_TIE_SHIFT),  504u | (1u << MCQ_SEAT_TIE_SHIFT),  420u | (1u << MCQ_SEAT_TIE_SHIFT),
        360u | (1u << MCQ_SEAT_TIE_SHIFT),  315u | (1u << MCQ_SEAT_TIE_SHIFT),  280u | (1u << MCQ_SEAT_TIE_SHIFT),
        252u | (1u << MCQ_SEAT_TIE_SHIFT)};
    return kInc[k - 1u];
}

// ------------------------------------------------------------------------------------------ dealing without search
// list.pop(r) on the ordered remaining deck, reformulated so that no k-th-set-bit search is needed:
// the base deck (query's deck minus table cards and hero, wave-uniform) is a table base[0..L0) in LDS; every card
// already dealt in this iteration is a HOLE, remembered by its coordinate t in the CURRENT (shrunk) list, i.e.
// the number of not-yet-dealt cards below it.  Then for a draw r on the current list
//     base position s = r + #{holes with t <= r};   afterwards every hole with t > r moves down by one and the
//     new hole has t = r.
// Holes are independent of each other (no ordering to maintain), so four of them are handled per register with
// byte-SWAR arithmetic: with rb = 0x80808080 | r * 0x01010101, bit 7 of each byte of (rb - h) says t <= r.
// Unused byte slots hold the sentinel 0x7F and are decremented along (23 draws at most: always > 49 >= r).
// This is an exact restatement of montecarlo_python.py:178-179,188 (checked against list.pop in the tests).
#define MCQ_HOLE_SENTINEL 0x7F7F7F7Fu
// A BIASED register (the second one of a pair that mcq_hole_count2 counts with one popcount, see there) stores t + 0x40 in
// every byte.  The three functions that write a register take the bias as a template argument, and it costs no
// instruction in any of them: it is a different constant where there already is one.
//   * Coordinates are at most 49, so a stored coordinate is at most 0x71.
//   * A free slot stores the SAME sentinel, 0x7F: as a coordinate it now stands for 0x3F, and moved down by s scans for
//     0x3F - s, which stays above 49 >= r while s <= 13 (MCQ_BIAS_MAX_SCANS).  The slots of a register fill in rising
//     order, one a draw, so a free slot sees three scans at the most before it is filled or its epoch closes
//     (mcq_plan_slot_scans); a closed register is never scanned again.
//   * With rb = splat(r | 0x80) the byte of rb - h is 0x40 + r - t, in [15, 113] for a hole and in [1, 63] for a free
//     slot: never a borrow into the next byte, bit 7 clear, and bit 6 says t <= r.
#define MCQ_HOLE_BIAS 0x40404040u
#define MCQ_BIAS_MAX_SCANS 13
static_assert(0x40 + 49 <= 0x7F && 0x40 + 0x3F <= 0x7F, "a biased byte never exceeds 0x7F: bit 7 stays clear");
static_assert(0x3F - MCQ_BIAS_MAX_SCANS > 49, "a free slot of a biased register stays above every draw");

// MODE of a scan: MCQ_SCAN_PLAIN; MCQ_SCAN_BIASED; MCQ_SCAN_TO_BIASED, the first scan of a register that mcq_hole_pair wrote
// plain a draw before: it reads the plain bytes and leaves them biased.  Only the two holes take the bias there -- slot 2 is
// filled by this draw's mcq_hole_put, which brings its own, and slot 3 keeps its byte, 0x7D, which is a biased register's
// free slot as it stands -- so the bias joins the constant of the scan's add and the pair's literal stays the one every
// register shares (a second literal is a second move an iteration).
#define MCQ_SCAN_PLAIN 0
#define MCQ_SCAN_BIASED 1
#define MCQ_SCAN_TO_BIASED 2
template <int MODE = MCQ_SCAN_PLAIN>
MCQ_HD void mcq_hole_reg(uint32_t rb, uint32_t &h, uint32_t &k) {
#ifdef MCQ_ABLATE_HOLES /* diagnostic timing build: wrong results */
    k += (rb ^ h) & 1u;
    return;
#endif
    const uint32_t f = ((rb - h) >> (MODE == MCQ_SCAN_BIASED ? 6 : 7)) & 0x01010101u; /* byte i = 1 iff t_i <= r */
    k = mcq_sad_u8(f, k);                             /* k += number of such holes */
    h = h + f - 0x01010101u + (MODE == MCQ_SCAN_TO_BIASED ? MCQ_HOLE_BIAS & 0xFFFFu : 0u); /* every other hole moves down by one */
}

// Store t = r in byte SLOT of a register whose slots fill in rising order: the slot still holds the sentinel, moved down
// once by each scan the register has seen since its slot 0 was filled -- SLOT scans, so 0x7F - SLOT exactly -- and the
// insert is the ADD of (r - that) at the slot's place.  rp = r | 0x80, the draw as it arrives (one byte).  After a scan
// the constant joins the scan's own (h + f - 0x01010101 + constant: one v_add3_u32) and the insert is one v_lshl_add_u32;
// slot 0 of a fresh register is one add of a constant to rp.  (A bit-field insert with the mask as a literal is not
// encodable in the three-operand form: the compiler splits it into an and and a three-operand logic instruction.)
// BIASED: the slot is to hold r + 0x40, which lowers the constant by that much.
template <int SLOT, bool BIASED = false>
MCQ_HD void mcq_hole_put(uint32_t &h, uint32_t rp) {
    constexpr uint32_t sh = 8u * (SLOT & 3);
#ifdef MCQ_ABLATE_HOLES /* diagnostic timing build (wrong results): its scans do not move the sentinel */
    h = mcq_bfi(0x7Fu << sh, rp << sh, h);
    return;
#endif
    h = h + (rp << sh) - ((0x80u + 0x7Fu - (uint32_t)(SLOT & 3) - (BIASED ? 0x40u : 0u)) << sh);
}

// A hole that is ALONE in its register is one comparison, not a scan.  The first draw into a register leaves itself
// there as it arrived (h = rp0 = t0 | 0x80: a copy, no instruction); the second draw finds f = [t0 <= r], k += f, and
// writes the register whole, as a fresh one looks after the insert of rp0 at slot 0, the scan and the insert of rp at
// slot 1: bytes 3 and 2 the sentinel moved down once, byte 1 = r, byte 0 = t0 + f - 1.  Both draws carry the same
// | 0x80, so they compare as they arrive, and their two biases and the -1 fold into the literal: v_cmp_le_u32,
// v_addc_co_u32 (k), v_lshl_add_u32, v_addc_co_u32 (h) -- four instructions for the eight of the scan and the two
// inserts, and the VCC of a vector compare is read at once.  BIASED: bytes 1 and 0 take 0x40 each from the literal (only
// where the register's epoch closes behind this draw: else its next scan biases it, MCQ_SCAN_TO_BIASED).
template <bool BIASED = false>
MCQ_HD void mcq_hole_pair(uint32_t rp, uint32_t &h, uint32_t &k) {
    const uint32_t rp0 = h;
#ifdef MCQ_ABLATE_HOLES /* diagnostic timing build: wrong results */
    k += (rp ^ rp0) & 1u;
    h = (rp << 8) + rp0;
    return;
#endif
    const uint32_t f = rp0 <= rp ? 1u : 0u;
    k = k + f;
    const uint32_t t = mcq_opaque((rp << 8) + rp0);
    uint32_t c = MCQ_HOLE_SENTINEL - 0x01010101u - 0x7E7Eu - 0x8080u - 1u + (BIASED ? MCQ_HOLE_BIAS & 0xFFFFu : 0u); /* 0x7E7D7F7F */
#if defined(__HIP_DEVICE_COMPILE__)
    /* t and the literal pinned in registers, the flag as a carry: left to itself the compiler selects between the literal
     * and the literal + 1 and adds (five instructions, two registers for the pair of constants).  Not volatile: the
     * literal's register is set outside the loop where the compiler finds room. */
    asm("" : "+v"(c));
    unsigned carry_out; /* never set (the sum stays below 2^31) and never read: __builtin_addc is here for its carry IN */
    h = __builtin_addc(t, c, f, &carry_out);
#else
    h = t + c + f;
#endif
}

// Draws arrive as rp = r | 0x80 (r < 64).  Returned: base position + 128 (the caller's table pointer is biased).
// opponent draw number J (0-based; J holes precede it, all in H[0 .. (J+3)/4)).  The first draw into a register (J = 0,
// 4, 8: the first card of a pair) scans the full registers before it and leaves itself in its own, where the pair's
// second card -- the only draw that meets a register holding one hole -- finds it (mcq_hole_pair).
template <int J>
MCQ_HD uint32_t mcq_draw_opp(uint32_t rp, uint32_t (&H)[5]) {
    uint32_t k = rp;
    if (J % 4 == 1) mcq_hole_pair(rp, H[J / 4], k);
    if (J % 4 == 0) H[J / 4] = rp;
    if (J >= 2) {
        const uint32_t rb = mcq_splat_byte(rp);
#pragma unroll
        for (int i = 0; i < (J % 4 < 2 ? J / 4 : J / 4 + 1); i++) mcq_hole_reg(rb, H[i], k);
        if (J % 4 >= 2) mcq_hole_put<J>(H[J / 4], rp);
    }
    return mcq_opaque(k); /* materialise k so that the table address is one shift-add */
}

// Count only: k += number of holes of the register with t <= r (the register is not updated).
MCQ_HD void mcq_hole_count(uint32_t rb, uint32_t h, uint32_t &k) {
#ifdef MCQ_ABLATE_HOLES /* diagnostic timing build: wrong results */
    k += (rb ^ h) & 1u;
    return;
#endif
    k = mcq_opaque(mcq_popc((rb - h) & 0x80808080u) + k); /* v_sub, v_and, v_bcnt with its add (opaque: else the compiler
                                                            counts into zero and sums afterwards: one more add3) */
}
// Two registers of one level with ONE popcount: h0 as it is, h1b biased (MCQ_HOLE_BIAS, see there for why neither
// subtraction borrows).  [t <= p] stands in bit 7 of every byte of pb - h0 and in bit 6 of every byte of pb - h1b, where
// bit 7 is clear; the select takes bit 7 from the first and the rest from the second, and the mask keeps the eight
// indicators: v_sub, v_sub, v_bfi (assembled as v_bitop3), v_and, v_bcnt with its add -- five for six, and one
// instruction of the slow class fewer.  The select's mask is left to the compiler, which keeps it in an SGPR (the
// three-operand form takes a scalar operand, not a literal); pinned in a VGPR it was set anew in every iteration.
MCQ_HD void mcq_hole_count2(uint32_t pb, uint32_t h0, uint32_t h1b, uint32_t &k) {
#ifdef MCQ_ABLATE_HOLES /* diagnostic timing build: wrong results */
    k += (pb ^ h0 ^ h1b) & 1u;
    return;
#endif
    const uint32_t m = mcq_bfi(0x80808080u, pb - h0, pb - h1b) & 0xC0C0C0C0u;
    k = mcq_opaque(mcq_popc(m) + k);
}

// table draw number K (0..4).  Two levels, because the table is dealt after ALL opponents (l.215-217): the K earlier
// table holes live in their own register hb, in coordinates of the current list, and are counted and moved as in
// mcq_hole_reg; that gives the draw's position p in the list as it was when the opponents had been dealt -- and in
// THAT list the opponents' holes (NREGS registers) have fixed coordinates from here on: they are only counted
// against p (3 instructions per register instead of 5) and never moved again.
// NREGS is a template parameter: with a run-time bound the compiler scans all five registers and discards the
// unused ones with selects (7 instructions per register instead of 0).
// The first table draw leaves itself in hb as it arrived; the second one meets it alone there (mcq_hole_pair).
template <int K, int NREGS>
MCQ_HD uint32_t mcq_draw_table(uint32_t rp, const uint32_t (&H)[5], uint32_t &hb) {
    uint32_t p = rp; /* r | 0x80 */
    if (K == 0) {
        hb = rp;
    } else if (K == 1) {
        mcq_hole_pair(rp, hb, p);
    } else {
        const uint32_t rb = mcq_splat_byte(rp);
        mcq_hole_reg(rb, hb, p);
        if (K < 4) mcq_hole_put<K>(hb, rp); /* the hole of a fifth table card is never looked at */
    }
    uint32_t k = p; /* position among the cards the opponents left, still | 0x80 */
    if (NREGS > 0) {
        const uint32_t pb = mcq_splat_byte(p);
#pragma unroll
        for (int i = 0; i < NREGS; i++) mcq_hole_count(pb, H[i], k);
    }
    return mcq_opaque(k);
}

// the missing table cards (montecarlo_python.py:185-189) after opponents whose holes fill NREGS registers
template <int NREGS, class Draws, int NDEAL = -1, class Deck = McqDeckAoS>
MCQ_HD void mcq_deal_table(const McqQueryCtx &qc, Draws &dr, const Deck &deck, const uint32_t (&H)[5], uint32_t L,
                           McqSumBoard &b) {
    uint32_t hb = MCQ_HOLE_SENTINEL;
    /* scalar compares, no lane masks kept in SGPR pairs; NDEAL >= 0: known at compile time, no branches at all */
    const uint32_t n_deal = NDEAL >= 0 ? (uint32_t)NDEAL : mcq_opaque_uniform(qc.n_deal);
    /* A card joins the table one draw late: its LDS read leaves at the end of its block and is waited for behind the
     * next draw's arithmetic (the blocks are separate basic blocks, the compiler cannot move the wait itself). */
    McqCard pend = {0u, 0u, 0u, 0u};
#define MCQ_TABLE(K)                                                                                            \
    if (K < n_deal) {                                                                                           \
        const uint32_t at = mcq_draw_table<K, NREGS>(dr.template table<K>(L - Draws::kTableShort), H, hb); /* l.188 */ \
        if (K > 0) b.add(pend);                                                                                 \
        pend = deck.card(at);                                                                                   \
        L -= 1;                                                                                                 \
    }
    MCQ_TABLE(0) MCQ_TABLE(1) MCQ_TABLE(2) MCQ_TABLE(3) MCQ_TABLE(4)
#undef MCQ_TABLE
    if (n_deal > 0u) b.add(pend);
}

// ------------------------------------------------------------------------------------------ dealing in epochs
// The two-level argument of mcq_draw_table does not depend on where the split is, and it nests.  Cut the N draws of an
// iteration at CHECKPOINTS (a checkpoint c stands before draw c); the draws between two checkpoints are an EPOCH.
//   * Holes of the current epoch move, as in mcq_draw_opp: draw j of its epoch behaves as opponent draw j does on the
//     epoch's own registers, and that gives its position p in the list as it was at the epoch's opening checkpoint.
//   * Holes of a closed epoch keep the coordinates they had in the list at their CLOSING checkpoint and are never written
//     again.  p is mapped through the closed epochs, most recent first, each with p += #{t <= p} -- a count
//     (mcq_hole_count), or one comparison for a hole left alone in its register (it is still the draw as it arrived).
//   * The last draw of all leaves no hole: it only counts, in its own epoch too.
// The base position equals list.pop's for any set of checkpoints (tests/test_epoch_dealing_host.py).  Where the
// checkpoints stand only changes the number of instructions, and that is counted here, in the costs of the code above:
//   moving scan 5 per register; splat 1 per draw and level; insert at slot >= 2: 1; mcq_hole_pair 4; count 3 per register
//   (plus the level's splat); a lone hole compared directly 2.
// The costs depend on the NUMBER of draws alone (an opponent's card and a table card are dealt alike), so a plan is a
// function of n = 2 * NOPP + NDEAL and of the rule:
//   rule 1..4: the cheapest set of at most that many checkpoints (dynamic programme over the last checkpoint);
//   MCQ_DEAL_FULLREG: a checkpoint wherever a register is full ("a full register is never written again").
// 6-max before the flop (15 draws): one checkpoint behind the opponents, the dealing before there were plans, 156;
// {8} 148, {8, 12} 145, {8, 12, 13} 143, every full register {4, 8, 12} 146.
#define MCQ_DEAL_FULLREG 9
#define MCQ_PLAN_MAX_DRAWS (2 * MCQ_MAX_OPP + 5)
#define MCQ_PLAN_MAX_EPOCHS 6
#define MCQ_PLAN_REGS 6 /* hole registers of a plan: what H[5] and hb of the dealing without plans are */
struct McqDealPlan {
    int n_draws, n_epochs;
    int first[MCQ_PLAN_MAX_EPOCHS + 1]; /* draws before epoch e; first[n_epochs] = n_draws */
    int reg0[MCQ_PLAN_MAX_EPOCHS + 1];  /* the epoch's first register; reg0[n_epochs] = registers in all */
    constexpr int epoch_of(int d) const {
        int e = 0;
        while (e + 1 < n_epochs && d >= first[e + 1]) e++;
        return e;
    }
    constexpr int size(int e) const { return first[e + 1] - first[e]; }
};
// registers of `holes` holes that a count reads (two and more holes: sentinels fill the rest) / a hole left alone
constexpr int mcq_plan_count_regs(int holes) { return holes / 4 + (holes % 4 >= 2 ? 1 : 0); }
constexpr bool mcq_plan_lone(int holes) { return holes % 4 == 1; }
// instructions with which a later draw passes a closed epoch of n holes
constexpr int mcq_plan_cost_closed(int n) {
    return (mcq_plan_count_regs(n) > 0 ? 1 + 3 * mcq_plan_count_regs(n) : 0) + (mcq_plan_lone(n) ? 2 : 0);
}
// instructions of draw j of its epoch among the epoch's own holes
constexpr int mcq_plan_cost_own(int j, bool last) {
    if (last) return mcq_plan_cost_closed(j);
    int c = j % 4 == 1 ? 4 : 0;
    if (j >= 2) c += 1 + 5 * (j % 4 < 2 ? j / 4 : j / 4 + 1) + (j % 4 >= 2 ? 1 : 0);
    return c;
}
// an epoch of draws [a, b) of n: its own steps, and what the n - b later draws pay to pass it
constexpr int mcq_plan_cost_epoch(int a, int b, int n) {
    int c = 0;
    for (int d = a; d < b; d++) c += mcq_plan_cost_own(d - a, d == n - 1);
    return c + (n - b) * mcq_plan_cost_closed(b - a);
}
constexpr McqDealPlan mcq_deal_plan(int n, int rule) {
    McqDealPlan pl = {};
    pl.n_draws = n;
    int cps[MCQ_PLAN_MAX_DRAWS + 1] = {}, n_cp = 0;
    if (rule == MCQ_DEAL_FULLREG) {
        for (int c = 4; c < n; c += 4) cps[n_cp++] = c;
    } else {
        /* f[m][b]: cheapest way to deal draws [0, b) in m epochs that are all closed at b (b == n: the last one open) */
        constexpr int kInf = 1 << 28;
        int f[MCQ_PLAN_MAX_EPOCHS + 1][MCQ_PLAN_MAX_DRAWS + 1] = {}, from[MCQ_PLAN_MAX_EPOCHS + 1][MCQ_PLAN_MAX_DRAWS + 1] = {};
        for (int m = 0; m <= rule + 1; m++)
            for (int b = 0; b <= n; b++) f[m][b] = m == 0 && b == 0 ? 0 : kInf;
        for (int m = 1; m <= rule + 1; m++)
            for (int b = 1; b <= n; b++)
                for (int a = 0; a < b; a++) {
                    if (f[m - 1][a] >= kInf) continue;
                    const int c = f[m - 1][a] + mcq_plan_cost_epoch(a, b, n);
                    if (c < f[m][b]) { f[m][b] = c; from[m][b] = a; }
                }
        int best = 1;
        for (int m = 2; m <= rule + 1; m++)
            if (f[m][n] < f[best][n]) best = m; /* fewer checkpoints where more do not pay */
        int b = n;
        for (int m = best; m >= 1; m--) {
            b = from[m][b];
            if (m > 1) cps[m - 2] = b;
        }
        n_cp = best - 1;
    }
    pl.n_epochs = n_cp + 1;
    for (int e = 1; e <= n_cp; e++) pl.first[e] = cps[e - 1];
    pl.first[pl.n_epochs] = n;
    for (int e = 0; e < pl.n_epochs; e++) {
        const int holes = pl.size(e) - (e == pl.n_epochs - 1 ? 1 : 0); /* the last draw leaves none */
        pl.reg0[e + 1] = pl.reg0[e] + (holes + 3) / 4;
    }
    return pl;
}
constexpr int mcq_plan_cost(const McqDealPlan &pl) {
    int c = 0;
    for (int e = 0; e < pl.n_epochs; e++) c += mcq_plan_cost_epoch(pl.first[e], pl.first[e + 1], pl.n_draws);
    return c;
}
constexpr bool mcq_plan_valid(const McqDealPlan &pl) {
    if (pl.n_epochs < 1 || pl.n_epochs > MCQ_PLAN_MAX_EPOCHS || pl.first[0] != 0 || pl.first[pl.n_epochs] != pl.n_draws) return false;
    for (int e = 0; e < pl.n_epochs; e++) {
        if (pl.size(e) < 1) return false;
        /* an epoch holds at most what its registers hold (the last draw of all needs no slot) */
        if (pl.size(e) - (e == pl.n_epochs - 1 ? 1 : 0) > 4 * (pl.reg0[e + 1] - pl.reg0[e])) return false;
    }
    return pl.reg0[pl.n_epochs] <= MCQ_PLAN_REGS; /* no more hole registers live than without plans */
}
// the plan of (N, RULE), worked out once per pair
template <int N, int RULE>
struct McqPlanOf {
    static constexpr McqDealPlan pl = mcq_deal_plan(N, RULE);
    static_assert(mcq_plan_valid(pl), "dealing plan");
};
static_assert(mcq_plan_cost(mcq_deal_plan(15, 1)) == 148 && mcq_deal_plan(15, 1).first[1] == 8, "6-max before the flop, {8}");
static_assert(mcq_plan_cost(mcq_deal_plan(15, 2)) == 145 && mcq_deal_plan(15, 2).first[2] == 12, "6-max before the flop, {8, 12}");
static_assert(mcq_plan_cost(mcq_deal_plan(15, 3)) == 143 && mcq_deal_plan(15, 3).first[3] == 13, "6-max before the flop, {8, 12, 13}");
static_assert(mcq_plan_cost(mcq_deal_plan(15, MCQ_DEAL_FULLREG)) == 146, "6-max before the flop, {4, 8, 12}");
static_assert(mcq_plan_cost(mcq_deal_plan(23, 3)) == 308 && mcq_plan_cost(mcq_deal_plan(12, 3)) == 98, "ten players; 5 opponents, 2 to come");

// Counting in pairs (mcq_hole_count2).  Wherever a level counts two or more registers they are taken two at a time, the
// epoch's registers 0 with 1, 2 with 3; the second of each pair lives BIASED (MCQ_HOLE_BIAS) from its pair draw or the scan behind it on
// (mcq_plan_biased_by_pair), an odd register left over is counted singly.  Which registers are biased follows from the plan alone: the holes its epoch ends
// with.  The plans themselves and mcq_plan_cost stay what they were (the checkpoints are chosen by the single counts);
// mcq_plan_cost_paired is the cost of the same plan with the paired primitive: 5 a pair for 6.
#ifndef MCQ_COUNT_PAIRED
#define MCQ_COUNT_PAIRED 1 /* measured on the 6-max preflop shape: DESIGN.md, section 7, r20 */
#endif
// holes epoch e ends with (the last draw of all leaves none)
constexpr int mcq_plan_holes(const McqDealPlan &pl, int e) { return pl.size(e) - (e == pl.n_epochs - 1 ? 1 : 0); }
// scans that move a free slot of an epoch's register i down before the slot is filled or the epoch closes with `holes`
// holes: the register is written whole by draw 4i + 1 of its epoch, as if scanned once, and scanned by every later draw
constexpr int mcq_plan_slot_scans(int holes, int i) {
    const int s = holes - 4 * i - 1;
    return s < 0 ? 0 : s > 3 ? 3 : s;
}
// whether register i of an epoch that ends with `holes` holes is the biased half of a pair: a plan that broke the bound on
// the free slots would count that register singly
constexpr bool mcq_plan_biased(int holes, int i) {
    return (i & 1) != 0 && i < mcq_plan_count_regs(holes) && mcq_plan_slot_scans(holes, i) <= MCQ_BIAS_MAX_SCANS;
}
constexpr int mcq_plan_pairs(int holes) {
    int c = 0;
    for (int i = 1; i < mcq_plan_count_regs(holes); i += 2) c += mcq_plan_biased(holes, i) ? 1 : 0;
    return c;
}
constexpr int mcq_plan_cost_closed_paired(int n) { return mcq_plan_cost_closed(n) - mcq_plan_pairs(n); }
constexpr int mcq_plan_cost_paired(const McqDealPlan &pl) {
    int c = 0;
    for (int e = 0; e < pl.n_epochs; e++) {
        const int a = pl.first[e], b = pl.first[e + 1], n = pl.n_draws;
        for (int d = a; d < b; d++) c += d == n - 1 ? mcq_plan_cost_closed_paired(d - a) : mcq_plan_cost_own(d - a, false);
        c += (n - b) * mcq_plan_cost_closed_paired(b - a);
    }
    return c;
}
static_assert(mcq_plan_cost_paired(mcq_deal_plan(15, 3)) == 136, "6-max before the flop: draws 8..14 pass one pair each");
static_assert(mcq_plan_cost_paired(mcq_deal_plan(23, 3)) == 286, "ten players, {8, 16, 20}: 15 + 7 passes over a full pair");
static_assert(mcq_plan_cost_paired(mcq_deal_plan(15, 1)) == 140 && mcq_plan_cost_paired(mcq_deal_plan(15, 2)) == 138,
              "6-max before the flop: {8}, whose last draw counts six holes of its own epoch in a pair, and {8, 12}");
static_assert(mcq_plan_biased(8, 1) && mcq_plan_biased(6, 1) && !mcq_plan_biased(5, 1) && !mcq_plan_biased(8, 0) &&
              mcq_plan_biased(16, 3) && !mcq_plan_biased(12, 2), "the second register of a pair, full or partly filled");

// the epoch's registers that a level counts, from register I on: in pairs where the plan has them, else one by one
template <int N, int RULE, int EE, int PAIRED, int I = 0>
MCQ_HD void mcq_epoch_count(uint32_t pb, const uint32_t (&E)[MCQ_PLAN_REGS], uint32_t &k) {
    constexpr int holes = mcq_plan_holes(McqPlanOf<N, RULE>::pl, EE), r0 = McqPlanOf<N, RULE>::pl.reg0[EE];
    if constexpr (I < mcq_plan_count_regs(holes)) {
        if constexpr (PAIRED != 0 && mcq_plan_biased(holes, I + 1)) {
            mcq_hole_count2(pb, E[r0 + I], E[r0 + I + 1], k);
            mcq_epoch_count<N, RULE, EE, PAIRED, I + 2>(pb, E, k);
        } else {
            mcq_hole_count(pb, E[r0 + I], k);
            mcq_epoch_count<N, RULE, EE, PAIRED, I + 1>(pb, E, k);
        }
    }
}
// A biased register's first write is its pair draw (draw 4i + 1 of the epoch, mcq_hole_pair) only where the epoch closes
// right behind it; else the pair is written plain and the scan of the next draw, 4i + 2, biases it (MCQ_SCAN_TO_BIASED).
constexpr bool mcq_plan_biased_by_pair(int holes, int i) { return mcq_plan_biased(holes, i) && holes == 4 * i + 2; }
constexpr int mcq_plan_scan_mode(int holes, int i, int j) { /* draw j of the epoch scans its register i */
    return !mcq_plan_biased(holes, i) ? MCQ_SCAN_PLAIN
           : (j == 4 * i + 2 && !mcq_plan_biased_by_pair(holes, i)) ? MCQ_SCAN_TO_BIASED : MCQ_SCAN_BIASED;
}
// the moving scan of draw J of the epoch over its registers I .. CNT - 1, each by the bit its indicator stands in
template <int N, int RULE, int EE, int PAIRED, int J, int CNT, int I = 0>
MCQ_HD void mcq_epoch_scan(uint32_t rb, uint32_t (&E)[MCQ_PLAN_REGS], uint32_t &k) {
    if constexpr (I < CNT) {
        constexpr int holes = mcq_plan_holes(McqPlanOf<N, RULE>::pl, EE), r0 = McqPlanOf<N, RULE>::pl.reg0[EE];
        mcq_hole_reg<(PAIRED != 0 ? mcq_plan_scan_mode(holes, I, J) : MCQ_SCAN_PLAIN)>(rb, E[r0 + I], k);
        mcq_epoch_scan<N, RULE, EE, PAIRED, J, CNT, I + 1>(rb, E, k);
    }
}

// Draw number D of the N an iteration deals by the plan (N, RULE).  E: the plan's hole registers, epoch by epoch.
// Returned: base position + 128, as mcq_draw_opp / mcq_draw_table return it.
template <int N, int RULE, int EE, int PAIRED = MCQ_COUNT_PAIRED> /* through the closed epochs EE, EE - 1, .., 0 */
MCQ_HD void mcq_epoch_pass(const uint32_t (&E)[MCQ_PLAN_REGS], uint32_t &k) {
    if constexpr (EE >= 0) {
        constexpr int n = McqPlanOf<N, RULE>::pl.size(EE), r0 = McqPlanOf<N, RULE>::pl.reg0[EE];
        const uint32_t p = k; /* position in the list at the epoch's closing checkpoint, still | 0x80 */
        if constexpr (mcq_plan_lone(n)) k += E[r0 + n / 4] <= p ? 1u : 0u;
        if constexpr (mcq_plan_count_regs(n) > 0) {
            const uint32_t pb = mcq_splat_byte(p);
            mcq_epoch_count<N, RULE, EE, PAIRED>(pb, E, k);
        }
        mcq_epoch_pass<N, RULE, EE - 1, PAIRED>(E, k);
    }
}
#if defined(__GNUC__) && !defined(__clang__)
/* (a host build with GCC folds the first draw of a plan into mcq_draw_opp<0>, whose code is the same, and then warns that
 * the array of the one is not the size of the other's) */
#define MCQ_NO_FOLD __attribute__((no_icf))
#else
#define MCQ_NO_FOLD
#endif
template <int N, int RULE, int D, int PAIRED = MCQ_COUNT_PAIRED>
MCQ_NO_FOLD MCQ_HD uint32_t mcq_draw_epoch(uint32_t rp, uint32_t (&E)[MCQ_PLAN_REGS]) {
    if constexpr (D >= N) {
        return rp; /* (the unrolled callers name draws their form never makes) */
    } else {
        constexpr int e = McqPlanOf<N, RULE>::pl.epoch_of(D), J = D - McqPlanOf<N, RULE>::pl.first[e],
                      R0 = McqPlanOf<N, RULE>::pl.reg0[e];
        constexpr int kHoles = mcq_plan_holes(McqPlanOf<N, RULE>::pl, e);
        constexpr bool kBiased = PAIRED != 0 && mcq_plan_biased(kHoles, J / 4); /* the register this draw's hole goes to */
        uint32_t k = rp;
        if constexpr (D == N - 1) { /* count only */
            if constexpr (mcq_plan_lone(J)) k += E[R0 + J / 4] <= rp ? 1u : 0u;
            if constexpr (mcq_plan_count_regs(J) > 0) {
                const uint32_t rb = mcq_splat_byte(rp);
                mcq_epoch_count<N, RULE, e, PAIRED>(rb, E, k); /* the J holes are all the last epoch ends with */
            }
        } else { /* mcq_draw_opp<J> on the epoch's registers */
            if constexpr (J % 4 == 1) mcq_hole_pair<(PAIRED != 0 && mcq_plan_biased_by_pair(kHoles, J / 4))>(rp, E[R0 + J / 4], k);
            if constexpr (J % 4 == 0) E[R0 + J / 4] = rp;
            if constexpr (J >= 2) {
                const uint32_t rb = mcq_splat_byte(rp);
                mcq_epoch_scan<N, RULE, e, PAIRED, J, (J % 4 < 2 ? J / 4 : J / 4 + 1)>(rb, E, k);
                if constexpr (J % 4 >= 2) mcq_hole_put<J, kBiased>(E[R0 + J / 4], rp);
            }
        }
        mcq_epoch_pass<N, RULE, e - 1, PAIRED>(E, k);
        return mcq_opaque(k);
    }
}

// The rule by which the straight forms of mcq_iteration_sum deal (0: without plans, mcq_draw_opp / mcq_draw_table).
#ifndef MCQ_DEAL_RULE
#define MCQ_DEAL_RULE 3 /* measured on the 6-max preflop shape against rules 1, 2 and MCQ_DEAL_FULLREG: DESIGN.md, section 7, r17 */
#endif
// the draws of a straight form's plan: where the table cards to come are counted at run time, the plan is that of five,
// and an iteration with fewer stops early in it
constexpr int mcq_plan_draws(int nopp, int ndeal) { return 2 * nopp + (ndeal >= 0 ? ndeal : 5); }

// Whether the straight forms read the opponents' cards by the flush suit (0: where they are dealt, all four suits).
#ifndef MCQ_HOLE_BY_SUIT
#define MCQ_HOLE_BY_SUIT 1 /* measured on the 6-max preflop shape: DESIGN.md, section 7, r19 */
#endif
#ifndef MCQ_L0_CONST
#define MCQ_L0_CONST 1
#endif
// opponent draw number D: by the plan's rule, or (RULE 0) as before there were plans
template <int N, int RULE, int D, int PAIRED = MCQ_COUNT_PAIRED>
MCQ_HD uint32_t mcq_draw_opp_by(uint32_t rp, uint32_t (&H)[5], uint32_t (&E)[MCQ_PLAN_REGS]) {
    if constexpr (RULE != 0) return mcq_draw_epoch<N, RULE, D, PAIRED>(rp, E);
    else return mcq_draw_opp<D>(rp, H);
}
// mcq_deal_table by a plan: the table's draws are the plan's draws D0, D0 + 1, ..
template <int N, int RULE, int D0, class Draws, int NDEAL = -1, class Deck = McqDeckAoS, int PAIRED = MCQ_COUNT_PAIRED>
MCQ_HD void mcq_deal_table_plan(const McqQueryCtx &qc, Draws &dr, const Deck &deck, uint32_t (&E)[MCQ_PLAN_REGS], uint32_t L,
                                McqSumBoard &b) {
    const uint32_t n_deal = NDEAL >= 0 ? (uint32_t)NDEAL : mcq_opaque_uniform(qc.n_deal);
    McqCard pend = {0u, 0u, 0u, 0u}; /* a card joins the table one draw late, see mcq_deal_table */
#define MCQ_TABLE(K)                                                                                                  \
    if (K < n_deal) {                                                                                                 \
        const uint32_t at = mcq_draw_epoch<N, RULE, D0 + K, PAIRED>(dr.template table<K>(L - Draws::kTableShort), E); /* l.188 */ \
        if (K > 0) b.add(pend);                                                                                       \
        pend = deck.card(at);                                                                                         \
        L -= 1;                                                                                                       \
    }
    MCQ_TABLE(0) MCQ_TABLE(1) MCQ_TABLE(2) MCQ_TABLE(3) MCQ_TABLE(4)
#undef MCQ_TABLE
    if (n_deal > 0u) b.add(pend);
}

// mcq_sum_first / mcq_sum_ids of a hand whose two cards were read by the flush suit (hole_by_suit): the rank sum is one
// three-input add, the flush mask one three-input or, and nothing of the other three suits was ever loaded.
MCQ_HD void mcq_sum_first_by_suit(const McqSumBoard &b, const McqFlushSel &fs, const McqPair &c1, const McqPair &c2,
                                  const McqSumTabs &t, uint32_t &s, uint32_t &d, uint32_t &flush_id) {
    s = b.sum + c1.a + c2.a;
    flush_id = mcq_ld_u32(t.tfid, fs.bfl4 | c1.b | c2.b);
    d = mcq_ld_u16(t.hoff, s & (MCQ_SUM_MASK << 1));
}
MCQ_HD void mcq_sum_ids_by_suit(const McqSumBoard &b, const McqFlushSel &fs, const McqPair &c1, const McqPair &c2,
                                const McqSumTabs &t, uint32_t &rank_id, uint32_t &flush_id) {
#ifdef MCQ_ABLATE_EVAL /* diagnostic timing build: wrong results */
    rank_id = ((b.sum ^ c1.a ^ c2.a ^ ((c1.b | c2.b) >> 3)) & 0xFFFu) | (1u << MCQ_ID_SHIFT);
    flush_id = 0u;
    return;
#endif
    uint32_t s, d;
    mcq_sum_first_by_suit(b, fs, c1, c2, t, s, d, flush_id);
    rank_id = mcq_sum_rank(t, s, d);
}

// The late join of an opponent pair (mcq_iteration_sum): where the second card's suit masks may be used from.  Device: an
// empty volatile asm on the two registers; a host build has no scheduler to hold.
MCQ_HD void mcq_join_hold(McqCard &c) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(c.los), "+v"(c.his));
#else
    (void)c;
#endif
}
// One Monte-Carlo iteration of one lane.  The opponents' hole cards stay in registers (statically indexed:
// everything below is unrolled over the opponent number) until the table is complete: the reference deals
// ALL opponents before any table card (montecarlo_python.py:215-217).
// NOPP / NDEAL >= 0: the number of opponents / of table cards to come is known at compile time (it must equal
// qc.n_opp / qc.n_deal): the iteration is ONE basic block, which lets the compiler send lookups early and wait late
// across hands and draws -- the wave-uniform branches of the general form are scheduling barriers.
// Acc = McqLaneAccWays: the split-pot form (see there); McqLaneAcc: the code is what it was before that form existed.
// The hands are in the sum form (McqSumBoard / McqSumHole, ids instead of keys); mcq_iteration / mcq_iterations keep the
// mask form's table arguments for the host builds of this file and find the sum-form tables behind them
// (mcq_sum_tabs_of), the kernels call the _sum forms with their LDS image.
// RULE: the straight forms (NOPP >= 1) deal by the plan of that rule (mcq_deal_plan), 0 and the general form as before
// there were plans (mcq_draw_opp, mcq_deal_table): same draws, same positions, fewer instructions.
// BYSUIT: the straight forms keep the POSITIONS of the opponents' cards while they deal and read the cards themselves behind
// the table, by the flush suit (hole_by_suit: one 8-byte read a card, one add and one or a hand); false and the general
// form: the cards are read where they are dealt, all four suits (hole_card), and joined as described below.
// PAIRED: the dealing by a plan counts a closed epoch's registers two per popcount (mcq_hole_count2); 0: one by one.
template <class Draws, int NOPP = -1, int NDEAL = -1, class Acc = McqLaneAcc, class Deck = McqDeckAoS,
          int RULE = (NOPP >= 1 ? MCQ_DEAL_RULE : 0), bool BYSUIT = (NOPP >= 1 && MCQ_HOLE_BY_SUIT != 0),
          int PAIRED = MCQ_COUNT_PAIRED>
// deck = the base deck table behind its accessor (McqDeckAoS / McqDeckSplit), its pointer biased by -128 entries: draw
// indices carry a bias of 128 (r | 0x80).
MCQ_HD void mcq_iteration_sum(const McqQueryCtx &qc, Draws &dr, const Deck &deck, const McqSumTabs &tabs, Acc &acc) {
    static_assert(RULE == 0 || NOPP >= 1, "a plan needs the number of opponents at compile time");
    static_assert(!BYSUIT || NOPP >= 1, "only the straight forms read the opponents' cards by suit");
    constexpr int kN = mcq_plan_draws(NOPP, NDEAL);
    uint32_t H[5] = {MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL};
    uint32_t E[MCQ_PLAN_REGS] = {MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL,
                                 MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL, MCQ_HOLE_SENTINEL};
    /* the deck's length is 50 - (5 - n_deal): a constant where the table cards to come are, and the pair decode's
     * `dd + 128` a literal of its select instead of a move from a scalar register */
    uint32_t L = MCQ_L0_CONST && NDEAL >= 0 ? (uint32_t)(45 + NDEAL) : qc.L0;
    McqSumHole opp[MCQ_MAX_OPP];
    const uint32_t n_opp_d = NOPP >= 0 ? (uint32_t)NOPP : mcq_opaque_uniform(qc.n_opp);
    /* BYSUIT (every straight form the kernels run): of an opponent's card only its POSITION is kept while the iteration deals
     * -- positions depend on the draws alone, the cards' contents are first used behind the table -- and the card is read
     * there, by the flush suit.  No card of an opponent is waited for during the dealing, so there is no join to hold back.
     * Without BYSUIT (host builds that name it: the form before there was a hole table): a pair joins its hand one pair late, as a table card joins the table one draw late (mcq_deal_table).
     * opp[P].set -- one add of the rank weights, two v_or of the suit masks -- is the first use of the pair's four LDS
     * reads, and where it follows them the wave waits there with lgkmcnt(0).  Held back behind the NEXT pair's reads (the
     * last pair's behind the table's draws) the wait becomes lgkmcnt(4) and the next pair's arithmetic covers it.  The
     * iteration is one basic block here and the compiler's scheduler ignores the order of the source for plain
     * arithmetic, so mcq_join_hold ties the second card's masks to the place in the source: an empty volatile asm, which
     * keeps its order among the volatile asms of the draws (mcq_opaque) before and behind it.  The general form keeps
     * the old order: its wave-uniform branches already separate the blocks -- and with it every caller of the general
     * form: the one-launch kernel (mcq_eval_direct_kernel, which has no straight dispatch), parity mode with split-pot
     * rows and parity mode with six or more opponents (mcq_iterations_replay4). */
    constexpr bool kLate = NOPP >= 1 && !BYSUIT; /* every such form, both accumulators, every draw policy: none needs a register more */
    McqCard j1 = {0u, 0u, 0u, 0u}, j2 = {0u, 0u, 0u, 0u}; /* the pair that has not joined yet */
    uint32_t at_h[2 * MCQ_MAX_OPP]; /* BYSUIT: where the opponents' cards lie (base position + 128) */
#define MCQ_OPP(P)                                                                                             \
    if (P < n_opp_d) {                                                                                         \
        uint32_t r1, r2;                                                                                       \
        dr.template pair<P>(L, r1, r2); /* r1 in [0,L-1], r2 in [0,L-2], r1 != r2 (l.167-176), both | 0x80 */  \
        if constexpr (BYSUIT) {                                                                                \
            at_h[2 * P] = mcq_draw_opp_by<kN, RULE, 2 * P, PAIRED>(r1, H, E);         /* deck.pop(r1) (l.178) */          \
            at_h[2 * P + 1] = mcq_draw_opp_by<kN, RULE, 2 * P + 1, PAIRED>(r2, H, E); /* deck.pop(r2), shrunk list (l.179) */ \
        } else {                                                                                               \
            const McqCard c1 = deck.hole_card(mcq_draw_opp_by<kN, RULE, 2 * P, PAIRED>(r1, H, E));     /* deck.pop(r1) */ \
            const McqCard c2 = deck.hole_card(mcq_draw_opp_by<kN, RULE, 2 * P + 1, PAIRED>(r2, H, E)); /* deck.pop(r2) */ \
            if constexpr (kLate) {                                                                             \
                if (P > 0) {                                                                                   \
                    mcq_join_hold(j2);                                                                         \
                    opp[P > 0 ? P - 1 : 0].set(j1, j2);                                                        \
                }                                                                                              \
                j1 = c1;                                                                                       \
                j2 = c2;                                                                                       \
            } else {                                                                                           \
                opp[P].set(c1, c2);                                                                            \
            }                                                                                                  \
        }                                                                                                      \
        L -= 2;                                                                                                \
    }
    MCQ_OPP(0) MCQ_OPP(1) MCQ_OPP(2) MCQ_OPP(3) MCQ_OPP(4) MCQ_OPP(5) MCQ_OPP(6) MCQ_OPP(7) MCQ_OPP(8)
#undef MCQ_OPP
    McqSumBoard b = qc.board_s;
    if (NDEAL == 5) b.clear(); /* all five to come: the known table is empty, nothing to add the cards to */
    if constexpr (RULE != 0) {
        mcq_deal_table_plan<kN, RULE, 2 * NOPP, Draws, NDEAL, Deck, PAIRED>(qc, dr, deck, E, L, b);
    } else if (NOPP >= 0) {
        mcq_deal_table<(NOPP >= 0 ? (2 * NOPP + 3) / 4 : 0), Draws, NDEAL>(qc, dr, deck, H, L, b);
    } else switch (mcq_opaque_uniform((2u * qc.n_opp + 3u) / 4u)) { /* registers holding the opponents' holes: wave-uniform */
        case 0: mcq_deal_table<0, Draws>(qc, dr, deck, H, L, b); break;
        case 1: mcq_deal_table<1, Draws>(qc, dr, deck, H, L, b); break;
        case 2: mcq_deal_table<2, Draws>(qc, dr, deck, H, L, b); break;
        case 3: mcq_deal_table<3, Draws>(qc, dr, deck, H, L, b); break;
        case 4: mcq_deal_table<4, Draws>(qc, dr, deck, H, L, b); break;
        default: mcq_deal_table<5, Draws>(qc, dr, deck, H, L, b); break;
    }
    if constexpr (kLate) { /* the last pair, behind the table's draws */
        mcq_join_hold(j2);
        opp[NOPP >= 1 ? NOPP - 1 : 0].set(j1, j2);
    }
    McqFlushSel fs;
    McqPair hc[2 * MCQ_MAX_OPP]; /* BYSUIT: the opponents' cards, read here: every read sent before hero's hand is looked up */
    if constexpr (BYSUIT) {
        const uint32_t key = deck.suit_key(fs.from_board_suit(b));
#pragma unroll
        for (int i = 0; i < 2 * NOPP; i++) hc[i] = deck.hole_by_suit(at_h[i], key);
    } else {
        fs.from_board(b);
    }
    const uint32_t hk = mcq_sum_key(b, fs, qc.hero_s, tabs);
    uint32_t best = 0;
    uint32_t n_equal = 0; /* (split-pot form only) opponents whose id equals hero's */
    const uint32_t n_opp_e = NOPP >= 0 ? (uint32_t)NOPP : mcq_opaque_uniform(qc.n_opp); /* a fresh scalar compare per block, see mcq_opaque_uniform */
#define MCQ_EVAL(P) /* the opponents' best id straight from the two lookups: one v_max3_u32 per hand */ \
    if (P < n_opp_e) {                                                     \
        uint32_t rid, fid;                                                 \
        if constexpr (BYSUIT) mcq_sum_ids_by_suit(b, fs, hc[2 * P], hc[2 * P + 1], tabs, rid, fid); \
        else mcq_sum_ids(b, fs, opp[P], tabs, rid, fid);                   \
        if (Acc::kWays) { /* the hand's own id: max, compare, add with carry, max */ \
            const uint32_t k = rid > fid ? rid : fid;                      \
            n_equal += k == hk ? 1u : 0u;                                  \
            best = k > best ? k : best;                                    \
        } else {                                                           \
            best = mcq_max3(best, rid, fid);                               \
        }                                                                  \
    }
#ifndef MCQ_ABLATE_EVAL
    if constexpr (NOPP >= 1 && !Acc::kWays) {
        /* Straight form: the hands' lookups in sweeps -- every hand's first reads, then every second-level read, then the
         * maxima -- so that the order of the source already overlaps the hands' dependent read pairs.  (The compiler
         * leaves the 6-max preflop block in the order of the source since its table starts empty, as the disassembly
         * shows; hand by hand, that order waits for every read where it is sent: 3.67 ms against 3.53 in sweeps.) */
        uint32_t s[MCQ_MAX_OPP], d[MCQ_MAX_OPP], fid[MCQ_MAX_OPP], rid[MCQ_MAX_OPP];
#pragma unroll
        for (int P = 0; P < NOPP; P++) {
            if constexpr (BYSUIT) mcq_sum_first_by_suit(b, fs, hc[2 * P], hc[2 * P + 1], tabs, s[P], d[P], fid[P]);
            else mcq_sum_first(b, fs, opp[P], tabs, s[P], d[P], fid[P]);
        }
#pragma unroll
        for (int P = 0; P < NOPP; P++) rid[P] = mcq_sum_rank(tabs, s[P], d[P]);
#pragma unroll
        for (int P = 0; P < NOPP; P++) best = mcq_max3(best, rid[P], fid[P]);
    } else
#endif
    {
        MCQ_EVAL(0) MCQ_EVAL(1) MCQ_EVAL(2) MCQ_EVAL(3) MCQ_EVAL(4) MCQ_EVAL(5) MCQ_EVAL(6) MCQ_EVAL(7) MCQ_EVAL(8)
    }
#undef MCQ_EVAL
    uint64_t won = hk >= best ? 1u : 0u; /* ties go to hero (hand_evaluator.py:23) */
    acc.types += won << (6u * (hk >> MCQ_ID_SHIFT));
    if constexpr (Acc::kWays) acc.ways += won << (6u * n_equal); /* pot shared by 1 + n_equal hands */
    else acc.tie += hk == best ? 1u : 0u;
}
template <class Draws, int NOPP = -1, int NDEAL = -1, class Acc = McqLaneAcc>
MCQ_HD void mcq_iteration(const McqQueryCtx &qc, Draws &dr, const McqCard *base128, const uint32_t *tf,
                          const uint32_t *, const uint32_t *, Acc &acc) {
    const McqDeckAoS deck = {base128};
    mcq_iteration_sum<Draws, NOPP, NDEAL, Acc>(qc, dr, deck, mcq_sum_tabs_of(tf), acc);
}

// `cnt` iterations of one lane.  STRAIGHT: by the (wave-uniform) number of opponents, and before the flop also by the
// number of table cards, the loop body is a specialisation of mcq_iteration without branches -- one basic block, in
// which the compiler sends lookups early and waits late across hands and draws (6-max before the flop: 6.37 -> 6.00 ms;
// the general form's wave-uniform branches are scheduling barriers).  Same arithmetic, same results.
template <bool STRAIGHT, class Draws, class Acc, class Deck>
MCQ_HD void mcq_iterations_sum(const McqQueryCtx &qc, Draws &dr, const Deck &deck, const McqSumTabs &tabs, Acc &acc,
                               uint32_t cnt) {
    if (STRAIGHT) {
#define MCQ_STRAIGHT(N)                                                                                   \
    case N:                                                                                               \
        if (qc.n_deal == 5u)                                                                          \
            for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, N, 5, Acc>(qc, dr, deck, tabs, acc); \
        else if (qc.n_deal == 2u)                                                                         \
            for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, N, 2, Acc>(qc, dr, deck, tabs, acc); \
        else if (qc.n_deal == 1u)                                                                         \
            for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, N, 1, Acc>(qc, dr, deck, tabs, acc); \
        else                                                                                              \
            for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, N, -1, Acc>(qc, dr, deck, tabs, acc); \
        return;
        switch (qc.n_opp) {
            MCQ_STRAIGHT(1) MCQ_STRAIGHT(2) MCQ_STRAIGHT(3) MCQ_STRAIGHT(4) MCQ_STRAIGHT(5) MCQ_STRAIGHT(6) MCQ_STRAIGHT(7)
            case 8: /* (only the form with the table cards counted at run time: the others spill registers) */
                for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, 8, -1, Acc>(qc, dr, deck, tabs, acc);
                return;
            case 9:
                for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, 9, -1, Acc>(qc, dr, deck, tabs, acc);
                return;
            default: break; /* hero alone: the general form */
        }
#undef MCQ_STRAIGHT
    }
    for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, -1, -1, Acc>(qc, dr, deck, tabs, acc);
}
template <bool STRAIGHT, class Draws, class Acc>
MCQ_HD void mcq_iterations(const McqQueryCtx &qc, Draws &dr, const McqCard *base128, const uint32_t *tf, const uint32_t *,
                           const uint32_t *, Acc &acc, uint32_t cnt) {
    const McqDeckAoS deck = {base128};
    mcq_iterations_sum<STRAIGHT>(qc, dr, deck, mcq_sum_tabs_of(tf), acc, cnt);
}

// Parity mode: the (up to four) iterations a lane takes from one McqReplayDraws4 load.  As in mcq_iterations_sum the loop
// body is picked by the (wave-uniform) number of opponents, so that the opponents' deals and hands are straight code
// without the general form's scalar compare and branch per opponent; the table cards to come stay counted at run time.
// Same arithmetic, same results.
template <class Acc, class Deck>
MCQ_HD void mcq_iterations_replay4(const McqQueryCtx &qc, McqReplayDraws4 &dr, const Deck &deck, const McqSumTabs &tabs,
                                   Acc &acc, uint32_t cnt4) {
#define MCQ_REPLAY4(N)                                                                      \
    case N:                                                                                 \
        for (uint32_t k = 0; k < cnt4; k++) {                                               \
            dr.sh = 8u * k;                                                                 \
            mcq_iteration_sum<McqReplayDraws4, N, -1, Acc>(qc, dr, deck, tabs, acc);        \
        }                                                                                   \
        return;
    /* (not the split-pot form: it sits at the register limit and the straight forms spill there, 24-40 bytes per lane) */
    if constexpr (!Acc::kWays) switch (qc.n_opp) {
        MCQ_REPLAY4(1) MCQ_REPLAY4(2) MCQ_REPLAY4(3) MCQ_REPLAY4(4) MCQ_REPLAY4(5)
        default: break; /* hero alone, and seven to ten players (the straight forms of six and more opponents spill registers
                           beside the 23 draw words of McqReplayDraws4): the general form */
    }
#undef MCQ_REPLAY4
    for (uint32_t k = 0; k < cnt4; k++) {
        dr.sh = 8u * k;
        mcq_iteration_sum<McqReplayDraws4, -1, -1, Acc>(qc, dr, deck, tabs, acc);
    }
}

// ================================================================================================ extended queries
// SURVEY 8f-2, all of run_montecarlo's arguments: opponent ranges (montecarlo_python.py:165-181 with :36-112), ghost
// cards (:206-208), any number of known hands in the order of original_player_card_list, each two cards or a SET of
// preflop classes (:133-163).  The deck of an iteration is a 52-bit mask per lane (card-id order = the reference's
// list order); cards come from a 52-entry table, the dealt hands' card ids wait in LDS.
//
// A range is a 169-bit set; the bit of two cards is how get_two_short_notation (:24-34) names them:
// suited -> 13*min+max, off-suit -> 13*max+min, pair -> 14*rank.
//
// Production mode ("MCQ-CTR v5x") deals the reference's LAW without its index arithmetic and without its re-draw
// loop over all L(L-1) index pairs.  The reference accepts, equally often, every ordered index pair (r1, r2),
// r1 in [0,L), r2 in [0,L-1), r1 != r2, whose classes are allowed (:167-176); as cards: every ordered pair (A, B) of
// distinct cards of the current deck with B not the deck's highest card.  Per range there is a fixed CANDIDATE LIST
//     P' = [(a, b) for a in 0..51 for b in 0..51 if a != b and a, b in U and class(a, b) allowed]
// over U = the cards that can still be in the deck at that point whatever was drawn before (52 minus ghost, table and
// the LIST hands dealt earlier; all list hands for the opponents), laid out once per query by mcq_ext_lists_kernel.
// A trial: one word u, (A, B) = P'[mulhi32(u, |P'|)], accepted iff A and B are still in the deck and B is not its
// highest card -- uniform on exactly the reference's accepted set.  A known hand leaves by value (:146-161); an
// opponent is dealt A and, as deck.pop(r1); deck.pop(r2) deal (:178-179), B if B lies below A, else the card that
// FOLLOWS B in the deck (the reference's quirk: the range test looks at the unpopped list).  With the top quarter of
// the classes a trial of the reference's loop succeeds one time in ~25, a trial here three times in four.
// Opponents to whom every class is allowed are dealt by index exactly as the plain path deals them (MCQ-CTR v5, one
// word per pair), so an extension record that restricts nothing gives the plain path's tallies bit for bit.
#define MCQ_EXT_WORDS 76u         /* sizeof(mcq_query_ext) / 4 */
#define MCQ_EXT_MAX_LISTS 11u     /* ten known hands as ranges + the opponents */
#define MCQ_EXT_LIST_STRIDE 2704u /* entries reserved per candidate list (52 * 52 >= 52 * 51) */
#define MCQ_EXT_MAX_TRIALS 65536u /* bound of a re-draw loop: a range that cannot be dealt must not hang */

struct McqExtRec { /* the 304-byte mcq_query_ext record as words (any address space) */
    const uint32_t *w;
    MCQ_HDM uint32_t ghost(uint32_t i) const { return (w[0] >> (8u * i)) & 0xFFu; } /* 0xFF = none */
    MCQ_HDM uint32_t hero_is_range() const { return (w[0] >> 16) & 0xFFu; }
    MCQ_HDM uint32_t n_known() const { return w[0] >> 24; }
    MCQ_HDM uint32_t known_head(uint32_t k) const { return w[13u + 7u * k]; } /* cards[2], is_range, reserved */
    /* word offsets of the 6-word sets */
    MCQ_HDM uint32_t opp_set() const { return 1u; }
    MCQ_HDM uint32_t hero_set() const { return 7u; }
    MCQ_HDM uint32_t known_set(uint32_t k) const { return 14u + 7u * k; }
};

MCQ_HD uint32_t mcq_class_index(uint32_t a, uint32_t b) {
    const uint32_t ra = a >> 2, rb = b >> 2, lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
    if (ra == rb) return 14u * ra;
    return (a & 3u) == (b & 3u) ? 13u * lo + hi : 13u * hi + lo;
}
MCQ_HD bool mcq_in_range(const uint32_t *bits, uint32_t a, uint32_t b) {
    const uint32_t i = mcq_class_index(a, b);
    return (bits[i >> 5] >> (i & 31u)) & 1u;
}

/* hand h of the query (0 = hero, 1.. = known[h - 1]): cards a | b << 8 | is_range << 16 */
MCQ_HD uint32_t mcq_ext_hand(const McqQueryWords &q, const McqExtRec &e, uint32_t h) {
    if (h == 0) return e.hero_is_range() ? 0x10000u : (q.card(0) | (q.card(1) << 8));
    const uint32_t hd = e.known_head(h - 1u);
    return (hd >> 16) & 0xFFu ? 0x10000u : (hd & 0xFFFFu);
}
MCQ_HD uint32_t mcq_ext_hand_set(const McqExtRec &e, uint32_t h) { return h == 0 ? e.hero_set() : e.known_set(h - 1u); }

/* opponents unrestricted (every one of the 169 classes allowed)? */
MCQ_HD bool mcq_ext_opp_all(const McqExtRec &e) {
    uint32_t all = e.w[e.opp_set() + 5u] | ~0x1FFu;
    for (uint32_t i = 0; i < 5; i++) all &= e.w[e.opp_set() + i];
    return all == 0xFFFFFFFFu;
}

/* candidate lists of a query: one per known hand given as a range, in hand order, then one for the opponents
 * unless every class is allowed to them (they are then dealt by index, exactly as the plain path deals) */
MCQ_HD uint32_t mcq_ext_n_lists(const McqQueryWords &q, const McqExtRec &e) {
    uint32_t n = q.n_players() > 1u + e.n_known() && !mcq_ext_opp_all(e) ? 1u : 0u;
    for (uint32_t h = 0; h <= e.n_known(); h++) n += mcq_ext_hand(q, e, h) >> 16;
    return n;
}

/* Streams of the production mode (MCQ-CTR v5x): a query that draws from candidate lists and has at most
 * MCQ_EXT_SHORT_RUNS iterations cuts them into streams of MCQ_EXT_SHORT_STREAM iterations instead of MCQ_STREAM_ITERS --
 * a trial loop consumes a number of words nobody knows beforehand, so a stream cannot be entered half way as the plain
 * path's can, and a 1000-run query would otherwise be 63 lanes of ONE wave, sixteen iterations each, one behind the
 * other (34 us); so it is 500 lanes of eight waves, two iterations each.  Long queries keep the long streams (one
 * Philox block per sixteen iterations), and so does a query without lists: it deals exactly as the plain path. */
#define MCQ_EXT_SHORT_STREAM 2u
#define MCQ_EXT_SHORT_RUNS 8192u
MCQ_HD uint32_t mcq_ext_stream_iters(const McqQueryWords &q, const McqExtRec &e) {
    return q.runs() <= MCQ_EXT_SHORT_RUNS && mcq_ext_n_lists(q, e) != 0u ? MCQ_EXT_SHORT_STREAM : MCQ_STREAM_ITERS;
}
/* wave tasks (64 streams) of a query whose streams hold s_iters iterations, and what one costs (the unit of the cost
 * axis the kernels cut: three per weight and two iterations of a stream) */
MCQ_HD uint32_t mcq_ext_task_count(const McqQueryWords &q, uint32_t s_iters) {
    const uint32_t per = s_iters * MCQ_WAVE;
    return q.runs() / per + (q.runs() % per != 0u ? 1u : 0u);
}
MCQ_HD uint32_t mcq_ext_task_weight(const McqQueryWords &q, uint32_t s_iters) { return 3u * mcq_task_weight(q) * (s_iters >> 1); }

MCQ_HD uint64_t mcq_ext_base_deck(const McqQueryWords &q, const McqExtRec &e) { /* 52 cards minus ghost and table */
    uint64_t deck = (1ull << 52) - 1;
    for (uint32_t i = 0; i < q.n_board(); i++) deck &= ~(1ull << q.card(2u + i));
    if (e.ghost(0) != 0xFFu) deck &= ~((1ull << e.ghost(0)) | (1ull << e.ghost(1)));
    return deck;
}

/* list `li` of the query: the cards U its candidates are made of and the word offset of its class set */
MCQ_HD void mcq_ext_list_plan(const McqQueryWords &q, const McqExtRec &e, uint32_t li, uint64_t &U, uint32_t &set_off) {
    U = mcq_ext_base_deck(q, e);
    set_off = e.opp_set();
    uint32_t seen = 0;
    for (uint32_t h = 0; h <= e.n_known(); h++) {
        const uint32_t hd = mcq_ext_hand(q, e, h);
        if (hd >> 16) {
            if (seen == li) { set_off = mcq_ext_hand_set(e, h); return; }
            seen++;
        } else {
            U &= ~((1ull << (hd & 0xFFu)) | (1ull << ((hd >> 8) & 0xFFu)));
        }
    }
}

/* is candidate c = 52 * a + b on a list? */
MCQ_HD bool mcq_ext_candidate(uint64_t U, const uint32_t *set, uint32_t c) {
    const uint32_t a = c / 52u, b = c - 52u * a;
    return c < 2704u && a != b && ((U >> a) & 1u) && ((U >> b) & 1u) && mcq_in_range(set, a, b);
}

// every card named twice is an error; a range that is used must not be empty
MCQ_HD bool mcq_query_ext_valid(const McqQueryWords &q, const McqExtRec &e) {
    if (q.n_board() > 5 || q.n_players() < 1 || q.n_players() > 10 || q.reserved() != 0) return false;
    if (e.hero_is_range() > 1 || e.n_known() > MCQ_MAX_KNOWN || q.n_players() < 1u + e.n_known()) return false;
    uint64_t seen = 0;
    bool ok = true;
    for (uint32_t i = 0; i < q.n_board(); i++) {
        const uint32_t c = q.card(2u + i);
        ok = ok && c < 52 && !((seen >> (c & 63u)) & 1);
        seen |= 1ull << (c & 63u);
    }
    if (e.ghost(0) != 0xFFu || e.ghost(1) != 0xFFu)
        for (uint32_t i = 0; i < 2; i++) {
            const uint32_t c = e.ghost(i);
            ok = ok && c < 52 && !((seen >> (c & 63u)) & 1);
            seen |= 1ull << (c & 63u);
        }
    for (uint32_t h = 0; h <= e.n_known(); h++) {
        if (h > 0) {
            const uint32_t hd = e.known_head(h - 1u);
            if (((hd >> 16) & 0xFFu) > 1u || (hd >> 24) != 0u) return false;
        }
        const uint32_t hd = mcq_ext_hand(q, e, h);
        if (hd >> 16) {
            const uint32_t off = mcq_ext_hand_set(e, h);
            uint32_t any = 0;
            for (uint32_t i = 0; i < 6; i++) any |= e.w[off + i];
            ok = ok && any != 0;
        } else {
            for (uint32_t i = 0; i < 2; i++) {
                const uint32_t c = (hd >> (8u * i)) & 0xFFu;
                ok = ok && c < 52 && !((seen >> (c & 63u)) & 1);
                seen |= 1ull << (c & 63u);
            }
        }
    }
    if (q.n_players() > 1u + e.n_known()) {
        uint32_t any = 0;
        for (uint32_t i = 0; i < 6; i++) any |= e.w[e.opp_set() + i];
        ok = ok && any != 0;
    }
    return ok;
}

struct McqExtCtx { /* wave-uniform */
    uint32_t deck_lo, deck_hi;            /* 52 cards minus ghost and table */
    uint32_t n_players, n_hands, n_deal, runs; /* n_hands = 1 + n_known */
    bool opp_all;                         /* every class allowed to the opponents: dealt by index as in the plain path */
    McqBoard board;
    /* the common ranged query -- hero two cards, no further known hand, every opponent drawn from ONE candidate list --
     * takes mcq_iteration_ext_fast: */
    bool fast;
    uint32_t fdeck_lo, fdeck_hi;          /* the deck without hero's cards too */
    McqHole hero;
};
struct McqExtWaveCtx { /* per wave, in LDS: what the iteration indexes at run time */
    uint32_t hand[10];                  /* mcq_ext_hand of every known hand */
    uint32_t cnt[MCQ_EXT_MAX_LISTS];    /* sizes of the candidate lists */
    uint32_t pad_[3];
    const uint16_t *list[MCQ_EXT_MAX_LISTS]; /* where each list lies: HBM, or the block's LDS when its queries' lists fit */
};

MCQ_HD void mcq_ext_ctx(const McqQueryWords &q, const McqExtRec &e, McqExtCtx &c) {
    const uint64_t deck = mcq_ext_base_deck(q, e);
    c.board.clear();
    for (uint32_t i = 0; i < q.n_board(); i++) c.board.add(mcq_card(q.card(2u + i)));
    c.deck_lo = (uint32_t)deck;
    c.deck_hi = (uint32_t)(deck >> 32);
    c.n_players = q.n_players();
    c.n_hands = 1u + e.n_known();
    c.n_deal = 5u - q.n_board();
    c.runs = q.runs();
    c.opp_all = mcq_ext_opp_all(e);
    c.fast = !e.hero_is_range() && e.n_known() == 0u && !c.opp_all && q.n_players() >= 2u;
    const uint32_t h0 = q.card(0), h1 = q.card(1);
    const uint64_t fdeck = deck & ~(((uint64_t)1 << (h0 & 63u)) | ((uint64_t)1 << (h1 & 63u)));
    c.fdeck_lo = (uint32_t)fdeck;
    c.fdeck_hi = (uint32_t)(fdeck >> 32);
    c.hero.set(mcq_card(h0 < 52u ? h0 : 0u), mcq_card(h1 < 52u ? h1 : 0u));
}

/* deck mask helpers (52 bits in two words) */
MCQ_HD bool mcq_deck_has(uint32_t lo, uint32_t hi, uint32_t c) { return (((c & 32u) ? hi : lo) >> (c & 31u)) & 1u; }
MCQ_HD void mcq_deck_take(uint32_t &lo, uint32_t &hi, uint32_t c) {
    const uint32_t bit = 1u << (c & 31u);
    lo &= (c & 32u) ? 0xFFFFFFFFu : ~bit;
    hi &= (c & 32u) ? ~bit : 0xFFFFFFFFu;
}
MCQ_HD uint32_t mcq_deck_top(uint32_t lo, uint32_t hi) { /* highest card, deck not empty */
    return hi ? 63u - mcq_clz(hi) : 31u - mcq_clz(lo | 1u);
}
MCQ_HD uint32_t mcq_deck_next(uint32_t lo, uint32_t hi, uint32_t c) { /* the card that follows c; c is not the top */
    const uint64_t above = ((((uint64_t)hi << 32) | lo) >> c) >> 1; /* cards above c, bit 0 = c + 1 */
    const uint32_t alo = (uint32_t)above, ahi = (uint32_t)(above >> 32);
    const uint32_t low = alo ? alo & (0u - alo) : ahi & (0u - ahi);
    return c + 1u + (alo ? 31u - mcq_clz(low | 1u) : 63u - mcq_clz(low | 1u));
}

// Draw policies (the extended path is not unrolled).
struct McqExtCtrDraws {
    static constexpr bool kReplay = false;
    McqStreamRng rng;
    uint32_t w;
    MCQ_HDM void start(uint64_t seed, uint64_t qid, uint32_t stream) {
        w = 0;
        rng.seed(seed, qid, stream);
    }
    MCQ_HDM uint32_t pick(uint32_t n) { return mcq_mulhi(rng.next(), n); } /* a candidate of a list of n */
    MCQ_HDM void pair(uint32_t &, uint32_t &) {}
    MCQ_HDM void index_pair(uint32_t L, uint32_t &r1, uint32_t &r2) { /* MCQ-CTR v5 as the plain path: McqCtrDrawsT::pair */
        const uint32_t dd = L - 1u;
        const uint32_t u = rng.next();
        uint32_t frac;
        const uint32_t a = mcq_mulhilo_p128(u, dd, 0ull, frac);
        const uint32_t c = mcq_mulhi(frac, dd);
        r1 = a == c ? dd : a;
        r2 = c;
    }
    MCQ_HDM uint32_t table(uint32_t k, uint32_t n) {
        if ((k & 1u) == 0) {
            const uint32_t u = rng.next();
            return mcq_mulhilo_p128(u, n, 0ull, w);
        }
        return mcq_mulhi(w, n);
    }
};
struct McqExtReplayDraws { /* accepted draws from the host, all in list.pop order */
    static constexpr bool kReplay = true;
    const uint8_t *p;
    uint64_t stride;
    MCQ_HDM uint32_t pick(uint32_t) { return 0; }
    MCQ_HDM void index_pair(uint32_t, uint32_t &, uint32_t &) {}
    MCQ_HDM void pair(uint32_t &r1, uint32_t &r2) {
        r1 = p[0] & 0x7Fu; /* the host stores every draw as r | 0x80 */
        r2 = p[stride] & 0x7Fu;
        p += 2 * stride;
    }
    MCQ_HDM uint32_t table(uint32_t, uint32_t) {
        uint32_t v = p[0] & 0x7Fu;
        p += stride;
        return v;
    }
};

// One iteration of an extended query.  ids: this lane's slot array (stride `ids_stride` words) for the dealt
// hands; cards: the 52-entry card table; wc.list: the query's candidate lists,
// wc: the known hands and the list sizes.  Returns false when a range could not be dealt within
// MCQ_EXT_MAX_TRIALS attempts.
// Acc = McqLaneAccWays: the split-pot form, as in mcq_iteration -- the iterations hero does not lose are split by how many
// OTHER hands (known, ranged or random alike, each by its key) equal hero's.  A stream of the extended path holds
// sixteen or two iterations (mcq_ext_stream_iters), and a lane runs one stream per task: a 6-bit field never overflows.
#if !defined(__HIP_DEVICE_COMPILE__) && defined(MCQ_EXT_DEAL_HOOK)
#define MCQ_EXT_DEALT(h, c1, c2) MCQ_EXT_DEAL_HOOK(h, c1, c2) /* host test builds only: the hands of the iteration */
#else
#define MCQ_EXT_DEALT(h, c1, c2) ((void)0)
#endif
template <class Draws, bool LDS_LIST = false /* the candidate lists lie in LDS: see mcq_iteration_ext_fast */, class Acc = McqLaneAcc>
MCQ_HD bool mcq_iteration_ext(const McqExtCtx &qc, const McqExtWaveCtx &wc, Draws &dr, const McqCard *cards,
                              const uint32_t *sel8, uint16_t *ids, uint32_t ids_stride,
                              const uint32_t *tf, const uint32_t *tops, const uint32_t *sd, Acc &acc) {
    static_assert(MCQ_STREAM_ITERS < 64u && MCQ_EXT_SHORT_STREAM < 64u, "6-bit fields of the lane accumulator");
    uint32_t dlo = qc.deck_lo, dhi = qc.deck_hi;
    bool dealt = true;
    uint32_t li = 0; /* candidate list of the next known hand given as a range; the opponents' comes after them */
    for (uint32_t h = 0; h < qc.n_players; h++) {
        const bool known = h < qc.n_hands;
        const uint32_t hd = known ? wc.hand[h] : 0x10000u;
        uint32_t c1, c2;
        if (!(hd >> 16)) { /* two cards: they leave by value, if they are still there (l.150-161) */
            c1 = hd & 0xFFu;
            c2 = (hd >> 8) & 0xFFu;
        } else if (Draws::kReplay) {
            uint32_t r1, r2;
            dr.pair(r1, r2);
            c1 = mcq_select_pop(dlo, dhi, r1, sel8);
            c2 = mcq_select_pop(dlo, dhi, r2, sel8);
        } else if (!known && qc.opp_all) { /* no range to respect: one word, never re-drawn, popped in turn (l.178-179) */
            uint32_t r1, r2;
            acc.passes++;
            dr.index_pair(mcq_popc(dlo) + mcq_popc(dhi), r1, r2);
            c1 = mcq_select_pop(dlo, dhi, r1, sel8);
            c2 = mcq_select_pop(dlo, dhi, r2, sel8);
        } else {
            const uint32_t n = wc.cnt[li];
            const uint16_t *list = wc.list[li];
#if defined(__HIP_DEVICE_COMPILE__)
            typedef __attribute__((address_space(3))) const uint16_t *LdsList;
            const LdsList list_l = (LdsList)(uintptr_t)list;
#define MCQ_XLIST(i) (LDS_LIST ? (uint32_t)list_l[i] : (uint32_t)list[i])
#else
#define MCQ_XLIST(i) ((uint32_t)list[i])
#endif
            const uint32_t top = mcq_deck_top(dlo, dhi);
            bool ok = false;
            c1 = c2 = 0;
            uint32_t trial = 0;
            for (; trial < MCQ_EXT_MAX_TRIALS && !ok; trial++) {
                const uint32_t e = MCQ_XLIST(dr.pick(n));
                c1 = e & 0xFFu;
                c2 = e >> 8;
                ok = mcq_deck_has(dlo, dhi, c1) && mcq_deck_has(dlo, dhi, c2) && c2 != top;
            }
#undef MCQ_XLIST
            acc.passes += trial;
            dealt = dealt && ok;
            if (!known && ok && c2 > c1) c2 = mcq_deck_next(dlo, dhi, c2); /* deck.pop(r2) after deck.pop(r1), l.178-179 */
        }
        if (known && (hd >> 16)) li++;
        mcq_deck_take(dlo, dhi, c1 < 52u ? c1 : 0u);
        mcq_deck_take(dlo, dhi, c2 < 52u ? c2 : 0u);
        ids[h * ids_stride] = (uint16_t)(c1 | (c2 << 8));
    }
    McqBoard b = qc.board;
    for (uint32_t k = 0; k < qc.n_deal; k++) {
        const uint32_t L = mcq_popc(dlo) + mcq_popc(dhi);
        const uint32_t c = mcq_select_pop(dlo, dhi, dr.table(k, L - 1u), sel8);
        MCQ_EXT_DEALT(0x100u + k, c, 0u);
        b.add(cards[c < 52u ? c : 0u]);
    }
    McqFlushSel fs;
    fs.from_board(b);
    uint32_t hk = 0, best = 0;
    uint32_t n_equal = 0; /* (split-pot form only) other hands whose key equals hero's */
    if constexpr (Acc::kSeats) { /* the best of ALL hands and the seats that hold it; no key is kept */
        uint32_t level = 0;
        for (uint32_t h = 0; h < qc.n_players; h++) {
            const uint32_t v = ids[h * ids_stride];
            MCQ_EXT_DEALT(h, v & 0xFFu, (v >> 8) & 0xFFu);
            McqHole hh;
            hh.set(cards[v & 0xFFu], cards[(v >> 8) & 0xFFu]);
            const uint32_t k = mcq_eval_key(b, fs, hh, tf, tops, sd);
            level = k > best ? 0u : level;
            level |= k >= best ? 1u << h : 0u;
            best = k > best ? k : best;
        }
        const uint32_t inc = mcq_seat_increment(mcq_popc(level)); /* (hero is always dealt: at least one seat) */
#pragma unroll
        for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) acc.seat[s] += ((level >> s) & 1u) ? inc : 0u;
        return dealt;
    }
    for (uint32_t h = 0; h < qc.n_players; h++) {
        const uint32_t v = ids[h * ids_stride];
        MCQ_EXT_DEALT(h, v & 0xFFu, (v >> 8) & 0xFFu);
        McqHole hh;
        hh.set(cards[v & 0xFFu], cards[(v >> 8) & 0xFFu]);
        const uint32_t k = mcq_eval_key(b, fs, hh, tf, tops, sd);
        if (h == 0) hk = k;
        else {
            best = k > best ? k : best;
            if (Acc::kWays) n_equal += k == hk ? 1u : 0u; /* (hero comes first: hk is known) */
        }
    }
    if constexpr (!Acc::kSeats) {
        uint64_t won = hk >= best ? 1u : 0u;
        acc.types += won << (6u * (hk >> MCQ_KEY_SHIFT));
        if constexpr (Acc::kWays) acc.ways += won << (6u * n_equal); /* pot shared by 1 + n_equal hands */
        else acc.tie += hk == best ? 1u : 0u;
    }
    return dealt;
}

// The common ranged query in straight code: hero two cards, no further known hand, all n_players - 1 opponents drawn
// from ONE candidate list (wc.list[0]).  The same draws in the same order as mcq_iteration_ext -- one word per trial,
// then the table cards two per word -- hence the same tallies bit for bit; what it saves is the general form's
// bookkeeping: the deck is one 64-bit mask tested with two shifts per trial, the opponents' hands stay in registers
// (unrolled over the opponent number, as in mcq_iteration) instead of travelling through LDS as card ids, the deck's
// length is known without counting (every lane deals two cards per opponent), hero's hand is part of the query context.
// 6-max at the top quarter of the classes: ~1650 -> ~900 VALU instructions per wave-iteration.
// (PIN: keep the opponent count in a scalar register of its own, see mcq_opaque_uniform; the one-launch kernel, whose
// query context comes out of LDS, cannot: the backend refuses the copy.)
// (LDS_LIST: the caller knows the candidate list lies in LDS -- staged by the block -- so a trial reads it with a
// 32-bit LDS address instead of through a generic pointer: a flat load waits for both memory counters and takes
// several times as long, in a loop where every trial is one dependent chain word -> index -> entry -> test.)
// (Acc: as mcq_iteration_ext -- the split-pot form counts the equal keys where the maximum is taken.)
template <class Draws, bool PIN = true, bool LDS_LIST = false, class Acc = McqLaneAcc>
MCQ_HD bool mcq_iteration_ext_fast(const McqExtCtx &qc, const McqExtWaveCtx &wc, Draws &dr, const McqCard *cards,
                                   const uint32_t *sel8, const uint32_t *tf, const uint32_t *tops, const uint32_t *sd,
                                   Acc &acc) {
    uint64_t deck = ((uint64_t)qc.fdeck_hi << 32) | qc.fdeck_lo;
    const uint32_t n = wc.cnt[0];
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) const uint16_t *LdsList;
    const uint16_t *list_g = wc.list[0];
    const LdsList list_l = (LdsList)(uintptr_t)list_g; /* (the low half of a generic LDS address is the LDS address) */
#define MCQ_XLIST(i) (LDS_LIST ? (uint32_t)list_l[i] : (uint32_t)list_g[i])
#else
    const uint16_t *list_g = wc.list[0];
#define MCQ_XLIST(i) ((uint32_t)list_g[i])
#endif
    const uint32_t n_opp = PIN ? mcq_opaque_uniform(qc.n_players - 1u) : qc.n_players - 1u;
    McqHole opp[MCQ_MAX_OPP];
    bool dealt = true;
#define MCQ_XOPP(P)                                                                                                 \
    if (P < n_opp) {                                                                                                \
        const uint32_t dhi = (uint32_t)(deck >> 32), dlo = (uint32_t)deck;                                          \
        const uint32_t top = mcq_deck_top(dlo, dhi);                                                                \
        uint32_t c1 = 0, c2 = 0, trial = 0;                                                                         \
        bool ok = false;                                                                                            \
        for (; trial < MCQ_EXT_MAX_TRIALS && !ok; trial++) {                                                        \
            const uint32_t e = MCQ_XLIST(dr.pick(n));                                                               \
            c1 = e & 0xFFu;                                                                                         \
            c2 = e >> 8;                                                                                            \
            ok = (((deck >> c1) & (deck >> c2)) & 1u) != 0u && c2 != top; /* both still there, B not the highest */ \
        }                                                                                                           \
        acc.passes += trial; /* (the lane's own count: lanes leave the loop at different trials) */                 \
        dealt = dealt && ok;                                                                                        \
        if (ok && c2 > c1) c2 = mcq_deck_next(dlo, dhi, c2); /* deck.pop(r2) after deck.pop(r1), l.178-179 */       \
        /* (c1, c2 are entries of the list -- card ids below 52 -- or, with an empty trial budget, zero: no clamp) */ \
        deck &= ~(((uint64_t)1 << c1) | ((uint64_t)1 << c2));                                                       \
        MCQ_EXT_DEALT(P + 1u, c1, c2);                                                                              \
        opp[P].set(cards[c1], cards[c2]);                                                                           \
    }
    MCQ_XOPP(0) MCQ_XOPP(1) MCQ_XOPP(2) MCQ_XOPP(3) MCQ_XOPP(4) MCQ_XOPP(5) MCQ_XOPP(6) MCQ_XOPP(7) MCQ_XOPP(8)
#undef MCQ_XOPP
#undef MCQ_XLIST
    uint32_t dlo = (uint32_t)deck, dhi = (uint32_t)(deck >> 32);
    uint32_t L = mcq_popc(qc.fdeck_lo) + mcq_popc(qc.fdeck_hi) - 2u * n_opp; /* wave-uniform: no counting per lane */
    McqBoard b = qc.board;
    for (uint32_t k = 0; k < qc.n_deal; k++, L--) {
        const uint32_t c = mcq_select_pop(dlo, dhi, dr.table(k, L - 1u), sel8);
        MCQ_EXT_DEALT(0x100u + k, c, 0u);
        b.add(cards[c < 52u ? c : 0u]);
    }
    McqFlushSel fs;
    fs.from_board(b);
    const uint32_t hk = mcq_eval_key(b, fs, qc.hero, tf, tops, sd);
    uint32_t best = 0;
    uint32_t n_equal = 0; /* (split-pot form only) opponents whose key equals hero's */
    const uint32_t n_opp_e = PIN ? mcq_opaque_uniform(qc.n_players - 1u) : qc.n_players - 1u;
#define MCQ_XEVAL(P)                                                  \
    if (P < n_opp_e) {                                                \
        const uint32_t k = mcq_eval_key(b, fs, opp[P], tf, tops, sd); \
        if (Acc::kWays) n_equal += k == hk ? 1u : 0u;                 \
        best = k > best ? k : best;                                   \
    }
    MCQ_XEVAL(0) MCQ_XEVAL(1) MCQ_XEVAL(2) MCQ_XEVAL(3) MCQ_XEVAL(4) MCQ_XEVAL(5) MCQ_XEVAL(6) MCQ_XEVAL(7) MCQ_XEVAL(8)
#undef MCQ_XEVAL
    uint64_t won = hk >= best ? 1u : 0u;
    acc.types += won << (6u * (hk >> MCQ_KEY_SHIFT));
    if constexpr (Acc::kWays) acc.ways += won << (6u * n_equal); /* pot shared by 1 + n_equal hands */
    else acc.tie += hk == best ? 1u : 0u;
    return dealt;
}
