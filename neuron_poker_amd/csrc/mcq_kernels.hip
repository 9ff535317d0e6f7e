// mcq_kernels.hip -- gfx950 kernels of the equity engine.
//
// Work decomposition: a WAVE TASK is 1024 iterations of one query; the 64 lanes of the
// wave each run 16 of them (production mode: lane = one RNG stream of 16 consecutive iterations; parity
// mode: iterations interleaved so that the draw bytes of a wave are contiguous).  All lanes of a wave work
// on the same query, so deck length, loop bounds and the query record are wave-uniform (SGPRs, scalar
// branches) and no lane diverges.  The task list, weighted by an instruction estimate per query, is cut into
// one contiguous slice per resident wave: a wave keeps its tallies in registers while the query stays the
// same and issues one set of atomics per (wave, query) -- HBM traffic stays at the algorithmic 120 B/query
// plus a few KB of table image per block.
//
// Memory: 16 B in / 104 B out per QUERY; per iteration nothing touches HBM in production mode (parity mode
// reads <= 23 draw bytes).  LDS holds the lookup tables (the bulk kernel: the 115 KB rank-sum image; the flush table is read
// from global memory), one 64-entry base deck per wave (16 KB a block) and, in the bulk kernel, one hole table per wave: the
// same cards by flush suit, as the opponents' hands read them (25 KB a block) -- 156 KB of the CU's 160.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "mcq_axis.hpp"
#include "mcq_device.hpp"
#include "mcq_exact.hpp"
#include "mcq_exact_ext.hpp"
#include "mcq_exact_hero.hpp"
#include "mcq_exact_hero_pre.hpp"
#include "mcq_exact_matrix.hpp"
#include "mcq_exact_runout.hpp"
#include "mcq_hands.hpp"
#include "mcq_internal.hpp"
#include "mcq_mt.hpp"
#include "mcq_mt_ext.hpp"
#include "mcq_mt_blocks.hpp"
#include "mcq_ranges.hpp"
#include "mcq_stage.hpp"
#include "mcq_tally.hpp"

namespace {

/* The base decks of a block's waves (McqDeckSplit): the X arrays of all waves, 64 entries each, then their Y arrays ONE
 * entry further than a whole number of arrays, so that the distance between a card's two reads is no offset pair a
 * two-address read could encode.  Entry 63 of the last wave's Y array would lie behind the table: it is never written (a
 * deck holds 50 cards at most, the entries behind it are nobody's). */
constexpr uint32_t kDeckY = 1024 + 1;
typedef McqDeckSplit<kDeckY> McqDeckLds;
constexpr int kMaxBlock = 1024; /* 16 waves = 4 per SIMD; one block per CU: tables 97-115 KB + 16 base decks 16 KB (+ 16 hole tables 25 KB) of the 160 KB LDS */
static_assert(kDeckY == kMaxBlock + 1 && 8u * kDeckY >= 2048u && (8u * kDeckY) % 512u != 0u,
              "the Y arrays start one entry behind the block's X arrays: beyond a two-address read's offsets");
static_assert((kMaxBlock - 64) + kDeckY + 62 < 2 * kMaxBlock, "entries 0..62 of the last wave's Y array lie inside base_tab");
/* The bulk kernel's deck: beside them one hole table per wave, the opponents' cards by flush suit (McqDeckBySuit).  The
 * layout is a measured choice: 1 suit-major, 0 position-major. */
#ifndef MCQ_HOLE_LAYOUT
#define MCQ_HOLE_LAYOUT 1
#endif
typedef McqDeckBySuit<kDeckY, MCQ_HOLE_LAYOUT ? 3u : 5u, MCQ_HOLE_LAYOUT ? 8u * MCQ_HOLE_POSITIONS : 8u> McqDeckBulk;
constexpr uint32_t kHoleShift = MCQ_HOLE_LAYOUT ? 3u : 5u;
constexpr int kExtBlock = 1024; /* extended queries: 40 KB of dealt card ids beside the tables */

// A launch with or without the pair of timestamp events (mcq_set_kernel_timing): the timestamped form costs a
// one-launch query about 6 us of its call time on this pool (tools/launch_floor.hip), so it is only used on request.
#define MCQ_LAUNCH_TIMED(kern, grid, block, ...)                                                  \
    do {                                                                                          \
        if (t0 || t1) hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, s, t0, t1, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, s, __VA_ARGS__);                \
    } while (0)

// Sum over the 64 lanes of a whole wave (EXEC full), wave-uniform result: four DPP adds bring every 16-lane row to
// its row sum (quad_perm [1,0,3,2], [2,3,0,1], row_ror:4, row_ror:8 -- plain VALU rate), four v_readlane add the rows.
// The shuffle form below goes through the LDS crossbar once per step (ds_bpermute): ~1 us for a row of twelve sums.
__device__ __forceinline__ uint32_t wave_sum_dpp(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

struct LdsTablesEval { /* per block: what the kernels keep in LDS; tf stays in global memory (see McqTables) */
    uint32_t tops[8192];
    uint32_t sd[16384];
    uint32_t sel8[256];
};
static_assert(__builtin_offsetof(LdsTablesEval, sel8) == MCQ_TF_BYTE_OFFSET, "first 96 KB of McqTables");

__device__ __forceinline__ void load_tables(LdsTablesEval &dst, const McqTables *__restrict__ g) {
    const uint4 *src = reinterpret_cast<const uint4 *>(g);
    uint4 *d = reinterpret_cast<uint4 *>(&dst);
    constexpr uint32_t kVec = MCQ_TF_BYTE_OFFSET / 16; /* tops, sd | kc */
    uint32_t i = threadIdx.x;
    for (; i + 7u * blockDim.x < kVec; i += 8u * blockDim.x) { /* eight 16-byte loads in flight per lane */
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = src[i + k * blockDim.x];
#pragma unroll
        for (int k = 0; k < 8; k++) d[i + k * blockDim.x] = v[k];
    }
    for (; i < kVec; i += blockDim.x) d[i] = src[i];
    for (uint32_t j = threadIdx.x; j < 256u; j += blockDim.x) dst.sel8[j] = g->sel8[j];
    __syncthreads();
}

// The plain evaluation kernels' image: the rank-sum hash and sel8 (McqSumImage, 115 KB), one contiguous copy.
__device__ __forceinline__ void load_sum_tables(McqSumImage &dst, const McqTables *__restrict__ g) {
    const uint4 *src = reinterpret_cast<const uint4 *>(&g->sum);
    uint4 *d = reinterpret_cast<uint4 *>(&dst);
    constexpr uint32_t kVec = sizeof(McqSumImage) / 16;
    uint32_t i = threadIdx.x;
    for (; i + 7u * blockDim.x < kVec; i += 8u * blockDim.x) { /* eight 16-byte loads in flight per lane */
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = src[i + k * blockDim.x];
#pragma unroll
        for (int k = 0; k < 8; k++) d[i + k * blockDim.x] = v[k];
    }
    for (; i < kVec; i += blockDim.x) d[i] = src[i];
    __syncthreads();
}

// Exclusive prefix sum of one value per thread (T: uint32_t or uint64_t) over a block of WAVES waves (two barriers):
// wave-level scan by shuffles, the wave totals through LDS.  Returns the sum of the values of all lower threads;
// *total = block sum.
template <class T, uint32_t WAVES>
__device__ __forceinline__ T block_exclusive_scan(T v, T *wave_tot /* LDS, WAVES entries */, T *total) {
    typedef std::conditional_t<sizeof(T) == 8, unsigned long long, unsigned int> Shfl;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = (T)__shfl_up((Shfl)inc, off, 64);
        if (lane >= (uint32_t)off) inc += o;
    }
    __syncthreads(); /* wave_tot may still be read from the previous call */
    if (lane == 63u) wave_tot[wv] = inc;
    __syncthreads();
    T at = inc - v, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < WAVES; k++) {
        const T t = wave_tot[k];
        at += k < wv ? t : (T)0;
        all += t;
    }
    *total = all;
    return at;
}

// ---------------------------------------------------------------------------------------------- prep
// The preparation of a batch on the extended and the ranges path, one block of 1024 threads: price(i) says whether record
// i is valid, what it costs on the cost axis (mcq_axis.hpp; nothing when it is invalid) and the `runs` its row starts with.
// Writes the rows -- runs, passes = 0 (UINT64_MAX marks an invalid record), zeros behind them -- and the exclusive
// prefix of the costs, 1024 records at a time with the running total carried over; prefix[n] = the total.
struct McqPrepRecord {
    bool ok;
    uint64_t cost, runs;
};
template <uint32_t ROW_WORDS, class Price>
__device__ __forceinline__ void mcq_prep_rows(uint32_t n, mcq_result *__restrict__ res, uint64_t *__restrict__ prefix, Price price) {
    __shared__ uint64_t wave_tot[16];
    uint64_t carry = 0; /* every thread keeps the running total */
    const uint32_t tid = threadIdx.x;
    for (uint32_t base = 0; base < n; base += 1024) {
        uint32_t i = base + tid;
        uint64_t cost = 0;
        if (i < n) {
            const McqPrepRecord rec = price(i);
            cost = rec.ok ? rec.cost : 0ull;
            uint64_t *r = reinterpret_cast<uint64_t *>(res) + (size_t)i * ROW_WORDS;
            r[0] = rec.ok ? rec.runs : 0ull;
            r[1] = rec.ok ? 0ull : ~0ull;
#pragma unroll
            for (int k = 2; k < (int)ROW_WORDS; k++) r[k] = 0;
        }
        uint64_t chunk_total;
        const uint64_t before = block_exclusive_scan<uint64_t, 16>(cost, wave_tot, &chunk_total);
        if (i < n) prefix[i] = carry + before;
        carry += chunk_total;
    }
    if (tid == 0) prefix[n] = carry;
}

// The plain path's preparation, one block: the same rows, markers and prefix (its own chunk loop), and what only this
// path has -- the share of a query that belongs to this launch, the invalid marker from ONE share only, and the task sums
// that pick the small batches' cut.
// ROW_WORDS: 64-bit words of a result row, 13 (mcq_result) or 22 (mcq_result_ways).
template <uint32_t ROW_WORDS>
__global__ __launch_bounds__(1024) void mcq_prep_kernel(const mcq_query *__restrict__ q, uint32_t n,
                                                        mcq_result *__restrict__ res, uint64_t *__restrict__ prefix,
                                                        uint32_t part_idx, uint32_t n_parts, uint32_t n_cu,
                                                        uint32_t split_max) {
    __shared__ uint64_t wave_tot[16];
    uint64_t carry = 0; /* every thread keeps the running total */
    __shared__ unsigned long long sum_tasks;
    __shared__ uint32_t max_tasks;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        sum_tasks = 0;
        max_tasks = 0;
    }
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024) {
        uint32_t i = base + tid;
        uint64_t cost = 0;
        uint32_t my_tasks = 0;
        if (i < n) {
            const uint4 raw = reinterpret_cast<const uint4 *>(q)[i];
            const McqQueryWords qq = {raw.x, raw.y, raw.z, raw.w};
            bool ok = mcq_query_valid(qq);
            /* this launch's share of the query: tasks [t_lo, t_hi) (everything unless the iterations are split
             * over devices, mcq_eval_batch_part) */
            const McqPart pt = mcq_part(mcq_task_count(qq), qq.runs(), part_idx, n_parts);
            cost = ok ? (uint64_t)(pt.t_hi - pt.t_lo) * mcq_task_weight(qq) : 0ull;
            my_tasks = ok ? pt.t_hi - pt.t_lo : 0u;
            uint64_t *r = ROW_WORDS == 13u ? reinterpret_cast<uint64_t *>(res + i)
                                           : reinterpret_cast<uint64_t *>(res) + (size_t)i * ROW_WORDS;
            r[0] = ok ? pt.runs : 0ull;
            r[1] = ok || part_idx != 0u ? 0ull : ~0ull; /* the marker of an invalid query: from ONE share only, so that the
                                                          * sum of the shares (same-device add, all-reduce) still shows it */
#pragma unroll
            for (int k = 2; k < (int)ROW_WORDS; k++) r[k] = 0;
        }
        if (n <= 1024u) { /* a possible small batch: what mcq_pick_split needs (below); one atomic per wave */
            const uint32_t ws = wave_sum(my_tasks);
            uint32_t wm = my_tasks;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const uint32_t o = __shfl_xor(wm, off, 64);
                wm = o > wm ? o : wm;
            }
            if ((tid & 63u) == 0u && ws) {
                atomicAdd(&sum_tasks, (unsigned long long)ws);
                atomicMax(&max_tasks, wm);
            }
        }
        uint64_t chunk_total;
        const uint64_t before = block_exclusive_scan<uint64_t, 16>(cost, wave_tot, &chunk_total);
        if (i < n) prefix[i] = carry + before;
        carry += chunk_total;
    }
    __syncthreads(); /* sum_tasks / max_tasks are complete */
    if (tid == 0) {
        prefix[n] = carry;
        /* the cut for MCQ_SPLIT_FROM_PREP launches (queries resident in HBM, at most 1024 of them) */
        prefix[n + 1] = n <= 1024u && sum_tasks ? mcq_pick_split(sum_tasks, max_tasks, n_cu, split_max) : 0u;
        prefix[n + 2] = 0; /* work counter of mcq_mt_parse_kernel */
    }
}

// ---------------------------------------------------------------------------------------------- parity mode: MT19937
// TWO waves per query walk np.random.seed(seed32 + query index)'s stream (mcq_mt.hpp) and leave the accepted draws in
// the draw-major global buffer the evaluation kernel reads, `passes` in the query's result row:
//   wave 0, the PRODUCER, owns the 624-word state: it regenerates a block and tempers it into a buffer of
//           (y & 63) | 0x80 bytes -- independent work at the full issue rate, a block ahead of
//   wave 1, the PARSER, whose chain of dependent steps per batch of 64 words (mcq_mt_batch) is what bounds the walk: it
//           only reads bytes.
// One block = one pair = 128 threads: the block barrier is the pair's hand-over, once per 624 words (two buffers: the
// producer fills block b + 1 while block b is parsed).  The parser tells the producer at which barrier to stop.
// Queries are handed out through an atomic counter (their lengths differ).  7.7 KB of LDS per pair: 16 pairs per CU.
constexpr int kMtBlock = 128;
constexpr uint32_t kMtBlocksPerCu = 16u; /* grid cap of the launch: what a CU holds at once, 16 work-groups */
struct McqMtPairWave { /* what mcq_mt_batch touches: the position tables and the ring as in McqMtWave, the words as bytes */
    uint32_t ptab[MCQ_MT_POSITIONS];
    uint8_t ring[(MCQ_MT_MAX_DRAWS + 1u) * MCQ_MT_ROW];
    uint8_t yb[2][MCQ_MT_N + 64u]; /* + 64: a batch reads 64 bytes from its position */
    volatile uint32_t stop_at;     /* the producer leaves behind its barrier number stop_at (0 = not yet known) */
    uint32_t qi;
};
struct McqMtProducer {
    uint32_t mt[MCQ_MT_N + 64u];
};
/* the buffer being parsed: st.src, its byte offset (the first hand-over makes it buffer 0: the state starts at buffer 1) */
constexpr uint32_t kMtYbBytes = MCQ_MT_N + 64u;
__device__ __forceinline__ uint32_t mcq_mt_word_yb(const McqMtPairWave &w, const McqMtState &st, uint32_t i) {
    return (&w.yb[0][0])[st.src + i];
}
__device__ __forceinline__ void mcq_mt_emit_lane(McqMtPairWave &, bool, uint32_t, uint32_t, uint32_t, uint32_t) {}
__device__ __forceinline__ constexpr bool mcq_mt_padded(const McqMtPairWave &) { return true; } /* yb[.][624 .. 688) = 0xFF */
__device__ __forceinline__ void mcq_mt_next_block(McqMtPairWave &, McqMtState &st) {
    __syncthreads(); /* the producer has filled the other buffer; it may now overwrite the one just parsed */
    st.blocks += 1u; /* (= barriers the parser has passed) */
    st.src = kMtYbBytes - st.src;
}

__global__ __launch_bounds__(kMtBlock) void mcq_mt_parse_kernel(const mcq_query *__restrict__ queries, uint32_t n,
                                                                uint32_t seed32, uint8_t *__restrict__ draws,
                                                                const uint64_t *__restrict__ draw_off,
                                                                mcq_result *__restrict__ res, uint32_t *__restrict__ counter,
                                                                uint32_t row_words) {
    __shared__ __attribute__((aligned(16))) McqMtPairWave w;
    __shared__ __attribute__((aligned(16))) McqMtProducer prod;
    const uint32_t lane = threadIdx.x & 63u;
    const bool producer = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0u;
    w.yb[threadIdx.x >> 6][MCQ_MT_N + lane] = 0xFFu; /* behind both buffers' words: accepted nowhere (mcq_mt_padded) */
    for (;;) {
        if (threadIdx.x == 0) {
            w.qi = atomicAdd(counter, 1u);
            w.stop_at = 0u;
        }
        __syncthreads();
        const uint32_t qi = __builtin_amdgcn_readfirstlane(w.qi);
        if (qi >= n) break;
        const uint4 raw = reinterpret_cast<const uint4 *>(queries)[qi];
        const McqQueryWords q = {(uint32_t)__builtin_amdgcn_readfirstlane(raw.x), (uint32_t)__builtin_amdgcn_readfirstlane(raw.y),
                                 (uint32_t)__builtin_amdgcn_readfirstlane(raw.z), (uint32_t)__builtin_amdgcn_readfirstlane(raw.w)};
        const uint32_t n_opp = q.n_players() - 1u, n_deal = 5u - q.n_board(), runs = q.runs();
        /* block-uniform: invalid queries and queries that draw nothing keep passes = 0 */
        if (mcq_query_valid(q) && 2u * n_opp + n_deal != 0u && runs != 0u) {
            if (producer) {
                mcq_mt_seed(prod, seed32 + qi);
                MCQ_WAVE_SYNC();
                for (uint32_t b = 0;; b++) {
                    mcq_mt_regenerate(prod);
                    uint8_t *dst = w.yb[b & 1u];
#pragma unroll
                    for (uint32_t k = 0; k < MCQ_MT_N + 63u; k += 64u) /* ten steps of independent lanes */
                        if (k + lane < MCQ_MT_N) dst[k + lane] = (uint8_t)((mcq_mt_temper(prod.mt[k + lane]) & 63u) | 0x80u);
                    __syncthreads(); /* barrier number b + 1: block b is there */
                    if (w.stop_at == b + 1u) break;
                }
            } else {
                McqMtState st = {MCQ_MT_N, 0u, 0u, 0u, 0ull, 0u, kMtYbBytes};
                mcq_mt_parse_query(w, st, 50u - q.n_board(), n_opp, n_deal, runs, draws + draw_off[qi],
                                   ((uint64_t)runs + 63u) & ~63ull);
                /* every lane stores the same word: a store under `lane == 0` here would be a divergent branch in front of
                 * the barrier */
                reinterpret_cast<unsigned long long *>(res)[(size_t)qi * row_words + 1u] = st.passes;
                if (lane == 0) w.stop_at = st.blocks + 1u; /* the producer is filling one more block: it leaves behind the next barrier */
                __syncthreads();
            }
        }
        __syncthreads(); /* both waves are done with this query's LDS */
    }
}

// The same for extended queries (mcq_mt_ext.hpp: the reference's loops over ranges, ghost cards and known hands walked
// stage by stage).  6.5 KB of LDS per wave.  A query whose range cannot be dealt gets passes = UINT64_MAX.
// ROW_WORDS: as mcq_prep_kernel (the walk itself, and what it stores, are the same for either row).
constexpr int kMtExtBlock = 256;
constexpr uint32_t kMtExtBlocksPerCu = 5u; /* grid cap of the launch: what fits a CU at once, 27 KB of LDS per block */
template <uint32_t ROW_WORDS>
__global__ __launch_bounds__(kMtExtBlock) void mcq_mt_parse_ext_kernel(const mcq_query *__restrict__ queries,
                                                                    const mcq_query_ext *__restrict__ ext, uint32_t n, uint32_t seed32,
                                                                    uint8_t *__restrict__ draws, const uint64_t *__restrict__ draw_off,
                                                                    mcq_result *__restrict__ res, uint32_t *__restrict__ counter) {
    __shared__ __attribute__((aligned(16))) McqMtExtWave ws[kMtExtBlock / 64];
    McqMtExtWave &w = ws[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u;
    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(counter, 1u);
        const uint32_t qi = __builtin_amdgcn_readfirstlane(t);
        if (qi >= n) break;
        const uint4 raw = reinterpret_cast<const uint4 *>(queries)[qi];
        const McqQueryWords q = {(uint32_t)__builtin_amdgcn_readfirstlane(raw.x), (uint32_t)__builtin_amdgcn_readfirstlane(raw.y),
                                 (uint32_t)__builtin_amdgcn_readfirstlane(raw.z), (uint32_t)__builtin_amdgcn_readfirstlane(raw.w)};
        const uint32_t *ew = reinterpret_cast<const uint32_t *>(ext + qi);
        const McqExtRec er = {ew};
        if (mcq_query_ext_valid(q, er) && q.runs() != 0u) { /* wave-uniform */
            MCQ_WAVE_SYNC(); /* the previous query's reads of this wave's LDS are done */
            mcq_mt_seed(w, seed32 + qi);
            MCQ_WAVE_SYNC();
            McqMtExtState st = {MCQ_MT_N, 0u, 0u, 0u, 0u, 0u, 0ull, false};
            const bool ok = mcq_mt_parse_query_ext(w, st, q, ew, draws + draw_off[qi], ((uint64_t)q.runs() + 63u) & ~63ull);
            /* (every lane stores the same word: no divergent branch in front of the loop's back edge) */
            (reinterpret_cast<unsigned long long *>(res) + (size_t)qi * ROW_WORDS)[1] = ok ? st.passes : ~0ull;
        }
    }
}

// ---------------------------------------------------------------------------------------------- few long queries
// mcq_mt_blocks.hpp: the stream of a query parsed with its state blocks side by side -- four kernels behind one another
// on the stream.  blk_off[q] .. blk_off[q + 1]: the query's blocks in the shared arrays (none: the query draws nothing
// or is invalid); gridDim.y = queries where the grid is two-dimensional.
//
// 1. generate.  The MT19937 recurrence is the one serial thing left: x[k] of the next state needs x[k], x[k + 1] and
// x[k + 397] of this one, or -- from k = 227 on -- x[k - 227] of the NEXT: three sweeps of at most 227 words, each
// waiting for the one before.  But the word a sweep waits for is the one the SAME thread has just made (k - 227 is
// thread t's word of the sweep before), so thread t makes x[t], x[227 + t] and x[454 + t] out of registers, from seven
// words of the finished state that it reads at once -- one LDS round trip and one barrier per block instead of three
// (1.73 -> 0.6 ms for the 3 900 blocks of a 6-max 100 000-run query).  (x[623] needs the new x[0]: its thread makes that
// one a second time.)  Two state buffers; three more waves copy the state the first four are reading to HBM as it is --
// 2 496 B per block; the waves that read it temper it (mcq_mtb_load_block): off the chain, and side by side.
//
// Round 4: a query's blocks in SEGMENTS of MCQ_MTB_SEG, one work-group each, side by side.  The generator is linear over
// GF(2): the state J words ahead is a fixed XOR combination of 19 937 + 623 consecutive words, the same for every seed
// (mcq_mt_jump_table.inc: t^J mod the characteristic polynomial, made and checked against numpy by
// tools/mt_jump_table.py).  Per round of MCQ_MTB_MAX_SEG segments, from base block `base` (state number `base`: the seed
// state, or the last block of the round before): (a) this kernel, one work-group per query, makes the first 33 blocks --
// the words every jump of the round combines; (b) mcq_mtb_jump_kernel: segment g's start state, kMtbJumpSplit work-groups
// each XORing their share of the polynomial's terms over all 624 words (partial sums to HBM); (c) this kernel again, a
// work-group per (segment, query): start state = the seed state / the block in front / the XOR of the partial sums.
#define MCQ_MTB_TABLE_ATTR __device__ const
#include "mcq_mt_jump_table.inc"
constexpr uint32_t kMtbJumpSplit = 8, kMtbJumpWords = MCQ_MT_N / kMtbJumpSplit; /* 78 words of the polynomial per work-group */
constexpr uint32_t kMtbJumpSpan = MCQ_MT_N / 32u + 14u; /* blocks whose words a round's jumps read: 19 937 + 623 words = 33 */
static_assert(kMtbJumpSplit * kMtbJumpWords == MCQ_MT_N && kMtbJumpWords % 2u == 0u, "the polynomial's words split evenly, in pairs");
static_assert(kMtbJumpSpan * MCQ_MT_N >= 32u * MCQ_MT_N + MCQ_MT_N - 1u && kMtbJumpSpan == 33u && kMtbJumpSpan <= MCQ_MTB_SEG, "words 0 .. 20 590");
constexpr int kMtbGenBlock = 512;
/* part: [query][segment - 1][kMtbJumpSplit][624] partial sums of the jumps (mcq_mtb_jump_kernel).  limit: blocks a
 * work-group makes at most (kMtbJumpSpan for step (a), MCQ_MTB_SEG for step (c)) */
__global__ __launch_bounds__(kMtbGenBlock) void mcq_mtb_generate_kernel(const uint32_t *__restrict__ blk_off, uint32_t seed32,
                                                                       uint32_t *__restrict__ raw, const uint32_t *__restrict__ part,
                                                                       uint32_t base, uint32_t limit, uint32_t for_jumps) {
    __shared__ __attribute__((aligned(16))) uint32_t mt[2][MCQ_MT_N + 8u];
    const uint32_t qi = blockIdx.y, g = blockIdx.x, tid = threadIdx.x, first = blk_off[qi], nb_q = blk_off[qi + 1u] - first;
    const uint32_t start = base + g * MCQ_MTB_SEG;
    if (start >= nb_q) return; /* (block-uniform) */
    if (for_jumps && nb_q - base <= MCQ_MTB_SEG) return; /* step (a) of a query with one segment: no jump reads it */
    const uint32_t nb = nb_q - start < limit ? nb_q - start : limit;
    if (start == 0u) {
        if (tid == 0) { /* np.random.seed: init_genrand, a serial recurrence */
            uint32_t x = seed32 + qi;
            mt[0][0] = x;
            for (uint32_t i = 1; i < MCQ_MT_N; i++) {
                x = 1812433253u * (x ^ (x >> 30)) + i;
                mt[0][i] = x;
            }
        }
    } else if (g == 0u) { /* a later round: the block in front */
        const uint32_t *src = raw + (uint64_t)(first + start - 1u) * MCQ_MT_N;
        for (uint32_t i = tid; i < MCQ_MT_N; i += kMtbGenBlock) mt[0][i] = src[i];
    } else { /* the jump's partial sums */
        const uint32_t *src = part + ((uint64_t)qi * (MCQ_MTB_MAX_SEG - 1u) + (g - 1u)) * kMtbJumpSplit * MCQ_MT_N;
        for (uint32_t i = tid; i < MCQ_MT_N; i += kMtbGenBlock) {
            uint32_t x = 0;
#pragma unroll
            for (uint32_t w = 0; w < kMtbJumpSplit; w++) x ^= src[w * MCQ_MT_N + i];
            mt[0][i] = x;
        }
    }
    __syncthreads();
    uint32_t *dst = raw + (uint64_t)(first + start) * MCQ_MT_N;
    /* two loops with the same barriers: the waves that make the state, the waves that copy it out */
    if (tid < 256u) { /* (wave-uniform) */
        /* every read up front, none behind a condition on the thread (indices clamped instead): ONE round trip to LDS per
         * block.  Threads 227 .. 255 repeat thread 226's work and store nothing. */
        const uint32_t t = tid < 226u ? tid : 226u, tc = t < 169u ? t : 169u;
        const bool w_ab = tid < 227u, w_c = tid < 170u, is_last = tid == 169u;
        for (uint32_t b = 0; b <= nb; b++) { /* state b -> state b + 1 */
            const uint32_t *S = mt[b & 1u];
            uint32_t *N = mt[(b + 1u) & 1u];
            if (b < nb) {
                const uint32_t a0 = S[t], a1 = S[t + 1u], f = S[t + MCQ_MT_M], b0 = S[227u + t], b1 = S[228u + t];
                const uint32_t c0 = S[454u + tc], c1o = S[455u + tc] /* (tc = 169: the padding behind the state) */;
                /* (opaque, or the compiler moves these three reads into thread 169's branch, behind the wait for the others) */
                uint32_t z0 = S[0], z1 = S[1], zf = S[MCQ_MT_M];
                asm volatile("" : "+v"(z0), "+v"(z1), "+v"(zf));
                const uint32_t c1 = is_last ? zf ^ mcq_mt_twist(z0, z1) /* the new x[0] */ : c1o;
                const uint32_t nA = f ^ mcq_mt_twist(a0, a1);
                const uint32_t nB = nA ^ mcq_mt_twist(b0, b1);
                if (w_ab) {
                    N[t] = nA;
                    N[227u + t] = nB;
                }
                if (w_c) N[454u + t] = nB ^ mcq_mt_twist(c0, c1);
            }
            __syncthreads(); /* state b + 1 is complete; state b has been read for the last time */
        }
    } else {
        const uint32_t t = tid - 256u;
        for (uint32_t b = 0; b <= nb; b++) { /* the segment's block b - 1 = state b */
            if (b >= 1u && t < MCQ_MT_N / 4u)
                reinterpret_cast<uint4 *>(dst + (uint64_t)(b - 1u) * MCQ_MT_N)[t] = *reinterpret_cast<const uint4 *>(mt[b & 1u] + 4u * t);
            __syncthreads();
        }
    }
}

// 1b. jump: work-group (segment g >= 1, share w) of a query: out[j] = XOR over the set coefficients i of its 78 words of
// the polynomial of y[i + j], j < 624 -- y = the round's first 33 blocks.  The floor is LDS bandwidth (6.2 M word reads per
// jump), so the reads are 16 bytes wide: a lane owns j = 4 l .. 4 l + 3 (+ 256, + 512) and reads y[i + 4 l ..] with ONE
// ds_read_b128 -- aligned whatever i is, because the share's window of y lies in LDS four times, shifted by 0 .. 3 words.
// The set coefficients are laid out once per work-group as a list of byte offsets (copy + aligned position) in LDS, so a
// term costs no scalar bit scan: a broadcast read serves eight terms, each term one address add, three wide reads and
// twelve XORs.  Sixteen waves take the list's terms in turn and add their sums up through LDS.
constexpr int kMtbJumpBlock = 1024;
constexpr uint32_t kMtbJumpTerms = kMtbJumpWords * 32u;           /* coefficients of a share: 2496 */
constexpr uint32_t kMtbJumpCopy = kMtbJumpTerms + 768u;           /* words of one copy of the window: terms + the lanes' offsets */
__global__ __launch_bounds__(kMtbJumpBlock) void mcq_mtb_jump_kernel(const uint32_t *__restrict__ blk_off,
                                                                    const uint32_t *__restrict__ raw, uint32_t *__restrict__ part,
                                                                    uint32_t base) {
    __shared__ __attribute__((aligned(16))) uint32_t s_y[4][kMtbJumpCopy]; /* s_y[c][k] = y[i_lo + k + c]; later: the waves' sums */
    __shared__ __attribute__((aligned(16))) uint16_t s_list[kMtbJumpTerms + 8u * (kMtbJumpBlock / 64)];
    __shared__ uint32_t s_cnt[kMtbJumpWords + 1u], s_pop[kMtbJumpWords];
    static_assert(sizeof(s_y) >= (kMtbJumpBlock / 64) * 768u * 4u, "the sums of sixteen waves fit where the window was");
    static_assert(4u * kMtbJumpCopy * 4u < 65536u, "byte offsets as 16-bit words");
    const uint32_t qi = blockIdx.y, g = blockIdx.x / kMtbJumpSplit + 1u, w = blockIdx.x % kMtbJumpSplit, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t first = blk_off[qi], nb_q = blk_off[qi + 1u] - first;
    if (base + g * MCQ_MTB_SEG >= nb_q) return; /* (block-uniform) */
    const uint32_t i_lo = w * kMtbJumpTerms;
    const uint32_t *src = raw + (uint64_t)(first + base) * MCQ_MT_N;
    constexpr uint32_t kSpanWords = kMtbJumpSpan * MCQ_MT_N;
    for (uint32_t k = tid; k < kMtbJumpCopy + 3u; k += kMtbJumpBlock) {
        const uint32_t v = i_lo + k < kSpanWords ? src[i_lo + k] : 0u;
#pragma unroll
        for (uint32_t c = 0; c < 4u; c++)
            if (k >= c && k - c < kMtbJumpCopy) s_y[c][k - c] = v;
    }
    const uint32_t *gw = kMtJump[g - 1u] + w * kMtbJumpWords;
    if (tid < kMtbJumpWords) s_pop[tid] = (uint32_t)__builtin_popcount(gw[tid]);
    __syncthreads();
    if (tid <= kMtbJumpWords) { /* terms in front of word tid: independent reads, no chain */
        uint32_t x = 0;
#pragma unroll
        for (uint32_t k = 0; k < kMtbJumpWords; k++) x += k < tid ? s_pop[k] : 0u;
        s_cnt[tid] = x;
    }
    __syncthreads();
    const uint32_t n_terms = s_cnt[kMtbJumpWords];
    for (uint32_t t = tid; t < kMtbJumpTerms; t += kMtbJumpBlock) {
        const uint32_t word = gw[t >> 5], bit = t & 31u;
        if ((word >> bit) & 1u) {
            const uint32_t c = t & 3u;
            s_list[s_cnt[t >> 5] + (uint32_t)__builtin_popcount(word & ((1u << bit) - 1u))] = (uint16_t)((c * kMtbJumpCopy + (t - c)) * 4u);
        }
    }
    /* padding: a wave reads its terms eight at a time; the terms behind the last point at ... a term twice = no term */
    if (tid < 8u * (kMtbJumpBlock / 64)) s_list[n_terms + tid] = 0xFFFFu;
    __syncthreads();
    uint4 acc[3] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    const char *ybase = reinterpret_cast<const char *>(&s_y[0][0]) + 16u * lane;
    /* wave wv takes the terms 8 (16 k + wv) .. + 8 */
    for (uint32_t t0 = 8u * wv; t0 < n_terms; t0 += 8u * (kMtbJumpBlock / 64)) {
        const uint4 pkv = *reinterpret_cast<const uint4 *>(s_list + t0); /* (a broadcast read; into scalar registers) */
        const uint32_t pk[4] = {(uint32_t)__builtin_amdgcn_readfirstlane(pkv.x), (uint32_t)__builtin_amdgcn_readfirstlane(pkv.y),
                                (uint32_t)__builtin_amdgcn_readfirstlane(pkv.z), (uint32_t)__builtin_amdgcn_readfirstlane(pkv.w)};
        const uint32_t off[8] = {pk[0] & 0xFFFFu, pk[0] >> 16, pk[1] & 0xFFFFu, pk[1] >> 16, pk[2] & 0xFFFFu, pk[2] >> 16, pk[3] & 0xFFFFu, pk[3] >> 16};
#pragma unroll
        for (uint32_t u = 0; u < 8u; u++) {
            if (off[u] == 0xFFFFu) break; /* (wave-uniform: behind the list's end) */
            const char *p = ybase + off[u];
#pragma unroll
            for (uint32_t h = 0; h < 3u; h++) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p + 1024u * h);
                acc[h].x ^= v.x;
                acc[h].y ^= v.y;
                acc[h].z ^= v.z;
                acc[h].w ^= v.w;
            }
        }
    }
    __syncthreads(); /* the window has been read for the last time */
    uint32_t *sums = &s_y[0][0]; /* [wave][768] */
#pragma unroll
    for (uint32_t h = 0; h < 3u; h++) *reinterpret_cast<uint4 *>(sums + wv * 768u + 256u * h + 4u * lane) = acc[h];
    __syncthreads();
    if (tid < MCQ_MT_N) {
        uint32_t x = 0;
#pragma unroll
        for (uint32_t k = 0; k < kMtbJumpBlock / 64; k++) x ^= sums[k * 768u + tid];
        part[(((uint64_t)qi * (MCQ_MTB_MAX_SEG - 1u) + (g - 1u)) * kMtbJumpSplit + w) * MCQ_MT_N + tid] = x;
    }
}

// 2. scan: one wave per (query, block); lane = entry state (mcq_mtb_automaton), the block's bytes through LDS.
constexpr int kMtbBlock = 256;
constexpr int kMtbParseBlock = 1024; /* parse: sixteen blocks per work-group (70 KB of LDS, two work-groups per CU), their attempts in one atomic */
/* a block's state words -> its bytes (y & 63) | 0x80 in LDS (dst: MCQ_MT_N + 64 bytes, the last 64 padding) */
__device__ __forceinline__ void mcq_mtb_load_block(const uint32_t *__restrict__ src, uint8_t *dst, uint32_t lane) {
    uint32_t y[10];
#pragma unroll
    for (uint32_t k = 0; k < 10u; k++) y[k] = src[64u * k + lane < MCQ_MT_N ? 64u * k + lane : MCQ_MT_N - 1u];
#pragma unroll
    for (uint32_t k = 0; k < 10u; k++)
        if (64u * k + lane < MCQ_MT_N) dst[64u * k + lane] = (uint8_t)((mcq_mt_temper(y[k]) & 63u) | 0x80u);
    dst[MCQ_MT_N + lane] = 0xFFu; /* (mcq_mt_padded) */
    MCQ_WAVE_SYNC();
}
__device__ __forceinline__ McqMtbPlan mcq_mtb_plan_of(const mcq_query *__restrict__ queries, uint32_t qi) {
    const uint4 raw = reinterpret_cast<const uint4 *>(queries)[qi];
    const McqQueryWords q = {(uint32_t)__builtin_amdgcn_readfirstlane(raw.x), (uint32_t)__builtin_amdgcn_readfirstlane(raw.y),
                             (uint32_t)__builtin_amdgcn_readfirstlane(raw.z), (uint32_t)__builtin_amdgcn_readfirstlane(raw.w)};
    return mcq_mtb_plan(50u - q.n_board(), q.n_players() - 1u, 5u - q.n_board(), q.runs());
}
__global__ __launch_bounds__(kMtbBlock) void mcq_mtb_scan_kernel(const mcq_query *__restrict__ queries,
                                                                const uint32_t *__restrict__ blk_off,
                                                                const uint32_t *__restrict__ raw, uint32_t *__restrict__ exits) {
    /* A block has n_st = D + n_opp <= 32 entry states, a wave has 64 lanes, and the automaton is a chain: a wave that is
     * alone or almost alone on its SIMD issues one vector instruction per 5-8 cycles whatever their dependence.  So a wave
     * takes ONE block and cuts it into U = 2 .. 8 PARTS (as many as 64 / n_st allows: eight for a heads-up query, three
     * six-max, two with nine or ten players), lane = (part, entry state): every part is walked from every entry state side
     * by side, and the block's exit words are composed from the parts' as a group's are from its blocks'
     * (mcq_mtb_compose_step) -- twice the waves of the version before, a chain of 624 / U words instead of 624.
     * (Round 4.  Measured on the 3 900 blocks of a 6-max 100 000-run query: one block per wave, 32 lanes idle, 98 us; two
     * blocks per wave 75 us; a branch-free step with both candidate table words fetched ahead 78 us; two or four blocks per
     * wave-half word by word in turn 106-125 us; two halves of one block 58 us; this: see profiles/r08_mtb_kernels.txt.) */
    __shared__ __attribute__((aligned(16))) uint8_t s_yb[kMtbBlock / 64][MCQ_MT_N + 64u];
    __shared__ uint32_t s_pos[kMtbBlock / 64][MCQ_MTB_POS];
    __shared__ uint32_t s_ex[kMtbBlock / 64][8][MCQ_MTB_LANES];
    static_assert(MCQ_MT_N % 8u == 0u && MCQ_MT_N % 6u == 0u, "parts of 78, 104, 156, 208, 312 words");
    const uint32_t qi = blockIdx.y, lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t first = blk_off[qi], nb = blk_off[qi + 1u] - first, b = blockIdx.x * (kMtbBlock / 64) + wv;
    if (b >= nb) return; /* (wave-uniform; no block barrier below) */
    const McqMtbPlan pl = mcq_mtb_plan_of(queries, qi);
    const uint32_t n_st = pl.D + (pl.two_opp >> 1), U = mcq_mtb_parts(pl), W = MCQ_MT_N / U; /* (wave-uniform) U * n_st <= 64 */
    if (lane < MCQ_MTB_POS) s_pos[wv][lane] = mcq_mtb_pos_word(pl, lane < pl.D ? lane : 0u);
    mcq_mtb_load_block(raw + (uint64_t)(first + b) * MCQ_MT_N, s_yb[wv], lane); /* (ends with a wave barrier) */
    const uint32_t u = (lane * ((65536u + n_st - 1u) / n_st)) >> 16, e = lane - u * n_st; /* lane / n_st, lane % n_st (lane < 64) */
    if (u < U) s_ex[wv][u][e] = mcq_mtb_automaton_n(s_yb[wv] + u * W, W, s_pos[wv], pl, e);
    MCQ_WAVE_SYNC();
    if (lane < MCQ_MTB_LANES)
        exits[(uint64_t)(first + b) * MCQ_MTB_LANES + lane] = mcq_mtb_exit_from_parts(&s_ex[wv][0][0], U, pl, lane);
}

// 3. stitch, in two levels (mcq_mt_blocks.hpp).  grp_off[q] .. grp_off[q + 1]: the query's groups of MCQ_MTB_GROUP blocks.
// 3a. compose: one wave per (query, group); the group's exit words through LDS, lane = entry state of the group.
__global__ __launch_bounds__(kMtbBlock) void mcq_mtb_compose_kernel(const mcq_query *__restrict__ queries,
                                                                   const uint32_t *__restrict__ blk_off,
                                                                   const uint32_t *__restrict__ grp_off,
                                                                   const uint32_t *__restrict__ exits,
                                                                   uint32_t *__restrict__ gword, uint32_t *__restrict__ gits) {
    __shared__ __attribute__((aligned(16))) uint32_t s_ex[kMtbBlock / 64][MCQ_MTB_GROUP * MCQ_MTB_LANES];
    const uint32_t qi = blockIdx.y, lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t first = blk_off[qi], nb = blk_off[qi + 1u] - first, g = blockIdx.x * (kMtbBlock / 64) + wv;
    if (g * MCQ_MTB_GROUP >= nb) return; /* (wave-uniform; no block barrier below) */
    const McqMtbPlan pl = mcq_mtb_plan_of(queries, qi);
    const uint32_t b0 = g * MCQ_MTB_GROUP, cnt = nb - b0 < MCQ_MTB_GROUP ? nb - b0 : MCQ_MTB_GROUP;
    const uint4 *src = reinterpret_cast<const uint4 *>(exits + (uint64_t)(first + b0) * MCQ_MTB_LANES);
    for (uint32_t k = lane; k < cnt * (MCQ_MTB_LANES / 4u); k += 64u) reinterpret_cast<uint4 *>(s_ex[wv])[k] = src[k];
    MCQ_WAVE_SYNC();
    McqMtbWalk s = mcq_mtb_walk_from(pl, lane);
    if (lane < pl.D + (pl.two_opp >> 1))
        for (uint32_t k = 0; k < cnt; k++) mcq_mtb_compose_step(s_ex[wv] + k * MCQ_MTB_LANES, pl, s);
    if (lane < MCQ_MTB_LANES) {
        gword[(uint64_t)(grp_off[qi] + g) * MCQ_MTB_LANES + lane] = mcq_mtb_walk_word(s);
        gits[(uint64_t)(grp_off[qi] + g) * MCQ_MTB_LANES + lane] = s.its;
    }
}

// 3b. one wave per query follows the GROUPS' exits, 128 groups' words in LDS at a time; every lane carries the same state
// (the LDS reads are broadcasts).  gentry[group] = the walk in front of the group.  ovf[q] = 1: the stream has not ended
// within the query's blocks -- its row gets passes = UINT64_MAX and the host falls back to the serial walk.
constexpr uint32_t kMtbChunk = 128;
__global__ __launch_bounds__(64) void mcq_mtb_stitch_kernel(const mcq_query *__restrict__ queries,
                                                            const uint32_t *__restrict__ blk_off,
                                                            const uint32_t *__restrict__ grp_off,
                                                            const uint32_t *__restrict__ gword, const uint32_t *__restrict__ gits,
                                                            McqMtbEntry *__restrict__ gentry, uint32_t *__restrict__ ovf,
                                                            mcq_result *__restrict__ res) {
    __shared__ __attribute__((aligned(16))) uint32_t s_w[kMtbChunk * MCQ_MTB_LANES], s_i[kMtbChunk * MCQ_MTB_LANES];
    __shared__ McqMtbEntry s_en[kMtbChunk];
    const uint32_t qi = blockIdx.x, lane = threadIdx.x;
    const uint32_t gfirst = grp_off[qi], ng = grp_off[qi + 1u] - gfirst;
    if (blk_off[qi + 1u] == blk_off[qi]) {
        if (lane == 0) ovf[qi] = 0u;
        return;
    }
    const McqMtbPlan pl = mcq_mtb_plan_of(queries, qi);
    uint32_t d = 0, pend = 0, it = 0;
    for (uint32_t g0 = 0; g0 < ng; g0 += kMtbChunk) {
        const uint32_t cnt = ng - g0 < kMtbChunk ? ng - g0 : kMtbChunk;
        const uint4 *sw = reinterpret_cast<const uint4 *>(gword + (uint64_t)(gfirst + g0) * MCQ_MTB_LANES);
        const uint4 *si = reinterpret_cast<const uint4 *>(gits + (uint64_t)(gfirst + g0) * MCQ_MTB_LANES);
        for (uint32_t k = lane; k < cnt * (MCQ_MTB_LANES / 4u); k += 64u) {
            reinterpret_cast<uint4 *>(s_w)[k] = sw[k];
            reinterpret_cast<uint4 *>(s_i)[k] = si[k];
        }
        MCQ_WAVE_SYNC();
        for (uint32_t k = 0; k < cnt; k++) {
            /* (every lane stores the same words: no branch on the lane number inside the chain) */
            s_en[k].it0 = it;
            s_en[k].dp = d | (pend << 8) | (it < pl.runs ? 0x80000000u : 0u);
            mcq_mtb_stitch_group(s_w + k * MCQ_MTB_LANES, s_i + k * MCQ_MTB_LANES, pl, d, pend, it);
        }
        MCQ_WAVE_SYNC();
        for (uint32_t k = lane; k < cnt; k += 64u) gentry[gfirst + g0 + k] = s_en[k];
        MCQ_WAVE_SYNC();
    }
    if (lane == 0) {
        ovf[qi] = it < pl.runs ? 1u : 0u;
        if (it < pl.runs) reinterpret_cast<unsigned long long *>(res + qi)[1] = ~0ull;
    }
}

// 3c. expand: one wave per (query, group) follows the group's blocks from the group's entry and notes theirs.
__global__ __launch_bounds__(kMtbBlock) void mcq_mtb_expand_kernel(const mcq_query *__restrict__ queries,
                                                                  const uint32_t *__restrict__ blk_off,
                                                                  const uint32_t *__restrict__ grp_off,
                                                                  const uint32_t *__restrict__ exits,
                                                                  const McqMtbEntry *__restrict__ gentry,
                                                                  McqMtbEntry *__restrict__ entries) {
    __shared__ __attribute__((aligned(16))) uint32_t s_ex[kMtbBlock / 64][MCQ_MTB_GROUP * MCQ_MTB_LANES];
    __shared__ McqMtbEntry s_en[kMtbBlock / 64][MCQ_MTB_GROUP];
    const uint32_t qi = blockIdx.y, lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t first = blk_off[qi], nb = blk_off[qi + 1u] - first, g = blockIdx.x * (kMtbBlock / 64) + wv;
    if (g * MCQ_MTB_GROUP >= nb) return; /* (wave-uniform; no block barrier below) */
    const McqMtbPlan pl = mcq_mtb_plan_of(queries, qi);
    const uint32_t b0 = g * MCQ_MTB_GROUP, cnt = nb - b0 < MCQ_MTB_GROUP ? nb - b0 : MCQ_MTB_GROUP;
    const uint4 *src = reinterpret_cast<const uint4 *>(exits + (uint64_t)(first + b0) * MCQ_MTB_LANES);
    for (uint32_t k = lane; k < cnt * (MCQ_MTB_LANES / 4u); k += 64u) reinterpret_cast<uint4 *>(s_ex[wv])[k] = src[k];
    const McqMtbEntry ge = gentry[grp_off[qi] + g];
    uint32_t d = ge.dp & 0xFFu, pend = (ge.dp >> 8) & 0x7Fu, it = ge.it0;
    MCQ_WAVE_SYNC();
    for (uint32_t k = 0; k < cnt; k++) {
        s_en[wv][k].it0 = it;
        s_en[wv][k].dp = d | (pend << 8) | (it < pl.runs ? 0x80000000u : 0u);
        mcq_mtb_stitch_step(s_ex[wv] + k * MCQ_MTB_LANES, pl, d, pend, it);
    }
    MCQ_WAVE_SYNC();
    if (lane < cnt) entries[first + b0 + lane] = s_en[wv][lane];
}

// 4. parse: one wave per (query, block) from the block's true entry (mcq_mtb_parse_block: the batch code of the serial
// walk), draws straight to the draw buffer, the attempts added to the row's `passes`.
__global__ __launch_bounds__(kMtbParseBlock) void mcq_mtb_parse_kernel(const mcq_query *__restrict__ queries,
                                                                 const uint32_t *__restrict__ blk_off,
                                                                 const uint32_t *__restrict__ state,
                                                                 const McqMtbEntry *__restrict__ entries,
                                                                 const uint32_t *__restrict__ ovf, uint8_t *__restrict__ draws,
                                                                 const uint64_t *__restrict__ draw_off, mcq_result *__restrict__ res) {
    __shared__ __attribute__((aligned(16))) McqMtBlockWave ws[kMtbParseBlock / 64];
    __shared__ unsigned long long s_passes[kMtbParseBlock / 64];
    const uint32_t qi = blockIdx.y, lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t first = blk_off[qi], nb = blk_off[qi + 1u] - first, b = blockIdx.x * (kMtbParseBlock / 64) + wv;
    if (blockIdx.x * (kMtbParseBlock / 64) >= nb) return; /* (block-uniform) */
    const bool mine = b < nb;                                         /* (wave-uniform) */
    if (ovf[qi] != 0u) { /* (block-uniform) */
        /* the stream ran past the query's blocks: the host repeats the call with the serial walk; the evaluation kernel
         * behind this one still reads the query's draws -- give it valid ones (index 0), not whatever the buffer held */
        if (!mine) return;
        const uint4 raw = reinterpret_cast<const uint4 *>(queries)[qi];
        const McqQueryWords q = {raw.x, raw.y, raw.z, raw.w};
        const uint64_t bytes = (((uint64_t)q.runs() + 63u) & ~63ull) * (2u * (q.n_players() - 1u) + 5u - q.n_board());
        const uint64_t per = ((bytes + nb - 1u) / nb + 15u) & ~15ull, lo = (uint64_t)b * per, hi = lo + per < bytes ? lo + per : bytes;
        uint4 *dst = reinterpret_cast<uint4 *>(draws + draw_off[qi]);
        for (uint64_t k = lo / 16u + lane; k < hi / 16u; k += 64u) dst[k] = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
        return;
    }
    uint64_t passes = 0;
    if (mine) {
        /* (into scalar registers by hand: the compiler knows that a load at a uniform address is uniform, drops a
         * readfirstlane of it -- and then cannot pin the walk's state in SGPRs where mcq_mt_batch asks for that) */
        const McqMtbEntry en0 = entries[first + b];
        McqMtbEntry en;
        asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(en.it0) : "v"(en0.it0));
        asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(en.dp) : "v"(en0.dp));
        if (en.dp >> 31) { /* (else: the stream ended in an earlier block) */
            McqMtBlockWave &w = ws[wv];
            const uint4 raw = reinterpret_cast<const uint4 *>(queries)[qi];
            const McqQueryWords q = {(uint32_t)__builtin_amdgcn_readfirstlane(raw.x), (uint32_t)__builtin_amdgcn_readfirstlane(raw.y),
                                     (uint32_t)__builtin_amdgcn_readfirstlane(raw.z), (uint32_t)__builtin_amdgcn_readfirstlane(raw.w)};
            const uint32_t L0 = 50u - q.n_board(), n_opp = q.n_players() - 1u, n_deal = 5u - q.n_board(), runs = q.runs();
            mcq_mtb_load_block(state + (uint64_t)(first + b) * MCQ_MT_N, w.yb, lane);
            if (lane == 0) {
                w.draws = draws + draw_off[qi];
                w.stride = ((uint64_t)runs + 63u) & ~63ull;
                w.two_opp = 2u * n_opp;
            }
            mcq_mt_fill_ptab(w, L0, n_opp, 2u * n_opp + n_deal); /* (ends with a wave barrier) */
            passes = mcq_mtb_parse_block(w, L0, n_opp, n_deal, runs, en);
        }
    }
    /* the attempts of the work-group's blocks in ONE atomic: thousands of them on one row's word serialise (14 ns each:
     * 3 900 blocks of a 6-max 100 000-run query 54 us, the whole parse kernel's time) */
    if (lane == 0) s_passes[wv] = passes;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kMtbParseBlock / 64; k++) sum += s_passes[k];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(res + qi) + 1, sum);
    }
}

// ---------------------------------------------------------------------------------------------- multi-GPU helper
// dst[i] += src[i]: adds the tally matrix of a second shard on the same device (mcq_multi.cpp) -- HBM-bound
// streaming, two 16-byte loads and one store per lane.
constexpr uint64_t kAddMaxBlocks = 2048; /* grid cap of the launch: the lanes stride over what is left */
__global__ __launch_bounds__(256) void mcq_add_u64_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src,
                                                          uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n2 = n >> 1;
    ulonglong2 *d2 = reinterpret_cast<ulonglong2 *>(dst);
    const ulonglong2 *s2 = reinterpret_cast<const ulonglong2 *>(src);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        ulonglong2 a = d2[i];
        const ulonglong2 b = s2[i];
        a.x += b.x;
        a.y += b.y;
        d2[i] = a;
    }
    if ((n & 1ull) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] += src[n - 1];
}

// ---------------------------------------------------------------------------------------------- completion
// The end of a kernel whose results the host picks up by polling a flag (every thread of every block calls it, behind
// its last store): ONE system-scope release per block, behind the barrier that orders the other waves' stores before it
// -- a fence in every wave would write the L2 back once per wave -- then the count of finished blocks (`done`: device
// memory, zero before the launch, reset for the next launch on the stream).  Each block counts itself in behind its own
// release, so the one that completes the count has seen every block's results leave: it raises *done_flag (pinned host
// memory) to `ticket`.
__device__ __forceinline__ void mcq_block_done(uint32_t *__restrict__ done, volatile uint32_t *done_flag, uint32_t ticket) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system(); /* this block's results have reached the host's memory */
        bool last = true;
        if (gridDim.x > 1u) {
            last = atomicAdd(done, 1u) + 1u == gridDim.x;
            if (last) *done = 0;
        }
        if (last) *done_flag = ticket;
    }
}

// ---------------------------------------------------------------------------------------------- publish
// Behind the evaluation kernel of a host-buffer call with few rows: moves the finished rows from HBM into pinned
// host memory, leaves the HBM rows zero for the next call and raises a flag the host is polling -- instead of a
// D2H copy, a stream synchronisation (24 us on this pool against 7.5 us for a flag, tools/launch_floor.hip) and a
// memset.  16-byte words; the last block to finish (device counter, reset for the next launch) writes the flag.
constexpr uint64_t kPublishMaxBlocks = 64; /* grid cap of the launch (few rows: every block counts itself in at `done`) */
__global__ __launch_bounds__(256) void mcq_publish_kernel(ulonglong2 *__restrict__ d_rows, ulonglong2 *__restrict__ h_rows,
                                                          uint64_t n_words16, uint32_t *__restrict__ done,
                                                          volatile uint32_t *done_flag, uint32_t ticket) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const ulonglong2 zero = {0ull, 0ull};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words16; i += stride) {
        h_rows[i] = d_rows[i];
        d_rows[i] = zero;
    }
    mcq_block_done(done, done_flag, ticket);
}

// ---------------------------------------------------------------------------------------------- eval
/* The wave tallies (mcq_tally.hpp: lane states, counter-to-word table, lanes -> row step) wired to this wave's reductions --
 * shuffles for a flush in the middle of the work, DPP where the whole wave is active -- and to the row's atomics. */
struct WaveSum {
    __device__ __forceinline__ uint32_t operator()(uint32_t v) const { return wave_sum(v); }
};
struct WaveSumDpp {
    __device__ __forceinline__ uint32_t operator()(uint32_t v) const { return wave_sum_dpp(v); }
};
struct RowAtomicAdd {
    __device__ __forceinline__ void operator()(unsigned long long *word, unsigned long long v) const { atomicAdd(word, v); }
};
template <class State> struct WaveTallyOf : State {
    __device__ __forceinline__ uint64_t row_value(uint32_t lane) const { return State::row_value(lane, WaveSum()); }
    __device__ __forceinline__ uint64_t row_words(uint32_t lane) const { return State::row_words(lane, WaveSumDpp()); }
    /* ... -> one 64-bit atomic per counter that is not zero.  (Written out here and not behind a functor for the atomic,
     * as the per-seat flush is: that form changed the instruction order of the sliced kernels.) */
    template <class Row> __device__ __forceinline__ void flush(Row *row, uint32_t lane) {
        if (!this->dirty) return;
        const uint64_t mine = row_value(lane);
        if (lane < State::kLanes && mine != 0)
            atomicAdd(reinterpret_cast<unsigned long long *>(row) + 1 + lane, (unsigned long long)mine);
        this->clear();
    }
};
typedef WaveTallyOf<McqTally> WaveTally;
typedef WaveTallyOf<McqTallyWays> WaveTallyWays;
struct WaveTallySeats : McqTallySeats {
    __device__ __forceinline__ void add(const McqLaneAccSeats &a, uint32_t lane) { McqTallySeats::add(a, lane, WaveSumDpp()); }
    __device__ __forceinline__ void flush(unsigned long long *row, uint32_t lane) { McqTallySeats::flush(row, lane, RowAtomicAdd()); }
};
/* what a kernel instantiation works with: the lane accumulator, the wave tally, the row's length in 64-bit words and the
 * lanes that hold one word of it each (every word but `runs`).  KIND: MCQ_ROW_PLAIN (0 = false), MCQ_ROW_WAYS (1 = true),
 * MCQ_ROW_SEATS (the extended general path only). */
#define MCQ_ROW_PLAIN 0
#define MCQ_ROW_WAYS 1
#define MCQ_ROW_SEATS 2
template <int KIND> struct McqRowKind {
    typedef McqLaneAcc Acc;
    typedef WaveTally Tally;
    static constexpr uint32_t kWords = Tally::kWords, kLanes = Tally::kLanes;
    static __device__ __forceinline__ mcq_result *row(mcq_result *res, uint32_t i) { return res + i; }
};
template <> struct McqRowKind<MCQ_ROW_WAYS> {
    typedef McqLaneAccWays Acc;
    typedef WaveTallyWays Tally;
    static constexpr uint32_t kWords = Tally::kWords, kLanes = Tally::kLanes;
    static __device__ __forceinline__ unsigned long long *row(mcq_result *res, uint32_t i) {
        return reinterpret_cast<unsigned long long *>(res) + (size_t)i * kWords;
    }
};
template <> struct McqRowKind<MCQ_ROW_SEATS> {
    typedef McqLaneAccSeats Acc;
    typedef WaveTallySeats Tally;
    static constexpr uint32_t kWords = Tally::kWords; /* lanes 0..30 hold words 1..31 */
    static __device__ __forceinline__ unsigned long long *row(mcq_result *res, uint32_t i) {
        return reinterpret_cast<unsigned long long *>(res) + (size_t)i * kWords;
    }
};

template <int MODE, bool SPLIT, bool WAYS>
__global__ __launch_bounds__(kMaxBlock) void mcq_eval_kernel(const mcq_query *__restrict__ queries, uint32_t n,
                                                             const uint64_t *__restrict__ prefix,
                                                             mcq_result *__restrict__ res, uint64_t seed,
                                                             uint64_t first_qid, const McqTables *__restrict__ g_tab,
                                                             const uint8_t *__restrict__ draws,
                                                             const uint64_t *__restrict__ draw_off, uint32_t split_arg,
                                                             uint32_t part, uint32_t n_parts, uint32_t work_wpb) {
    /* SPLIT = false: the bulk path, compiled without the cut */
    const uint32_t split = !SPLIT ? 0u
                           : split_arg == MCQ_SPLIT_FROM_PREP ? (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)prefix[n + 1])
                                                              : split_arg;
    /* split (0..4): small batches cut every 1024-iteration task into 2^split sub-tasks of 16 >> split iterations per
     * lane so that more waves share the work; the iterations and their random numbers stay the same (a sub-task
     * skips ahead in its lane's stream), so the tallies do not depend on it. */
    __shared__ __attribute__((aligned(16))) McqSumImage tab; /* first: the hash is read at constant offsets from LDS address 0 */
    __shared__ McqPair base_tab[2 * kMaxBlock]; /* per wave: the query's ordered remaining deck, 2 x 64 entries x 8 B (kDeckY) */
    __shared__ __attribute__((aligned(8))) char hole_tab[(kMaxBlock / 64) * MCQ_HOLE_WAVE_BYTES]; /* per wave: its cards by suit */
    static_assert(sizeof(McqSumImage) + sizeof(base_tab) + sizeof(hole_tab) + 8u * McqRowKind<MCQ_ROW_WAYS>::kLanes + 8u <= 160u * 1024u &&
                      sizeof(McqSumImage) == 117760u && sizeof(base_tab) == 16384u && sizeof(hole_tab) == 25600u,
                  "image, base decks, hole tables, s_row, s_key and s_done in the 160 KB of a CU");
    /* SPLIT (small batches): the rows the work-group's waves END on are added up in LDS when they are one query's -- a
     * single long query is hundreds of waves, and twelve atomics per wave on ONE row serialise (a 100 000-run query: 392
     * waves, 18 us where the arithmetic takes 6) -- and the last wave sends the sum: s_key = that query (claimed by the
     * first wave to finish), s_done = waves that have finished */
    typedef McqRowKind<WAYS ? MCQ_ROW_WAYS : MCQ_ROW_PLAIN> Row; /* WAYS: 22-word rows with the ties split by the hands that share the pot */
    constexpr uint32_t kLanes = Row::kLanes;
    __shared__ unsigned long long s_row[kLanes];
    __shared__ uint32_t s_key, s_done;
    if (SPLIT) {
        if (threadIdx.x < kLanes) s_row[threadIdx.x] = 0ull;
        if (threadIdx.x == kLanes) {
            s_key = 0xFFFFFFFFu;
            s_done = 0u;
        }
    }
    load_sum_tables(tab, g_tab); /* (ends with a block barrier) */
    const McqSumTabs tabs = {tab.hoff, tab.hrank, g_tab->tfid};

    const uint32_t lane = threadIdx.x & 63u;
    /* Parity mode's split-pot instance sits at the register limit: there a flush forms its row address where it is used
     * (the lane number hidden from the optimiser); kept across the iteration loops it went to scratch. */
    auto flush_lane = [&]() { return WAYS && MODE == MCQ_MODE_REPLAY_MT19937 ? mcq_opaque(lane) : lane; };
    /* small batches launch more waves than take work: the extra ones only help to bring the 115 KB table image in */
    const uint32_t waves_per_block = work_wpb ? work_wpb : blockDim.x >> 6;
    if ((threadIdx.x >> 6) >= waves_per_block) return;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * waves_per_block + (threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * waves_per_block;
    const uint32_t chunk = MCQ_STREAM_ITERS >> split, sub_mask = (1u << split) - 1u;
    const uint64_t total = prefix[n] << split; /* cost axis in sub-task units */
    /* this wave's slice of the cost axis; a task belongs to the slice its start position falls into */
    const uint64_t lo = total * wave / n_waves, hi = total * (wave + 1ull) / n_waves;
    McqPair *base = base_tab + (threadIdx.x & ~63u);
    char *holes = hole_tab + (threadIdx.x >> 6) * MCQ_HOLE_WAVE_BYTES;
    const McqDeckBulk deck = {{base - 128}, holes - (128u << kHoleShift)};

    uint32_t a = 0, b = n; /* last query with prefix <= lo: it has a positive cost because lo < total */
    while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if ((prefix[mid] << split) <= lo) a = mid; else b = mid;
    }
    uint32_t qi = __builtin_amdgcn_readfirstlane(a);
    uint32_t task = 0, task0 = 0, n_tasks = 0, weight = 1; /* tasks [task0, n_tasks) of the query are this launch's */
    uint64_t pfx = 0;
    McqQueryCtx qc;
    typename Row::Tally tally;
    tally.clear();
    bool fresh = true; /* query record qi not loaded yet */
    for (; lo < hi;) { /* (a wave without a slice goes straight to the end: the work-group counts it there) */
        if (fresh) {
            if (qi >= n) break;
            const uint4 raw = reinterpret_cast<const uint4 *>(queries)[qi];
            const McqQueryWords q = {raw.x, raw.y, raw.z, raw.w};
            pfx = prefix[qi] << split;
            const bool ok = (prefix[qi + 1] << split) > pfx; /* zero cost: invalid or runs == 0 */
            const McqPart pt = mcq_part(mcq_task_count(q), q.runs(), part, n_parts);
            task0 = pt.t_lo << split;
            n_tasks = ok ? pt.t_hi << split : 0u;
            weight = mcq_task_weight(q);
            task = task0;
            if (pfx < lo) task = task0 + (uint32_t)((lo - pfx + weight - 1) / weight); /* only for the first query */
            fresh = false;
            if (ok) {
                mcq_query_ctx(q, qc);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); /* earlier lookups are done (same wave) */
                if (lane < 63u) {
                    const McqCard c = mcq_base_entry(qc, lane, tab.sel8);
                    McqDeckBulk::put(base, lane, c);
                    if (lane < MCQ_HOLE_POSITIONS) McqDeckBulk::put_holes(holes, lane, c);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (task >= n_tasks) {
            tally.flush(Row::row(res, qi), flush_lane());
            qi++;
            fresh = true;
            continue;
        }
        if (pfx + (uint64_t)(task - task0) * weight >= hi) break;

        typename Row::Acc acc = {};
        if (MODE != MCQ_MODE_REPLAY_MT19937) {
            const uint32_t stream = (task >> split) * MCQ_WAVE + lane, sub = task & sub_mask;
            const uint64_t it0 = (uint64_t)stream * MCQ_STREAM_ITERS + sub * chunk;
            if (it0 < qc.runs) {
                McqCtrDrawsT<MODE == MCQ_INTERNAL_MODE_UNIFORM> dr;
                dr.start(seed, first_qid + qi, stream);
                /* words per iteration: one per opponent, one per two table cards */
                for (uint32_t k = sub * chunk * (qc.n_opp + ((qc.n_deal + 1u) >> 1)); k != 0; k--) dr.rng.next();
                const uint32_t cnt = (uint32_t)min((uint64_t)chunk, (uint64_t)qc.runs - it0);
                mcq_iterations_sum<true>(qc, dr, deck, tabs, acc, cnt); /* both dealing laws */
                acc.passes = cnt * qc.n_opp; /* MCQ-CTR v5: one attempt per opponent, never re-drawn */
            }
        } else {
            /* a lane takes FOUR consecutive iterations at a time (one 32-bit load per draw row, McqReplayDraws4); a task
             * is four such groups per lane, a sub-task (split <= 2: the host never cuts this mode finer) whole groups */
            const uint64_t stride = (qc.runs + 63u) & ~63ull;
            const uint8_t *dbase = draws + draw_off[qi];
            const uint32_t groups = chunk >> 2;
            for (uint32_t g = (task & sub_mask) * groups, ge = g + groups; g < ge; g++) {
                const uint64_t it4 = (uint64_t)(task >> split) * MCQ_TASK_ITERS + (g * MCQ_WAVE + lane) * 4u;
                if (it4 < qc.runs) {
                    McqReplayDraws4 dr;
                    dr.load(dbase + it4, stride, qc.n_opp, qc.n_deal);
                    const uint32_t cnt4 = (uint32_t)min((uint64_t)4u, (uint64_t)qc.runs - it4);
                    mcq_iterations_replay4(qc, dr, deck, tabs, acc, cnt4);
                }
            }
            acc.passes = 0; /* `passes` comes from the stream walk: mcq_mt_parse_kernel writes it into the row (the host walk
                             * of mcq_eval_batch_numpy_stream patches it in afterwards) */
        }
        tally.add(acc);
        if constexpr (WAYS) {
            if (tally.full()) tally.flush(Row::row(res, qi), flush_lane()); /* its packed counters are about to overflow */
        }
        task++;
    }
    if (!SPLIT) {
        if (qi < n) tally.flush(Row::row(res, qi), flush_lane());
        return;
    }
    const bool have = qi < n && tally.dirty; /* (wave-uniform) */
    if (have) {
        const uint64_t mine = tally.row_value(lane);
        uint32_t key = 0;
        if (lane == 0) key = atomicCAS(&s_key, 0xFFFFFFFFu, qi);
        key = __builtin_amdgcn_readfirstlane(key);
        if (key == 0xFFFFFFFFu || key == qi) {
            if (lane < kLanes && mine != 0) atomicAdd(&s_row[lane], (unsigned long long)mine);
        } else if (lane < kLanes && mine != 0) { /* another query's tail: straight to its row */
            atomicAdd(reinterpret_cast<unsigned long long *>(Row::row(res, qi)) + 1 + lane, (unsigned long long)mine);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); /* the sums are in LDS before this wave counts as finished */
    uint32_t done = 0;
    if (lane == 0) done = atomicAdd(&s_done, 1u);
    done = __builtin_amdgcn_readfirstlane(done);
    if (done + 1u == waves_per_block) { /* the last wave of the work-group */
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        const uint32_t key = *(volatile uint32_t *)&s_key;
        if (key != 0xFFFFFFFFu && lane < kLanes) {
            const unsigned long long v = *(volatile unsigned long long *)&s_row[lane];
            if (v != 0) atomicAdd(reinterpret_cast<unsigned long long *>(Row::row(res, key)) + 1 + lane, v);
        }
    }
}

// ---------------------------------------------------------------------------------------------- eval, small queries
// The reference's own call pattern is thousands of SMALL queries (1000 runs each, gym_env/env.py:22,261-262).  For
// those the cost of a call is not the arithmetic but the launches and copies around it, so this kernel needs
// nothing else: it takes the query records from its own arguments (a launch of up to 128 waves) or straight from the
// library's pinned, device-visible staging memory, every query is owned by ONE block -- 2^split <= 8 waves take the
// 2^split cuts of each of its 1024-iteration tasks -- the waves' sums meet in LDS and one wave stores the finished
// 104-byte row straight into pinned host memory.  No prep kernel, no atomics in HBM, no zeroing, no copy kernels.
// Iterations, random numbers and hence tallies are those of mcq_eval_kernel (same streams, same cut arithmetic).
// The host lays the work out (eval_host_philox in mcq_host.cpp): every query gets a power-of-two number of waves in
// proportion to its cost, so that all waves carry about the same work, and the waves of a query sit side by side in
// one block.  Wave `v` of block `b` in round `r` finds its work at index (r * gridDim.x + b) * 16 + v:
//   work_qi[]   the query's index (its RNG stream key and result row), or MCQ_DIRECT_IDLE
//   work_rec[]  a copy of the 16-byte query record whose reserved bytes carry log2(waves of the query) and this
//               wave's cut number
// -- both read by a few lanes per block, eight rounds at a time, into LDS while the table image travels global -> LDS
// (every wave fetching its own record over PCIe costs more than the arithmetic; from the kernel arguments a wave does
// read its first record itself, by scalar loads, and sets its generator up before the image has landed).  done[0]
// (device memory, zero before the launch, reset by the last block) counts finished blocks of a grid of several; the
// last one raises done_flag (pinned host memory) to `ticket` after a system-scope fence, which lets the host pick the
// rows up without waiting for the end-of-grid handshake.
#define MCQ_DIRECT_STAGE_ROUNDS 8u
#ifdef MCQ_DIRECT_STAMPS /* diagnostic build (tools/direct_stamps.py): 100 MHz timestamps of block 0's waves */
__device__ unsigned long long mcq_direct_stamps[16][16];
#define MCQ_STAMP(k)                                                                                           \
    do {                                                                                                       \
        if (blockIdx.x == 0 && (threadIdx.x & 63u) == 0) mcq_direct_stamps[threadIdx.x >> 6][k] = wall_clock64(); \
    } while (0)
extern "C" __attribute__((visibility("default"))) int mcq_debug_read_stamps(unsigned long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mcq_direct_stamps), sizeof(mcq_direct_stamps));
}
#else
#define MCQ_STAMP(k)
#endif
// Queries resident in HBM (mcq_eval_batch_device_small; use_karg == 2): nobody has laid the work out -- slot `at` IS the
// wave number: every query gets 2^lg waves (the host picks lg from the query COUNT alone), slot at -> query at >> lg, cut
// at & (2^lg - 1); work_rec points at the caller's mcq_query array.  The queries are validated here: one that is invalid
// or has more than MCQ_DIRECT_DEV_TASKS tasks gets runs = 0, passes = UINT64_MAX and no work, one without iterations a
// row of zeros (the slot of its first wave writes it).
#define MCQ_DIRECT_DEV_TASKS 8u
template <uint32_t ROW_WORDS>
__device__ __forceinline__ void mcq_direct_fetch_dev(const uint4 *__restrict__ queries, size_t at, uint32_t n, uint32_t lg,
                                                     mcq_result *__restrict__ res, uint32_t &qi, uint4 &rec) {
    const uint32_t q = (uint32_t)(at >> lg), sub = (uint32_t)at & ((1u << lg) - 1u);
    qi = MCQ_DIRECT_IDLE;
    if (q >= n) return;
    rec = queries[q];
    const McqQueryWords w = {rec.x, rec.y, rec.z, rec.w};
    const bool ok = mcq_query_valid(w) && mcq_task_count(w) <= MCQ_DIRECT_DEV_TASKS;
    if (ok && w.runs() != 0u) {
        qi = q;
        rec.z |= (lg << 8) | (sub << 16); /* reserved[0], reserved[1]: as the host's layout writes them */
    } else if (sub == 0u) {
        unsigned long long *r = reinterpret_cast<unsigned long long *>(res) + (size_t)q * ROW_WORDS;
        r[0] = 0ull;
        r[1] = ok ? 0ull : ~0ull;
#pragma unroll
        for (int k = 2; k < (int)ROW_WORDS; k++) r[k] = 0ull;
    }
}

template <int MODE, bool WAYS>
__global__ __launch_bounds__(kMaxBlock) void mcq_eval_direct_kernel(const uint4 *__restrict__ work_rec,
                                                                    const uint32_t *__restrict__ work_qi, uint32_t rounds,
                                                                    uint32_t merge, mcq_result *__restrict__ res, uint64_t seed,
                                                                    uint64_t first_qid, const McqTables *__restrict__ g_tab,
                                                                    uint32_t *__restrict__ done, volatile uint32_t *done_flag,
                                                                    uint32_t ticket, uint32_t use_karg, McqDirectKarg karg) {
    constexpr uint32_t kWaves = kMaxBlock / 64, kStage = MCQ_DIRECT_STAGE_ROUNDS * kWaves;
    __shared__ __attribute__((aligned(16))) McqSumImage tab; /* first: the hash is read at constant offsets from LDS address 0 */
    __shared__ McqPair base_tab[2 * kMaxBlock]; /* as in mcq_eval_kernel */
    typedef McqRowKind<WAYS ? MCQ_ROW_WAYS : MCQ_ROW_PLAIN> Row; /* WAYS: 22-word rows, tie_ways[9] behind by_type[9] */
    constexpr uint32_t kLanes = Row::kLanes;
    __shared__ unsigned long long partial[2][kWaves][kLanes]; /* [round parity][wave][passes, win, tie, by_type[9](, tie_ways[9])] */
    __shared__ uint4 s_rec[kStage];
    __shared__ uint32_t s_qi[kStage];

    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    McqPair *base = base_tab + (threadIdx.x & ~63u);
    const McqDeckLds deck = {base - 128};
    const McqSumTabs tabs = {tab.hoff, tab.hrank, g_tab->tfid};
    typedef McqCtrDrawsT<MODE == MCQ_INTERNAL_MODE_UNIFORM> Draws;
    /* The start of a one-launch query is a chain of latencies, so they overlap: the first rounds' work is asked for,
     * the table image is sent on its way global -> LDS without passing through registers (global_load_lds_dwordx4:
     * every wave instruction moves 1 KB), and while it travels every wave prepares the generator of its first task
     * (Philox, and for a query cut over several waves the walk to this wave's place in the lane streams).  One
     * barrier then publishes the image and the staged work. */
    MCQ_STAMP(0);
    /* a small launch (its work came with the kernel arguments): this wave's round-0 record by scalar loads from its
     * own copy -- the staged one needs the barrier.  (Not for work in pinned host memory: a small read per wave
     * across PCIe costs more than it hides.) */
    uint32_t qi0 = MCQ_DIRECT_IDLE;
    uint4 raw0 = {0u, 0u, 0u, 0u};
    if (use_karg == 1u) {
        const size_t at0 = (size_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(wib);
        qi0 = karg.qi[at0];
        raw0 = make_uint4(karg.rec[at0][0], karg.rec[at0][1], karg.rec[at0][2], karg.rec[at0][3]);
    }
    uint4 pre_rec = {0u, 0u, 0u, 0u};
    uint32_t pre_qi = MCQ_DIRECT_IDLE;
    if (threadIdx.x < kStage && threadIdx.x / kWaves < rounds) {
        const size_t at = ((size_t)(threadIdx.x / kWaves) * gridDim.x + blockIdx.x) * kWaves + threadIdx.x % kWaves;
        if (use_karg == 1u) {
            pre_qi = karg.qi[at];
            pre_rec = make_uint4(karg.rec[at][0], karg.rec[at][1], karg.rec[at][2], karg.rec[at][3]);
        } else if (use_karg == 2u) {
            mcq_direct_fetch_dev<Row::kWords>(work_rec, at, karg.qi[0], karg.qi[1], res, pre_qi, pre_rec);
        } else {
            pre_qi = work_qi[at];
            pre_rec = work_rec[at];
        }
    }
    {
        typedef const __attribute__((address_space(1))) void *GlobalPtr;
        typedef __attribute__((address_space(3))) void *LdsPtr;
        constexpr uint32_t kChunks = sizeof(McqSumImage) / 1024u; /* hoff, hrank, sel8: 1 KB per wave instruction */
        const char *src = reinterpret_cast<const char *>(&g_tab->sum);
        char *dst = reinterpret_cast<char *>(&tab);
        /* the same number of pieces for every wave (a wave whose last piece would lie behind the image sends the
         * image's last one again: same bytes, same place), so that the count of loads in flight is a constant the
         * compiler can wait against */
        constexpr uint32_t kPer = (kChunks + kWaves - 1u) / kWaves;
        const uint32_t wu = __builtin_amdgcn_readfirstlane(wib);
#pragma unroll
        for (uint32_t k = 0; k < kPer; k++) {
            const uint32_t at = wu + k * kWaves, c = at < kChunks ? at : kChunks - 1u;
            __builtin_amdgcn_global_load_lds((GlobalPtr)(src + c * 1024u + lane * 16u), (LdsPtr)(dst + c * 1024u), 16, 0, 0);
        }
    }
    /* round 0, task 0 of this wave: the lanes that have iterations to run there */
    Draws dr0;
    {
        const uint32_t qi = __builtin_amdgcn_readfirstlane(qi0);
        if (qi != MCQ_DIRECT_IDLE) {
            const uint32_t w2 = __builtin_amdgcn_readfirstlane(raw0.z);
            const uint32_t split = (w2 >> 8) & 0xFFu, sub = (w2 >> 16) & 0xFFu;
            const uint32_t chunk = MCQ_STREAM_ITERS >> split;
            const McqQueryWords q = {(uint32_t)__builtin_amdgcn_readfirstlane(raw0.x), (uint32_t)__builtin_amdgcn_readfirstlane(raw0.y),
                                     w2 & 0xFFu, (uint32_t)__builtin_amdgcn_readfirstlane(raw0.w)};
            McqQueryCtx qc;
            mcq_query_ctx(q, qc);
            if ((uint64_t)lane * MCQ_STREAM_ITERS + sub * chunk < qc.runs) {
                dr0.start(seed, first_qid + qi, lane);
                for (uint32_t k = sub * chunk * (qc.n_opp + ((qc.n_deal + 1u) >> 1)); k != 0; k--) dr0.rng.next();
            }
        }
    }
    MCQ_STAMP(1);
    for (uint32_t g0 = 0; g0 < rounds; g0 += MCQ_DIRECT_STAGE_ROUNDS) {
        if (g0) __syncthreads(); /* the previous rounds' work has been read by every wave */
        else __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0): this wave's pieces of the table image have landed */
        if (threadIdx.x < kStage) {
            if (g0) {
                const uint32_t r = g0 + threadIdx.x / kWaves;
                pre_qi = MCQ_DIRECT_IDLE;
                if (r < rounds) {
                    const size_t at = ((size_t)r * gridDim.x + blockIdx.x) * kWaves + threadIdx.x % kWaves;
                    if (use_karg == 2u) {
                        mcq_direct_fetch_dev<Row::kWords>(work_rec, at, karg.qi[0], karg.qi[1], res, pre_qi, pre_rec);
                    } else {
                        pre_qi = work_qi[at];
                        pre_rec = work_rec[at];
                    }
                }
            }
            s_qi[threadIdx.x] = pre_qi;
            s_rec[threadIdx.x] = pre_rec;
        }
        __syncthreads();
        MCQ_STAMP(2);
        const uint32_t g1 = g0 + MCQ_DIRECT_STAGE_ROUNDS < rounds ? g0 + MCQ_DIRECT_STAGE_ROUNDS : rounds;
        for (uint32_t round = g0; round < g1; round++) {
            const uint32_t at = (round - g0) * kWaves + wib;
            const uint32_t qi = __builtin_amdgcn_readfirstlane(s_qi[at]);
            const bool work = qi != MCQ_DIRECT_IDLE;
            const uint4 raw = s_rec[at];
            const uint32_t w2 = __builtin_amdgcn_readfirstlane(raw.z);
            const uint32_t split = (w2 >> 8) & 0xFFu, sub = (w2 >> 16) & 0xFFu, wpq = 1u << split;
            const uint32_t chunk = MCQ_STREAM_ITERS >> split;
            unsigned long long mine = 0; /* lane k < 12: word k + 1 of the row */
            uint32_t runs = 0;
            if (work) {
                const McqQueryWords q = {(uint32_t)__builtin_amdgcn_readfirstlane(raw.x), (uint32_t)__builtin_amdgcn_readfirstlane(raw.y),
                                         w2 & 0xFFu, (uint32_t)__builtin_amdgcn_readfirstlane(raw.w)};
                McqQueryCtx qc;
                mcq_query_ctx(q, qc);
                runs = qc.runs;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); /* the previous query's lookups are done */
                if (lane < 63u) McqDeckLds::put(base, lane, mcq_base_entry(qc, lane, tab.sel8));
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                MCQ_STAMP(3);
                typename Row::Tally tally;
                tally.clear();
                const uint32_t tasks = mcq_task_count(q);
                for (uint32_t task = 0; task < tasks; task++) {
                    typename Row::Acc acc = {};
                    const uint32_t stream = task * MCQ_WAVE + lane;
                    const uint64_t it0 = (uint64_t)stream * MCQ_STREAM_ITERS + sub * chunk;
                    if (it0 < qc.runs) {
                        Draws dr;
                        if (use_karg == 1u && round == 0u && task == 0u) {
                            dr = dr0; /* prepared while the table image was on its way */
                        } else {
                            dr.start(seed, first_qid + qi, stream);
                            for (uint32_t k = sub * chunk * (qc.n_opp + ((qc.n_deal + 1u) >> 1)); k != 0; k--) dr.rng.next();
                        }
                        MCQ_STAMP(5);
                        const uint32_t cnt = (uint32_t)min((uint64_t)chunk, (uint64_t)qc.runs - it0);
                        for (uint32_t j = 0; j < cnt; j++) mcq_iteration_sum<Draws, -1, -1, typename Row::Acc>(qc, dr, deck, tabs, acc);
                        acc.passes = cnt * qc.n_opp;
                        MCQ_STAMP(6);
                    }
                    tally.add(acc);
                    MCQ_STAMP(7);
                }
                mine = tally.row_words(lane);
            }
            /* Row word w = min(lane, 12): lanes 13..63 repeat lane 12's store (same address, same value) so that no
             * branch on the lane number stands in front of the loop's back edge -- the wave stays whole for the
             * cross-lane steps of the next round. */
            const uint32_t w = lane < kLanes ? lane : kLanes;
            if (!merge) { /* no query of this launch has more than one wave: a wave's sums are the row */
                const unsigned long long up = __shfl(mine, (int)((w + 63u) & 63u), 64); /* every lane takes part */
                if (work) reinterpret_cast<unsigned long long *>(Row::row(res, qi))[w] = w == 0u ? (unsigned long long)runs : up;
                continue;
            }
            if (lane < kLanes) partial[round & 1u][wib][lane] = mine;
            MCQ_STAMP(8);
            __syncthreads(); /* every wave of the block, every round; two buffers: a wave may run one round ahead */
            if (work && sub == 0u) {
                unsigned long long v = runs;
                if (w > 0u) {
                    v = 0;
                    for (uint32_t k = 0; k < wpq; k++) v += partial[round & 1u][wib + k][w - 1u];
                }
                reinterpret_cast<unsigned long long *>(Row::row(res, qi))[w] = v;
            }
            MCQ_STAMP(9);
        }
    }
    /* completion: rows first (ONE system-scope release per block, behind the barrier that orders the other waves'
     * stores before it -- a fence in every wave would write the L2 back 16 times over), then the count; the block
     * that completes the count tells the host */
    __syncthreads();
    MCQ_STAMP(10);
    if (threadIdx.x == 0) {
        __threadfence_system(); /* this block's rows have reached the host's memory */
        MCQ_STAMP(11);
        bool last = true;
        if (gridDim.x > 1u) { /* each block counts itself in behind its own release; the one that completes the
                               * count has therefore seen every block's rows leave */
            last = atomicAdd(done, 1u) + 1u == gridDim.x;
            if (last) *done = 0; /* ready for the next launch on this stream */
        }
        if (last) *done_flag = ticket;
        MCQ_STAMP(12);
    }
}

// ---------------------------------------------------------------------------------------------- extended queries
// SURVEY 8f-2 (ranges, ghost cards, any number of known hands, each two cards or a range): the slicing and tallying
// of the plain path (the cost axis: mcq_axis.hpp), the mask-based iteration of mcq_iteration_ext.  Production mode draws from candidate lists that
// mcq_ext_lists_kernel lays out once per query (mcq_device.hpp).  A range that could not be dealt zeroes the row's
// `runs`.  ROW_WORDS / WAYS: 22-word rows (mcq_result_ways) with the ties split as in the plain kernels; the failed-range
// marker (runs := 0) and the invalid marker (passes = UINT64_MAX) leave zeros in the nine further words.
template <uint32_t ROW_WORDS>
__global__ __launch_bounds__(1024) void mcq_prep_ext_kernel(const mcq_query *__restrict__ q,
                                                            const mcq_query_ext *__restrict__ ext, uint32_t n, int mode,
                                                            mcq_result *__restrict__ res, uint64_t *__restrict__ prefix) {
    mcq_prep_rows<ROW_WORDS>(n, res, prefix, [&](uint32_t i) -> McqPrepRecord {
        const uint4 raw = reinterpret_cast<const uint4 *>(q)[i];
        const McqQueryWords qq = {raw.x, raw.y, raw.z, raw.w};
        const McqExtRec er = {reinterpret_cast<const uint32_t *>(ext + i)};
        const bool ok = mcq_query_ext_valid(qq, er);
        const uint32_t s_iters = ok && mode == MCQ_MODE_PHILOX ? mcq_ext_stream_iters(qq, er) : MCQ_STREAM_ITERS;
        /* (an invalid record is priced as well -- on MCQ_STREAM_ITERS, nothing is read outside the record -- and
         * mcq_prep_rows drops the price: with the guard here the kernel takes two more registers than it did) */
        return {ok, (uint64_t)mcq_ext_task_count(qq, s_iters) * mcq_ext_task_weight(qq, s_iters), qq.runs()};
    });
    if (threadIdx.x == 0) {
        prefix[n + 1] = 0;
        prefix[n + 2] = 0; /* work counter of mcq_mt_parse_ext_kernel */
    }
}

// The candidate lists of the production mode: one block per query; list li of the query = all ordered pairs (a, b) of
// cards of U_li whose class its range allows, in the order of 52 * a + b (the specification's order: the oracle builds
// the same list).  Every thread looks at eleven consecutive candidates; a block scan of the counts puts the survivors
// in order (the steps: mcq_stage.hpp).  cnts[query * lists_stride + li] = the list's length (0 for a query that is
// invalid).  The second launch bound is there to keep the occupancy at five waves per SIMD (96 VGPRs): what a thread holds
// per candidate stays in registers across the lists, and without the bound the compiler takes 100.
constexpr int kListBlock = 256;
__global__ __launch_bounds__(kListBlock, 5) void mcq_ext_lists_kernel(const mcq_query *__restrict__ q,
                                                                   const mcq_query_ext *__restrict__ ext, uint32_t lists_stride,
                                                                   uint16_t *__restrict__ lists, uint32_t *__restrict__ cnts) {
    __shared__ uint32_t wave_tot[kListBlock / 64];
    const uint32_t qi = blockIdx.x, tid = threadIdx.x;
    const uint4 raw = reinterpret_cast<const uint4 *>(q)[qi];
    const McqQueryWords qq = {raw.x, raw.y, raw.z, raw.w};
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(ext + qi)};
    const bool valid = mcq_query_ext_valid(qq, er);
    const uint32_t n_lists = valid ? mcq_ext_n_lists(qq, er) : 0u;
    for (uint32_t li = 0; li < lists_stride; li++) {
        if (li >= n_lists) { /* block-uniform */
            if (tid == 0) cnts[(size_t)qi * lists_stride + li] = 0;
            continue;
        }
        uint64_t U;
        uint32_t set_off;
        mcq_ext_list_plan(qq, er, li, U, set_off);
        constexpr uint32_t kPer = (2704u + kListBlock - 1) / kListBlock; /* 11 */
        const uint32_t mask = mcq_ext_list_mask<kPer>(U, er.w + set_off, tid);
        uint32_t total;
        const uint32_t at = block_exclusive_scan<uint32_t, kListBlock / 64>((uint32_t)__popc(mask), wave_tot, &total);
        mcq_ext_list_scatter<kPer>(mask, tid, at, lists + ((size_t)qi * lists_stride + li) * MCQ_EXT_LIST_STRIDE);
        if (tid == 0) cnts[(size_t)qi * lists_stride + li] = total;
    }
}

template <int MODE, int ROW>
__global__ __launch_bounds__(kExtBlock) void mcq_eval_ext_kernel(const mcq_query *__restrict__ queries,
                                                                 const mcq_query_ext *__restrict__ ext, uint32_t n,
                                                                 const uint64_t *__restrict__ prefix,
                                                                 mcq_result *__restrict__ res, uint64_t seed,
                                                                 uint64_t first_qid, const McqTables *__restrict__ g_tab,
                                                                 const uint8_t *__restrict__ draws,
                                                                 const uint64_t *__restrict__ draw_off,
                                                                 const uint16_t *__restrict__ lists,
                                                                 const uint32_t *__restrict__ cnts, uint32_t lists_stride) {
    typedef McqRowKind<ROW> Row; /* MCQ_ROW_WAYS: 22-word rows with the ties split by the hands that share the pot;
                                    MCQ_ROW_SEATS: 32-word rows, every hand's win, tie and share (production mode only) */
    typedef typename Row::Acc Acc;
    constexpr bool SEATS = ROW == MCQ_ROW_SEATS;
    static_assert(!SEATS || MODE == MCQ_MODE_PHILOX, "the per-seat rows have no parity form");
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab;
    __shared__ McqCard cards[64];
    __shared__ McqExtWaveCtx wave_ctx[kExtBlock / 64];
    __shared__ uint16_t ids[(MCQ_MAX_OPP + 1) * kExtBlock];
    /* The candidate lists of the production mode are read once per trial at a random index: from HBM that is a
     * dependent ~700-cycle load per trial, several per opponent, and it -- not the arithmetic -- bounded the kernel
     * (34 000 cycles per wave-iteration at the top quarter of the classes).  So a block first brings the lists of ITS
     * queries -- a block's waves cover a contiguous piece of the cost axis, hence consecutive queries -- into LDS when
     * they fit (36 KB beside the tables; 2 B per ordered card pair), and the trials read them there. */
    __shared__ __attribute__((aligned(16))) uint16_t s_lists[MCQ_EXT_STAGE_ENTRIES];
    __shared__ uint32_t s_list_off[MCQ_EXT_STAGE_LISTS + 1];
    __shared__ uint32_t s_stage[3]; /* first query, number of queries, staged? */
    if (threadIdx.x < 64) cards[threadIdx.x] = mcq_card(threadIdx.x < 52 ? threadIdx.x : 0u);
    load_tables(tab, g_tab);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * waves_per_block + (threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * waves_per_block;
    const uint64_t total = prefix[n];
    const McqAxisSlice slice = mcq_axis_slice(total, wave, n_waves);
    const uint64_t lo = slice.lo, hi = slice.hi;
    if (MODE == MCQ_MODE_PHILOX) {
        if (threadIdx.x == 0) { /* the block's queries: those whose cost interval meets the block's piece of the axis */
            const McqAxisRecords mine = mcq_axis_block_records(prefix, n, blockIdx.x, waves_per_block, gridDim.x);
            const uint32_t qa = mine.first, nq = mine.count;
            const uint32_t staged = mcq_ext_stage_lists(qa, nq, lists_stride, cnts, s_list_off) ? 1u : 0u;
            s_stage[0] = qa;
            s_stage[1] = nq;
            s_stage[2] = staged;
        }
        __syncthreads();
        if (s_stage[2]) {
            const uint32_t qa = s_stage[0], n_l = s_stage[1] * lists_stride;
            for (uint32_t k = 0; k < n_l; k++) { /* (block-uniform loop; 1024 threads copy 4 KB in one step) */
                const uint32_t off = s_list_off[k], words = (s_list_off[k + 1] - off) >> 1;
                const uint32_t *src = reinterpret_cast<const uint32_t *>(lists + ((size_t)qa * lists_stride + k) * MCQ_EXT_LIST_STRIDE);
                uint32_t *dst = reinterpret_cast<uint32_t *>(s_lists + off);
                for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) dst[w] = src[w];
            }
        }
        __syncthreads();
    }
    if (lo >= hi) return;
    McqExtWaveCtx &wc = wave_ctx[threadIdx.x >> 6];
    uint16_t *my_ids = ids + threadIdx.x;

    uint32_t qi = __builtin_amdgcn_readfirstlane(mcq_axis_last_le(prefix, n, lo)); /* it has a cost: lo < total */
    uint32_t task = 0, n_tasks = 0, weight = 1, s_iters = MCQ_STREAM_ITERS;
    uint64_t pfx = 0;
    McqExtCtx qc;
    typename Row::Tally tally;
    tally.clear();
    bool failed = false, fresh = true, list_in_lds = false;
    for (;;) {
        if (fresh) {
            if (qi >= n) break;
            const uint4 raw = reinterpret_cast<const uint4 *>(queries)[qi];
            const McqQueryWords q = {raw.x, raw.y, raw.z, raw.w};
            pfx = prefix[qi];
            bool ok = prefix[qi + 1] > pfx;
            const McqExtRec er = {reinterpret_cast<const uint32_t *>(ext + qi)};
            s_iters = ok && MODE == MCQ_MODE_PHILOX ? mcq_ext_stream_iters(q, er) : MCQ_STREAM_ITERS;
            weight = mcq_ext_task_weight(q, s_iters);
            task = mcq_axis_first_task(pfx, lo, weight); /* (not 0 only for the wave's first record) */
            fresh = false;
            if (ok) {
                mcq_ext_ctx(q, er, qc);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (lane < 10u) wc.hand[lane] = lane < qc.n_hands ? mcq_ext_hand(q, er, lane) : 0u;
                if (MODE == MCQ_MODE_PHILOX) {
                    const uint32_t n_lists = mcq_ext_n_lists(q, er);
                    list_in_lds = __builtin_amdgcn_readfirstlane(s_stage[2] && qi - s_stage[0] < s_stage[1] ? 1 : 0) != 0;
                    uint32_t c = 1;
                    if (lane < MCQ_EXT_MAX_LISTS) {
                        c = lane < n_lists ? cnts[(size_t)qi * lists_stride + lane] : 1u;
                        wc.cnt[lane] = c;
                        const uint16_t *lp = lists + ((size_t)qi * lists_stride + (lane < lists_stride ? lane : 0u)) * MCQ_EXT_LIST_STRIDE;
                        if (s_stage[2] && qi - s_stage[0] < s_stage[1] && lane < lists_stride)
                            lp = s_lists + s_list_off[(qi - s_stage[0]) * lists_stride + lane];
                        wc.list[lane] = lp;
                    }
                    if (__any(c == 0u)) { /* a range no pair of cards can satisfy: nothing to deal from */
                        failed = true;
                        ok = false;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            n_tasks = ok ? mcq_ext_task_count(q, s_iters) : 0u;
        }
        if (task >= n_tasks) {
            if (__any(failed)) {
                if (lane == 0) atomicExch(reinterpret_cast<unsigned long long *>(Row::row(res, qi)), 0ull); /* runs := 0 */
                failed = false;
            }
            tally.flush(Row::row(res, qi), lane);
            qi++;
            fresh = true;
            continue;
        }
        if (!mcq_axis_owns(pfx, task, weight, hi)) break; /* the task belongs to a later slice */

        Acc acc = {};
        if (MODE == MCQ_MODE_PHILOX) {
            const uint32_t stream = task * MCQ_WAVE + lane;
            const uint64_t it0 = (uint64_t)stream * s_iters;
            if (it0 < qc.runs) {
                McqExtCtrDraws dr;
                dr.start(seed, first_qid + qi, stream);
                const uint32_t cnt = (uint32_t)min((uint64_t)s_iters, (uint64_t)qc.runs - it0);
                if constexpr (SEATS) { /* the general form only: the same draws and hands as the other rows' two forms */
                    if (list_in_lds)
                        for (uint32_t j = 0; j < cnt && !failed; j++)
                            failed = !mcq_iteration_ext<McqExtCtrDraws, true, Acc>(qc, wc, dr, cards, tab.sel8, my_ids, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
                    else
                        for (uint32_t j = 0; j < cnt && !failed; j++)
                            failed = !mcq_iteration_ext<McqExtCtrDraws, false, Acc>(qc, wc, dr, cards, tab.sel8, my_ids, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
                } else if (qc.fast && list_in_lds) /* (wave-uniform) */
                    for (uint32_t j = 0; j < cnt && !failed; j++)
                        failed = !mcq_iteration_ext_fast<McqExtCtrDraws, true, true, Acc>(qc, wc, dr, cards, tab.sel8, g_tab->tf, tab.tops, tab.sd, acc);
                else if (qc.fast)
                    for (uint32_t j = 0; j < cnt && !failed; j++)
                        failed = !mcq_iteration_ext_fast<McqExtCtrDraws, true, false, Acc>(qc, wc, dr, cards, tab.sel8, g_tab->tf, tab.tops, tab.sd, acc);
                else if (list_in_lds)
                    for (uint32_t j = 0; j < cnt && !failed; j++)
                        failed = !mcq_iteration_ext<McqExtCtrDraws, true, Acc>(qc, wc, dr, cards, tab.sel8, my_ids, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
                else
                    for (uint32_t j = 0; j < cnt && !failed; j++)
                        failed = !mcq_iteration_ext<McqExtCtrDraws, false, Acc>(qc, wc, dr, cards, tab.sel8, my_ids, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
            }
        } else if constexpr (!SEATS) {
            const uint64_t stride = (qc.runs + 63u) & ~63ull;
            const uint8_t *dbase = draws + draw_off[qi];
            for (uint32_t j = 0; j < MCQ_STREAM_ITERS; j++) {
                const uint64_t it = (uint64_t)task * MCQ_TASK_ITERS + j * MCQ_WAVE + lane;
                if (it < qc.runs) {
                    McqExtReplayDraws dr = {dbase + it, stride};
                    mcq_iteration_ext<McqExtReplayDraws, false, Acc>(qc, wc, dr, cards, tab.sel8, my_ids, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
                }
            }
            acc.passes = 0;
        }
        if constexpr (SEATS) tally.add(acc, lane);
        else tally.add(acc);
        if constexpr (ROW == MCQ_ROW_WAYS) {
            if (tally.full()) tally.flush(Row::row(res, qi), lane); /* its packed counters are about to overflow */
        }
        task++;
    }
    if (qi < n) {
        if (__any(failed) && lane == 0) atomicExch(reinterpret_cast<unsigned long long *>(Row::row(res, qi)), 0ull);
        tally.flush(Row::row(res, qi), lane);
    }
}

// ---------------------------------------------------------------------------------------------- a weighted range per seat
// mcq_eval_batch_ranges: the law, the word -> hand mapping and the lane code are in mcq_ranges.hpp.
// Preparation, one block per DISTINCT table: the 1326 inclusive prefix sums of its weights (six consecutive hands per
// thread, a block scan of the threads' sums), the last of them the total, and behind them the number of non-zero entries
// and the index of the last one (a table with one entry is a known hand, see mcq_ranges.hpp).  Nothing
// here depends on a record -- the table cards are handled by the per-seat re-draw -- so device memory is 5.3 KB per
// table, not per record and seat.
constexpr int kRgTabBlock = 256;
__global__ __launch_bounds__(kRgTabBlock) void mcq_ranges_tables_kernel(const uint16_t *__restrict__ tables,
                                                                        uint32_t *__restrict__ cum) {
    __shared__ uint32_t wave_tot[kRgTabBlock / 64];
    __shared__ uint32_t s_nnz, s_last;
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t kPer = (MCQ_HAND_ROWS + kRgTabBlock - 1) / kRgTabBlock; /* 6 */
    const uint16_t *src = tables + (size_t)blockIdx.x * MCQ_HAND_ROWS;
    uint32_t v[kPer], mine = 0, nnz = 0, last = 0;
    if (tid == 0) s_nnz = s_last = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
        const uint32_t i = tid * kPer + k;
        v[k] = i < MCQ_HAND_ROWS ? (uint32_t)src[i] : 0u;
        mine += v[k];
        nnz += v[k] != 0u ? 1u : 0u;
        last = v[k] != 0u ? i : last;
    }
    __syncthreads();
    if (nnz) { /* the known-hand form of a table: how many entries are not zero, and the last of them */
        atomicAdd(&s_nnz, nnz);
        atomicMax(&s_last, last);
    }
    uint32_t total; /* not used: the last hand's inclusive sum, stored by the loop below, is the table's total */
    uint32_t at = block_exclusive_scan<uint32_t, kRgTabBlock / 64>(mine, wave_tot, &total);
    uint32_t *dst = cum + (size_t)blockIdx.x * MCQ_RG_CUM_STRIDE;
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
        const uint32_t i = tid * kPer + k;
        at += v[k];
        if (i < MCQ_HAND_ROWS) dst[i] = at;
    }
    if (tid == 0) { /* (behind the scan's barriers: every thread's atomics have landed) */
        dst[MCQ_RG_NNZ_WORD] = s_nnz;
        dst[MCQ_RG_LAST_WORD] = s_last;
    }
}

/* rows and cost prefix of the records (mcq_prep_rows; nothing is written behind prefix[n]); a task costs its price by
 * seats and street times trials[i], the host's estimate of the record's whole trials per iteration */
__global__ __launch_bounds__(1024) void mcq_prep_ranges_kernel(const mcq_query *__restrict__ q, const uint32_t *__restrict__ trials,
                                                               uint32_t n, mcq_result *__restrict__ res,
                                                               uint64_t *__restrict__ prefix) {
    mcq_prep_rows<McqRowKind<MCQ_ROW_SEATS>::kWords>(n, res, prefix, [&](uint32_t i) -> McqPrepRecord {
        const uint4 raw = reinterpret_cast<const uint4 *>(q)[i];
        const McqQueryWords qq = {raw.x, raw.y, raw.z, raw.w};
        const bool ok = mcq_ranges_query_valid(qq);
        return {ok, ok ? (uint64_t)mcq_ranges_task_count(qq) * (mcq_ranges_task_weight(qq) * trials[i]) : 0ull, qq.runs()};
    });
}

// The evaluation: waves over the cost axis (the rule and the arithmetic of mcq_axis.hpp, written out here as
// mcq_eval_ext_kernel had it: through the header's calls this kernel came out 0.65 % slower, profiles/axis_walk_ab.txt),
// sixteen-iteration streams of mcq_iteration_ranges, the per-seat wave tally and its flush.  A draw is one dependent chain, word -> t ->
// eleven steps of a binary search in the seat's prepared table -> hand -> test, so where the table lies decides the
// kernel: a block first brings the prepared tables that ITS records name (a block's waves cover a contiguous piece of
// the cost axis, hence consecutive records) into LDS when there are at most MCQ_RG_STAGE_TABLES distinct ones among at
// most MCQ_RG_STAGE_QUERIES records (32 KB beside the evaluator's tables and the hands' card ids: 152 KB in all, one
// block per CU as for the other evaluation kernels), and the draws read them there with 32-bit LDS addresses; otherwise
// they read them from HBM.  Lanes whose trial is accepted wait for the rest of the wave.  A record without an accepted
// trial zeroes the row's `runs`.
__global__ __launch_bounds__(kExtBlock) void mcq_eval_ranges_kernel(const mcq_query *__restrict__ queries,
                                                                    const uint32_t *__restrict__ seat_table,
                                                                    const uint32_t *__restrict__ cum,
                                                                    const uint32_t *__restrict__ trials, uint32_t n,
                                                                    const uint64_t *__restrict__ prefix,
                                                                    mcq_result *__restrict__ res, uint64_t seed,
                                                                    uint64_t first_qid, const McqTables *__restrict__ g_tab) {
    typedef McqRowKind<MCQ_ROW_SEATS> Row;
    typedef typename Row::Acc Acc;
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab;
    __shared__ McqCard cards[64];
    __shared__ McqRangesWaveCtx wave_ctx[kExtBlock / 64];
    __shared__ uint16_t ids[MCQ_MAX_SEATS * kExtBlock];
    __shared__ __attribute__((aligned(16))) uint32_t s_cum[MCQ_RG_STAGE_TABLES * MCQ_RG_CUM_STRIDE];
    __shared__ uint32_t s_tab_id[MCQ_RG_STAGE_TABLES];
    __shared__ uint32_t s_stage[3]; /* first record, number of records, staged tables (0: nothing staged) */
    if (threadIdx.x < 64) cards[threadIdx.x] = mcq_card(threadIdx.x < 52 ? threadIdx.x : 0u);
    load_tables(tab, g_tab);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * waves_per_block + (threadIdx.x >> 6));
    const uint64_t n_waves = (uint64_t)gridDim.x * waves_per_block;
    const uint64_t total = prefix[n];
    const uint64_t lo = total * wave / n_waves, hi = total * (wave + 1ull) / n_waves;
    if (threadIdx.x == 0) { /* the block's records: those whose cost interval meets the block's piece of the axis
                             * (mcq_axis_block_records written out: profiles/block_steps_ab.txt) */
        const uint64_t blo = total * ((uint64_t)blockIdx.x * waves_per_block) / n_waves;
        const uint64_t bhi = total * ((uint64_t)(blockIdx.x + 1u) * waves_per_block) / n_waves;
        uint32_t qa = 0, nq = 0, n_tab = 0;
        if (blo < bhi) {
            uint32_t a = 0, b = n;
            while (b - a > 1) {
                const uint32_t mid = (a + b) >> 1;
                if (prefix[mid] <= blo) a = mid; else b = mid;
            }
            qa = a;
            b = n;
            while (b - a > 1) { /* last record that starts before the block's end */
                const uint32_t mid = (a + b) >> 1;
                if (prefix[mid] < bhi) a = mid; else b = mid;
            }
            nq = a - qa + 1u;
            n_tab = mcq_ranges_stage_tables(reinterpret_cast<const uint32_t *>(queries), seat_table, cum, qa, nq, s_tab_id);
        }
        s_stage[0] = qa;
        s_stage[1] = nq;
        s_stage[2] = n_tab;
    }
    __syncthreads();
    {
        const uint32_t words = s_stage[2] * MCQ_RG_CUM_STRIDE; /* (at most MCQ_RG_STAGE_TABLES tables: inside s_cum) */
        for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
            const uint32_t k = w / MCQ_RG_CUM_STRIDE;
            s_cum[w] = cum[(size_t)s_tab_id[k] * MCQ_RG_CUM_STRIDE + (w - k * MCQ_RG_CUM_STRIDE)];
        }
    }
    __syncthreads();
    if (lo >= hi) return;
    McqRangesWaveCtx &wc = wave_ctx[threadIdx.x >> 6];
    uint16_t *my_ids = ids + threadIdx.x;

    uint32_t a = 0, b = n;
    while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if (prefix[mid] <= lo) a = mid; else b = mid;
    }
    uint32_t qi = __builtin_amdgcn_readfirstlane(a);
    uint32_t task = 0, n_tasks = 0, weight = 1;
    uint64_t pfx = 0;
    McqRangesCtx qc;
    typename Row::Tally tally;
    tally.clear();
    bool failed = false, fresh = true, tab_in_lds = false;
    for (;;) {
        if (fresh) {
            if (qi >= n) break;
            const uint4 raw = reinterpret_cast<const uint4 *>(queries)[qi];
            const McqQueryWords q = {raw.x, raw.y, raw.z, raw.w};
            pfx = prefix[qi];
            const bool ok = prefix[qi + 1] > pfx;
            weight = mcq_ranges_task_weight(q) * trials[qi]; /* (as mcq_prep_ranges_kernel priced it) */
            task = 0;
            if (pfx < lo) task = (uint32_t)((lo - pfx + weight - 1) / weight);
            fresh = false;
            if (ok) {
                mcq_ranges_ctx(q, qc);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                const uint32_t n_staged = s_stage[2];
                tab_in_lds = __builtin_amdgcn_readfirstlane(n_staged != 0u && qi - s_stage[0] < s_stage[1] ? 1 : 0) != 0;
                if (lane < MCQ_MAX_SEATS) { /* (entries at or above n_players are not read: they may name anything) */
                    const uint32_t t = seat_table[(size_t)qi * MCQ_MAX_SEATS + (lane < qc.n_players ? lane : 0u)];
                    const uint32_t *cp = cum + (size_t)t * MCQ_RG_CUM_STRIDE;
                    const uint32_t tot = mcq_ranges_seat_total(cp);
                    wc.total[lane] = tot;
                    if (tab_in_lds && !(tot & MCQ_RG_KNOWN)) { /* every table of a staged record is among the staged ones */
                        cp = s_cum + mcq_ranges_stage_slot(s_tab_id, n_staged, t) * MCQ_RG_CUM_STRIDE;
                    }
                    wc.cum[lane] = cp;
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            n_tasks = ok ? mcq_ranges_task_count(q) : 0u;
        }
        if (task >= n_tasks) {
            if (__any(failed)) {
                if (lane == 0) atomicExch(reinterpret_cast<unsigned long long *>(Row::row(res, qi)), 0ull); /* runs := 0 */
                failed = false;
            }
            tally.flush(Row::row(res, qi), lane);
            qi++;
            fresh = true;
            continue;
        }
        if (pfx + (uint64_t)task * weight >= hi) break;

        Acc acc = {};
        const uint32_t stream = task * MCQ_WAVE + lane;
        const uint64_t it0 = (uint64_t)stream * MCQ_STREAM_ITERS;
        if (it0 < qc.runs) {
            McqExtCtrDraws dr;
            dr.start(seed, first_qid + qi, stream);
            const uint32_t cnt = (uint32_t)min((uint64_t)MCQ_STREAM_ITERS, (uint64_t)qc.runs - it0);
            if (tab_in_lds) /* (wave-uniform) */
                for (uint32_t j = 0; j < cnt && !failed; j++)
                    failed = !mcq_iteration_ranges<McqExtCtrDraws, true, Acc>(qc, wc, dr, cards, tab.sel8, my_ids, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
            else
                for (uint32_t j = 0; j < cnt && !failed; j++)
                    failed = !mcq_iteration_ranges<McqExtCtrDraws, false, Acc>(qc, wc, dr, cards, tab.sel8, my_ids, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
        }
        tally.add(acc, lane);
        task++;
    }
    if (qi < n) {
        if (__any(failed) && lane == 0) atomicExch(reinterpret_cast<unsigned long long *>(Row::row(res, qi)), 0ull);
        tally.flush(Row::row(res, qi), lane);
    }
}

// mcq_eval_batch_ranges_hands: the same records, streams and per-seat rows, and beside them the watched seat's tally PER
// HAND (mcq_hands.hpp).  The kernel above lets every wave walk its own piece of the cost axis, so the waves of a block may
// be on different records at once; a table keyed by hand alone needs the whole block on ONE record.  So the axis is cut per
// BLOCK here -- block b owns [total b / grid, total (b + 1) / grid) -- and the block walks its records one after the other,
// the tasks of a record's piece going to the waves in rounds (task = first + round * waves + wave).  The cut only decides
// which block runs which task: the tasks of a record are numbered as above, so the rows are those of the kernel above.
// Every accepted iteration adds the watched seat's hand to the block's table in LDS (one LDS atomic, three when the seat is
// level with the best); at the end of a record's piece, and every MCQ_HT_FLUSH_ROUNDS rounds within it (a uint32 word holds
// 104 rounds of shares), the block meets, every thread adds its non-zero words to the record's rows in HBM with 64-bit
// atomics -- other blocks hold other pieces of the record -- and clears them, and the block meets again.  No global atomic
// per lane and iteration: a one-hot watched seat would put a thousand lanes on one address.
// Barriers: each sits under conditions computed from blockIdx, the prefix and the round counter alone -- never under a
// lane's or a wave's progress (`failed`, a stream's iteration count, a wave without a task in its last round).  Between two
// flushes the waves do not meet: a wave may run ahead of the others, but by no more than the rounds between two flushes.
// LDS: the evaluator's tables 97 KB, the hands' card ids 20 KB, the table of hands 21 KB, which leaves room for
// MCQ_RG_HANDS_STAGE_TABLES = 3 staged tables (16 KB) instead of six: 156 KB of 160.  Records that name more read them
// from HBM, the form the kernel above has as well.
struct LdsHandAdd { /* table[word] += v in LDS, nothing returned */
    __attribute__((address_space(3))) uint32_t *table;
    __device__ __forceinline__ void operator()(uint32_t word, uint32_t v) const {
        __hip_atomic_fetch_add(table + word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};
__global__ __launch_bounds__(kExtBlock) void mcq_eval_ranges_hands_kernel(const mcq_query *__restrict__ queries,
                                                                          const uint32_t *__restrict__ seat_table,
                                                                          const uint32_t *__restrict__ cum,
                                                                          const uint32_t *__restrict__ trials, uint32_t n,
                                                                          const uint64_t *__restrict__ prefix,
                                                                          mcq_result *__restrict__ res,
                                                                          unsigned long long *__restrict__ hand_rows,
                                                                          uint32_t seat, uint64_t seed, uint64_t first_qid,
                                                                          const McqTables *__restrict__ g_tab) {
    typedef McqRowKind<MCQ_ROW_SEATS> Row;
    typedef McqLaneAccSeatsHands<LdsHandAdd> Acc;
    static_assert(kExtBlock / 64 == MCQ_HT_BLOCK_WAVES, "the flush bound counts a round of sixteen waves");
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab;
    __shared__ McqCard cards[64];
    __shared__ McqRangesWaveCtx wave_ctx[kExtBlock / 64];
    __shared__ uint16_t ids[MCQ_MAX_SEATS * kExtBlock];
    __shared__ __attribute__((aligned(16))) uint32_t s_cum[MCQ_RG_HANDS_STAGE_TABLES * MCQ_RG_CUM_STRIDE];
    __shared__ uint32_t s_tab_id[MCQ_RG_HANDS_STAGE_TABLES];
    __shared__ uint32_t s_stage[3]; /* first record, number of records, staged tables (0: nothing staged) */
    __shared__ uint32_t s_hands[MCQ_HT_TABLE_WORDS];
    if (threadIdx.x < 64) cards[threadIdx.x] = mcq_card(threadIdx.x < 52 ? threadIdx.x : 0u);
    for (uint32_t w = threadIdx.x; w < MCQ_HT_TABLE_WORDS; w += blockDim.x) s_hands[w] = 0u;
    load_tables(tab, g_tab);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = blockDim.x >> 6;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t total = prefix[n];
    const uint64_t blo = total * blockIdx.x / gridDim.x, bhi = total * (blockIdx.x + 1ull) / gridDim.x; /* the BLOCK's piece */
    if (threadIdx.x == 0) { /* the block's records, as above, and which of their tables it stages */
        uint32_t qa = 0, nq = 0, n_tab = 0;
        if (blo < bhi) {
            uint32_t a = 0, b = n;
            while (b - a > 1) {
                const uint32_t mid = (a + b) >> 1;
                if (prefix[mid] <= blo) a = mid; else b = mid;
            }
            qa = a;
            b = n;
            while (b - a > 1) { /* last record that starts before the block's end */
                const uint32_t mid = (a + b) >> 1;
                if (prefix[mid] < bhi) a = mid; else b = mid;
            }
            nq = a - qa + 1u;
            n_tab = mcq_ranges_stage_tables<MCQ_RG_HANDS_STAGE_TABLES>(reinterpret_cast<const uint32_t *>(queries), seat_table, cum,
                                                                       qa, nq, s_tab_id);
        }
        s_stage[0] = qa;
        s_stage[1] = nq;
        s_stage[2] = n_tab;
    }
    __syncthreads();
    {
        const uint32_t words = s_stage[2] * MCQ_RG_CUM_STRIDE; /* (at most MCQ_RG_HANDS_STAGE_TABLES tables: inside s_cum) */
        for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
            const uint32_t k = w / MCQ_RG_CUM_STRIDE;
            s_cum[w] = cum[(size_t)s_tab_id[k] * MCQ_RG_CUM_STRIDE + (w - k * MCQ_RG_CUM_STRIDE)];
        }
    }
    __syncthreads();
    McqRangesWaveCtx &wc = wave_ctx[threadIdx.x >> 6];
    uint16_t *my_ids = ids + threadIdx.x;
    const uint32_t q_first = __builtin_amdgcn_readfirstlane(s_stage[0]);
    const uint32_t q_end = q_first + __builtin_amdgcn_readfirstlane(s_stage[1]); /* (no record: the loop does not run) */
    const uint32_t n_staged = __builtin_amdgcn_readfirstlane(s_stage[2]);
    const bool tab_in_lds = n_staged != 0u; /* every table of the block's records is staged, or none */
    typename Row::Tally tally;
    tally.clear();
    /* block-uniform from here to the end: qi, the piece, the rounds and `since` come from the prefix and blockIdx alone */
    for (uint32_t qi = q_first; qi < q_end; qi++) {
        const uint4 raw = reinterpret_cast<const uint4 *>(queries)[qi];
        const McqQueryWords q = {raw.x, raw.y, raw.z, raw.w};
        const uint64_t pfx = prefix[qi];
        const bool ok = prefix[qi + 1] > pfx;
        const uint32_t weight = mcq_ranges_task_weight(q) * trials[qi]; /* (as mcq_prep_ranges_kernel priced it) */
        McqHandsPiece piece = mcq_hands_piece(pfx, weight, ok ? mcq_ranges_task_count(q) : 0u, blo, bhi);
        piece.first = __builtin_amdgcn_readfirstlane(piece.first);
        piece.end = __builtin_amdgcn_readfirstlane(piece.end);
        const uint32_t rounds = __builtin_amdgcn_readfirstlane(mcq_hands_rounds(piece, waves));
        if (rounds == 0u) continue; /* (nothing added: the table is clear, no barrier is owed) */
        McqRangesCtx qc;
        mcq_ranges_ctx(q, qc);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < MCQ_MAX_SEATS) { /* (entries at or above n_players are not read: they may name anything) */
            const uint32_t t = seat_table[(size_t)qi * MCQ_MAX_SEATS + (lane < qc.n_players ? lane : 0u)];
            const uint32_t *cp = cum + (size_t)t * MCQ_RG_CUM_STRIDE;
            const uint32_t tot = mcq_ranges_seat_total(cp);
            wc.total[lane] = tot;
            if (tab_in_lds && !(tot & MCQ_RG_KNOWN)) cp = s_cum + mcq_ranges_stage_slot(s_tab_id, n_staged, t) * MCQ_RG_CUM_STRIDE;
            wc.cum[lane] = cp;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        unsigned long long *rows = hand_rows + (size_t)qi * MCQ_HT_TABLE_WORDS;
        bool failed = false;
        uint32_t since = 0;
        for (uint32_t round = 0; round < rounds; round++) {
            const uint32_t task = piece.first + round * waves + wv;
            if (task < piece.end) { /* (wave-uniform; a wave without a task goes on to the round's end) */
                Acc acc = {};
                acc.add.table = (__attribute__((address_space(3))) uint32_t *)s_hands;
                acc.watched = seat;
                const uint32_t stream = task * MCQ_WAVE + lane;
                const uint64_t it0 = (uint64_t)stream * MCQ_STREAM_ITERS;
                if (it0 < qc.runs) {
                    McqExtCtrDraws dr;
                    dr.start(seed, first_qid + qi, stream);
                    const uint32_t cnt = (uint32_t)min((uint64_t)MCQ_STREAM_ITERS, (uint64_t)qc.runs - it0);
                    if (tab_in_lds) /* (block-uniform) */
                        for (uint32_t j = 0; j < cnt && !failed; j++)
                            failed = !mcq_iteration_ranges<McqExtCtrDraws, true, Acc>(qc, wc, dr, cards, tab.sel8, my_ids, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
                    else
                        for (uint32_t j = 0; j < cnt && !failed; j++)
                            failed = !mcq_iteration_ranges<McqExtCtrDraws, false, Acc>(qc, wc, dr, cards, tab.sel8, my_ids, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
                }
                tally.add(acc, lane);
            }
            since++;
            if (mcq_hands_flush_due(since, rounds - 1u - round)) { /* (block-uniform: the round counter and the piece) */
                __syncthreads();
                mcq_hands_flush(s_hands, threadIdx.x, blockDim.x, rows, RowAtomicAdd());
                __syncthreads();
                since = 0;
            }
        }
        if (__any(failed) && lane == 0) atomicExch(reinterpret_cast<unsigned long long *>(Row::row(res, qi)), 0ull); /* runs := 0 */
        tally.flush(Row::row(res, qi), lane);
        __syncthreads(); /* the end of the record's piece: the table goes to its rows and is clear for the next record */
        mcq_hands_flush(s_hands, threadIdx.x, blockDim.x, rows, RowAtomicAdd());
        __syncthreads();
    }
}

// A FEW extended queries in ONE launch (production mode; what a decision of the reference's agents asks for: ONE ranged
// query of a thousand iterations, agent_*.py -> get_equity -> run_montecarlo).  The general path above is six stream
// operations (two copies, prep, lists, evaluation, copy back: 140 us for such a query); here the queries travel in the
// kernel arguments, a block takes ONE query, or one part of one -- a wave task per wave and as few working waves per
// block as the launch's 32 blocks allow (4, 8 or 16: waves that share a SIMD take turns at its vector unit, one wave
// per SIMD runs two iterations in 5 us, four in 9; all sixteen waves help with the tables and the lists): validates it, lays its candidate lists
// out in its own LDS (what mcq_ext_lists_kernel does into HBM), runs its wave tasks, adds the waves' rows up in LDS and
// stores the row into the host's pinned result buffer, one row per BLOCK (the host adds the parts of a query); the last
// block to finish raises the completion flag (as mcq_eval_direct_kernel does).  The host sends queries here whose lists fit (at most MCQ_EXT_SMALL_LISTS) and
// that have at most MCQ_EXT_SMALL_TASKS wave tasks.  Same streams, same draws, same tallies as the general path.
template <bool WAYS>
__global__ __launch_bounds__(kExtBlock) void mcq_eval_ext_small_kernel(McqExtSmallKarg karg, mcq_result *__restrict__ res,
                                                                       uint64_t seed, uint64_t first_qid,
                                                                       const McqTables *__restrict__ g_tab,
                                                                       uint32_t *__restrict__ done, volatile uint32_t *done_flag,
                                                                       uint32_t ticket) {
    typedef McqRowKind<WAYS ? MCQ_ROW_WAYS : MCQ_ROW_PLAIN> Row; /* WAYS: one 22-word row per block */
    typedef typename Row::Acc Acc;
    constexpr uint32_t kWaves = kExtBlock / 64;
    constexpr uint32_t kStageEntries = MCQ_EXT_SMALL_LISTS * MCQ_EXT_LIST_STRIDE;
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab;
    __shared__ McqCard cards[64];
    __shared__ McqExtWaveCtx wave_ctx; /* one query per block: one context */
    __shared__ uint16_t ids[(MCQ_MAX_OPP + 1) * kExtBlock];
    __shared__ __attribute__((aligned(16))) uint16_t s_lists[kStageEntries];
    __shared__ uint32_t s_rec[4 + MCQ_EXT_WORDS];
    __shared__ uint32_t wave_tot[kWaves];
    __shared__ unsigned long long partial[kWaves][Row::kLanes];
    __shared__ uint32_t s_failed;
    const McqExtSmallBlock me = mcq_ext_small_unpack(karg.blk[blockIdx.x]);
    const uint32_t qi = me.query, part = me.part, parts = me.parts, wpb = me.wpb;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid < 64) cards[tid] = mcq_card(tid < 52 ? tid : 0u);
    if (tid >= 4u && tid < 4u + MCQ_EXT_WORDS) s_rec[tid] = karg.ext[qi][tid - 4u];
    if (tid == 0) s_failed = 0;
    load_tables(tab, g_tab); /* (ends with a barrier) */
    /* (the query words by scalar loads from the kernel arguments: the iteration wants n_players in an SGPR) */
    const McqQueryWords q = {karg.q[qi][0], karg.q[qi][1], karg.q[qi][2], karg.q[qi][3]};
    const McqExtRec er = {s_rec + 4};
    const bool valid = __builtin_amdgcn_readfirstlane(mcq_query_ext_valid(q, er) ? 1 : 0) != 0;
    const uint32_t n_lists = __builtin_amdgcn_readfirstlane(valid ? mcq_ext_n_lists(q, er) : 0u);
    bool ok = valid && n_lists <= MCQ_EXT_SMALL_LISTS;
    /* the candidate lists, in the order of 52 * a + b: every thread looks at three consecutive candidates, a block scan
     * of the counts puts the survivors in order (the steps: mcq_stage.hpp) */
    uint32_t list_at = 0;
    for (uint32_t li = 0; li < n_lists && ok; li++) { /* (block-uniform) */
        uint64_t U;
        uint32_t set_off;
        mcq_ext_list_plan(q, er, li, U, set_off);
        constexpr uint32_t kPer = (2704u + kExtBlock - 1) / kExtBlock; /* 3 */
        const uint32_t mask = mcq_ext_list_mask<kPer>(U, er.w + set_off, tid);
        uint32_t total;
        const uint32_t at = block_exclusive_scan<uint32_t, kWaves>((uint32_t)__popc(mask), wave_tot, &total);
        total = __builtin_amdgcn_readfirstlane(total);
        mcq_ext_list_scatter<kPer>(mask, tid, at, s_lists + list_at);
        if (tid == 0) {
            wave_ctx.cnt[li] = total;
            wave_ctx.list[li] = s_lists + list_at;
        }
        if (total == 0u) ok = false; /* a range no pair of cards can satisfy: nothing to deal from */
        list_at += total;
    }
    McqExtCtx qc;
    mcq_ext_ctx(q, er, qc);
    /* (what came out of the record in LDS is wave-uniform: say so) */
    qc.deck_lo = __builtin_amdgcn_readfirstlane(qc.deck_lo);
    qc.deck_hi = __builtin_amdgcn_readfirstlane(qc.deck_hi);
    qc.fdeck_lo = __builtin_amdgcn_readfirstlane(qc.fdeck_lo);
    qc.fdeck_hi = __builtin_amdgcn_readfirstlane(qc.fdeck_hi);
    qc.n_hands = __builtin_amdgcn_readfirstlane(qc.n_hands);
    qc.opp_all = __builtin_amdgcn_readfirstlane(qc.opp_all ? 1 : 0) != 0;
    qc.fast = __builtin_amdgcn_readfirstlane(qc.fast ? 1 : 0) != 0;
    if (tid < 10u) wave_ctx.hand[tid] = tid < qc.n_hands ? mcq_ext_hand(q, er, tid) : 0u;
    if (tid >= 64u && tid < 64u + MCQ_EXT_MAX_LISTS && tid - 64u >= n_lists) { /* never read; defined all the same */
        wave_ctx.cnt[tid - 64u] = 1u;
        wave_ctx.list[tid - 64u] = s_lists;
    }
    __syncthreads();
    const uint32_t s_iters = __builtin_amdgcn_readfirstlane(valid ? mcq_ext_stream_iters(q, er) : MCQ_STREAM_ITERS);
    const uint32_t n_tasks = __builtin_amdgcn_readfirstlane(ok ? mcq_ext_task_count(q, s_iters) : 0u);
    typename Row::Tally tally;
    tally.clear();
    bool failed = false;
    for (uint32_t task = part * wpb + __builtin_amdgcn_readfirstlane(wv); wv < wpb && task < n_tasks; task += parts * wpb) {
        Acc acc = {};
        const uint32_t stream = task * MCQ_WAVE + lane;
        const uint64_t it0 = (uint64_t)stream * s_iters;
        if (it0 < qc.runs) {
            McqExtCtrDraws dr;
            dr.start(seed, first_qid + qi, stream);
            const uint32_t cnt = (uint32_t)min((uint64_t)s_iters, (uint64_t)qc.runs - it0);
            if (qc.fast) /* (block-uniform) */
                for (uint32_t j = 0; j < cnt && !failed; j++)
                    failed = !mcq_iteration_ext_fast<McqExtCtrDraws, false, true, Acc>(qc, wave_ctx, dr, cards, tab.sel8, g_tab->tf, tab.tops, tab.sd, acc);
            else
                for (uint32_t j = 0; j < cnt && !failed; j++)
                    failed = !mcq_iteration_ext<McqExtCtrDraws, true, Acc>(qc, wave_ctx, dr, cards, tab.sel8, ids + tid, kExtBlock, g_tab->tf, tab.tops, tab.sd, acc);
        }
        tally.add(acc);
    }
    if (__any(failed) && lane == 0) atomicOr(&s_failed, 1u);
    const unsigned long long mine = tally.row_words(lane);
    if (lane < Row::kLanes) partial[wv][lane] = mine;
    __syncthreads();
    if (tid < Row::kWords) { /* word tid of the row */
        unsigned long long v = 0;
        if (tid > 0u)
            for (uint32_t k = 0; k < kWaves; k++) v += partial[k][tid - 1u];
        const bool bad = !ok || s_failed != 0u;
        if (tid == 0u) v = bad ? 0ull : (unsigned long long)qc.runs;
        else if (bad) v = tid == 1u && !valid ? ~0ull : 0ull; /* invalid: passes = UINT64_MAX, as mcq_prep_ext_kernel marks it */
        reinterpret_cast<unsigned long long *>(Row::row(res, blockIdx.x))[tid] = v;
    }
    mcq_block_done(done, done_flag, ticket);
}

// ---------------------------------------------------------------------------------------------- showdown
// hand_evaluator.get_winner (tools/hand_evaluator.py:9-24) for many tables: the same ranking key as the Monte-Carlo path.
// HBM/PCIe-bound byte work (7 bytes in per hand, 2 bytes out per table), so the layout is what matters: a block takes a
// TILE of 256 tables, whose hands are one contiguous run of 256 * n_players * 7 bytes -- staged into LDS with 16-byte
// loads straight from the caller-visible buffer (pinned host memory or HBM), evaluated one table per thread with the
// lookup tables read through the vector L1 / L2 (2 M lookups: not worth 97 KB of LDS per block), results leave as
// 16-byte stores.  A hand that does not hold seven distinct ids < 52 marks `bad` (the host reports MCQ_EINVAL) --
// validation on the device, as mcq_prep_kernel does for queries.  With ticket != 0 the last block to finish raises the
// host's completion flag behind a system-scope release, as mcq_publish_kernel does.
constexpr int kShowBlock = 256;
constexpr uint32_t kShowBlocksPerCu = 5u; /* grid cap of the launch: 30 KB of LDS per block, five blocks per CU */
__global__ __launch_bounds__(kShowBlock) void mcq_showdown_kernel(const uint8_t *__restrict__ hands, uint32_t n_tables,
                                                                  uint32_t n_players, const McqTables *__restrict__ g_tab,
                                                                  uint8_t *__restrict__ winner, uint8_t *__restrict__ wtype,
                                                                  uint32_t *__restrict__ keys, uint32_t *__restrict__ bad,
                                                                  uint32_t *__restrict__ done, volatile uint32_t *done_flag,
                                                                  uint32_t ticket) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kShowBlock * 7 * 10];
    __shared__ __attribute__((aligned(16))) uint32_t tile_keys[kShowBlock * 10];
    __shared__ __attribute__((aligned(16))) uint8_t tile_win[kShowBlock], tile_type[kShowBlock];
    const uint32_t per_table = 7u * n_players, n_tiles = (n_tables + kShowBlock - 1u) / kShowBlock;
    for (uint32_t t0 = blockIdx.x; t0 < n_tiles; t0 += gridDim.x) {
        const uint32_t first = t0 * kShowBlock, cnt = min((uint32_t)kShowBlock, n_tables - first);
        const uint32_t bytes = cnt * per_table, vecs = (bytes + 15u) / 16u; /* the buffers are padded to 16 bytes */
        const uint4 *src = reinterpret_cast<const uint4 *>(hands + (size_t)first * per_table); /* 256 * 7 * P: a multiple of 16 */
        __syncthreads(); /* the previous tile has been read */
        for (uint32_t i = threadIdx.x; i < vecs; i += kShowBlock) reinterpret_cast<uint4 *>(tile)[i] = src[i];
        __syncthreads();
        if (threadIdx.x < cnt) {
            const uint8_t *h = tile + threadIdx.x * per_table;
            uint32_t best = 0, w = 0;
            bool ok = true;
            for (uint32_t p = 0; p < n_players; p++, h += 7) {
                uint64_t seen = 0;
                uint32_t c[7];
#pragma unroll
                for (int k = 0; k < 7; k++) {
                    c[k] = h[k];
                    ok = ok && c[k] < 52u && !((seen >> (c[k] & 63u)) & 1ull);
                    seen |= 1ull << (c[k] & 63u);
                    c[k] = c[k] < 52u ? c[k] : 0u;
                }
                McqBoard b;
                b.clear();
#pragma unroll
                for (int k = 2; k < 7; k++) b.add(mcq_card(c[k]));
                McqHole hole;
                hole.set(mcq_card(c[0]), mcq_card(c[1]));
                McqFlushSel fs;
                fs.from_board(b);
                const uint32_t key = mcq_eval_key(b, fs, hole, g_tab->tf, g_tab->tops, g_tab->sd);
                tile_keys[threadIdx.x * n_players + p] = key;
                if (key > best) { best = key; w = p; } /* strict: the first of equal hands stays (hand_evaluator.py:23) */
            }
            tile_win[threadIdx.x] = (uint8_t)w;
            tile_type[threadIdx.x] = (uint8_t)mcq_key_type(best);
            if (!ok) *reinterpret_cast<volatile uint32_t *>(bad) = 1u; /* (a plain store: every writer writes the same word) */
        }
        __syncthreads();
        /* results: whole 16-byte words (the output buffers are padded to the tile) */
        if (threadIdx.x < kShowBlock / 16) {
            reinterpret_cast<uint4 *>(winner + first)[threadIdx.x] = reinterpret_cast<const uint4 *>(tile_win)[threadIdx.x];
            reinterpret_cast<uint4 *>(wtype + first)[threadIdx.x] = reinterpret_cast<const uint4 *>(tile_type)[threadIdx.x];
        }
        if (keys) {
            const uint32_t kv = (cnt * n_players + 3u) / 4u;
            uint4 *dst = reinterpret_cast<uint4 *>(keys + (size_t)first * n_players); /* 256 * P keys: a multiple of four */
            for (uint32_t i = threadIdx.x; i < kv; i += kShowBlock) dst[i] = reinterpret_cast<const uint4 *>(tile_keys)[i];
        }
    }
    if (ticket == 0u) return; /* not the last launch of the call */
    mcq_block_done(done, done_flag, ticket); /* (the results and `bad`) */
}

// ---------------------------------------------------------------------------------------------- exact enumeration
// one query per launch, see mcq_exact.hpp.  Work unit = (table completion, slice of first
// opponent hands); a wave takes units wave, wave + n_waves, ...  Per-lane 64-bit sums by role: lane 0 total
// weight (-> runs), lane 2 strict wins, lane 3 ties, lane 4 + t hero's winning hand type t; one atomic each
// at the end.
template <bool TWO_OPP>
__global__ __launch_bounds__(TWO_OPP ? 384 : 1024) void mcq_exact_kernel(const McqExactJob *__restrict__ jobs, int law,
                                                                        mcq_result *__restrict__ rows,
                                                                        const McqTables *__restrict__ g_tab) {
    /* blockIdx.y = the job (one query); its first `grid` blocks work, the others leave at once */
    const McqExactJob job = jobs[blockIdx.y];
    if (blockIdx.x >= job.grid) return;
    const uint4 raw = make_uint4(job.rec[0], job.rec[1], job.rec[2], job.rec[3]);
    const uint32_t n_boards = job.n_boards, slices = job.slices;
    mcq_result *row = rows + job.row;
    constexpr uint32_t kWaves = TWO_OPP ? 6u : 16u; /* what fits beside the 97 KB of tables */
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab; /* tf from global memory, as in the evaluation kernels */
    __shared__ uint16_t pair_xy[MCQ_EXACT_PAIRS + 2];
    __shared__ McqCard rem_card_all[kWaves][64];
    __shared__ uint32_t rem_pos_all[kWaves][64];
    __shared__ uint32_t keys_all[TWO_OPP ? kWaves : 1u][TWO_OPP ? MCQ_EXACT_PAIRS + 2 : 1u];
    __shared__ uint16_t rec_all[TWO_OPP ? kWaves : 1u][TWO_OPP ? MCQ_EXACT_PAIRS + 2 : 1u];
    load_tables(tab, g_tab);
    for (uint32_t i = threadIdx.x; i < MCQ_EXACT_PAIRS; i += blockDim.x) {
        uint32_t x, y;
        mcq_exact_pair_xy(i, x, y);
        pair_xy[i] = (uint16_t)(x | (y << 8));
    }
    __syncthreads();

    const McqQueryWords q = {raw.x, raw.y, raw.z, raw.w};
    McqExactQuery e;
    if (!mcq_exact_query(q, law, e)) return; /* the host has validated the query */
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wib);
    const uint32_t n_waves = job.grid * kWaves;
    McqCard *rem_card = rem_card_all[wib];
    uint32_t *rem_pos = rem_pos_all[wib];
    uint32_t *keys = TWO_OPP ? keys_all[wib] : nullptr;
    uint16_t *rec = TWO_OPP ? rec_all[wib] : nullptr;

    unsigned long long sum = 0;
    const uint64_t n_units = (uint64_t)n_boards * slices;
    for (uint64_t unit = wave; unit < n_units; unit += n_waves) {
        const uint32_t board = (uint32_t)(unit / slices), slice = (uint32_t)(unit % slices);
        uint32_t pos[5];
        mcq_exact_unrank(board, e.L, e.k, pos);
        McqExactBoard bd;
        mcq_exact_board(e, pos, tab.sel8, g_tab->tf, tab.tops, tab.sd, bd);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); /* the previous unit's reads are done (same wave) */
        if (lane < MCQ_EXACT_REM) {
            const uint32_t rp = mcq_exact_rem_pos(pos, lane);
            rem_pos[lane] = rp;
            rem_card[lane] = mcq_card(mcq_exact_card_at(e, rp, tab.sel8));
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        McqExactAcc acc = {0, 0, 0};
        mcq_exact_pass_a(e, bd, lane, pair_xy, rem_card, rem_pos, g_tab->tf, tab.tops, tab.sd, keys, rec, acc);
        if (TWO_OPP) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            mcq_exact_pass_b(e, bd, lane, MCQ_EXACT_PAIRS * slice / slices, MCQ_EXACT_PAIRS * (slice + 1u) / slices,
                             pair_xy, keys, rec, acc);
        }
        const uint32_t win = wave_sum(acc.win), tie = wave_sum(acc.tie), tot = wave_sum(acc.tot);
        const uint32_t type = mcq_key_type(bd.hero_key);
        if (lane == 0u) sum += tot;
        if (lane == 2u) sum += win;
        if (lane == 3u) sum += tie;
        if (lane == 4u + type) sum += win + tie;
    }
    if (lane < 13u && sum != 0ull) atomicAdd(reinterpret_cast<unsigned long long *>(row) + lane, sum);
}

// ---------------------------------------------------------------------------------------------- exact enumeration, extended
// SURVEY 8f-3 x 8f-2, see mcq_exact_ext.hpp; one job per query (blockIdx.y), all of one KIND = random opponents:
//   0  a lane per table completion (hand against known hands: C(48, 5) completions preflop, nothing else to do);
//   1  a wave per completion, lanes over the candidate hands, as mcq_exact_kernel<false>;
//   2  a BLOCK per completion: its 1024 threads make the candidate keys once (LDS), then thread t owns first hand
//      group * 1024 + t (an R-pair: fixed across completions) and walks every second hand; its sums stay in registers
//      until the block's last completion and go to h1_sums[job.h1_off + 12 * hand] (integer atomics: deterministic).
//      LDS: 97 KB of tables + 10 KB of keys and records, one block of 16 waves per CU.
// Kinds 0 and 1 add into the zeroed row rows[job.row]: lane l adds word l of the row, one atomic at the end.
// ROW = MCQ_ROW_WAYS (kinds 0 and 1): 22-word rows; word 13 + (k - 2) is the weight of the ties shared by k hands
// (mcq_exact_ext_row_word).  ROW = MCQ_ROW_SEATS (kinds 0 and 1): 32-word rows of mcq_result_seats
// (mcq_exact_ext_seats_word).  Two random opponents have neither form.
// Three bodies, one per kind; what differs by ROW is a small policy: McqExactLoneSums<ROW> (kind 0: a lane's counters over
// its completions and their flush into lane roles) and McqExactRow<ROW> (kind 1: a lane's accumulator over the candidates of
// one completion, the pass that fills it and the row word that the wave sums give).  mcq_exact_runout_kernel uses the same
// loops with "store the completion's row" in place of "add to a running sum".

// Block prologue of the family (also of the hero bodies below): the record's extension words, the pair list (N_PAIRS entries
// x | y << 8), the evaluator's tables, the query -- built by thread 0, the host has validated it; build(words, record)
// returns its McqExactExtQuery -- and the deck's card ids by R-position (zero at and above L).  Ends with a barrier.
template <uint32_t N_PAIRS, class Build>
__device__ __forceinline__ void exact_prologue(const McqExactExtJob &job, const uint32_t *__restrict__ ext,
                                               const McqTables *__restrict__ g_tab, LdsTablesEval &tab, uint16_t *pair_xy,
                                               uint32_t *xw, uint8_t *r_id, Build build) {
    const uint32_t tid = threadIdx.x;
    if (tid < MCQ_EXT_WORDS) xw[tid] = ext[(size_t)job.ext * MCQ_EXT_WORDS + tid];
    if (tid < 64u) r_id[tid] = 0;
    for (uint32_t i = tid; i < N_PAIRS; i += blockDim.x) {
        uint32_t x, y;
        mcq_exact_pair_xy(i, x, y);
        pair_xy[i] = (uint16_t)(x | (y << 8));
    }
    load_tables(tab, g_tab); /* ends with a barrier */
    if (tid == 0) {
        const McqExtRec er = {xw};
        mcq_exact_ext_r_ids(build({job.rec[0], job.rec[1], job.rec[2], job.rec[3]}, er), r_id);
    }
    __syncthreads();
}

/* A thread's view of its block's LDS beside the 97 KB of tables.  The arrays are declared by the kernel itself (a kernel
 * pays only for those it reads: kind 0 keeps no pair list, no range bits and no rem lists); rem_card / rem_pos are the
 * thread's own wave's (kind 1) or the block's (kind 2). */
struct McqExactExtBlock {
    static constexpr uint32_t kWaves = 16u;
    LdsTablesEval &tab;
    McqExactExtQuery &xq;
    uint16_t *pair_xy;
    uint8_t *r_id, *cb_tab;
    McqCard *rem_card;
    uint32_t *rem_pos;
};

/* ... and its filling: the prologue, then (kinds 1 and 2) the range bits of every R-pair */
template <uint32_t KIND, class Build>
__device__ __forceinline__ void exact_ext_setup(const McqExactExtJob &job, const uint32_t *__restrict__ ext,
                                                const McqTables *__restrict__ g_tab, const McqExactExtBlock &s, uint32_t *xw,
                                                Build build) {
    exact_prologue<MCQ_EXACT_PAIRS>(job, ext, g_tab, s.tab, s.pair_xy, xw, s.r_id, build);
    if (KIND != 0u) {
        mcq_exact_ext_cb_table(s.xq, s.r_id, threadIdx.x, blockDim.x, s.cb_tab);
        __syncthreads();
    }
}

// One completion whose candidate hands its owner's threads share -- a wave (`who` = the lane) or, BLOCK, the block (`who`
// = the thread): its R-positions, board and known hands, then the m cards left in rem_pos / rem_card, written between two
// fences (the owner's reads of the previous completion are done; the new lists are visible) and ready after the barrier.
template <bool BLOCK>
__device__ __forceinline__ McqExactKnown exact_step(const McqExactExtBlock &s, uint32_t board, const McqTables *__restrict__ g_tab,
                                                    uint32_t who, uint32_t pos[5], McqExactBoard &bd) {
    const McqExactExtQuery &e = s.xq;
    mcq_exact_unrank(board, e.b.L, e.b.k, pos);
    mcq_exact_board(e.b, pos, s.tab.sel8, g_tab->tf, s.tab.tops, s.tab.sd, bd);
    const McqExactKnown kn = mcq_exact_ext_known(e, bd, g_tab->tf, s.tab.tops, s.tab.sd);
    if (BLOCK) __syncthreads();
    else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (who < e.m) {
        const uint32_t rp = mcq_exact_rem_pos(pos, who);
        s.rem_pos[who] = rp;
        s.rem_card[who] = mcq_card(s.r_id[rp]);
    }
    if (BLOCK) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    return kn;
}

// Kind 0: a lane per completion -- on(idx) for the completions this thread owns.
template <class On>
__device__ __forceinline__ void exact_lane_loop(const McqExactExtJob &job, On on) {
    for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < job.n_boards; idx += job.grid * blockDim.x) on(idx);
}

/* ... and a lane's counters over them.  Plain and split-pot rows: weights of 0 or 1, at most C(48, 5) / 1024 + 1 = 1673 per
 * lane; a tie without a random opponent is shared by 1 + n_eq hands (n_eq >= 1).  word(lane) = word `lane` of the row
 * after the wave sums. */
template <int ROW> struct McqExactLoneSums {
    static constexpr bool kWays = ROW == MCQ_ROW_WAYS;
    McqExactAcc acc;
    uint32_t by_type[9], ways[kWays ? MCQ_N_WAYS : 1u];
    __device__ __forceinline__ void add(const McqExactBoard &bd, const McqExactKnown &kn, uint32_t w) {
        const McqExactAcc a = mcq_exact_ext_lone_acc(bd, kn, w);
        const uint32_t t = mcq_key_type(bd.hero_key);
        acc.win += a.win;
        acc.tie += a.tie;
        acc.tot += a.tot;
#pragma unroll
        for (uint32_t j = 0; j < 9; j++) by_type[j] += j == t ? a.win + a.tie : 0u;
        if constexpr (kWays) {
#pragma unroll
            for (uint32_t j = 0; j < MCQ_N_WAYS; j++) ways[j] += j + 1u == kn.n_eq ? a.tie : 0u;
        }
    }
    __device__ __forceinline__ unsigned long long word(uint32_t lane) const {
        const uint32_t tot = wave_sum(acc.tot), win = wave_sum(acc.win), tie = wave_sum(acc.tie);
        uint32_t mine = lane < 4u ? (uint32_t)mcq_exact_ext_row_word(lane, win, tie, tot, 0u, 0u, 0u) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 9; j++) {
            const uint32_t v = wave_sum(by_type[j]);
            mine = lane == 4u + j ? v : mine;
        }
        if constexpr (kWays) {
#pragma unroll
            for (uint32_t j = 0; j < MCQ_N_WAYS; j++) {
                const uint32_t v = wave_sum(ways[j]);
                mine = lane == 13u + j ? v : mine;
            }
        }
        return mine;
    }
};
/* Per seat (the all-in case): a lane ranks every hand of its completion and keeps the level seats' weights.  A seat's
 * share, in units of 2520 / k, stays below 2^23 per lane and 2^29 per wave; win and tie share one word as 16-bit halves
 * (64 lanes x 1673 does not fit a half: they are summed apart). */
template <> struct McqExactLoneSums<MCQ_ROW_SEATS> {
    uint32_t tot, share[MCQ_MAX_SEATS], wt[MCQ_MAX_SEATS];
    __device__ __forceinline__ void add(const McqExactBoard &, const McqExactKnown &kn, uint32_t w) {
        const uint32_t inc = w ? mcq_seat_increment(mcq_popc(kn.level)) : 0u;
        tot += w;
#pragma unroll
        for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) {
            const bool on = ((kn.level >> s) & 1u) != 0u;
            share[s] += on ? inc & 0xFFFFu : 0u;
            wt[s] += on ? ((inc >> MCQ_SEAT_WIN_SHIFT) & 1u) | (((inc >> MCQ_SEAT_TIE_SHIFT) & 1u) << 16) : 0u;
        }
    }
    __device__ __forceinline__ unsigned long long word(uint32_t lane) const {
        const uint32_t t = wave_sum(tot);
        unsigned long long mine = lane == 0u ? t : 0ull;
#pragma unroll
        for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) {
            const uint32_t win = wave_sum(wt[s] & 0xFFFFu), tie = wave_sum(wt[s] >> 16), sh = wave_sum(share[s]);
            mine = lane == 2u + 3u * s ? win : lane == 3u + 3u * s ? tie : lane == 4u + 3u * s ? sh : mine;
        }
        return mine;
    }
};

// Kind 1: what a row form does with one completion.  Plain and split-pot: the candidates' outcomes against the known hands'
// best; the split-pot form keeps tie_c as well and names n_eq (one random opponent leaves at most eight known hands:
// word 13 + n_eq <= 21).
template <int ROW> struct McqExactRow {
    typedef std::conditional_t<ROW == MCQ_ROW_WAYS, McqExactAccWays, McqExactAcc> Acc;
    static __device__ __forceinline__ void pass(const McqExactExtBlock &s, const McqTables *__restrict__ g_tab,
                                                const McqExactBoard &bd, const McqExactKnown &kn, uint32_t lane, Acc &acc) {
        mcq_exact_ext_pass_a_tally(s.xq, bd, kn.best, lane, 64u, s.pair_xy, s.rem_card, s.rem_pos, s.cb_tab, g_tab->tf, s.tab.tops,
                             s.tab.sd, acc);
    }
    static __device__ __forceinline__ unsigned long long word(uint32_t lane, const McqExactExtQuery &, const McqExactBoard &bd,
                                                              const McqExactKnown &kn, const Acc &acc, uint32_t tot) {
        const uint32_t win = wave_sum(acc.win), tie = wave_sum(acc.tie), type = mcq_key_type(bd.hero_key);
        if constexpr (Acc::kWays) return mcq_exact_ext_row_word(lane, win, tie, tot, wave_sum(acc.tie_c), type, kn.n_eq);
        else return mcq_exact_ext_row_word(lane, win, tie, tot, 0u, type, 0u);
    }
};
/* Per seat: the best key among hero and the known hands is wave-uniform, so a lane keeps the candidates' weight above it,
 * level with it and in all (lanes 32..63: seats nobody holds, nothing) */
template <> struct McqExactRow<MCQ_ROW_SEATS> {
    typedef McqExactAccSeats Acc;
    static __device__ __forceinline__ void pass(const McqExactExtBlock &s, const McqTables *__restrict__ g_tab,
                                                const McqExactBoard &bd, const McqExactKnown &kn, uint32_t lane, Acc &acc) {
        mcq_exact_ext_pass_seats(s.xq, bd, kn.top, lane, 64u, s.pair_xy, s.rem_card, s.rem_pos, s.cb_tab, g_tab->tf, s.tab.tops,
                                 s.tab.sd, acc);
    }
    static __device__ __forceinline__ unsigned long long word(uint32_t lane, const McqExactExtQuery &e, const McqExactBoard &,
                                                              const McqExactKnown &kn, const Acc &acc, uint32_t tot) {
        return mcq_exact_ext_seats_word(lane, kn.level, e.n_known, wave_sum(acc.gt), wave_sum(acc.eq), tot);
    }
};

// Kind 1: a wave per completion, lanes over the candidate hands -- on(pos, tot, word) gets the completion's R-positions,
// its total weight and, in lane l, word l of its row.
template <int ROW, class On>
__device__ __forceinline__ void exact_wave_loop(const McqExactExtJob &job, const McqExactExtBlock &s,
                                                const McqTables *__restrict__ g_tab, On on) {
    typedef McqExactRow<ROW> Row;
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * s.kWaves + wib), n_waves = job.grid * s.kWaves;
    for (uint32_t board = wave; board < job.n_boards; board += n_waves) {
        uint32_t pos[5];
        McqExactBoard bd;
        const McqExactKnown kn = exact_step<false>(s, board, g_tab, lane, pos, bd);
        typename Row::Acc acc = {};
        Row::pass(s, g_tab, bd, kn, lane, acc);
        const uint32_t tot = wave_sum(acc.tot);
        on(pos, tot, Row::word(lane, s.xq, bd, kn, acc, tot));
    }
}

template <uint32_t KIND, int ROW>
__global__ __launch_bounds__(1024) void mcq_exact_ext_kernel(const McqExactExtJob *__restrict__ jobs, const uint32_t *__restrict__ ext,
                                                             int law, mcq_result *__restrict__ rows,
                                                             unsigned long long *__restrict__ h1_sums,
                                                             const McqTables *__restrict__ g_tab) {
    const McqExactExtJob job = jobs[blockIdx.y];
    if (blockIdx.x >= job.grid) return;
    static_assert(ROW == MCQ_ROW_PLAIN || KIND <= 1u, "two random opponents have no split-pot and no per-seat form");
    constexpr uint32_t kRem = KIND == 1u ? McqExactExtBlock::kWaves : 1u;
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab;
    __shared__ uint16_t pair_xy[MCQ_EXACT_PAIRS + 2];
    __shared__ uint32_t xw[MCQ_EXT_WORDS];
    __shared__ McqExactExtQuery xq;
    __shared__ uint8_t r_id[64];
    __shared__ uint8_t cb_tab[KIND != 0u ? MCQ_XX_MAX_RP : 1u];
    __shared__ McqCard rem_card[kRem][64];
    __shared__ uint32_t rem_pos[kRem][64];
    __shared__ uint32_t keys[KIND == 2u ? MCQ_EXACT_PAIRS + 2 : 1u];
    __shared__ uint32_t recs[KIND == 2u ? MCQ_EXACT_PAIRS + 2 : 1u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wib = KIND == 1u ? tid >> 6 : 0u;
    const McqExactExtBlock s = {tab, xq, pair_xy, r_id, cb_tab, rem_card[wib], rem_pos[wib]};
    exact_ext_setup<KIND>(job, ext, g_tab, s, xw, [&](const McqQueryWords &q, const McqExtRec &er) -> const McqExactExtQuery & {
        (void)mcq_exact_ext_query(q, er, law, xq);
        return xq;
    });
    const McqExactExtQuery &e = xq;
    unsigned long long *row = reinterpret_cast<unsigned long long *>(McqRowKind<ROW>::row(rows, job.row));

    if constexpr (KIND == 0u) {
        McqExactLoneSums<ROW> c = {};
        exact_lane_loop(job, [&](uint32_t idx) {
            uint32_t pos[5];
            McqExactBoard bd;
            McqExactKnown kn;
            const uint32_t w = mcq_exact_ext_lone_known(e, idx, tab.sel8, g_tab->tf, tab.tops, tab.sd, pos, bd, kn);
            c.add(bd, kn, w);
        });
        const unsigned long long mine = c.word(lane);
        if (lane < McqRowKind<ROW>::kWords && mine != 0ull) atomicAdd(row + lane, mine);
    } else if constexpr (KIND == 1u) {
        unsigned long long sum = 0;
        exact_wave_loop<ROW>(job, s, g_tab, [&](const uint32_t *, uint32_t, unsigned long long word) { sum += word; });
        if (lane < McqRowKind<ROW>::kWords && sum != 0ull) atomicAdd(row + lane, sum);
    } else {
        const uint32_t groups = job.groups, group = blockIdx.x % groups, h = group * blockDim.x + tid;
        const bool own = h < e.n_rp;
        uint32_t qa = 0, qb = 1;
        if (own) mcq_exact_pair_xy(h, qa, qb);
        McqExactExtSums sums = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
        for (uint32_t board = blockIdx.x / groups; board < job.n_boards; board += job.grid / groups) {
            uint32_t pos[5];
            McqExactBoard bd;
            /* (its first barrier: the previous completion's pass B is done with keys and records) */
            const uint32_t kb = exact_step<true>(s, board, g_tab, tid, pos, bd).best;
            mcq_exact_ext_pass_a_store(e, bd, kb, tid, blockDim.x, pair_xy, s.rem_card, s.rem_pos, cb_tab, g_tab->tf, tab.tops,
                                       tab.sd, keys, recs);
            __syncthreads();
            const uint32_t mi = own ? mcq_exact_ext_m_index(e, pos, qa, qb) : e.n_pairs;
            if (mi < e.n_pairs) {
                McqExactAcc acc = {0, 0, 0};
                mcq_exact_ext_pass_b(e, bd, qa, qb, mi, keys, recs, acc);
                mcq_exact_ext_add(sums, acc, mcq_key_type(bd.hero_key));
            }
        }
        if (own) {
            unsigned long long *dst = h1_sums + job.h1_off + (size_t)h * MCQ_XX_SUMS;
            if (sums.win) atomicAdd(dst + 0, sums.win);
            if (sums.tie) atomicAdd(dst + 1, sums.tie);
            if (sums.tot) atomicAdd(dst + 2, sums.tot);
#pragma unroll
            for (uint32_t t = 0; t < 9; t++)
                if (sums.type[t]) atomicAdd(dst + 3 + t, sums.type[t]);
        }
    }
}

// ---------------------------------------------------------------------------------------------- exact enumeration, hero range
// Four kernels -- postflop or preflop, class bits or a weight per hand (McqHeroKind<W>, mcq_exact_hero.hpp) -- made of two
// bodies, one per street, of exact_prologue above (every D-pair as qa | qb << 8 in its pair list) and of the helpers below,
// which both bodies share.  One job per query (blockIdx.y), a BLOCK of 1024 threads per table completion, one block of 16
// waves per CU.

// the prologue's query builder: thread 0 fills the block's McqExactHeroQuery
__device__ __forceinline__ auto hero_query(int law, McqExactHeroQuery &xq) {
    return [law, &xq](const McqQueryWords &q, const McqExtRec &er) -> const McqExactExtQuery & {
        (void)mcq_exact_hero_query(q, er, law, false, xq);
        return xq.x;
    };
}

// W = true: the block's two weight tables per D-pair, folded from the query row's tables in wts -- the opponent's [1326]
// uint16, then the hero's; hero_w == 0: the hero's is not there and every hand of the hero's classes weighs 1.
__device__ __forceinline__ void hero_fold_weights(const McqExactHeroQuery &e, const uint8_t *r_id, const uint16_t *__restrict__ wts,
                                                  uint32_t row, uint32_t hero_w, uint16_t *ow_tab, uint16_t *hw_tab) {
    const uint16_t *w_opp = wts + (size_t)row * 2u * MCQ_XH_ROWS;
    mcq_exact_hero_w_tables(e, r_id, w_opp, hero_w ? w_opp + MCQ_XH_ROWS : nullptr, threadIdx.x, blockDim.x, ow_tab, hw_tab);
}

// Ballot compaction: on(rp) says of D-pair rp < n_rp whether it is allowed (bit 0) and live (bit 1).  `ranked` gets the
// D-pairs with a bit set, ascending; LISTS: `allowed` and `live` get their slots in `ranked`.  n[0..3) = allowed, live,
// ranked (without LISTS the caller sets no live bit: `ranked` is the allowed list and only n[2] is counted).  Two passes of
// 64 D-pairs per wave -- count per chunk, barrier, prefix and scatter, barrier --, so every block makes the same lists.
// chunk_cnt: [LISTS ? 3 : 1][(MAX_PAIRS + 63) / 64].
template <uint32_t MAX_PAIRS, bool LISTS, class On>
__device__ __forceinline__ void hero_compact(uint32_t n_rp, On on, uint32_t *chunk_cnt, uint16_t *ranked, uint16_t *allowed,
                                             uint16_t *live, uint32_t n[3]) {
    constexpr uint32_t kChunks = (MAX_PAIRS + 63u) / 64u;
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    uint32_t *cnt_r = chunk_cnt, *cnt_a = chunk_cnt + (LISTS ? kChunks : 0u), *cnt_l = chunk_cnt + (LISTS ? 2u * kChunks : 0u);
#pragma unroll
    for (uint32_t pass = 0; pass < 2u; pass++) {
        for (uint32_t c = wib; c < kChunks; c += 16u) {
            const uint32_t rp = c * 64u + lane, bits = on(rp);
            const unsigned long long ma = __ballot((bits & 1u) != 0u), ml = LISTS ? __ballot((bits & 2u) != 0u) : 0ull;
            if (pass == 0u) {
                if (lane == 0u) {
                    if (LISTS) {
                        cnt_a[c] = (uint32_t)__popcll(ma);
                        cnt_l[c] = (uint32_t)__popcll(ml);
                    }
                    cnt_r[c] = (uint32_t)__popcll(ma | ml);
                }
                continue;
            }
            const unsigned long long below = (1ull << lane) - 1ull;
            uint32_t base_a = 0, base_l = 0, base_r = 0;
            for (uint32_t j = 0; j < c; j++) {
                if (LISTS) {
                    base_a += cnt_a[j];
                    base_l += cnt_l[j];
                }
                base_r += cnt_r[j];
            }
            const uint32_t slot = base_r + (uint32_t)__popcll((ma | ml) & below);
            if (bits != 0u) ranked[slot] = (uint16_t)rp;
            if (LISTS) {
                if (bits & 1u) allowed[base_a + (uint32_t)__popcll(ma & below)] = (uint16_t)slot;
                if (bits & 2u) live[base_l + (uint32_t)__popcll(ml & below)] = (uint16_t)slot;
            }
        }
        if (pass == 0u) __syncthreads();
    }
    n[0] = n[1] = n[2] = 0u;
    for (uint32_t j = 0; j < kChunks; j++) {
        if (LISTS) {
            n[0] += cnt_a[j];
            n[1] += cnt_l[j];
        }
        n[2] += cnt_r[j];
    }
    __syncthreads();
}

// Row flush: a hero hand's twelve sums into its mcq_result row (runs, passes, win, tie, by_type[9]) among the query's zeroed
// [1326][13] rows -- 64-bit integer atomics, so the result is deterministic.
template <class Sums>
__device__ __forceinline__ void hero_flush(unsigned long long *__restrict__ rows, uint32_t q_row, uint32_t row, const Sums &s) {
    unsigned long long *dst = rows + ((size_t)q_row * MCQ_XH_ROWS + row) * 13u;
    if (s.tot) atomicAdd(dst + 0, (unsigned long long)s.tot);
    if (s.win) atomicAdd(dst + 2, (unsigned long long)s.win);
    if (s.tie) atomicAdd(dst + 3, (unsigned long long)s.tie);
#pragma unroll
    for (uint32_t t = 0; t < 9; t++)
        if (s.type[t]) atomicAdd(dst + 4 + t, (unsigned long long)s.type[t]);
}

// Postflop (mcq_exact_hero.hpp): the shape of mcq_exact_ext_kernel's kind 2 with the first hand being the HERO's.  Per
// completion the 1024 threads rank the C(m, 2) <= 1081 candidate hands once (LDS), then thread t of group g owns the
// (g * 1024 + t)-th ALLOWED hero hand (a D-pair, fixed across completions; the hands outside the range or the deck are not
// on the list and cost no walk) and walks every candidate as the opponent's hand with broadcast LDS reads: three barriers
// per completion.  Its twelve sums stay in registers until the block's last completion.
// W = true: the uniform law only.  The opponent's table is ow_tab (4.7 KB with hw_tab, in place of the 1.2 KB of range
// bits), the allowed list is made from hw_tab; a completion's sums are 32-bit as before and are added ONCE per completion
// into twelve 64-bit sums.
// LDS: 97 KB of tables + 8.7 KB of keys and records + 6 KB of lists.
template <bool W>
__device__ __forceinline__ void hero_body(const McqExactExtJob *__restrict__ jobs, const uint32_t *__restrict__ ext, int law,
                                          const uint16_t *__restrict__ wts, uint32_t hero_w, unsigned long long *__restrict__ rows,
                                          const McqTables *__restrict__ g_tab) {
    typedef McqHeroKind<W> Kind;
    const McqExactExtJob job = jobs[blockIdx.y];
    if (blockIdx.x >= job.grid) return;
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab;
    __shared__ uint16_t pair_xy[MCQ_XH_MAX_HANDS]; /* every D-pair; the candidate hands are its first n_pairs entries */
    __shared__ uint32_t xw[MCQ_EXT_WORDS];
    __shared__ McqExactHeroQuery xq;
    __shared__ uint8_t r_id[64];
    __shared__ typename Kind::opp_t opp_tab[W ? MCQ_XH_MAX_HANDS : MCQ_XX_MAX_RP + 3u];
    __shared__ uint16_t own_list[MCQ_XH_MAX_HANDS];
    __shared__ uint32_t chunk_cnt[(MCQ_XH_MAX_HANDS + 63u) / 64u];
    __shared__ McqCard rem_card[64];
    __shared__ uint32_t rem_pos[64];
    __shared__ uint32_t keys[MCQ_XH_MAX_PAIRS + 3u];
    __shared__ uint32_t recs[MCQ_XH_MAX_PAIRS + 3u];
    static_assert(MCQ_XH_MAX_PAIRS <= MCQ_XH_MAX_HANDS, "pair_xy covers the candidate hands");
    const uint32_t tid = threadIdx.x;
    exact_prologue<MCQ_XH_MAX_HANDS>(job, ext, g_tab, tab, pair_xy, xw, r_id, hero_query(law, xq));
    const McqExactHeroQuery &e = xq;
    const uint16_t *hw_tab = nullptr;
    if constexpr (W) {
        __shared__ uint16_t hw[MCQ_XH_MAX_HANDS];
        hero_fold_weights(e, r_id, wts, job.row, hero_w, opp_tab, hw);
        hw_tab = hw;
        __syncthreads();
    } else {
        mcq_exact_ext_cb_table(e.x, r_id, tid, blockDim.x, opp_tab); /* (the list does not read it: no barrier yet) */
    }
    uint32_t n[3];
    hero_compact<MCQ_XH_MAX_HANDS, false>(
        e.x.n_rp,
        [&](uint32_t rp) -> uint32_t {
            const uint32_t xy = pair_xy[rp < MCQ_XH_MAX_HANDS ? rp : 0u];
            return rp < e.x.n_rp && Kind::allowed(e, r_id, hw_tab, rp, xy & 0xFFu, xy >> 8) ? 1u : 0u;
        },
        chunk_cnt, own_list, nullptr, nullptr, n);
    const uint32_t n_own = n[2];

    const uint32_t groups = job.groups, group = blockIdx.x % groups, idx = group * blockDim.x + tid;
    const bool own = idx < n_own;
    const uint32_t hxy = pair_xy[own ? own_list[idx] : 0u], qa = hxy & 0xFFu, qb = hxy >> 8;
    typename Kind::Sums s = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    for (uint32_t board = blockIdx.x / groups; board < job.n_boards; board += job.grid / groups) {
        uint32_t pos[5];
        mcq_exact_unrank(board, e.x.b.L, e.x.b.k, pos);
        McqExactBoard bd;
        mcq_exact_hero_board(e.x.b, pos, r_id, bd);
        __syncthreads(); /* the previous completion's walk is done with keys and records */
        if (tid < e.x.m) {
            const uint32_t rp = mcq_exact_rem_pos(pos, tid);
            rem_pos[tid] = rp;
            rem_card[tid] = mcq_card(r_id[rp]);
        }
        __syncthreads();
        mcq_exact_hero_rank<W>(e, bd, tid, blockDim.x, pair_xy, rem_card, rem_pos, opp_tab, g_tab->tf, tab.tops, tab.sd, keys, recs);
        __syncthreads();
        const uint32_t mi = own ? mcq_exact_ext_m_index(e.x, pos, qa, qb) : e.x.n_pairs;
        if (mi < e.x.n_pairs) {
            McqExactAcc acc = {0, 0, 0};
            const uint32_t type = mcq_exact_hero_walk<W>(e, bd, qa, qb, mi, keys, recs, acc);
            mcq_exact_hero_add(s, acc, type);
        }
    }
    if (own) hero_flush(rows, job.row, mcq_exact_hero_row(r_id, qa, qb), s);
}

__global__ __launch_bounds__(1024) void mcq_exact_hero_kernel(const McqExactExtJob *__restrict__ jobs, const uint32_t *__restrict__ ext,
                                                              int law, unsigned long long *__restrict__ rows,
                                                              const McqTables *__restrict__ g_tab) {
    hero_body<false>(jobs, ext, law, nullptr, 0u, rows, g_tab);
}

__global__ __launch_bounds__(1024) void mcq_exact_hero_w_kernel(const McqExactExtJob *__restrict__ jobs, const uint32_t *__restrict__ ext,
                                                                const uint16_t *__restrict__ wts, uint32_t hero_w,
                                                                unsigned long long *__restrict__ rows,
                                                                const McqTables *__restrict__ g_tab) {
    hero_body<true>(jobs, ext, MCQ_LAW_UNIFORM, wts, hero_w, rows, g_tab);
}

// Preflop (mcq_exact_hero_pre.hpp): the shape of hero_body with everything indexed by D-pair.  The blocks of a group share
// the launch's slice [lo, hi) in runs of consecutive completions (the first one unranked, the others by
// mcq_exact_hero_pre_next).  Once per block the three lists are made -- `ranked` (D-pairs), `allowed` and `live` (slots of
// `ranked`).  Per completion the 1024 threads rank the slots of `ranked` (a pair that a table card touches: key 0, record
// 0), then thread t of group g owns the (g * 1024 + t)-th allowed hero hand and walks `live` with broadcast LDS reads; its
// own key waits at its own slot.  A group of n_g < 513 hands gives each hand 1024 / n_g threads (64 at most), which share
// its walk and keep sums of their own (mcq_exact_hero_pre_share).  Two barriers per completion: ranking may start only after
// the last walk, the walk only after the ranking.  The rows are shared by the launches of a call.
// W = false: twelve 32-bit sums per thread -- the host bounds the completions a block owns per launch (MCQ_XP_MAX_OWNED).
// W = true: the uniform law only; the lists' two predicates are read from ow_tab / hw_tab; a completion's 32-bit sums are
// added ONCE per completion into twelve 64-bit sums per thread, so no bound on the completions a block owns is needed.
// LDS: 97 KB of tables + 10.6 KB of keys and records + 8 KB of lists + 2.6 KB of D-pairs + 1.3 KB of range bits or 5.3 KB
// of weights.
template <bool W>
__device__ __forceinline__ void hero_pre_body(const McqExactExtJob *__restrict__ jobs, const uint32_t *__restrict__ ext, int law,
                                              const uint16_t *__restrict__ wts, uint32_t hero_w, uint32_t lo, uint32_t hi,
                                              unsigned long long *__restrict__ rows, const McqTables *__restrict__ g_tab) {
    typedef McqHeroKind<W> Kind;
    const McqExactExtJob job = jobs[blockIdx.y];
    if (blockIdx.x >= job.grid || lo >= job.n_boards) return;
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab;
    __shared__ uint16_t pair_xy[MCQ_XP_MAX_PAIRS]; /* every D-pair: qa | qb << 8 */
    __shared__ uint32_t xw[MCQ_EXT_WORDS];
    __shared__ McqExactHeroQuery xq;
    __shared__ uint8_t r_id[64];
    __shared__ McqCard d_card[64];
    __shared__ typename Kind::opp_t opp_tab[W ? MCQ_XP_MAX_PAIRS : MCQ_XP_MAX_PAIRS + 2u];
    __shared__ uint16_t allowed[MCQ_XP_MAX_PAIRS], live[MCQ_XP_MAX_PAIRS], ranked[MCQ_XP_MAX_PAIRS];
    __shared__ uint32_t chunk_cnt[3u * ((MCQ_XP_MAX_PAIRS + 63u) / 64u)];
    __shared__ uint32_t keys[MCQ_XP_MAX_PAIRS + 2u];
    __shared__ uint32_t recs[MCQ_XP_MAX_PAIRS + 2u];
    const uint32_t tid = threadIdx.x;
    exact_prologue<MCQ_XP_MAX_PAIRS>(job, ext, g_tab, tab, pair_xy, xw, r_id, hero_query(law, xq));
    const McqExactHeroQuery &e = xq;
    if (tid < e.x.b.L) d_card[tid] = mcq_card(r_id[tid]);
    const uint16_t *hw_tab = nullptr;
    if constexpr (W) {
        __shared__ uint16_t hw[MCQ_XP_MAX_PAIRS];
        hero_fold_weights(e, r_id, wts, job.row, hero_w, opp_tab, hw);
        hw_tab = hw;
    } else {
        for (uint32_t rp = tid; rp < e.x.n_rp; rp += blockDim.x) {
            const uint32_t xy = pair_xy[rp];
            opp_tab[rp] = (uint8_t)mcq_exact_ext_cbits(e.x, r_id, xy & 0xFFu, xy >> 8);
        }
    }
    __syncthreads();
    uint32_t n[3];
    hero_compact<MCQ_XP_MAX_PAIRS, true>(
        e.x.n_rp,
        [&](uint32_t rp) -> uint32_t {
            const uint32_t xy = pair_xy[rp < MCQ_XP_MAX_PAIRS ? rp : 0u];
            if (rp >= e.x.n_rp) return 0u;
            return (Kind::allowed(e, r_id, hw_tab, rp, xy & 0xFFu, xy >> 8) ? 1u : 0u) | (opp_tab[rp] != 0u ? 2u : 0u);
        },
        chunk_cnt, ranked, allowed, live, n);
    const uint32_t n_allowed = n[0], n_live = n[1], n_ranked = n[2];

    const uint32_t groups = job.groups, group = blockIdx.x % groups, first = group * blockDim.x;
    const uint32_t n_g = n_allowed > first ? (n_allowed - first < blockDim.x ? n_allowed - first : blockDim.x) : 0u;
    const uint32_t share = mcq_exact_hero_pre_share(n_g), hand = tid / share, sub = tid - hand * share;
    const bool own = hand < n_g;
    const uint32_t own_slot = own ? allowed[first + hand] : 0u;
    const uint32_t hxy = pair_xy[n_ranked ? ranked[own_slot] : 0u], qa = hxy & 0xFFu, qb = hxy >> 8;
    /* the block's run of consecutive completions: the first one unranked, the others by stepping */
    const uint32_t end = hi < job.n_boards ? hi : job.n_boards, run = mcq_exact_hero_pre_owned(end - lo, job.grid / groups);
    const uint32_t b0 = lo + (blockIdx.x / groups) * run, b1 = end - b0 < run ? end : b0 + run;
    typename Kind::Sums s = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    uint32_t pos[5];
    if (b0 < end) mcq_exact_unrank(b0, e.x.b.L, e.x.b.k, pos);
    for (uint32_t board = b0; board < b1 && b0 < end; board++) {
        if (board != b0) mcq_exact_hero_pre_next(pos, e.x.b.k);
        McqExactBoard bd;
        mcq_exact_hero_board(e.x.b, pos, r_id, bd);
        const uint64_t taken = mcq_exact_hero_pre_mask(e.x.b, pos);
        __syncthreads(); /* the previous completion's walk is done with keys and records */
        mcq_exact_hero_pre_rank<W>(e, bd, taken, tid, blockDim.x, ranked, n_ranked, pair_xy, d_card, opp_tab, g_tab->tf, tab.tops, tab.sd,
                                   keys, recs);
        __syncthreads();
        if (own && keys[own_slot] != 0u) {
            McqExactAcc acc = {0, 0, 0};
            const uint32_t type = mcq_exact_hero_pre_walk<W>(e, bd, qa, qb, own_slot, live, n_live, sub, share, keys, recs, acc);
            mcq_exact_hero_add(s, acc, type);
        }
    }
    if (own) hero_flush(rows, job.row, mcq_exact_hero_row(r_id, qa, qb), s);
}

__global__ __launch_bounds__(1024) void mcq_exact_hero_pre_kernel(const McqExactExtJob *__restrict__ jobs, const uint32_t *__restrict__ ext,
                                                                  int law, uint32_t lo, uint32_t hi,
                                                                  unsigned long long *__restrict__ rows,
                                                                  const McqTables *__restrict__ g_tab) {
    hero_pre_body<false>(jobs, ext, law, nullptr, 0u, lo, hi, rows, g_tab);
}

__global__ __launch_bounds__(1024) void mcq_exact_hero_pre_w_kernel(const McqExactExtJob *__restrict__ jobs, const uint32_t *__restrict__ ext,
                                                                    const uint16_t *__restrict__ wts, uint32_t hero_w, uint32_t lo,
                                                                    uint32_t hi, unsigned long long *__restrict__ rows,
                                                                    const McqTables *__restrict__ g_tab) {
    hero_pre_body<true>(jobs, ext, MCQ_LAW_UNIFORM, wts, hero_w, lo, hi, rows, g_tab);
}

// ---------------------------------------------------------------------------------------------- exact enumeration, per runout
// See mcq_exact_runout.hpp; the shape of mcq_exact_ext_kernel<KIND, MCQ_ROW_WAYS>, kinds 0 and 1 (LDS: the same 97 KB
// table image, pair list, range bits and per-wave rem_card / rem_pos), with flop and turn records only.  The sums of a
// completion are not folded: its owner -- a lane (kind 0), a wave after its wave sums (kind 1) -- stores the completion's
// 22 words once into the zeroed row of its slot among the record's MCQ_XR_ROWS rows.  One owner per completion and one
// completion per slot: plain stores, no atomics.
template <uint32_t KIND>
__global__ __launch_bounds__(1024) void mcq_exact_runout_kernel(const McqExactExtJob *__restrict__ jobs, const uint32_t *__restrict__ ext,
                                                                int law, unsigned long long *__restrict__ card_rows,
                                                                unsigned long long *__restrict__ pair_rows,
                                                                const McqTables *__restrict__ g_tab) {
    const McqExactExtJob job = jobs[blockIdx.y];
    if (blockIdx.x >= job.grid) return;
    constexpr uint32_t kRem = KIND == 1u ? McqExactExtBlock::kWaves : 1u;
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab;
    __shared__ uint16_t pair_xy[MCQ_EXACT_PAIRS + 2];
    __shared__ uint32_t xw[MCQ_EXT_WORDS];
    __shared__ McqExactExtQuery xq;
    __shared__ uint8_t r_id[64];
    __shared__ uint8_t cb_tab[KIND != 0u ? MCQ_XX_MAX_RP : 1u];
    __shared__ McqCard rem_card[kRem][64];
    __shared__ uint32_t rem_pos[kRem][64];
    const uint32_t lane = threadIdx.x & 63u, wib = KIND == 1u ? threadIdx.x >> 6 : 0u;
    const McqExactExtBlock s = {tab, xq, pair_xy, r_id, cb_tab, rem_card[wib], rem_pos[wib]};
    exact_ext_setup<KIND>(job, ext, g_tab, s, xw, [&](const McqQueryWords &q, const McqExtRec &er) -> const McqExactExtQuery & {
        (void)mcq_exact_runout_query(q, er, law, xq);
        return xq;
    });
    const McqExactExtQuery &e = xq;
    /* the record's rows: slots below MCQ_XR_CARD_ROWS among the card rows, the others among the pair rows */
    unsigned long long *rec_cards = card_rows + (size_t)job.row * (MCQ_XR_CARD_ROWS * MCQ_XR_WORDS);
    unsigned long long *rec_pairs = pair_rows + (size_t)job.row * (MCQ_XR_PAIR_ROWS * MCQ_XR_WORDS);

    if constexpr (KIND == 0u) {
        exact_lane_loop(job, [&](uint32_t idx) {
            McqExactAcc a = {0, 0, 0};
            uint32_t type, n_eq;
            const uint32_t slot = mcq_exact_runout_lone(e, idx, r_id, tab.sel8, g_tab->tf, tab.tops, tab.sd, a, type, n_eq);
            if (a.tot == 0u || slot >= MCQ_XR_ROWS) return; /* no weight: the row stays zero */
            ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(mcq_exact_runout_row(rec_cards, rec_pairs, slot)); /* 176-byte rows: 16-byte aligned */
#pragma unroll
            for (uint32_t w = 0; w < MCQ_XR_WORDS; w += 2u)
                dst[w / 2u] = make_ulonglong2(mcq_exact_ext_row_word(w, a.win, a.tie, a.tot, 0u, type, n_eq),
                                              mcq_exact_ext_row_word(w + 1u, a.win, a.tie, a.tot, 0u, type, n_eq));
        });
    } else {
        exact_wave_loop<MCQ_ROW_WAYS>(job, s, g_tab, [&](const uint32_t *pos, uint32_t tot, unsigned long long word) {
            const uint32_t slot = mcq_exact_runout_slot(e, r_id, pos);
            /* lane l stores word l of the row */
            if (tot != 0u && slot < MCQ_XR_ROWS && lane < MCQ_XR_WORDS) mcq_exact_runout_row(rec_cards, rec_pairs, slot)[lane] = word;
        });
    }
}

// k = 2: the record's 52 card rows from its pair rows, thread (card, word); a turn record's card rows are the
// completion rows themselves and stay as they are.
__global__ __launch_bounds__(256) void mcq_exact_runout_cards_kernel(const McqExactExtJob *__restrict__ jobs,
                                                                     unsigned long long *__restrict__ card_rows,
                                                                     const unsigned long long *__restrict__ pair_rows) {
    const McqExactExtJob job = jobs[blockIdx.y];
    const McqQueryWords q = {job.rec[0], job.rec[1], job.rec[2], job.rec[3]};
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (q.n_board() != 3u || t >= MCQ_XR_CARD_ROWS * MCQ_XR_WORDS) return;
    card_rows[(size_t)job.row * (MCQ_XR_CARD_ROWS * MCQ_XR_WORDS) + t] = mcq_exact_runout_card_word(
        pair_rows + (size_t)job.row * (MCQ_XR_PAIR_ROWS * MCQ_XR_WORDS), t / MCQ_XR_WORDS, t % MCQ_XR_WORDS);
}

}  // namespace

// ---------------------------------------------------------------------------------------------- launchers
hipError_t mcq_launch_prep(const mcq_query *d_q, uint32_t n, mcq_result *d_res, uint64_t *d_prefix, uint32_t part,
                           uint32_t n_parts, uint32_t n_cu, uint32_t split_max, hipStream_t s, uint32_t row_words) {
    if (n_parts == 0 || part >= n_parts || (row_words != 13u && row_words != 22u)) return hipErrorInvalidValue;
    if (row_words == 13u)
        hipLaunchKernelGGL(mcq_prep_kernel<13u>, dim3(1), dim3(1024), 0, s, d_q, n, d_res, d_prefix, part, n_parts, n_cu, split_max);
    else
        hipLaunchKernelGGL(mcq_prep_kernel<22u>, dim3(1), dim3(1024), 0, s, d_q, n, d_res, d_prefix, part, n_parts, n_cu, split_max);
    return hipGetLastError();
}

/* t0 / t1 (either may be null): events that take the kernel's own begin / end timestamps (hipExtLaunchKernel: read
 * from the dispatch packet's completion signal -- no marker packets in the queue around a short kernel) */
hipError_t mcq_launch_eval(int mode, const mcq_query *d_q, uint32_t n, const uint64_t *d_prefix, mcq_result *d_res,
                           uint64_t seed, uint64_t first_qid, const McqTables *d_luts, const uint8_t *d_draws,
                           const uint64_t *d_draw_off, uint32_t grid, uint32_t block, uint32_t split, uint32_t part,
                           uint32_t n_parts, hipStream_t s, hipEvent_t t0, hipEvent_t t1, uint32_t work_wpb, bool ways) {
    if ((split > 4 && split != MCQ_SPLIT_FROM_PREP) || n_parts == 0 || part >= n_parts) return hipErrorInvalidValue;
    if (mode == MCQ_MODE_REPLAY_MT19937 && split > 2) return hipErrorInvalidValue; /* its lanes take four iterations at a time */
#define MCQ_LAUNCH_EVAL_W(M, W)                                                                                     \
    do {                                                                                                            \
        if (split)                                                                                                  \
            MCQ_LAUNCH_TIMED((mcq_eval_kernel<M, true, W>), grid, block, d_q, n,     \
                                  d_prefix, d_res, seed, first_qid, d_luts, d_draws, d_draw_off, split, part, n_parts, work_wpb); \
        else                                                                                                        \
            MCQ_LAUNCH_TIMED((mcq_eval_kernel<M, false, W>), grid, block, d_q, n,    \
                                  d_prefix, d_res, seed, first_qid, d_luts, d_draws, d_draw_off, 0u, part, n_parts, work_wpb); \
    } while (0)
#define MCQ_LAUNCH_EVAL(M)                        \
    do {                                          \
        if (ways) MCQ_LAUNCH_EVAL_W(M, true);     \
        else MCQ_LAUNCH_EVAL_W(M, false);         \
    } while (0)
    if (mode == MCQ_MODE_PHILOX) MCQ_LAUNCH_EVAL(MCQ_MODE_PHILOX);
    else if (mode == MCQ_INTERNAL_MODE_UNIFORM) MCQ_LAUNCH_EVAL(MCQ_INTERNAL_MODE_UNIFORM);
    else MCQ_LAUNCH_EVAL(MCQ_MODE_REPLAY_MT19937);
#undef MCQ_LAUNCH_EVAL
#undef MCQ_LAUNCH_EVAL_W
    return hipGetLastError();
}

hipError_t mcq_launch_eval_direct(int mode, const void *work_rec, const uint32_t *work_qi, uint32_t rounds, uint32_t merge,
                                  mcq_result *res, uint64_t seed, uint64_t first_qid, const McqTables *d_luts, uint32_t grid,
                                  uint32_t *d_done, uint32_t *done_flag, uint32_t ticket, hipStream_t s, hipEvent_t t0,
                                  hipEvent_t t1, const McqDirectKarg *karg, uint32_t dev_n, uint32_t dev_lg, bool ways) {
    if (grid == 0 || rounds == 0) return hipErrorInvalidValue;
    if (karg && (uint64_t)grid * rounds * (kMaxBlock / 64) > MCQ_DIRECT_KARG_SLOTS) return hipErrorInvalidValue;
    if (karg && rounds > MCQ_DIRECT_STAGE_ROUNDS) return hipErrorInvalidValue; /* the kernel reads them in its first stage only */
    if (dev_n && (karg || work_qi || dev_lg > 4u)) return hipErrorInvalidValue;
    const uint4 *rec = static_cast<const uint4 *>(work_rec);
    static const McqDirectKarg none = {};
    McqDirectKarg dev = {}; /* queries in HBM: their number and the cut travel in the argument block */
    dev.qi[0] = dev_n;
    dev.qi[1] = dev_lg;
    const uint32_t use = dev_n ? 2u : karg ? 1u : 0u;
    const McqDirectKarg &ka = dev_n ? dev : karg ? *karg : none;
#define MCQ_LAUNCH_DIRECT(M, W)                                                                                  \
    MCQ_LAUNCH_TIMED((mcq_eval_direct_kernel<M, W>), grid, kMaxBlock, rec, work_qi, rounds, merge, res, seed, first_qid, \
                     d_luts, d_done, done_flag, ticket, use, ka)
    if (mode == MCQ_INTERNAL_MODE_UNIFORM) {
        if (ways) MCQ_LAUNCH_DIRECT(MCQ_INTERNAL_MODE_UNIFORM, true);
        else MCQ_LAUNCH_DIRECT(MCQ_INTERNAL_MODE_UNIFORM, false);
    } else {
        if (ways) MCQ_LAUNCH_DIRECT(MCQ_MODE_PHILOX, true);
        else MCQ_LAUNCH_DIRECT(MCQ_MODE_PHILOX, false);
    }
#undef MCQ_LAUNCH_DIRECT
    return hipGetLastError();
}

hipError_t mcq_launch_mt_parse(const mcq_query *d_q, uint32_t n, uint32_t seed32, uint8_t *d_draws, const uint64_t *d_draw_off,
                               mcq_result *d_res, uint32_t *d_counter, uint32_t n_cu, hipStream_t s, uint32_t row_words) {
    if (n == 0) return hipSuccess;
    uint32_t blocks = n; /* one pair of waves per query */
    if (blocks > kMtBlocksPerCu * n_cu) blocks = kMtBlocksPerCu * n_cu;
    hipLaunchKernelGGL(mcq_mt_parse_kernel, dim3(blocks), dim3(kMtBlock), 0, s, d_q, n, seed32, d_draws, d_draw_off, d_res,
                       d_counter, row_words);
    return hipGetLastError();
}

uint64_t mcq_mtb_part_words(void) { return (uint64_t)(MCQ_MTB_MAX_SEG - 1u) * kMtbJumpSplit * MCQ_MT_N; }
hipError_t mcq_launch_mt_blocks(const mcq_query *d_q, uint32_t n, uint32_t seed32, const uint32_t *d_blk_off,
                                const uint32_t *d_grp_off, uint32_t max_blocks, uint32_t *d_raw, uint32_t *d_exits, void *d_entries,
                                uint32_t *d_gword, uint32_t *d_gits, void *d_gentry, uint32_t *d_ovf, uint8_t *d_draws,
                                const uint64_t *d_draw_off, mcq_result *d_res, uint32_t *d_part, hipStream_t s) {
    if (n == 0 || max_blocks == 0) return hipSuccess;
    constexpr uint32_t kWaves = kMtbBlock / 64;
    const uint32_t max_groups = (max_blocks + MCQ_MTB_GROUP - 1u) / MCQ_MTB_GROUP;
    const dim3 per_block((max_blocks + kWaves - 1) / kWaves, n), per_group((max_groups + kWaves - 1) / kWaves, n);
    if (!d_part) { /* no jumps (MCQ_MT_JUMP=0): one work-group per query makes all its blocks, one behind the other */
        hipLaunchKernelGGL(mcq_mtb_generate_kernel, dim3(1, n), dim3(kMtbGenBlock), 0, s, d_blk_off, seed32, d_raw, d_part, 0u,
                           max_blocks, 0u);
    } else {
        constexpr uint32_t kRound = MCQ_MTB_SEG * MCQ_MTB_MAX_SEG;
        for (uint32_t base = 0; base < max_blocks; base += kRound) {
            const uint32_t left = max_blocks - base, segs = left >= kRound ? MCQ_MTB_MAX_SEG : (left + MCQ_MTB_SEG - 1u) / MCQ_MTB_SEG;
            if (segs > 1u) {
                hipLaunchKernelGGL(mcq_mtb_generate_kernel, dim3(1, n), dim3(kMtbGenBlock), 0, s, d_blk_off, seed32, d_raw, d_part,
                                   base, kMtbJumpSpan, 1u);
                hipLaunchKernelGGL(mcq_mtb_jump_kernel, dim3((segs - 1u) * kMtbJumpSplit, n), dim3(kMtbJumpBlock), 0, s, d_blk_off,
                                   d_raw, d_part, base);
            }
            hipLaunchKernelGGL(mcq_mtb_generate_kernel, dim3(segs, n), dim3(kMtbGenBlock), 0, s, d_blk_off, seed32, d_raw, d_part,
                               base, (uint32_t)MCQ_MTB_SEG, 0u);
        }
    }
    hipLaunchKernelGGL(mcq_mtb_scan_kernel, per_block, dim3(kMtbBlock), 0, s, d_q, d_blk_off, d_raw, d_exits);
    hipLaunchKernelGGL(mcq_mtb_compose_kernel, per_group, dim3(kMtbBlock), 0, s, d_q, d_blk_off, d_grp_off, d_exits, d_gword, d_gits);
    hipLaunchKernelGGL(mcq_mtb_stitch_kernel, dim3(n), dim3(64), 0, s, d_q, d_blk_off, d_grp_off, d_gword, d_gits,
                       reinterpret_cast<McqMtbEntry *>(d_gentry), d_ovf, d_res);
    hipLaunchKernelGGL(mcq_mtb_expand_kernel, per_group, dim3(kMtbBlock), 0, s, d_q, d_blk_off, d_grp_off, d_exits,
                       reinterpret_cast<const McqMtbEntry *>(d_gentry), reinterpret_cast<McqMtbEntry *>(d_entries));
    const dim3 per_parse_block((max_blocks + kMtbParseBlock / 64 - 1) / (kMtbParseBlock / 64), n);
    hipLaunchKernelGGL(mcq_mtb_parse_kernel, per_parse_block, dim3(kMtbParseBlock), 0, s, d_q, d_blk_off, d_raw,
                       reinterpret_cast<const McqMtbEntry *>(d_entries), d_ovf, d_draws, d_draw_off, d_res);
    return hipGetLastError();
}

hipError_t mcq_launch_mt_parse_ext(const mcq_query *d_q, const mcq_query_ext *d_ext, uint32_t n, uint32_t seed32, uint8_t *d_draws,
                                   const uint64_t *d_draw_off, mcq_result *d_res, uint32_t *d_counter, uint32_t n_cu, hipStream_t s,
                                   uint32_t row_words) {
    if (n == 0) return hipSuccess;
    if (row_words != 13u && row_words != 22u) return hipErrorInvalidValue;
    uint32_t blocks = (n + kMtExtBlock / 64 - 1) / (kMtExtBlock / 64);
    if (blocks > kMtExtBlocksPerCu * n_cu) blocks = kMtExtBlocksPerCu * n_cu;
    if (row_words == 13u)
        hipLaunchKernelGGL(mcq_mt_parse_ext_kernel<13u>, dim3(blocks), dim3(kMtExtBlock), 0, s, d_q, d_ext, n, seed32, d_draws,
                           d_draw_off, d_res, d_counter);
    else
        hipLaunchKernelGGL(mcq_mt_parse_ext_kernel<22u>, dim3(blocks), dim3(kMtExtBlock), 0, s, d_q, d_ext, n, seed32, d_draws,
                           d_draw_off, d_res, d_counter);
    return hipGetLastError();
}

hipError_t mcq_launch_publish(mcq_result *d_rows, mcq_result *h_rows_dev, uint64_t n_rows, uint32_t *d_done,
                              uint32_t *done_flag, uint32_t ticket, hipStream_t s, uint32_t row_bytes) {
    static_assert(sizeof(mcq_result) % 16 == 8, "13 x 8 bytes");
    if (n_rows == 0 || (n_rows & 1ull)) return hipErrorInvalidValue; /* whole 16-byte words: the caller rounds the rows up */
    const uint64_t words = n_rows * row_bytes / 16u;
    uint64_t blocks = (words + 1023u) / 1024u; /* four words per thread */
    if (blocks > kPublishMaxBlocks) blocks = kPublishMaxBlocks;
    hipLaunchKernelGGL(mcq_publish_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, reinterpret_cast<ulonglong2 *>(d_rows),
                       reinterpret_cast<ulonglong2 *>(h_rows_dev), words, d_done, done_flag, ticket);
    return hipGetLastError();
}

hipError_t mcq_launch_add_u64(uint64_t *d_dst, const uint64_t *d_src, uint64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n / 2 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > kAddMaxBlocks) blocks = kAddMaxBlocks;
    hipLaunchKernelGGL(mcq_add_u64_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, d_dst, d_src, n);
    return hipGetLastError();
}

hipError_t mcq_launch_prep_ext(const mcq_query *d_q, const mcq_query_ext *d_ext, uint32_t n, int mode, mcq_result *d_res,
                               uint64_t *d_prefix, hipStream_t s, uint32_t row_words) {
    if (row_words != 13u && row_words != 22u && row_words != 32u) return hipErrorInvalidValue;
    if (row_words == 13u)
        hipLaunchKernelGGL(mcq_prep_ext_kernel<13u>, dim3(1), dim3(1024), 0, s, d_q, d_ext, n, mode, d_res, d_prefix);
    else if (row_words == 32u)
        hipLaunchKernelGGL(mcq_prep_ext_kernel<32u>, dim3(1), dim3(1024), 0, s, d_q, d_ext, n, mode, d_res, d_prefix);
    else
        hipLaunchKernelGGL(mcq_prep_ext_kernel<22u>, dim3(1), dim3(1024), 0, s, d_q, d_ext, n, mode, d_res, d_prefix);
    return hipGetLastError();
}

hipError_t mcq_launch_ext_lists(const mcq_query *d_q, const mcq_query_ext *d_ext, uint32_t n, uint32_t lists_stride,
                                uint16_t *d_lists, uint32_t *d_cnts, hipStream_t s) {
    if (n == 0 || lists_stride == 0) return hipSuccess;
    hipLaunchKernelGGL(mcq_ext_lists_kernel, dim3(n), dim3(kListBlock), 0, s, d_q, d_ext, lists_stride, d_lists, d_cnts);
    return hipGetLastError();
}

hipError_t mcq_launch_eval_ext(int mode, const mcq_query *d_q, const mcq_query_ext *d_ext, uint32_t n,
                               const uint64_t *d_prefix, mcq_result *d_res, uint64_t seed, uint64_t first_qid,
                               const McqTables *d_luts, const uint8_t *d_draws, const uint64_t *d_draw_off,
                               const uint16_t *d_lists, const uint32_t *d_cnts, uint32_t lists_stride, uint32_t grid,
                               uint32_t block, hipStream_t s, hipEvent_t t0, hipEvent_t t1, bool ways, bool seats) {
    if (seats && (ways || mode != MCQ_MODE_PHILOX)) return hipErrorInvalidValue;
#define MCQ_LAUNCH_EXT(M, W)                                                                                        \
    MCQ_LAUNCH_TIMED((mcq_eval_ext_kernel<M, W>), grid, block, d_q, d_ext, n, d_prefix, d_res, seed, first_qid, d_luts, d_draws, \
                     d_draw_off, d_lists, d_cnts, lists_stride)
    if (mode == MCQ_MODE_PHILOX) {
        if (seats) MCQ_LAUNCH_EXT(MCQ_MODE_PHILOX, MCQ_ROW_SEATS);
        else if (ways) MCQ_LAUNCH_EXT(MCQ_MODE_PHILOX, MCQ_ROW_WAYS);
        else MCQ_LAUNCH_EXT(MCQ_MODE_PHILOX, MCQ_ROW_PLAIN);
    } else {
        if (ways) MCQ_LAUNCH_EXT(MCQ_MODE_REPLAY_MT19937, MCQ_ROW_WAYS);
        else MCQ_LAUNCH_EXT(MCQ_MODE_REPLAY_MT19937, MCQ_ROW_PLAIN);
    }
#undef MCQ_LAUNCH_EXT
    return hipGetLastError();
}

hipError_t mcq_launch_eval_ranges(const mcq_query *d_q, const uint32_t *d_seat_table, const uint32_t *d_trials,
                                  const uint16_t *d_tables, uint32_t n_tables, uint32_t *d_cum, uint32_t n, uint64_t *d_prefix, mcq_result *d_res, uint64_t seed,
                                  uint64_t first_qid, const McqTables *d_luts, uint32_t grid, uint32_t block, hipStream_t s,
                                  hipEvent_t t0, hipEvent_t t1) {
    if (n == 0 || n_tables == 0 || block > (uint32_t)kExtBlock) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mcq_ranges_tables_kernel, dim3(n_tables), dim3(kRgTabBlock), 0, s, d_tables, d_cum);
    hipLaunchKernelGGL(mcq_prep_ranges_kernel, dim3(1), dim3(1024), 0, s, d_q, d_trials, n, d_res, d_prefix);
    MCQ_LAUNCH_TIMED(mcq_eval_ranges_kernel, grid, block, d_q, d_seat_table, (const uint32_t *)d_cum, d_trials, n,
                     (const uint64_t *)d_prefix, d_res, seed, first_qid, d_luts);
    return hipGetLastError();
}

hipError_t mcq_launch_eval_ranges_hands(const mcq_query *d_q, const uint32_t *d_seat_table, const uint32_t *d_trials,
                                        const uint16_t *d_tables, uint32_t n_tables, uint32_t *d_cum, uint32_t n, uint64_t *d_prefix,
                                        mcq_result *d_res, mcq_hand_row *d_hands, uint32_t seat, uint64_t seed, uint64_t first_qid,
                                        const McqTables *d_luts, uint32_t grid, uint32_t block, hipStream_t s, hipEvent_t t0,
                                        hipEvent_t t1) {
    if (n == 0 || n_tables == 0 || block > (uint32_t)kExtBlock || !d_hands || seat >= MCQ_MAX_SEATS) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(d_hands, 0, (size_t)n * MCQ_HAND_ROWS * sizeof(mcq_hand_row), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mcq_ranges_tables_kernel, dim3(n_tables), dim3(kRgTabBlock), 0, s, d_tables, d_cum);
    hipLaunchKernelGGL(mcq_prep_ranges_kernel, dim3(1), dim3(1024), 0, s, d_q, d_trials, n, d_res, d_prefix);
    MCQ_LAUNCH_TIMED(mcq_eval_ranges_hands_kernel, grid, block, d_q, d_seat_table, (const uint32_t *)d_cum, d_trials, n,
                     (const uint64_t *)d_prefix, d_res, reinterpret_cast<unsigned long long *>(d_hands), seat, seed, first_qid,
                     d_luts);
    return hipGetLastError();
}

hipError_t mcq_launch_eval_ext_small(const McqExtSmallKarg *karg, uint32_t n, /* blocks */ mcq_result *h_res_dev, uint64_t seed,
                                     uint64_t first_qid, const McqTables *d_luts, uint32_t *d_done, uint32_t *done_flag,
                                     uint32_t ticket, hipStream_t s, hipEvent_t t0, hipEvent_t t1, bool ways) {
    if (n == 0 || n > MCQ_EXT_SMALL_BLOCKS) return hipErrorInvalidValue;
    if (ways)
        MCQ_LAUNCH_TIMED(mcq_eval_ext_small_kernel<true>, n, kExtBlock, *karg, h_res_dev, seed, first_qid, d_luts, d_done, done_flag, ticket);
    else
        MCQ_LAUNCH_TIMED(mcq_eval_ext_small_kernel<false>, n, kExtBlock, *karg, h_res_dev, seed, first_qid, d_luts, d_done, done_flag, ticket);
    return hipGetLastError();
}

hipError_t mcq_launch_showdown(const uint8_t *hands, uint32_t n_tables, uint32_t n_players, const McqTables *d_luts,
                               uint8_t *winner, uint8_t *wtype, uint32_t *keys, uint32_t *bad, uint32_t *d_done,
                               uint32_t *done_flag, uint32_t ticket, uint32_t n_cu, hipStream_t s) {
    if (n_tables == 0 || n_players < 1 || n_players > 10) return hipErrorInvalidValue;
    uint32_t grid = (n_tables + kShowBlock - 1) / kShowBlock;
    if (grid > kShowBlocksPerCu * n_cu) grid = kShowBlocksPerCu * n_cu;
    hipLaunchKernelGGL(mcq_showdown_kernel, dim3(grid), dim3(kShowBlock), 0, s, hands, n_tables, n_players, d_luts, winner,
                       wtype, keys, bad, d_done, done_flag, ticket);
    return hipGetLastError();
}

hipError_t mcq_launch_exact(const McqExactJob *d_jobs, uint32_t n_jobs, uint32_t max_grid, bool two_opp, int law,
                            mcq_result *d_rows, const McqTables *d_luts, hipStream_t s) {
    if (n_jobs == 0) return hipSuccess;
    if (n_jobs > 65535u || max_grid == 0) return hipErrorInvalidValue;
    if (two_opp)
        hipLaunchKernelGGL(mcq_exact_kernel<true>, dim3(max_grid, n_jobs), dim3(384), 0, s, d_jobs, law, d_rows, d_luts);
    else
        hipLaunchKernelGGL(mcq_exact_kernel<false>, dim3(max_grid, n_jobs), dim3(1024), 0, s, d_jobs, law, d_rows, d_luts);
    return hipGetLastError();
}

hipError_t mcq_launch_exact_ext(const McqExactExtJob *d_jobs, uint32_t n_jobs, uint32_t max_grid, uint32_t kind,
                                const uint32_t *d_ext, int law, mcq_result *d_rows, unsigned long long *d_h1,
                                const McqTables *d_luts, hipStream_t s, bool ways, bool seats) {
    if (n_jobs == 0) return hipSuccess;
    if (n_jobs > 65535u || max_grid == 0 || kind > 2u || (ways && kind == 2u) || (seats && (ways || kind == 2u)))
        return hipErrorInvalidValue;
#define MCQ_LAUNCH_XX(K, W) \
    hipLaunchKernelGGL((mcq_exact_ext_kernel<K, W>), dim3(max_grid, n_jobs), dim3(1024), 0, s, d_jobs, d_ext, law, d_rows, d_h1, d_luts)
    if (kind == 0u) {
        if (seats) MCQ_LAUNCH_XX(0u, MCQ_ROW_SEATS);
        else if (ways) MCQ_LAUNCH_XX(0u, MCQ_ROW_WAYS);
        else MCQ_LAUNCH_XX(0u, MCQ_ROW_PLAIN);
    } else if (kind == 1u) {
        if (seats) MCQ_LAUNCH_XX(1u, MCQ_ROW_SEATS);
        else if (ways) MCQ_LAUNCH_XX(1u, MCQ_ROW_WAYS);
        else MCQ_LAUNCH_XX(1u, MCQ_ROW_PLAIN);
    } else {
        MCQ_LAUNCH_XX(2u, MCQ_ROW_PLAIN);
    }
#undef MCQ_LAUNCH_XX
    return hipGetLastError();
}

hipError_t mcq_launch_exact_hero(bool preflop, bool weighted, const McqExactExtJob *d_jobs, uint32_t n_jobs, uint32_t max_grid,
                                 const uint32_t *d_ext, int law, const uint16_t *d_wts, bool hero_w, uint32_t lo, uint32_t hi,
                                 mcq_result *d_rows, const McqTables *d_luts, hipStream_t s) {
    if (n_jobs == 0) return hipSuccess;
    if (n_jobs > 65535u || max_grid == 0 || (weighted && !d_wts)) return hipErrorInvalidValue;
    if (preflop && (lo >= hi || hi - lo > MCQ_XP_MAX_OWNED)) return hipErrorInvalidValue;
    const dim3 grid(max_grid, n_jobs), block(1024);
    const uint32_t hw = hero_w ? 1u : 0u;
    unsigned long long *rows = reinterpret_cast<unsigned long long *>(d_rows);
    if (!preflop && !weighted) hipLaunchKernelGGL(mcq_exact_hero_kernel, grid, block, 0, s, d_jobs, d_ext, law, rows, d_luts);
    else if (!preflop) hipLaunchKernelGGL(mcq_exact_hero_w_kernel, grid, block, 0, s, d_jobs, d_ext, d_wts, hw, rows, d_luts);
    else if (!weighted) hipLaunchKernelGGL(mcq_exact_hero_pre_kernel, grid, block, 0, s, d_jobs, d_ext, law, lo, hi, rows, d_luts);
    else hipLaunchKernelGGL(mcq_exact_hero_pre_w_kernel, grid, block, 0, s, d_jobs, d_ext, d_wts, hw, lo, hi, rows, d_luts);
    return hipGetLastError();
}

hipError_t mcq_launch_exact_runouts(const McqExactExtJob *d_jobs, uint32_t n_jobs, uint32_t max_grid, uint32_t kind,
                                    const uint32_t *d_ext, int law, mcq_result_ways *d_cards, mcq_result_ways *d_pairs,
                                    const McqTables *d_luts, hipStream_t s) {
    if (n_jobs == 0) return hipSuccess;
    if (n_jobs > 65535u || max_grid == 0 || kind > 1u) return hipErrorInvalidValue;
    unsigned long long *cards = reinterpret_cast<unsigned long long *>(d_cards), *pairs = reinterpret_cast<unsigned long long *>(d_pairs);
    if (kind == 0u)
        hipLaunchKernelGGL(mcq_exact_runout_kernel<0u>, dim3(max_grid, n_jobs), dim3(1024), 0, s, d_jobs, d_ext, law, cards, pairs, d_luts);
    else
        hipLaunchKernelGGL(mcq_exact_runout_kernel<1u>, dim3(max_grid, n_jobs), dim3(1024), 0, s, d_jobs, d_ext, law, cards, pairs, d_luts);
    return hipGetLastError();
}

hipError_t mcq_launch_exact_runout_cards(const McqExactExtJob *d_jobs, uint32_t n_jobs, mcq_result_ways *d_cards,
                                         const mcq_result_ways *d_pairs, hipStream_t s) {
    if (n_jobs == 0) return hipSuccess;
    if (n_jobs > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mcq_exact_runout_cards_kernel, dim3((MCQ_XR_CARD_ROWS * MCQ_XR_WORDS + 255u) / 256u, n_jobs), dim3(256), 0, s,
                       d_jobs, reinterpret_cast<unsigned long long *>(d_cards), reinterpret_cast<const unsigned long long *>(d_pairs));
    return hipGetLastError();
}

hipError_t mcq_eval_occupancy(int mode, int block, int *blocks_per_cu) {
    if (mode == MCQ_MODE_PHILOX)
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, mcq_eval_kernel<MCQ_MODE_PHILOX, false, false>, block, 0);
    if (mode == MCQ_INTERNAL_MODE_UNIFORM)
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, mcq_eval_kernel<MCQ_INTERNAL_MODE_UNIFORM, false, false>,
                                                            block, 0);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, mcq_eval_kernel<MCQ_MODE_REPLAY_MT19937, false, false>, block, 0);
}

// ---------------------------------------------------------------------------------------------- exact enumeration, the matrix
// mcq_exact_matrix (mcq_exact_matrix.hpp): three kernels per launch group, one job per record (blockIdx.y);
// the jobs of a group travel in the kernel arguments.
namespace {

// (a) Ranking.  A block of 1024 threads per table completion at a time (blockIdx.x, then + gridDim.x): the word of every
// D-pair on it -- 0 = dead, else key + 1 -- into row `board` of the record's key table, `stride` words a row.  The padding
// (D-pairs from n_rp to stride, rows from n_boards to stages * MCQ_XM_STAGE) is written as dead, so the count kernel reads
// whole tiles and whole stages and tests no bound.  LDS: 97 KB of tables, one block of 16 waves per CU.
__global__ __launch_bounds__(1024) void mcq_exact_matrix_rank_kernel(const McqMatrixJobs jobs, uint32_t *__restrict__ keys,
                                                                      size_t key_words, const McqTables *__restrict__ g_tab) {
    const McqMatrixJob &job = jobs.job[blockIdx.y]; /* (the kernel arguments: scalar loads) */
    const uint32_t rows = job.stages * MCQ_XM_STAGE, stride = job.stride, tid = threadIdx.x;
    if (blockIdx.x >= rows) return;
    __shared__ __attribute__((aligned(16))) LdsTablesEval tab;
    __shared__ uint16_t pair_xy[MCQ_XH_MAX_HANDS];
    __shared__ McqMatrixQuery xq;
    __shared__ uint8_t r_id[64];
    for (uint32_t i = tid; i < MCQ_XH_MAX_HANDS; i += blockDim.x) {
        uint32_t x, y;
        mcq_exact_pair_xy(i, x, y);
        pair_xy[i] = (uint16_t)(x | (y << 8));
    }
    load_tables(tab, g_tab); /* ends with a barrier */
    if (tid == 0) {
        (void)mcq_matrix_query_build(job.q, xq); /* the host has validated it */
        mcq_matrix_r_ids(xq, r_id);
    }
    __syncthreads();
    const McqMatrixQuery &e = xq;
    uint32_t *dst = keys + (size_t)job.slot * key_words;
    for (uint32_t board = blockIdx.x; board < rows; board += gridDim.x) {
        uint32_t *row = dst + (size_t)board * stride;
        if (board >= e.n_boards) {
            for (uint32_t rp = tid; rp < stride; rp += blockDim.x) row[rp] = 0u;
            continue;
        }
        uint32_t pos[5];
        mcq_exact_unrank(board, e.b.L, e.b.k, pos);
        McqExactBoard bd;
        mcq_exact_hero_board(e.b, pos, r_id, bd);
        for (uint32_t rp = tid; rp < stride; rp += blockDim.x)
            row[rp] = rp < e.n_rp ? mcq_matrix_rank(bd, pos, r_id, pair_xy[rp], g_tab->tf, tab.tops, tab.sd) : 0u;
    }
}

// (b) Counting.  A block of 256 threads owns a tile of MCQ_XM_TILE x MCQ_XM_TILE D-pairs (row tile blockIdx.x / tiles, column
// tile blockIdx.x % tiles) and walks every completion; thread (ty, tx) of 16 x 16 holds the TH x TG = 4 x 4 counters of row
// hands ty * 4 .. + 3 and column hands tx * 4 .. + 3 in registers for the whole loop and stores them once, as uint16.
// The words travel global -> registers -> LDS in stages of MCQ_XM_STAGE completions, two LDS buffers: while a stage is
// counted the next one's two 16-byte loads per thread are in flight, they are written to the other buffer behind the
// counting, one barrier per stage.  A stage in LDS is [completion][64 row words | 64 column words], the column words with
// the dead mark already turned (mcq_matrix_col): per completion a thread reads its 4 row words and its 4 column words with
// one 16-byte LDS read each -- within a wave the row reads are 4 addresses (broadcast) and the column reads 16 consecutive
// 16-byte slots, one bank row -- and does 16 compare-and-adds.
// The tile: a flop has 19 x 19 = 361 tiles of 4 waves, 1444 waves on 1024 SIMDs; 16 counters a thread keep the kernel small
// enough in registers for every wave of a CU's share to be resident at once.  LDS: 16 KB.
constexpr uint32_t kMatrixCountBlock = (MCQ_XM_TILE / MCQ_XM_TH) * (MCQ_XM_TILE / MCQ_XM_TG);
constexpr uint32_t kMatrixStageVecs = MCQ_XM_STAGE * 2u * MCQ_XM_TILE / 4u / kMatrixCountBlock; /* 16-byte loads per thread and stage */
static_assert(MCQ_XM_TH == 4u && MCQ_XM_TG == 4u && kMatrixCountBlock == 256u, "a thread's row and column words are one uint4 each");
static_assert(kMatrixStageVecs * kMatrixCountBlock * 4u == MCQ_XM_STAGE * 2u * MCQ_XM_TILE && kMatrixCountBlock % (2u * MCQ_XM_TILE / 4u) == 0u,
              "a stage is whole loads, and a thread's loads of a stage lie in the same part of their rows");

__global__ __launch_bounds__(kMatrixCountBlock) void mcq_exact_matrix_count_kernel(const McqMatrixJobs jobs,
                                                                                  const uint32_t *__restrict__ keys, size_t key_words,
                                                                                  uint16_t *__restrict__ cnt, size_t cnt_words) {
    const McqMatrixJob &job = jobs.job[blockIdx.y]; /* (the kernel arguments: scalar loads) */
    const uint32_t stride = job.stride, tiles = stride / MCQ_XM_TILE, stages = job.stages;
    if (blockIdx.x >= tiles * tiles) return;
    __shared__ __attribute__((aligned(16))) uint32_t buf[2][MCQ_XM_STAGE][2u * MCQ_XM_TILE];
    const uint32_t tid = threadIdx.x, tx = tid % (MCQ_XM_TILE / MCQ_XM_TG), ty = tid / (MCQ_XM_TILE / MCQ_XM_TG);
    const uint32_t row0 = blockIdx.x / tiles * MCQ_XM_TILE, col0 = blockIdx.x % tiles * MCQ_XM_TILE;
    /* staging: load v of a stage covers completion (tid + v * 256) / 32 of it, part tid % 32 of its 32 16-byte pieces: the
     * first 16 are the tile's row words, the others its column words */
    constexpr uint32_t kParts = 2u * MCQ_XM_TILE / 4u;
    const uint32_t part = tid % kParts, comp0 = tid / kParts;
    const bool is_col = part >= kParts / 2u;
    const uint32_t *src = keys + (size_t)job.slot * key_words + (is_col ? col0 + (part - kParts / 2u) * 4u : row0 + part * 4u);
    uint4 v[kMatrixStageVecs];
    auto fetch = [&](uint32_t stage) {
#pragma unroll
        for (uint32_t i = 0; i < kMatrixStageVecs; i++) {
            const uint32_t comp = stage * MCQ_XM_STAGE + comp0 + i * (kMatrixCountBlock / kParts);
            v[i] = *reinterpret_cast<const uint4 *>(src + (size_t)comp * stride);
        }
    };
    auto put = [&](uint32_t b) {
#pragma unroll
        for (uint32_t i = 0; i < kMatrixStageVecs; i++) {
            uint4 w = v[i];
            if (is_col) w = make_uint4(mcq_matrix_col(w.x), mcq_matrix_col(w.y), mcq_matrix_col(w.z), mcq_matrix_col(w.w));
            *reinterpret_cast<uint4 *>(&buf[b][comp0 + i * (kMatrixCountBlock / kParts)][part * 4u]) = w;
        }
    };
    uint32_t acc[MCQ_XM_TH][MCQ_XM_TG];
#pragma unroll
    for (uint32_t a = 0; a < MCQ_XM_TH; a++)
#pragma unroll
        for (uint32_t b = 0; b < MCQ_XM_TG; b++) acc[a][b] = 0u;
    fetch(0u);
    put(0u);
    __syncthreads();
    for (uint32_t s = 0; s < stages; s++) {
        const bool more = s + 1u < stages; /* block-uniform */
        if (more) fetch(s + 1u);
        const uint32_t(*cur)[2u * MCQ_XM_TILE] = buf[s & 1u];
#pragma unroll
        for (uint32_t c = 0; c < MCQ_XM_STAGE; c++) {
            const uint4 rv = *reinterpret_cast<const uint4 *>(&cur[c][ty * MCQ_XM_TH]);
            const uint4 cv = *reinterpret_cast<const uint4 *>(&cur[c][MCQ_XM_TILE + tx * MCQ_XM_TG]);
            const uint32_t row[MCQ_XM_TH] = {rv.x, rv.y, rv.z, rv.w}, col[MCQ_XM_TG] = {cv.x, cv.y, cv.z, cv.w};
            mcq_matrix_count<MCQ_XM_TH, MCQ_XM_TG>(acc, row, col);
        }
        if (more) put((s + 1u) & 1u); /* the buffer stage s - 1 was counted from: every thread has passed the barrier behind it */
        __syncthreads();
    }
    uint16_t *dst = cnt + (size_t)job.slot * cnt_words + (size_t)(row0 + ty * MCQ_XM_TH) * stride + col0 + tx * MCQ_XM_TG;
#pragma unroll
    for (uint32_t a = 0; a < MCQ_XM_TH; a++) /* (padding rows and columns lie inside the slot: no edge test) */
        *reinterpret_cast<uint2 *>(dst + (size_t)a * stride) = make_uint2(acc[a][0] | (acc[a][1] << 16), acc[a][2] | (acc[a][3] << 16));
}

// (c) Finish: rows blockIdx.x, + gridDim.x, ... of the record's [1326][1326] matrices from its counts by D-pair
// (mcq_matrix_entry) -- every entry is written, the zeros too; tie == null: win alone.
__global__ __launch_bounds__(256) void mcq_exact_matrix_finish_kernel(const McqMatrixJobs jobs, const uint16_t *__restrict__ cnt,
                                                                      size_t cnt_words, uint16_t *__restrict__ win,
                                                                      uint16_t *__restrict__ tie) {
    const McqMatrixJob &job = jobs.job[blockIdx.y]; /* (the kernel arguments: scalar loads) */
    __shared__ McqMatrixQuery xq;
    __shared__ uint8_t r_id[64], pos_of[52];
    __shared__ uint16_t cards[MCQ_XH_ROWS], dpair[MCQ_XH_ROWS];
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        (void)mcq_matrix_query_build(job.q, xq);
        mcq_matrix_r_ids(xq, r_id);
        mcq_matrix_pos_of(xq, r_id, pos_of);
    }
    __syncthreads();
    mcq_matrix_hands(pos_of, tid, blockDim.x, cards, dpair);
    __syncthreads();
    const uint16_t *src = cnt + (size_t)job.slot * cnt_words;
    const size_t base = (size_t)job.out * MCQ_XH_ROWS * MCQ_XH_ROWS;
    for (uint32_t r = blockIdx.x; r < MCQ_XH_ROWS; r += gridDim.x)
        for (uint32_t c = tid; c < MCQ_XH_ROWS; c += blockDim.x) {
            uint32_t w, t;
            mcq_matrix_entry(xq, src, job.stride, cards, dpair, r, c, w, t);
            const size_t at = base + (size_t)r * MCQ_XH_ROWS + c;
            win[at] = (uint16_t)w;
            if (tie) tie[at] = (uint16_t)t;
        }
}

}  // namespace

hipError_t mcq_launch_exact_matrix(const McqMatrixJob *jobs, uint32_t n_jobs, uint32_t rank_grid, uint32_t finish_grid,
                                   uint32_t max_stride, uint32_t *d_keys, size_t key_words, uint16_t *d_cnt, size_t cnt_words,
                                   uint16_t *d_win, uint16_t *d_tie, const McqTables *d_luts, hipStream_t s, hipEvent_t *ev) {
    if (n_jobs == 0) return hipSuccess;
    const uint32_t tiles = max_stride / MCQ_XM_TILE;
    if (n_jobs > MCQ_XM_MAX_CHUNK || rank_grid == 0 || finish_grid == 0 || tiles == 0 || max_stride % MCQ_XM_TILE != 0u ||
        max_stride > MCQ_XM_MAX_STRIDE || cnt_words < (size_t)max_stride * max_stride || !d_win)
        return hipErrorInvalidValue;
    McqMatrixJobs d_jobs;
    __builtin_memset(&d_jobs, 0, sizeof d_jobs);
    __builtin_memcpy(d_jobs.job, jobs, n_jobs * sizeof(McqMatrixJob));
    hipEvent_t t0 = ev ? ev[0] : nullptr, t1 = ev ? ev[1] : nullptr;
    MCQ_LAUNCH_TIMED(mcq_exact_matrix_rank_kernel, dim3(rank_grid, n_jobs), 1024, d_jobs, d_keys, key_words, d_luts);
    t0 = ev ? ev[2] : nullptr, t1 = ev ? ev[3] : nullptr;
    MCQ_LAUNCH_TIMED(mcq_exact_matrix_count_kernel, dim3(tiles * tiles, n_jobs), kMatrixCountBlock, d_jobs, d_keys, key_words, d_cnt,
                     cnt_words);
    t0 = ev ? ev[4] : nullptr, t1 = ev ? ev[5] : nullptr;
    MCQ_LAUNCH_TIMED(mcq_exact_matrix_finish_kernel, dim3(finish_grid, n_jobs), 256, d_jobs, d_cnt, cnt_words, d_win, d_tie);
    return hipGetLastError();
}
