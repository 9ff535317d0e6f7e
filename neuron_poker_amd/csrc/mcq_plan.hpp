// mcq_plan.hpp -- LAUNCH PLANS: what turns "these records on this many CUs" into a grid, a block size, a cut and a path.
// Plain functions of integers and records, no HIP and no context: mcq_host.cpp and mcq_kernels.hip compile them into the
// library, tests/hostsim_plan for the host, where tests/test_plan_host.py holds them to the Python statements the GPU
// tests build their batches around (tests/ext_grid.py, tests/exact_grid.py, tests/test_eval_kernel_matrix.py).
//
//   geometry         grid, block, cut and working waves of the sliced kernels (bulk, extended, ranges)
//   small-query cut  2^lg waves per query of the one-launch kernel in its device mode, from the query count alone
//   one-launch ext   does a batch of extended queries fit mcq_eval_ext_small_kernel, and which block runs what
//   ranges price     a record's estimated whole trials per iteration (scheduling only)
//   exact plans      one job per record of the enumeration kernels
//
// The cost axis (mcq_axis.hpp), the one-launch work layout (mcq_layout.hpp) and mcq_pick_split (mcq_device.hpp) are the
// other three pieces; no entry point plans inline.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mcq_device.hpp"
#include "mcq_exact_ext.hpp"
#include "mcq_exact_hero_pre.hpp"
#include "mcq_ranges.hpp"

// ---------------------------------------------------------------------------------------------- geometry
#define MCQ_PLAN_BLOCK 1024u /* threads per block of the evaluation kernels */
#define MCQ_PLAN_WAVES (MCQ_PLAN_BLOCK / 64u)

/* what a plan reads of the device and of the tuning knobs (mcq_ctx::knobs) */
struct McqPlanKnobs {
    uint32_t n_cu = 0;
    uint32_t occ[3] = {1, 1, 1}; /* resident MCQ_PLAN_BLOCK-thread blocks per CU of the eval kernels (by internal mode) */
    uint32_t grid_cap = 0;   /* sliced launches (mcq_eval_kernel, mcq_eval_ext_kernel) get at most this many blocks; 0: no cap (MCQ_GRID_CAP, tests) */
    uint32_t split_max = 4;  /* finest cut of a task for small batches: 16 >> split_max iterations per lane (MCQ_SPLIT_MAX) */
    uint32_t load_waves = 16; /* waves per block that load the table image when fewer take work (MCQ_LOAD_WAVES) */
};
struct McqGeometry {
    uint32_t grid, block, split; /* split: the bulk kernel's cut of a task (mcq_pick_split); 0 for the other kernels */
    uint32_t work_wpb; /* the bulk kernel: waves per block that take work when more are launched to load the tables; 0: all */
};
/* a launch whose total task count is known (host entry) or unknown (0).  bulk: mcq_eval_kernel, which takes a cut and
 * idle loading waves; max_tasks (bulk): the most tasks of one query, 0 = unknown */
static inline McqGeometry mcq_plan_geometry(const McqPlanKnobs &k, int mode, uint64_t total_tasks, bool bulk = false,
                                            uint64_t max_tasks = 0) {
    const uint32_t full = k.n_cu * k.occ[mode];
    McqGeometry g = {0u, MCQ_PLAN_BLOCK, 0u, 0u};
    if (total_tasks == 0) {
        g.grid = k.grid_cap && full > k.grid_cap ? k.grid_cap : full;
        return g;
    }
    if (bulk) { /* small batches are cut finer, see mcq_pick_split */
        g.split = mcq_pick_split(total_tasks, max_tasks ? max_tasks : total_tasks, k.n_cu, k.split_max);
        total_tasks <<= g.split;
    }
    /* one block per CU (the LDS tables allow no more); few tasks are spread over all CUs with fewer waves per
     * block: 98 tasks of a single 100k query -> 98 one-wave blocks, 1024 tasks -> 256 four-wave blocks */
    uint64_t wpb = (total_tasks + (uint64_t)k.n_cu - 1) / (uint64_t)k.n_cu;
    if (wpb < 1) wpb = 1;
    if (wpb > MCQ_PLAN_WAVES) wpb = MCQ_PLAN_WAVES;
    const uint64_t blocks = (total_tasks + wpb - 1) / wpb;
    g.grid = (uint32_t)(blocks < (uint64_t)k.n_cu ? blocks : (wpb == MCQ_PLAN_WAVES ? full : (uint64_t)k.n_cu));
    /* the block brings 97 KB of tables into LDS before anything else happens: more waves than take work shorten
     * that (six 16-byte loads per lane with 16 waves, one round trip, instead of 24 with four) */
    uint64_t launch = wpb < k.load_waves ? k.load_waves : wpb;
    if (bulk && launch != wpb) g.work_wpb = (uint32_t)wpb;
    else launch = wpb < 4 ? 4 : wpb;
    g.block = (uint32_t)(64 * launch);
    /* tests: fewer blocks than the work asks for, so that a wave's slice is many tasks of one query (streams are keyed by
     * query id and iteration: the tallies do not depend on the number of blocks) */
    if (k.grid_cap && g.grid > k.grid_cap) g.grid = k.grid_cap;
    return g;
}

// ---------------------------------------------------------------------------------------------- the small-query cut
/* n small queries for mcq_eval_direct_kernel's device mode: about 16 waves per CU in all, at most eight per query (a
 * sixteenth wave steps over fifteen iterations' words), sixteen waves per block, the blocks in whole rounds */
struct McqSmallCut { uint32_t lg, grid, rounds; }; /* 2^lg waves per query */
static inline McqSmallCut mcq_plan_small_cut(uint64_t n, uint32_t n_cu, uint32_t split_max) {
    McqSmallCut c = {0u, 0u, 0u};
    while (c.lg < 3u && (n << (c.lg + 1u)) <= 16ull * n_cu) c.lg++;
    if (split_max < c.lg) c.lg = split_max;
    const uint64_t blocks = ((n << c.lg) + 15u) / 16u;
    c.grid = (uint32_t)(blocks < (uint64_t)n_cu ? blocks : (uint64_t)n_cu);
    c.rounds = (uint32_t)((blocks + c.grid - 1u) / c.grid);
    return c;
}

// ---------------------------------------------------------------------------------------------- one-launch extended path
/* a few extended queries in one launch (mcq_eval_ext_small_kernel): the queries and their extension records travel in
 * the kernel arguments */
#define MCQ_EXT_SMALL_Q 8u      /* queries per launch (8 x 320 B of kernel arguments) */
#define MCQ_EXT_SMALL_LISTS 6u  /* candidate lists per query that fit the block's LDS (6 x 2704 x 2 B) */
#define MCQ_EXT_SMALL_TASKS 64u /* wave tasks per query */
#define MCQ_EXT_SMALL_BLOCKS 32u /* blocks per launch: a query is cut into parts of 4, 8 or 16 wave tasks, whatever fits */
struct McqExtSmallKarg {
    uint32_t q[MCQ_EXT_SMALL_Q][4];
    uint32_t ext[MCQ_EXT_SMALL_Q][76];
    uint32_t blk[MCQ_EXT_SMALL_BLOCKS]; /* block b: mcq_ext_small_pack; its row goes to row b of the result buffer */
};
/* a block's word: query | part << 8 | parts << 16 | waves that take tasks << 24 */
struct McqExtSmallBlock { uint32_t query, part, parts, wpb; };
MCQ_HD uint32_t mcq_ext_small_pack(const McqExtSmallBlock &b) { return b.query | (b.part << 8) | (b.parts << 16) | (b.wpb << 24); }
MCQ_HD McqExtSmallBlock mcq_ext_small_unpack(uint32_t blk) {
    return McqExtSmallBlock{blk & 0xFFu, (blk >> 8) & 0xFFu, (blk >> 16) & 0xFFu, blk >> 24};
}
/* does a batch fit: n queries, lists_stride = the most candidate lists and most_tasks = the most wave tasks of one */
static inline bool mcq_ext_small_fits(size_t n, uint32_t lists_stride, uint32_t most_tasks) {
    return n <= MCQ_EXT_SMALL_Q && lists_stride <= MCQ_EXT_SMALL_LISTS && most_tasks <= MCQ_EXT_SMALL_TASKS;
}
struct McqExtSmallPlan {
    uint32_t wpb, n_blocks;                     /* working waves per block; blocks of the launch */
    uint32_t first_block[MCQ_EXT_SMALL_Q + 1];  /* query i owns blocks first_block[i] .. first_block[i + 1] */
};
/* tasks[i]: the wave tasks of query i of a batch that fits (so sixteen waves per block always suffice: 8 x 64 / 16 = 32
 * blocks) -> the plan and blk[0 .. n_blocks) */
static inline McqExtSmallPlan mcq_ext_small_plan(const uint32_t *tasks, uint32_t n, uint32_t *blk) {
    McqExtSmallPlan p;
    p.wpb = 4; /* working waves per block: the fewest with which the launch's blocks suffice */
    for (; p.wpb < 16u; p.wpb <<= 1) {
        uint32_t need = 0;
        for (uint32_t i = 0; i < n; i++) need += tasks[i] > p.wpb ? (tasks[i] + p.wpb - 1u) / p.wpb : 1u;
        if (need <= MCQ_EXT_SMALL_BLOCKS) break;
    }
    p.n_blocks = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t parts = tasks[i] > p.wpb ? (tasks[i] + p.wpb - 1u) / p.wpb : 1u;
        p.first_block[i] = p.n_blocks;
        for (uint32_t part = 0; part < parts; part++) blk[p.n_blocks++] = mcq_ext_small_pack(McqExtSmallBlock{i, part, parts, p.wpb});
    }
    p.first_block[n] = p.n_blocks;
    return p;
}

// ---------------------------------------------------------------------------------------------- the ranges price
/* weight of the hands of a table that are clear of a set B of table cards, by inclusion and exclusion:
 * total - sum_{c in B} (weight of the hands that hold c) + sum_{c < c' in B} w[{c, c'}].
 * The first pass, per table: wc[c] = the weight of the hands that hold card c, wc[52] = the total */
#define MCQ_RG_WITH_CARD_STRIDE 53u
static inline void mcq_ranges_with_card(const uint16_t *w, uint32_t *wc) {
    for (uint32_t c = 0; c < MCQ_RG_WITH_CARD_STRIDE; c++) wc[c] = 0;
    for (uint32_t b = 1; b < 52u; b++)
        for (uint32_t a = 0; a < b; a++) {
            const uint32_t v = w[MCQ_HAND_INDEX(a, b)];
            wc[a] += v;
            wc[b] += v;
            wc[52] += v;
        }
}
#define MCQ_RG_REFUSED_TABLE 1u /* a seat names a table that is not there */
#define MCQ_RG_REFUSED_CLEAR 2u /* a seat's table has no hand of positive weight clear of the table cards */
struct McqRangesPrice {
    uint32_t price;                /* estimated whole trials per iteration, 1 .. MCQ_RG_MAX_PRICE; 0: refused */
    uint32_t refused, seat, table; /* why (MCQ_RG_REFUSED_*), and where */
};
/* The price of a valid record (mcq_ranges_query_valid) whose seat s draws from table seat_table_row[s]; with_card: the
 * first pass of all n_tables tables.  P(no two seats share a card) as if the pairs of seats collided independently, and
 * a pair with probability sum_c P(s holds c) P(s' holds c) (a shared hand counts twice: an overestimate, bounded below). */
static inline McqRangesPrice mcq_ranges_price(const uint16_t *tables, size_t n_tables, const uint32_t *with_card,
                                              const McqQueryWords &qw, const uint32_t *seat_table_row) {
    double held[MCQ_MAX_SEATS * 52u]; /* per seat: P(its hand holds card c), given that it is clear of the table */
    for (uint32_t s = 0; s < qw.n_players(); s++) {
        const uint32_t t = seat_table_row[s];
        if (t >= n_tables) return McqRangesPrice{0u, MCQ_RG_REFUSED_TABLE, s, t};
        const uint32_t *wc = with_card + (size_t)t * MCQ_RG_WITH_CARD_STRIDE;
        const uint16_t *w = tables + (size_t)t * MCQ_HAND_ROWS;
        uint64_t blocked = 0; /* weight of the hands that hold a table card */
        for (uint32_t k = 0; k < qw.n_board(); k++) {
            const uint32_t ck = qw.card(2u + k);
            blocked += wc[ck];
            for (uint32_t j = 0; j < k; j++) {
                const uint32_t cj = qw.card(2u + j);
                blocked -= w[MCQ_HAND_INDEX((cj < ck ? cj : ck), (cj < ck ? ck : cj))];
            }
        }
        if (blocked >= wc[52]) return McqRangesPrice{0u, MCQ_RG_REFUSED_CLEAR, s, t};
        const double clear = (double)(wc[52] - blocked);
        const uint64_t bm = mcq_ranges_board_mask(qw);
        for (uint32_t c = 0; c < 52u; c++) {
            uint64_t with_c = (bm >> c) & 1u ? 0u : wc[c];
            if (with_c)
                for (uint32_t k = 0; k < qw.n_board(); k++) {
                    const uint32_t ck = qw.card(2u + k);
                    with_c -= w[MCQ_HAND_INDEX((c < ck ? c : ck), (c < ck ? ck : c))];
                }
            held[s * 52u + c] = (double)with_c / clear;
        }
    }
    double accept = 1.0;
    for (uint32_t s = 1; s < qw.n_players(); s++)
        for (uint32_t r = 0; r < s; r++) {
            double hit = 0.0;
            for (uint32_t c = 0; c < 52u; c++) hit += held[s * 52u + c] * held[r * 52u + c];
            accept *= hit < 0.99 ? 1.0 - hit : 0.01;
        }
    const double est = accept > 1.0 / MCQ_RG_MAX_PRICE ? 1.0 / accept : (double)MCQ_RG_MAX_PRICE;
    return McqRangesPrice{(uint32_t)(est + 0.5), 0u, 0u, 0u};
}

// ---------------------------------------------------------------------------------------------- the exact plans
/* exact enumeration (n_players <= 3), any number of queries per launch: one job per query (blockIdx.y), all of the same
 * kind -- two opponents or fewer; every job adds into its zeroed row d_rows[job.row] */
struct McqExactJob {
    uint32_t rec[4];                        /* the 16-byte query record */
    uint32_t n_boards, slices, row, grid;   /* table completions, cuts of the first-opponent loop, result row, blocks that work */
};
static inline void mcq_exact_plan(const mcq_query *q, uint32_t row, uint32_t n_cu, McqExactJob *job) {
    __builtin_memcpy(job->rec, q, 16);
    const uint32_t L = 50u - q->n_board, k = 5u - q->n_board;
    job->n_boards = mcq_exact_binom(L, k);
    job->row = row;
    if (q->n_players == 3) {
        /* few completions (turn, river): cut the first-opponent loop so that every wave has work */
        uint32_t slices = 1;
        while (slices < 64u && (uint64_t)job->n_boards * slices < 6ull * n_cu * 4ull) slices *= 2u;
        const uint64_t units = (uint64_t)job->n_boards * slices;
        job->slices = slices;
        job->grid = (uint32_t)((units + 5u) / 6u < n_cu ? (units + 5u) / 6u : n_cu);
    } else {
        job->slices = 1u;
        job->grid = (job->n_boards + 15u) / 16u < n_cu ? (job->n_boards + 15u) / 16u : n_cu;
    }
}
/* exact enumeration of extended queries (mcq_exact_ext.hpp): one job per query, one launch per kind = random opponents
 * (0, 1, 2); the extension records lie in device-visible memory, 76 words each.  Kinds 0 and 1 add into the zeroed row
 * d_rows[job.row], kind 2 into the zeroed per-first-hand sums d_h1[h1_off + 12 * hand] (hand < C(L, 2)). */
struct McqExactExtJob {
    uint32_t rec[4];                      /* the 16-byte query record */
    uint32_t ext, n_boards, row, grid;    /* its extension record, table completions, result row, blocks that work */
    uint32_t groups, h1_off, pad_[2];     /* kind 2: blocks per completion (1024 first hands each), offset of its sums */
};
/* plan of one job (L = |R|, the cards the opponents are dealt from) -> its grid */
static inline uint32_t mcq_exact_ext_plan(const mcq_query *q, uint32_t ext, uint32_t row, uint32_t kind, uint32_t L,
                                          uint32_t h1_off, uint32_t n_cu, McqExactExtJob *job) {
    __builtin_memcpy(job->rec, q, 16);
    const uint32_t k = 5u - q->n_board, n_rp = L * (L - 1u) / 2u;
    job->ext = ext;
    job->n_boards = mcq_exact_binom(L, k);
    job->row = row;
    job->h1_off = h1_off;
    job->groups = 1u;
    if (kind == 0u) {
        const uint32_t blocks = (job->n_boards + 1023u) / 1024u;
        job->grid = blocks < n_cu ? blocks : n_cu;
    } else if (kind == 1u) {
        const uint32_t blocks = (job->n_boards + 15u) / 16u;
        job->grid = blocks < n_cu ? blocks : n_cu;
    } else {
        job->groups = (n_rp + 1023u) / 1024u;
        uint32_t per = n_cu / job->groups;
        if (per < 1u) per = 1u;
        if (per > job->n_boards) per = job->n_boards;
        job->grid = per * job->groups;
    }
    return job->grid;
}
/* hero-range enumeration (mcq_exact_hero.hpp, preflop: mcq_exact_hero_pre.hpp): one job per query, L = |D|, n_allowed = its
 * allowed hero hands (> 0); d_rows holds zeroed [MCQ_HAND_ROWS] mcq_result rows per query, job->row = the query's index.
 * preflop: the completions go out in launches of `slice`, each over [lo, hi) with hi - lo <= slice, all adding into the same
 * rows; the plan returns 0 when a block would own more completions per launch than a thread's 32-bit sums allow
 * (MCQ_XP_MAX_OWNED; the 64-bit sums of the weighted kernel need no bound, the plan is the same).  Postflop: one launch,
 * slice, lo and hi are not read. */
static inline uint32_t mcq_exact_hero_plan(bool preflop, const mcq_query *q, uint32_t ext, uint32_t row, uint32_t L,
                                           uint32_t n_allowed, uint32_t n_cu, uint32_t slice, McqExactExtJob *job) {
    __builtin_memcpy(job->rec, q, 16);
    job->ext = ext;
    job->n_boards = mcq_exact_binom(L, 5u - q->n_board);
    job->row = row;
    job->h1_off = 0u;
    job->groups = (n_allowed + 1023u) / 1024u;
    uint32_t per = n_cu / job->groups;
    if (per < 1u) per = 1u;
    if (preflop && per > slice) per = slice;
    if (per > job->n_boards) per = job->n_boards;
    job->grid = per * job->groups;
    /* preflop, a thread's 32-bit sums: the completions one block owns in a launch */
    if (preflop && (slice == 0u || mcq_exact_hero_pre_owned(slice, per) > MCQ_XP_MAX_OWNED)) return 0u;
    return job->grid;
}
