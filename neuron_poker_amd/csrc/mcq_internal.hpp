// mcq_internal.hpp -- launch functions shared between mcq_kernels.hip and mcq_host.cpp (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcq.h"
#include "mcq_plan.hpp"
#include "mcq_tally.hpp" /* MCQ_DIRECT_TASKS_LIMIT */

struct McqTables;

#define MCQ_INTERNAL_MODE_UNIFORM 2 /* MCQ_MODE_PHILOX with the context's dealing law set to MCQ_LAW_UNIFORM */

/* resident blocks per CU of the bulk evaluation kernel of a mode at `block` threads (McqPlanKnobs::occ) */
hipError_t mcq_eval_occupancy(int mode, int block, int *blocks_per_cu);

hipError_t mcq_launch_prep(const mcq_query *d_q, uint32_t n, mcq_result *d_res, uint64_t *d_prefix, uint32_t part,
                           uint32_t n_parts, uint32_t n_cu, uint32_t split_max, hipStream_t s,
                           uint32_t row_words = 13 /* 64-bit words per result row: 22 for mcq_result_ways rows */);
hipError_t mcq_launch_eval(int mode, const mcq_query *d_q, uint32_t n, const uint64_t *d_prefix, mcq_result *d_res,
                           uint64_t seed, uint64_t first_qid, const McqTables *d_luts, const uint8_t *d_draws,
                           const uint64_t *d_draw_off, uint32_t grid, uint32_t block, uint32_t split, uint32_t part,
                           uint32_t n_parts, hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr, uint32_t work_wpb = 0,
                           bool ways = false /* d_res holds mcq_result_ways rows: the instantiation that splits the ties */);
/* exact enumeration: the jobs are planned by mcq_exact_plan, mcq_exact_ext_plan (one launch per kind) and mcq_exact_hero_plan
 * (mcq_plan.hpp) */
hipError_t mcq_launch_exact_ext(const McqExactExtJob *d_jobs, uint32_t n_jobs, uint32_t max_grid, uint32_t kind,
                                const uint32_t *d_ext, int law, mcq_result *d_rows, unsigned long long *d_h1,
                                const McqTables *d_luts, hipStream_t s,
                                bool ways = false /* kinds 0 and 1: d_rows holds zeroed mcq_result_ways rows */,
                                bool seats = false /* kind 0: d_rows holds zeroed mcq_result_seats rows */);
/* weighted: a weight per hand, uniform law (law is not read); d_wts holds 2 * MCQ_HAND_ROWS uint16 per query -- the opponent's
 * table, then the hero's, which is read only with hero_w (else every hand of his classes weighs 1).  n_allowed is then
 * counted from the hero's folded table. */
hipError_t mcq_launch_exact_hero(bool preflop, bool weighted, const McqExactExtJob *d_jobs, uint32_t n_jobs, uint32_t max_grid,
                                 const uint32_t *d_ext, int law, const uint16_t *d_wts, bool hero_w, uint32_t lo, uint32_t hi,
                                 mcq_result *d_rows, const McqTables *d_luts, hipStream_t s);
/* the hand-against-hand matrix (mcq_exact_matrix.hpp): one job per record, validated by the host, at most MCQ_XM_MAX_CHUNK
 * of them per call: they travel in the kernel arguments (512 B), so a call leaves nothing behind that a later call on
 * another stream could overwrite.  Three launches.  A job's
 * scratch is slot `slot` of d_keys (key_words 32-bit words per slot: at least stages * MCQ_XM_STAGE rows of `stride` words)
 * and of d_cnt (cnt_words 16-bit words per slot: at least stride * stride); its matrices are number `out` of d_win / d_tie
 * ([MCQ_HAND_ROWS][MCQ_HAND_ROWS] uint16 each; d_tie may be null).  rank_grid blocks rank a job's completions and
 * finish_grid blocks write its rows; ev (or null): six events, a pair of timestamps per kernel in launch order. */
struct McqMatrixJob {
    mcq_matrix_query q;                   /* the 16-byte record */
    uint32_t out, slot, stride, stages;   /* mcq_matrix_stride, mcq_matrix_stages of the record */
};
#define MCQ_XM_MAX_CHUNK 16u
struct McqMatrixJobs {
    McqMatrixJob job[MCQ_XM_MAX_CHUNK];
};
hipError_t mcq_launch_exact_matrix(const McqMatrixJob *jobs /* host */, uint32_t n_jobs, uint32_t rank_grid, uint32_t finish_grid,
                                   uint32_t max_stride, uint32_t *d_keys, size_t key_words, uint16_t *d_cnt, size_t cnt_words,
                                   uint16_t *d_win, uint16_t *d_tie, const McqTables *d_luts, hipStream_t s, hipEvent_t *ev);
/* per-runout enumeration (mcq_exact_runout.hpp): flop and turn records with at most one random opponent, jobs planned by
 * mcq_exact_ext_plan (kind 0 or 1, job->row = the record's index); d_cards holds 52 and d_pairs MCQ_HAND_ROWS zeroed
 * mcq_result_ways rows per record.  The second launch takes the jobs of both kinds and fills the card rows of the flop
 * records from their pair rows. */
hipError_t mcq_launch_exact_runouts(const McqExactExtJob *d_jobs, uint32_t n_jobs, uint32_t max_grid, uint32_t kind,
                                    const uint32_t *d_ext, int law, mcq_result_ways *d_cards, mcq_result_ways *d_pairs,
                                    const McqTables *d_luts, hipStream_t s);
hipError_t mcq_launch_exact_runout_cards(const McqExactExtJob *d_jobs, uint32_t n_jobs, mcq_result_ways *d_cards,
                                         const mcq_result_ways *d_pairs, hipStream_t s);
hipError_t mcq_launch_exact(const McqExactJob *d_jobs, uint32_t n_jobs, uint32_t max_grid, bool two_opp, int law,
                            mcq_result *d_rows, const McqTables *d_luts, hipStream_t s);
/* hands / winner / wtype / keys: device-visible memory (pinned host memory or HBM), 16-byte aligned and padded to whole
 * tiles of 256 tables; *bad is set when a hand is not seven distinct ids < 52; ticket != 0: the last block raises
 * *done_flag behind a system-scope release (d_done: a zeroed device word) */
hipError_t mcq_launch_showdown(const uint8_t *hands, uint32_t n_tables, uint32_t n_players, const McqTables *d_luts,
                               uint8_t *winner, uint8_t *wtype, uint32_t *keys, uint32_t *bad, uint32_t *d_done,
                               uint32_t *done_flag, uint32_t ticket, uint32_t n_cu, hipStream_t s);
/* a few extended queries in one launch (mcq_eval_ext_small_kernel, planned by mcq_ext_small_plan): n_blocks rows come back */
hipError_t mcq_launch_eval_ext_small(const McqExtSmallKarg *karg, uint32_t n_blocks, mcq_result *h_res_dev, uint64_t seed,
                                     uint64_t first_qid, const McqTables *d_luts, uint32_t *d_done, uint32_t *done_flag,
                                     uint32_t ticket, hipStream_t s, hipEvent_t t0, hipEvent_t t1,
                                     bool ways = false /* one mcq_result_ways row per block */);
hipError_t mcq_launch_prep_ext(const mcq_query *d_q, const mcq_query_ext *d_ext, uint32_t n, int mode, mcq_result *d_res,
                               uint64_t *d_prefix, hipStream_t s, uint32_t row_words = 13);
/* production mode of the extended queries: lays out the candidate lists (lists_stride per query, MCQ_EXT_LIST_STRIDE
 * uint16 entries each) and their lengths */
hipError_t mcq_launch_ext_lists(const mcq_query *d_q, const mcq_query_ext *d_ext, uint32_t n, uint32_t lists_stride,
                                uint16_t *d_lists, uint32_t *d_cnts, hipStream_t s);
hipError_t mcq_launch_eval_ext(int mode, const mcq_query *d_q, const mcq_query_ext *d_ext, uint32_t n,
                               const uint64_t *d_prefix, mcq_result *d_res, uint64_t seed, uint64_t first_qid,
                               const McqTables *d_luts, const uint8_t *d_draws, const uint64_t *d_draw_off,
                               const uint16_t *d_lists, const uint32_t *d_cnts, uint32_t lists_stride, uint32_t grid,
                               uint32_t block, hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr,
                               bool ways = false /* d_res holds mcq_result_ways rows (prepared with row_words = 22) */,
                               bool seats = false /* production mode: mcq_result_seats rows (row_words = 32) */);
/* a weighted range per seat (mcq_ranges.hpp), three launches: the prepared tables (d_tables: n_tables x MCQ_HAND_ROWS
 * uint16 -> d_cum: n_tables x MCQ_RG_CUM_STRIDE uint32), rows and cost prefix (d_prefix: n + 1 words), the evaluation
 * (d_seat_table: n x 10 table numbers, all below n_tables for the seats of a record; mcq_result_seats rows).  d_trials: n
 * words, the host's estimate of each record's whole trials per iteration (1 .. MCQ_RG_MAX_PRICE): scheduling only */
hipError_t mcq_launch_eval_ranges(const mcq_query *d_q, const uint32_t *d_seat_table, const uint32_t *d_trials,
                                  const uint16_t *d_tables, uint32_t n_tables, uint32_t *d_cum, uint32_t n, uint64_t *d_prefix, mcq_result *d_res, uint64_t seed,
                                  uint64_t first_qid, const McqTables *d_luts, uint32_t grid, uint32_t block, hipStream_t s,
                                  hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
/* ... with the watched seat's tally per hand (mcq_hands.hpp; mcq_eval_ranges_hands_kernel): d_hands, n x MCQ_HAND_ROWS
 * rows, is zeroed on the stream first; seat < n_players of every record */
hipError_t mcq_launch_eval_ranges_hands(const mcq_query *d_q, const uint32_t *d_seat_table, const uint32_t *d_trials,
                                        const uint16_t *d_tables, uint32_t n_tables, uint32_t *d_cum, uint32_t n, uint64_t *d_prefix,
                                        mcq_result *d_res, mcq_hand_row *d_hands, uint32_t seat, uint64_t seed, uint64_t first_qid,
                                        const McqTables *d_luts, uint32_t grid, uint32_t block, hipStream_t s,
                                        hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
/* host-buffer calls with few rows: d_rows[0..n_rows) -> pinned host memory (device address h_rows_dev), d_rows zeroed,
 * then *done_flag = ticket; n_rows even (buffers hold the odd row's neighbour), d_done a zeroed device word */
hipError_t mcq_launch_publish(mcq_result *d_rows, mcq_result *h_rows_dev, uint64_t n_rows, uint32_t *d_done,
                              uint32_t *done_flag, uint32_t ticket, hipStream_t s, uint32_t row_bytes = sizeof(mcq_result));
/* dst[i] += src[i], i < n (tally matrices of two shards on one device, both 16-byte aligned) */
hipError_t mcq_launch_add_u64(uint64_t *d_dst, const uint64_t *d_src, uint64_t n, hipStream_t s);
/* parity mode: one wave per query parses np.random.seed(seed32 + i)'s MT19937 stream into d_draws (+ passes into the
 * result rows); d_counter must be zero (the prep kernel leaves one behind the cost prefix) */
hipError_t mcq_launch_mt_parse(const mcq_query *d_q, uint32_t n, uint32_t seed32, uint8_t *d_draws, const uint64_t *d_draw_off,
                               mcq_result *d_res, uint32_t *d_counter, uint32_t n_cu, hipStream_t s, uint32_t row_words = 13);
/* ... for few long queries (mcq_mt_blocks.hpp): the state blocks of a query side by side.  d_blk_off[q] .. d_blk_off[q + 1]:
 * the query's blocks in d_raw (624 state words each), d_exits (MCQ_MTB_LANES words each), d_entries (8 B each); max_blocks = the most
 * blocks of one query; d_grp_off likewise for the query's groups of MCQ_MTB_GROUP blocks in d_gword / d_gits (MCQ_MTB_LANES
 * words each) and d_gentry (8 B each); d_ovf[n].  A query whose stream does not end within its blocks gets passes = UINT64_MAX.  The
 * rows' passes must be zero (the prep kernel). */
hipError_t mcq_launch_mt_blocks(const mcq_query *d_q, uint32_t n, uint32_t seed32, const uint32_t *d_blk_off,
                                const uint32_t *d_grp_off, uint32_t max_blocks, uint32_t *d_raw, uint32_t *d_exits, void *d_entries,
                                uint32_t *d_gword, uint32_t *d_gits, void *d_gentry, uint32_t *d_ovf, uint8_t *d_draws,
                                const uint64_t *d_draw_off, mcq_result *d_res,
                                uint32_t *d_part /* n x mcq_mtb_part_words() words: the segments' start states by jump-ahead;
                                                    null: one work-group per query makes all its blocks */,
                                hipStream_t s);
uint64_t mcq_mtb_part_words(void); /* per query */
/* ... and for extended queries (mcq_mt_ext.hpp); d_counter zero (mcq_prep_ext_kernel leaves one behind its prefix); a
 * query whose range cannot be dealt gets passes = UINT64_MAX */
hipError_t mcq_launch_mt_parse_ext(const mcq_query *d_q, const mcq_query_ext *d_ext, uint32_t n, uint32_t seed32, uint8_t *d_draws,
                                   const uint64_t *d_draw_off, mcq_result *d_res, uint32_t *d_counter, uint32_t n_cu, hipStream_t s,
                                   uint32_t row_words = 13);
/* small queries, one launch and nothing else: work_rec / work_qi (the work laid out wave by wave, see the kernel), res
 * and done_flag may be pinned host memory (device-visible); d_done: a zeroed device word */
#define MCQ_DIRECT_IDLE 0xFFFFFFFFu
#define MCQ_DIRECT_KARG_SLOTS 128u /* one-launch path: the work of a launch this small travels in the kernel arguments */
struct McqDirectKarg {
    uint32_t rec[MCQ_DIRECT_KARG_SLOTS][4]; /* per wave slot: the query record (16 B) */
    uint32_t qi[MCQ_DIRECT_KARG_SLOTS];     /* per wave slot: the query index or MCQ_DIRECT_IDLE */
};
hipError_t mcq_launch_eval_direct(int mode, const void *work_rec, const uint32_t *work_qi, uint32_t rounds, uint32_t merge,
                                  mcq_result *res, uint64_t seed, uint64_t first_qid, const McqTables *d_luts, uint32_t grid,
                                  uint32_t *d_done, uint32_t *done_flag, uint32_t ticket, hipStream_t s, hipEvent_t t0,
                                  hipEvent_t t1, const McqDirectKarg *karg /* or null: read work_rec / work_qi */,
                                  uint32_t dev_n = 0 /* != 0: work_rec is the caller's mcq_query[dev_n] in HBM, work_qi null: */,
                                  uint32_t dev_lg = 0 /* every query 2^dev_lg waves; validated on the device */,
                                  bool ways = false /* res holds mcq_result_ways rows */);
