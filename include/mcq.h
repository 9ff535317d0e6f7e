/*
 * mcq.h -- C ABI of libmcq_hip.so: the MI355X (gfx950) Monte-Carlo poker-equity engine.
 *
 * This is the drop-in boundary for ONE path of jaronlong52/neuron_poker: the equity query
 *   tools/montecarlo_python.py:401-406  get_equity(player_cards, table_cards, players, runs) -> float
 *   tools/montecarlo_python.py:191-252  MonteCarlo.run_montecarlo(...) -> (equity, winTypesDict)
 * which gym_env/env.py:75-81 selects once and calls at gym_env/env.py:249-262.  The reference has no C ABI
 * of its own (its native variant is a pybind11 module, tools/montecarlo_cpp/pymontecarlo.cpp:21-23, with the
 * same four-argument call); the functions below are what a Python binding for this path binds instead --
 * neuron_poker_amd/montecarlo_hip.py does so through ctypes, and INTEGRATION.md shows the stub.
 *
 * Plain C: pointers and sizes only, no C++ or torch types.  All functions return MCQ_OK (0) or a negative
 * MCQ_E* code and never throw or abort; mcq_last_error() returns a thread-local description of the last
 * failure.  Card id c = 4*rank + suit with rank = index in "23456789TJQKA", suit = index in "CDHS"
 * (tools/hand_evaluator.py:5-6; the deck order of tools/montecarlo_python.py:114-119 is ascending c).
 */
#ifndef MCQ_H
#define MCQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define MCQ_API __attribute__((visibility("default")))
#else
#define MCQ_API
#endif

#define MCQ_VERSION_MAJOR 0
#define MCQ_VERSION_MINOR 5
#define MCQ_VERSION_PATCH 0

/* error codes */
#define MCQ_OK 0
#define MCQ_EINVAL (-1)  /* bad argument: card out of range, duplicate card, n_players not in [1,10], ... */
#define MCQ_EDEVICE (-2) /* HIP runtime failure; mcq_last_error() carries the HIP error string */
#define MCQ_ENOMEM (-3)  /* host or device allocation failed */
#define MCQ_EBUSY (-4)   /* another call is running on this context (or mcq_multi object): one call in flight per context */

/* random-number front ends (the deal -> evaluate -> tally body is shared) */
#define MCQ_MODE_PHILOX 0         /* production: counter-based streams, Philox4x32-10 keyed MWC64X (MCQ-CTR v5) */
#define MCQ_MODE_REPLAY_MT19937 1 /* parity: query i replays np.random.seed((seed + first_query_id + i) mod 2^32)
                                     exactly as tools/montecarlo_python.py consumes it -> bit-exact tallies */

/* dealing law of MCQ_MODE_PHILOX (mcq_set_dealing_law); the parity mode always follows the reference */
#define MCQ_LAW_REFERENCE 0 /* default: tools/montecarlo_python.py's law incl. its index bias (:170, :188) */
#define MCQ_LAW_UNIFORM 1   /* opt-in: every remaining card equally likely -- what tools/montecarlo_cython.pyx:188
                               and tools/montecarlo_cpp/Montecarlo.cpp:296-312 deal */

/* One equity query (16 bytes, no pointers).  Mirrors the arguments of get_equity
 * (tools/montecarlo_python.py:401): hero's two cards, 0/3/4/5 known table cards, players, runs. */
typedef struct mcq_query {
    uint8_t hole[2];     /* hero's cards */
    uint8_t board[5];    /* known table cards, first n_board entries used */
    uint8_t n_board;     /* 0..5 */
    uint8_t n_players;   /* hero + opponents, 1..10 (gym_env/env.py:249 passes sum(alive)) */
    uint8_t reserved[3]; /* must be 0 */
    uint32_t runs;       /* iterations (maxRuns); exactly this many are executed, no wall-clock cut-off */
} mcq_query;

/* Per-query tallies (104 bytes, unsigned integers only).
 * Reference's wins (montecarlo_python.py:223-229, ties go to hero: hand_evaluator.py:23) = win + tie
 * = sum(by_type); equity = (win + tie) / runs (montecarlo_python.py:243).
 * by_type order = HighCard, Pair, TwoPair, ThreeOfAKind, Straight, Flush, FullHouse, FoufOfAKind [sic],
 * StraightFlush (hand_evaluator.py:92-115): hero's hand type in the iterations he wins.
 * passes = opponent-deal attempts (montecarlo_python.py:168). */
typedef struct mcq_result {
    uint64_t runs;
    uint64_t passes;
    uint64_t win; /* hero strictly best */
    uint64_t tie; /* hero best together with at least one opponent (credited to hero by the reference) */
    uint64_t by_type[9];
} mcq_result;

/* Per-query tallies with the ties split by how many hands share the pot (176 bytes).  `r` is exactly what
 * mcq_eval_batch writes for the same (query, seed, query id, mode, dealing law).  tie_ways[k - 2] counts the iterations in
 * which hero is best together with k - 1 opponents, k = 2..10: sum(tie_ways) == r.tie, and tie_ways[k - 2] == 0 for
 * k > n_players.  The reference credits a tied pot to hero in full (equity = (win + tie) / runs); hero's expected SHARE of
 * the pot is
 *     (r.win + sum_k tie_ways[k - 2] / k) / r.runs.
 * "Equal" means equal ranking key, the reference's own comparison with its quirks (hand_evaluator.py:9-24): a board that
 * plays for everybody does not always tie every hand there.  All counters are integers and add across shards. */
typedef struct mcq_result_ways {
    mcq_result r;
    uint64_t tie_ways[9];
} mcq_result_ways;

/* Per-SEAT tallies of an extended query (256 bytes): what every hand of the query is worth, from ONE run of the
 * iterations -- one random stream, so the shares add up to one pot.  Seat 0 is the hero, seats 1..n_known are
 * mcq_query_ext.known[0..] in the order of original_player_card_list, the seats after them are the random or ranged
 * opponents in dealing order; seats at or above n_players are all zero.  Per iteration, with best = the greatest ranking
 * key among the n_players hands and k = the number of hands holding it, each of those k seats gets
 *     win += (k == 1),  tie += (k > 1),  share += MCQ_SHARE_UNIT / k
 * so the pot share of seat s is seat[s].share / (MCQ_SHARE_UNIT * runs) and sum_s seat[s].share == MCQ_SHARE_UNIT * runs
 * exactly.  "Equal" means equal ranking key, as for mcq_result_ways.  All counters are integers and add across shards and
 * calls.  runs and passes are what mcq_eval_batch_ext writes. */
#define MCQ_SHARE_UNIT 2520u /* lcm(1..10): a pot split k ways gives each hand 2520 / k units, exactly */
typedef struct mcq_seat {
    uint64_t win;   /* this hand strictly best */
    uint64_t tie;   /* this hand best together with at least one other */
    uint64_t share; /* sum of MCQ_SHARE_UNIT / k over the iterations in which it is best */
} mcq_seat;
typedef struct mcq_result_seats {
    uint64_t runs, passes;
    mcq_seat seat[10];
} mcq_result_seats;

/* Optional extension of a query (304 bytes) for the rest of run_montecarlo's arguments:
 * ghost_cards (tools/montecarlo_python.py:206-208), any number of further known hands (collusion players, :133-163),
 * the hero or any known hand given as a SET of preflop classes instead of two cards (:136-148), and opponents
 * restricted to a range (:165-181 with :36-112).  A range is a 169-bit set of classes; the bit of a class is how
 * get_two_short_notation (:24-34) names two cards: suited -> 13*min+max, off-suit -> 13*max+min, pair -> 14*rank
 * (rank = index in "23456789TJQKA").  "Every class" = all 169 bits set.
 * The known hands are dealt in the order of original_player_card_list: hero, known[0], known[1], ...; a hand
 * given as a range is drawn from the deck as it is at that point (:136-148) -- it may take a card that a LATER hand
 * names, which then simply is not in the deck any more (the reference's try/except, :154-161). */
#define MCQ_MAX_KNOWN 9
typedef struct mcq_known_hand {
    uint8_t cards[2];   /* the hand, when is_range == 0 */
    uint8_t is_range;   /* 1: drawn from `range` every iteration, cards ignored */
    uint8_t reserved;   /* must be 0 */
    uint32_t range[6];
} mcq_known_hand;       /* 28 bytes */

typedef struct mcq_query_ext {
    uint8_t ghost[2];      /* two cards taken out of the deck, 0xFF 0xFF = none */
    uint8_t hero_is_range; /* 1: mcq_query.hole is ignored, hero's hand is drawn from hero_range every iteration */
    uint8_t n_known;       /* further known hands after the hero, 0..MCQ_MAX_KNOWN; they count in n_players */
    uint32_t opp_range[6];
    uint32_t hero_range[6];
    mcq_known_hand known[MCQ_MAX_KNOWN];
} mcq_query_ext;           /* 304 bytes */

typedef struct mcq_ctx mcq_ctx;

/* Number of HIP devices visible, or a negative MCQ_E* code. */
MCQ_API int mcq_device_count(void);

/* Create an engine bound to HIP device `device` (one context per GPU / per process rank).  Owns its stream,
 * device and pinned staging buffers and lookup tables until mcq_destroy.  Not re-entrant: one call in flight
 * per context -- create one per thread (they are cheap: a stream, a table image, staging buffers that grow on demand).
 * The library checks it: an entry point called while another call is running on the same context returns MCQ_EBUSY
 * and touches nothing.  Returns NULL on failure (see mcq_last_error). flags must be 0. */
MCQ_API mcq_ctx *mcq_create(int device, int flags);
MCQ_API void mcq_destroy(mcq_ctx *ctx);

/* Evaluate n queries held in HOST memory; blocks until out[0..n) is written.  The caller owns q and out.
 * Query i uses query id first_query_id + i, so a batch split into shards (other ranks, other calls) with
 * the matching first_query_id gives bit-identical per-query tallies.  All queries are validated first;
 * on MCQ_EINVAL nothing is launched and out is untouched.
 * MCQ_MODE_PHILOX: batches of small queries (at most 8192 iterations each -- the reference asks for 1000,
 * gym_env/env.py:22) cost ONE kernel launch: the kernel takes the records from its arguments (up to eight queries) or
 * from pinned host memory and stores the finished rows to pinned host memory, no copy, prep or zeroing launches around
 * it, and the call returns when a flag the kernel raises there is seen (about 19 us for one 1000-run query); larger
 * queries are priced on the host and sliced over the whole GPU.  MCQ_MODE_REPLAY_MT19937: numpy's MT19937 stream of every
 * query is walked on the GPU -- a pair of waves per query for batches; for a call of at most 64 long queries the 624-word
 * state blocks of a query are generated in segments side by side (start states by jump-ahead) and parsed side by side
 * (one 100 000-run query: 0.16-0.33 ms; environment switches MCQ_MT_BLOCKS, MCQ_MT_JUMP: INTEGRATION.md). */
MCQ_API int mcq_eval_batch(mcq_ctx *ctx, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id, int mode,
                   mcq_result *out);

/* n == 1 convenience: exactly get_equity's arguments after card-string conversion. */
MCQ_API int mcq_eval_one(mcq_ctx *ctx, const mcq_query *q, uint64_t seed, int mode, mcq_result *out);

/* mcq_eval_batch with one mcq_query_ext per query (host buffers).  A range that cannot be dealt from the cards
 * left (the reference would loop forever) gives MCQ_EINVAL after a bounded number of attempts.
 * MCQ_MODE_PHILOX deals the reference's law without its re-draw loops: per range, a list of the ordered card pairs
 * the range allows is laid out once per query, a trial picks one of them with one random word and is accepted iff
 * both cards are still in the deck (and the second is not the deck's highest card, which the reference's index
 * range excludes) -- `passes` counts these trials, not the reference's.  Streams (MCQ-CTR v5x): as mcq_eval_batch,
 * sixteen iterations each, but two for a query that draws from a list and has at most 8192 iterations.
 * Up to eight queries of at most 8192 iterations (six candidate lists) per call take ONE kernel launch: the call
 * pattern of the reference's agents, one ranged query per decision -- 25 us per call.
 * MCQ_MODE_PHILOX follows MCQ_LAW_REFERENCE only: on a context set to MCQ_LAW_UNIFORM it gives MCQ_EINVAL. */
MCQ_API int mcq_eval_batch_ext(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, uint64_t seed,
                       uint64_t first_query_id, int mode, mcq_result *out);

/* mcq_eval_batch_ext writing mcq_result_ways rows: out[i].r is bit for bit what mcq_eval_batch_ext writes for the same
 * arguments, and tie_ways[k - 2] counts the iterations in which hero is best together with k - 1 OTHER hands -- further
 * known hands, hands drawn from a range and random opponents alike, each compared by its ranking key (a known hand that
 * lost a card to an earlier ranged hand, montecarlo_python.py:154-161, is evaluated with the cards it names, as the
 * credited tallies evaluate it).  Every contract of mcq_eval_batch_ext holds: both modes, validation first and MCQ_EINVAL
 * leaves out untouched, MCQ_EBUSY, the undealable range, the refusal under MCQ_LAW_UNIFORM, sharding by first_query_id,
 * the one-launch path for up to eight small queries. */
MCQ_API int mcq_eval_batch_ext_ways(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, uint64_t seed,
                                    uint64_t first_query_id, int mode, mcq_result_ways *out);

/* mcq_eval_batch_ext writing mcq_result_seats rows: every hand's win, tie and pot share from the same iterations.  The
 * streams are those of mcq_eval_batch_ext (MCQ-CTR v5x keyed by (seed, first_query_id + i), same draws, same acceptance),
 * so the hero's seat is pinned to the mcq_eval_batch_ext_ways row of the same arguments: runs, passes, seat[0].win and
 * seat[0].tie equal that row's runs, passes, win and tie, and
 *     seat[0].share == MCQ_SHARE_UNIT * win + sum_k (MCQ_SHARE_UNIT / k) * tie_ways[k - 2].
 * A known hand that lost a card to an earlier ranged hand is evaluated with the cards it names, as there.  Every contract
 * of mcq_eval_batch_ext holds: validation first and MCQ_EINVAL leaves out untouched, MCQ_EBUSY, the undealable range, the
 * refusal under MCQ_LAW_UNIFORM, sharding by first_query_id.
 * MCQ_MODE_PHILOX only: MCQ_MODE_REPLAY_MT19937 gives MCQ_EINVAL -- the reference has no per-seat number to be bit-exact
 * against, and the parity walk for rows of this width is not built.  Every call takes the general path (prep, candidate
 * lists, evaluation kernel); the one-launch path for small queries has no per-seat form. */
MCQ_API int mcq_eval_batch_ext_seats(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, uint64_t seed,
                                     uint64_t first_query_id, int mode, mcq_result_seats *out);

/* Parity mode coupled to numpy's GLOBAL random state, as consecutive reference calls are: the n
 * queries consume ONE MT19937 stream in order.  mt_key[624] / *mt_pos are numpy's state words and position
 * (np.random.get_state()[1], [2]); on return they hold the state after the last query, so
 * np.random.set_state(...) leaves numpy exactly where the reference's own calls would have left it. */
MCQ_API int mcq_eval_batch_numpy_stream(mcq_ctx *ctx, const mcq_query *q, size_t n, uint32_t *mt_key, uint32_t *mt_pos,
                                mcq_result *out);

/* Same computation with queries and results RESIDENT IN HBM: d_queries -> mcq_query[n], d_results ->
 * mcq_result[n] (overwritten), both device pointers on this context's device; hip_stream is the hipStream_t
 * to launch on (NULL = HIP's null stream, as everywhere in HIP).  Asynchronous: returns after enqueueing,
 * no host synchronisation once the context's scratch is large enough (first call / larger n allocate).
 * MCQ_MODE_PHILOX only.  Invalid queries cannot be rejected up front here: their result has runs = 0 and
 * passes = UINT64_MAX. */
MCQ_API int mcq_eval_batch_device(mcq_ctx *ctx, const void *d_queries, size_t n, uint64_t seed, uint64_t first_query_id,
                          void *d_results, void *hip_stream);

/* mcq_eval_batch_device for SMALL queries -- at most 8192 iterations each, the reference's own call pattern (1000 runs,
 * gym_env/env.py:22) -- in ONE kernel launch: no pricing kernel in front, no atomics; every query is owned by a few
 * waves of one block and its finished row is stored once.  Same arguments, same tallies (the RNG streams are keyed by
 * query id and iteration, not by the schedule).  A query with more than 8192 iterations is NOT evaluated here: like an
 * invalid one it gets runs = 0, passes = UINT64_MAX.  Asynchronous on hip_stream; can be captured into a HIP graph after
 * one ordinary call on the context. */
MCQ_API int mcq_eval_batch_device_small(mcq_ctx *ctx, const void *d_queries, size_t n, uint64_t seed, uint64_t first_query_id,
                                        void *d_results, void *hip_stream);

/* mcq_eval_batch / mcq_eval_batch_device writing mcq_result_ways rows (the split-pot tallies above); every contract of
 * those two entries holds: validation first and MCQ_EINVAL touches nothing (host entry), MCQ_EBUSY, an invalid device query
 * gets runs = 0, passes = UINT64_MAX and zeros behind them, sharding by first_query_id, the context's dealing law, kernel
 * timing.  The host entry takes both modes and keeps the one-launch path for small batches (parity mode always walks
 * the streams with a pair of waves per query).  The device entry (MCQ_MODE_PHILOX, asynchronous) cannot see the queries:
 * it prices them on the device and runs the evaluation kernel, cut finer for up to 1024 small queries, whatever their
 * size; d_results -> mcq_result_ways[n].
 * Extended queries have their own split-pot entries, mcq_eval_batch_ext_ways and mcq_exact_batch_ext_ways (below).  The
 * plain exact enumeration, the extended one with two random opponents and mcq_multi_* have no split-pot form. */
MCQ_API int mcq_eval_batch_ways(mcq_ctx *ctx, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id, int mode,
                                mcq_result_ways *out);
MCQ_API int mcq_eval_batch_device_ways(mcq_ctx *ctx, const void *d_queries, size_t n, uint64_t seed, uint64_t first_query_id,
                                       void *d_results, void *hip_stream);

/* Showdown with the same device evaluator (tools/hand_evaluator.py:9-24 get_winner / eval_best_hand):
 * hands = n_tables x n_players x 7 card ids (host); winner[t] = index of the best hand (first of equals),
 * winner_type[t] = its by_type index, keys (optional, n_tables x n_players) = the 32-bit ranking keys: a
 * greater key is a stronger hand, equal keys tie; MCQ_KEY_TYPE(key) is the hand's by_type index. */
#define MCQ_KEY_TYPE(key) (((key) >> 28) - (((key) >> 28) >= 6u ? 1u : 0u))
MCQ_API int mcq_showdown(mcq_ctx *ctx, const uint8_t *hands, size_t n_tables, int n_players, uint8_t *winner,
                 uint8_t *winner_type, uint32_t *keys);

/* One share of a batch whose ITERATIONS are split over several devices (few large queries).  Every query
 * is cut at task boundaries (1024 iterations) into n_parts contiguous ranges; this call evaluates range `part` of
 * every query under the same streams (seed, first_query_id + i) an unsplit call uses, so the rows of all parts add
 * up -- runs included -- to exactly what mcq_eval_batch returns.  MCQ_MODE_PHILOX only. */
MCQ_API int mcq_eval_batch_part(mcq_ctx *ctx, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id,
                                uint32_t part, uint32_t n_parts, mcq_result *out);

/* Exact equity by exhaustive enumeration (what tools/montecarlo_cpp/Test.cpp:176-217 approximates with
 * 1 % bands): every opponent hand and every completion of the table, weighted as the dealing law `law` (MCQ_LAW_*)
 * deals them -- for MCQ_LAW_REFERENCE the exact distribution of tools/montecarlo_python.py:121-189, index bias
 * included.  n_players 1..3; q[i].runs is ignored.  out[i]: runs = total weight, win / tie / by_type = weight of
 * the outcomes (integers; equity = (win + tie) / runs exactly), passes = 0.  Preflop heads-up = 2.1e9 hand
 * evaluations, three players preflop = 1.2e12 pair comparisons. */
MCQ_API int mcq_exact_batch(mcq_ctx *ctx, const mcq_query *q, size_t n, int law, mcq_result *out);

/* Exact enumeration of EXTENDED queries (SURVEY 8f-3 with 8f-2): hand against hand(s), ghost cards, opponents holding a
 * range.  Accepted: hero given as two cards, 0..9 further known hands each given as two cards (is_range == 0), optional
 * ghost cards, 0, 1 or 2 random opponents (n_players - 1 - n_known) drawn from opp_range, both laws.  Refused with
 * MCQ_EINVAL, nothing launched: whatever mcq_eval_batch_ext refuses, hero_is_range, a known hand given as a range, more
 * than two random opponents, and a range that cannot be dealt on some branch of positive probability.  A hero range is
 * an outer sum over the hero's hands -- out of reach preflop, and postflop, heads-up, the business of
 * mcq_exact_batch_hero_range below, which shares the ranking of the opponent's hands among all hero hands; ranged known
 * hands (the reference's pop-by-value quirk, montecarlo_python.py:154-161) are left out on purpose.
 * MCQ_LAW_REFERENCE: every ordered pair (A, B) of the current deck is equally likely provided A != B, B is not the
 * deck's highest card and class(A, B) is allowed; A is dealt, then B if B < A, else the card that follows B
 * (montecarlo_python.py:165-181); a table card is never the highest card left.  MCQ_LAW_UNIFORM: every allowed
 * unordered hand still in the deck and every table completion equally likely.
 * prob[i] is always filled.  weights (may be NULL) gets integer weights as mcq_exact_batch writes them (runs = total
 * weight, passes = 0, prob = weight / runs) whenever one common total exists: without a range, or with at most one
 * random opponent.  With a range and two random opponents the second opponent's normaliser depends on the first
 * opponent's hand; that row of weights is zeroed.  Deterministic: sums in integers per first opponent hand, combined
 * on the host in a fixed order.  A record that restricts nothing gives mcq_exact_batch's weights bit for bit. */
typedef struct mcq_exact_prob {
    double win;        /* P(hero strictly best) */
    double tie;        /* P(hero best together with at least one other hand; credited to hero, as the reference does) */
    double by_type[9]; /* P(hero wins or ties holding hand type t); sums to win + tie */
} mcq_exact_prob;      /* 88 bytes */
MCQ_API int mcq_exact_batch_ext(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                                mcq_exact_prob *prob, mcq_result *weights);

/* The same enumeration with the ties split by how many hands share the pot, for records with AT MOST ONE random
 * opponent (hand against known hands; one opponent, ranged or not): prob[i].p is what mcq_exact_batch_ext returns,
 * prob[i].tie_ways[k - 2] = P(hero is best together with k - 1 other hands), k = 2..10, and hero's exact pot share is
 * p.win + sum_k tie_ways[k - 2] / k.  weights (may be NULL) is always defined here -- one random opponent at most means
 * one common total -- as mcq_result_ways rows: r as mcq_exact_batch_ext's weights, sum(tie_ways) == r.tie exactly.
 * Refused with MCQ_EINVAL, nothing launched: whatever mcq_exact_batch_ext refuses, and TWO random opponents (the
 * per-first-hand normalisers of that enumeration would each need nine more sums). */
typedef struct mcq_exact_prob_ways {
    mcq_exact_prob p;
    double tie_ways[9];
} mcq_exact_prob_ways; /* 160 bytes */
MCQ_API int mcq_exact_batch_ext_ways(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                                     mcq_exact_prob_ways *prob, mcq_result_ways *weights);

/* The ALL-IN case, exact and per seat: records with NO random opponent (n_players == 1 + n_known, 2..10 hands, every hand
 * given as two cards, optional ghost cards, 0/3/4/5 table cards, both laws).  Every table completion (at most
 * C(48, 5) = 1 712 304, each of weight 0 or 1) is ranked for every hand: weights[i].runs = total weight, passes = 0,
 * seat[s].win and seat[s].tie in weight units, seat[s].share in weight x MCQ_SHARE_UNIT units -- the exact pot share of
 * seat s is seat[s].share / (MCQ_SHARE_UNIT * runs).  Seat 0's win and tie are mcq_exact_batch_ext_ways's weights, and
 * because the deck and the completion weights do not depend on the order of the hands, seat s equals the hero columns of
 * the record with hand s rotated to the front.
 * Refused with MCQ_EINVAL, nothing launched: whatever mcq_exact_batch_ext refuses, and any record with a random opponent
 * (one random opponent is enumerated per seat by mcq_exact_batch_ext_seats below; two are by neither entry). */
MCQ_API int mcq_exact_batch_seats(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                                  mcq_result_seats *weights);

/* The same rows for records with AT MOST ONE random opponent (n_players - 1 - n_known is 0 or 1), drawn from opp_range,
 * restricted or not: whatever mcq_exact_batch_ext_ways accepts.  Seat order as mcq_eval_batch_ext_seats: seat 0 the hero,
 * seats 1..n_known the known hands, seat 1 + n_known the random opponent; seats at or above n_players are zero.
 * weights[i] as mcq_exact_batch_seats writes it: runs = the total weight (one random opponent at most means one common
 * total), passes = 0, seat[s].win and seat[s].tie in weight units, seat[s].share in weight x MCQ_SHARE_UNIT units, and
 * sum_s seat[s].share == MCQ_SHARE_UNIT * runs exactly.  Seat 0's win and tie are mcq_exact_batch_ext_ways's weights.  The
 * cards the opponent is dealt from do not depend on the order of the known hands, so known seat s still equals the hero
 * columns of the record with hand s rotated to the front.  A record without a random opponent gives
 * mcq_exact_batch_seats's row bit for bit; a batch may mix the two shapes.
 * Refused with MCQ_EINVAL, nothing launched, weights untouched: whatever mcq_exact_batch_ext refuses (a hero range, a
 * ranged known hand, a range that cannot be dealt, a bad law among them), and TWO random opponents: with a range they
 * have no common total, and without one their weights are kept per first hand, so each first hand would need the sums
 * of every seat. */
MCQ_API int mcq_exact_batch_ext_seats(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                                      mcq_result_seats *weights);

/* Exact RANGE against RANGE, postflop and heads-up: every hand of the hero's range from ONE enumeration per record.
 * Accepted: ext[i].hero_is_range == 1 with hero_range (q[i].hole is ignored), n_known == 0, n_players == 2 -- one random
 * opponent drawn from opp_range, restricted or not --, 3, 4 or 5 table cards, optional ghost cards, both laws.
 * D = the 52 cards minus table and ghost.  For every hand {a < b} of D whose class is in hero_range,
 * rows[i * MCQ_HAND_ROWS + MCQ_HAND_INDEX(a, b)] is bit for bit the weights row mcq_exact_batch_ext writes for the same
 * record with the hero given as those two cards (runs = total weight, passes = 0; under MCQ_LAW_REFERENCE the opponent's
 * index bias on the deck without the hero's cards and the rule that a table card is never the highest card left
 * included); every other row is zero.  Heads-up pot share of that hand: (win + tie / 2) / runs.
 * agg[i] (agg may be NULL) = sum_h w_h x_h / runs_h / sum_h w_h over the allowed hands, x = win, tie, by_type[t], combined
 * on the host in ascending row order; w_h = how often the law deals hero that hand: 1 under MCQ_LAW_UNIFORM, and
 * 2 - [b is the highest card of D] under MCQ_LAW_REFERENCE (montecarlo_python.py:136-148: the ordered pairs (A, B) with B
 * not the deck's highest card, the hand leaves by value) -- what mcq_eval_batch_ext with hero_is_range == 1 converges to.
 * Refused with MCQ_EINVAL, rows and agg untouched: whatever mcq_eval_batch_ext refuses, hero_is_range == 0, n_known != 0,
 * n_players != 2, fewer than three table cards (preflop every hero hand meets C(50, 5) completions), a bad law, more
 * than MCQ_HERO_RANGE_MAX_BATCH records, no allowed hero hand in D -- all before anything is launched -- and an allowed
 * hero hand against which the opponent's range cannot be dealt (mcq_exact_batch_ext's "cannot be dealt on some branch of
 * positive probability"; seen as a row without weight, before anything is copied to the caller).
 * Deterministic: integer sums per hero hand.  Each record costs MCQ_HAND_ROWS * sizeof(mcq_result) = 138 KB of rows. */
#define MCQ_HAND_ROWS 1326u /* C(52, 2) */
#define MCQ_HAND_INDEX(a, b) /* a < b card ids */ ((b) * ((b) - 1u) / 2u + (a))
#define MCQ_HERO_RANGE_MAX_BATCH 1024u
MCQ_API int mcq_exact_batch_hero_range(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                                       mcq_result *rows /* [n][MCQ_HAND_ROWS] */, mcq_exact_prob *agg /* [n], may be NULL */);

/* Exact range against range with WEIGHTED HANDS, postflop and heads-up: mcq_exact_batch_hero_range with a weight per
 * two-card hand on both sides -- "calls with AQo half of the time", a reach probability per combo, "AhKh but not AsKs" --
 * in place of the in-or-out of a preflop class.  Weights are integers 0..MCQ_COMBO_WEIGHT_MAX; a caller with probabilities
 * scales them (only the ratios matter).
 * Accepted: exactly what mcq_exact_batch_hero_range accepts -- hero_is_range == 1, n_known == 0, n_players == 2, 3, 4 or 5
 * table cards, optional ghost cards, at most MCQ_HERO_RANGE_MAX_BATCH records.
 * The law is always MCQ_LAW_UNIFORM, so there is no law argument: the reference's law tests the class of the drawn index
 * pair (A, B) and then deals "the card after B", and a weight per dealt hand has no meaning there.
 * Definitions.  D = the 52 cards minus table and ghost cards, k = 5 - n_board.  Both tables hold MCQ_HAND_ROWS entries per
 * record, indexed by MCQ_HAND_INDEX(a, b):
 *   eff_opp(g)  = opp_weights[i][MCQ_HAND_INDEX(g)]                      if class(g) is in opp_range,  else 0
 *   eff_hero(h) = hero_weights ? hero_weights[i][MCQ_HAND_INDEX(h)] : 1  if class(h) is in hero_range, else 0
 * The class sets stay in force; "every class" in both sets leaves the weights alone to define the ranges.  Entries of
 * either table for a hand that holds a table or ghost card are ignored (they need not be zero).
 * Rows.  A hero hand h of D is allowed iff eff_hero(h) > 0; the rows of all other hands are zero.  For an allowed hand,
 * with T over the k-subsets of D minus h and g over the two-card hands of D minus h minus T:
 *   runs       = sum_T sum_g eff_opp(g)                     (at most 1081 * 990 * 65535, about 7.0e10)
 *   win        = the same sum over the g that lose to h on T,   tie = over the g level with h
 *   by_type[t] = the part of win + tie in which h makes hand type t,   passes = 0
 * -- integers, deterministic.  The rows are linear in opp_weights word for word, and with every opp_weights entry 1 and
 * hero_weights == NULL rows and agg equal mcq_exact_batch_hero_range(..., MCQ_LAW_UNIFORM, ...) bit for bit.
 * agg[i] (agg may be NULL) = sum_h eff_hero(h) x_h / runs_h / sum_h eff_hero(h) over the allowed hands, x = win, tie,
 * by_type[t], in doubles on the host in ascending row order.
 * Refused with MCQ_EINVAL, nothing launched, rows and agg untouched: whatever mcq_exact_batch_hero_range refuses,
 * opp_weights == NULL, no allowed hero hand (eff_hero is 0 everywhere in D); and -- before anything is copied to the
 * caller -- an allowed hero hand whose row has no weight (eff_opp is 0 for every hand that shares no card with it).
 * MCQ_EBUSY as everywhere.
 * Not covered: the reference's law, more than one opponent (by Monte Carlo: mcq_eval_batch_ranges).  Before the flop:
 * mcq_exact_batch_hero_range_preflop_weighted below. */
#define MCQ_COMBO_WEIGHT_MAX 65535u
MCQ_API int mcq_exact_batch_hero_range_weighted(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n,
                                                const uint16_t *opp_weights /* [n][MCQ_HAND_ROWS] */,
                                                const uint16_t *hero_weights /* [n][MCQ_HAND_ROWS], may be NULL: every allowed hand weighs 1 */,
                                                mcq_result *rows /* [n][MCQ_HAND_ROWS] */,
                                                mcq_exact_prob *agg /* [n], may be NULL */);

/* Exact RANGE against RANGE BEFORE THE FLOP, heads-up: every hand of the hero's range from ONE enumeration of the
 * C(|D|, 5) table completions per record.  An entry of its own because a record takes from tens of milliseconds (narrow
 * ranges) to seconds (every hand against every hand), not the millisecond of mcq_exact_batch_hero_range.
 * Accepted: n_board == 0, ext[i].hero_is_range == 1 with hero_range (q[i].hole is ignored), n_known == 0, n_players == 2 --
 * one random opponent drawn from opp_range, restricted or not --, optional ghost cards, both laws.
 * D = the 52 cards minus the ghost cards (52 or 50).  rows and agg are laid out and defined exactly as
 * mcq_exact_batch_hero_range's: rows[i * MCQ_HAND_ROWS + MCQ_HAND_INDEX(a, b)] is bit for bit the weights row
 * mcq_exact_batch_ext writes for the same record with the hero given as those two cards (runs = total weight, passes = 0),
 * every other row is zero, and agg[i] (agg may be NULL) combines the allowed rows with w_h = 1 under MCQ_LAW_UNIFORM and
 * 2 - [b is the highest card of D] under MCQ_LAW_REFERENCE, on the host in ascending row order.
 * Cost: only the hands that a range allows are ranked and walked (hero's hands and the hands the opponent can hold), so a
 * call scales with the ranges.  The completions are sent in slices, several kernel launches per call (262 144 completions
 * each unless MCQ_HERO_PRE_SLICE says otherwise): no single launch holds the GPU for the whole call.
 * Refused with MCQ_EINVAL, rows and agg untouched: a bad law, any table card (mcq_exact_batch_hero_range enumerates the
 * flop, turn and river), whatever that entry refuses otherwise (what mcq_eval_batch_ext refuses, hero_is_range == 0,
 * n_known != 0, n_players != 2, no allowed hero hand in D), more than MCQ_HERO_PREFLOP_MAX_BATCH records -- all before
 * anything is launched -- and an allowed hero hand against which the opponent's range cannot be dealt (seen as a row
 * without weight, before anything is copied to the caller).  MCQ_EBUSY as everywhere.
 * Deterministic: integer sums per hero hand.  Each record costs MCQ_HAND_ROWS * sizeof(mcq_result) = 138 KB of rows. */
#define MCQ_HERO_PREFLOP_MAX_BATCH 64u
MCQ_API int mcq_exact_batch_hero_range_preflop(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                                               mcq_result *rows /* [n][MCQ_HAND_ROWS] */,
                                               mcq_exact_prob *agg /* [n], may be NULL */);

/* Exact range against range with WEIGHTED HANDS BEFORE THE FLOP, heads-up: mcq_exact_batch_hero_range_preflop with a weight
 * per two-card hand on both sides -- opening, 3-bet and calling ranges as mixed strategies ("raise A5s 40 % of the time"),
 * a reach probability per combo.  Weights are integers 0..MCQ_COMBO_WEIGHT_MAX.
 * Accepted: exactly what mcq_exact_batch_hero_range_preflop accepts -- n_board == 0, hero_is_range == 1, n_known == 0,
 * n_players == 2, optional ghost cards (|D| = 52 or 50), at most MCQ_HERO_PREFLOP_MAX_BATCH records.
 * The law is always MCQ_LAW_UNIFORM, so there is no law argument, for the reason mcq_exact_batch_hero_range_weighted states.
 * Definitions: word for word those of mcq_exact_batch_hero_range_weighted with k = 5 and D = the 52 cards minus the ghost
 * cards.  eff_opp and eff_hero fold the class sets and the tables (entries for a hand that holds a ghost card are ignored);
 * a hero hand h of D is allowed iff eff_hero(h) > 0, every other row is zero, and for an allowed hand, with T over the
 * 5-subsets of D minus h and g over the two-card hands of D minus h minus T,
 *   runs = sum_T sum_g eff_opp(g)          (at most C(48, 5) * 1081 * 65535, about 1.2e14)
 * win, tie, by_type[9] its parts as there, passes = 0 -- integers, deterministic, linear in opp_weights.  With every
 * opp_weights entry 1 and hero_weights == NULL rows and agg equal mcq_exact_batch_hero_range_preflop(..., MCQ_LAW_UNIFORM,
 * ...) bit for bit.  agg[i] (agg may be NULL) = sum_h eff_hero(h) x_h / runs_h / sum_h eff_hero(h) over the allowed hands,
 * in doubles on the host in ascending row order.
 * Cost and launches: as mcq_exact_batch_hero_range_preflop's -- only hands of positive weight are ranked and walked, the
 * completions go out in the same slices (MCQ_HERO_PRE_SLICE).
 * Refused with MCQ_EINVAL, nothing launched, rows and agg untouched: whatever mcq_exact_batch_hero_range_preflop refuses
 * (any table card and more than MCQ_HERO_PREFLOP_MAX_BATCH records among it), opp_weights == NULL, no hero hand of positive
 * effective weight in D, and an allowed hero hand against which no opponent hand of positive effective weight is left.
 * The last is decided on the host before the enumeration: before the flop it is exact, because a hand g with eff_opp(g) > 0
 * that shares no card with h leaves |D| - 4 >= 5 cards for a completion that avoids both.  MCQ_EBUSY as everywhere.
 * Not covered: the reference's law, more than one opponent (by Monte Carlo: mcq_eval_batch_ranges). */
MCQ_API int mcq_exact_batch_hero_range_preflop_weighted(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n,
                                                        const uint16_t *opp_weights /* [n][MCQ_HAND_ROWS] */,
                                                        const uint16_t *hero_weights /* [n][MCQ_HAND_ROWS], may be NULL: every allowed hand weighs 1 */,
                                                        mcq_result *rows /* [n][MCQ_HAND_ROWS] */,
                                                        mcq_exact_prob *agg /* [n], may be NULL */);

/* Monte-Carlo MULTIWAY equity with a WEIGHTED RANGE PER SEAT: seat 0 opens this range, seat 1 three-bets that one, seat 2
 * cold-calls a third -- what is each range worth on this board?  2..10 seats, a weight per two-card hand and seat.
 * A record is q[i] (hole is ignored; n_board 0, 3, 4 or 5; n_players = p, 2..10; runs >= 1) and, for every seat s < p, the
 * weight table w_s = tables[seat_table[i * 10 + s]]: MCQ_HAND_ROWS uint16 entries 0..MCQ_COMBO_WEIGHT_MAX indexed by
 * MCQ_HAND_INDEX.  Entries of seat_table at s >= n_players are ignored.  Tables are shared by index: "every opponent holds
 * the same range" over 4096 boards is one table, not 24 576.  A known hand is a table with one non-zero entry (such a seat
 * holds its hand in every trial and takes no random word: the mapping below would select that hand for every word).
 * The law.  B = the table cards, eff_s(h) = w_s[h] if h holds no card of B, else 0.  One iteration deals the p hands with
 *     P(h_0, .., h_{p-1})  ~  prod_s eff_s(h_s) * [the hands are pairwise disjoint]
 * and then the 5 - n_board missing table cards uniformly without replacement from the 52 - n_board - 2p cards left.  This
 * is the JOINT law: symmetric in the seats, so permuting the seats permutes the rows in distribution.  It is NOT the
 * sequential "hero first, then each opponent from what is left" law that agg of the hero-range entries describes (there the
 * hero's hands are weighted by eff_hero alone; here every seat's hands are also weighted by how much room they leave the
 * others).  The context's dealing-law switch does not matter: this entry is uniform by definition, and the reference's
 * "never the highest card" does not apply to its table cards.
 * It is realised by rejection, which is exact: (1) seat s draws a hand with probability w_s[h] / sum(w_s), one random word u
 * per draw: t = mulhi32(u, total_s), the hand is the first index in ascending MCQ_HAND_INDEX order whose inclusive cumulative
 * weight exceeds t (total_s < 2^27; a hand's probability is off by less than 2^-32); (2) that seat alone draws again while
 * its hand holds a table card; (3) when two seats' hands share a card the WHOLE trial is abandoned, at the first collision,
 * and every seat draws again.  Streams: those of mcq_eval_batch_ext (keyed by (seed, first_query_id + i, task * 64 + lane),
 * sixteen iterations each), so a row depends on (record, tables, seed, query id) only -- not on the batch around it, on how
 * the tables are numbered or shared, or on the launch shape -- and a batch split into calls with the matching first_query_id
 * gives the same rows.
 * Row: runs; passes = whole trials (passes >= runs, and == runs when the supports cannot collide); seat[s].win / tie / share
 * exactly as mcq_eval_batch_ext_seats defines them: "best" by ranking key, share += MCQ_SHARE_UNIT / k, sum_s share ==
 * MCQ_SHARE_UNIT * runs exactly, seats >= n_players zero.
 * Refused with MCQ_EINVAL, nothing launched, out untouched: a null context or buffer (n == 0 returns MCQ_OK), n_tables == 0,
 * an invalid record (a duplicate or out-of-range table card, non-zero reserved, n_board of 1 or 2, n_players outside 2..10,
 * runs == 0), a seat_table entry >= n_tables, a seat whose table has no hand of positive weight clear of the table cards.
 * A record whose seats block each other (two seats both holding only AsAh) is seen on the device: an iteration without an
 * accepted trial within 65536 marks the row and the call returns MCQ_EINVAL with out untouched, as mcq_eval_batch_ext does
 * for a range that cannot be dealt; the per-seat re-draw is bounded the same way.  MCQ_EBUSY as everywhere.
 * Cost: whole-trial rejection is inherent to the law.  With every hand allowed to every seat, trials per iteration are about
 * 1.1 at two seats, 1.3 at three, 3.6 at six and 55 at ten before the flop, and 75 at ten on a flop (a table hit is re-drawn
 * by its seat alone and abandons nothing, but three cards fewer are left to be disjoint on).  Ten wide ranges are expensive,
 * and narrow ranges crowded on the same cards can be worse (nine opponents on the top quarter of the classes: refused).  Device memory: 8 KB per distinct table.
 * Not covered: dead or ghost cards, the one-launch path for small queries, a device-resident or torch entry, the parity
 * mode (the reference has nothing to match), mcq_multi_*.  The breakdown by the hands of one seat:
 * mcq_eval_batch_ranges_hands. */
MCQ_API int mcq_eval_batch_ranges(mcq_ctx *ctx, const mcq_query *q, const uint32_t *seat_table /* [n][10] */,
                                  const uint16_t *tables /* [n_tables][MCQ_HAND_ROWS] */, size_t n_tables, size_t n,
                                  uint64_t seed, uint64_t first_query_id, mcq_result_seats *out);

/* mcq_eval_batch_ranges with the BREAKDOWN BY HAND of one seat: which hands of the range carry its equity -- how often each
 * is dealt, how often it wins or ties, what pot share it takes against these other ranges.  The records, the tables, the law
 * (MCQ-RG v1), the streams (keyed by (seed, first_query_id + i, task * 64 + lane), sixteen iterations each) and the refusals
 * are those of mcq_eval_batch_ranges, word for word.  `seat` is the watched seat, one value per call, 0..9.
 *  1. out[i] is bit for bit the row mcq_eval_batch_ranges writes for the same arguments (the schedule differs, the streams
 *     do not).
 *  2. hands[i * MCQ_HAND_ROWS + MCQ_HAND_INDEX(a, b)] describes the iterations in which the watched seat held {a < b}: runs
 *     counts them; win, tie and share are that seat's increments in them, exactly as mcq_seat defines them.  A hand the
 *     seat cannot hold -- zero weight, or a table card in it -- has a zero row.
 *  3. Summed over the MCQ_HAND_ROWS rows: runs == out[i].runs, and win, tie, share == out[i].seat[seat].win, .tie, .share,
 *     exactly.
 *  4. The conditional equity of a hand is (win + tie) / runs, its pot share is share / (MCQ_SHARE_UNIT * runs).
 *  5. A row depends on (record, tables, seed, query id, seat) only -- not on the batch, the launch shape or MCQ_GRID_CAP --
 *     and a batch split into calls with the matching first_query_id gives the same rows.
 *  6. A watched seat whose table is one-hot (a known hand) is legal: its one row equals the seat's whole row.
 * Refused with MCQ_EINVAL, nothing launched, out and hands untouched: whatever mcq_eval_batch_ranges refuses, hands == NULL,
 * seat >= n_players of any record, n > MCQ_RANGES_HANDS_MAX_BATCH.  A record whose seats block each other is seen on the
 * device, as there: MCQ_EINVAL with both outputs untouched.  MCQ_EBUSY as everywhere; n == 0 returns MCQ_OK.
 * Device memory: 42 KB of rows per record, beside what mcq_eval_batch_ranges takes.  Runs up to 2^32 - 1 stay exact.
 * Not covered: several watched seats in one call, and what mcq_eval_batch_ranges does not cover. */
typedef struct mcq_hand_row {
    uint64_t runs;  /* iterations in which the watched seat held this hand */
    uint64_t win;   /* ... and was the only best hand */
    uint64_t tie;   /* ... and was one of several best hands */
    uint64_t share; /* sum of MCQ_SHARE_UNIT / k over those two */
} mcq_hand_row;     /* 32 bytes */
#define MCQ_RANGES_HANDS_MAX_BATCH 1024u
MCQ_API int mcq_eval_batch_ranges_hands(mcq_ctx *ctx, const mcq_query *q, const uint32_t *seat_table /* [n][10] */,
                                        const uint16_t *tables /* [n_tables][MCQ_HAND_ROWS] */, size_t n_tables, size_t n,
                                        uint64_t seed, uint64_t first_query_id, uint32_t seat,
                                        mcq_result_seats *out /* [n] */, mcq_hand_row *hands /* [n][MCQ_HAND_ROWS] */);

/* Exact equity PER RUNOUT, on the flop and the turn: which cards help and how much, from ONE enumeration per record.
 * Accepted: whatever mcq_exact_batch_ext_ways accepts -- hero given as two cards, 0..9 known hands each given as two cards,
 * optional ghost cards, at most one random opponent, ranged or not, both laws -- with 3 or 4 table cards; a batch may mix
 * the shapes.  R = the cards the opponent and the table are dealt from, k = 5 - n_board cards to come.
 * Every row is an mcq_result_ways weight row exactly as mcq_exact_batch_ext_ways writes it (runs = weight, passes = 0,
 * sum(tie_ways) == r.tie), restricted to part of the table completions:
 *   k = 1 (turn)  cards[i * 52 + c] = the row of the single completion "river = card id c"; pairs[i][*] all zero;
 *   k = 2 (flop)  pairs[i * MCQ_HAND_ROWS + MCQ_HAND_INDEX(a, b)] = the row of the completion {a < b};
 *                 cards[i * 52 + c] = the sum of the pair rows that contain c.
 * The row of a card or pair that cannot come -- not in R, or impossible under MCQ_LAW_REFERENCE, where a table card is
 * never the highest card left -- is zero.  The rows of a record add up, word for word, to its mcq_exact_batch_ext_ways
 * weights row: the card rows for k = 1, the pair rows for k = 2 (the card rows of a flop add up to twice that row).
 * Hero's hand type is fixed by the completion, so a completion row has at most one non-zero by_type entry, win + tie.
 * Equity given that c comes next: (win + tie) / runs of cards[i * 52 + c] (pot share: the tie_ways formula of
 * mcq_result_ways); P(c is the next card) = cards[i * 52 + c].runs / (k * total runs).  That holds under
 * MCQ_LAW_REFERENCE too: for a fixed opponent hand a pair {a < b} is allowed in both dealing orders or in neither -- it is
 * refused exactly when b is the highest card left (a then b: b would be the last card of the deck without a; b then a: b
 * would be the last card of the deck; a itself is never the highest while b is there, and once b has gone a card above b
 * remains) --, every allowed ORDERED draw is equally likely, and the number of allowed ordered draws, (d - 1) (d - 2) or d - 1
 * with d cards left after the opponent's hand, does not depend on that hand.  So each order of an allowed
 * pair carries half its weight, and the first card's weight is the sum over its pairs of one half: the card row over k.
 * pairs may be NULL (the pair rows are then not copied back).  Refused with MCQ_EINVAL, nothing launched, cards and pairs
 * untouched for the whole batch: whatever mcq_exact_batch_ext_ways refuses (a hero range, a ranged known hand, two random
 * opponents, a range that cannot be dealt, a bad law, an invalid record), 0 table cards (C(50, 5) rows per record), 5 table
 * cards (no card to come), n > MCQ_RUNOUT_MAX_BATCH.  Deterministic: every completion has one owner that stores its row
 * once, the card rows are integer sums in a fixed order; a batch gives what the single calls give.  Device scratch:
 * (52 + MCQ_HAND_ROWS) rows of 176 bytes = 243 KB per record. */
#define MCQ_RUNOUT_CARD_ROWS 52u
#define MCQ_RUNOUT_MAX_BATCH 1024u
MCQ_API int mcq_exact_batch_ext_runouts(mcq_ctx *ctx, const mcq_query *q, const mcq_query_ext *ext, size_t n, int law,
                                        mcq_result_ways *cards /* [n][52] */,
                                        mcq_result_ways *pairs /* [n][MCQ_HAND_ROWS], may be NULL */);

/* The exact hand-against-hand matrix of a board: every two-card hand against every other one, heads-up, from ONE enumeration
 * per record -- the linear map whose weighted row sums mcq_exact_batch_hero_range_weighted returns.  The law is always
 * MCQ_LAW_UNIFORM (no law argument: under the reference's law the weight of a completion depends on both hands, so a pair's
 * total would not be a constant).  3 to 5 table cards; a batch may mix the streets.
 * Definitions.  D = the 52 cards minus the table cards and the dead cards, L = |D|, k = 5 - n_board, total[i] = C(L - 4, k).
 * For two-card hands h, g of D that share no card, with T running over the k-subsets of D minus h minus g:
 *   win[i][MCQ_HAND_INDEX(h)][MCQ_HAND_INDEX(g)] = the number of T on which h ranks strictly above g,
 *   tie[i][MCQ_HAND_INDEX(h)][MCQ_HAND_INDEX(g)] = the number of T on which they are level,
 * so win[h][g] + win[g][h] + tie[h][g] == total and tie is symmetric.  Every other entry is written as 0: the diagonal, pairs
 * that share a card, hands that hold a table or a dead card.  The ranking is the evaluator's, as in every other entry.
 * Refused with MCQ_EINVAL, nothing launched, the outputs untouched for the whole batch: n_board outside 3..5 (preflop is
 * C(48, 5) completions with 32-bit counts: not this entry), a card id >= 52, a table card twice, a table card that is also
 * dead, reserved bytes or mask bits 52..63 not 0, L - 4 < k (no pair of hands leaves a completion), n == 0,
 * n > MCQ_MATRIX_MAX_BATCH, win == NULL.  Deterministic: integer counts, every entry has one owner that stores it once; a
 * batch gives what the single calls give, however the library cuts it into launches.  Each record costs
 * MCQ_HAND_ROWS * MCQ_HAND_ROWS * 2 = 3.5 MB per matrix. */
typedef struct mcq_matrix_query { /* 16 bytes */
    uint8_t board[5];             /* n_board of them used, distinct card ids < 52; the others are not read */
    uint8_t n_board;              /* 3, 4 or 5 */
    uint8_t reserved[2];          /* 0 */
    uint64_t dead;                /* bit c set: card c is out of the deck (bits 52..63 must be 0) */
} mcq_matrix_query;
#define MCQ_MATRIX_MAX_BATCH 256u
MCQ_API int mcq_exact_matrix(mcq_ctx *ctx, const mcq_matrix_query *q, size_t n,
                             uint16_t *win /* [n][MCQ_HAND_ROWS][MCQ_HAND_ROWS] */,
                             uint16_t *tie /* [n][MCQ_HAND_ROWS][MCQ_HAND_ROWS], may be NULL */,
                             uint32_t *total /* [n], may be NULL */);
/* The same with the matrices written to DEVICE memory on hip_stream (NULL = the null stream).  The records are host memory
 * and are validated on the host before anything is launched (unlike mcq_eval_batch_device, which cannot refuse a record);
 * total is host memory and is filled before the call returns.  Asynchronous once the context's scratch for this stream is
 * large enough (it grows on the first call of a size); not to be captured into a graph. */
MCQ_API int mcq_exact_matrix_device(mcq_ctx *ctx, const mcq_matrix_query *q /* host */, size_t n,
                                    void *d_win /* uint16 [n][MCQ_HAND_ROWS][MCQ_HAND_ROWS] */,
                                    void *d_tie /* likewise, may be NULL */, uint32_t *total /* host [n], may be NULL */,
                                    void *hip_stream);

/* Select the dealing law used by MCQ_MODE_PHILOX on this context (MCQ_LAW_*).  Extended queries
 * (mcq_eval_batch_ext) are dealt by the reference's law only: under MCQ_LAW_UNIFORM that call gives MCQ_EINVAL.
 * mcq_eval_batch_ranges does not look at the switch: its law is uniform by definition. */
MCQ_API int mcq_set_dealing_law(mcq_ctx *ctx, int law);

/* Kernel timing (off by default: a timestamped launch costs a small query about 6 us of its call time).  When on,
 * every evaluation-kernel launch carries a pair of HIP events that take the kernel's own begin and end timestamps
 * on the stream it is launched on (a ring of the 64 most recent launches; in parity mode the pair spans the stream
 * walk and the evaluation kernel; launches recorded into a stream capture are not timed).  mcq_kernel_times writes
 * the durations in milliseconds of the latest min(max_n, 64, launches so far) launches, oldest first, and returns how
 * many; it waits for the newest of them to have finished.  mcq_last_kernel_ms: the most recent host-entry call's
 * total (all chunks), else the latest launch; 0 while timing is off.  The contexts of an mcq_multi always time. */
MCQ_API int mcq_set_kernel_timing(mcq_ctx *ctx, int on);
MCQ_API int mcq_kernel_times(mcq_ctx *ctx, float *ms, int max_n);
MCQ_API float mcq_last_kernel_ms(mcq_ctx *ctx);

/* ---- Lock-step table driver (BASELINE configs[4]; replaces the loop gym_env/env.py:170-200 + 224-262 runs per
 * table: observe -> get_equity -> agent -> step).  T tables of n_seats seats play No-Limit Hold'em with the
 * reference's table rules (gym_env/env.py, gym_env/cycle.py); every table always has exactly one pending equity
 * query, finished episodes restart at once.  mcq_tables_begin writes the n_tables pending queries (table i ->
 * q[i]) and returns n_tables; mcq_tables_resume takes their equities ((win + tie) / runs) and advances every
 * table to its next query.  mcq_tables_run does `lock_steps` rounds of begin -> ONE mcq_eval_batch
 * (MCQ_MODE_PHILOX, seed cfg.seed, query ids counting up across calls) -> resume, and needs a context; it
 * runs the tables in two or three groups on streams (and host threads) of their own so that the host steps one
 * group while the other groups' batches are on the GPU -- every query keeps the id it has in the one-batch schedule,
 * so the results are the same.
 * begin/resume alone need no GPU (ctx may be NULL): that is how the CPU tests pin the rules.
 * seat_kind: 0 = equity agent (agents/agent_consider_equity.py:25-56 with min_call_equity / min_bet_equity of
 * the seat), 1 = random agent (agents/agent_random.py:21-29, drawing from the table's own generator).
 * Dealing and random seats draw from one xoshiro128++ per table, seeded by Philox4x32-10(counter = {table, 0, 0,
 * 'TBL1'}, key = seed); a bounded draw is mulhi32(next(), bound). */
typedef struct mcq_tables mcq_tables;
typedef struct mcq_tables_config {
    uint32_t n_tables, n_seats;     /* 2..10 seats */
    uint32_t runs;                  /* iterations per equity query (the reference uses 1000, env.py:261) */
    uint32_t max_raises;            /* per seat and street (env.py:92: 2) */
    double initial_stacks, small_blind, big_blind;
    uint64_t seed;
    uint8_t seat_kind[10];
    uint8_t reserved[6];            /* [0]: host threads stepping the tables (0 = automatic); [1]: 1 = do not split
                                     * the tables into groups on streams of their own (mcq_tables_run); [2]: 1 = three more
                                     * equity queries per observation, answers unused, as HoldemTable(calculate_equity=
                                     * True) issues them (gym_env/env.py:248-256); rest 0 */
    double min_call_equity[10], min_bet_equity[10];
} mcq_tables_config;

MCQ_API mcq_tables *mcq_tables_create(mcq_ctx *ctx, const mcq_tables_config *cfg); /* NULL + mcq_last_error */
MCQ_API void mcq_tables_destroy(mcq_tables *t);
MCQ_API size_t mcq_tables_begin(mcq_tables *t, mcq_query *q);
MCQ_API int mcq_tables_resume(mcq_tables *t, const double *equity);
MCQ_API int mcq_tables_run(mcq_tables *t, uint32_t lock_steps, uint64_t stats[3]);
/* stats: agent actions executed (env steps), equity queries issued, episodes finished -- totals since create */
MCQ_API void mcq_tables_stats(const mcq_tables *t, uint64_t stats[3]);
/* one table: stacks[n_seats]; info[8] = stage, seat to act, last winner, episodes, env steps, queries,
 * legal-move bit mask (bit = gym_env/enums.py Action value), driver phase */
MCQ_API int mcq_tables_state(const mcq_tables *t, uint32_t table, double *stacks, int32_t info[8]);

/* ---- One node, several GPUs, ONE process (the reference itself is single-device, so this has no
 * counterpart there -- it is what a batched caller of get_equity binds when a node has more than one GPU).
 * The batch is partitioned over n_shards SHARDS, shard s on HIP device devices[s] (devices = NULL: shard s on
 * device s); a device may appear more than once (an 8-way partition rehearsed on one GPU, or several streams per
 * GPU).  Each shard owns an engine context, a host worker thread and a stream.  Partition of a call:
 *   MCQ_PARTITION_QUERIES     shard s evaluates queries [n*s/k, n*(s+1)/k) under their own query ids
 *   MCQ_PARTITION_ITERATIONS  every shard evaluates share s of k of EVERY query's iterations (few large queries)
 *   MCQ_PARTITION_AUTO        queries when n >= 256 * n_shards, else iterations
 * Every shard fills its part of a zero-initialised [n, 13] uint64 tally matrix on its device; shards that share a
 * device are added there, and ONE ncclAllReduce(ncclUint64, ncclSum) over the distinct devices (communicators
 * from ncclCommInitAll, owned by the mcq_multi object; RCCL over xGMI) leaves the complete matrix on every device;
 * out[0..n) is copied from the first.  The tallies are bit-identical to mcq_eval_batch on one context with the same
 * (seed, first_query_id), whatever the partition.  MCQ_MODE_PHILOX.  RCCL is bound (dlopen) when the first
 * mcq_multi is created; a process that never creates one never maps it.
 * STATUS: with more than one DISTINCT device this entry has NOT been exercised on hardware yet (no multi-GPU node was
 * reachable while it was built): the partitions, the same-device add and a one-rank RCCL communicator are tested on
 * one GPU, where all shards share the device; ncclCommInitAll over several devices, the grouped all-reduce and the
 * per-device stream waits run for the first time on a multi-GPU node. */
#define MCQ_PARTITION_AUTO 0
#define MCQ_PARTITION_QUERIES 1
#define MCQ_PARTITION_ITERATIONS 2
typedef struct mcq_multi mcq_multi;
MCQ_API mcq_multi *mcq_multi_create(const int *devices, int n_shards, int flags); /* NULL + mcq_last_error; flags 0 */
MCQ_API void mcq_multi_destroy(mcq_multi *m);
MCQ_API int mcq_multi_eval_batch(mcq_multi *m, const mcq_query *q, size_t n, uint64_t seed, uint64_t first_query_id,
                                 int partition, mcq_result *out);
/* The same with queries and results RESIDENT IN HBM (no PCIe in the call): one device pointer pair per shard, on that
 * shard's device.  d_queries[s]: MCQ_PARTITION_QUERIES -> the shard's block, queries [n*s/k, n*(s+1)/k) of the batch
 * (k shards); MCQ_PARTITION_ITERATIONS -> all n queries.  d_results[s] -> mcq_result[n], overwritten: after the
 * all-reduce EVERY shard's buffer holds the complete matrix.  Blocks until all devices have finished.  The host never
 * sees the queries, so they are validated on the device: an invalid query's row has runs = 0 and passes = UINT64_MAX
 * (under either partition: only one share of a query writes the marker, so the sum over the shares keeps it). */
MCQ_API int mcq_multi_eval_batch_device(mcq_multi *m, const void *const *d_queries, size_t n, uint64_t seed,
                                        uint64_t first_query_id, int partition, void *const *d_results);
MCQ_API int mcq_multi_set_dealing_law(mcq_multi *m, int law);
/* info: shards, distinct devices (= ranks of the all-reduce), RCCL version code, partition of the last call */
MCQ_API int mcq_multi_info(const mcq_multi *m, int info[4]);
/* last call, milliseconds: slowest shard's evaluation kernel, the all-reduce (device 0's stream), whole call (wall) */
MCQ_API int mcq_multi_times(const mcq_multi *m, float ms[3]);

MCQ_API const char *mcq_last_error(void);
MCQ_API void mcq_version(int *major, int *minor, int *patch);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_H */
