// hs_hero_preflop_weighted.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the WEIGHTED lane code of the preflop hero-range exact enumeration (neuron_poker_amd/csrc/mcq_exact_hero_pre.hpp,
// "weighted hands") for the HOST compiler and walks mcq_exact_hero_pre_w_kernel's decomposition on the CPU -- the two tables
// per D-pair, the three lists made from them, the check that every allowed hero hand is left an opponent, then completion by
// completion the ranking lanes and the hero hands one after the other with their walks shared as a block shares them, a
// completion's 32-bit sums added once into the 64-bit ones -- over a range [lo, hi) of completions.  Generic in k = 0..5, so
// that the lane code can be pinned against mcq_exact_hero.hpp's weighted section (k <= 2) and against a literal walk of the
// definition (k = 5) in a container without a GPU.
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../hostsim/hs_walk.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_hero_pre.hpp"

namespace {
uint32_t host_threads(uint32_t most) {
    uint32_t n = std::thread::hardware_concurrency();
    n = n < 1u ? 1u : n > 8u ? 8u : n;
    return n > most ? (most ? most : 1u) : n;
}
std::atomic<uint64_t> g_walked{0}; /* completions ranked since the library was loaded */
}  // namespace

// how many completions every call so far has ranked: a refusal made before the enumeration leaves it alone
extern "C" uint64_t hs_hero_pre_w_walked(void) { return g_walked.load(); }

// -> 0, or the refusal MCQ_XH_* (1..7; 5 is never given: any number of table cards is taken), -2 for an empty completion
// range, -3 without an opponent table.  opp_w, hero_w: MCQ_XH_ROWS uint16 each, hero_w may be null.  rows: MCQ_XH_ROWS x 13
// words, the PARTIAL rows of the completions [lo, min(hi, C(|D|, k))); agg: 11 doubles, written (with the backstop of
// mcq_exact_hero_w_finish) only when the range covers every completion.  counts: allowed, live, ranked, C(|D|, k).
// Everything is untouched by a refusal; MCQ_XH_UNDEALABLE comes from mcq_exact_hero_pre_w_undealable, before any completion.
extern "C" int hs_hero_pre_w(const mcq_query *q, const mcq_query_ext *x, const uint16_t *opp_w, const uint16_t *hero_w, uint32_t lo,
                             uint32_t hi, uint64_t *rows_out, double *agg, uint32_t *counts) {
    const McqTables &t = hs::luts();
    McqExactHeroQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    if (!opp_w) return -3;
    const int why = mcq_exact_hero_pre_query(mcq_query_words(*q), er, MCQ_LAW_UNIFORM, e);
    if (why) return why;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e.x, r_id);
    std::vector<uint16_t> ow_tab(MCQ_XP_MAX_PAIRS), hw_tab(MCQ_XP_MAX_PAIRS);
    for (uint32_t lane = 0; lane < 1024u; lane++)
        mcq_exact_hero_w_tables(e, r_id, opp_w, hero_w, lane, 1024u, ow_tab.data(), hw_tab.data());
    std::vector<uint16_t> allowed(MCQ_XP_MAX_PAIRS), live(MCQ_XP_MAX_PAIRS), ranked(MCQ_XP_MAX_PAIRS), pair_xy(MCQ_XP_MAX_PAIRS);
    uint32_t n[3];
    mcq_exact_hero_pre_w_lists(e, ow_tab.data(), hw_tab.data(), allowed.data(), live.data(), ranked.data(), n);
    e.n_allowed = n[0];
    if (e.n_allowed != mcq_exact_hero_w_count(e, hw_tab.data(), nullptr)) return -9; /* what the host plans with */
    if (e.n_allowed == 0u) return MCQ_XH_EMPTY;
    if (mcq_exact_hero_pre_w_undealable(e, ow_tab.data(), hw_tab.data()) != MCQ_XP_MAX_PAIRS) return MCQ_XH_UNDEALABLE;
    for (uint32_t i = 0; i < MCQ_XP_MAX_PAIRS; i++) {
        uint32_t a, b;
        mcq_exact_pair_xy(i, a, b);
        pair_xy[i] = (uint16_t)(a | (b << 8));
    }
    McqCard d_card[64];
    for (uint32_t p = 0; p < e.x.b.L; p++) d_card[p] = mcq_card(r_id[p]);
    const uint32_t n_boards = mcq_exact_binom(e.x.b.L, e.x.b.k);
    hi = hi > n_boards ? n_boards : hi;
    if (lo >= hi) return -2;
    const bool whole = lo == 0u && hi == n_boards;
    /* the completions are shared out among a few host threads, each with its own keys, records and 64-bit sums (the
     * kernel's blocks likewise: no bound on the completions one of them owns) */
    const uint32_t n_thr = host_threads(hi - lo);
    const McqExactHeroSumsW zero = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    std::vector<std::vector<McqExactHeroSumsW>> part(n_thr, std::vector<McqExactHeroSumsW>(e.n_allowed, zero));
    auto work = [&](uint32_t thr) {
        std::vector<uint32_t> keys(MCQ_XP_MAX_PAIRS), rec(MCQ_XP_MAX_PAIRS);
        std::vector<McqExactHeroSumsW> &mine = part[thr];
        /* a run of consecutive completions per thread, as a block's: the first one unranked, the others by stepping */
        const uint32_t run = mcq_exact_hero_pre_owned(hi - lo, n_thr), b0 = lo + thr * run, b1 = hi - b0 < run ? hi : b0 + run;
        uint32_t pos[5];
        if (b0 < hi) mcq_exact_unrank(b0, e.x.b.L, e.x.b.k, pos);
        for (uint32_t board = b0; board < b1 && b0 < hi; board++) {
            if (board != b0) mcq_exact_hero_pre_next(pos, e.x.b.k);
            McqExactBoard bd;
            mcq_exact_hero_board(e.x.b, pos, r_id, bd);
            const uint64_t taken = mcq_exact_hero_pre_mask(e.x.b, pos);
            g_walked.fetch_add(1u);
            for (uint32_t lane = 0; lane < 1024u; lane++)
                mcq_exact_hero_pre_w_rank(bd, taken, lane, 1024u, ranked.data(), n[2], pair_xy.data(), d_card, ow_tab.data(), t.tf,
                                          t.tops, t.sd, keys.data(), rec.data());
            for (uint32_t idx = 0; idx < e.n_allowed; idx++) { /* hand idx & 1023 of group idx >> 10 */
                const uint32_t own = allowed[idx], hxy = pair_xy[ranked[own]], qa = hxy & 0xFFu, qb = hxy >> 8;
                if (keys[own] == 0u) continue;
                const uint32_t first = idx & ~1023u, n_g = e.n_allowed - first < 1024u ? e.n_allowed - first : 1024u;
                const uint32_t share = mcq_exact_hero_pre_share(n_g);
                for (uint32_t sub = 0; sub < share; sub++) { /* the threads that share this hand's walk */
                    McqExactAcc acc = {0, 0, 0};
                    const uint32_t type = mcq_exact_hero_pre_w_walk(qa, qb, own, live.data(), n[1], sub, share, keys.data(), rec.data(), acc);
                    mcq_exact_hero_w_add(mine[idx], acc, type);
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t thr = 1; thr < n_thr; thr++) pool.emplace_back(work, thr);
    work(0u);
    for (std::thread &th : pool) th.join();
    std::vector<mcq_result> rows(MCQ_XH_ROWS);
    memset(rows.data(), 0, MCQ_XH_ROWS * sizeof(mcq_result));
    for (uint32_t idx = 0; idx < e.n_allowed; idx++) {
        const uint32_t hxy = pair_xy[ranked[allowed[idx]]];
        mcq_result &r = rows[mcq_exact_hero_row(r_id, hxy & 0xFFu, hxy >> 8)];
        for (uint32_t thr = 0; thr < n_thr; thr++) { /* (the kernel's atomics) */
            const McqExactHeroSumsW &a = part[thr][idx];
            r.runs += a.tot;
            r.win += a.win;
            r.tie += a.tie;
            for (uint32_t k = 0; k < 9; k++) r.by_type[k] += a.type[k];
        }
    }
    mcq_exact_prob p;
    if (whole && !mcq_exact_hero_w_finish(e, r_id, hw_tab.data(), rows.data(), p)) return MCQ_XH_UNDEALABLE;
    memcpy(rows_out, rows.data(), MCQ_XH_ROWS * sizeof(mcq_result));
    if (whole) memcpy(agg, &p, sizeof p);
    counts[0] = n[0];
    counts[1] = n[1];
    counts[2] = n[2];
    counts[3] = n_boards;
    return 0;
}

// the rows of the allowed hero hands in list order (position i of `allowed` -> its row) -> their number, or -1
extern "C" int hs_hero_pre_w_allowed(const mcq_query *q, const mcq_query_ext *x, const uint16_t *opp_w, const uint16_t *hero_w,
                                     uint32_t *row_of) {
    McqExactHeroQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    if (!opp_w || mcq_exact_hero_pre_query(mcq_query_words(*q), er, MCQ_LAW_UNIFORM, e)) return -1;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e.x, r_id);
    std::vector<uint16_t> ow_tab(MCQ_XP_MAX_PAIRS), hw_tab(MCQ_XP_MAX_PAIRS);
    mcq_exact_hero_w_tables(e, r_id, opp_w, hero_w, 0u, 1u, ow_tab.data(), hw_tab.data());
    std::vector<uint16_t> allowed(MCQ_XP_MAX_PAIRS), live(MCQ_XP_MAX_PAIRS), ranked(MCQ_XP_MAX_PAIRS);
    uint32_t n[3];
    mcq_exact_hero_pre_w_lists(e, ow_tab.data(), hw_tab.data(), allowed.data(), live.data(), ranked.data(), n);
    for (uint32_t i = 0; i < n[0]; i++) {
        uint32_t qa, qb;
        mcq_exact_pair_xy(ranked[allowed[i]], qa, qb);
        row_of[i] = mcq_exact_hero_row(r_id, qa, qb);
    }
    return (int)n[0];
}
