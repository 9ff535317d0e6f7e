// hs_hero_weighted.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the WEIGHTED lane code of the hero-range exact enumeration (neuron_poker_amd/csrc/mcq_exact_hero.hpp, "weighted
// hands") for the HOST compiler and walks mcq_exact_hero_w_kernel's decomposition on the CPU -- the two tables per D-pair,
// the allowed list, then completion by completion the ranking lanes and the hero hands one after the other, a completion's
// 32-bit sums added once into the 64-bit ones -- and finishes the rows as the library's host side does, so that the GPU's
// output can be pinned bit for bit and the lane code checked against an independent walk in a container without a GPU.
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../hostsim/hs_walk.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_hero.hpp"

// -> 0, the refusal MCQ_XH_* (1..7), or -2 (no opponent table).  opp_w, hero_w: MCQ_XH_ROWS uint16 each, hero_w may be
// null.  rows: MCQ_XH_ROWS x 13 words, agg: 11 doubles; both untouched by a refusal.
extern "C" int hs_hero_weighted(const mcq_query *q, const mcq_query_ext *x, const uint16_t *opp_w, const uint16_t *hero_w,
                                uint64_t *rows_out, double *agg) {
    const McqTables &t = hs::luts();
    McqExactHeroQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    if (!opp_w) return -2;
    const int why = mcq_exact_hero_query(mcq_query_words(*q), er, MCQ_LAW_UNIFORM, e);
    if (why) return why;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e.x, r_id);
    std::vector<uint16_t> ow_tab(MCQ_XH_MAX_HANDS), hw_tab(MCQ_XH_MAX_HANDS), own(MCQ_XH_MAX_HANDS);
    for (uint32_t lane = 0; lane < 1024u; lane++)
        mcq_exact_hero_w_tables(e, r_id, opp_w, hero_w, lane, 1024u, ow_tab.data(), hw_tab.data());
    e.n_allowed = mcq_exact_hero_w_count(e, hw_tab.data(), own.data());
    if (e.n_allowed == 0u) return MCQ_XH_EMPTY;
    std::vector<uint16_t> pair_xy(MCQ_XH_MAX_HANDS);
    for (uint32_t i = 0; i < MCQ_XH_MAX_HANDS; i++) {
        uint32_t a, b;
        mcq_exact_pair_xy(i, a, b);
        pair_xy[i] = (uint16_t)(a | (b << 8));
    }
    /* the completions are shared out among a few host threads, each with its own keys, records and sums (the kernel's
     * blocks likewise); the sums are integers, so the order in which they are added does not matter */
    const uint32_t n_boards = mcq_exact_binom(e.x.b.L, e.x.b.k);
    uint32_t n_thr = std::thread::hardware_concurrency();
    n_thr = n_thr < 1u ? 1u : n_thr > 8u ? 8u : n_thr;
    n_thr = n_thr > n_boards ? n_boards : n_thr;
    const McqExactHeroSumsW zero = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    std::vector<std::vector<McqExactHeroSumsW>> part(n_thr, std::vector<McqExactHeroSumsW>(e.n_allowed, zero));
    auto work = [&](uint32_t thr) {
        std::vector<uint32_t> keys(MCQ_XH_MAX_PAIRS), rec(MCQ_XH_MAX_PAIRS);
        std::vector<McqExactHeroSumsW> &mine = part[thr];
        for (uint32_t board = thr; board < n_boards; board += n_thr) {
            uint32_t pos[5];
            mcq_exact_unrank(board, e.x.b.L, e.x.b.k, pos);
            McqExactBoard bd;
            mcq_exact_hero_board(e.x.b, pos, r_id, bd);
            McqCard rem_card[64];
            uint32_t rem_pos[64];
            for (uint32_t l = 0; l < e.x.m; l++) {
                rem_pos[l] = mcq_exact_rem_pos(pos, l);
                rem_card[l] = mcq_card(r_id[rem_pos[l]]);
            }
            for (uint32_t lane = 0; lane < 1024u; lane++)
                mcq_exact_hero_w_rank(e, bd, lane, 1024u, pair_xy.data(), rem_card, rem_pos, ow_tab.data(), t.tf, t.tops, t.sd,
                                      keys.data(), rec.data());
            for (uint32_t idx = 0; idx < e.n_allowed; idx++) { /* thread idx & 1023 of group idx >> 10 */
                const uint32_t hxy = pair_xy[own[idx]], qa = hxy & 0xFFu, qb = hxy >> 8;
                const uint32_t mi = mcq_exact_ext_m_index(e.x, pos, qa, qb);
                if (mi >= e.x.n_pairs) continue;
                McqExactAcc acc = {0, 0, 0};
                const uint32_t type = mcq_exact_hero_w_walk(e, qa, qb, mi, keys.data(), rec.data(), acc);
                mcq_exact_hero_w_add(mine[idx], acc, type);
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
        const uint32_t hxy = pair_xy[own[idx]];
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
    if (!mcq_exact_hero_w_finish(e, r_id, hw_tab.data(), rows.data(), p)) return MCQ_XH_UNDEALABLE;
    memcpy(rows_out, rows.data(), MCQ_XH_ROWS * sizeof(mcq_result));
    memcpy(agg, &p, sizeof p);
    return 0;
}
