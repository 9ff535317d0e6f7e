// hs_hero_range.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the lane code of the hero-range exact enumeration (neuron_poker_amd/csrc/mcq_exact_hero.hpp) for the HOST
// compiler and walks mcq_exact_hero_kernel's decomposition on the CPU -- completion by completion, the ranking lanes and
// then the hero hands one after the other -- and finishes the rows as the library's host side does, so that the
// GPU's output can be pinned bit for bit and the lane code checked against independent walks in a container without a GPU.
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../hostsim/hs_walk.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_hero.hpp"

// -> 0, or the refusal MCQ_XH_* (1..7).  rows: MCQ_XH_ROWS x 13 words, agg: 11 doubles; both untouched by a refusal.
extern "C" int hs_hero_range(const mcq_query *q, const mcq_query_ext *x, int law, uint64_t *rows_out, double *agg) {
    const McqTables &t = hs::luts();
    McqExactHeroQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    if (law != MCQ_LAW_REFERENCE && law != MCQ_LAW_UNIFORM) return -1;
    const int why = mcq_exact_hero_query(mcq_query_words(*q), er, law, e);
    if (why) return why;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e.x, r_id);
    std::vector<uint16_t> own(MCQ_XH_MAX_HANDS);
    e.n_allowed = mcq_exact_hero_count(e, r_id, own.data());
    if (e.n_allowed == 0u) return MCQ_XH_EMPTY;
    std::vector<uint8_t> cb_tab(MCQ_XX_MAX_RP);
    mcq_exact_ext_cb_table(e.x, r_id, 0u, 1u, cb_tab.data());
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
    const McqExactHeroSums zero = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    std::vector<std::vector<McqExactHeroSums>> part(n_thr, std::vector<McqExactHeroSums>(e.n_allowed, zero));
    auto work = [&](uint32_t thr) {
        std::vector<uint32_t> keys(MCQ_XH_MAX_PAIRS), rec(MCQ_XH_MAX_PAIRS);
        std::vector<McqExactHeroSums> &mine = part[thr];
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
                mcq_exact_hero_rank(e, bd, lane, 1024u, pair_xy.data(), rem_card, rem_pos, cb_tab.data(), t.tf, t.tops, t.sd,
                                    keys.data(), rec.data());
            for (uint32_t idx = 0; idx < e.n_allowed; idx++) { /* thread idx & 1023 of group idx >> 10 */
                const uint32_t hxy = pair_xy[own[idx]], qa = hxy & 0xFFu, qb = hxy >> 8;
                const uint32_t mi = mcq_exact_ext_m_index(e.x, pos, qa, qb);
                if (mi >= e.x.n_pairs) continue;
                McqExactAcc acc = {0, 0, 0};
                const uint32_t type = mcq_exact_hero_walk(e, bd, qa, qb, mi, keys.data(), rec.data(), acc);
                mcq_exact_hero_add(mine[idx], acc, type);
            }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t thr = 1; thr < n_thr; thr++) pool.emplace_back(work, thr);
    work(0u);
    for (std::thread &th : pool) th.join();
    std::vector<McqExactHeroSums> sums(e.n_allowed, zero);
    for (uint32_t thr = 0; thr < n_thr; thr++)
        for (uint32_t idx = 0; idx < e.n_allowed; idx++) {
            McqExactHeroSums &d = sums[idx];
            const McqExactHeroSums &a = part[thr][idx];
            d.win += a.win;
            d.tie += a.tie;
            d.tot += a.tot;
            for (uint32_t k = 0; k < 9; k++) d.type[k] += a.type[k];
        }
    std::vector<mcq_result> rows(MCQ_XH_ROWS);
    memset(rows.data(), 0, MCQ_XH_ROWS * sizeof(mcq_result));
    for (uint32_t idx = 0; idx < e.n_allowed; idx++) {
        const uint32_t hxy = pair_xy[own[idx]];
        mcq_result &r = rows[mcq_exact_hero_row(r_id, hxy & 0xFFu, hxy >> 8)];
        r.runs = sums[idx].tot;
        r.win = sums[idx].win;
        r.tie = sums[idx].tie;
        for (uint32_t k = 0; k < 9; k++) r.by_type[k] = sums[idx].type[k];
    }
    mcq_exact_prob p;
    if (!mcq_exact_hero_finish(e, r_id, rows.data(), p)) return MCQ_XH_UNDEALABLE;
    memcpy(rows_out, rows.data(), MCQ_XH_ROWS * sizeof(mcq_result));
    memcpy(agg, &p, sizeof p);
    return 0;
}

// the hero's draw weights: wt[row] = how often the law deals hero that hand in proportion (0: not an allowed hand of D);
// -> the number of allowed hands, or -1
extern "C" int hs_hero_weights(const mcq_query *q, const mcq_query_ext *x, int law, uint32_t *wt) {
    McqExactHeroQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    if (mcq_exact_hero_query(mcq_query_words(*q), er, law, e)) return -1;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e.x, r_id);
    int n = 0;
    for (uint32_t i = 0; i < MCQ_XH_ROWS; i++) wt[i] = 0;
    for (uint32_t qb = 1; qb < e.x.b.L; qb++)
        for (uint32_t qa = 0; qa < qb; qa++)
            if (mcq_exact_hero_allowed(e, r_id, qa, qb)) {
                wt[mcq_exact_hero_row(r_id, qa, qb)] = mcq_exact_hero_weight(e, qb);
                n++;
            }
    return n;
}
