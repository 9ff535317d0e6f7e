// hs_hero_preflop.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the lane code of the preflop hero-range exact enumeration (neuron_poker_amd/csrc/mcq_exact_hero_pre.hpp) for the
// HOST compiler and walks mcq_exact_hero_pre_kernel's decomposition on the CPU -- the three lists, then completion by
// completion the ranking lanes and the hero hands one after the other -- over a range [lo, hi) of completions, so that
// the lane code can be pinned against mcq_exact_hero.hpp (k <= 2) and against the slow reference below (k = 5) in a
// container without a GPU.
#include <stdint.h>
#include <string.h>

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
}  // namespace

// -> 0, or the refusal MCQ_XH_* (1..7; 5 is never given: any number of table cards is taken), -1 for a bad law, -2 for an
// empty completion range.  rows: MCQ_XH_ROWS x 13 words, the PARTIAL rows of the completions [lo, min(hi, C(|D|, k)));
// agg: 11 doubles, written (and the undealable range refused) only when the range covers every completion.  counts:
// allowed, live, ranked, C(|D|, k).  Everything is untouched by a refusal.
extern "C" int hs_hero_pre(const mcq_query *q, const mcq_query_ext *x, int law, uint32_t lo, uint32_t hi, uint64_t *rows_out,
                           double *agg, uint32_t *counts) {
    const McqTables &t = hs::luts();
    McqExactHeroQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    if (law != MCQ_LAW_REFERENCE && law != MCQ_LAW_UNIFORM) return -1;
    const int why = mcq_exact_hero_pre_query(mcq_query_words(*q), er, law, e);
    if (why) return why;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e.x, r_id);
    std::vector<uint8_t> cb_tab(MCQ_XP_MAX_PAIRS);
    mcq_exact_ext_cb_table(e.x, r_id, 0u, 1u, cb_tab.data());
    std::vector<uint16_t> allowed(MCQ_XP_MAX_PAIRS), live(MCQ_XP_MAX_PAIRS), ranked(MCQ_XP_MAX_PAIRS), pair_xy(MCQ_XP_MAX_PAIRS);
    uint32_t n[3];
    mcq_exact_hero_pre_lists(e, r_id, cb_tab.data(), allowed.data(), live.data(), ranked.data(), n);
    e.n_allowed = n[0];
    if (e.n_allowed == 0u) return MCQ_XH_EMPTY;
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
    /* the completions are shared out among a few host threads, each with its own keys, records and sums (the kernel's
     * blocks likewise); a thread's sums are 32-bit as the kernel's, checked against the bound the plan keeps */
    const uint32_t n_thr = host_threads(hi - lo);
    if (mcq_exact_hero_pre_owned(hi - lo, n_thr) > MCQ_XP_MAX_OWNED) return -2;
    const McqExactHeroSums zero = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
    std::vector<std::vector<McqExactHeroSums>> part(n_thr, std::vector<McqExactHeroSums>(e.n_allowed, zero));
    auto work = [&](uint32_t thr) {
        std::vector<uint32_t> keys(MCQ_XP_MAX_PAIRS), rec(MCQ_XP_MAX_PAIRS);
        std::vector<McqExactHeroSums> &mine = part[thr];
        /* a run of consecutive completions per thread, as a block's: the first one unranked, the others by stepping */
        const uint32_t run = mcq_exact_hero_pre_owned(hi - lo, n_thr), b0 = lo + thr * run, b1 = hi - b0 < run ? hi : b0 + run;
        uint32_t pos[5];
        if (b0 < hi) mcq_exact_unrank(b0, e.x.b.L, e.x.b.k, pos);
        for (uint32_t board = b0; board < b1 && b0 < hi; board++) {
            if (board != b0) mcq_exact_hero_pre_next(pos, e.x.b.k);
            McqExactBoard bd;
            mcq_exact_hero_board(e.x.b, pos, r_id, bd);
            const uint64_t taken = mcq_exact_hero_pre_mask(e.x.b, pos);
            for (uint32_t lane = 0; lane < 1024u; lane++)
                mcq_exact_hero_pre_rank(e, bd, taken, lane, 1024u, ranked.data(), n[2], pair_xy.data(), d_card, cb_tab.data(),
                                        t.tf, t.tops, t.sd, keys.data(), rec.data());
            for (uint32_t idx = 0; idx < e.n_allowed; idx++) { /* hand idx & 1023 of group idx >> 10 */
                const uint32_t own = allowed[idx], hxy = pair_xy[ranked[own]], qa = hxy & 0xFFu, qb = hxy >> 8;
                if (keys[own] == 0u) continue;
                const uint32_t first = idx & ~1023u, n_g = e.n_allowed - first < 1024u ? e.n_allowed - first : 1024u;
                const uint32_t share = mcq_exact_hero_pre_share(n_g);
                for (uint32_t sub = 0; sub < share; sub++) { /* the threads that share this hand's walk */
                    McqExactAcc acc = {0, 0, 0};
                    const uint32_t type =
                        mcq_exact_hero_pre_walk(e, bd, qa, qb, own, live.data(), n[1], sub, share, keys.data(), rec.data(), acc);
                    mcq_exact_hero_add(mine[idx], acc, type);
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
        for (uint32_t thr = 0; thr < n_thr; thr++) { /* across "launches": 64-bit */
            const McqExactHeroSums &a = part[thr][idx];
            r.runs += a.tot;
            r.win += a.win;
            r.tie += a.tie;
            for (uint32_t k = 0; k < 9; k++) r.by_type[k] += a.type[k];
        }
    }
    mcq_exact_prob p;
    if (whole && !mcq_exact_hero_finish(e, r_id, rows.data(), p)) return MCQ_XH_UNDEALABLE;
    memcpy(rows_out, rows.data(), MCQ_XH_ROWS * sizeof(mcq_result));
    if (whole) memcpy(agg, &p, sizeof p);
    counts[0] = n[0];
    counts[1] = n[1];
    counts[2] = n[2];
    counts[3] = n_boards;
    return 0;
}

// the rows of the allowed hero hands in list order (position i of `allowed` -> its row) -> their number, or -1
extern "C" int hs_hero_pre_allowed(const mcq_query *q, const mcq_query_ext *x, uint32_t *row_of) {
    McqExactHeroQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    if (mcq_exact_hero_pre_query(mcq_query_words(*q), er, MCQ_LAW_REFERENCE, e)) return -1;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e.x, r_id);
    std::vector<uint8_t> cb_tab(MCQ_XP_MAX_PAIRS);
    mcq_exact_ext_cb_table(e.x, r_id, 0u, 1u, cb_tab.data());
    std::vector<uint16_t> allowed(MCQ_XP_MAX_PAIRS), live(MCQ_XP_MAX_PAIRS), ranked(MCQ_XP_MAX_PAIRS);
    uint32_t n[3];
    mcq_exact_hero_pre_lists(e, r_id, cb_tab.data(), allowed.data(), live.data(), ranked.data(), n);
    for (uint32_t i = 0; i < n[0]; i++) {
        uint32_t qa, qb;
        mcq_exact_pair_xy(ranked[allowed[i]], qa, qb);
        row_of[i] = mcq_exact_hero_row(r_id, qa, qb);
    }
    return (int)n[0];
}

// mcq_exact_unrank and mcq_exact_binom as they are: out[5 i ..] = the positions of idx[i]
extern "C" void hs_unrank(const uint32_t *idx, uint32_t n, uint32_t L, uint32_t k, uint32_t *out) {
    for (uint32_t i = 0; i < n; i++) mcq_exact_unrank(idx[i], L, k, out + 5u * i);
}
// out[5 i ..] = the completion that follows in[5 i ..] (mcq_exact_hero_pre_next)
extern "C" void hs_next(const uint32_t *in, uint32_t n, uint32_t k, uint32_t *out) {
    for (uint32_t i = 0; i < n; i++) {
        memcpy(out + 5u * i, in + 5u * i, 20);
        mcq_exact_hero_pre_next(out + 5u * i, k);
    }
}
extern "C" uint32_t hs_binom(uint32_t n, uint32_t k) { return mcq_exact_binom(n, k); }

// what the host plan is made of
extern "C" uint32_t hs_pre_slice(uint64_t want) { return mcq_exact_hero_pre_slice(want); }
extern "C" uint32_t hs_pre_owned(uint32_t slice, uint32_t per) { return mcq_exact_hero_pre_owned(slice, per); }
extern "C" uint32_t hs_pre_max_owned(void) { return MCQ_XP_MAX_OWNED; }
extern "C" uint32_t hs_pre_share(uint32_t n_g) { return mcq_exact_hero_pre_share(n_g); }

// ---------------------------------------------------------------------------------------------------------------------
// The SLOW REFERENCE, deliberately different: one hero hand at a time.  Its deck is R = D minus the hand and everything
// is an R-position: the opponent's weight is the FIRST hand's (mcq_exact_ext_cbits / mcq_exact_ext_w1 on R), and under the
// reference law a completion T counts iff some card of R above max(T) is outside the opponent's hand.  The completions are
// the same ones -- those of D with the indices [lo, lo + count) in the combinatorial number system, reached by stepping
// from the combination `start` (D-positions, ascending: the caller unranks lo) --, and those that hit the hand are skipped.
// Only mcq_eval_key and the two weight functions are shared with the code under test.
// hands: n_hands x 2 card ids (a < b, both in D); rows_out: n_hands x 13 words (runs, 0, win, tie, by_type[9]).
extern "C" int hs_slow_ref(const uint8_t *deck, uint32_t Ld, const uint32_t *opp_bits, int law, const uint32_t *start,
                           uint32_t count, const uint8_t *hands, uint32_t n_hands, uint64_t *rows_out) {
    const McqTables &t = hs::luts();
    const bool ref = law == MCQ_LAW_REFERENCE;
    auto one = [&](uint32_t hi_) {
        const uint32_t ha = hands[2u * hi_], hb = hands[2u * hi_ + 1u];
        uint8_t r_id[64];
        uint32_t Lr = 0;
        for (uint32_t i = 0; i < Ld; i++)
            if (deck[i] != ha && deck[i] != hb) r_id[Lr++] = deck[i];
        McqExactExtQuery ex;
        memset(&ex, 0, sizeof ex);
        for (uint32_t i = 0; i < 6; i++) ex.bits[i] = opp_bits[i];
        uint64_t *row = rows_out + 13u * hi_;
        for (uint32_t i = 0; i < 13; i++) row[i] = 0;
        uint32_t c[5] = {start[0], start[1], start[2], start[3], start[4]};
        for (uint32_t n = 0; n < count; n++) {
            bool hit = false;
            uint64_t tmask = 0;
            McqBoard b;
            b.clear();
            for (uint32_t i = 0; i < 5; i++) {
                const uint32_t card = deck[c[i]];
                hit |= card == ha || card == hb;
                tmask |= 1ull << card;
                b.add(mcq_card(card));
            }
            if (!hit) {
                McqFlushSel fs;
                fs.from_board(b);
                McqHole hh;
                hh.set(mcq_card(ha), mcq_card(hb));
                const uint32_t kh = mcq_eval_key(b, fs, hh, t.tf, t.tops, t.sd), type = mcq_key_type(kh);
                const uint32_t max_t = deck[c[4]];
                uint32_t above_r = 0; /* cards of R above max(T) */
                for (uint32_t p = 0; p < Lr; p++) above_r += r_id[p] > max_t ? 1u : 0u;
                uint64_t win = 0, tie = 0, tot = 0;
                for (uint32_t pb = 1; pb < Lr; pb++) {
                    if ((tmask >> r_id[pb]) & 1ull) continue;
                    for (uint32_t pa = 0; pa < pb; pa++) {
                        if ((tmask >> r_id[pa]) & 1ull) continue;
                        const uint32_t w = mcq_exact_ext_w1(ref, mcq_exact_ext_cbits(ex, r_id, pa, pb), pa, pb);
                        if (w == 0u) continue;
                        const uint32_t in_hand = (r_id[pa] > max_t ? 1u : 0u) + (r_id[pb] > max_t ? 1u : 0u);
                        if (ref && above_r - in_hand == 0u) continue;
                        McqHole oh;
                        oh.set(mcq_card(r_id[pa]), mcq_card(r_id[pb]));
                        const uint32_t ko = mcq_eval_key(b, fs, oh, t.tf, t.tops, t.sd);
                        tot += w;
                        if (ko < kh) win += w;
                        if (ko == kh) tie += w;
                    }
                }
                row[0] += tot;
                row[2] += win;
                row[3] += tie;
                row[4u + type] += win + tie;
            }
            /* the next combination in the order of the combinatorial number system (colex) */
            uint32_t i = 0;
            while (i < 4u && c[i] + 1u == c[i + 1u]) i++;
            c[i]++;
            for (uint32_t j = 0; j < i; j++) c[j] = j;
            if (c[4] >= Ld && n + 1u < count) return;
        }
    };
    const uint32_t n_thr = host_threads(n_hands);
    std::vector<std::thread> pool;
    for (uint32_t thr = 0; thr < n_thr; thr++)
        pool.emplace_back([&, thr] { for (uint32_t h = thr; h < n_hands; h += n_thr) one(h); });
    for (std::thread &th : pool) th.join();
    return 0;
}
