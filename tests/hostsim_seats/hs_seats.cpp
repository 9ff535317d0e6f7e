// hs_seats.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the product's EXTENDED lane code with the per-seat switch ON (McqLaneAccSeats: mcq_iteration_ext,
// neuron_poker_amd/csrc/mcq_device.hpp) for the HOST compiler and walks the kernel's stream / lane decomposition
// sequentially, as tests/hostsim_ext_ways does for the split-pot form: one McqLaneAccSeats per stream, unpacked into the
// 32-word row as WaveTallySeats unpacks it.  It also hands back every iteration's dealt hands (MCQ_EXT_DEAL_HOOK, host
// builds only), from which the tests recount every seat with the oracle's own comparison, and walks the all-in
// enumeration's per-seat lane code (mcq_exact_ext_lone_seats, mcq_exact_ext.hpp) completion by completion.
#include <stdint.h>
#include <string.h>

#include <vector>

namespace {
thread_local uint8_t *g_hands = nullptr; /* the current iteration's record: n_players x 2 ids, then five table ids */
thread_local uint32_t g_players = 0, g_board = 0;
inline void hs_dealt(uint32_t h, uint32_t c1, uint32_t c2) {
    if (!g_hands) return;
    if (h >= 0x100u) g_hands[2u * g_players + g_board + (h - 0x100u)] = (uint8_t)c1; /* table card number h - 0x100 to come */
    else { g_hands[2u * h] = (uint8_t)c1; g_hands[2u * h + 1u] = (uint8_t)c2; }
}
}  // namespace
#define MCQ_EXT_DEAL_HOOK(h, c1, c2) hs_dealt(h, c1, c2)

#include "../hostsim/hs_walk.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_ext.hpp"

extern "C" {

// MCQ-CTR v5x streams of (seed, qid), every iteration through mcq_iteration_ext.  out: 32 words.
// hands (may be null): runs x (2 n_players + 5) card ids.
int hs_seats_run(const mcq_query *q, const mcq_query_ext *e, uint64_t seed, uint64_t qid, mcq_result_seats *out, uint8_t *hands) {
    hs::ExtQuery x(q, e);
    if (!x.valid || x.empty_list) return MCQ_EINVAL;
    const McqTables &t = hs::luts();
    const uint32_t rec = 2u * q->n_players + 5u;
    g_players = q->n_players;
    g_board = q->n_board;
    struct Unhook { ~Unhook() { g_hands = nullptr; } } unhook;
    return x.walk<McqLaneAccSeats>(seed, qid, reinterpret_cast<uint64_t *>(out), [&](McqExtCtrDraws &dr, McqLaneAccSeats &acc, uint64_t it) {
        if (hands) {
            g_hands = hands + it * rec;
            for (uint32_t k = 0; k < q->n_board; k++) g_hands[2u * q->n_players + k] = q->board[k];
        }
        return mcq_iteration_ext<McqExtCtrDraws, false, McqLaneAccSeats>(x.qc, x.wc, dr, x.cards, t.sel8, x.ids, 1, t.tf, t.tops, t.sd, acc);
    });
}

// The all-in enumeration's per-seat lane code, walked as mcq_exact_ext_kernel<0, MCQ_ROW_SEATS> walks it.
// -> 0, MCQ_XX_* (1..4), 5 = cannot be dealt, 7 = a random opponent.  weights: 32 words.
int hs_seats_exact(const mcq_query *q, const mcq_query_ext *x, int law, mcq_result_seats *weights) {
    const McqTables &t = hs::luts();
    McqExactExtQuery e;
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(x)};
    const int why = mcq_exact_ext_query(mcq_query_words(*q), er, law, e);
    if (why) return why;
    uint8_t r_id[64];
    mcq_exact_ext_r_ids(e, r_id);
    if (!mcq_exact_ext_dealable(e, r_id)) return 5;
    if (e.b.n_opp != 0u) return 7;
    mcq_result_seats w;
    memset(&w, 0, sizeof w);
    const uint32_t n_boards = mcq_exact_binom(e.b.L, e.b.k);
    for (uint32_t board = 0; board < n_boards; board++) {
        uint32_t level, k;
        const uint32_t wt = mcq_exact_ext_lone_seats(e, board, t.sel8, t.tf, t.tops, t.sd, level, k);
        if (!wt) continue;
        const uint32_t inc = mcq_seat_increment(k);
        w.runs += wt;
        for (uint32_t s = 0; s < MCQ_MAX_SEATS; s++) {
            if (!((level >> s) & 1u)) continue;
            w.seat[s].share += inc & 0xFFFFu;
            w.seat[s].win += (inc >> MCQ_SEAT_WIN_SHIFT) & 1u;
            w.seat[s].tie += (inc >> MCQ_SEAT_TIE_SHIFT) & 1u;
        }
    }
    memcpy(weights, &w, sizeof w);
    return 0;
}
}
