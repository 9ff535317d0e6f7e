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

#include "../../neuron_poker_amd/csrc/mcq_device.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_ext.hpp"
#include "../../neuron_poker_amd/csrc/mcq_tally.hpp"

namespace {
McqTables g_tab;
bool g_init = false;
const McqTables &luts() {
    if (!g_init) { mcq_fill_tables(&g_tab); g_init = true; }
    return g_tab;
}
}  // namespace

extern "C" {

// MCQ-CTR v5x streams of (seed, qid), every iteration through mcq_iteration_ext.  out: 32 words.
// hands (may be null): runs x (2 n_players + 5) card ids.
int hs_seats_run(const mcq_query *q, const mcq_query_ext *e, uint64_t seed, uint64_t qid, mcq_result_seats *out, uint8_t *hands) {
    const McqExtRec er = {reinterpret_cast<const uint32_t *>(e)};
    const McqQueryWords qw = mcq_query_words(*q);
    if (!mcq_query_ext_valid(qw, er)) return MCQ_EINVAL;
    const McqTables &t = luts();
    McqExtCtx qc;
    mcq_ext_ctx(qw, er, qc);
    McqExtWaveCtx wc;
    memset(&wc, 0, sizeof wc);
    for (uint32_t h = 0; h < qc.n_hands; h++) wc.hand[h] = mcq_ext_hand(qw, er, h);
    const uint32_t n_lists = mcq_ext_n_lists(qw, er);
    std::vector<uint16_t> lists((size_t)(n_lists ? n_lists : 1) * MCQ_EXT_LIST_STRIDE);
    for (uint32_t li = 0; li < n_lists; li++) { /* as mcq_ext_lists_kernel lays them out */
        uint64_t U;
        uint32_t set_off, cnt = 0;
        mcq_ext_list_plan(qw, er, li, U, set_off);
        for (uint32_t c = 0; c < 2704u; c++)
            if (mcq_ext_candidate(U, er.w + set_off, c)) lists[(size_t)li * MCQ_EXT_LIST_STRIDE + cnt++] = (uint16_t)((c / 52u) | ((c % 52u) << 8));
        wc.cnt[li] = cnt;
        wc.list[li] = lists.data() + (size_t)li * MCQ_EXT_LIST_STRIDE;
        if (cnt == 0) return MCQ_EINVAL;
    }
    McqCard cards[64];
    for (uint32_t c = 0; c < 64; c++) cards[c] = mcq_card(c < 52 ? c : 0);
    memset(out, 0, sizeof(*out));
    out->runs = q->runs;
    uint16_t ids[MCQ_MAX_OPP + 1];
    const uint32_t rec = 2u * q->n_players + 5u;
    g_players = q->n_players;
    g_board = q->n_board;
    struct Unhook { ~Unhook() { g_hands = nullptr; } } unhook;
    const uint32_t s_iters = mcq_ext_stream_iters(qw, er);
    const uint32_t n_streams = (q->runs + s_iters - 1) / s_iters;
    for (uint32_t s = 0; s < n_streams; s++) {
        McqExtCtrDraws dr;
        dr.start(seed, qid, s);
        McqLaneAccSeats acc = {};
        for (uint32_t j = 0; j < s_iters; j++) {
            const uint64_t it = (uint64_t)s * s_iters + j;
            if (it >= q->runs) break;
            if (hands) {
                g_hands = hands + it * rec;
                for (uint32_t k = 0; k < q->n_board; k++) g_hands[2u * q->n_players + k] = q->board[k];
            }
            if (!mcq_iteration_ext<McqExtCtrDraws, false, McqLaneAccSeats>(qc, wc, dr, cards, t.sel8, ids, 1, t.tf, t.tops, t.sd, acc))
                return MCQ_EINVAL;
        }
        mcq_tally_fold(acc, reinterpret_cast<uint64_t *>(out));
    }
    return MCQ_OK;
}

// The all-in enumeration's per-seat lane code, walked as mcq_exact_ext_kernel<0, MCQ_ROW_SEATS> walks it.
// -> 0, MCQ_XX_* (1..4), 5 = cannot be dealt, 7 = a random opponent.  weights: 32 words.
int hs_seats_exact(const mcq_query *q, const mcq_query_ext *x, int law, mcq_result_seats *weights) {
    const McqTables &t = luts();
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
