// hs_sum.cpp -- TEST-ONLY host build of the sum-form evaluator (rank-sum hash, ids instead of keys).
//
// Compiles neuron_poker_amd/csrc/mcq_device.hpp for the HOST compiler and exposes the sum-form tables, the rank
// multisets they are built from, and a sweep of the sum-form key beside mcq_eval_key over all 7-card hands.
#include <thread>

#include "../hostsim/hs_walk.hpp"

namespace {
struct Checked { /* the filled tables with the sum form built again, for the verdict */
    McqTables t;
    uint32_t n_ids[MCQ_N_CODES];
    bool ok;
    Checked() : t(hs::luts()) { ok = mcq_fill_sum_tables_checked(&t, n_ids); }
};
const Checked &checked() {
    static const Checked c;
    return c;
}
const McqTables &checked_tables() { return checked().t; }
}  // namespace

extern "C" {
// sizes: rows, slots, shift, bytes of the LDS image, 1 if the tables fit, then the ids per type code (MCQ_N_CODES)
void hs_sum_info(uint32_t *out) {
    out[0] = MCQ_SUM_ROWS; out[1] = MCQ_SUM_SLOTS; out[2] = MCQ_SUM_SHIFT; out[3] = (uint32_t)sizeof(McqSumImage);
    out[4] = checked().ok ? 1u : 0u;
    for (uint32_t c = 0; c < MCQ_N_CODES; c++) out[5 + c] = checked().n_ids[c];
}
void hs_sum_tables(uint16_t *hoff, uint16_t *hrank, uint32_t *tfid, uint32_t *tf) {
    const McqTables &t = checked_tables();
    memcpy(hoff, t.sum.hoff, sizeof(t.sum.hoff));
    memcpy(hrank, t.sum.hrank, sizeof(t.sum.hrank));
    memcpy(tfid, t.tfid, sizeof(t.tfid));
    memcpy(tf, t.tf, 8192 * sizeof(uint32_t));
}
void hs_sum_weights(uint32_t *w) {
    for (uint32_t r = 0; r < 13; r++) w[r] = mcq_rank_weight(r);
}
// Every rank multiset (seven cards, at most four of a rank), enumerated here by seven nested rank choices, not by the
// product's walk: its weight sum and its key by mcq_eval_key without a flush.  Returns their number (cap: 65536).
uint32_t hs_sum_multisets(uint32_t *sums, uint32_t *keys) {
    const McqTables &t = checked_tables();
    uint32_t n = 0, r[7];
    for (r[0] = 0; r[0] < 13; r[0]++) for (r[1] = r[0]; r[1] < 13; r[1]++) for (r[2] = r[1]; r[2] < 13; r[2]++)
    for (r[3] = r[2]; r[3] < 13; r[3]++) for (r[4] = r[3]; r[4] < 13; r[4]++) for (r[5] = r[4]; r[5] < 13; r[5]++)
    for (r[6] = r[5]; r[6] < 13; r[6]++) {
        if (r[0] == r[4] || r[1] == r[5] || r[2] == r[6]) continue; /* five of a rank */
        McqBoard b;
        b.clear();
        McqCard c[7];
        uint32_t s = 0;
        for (int k = 0; k < 7; k++) {
            c[k].rb = 4u << r[k];
            c[k].cnt = c[k].los = c[k].his = 0u;
            s += mcq_rank_weight(r[k]);
        }
        for (int k = 0; k < 5; k++) b.add(c[k]);
        McqFlushSel fs;
        fs.from_board(b);
        McqHole h;
        h.set(c[5], c[6]);
        if (n < 65536u) {
            sums[n] = s;
            keys[n] = mcq_eval_key(b, fs, h, t.tf, t.tops, t.sd);
        }
        n++;
    }
    return n;
}
// All 7-card hands whose lowest card c0 satisfies c0 % stride == phase (stride 1: all 133 784 560): the five lowest
// cards are the table, the two highest the hole.  key_of_id[id] = the mask-form key of the hands with that sum-form
// id.  Returns the number of hands seen; *bad counts hands whose id maps to two different keys or whose type
// (mcq_id_type) differs from mcq_key_type of the key.
uint64_t hs_sum_sweep(uint32_t threads, uint32_t stride, uint32_t phase, uint32_t *key_of_id /* 65536 */, uint64_t *bad) {
    const McqTables &t = checked_tables();
    const McqSumTabs st = mcq_sum_tabs_of(t.tf);
    if (threads < 1) threads = 1;
    std::vector<std::vector<uint32_t>> maps(threads, std::vector<uint32_t>(65536, 0u));
    std::vector<uint64_t> seen(threads, 0), wrong(threads, 0);
    auto work = [&](uint32_t tid) {
        std::vector<uint32_t> &map = maps[tid];
        uint32_t job = 0;
        for (uint32_t c0 = phase; c0 < 46; c0 += stride)
            for (uint32_t c1 = c0 + 1; c1 < 47; c1++) {
                if (job++ % threads != tid) continue;
                for (uint32_t c2 = c1 + 1; c2 < 48; c2++) for (uint32_t c3 = c2 + 1; c3 < 49; c3++)
                for (uint32_t c4 = c3 + 1; c4 < 50; c4++) {
                    const uint32_t tc[5] = {c0, c1, c2, c3, c4};
                    McqBoard b;
                    McqSumBoard sb;
                    b.clear();
                    sb.clear();
                    for (int k = 0; k < 5; k++) {
                        b.add(mcq_card(tc[k]));
                        sb.add(mcq_card_sum(tc[k]));
                    }
                    McqFlushSel fs, sfs;
                    fs.from_board(b);
                    sfs.from_board(sb);
                    for (uint32_t c5 = c4 + 1; c5 < 51; c5++) for (uint32_t c6 = c5 + 1; c6 < 52; c6++) {
                        McqHole h;
                        McqSumHole sh;
                        h.set(mcq_card(c5), mcq_card(c6));
                        sh.set(mcq_card_sum(c5), mcq_card_sum(c6));
                        const uint32_t key = mcq_eval_key(b, fs, h, t.tf, t.tops, t.sd);
                        const uint32_t id = mcq_sum_key(sb, sfs, sh, st);
                        seen[tid]++;
                        if (id > 0xFFFFu || mcq_id_type(id) != mcq_key_type(key)) { wrong[tid]++; continue; }
                        if (map[id] == 0u) map[id] = key;
                        else if (map[id] != key) wrong[tid]++;
                    }
                }
            }
    };
    std::vector<std::thread> pool;
    for (uint32_t i = 1; i < threads; i++) pool.emplace_back(work, i);
    work(0);
    for (auto &th : pool) th.join();
    uint64_t n = 0, w = 0;
    for (uint32_t i = 0; i < 65536u; i++) key_of_id[i] = 0u;
    for (uint32_t tid = 0; tid < threads; tid++) {
        n += seen[tid];
        w += wrong[tid];
        for (uint32_t i = 0; i < 65536u; i++) {
            if (!maps[tid][i]) continue;
            if (key_of_id[i] == 0u) key_of_id[i] = maps[tid][i];
            else if (key_of_id[i] != maps[tid][i]) w++;
        }
    }
    *bad = w;
    return n;
}
}
