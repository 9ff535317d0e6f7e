// hs_matrix.cpp -- TEST HARNESS ONLY (built and loaded by tests/, never by the product).
//
// Compiles the lane code of the hand-against-hand matrix (neuron_poker_amd/csrc/mcq_exact_matrix.hpp) for the HOST compiler
// and walks the three kernels' decomposition on the CPU -- the key table row by row with its padding, then tile by tile and
// stage by stage the 256 threads' register tiles fed from a staged image with the column words turned, then every entry of
// the [1326][1326] matrices from the counts by D-pair --, so that the GPU's output can be pinned bit for bit and the lane
// code checked against an independent walk in a container without a GPU.
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../hostsim/hs_walk.hpp"
#include "../../neuron_poker_amd/csrc/mcq_exact_matrix.hpp"

// -> 0, the refusal MCQ_XM_* (1..7), or -2 (no win matrix).  win, tie: [1326][1326] uint16 (tie may be null), total: one
// word (may be null); all untouched by a refusal.
extern "C" int hs_matrix(const mcq_matrix_query *q, uint16_t *win, uint16_t *tie, uint32_t *total) {
    const McqTables &t = hs::luts();
    if (!win) return -2;
    McqMatrixQuery e;
    const int why = mcq_matrix_query_build(*q, e);
    if (why) return why;
    uint8_t r_id[64], pos_of[52];
    mcq_matrix_r_ids(e, r_id);
    const uint32_t stride = mcq_matrix_stride(e.n_rp), stages = mcq_matrix_stages(e.n_boards), rows = stages * MCQ_XM_STAGE;
    std::vector<uint16_t> pair_xy(MCQ_XH_MAX_HANDS);
    for (uint32_t i = 0; i < MCQ_XH_MAX_HANDS; i++) {
        uint32_t a, b;
        mcq_exact_pair_xy(i, a, b);
        pair_xy[i] = (uint16_t)(a | (b << 8));
    }
    /* (a) the key table, its padding written as dead */
    std::vector<uint32_t> keys((size_t)rows * stride);
    for (uint32_t board = 0; board < rows; board++) {
        uint32_t *row = &keys[(size_t)board * stride];
        if (board >= e.n_boards) {
            for (uint32_t rp = 0; rp < stride; rp++) row[rp] = 0u;
            continue;
        }
        uint32_t pos[5];
        mcq_exact_unrank(board, e.b.L, e.b.k, pos);
        McqExactBoard bd;
        mcq_exact_hero_board(e.b, pos, r_id, bd);
        for (uint32_t rp = 0; rp < stride; rp++)
            row[rp] = rp < e.n_rp ? mcq_matrix_rank(bd, pos, r_id, pair_xy[rp], t.tf, t.tops, t.sd) : 0u;
    }
    /* (b) the counts by D-pair: a tile per block, shared out among a few host threads (a tile has one owner) */
    const uint32_t tiles = stride / MCQ_XM_TILE, per_side = MCQ_XM_TILE / MCQ_XM_TG;
    std::vector<uint16_t> cnt((size_t)stride * stride);
    uint32_t n_thr = std::thread::hardware_concurrency();
    n_thr = n_thr < 1u ? 1u : n_thr > 8u ? 8u : n_thr;
    n_thr = n_thr > tiles * tiles ? tiles * tiles : n_thr;
    auto work = [&](uint32_t thr) {
        std::vector<uint32_t> buf((size_t)MCQ_XM_STAGE * 2u * MCQ_XM_TILE);
        std::vector<uint32_t> acc((size_t)MCQ_XM_TILE * MCQ_XM_TILE);
        for (uint32_t tile = thr; tile < tiles * tiles; tile += n_thr) {
            const uint32_t row0 = tile / tiles * MCQ_XM_TILE, col0 = tile % tiles * MCQ_XM_TILE;
            std::fill(acc.begin(), acc.end(), 0u);
            for (uint32_t s = 0; s < stages; s++) {
                for (uint32_t c = 0; c < MCQ_XM_STAGE; c++) { /* the staged image */
                    const uint32_t *src = &keys[(size_t)(s * MCQ_XM_STAGE + c) * stride];
                    uint32_t *dst = &buf[(size_t)c * 2u * MCQ_XM_TILE];
                    for (uint32_t i = 0; i < MCQ_XM_TILE; i++) {
                        dst[i] = src[row0 + i];
                        dst[MCQ_XM_TILE + i] = mcq_matrix_col(src[col0 + i]);
                    }
                }
                for (uint32_t tid = 0; tid < per_side * (MCQ_XM_TILE / MCQ_XM_TH); tid++) { /* thread (ty, tx) */
                    const uint32_t tx = tid % per_side, ty = tid / per_side;
                    uint32_t reg[MCQ_XM_TH][MCQ_XM_TG];
                    for (uint32_t a = 0; a < MCQ_XM_TH; a++)
                        for (uint32_t b = 0; b < MCQ_XM_TG; b++) reg[a][b] = acc[(size_t)(ty * MCQ_XM_TH + a) * MCQ_XM_TILE + tx * MCQ_XM_TG + b];
                    for (uint32_t c = 0; c < MCQ_XM_STAGE; c++) {
                        const uint32_t *st = &buf[(size_t)c * 2u * MCQ_XM_TILE];
                        mcq_matrix_count<MCQ_XM_TH, MCQ_XM_TG>(reg, st + ty * MCQ_XM_TH, st + MCQ_XM_TILE + tx * MCQ_XM_TG);
                    }
                    for (uint32_t a = 0; a < MCQ_XM_TH; a++)
                        for (uint32_t b = 0; b < MCQ_XM_TG; b++) acc[(size_t)(ty * MCQ_XM_TH + a) * MCQ_XM_TILE + tx * MCQ_XM_TG + b] = reg[a][b];
                }
            }
            for (uint32_t i = 0; i < MCQ_XM_TILE; i++)
                for (uint32_t j = 0; j < MCQ_XM_TILE; j++)
                    cnt[(size_t)(row0 + i) * stride + col0 + j] = (uint16_t)acc[(size_t)i * MCQ_XM_TILE + j];
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t thr = 1; thr < n_thr; thr++) pool.emplace_back(work, thr);
    work(0u);
    for (std::thread &th : pool) th.join();
    /* (c) every entry of the matrices */
    mcq_matrix_pos_of(e, r_id, pos_of);
    std::vector<uint16_t> cards(MCQ_XH_ROWS), dpair(MCQ_XH_ROWS);
    for (uint32_t lane = 0; lane < 256u; lane++) mcq_matrix_hands(pos_of, lane, 256u, cards.data(), dpair.data());
    for (uint32_t r = 0; r < MCQ_XH_ROWS; r++)
        for (uint32_t c = 0; c < MCQ_XH_ROWS; c++) {
            uint32_t w, ti;
            mcq_matrix_entry(e, cnt.data(), stride, cards.data(), dpair.data(), r, c, w, ti);
            win[(size_t)r * MCQ_XH_ROWS + c] = (uint16_t)w;
            if (tie) tie[(size_t)r * MCQ_XH_ROWS + c] = (uint16_t)ti;
        }
    if (total) *total = e.total;
    return 0;
}
