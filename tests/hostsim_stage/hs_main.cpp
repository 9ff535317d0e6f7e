// hs_main.cpp -- TEST HARNESS ONLY: every function of neuron_poker_amd/csrc/mcq_stage.hpp driven at the bounds of its
// arrays by a program of its own, which the tests build with AddressSanitizer and UndefinedBehaviorSanitizer.  Every
// array is a heap block of exactly the size the kernels give it.  One line per case, then "ok: <cases>" or "FAILED".
#include <stdio.h>

#include "hs_stage.hpp"

namespace {
const uint32_t kNotWritten = 0xFFFFFFFFu;

/* nq records of lists_stride lists of `len` entries each, behind `first` records that must not be read as the block's */
bool ext_case(uint32_t first, uint32_t nq, uint32_t lists_stride, uint32_t len, bool want) {
    std::vector<uint32_t> cnts((size_t)(first + nq) * lists_stride, len), off(MCQ_EXT_STAGE_LISTS + 1u, kNotWritten);
    for (size_t k = 0; k < (size_t)first * lists_stride; k++) cnts[k] = 2704u;
    const bool staged = mcq_ext_stage_lists(first, nq, lists_stride, cnts.data(), off.data());
    const uint32_t n_l = nq * lists_stride, words = (len + 1u) & ~1u;
    bool ok = staged == want;
    if (n_l == 0u || n_l > MCQ_EXT_STAGE_LISTS) { /* no record, or refused by the count: nothing is written */
        for (uint32_t k = 0; k <= MCQ_EXT_STAGE_LISTS; k++) ok = ok && off[k] == kNotWritten;
        return ok && !staged;
    }
    uint32_t written = 0;
    for (uint32_t k = 0; k < n_l && (uint64_t)k * words <= MCQ_EXT_STAGE_ENTRIES; k++, written++) ok = ok && off[k] == k * words;
    if (staged) ok = ok && written == n_l && off[n_l] == n_l * words;
    else ok = ok && off[n_l] == written * words && off[n_l] > MCQ_EXT_STAGE_ENTRIES;
    for (uint32_t k = written; k < n_l; k++) ok = ok && off[k] == kNotWritten;
    for (uint32_t k = n_l + 1u; k <= MCQ_EXT_STAGE_LISTS; k++) ok = ok && off[k] == kNotWritten;
    return ok;
}

/* nq records of `seats` seats behind `first` others; seat s of record j draws from table (j + s) % n_named, and the
 * tables from n_named on are known hands, one of which sits on every record's last seat when `known` */
uint32_t ranges_case(uint32_t first, uint32_t nq, uint32_t seats, uint32_t n_named, bool known, std::vector<uint32_t> &tab_id) {
    const uint32_t n = first + nq, n_tables = n_named + 4u;
    std::vector<uint32_t> q((size_t)n * 4u, 0u), seat((size_t)n * MCQ_MAX_SEATS, kNotWritten), cum((size_t)n_tables * MCQ_RG_CUM_STRIDE, 0u);
    for (uint32_t t = 0; t < n_tables; t++) cum[(size_t)t * MCQ_RG_CUM_STRIDE + MCQ_RG_NNZ_WORD] = t < n_named ? 300u : 1u;
    for (uint32_t j = 0; j < n; j++) {
        q[(size_t)j * 4u + 2u] = seats | 0x03000000u; /* (the word's other bytes are not the seats') */
        for (uint32_t s = 0; s < seats; s++) seat[(size_t)j * MCQ_MAX_SEATS + s] = (j + s) % n_named;
        if (known) seat[(size_t)j * MCQ_MAX_SEATS + seats - 1u] = n_named + j % 4u;
    }
    tab_id.assign(MCQ_RG_STAGE_TABLES, kNotWritten);
    return mcq_ranges_stage_tables(q.data(), seat.data(), cum.data(), first, nq, tab_id.data());
}

bool list_case(uint64_t U, const uint32_t *set, uint32_t want_len) {
    std::vector<uint16_t> serial;
    for (uint32_t c = 0; c < 2704u; c++)
        if (mcq_ext_candidate(U, set, c)) serial.push_back((uint16_t)((c / 52u) | ((c % 52u) << 8)));
    return serial.size() == want_len && hs::compact<11, 256>(U, set) == serial && hs::compact<3, 1024>(U, set) == serial;
}
}  // namespace

int main() {
    unsigned cases = 0, failed = 0;
    auto report = [&](const char *what, bool ok) {
        printf("%s: %s\n", what, ok ? "holds" : "DIFFERS");
        cases++;
        failed += ok ? 0u : 1u;
    };
    /* 96 lists: the closing offset is the 97th entry */
    report("ext, 96 records of one list", ext_case(3, 96, 1, 191, true));
    report("ext, 97 records of one list", ext_case(3, 97, 1, 2, false));
    report("ext, 9 records of 10 lists", ext_case(1, 9, 10, 101, true));
    report("ext, 10 records of 10 lists", ext_case(1, 10, 10, 1, false));
    report("ext, 96 lists that end on the capacity", ext_case(0, 96, 1, MCQ_EXT_STAGE_ENTRIES / 96u, true));
    report("ext, 96 lists, the last one beyond it", ext_case(0, 96, 1, MCQ_EXT_STAGE_ENTRIES / 96u + 1u, false));
    report("ext, 90 full lists", ext_case(2, 9, 10, 2704, false));
    report("ext, no record", ext_case(5, 0, 10, 7, false));
    {
        std::vector<uint32_t> id;
        bool ok = ranges_case(2, 32, 6, 6, false, id) == 6u;
        for (uint32_t k = 0; k < 6u; k++) ok = ok && id[k] == (2u + k) % 6u; /* in the order the seats name them */
        for (uint32_t k = 0; k < 6u; k++) ok = ok && mcq_ranges_stage_slot(id.data(), 6u, id[k]) == k;
        report("ranges, 32 records on six tables", ok);
        report("ranges, a seventh table", ranges_case(2, 32, 6, 7, false, id) == 0u);
        report("ranges, a 33rd record", ranges_case(2, 33, 6, 6, false, id) == 0u);
        ok = ranges_case(0, 32, 7, 6, true, id) == 6u;
        for (uint32_t k = 0; k < 6u; k++) ok = ok && mcq_ranges_stage_slot(id.data(), 6u, id[k]) == k;
        report("ranges, six tables and four known hands", ok);
        ok = ranges_case(0, 32, MCQ_MAX_SEATS, 1, false, id) == 1u && id[0] == 0u && id[1] == kNotWritten;
        report("ranges, ten seats on one table", ok && mcq_ranges_stage_slot(id.data(), 1u, 0u) == 0u);
        report("ranges, no record", ranges_case(4, 0, 2, 6, false, id) == 0u && id[0] == kNotWritten);
    }
    {
        const uint32_t every[hs::kSetWords] = {~0u, ~0u, ~0u, ~0u, ~0u, 0x1FFu}, none[hs::kSetWords] = {};
        uint32_t aces[hs::kSetWords] = {};
        const uint32_t aa = mcq_class_index(48, 49);
        aces[aa >> 5] = 1u << (aa & 31u);
        report("lists, the full deck and every class", list_case((1ull << 52) - 1ull, every, 2652));
        report("lists, no class", list_case((1ull << 52) - 1ull, none, 0));
        report("lists, no card", list_case(0, every, 0));
        report("lists, the two highest cards", list_case(3ull << 50, every, 2));
        report("lists, the aces", list_case((1ull << 52) - 1ull, aces, 12));
    }
    if (failed) printf("FAILED: %u of %u\n", failed, cases);
    else printf("ok: %u\n", cases);
    return failed ? 1 : 0;
}
