// mcq_stage.hpp -- what a BLOCK of the Monte-Carlo kernels decides and lays out before its waves start: which of its
// records' candidate lists (extended queries) or prepared tables (a weighted range per seat) it keeps in LDS, and the
// per-thread steps of the candidate lists' compaction.  Plain integer code, written MCQ_HD: mcq_kernels.hip compiles it
// for gfx950, tests/hostsim_stage for the host.  One thread of a block runs a staging decision, once; a block's records
// are those of mcq_axis_block_records (mcq_axis.hpp).
#pragma once
#include "mcq_axis.hpp"
#include "mcq_ranges.hpp"

// ---------------------------------------------------------------------------------------------- extended queries
#define MCQ_EXT_STAGE_ENTRIES (18u * 1024u) /* 16-bit entries of candidate lists a block keeps in LDS (36 KB) */
#define MCQ_EXT_STAGE_LISTS 96u             /* ... in at most this many lists (their offsets: one more word) */

/* Do the candidate lists of records first .. first + nq - 1 fit (cnts[record * lists_stride + li] = a list's length)?
 * A list takes whole 32-bit words.  off[k] = where list k of the nq * lists_stride begins, off[nq * lists_stride] = where
 * the last one ends: written when the lists are at most MCQ_EXT_STAGE_LISTS, up to the first that begins beyond the
 * capacity, and the closing entry always -- so off has MCQ_EXT_STAGE_LISTS + 1 entries. */
MCQ_HD bool mcq_ext_stage_lists(uint32_t first, uint32_t nq, uint32_t lists_stride, const uint32_t *cnts, uint32_t *off) {
    if (nq == 0u || (uint64_t)nq * lists_stride > MCQ_EXT_STAGE_LISTS) return false;
    uint32_t at = 0;
    for (uint32_t k = 0; k < nq * lists_stride; k++) {
        off[k] = at;
        at += (cnts[(size_t)first * lists_stride + k] + 1u) & ~1u; /* whole 32-bit words */
        if (at > MCQ_EXT_STAGE_ENTRIES) break;
    }
    off[nq * lists_stride] = at;
    return at <= MCQ_EXT_STAGE_ENTRIES;
}

// ---------------------------------------------------------------------------------------------- a weighted range per seat
/* The distinct tables that records first .. first + nq - 1 draw from -> tab_id[0 .. the number returned), in the order
 * the seats name them; 0: nothing is staged (no record, more than MCQ_RG_STAGE_QUERIES of them, a table beyond
 * MCQ_RG_STAGE_TABLES, or known hands only).  query_words: the records, four words each; seats at or above a record's
 * n_players are not read; a table with one entry is a known hand, which reads no table.  MAX_TABLES: the room of the
 * kernel that asks (mcq_eval_ranges_hands_kernel keeps MCQ_RG_HANDS_STAGE_TABLES beside its table of hands). */
template <uint32_t MAX_TABLES = MCQ_RG_STAGE_TABLES>
MCQ_HD uint32_t mcq_ranges_stage_tables(const uint32_t *query_words, const uint32_t *seat_table, const uint32_t *cum,
                                        uint32_t first, uint32_t nq, uint32_t *tab_id /* MAX_TABLES entries */) {
    uint32_t n_tab = 0;
    bool fits = nq <= MCQ_RG_STAGE_QUERIES;
    for (uint32_t j = 0; j < nq && fits; j++) {
        const uint32_t p = query_words[(size_t)(first + j) * 4u + 2u] & 0xFFu; /* McqQueryWords::n_players */
        for (uint32_t s = 0; s < p && s < MCQ_MAX_SEATS && fits; s++) {
            const uint32_t t = seat_table[(size_t)(first + j) * MCQ_MAX_SEATS + s];
            if (cum[(size_t)t * MCQ_RG_CUM_STRIDE + MCQ_RG_NNZ_WORD] == 1u) continue; /* a known hand reads no table */
            uint32_t k = 0;
            while (k < n_tab && tab_id[k] != t) k++;
            if (k < n_tab) continue;
            if (n_tab == MAX_TABLES) fits = false;
            else tab_id[n_tab++] = t;
        }
    }
    return fits ? n_tab : 0u;
}
/* the slot of table t among the n_staged >= 1 staged ones; t is one of them (every table of a staged record is) */
MCQ_HD uint32_t mcq_ranges_stage_slot(const uint32_t *tab_id, uint32_t n_staged, uint32_t t) {
    uint32_t k = 0;
    while (k + 1u < n_staged && tab_id[k] != t) k++;
    return k;
}

// ---------------------------------------------------------------------------------------------- candidate lists
/* A list = all ordered pairs (a, b) of cards of U whose class `set` allows, in the order of c = 52 * a + b.  Thread i
 * looks at the PER consecutive candidates from PER * i on: bit k of its mask = candidate PER * i + k is on the list.
 * With `at` = the survivors of all lower threads (an exclusive sum of the masks' populations) it writes its own as
 * a | b << 8 from dst[at] on; returns where it stopped. */
template <uint32_t PER>
MCQ_HD uint32_t mcq_ext_list_mask(uint64_t U, const uint32_t *set, uint32_t thread) {
    static_assert(PER >= 1u && PER <= 32u, "one bit per candidate");
    uint32_t mask = 0;
    for (uint32_t k = 0; k < PER; k++)
        if (mcq_ext_candidate(U, set, thread * PER + k)) mask |= 1u << k;
    return mask;
}
template <uint32_t PER>
MCQ_HD uint32_t mcq_ext_list_scatter(uint32_t mask, uint32_t thread, uint32_t at, uint16_t *dst) {
    for (uint32_t k = 0; k < PER; k++)
        if ((mask >> k) & 1u) {
            const uint32_t c = thread * PER + k, a = c / 52u;
            dst[at++] = (uint16_t)(a | ((c - 52u * a) << 8));
        }
    return at;
}
