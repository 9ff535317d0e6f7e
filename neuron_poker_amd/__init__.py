"""neuron_poker_amd -- MI355X-native Monte-Carlo equity engine behind neuron_poker's equity call surface.

    from neuron_poker_amd import montecarlo_hip
    montecarlo_hip.get_equity({'AH', 'KH'}, set(), 2, 100000)          # tools.montecarlo_python.get_equity
    montecarlo_hip.MonteCarlo().run_montecarlo([['AH', 'KH']], [], 2, 1, maxRuns=10000, timeout=0, ghost_cards='')

The compute path is libmcq_hip.so (hand-written HIP for gfx950, C ABI in include/mcq.h) loaded through
ctypes; there is no CPU fallback -- importing works anywhere, evaluating needs the library and a GPU.
"""
from .cards import card_id, card_str, key_type, TYPES  # noqa: F401
from ._lib import (Engine, MODE_PHILOX, MODE_REPLAY_MT19937, QUERY_DTYPE, QUERY_EXT_DTYPE, RESULT_DTYPE, RESULT_WAYS_DTYPE, EXACT_PROB_WAYS_DTYPE, McqError,  # noqa: F401
                   RESULT_SEATS, RESULT_SEATS_DTYPE, SHARE_UNIT, seat_shares,
                   McqBusyError, pot_share, load_library, library_path, pack_queries, pack_query_ext, range_bits, class_bit, default_engine, Tables, hand_index, HAND_ROWS,
                   MultiEngine, MATRIX_QUERY_DTYPE, pack_matrix_query, HAND_ROW_DTYPE)
from .montecarlo_hip import get_seat_equities, get_seat_equities_exact, get_range_equity_exact, get_runout_equities, get_preflop_range_equity_exact, preflop_class_table, get_range_equity_exact_weighted, get_preflop_range_equity_exact_weighted, get_range_equities, get_equity_matrix, matrix_equity, get_range_hand_equities  # noqa: F401

__all__ = ["card_id", "card_str", "key_type", "TYPES", "Engine", "MODE_PHILOX", "MODE_REPLAY_MT19937", "QUERY_DTYPE",
           "QUERY_EXT_DTYPE", "RESULT_DTYPE", "RESULT_WAYS_DTYPE", "EXACT_PROB_WAYS_DTYPE", "RESULT_SEATS", "RESULT_SEATS_DTYPE", "SHARE_UNIT", "pot_share", "seat_shares", "get_seat_equities", "get_seat_equities_exact",
           "McqError", "McqBusyError", "load_library", "library_path", "pack_queries", "pack_query_ext",
           "range_bits", "class_bit", "default_engine", "Tables", "MultiEngine", "hand_index", "HAND_ROWS",
           "get_range_equity_exact", "get_runout_equities", "get_preflop_range_equity_exact", "preflop_class_table",
           "get_range_equity_exact_weighted", "get_preflop_range_equity_exact_weighted", "get_range_equities",
           "MATRIX_QUERY_DTYPE", "pack_matrix_query", "get_equity_matrix", "matrix_equity", "HAND_ROW_DTYPE",
           "get_range_hand_equities"]
