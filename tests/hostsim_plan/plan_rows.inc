// plan_rows.inc -- TEST FIXTURE: (results | inputs) rows of the launch plans (neuron_poker_amd/csrc/mcq_plan.hpp), taken from
// the host layer as it stood before the plans moved into the header.  tests/test_plan_host.py reads them as text,
// hs_main.cpp as macro calls; hs_rows.hpp says what the columns are and recomputes the results.
/* grid, block, split, work_wpb | n_cu, occ, grid_cap, split_max, load_waves, bulk, total_tasks, max_tasks */
PLAN_GEOMETRY(512, 1024, 0, 0, 256, 2, 0, 4, 16, 1, 0, 0) /* task count unknown: every resident block */
PLAN_GEOMETRY(100, 1024, 0, 0, 256, 2, 100, 4, 16, 1, 0, 0) /* ... under a grid cap */
PLAN_GEOMETRY(252, 1024, 0, 4, 256, 1, 0, 4, 16, 1, 1008, 0) /* four working waves of sixteen */
PLAN_GEOMETRY(225, 1024, 0, 5, 256, 1, 0, 4, 16, 1, 1124, 0) /* five */
PLAN_GEOMETRY(252, 1024, 0, 8, 256, 1, 0, 4, 16, 1, 2016, 0) /* eight */
PLAN_GEOMETRY(196, 1024, 2, 2, 256, 2, 0, 4, 16, 1, 98, 98) /* one 100k query: cut in four, 392 tasks */
PLAN_GEOMETRY(512, 1024, 0, 0, 256, 2, 0, 4, 16, 1, 401408, 98) /* the bulk: two blocks per CU, all waves work */
PLAN_GEOMETRY(252, 256, 0, 0, 256, 2, 0, 4, 4, 1, 1008, 0) /* MCQ_LOAD_WAVES=4: nobody idles */
PLAN_GEOMETRY(150, 384, 0, 2, 256, 2, 0, 4, 6, 1, 300, 300) /* six loading waves, two working */
PLAN_GEOMETRY(7, 1024, 0, 0, 256, 2, 7, 4, 16, 1, 5000, 10) /* MCQ_GRID_CAP=7 */
PLAN_GEOMETRY(98, 1024, 0, 1, 256, 2, 0, 0, 16, 1, 98, 98) /* MCQ_SPLIT_MAX=0 */
PLAN_GEOMETRY(40, 256, 2, 0, 64, 2, 0, 2, 1, 1, 10, 3) /* cut by the longest query, at least four waves */
PLAN_GEOMETRY(252, 256, 0, 0, 256, 2, 0, 4, 16, 0, 1008, 0) /* extended and ranges kernels: no cut, no idle waves */
PLAN_GEOMETRY(1, 256, 0, 0, 256, 2, 0, 4, 16, 0, 1, 0) /* ... one task */
PLAN_GEOMETRY(304, 1024, 0, 0, 304, 1, 0, 4, 16, 0, 100000, 0) /* ... sixteen waves, one block per CU */
PLAN_GEOMETRY(608, 1024, 0, 0, 304, 2, 0, 4, 16, 0, 100000, 0) /* ... two */
PLAN_GEOMETRY(5, 1024, 0, 0, 8, 2, 5, 4, 16, 0, 1000, 0) /* ... capped */
/* lg, grid, rounds | n, n_cu, split_max */
PLAN_SMALL_CUT(3, 1, 1, 1, 256, 4)
PLAN_SMALL_CUT(3, 64, 1, 128, 256, 4)
PLAN_SMALL_CUT(3, 256, 1, 512, 256, 4)
PLAN_SMALL_CUT(2, 129, 1, 513, 256, 4)
PLAN_SMALL_CUT(2, 256, 1, 1024, 256, 4)
PLAN_SMALL_CUT(1, 129, 1, 1025, 256, 4)
PLAN_SMALL_CUT(1, 256, 1, 2048, 256, 4)
PLAN_SMALL_CUT(0, 129, 1, 2049, 256, 4)
PLAN_SMALL_CUT(0, 256, 1, 4096, 256, 4)
PLAN_SMALL_CUT(0, 256, 2, 4097, 256, 4)
PLAN_SMALL_CUT(0, 256, 25, 100000, 256, 4)
PLAN_SMALL_CUT(1, 64, 1, 512, 256, 1)
PLAN_SMALL_CUT(0, 32, 1, 512, 256, 0)
PLAN_SMALL_CUT(0, 304, 3450, 16777215, 304, 4)
PLAN_SMALL_CUT(3, 5, 1, 9, 8, 4)
/* n_boards, slices, grid | n_board, n_players, n_cu */
PLAN_EXACT(2118760, 1, 256, 0, 2, 256)
PLAN_EXACT(1, 64, 11, 5, 3, 256)
PLAN_EXACT(46, 64, 256, 4, 3, 256)
PLAN_EXACT(1081, 8, 256, 3, 3, 256)
PLAN_EXACT(2118760, 1, 256, 0, 3, 256)
PLAN_EXACT(1, 1, 1, 5, 1, 256)
PLAN_EXACT(46, 1, 3, 4, 2, 8)
PLAN_EXACT(1081, 1, 68, 3, 2, 256)
PLAN_EXACT(1, 64, 8, 5, 3, 8)
PLAN_EXACT(46, 8, 8, 4, 3, 8)
PLAN_EXACT(2118760, 1, 304, 0, 1, 304)
PLAN_EXACT(1081, 1, 1, 3, 3, 1)
/* returned, n_boards, grid, groups | which (0: mcq_exact_ext_plan, x = kind; 1, 2: mcq_exact_hero_plan post- and preflop, x = n_allowed), n_board, x, L, n_cu, slice */
PLAN_EXACT_EXT(1, 1, 1, 1, 0, 5, 0, 45, 256, 0)
PLAN_EXACT_EXT(2, 1081, 2, 1, 0, 3, 0, 47, 256, 0)
PLAN_EXACT_EXT(256, 1712304, 256, 1, 0, 0, 0, 48, 256, 0)
PLAN_EXACT_EXT(1, 1, 1, 1, 0, 5, 1, 43, 256, 0)
PLAN_EXACT_EXT(3, 46, 3, 1, 0, 4, 1, 46, 8, 0)
PLAN_EXACT_EXT(68, 1081, 68, 1, 0, 3, 1, 47, 256, 0)
PLAN_EXACT_EXT(1, 1, 1, 1, 0, 5, 2, 45, 256, 0)
PLAN_EXACT_EXT(92, 46, 92, 2, 0, 4, 2, 46, 256, 0)
PLAN_EXACT_EXT(8, 1081, 8, 2, 0, 3, 2, 47, 8, 0)
PLAN_EXACT_EXT(2, 1225, 2, 2, 0, 3, 2, 50, 1, 0)
PLAN_EXACT_EXT(44, 44, 44, 1, 0, 4, 2, 44, 304, 0)
PLAN_EXACT_EXT(256, 2118760, 256, 1, 0, 0, 1, 50, 256, 0)
PLAN_EXACT_EXT(256, 1081, 256, 2, 1, 3, 1326, 47, 256, 0)
PLAN_EXACT_EXT(1, 1, 1, 1, 1, 5, 1, 45, 256, 0)
PLAN_EXACT_EXT(8, 46, 8, 2, 1, 4, 1025, 46, 8, 0)
PLAN_EXACT_EXT(2, 1, 2, 2, 1, 3, 1025, 2, 8, 0)
PLAN_EXACT_EXT(2, 1, 2, 2, 1, 3, 1025, 2, 1, 0)
PLAN_EXACT_EXT(6, 6, 6, 1, 1, 0, 1, 6, 8, 0)
PLAN_EXACT_EXT(256, 2118760, 256, 2, 2, 0, 1326, 50, 256, 65536)
PLAN_EXACT_EXT(8, 126, 8, 1, 2, 0, 1, 9, 8, 1000)
PLAN_EXACT_EXT(8, 6, 8, 2, 2, 0, 1025, 6, 8, 7)
PLAN_EXACT_EXT(2, 6, 2, 2, 2, 0, 1025, 6, 1, 2)
PLAN_EXACT_EXT(12, 6, 12, 2, 2, 0, 1025, 6, 64, 7)
PLAN_EXACT_EXT(1, 6, 1, 1, 2, 0, 1, 6, 8, 1)
PLAN_EXACT_EXT(2, 6, 2, 2, 2, 0, 1025, 6, 1, 1)
PLAN_EXACT_EXT(0, 126, 8, 1, 2, 0, 1, 9, 8, 384000000)
PLAN_EXACT_EXT(0, 6, 2, 2, 2, 0, 1025, 6, 1, 2118760)
PLAN_EXACT_EXT(0, 2118760, 256, 2, 2, 0, 1326, 50, 256, 384000001)
PLAN_EXACT_EXT(0, 6, 0, 1, 2, 0, 1, 6, 8, 0)
PLAN_EXACT_EXT(0, 6, 0, 2, 2, 0, 1025, 6, 1, 0)
/* price, refused, seat, table | n_board, five table cards, n_players, n_tables, the seats' table numbers, then kind, a, b, w per table (hs_rows.hpp) */
PLAN_PRICE(100, 0, 0, 0, 0, 45, 12, 46, 24, 47, 2, 1, 0, 0, 1, 0, 1, 3) /* two seats hold the same hand */
PLAN_PRICE(100, 0, 0, 0, 5, 45, 42, 13, 43, 21, 2, 1, 0, 0, 1, 0, 51, 2) /* two seats hold the same hand */
PLAN_PRICE(1, 0, 0, 0, 0, 11, 1, 49, 46, 12, 3, 1, 0, 0, 0, 0, 0, 0, 1) /* no two seats can collide */
PLAN_PRICE(1, 0, 0, 0, 4, 5, 33, 35, 37, 10, 2, 3, 1, 2, 3, 51, 0, 65535, 0, 0, 0, 65535, 3, 17, 0, 9) /* no two seats can collide */
PLAN_PRICE(256, 0, 0, 0, 0, 7, 43, 32, 26, 11, 3, 2, 0, 0, 0, 1, 5, 4, 9, 3, 51, 0, 65535) /* three seats block each other: the cap */
PLAN_PRICE(256, 0, 0, 0, 3, 12, 26, 42, 3, 16, 3, 1, 0, 0, 0, 1, 0, 1, 3) /* three seats block each other: the cap */
PLAN_PRICE(2, 0, 0, 0, 0, 20, 22, 9, 31, 21, 4, 3, 2, 1, 0, 0, 2, 97, 11, 3, 0, 0, 0, 1, 2, 663, 5, 2) /* in between */
PLAN_PRICE(119, 0, 0, 0, 3, 19, 50, 15, 26, 21, 3, 3, 2, 0, 1, 1, 12, 40, 65535, 1, 12, 40, 65535, 0, 0, 0, 65535) /* in between */
PLAN_PRICE(114, 0, 0, 0, 4, 36, 51, 5, 38, 27, 3, 3, 0, 1, 1, 3, 4, 0, 3, 3, 17, 0, 9, 0, 0, 0, 65535) /* in between */
PLAN_PRICE(184, 0, 0, 0, 5, 19, 25, 34, 36, 37, 4, 3, 0, 2, 2, 0, 3, 51, 0, 65535, 1, 5, 4, 9, 2, 7, 3, 65535) /* in between */
PLAN_PRICE(0, 1, 0, 1, 0, 50, 33, 7, 9, 0, 2, 1, 1, 0, 0, 0, 0, 1) /* refused: a table number out of range */
PLAN_PRICE(0, 1, 1, 3, 4, 29, 38, 2, 30, 34, 3, 2, 1, 3, 0, 2, 13, 0, 1, 1, 0, 51, 2) /* refused: a table number out of range */
PLAN_PRICE(0, 2, 2, 0, 0, 30, 33, 37, 46, 38, 4, 3, 2, 2, 0, 0, 4, 0, 0, 0, 2, 2, 1, 5, 3, 51, 0, 65535) /* refused: nothing clear of the table cards */
PLAN_PRICE(0, 2, 0, 0, 3, 51, 30, 4, 29, 37, 4, 1, 0, 0, 0, 0, 1, 5, 4, 9) /* refused: nothing clear of the table cards */
PLAN_PRICE(0, 2, 0, 0, 4, 50, 51, 4, 20, 18, 3, 3, 0, 1, 0, 3, 4, 0, 3, 3, 17, 0, 9, 1, 5, 4, 9) /* refused: nothing clear of the table cards */
