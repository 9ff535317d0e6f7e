"""Expected split-pot rows (mcq_result_ways) from the oracle's per-iteration trace -- shared by the ways tests.

oracle.run(..., keep=runs) returns every iteration's seven-card hands.  Hero (hand 0) is best iff no opponent compares
greater (oracle.compare, the reference's own comparison, quirks included); the pot is then shared by k = 1 + #equal
hands.  ways[1] must be the oracle's win and sum(ways[2:]) its tie: the helper checks that on every case."""
import numpy as np

from oracle import oracle as O

# (hero, board, n_players): cases in which the number of hands sharing the pot varies (k = 2, 3, 4, 6, 9, 10 occur)
CASES = [
    (["AH", "KH"], [], 6),
    (["7C", "2D"], [], 10),
    (["2C", "3D"], ["TS", "JS", "QS", "KS", "AS"], 6),
    (["2C", "3D"], ["KC", "KD", "KH", "KS"], 6),
    (["2C", "2D"], ["5C", "6D", "7H", "8S"], 6),
    (["AC", "QD"], ["AD", "AH", "KS"], 4),
    (["2C", "7D"], ["TS", "JD", "QH"], 9),
]
RUNS, SEED, QID = 4096, 7, 3
MODES = [O.MODE_MT, O.MODE_CTR, O.MODE_CTR_UNIFORM]


def query(hero, board, n_players, runs):
    b = [O.card_id(c) if isinstance(c, str) else int(c) for c in board]
    h = [O.card_id(c) if isinstance(c, str) else int(c) for c in hero]
    return O.pack_queries([h], [b + [255] * (5 - len(b))], n_players, runs)[0]


def expected_row(mode, hero, board, n_players, runs, seed, qid):
    """-> the 22 words of the query's mcq_result_ways row, from the oracle's tallies and its trace."""
    if mode == O.MODE_MT:   # the library's parity mode seeds query `qid` with (seed + qid) mod 2^32; oracle.run takes that seed
        seed, qid = (seed + qid) & 0xFFFFFFFF, 0
    r = O.run(mode, hero, board, n_players, runs, seed, qid, keep=runs)
    ways = np.zeros(11, np.uint64)          # ways[k]: iterations in which hero is best and k hands share the pot
    for hands in r["trace"]:
        cmp = [O.compare(hands[p], hands[0]) for p in range(1, n_players)]   # > 0: the opponent's hand is greater
        if not any(c > 0 for c in cmp):
            ways[1 + sum(1 for c in cmp if c == 0)] += 1
    assert int(ways[1]) == r["win"] and int(ways[2:].sum()) == r["tie"], (ways, r["win"], r["tie"])
    assert not ways[n_players + 1:].any()
    return np.concatenate([r["tallies"], ways[2:]]).astype(np.uint64)


def expected_row_fast(mode, hero, board, n_players, runs, seed, qid, threads=1):
    """expected_row for long queries: the same trace, scored in one oracle.score_batch call (calc_score of every hand as an
    order-preserving integer) and compared in numpy instead of one oracle.compare per pair of hands.
    tests/test_ways_host.py holds it equal to expected_row, word for word."""
    if mode == O.MODE_MT:
        seed, qid = (seed + qid) & 0xFFFFFFFF, 0
    r = O.run(mode, hero, board, n_players, runs, seed, qid, keep=runs)
    score = O.score_batch(r["trace"].reshape(-1, 7), threads).reshape(runs, n_players)
    mine, theirs = score[:, :1], score[:, 1:]
    best = ~(theirs > mine).any(axis=1)                    # no opponent's hand is greater
    k = 1 + (theirs == mine).sum(axis=1)                   # hands that share the pot
    ways = np.bincount(k[best], minlength=11).astype(np.uint64)
    assert int(ways[1]) == r["win"] and int(ways[2:].sum()) == r["tie"], (ways, r["win"], r["tie"])
    assert not ways[n_players + 1:].any()
    return np.concatenate([r["tallies"], ways[2:]]).astype(np.uint64)


_cache = {}


def expected_case(mode, i, runs=RUNS, seed=SEED, qid=QID):
    key = (mode, i, runs, seed, qid)
    if key not in _cache:
        hero, board, n = CASES[i]
        _cache[key] = expected_row(mode, hero, board, n, runs, seed, qid)
    return _cache[key]


def assert_cases_vary(rows):
    """The cases must exercise what they claim: at least three different k >= 3 occur, and some tie is not two-way."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 22)
    assert int((rows[:, 14:22].sum(0) != 0).sum()) >= 3, rows[:, 13:22]
    assert (rows[:, 13] != rows[:, 3]).any()
