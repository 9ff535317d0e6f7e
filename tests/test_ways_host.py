"""Split-pot tallies, host side: the lane code with the switch on (tests/hostsim_ways) against the oracle's
per-iteration trace (tests/ways_expect.py), integer for integer.  No GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hostsim_ways as H
from tests import ways_expect as W


@pytest.mark.parametrize("mode", W.MODES)
def test_lane_code_equals_the_trace_on_the_cases_that_make_k_vary(mode):
    exp = [W.expected_case(mode, i) for i in range(len(W.CASES))]
    W.assert_cases_vary(exp)
    for i, (hero, board, n) in enumerate(W.CASES):
        q = W.query(hero, board, n, W.RUNS)
        for general in (False, True):    # the bulk kernel's straight forms and the general form of the one-launch kernel
            got = H.run(mode, q, W.SEED, W.QID, general=general)
            assert np.array_equal(got, exp[i]), (mode, i, general, got, exp[i])
            assert got[13:].sum() == got[3] and not got[13 + n - 1:].any()


@pytest.mark.parametrize("mode", W.MODES)
def test_lane_code_on_random_hands_every_player_count_and_street(mode):
    """1-10 players x {0, 3, 4, 5} table cards: the 13 plain words are oracle.run's tallies, the nine ways the trace's."""
    g = np.random.default_rng(1234 + mode)
    for n in range(1, 11):
        for nb in (0, 3, 4, 5):
            cards = [int(c) for c in g.permutation(52)[:2 + nb]]
            runs, seed, qid = 300, int(g.integers(1, 2 ** 31)), int(g.integers(0, 1000))
            exp = W.expected_row(mode, cards[:2], cards[2:], n, runs, seed, qid)
            plain = O.run(mode, cards[:2], cards[2:], n, runs, (seed + qid) & 0xFFFFFFFF if mode == O.MODE_MT else seed,
                          0 if mode == O.MODE_MT else qid)["tallies"]
            for general in (False, True):
                got = H.run(mode, W.query(cards[:2], cards[2:], n, runs), seed, qid, general=general)
                assert np.array_equal(got[:13], plain), (mode, n, nb, general)
                assert np.array_equal(got, exp), (mode, n, nb, general, got, exp)


@pytest.mark.parametrize("mode", W.MODES)
def test_vectorised_recount_equals_the_pairwise_one(mode):
    """ways_expect.expected_row_fast (packed scores compared in numpy: what the long-query GPU tests expect rows from)
    against expected_row (oracle.compare per pair of hands), word for word, on the cases in which k varies -- and on the
    two further boards the long-query tests take from tests/hot_boards.py, where the reference's quads rule and the wheel
    decide what compares equal."""
    from tests import hot_boards as HB
    for i, (hero, board, n) in enumerate(W.CASES):
        fast = W.expected_row_fast(mode, hero, board, n, W.RUNS, W.SEED, W.QID, threads=4)
        assert np.array_equal(fast, W.expected_case(mode, i)), (mode, i, fast, W.expected_case(mode, i))
    for s in (8, 16):
        hero, board = HB.SITUATIONS[s]
        fast = W.expected_row_fast(mode, hero, board, 6, 1000, W.SEED, W.QID + s, threads=4)
        assert np.array_equal(fast, W.expected_row(mode, hero, board, 6, 1000, W.SEED, W.QID + s)), (mode, s)


def test_sanity_against_arithmetic():
    """Heads-up every tie is two-way; alone at the table hero wins every iteration."""
    for mode in W.MODES:
        hu = H.run(mode, W.query(["AH", "KH"], ["AD", "KD", "QS", "JS", "TS"], 2, 2000), 5, 1)
        assert hu[3] > 0 and hu[13] == hu[3] and not hu[14:].any()     # the straight on the board plays for both
        alone = H.run(mode, W.query(["7C", "2D"], [], 1, 777), 5, 1)
        assert alone[0] == 777 and alone[2] == 777 and alone[3] == 0 and not alone[13:].any()


def test_pot_share_is_the_formula():
    import neuron_poker_amd as npa
    rows = np.zeros(2, npa.RESULT_WAYS_DTYPE)
    rows["runs"] = [1000, 0]
    rows["win"] = [100, 0]
    rows["tie"] = [60, 0]
    rows["tie_ways"][0] = [30, 0, 0, 0, 20, 0, 0, 0, 10]
    assert np.allclose(npa.pot_share(rows), [(100 + 30 / 2 + 20 / 6 + 10 / 10) / 1000, 0.0], rtol=0, atol=1e-15)
    assert np.array_equal(npa.pot_share(rows), npa.pot_share(rows.view(np.uint64).reshape(2, 22)))
