"""mcq_exact_batch_ext_runouts on the GPU: the kernels' rows against the host build of the same lane code (pinned to the
literal walk in tests/test_runouts_host.py), their sums against the existing split-pot enumeration, under the uniform law
every row against the record with the cards appended to the table, and the conventions of an entry (determinism, batch
invariance, refusals, MCQ_EBUSY, the Python surface)."""
import threading
import time

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import hostsim_runouts as HS
from tests import runout_literal as RL

pytestmark = pytest.mark.gpu
SENTINEL = 0xABABABABABABABAB
LAWS = ["reference", "uniform"]
# the mixed batch, twice over: both kinds, both streets, ranges, ghost cards, known hands
BATCH = RL.GPU_CASES * 2
_host = {}


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w22(rows):
    a = np.ascontiguousarray(rows)
    return a.view(np.uint64).reshape(a.shape[0], -1, 22)


def host_rows(name, law):
    """The host build's (cards, pairs) of a case, computed once and left unchanged."""
    key = (name, law)
    if key not in _host:
        c, p = HS.runouts(*RL.records(RL.CASES[name]), law)
        c.setflags(write=False)
        p.setflags(write=False)
        _host[key] = (c, p)
    return _host[key]


def k_of(name):
    return 5 - len(RL.CASES[name][1])


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("law", LAWS)
def test_mixed_batch_against_the_host_build_and_the_ways_entry(monkeypatch, law, cap):
    """cap = 1: the plans see one CU (MCQ_EXACT_CU), so the stride loops run their later rounds: the 16 waves of the one
    block own up to 68 completions each of a record with a random opponent, and 57 lanes own two of flop_alone's 1081;
    cap = None: the device's own grid."""
    if cap is None:
        monkeypatch.delenv("MCQ_EXACT_CU", raising=False)
    else:
        monkeypatch.setenv("MCQ_EXACT_CU", str(cap))
    e = npa.Engine(0)
    try:
        q, x = RL.batch(BATCH)
        cards, pairs = e.exact_ext_runouts(q, x, law)
        _, ways = e.exact_ext_ways(q, x, law)
    finally:
        e.close()
    cards, pairs, ways = w22(cards), w22(pairs), np.ascontiguousarray(ways).view(np.uint64).reshape(-1, 22)
    for i, name in enumerate(BATCH):
        hc, hp = host_rows(name, LAWS.index(law))
        assert np.array_equal(cards[i], hc), (name, law, cap)
        assert np.array_equal(pairs[i], hp), (name, law, cap)
        one = cards[i] if k_of(name) == 1 else pairs[i]
        assert np.array_equal(one.sum(axis=0), ways[i]), (name, law, cap)
        assert int(ways[i][0]) > 0


def test_uniform_law_rows_are_the_records_with_the_cards_appended(eng):
    """Case (e), 47 cards left: every pair row is the weights row of the river record with both cards on the table -- ONE
    exact_ext_ways call over all 1081 records -- and every card row the row of the turn record, 47 records in one call."""
    case = RL.CASES["flop_any"]
    hero, table, n_players, _, _, _ = RL.parts(case)
    deck = RL.deck(case)
    q, x = RL.records(case)
    cards, pairs = eng.exact_ext_runouts(q, x, "uniform")
    cards, pairs = w22(cards)[0], w22(pairs)[0]
    hands = [(a, b) for b in deck for a in deck if a < b]
    assert len(hands) == 1081
    rq = np.concatenate([_lib.pack_query_one(hero, table + [a, b], n_players, 1) for a, b in hands])
    _, river = eng.exact_ext_ways(rq, _lib.pack_query_ext(len(hands)), "uniform")
    river = np.ascontiguousarray(river).view(np.uint64).reshape(-1, 22)
    assert np.array_equal(np.stack([pairs[_lib.hand_index(a, b)] for a, b in hands]), river)
    live = np.zeros(1326, bool)
    live[[_lib.hand_index(a, b) for a, b in hands]] = True
    assert not pairs[~live].any()
    tq = np.concatenate([_lib.pack_query_one(hero, table + [c], n_players, 1) for c in deck])
    _, turn = eng.exact_ext_ways(tq, _lib.pack_query_ext(len(deck)), "uniform")
    turn = np.ascontiguousarray(turn).view(np.uint64).reshape(-1, 22)
    assert len(deck) == 47 and np.array_equal(cards[deck], turn)
    assert not cards[[c for c in range(52) if c not in deck]].any()


def test_two_calls_give_identical_bytes(eng):
    q, x = RL.batch(RL.GPU_CASES)
    for law in LAWS:
        a, b = eng.exact_ext_runouts(q, x, law), eng.exact_ext_runouts(q, x, law)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert w22(a[0])[:, :, 0].any(axis=1).all()


def test_a_batch_of_three_equals_three_single_calls(eng):
    names = ["turn_known_ghost", "flop_allin", "flop_3cls"]
    q, x = RL.batch(names)
    for law in LAWS:
        cards, pairs = eng.exact_ext_runouts(q, x, law)
        for i in range(3):
            c1, p1 = eng.exact_ext_runouts(q[i:i + 1], x[i:i + 1], law)
            assert cards[i].tobytes() == c1[0].tobytes() and pairs[i].tobytes() == p1[0].tobytes(), (names[i], law)


def test_null_pairs_gives_the_same_cards(eng):
    q, x = RL.batch(RL.GPU_CASES)
    for law in LAWS:
        cards, _ = eng.exact_ext_runouts(q, x, law)
        only, none = eng.exact_ext_runouts(q, x, law, want_pairs=False)
        assert none is None and only.tobytes() == cards.tobytes()


def test_refusals_leave_the_outputs_untouched(eng):
    case = RL.CASES["turn_known_ghost"]
    hero, table, n_players, known, ghost, opp = RL.parts(case)
    good = RL.records(case)

    def one(board, players=n_players):
        return _lib.pack_query_one(hero, board, players, 1)
    xh = _lib.pack_query_ext(1, ghost=ghost, known=known, opp_range=opp, hero_range=_lib.range_bits(["AA"]))
    xk = _lib.pack_query_ext(1, ghost=ghost, known=[_lib.range_bits(["AA", "KK"])], opp_range=opp)
    qd = good[0].copy()
    qd["board"][0, 1] = qd["board"][0, 0]
    undealable = (_lib.pack_query_one([RL.C("AD"), RL.C("AC")], [RL.C("AH"), RL.C("7H"), RL.C("2S")], 2, 1),
                  _lib.pack_query_ext(1, opp_range=_lib.range_bits(["AA"])))
    refused = [(good[0], xh, 0, "hero range"), (good[0], xk, 0, "known hand given as a range"),
               (one(table, n_players + 1), good[1], 0, "two random opponents"), undealable + (0, "cannot be dealt"),
               undealable + (1, "cannot be dealt"), good + (2, "bad law"), (qd, good[1], 0, "invalid"),
               (one([]), good[1], 0, "C(50, 5)"), (one(table + [RL.C("2D")]), good[1], 0, "no card to come")]
    L = eng._lib
    entry = L.mcq_exact_batch_ext_runouts
    for q, x, law, why in refused:
        cards = np.full((52, 22), SENTINEL, np.uint64)
        pairs = np.full((1326, 22), SENTINEL, np.uint64)
        rc = entry(eng._ctx, q.ctypes.data, x.ctypes.data, 1, law, cards.ctypes.data, pairs.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and (cards == SENTINEL).all() and (pairs == SENTINEL).all(), why
        assert why.encode() in L.mcq_last_error(), (why, L.mcq_last_error())
        # ... and as the second record of a batch: nothing is written for the record before it either
        if why == "bad law":
            continue
        cards = np.full((2, 52, 22), SENTINEL, np.uint64)
        pairs = np.full((2, 1326, 22), SENTINEL, np.uint64)
        q2, x2 = np.concatenate([good[0], q]), np.concatenate([good[1], x])
        rc = entry(eng._ctx, q2.ctypes.data, x2.ctypes.data, 2, law, cards.ctypes.data, pairs.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and (cards == SENTINEL).all() and (pairs == SENTINEL).all(), why
        assert b"query 1" in L.mcq_last_error() and why.encode() in L.mcq_last_error(), (why, L.mcq_last_error())
    # more records than MCQ_RUNOUT_MAX_BATCH: refused before a row is looked at
    n = _lib.RUNOUT_MAX_BATCH + 1
    qn, xn = np.repeat(good[0], n), np.repeat(good[1], n)
    cards = np.full((52, 22), SENTINEL, np.uint64)
    assert entry(eng._ctx, qn.ctypes.data, xn.ctypes.data, n, 0, cards.ctypes.data, None) == _lib.MCQ_EINVAL
    assert b"MCQ_RUNOUT_MAX_BATCH" in L.mcq_last_error() and (cards == SENTINEL).all()
    with pytest.raises(ValueError):
        eng.exact_ext_runouts(*good, law="production")
    # the same context goes on
    cards, pairs = eng.exact_ext_runouts(*good)
    hc, hp = host_rows("turn_known_ghost", 0)
    assert np.array_equal(w22(cards)[0], hc) and np.array_equal(w22(pairs)[0], hp) and hc[:, 0].any()


def test_second_call_on_a_busy_context_is_turned_away(eng):
    """One call in flight per context: while a batch of full flops is enumerated, a second caller gets MCQ_EBUSY and the
    long call is not disturbed."""
    big = RL.batch(["flop_any"] * 384)
    small = RL.records(RL.CASES["turn_3cls"])
    want_small = eng.exact_ext_runouts(*small)[0].tobytes()
    want_big = eng.exact_ext_runouts(*big)[1].tobytes()
    started, results, busy = threading.Event(), [], [0]

    def long_call():
        started.set()
        while not results:
            try:
                results.append(eng.exact_ext_runouts(*big)[1].tobytes())
            except npa.McqBusyError as e:      # the short call was in flight: turned away likewise, try again
                assert "context busy" in str(e)
                busy[0] += 1
    th = threading.Thread(target=long_call)
    th.start()
    started.wait()
    deadline = time.time() + 5
    while th.is_alive() and time.time() < deadline:
        try:
            assert eng.exact_ext_runouts(*small)[0].tobytes() == want_small   # got in between two calls: fine
        except npa.McqBusyError as e:
            assert "context busy" in str(e)
            busy[0] += 1
    th.join()
    assert busy[0] > 0
    assert results[0] == want_big
    assert eng.exact_ext_runouts(*small)[0].tobytes() == want_small


@pytest.mark.parametrize("ties", ["credited", "split"])
@pytest.mark.parametrize("name", ["turn_known_ghost", "flop_3cls", "flop_allin"])
def test_get_runout_equities(eng, name, ties):
    hero, table, n_players, known, ghost, opp = RL.CASES[name]
    k = k_of(name)
    args = dict(known_hands=known, ghost_cards=ghost, opponent_range=opp, ties=ties)
    for law in LAWS:
        eq, by_card, by_pair = mh.get_runout_equities(hero, table, n_players, law, eng, pairs=True, **args)
        two = mh.get_runout_equities(hero, table, n_players, law, eng, **args)
        assert two == (eq, by_card)
        want, _ = mh.get_equity_exact(hero, table, n_players, law, eng, known_hands=known, ghost_cards=ghost or '',
                                      opponent_range=1 if opp is None else opp, ties=ties)
        assert abs(eq - want) <= 1e-12, (name, law, ties, eq, want)
        cards, pairs = eng.exact_ext_runouts(*RL.records(RL.CASES[name]), law)
        cards, pairs = w22(cards)[0], w22(pairs)[0]
        total = int((cards if k == 1 else pairs)[:, 0].sum())

        def value(r):
            r = [int(v) for v in r]
            share = r[2] + (sum(r[13 + j] / (j + 2.0) for j in range(9)) if ties == "split" else r[3])
            return share / r[0]
        assert sorted(by_card) == sorted(npa.card_str(c) for c in range(52) if cards[c, 0])
        for c in range(52):
            if cards[c, 0]:
                e, p = by_card[npa.card_str(c)]
                assert e == pytest.approx(value(cards[c]), abs=1e-12) and p == pytest.approx(int(cards[c, 0]) / (k * total), abs=1e-15)
        assert abs(sum(p for _, p in by_card.values()) - 1.0) <= 1e-12
        assert abs(sum(e * p for e, p in by_card.values()) - eq) <= 1e-12       # the law of total expectation
        assert len(by_pair) == int((pairs[:, 0] != 0).sum()) and (len(by_pair) > 0) == (k == 2)
        for (a, b), (e, p) in by_pair.items():
            r = pairs[_lib.hand_index(npa.card_id(a), npa.card_id(b))]
            assert npa.card_id(a) < npa.card_id(b)
            assert e == pytest.approx(value(r), abs=1e-12) and p == pytest.approx(int(r[0]) / total, abs=1e-15)
        if k == 2:
            assert abs(sum(p for _, p in by_pair.values()) - 1.0) <= 1e-12
    with pytest.raises(ValueError):
        mh.get_runout_equities(hero, [], n_players, engine=eng, **args)                     # preflop
    with pytest.raises(ValueError):
        mh.get_runout_equities(hero, (table + ["2D", "3S"])[:5], n_players, engine=eng, **args)   # the river
    with pytest.raises(ValueError):
        mh.get_runout_equities(hero, table, n_players, engine=eng, **dict(args, ties="half"))
    with pytest.raises(ValueError):
        mh.get_runout_equities(hero, table, len(known) + 3, engine=eng, **args)             # two random opponents
