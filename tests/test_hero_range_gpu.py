"""mcq_exact_batch_hero_range on the GPU: the kernel's rows against the host build of the same lane code and against
the one-record enumeration, the Monte-Carlo kernels' hero ranges against its aggregate, and the conventions of an entry
(determinism, batch invariance, refusals, MCQ_EBUSY)."""
import threading
import time

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import hero_range_cases as HC
from tests import hostsim_hero_range as HS
from tests import lawstats as LS

pytestmark = pytest.mark.gpu
SENTINEL = 0xABABABABABABABAB
LAWS = ["reference", "uniform"]
# streets mixed; flop_all: 1176 completions (more blocks than CUs), 1176 hero hands (two thread groups)
GRID = ["river_all", "flop_3cls", "turn_ghost", "flop_all", "turn_one_class", "river_small"]


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w13(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, HS.ROWS, 13)


def agg11(agg):
    return np.ascontiguousarray(agg).view(np.float64).reshape(-1, 11)


@pytest.mark.parametrize("law", LAWS)
def test_grid_of_records_against_the_host_build_and_the_one_record_entry(eng, law):
    code = LAWS.index(law)
    q, x = HC.batch([HC.CASES[n] for n in GRID])
    rows, agg = eng.exact_hero_range(q, x, law)
    got, got_agg = w13(rows), agg11(agg)
    hq, hx, where = [], [], []
    for i, name in enumerate(GRID):
        want, want_agg = HS.hero_range(*HC.records(HC.CASES[name]), code)
        assert np.array_equal(got[i], want), (name, law)
        assert np.array_equal(got_agg[i], want_agg), (name, law)      # the same host code on the same integers
        hands = HC.allowed_hands(HC.CASES[name])
        assert int((got[i][:, 0] != 0).sum()) == len(hands)
        a, b = HC.hand_records(HC.CASES[name], hands)
        hq.append(a)
        hx.append(b)
        where += [(i, _lib.hand_index(*h)) for h in hands]
    _, one = eng.exact_ext(np.concatenate(hq), np.concatenate(hx), law)   # ONE batched call over every allowed hand
    one = np.ascontiguousarray(one).view(np.uint64).reshape(-1, 13)
    assert len(one) == len(where) > 2000
    mine = np.stack([got[i][r] for i, r in where])
    assert np.array_equal(mine, one)


def test_unrestricted_opponent_range_gives_the_plain_rows(eng):
    """A turn whose opp_range has all 169 bits set: per hand, Engine.exact's row."""
    case = HC.CASES["turn_vs_any"]
    q, x = HC.records(case)
    assert (x["opp_range"][0] == _lib.ALL_CLASSES).all()
    hands = HC.allowed_hands(case)
    plain = npa.pack_queries(hands, [HC.parts(case)[2] + [255]] * len(hands), 2, 1)
    for law in LAWS:
        got = w13(eng.exact_hero_range(q, x, law)[0])[0]
        want = np.ascontiguousarray(eng.exact(plain, law)).view(np.uint64).reshape(-1, 13)
        assert np.array_equal(np.stack([got[_lib.hand_index(*h)] for h in hands]), want), law


@pytest.mark.parametrize("name", ["flop_top25", "turn_vs_any"])
def test_monte_carlo_hero_range_converges_to_the_reference_law_aggregate(eng, name):
    """10^8 production iterations of mcq_eval_batch_ext with hero_is_range = 1 against agg under the reference's law
    (eleven statistics, 5.5 sigma: tests/lawstats.py); the uniform law's aggregate lies outside that bound."""
    q, x = HC.records(HC.CASES[name])
    ref = agg11(eng.exact_hero_range(q, x, "reference")[1])[0]
    uni = agg11(eng.exact_hero_range(q, x, "uniform")[1])[0]
    q["runs"] = 100000000
    mc = eng.eval_batch_ext(q, x, seed=20240 + len(name))
    assert int(mc["runs"][0]) == 100000000
    LS.check("%s, reference law" % name, LS.one_sample(mc, ref))
    off = LS.one_sample(mc, uni)
    print(LS.report("%s, uniform law" % name, off))
    assert LS.max_z(off) > LS.BOUND


def test_two_calls_give_identical_rows(eng):
    q, x = HC.batch([HC.CASES[n] for n in ("flop_top25", "river_all", "turn_ghost")])
    a, b = eng.exact_hero_range(q, x), eng.exact_hero_range(q, x)
    assert np.array_equal(w13(a[0]), w13(b[0])) and np.array_equal(agg11(a[1]), agg11(b[1]))
    assert w13(a[0])[:, :, 0].any(axis=1).all()


def test_a_batch_of_three_equals_three_single_calls(eng):
    names = ["turn_ghost", "flop_3cls", "river_small"]
    q, x = HC.batch([HC.CASES[n] for n in names])
    for law in LAWS:
        rows, agg = eng.exact_hero_range(q, x, law)
        for i in range(3):
            r1, a1 = eng.exact_hero_range(q[i:i + 1], x[i:i + 1], law)
            assert np.array_equal(w13(rows)[i], w13(r1)[0]) and np.array_equal(agg11(agg)[i], agg11(a1)[0]), (names[i], law)


def test_refusals_leave_the_outputs_untouched(eng):
    case = HC.CASES["turn_ghost"]
    good = HC.records(case)
    qh, xh = HC.records(case, hero_is_range=False)
    qh["hole"][0] = [HC.C("3C"), HC.C("3D")]
    q3, xk = good[0].copy(), good[1].copy()
    q3["n_players"] = 3
    xk["n_known"] = 1
    xk["known"]["cards"][0, 0] = [HC.C("3C"), HC.C("3D")]
    qd = good[0].copy()
    qd["board"][0, 1] = qd["board"][0, 0]
    xe = good[1].copy()
    xe["opp_range"] = 0
    refused = [(qh, xh, 0, "hero_is_range"), (q3, xk, 0, "n_known"), (HC.records(case, n_players=3) + (0, "n_players")),
               (_lib.pack_query_one([0, 0], [], 2, 1), good[1], 0, "C(50, 5)"), good + (2, "bad law"), (qd, good[1], 0, "invalid"),
               (good[0], xe, 0, "invalid"), HC.records(({"77"}, None, ["7C", "7D", "7H", "2S"], None)) + (0, "no hand"),
               HC.records(HC.UNDEALABLE) + (0, "cannot be dealt"), HC.records(HC.UNDEALABLE) + (1, "cannot be dealt")]
    L = eng._lib
    for q, x, law, why in refused:
        rows = np.full((HS.ROWS, 13), SENTINEL, np.uint64)
        agg = np.full(11, -3.0)
        rc = L.mcq_exact_batch_hero_range(eng._ctx, q.ctypes.data, x.ctypes.data, 1, law, rows.ctypes.data, agg.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and (rows == SENTINEL).all() and (agg == -3.0).all(), why
        assert why.encode() in L.mcq_last_error(), (why, L.mcq_last_error())
    # a refusal inside a batch: nothing is written for the records before it either
    rows = np.full((2, HS.ROWS, 13), SENTINEL, np.uint64)
    q, x = np.concatenate([good[0], HC.records(HC.UNDEALABLE)[0]]), np.concatenate([good[1], HC.records(HC.UNDEALABLE)[1]])
    rc = L.mcq_exact_batch_hero_range(eng._ctx, q.ctypes.data, x.ctypes.data, 2, 0, rows.ctypes.data, None)
    assert rc == _lib.MCQ_EINVAL and (rows == SENTINEL).all()
    with pytest.raises(ValueError):
        eng.exact_hero_range(*good, law="production")
    # the existing entries keep their refusal of a hero range
    with pytest.raises(ValueError):
        eng.exact_ext(*good)
    with pytest.raises(ValueError):
        mh.MonteCarlo(eng).run_montecarlo([{"AKS", "QQ"}], ["2D", "9H", "JS"], 2, None, 1000, 0, '', mode="exact")
    rows, agg = eng.exact_hero_range(good[0], good[1], "reference", )     # the same context goes on; agg may be NULL
    out = np.zeros((HS.ROWS, 13), np.uint64)
    assert L.mcq_exact_batch_hero_range(eng._ctx, good[0].ctypes.data, good[1].ctypes.data, 1, 0, out.ctypes.data, None) == 0
    assert np.array_equal(out, w13(rows)[0]) and out[:, 0].any()


def test_second_call_on_a_busy_context_is_turned_away(eng):
    """One call in flight per context: while a batch of full flops is enumerated, a second caller gets MCQ_EBUSY and the
    long call is not disturbed."""
    big = HC.batch([HC.CASES["flop_all"]] * 6)
    small = HC.records(HC.CASES["turn_one_class"])
    want_small = w13(eng.exact_hero_range(*small)[0])
    want_big = w13(eng.exact_hero_range(*big)[0])
    started, results, busy = threading.Event(), [], [0]

    def long_call():
        started.set()
        while not results:
            try:
                results.append(w13(eng.exact_hero_range(*big)[0]))
            except npa.McqBusyError as e:      # the short call was in flight: turned away likewise, try again
                assert "context busy" in str(e)
                busy[0] += 1
    th = threading.Thread(target=long_call)
    th.start()
    started.wait()
    deadline = time.time() + 5
    while th.is_alive() and time.time() < deadline:
        try:
            assert np.array_equal(w13(eng.exact_hero_range(*small)[0]), want_small)   # got in between two calls: fine
        except npa.McqBusyError as e:
            assert "context busy" in str(e)
            busy[0] += 1
    th.join()
    assert busy[0] > 0
    assert np.array_equal(results[0], want_big)
    assert np.array_equal(w13(eng.exact_hero_range(*small)[0]), want_small)


@pytest.mark.parametrize("ties", ["credited", "split"])
def test_get_range_equity_exact(eng, ties):
    hero, opp, table, ghost = HC.CASES["turn_ghost"]
    for law in LAWS:
        eq, hands = mh.get_range_equity_exact(hero, table, opponent_range=opp, dealing=law, ghost_cards=ghost, engine=eng, ties=ties)
        rows = w13(eng.exact_hero_range(*HC.records(HC.CASES["turn_ghost"]), law)[0])[0]
        allowed = HC.allowed_hands(HC.CASES["turn_ghost"])
        assert sorted(hands) == sorted((npa.card_str(a), npa.card_str(b)) for a, b in allowed)
        num = den = 0.0
        for a, b in allowed:
            r = [int(v) for v in rows[_lib.hand_index(a, b)]]
            e, w = hands[(npa.card_str(a), npa.card_str(b))]
            want = (r[2] + (r[3] / 2.0 if ties == "split" else r[3])) / r[0]
            assert e == pytest.approx(want, abs=1e-15)
            assert w == (1 if law == "uniform" or 50 in (a, b) else 2)       # AS is on the table: AH is the deck's top
            num += w * want
            den += w
        assert eq == pytest.approx(num / den, abs=1e-12)
        if ties == "credited":
            agg = eng.exact_hero_range(*HC.records(HC.CASES["turn_ghost"]), law)[1][0]
            assert eq == pytest.approx(float(agg["win"] + agg["tie"]), abs=1e-12)
    with pytest.raises(ValueError):
        mh.get_range_equity_exact({"AKS"}, [], engine=eng)                        # preflop
    with pytest.raises(ValueError):
        mh.get_range_equity_exact({"AKS"}, table, engine=eng, ties="half")
