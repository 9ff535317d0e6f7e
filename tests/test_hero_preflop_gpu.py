"""mcq_exact_batch_hero_range_preflop on the GPU: every allowed hero hand's row against the one-record enumeration
(Engine.exact_ext) bit for bit, both groups of blocks and their boundary, the slicing of the completions into launches, the
Monte-Carlo kernels' hero ranges against its aggregate, and the conventions of an entry (determinism, batch invariance,
refusals, MCQ_EBUSY).  k = 5 and |D| >= 50 cannot shrink: these are the smallest shapes that exist before the flop."""
import math
import threading
import time

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import hero_preflop_cases as PC
from tests import hero_range_cases as HC
from tests import lawstats as LS

pytestmark = pytest.mark.gpu
SENTINEL = 0xABABABABABABABAB
LAWS = ["reference", "uniform"]
ROWS = 1326
# case 1: narrow ranges, the whole enumeration
NARROW = {(opp_name, n_deck): PC.case(PC.NARROW_HERO, opp, n_deck)
          for opp_name, opp in (("3cls", PC.OPP_3CLS), ("top10", PC.TOP10)) for n_deck in (52, 50)}
_narrow = {}


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w13(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, ROWS, 13)


def agg11(agg):
    return np.ascontiguousarray(agg).view(np.float64).reshape(-1, 11)


def narrow_rows(eng, key, law):
    """(rows[1326, 13], agg[11]) of a case-1 record from the module's engine (default slice), computed once, left unchanged."""
    k = key + (law,)
    if k not in _narrow:
        rows, agg = eng.exact_hero_range_preflop(*HC.records(NARROW[key]), law)
        r, a = w13(rows)[0].copy(), agg11(agg)[0].copy()
        r.setflags(write=False)
        a.setflags(write=False)
        _narrow[k] = (r, a)
    return _narrow[k]


def one_record_rows(eng, c, hands, law):
    """Engine.exact_ext's weights rows of the records with the hero holding each hand: ONE batched call."""
    q, x = HC.hand_records(c, hands)
    _, w = eng.exact_ext(q, x, law)
    return np.ascontiguousarray(w).view(np.uint64).reshape(-1, 13)


def recombined(c, rows, hands, law):
    """agg from the rows as the host combines them: ascending row order, w = 2 - [the hand holds D's top card] (reference)."""
    top = max(HC.deck(c))
    num, den = [0.0] * 11, 0.0
    for a, b in hands:
        r = [int(v) for v in rows[_lib.hand_index(a, b)]]
        w = 1.0 if law == "uniform" or top in (a, b) else 2.0
        runs = float(r[0])
        num[0] += w * float(r[2]) / runs
        num[1] += w * float(r[3]) / runs
        for t in range(9):
            num[2 + t] += w * float(r[4 + t]) / runs
        den += w
    return [v / den for v in num]


@pytest.mark.parametrize("law", LAWS)
def test_narrow_ranges_every_allowed_row_is_the_one_record_row(eng, law):
    for key, c in NARROW.items():
        rows, agg = narrow_rows(eng, key, law)
        hands = HC.allowed_hands(c)
        assert len(hands) == (10 if key[1] == 52 else 3)
        one = one_record_rows(eng, c, hands, law)
        live = np.zeros(ROWS, bool)
        for h, want in zip(hands, one):
            i = _lib.hand_index(*h)
            live[i] = True
            assert want[0] > 0 and want[1] == 0
            assert np.array_equal(rows[i], want), (key, law, h, rows[i], want)
        assert (rows[~live] == 0).all(), (key, law)
        want_agg = recombined(c, rows, hands, law)
        assert np.allclose(agg, want_agg, rtol=0, atol=1e-13), (key, law, agg, want_agg)


@pytest.mark.parametrize("law", LAWS)
def test_both_groups_and_their_boundary(eng, law):
    """1326 hero hands in two groups of blocks against {AA, KK}: the rows of the CPU test's eight hands, and under the
    uniform law every row's total weight in closed form."""
    c = PC.case(None, {"AA", "KK"}, 52)
    rows = w13(eng.exact_hero_range_preflop(*HC.records(c), law)[0])[0]
    assert (rows[:, 0] != 0).all() and (rows[:, 1] == 0).all()
    want_rows = PC.boundary_hands(52)
    assert {0, 1023, 1024, 1325} <= set(want_rows)
    hands = [PC.ROW_HANDS[r] for r in want_rows]
    one = one_record_rows(eng, c, hands, law)
    for r, want in zip(want_rows, one):
        assert np.array_equal(rows[r], want), (law, r, rows[r], want)
    assert (rows[:, 2] + rows[:, 3] == rows[:, 4:].sum(axis=1)).all()
    if law == "uniform":
        opp = [(a, b) for a, b in PC.ROW_HANDS if a >> 2 == b >> 2 and a >> 2 in (11, 12)]      # KK and AA
        assert len(opp) == 12
        boards = math.comb(52 - 4, 5)
        for r, (a, b) in enumerate(PC.ROW_HANDS):
            n = sum(1 for g in opp if not {a, b} & set(g))
            assert int(rows[r, 0]) == n * boards, (a, b)


def test_slices_batches_and_repeats(eng, monkeypatch):
    """A slice forcing 11 (52 cards) and 9 (50 cards) launches, a slice as large as a thread's 32-bit sums allow (two
    launches) and the default give identical rows; two records in one call equal two calls; a repeat is byte-identical."""
    keys = [("top10", 52), ("3cls", 50)]
    q, x = HC.batch([NARROW[k] for k in keys])
    for law in LAWS:
        both_r, both_a = eng.exact_hero_range_preflop(q, x, law)
        again_r, again_a = eng.exact_hero_range_preflop(q, x, law)
        assert both_r.tobytes() == again_r.tobytes() and both_a.tobytes() == again_a.tobytes()
        for i, k in enumerate(keys):
            r, a = narrow_rows(eng, k, law)
            assert np.array_equal(w13(both_r)[i], r) and np.array_equal(agg11(both_a)[i], a), (k, law)
    for slice_ in ("249999", "2598960"):
        monkeypatch.setenv("MCQ_HERO_PRE_SLICE", slice_)
        e2 = npa.Engine(0)
        try:
            assert math.comb(50, 5) // 249999 >= 8
            for law in LAWS:
                r2, a2 = e2.exact_hero_range_preflop(q, x, law)
                for i, k in enumerate(keys):
                    r, a = narrow_rows(eng, k, law)
                    assert np.array_equal(w13(r2)[i], r) and np.array_equal(agg11(a2)[i], a), (slice_, k, law)
        finally:
            e2.close()


def test_monte_carlo_hero_range_converges_to_the_reference_law_aggregate(eng):
    """10^8 production iterations of mcq_eval_batch_ext with hero_is_range = 1 against agg under the reference's law (eleven
    statistics, 5.5 sigma: tests/lawstats.py); the uniform law's aggregate lies outside that bound (that the two differ by
    more than twice the bound is checked on the CPU: tests/test_hero_preflop_host.py)."""
    key = ("3cls", 52)
    ref, uni = narrow_rows(eng, key, "reference")[1], narrow_rows(eng, key, "uniform")[1]
    q, x = HC.records(NARROW[key])
    q["runs"] = 100000000
    mc = eng.eval_batch_ext(q, x, seed=520052)
    assert int(mc["runs"][0]) == 100000000
    LS.check("preflop {AA, AKs} v {KK, QQ, AKo}, reference law", LS.one_sample(mc, ref))
    off = LS.one_sample(mc, uni)
    print(LS.report("preflop, uniform law", off))
    assert LS.max_z(off) > LS.BOUND


def test_refusals_leave_the_outputs_untouched(eng):
    c = NARROW[("3cls", 50)]
    good = HC.records(c)
    qh, xh = HC.records(c, hero_is_range=False)
    qh["hole"][0] = [HC.C("3C"), HC.C("3D")]
    q3, xk = good[0].copy(), good[1].copy()
    q3["n_players"] = 3
    xk["n_known"] = 1
    xk["known"]["cards"][0, 0] = [HC.C("3C"), HC.C("3D")]
    xe = good[1].copy()
    xe["opp_range"] = 0
    flop = HC.records(HC.CASES["flop_3cls"])
    undealable = HC.records(({"AA"}, {"AA"}, [], ["AH", "AS"]))          # AC AD against AA: no aces left
    refused = [(flop[0], flop[1], 0, "mcq_exact_batch_hero_range takes the flop"), HC.records(c, n_players=3) + (0, "n_players"),
               (q3, xk, 0, "n_known"), (qh, xh, 0, "hero_is_range"), good + (2, "bad law"), (good[0], xe, 0, "invalid"),
               undealable + (0, "cannot be dealt"), undealable + (1, "cannot be dealt")]
    L = eng._lib
    entry = L.mcq_exact_batch_hero_range_preflop
    for q, x, law, why in refused:
        rows = np.full((ROWS, 13), SENTINEL, np.uint64)
        agg = np.full(11, -3.0)
        rc = entry(eng._ctx, q.ctypes.data, x.ctypes.data, 1, law, rows.ctypes.data, agg.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and (rows == SENTINEL).all() and (agg == -3.0).all(), why
        assert why.encode() in L.mcq_last_error(), (why, L.mcq_last_error())
    # 65 records; a refusal inside a batch: nothing is written for the records before it either
    q65, x65 = np.concatenate([good[0]] * 65), np.concatenate([good[1]] * 65)
    rows = np.full((65, ROWS, 13), SENTINEL, np.uint64)
    assert entry(eng._ctx, q65.ctypes.data, x65.ctypes.data, 65, 0, rows.ctypes.data, None) == _lib.MCQ_EINVAL
    assert b"MCQ_HERO_PREFLOP_MAX_BATCH" in L.mcq_last_error() and (rows == SENTINEL).all()
    q2, x2 = np.concatenate([good[0], undealable[0]]), np.concatenate([good[1], undealable[1]])
    assert entry(eng._ctx, q2.ctypes.data, x2.ctypes.data, 2, 0, rows.ctypes.data, None) == _lib.MCQ_EINVAL
    assert (rows == SENTINEL).all()
    with pytest.raises(ValueError):
        eng.exact_hero_range_preflop(*good, law="production")
    with pytest.raises(ValueError):
        eng.exact_hero_range_preflop(*flop)
    # the postflop entry keeps its refusal of an empty table
    with pytest.raises(ValueError):
        eng.exact_hero_range(*good)
    with pytest.raises(ValueError):
        mh.get_range_equity_exact(PC.NARROW_HERO, [], engine=eng)
    # the same context goes on; agg may be NULL
    out = np.zeros((ROWS, 13), np.uint64)
    assert entry(eng._ctx, good[0].ctypes.data, good[1].ctypes.data, 1, 0, out.ctypes.data, None) == 0
    assert np.array_equal(out, narrow_rows(eng, ("3cls", 50), "reference")[0]) and out[:, 0].any()


def test_second_call_on_a_busy_context_is_turned_away(eng):
    """One call in flight per context: while a batch is enumerated, a second caller gets MCQ_EBUSY and the long call is not
    disturbed."""
    big = HC.batch([PC.case(None, {"AA", "KK"}, 52)] * 4)
    small = HC.records(NARROW[("3cls", 50)])
    want_small = narrow_rows(eng, ("3cls", 50), "reference")[0]
    started, results, busy = threading.Event(), [], [0]

    def long_call():
        started.set()
        while not results:
            try:
                results.append(w13(eng.exact_hero_range_preflop(*big)[0]))
            except npa.McqBusyError as e:      # the short call was in flight: turned away likewise, try again
                assert "context busy" in str(e)
                busy[0] += 1
    th = threading.Thread(target=long_call)
    th.start()
    started.wait()
    deadline = time.time() + 5
    while th.is_alive() and time.time() < deadline:
        try:
            assert np.array_equal(w13(eng.exact_hero_range_preflop(*small)[0])[0], want_small)   # got in between two calls
        except npa.McqBusyError as e:
            assert "context busy" in str(e)
            busy[0] += 1
    th.join()
    assert busy[0] > 0
    assert all(np.array_equal(results[0][i], results[0][0]) for i in range(4)) and (results[0][0][:, 0] != 0).all()
    assert np.array_equal(w13(eng.exact_hero_range_preflop(*small)[0])[0], want_small)


@pytest.mark.parametrize("ties", ["credited", "split"])
def test_get_preflop_range_equity_exact(eng, ties):
    """Hand by hand what get_equity_exact gives with the hero holding that hand, on case 1; the class table."""
    for law in LAWS:
        eq, hands, classes = mh.get_preflop_range_equity_exact(PC.NARROW_HERO, opponent_range=PC.TOP10, dealing=law, engine=eng,
                                                               ties=ties, by_class=True)
        allowed = HC.allowed_hands(NARROW[("top10", 52)])
        assert sorted(hands) == sorted((npa.card_str(a), npa.card_str(b)) for a, b in allowed)
        num = den = 0.0
        for a, b in allowed:
            e, w = hands[(npa.card_str(a), npa.card_str(b))]
            assert w == (1 if law == "uniform" or 51 in (a, b) else 2)
            if law == "reference" or (a, b) in (allowed[0], allowed[-1]):
                want, _ = mh.get_equity_exact([npa.card_str(a), npa.card_str(b)], [], 2, law, eng, opponent_range=PC.TOP10, ties=ties)
                assert e == pytest.approx(want, abs=1e-12)
            num += w * e
            den += w
        assert eq == pytest.approx(num / den, abs=1e-12)
        assert set(classes) == {"AA", "AKS"}
        assert classes["AA"][1] + classes["AKS"][1] == den
        aa = [hands[k] for k in hands if k[0][0] == "A" and k[1][0] == "A"]
        assert len(aa) == 6 and classes["AA"][0] == pytest.approx(sum(e * w for e, w in aa) / sum(w for _, w in aa), abs=1e-15)
    two = mh.get_preflop_range_equity_exact(PC.NARROW_HERO, opponent_range=PC.OPP_3CLS, ghost_cards=["AH", "AS"], engine=eng)
    assert len(two) == 2 and len(two[1]) == 3
