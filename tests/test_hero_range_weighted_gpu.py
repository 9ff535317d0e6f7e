"""mcq_exact_batch_hero_range_weighted on the GPU: the kernel's rows against the host build of the same lane code, against
the unweighted entry (all weights 1, class-aligned tables, the all-65535 flop), and the conventions of an entry
(determinism, batch invariance, refusals); the public function on top."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from neuron_poker_amd import montecarlo_hip as mh
from tests import hero_range_cases as HC
from tests import hostsim_hero_weighted as HW
from tests import weighted_range_cases as WC

pytestmark = pytest.mark.gpu
SENTINEL = 0xABABABABABABABAB
# the river with every hand allowed (1081 hero hands: the second thread group works), the ghost turn, the narrow flop
# with hero weights, a flop with every hand allowed against the hand-level table
MIXED = ["river_hand_level", "turn_ghost_class", "flop_3cls_hero", "flop_all_hand_level"]
_host = {}


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w13(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, HW.ROWS, 13)


def agg11(agg):
    return np.ascontiguousarray(agg).view(np.float64).reshape(-1, 11)


def host(name):
    """The host build's (rows, agg) of a weighted case, computed once and left unchanged."""
    if name not in _host:
        q, x, ow, hw = WC.records(name)
        r, a = HW.hero_weighted(q, x, ow, hw)
        r.setflags(write=False)
        _host[name] = (r, a)
    return _host[name]


def _check_mixed(e):
    q, x, ow, hw = WC.batch(MIXED)
    rows, agg = e.exact_hero_range_weighted(q, x, ow, hw)
    for i, name in enumerate(MIXED):
        want, want_agg = host(name)
        assert np.array_equal(w13(rows)[i], want), name
        assert np.array_equal(agg11(agg)[i], want_agg), name        # the same host code on the same integers
    assert int((w13(rows)[0][:, 0] != 0).sum()) == 1081
    assert int(w13(rows)[3][:, 0].max()) > 2 ** 32                   # the flop's sums do pass 32 bits


def test_mixed_batch_against_the_host_build(eng):
    _check_mixed(eng)


def test_mixed_batch_when_one_block_owns_every_completion(monkeypatch):
    """A fresh engine that reads MCQ_EXACT_CU=1: a block per thread group walks all 1176 completions of a flop, so every
    64-bit sum is carried across them in one thread."""
    monkeypatch.setenv("MCQ_EXACT_CU", "1")
    e = npa.Engine(0)
    try:
        _check_mixed(e)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["flop_top25", "turn_vs_any"])
def test_all_weights_one_is_the_unweighted_entry(eng, name):
    q, x = HC.records(HC.CASES[name])
    want, want_agg = eng.exact_hero_range(q, x, "uniform")
    rows, agg = eng.exact_hero_range_weighted(q, x, WC.ones().reshape(1, -1))
    assert rows.tobytes() == want.tobytes() and agg.tobytes() == want_agg.tobytes()
    assert w13(rows)[0][:, 0].any()


def test_class_aligned_table_is_a_sum_of_unweighted_calls(eng):
    """rows == sum_v v x exact_hero_range(opp_range = the classes of weight v inside the case's opponent range): the
    kernel against code that knows nothing of weights."""
    base, ow, _ = WC.WCASES["flop_top25_class"]
    q, x, ow1, _ = WC.records("flop_top25_class")
    rows, _ = eng.exact_hero_range_weighted(q, x, ow1)
    want = np.zeros((HW.ROWS, 13), np.uint64)
    opp_bits = x["opp_range"][0]
    seen = 0
    for v in (1, 3, 1000):
        bits = np.zeros(6, np.uint32)
        for c in range(169):
            if (ow[WC.CLASS_OF == c] == v).all() and (int(opp_bits[c >> 5]) >> (c & 31)) & 1:
                bits[c >> 5] |= np.uint32(1 << (c & 31))
        assert bits.any(), v
        xv = x.copy()
        xv["opp_range"][0] = bits
        want += np.uint64(v) * w13(eng.exact_hero_range(q, xv, "uniform")[0])[0]
        seen += 1
    assert seen == 3 and np.array_equal(w13(rows)[0], want) and want[:, 0].any()


def test_full_flop_with_every_weight_65535(eng):
    """Rows == 65535 x the unweighted rows: 7.0e10 per hero hand, the overflow pin on the device."""
    q, x, ow, _ = WC.records("flop_all_max")
    plain, plain_agg = eng.exact_hero_range(q, x, "uniform")
    rows, agg = eng.exact_hero_range_weighted(q, x, ow)
    got = w13(rows)[0]
    assert np.array_equal(got, w13(plain)[0] * np.uint64(WC.WMAX))
    assert int((got[:, 0] == 1081 * 990 * WC.WMAX).sum()) == 1176
    assert np.allclose(agg11(agg), agg11(plain_agg), rtol=0, atol=1e-15)


def test_zero_hero_weights_inside_an_allowed_class(eng):
    base, _, hw = WC.WCASES["turn_hero_zeros"]
    case = HC.CASES[base]
    q, x, ow1, hw1 = WC.records("turn_hero_zeros")
    rows, agg = eng.exact_hero_range_weighted(q, x, ow1, hw1)
    r = w13(rows)[0]
    by_class = HC.allowed_hands(case)
    zero = [h for h in by_class if hw[_lib.hand_index(*h)] == 0]
    live = [h for h in by_class if hw[_lib.hand_index(*h)] != 0]
    assert len(zero) > 10 and len(live) > 10
    assert all((r[_lib.hand_index(*h)] == 0).all() for h in zero)
    assert int((r[:, 0] != 0).sum()) == len(live)
    idx = np.array([_lib.hand_index(*h) for h in live])
    w = hw[idx].astype(np.float64)
    runs = r[idx, 0].astype(np.float64)
    want = [(w * r[idx, 2 + k].astype(np.float64) / runs).sum() / w.sum() for k in range(11)]
    assert np.abs(agg11(agg)[0] - np.array(want)).max() <= 1e-12
    assert np.array_equal(r, host("turn_hero_zeros")[0])


def test_two_calls_give_identical_rows_and_a_batch_equals_single_calls(eng):
    names = ["turn_ghost_class", "flop_3cls_hero", "river_hand_level"]
    q, x, ow, hw = WC.batch(names)
    a, b = eng.exact_hero_range_weighted(q, x, ow, hw), eng.exact_hero_range_weighted(q, x, ow, hw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert w13(a[0])[:, :, 0].any(axis=1).all()
    for i in range(3):
        r1, a1 = eng.exact_hero_range_weighted(q[i:i + 1], x[i:i + 1], ow[i:i + 1], hw[i:i + 1])
        assert np.array_equal(w13(a[0])[i], w13(r1)[0]) and np.array_equal(agg11(a[1])[i], agg11(a1)[0]), names[i]


def test_refusals_leave_the_outputs_untouched(eng):
    case = HC.CASES["turn_ghost"]
    good = HC.records(case)
    ones = WC.ones()
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
    river = HC.records(HC.CASES["river_all"])
    victim = HC.allowed_hands(HC.CASES["river_all"])[500]
    sharing = np.array([1 if set(h) & set(victim) else 0 for h in WC.HANDS], np.uint16)
    zeros = np.zeros(WC.ROWS, np.uint16)
    refused = [(qh, xh, ones, None, "hero_is_range"), (q3, xk, ones, None, "n_known"),
               HC.records(case, n_players=3) + (ones, None, "n_players"),
               (_lib.pack_query_one([0, 0], [], 2, 1), good[1], ones, None, "C(50, 5)"), (qd, good[1], ones, None, "invalid"),
               (good[0], xe, ones, None, "invalid"), good + (None, ones, "null opp_weights"),
               HC.records(({"77"}, None, ["7C", "7D", "7H", "2S"], None)) + (ones, None, "no hand"),
               good + (ones, zeros, "no hand"),
               HC.records(HC.UNDEALABLE) + (ones, None, "cannot be dealt"), good + (zeros, None, "cannot be dealt"),
               river + (sharing, None, "cannot be dealt")]
    L = eng._lib
    for q, x, ow, hw, why in refused:
        rows = np.full((HW.ROWS, 13), SENTINEL, np.uint64)
        agg = np.full(11, -3.0)
        rc = L.mcq_exact_batch_hero_range_weighted(eng._ctx, q.ctypes.data, x.ctypes.data, 1, None if ow is None else ow.ctypes.data,
                                                   None if hw is None else hw.ctypes.data, rows.ctypes.data, agg.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and (rows == SENTINEL).all() and (agg == -3.0).all(), why
        assert why.encode() in L.mcq_last_error(), (why, L.mcq_last_error())
    # a refusal inside a batch: nothing is written for the records before it either
    rows = np.full((2, HW.ROWS, 13), SENTINEL, np.uint64)
    q, x = np.concatenate([good[0], river[0]]), np.concatenate([good[1], river[1]])
    ow = np.stack([ones, sharing])
    rc = L.mcq_exact_batch_hero_range_weighted(eng._ctx, q.ctypes.data, x.ctypes.data, 2, ow.ctypes.data, None, rows.ctypes.data, None)
    assert rc == _lib.MCQ_EINVAL and (rows == SENTINEL).all()
    # without the hand it cannot be dealt against, the same opponent table is fine; the context goes on; agg may be NULL
    hero_without = np.array([0 if h == victim else 1 for h in WC.HANDS], np.uint16)
    out = np.zeros((HW.ROWS, 13), np.uint64)
    assert L.mcq_exact_batch_hero_range_weighted(eng._ctx, river[0].ctypes.data, river[1].ctypes.data, 1, sharing.ctypes.data,
                                                 hero_without.ctypes.data, out.ctypes.data, None) == 0
    assert int((out[:, 0] != 0).sum()) == 1080 and (out[_lib.hand_index(*victim)] == 0).all()
    with pytest.raises(ValueError):
        eng.exact_hero_range_weighted(good[0], good[1], ones)                   # shape [1326], not [1, 1326]
    with pytest.raises(ValueError):
        eng.exact_hero_range_weighted(good[0], good[1], ones.reshape(1, -1).astype(np.uint32))


def test_public_function_with_plain_ranges_is_the_uniform_law(eng):
    hero, opp, table, ghost = HC.CASES["turn_ghost"]
    for ties in ("credited", "split"):
        want_eq, want = mh.get_range_equity_exact(hero, table, opponent_range=opp, dealing="uniform", ghost_cards=ghost, engine=eng,
                                                  ties=ties)
        eq, hands = mh.get_range_equity_exact_weighted(hero, table, opp, ghost_cards=ghost, engine=eng, ties=ties)
        assert hands == {h: (e, 1.0) for h, (e, w) in want.items()} and all(w == 1 for _, w in want.values())
        assert eq == pytest.approx(want_eq, abs=1e-15)
    with pytest.raises(ValueError):
        mh.get_range_equity_exact_weighted({"AKS"}, [], 1, engine=eng)                          # preflop
    with pytest.raises(ValueError):
        mh.get_range_equity_exact_weighted({"AKS"}, table, 1, engine=eng, ties="half")


def test_public_function_with_dicts_and_split_ties(eng):
    """Hero: AhKh for certain and AKo half of the time; the opponent calls with AQo half of the time, always with QQ, and
    with KsQs but no other KQs.  Checked against the entry called with tables built by hand."""
    table = ["QD", "9S", "4H", "AC"]
    hero = {("AH", "KH"): 1.0, "AKO": 0.5}
    opp = {"AQO": 0.5, "QQ": 1, ("KS", "QS"): 1.0}
    eq, hands = mh.get_range_equity_exact_weighted(hero, table, opp, engine=eng, ties="split")
    cid = npa.card_id
    ow, hw = np.zeros((1, WC.ROWS), np.uint16), np.zeros((1, WC.ROWS), np.uint16)
    for i, (a, b) in enumerate(WC.HANDS):
        ra, rb, suited = a >> 2, b >> 2, (a & 3) == (b & 3)
        if {ra, rb} == {12, 10} and not suited:
            ow[0, i] = 32768
        if ra == rb == 10:
            ow[0, i] = 65535
        if {ra, rb} == {12, 11} and not suited:
            hw[0, i] = 32768
    ow[0, _lib.hand_index(cid("KS"), cid("QS"))] = 65535
    hw[0, _lib.hand_index(cid("AH"), cid("KH"))] = 65535
    q = _lib.pack_query_one([0, 0], [cid(c) for c in table], 2, 1)
    x = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES)
    r = w13(eng.exact_hero_range_weighted(q, x, ow, hw)[0])[0]
    live = np.flatnonzero(r[:, 0])
    assert len(live) == 1 + 9 == len(hands)                            # AC is on the table: nine AKo are left
    num = den = 0.0
    for i in live:
        a, b = WC.HANDS[i]
        e, w = hands[(npa.card_str(a), npa.card_str(b))]
        assert e == pytest.approx((int(r[i, 2]) + int(r[i, 3]) / 2.0) / int(r[i, 0]), abs=1e-15)
        assert w == int(hw[0, i]) / 65535.0 and w in (1.0, 32768 / 65535.0)
        num += w * e
        den += w
    assert eq == pytest.approx(num / den, abs=1e-12)
    with pytest.raises(ValueError):
        mh.get_range_equity_exact_weighted(hero, table, {"AQO": 1e-6}, engine=eng)


def test_single_hand_against_the_literal_walk(eng):
    """One weighted river row for a single hero hand."""
    case = HC.CASES["river_all"]
    ow = WC.hand_level(31)
    h = HC.allowed_hands(case)[123]
    hw = np.zeros((1, WC.ROWS), np.uint16)
    hw[0, _lib.hand_index(*h)] = 5
    q, x = HC.records(case)
    rows, agg = eng.exact_hero_range_weighted(q, x, ow.reshape(1, -1), hw)
    sums, lit_agg = WC.literal(case, ow, hw[0])
    assert list(sums) == [h]
    r = w13(rows)[0]
    assert WC.row_ints(r[_lib.hand_index(*h)]) == sums[h] and int((r[:, 0] != 0).sum()) == 1
    assert np.abs(agg11(agg)[0] - np.array([float(v) for v in lit_agg])).max() <= 1e-12
