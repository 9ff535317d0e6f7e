"""mcq_exact_batch_hero_range_preflop_weighted on the GPU: every allowed row against its decomposition into known-hand
records (Engine.exact_ext, code that knows nothing of weights or ranges), against the unweighted preflop entry (all weights
1, class-aligned tables, every weight 65535), both groups of blocks with a holed hero table, the 64-bit sums, the slicing,
and the conventions of an entry (determinism, batch invariance, refusals, MCQ_EBUSY); the public function on top.  k = 5
and |D| >= 50 cannot shrink, so the ranges are narrow."""
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
from tests import test_hero_preflop_gpu as TP
from tests import weighted_preflop_cases as WP
from tests import weighted_range_cases as WC

pytestmark = pytest.mark.gpu
SENTINEL = 0xABABABABABABABAB
ROWS = 1326
NARROW = ["narrow_3cls_52", "narrow_3cls_50", "narrow_top10_52", "narrow_top10_50"]
_rows = {}
_known = {}


@pytest.fixture(scope="module")
def eng():
    e = npa.Engine(0)
    yield e
    e.close()


def w13(rows):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, ROWS, 13)


def agg11(agg):
    return np.ascontiguousarray(agg).view(np.float64).reshape(-1, 11)


def case_rows(eng, name):
    """(rows[1326, 13], agg[11]) of a case from the module's engine (default slice), computed once, left unchanged."""
    if name not in _rows:
        rows, agg = eng.exact_hero_range_preflop_weighted(*WP.records(name))
        r, a = w13(rows)[0].copy(), agg11(agg)[0].copy()
        r.setflags(write=False)
        a.setflags(write=False)
        _rows[name] = (r, a)
    return _rows[name]


def known_hand_rows(eng, ghost, pairs):
    """{(h, g): the 13-word weights row of Engine.exact_ext, uniform law, for the hero holding h against the KNOWN hand g and
    no random opponent} -- ONE batched call for the pairs not seen before."""
    key = tuple(ghost or ())
    new = [p for p in dict.fromkeys(pairs) if (key, p) not in _known]
    if new:
        q = np.concatenate([_lib.pack_query_one(list(h), [], 2, 1) for h, _ in new])
        x = _lib.pack_query_ext(len(new), ghost=ghost, known2=[0, 1])
        for i, (_, g) in enumerate(new):
            x["known"]["cards"][i, 0] = list(g)
        _, w = eng.exact_ext(q, x, "uniform")
        w = np.ascontiguousarray(w).view(np.uint64).reshape(-1, 13)
        for p, row in zip(new, w):
            _known[(key, p)] = [int(v) for v in row]
    return {p: _known[(key, p)] for p in pairs}


def decomposition(eng, case, eff_o, hands):
    """{h: the 13 words sum_g eff_opp(g) x row(h against the known hand g) over the g that share no card with h}."""
    ghost = HC.parts(case)[3]
    live = [(WC.HANDS[i], int(eff_o[i])) for i in np.flatnonzero(eff_o)]
    pairs = [(h, g) for h in hands for g, _ in live if not set(h) & set(g)]
    one = known_hand_rows(eng, ghost, pairs)
    boards = math.comb(len(HC.deck(case)) - 4, 5)
    out = {}
    for h in hands:
        s = [0] * 13
        for g, w in live:
            if set(h) & set(g):
                continue
            r = one[(h, g)]
            assert r[0] == boards and r[1] == 0                                   # every completion once
            for k in range(13):
                s[k] += w * r[k]
        out[h] = s
    return out


def recombined(rows, eff_h):
    """agg from the rows as the host combines them: ascending row order, the weights eff_hero, in doubles."""
    num, den = [0.0] * 11, 0.0
    for i in np.flatnonzero(eff_h):
        r = [int(v) for v in rows[i]]
        w, runs = float(eff_h[i]), float(r[0])
        num[0] += w * float(r[2]) / runs
        num[1] += w * float(r[3]) / runs
        for t in range(9):
            num[2 + t] += w * float(r[4 + t]) / runs
        den += w
    return [v / den for v in num]


# ---- 1. the ground truth: known-hand records
@pytest.mark.parametrize("name", NARROW)
def test_every_allowed_row_is_the_weighted_sum_of_known_hand_rows(eng, name):
    case = WP.WPCASES[name][0]
    rows, agg = case_rows(eng, name)
    eff_o, eff_h = WP.effective(name)
    hands = WP.allowed_hands(name)
    assert 0 < len(hands) < len(HC.allowed_hands(case))                           # the hero's table zeroes some
    want = decomposition(eng, case, eff_o, hands)
    live = np.zeros(ROWS, bool)
    for h in hands:
        i = _lib.hand_index(*h)
        live[i] = True
        got = [int(v) for v in rows[i]]
        assert got == want[h] and got[0] > 0, (name, h, got, want[h])
    assert (rows[~live] == 0).all(), name
    assert np.allclose(agg, recombined(rows, eff_h), rtol=0, atol=1e-13), name


# ---- 2. all weights 1: the unweighted entry under the uniform law
def test_all_weights_one_is_the_unweighted_entry_bit_for_bit(eng):
    ones = WC.ones().reshape(1, -1)
    assert len(TP.NARROW) == 4
    for key, c in TP.NARROW.items():
        q, x = HC.records(c)
        want, want_agg = eng.exact_hero_range_preflop(q, x, "uniform")
        rows, agg = eng.exact_hero_range_preflop_weighted(q, x, ones)
        assert rows.tobytes() == want.tobytes() and agg.tobytes() == want_agg.tobytes(), key
        assert w13(rows)[0][:, 0].any()


def all_vs_aa_kk(eng):
    """The unweighted uniform-law rows of every class against {AA, KK}, once."""
    if "plain" not in _rows:
        r = w13(eng.exact_hero_range_preflop(*HC.records(PC.case(None, WP.AA_KK, 52)), "uniform")[0])[0].copy()
        r.setflags(write=False)
        _rows["plain"] = r
    return _rows["plain"]


def test_all_weights_one_both_groups_of_blocks(eng):
    q, x = HC.records(PC.case(None, WP.AA_KK, 52))
    want, want_agg = eng.exact_hero_range_preflop(q, x, "uniform")
    rows, agg = eng.exact_hero_range_preflop_weighted(q, x, WC.ones().reshape(1, -1))
    assert rows.tobytes() == want.tobytes() and agg.tobytes() == want_agg.tobytes()
    assert (w13(rows)[0][:, 0] != 0).all() and np.array_equal(w13(want)[0], all_vs_aa_kk(eng))


# ---- 3. a class-aligned table
def test_class_aligned_table_is_a_sum_of_unweighted_calls(eng):
    """rows == sum_v v x exact_hero_range_preflop(opp_range = the classes of weight v inside the top 10 %)."""
    c = PC.case(PC.NARROW_HERO, PC.TOP10, 52)
    q, x = HC.records(c)
    ow = WC.class_aligned(61)
    rows, _ = eng.exact_hero_range_preflop_weighted(q, x, ow.reshape(1, -1))
    want = np.zeros((ROWS, 13), np.uint64)
    opp_bits = x["opp_range"][0]
    seen = {}
    for v in (0, 1, 3, 1000):
        bits = np.zeros(6, np.uint32)
        for k in range(169):
            if (ow[WC.CLASS_OF == k] == v).all() and (int(opp_bits[k >> 5]) >> (k & 31)) & 1:
                bits[k >> 5] |= np.uint32(1 << (k & 31))
                seen[v] = seen.get(v, 0) + 1
        assert bits.any(), v
        if v:
            xv = x.copy()
            xv["opp_range"][0] = bits
            want += np.uint64(v) * w13(eng.exact_hero_range_preflop(q, xv, "uniform")[0])[0]
    assert sum(seen.values()) == sum(bin(int(w)).count("1") for w in opp_bits) == 16 and len(seen) == 4
    assert np.array_equal(w13(rows)[0], want) and int((want[:, 0] != 0).sum()) == 10


# ---- 4. the group boundary with a holed hero table
def test_group_boundary_with_a_holed_hero_table(eng):
    name = "holed_52"
    case = WP.WPCASES[name][0]
    rows, agg = case_rows(eng, name)
    eff_o, eff_h = WP.effective(name)
    hands = WP.allowed_hands(name)
    n = len(hands)
    assert 1024 < n < 1326 and _lib.hand_index(*hands[1023]) != 1023
    at = [0, 1, 511, 1023, 1024, 1025, n - 2, n - 1]
    some = [hands[i] for i in at]
    want = decomposition(eng, case, eff_o, some)
    for h in some:
        got = [int(v) for v in rows[_lib.hand_index(*h)]]
        assert got == want[h] and got[0] > 0, (h, got, want[h])
    assert int((rows[:, 0] != 0).sum()) == n and (rows[eff_h == 0] == 0).all() and int((eff_h == 0).sum()) > 200
    assert (rows[:, 2] + rows[:, 3] == rows[:, 4:].sum(axis=1)).all()
    assert np.allclose(agg, recombined(rows, eff_h), rtol=0, atol=1e-13)


# ---- 5. the 64-bit sums on the device
def test_every_weight_65535_with_long_runs_per_block(monkeypatch):
    """A slice of 1 500 000 completions over CUs / 2 blocks per group: one block owns more than 2^32 / (12 x 65535)
    completions in a launch, so 32-bit sums per thread would wrap."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = cus // 2                                                               # two groups of blocks share the CUs
    owned = -(-1500000 // per)
    assert owned * 12 * WC.WMAX > 2 ** 32 and owned > 5461, (cus, owned)
    monkeypatch.setenv("MCQ_HERO_PRE_SLICE", "1500000")
    e2 = npa.Engine(0)
    try:
        plain = all_vs_aa_kk(e2)
        q, x = HC.records(PC.case(None, WP.AA_KK, 52))
        rows, agg = e2.exact_hero_range_preflop_weighted(q, x, WC.all_max().reshape(1, -1))
    finally:
        e2.close()
    got = w13(rows)[0]
    assert np.array_equal(got, plain * np.uint64(WC.WMAX))
    full = 12 * math.comb(48, 5) * WC.WMAX
    for r, (a, b) in enumerate(PC.ROW_HANDS):
        if a >> 2 < 11 and b >> 2 < 11:                                          # neither an ace nor a king
            assert int(got[r, 0]) == full, (a, b)
    assert full > 2 ** 40


# ---- 6. slices, batches, repeats
def test_slices_batches_and_repeats(eng, monkeypatch):
    names = ["narrow_top10_52", "narrow_3cls_50"]
    recs = [WP.records(n) for n in names]
    q, x = np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])
    ow = np.concatenate([r[2] for r in recs])
    hw = np.concatenate([recs[0][3], WC.ones().reshape(1, -1)])                  # the second record: every hero weight 1
    both_r, both_a = eng.exact_hero_range_preflop_weighted(q, x, ow, hw)
    again_r, again_a = eng.exact_hero_range_preflop_weighted(q, x, ow, hw)
    assert both_r.tobytes() == again_r.tobytes() and both_a.tobytes() == again_a.tobytes()
    r0, a0 = case_rows(eng, names[0])
    assert np.array_equal(w13(both_r)[0], r0) and np.array_equal(agg11(both_a)[0], a0)
    null_r, null_a = eng.exact_hero_range_preflop_weighted(recs[1][0], recs[1][1], recs[1][2], None)
    assert np.array_equal(w13(both_r)[1], w13(null_r)[0]) and np.array_equal(agg11(both_a)[1], agg11(null_a)[0])
    assert not np.array_equal(w13(null_r)[0], case_rows(eng, names[1])[0])       # (the hero table of the case differs)
    assert w13(both_r)[:, :, 0].any(axis=1).all()
    for slice_ in ("249999", "1500000"):
        monkeypatch.setenv("MCQ_HERO_PRE_SLICE", slice_)
        e2 = npa.Engine(0)
        try:
            r2, a2 = e2.exact_hero_range_preflop_weighted(q, x, ow, hw)
            assert r2.tobytes() == both_r.tobytes() and a2.tobytes() == both_a.tobytes(), slice_
        finally:
            e2.close()


# ---- 7. refusals
def test_refusals_leave_the_outputs_untouched(eng):
    c = WP.WPCASES["narrow_3cls_50"][0]
    good = HC.records(c)
    ones, zeros = WC.ones(), np.zeros(WC.ROWS, np.uint16)
    qh, xh = HC.records(c, hero_is_range=False)
    qh["hole"][0] = [HC.C("3C"), HC.C("3D")]
    q3, xk = good[0].copy(), good[1].copy()
    q3["n_players"] = 3
    xk["n_known"] = 1
    xk["known"]["cards"][0, 0] = [HC.C("3C"), HC.C("3D")]
    xe = good[1].copy()
    xe["opp_range"] = 0
    flop = HC.records(HC.CASES["flop_3cls"])
    undealable = HC.records(({"AA"}, {"AA"}, [], ["AH", "AS"]))                  # AC AD against AA: no aces left
    aks = HC.records(PC.case({"AKS"}, None, 52))
    only = zeros.copy()
    only[_lib.hand_index(HC.C("AH"), HC.C("AS"))] = 9                            # shares a card with AhKh and AsKs
    refused = [(flop[0], flop[1], ones, None, "mcq_exact_batch_hero_range_weighted takes the flop"),
               HC.records(c, n_players=3) + (ones, None, "n_players"), (q3, xk, ones, None, "n_known"),
               (qh, xh, ones, None, "hero_is_range"), (good[0], xe, ones, None, "invalid"),
               good + (None, ones, "null opp_weights"), good + (ones, zeros, "no hand"),
               undealable + (ones, None, "cannot be dealt"), good + (zeros, None, "cannot be dealt"),
               aks + (only, None, "cannot be dealt")]
    L = eng._lib
    entry = L.mcq_exact_batch_hero_range_preflop_weighted
    for q, x, ow, hw, why in refused:
        rows = np.full((ROWS, 13), SENTINEL, np.uint64)
        agg = np.full(11, -3.0)
        rc = entry(eng._ctx, q.ctypes.data, x.ctypes.data, 1, None if ow is None else ow.ctypes.data,
                   None if hw is None else hw.ctypes.data, rows.ctypes.data, agg.ctypes.data)
        assert rc == _lib.MCQ_EINVAL and (rows == SENTINEL).all() and (agg == -3.0).all(), why
        assert why.encode() in L.mcq_last_error(), (why, L.mcq_last_error())
    # 65 records; a refusal in the second record of a batch: nothing is written for the record before it either
    q65, x65, w65 = np.concatenate([good[0]] * 65), np.concatenate([good[1]] * 65), np.stack([ones] * 65)
    rows = np.full((65, ROWS, 13), SENTINEL, np.uint64)
    assert entry(eng._ctx, q65.ctypes.data, x65.ctypes.data, 65, w65.ctypes.data, None, rows.ctypes.data, None) == _lib.MCQ_EINVAL
    assert b"MCQ_HERO_PREFLOP_MAX_BATCH" in L.mcq_last_error() and (rows == SENTINEL).all()
    q2, x2, w2 = np.concatenate([aks[0], aks[0]]), np.concatenate([aks[1], aks[1]]), np.stack([ones, only])
    assert entry(eng._ctx, q2.ctypes.data, x2.ctypes.data, 2, w2.ctypes.data, None, rows.ctypes.data, None) == _lib.MCQ_EINVAL
    assert b"query 1:" in L.mcq_last_error() and (rows == SENTINEL).all()
    with pytest.raises(ValueError):
        eng.exact_hero_range_preflop_weighted(good[0], good[1], ones)           # shape [1326], not [1, 1326]
    with pytest.raises(ValueError):
        eng.exact_hero_range_preflop_weighted(*flop, ones.reshape(1, -1))
    # the postflop weighted entry keeps its refusal of an empty table
    with pytest.raises(ValueError):
        eng.exact_hero_range_weighted(good[0], good[1], ones.reshape(1, -1))
    with pytest.raises(ValueError):
        mh.get_range_equity_exact_weighted(PC.NARROW_HERO, [], 1, engine=eng)
    # without the two hands it cannot be dealt against, the same opponent table is fine; the same context goes on; agg
    # may be NULL
    hero_without = ones.copy()
    hero_without[[_lib.hand_index(HC.C("KH"), HC.C("AH")), _lib.hand_index(HC.C("KS"), HC.C("AS"))]] = 0
    out = np.zeros((ROWS, 13), np.uint64)
    assert entry(eng._ctx, aks[0].ctypes.data, aks[1].ctypes.data, 1, only.ctypes.data, hero_without.ctypes.data, out.ctypes.data,
                 None) == 0
    assert int((out[:, 0] != 0).sum()) == 2 and (out[out[:, 0] != 0, 0] == 9 * math.comb(48, 5)).all()


# ---- 8. MCQ_EBUSY
def test_second_call_on_a_busy_context_is_turned_away(eng):
    """One call in flight per context: while a batch is enumerated, a second caller gets MCQ_EBUSY and the long call is not
    disturbed."""
    n = 4
    qb, xb = HC.batch([PC.case(None, WP.AA_KK, 52)] * n)
    wb = np.stack([WC.ones()] * n)
    small = WP.records("narrow_3cls_50")
    want_small = case_rows(eng, "narrow_3cls_50")[0]
    started, results, busy = threading.Event(), [], [0]

    def long_call():
        started.set()
        while not results:
            try:
                results.append(w13(eng.exact_hero_range_preflop_weighted(qb, xb, wb)[0]))
            except npa.McqBusyError as e:      # the short call was in flight: turned away likewise, try again
                assert "context busy" in str(e)
                busy[0] += 1
    th = threading.Thread(target=long_call)
    th.start()
    started.wait()
    deadline = time.time() + 5
    while th.is_alive() and time.time() < deadline:
        try:
            assert np.array_equal(w13(eng.exact_hero_range_preflop_weighted(*small)[0])[0], want_small)   # got in between two calls
        except npa.McqBusyError as e:
            assert "context busy" in str(e)
            busy[0] += 1
    th.join()
    assert busy[0] > 0
    assert all(np.array_equal(results[0][i], all_vs_aa_kk(eng)) for i in range(n))
    assert np.array_equal(w13(eng.exact_hero_range_preflop_weighted(*small)[0])[0], want_small)


# ---- 9. the public function
def test_public_function_with_plain_ranges_is_the_uniform_law(eng):
    for ties in ("credited", "split"):
        want_eq, want = mh.get_preflop_range_equity_exact(PC.NARROW_HERO, PC.TOP10, dealing="uniform", engine=eng, ties=ties)
        eq, hands, classes = mh.get_preflop_range_equity_exact_weighted(PC.NARROW_HERO, PC.TOP10, engine=eng, ties=ties, by_class=True)
        assert hands == {h: (e, 1.0) for h, (e, w) in want.items()} and all(w == 1 for _, w in want.values()) and len(hands) == 10
        assert eq == pytest.approx(want_eq, abs=1e-15)
        assert set(classes) == {"AA", "AKS"} and classes["AA"][1] == 6.0 and classes["AKS"][1] == 4.0
    two = mh.get_preflop_range_equity_exact_weighted(PC.NARROW_HERO, PC.OPP_3CLS, ghost_cards=["AH", "AS"], engine=eng)
    assert len(two) == 2 and len(two[1]) == 3


@pytest.mark.parametrize("ties", ["credited", "split"])
def test_public_function_with_dicts(eng, ties):
    """Hero raises AhKh for certain, A5s 40 % of the time and QQ always; the opponent calls with AQo half of the time,
    always with JJ, and with KsQs but no other KQs.  Checked against the entry called with tables built by hand."""
    hero = {("AH", "KH"): 1.0, "A5S": 0.4, "QQ": 1}
    opp = {"AQO": 0.5, "JJ": 1, ("KS", "QS"): 1.0}
    eq, hands, classes = mh.get_preflop_range_equity_exact_weighted(hero, opp, engine=eng, ties=ties, by_class=True)
    cid = npa.card_id
    ow, hw = np.zeros((1, WC.ROWS), np.uint16), np.zeros((1, WC.ROWS), np.uint16)
    for i, (a, b) in enumerate(WC.HANDS):
        ra, rb, suited = a >> 2, b >> 2, (a & 3) == (b & 3)
        if {ra, rb} == {12, 10} and not suited:
            ow[0, i] = 32768
        if ra == rb == 9:
            ow[0, i] = 65535
        if {ra, rb} == {12, 3} and suited:
            hw[0, i] = mh.quantise_weight(0.4)
        if ra == rb == 10:
            hw[0, i] = 65535
    ow[0, _lib.hand_index(cid("KS"), cid("QS"))] = 65535
    hw[0, _lib.hand_index(cid("AH"), cid("KH"))] = 65535
    q = _lib.pack_query_one([0, 0], [], 2, 1)
    x = _lib.pack_query_ext(1, hero_range=_lib.ALL_CLASSES)
    r = w13(eng.exact_hero_range_preflop_weighted(q, x, ow, hw)[0])[0]
    live = np.flatnonzero(r[:, 0])
    assert len(live) == 1 + 4 + 6 == len(hands)
    num = den = 0.0
    for i in live:
        a, b = WC.HANDS[i]
        e, w = hands[(npa.card_str(a), npa.card_str(b))]
        tie = int(r[i, 3]) / 2.0 if ties == "split" else int(r[i, 3])
        assert e == pytest.approx((int(r[i, 2]) + tie) / int(r[i, 0]), abs=1e-15)
        assert w == int(hw[0, i]) / 65535.0 and w in (1.0, 26214 / 65535.0)
        num += w * e
        den += w
    assert eq == pytest.approx(num / den, abs=1e-12)
    assert set(classes) == {"AKS", "A5S", "QQ"}
    assert sum(w for _, w in classes.values()) == pytest.approx(den, abs=1e-12)
    assert classes["A5S"][1] == pytest.approx(4 * 26214 / 65535.0, abs=1e-15) and classes["QQ"][1] == 6.0


def test_single_hand_against_a_single_hand_is_the_known_hand_enumeration(eng):
    h, g = ("AH", "KH"), ("QC", "QD")
    for ties in ("credited", "split"):
        eq, hands = mh.get_preflop_range_equity_exact_weighted({h: 1.0}, {g: 0.3}, engine=eng, ties=ties)
        want, _ = mh.get_equity_exact(list(h), [], 2, "uniform", eng, known_hands=[list(g)], ties=ties)
        assert list(hands) == [tuple(sorted(h, key=npa.card_id))] and eq == pytest.approx(want, abs=1e-15)
        assert hands[list(hands)[0]] == (eq, 1.0)
