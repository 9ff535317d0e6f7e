"""Test helper: the cases of the WEIGHTED preflop hero-range exact enumeration (mcq_exact_batch_hero_range_preflop_weighted)
and an independent ground truth on slices of the completions.

A case is a tests/hero_preflop_cases.py case (hero classes, opponent classes, no table cards, ghost cards) with two weight
tables beside it, made by the table makers of tests/weighted_range_cases.py: opp[1326] and hero[1326] (or None) of uint16,
indexed by hand_index(a, b).  The class sets stay in force.

literal_slice(case, opp, hero, lo, hi) walks the definition directly on the completions [lo, hi) in mcq_exact_unrank's order
(PC.unrank): per completion T every hand of D minus T is scored by the oracle's evaluator (oracle.score_batch) and eff_opp(g)
goes to win / tie / runs / by_type of every allowed hero hand h of D minus T for the g that share no card with h.  Exact
Python ints; none of the library's lane code is involved.
"""
import numpy as np

from neuron_poker_amd import _lib
from oracle import oracle as O
from tests import hero_preflop_cases as PC
from tests import hero_range_cases as HC
from tests import weighted_range_cases as WC

ROWS = WC.ROWS
WMAX = WC.WMAX
HANDS = WC.HANDS
ALL = None                                     # every class
AA_KK = {"AA", "KK"}

# name -> (case of tests/hero_preflop_cases.py, opponent table, hero table or None)
WPCASES = {
    # the host test's slices: 22 (52 cards) / 15 (50 cards) hero hands before the table zeroes some; 17 opponent classes
    "host_52": (PC.case(PC.HOST_HERO, PC.TOP10, 52), WC.hand_level(41), WC.hero_table(42)),
    "host_50": (PC.case(PC.HOST_HERO, PC.TOP10, 50), WC.hand_level(41), WC.hero_table(42)),
    # the GPU test's whole enumerations: 10 (52 cards) / 3 (50 cards) hero hands before the table zeroes some
    "narrow_3cls_52": (PC.case(PC.NARROW_HERO, PC.OPP_3CLS, 52), WC.hand_level(43), WC.hero_table(46)),
    "narrow_3cls_50": (PC.case(PC.NARROW_HERO, PC.OPP_3CLS, 50), WC.hand_level(43), WC.hero_table(46)),
    "narrow_top10_52": (PC.case(PC.NARROW_HERO, PC.TOP10, 52), WC.hand_level(45), WC.hero_table(46)),
    "narrow_top10_50": (PC.case(PC.NARROW_HERO, PC.TOP10, 50), WC.hand_level(45), WC.hero_table(46)),
}


def holed_hero(seed):
    """A hero table that zeroes about a fifth of the hands; the others weigh 1, 2 or 9."""
    g = np.random.default_rng(seed)
    return g.choice(np.array([0, 1, 1, 2, 9], np.uint16), ROWS).astype(np.uint16)


# every class with holes against {AA, KK} hand-level: more than 1024 allowed hands whose list position is not their row
WPCASES["holed_52"] = (PC.case(ALL, AA_KK, 52), WC.hand_level(47), holed_hero(48))
for _w in WPCASES.values():
    for _t in _w[1:]:
        if _t is not None:
            _t.setflags(write=False)


def effective(name):
    """-> (eff_opp[1326], eff_hero[1326]) of a case as Python-int arrays (WC.effective)."""
    c, ow, hw = WPCASES[name]
    return WC.effective(c, ow, hw)


def allowed_hands(name):
    """The hero hands of positive effective weight, in ascending row order (= the order of the kernel's `allowed` list)."""
    eff_h = effective(name)[1]
    return [HANDS[i] for i in np.flatnonzero(eff_h)]


def disjoint_opponent(eff_o, h):
    """Is an opponent hand of positive weight left that shares no card with h?"""
    return any(not (set(HANDS[i]) & set(h)) for i in np.flatnonzero(eff_o))


def _class_in(bits, c):
    return bits is None or (int(bits[c >> 5]) >> (c & 31)) & 1


for _name, (_c, _ow, _hw) in WPCASES.items():
    _eo, _eh = WC.effective(_c, _ow, _hw)
    _ob, _hb = HC.parts(_c)[1], HC.parts(_c)[0]
    # the opponent's table has both zero and non-zero hands inside at least one of the opponent's classes ...
    assert any(_class_in(_ob, k) for k in WC.split_classes(_ow)), _name
    # ... the hero's table leaves some hands of the hero's classes in and some out ...
    _in_class = [h for h in HC.allowed_hands(_c)]
    assert 0 < int((_eh != 0).sum()) < len(_in_class), (_name, int((_eh != 0).sum()), len(_in_class))
    # ... and every allowed hero hand has a disjoint opponent hand of positive weight
    assert all(disjoint_opponent(_eo, HANDS[i]) for i in np.flatnonzero(_eh)), _name
assert int((effective("holed_52")[1] != 0).sum()) > 1024


def records(name):
    """-> (mcq_query, mcq_query_ext, opp[1, 1326], hero[1, 1326] or None) of a case."""
    c, ow, hw = WPCASES[name]
    q, x = HC.records(c)
    return q, x, ow.reshape(1, ROWS), None if hw is None else hw.reshape(1, ROWS)


def literal_slice(case, opp, hero, lo, hi, only=None):
    """-> {hand: [runs, win, tie, by_type[9]] as Python ints}: the part of every allowed hero hand's row that the
    completions [lo, hi) give.  only: walk just these hero hands."""
    eff_o, eff_h = WC.effective(case, opp, hero)
    d = HC.deck(case)
    L = len(d)
    pairs = np.array([(a, b) for b in d for a in d if a < b], np.int64)              # every hand of D
    wt_all = eff_o[pairs[:, 1] * (pairs[:, 1] - 1) // 2 + pairs[:, 0]].astype(np.int64)
    allowed = [h for h in (tuple(int(v) for v in p) for p in pairs) if eff_h[_lib.hand_index(*h)] > 0]
    if only is not None:
        allowed = [h for h in allowed if h in only]
    at = {tuple(int(v) for v in p): i for i, p in enumerate(pairs)}
    own = np.array([at[h] for h in allowed])
    ha, hb = np.array([h[0] for h in allowed])[:, None], np.array([h[1] for h in allowed])[:, None]
    free = (pairs[None, :, 0] != ha) & (pairs[None, :, 0] != hb) & (pairs[None, :, 1] != ha) & (pairs[None, :, 1] != hb)
    sums = np.zeros((len(allowed), 12), object)
    sums[:] = 0
    chunk = 64
    for c0 in range(lo, hi, chunk):
        idx = range(c0, min(hi, c0 + chunk))
        tables = [[d[p] for p in PC.unrank(i, L, 5)] for i in idx]
        keep = [~np.isin(pairs, T).any(axis=1) for T in tables]                      # the hands of D minus T
        seven = np.concatenate([np.concatenate([pairs[k], np.tile(np.array(T, np.int64), (int(k.sum()), 1))], axis=1)
                                for T, k in zip(tables, keep)])
        score_all = O.score_batch(seven.astype(np.uint8), threads=8)
        at0 = 0
        for T, k in zip(tables, keep):
            n = int(k.sum())
            score = np.zeros(len(pairs), np.uint64)
            score[k] = score_all[at0:at0 + n]
            at0 += n
            here = k[own]                                                           # the hero hands that T leaves alone
            if not here.any():
                continue
            sh = score[own][:, None]
            w = np.where(free & k[None, :], wt_all[None, :], 0)                     # [hero hand, opponent hand]
            win = np.where(score[None, :] < sh, w, 0).sum(axis=1)
            tie = np.where(score[None, :] == sh, w, 0).sum(axis=1)
            tot = w.sum(axis=1)
            typ = (score[own] >> np.uint64(32)).astype(np.int64)
            for i in np.flatnonzero(here):
                s = sums[i]
                s[0] += int(tot[i])
                s[1] += int(win[i])
                s[2] += int(tie[i])
                s[3 + int(typ[i])] += int(win[i]) + int(tie[i])
    return {h: [int(v) for v in sums[i]] for i, h in enumerate(allowed)}


row_ints = WC.row_ints
