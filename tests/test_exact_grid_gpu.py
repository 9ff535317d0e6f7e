"""The exact-enumeration kernels against the grid of tests/exact_grid.py, with MCQ_EXACT_CU capping the CU
count the plans see: at 1 and 3 a wave of mcq_exact_kernel<false|true> and of mcq_exact_ext_kernel<1, *>, a block of
<2, plain> and (preflop, or alone on a flop) a lane of <0, *> own several table completions on records whose rows the host
builds of the lane code give and tests/test_exact_grid_host.py pins to the literal walks -- which plans do that is asserted
there, without a GPU (test_capped_plans_give_every_owner_several_completions).  Every row is compared bit for bit."""
import numpy as np
import pytest

import neuron_poker_amd as npa
from tests import exact_grid as G
from tests.seats_expect import check_invariants

pytestmark = pytest.mark.gpu
CAPS = (1, 3, None)


def _engine(monkeypatch, cap):
    """A fresh engine that reads MCQ_EXACT_CU=cap at creation (None: the switch unset)."""
    if cap is None:
        monkeypatch.delenv("MCQ_EXACT_CU", raising=False)
    else:
        monkeypatch.setenv("MCQ_EXACT_CU", str(cap))
    return npa.Engine(0)


def _u64(rows, words):
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1, words)


def _call(eng, entry, recs, law):
    """-> (weight rows [n, words] uint64, prob bytes per record or None)."""
    q, e = G.pack(recs)
    if entry == "exact":
        return _u64(eng.exact(q, law), 13), None
    if entry == "ext":
        prob, w = eng.exact_ext(q, e, law)
        return _u64(w, 13), prob.view(np.float64).reshape(-1, 11)
    if entry == "ways":
        prob, w = eng.exact_ext_ways(q, e, law)
        return _u64(w, 22), prob.view(np.float64).reshape(-1, 20)
    fn = eng.exact_seats if entry == "seats" else eng.exact_ext_seats
    return _u64(fn(q, e, law), 32), None


def _check_prob(entry, recs, law, rows, prob):
    """The probabilities are the host build's, byte for byte (ways: p, then tie_ways = weights / runs)."""
    if prob is None:
        return
    for i, r in enumerate(recs):
        assert prob[i, :11].tobytes() == G.plain_row(r, law)[0].tobytes(), (entry, r, law)
        if entry == "ways":
            assert prob[i, 11:].tobytes() == (rows[i, 13:].astype(np.float64) / np.float64(rows[i, 0])).tobytes(), (r, law)


@pytest.mark.parametrize("law", G.LAWS)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("entry", list(G.WORDS))
def test_whole_grid_in_one_call_twice_then_each_record_alone(monkeypatch, entry, cap, law):
    """(a) one call per entry point, kinds interleaved, two jobs of kind 2 and more in it (a non-zero h1_off): weights and
    probabilities equal the host rows bit for bit; (b) the same call again on the same engine: identical (the row buffer
    and the per-first-hand sums are zeroed per call); (c) every record alone (max_grid of a one-job launch).
    Wall time on an MI355X: 0.14 to 1.2 s a case; 5.7 to 8.9 s for the first case of a law in a session (ext, cap 1), which
    also walks the grid's host rows, cached for every later case."""
    eng = _engine(monkeypatch, cap)
    try:
        recs = G.batch(entry)
        want = G.expect(entry, recs, law)
        rows, prob = _call(eng, entry, recs, law)
        bad = [r.name for i, r in enumerate(recs) if not (rows[i] == want[i]).all()]
        assert not bad, (entry, cap, law, bad)
        _check_prob(entry, recs, law, rows, prob)
        rows2, prob2 = _call(eng, entry, recs, law)
        assert rows2.tobytes() == rows.tobytes() and (prob is None or prob2.tobytes() == prob.tobytes())
        for i, r in enumerate(recs):
            one, p1 = _call(eng, entry, [r], law)
            assert (one[0] == want[i]).all(), (entry, cap, law, r)
            assert prob is None or p1.tobytes() == prob[i:i + 1].tobytes(), (entry, cap, law, r)
    finally:
        eng.close()


@pytest.mark.parametrize("law", G.LAWS)
@pytest.mark.parametrize("cap", CAPS)
def test_cross_entry_identities(monkeypatch, cap, law):
    """(d) include/mcq.h: seat 0 of the per-seat rows carries the split-pot weights; a record that restricts nothing gives
    the row of `exact`; exact_ext_seats equals exact_seats on all-in records; the shares add up to 2520 x runs.
    Wall time on an MI355X: 0.15 s (unset) to 0.52 s (cap 1) a case."""
    eng = _engine(monkeypatch, cap)
    try:
        got = {en: dict(zip([r.name for r in G.batch(en)], _call(eng, en, G.batch(en), law)[0])) for en in G.WORDS}
    finally:
        eng.close()
    n = 0
    for r in G.grid():
        if "ways" in r.entries:
            ways, seats = got["ways"][r.name], got["ext_seats"][r.name]
            assert (ways[:13] == got["ext"][r.name]).all(), r
            assert seats[0] == ways[0] and (seats[2:4] == ways[2:4]).all(), r
            share = G.UNIT * int(ways[2]) + sum((G.UNIT // k) * int(ways[13 + k - 2]) for k in range(2, 11))
            assert int(seats[4]) == share, r
            check_invariants(seats, r.n_players)
            n += 1
        if "exact" in r.entries:
            assert (got["exact"][r.name] == got["ext"][r.name]).all(), r
        if "seats" in r.entries:
            assert (got["seats"][r.name] == got["ext_seats"][r.name]).all(), r
            check_invariants(got["seats"][r.name], r.n_players)
    assert n >= 40


@pytest.mark.parametrize("law", G.LAWS)
@pytest.mark.parametrize("cap", (1, None))
def test_all_in_preflop_equals_the_plain_enumeration(monkeypatch, cap, law):
    """Kind 0 preflop, 2, 3 and 10 hands, against every C(L, 5) completion scored by oracle.score_batch (exact integers).
    At cap 1 one block walks them all: 1673 completions a lane with two hands, the bound the packed win/tie halves of
    <0, SEATS> were sized for.  Wall time on an MI355X: 1.0 s a case at cap 1, 0.14 s unset (the enumeration is cached)."""
    mine = [r for r in G.grid() if r.nb == 0]
    assert [r.n_known + 1 for r in mine] == [2, 3, 10] and (cap != 1 or G.busiest(mine[0], "ext", 1) == 1673)
    eng = _engine(monkeypatch, cap)
    try:
        rows = {en: _call(eng, en, mine, law)[0] for en in ("ext", "ways", "seats", "ext_seats")}
    finally:
        eng.close()
    for i, r in enumerate(mine):
        plain, ways, seats = G.enumerate_all_in(r, law)
        assert (rows["ext"][i] == plain).all() and (rows["ways"][i] == ways).all(), (r, cap, law)
        assert (rows["seats"][i] == seats).all() and (rows["ext_seats"][i] == seats).all(), (r, cap, law)


PARTITION_CAP = 32      # a wave of kind 1 owns 8 times the completions it owns on 256 CUs


@pytest.mark.parametrize("entry", ["exact", "ext", "ways", "ext_seats", "exact_three_flop"])
def test_partition_invariance_where_no_host_row_exists(monkeypatch, entry):
    """Heads-up preflop (C(50, 5) or C(46, 5) completions x 990 or 820 hands: no host walk) gives the same bits at the
    default and at MCQ_EXACT_CU = 32, under both laws; so does the three-player flop of `exact`, which the grid leaves out,
    at caps 1 and 3.  Integer atomics: any order of the same terms gives the same sums, so a difference is a wrong term.

    ext_seats runs unrestricted: a completion adds 2520 x its weight to the share words, so at cap 32 (512 waves, 2676
    completions each) the hero's share passes 2^32 in some wave, while on a device of 86 CUs and more no wave's can
    (asserted below) -- the wave's 64-bit sum, narrowed to 32 bits, would give other bits at the cap than at the default.
    Wall time on an MI355X: 0.41 s (exact); every other case below 2.4 s."""
    name = entry
    if entry == "exact_three_flop":
        recs, caps, entry = [G.Rec("three_flop", [48, 49], [0, 5, 10], 3)], (None, 1, 3), "exact"
    else:
        rng, ghost = {"exact": ("none", None), "ext_seats": ("none", G._ids(["2C", "2D"]))}.get(entry, ("top25", G._ids(["2C", "2D"])))
        recs, caps = [G.Rec("hu_preflop", G._ids(["AH", "KH"]), [], 2, (), ghost, rng)], (None, PARTITION_CAP)
    out = []
    for cap in caps:
        eng = _engine(monkeypatch, cap)
        try:
            out.append([_call(eng, entry, recs, law) for law in G.LAWS])
        finally:
            eng.close()
    for other in out[1:]:
        for (rows, prob), (rows0, prob0) in zip(other, out[0]):
            assert rows0[0, 0] > 0 and rows.tobytes() == rows0.tobytes()
            assert prob0 is None or prob.tobytes() == prob0.tobytes()
    if name == "ext_seats":
        n_boards, hands = G.binom(46, 5), G.binom(41, 2)
        for rows, _ in out[0]:      # the hero's share, spread over the cap's 512 waves, is above 2^32 a wave
            assert int(rows[0, 4]) // (PARTITION_CAP * 16) >= 1 << 32
        # a wave of an 86-CU device walks 996 completions, each adds 2520 x (2 x 820) at the most
        assert -(-n_boards // (86 * 16)) * G.UNIT * 2 * hands < 1 << 32
