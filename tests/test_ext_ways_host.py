"""Split-pot rows of EXTENDED queries, without a GPU: the lane code (mcq_iteration_ext / mcq_iteration_ext_fast with
McqLaneAccWays, the exact enumeration's per-k weights) compiled for the host and pinned by the checks listed in
tests/ext_ways_cases.py; the ABI and the layout of the new entries."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import neuron_poker_amd as npa
from neuron_poker_amd import _lib
from oracle import oracle as O
from tests import ext_ways_cases as XC
from tests import exact_ways_literal as XL
from tests import hostsim_ext_ways as H
from tests import hostsim_ways as HW
from tests import ways_expect as WE

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
RUNS = 1024


@pytest.mark.parametrize("replay", [False, True], ids=["ctr", "replay"])
@pytest.mark.parametrize("i", range(len(XC.CASES)), ids=[c["name"] for c in XC.CASES])
def test_recount(i, replay):
    """The row's ways are what the dealt hands say under the oracle's comparison; words 0..12 are the oracle's."""
    case = XC.CASES[i]
    q, ext = XC.records(case, RUNS)
    seed = (XC.SEED + XC.QID) & 0xFFFFFFFF if replay else XC.SEED
    row, hands = H.run(replay, q, ext, seed, 0 if replay else XC.QID, hands=True)
    assert (hands != 255).all()
    ways, win, tie = XC.recount(hands, case["n"])
    assert np.array_equal(row[13:22], ways), (row[13:22], ways)
    assert (int(row[2]), int(row[3])) == (win, tie)
    assert np.array_equal(row[:13], XC.oracle_tallies(O.MODE_MT if replay else O.MODE_CTR, case, RUNS))
    assert int(row[13:22].sum()) == int(row[3]) and not row[13 + case["n"] - 1:22].any()


def test_undealable_range_is_refused():
    q, ext = XC.records(XC.UNDEALABLE, 64)
    with pytest.raises(ValueError):
        H.run(False, q, ext, XC.SEED, XC.QID)


def test_cases_vary():
    XC.assert_cases_vary([XC.hostsim_row(i, RUNS, False) for i in range(len(XC.CASES))])


def test_fast_form_equals_general_form():
    n_fast = 0
    for i, case in enumerate(XC.CASES):
        q, ext = XC.records(case, RUNS)
        if not H.is_fast(q, ext):
            continue
        n_fast += 1
        assert np.array_equal(XC.hostsim_row(i, RUNS, False), XC.hostsim_row(i, RUNS, False, general=True)), case["name"]
    assert n_fast >= 2
    # ... and with every opponent count the unrolled form has
    for n in range(2, 11):
        q = npa.pack_queries([[npa.card_id("AC"), npa.card_id("QD")]], [[npa.card_id("AD"), npa.card_id("AH"), 255, 255, 255]], n, 300)
        ext = npa.pack_query_ext(1, opp_range=npa.range_bits(XC.top_classes(0.5)))
        assert H.is_fast(q, ext)
        assert np.array_equal(H.run(False, q, ext, 3, 9), H.run(False, q, ext, 3, 9, general=True)), n


@pytest.mark.parametrize("mode", [O.MODE_CTR, O.MODE_MT], ids=["ctr", "replay"])
def test_nothing_restricted_is_the_plain_row(mode):
    """An extension record that restricts nothing gives tests/hostsim_ways's row bit for bit."""
    for hero, board, n in WE.CASES:
        q = WE.query(hero, board, n, 700)
        ext = npa.pack_query_ext(1)
        replay = mode == O.MODE_MT
        got = H.run(replay, q, ext, (WE.SEED + WE.QID) & 0xFFFFFFFF if replay else WE.SEED, 0 if replay else WE.QID)
        assert np.array_equal(got, HW.run(mode, q, WE.SEED, WE.QID)), (hero, board, n)


def _ids(cards):
    return [npa.card_id(c) for c in cards]


# small exact cases: river and turn boards; (hero, board, n_players, known, ghost, opponents' classes)
EXACT_SMALL = [
    (["2C", "3D"], ["TS", "JS", "QS", "KS", "AS"], 4, [["4H", "5D"], ["9C", "9D"], ["AH", "AD"]], None, None),
    (["AH", "KD"], ["2C", "7D", "9H", "JS"], 3, [["AS", "KC"], ["AD", "KH"]], None, None),
    (["AH", "KD"], ["2C", "7D", "9H", "JS", "3S"], 3, [["AS", "KC"]], None, ["AKO", "AKS", "QQ"]),
    (["AC", "QD"], ["AD", "AH", "KS", "4C"], 2, [], None, ["AQO", "AQS", "AKO"]),
    (["2C", "3D"], ["KC", "KD", "KH", "KS"], 3, [["4H", "5D"]], ["AS", "AD"], None),
    (["AC", "QD"], ["AD", "AH", "KS", "4C"], 4, [["AS", "QC"], ["QH", "QS"]], None, ["AQO", "AQS", "AKO", "72O"]),
]


def exact_records(case):
    hero, board, n, known, ghost, opp = case
    b = _ids(board)
    q = npa.pack_queries([_ids(hero)], [b + [255] * (5 - len(b))], n, 1)
    ext = npa.pack_query_ext(1, ghost=_ids(ghost) if ghost else None, known=[_ids(h) for h in known],
                             opp_range=npa.range_bits(opp) if opp is not None else None)
    return q, ext


@pytest.mark.parametrize("law", [0, 1], ids=["reference", "uniform"])
@pytest.mark.parametrize("ci", range(len(EXACT_SMALL)))
def test_exact_weights_against_the_literal_walk(ci, law):
    case = EXACT_SMALL[ci]
    hero, board, n, known, ghost, opp = case
    q, ext = exact_records(case)
    w = H.exact(q, ext, law)
    win, ties = XL.exact_ways(_ids(hero), _ids(board), n, [_ids(h) for h in known], _ids(ghost) if ghost else None,
                              npa.range_bits(opp) if opp is not None else None, uniform=bool(law))
    tot = int(w[0])
    assert Fraction(int(w[2]), tot) == win
    assert [Fraction(int(x), tot) for x in w[13:22]] == ties
    assert int(w[13:22].sum()) == int(w[3])
    assert sum(1 for t in ties if t) >= 1
    # words 0..12: the credited enumeration's weights
    from tests import hostsim_exact_ext as HX
    assert np.array_equal(HX.exact_ext(q, ext, uniform=bool(law))[1], w[:13])


def test_exact_literal_walk_sees_three_way_ties():
    """The small cases hold ties among three and four hands, not only two."""
    ks = set()
    for case in EXACT_SMALL:
        q, ext = exact_records(case)
        w = H.exact(q, ext, 0)
        ks |= {k + 2 for k in range(9) if w[13 + k]}
    assert {2, 3, 4} <= ks, ks


def test_exact_two_random_opponents_refused_by_host_build():
    q = npa.pack_queries([_ids(["AH", "KD"])], [_ids(["2C", "7D", "9H", "JS", "3S"])], 3, 1)
    with pytest.raises(ValueError):
        H.exact(q, npa.pack_query_ext(1), 0)


def test_pot_share_exact_rows():
    rows = np.zeros((1, 22), np.uint64)
    rows[0, 0], rows[0, 2], rows[0, 3], rows[0, 13], rows[0, 14] = 12, 3, 5, 2, 3
    assert _lib.pot_share(rows, exact=True) == [Fraction(3 + 1 + 1, 12)]
    assert _lib.pot_share(rows)[0] == pytest.approx(5 / 12)


def test_bad_ties_value_raises_before_the_gpu():
    from neuron_poker_amd import montecarlo_hip as mh
    with pytest.raises(ValueError):
        mh.MonteCarlo(engine=object()).run_montecarlo([["AH", "KD"]], [], 2, 1, maxRuns=10, timeout=0, ghost_cards="", ties="half")
    with pytest.raises(ValueError):
        mh.get_equity_exact(["AH", "KD"], [], 2, engine=object(), ties="half")


def test_abi_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mcq.h")).read()
    lib = npa.load_library()
    for name in ("mcq_eval_batch_ext_ways", "mcq_exact_batch_ext_ways"):
        assert "MCQ_API int %s(" % name in hdr
        assert hasattr(lib, name)
    assert "Extended queries, the exact enumerations and mcq_multi_* have no split-pot form" not in hdr


def test_exact_prob_ways_layout(tmp_path):
    assert _lib.EXACT_PROB_WAYS_DTYPE.itemsize == 160
    assert _lib.EXACT_PROB_WAYS_DTYPE.fields["tie_ways"][1] == 88
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "mcq.h"\n'
                   '_Static_assert(sizeof(mcq_exact_prob_ways) == 160, "size");\n'
                   '_Static_assert(offsetof(mcq_exact_prob_ways, tie_ways) == 88, "offset");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "layout.o")])
