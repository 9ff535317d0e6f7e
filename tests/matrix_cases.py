"""The named records of the hand-against-hand matrix tests (tests/test_matrix_*.py): boards on which ties are plentiful --
paired, and such that the board plays -- with their dead cards, the shape each one stands for, and what every test asserts
of a case before it trusts it: a tie somewhere and a hand that wins every completion somewhere."""
import numpy as np

from neuron_poker_amd import _lib
from neuron_poker_amd.cards import card_id

ROWS = _lib.HAND_ROWS


def C(*names):
    return [card_id(n) for n in names]


def _dead(board, n, seed):
    """n dead cards: a seeded draw from the cards that are not on the table"""
    rest = [c for c in range(52) if c not in board]
    return sorted(int(c) for c in np.random.RandomState(seed).permutation(rest)[:n])


def _all_but(board, keep):
    return [c for c in range(52) if c not in board and c not in keep]


_FLOP = C("KH", "KD", "7C")
_TINY = C("QS", "QH", "JS", "JH", "2C", "2D")     # the six cards left: QS JH and QH JS tie, the queens beat the jacks

# name -> (table cards, dead cards, hands of D, total)
CASES = {
    "river": (C("9C", "9D", "KH", "KS", "AC"), [], 1081, 1),
    "turn_dead2": (C("AS", "9D", "9H", "QC"), C("2C", "KD"), 1035, 42),
    "flop_dead20": (_FLOP, _dead(_FLOP, 20, 7), 406, 300),
    "flop_full": (C("AH", "KD", "7C"), [], 1176, 990),
    "flop_tiny": (C("AH", "KD", "7C"), _all_but(C("AH", "KD", "7C"), _TINY), 15, 1),
    "river_tiny": (C("AH", "KD", "7C", "3C", "3D"), _all_but(C("AH", "KD", "7C", "3C", "3D"), _TINY), 15, 1),
}
REFUSED_SHORT = (C("AH", "KD", "7C"), _all_but(C("AH", "KD", "7C"), _TINY[:4]))     # 45 dead cards: L = 4, k = 2
HOST_CASES = ["river", "turn_dead2", "flop_dead20", "flop_tiny", "river_tiny"]   # (flop_full: the GPU's cross-checks)
BATCH = ["river", "turn_dead2", "flop_dead20", "flop_tiny", "river_tiny"]


def record(name):
    board, dead = CASES[name][:2]
    return _lib.pack_matrix_query(board, dead)


def records(names):
    return np.concatenate([record(n) for n in names])


def deck(name):
    """D: the card ids that are neither on the table nor dead, ascending"""
    board, dead = CASES[name][:2]
    return [c for c in range(52) if c not in board and c not in dead]


def hands(name):
    """the two-card hands of D as (a < b), in the order of their hand_index"""
    d = deck(name)
    return sorted(((a, b) for i, a in enumerate(d) for b in d[i + 1:]), key=lambda h: _lib.hand_index(*h))


def meet_mask(name):
    """bool [1326, 1326]: the two hands lie in D and share no card"""
    hs = np.array(hands(name))
    idx = np.array([_lib.hand_index(a, b) for a, b in hs])
    apart = ((hs[:, None, 0] != hs[None, :, 0]) & (hs[:, None, 0] != hs[None, :, 1]) &
             (hs[:, None, 1] != hs[None, :, 0]) & (hs[:, None, 1] != hs[None, :, 1]))
    m = np.zeros((ROWS, ROWS), bool)
    m[np.ix_(idx, idx)] = apart
    return m


def check_shape(name, win, tie, total):
    """What every test asserts of its case: the shape it stands for, a tie somewhere, a hand that wins every completion."""
    n_hands, want_total = CASES[name][2:]
    assert len(hands(name)) == n_hands and total == want_total, (name, len(hands(name)), total)
    assert (tie > 0).any() and (win == total).any(), name


def check_structure(name, win, tie, total):
    """win + win.T + tie == total exactly on the pairs that can meet, zero elsewhere, tie symmetric."""
    m = meet_mask(name)
    w = win.astype(np.uint32)
    s = w + w.T + tie
    assert (s[m] == total).all() and not s[~m].any(), name
    assert not win[~m].any() and not tie[~m].any() and np.array_equal(tie, tie.T), name


_host = {}


def host(name):
    """The host build's (win, tie, total) of a case (tests/hostsim_matrix), computed once and left unchanged."""
    if name not in _host:
        from tests import hostsim_matrix as HM
        win, tie, total = HM.matrix(record(name))
        win.setflags(write=False)
        tie.setflags(write=False)
        _host[name] = (win, tie, total)
    return _host[name]
