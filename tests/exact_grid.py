"""The grid of EXACT-enumeration queries shared by tests/test_exact_grid_host.py and tests/test_exact_grid_gpu.py.

The exact kernels (mcq_exact_kernel<false|true>, mcq_exact_ext_kernel<0|1|2, plain|WAYS|SEATS>) size their grids by the
device's CU count, so on a large device a wave, lane or block owns more than one table completion only preflop, where
nothing bit-exact exists to compare with.  MCQ_EXACT_CU caps the CU count the plans see: with it the
code between two completions runs on flop, turn and river records, whose expected rows the host builds of the lane code
give (tests/hostsim, hostsim_exact_ext, hostsim_ext_ways, hostsim_seats, hostsim_exact_seats) and the host file pins to
the literal walks.  No GPU is needed to import this file.

KIND = the number of random opponents (0: every hand known, 1, 2), as the kernels' template argument.  Entry points:

    exact      Engine.exact            13 words   records that restrict nothing, 1 to 3 players
    ext        Engine.exact_ext        13 words   kinds 0, 1, 2 (+ mcq_exact_prob)
    ways       Engine.exact_ext_ways   22 words   kinds 0, 1
    seats      Engine.exact_seats      32 words   kind 0, two hands at least
    ext_seats  Engine.exact_ext_seats  32 words   kinds 0 (two hands at least), 1

Every record is run under both laws.  How a record is held to something independent of the lane code (Rec.literal):
    "walk"    tests/exact_literal.py, exact_ways_literal.py, exact_seats_literal.py in fractions
    "oracle"  oracle.exact (a record of kind 2 that restricts nothing: win and tie; a walk in fractions is half a minute on
              the river and half an hour on the turn)
    "numpy"   enumerate() below: every completion scored by oracle.score_batch (kind 0 preflop)
    None      the host build alone (flop records and what the literal walks take minutes for)
"""
import itertools
import json
import os

import numpy as np

from neuron_poker_amd import _lib
from neuron_poker_amd.cards import card_id
from oracle import oracle as O

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GEN_SEED = 20261018
LAWS = ("reference", "uniform")
STREETS = (3, 4, 5)
UNIT = 2520
with open(os.path.join(_ROOT, "neuron_poker_amd", "preflop_classes.json")) as _f:
    CLASSES = json.load(_f)
assert len(CLASSES) == 169

RANGES = {
    "none": None,                                                        # the packer's default: every class
    "top25": _lib.range_bits(CLASSES[-int(169 * 0.25):]),
    "pairs_ak": _lib.range_bits({"AA", "KK", "AKS", "AKO", "QQ"}),       # neighbour pairs (AcAd, ...)
    "one": _lib.range_bits({"T9O"}),                                     # one class, twelve hands
    "fat168": _lib.range_bits([c for c in CLASSES if c != "72O"]),
    "all169": _lib.range_bits(CLASSES),                                  # every class, spelt out
}
assert (RANGES["all169"] == _lib.ALL_CLASSES).all()
NARROW = ("top25", "pairs_ak", "one")
KNOWN_COUNTS = {0: (0, 1, 2, 5, 9), 1: (0, 1, 2, 5), 2: (0, 1, 2, 5)}    # 9: ten hands all-in


class Rec:
    """One exact query: cards as ids, the packed records, the kernels' KIND and what holds it (literal)."""

    def __init__(self, name, hero, board, n_players, known=(), ghost=None, rng="none", literal=None, tags=()):
        self.name, self.hero, self.board, self.n_players = name, list(hero), list(board), n_players
        self.known, self.ghost, self.rng = [list(h) for h in known], list(ghost) if ghost else None, rng
        self.literal, self.tags = literal, set(tags)
        self.nb, self.n_known = len(board), len(self.known)
        self.kind = n_players - 1 - self.n_known
        assert 0 <= self.kind <= 2
        self.q = _lib.pack_query_one(self.hero, self.board, n_players, 1)
        self.e = _lib.pack_query_ext(1, ghost=self.ghost, known=self.known, opp_range=RANGES[rng])
        self.L = 52 - self.nb - 2 - 2 * self.n_known - (2 if self.ghost else 0)       # cards left to deal from
        self.restricted_range = rng not in ("none", "all169")          # kind 2: no common total, no integer weights
        self.restricted = bool(self.known or self.ghost or self.restricted_range)

    @property
    def entries(self):
        out = ["ext"]
        if not self.restricted and not (self.kind == 2 and self.nb == 3):
            out.append("exact")
        if self.kind <= 1 and self.n_players >= 2:
            out += ["ways", "ext_seats"]
        if self.kind == 0 and self.n_players >= 2:
            out.append("seats")
        return out

    @property
    def hands(self):
        return [self.hero] + self.known

    def deck(self):
        gone = set(self.board) | set(self.ghost or []) | {c for h in self.hands for c in h}
        return [c for c in range(52) if c not in gone]

    def __repr__(self):
        return "Rec(%s: kind %d, %d table cards, %d known, %s%s)" % (self.name, self.kind, self.nb, self.n_known, self.rng,
                                                                   ", ghost" if self.ghost else "")


def _ids(cards):
    return [card_id(c) for c in cards]


def _literal_rule(kind, nb, n_known, rng, ghost):
    """What the literal walks finish in about a second: every river and turn record of kinds 0 and 1; of kind 2 the narrow
    set ranges (a top-25 % turn is 44 rivers of 1.7 s) and, through the oracle, what restricts nothing."""
    if nb == 3:
        return None
    if kind <= 1:
        return "walk"
    if rng in ("pairs_ak", "one") or (rng == "top25" and nb == 5):
        return "walk"
    if rng in ("none", "all169") and not n_known and not ghost:   # (river: 2 s; turn: about a minute a law)
        return "oracle"
    return None


def dealable(rec):
    """Can the reference deal the record's random opponents?  Every stage needs one accepted draw at least, after every hand
    the stage before it can deal (exact_literal._opponent, both laws) -- what mcq_exact_ext_dealable decides in the library.
    Only the narrow ranges are walked: a quarter of the classes and more cannot run dry on a deck of 31 cards and more."""
    from tests.exact_literal import _opponent, bits_to_set
    allowed = bits_to_set(RANGES[rec.rng])
    if rec.kind == 0 or allowed is None or len(allowed) > 40:
        return True
    deck = rec.deck()
    for uniform in (False, True):
        w1, n1 = _opponent(deck, allowed, uniform)
        if not n1 or (rec.kind == 2 and not all(_opponent([c for c in deck if c not in h1], allowed, uniform)[1] for h1 in w1)):
            return False
    return True


def make(name, kind, nb, n_known, rng, ghost, gen, literal="rule", tags=(), force=None):
    """A record with cards drawn by `gen`; a range that cannot be dealt from what is left is drawn again (no host build is
    walked here: importing the grid stays cheap).  force: cards a part must hold -- {"hero" | "known" | "ghost" | "board":
    [ids]} ("known": the last known hand)."""
    force = force or {}
    fixed = {c for v in force.values() for c in v}
    for _ in range(100):
        deck = [int(c) for c in gen.permutation(52) if int(c) not in fixed]

        def take(n, part=None):
            first = list(force.get(part, []))
            return first + [deck.pop() for _ in range(n - len(first))]
        known = [take(2, "known" if i == n_known - 1 else None) for i in range(n_known)]
        r = Rec(name, take(2, "hero"), take(nb, "board"), 1 + n_known + kind, known, take(2, "ghost") if ghost else None, rng,
                _literal_rule(kind, nb, n_known, rng, ghost) if literal == "rule" else literal, tags)
        if dealable(r):
            return r
    raise AssertionError(name)


_grid = None


def grid():
    """The records in canonical order."""
    global _grid
    if _grid is not None:
        return _grid
    from tests import exact_seats_cases as SC
    from tests import seats_expect as SE
    gen = np.random.default_rng(GEN_SEED)
    recs = []
    # -- the systematic part: kind x street x known hands, ranges and ghost cards in turn
    wide = ("none", "top25", "fat168", "pairs_ak", "all169", "one")
    turn = 0
    for kind in (0, 1, 2):
        for nb in STREETS:
            for n_known in KNOWN_COUNTS[kind]:
                flop2 = kind == 2 and nb == 3                             # walked with a narrow range (see assert_grid),
                for rep in range(1 if kind == 0 or flop2 else 2):       # once: four seconds on the host each
                    rng = "none" if kind == 0 else wide[turn % len(wide)]
                    ghost = bool((turn // 2 + rep) & 1) and 52 - nb - 2 * (1 + n_known + kind) >= 8
                    if flop2:
                        rng, ghost = {0: ("pairs_ak", False), 1: ("one", False), 2: ("pairs_ak", True), 5: ("top25", False)}[n_known]
                    recs.append(make("g%d_%d_%d_%d" % (kind, nb, n_known, rep), kind, nb, n_known, rng, ghost, gen))
                    turn += 1
    # -- records that restrict nothing: what `exact` takes, and exact_ext must give the same row
    for kind in (0, 1, 2):
        for nb in STREETS:
            if (kind, nb) != (2, 3) and (kind, nb) != (0, 3):
                recs.append(make("plain_%d_%d" % (kind, nb), kind, nb, 0, ("none", "all169")[(kind + nb) & 1], False, gen))
    # -- two random opponents with INTEGER weights (no range) and a literal walk in fractions: seven known hands and ghost
    #    cards leave the smallest deck there is, 31 cards on the river (3 s a law) and 30 on the turn (45 s a law)
    for nb in (5, 4):
        recs.append(make("int2_%d" % nb, 2, nb, 7, "none", True, gen, literal="walk", tags=("int2",)))
    recs.append(make("g0_3_lone_flop", 0, 3, 0, "none", False, gen))            # C(47, 2) = 1081 > 1024: a lane sees two
    # -- the reference law's top-of-deck rule ("a table card is never the highest card left"), every record literally walked
    t = 0
    for kind in (0, 1, 2):
        rng = {0: "none", 1: "top25", 2: "pairs_ak"}[kind]
        for what in ("hero51", "known51", "ghost51", "table51", "no51_50"):
            # a table card must still be dealt where the rule is about table cards alone: kind 0, and 51 on the table
            nb = 4 if what == "table51" or kind == 0 else (4, 5)[t & 1]
            t += 1
            force = {"hero51": {"hero": [51]}, "known51": {"known": [51]}, "ghost51": {"ghost": [51]}, "table51": {"board": [51]},
                     "no51_50": {"ghost": [50, 51]}}[what]
            r = make("top_%s_k%d" % (what, kind), kind, nb, 2 if what == "known51" or kind == 0 else t % 2, rng,
                     what in ("ghost51", "no51_50"), gen, literal="walk", tags=("top", what), force=force)
            recs.append(r)
    # -- tie structure: the board plays for ten seats, three level seats, an opponent that can level with the known hands
    for name, case in zip(SC.SMALL_IDS, SC.SMALL):
        if name in ("three_level", "ten_way", "royal_open"):
            hands, board, ghost, opp = case
            key = "seat_" + name
            RANGES[key] = _lib.range_bits(opp) if opp is not None else None
            recs.append(Rec("tie_" + name, _ids(hands[0]), _ids(board), len(hands) + 1, [_ids(h) for h in hands[1:]],
                            _ids(ghost) if ghost else None, key, "walk", ("tie", name)))
    hands, board, ghost = SE.EXACT_SMALL[5]
    recs.append(Rec("tie_ten_way_all_in", _ids(hands[0]), _ids(board), 10, [_ids(h) for h in hands[1:]], None, "none", "walk",
                    ("tie", "ten_way_all_in")))
    hands, board, ghost = SE.EXACT_SMALL[6]
    recs.append(Rec("tie_three_level_all_in", _ids(hands[0]), _ids(board), 10, [_ids(h) for h in hands[1:]], None, "none",
                    "walk", ("tie", "three_level_all_in")))
    # -- preflop, kind 0 only (the host walk of the other kinds is hours): 2, 3 and 10 hands against enumerate()
    for n_hands, ghost in ((2, False), (3, True), (10, False)):
        recs.append(make("pre_%d" % n_hands, 0, 0, n_hands - 1, "none", ghost, gen, literal="numpy", tags=("preflop",)))
    assert_grid(recs)
    _grid = recs
    return recs


def cells(recs):
    return {(en, r.kind, r.nb) for r in recs for en in r.entries}


CELLS = ({("ext", k, nb) for k in (0, 1, 2) for nb in STREETS} | {("ways", k, nb) for k in (0, 1) for nb in STREETS}
         | {("ext_seats", k, nb) for k in (0, 1) for nb in STREETS} | {("seats", 0, nb) for nb in STREETS}
         | {("exact", k, nb) for k in (0, 1, 2) for nb in STREETS if (k, nb) != (2, 3)}
         | {(en, 0, 0) for en in ("ext", "ways", "seats", "ext_seats")})


def assert_grid(recs):
    """No cell left out: every entry point at every shape it accepts, and what the grid leaves out on purpose.

    Two random opponents on the FLOP are walked with a restricted range only, and `exact` (which restricts nothing) has no
    flop record with two opponents: 1081 completions x 990 x 990 ordered pairs is too slow for the host walk that gives the
    expected row (tests/test_gpu_parity.py says the same).  Unrestricted kind 2 stays on turn and river.  The GPU file
    holds the three-player flop of `exact` to partition invariance instead.  Preflop is kind 0 only."""
    assert len({r.name for r in recs}) == len(recs)
    assert cells(recs) == CELLS, sorted(CELLS ^ cells(recs))
    for r in recs:
        if r.kind == 2 and r.nb == 3:
            assert r.rng in NARROW and "exact" not in r.entries, r
        if r.nb == 0:
            assert r.kind == 0 and r.literal == "numpy", r
    for kind in (0, 1, 2):
        mine = [r for r in recs if r.kind == kind and r.nb]
        for nb in STREETS:
            assert {r.n_known for r in mine if r.nb == nb} >= set(KNOWN_COUNTS[kind]), (kind, nb)
            assert {bool(r.ghost) for r in mine if r.nb == nb} == {False, True}, (kind, nb)
        if kind:
            assert {r.rng for r in mine} >= set(RANGES) - {k for k in RANGES if k.startswith("seat_")}, kind
            assert {r.rng for r in mine if r.nb == 3} >= set(NARROW), kind
        for what in ("hero51", "known51", "ghost51", "table51", "no51_50"):
            top = [r for r in mine if what in r.tags]
            assert top and all(r.literal == "walk" and (kind or r.nb < 5) for r in top), (kind, what)
    for r in recs:
        if "no51_50" in r.tags:
            assert sorted(r.ghost) == [50, 51] and max(r.deck()) <= 49, r
        if "ghost51" in r.tags:
            assert 51 in r.ghost and 51 not in r.deck()
    for nb in (4, 5):   # kind 2 with integer weights: a walked record with known hands and ghost cards, and what `exact` takes
        assert any("int2" in r.tags and r.nb == nb and r.literal == "walk" and r.known and r.ghost and not r.restricted_range
                   for r in recs)
        assert any("exact" in r.entries and r.kind == 2 and r.nb == nb and r.literal == "oracle" for r in recs)
    assert {r.n_known + 1 for r in recs if r.nb == 0} == {2, 3, 10}
    assert {n for r in recs if "tie" in r.tags for n in r.tags} >= {"ten_way", "three_level", "royal_open", "ten_way_all_in"}
    # at least two records of kind 2 travel in every batch (a non-zero h1_off), kinds interleaved (see batch())
    assert sum(1 for r in recs if r.kind == 2) >= 2


def batch(entry):
    """The records an entry point takes, kinds interleaved so that the host regroups rows and jobs."""
    mine = [r for r in grid() if entry in r.entries]
    by_kind = [[r for r in mine if r.kind == k] for k in (0, 1, 2)]
    out = [r for tup in itertools.zip_longest(*by_kind) for r in tup if r is not None]
    kinds = [r.kind for r in out]
    assert len(out) == len(mine) and (len(set(kinds)) == 1 or any(a > b for a, b in zip(kinds, kinds[1:])))
    return out


def pack(recs):
    return np.concatenate([r.q for r in recs]), np.concatenate([r.e for r in recs])


# ---- expected rows: the host builds of the lane code, one walk per (record, law), shared by both test files
_plain, _exact, _ways, _seats, _ext_seats = {}, {}, {}, {}, {}


def _cached(store, rec, law, fn):
    key = (rec.name, law)
    if key not in store:
        store[key] = fn()
    return store[key]


def plain_row(rec, law):
    """(prob [11] float64, weights [13]) of Engine.exact_ext."""
    from tests import hostsim_exact_ext as H
    return _cached(_plain, rec, law, lambda: H.exact_ext(rec.q, rec.e, law == "uniform"))


def exact_row(rec, law):
    from tests import hostsim as HS
    return _cached(_exact, rec, law, lambda: HS.exact(rec.q.view(np.uint8).reshape(16), law == "uniform"))


def ways_row(rec, law):
    from tests import hostsim_ext_ways as HW
    return _cached(_ways, rec, law, lambda: HW.exact(rec.q, rec.e, LAWS.index(law)))


def seats_row(rec, law):
    """The all-in build (tests/hostsim_seats)."""
    from tests import hostsim_seats as HS
    return _cached(_seats, rec, law, lambda: HS.exact(rec.q, rec.e, LAWS.index(law)))


def ext_seats_row(rec, law):
    """The build that walks one random opponent (tests/hostsim_exact_seats)."""
    from tests import hostsim_exact_seats as HX
    return _cached(_ext_seats, rec, law, lambda: HX.exact(rec.q, rec.e, LAWS.index(law)))


ROW = {"ext": lambda r, law: plain_row(r, law)[1], "exact": exact_row, "ways": ways_row, "seats": seats_row,
       "ext_seats": ext_seats_row}
WORDS = {"ext": 13, "exact": 13, "ways": 22, "seats": 32, "ext_seats": 32}


def expect(entry, recs, law):
    return np.stack([ROW[entry](r, law) for r in recs]).astype(np.uint64)


# ---- kind 0 by plain enumeration: every completion, every hand scored by the oracle
_enum = {}


def enumerate_all_in(rec, law, threads=16):
    """-> (plain [13], ways [22], seats [32]) integer rows of an all-in record, independent of the lane code.

    All C(L, 5 - nb) sets of table cards from the deck in card-id order.  The weight of a set restates the rule of
    tests/exact_seats_literal.py (exact_literal._tables): under the reference's law a table card is deck.pop(i) with
    i < len(deck) - 1, never the highest card left, so a set that holds the deck's highest card cannot be dealt and every
    other set can in each of its k! orders -- one common factor, which the integer rows drop: weight 0 or 1.  Under the
    uniform law every set has weight 1."""
    key = (rec.name, law)
    if key in _enum:
        return _enum[key]
    assert rec.kind == 0
    deck = np.array(rec.deck(), np.uint8)
    k = 5 - rec.nb
    sets = list(itertools.combinations(range(len(deck)), k))
    pos = np.array(sets, np.intp).reshape(len(sets), k)
    w = np.ones(len(pos), np.int64) if law == "uniform" else (pos != len(deck) - 1).all(1).astype(np.int64)
    table = np.concatenate([np.broadcast_to(np.array(rec.board, np.uint8), (len(pos), rec.nb)), deck[pos]], 1)
    hands = rec.hands
    scores = np.stack([O.score_batch(np.concatenate([np.broadcast_to(np.array(h, np.uint8), (len(pos), 2)), table], 1), threads)
                       for h in hands])
    level = scores == scores.max(0)
    n_level = level.sum(0)
    seats = np.zeros(32, np.uint64)
    seats[0] = w.sum()
    for s in range(len(hands)):
        seats[2 + 3 * s] = (w * (level[s] & (n_level == 1))).sum()
        seats[3 + 3 * s] = (w * (level[s] & (n_level > 1))).sum()
        seats[4 + 3 * s] = (w * level[s] * (UNIT // n_level)).sum()
    ways = np.zeros(22, np.uint64)
    ways[0], ways[2], ways[3] = seats[0], seats[2], seats[3]
    types = O.score_type(scores[0])
    for t in range(9):
        ways[4 + t] = (w * level[0] * (types == t)).sum()
    for n in range(2, 11):
        ways[13 + n - 2] = (w * (level[0] & (n_level == n))).sum()
    _enum[key] = (ways[:13].copy(), ways, seats)
    return _enum[key]


# ---- mirrors of mcq_exact_plan / mcq_exact_ext_plan (csrc/mcq_plan.hpp; tests/test_plan_host.py holds them to the header)
#      and of how the kernels walk a job
def binom(n, k):
    from math import comb
    return comb(n, k)


def plan_exact(rec, n_cu):
    """mcq_exact_plan -> (grid, slices, units, waves per block)."""
    n_boards = binom(50 - rec.nb, 5 - rec.nb)
    if rec.n_players == 3:
        slices = 1
        while slices < 64 and n_boards * slices < 6 * n_cu * 4:
            slices *= 2
        units = n_boards * slices
        return min(-(-units // 6), n_cu), slices, units, 6
    return min(-(-n_boards // 16), n_cu), 1, n_boards, 16


def plan_ext(rec, n_cu):
    """mcq_exact_ext_plan -> (grid, groups, completions)."""
    n_boards = binom(rec.L, 5 - rec.nb)
    if rec.kind == 0:
        return min(-(-n_boards // 1024), n_cu), 1, n_boards
    if rec.kind == 1:
        return min(-(-n_boards // 16), n_cu), 1, n_boards
    groups = -(-(rec.L * (rec.L - 1) // 2) // 1024)
    per = min(max(n_cu // groups, 1), n_boards)
    return per * groups, groups, n_boards


def busiest(rec, entry, n_cu):
    """The most units one owner walks: a wave of mcq_exact_kernel (unit = completion x slice), a lane of kind 0, a wave of
    kind 1, a block of kind 2."""
    if entry == "exact":
        grid, _, units, waves = plan_exact(rec, n_cu)
        return -(-units // (grid * waves))
    grid, groups, n_boards = plan_ext(rec, n_cu)
    owners = grid * 1024 if rec.kind == 0 else grid * 16 if rec.kind == 1 else grid // groups
    return -(-n_boards // owners)
