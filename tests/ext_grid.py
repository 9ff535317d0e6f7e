"""The grid of EXTENDED queries shared by tests/test_ext_kernel_grid_host.py and tests/test_ext_kernel_grid_gpu.py.

Every kind of restriction (K0..K7 below) at 2 to 10 players on every street, with run counts at the edges of a stream, of a
wave task and of the MCQ-CTR v5x stream rule (mcq_ext_stream_iters: a query that draws from a candidate list and has at
most 8192 iterations runs streams of 2 iterations, every other query streams of 16).  The records are generated from a
fixed numpy seed; the expected rows come from the host builds of the lane code (tests/hostsim_ext_ways: 22 words,
tests/hostsim_seats: 32 words), which the host file pins to the oracle, and are cached here for both files.

    kind  content                                                     lists    form
    K0    empty record                                                0        general (= the plain path)
    K1    opponent range                                              1        fast
    K2    ghost cards only                                            0        general
    K3    one known two-card hand, opponents unrestricted             0        general
    K4    known two-card hand + opponent range                        1 (*)    general
    K5    hero range                                                  1        general
    K6    hero range + ranged known hand + opponent range             3 (*)    general
    K7    5 to 9 known hands, cards and ranges mixed                  6/7/10   general
(*) one list fewer heads-up, where no opponent is left to draw from the opponents' range: what counts as a query that
draws from a list is what mcq_ext_n_lists says, nothing else.  Ten lists are the most a valid record has (ten hands, or
nine hands and the opponents): MCQ_EXT_MAX_LISTS = 11 is never reached."""
import json
import os

import numpy as np

import neuron_poker_amd as npa
from tests import hostsim_ext_ways as H
from tests import hostsim_seats as HS

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SEED = (1 << 41) | 0x9E3779B97   # >= 2^40: the high key word of the counter-mode streams is not zero
FQ = 1000003                     # first_query_id of the grid batch in its canonical order
GEN_SEED = 20240613
KINDS = ("K0", "K1", "K2", "K3", "K4", "K5", "K6", "K7")
STREETS = (0, 3, 4, 5)
RUNS_LISTED = (1, 2, 3, 127, 128, 129, 255, 257, 8191, 8192, 8193, 16385)
RUNS_PLAIN = (1, 15, 16, 17, 1023, 1024, 1025, 4097)
SHORT_RUNS = 8192                # MCQ_EXT_SHORT_RUNS
K7_LISTS = (6, 7, 10)

with open(os.path.join(_ROOT, "neuron_poker_amd", "preflop_classes.json")) as _f:
    CLASSES = json.load(_f)
assert len(CLASSES) == 169


def min_players(kind):
    return {"K7": 6}.get(kind, 2)    # 1 + n_known, and two players at least


CELLS = {(k, p, nb) for k in KINDS for p in range(min_players(k), 11) for nb in STREETS}


class Rec:
    """One extended query: the packed records, what the oracle's run_ex takes, and what the host layer cuts it by."""

    def __init__(self, kind, q, ext, oracle_args=None):
        self.kind, self.q, self.ext = kind, q, ext
        self.players, self.nb, self.runs = int(q["n_players"][0]), int(q["n_board"][0]), int(q["runs"][0])
        self.oracle_args = oracle_args          # hero, board, known, ghost, opp: card strings / class strings
        self.lists = H.n_lists(q, ext)
        self.s_iters = H.stream_iters(q, ext)
        self.tasks = H.task_count(q, ext)
        self.weight = H.task_weight(q, ext)
        self.fast = H.is_fast(q, ext)
        self.n_known = int(ext["n_known"][0])
        self.key = q.tobytes() + ext.tobytes()

    @property
    def cell(self):
        return self.kind, self.players, self.nb

    def with_runs(self, runs):
        """The same query with another run count."""
        q = self.q.copy()
        q["runs"] = runs
        return Rec(self.kind, q, self.ext, self.oracle_args)

    def __repr__(self):
        return "Rec(%s, %d players, %d table cards, %d runs, %d lists)" % (self.kind, self.players, self.nb, self.runs, self.lists)


def _classes(rng, lo=40, hi=80, fat=False):
    """A range: lo..hi of the 169 classes, or all but one (a fat list)."""
    if fat:
        drop = int(rng.integers(169))
        return sorted(c for i, c in enumerate(CLASSES) if i != drop)
    return sorted(rng.choice(CLASSES, int(rng.integers(lo, hi + 1)), replace=False).tolist())


def _k7_shape(players, lists, rng, all_in=False):
    """(n_known, ranged hands among hero + known, opponents' list?) of a K7 record with `lists` lists, or None.  all_in:
    every player's hand is known, no random opponent."""
    options = []
    for k in range(5, min(9, players - 1) + 1):
        for opp in ((1, 0) if players > 1 + k else (0,)):
            ranged = lists - opp
            if 1 <= ranged <= 1 + k:
                options.append((k, ranged, bool(opp)))
    if all_in:
        options = [o for o in options if o[0] == players - 1]
    return options[int(rng.integers(len(options)))] if options else None


def make(kind, players, nb, runs, rng, fat=False, lists=None, all_in=False):
    """A record of one kind.  fat: every range has 168 classes.  lists (K7): how many candidate lists."""
    deck = [int(c) for c in rng.permutation(52)]
    take = lambda n: [deck.pop() for _ in range(n)]   # noqa: E731
    names = lambda ids: [npa.card_str(c) for c in ids]   # noqa: E731
    board = take(nb)
    hero, ghost, opp, known = take(2), None, None, []         # known: two card ids, or a list of class strings
    hero_range = None
    wide = dict(lo=60, hi=100) if kind == "K7" else {}
    if kind in ("K1", "K4", "K6"):
        opp = _classes(rng, fat=fat)
    if kind == "K2":
        ghost = take(2)
    if kind in ("K3", "K4"):
        known = [take(2)]
    if kind in ("K5", "K6"):
        hero_range = _classes(rng, fat=fat)
    if kind == "K6":
        known = [_classes(rng, fat=fat)]
    if kind == "K7":
        n_known, ranged, opp_list = _k7_shape(players, lists, rng, all_in)
        is_range = np.zeros(1 + n_known, bool)
        is_range[rng.permutation(1 + n_known)[:ranged]] = True
        if is_range[0]:
            hero_range = _classes(rng, fat=fat, **wide)
        known = [_classes(rng, fat=fat, **wide) if r else take(2) for r in is_range[1:]]
        if opp_list:
            opp = _classes(rng, fat=fat, **wide)
    is_cards = lambda h: isinstance(h[0], int)   # noqa: E731
    ext = npa.pack_query_ext(1, ghost=ghost, hero_range=npa.range_bits(hero_range) if hero_range else None,
                             opp_range=npa.range_bits(opp) if opp else None,
                             known=[h if is_cards(h) else npa.range_bits(h) for h in known])
    args = dict(hero=hero_range if hero_range else names(hero), board=names(board), ghost=names(ghost) if ghost else None,
                opp=opp, known=[names(h) if is_cards(h) else h for h in known])
    q = npa.pack_queries([[0, 1] if hero_range else hero], [board + [255] * (5 - nb)], players, int(runs))
    return Rec(kind, q, ext, args)


def _probe_lists(kind, players):
    """Does a record of this kind at this player count draw from a list?  (K4 heads-up does not.)"""
    return kind in ("K1", "K5", "K6", "K7") or (kind == "K4" and players > 2)


_grid = None


def grid():
    """The records, in canonical order (record j has query id FQ + j).  Every cell twice: once with a run count that gives
    more than one task AND leaves a stream partly filled (129 / 257 iterations in streams of 2, 1025 in streams of 16), once
    with the next run count of its class, so that every kind sees every run count."""
    global _grid
    if _grid is not None:
        return _grid
    rng = np.random.default_rng(GEN_SEED)
    recs, turn = [], {}
    for kind in KINDS:
        for nb in STREETS:
            for players in range(min_players(kind), 11):
                listed = _probe_lists(kind, players)
                pool = RUNS_LISTED if listed else RUNS_PLAIN
                t = turn.get((kind, listed), 0)
                turn[(kind, listed)] = t + 1
                lists = None
                if kind == "K7":   # 6, 7 and 10 lists in turn, where the player count allows them (six players: 6 only)
                    want = [n for n in K7_LISTS[t % 3:] + K7_LISTS[:t % 3] if _k7_shape(players, n, np.random.default_rng(0))]
                    lists = 10 if players == 10 and nb == 0 else want[0]
                all_in = kind == "K7" and players == 10 and nb == 0    # ten hands, ten lists, nobody left to draw
                first = make(kind, players, nb, (129, 257)[t & 1] if listed else 1025, rng, lists=lists, all_in=all_in)
                recs.append(first)
                recs.append(first.with_runs(pool[t % len(pool)]) if t % 3 else
                            make(kind, players, nb, pool[t % len(pool)], rng, lists=lists, all_in=all_in))
    assert_grid(recs)
    _grid = recs
    return recs


def assert_grid(recs):
    """No cell left out, every run-count class, both stream rules, and the kinds are what the table above says."""
    assert {r.cell for r in recs} == CELLS, sorted(CELLS - {r.cell for r in recs})
    assert {r.cell for r in recs if r.tasks > 1} == CELLS
    assert {r.cell for r in recs if r.runs % r.s_iters} == CELLS
    for r in recs:
        assert r.lists == H.n_lists(r.q, r.ext) and (r.lists > 0) == _probe_lists(r.kind, r.players), r
        assert r.s_iters == (2 if r.lists and r.runs <= SHORT_RUNS else 16), r
        assert r.fast == (r.kind == "K1"), r
        assert r.players >= 1 + r.n_known
    for kind in KINDS:
        mine = [r for r in recs if r.kind == kind]
        listed = {r.runs for r in mine if r.lists}
        plain = {r.runs for r in mine if not r.lists}
        if kind in ("K0", "K2", "K3"):
            assert not listed and set(RUNS_PLAIN) <= plain, kind
        else:
            assert set(RUNS_LISTED) <= listed, (kind, sorted(listed))
            assert {r.s_iters for r in mine if r.lists} == {2, 16}, kind
        want = {"K0": {0}, "K1": {1}, "K2": {0}, "K3": {0}, "K4": {0, 1}, "K5": {1}, "K6": {2, 3}, "K7": set(K7_LISTS)}[kind]
        assert {r.lists for r in mine} == want, (kind, {r.lists for r in mine})
    assert {r.runs for r in recs if r.kind == "K4" and not r.lists} <= set(RUNS_PLAIN)
    k7 = [r for r in recs if r.kind == "K7"]
    assert {r.n_known for r in k7} == {5, 6, 7, 8, 9}
    assert any(r.players == 10 and r.n_known == 9 and r.lists == 10 for r in k7)      # all-in, no random opponent
    assert any(0 < int(r.ext["known"]["is_range"][0, :r.n_known].sum()) < r.n_known for r in k7)   # cards and ranges mixed


def pack(recs):
    return np.concatenate([r.q for r in recs]), np.concatenate([r.ext for r in recs])


# ---- expected rows: the host builds of the lane code, one walk per (record, query id), shared by both test files
_ways, _seats = {}, {}


def ways_row(rec, qid, seed=SEED):
    """The 22 words of the record as query `qid` (the form the kernels pick).  ValueError if it cannot be dealt."""
    key = (rec.key, qid, seed)
    if key not in _ways:
        _ways[key] = H.run(False, rec.q, rec.ext, seed, qid)
    return _ways[key]


def seats_row(rec, qid, seed=SEED):
    """The 32 words of the record as query `qid`."""
    key = (rec.key, qid, seed)
    if key not in _seats:
        _seats[key] = HS.run(rec.q, rec.ext, seed, qid)
    return _seats[key]


def expect(recs, fq, seed=SEED, seats=True):
    """The rows of a batch whose first query has id fq -> ([n, 22], [n, 32] or None)."""
    ways = np.stack([ways_row(r, fq + j, seed) for j, r in enumerate(recs)])
    return ways, np.stack([seats_row(r, fq + j, seed) for j, r in enumerate(recs)]) if seats else None


# ---- mirrors of the host layer's and the kernels' choices
SMALL_Q, SMALL_LISTS, SMALL_TASKS, SMALL_BLOCKS = 8, 6, 64, 32   # MCQ_EXT_SMALL_* (csrc/mcq_plan.hpp)
STAGE_ENTRIES, STAGE_LISTS = 18 * 1024, 96                        # MCQ_EXT_STAGE_ENTRIES, _LISTS (csrc/mcq_stage.hpp)
BLOCK_WAVES = 16                                                   # kBlock / 64


def small_plan(recs):
    """eval_batch_ext_impl's choice for the hero and ways rows under the default knobs: None = the general path, else
    (wpb, parts per query, blocks) of the one-launch kernel.  The mirror of mcq_ext_small_fits and mcq_ext_small_plan
    (csrc/mcq_plan.hpp); tests/test_plan_host.py holds the two together."""
    if len(recs) > SMALL_Q or max(max(r.lists for r in recs), 1) > SMALL_LISTS or max(r.tasks for r in recs) > SMALL_TASKS:
        return None
    parts = lambda r, wpb: -(-r.tasks // wpb) if r.tasks > wpb else 1   # noqa: E731
    wpb = 4
    while wpb < 16 and sum(parts(r, wpb) for r in recs) > SMALL_BLOCKS:
        wpb <<= 1
    p = [parts(r, wpb) for r in recs]
    return wpb, p, sum(p)


def geometry(total_tasks, n_cu, occ):
    """mcq_plan_geometry (csrc/mcq_plan.hpp) for the extended evaluation kernel -> (grid, waves per block);
    tests/test_plan_host.py holds the two together."""
    wpb = min(max(-(-total_tasks // n_cu), 1), BLOCK_WAVES)
    blocks = -(-total_tasks // wpb)
    grid = blocks if blocks < n_cu else (n_cu * occ if wpb == BLOCK_WAVES else n_cu)
    return grid, max(wpb, 4)


def block_records(prefix, n, blk, wpb, grid):
    """The records of block `blk` of `grid` blocks of `wpb` waves on the cost axis prefix[0..n] (Python integers): (first
    record, number of records), or None for a block without a piece of the axis.  The mirror of mcq_axis_block_records
    (csrc/mcq_axis.hpp); tests/test_axis_host.py holds the two together."""
    total, n_waves = int(prefix[n]), grid * wpb
    blo, bhi = total * (blk * wpb) // n_waves, total * ((blk + 1) * wpb) // n_waves
    if blo >= bhi:
        return None
    a, b = 0, n
    while b - a > 1:
        mid = (a + b) >> 1
        if prefix[mid] <= blo:
            a = mid
        else:
            b = mid
    qa = a
    b = n
    while b - a > 1:
        mid = (a + b) >> 1
        if prefix[mid] < bhi:
            a = mid
        else:
            b = mid
    return qa, a - qa + 1


_list_len = {}


def list_counts(recs, stride):
    """cnts[query * stride + li] as mcq_ext_lists_kernel leaves them: the lists' lengths, 0 behind a query's last list."""
    out = np.zeros(len(recs) * stride, np.uint32)
    for qi, r in enumerate(recs):
        if r.key not in _list_len:
            _list_len[r.key] = [H.list_len(r.q, r.ext, li) for li in range(r.lists)]
        out[qi * stride:qi * stride + r.lists] = _list_len[r.key]
    return out


def stage_lists(cnts, stride, qa, nq):
    """What a block of mcq_eval_ext_kernel decides about the candidate lists of its queries qa .. qa + nq - 1 -> ("staged"
    | "count" | "entries", {list: the offset the block stores for it}).  "count": more than 96 lists; "entries": the lists
    hold more than 18 432 entries.  The mirror of mcq_ext_stage_lists (csrc/mcq_stage.hpp); tests/test_stage_host.py holds
    the two together, limits included."""
    if nq * stride > STAGE_LISTS:
        return "count", {}
    at, off = 0, {}
    for k in range(nq * stride):
        off[k] = at
        at += (int(cnts[qa * stride + k]) + 1) & ~1     # whole 32-bit words
        if at > STAGE_ENTRIES:
            break
    off[nq * stride] = at
    return "staged" if at <= STAGE_ENTRIES else "entries", off


def staging(recs, n_cu, occ, offsets=False):
    """What every block of mcq_eval_ext_kernel decides about its queries' candidate lists, for a batch on the general
    path: a list, one entry per block with work, of (verdict of stage_lists, first query, queries), with `offsets` also
    the offsets."""
    n = len(recs)
    stride = max(max(r.lists for r in recs), 1)
    prefix = np.concatenate([[0], np.cumsum([r.tasks * r.weight for r in recs], dtype=np.uint64)]).astype(object)
    grid, wpb = geometry(sum(r.tasks for r in recs), n_cu, occ)
    cnts = list_counts(recs, stride)
    out = []
    for blk in range(grid):
        mine = block_records(prefix, n, blk, wpb, grid)
        if mine is None:
            continue
        verdict, off = stage_lists(cnts, stride, *mine)
        out.append((verdict, *mine, off) if offsets else (verdict, *mine))
    return out


# ---- the constructions of the GPU file (built here so that the host file checks the mirrors' verdicts without a GPU)
def pick(kind, players=None, lists=None, nb=None):
    """The first record of the grid of that kind (and player count, list count, street)."""
    for r in grid():
        if r.kind == kind and players in (None, r.players) and lists in (None, r.lists) and nb in (None, r.nb):
            return r
    raise KeyError((kind, players, lists, nb))


def _mix(kinds, runs):
    """Records of the given kinds (K7: six lists) at 3 to 7 players, streets in turn, with the given run counts."""
    return [pick(k, 6 if k == "K7" else 3 + j % 5, 6 if k == "K7" else None, STREETS[j % 4]).with_runs(r)
            for j, (k, r) in enumerate(zip(kinds, runs))]


_small = None


def small_batches():
    """name -> (records, first query id, the (wpb, blocks) the host must choose) for the one-launch kernel."""
    global _small
    if _small is None:
        b = {
            "wpb4_two_parts": (_mix(("K1", "K4", "K5", "K6", "K1", "K5", "K7", "K4"), [1024] * 8), (4, 16)),
            "wpb8": (_mix(("K1", "K5", "K4", "K6", "K1", "K7", "K5"), (1, 127, 129, 1000, 2047, 4500, 8192)), (8, 19)),
            "wpb16_32_blocks": (_mix(("K1", "K4", "K5", "K6", "K1", "K1", "K5", "K4"), [8192] * 8), (16, 32)),
            "one_64_task_query_among_one_task_queries": (_mix(("K1", "K5", "K4", "K6", "K1", "K7"), (8192, 1, 2, 3, 127, 128)), (4, 21)),
            "streams_of_16": (_mix(("K0", "K1", "K5", "K2", "K3"), (65536, 8193, 8193, 1025, 17)), (4, 24)),
            "one": (_mix(("K6",), (257,)), (4, 1)),
            "two": (_mix(("K1", "K0"), (1000, 1024)), (4, 3)),
            "three": (_mix(("K7", "K2", "K5"), (255, 4097, 3)), (4, 4)),
        }
        _small = {name: (recs, FQ + 10000 + 100 * i, want) for i, (name, (recs, want)) in enumerate(b.items())}
    return _small


_fences = None


def fence_batches():
    """name -> (records, first query id, one launch?)."""
    global _fences
    if _fences is None:
        thin = [pick(k, 2 + j, None, STREETS[j % 4]).with_runs(129) for j, k in enumerate(("K1", "K4", "K5", "K6", "K0", "K2", "K3", "K1", "K5"))]
        b = {"six_lists": ([pick("K7", 7, 6), pick("K1", 4)], True),
             "seven_lists": ([pick("K7", 8, 7), pick("K1", 4)], False),
             "ten_lists": ([pick("K7", 10, 10), pick("K1", 4)], False),
             "64_tasks": ([pick("K0", 3).with_runs(65536)], True),
             "65_tasks": ([pick("K0", 3).with_runs(65537)], False),
             "eight_queries": (thin[:8], True),
             "nine_queries": (thin, False)}
        _fences = {name: (recs, FQ + 20000 + 100 * i, small) for i, (name, (recs, small)) in enumerate(b.items())}
    return _fences


_placement = None


def placement_batches():
    """name -> (records, first query id) of the list-placement constructions (a) to (d) of the GPU file."""
    global _placement
    if _placement is None:
        rng = np.random.default_rng(GEN_SEED + 1)
        thin = [r for r in grid() if 0 < r.lists <= 3 and r.runs in (129, 257)]
        staged = [thin[(7 * j) % len(thin)] for j in range(12)]
        no_stage = [make("K7", 10, STREETS[j % 4], 129, rng, fat=True, lists=10, all_in=j % 3 == 0) for j in range(12)]
        fat_k1 = [make("K1", 2 + j % 9, STREETS[j // 9 % 4], 64, rng, fat=True) for j in range(36)]
        by_entries = [fat_k1[j % 36] for j in range(6000)]
        fat8 = [make("K7", 9 + j % 2, STREETS[j % 4], 64, rng, fat=True, lists=8 + j % 2) for j in range(12)]
        thin_k1 = [make("K1", 2 + j % 5, STREETS[j % 4], 2048, rng) for j in range(12)]
        mixed = [fat8[j % 12] for j in range(80)] + [thin_k1[j % 12] for j in range(160)]
        _placement = {"staged": (staged, FQ + 30000), "no_block_stages": (no_stage, FQ + 31000),
                      "refused_by_entries": (by_entries, FQ + 32000), "refusing_beside_staging": (mixed, FQ + 40000)}
    return _placement


def placement_verdicts(recs, n_cu):
    """The blocks' decisions at one and at two resident blocks per CU -> [set of verdicts, ...] and the per-block lists."""
    both = [staging(recs, n_cu, occ) for occ in (1, 2)]
    return [{v for v, _, _ in s} for s in both], both


def shuffled():
    """The grid in a fixed shuffled order under its own first query id: list-less queries on streams of 16, listed ones
    on streams of 2 and listed ones above 8192 iterations come to lie side by side on the waves' slices of the cost axis."""
    recs = grid()
    order = np.random.default_rng(GEN_SEED + 2).permutation(len(recs))
    return [recs[i] for i in order], FQ + 50000
