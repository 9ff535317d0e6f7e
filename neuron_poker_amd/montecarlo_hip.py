"""Drop-in for tools/montecarlo_python.py of neuron_poker, computed on an MI355X.

Same call surface, same meaning of the arguments, same attributes afterwards
(reference: tools/montecarlo_python.py:191-252 and :401-406):

    get_equity(player_cards, table_cards, players, runs) -> float
    MonteCarlo().run_montecarlo(original_player_card_list, original_table_card_list, player_amount, ui,
                                maxRuns, timeout, ghost_cards, opponent_range=1) -> (equity, winTypesDict)
        then .equity .winnerCardTypeList .winTypesDict .runs .passes

so `HoldemTable.get_equity = montecarlo_hip.get_equity` (gym_env/env.py:75-81) is the whole integration.
New and additive: get_equity_batch() evaluates many states in one launch.

Deliberate differences:
  * exactly `runs` iterations are executed; the reference's 1 s wall-clock cut-off (montecarlo_python.py:235,
    :405) is not reproduced, `timeout` and `ui` are accepted and ignored;
  * the library never touches numpy's global random state.  seed(s) makes results reproducible; in
    mode 'replay' a call after seed(s) returns exactly what the reference returns after np.random.seed(s);
  * a hero card that is also on the table is rejected with ValueError (the reference silently swallows it,
    montecarlo_python.py:154-161);
  * all of run_montecarlo's arguments are supported: opponent ranges (a fraction of the 169 preflop classes or an
    explicit set), ghost cards, and any number of known hands, each two cards or a set of classes
    (tools/montecarlo_python.py:36-112, 133-181, 206-208; bit-exact in mode 'replay').  A range that cannot be
    dealt from the remaining cards raises ValueError where the reference would loop forever.
"""
import json
import os
import struct
import threading
from collections import Counter

import numpy as np

from . import _lib
from .cards import TYPES, card_id, card_str

__all__ = ["get_equity", "get_pot_equity", "get_seat_equities", "get_seat_equities_exact", "get_equity_batch", "get_equity_exact", "get_range_equity_exact", "get_range_equity_exact_weighted", "get_range_equities", "get_range_hand_equities", "quantise_weight", "get_preflop_range_equity_exact", "get_preflop_range_equity_exact_weighted", "preflop_class_table", "get_runout_equities", "MonteCarlo", "seed",
           "configure", "get_equity_matrix", "matrix_equity"]

_state = {"couple_numpy": False,
          "mode": _lib.MODE_REPLAY_MT19937 if os.environ.get("MCQ_MODE", "philox").lower() == "replay"
          else _lib.MODE_PHILOX}
_lock = threading.Lock()


class _Stream(threading.local):
    """(seed, query counter) of the calling THREAD: seed(s) in a thread makes that thread's calls reproducible whatever
    other threads do meanwhile (every thread also has its own engine, _lib.default_engine()).  A thread that never
    called seed() starts from the operating system's entropy."""

    def __init__(self):
        self.seed = int.from_bytes(os.urandom(8), "little")
        self.counter = 0


_stream = _Stream()
_MODES = {"philox": _lib.MODE_PHILOX, "replay": _lib.MODE_REPLAY_MT19937,
          _lib.MODE_PHILOX: _lib.MODE_PHILOX, _lib.MODE_REPLAY_MT19937: _lib.MODE_REPLAY_MT19937}


def seed(s):
    """Counterpart of np.random.seed(s) for this module: the calling thread's next call uses stream `s`."""
    _stream.seed = int(s) & (2 ** 64 - 1)
    _stream.counter = 0


def configure(mode=None, couple_numpy=None, dealing=None):
    """mode: 'philox' (default, production) or 'replay' (bit-exact MT19937 replay of the reference).
    dealing: 'reference' (default: the Python reference's law incl. its index bias) or 'uniform' (unbiased, what
    the reference's Cython/C++ variants deal; production mode and plain queries only: an extended query -- a range,
    ghost cards, further known hands -- raises ValueError under it) -- applied to every thread's default engine and
    to the multi-GPU engines of get_equity_batch(n_gpus=...); call it while no equity call is running.
    couple_numpy=True (replay mode only): draw from numpy's GLOBAL random state and advance it exactly as the
    reference does, so that code sharing np.random with the equity call (gym_env/env.py:142,680,686 deals with
    it) follows the reference's trajectory after np.random.seed(s)."""
    if mode is not None:
        if mode not in _MODES:
            raise ValueError("mode must be 'philox' or 'replay'")
        _state["mode"] = _MODES[mode]
    if couple_numpy is not None:
        _state["couple_numpy"] = bool(couple_numpy)
    if dealing is not None:
        _lib.set_default_dealing_law(dealing)
        with _lock:
            multis = list(_MULTI.values())
        for me in multis:
            with me.lock:
                me.set_dealing_law(dealing)


_CLASS_ORDER = None
_TOP_BITS = {}   # take -> bit set of the last `take` classes of the equity order


def _class_order():
    """The 169 preflop classes in the order the reference sorts them by equity (ascending); generated from the
    reference by tests/golden/gen_golden.py into preflop_classes.json."""
    global _CLASS_ORDER
    if _CLASS_ORDER is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "preflop_classes.json")) as f:
            _CLASS_ORDER = json.load(f)
    return _CLASS_ORDER


def _opponent_range_bits(opponent_range):
    """run_montecarlo's opponent_range -> 169-bit set or None for "every class" (montecarlo_python.py:194-199 and
    :105-112: a number keeps the LAST int(169 * r) classes of the equity-sorted list -- and all of them when that
    is 0, as list[-0:] does --, anything else is used as the set of allowed classes)."""
    if type(opponent_range) in (float, int):
        take = int(169 * opponent_range)
        if take <= 0 or take >= 169:
            return None
        bits = _TOP_BITS.get(take)
        if bits is None:
            bits = _TOP_BITS[take] = _lib.range_bits(_class_order()[-take:])
        return bits
    return _lib.range_bits(opponent_range)


_EXT_CACHE = {}   # (opponent_range, ghost_cards, hero range, further known hands) -> mcq_query_ext record (1-element array)


def _ext_record(hero, hero_is_range, known_hands, ghost_cards, opponent_range, opp_bits):
    """The extension record of a run_montecarlo call.  An agent asks with the same ranges decision after decision (what
    changes is its cards and the table), and building the record -- class strings to bit sets, a numpy structured
    array -- costs more than the GPU call (60 of 86 us): the records of the last few distinct settings are kept."""
    def freeze(h):
        return frozenset(h) if isinstance(h, (set, frozenset)) else tuple(h)
    try:
        key = (opponent_range if type(opponent_range) in (float, int) else frozenset(opponent_range),
               ghost_cards if isinstance(ghost_cards, str) or ghost_cards is None else tuple(ghost_cards),
               frozenset(hero) if hero_is_range else None, tuple(freeze(h) for h in known_hands))
        ext = _EXT_CACHE.get(key)
    except TypeError:  # something unhashable inside: build it afresh
        key, ext = None, None
    if ext is None:
        ghost = _ghost_ids(ghost_cards)
        known = [_lib.range_bits(h) if isinstance(h, (set, frozenset)) else [card_id(c) for c in h] for h in known_hands]
        ext = _lib.pack_query_ext(1, ghost=ghost, known=known,
                                  hero_range=_lib.range_bits(hero) if hero_is_range else None, opp_range=opp_bits)
        if key is not None:
            if len(_EXT_CACHE) >= 64:
                _EXT_CACHE.clear()
            _EXT_CACHE[key] = ext
    return ext


def _take_ids(n):
    first = _stream.counter
    _stream.counter = first + n
    return _stream.seed, first


def _query(player_cards, table_cards, players, runs):
    hole = [card_id(c) for c in player_cards]
    board = [card_id(c) for c in table_cards]
    if len(hole) != 2:
        raise ValueError("player_cards must hold exactly two cards")
    if len(board) > 5:
        raise ValueError("table_cards holds more than five cards")
    players = int(players)
    runs = int(runs)
    if runs < 1:
        raise ValueError("runs must be >= 1")
    return _lib.pack_query_one(hole, board, players, runs)


def _hero_query(hero, table_cards, players, runs):
    """_query for a hero given as two cards or as a range (a set of classes): a range's record is made with two
    placeholder cards that pass _query's checks, and its hole, which the library does not read, is then zeroed."""
    if not isinstance(hero, (set, frozenset)):
        return _query(list(hero), table_cards, players, runs)
    q = _query(["2C", "2D"], table_cards, players, runs)
    q["hole"] = 0
    return q


def _split_ties(ties, whole="credited"):
    """The `ties` argument: `whole` (a tied pot counts for hero in full) or 'split'.  -> whether it is 'split'."""
    if ties not in (whole, "split"):
        raise ValueError("ties must be '%s' or 'split'" % whole)
    return ties == "split"


def _ghost_ids(ghost_cards, exactly_two=False):
    """run_montecarlo's ghost_cards ('' or None: none) -> the two card ids or None."""
    if ghost_cards == '' or ghost_cards is None:
        return None
    if exactly_two and len(ghost_cards) != 2:
        raise ValueError("ghost_cards is two cards or ''")
    return [card_id(ghost_cards[0]), card_id(ghost_cards[1])]


def _two_cards_each(hands, message="a known hand is two cards here (ranged known hands are not enumerated)"):
    """Known hands that an enumeration takes as two cards each: a range or another length raises ValueError(message)."""
    if any(isinstance(h, (set, frozenset)) or len(h) != 2 for h in hands):
        raise ValueError(message)


class MonteCarlo(object):
    """Mirror of tools/montecarlo_python.py:22 MonteCarlo for the path gym_env/env.py uses."""

    def __init__(self, engine=None):
        self._engine = engine
        self.equity = None
        self.winnerCardTypeList = Counter()
        self.winTypesDict = self.winnerCardTypeList.items()
        self.runs = 0
        self.passes = 0
        self.result = None

    def run_montecarlo(self, original_player_card_list, original_table_card_list, player_amount, ui, maxRuns,
                       timeout, ghost_cards, opponent_range=1, *, mode=None, seed=None, ties="credited"):
        """mode: None (the configured one), 'philox', 'replay', or 'exact' (the exact probabilities the Monte-Carlo modes
        converge to: see _run_exact).
        ties="credited" (default): a tied pot counts for hero in full, as the reference does.  ties="split": `equity`
        is hero's expected SHARE of the pot (a tie among k hands counts 1/k) and `result` the 22-word row
        (RESULT_WAYS_DTYPE); winnerCardTypeList stays on the credited counts.  Same streams, same query ids."""
        split = _split_ties(ties)
        eng = self._engine or _lib.default_engine()
        if mode == "exact":
            return self._run_exact(eng, original_player_card_list, original_table_card_list, player_amount, ghost_cards,
                                   opponent_range, split)
        m = _state["mode"] if mode is None else _MODES[mode]
        players = list(original_player_card_list)
        if not 1 <= len(players) <= 1 + _lib.MAX_KNOWN:
            raise ValueError("between one and ten known hands")
        hero = players[0]
        hero_is_range = isinstance(hero, (set, frozenset))
        opp_bits = _opponent_range_bits(opponent_range)
        plain = not hero_is_range and len(players) == 1 and opp_bits is None and (ghost_cards == '' or ghost_cards is None)
        q = _hero_query(hero, list(original_table_card_list), player_amount, maxRuns)
        if plain:
            if m == _lib.MODE_REPLAY_MT19937 and _state["couple_numpy"] and seed is None:
                if split:
                    raise ValueError("ties='split': configure(couple_numpy=True) has no split-pot form")
                res = eng.eval_batch_numpy_stream(q)[0]
            else:
                s, first = _take_ids(1) if seed is None else (int(seed), 0)
                res = (eng.eval_batch_ways if split else eng.eval_batch)(q, s, first_query_id=first, mode=m)[0]
        else:
            ext = _ext_record(hero, hero_is_range, players[1:], ghost_cards, opponent_range, opp_bits)
            s, first = _take_ids(1) if seed is None else (int(seed), 0)
            # (straight to the C ABI: Engine.eval_batch_ext's conversions of arrays that are already right cost 8 us)
            out = np.zeros(1, _lib.RESULT_WAYS_DTYPE if split else _lib.RESULT_DTYPE)
            entry = eng._lib.mcq_eval_batch_ext_ways if split else eng._lib.mcq_eval_batch_ext
            rc = entry(eng._ctx, q.ctypes.data, ext.ctypes.data, 1, s & 0xFFFFFFFFFFFFFFFF,
                       first & 0xFFFFFFFFFFFFFFFF, m, out.ctypes.data)
            if rc:
                _lib._raise(rc)
            res = out[0]
        runs = int(res["runs"])
        wins = int(res["win"]) + int(res["tie"])
        self.result = res
        self.equity = wins / runs                                   # montecarlo_python.py:243
        if split:
            self.equity = float(_lib.pot_share(np.array([res], _lib.RESULT_WAYS_DTYPE))[0])
        self.winnerCardTypeList = Counter({TYPES[t]: int(c) / runs   # :244-246
                                           for t, c in enumerate(res["by_type"]) if c})
        self.winTypesDict = self.winnerCardTypeList.items()          # :248
        self.runs = runs                                             # :249
        self.passes = int(res["passes"])                             # :250
        return self.equity, self.winTypesDict

    def _run_exact(self, eng, original_player_card_list, original_table_card_list, player_amount, ghost_cards,
                   opponent_range, split=False):
        """mode='exact': what run_montecarlo converges to, by enumeration (mcq_exact_batch_ext under the reference's law):
        equity and winTypesDict are the exact probabilities, result the row of integer weights (zero when there is
        none: a range with two random opponents), runs and passes 0.  Known hands are two cards each; a hero range,
        ranged known hands and more than two random opponents raise ValueError.  split: the exact pot share and the
        22-word row of weights (mcq_exact_batch_ext_ways: at most ONE random opponent)."""
        players = list(original_player_card_list)
        if not 1 <= len(players) <= 1 + _lib.MAX_KNOWN:
            raise ValueError("between one and ten known hands")
        if isinstance(players[0], (set, frozenset)):
            raise ValueError("mode='exact' needs the hero's two cards, not a range")
        _two_cards_each(players[1:], "mode='exact' needs every known hand as two cards")
        opp_bits = _opponent_range_bits(opponent_range)
        q = _query(list(players[0]), list(original_table_card_list), player_amount, 1)
        ext = _ext_record(list(players[0]), False, players[1:], ghost_cards, opponent_range, opp_bits)
        if split:
            prob, weights = eng.exact_ext_ways(q, ext, "reference")
            p = prob[0]["p"]
        else:
            prob, weights = eng.exact_ext(q, ext, "reference")
            p = prob[0]
        self.result = weights[0]
        self.equity = float(_lib.pot_share(weights)[0]) if split else float(p["win"] + p["tie"])
        self.winnerCardTypeList = Counter({TYPES[t]: float(v) for t, v in enumerate(p["by_type"]) if v})
        self.winTypesDict = self.winnerCardTypeList.items()
        self.runs = 0
        self.passes = 0
        return self.equity, self.winTypesDict


_CARD_ID = {r + s: 4 * i + j for i, r in enumerate("23456789TJQKA") for j, s in enumerate("CDHS")}
_fast = threading.local()   # per thread: (engine, ctypes query buffer, ctypes result buffer)


def get_equity(player_cards, table_cards, players, runs):
    """Get equity from a Monte-Carlo run -- tools/montecarlo_python.py:401-406, on the GPU.

    This is the call gym_env/env.py:261-262 makes at every step, so it does not go through MonteCarlo() and numpy: the
    16-byte record is packed into a reusable ctypes buffer and mcq_eval_batch is called directly (what
    run_montecarlo([list(player_cards)], list(table_cards), players, 1, maxRuns=runs, ...) computes, same streams)."""
    if _state["mode"] != _lib.MODE_PHILOX or _state["couple_numpy"]:
        simulation = MonteCarlo()
        simulation.run_montecarlo([list(player_cards)], list(table_cards), players, 1, maxRuns=runs, timeout=0,
                                  ghost_cards='', opponent_range=1)
        return simulation.equity
    try:
        hole = [_CARD_ID[c] for c in player_cards]
        board = [_CARD_ID[c] for c in table_cards]
    except (KeyError, TypeError):
        raise ValueError("a card is not in the deck: %r %r" % (player_cards, table_cards)) from None
    nb, runs, players = len(board), int(runs), int(players)
    if len(hole) != 2 or nb > 5:
        raise ValueError("player_cards must hold exactly two cards, table_cards at most five")
    if runs < 1:
        raise ValueError("runs must be >= 1")
    st = getattr(_fast, "st", None)
    eng = _lib.default_engine()
    if st is None or st[0] is not eng:
        import ctypes
        st = _fast.st = (eng, ctypes.create_string_buffer(16), (ctypes.c_uint64 * 13)())
    try:
        struct.pack_into("<2B5BBB3xI", st[1], 0, hole[0], hole[1], *(board + [0] * (5 - nb)), nb, players, runs)
    except struct.error as e:
        raise ValueError("n_players or runs out of range: %s" % e) from None
    s, first = _take_ids(1)
    rc = eng._lib.mcq_eval_batch(eng._ctx, st[1], 1, s, first, _lib.MODE_PHILOX, st[2])
    if rc:
        _lib._raise(rc)
    out = st[2]
    return (out[2] + out[3]) / out[0]


def get_pot_equity(player_cards, table_cards, players, runs, *, known_hands=(), ghost_cards=None, opponent_range=None):
    """get_equity's sibling: hero's expected SHARE of the pot, a tie among k hands counting 1/k (mcq_eval_batch_ways),
    where get_equity -- as the reference, tools/hand_evaluator.py:23 -- credits a tied pot to hero in full.  Same
    arguments, same seed()/stream state (a call takes one query id, as a get_equity call does) and the same configure()
    switches: mode and dealing law; couple_numpy has no split-pot form and raises ValueError.
    known_hands / ghost_cards / opponent_range (run_montecarlo's conventions; `players` counts the known hands): the
    extended split-pot entry (mcq_eval_batch_ext_ways) -- hand against hand, hand against range."""
    if _state["couple_numpy"] and _state["mode"] == _lib.MODE_REPLAY_MT19937:
        raise ValueError("get_pot_equity: configure(couple_numpy=True) has no split-pot form")
    if known_hands or ghost_cards or opponent_range is not None:
        sim = MonteCarlo()
        sim.run_montecarlo([list(player_cards)] + [h if isinstance(h, (set, frozenset)) else list(h) for h in known_hands],
                           list(table_cards), players, 1, maxRuns=runs, timeout=0, ghost_cards=ghost_cards or '',
                           opponent_range=1 if opponent_range is None else opponent_range, ties="split")
        return sim.equity
    q = _query(list(player_cards), list(table_cards), players, runs)
    s, first = _take_ids(1)
    rows = _lib.default_engine().eval_batch_ways(q, s, first_query_id=first, mode=_state["mode"])
    return float(_lib.pot_share(rows)[0])


def get_seat_equities(hands, table_cards, players=None, runs=10000, *, ghost_cards=None, opponent_range=None, exact=False,
                      dealing="reference"):
    """What EVERY hand is worth: the pot shares of all `players` seats from one run (mcq_eval_batch_ext_seats), a tie
    among k hands counting 1/k for each of them -- a list of `players` floats that sum to 1.
    hands[0] is the hero, the rest are the known hands in the order of original_player_card_list (each two cards, or for
    the Monte-Carlo form a set of class strings, as run_montecarlo takes them); the seats after them are the random
    opponents, drawn from opponent_range (run_montecarlo's conventions; None = every class), in dealing order.  `players`
    counts them all and defaults to len(hands).  One call takes one query id from the same seed() state as get_equity;
    production mode and the reference's dealing law, whatever configure() has set for the other calls.
    exact=True: the all-in case by enumeration (mcq_exact_batch_seats) under `dealing` ('reference' or 'uniform'): every
    hand two cards and no random opponent -- players != len(hands) raises ValueError; `runs` is ignored."""
    hands = [h if isinstance(h, (set, frozenset)) else list(h) for h in hands]
    if not 1 <= len(hands) <= 1 + _lib.MAX_KNOWN:
        raise ValueError("between one and ten hands")
    players = len(hands) if players is None else int(players)
    if exact and players != len(hands):
        raise ValueError("exact=True enumerates known hands only: players must equal len(hands)")
    if not exact and dealing != "reference":
        raise ValueError("the Monte-Carlo form deals the reference's law only (exact=True has dealing='uniform')")
    hero = hands[0]
    hero_is_range = isinstance(hero, (set, frozenset))
    if exact:
        _two_cards_each(hands, "exact=True needs every hand as two cards")
    opp_range = 1 if opponent_range is None else opponent_range
    q = _hero_query(hero, list(table_cards), players, 1 if exact else runs)
    ext = _ext_record(hero, hero_is_range, hands[1:], ghost_cards or '', opp_range, _opponent_range_bits(opp_range))
    eng = _lib.default_engine()
    if exact:
        rows = eng.exact_seats(q, ext, dealing)
    else:
        s, first = _take_ids(1)
        rows = eng.eval_batch_ext_seats(q, ext, s, first_query_id=first)
    return [float(x) for x in _lib.seat_shares(rows)[0, :players]]


def get_seat_equities_exact(hands, table_cards, players=None, ghost_cards=None, opponent_range=None, dealing="reference"):
    """get_seat_equities by enumeration with at most ONE random opponent (mcq_exact_batch_ext_seats): the exact pot shares
    of all `players` seats under `dealing` ('reference' or 'uniform') -- a list of `players` floats that sum to 1.
    hands[0] is the hero, the rest are the known hands, each two cards; `players` defaults to len(hands) (the all-in case)
    and may be len(hands) + 1: the last seat is then an opponent drawn from opponent_range (get_seat_equities'
    conventions; None = every class).  More than one random opponent or a hand given as a range raises ValueError: two
    random opponents have no per-seat enumeration, ranged hands are not enumerated at all.  No seed() state is used."""
    hands = [h if isinstance(h, (set, frozenset)) else list(h) for h in hands]
    if not 1 <= len(hands) <= 1 + _lib.MAX_KNOWN:
        raise ValueError("between one and ten hands")
    players = len(hands) if players is None else int(players)
    if not len(hands) <= players <= len(hands) + 1:
        raise ValueError("the per-seat enumeration takes at most one random opponent: players is len(hands) or len(hands) + 1")
    _two_cards_each(hands, "every hand is two cards here (ranged hands are not enumerated)")
    if dealing not in ("reference", "uniform"):
        raise ValueError("dealing must be 'reference' or 'uniform'")
    opp_range = 1 if opponent_range is None else opponent_range
    q = _query(hands[0], list(table_cards), players, 1)
    ext = _ext_record(hands[0], False, hands[1:], ghost_cards or '', opp_range, _opponent_range_bits(opp_range))
    rows = _lib.default_engine().exact_ext_seats(q, ext, dealing)
    return [float(x) for x in _lib.seat_shares(rows)[0, :players]]


_MULTI = {}   # tuple of device ordinals -> MultiEngine (made at first use, kept; its callers take turns on its lock)


def get_equity_batch(hole, board, n_players, runs, seed=None, first_query_id=0, mode=None, engine=None, n_gpus=None,
                     devices=None, ties="hero"):
    """Many states in one launch.

    hole [B,2] u8 card ids, board [B,5] u8 (0xFF = empty), n_players scalar or [B], runs scalar or [B].
    -> (equity[B] float64, tallies[B,13] uint64) with tally columns runs, passes, win, tie, by_type[9].
    Query i gets query id first_query_id + i: splitting a batch keeps every per-query tally identical.
    n_gpus > 1: the batch is sharded over the first n_gpus devices of the node -- counted from
    $MCQ_DEVICE / $LOCAL_RANK's device as the single-GPU path does -- by the library's multi-GPU entry (mcq_multi_*: one
    all-reduce of the integer tallies; production mode only); the tallies are the same integers as on one GPU, under the
    dealing law configure(dealing=...) has set.  devices=[...] names the shards' devices explicitly instead (one
    ordinal per shard, repeats allowed: several shards on one GPU).
    ties="split": the returned equity is hero's expected share of the pot (a tie among k hands counts 1/k) and the
    tallies are [B,22]: nine more columns, tie_ways[k - 2] for k = 2..10 hands sharing the pot (one GPU only).  The
    default "hero" credits ties to hero in full, as the reference does.
    STATUS of n_gpus > 1: untested on more than one distinct device (no multi-GPU node was reachable; the partitions,
    the same-device add and a one-rank RCCL communicator are tested on one GPU with devices=[0, 0, ...]).
    """
    split = _split_ties(ties, "hero")
    q = _lib.pack_queries(hole, board, n_players, runs)
    m = _state["mode"] if mode is None else _MODES[mode]
    if split and (devices is not None or (n_gpus is not None and int(n_gpus) > 1)):
        raise ValueError("ties='split' runs on one GPU (the multi-GPU entry has no split-pot rows)")
    if seed is None:
        s, base = _take_ids(len(q))
        first_query_id = base + first_query_id
    else:
        s = int(seed)
    if devices is None and n_gpus is not None and int(n_gpus) > 1:
        n_dev = _lib.load_library().mcq_device_count()
        if int(n_gpus) > n_dev:
            raise ValueError("n_gpus = %d, but %d HIP device(s) are visible" % (int(n_gpus), n_dev))
        dev0 = int(os.environ.get("MCQ_DEVICE", os.environ.get("LOCAL_RANK", "0"))) % max(n_dev, 1)
        devices = [(dev0 + k) % n_dev for k in range(int(n_gpus))]
    if devices is not None:
        if m != _lib.MODE_PHILOX or engine is not None:
            raise ValueError("n_gpus > 1 / devices: production mode on the library's own contexts only")
        key = tuple(int(d) for d in devices)
        with _lock:
            me = _MULTI.get(key)
            if me is None:
                me = _MULTI[key] = _lib.MultiEngine(list(key))
                if _lib.default_dealing_law() != "reference":
                    me.set_dealing_law(_lib.default_dealing_law())
        with me.lock:   # mcq_multi keeps per-call state: one call at a time per object
            res = me.eval_batch(q, s, first_query_id=first_query_id)
    else:
        eng = engine or _lib.default_engine()
        if split:
            res = eng.eval_batch_ways(q, s, first_query_id=first_query_id, mode=m)
            tallies = res.view(np.uint64).reshape(len(q), 22)
            return _lib.pot_share(tallies), tallies
        res = eng.eval_batch(q, s, first_query_id=first_query_id, mode=m)
    tallies = res.view(np.uint64).reshape(len(q), 13)
    runs_f = np.maximum(tallies[:, 0], 1).astype(np.float64)
    equity = (tallies[:, 2] + tallies[:, 3]).astype(np.float64) / runs_f
    return equity, tallies


def get_equity_exact(player_cards, table_cards, players, dealing="reference", engine=None, *, known_hands=(),
                     ghost_cards='', opponent_range=1, ties="credited"):
    """The number get_equity() converges to, by exhaustive enumeration on the GPU (1 to 3 players).

    dealing='reference': the exact expectation of tools/montecarlo_python.py's dealing (index bias included);
    'uniform': every remaining card equally likely (what montecarlo_cython.pyx / Montecarlo.cpp intend and
    tools/montecarlo_cpp/Test.cpp:176-217 checks within 1 %).  -> (equity, result row of integer weights).

    known_hands (further hands of two cards, in the order of original_player_card_list after the hero), ghost_cards and
    opponent_range follow run_montecarlo's conventions; `players` counts them all, and at most two of them may be random
    opponents (mcq_exact_batch_ext).  The row of weights is zero for a range with two random opponents: those outcomes
    have no common integer total, the equity is exact all the same.
    ties="split": the equity is hero's exact pot share and the row a RESULT_WAYS_DTYPE row of weights
    (mcq_exact_batch_ext_ways: at most ONE random opponent)."""
    split = _split_ties(ties)
    opp_bits = _opponent_range_bits(opponent_range)
    known_hands = [list(h) for h in known_hands]
    q = _query(list(player_cards), list(table_cards), players, 1)
    eng = engine or _lib.default_engine()
    if split:
        _two_cards_each(known_hands)
        ext = _ext_record(list(player_cards), False, known_hands, ghost_cards, opponent_range, opp_bits)
        _, weights = eng.exact_ext_ways(q, ext, dealing)
        return float(_lib.pot_share(weights)[0]), weights[0]
    if not known_hands and opp_bits is None and (ghost_cards == '' or ghost_cards is None):
        res = eng.exact(q, dealing)[0]
        return (int(res["win"]) + int(res["tie"])) / int(res["runs"]), res
    _two_cards_each(known_hands)
    ext = _ext_record(list(player_cards), False, known_hands, ghost_cards, opponent_range, opp_bits)
    prob, weights = eng.exact_ext(q, ext, dealing)
    return float(prob[0]["win"] + prob[0]["tie"]), weights[0]


_ROW_HANDS = [(a, b) for b in range(52) for a in range(b)]   # row _lib.hand_index(a, b) -> (a, b)


def get_range_equity_exact(hero_range, table_cards, opponent_range=1, dealing="reference", ghost_cards='', engine=None,
                           ties="credited"):
    """Exact equity of a hero RANGE against one random opponent, ranged or not, on the flop, turn or river: every hand
    of the range from one enumeration on the GPU (mcq_exact_batch_hero_range).

    hero_range and opponent_range follow run_montecarlo's conventions: a set of preflop class strings, or a number that
    keeps the top fraction of the 169 classes.  -> (equity, {(card, card): (equity_h, weight_h)}): per hand of the range
    that the remaining cards can make (card strings, lower card id first) its exact equity -- ties="credited": (win + tie) /
    runs as the reference credits a tie; ties="split": the heads-up pot share (win + tie / 2) / runs -- and how often
    `dealing` deals hero that hand in proportion; `equity` is their weighted mean, what run_montecarlo with a hero range
    converges to under dealing='reference'.  Preflop, further players and known hands raise ValueError."""
    _split_ties(ties)
    hero_bits = _opponent_range_bits(hero_range)
    if hero_bits is None:
        hero_bits = _lib.ALL_CLASSES
    opp_bits = _opponent_range_bits(opponent_range)
    board = [card_id(c) for c in table_cards]
    if len(board) > 5:
        raise ValueError("table_cards holds more than five cards")
    ghost = _ghost_ids(ghost_cards)
    q = _lib.pack_query_one([0, 0], board, 2, 1)
    ext = _lib.pack_query_ext(1, ghost=ghost, hero_range=hero_bits, opp_range=opp_bits)
    eng = engine or _lib.default_engine()
    rows, _ = eng.exact_hero_range(q, ext, dealing)
    return _range_rows_to_hands(rows[0], set(board) | set(ghost or []), dealing in ("uniform", 1), ties)


def quantise_weight(w):
    """A hand's weight in [0, 1] -> the integer 0..65535 the library works with: round(w * 65535).  A non-zero weight that
    would round to 0 (below 1 / 131070) raises ValueError: the hand would silently leave the range."""
    w = float(w)
    if not 0.0 <= w <= 1.0:
        raise ValueError("a weight is a number in [0, 1], not %r" % (w,))
    v = int(round(w * _lib.COMBO_WEIGHT_MAX))
    if v == 0 and w != 0.0:
        raise ValueError("the weight %r rounds to 0 of %d: give 0 to leave the hand out" % (w, _lib.COMBO_WEIGHT_MAX))
    return v


def _weighted_range(rng, what):
    """A range of get_range_equity_exact_weighted -> (class bits, weights[1, HAND_ROWS] uint16 or None for "every hand 1").
    A dict maps class strings ('AQO') and hands (('AH', 'KH')) to weights in [0, 1]: a hand's entry overrides its class's,
    whatever is not named weighs 0, and the class set is "every class" -- the weights alone define the range."""
    if not isinstance(rng, dict):
        bits = _opponent_range_bits(rng)
        return (_lib.ALL_CLASSES if bits is None else bits), None
    by_class, by_hand = {}, {}
    for key, w in rng.items():
        if isinstance(key, str):
            bit = _lib.class_bit(key)
            if bit is None:
                raise ValueError("%s: %r is no preflop class" % (what, key))
            by_class[bit] = quantise_weight(w)
        else:
            if len(key) != 2:
                raise ValueError("%s: a hand is two cards, not %r" % (what, key))
            by_hand[_lib.hand_index(card_id(key[0]), card_id(key[1]))] = quantise_weight(w)
    table = np.zeros((1, _lib.HAND_ROWS), np.uint16)
    for i, (a, b) in enumerate(_ROW_HANDS):
        table[0, i] = by_hand.get(i, by_class.get(_lib.class_bit(_hand_class(a, b)), 0))
    return _lib.ALL_CLASSES, table


def _seat_table(entry, what):
    """One seat of get_range_equities -> its weight table, uint16 [HAND_ROWS]: a two-card hand is one entry of
    COMBO_WEIGHT_MAX, a dict is what _weighted_range makes of it, a plain range (a set of classes, a top fraction) is the
    0/1 table of its class bits."""
    if isinstance(entry, (list, tuple)) and len(entry) == 2 and all(isinstance(c, str) and len(c) == 2 for c in entry) \
            and all(c[1] in "CDHS" for c in entry):
        a, b = card_id(entry[0]), card_id(entry[1])
        if a == b:
            raise ValueError("%s: a hand is two different cards, not %r" % (what, entry))
        table = np.zeros(_lib.HAND_ROWS, np.uint16)
        table[_lib.hand_index(a, b)] = _lib.COMBO_WEIGHT_MAX
        return table
    bits, table = _weighted_range(entry, what)
    if table is not None:
        return table[0]
    bits = np.asarray(bits, np.uint32)
    return np.array([(int(bits[bit >> 5]) >> (bit & 31)) & 1 for bit in
                     (_lib.class_bit(_hand_class(a, b)) for a, b in _ROW_HANDS)], np.uint16)


def _range_tables(ranges):
    """The seats of get_range_equities -> (tables uint16 [n_tables, HAND_ROWS], seat_table uint32 [1, 10]); seats whose
    tables are equal share one."""
    if not 2 <= len(ranges) <= 10:
        raise ValueError("between two and ten seats")
    tables, seen = [], {}
    seat_table = np.zeros((1, 10), np.uint32)
    for s, entry in enumerate(ranges):
        t = _seat_table(entry, "seat %d" % s)
        seat_table[0, s] = seen.setdefault(t.tobytes(), len(tables))
        if seat_table[0, s] == len(tables):
            tables.append(t)
    return np.stack(tables), seat_table


def get_range_equities(ranges, table_cards, runs=100000, *, engine=None):
    """Range against range against range: what the range of EVERY seat is worth on this board, by Monte Carlo
    (mcq_eval_batch_ranges).  `ranges` has one entry per seat, two to ten of them: a two-card hand (('AH', 'KH')), a range
    as run_montecarlo takes it -- a set of class strings or a top fraction, every hand of it weighing 1 -- or a dict of
    weights in [0, 1] by class ('AQO': 0.5) or by hand, as get_range_equity_exact_weighted takes it.  Seats with equal
    ranges share one table.  The hands of all seats are dealt JOINTLY: every deal of pairwise disjoint hands clear of the
    table cards is as likely as the product of its hands' weights -- symmetric in the seats, unlike a hero-first deal.
    -> ([(win, tie, share)] per seat, as fractions of `runs`; trials per iteration).  share is the seat's part of the pot,
    a tie among k hands counting 1 / k: the shares sum to 1.  One call takes one query id from the same seed() state as
    get_equity.  Seats whose ranges cannot be dealt together, or a seat without a hand clear of the table, raise
    ValueError."""
    ranges = list(ranges)
    tables, seat_table = _range_tables(ranges)
    board = [card_id(c) for c in table_cards]
    if len(board) > 5:
        raise ValueError("table_cards holds more than five cards")
    q = _lib.pack_query_one([0, 0], board, len(ranges), runs)
    eng = engine or _lib.default_engine()
    s, first = _take_ids(1)
    rows = eng.eval_batch_ranges(q, seat_table, tables, s, first_query_id=first)
    r, share = rows[0], _lib.seat_shares(rows)[0]
    n = float(r["runs"])
    return ([(float(r["seat"][k]["win"]) / n, float(r["seat"][k]["tie"]) / n, float(share[k])) for k in range(len(ranges))],
            float(r["passes"]) / n)


def get_range_hand_equities(ranges, table_cards, runs=100000, *, seat=0, engine=None):
    """get_range_equities with the breakdown by hand of one seat (mcq_eval_batch_ranges_hands): which hands of the range
    of seat `seat` carry its equity against these other ranges.  `ranges`, `table_cards`, `runs` and the seeding are those
    of get_range_equities: the same seed gives the same iterations.
    -> (seats, trials, per_hand): seats and trials as get_range_equities returns them, per_hand = {(card, card):
    (frequency, win, tie, pot_share)} for the hands the seat held at least once, lower card id first: frequency is the
    part of the iterations in which it held the hand; win, tie and pot_share are conditional on the hand."""
    ranges = list(ranges)
    tables, seat_table = _range_tables(ranges)
    if not 0 <= int(seat) < len(ranges):
        raise ValueError("seat %r: the seats are 0 .. %d" % (seat, len(ranges) - 1))
    board = [card_id(c) for c in table_cards]
    if len(board) > 5:
        raise ValueError("table_cards holds more than five cards")
    q = _lib.pack_query_one([0, 0], board, len(ranges), runs)
    eng = engine or _lib.default_engine()
    s, first = _take_ids(1)
    rows, hands = eng.eval_batch_ranges_hands(q, seat_table, tables, s, first_query_id=first, seat=int(seat))
    r, share, h = rows[0], _lib.seat_shares(rows)[0], hands[0]
    n = float(r["runs"])
    per_hand = {}
    for i in np.flatnonzero(h["runs"]):
        a, b = _ROW_HANDS[i]
        k = float(h["runs"][i])
        per_hand[(card_str(a), card_str(b))] = (k / n, float(h["win"][i]) / k, float(h["tie"][i]) / k,
                                                float(h["share"][i]) / (_lib.SHARE_UNIT * k))
    return ([(float(r["seat"][k]["win"]) / n, float(r["seat"][k]["tie"]) / n, float(share[k])) for k in range(len(ranges))],
            float(r["passes"]) / n, per_hand)


def get_range_equity_exact_weighted(hero, table_cards, opponent, ghost_cards='', engine=None, ties="credited"):
    """Exact equity of a WEIGHTED hero range against one opponent with a weighted range, on the flop, turn or river, every
    hand equally likely but for its weight (mcq_exact_batch_hero_range_weighted; the uniform law).

    hero and opponent are each a range as run_montecarlo takes it -- a set of class strings or a top fraction: every hand
    of it weighs 1 -- or a dict of weights in [0, 1] keyed by class string ('AQO': 0.5) or by hand (('AH', 'KH'): 1.0).  A
    hand's entry overrides its class's; whatever is not named weighs 0.  Weights are quantised to round(w * 65535)
    (quantise_weight; a non-zero weight that would become 0 raises ValueError).
    -> (equity, {(card, card): (equity_h, weight_h)}): per hero hand of positive weight that the remaining cards can make
    its exact equity against the weighted opponent -- ties as in get_range_equity_exact -- and its weight (the quantised
    one / 65535; 1.0 in a plain range); `equity` is their weighted mean.  Preflop raises ValueError, and so does a hero
    hand against which no opponent hand of positive weight is left."""
    _split_ties(ties)
    hero_bits, hero_w = _weighted_range(hero, "hero")
    opp_bits, opp_w = _weighted_range(opponent, "opponent")
    if opp_w is None:
        opp_w = np.ones((1, _lib.HAND_ROWS), np.uint16)
    board = [card_id(c) for c in table_cards]
    if len(board) > 5:
        raise ValueError("table_cards holds more than five cards")
    ghost = _ghost_ids(ghost_cards)
    q = _lib.pack_query_one([0, 0], board, 2, 1)
    ext = _lib.pack_query_ext(1, ghost=ghost, hero_range=hero_bits, opp_range=opp_bits)
    eng = engine or _lib.default_engine()
    rows, _ = eng.exact_hero_range_weighted(q, ext, opp_w, hero_w)
    return _weighted_rows_to_hands(rows[0], hero_w, ties)


def get_equity_matrix(table_cards, dead_cards='', engine=None):
    """The exact hand-against-hand matrix of a board with 3, 4 or 5 table cards (mcq_exact_matrix; heads-up, the uniform
    law): the table that the weighted range entries fold away.  table_cards and dead_cards are lists of card strings;
    dead_cards (any number, '' or None: none) leave the deck like ghost cards.
    -> (win, tie, total): uint16 arrays [1326, 1326] indexed by hand_index(card id, card id) on both axes -- win[h, g] = the
    table completions on which hand h beats hand g, tie[h, g] = those on which they are level -- and the completions of a
    pair of hands, total = win[h, g] + win[g, h] + tie[h, g] wherever h and g can both be dealt (they share no card and hold
    no table or dead card); every other entry is 0.  matrix_equity turns them into equities.  Preflop raises ValueError."""
    board = [card_id(c) for c in table_cards]
    if len(board) > 5:
        raise ValueError("table_cards holds more than five cards")
    dead = [card_id(c) for c in (dead_cards or [])]
    eng = engine or _lib.default_engine()
    win, tie, total = eng.exact_matrix(_lib.pack_matrix_query(board, dead))
    return win[0], tie[0], int(total[0])


def matrix_equity(win, tie, total, ties="split"):
    """get_equity_matrix's counts as a float64 matrix of the row hand's equity against the column hand: ties="split" the
    heads-up pot share (win + tie / 2) / total, ties="credited" (win + tie) / total as the reference credits a tie; NaN where
    the two hands cannot both be dealt."""
    split = _split_ties(ties)
    w, t = np.asarray(win, np.float64), np.asarray(tie, np.float64)
    dealt = (w + w.T + t) == float(total)
    eq = (w + (t / 2.0 if split else t)) / float(total)
    return np.where(dealt, eq, np.nan)


def _weighted_rows_to_hands(r, hero_w, ties):
    """The HAND_ROWS rows of one weighted record -> (equity, {(card, card): (equity_h, weight_h)}); hero_w = the hero's
    table [1, HAND_ROWS] or None (every hand 1)."""
    live = np.flatnonzero(r["runs"])
    tie = r["tie"][live].astype(np.float64)
    eq = (r["win"][live] + (tie / 2.0 if ties == "split" else tie)) / r["runs"][live]
    hands, num, den = {}, 0.0, 0.0
    for i, e in zip(live, eq):
        a, b = _ROW_HANDS[i]
        w = 1.0 if hero_w is None else int(hero_w[0, i]) / float(_lib.COMBO_WEIGHT_MAX)
        hands[(card_str(a), card_str(b))] = (float(e), w)
        num += w * float(e)
        den += w
    return num / den, hands


def _range_rows_to_hands(r, gone, uniform, ties):
    """The HAND_ROWS rows of one record -> (equity, {(card, card): (equity_h, weight_h)}); gone = the card ids that left
    the deck (table and ghost cards)."""
    live = np.flatnonzero(r["runs"])
    top = max(c for c in range(52) if c not in gone)
    tie = r["tie"][live].astype(np.float64)
    eq = (r["win"][live] + (tie / 2.0 if ties == "split" else tie)) / r["runs"][live]
    hands, num, den = {}, 0.0, 0.0
    for i, e in zip(live, eq):
        a, b = _ROW_HANDS[i]
        w = 1 if uniform or b == top else 2
        hands[(card_str(a), card_str(b))] = (float(e), w)
        num += w * float(e)
        den += w
    return num / den, hands


def _hand_class(a, b):
    """Preflop class string of the hand of card ids a, b: 'AA', 'AKS', 'AKO' -- the higher rank first."""
    from .cards import RANKS
    lo, hi = sorted((a >> 2, b >> 2))
    if lo == hi:
        return RANKS[hi] * 2
    return RANKS[hi] + RANKS[lo] + ("S" if (a & 3) == (b & 3) else "O")


def preflop_class_table(hands):
    """{(card, card): (equity, weight)} as get_preflop_range_equity_exact returns it -> {class string: (equity, weight)}:
    per preflop class its hands' total weight and their weighted mean equity."""
    num, den = {}, {}
    for (a, b), (e, w) in hands.items():
        c = _hand_class(card_id(a), card_id(b))
        num[c] = num.get(c, 0.0) + w * e
        den[c] = den.get(c, 0) + w
    return {c: (num[c] / den[c], den[c]) for c in den}


def get_preflop_range_equity_exact(hero_range, opponent_range=1, dealing="reference", ghost_cards='', engine=None,
                                   ties="credited", by_class=False):
    """Exact equity of a hero RANGE against one random opponent, ranged or not, BEFORE THE FLOP: every hand of the range
    from one enumeration of all table completions on the GPU (mcq_exact_batch_hero_range_preflop).  Narrow ranges take
    tens of milliseconds, every hand against every hand takes seconds.

    The arguments and the result are get_range_equity_exact's without table cards: -> (equity, {(card, card): (equity_h,
    weight_h)}).  by_class=True adds a third value, the 169-class table {class string: (equity, weight)}: per class of
    the range its hands' weighted mean equity and total weight under `dealing` (preflop_class_table)."""
    _split_ties(ties)
    if dealing not in ("reference", "uniform", 0, 1):
        raise ValueError("dealing must be 'reference' or 'uniform'")
    hero_bits = _opponent_range_bits(hero_range)
    if hero_bits is None:
        hero_bits = _lib.ALL_CLASSES
    if not np.asarray(hero_bits).any():
        raise ValueError("hero_range names no preflop class")
    opp_bits = _opponent_range_bits(opponent_range)
    ghost = _ghost_ids(ghost_cards, exactly_two=True)
    q = _lib.pack_query_one([0, 0], [], 2, 1)
    ext = _lib.pack_query_ext(1, ghost=ghost, hero_range=hero_bits, opp_range=opp_bits)
    eng = engine or _lib.default_engine()
    rows, _ = eng.exact_hero_range_preflop(q, ext, dealing)
    equity, hands = _range_rows_to_hands(rows[0], set(ghost or []), dealing in ("uniform", 1), ties)
    if by_class:
        return equity, hands, preflop_class_table(hands)
    return equity, hands


def get_preflop_range_equity_exact_weighted(hero, opponent, ghost_cards='', engine=None, ties="credited", by_class=False):
    """Exact equity of a WEIGHTED hero range against one opponent with a weighted range BEFORE THE FLOP, every hand equally
    likely but for its weight (mcq_exact_batch_hero_range_preflop_weighted; the uniform law): opening, 3-bet and calling
    ranges as mixed strategies.

    hero and opponent are given exactly as get_range_equity_exact_weighted takes them -- a set of class strings or a top
    fraction (every hand of it weighs 1), or a dict of weights in [0, 1] keyed by class string ('A5S': 0.4) or by hand
    (('AH', 'KH'): 1.0), quantised by quantise_weight.  -> (equity, {(card, card): (equity_h, weight_h)}) as that function
    returns it; by_class=True adds the class table {class string: (equity, weight)} of preflop_class_table.  A hero hand
    against which no opponent hand of positive weight is left raises ValueError."""
    _split_ties(ties)
    hero_bits, hero_w = _weighted_range(hero, "hero")
    opp_bits, opp_w = _weighted_range(opponent, "opponent")
    if not np.asarray(hero_bits).any():
        raise ValueError("hero names no preflop class")
    if opp_w is None:
        opp_w = np.ones((1, _lib.HAND_ROWS), np.uint16)
    ghost = _ghost_ids(ghost_cards, exactly_two=True)
    q = _lib.pack_query_one([0, 0], [], 2, 1)
    ext = _lib.pack_query_ext(1, ghost=ghost, hero_range=hero_bits, opp_range=opp_bits)
    eng = engine or _lib.default_engine()
    rows, _ = eng.exact_hero_range_preflop_weighted(q, ext, opp_w, hero_w)
    equity, hands = _weighted_rows_to_hands(rows[0], hero_w, ties)
    if by_class:
        return equity, hands, preflop_class_table(hands)
    return equity, hands


def get_runout_equities(player_cards, table_cards, players, dealing="reference", engine=None, *, known_hands=(),
                        ghost_cards=None, opponent_range=None, ties="credited", pairs=False):
    """Exact equity per RUNOUT on the flop or the turn: which cards help and how much, from one enumeration on the GPU
    (mcq_exact_batch_ext_runouts).

    The arguments are get_equity_exact's: known_hands (further hands of two cards), ghost_cards and opponent_range (None:
    every class) follow run_montecarlo's conventions, `players` counts every hand, and at most ONE of them may be a random
    opponent.  -> (equity, by_card): `equity` is what get_equity_exact returns for the same arguments, and by_card maps the
    card string of every card that can come next to (equity given that it comes next, probability that it comes next).
    pairs=True adds a third value that maps (card, card) -- lower card id first -- to (equity, probability) of that turn
    and river (empty on the turn, where by_card says it all).  ties="credited": (win + tie) / runs as the reference
    credits a tie; ties="split": hero's exact pot share.  Under dealing='reference' a card that would be the highest card
    left never comes (montecarlo_python.py:188) and is not listed.  Preflop, the river, two random opponents and ranged
    hands raise ValueError."""
    split = _split_ties(ties)
    if opponent_range is None:
        opponent_range = 1
    if ghost_cards is None:
        ghost_cards = ''
    known_hands = [list(h) for h in known_hands]
    _two_cards_each(known_hands)
    opp_bits = _opponent_range_bits(opponent_range)
    q = _query(list(player_cards), list(table_cards), players, 1)
    k = 5 - int(q["n_board"][0])
    ext = _ext_record(list(player_cards), False, known_hands, ghost_cards, opponent_range, opp_bits)
    eng = engine or _lib.default_engine()
    card_rows, pair_rows = eng.exact_ext_runouts(q, ext, dealing, want_pairs=bool(pairs))
    card_rows = card_rows[0].view(np.uint64).reshape(52, 22)

    def value(rows):
        """Equity of every weight row, exactly: the reference's credit or the pot share."""
        if split:
            return [float(v) for v in _lib.pot_share(rows, exact=True)]
        return [(int(r[2]) + int(r[3])) / max(int(r[0]), 1) for r in rows]

    total = card_rows.sum(axis=0) // np.uint64(k)       # the card rows of a flop hold every completion twice
    runs = int(total[0])
    equity = value(total.reshape(1, 22))[0]
    live = np.flatnonzero(card_rows[:, 0])
    by_card = {card_str(int(c)): (e, int(card_rows[c, 0]) / (k * runs)) for c, e in zip(live, value(card_rows[live]))}
    if not pairs:
        return equity, by_card
    pair_rows = pair_rows[0].view(np.uint64).reshape(_lib.HAND_ROWS, 22)
    live = np.flatnonzero(pair_rows[:, 0])
    by_pair = {(card_str(_ROW_HANDS[i][0]), card_str(_ROW_HANDS[i][1])): (e, int(pair_rows[i, 0]) / runs)
               for i, e in zip(live, value(pair_rows[live]))}
    return equity, by_card, by_pair
