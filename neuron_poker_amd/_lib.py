"""ctypes binding of libmcq_hip.so (C ABI: include/mcq.h).  No torch, no cffi.

The library is built in-tree by `python -m neuron_poker_amd.build` (or __graft_entry__.build()).  If it is
missing, or no HIP device can be opened, this module raises -- it never falls back to a CPU implementation.
"""
import ctypes as C
import importlib.util
import os
import struct
import sys
import threading

import numpy as np

MODE_PHILOX = 0
MODE_REPLAY_MT19937 = 1
MCQ_EINVAL, MCQ_EDEVICE, MCQ_ENOMEM, MCQ_EBUSY = -1, -2, -3, -4

QUERY_DTYPE = np.dtype([("hole", "u1", (2,)), ("board", "u1", (5,)), ("n_board", "u1"), ("n_players", "u1"),
                        ("reserved", "u1", (3,)), ("runs", "<u4")])
RESULT_DTYPE = np.dtype([("runs", "<u8"), ("passes", "<u8"), ("win", "<u8"), ("tie", "<u8"),
                         ("by_type", "<u8", (9,))])
# mcq_result_ways: the same 13 counters, then tie_ways[k - 2] = iterations in which k hands share the pot, k = 2..10
RESULT_WAYS_DTYPE = np.dtype(RESULT_DTYPE.descr + [("tie_ways", "<u8", (9,))])
# mcq_result_seats: runs, passes, then win / tie / share of every seat (seat 0 = hero, then the known hands, then the random
# or ranged opponents in dealing order); share counts SHARE_UNIT / k per iteration in which the seat is one of k best hands
SHARE_UNIT = 2520
SEAT_DTYPE = np.dtype([("win", "<u8"), ("tie", "<u8"), ("share", "<u8")])
RESULT_SEATS_DTYPE = np.dtype([("runs", "<u8"), ("passes", "<u8"), ("seat", SEAT_DTYPE, (10,))])
RESULT_SEATS = RESULT_SEATS_DTYPE
# mcq_hand_row: the iterations in which the watched seat of eval_batch_ranges_hands held one hand, and its increments in them
HAND_ROW_DTYPE = np.dtype([("runs", "<u8"), ("win", "<u8"), ("tie", "<u8"), ("share", "<u8")])
RANGES_HANDS_MAX_BATCH = 1024
KNOWN_HAND_DTYPE = np.dtype([("cards", "u1", (2,)), ("is_range", "u1"), ("reserved", "u1"), ("range", "<u4", (6,))])
MAX_KNOWN = 9
QUERY_EXT_DTYPE = np.dtype([("ghost", "u1", (2,)), ("hero_is_range", "u1"), ("n_known", "u1"), ("opp_range", "<u4", (6,)),
                            ("hero_range", "<u4", (6,)), ("known", KNOWN_HAND_DTYPE, (MAX_KNOWN,))])
TABLES_CONFIG_DTYPE = np.dtype([("n_tables", "<u4"), ("n_seats", "<u4"), ("runs", "<u4"), ("max_raises", "<u4"),
                                ("initial_stacks", "<f8"), ("small_blind", "<f8"), ("big_blind", "<f8"),
                                ("seed", "<u8"), ("seat_kind", "u1", (10,)), ("reserved", "u1", (6,)),
                                ("min_call_equity", "<f8", (10,)), ("min_bet_equity", "<f8", (10,))])
EXACT_PROB_DTYPE = np.dtype([("win", "<f8"), ("tie", "<f8"), ("by_type", "<f8", (9,))])
assert TABLES_CONFIG_DTYPE.itemsize == 224 and EXACT_PROB_DTYPE.itemsize == 88
assert QUERY_DTYPE.itemsize == 16 and RESULT_DTYPE.itemsize == 104 and QUERY_EXT_DTYPE.itemsize == 304
assert RESULT_WAYS_DTYPE.itemsize == 176
# mcq_exact_prob_ways: mcq_exact_prob, then tie_ways[k - 2] = P(k hands share the pot)
EXACT_PROB_WAYS_DTYPE = np.dtype([("p", EXACT_PROB_DTYPE), ("tie_ways", "<f8", (9,))])
assert EXACT_PROB_WAYS_DTYPE.itemsize == 160
ALL_CLASSES = np.array([0xFFFFFFFF] * 5 + [0x1FF], np.uint32)  # 169 bits

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_lock = threading.Lock()


class McqError(RuntimeError):
    """HIP / allocation failure reported by libmcq_hip.so (MCQ_EDEVICE, MCQ_ENOMEM)."""


class McqBusyError(McqError):
    """MCQ_EBUSY: a second call on a context (Engine / MultiEngine) while one is running on it -- a context allows ONE
    call in flight; use one Engine per thread (default_engine() does)."""


def library_path():
    return os.environ.get("MCQ_LIBRARY", os.path.join(_HERE, "libmcq_hip.so"))


def _share_hip_runtime_with_torch():
    """One process must hold ONE HIP/HSA runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7, the same as /opt/rocm's); if libmcq_hip.so bound the system copy and torch were imported
    afterwards, the second runtime would find no GPU.  So when a torch wheel with a bundled runtime is
    installed, that copy is mapped first and libmcq_hip.so resolves to it by SONAME.  MCQ_HIP_RUNTIME=system
    opts out (processes that never import torch)."""
    if os.environ.get("MCQ_HIP_RUNTIME", "auto") == "system" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


# The prototypes of include/mcq.h, in the header's order: (name, return type, argument types...).  Every pointer is a
# c_void_p (None = NULL), mcq_version's excepted.  tests/test_binding.py holds the table to the header type by type.
_I, _U32, _U64, _SZ, _P = C.c_int, C.c_uint32, C.c_uint64, C.c_size_t, C.c_void_p
_PROTOTYPES = (
    ("mcq_device_count", _I),
    ("mcq_create", _P, _I, _I),
    ("mcq_destroy", None, _P),
    ("mcq_eval_batch", _I, _P, _P, _SZ, _U64, _U64, _I, _P),
    ("mcq_eval_one", _I, _P, _P, _U64, _I, _P),
    ("mcq_eval_batch_ext", _I, _P, _P, _P, _SZ, _U64, _U64, _I, _P),
    ("mcq_eval_batch_ext_ways", _I, _P, _P, _P, _SZ, _U64, _U64, _I, _P),
    ("mcq_eval_batch_ext_seats", _I, _P, _P, _P, _SZ, _U64, _U64, _I, _P),
    ("mcq_eval_batch_numpy_stream", _I, _P, _P, _SZ, _P, _P, _P),
    ("mcq_eval_batch_device", _I, _P, _P, _SZ, _U64, _U64, _P, _P),
    ("mcq_eval_batch_device_small", _I, _P, _P, _SZ, _U64, _U64, _P, _P),
    ("mcq_eval_batch_ways", _I, _P, _P, _SZ, _U64, _U64, _I, _P),
    ("mcq_eval_batch_device_ways", _I, _P, _P, _SZ, _U64, _U64, _P, _P),
    ("mcq_showdown", _I, _P, _P, _SZ, _I, _P, _P, _P),
    ("mcq_eval_batch_part", _I, _P, _P, _SZ, _U64, _U64, _U32, _U32, _P),
    ("mcq_exact_batch", _I, _P, _P, _SZ, _I, _P),
    ("mcq_exact_batch_ext", _I, _P, _P, _P, _SZ, _I, _P, _P),
    ("mcq_exact_batch_ext_ways", _I, _P, _P, _P, _SZ, _I, _P, _P),
    ("mcq_exact_batch_seats", _I, _P, _P, _P, _SZ, _I, _P),
    ("mcq_exact_batch_ext_seats", _I, _P, _P, _P, _SZ, _I, _P),
    ("mcq_exact_batch_hero_range", _I, _P, _P, _P, _SZ, _I, _P, _P),
    ("mcq_exact_batch_hero_range_weighted", _I, _P, _P, _P, _SZ, _P, _P, _P, _P),
    ("mcq_exact_batch_hero_range_preflop", _I, _P, _P, _P, _SZ, _I, _P, _P),
    ("mcq_exact_batch_hero_range_preflop_weighted", _I, _P, _P, _P, _SZ, _P, _P, _P, _P),
    ("mcq_eval_batch_ranges", _I, _P, _P, _P, _P, _SZ, _SZ, _U64, _U64, _P),
    ("mcq_eval_batch_ranges_hands", _I, _P, _P, _P, _P, _SZ, _SZ, _U64, _U64, _U32, _P, _P),
    ("mcq_exact_batch_ext_runouts", _I, _P, _P, _P, _SZ, _I, _P, _P),
    ("mcq_exact_matrix", _I, _P, _P, _SZ, _P, _P, _P),
    ("mcq_exact_matrix_device", _I, _P, _P, _SZ, _P, _P, _P, _P),
    ("mcq_set_dealing_law", _I, _P, _I),
    ("mcq_set_kernel_timing", _I, _P, _I),
    ("mcq_kernel_times", _I, _P, _P, _I),
    ("mcq_last_kernel_ms", C.c_float, _P),
    ("mcq_tables_create", _P, _P, _P),
    ("mcq_tables_destroy", None, _P),
    ("mcq_tables_begin", _SZ, _P, _P),
    ("mcq_tables_resume", _I, _P, _P),
    ("mcq_tables_run", _I, _P, _U32, _P),
    ("mcq_tables_stats", None, _P, _P),
    ("mcq_tables_state", _I, _P, _U32, _P, _P),
    ("mcq_multi_create", _P, _P, _I, _I),
    ("mcq_multi_destroy", None, _P),
    ("mcq_multi_eval_batch", _I, _P, _P, _SZ, _U64, _U64, _I, _P),
    ("mcq_multi_eval_batch_device", _I, _P, _P, _SZ, _U64, _U64, _I, _P),
    ("mcq_multi_set_dealing_law", _I, _P, _I),
    ("mcq_multi_info", _I, _P, _P),
    ("mcq_multi_times", _I, _P, _P),
    ("mcq_last_error", C.c_char_p),
    ("mcq_version", None, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)),
)


def load_library():
    """Load libmcq_hip.so and declare the prototypes of include/mcq.h.  Loud failure if it is not built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not os.path.exists(path):
            raise ImportError("%s not found: build it with `python -m neuron_poker_amd.build` (hipcc, gfx950). "
                              "neuron_poker_amd has no CPU fallback." % path)
        _share_hip_runtime_with_torch()
        L = C.CDLL(path)
        for name, restype, *argtypes in _PROTOTYPES:
            fn = getattr(L, name)   # AttributeError names a symbol the library lacks
            fn.argtypes, fn.restype = argtypes, restype
        _lib = L
        return _lib


def _last_error():
    """mcq_last_error() of the calling thread as text ('' when there is none).  The loaded library is read without _lock:
    set_default_dealing_law and default_engine report an engine's error while they hold it."""
    return ((_lib or load_library()).mcq_last_error() or b"").decode("utf-8", "replace")


def _raise(rc):
    msg = _last_error()
    if rc == MCQ_EINVAL:
        raise ValueError(msg)
    if rc == MCQ_EBUSY:
        raise McqBusyError(msg)
    raise McqError("libmcq_hip error %d: %s" % (rc, msg))


# What every method of Engine, MultiEngine and Tables marshals its arguments with.  The checks raise before the engine is
# touched; a method checks the law first, then the records, then its tables.

def _call(fn, *args):
    """Call an entry point that returns MCQ_OK or an MCQ_E* code; the code is raised as _raise maps it."""
    rc = fn(*args)
    if rc:
        _raise(rc)


def _law_code(law):
    code = {"reference": 0, "uniform": 1, 0: 0, 1: 1}.get(law)
    if code is None:
        raise ValueError("law must be 'reference' or 'uniform'")
    return code


def _queries(queries, dtype=QUERY_DTYPE):
    """-> the records as one contiguous row of `dtype`"""
    return np.ascontiguousarray(queries, dtype=dtype).reshape(-1)


def _records(queries, ext):
    """-> (mcq_query[n], mcq_query_ext[n]), one extension record per query"""
    q, e = _queries(queries), _queries(ext, QUERY_EXT_DTYPE)
    if len(e) != len(q):
        raise ValueError("one mcq_query_ext per query")
    return q, e


def _u64(x):
    """a seed or a query id as the uint64_t the library takes"""
    return int(x) & 0xFFFFFFFFFFFFFFFF


def _opt(x):
    """an optional device pointer or stream handle: None (NULL) for None or 0"""
    return int(x) if x else None


def _addr(a):
    """the address of an optional array: None (NULL) for None"""
    return None if a is None else a.ctypes.data


def pack_queries(hole, board, n_players, runs):
    """Build mcq_query records.  hole [B,2] card ids; board [B,5] card ids, 0xFF = absent (any position: the
    known cards are left-packed here); n_players, runs scalar or [B]."""
    hole = np.asarray(hole, dtype=np.uint8).reshape(-1, 2)
    B = len(hole)
    board = np.asarray(board, dtype=np.uint8).reshape(B, 5)
    q = np.zeros(B, QUERY_DTYPE)
    q["hole"] = hole
    present = board != 255
    order = np.argsort(~present, axis=1, kind="stable")
    packed = np.take_along_axis(board, order, axis=1)
    nb = present.sum(1).astype(np.uint8)
    packed[np.arange(5)[None, :] >= nb[:, None]] = 0
    q["board"] = packed
    q["n_board"] = nb
    npl = np.broadcast_to(np.asarray(n_players), (B,))
    if (npl < 0).any() or (npl > 255).any():
        raise ValueError("n_players out of range")
    q["n_players"] = npl.astype(np.uint8)
    r = np.broadcast_to(np.asarray(runs), (B,))
    if (r < 0).any() or (r > 0xffffffff).any():
        raise ValueError("runs out of range")
    q["runs"] = r.astype(np.uint32)
    return q


def pot_share(rows, exact=False):
    """Hero's expected share of the pot, float64 [n], from rows of RESULT_WAYS_DTYPE (or an [n, 22] integer matrix):
    (win + sum_k tie_ways[k - 2] / k) / runs, k = 2..10 hands sharing the pot.  The reference's equity credits every tie
    to hero in full: (win + tie) / runs.  The rows may be Monte-Carlo tallies or the integer weights of
    Engine.exact_ext_ways; exact=True returns a list of fractions.Fraction instead, exact for such weights."""
    t = np.ascontiguousarray(rows)
    if exact:
        from fractions import Fraction
        if t.dtype == RESULT_WAYS_DTYPE:
            t = t.view(np.uint64)
        return [(int(r[2]) + sum(Fraction(int(r[13 + j]), j + 2) for j in range(9))) / max(int(r[0]), 1)
                for r in t.reshape(-1, 22)]
    if t.dtype == RESULT_WAYS_DTYPE:
        t = t.view(np.uint64)
    t = t.reshape(-1, 22).astype(np.float64)
    return (t[:, 2] + (t[:, 13:22] / np.arange(2, 11, dtype=np.float64)).sum(1)) / np.maximum(t[:, 0], 1.0)


def seat_shares(rows, n_players=None):
    """Pot share of every seat, float64 [B, 10], from rows of RESULT_SEATS_DTYPE (or a [B, 32] integer matrix) -- Monte-Carlo
    tallies of Engine.eval_batch_ext_seats or the integer weights of Engine.exact_seats alike: share / (SHARE_UNIT * runs).
    The columns of the seats nobody sits in (at or above a query's n_players) are 0.0 when n_players is None, as the rows
    hold them, and NaN when n_players (one number, or one per row) is passed."""
    t = np.ascontiguousarray(rows)
    if t.dtype == RESULT_SEATS_DTYPE:
        t = t.view(np.uint64)
    t = t.reshape(-1, 32)
    out = t[:, 4::3].astype(np.float64) / (float(SHARE_UNIT) * np.maximum(t[:, :1].astype(np.float64), 1.0))
    if n_players is not None:
        n = np.broadcast_to(np.asarray(n_players, np.int64).reshape(-1, 1), (len(out), 1))
        out[np.arange(10)[None, :] >= n] = np.nan
    return out


def pack_query_one(hole, board, n_players, runs):
    """One mcq_query record without the numpy machinery of pack_queries (the per-call path of get_equity):
    hole = two card ids, board = up to five card ids (left-packed as given)."""
    nb = len(board)
    if len(hole) != 2 or nb > 5:
        raise ValueError("two hole cards and at most five table cards")
    try:
        raw = struct.pack("<2B5BBB3xI", hole[0], hole[1], *(list(board) + [0] * (5 - nb)), nb, n_players, runs)
    except struct.error as e:
        raise ValueError("card id, n_players or runs out of range: %s" % e)
    return np.frombuffer(bytearray(raw), QUERY_DTYPE)  # writable


HAND_ROWS = 1326   # C(52, 2): MCQ_HAND_ROWS
HERO_PREFLOP_MAX_BATCH = 64   # MCQ_HERO_PREFLOP_MAX_BATCH
COMBO_WEIGHT_MAX = 65535      # MCQ_COMBO_WEIGHT_MAX
RUNOUT_CARD_ROWS = 52     # MCQ_RUNOUT_CARD_ROWS
RUNOUT_MAX_BATCH = 1024   # MCQ_RUNOUT_MAX_BATCH
MATRIX_MAX_BATCH = 256    # MCQ_MATRIX_MAX_BATCH
# mcq_matrix_query: a board of 3 to 5 table cards and a mask of dead cards (bit c: card id c is out of the deck)
MATRIX_QUERY_DTYPE = np.dtype([("board", "u1", (5,)), ("n_board", "u1"), ("reserved", "u1", (2,)), ("dead", "<u8")])
assert MATRIX_QUERY_DTYPE.itemsize == 16


def pack_matrix_query(board, dead=()):
    """One MATRIX_QUERY_DTYPE record from card ids: `board` the 3 to 5 table cards, `dead` the cards out of the deck."""
    board = [int(c) for c in board]
    if not 0 <= len(board) <= 5 or any(not 0 <= c < 256 for c in board):
        raise ValueError("a board is at most five card ids")
    q = np.zeros(1, MATRIX_QUERY_DTYPE)
    q["board"][0, :len(board)] = board
    q["n_board"] = len(board)
    mask = 0
    for c in dead:
        if not 0 <= int(c) < 64:
            raise ValueError("a dead card is a card id")
        mask |= 1 << int(c)
    q["dead"] = mask
    return q


def hand_index(a, b):
    """Row of the two-card hand {a, b} (card ids) among the HAND_ROWS rows of Engine.exact_hero_range: MCQ_HAND_INDEX."""
    a, b = int(a), int(b)
    if a == b or not (0 <= a < 52 and 0 <= b < 52):
        raise ValueError("a hand is two different card ids below 52")
    lo, hi = min(a, b), max(a, b)
    return hi * (hi - 1) // 2 + lo


def class_bit(name):
    """Bit of a preflop class string ('AKS', 'KAO', 'TT', ...) in a 169-bit range set; None if the string can never
    equal what get_two_short_notation produces (tools/montecarlo_python.py:24-34)."""
    from .cards import RANKS
    if not isinstance(name, str) or len(name) < 2:
        return None
    r1, r2 = RANKS.find(name[0]), RANKS.find(name[1])
    if r1 < 0 or r2 < 0:
        return None
    if r1 == r2:
        return 14 * r1 if len(name) == 2 else None
    if len(name) != 3 or name[2] not in "SO":
        return None
    lo, hi = min(r1, r2), max(r1, r2)
    return 13 * lo + hi if name[2] == "S" else 13 * hi + lo


def range_bits(classes):
    """169-bit set (6 little-endian uint32 words) of a collection of preflop class strings."""
    w = np.zeros(6, np.uint32)
    for c in classes:
        b = class_bit(c)
        if b is not None:
            w[b >> 5] |= np.uint32(1 << (b & 31))
    return w


def pack_query_ext(n, ghost=None, known2=None, hero_range=None, opp_range=None, known=None):
    """n mcq_query_ext records with the same settings.  ghost = two card ids or None; hero_range / opp_range = 6-word
    sets (range_bits) or None (hero given as cards / every class); known = the further known hands in the order of
    original_player_card_list, each two card ids or a 6-word set (known2 = one hand of two cards, kept for brevity)."""
    e = np.zeros(n, QUERY_EXT_DTYPE)
    e["ghost"] = 255 if ghost is None else np.asarray(ghost, np.uint8)
    e["hero_is_range"] = 0 if hero_range is None else 1
    e["hero_range"] = 0 if hero_range is None else np.asarray(hero_range, np.uint32)
    e["opp_range"] = ALL_CLASSES if opp_range is None else np.asarray(opp_range, np.uint32)
    hands = ([known2] if known2 is not None else []) + list(known or [])
    if len(hands) > MAX_KNOWN:
        raise ValueError("at most %d known hands besides the hero" % MAX_KNOWN)
    e["n_known"] = len(hands)
    for k, h in enumerate(hands):
        h = np.asarray(h)
        if h.size == 2:
            e["known"]["cards"][:, k] = h.astype(np.uint8)
        elif h.size == 6:
            e["known"]["is_range"][:, k] = 1
            e["known"]["range"][:, k] = h.astype(np.uint32)
        else:
            raise ValueError("a known hand is two card ids or a 6-word range set")
    return e


def _hero_weight_table(name, w, n):
    """a weight table of exact_hero_range*_weighted: uint16 [n, HAND_ROWS], contiguous"""
    if not isinstance(w, np.ndarray) or w.dtype != np.uint16 or w.shape != (n, HAND_ROWS):
        raise ValueError("%s is a uint16 array of shape [n, HAND_ROWS] = (%d, %d)" % (name, n, HAND_ROWS))
    return np.ascontiguousarray(w)


def _hero_range(eng, entry, queries, ext, law=None, weights=None):
    """What the four Engine.exact_hero_range* methods share: the law (weights is None) or the (opp_weights, hero_weights)
    tables, the records, the output arrays, the call of the library's `entry`.  Every ValueError is raised before the
    engine is touched.  -> (rows, agg)"""
    if weights is None:
        code = _law_code(law)
    q, e = _records(queries, ext)
    if weights is None:
        mid = (code,)
    else:
        opp = _hero_weight_table("opp_weights", weights[0], len(q))
        hero = None if weights[1] is None else _hero_weight_table("hero_weights", weights[1], len(q))
        mid = (opp.ctypes.data, _addr(hero))
    rows = np.zeros((len(q), HAND_ROWS), RESULT_DTYPE)
    agg = np.zeros(len(q), EXACT_PROB_DTYPE)
    _call(getattr(eng._lib, entry), eng._ctx, q.ctypes.data, e.ctypes.data, len(q), *mid, rows.ctypes.data, agg.ctypes.data)
    return rows, agg


class _Handle:
    """What Engine, MultiEngine and Tables share: the library in `_lib` and one native object, held in the attribute that
    `_handle` names and freed by the entry point that `_destroy` names, at close() or when the object is collected."""
    _handle = _destroy = None

    def close(self):
        if getattr(self, self._handle, None):
            getattr(self._lib, self._destroy)(getattr(self, self._handle))
            setattr(self, self._handle, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(_Handle):
    """One mcq_ctx: an equity engine bound to one GPU.  Not re-entrant: one call in flight per engine -- a second thread
    calling into the same Engine meanwhile gets McqBusyError (the library checks).  One Engine per thread."""
    _handle, _destroy = "_ctx", "mcq_destroy"

    def __init__(self, device=0, kernel_times=False):
        self._lib = load_library()
        self._ctx = self._lib.mcq_create(int(device), 0)
        if not self._ctx:
            raise McqError("mcq_create(device=%d) failed: %s" % (device, _last_error()))
        self.device = int(device)
        if kernel_times:
            self.set_kernel_timing(True)

    def set_kernel_timing(self, on):
        """Timestamp every evaluation-kernel launch (kernel_times / last_kernel_ms); off by default: it costs a small
        query about 6 us of its call time."""
        _call(self._lib.mcq_set_kernel_timing, self._ctx, 1 if on else 0)

    def set_dealing_law(self, law):
        """'reference' (default: the Python reference's law incl. its index bias) or 'uniform' (unbiased)."""
        code = _law_code(law)
        _call(self._lib.mcq_set_dealing_law, self._ctx, code)

    def eval_batch(self, queries, seed, first_query_id=0, mode=MODE_PHILOX, part=None):
        """queries: array of QUERY_DTYPE (host).  -> array of RESULT_DTYPE.
        part=(p, n): only share p of n of every query's iterations (mcq_eval_batch_part; the rows of all shares
        add up to the unsplit result)."""
        q = _queries(queries)
        out = np.empty(len(q), RESULT_DTYPE)   # every row is written by the library on success; on failure we raise
        if part is not None:
            if mode != MODE_PHILOX:
                raise ValueError("only the production mode can split the iterations of a query")
            _call(self._lib.mcq_eval_batch_part, self._ctx, q.ctypes.data, len(q), _u64(seed), _u64(first_query_id),
                  int(part[0]), int(part[1]), out.ctypes.data)
        else:
            _call(self._lib.mcq_eval_batch, self._ctx, q.ctypes.data, len(q), _u64(seed), _u64(first_query_id), int(mode),
                  out.ctypes.data)
        return out

    def eval_batch_ways(self, queries, seed, first_query_id=0, mode=MODE_PHILOX):
        """eval_batch with the ties split by the number of hands that share the pot (mcq_eval_batch_ways).
        -> array of RESULT_WAYS_DTYPE: the fields of RESULT_DTYPE exactly as eval_batch returns them, then tie_ways[9];
        pot_share(rows) is hero's expected share of the pot."""
        q = _queries(queries)
        out = np.empty(len(q), RESULT_WAYS_DTYPE)   # every row is written by the library on success; on failure we raise
        _call(self._lib.mcq_eval_batch_ways, self._ctx, q.ctypes.data, len(q), _u64(seed), _u64(first_query_id), int(mode),
              out.ctypes.data)
        return out

    def exact(self, queries, law="reference"):
        """Exact enumeration (1..3 players; `runs` of the queries is ignored).  -> RESULT_DTYPE rows of integer
        weights: runs = total weight, equity = (win + tie) / runs exactly."""
        code = _law_code(law)
        q = _queries(queries)
        out = np.zeros(len(q), RESULT_DTYPE)
        _call(self._lib.mcq_exact_batch, self._ctx, q.ctypes.data, len(q), code, out.ctypes.data)
        return out

    def exact_ext(self, queries, ext, law="reference"):
        """Exact enumeration of extended queries (mcq_exact_batch_ext: further known hands, ghost cards, an opponent range;
        at most two random opponents).  -> (prob, weights): EXACT_PROB_DTYPE rows (win, tie, by_type) and RESULT_DTYPE
        rows of integer weights -- zeroed for a query with a range and two random opponents (no common total)."""
        code = _law_code(law)
        q, e = _records(queries, ext)
        prob = np.zeros(len(q), EXACT_PROB_DTYPE)
        weights = np.zeros(len(q), RESULT_DTYPE)
        _call(self._lib.mcq_exact_batch_ext, self._ctx, q.ctypes.data, e.ctypes.data, len(q), code, prob.ctypes.data,
              weights.ctypes.data)
        return prob, weights

    def exact_hero_range(self, queries, ext, law="reference"):
        """Exact range against range, postflop and heads-up (mcq_exact_batch_hero_range): records with hero_is_range = 1,
        no known hands, one random opponent drawn from opp_range, 3 to 5 table cards.  -> (rows, agg): rows[n, HAND_ROWS]
        of RESULT_DTYPE -- row hand_index(a, b) holds, for every hand of the hero's range that the deck can make, the
        integer weights exact_ext gives the same record with the hero holding a and b, every other row is zero -- and
        agg[n] of EXACT_PROB_DTYPE, the rows combined with the weights by which the law deals hero his hands."""
        return _hero_range(self, "mcq_exact_batch_hero_range", queries, ext, law=law)

    def exact_hero_range_weighted(self, queries, ext, opp_weights, hero_weights=None):
        """exact_hero_range with a weight per HAND on both sides, under the uniform law
        (mcq_exact_batch_hero_range_weighted).  opp_weights and hero_weights are uint16 arrays [n, HAND_ROWS] indexed by
        hand_index(a, b); hero_weights=None weighs every hand of the hero's classes 1.  The class sets of the records stay
        in force (a hand outside its set weighs 0).  -> (rows, agg) laid out as exact_hero_range's: per hero hand of
        positive weight runs = the opponent's total weight, win, tie and by_type its parts; agg combines the rows with the
        hero's weights.  A wrong shape or dtype raises ValueError."""
        return _hero_range(self, "mcq_exact_batch_hero_range_weighted", queries, ext, weights=(opp_weights, hero_weights))

    def exact_hero_range_preflop(self, queries, ext, law="reference"):
        """Exact range against range BEFORE THE FLOP, heads-up (mcq_exact_batch_hero_range_preflop): records without
        table cards, hero_is_range = 1, no known hands, one random opponent drawn from opp_range; at most
        HERO_PREFLOP_MAX_BATCH of them.  -> (rows, agg) laid out as exact_hero_range's.  A record takes from tens of
        milliseconds (narrow ranges) to seconds (every hand against every hand)."""
        return _hero_range(self, "mcq_exact_batch_hero_range_preflop", queries, ext, law=law)

    def exact_hero_range_preflop_weighted(self, queries, ext, opp_weights, hero_weights=None):
        """exact_hero_range_preflop with a weight per HAND on both sides, under the uniform law
        (mcq_exact_batch_hero_range_preflop_weighted): records without table cards, at most HERO_PREFLOP_MAX_BATCH of
        them; opp_weights and hero_weights as exact_hero_range_weighted takes them -- uint16 arrays [n, HAND_ROWS] indexed
        by hand_index(a, b), hero_weights=None weighs every hand of the hero's classes 1, the class sets stay in force.
        -> (rows, agg) laid out as exact_hero_range_weighted's.  A wrong shape or dtype raises ValueError, and so does a
        hero hand of positive weight against which no opponent hand of positive weight is left (seen before anything is
        launched)."""
        return _hero_range(self, "mcq_exact_batch_hero_range_preflop_weighted", queries, ext,
                           weights=(opp_weights, hero_weights))

    def exact_ext_ways(self, queries, ext, law="reference"):
        """exact_ext with the ties split by the hands that share the pot (mcq_exact_batch_ext_ways; at most ONE random
        opponent).  -> (prob, weights): EXACT_PROB_WAYS_DTYPE rows (p as exact_ext's prob, tie_ways[9]) and
        RESULT_WAYS_DTYPE rows of integer weights, always defined; pot_share(weights, exact=True) is the exact share."""
        code = _law_code(law)
        q, e = _records(queries, ext)
        prob = np.zeros(len(q), EXACT_PROB_WAYS_DTYPE)
        weights = np.zeros(len(q), RESULT_WAYS_DTYPE)
        _call(self._lib.mcq_exact_batch_ext_ways, self._ctx, q.ctypes.data, e.ctypes.data, len(q), code, prob.ctypes.data,
              weights.ctypes.data)
        return prob, weights

    def exact_ext_runouts(self, queries, ext, law="reference", want_pairs=True):
        """Exact equity per runout on the flop and the turn (mcq_exact_batch_ext_runouts; what exact_ext_ways accepts, with 3
        or 4 table cards).  -> (cards[n, 52], pairs[n, HAND_ROWS] or None) of RESULT_WAYS_DTYPE: the integer weights of
        exact_ext_ways restricted to the table completions that hold the card (flop: the pair; the card rows are the sums
        of their pair rows).  The rows of what cannot come are zero; a turn record's pair rows are all zero.  Equity given
        that card c comes next: (win + tie) / runs of cards[i, c], or pot_share of that row."""
        code = _law_code(law)
        q, e = _records(queries, ext)
        cards = np.zeros((len(q), RUNOUT_CARD_ROWS), RESULT_WAYS_DTYPE)
        pairs = np.zeros((len(q), HAND_ROWS), RESULT_WAYS_DTYPE) if want_pairs else None
        _call(self._lib.mcq_exact_batch_ext_runouts, self._ctx, q.ctypes.data, e.ctypes.data, len(q), code, cards.ctypes.data,
              _addr(pairs))
        return cards, pairs

    def eval_batch_ext_ways(self, queries, ext, seed, first_query_id=0, mode=MODE_PHILOX):
        """eval_batch_ext with the ties split by the hands that share the pot (mcq_eval_batch_ext_ways).  -> array of
        RESULT_WAYS_DTYPE: the fields of RESULT_DTYPE exactly as eval_batch_ext returns them, then tie_ways[9]."""
        q, e = _records(queries, ext)
        out = np.zeros(len(q), RESULT_WAYS_DTYPE)
        _call(self._lib.mcq_eval_batch_ext_ways, self._ctx, q.ctypes.data, e.ctypes.data, len(q), _u64(seed),
              _u64(first_query_id), int(mode), out.ctypes.data)
        return out

    def eval_batch_ext_seats(self, queries, ext, seed, first_query_id=0):
        """eval_batch_ext with one tally per SEAT (mcq_eval_batch_ext_seats; production mode): every hand's win, tie and
        pot share from the same iterations.  -> array of RESULT_SEATS_DTYPE; runs, passes and seat 0's win and tie are
        what eval_batch_ext_ways returns for the same arguments; seat_shares(rows) gives the pot shares."""
        q, e = _records(queries, ext)
        out = np.zeros(len(q), RESULT_SEATS_DTYPE)
        _call(self._lib.mcq_eval_batch_ext_seats, self._ctx, q.ctypes.data, e.ctypes.data, len(q), _u64(seed),
              _u64(first_query_id), MODE_PHILOX, out.ctypes.data)
        return out

    def eval_batch_ranges(self, queries, seat_table, tables, seed, first_query_id=0):
        """Monte-Carlo multiway equity with a weighted range per SEAT (mcq_eval_batch_ranges): record i seats n_players
        ranges, seat s holding tables[seat_table[i, s]] -- uint16 weights [n_tables, HAND_ROWS] indexed by hand_index(a, b),
        shared by index; seat_table is uint32 [n, 10], its entries at or above n_players are ignored.  The hands are dealt
        jointly, proportional to the product of the seats' weights over the disjoint deals clear of the table cards; `hole`
        of the records is not read.  -> array of RESULT_SEATS_DTYPE (passes counts whole trials); seat_shares(rows) gives
        the pot shares.  A wrong shape or dtype raises ValueError before the engine is touched."""
        q = _queries(queries)
        if not isinstance(tables, np.ndarray) or tables.dtype != np.uint16 or tables.ndim != 2 or tables.shape[1] != HAND_ROWS \
                or tables.shape[0] == 0:
            raise ValueError("tables is a uint16 array of shape [n_tables >= 1, HAND_ROWS = %d]" % HAND_ROWS)
        if not isinstance(seat_table, np.ndarray) or seat_table.dtype != np.uint32 or seat_table.shape != (len(q), 10):
            raise ValueError("seat_table is a uint32 array of shape [n, 10] = (%d, 10)" % len(q))
        tb, st = np.ascontiguousarray(tables), np.ascontiguousarray(seat_table)
        out = np.zeros(len(q), RESULT_SEATS_DTYPE)
        _call(self._lib.mcq_eval_batch_ranges, self._ctx, q.ctypes.data, st.ctypes.data, tb.ctypes.data, len(tb), len(q),
              _u64(seed), _u64(first_query_id), out.ctypes.data)
        return out

    def eval_batch_ranges_hands(self, queries, seat_table, tables, seed, first_query_id=0, seat=0):
        """eval_batch_ranges with the breakdown by hand of seat `seat` (mcq_eval_batch_ranges_hands): the same arguments,
        streams and rows, and for every record the HAND_ROWS rows of HAND_ROW_DTYPE, indexed by hand_index(a, b): the
        iterations in which the seat held that hand and its win, tie and share in them (zero rows for hands it cannot hold).
        -> (rows [n], hands [n, HAND_ROWS]); at most RANGES_HANDS_MAX_BATCH records per call, seat below every record's
        n_players."""
        q = _queries(queries)
        if not isinstance(tables, np.ndarray) or tables.dtype != np.uint16 or tables.ndim != 2 or tables.shape[1] != HAND_ROWS \
                or tables.shape[0] == 0:
            raise ValueError("tables is a uint16 array of shape [n_tables >= 1, HAND_ROWS = %d]" % HAND_ROWS)
        if not isinstance(seat_table, np.ndarray) or seat_table.dtype != np.uint32 or seat_table.shape != (len(q), 10):
            raise ValueError("seat_table is a uint32 array of shape [n, 10] = (%d, 10)" % len(q))
        if not 0 <= int(seat) <= 9:
            raise ValueError("seat is 0..9")
        tb, st = np.ascontiguousarray(tables), np.ascontiguousarray(seat_table)
        out = np.zeros(len(q), RESULT_SEATS_DTYPE)
        hands = np.zeros((len(q), HAND_ROWS), HAND_ROW_DTYPE)
        _call(self._lib.mcq_eval_batch_ranges_hands, self._ctx, q.ctypes.data, st.ctypes.data, tb.ctypes.data, len(tb), len(q),
              _u64(seed), _u64(first_query_id), int(seat), out.ctypes.data, hands.ctypes.data)
        return out, hands

    def exact_seats(self, queries, ext, law="reference"):
        """Exact per-seat enumeration of the all-in case (mcq_exact_batch_seats): every hand known, no random opponent.
        -> RESULT_SEATS_DTYPE rows of integer weights: runs = total weight, seat[s].share / (SHARE_UNIT * runs) is the
        exact pot share of seat s (seat_shares(rows))."""
        code = _law_code(law)
        q, e = _records(queries, ext)
        out = np.zeros(len(q), RESULT_SEATS_DTYPE)
        _call(self._lib.mcq_exact_batch_seats, self._ctx, q.ctypes.data, e.ctypes.data, len(q), code, out.ctypes.data)
        return out

    def exact_ext_seats(self, queries, ext, law="reference"):
        """exact_seats for records with at most ONE random opponent, ranged or not (mcq_exact_batch_ext_seats): seat
        1 + n_known is that opponent.  -> RESULT_SEATS_DTYPE rows of integer weights as exact_seats returns them (and the
        same rows bit for bit for a record without a random opponent); seat_shares(rows) gives the exact pot shares.  Two
        random opponents raise ValueError."""
        code = _law_code(law)
        q, e = _records(queries, ext)
        out = np.zeros(len(q), RESULT_SEATS_DTYPE)
        _call(self._lib.mcq_exact_batch_ext_seats, self._ctx, q.ctypes.data, e.ctypes.data, len(q), code, out.ctypes.data)
        return out

    def exact_matrix(self, queries, want_tie=True):
        """The exact hand-against-hand matrices of MATRIX_QUERY_DTYPE records (mcq_exact_matrix): heads-up, uniform law,
        3 to 5 table cards.  -> (win, tie, total): win[i, hand_index(h), hand_index(g)] = the table completions on which
        hand h beats hand g, tie likewise (None without want_tie), both uint16 [n, HAND_ROWS, HAND_ROWS] and zero where the
        two hands cannot meet; total[i] = the completions of a pair of hands, win[h][g] + win[g][h] + tie[h][g]."""
        q = _queries(queries, MATRIX_QUERY_DTYPE)
        if not 1 <= len(q) <= MATRIX_MAX_BATCH:
            raise ValueError("1 to MATRIX_MAX_BATCH = %d records per call" % MATRIX_MAX_BATCH)
        win = np.zeros((len(q), HAND_ROWS, HAND_ROWS), np.uint16)
        tie = np.zeros((len(q), HAND_ROWS, HAND_ROWS), np.uint16) if want_tie else None
        total = np.zeros(len(q), np.uint32)
        _call(self._lib.mcq_exact_matrix, self._ctx, q.ctypes.data, len(q), win.ctypes.data, _addr(tie), total.ctypes.data)
        return win, tie, total

    def exact_matrix_device(self, queries, d_win, d_tie, stream=0):
        """exact_matrix with the matrices written to device memory (mcq_exact_matrix_device): d_win / d_tie are raw device
        pointers (ints) to n x HAND_ROWS x HAND_ROWS uint16 each, d_tie 0 or None for win alone, stream a hipStream_t handle
        (int) or 0.  The records are host memory and are validated before anything is launched.  Asynchronous.
        -> total (uint32 [n])."""
        q = _queries(queries, MATRIX_QUERY_DTYPE)
        total = np.zeros(len(q), np.uint32)
        _call(self._lib.mcq_exact_matrix_device, self._ctx, q.ctypes.data, len(q), _opt(d_win), _opt(d_tie), total.ctypes.data,
              _opt(stream))
        return total

    def eval_batch_ext(self, queries, ext, seed, first_query_id=0, mode=MODE_PHILOX):
        """queries with one QUERY_EXT_DTYPE record each (ranges, hero range, ghost cards, second known hand)."""
        q, e = _records(queries, ext)
        out = np.zeros(len(q), RESULT_DTYPE)
        _call(self._lib.mcq_eval_batch_ext, self._ctx, q.ctypes.data, e.ctypes.data, len(q), _u64(seed), _u64(first_query_id),
              int(mode), out.ctypes.data)
        return out

    def eval_batch_numpy_stream(self, queries):
        """Parity mode on numpy's GLOBAL random state: the queries consume np.random's MT19937 stream in order,
        exactly as consecutive reference calls do, and np.random is left where those calls would leave it."""
        q = _queries(queries)
        out = np.zeros(len(q), RESULT_DTYPE)
        st = np.random.get_state()
        key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
        pos = C.c_uint32(int(st[2]))
        _call(self._lib.mcq_eval_batch_numpy_stream, self._ctx, q.ctypes.data, len(q), key.ctypes.data, C.byref(pos),
              out.ctypes.data)
        np.random.set_state((st[0], key, int(pos.value), st[3], st[4]))
        return out

    def eval_batch_device(self, d_queries, n, seed, d_results, first_query_id=0, stream=None):
        """Device-resident entry: d_queries / d_results are raw device pointers (ints), stream a hipStream_t
        handle (int) or None.  Asynchronous."""
        _call(self._lib.mcq_eval_batch_device, self._ctx, int(d_queries), int(n), _u64(seed), _u64(first_query_id),
              int(d_results), _opt(stream))

    def eval_batch_device_ways(self, d_queries, n, seed, d_results, first_query_id=0, stream=None):
        """eval_batch_device writing mcq_result_ways rows: d_results -> n x 22 uint64 (176 bytes per query)."""
        _call(self._lib.mcq_eval_batch_device_ways, self._ctx, int(d_queries), int(n), _u64(seed), _u64(first_query_id),
              int(d_results), _opt(stream))

    def eval_batch_device_small(self, d_queries, n, seed, d_results, first_query_id=0, stream=None):
        """eval_batch_device for queries of at most 8192 iterations each: ONE kernel launch, no pricing kernel, no
        atomics (a longer query gets runs = 0, passes = 2**64 - 1 like an invalid one)."""
        _call(self._lib.mcq_eval_batch_device_small, self._ctx, int(d_queries), int(n), _u64(seed), _u64(first_query_id),
              int(d_results), _opt(stream))

    def showdown(self, hands, want_keys=False):
        """hands [T, P, 7] card ids -> (winner[T], winner_type[T][, keys[T, P]])."""
        h = np.ascontiguousarray(hands, dtype=np.uint8)
        if h.ndim != 3 or h.shape[2] != 7:
            raise ValueError("hands must have shape [tables, players, 7]")
        T, P = h.shape[0], h.shape[1]
        win = np.zeros(T, np.uint8)
        wt = np.zeros(T, np.uint8)
        keys = np.zeros((T, P), np.uint32) if want_keys else None
        _call(self._lib.mcq_showdown, self._ctx, h.ctypes.data, T, P, win.ctypes.data, wt.ctypes.data, _addr(keys))
        return (win, wt, keys) if want_keys else (win, wt)

    def kernel_times(self, max_n=64):
        """Durations (ms, HIP events on the launch stream) of the most recent evaluation-kernel launches."""
        ms = np.zeros(max(int(max_n), 1), np.float32)
        n = self._lib.mcq_kernel_times(self._ctx, ms.ctypes.data, int(max_n))
        if n < 0:
            _raise(n)
        return ms[:n]

    @property
    def last_kernel_ms(self):
        return float(self._lib.mcq_last_kernel_ms(self._ctx))


PARTITION_AUTO, PARTITION_QUERIES, PARTITION_ITERATIONS = 0, 1, 2
_PARTITIONS = {None: 0, "auto": 0, "queries": 1, "iterations": 2, 0: 0, 1: 1, 2: 2}


class MultiEngine(_Handle):
    """mcq_multi: one process driving several GPUs of a node (include/mcq.h).  The batch is partitioned over
    shards, ONE RCCL all-reduce of the integer tally matrix joins them; results are bit-identical to Engine.eval_batch.

    devices: one HIP device ordinal per shard (a device may repeat); None = every visible device once."""
    _handle, _destroy = "_m", "mcq_multi_destroy"

    def __init__(self, devices=None):
        self._lib = load_library()
        if devices is None:
            n = self._lib.mcq_device_count()
            if n <= 0:
                raise McqError("no HIP device visible: " + _last_error())
            devices = list(range(n))
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        self._m = self._lib.mcq_multi_create(devs.ctypes.data, len(devs), 0)
        if not self._m:
            raise McqError("mcq_multi_create(%s) failed: %s" % ([int(d) for d in devs], _last_error()))
        self.devices = [int(d) for d in devs]
        self.lock = threading.Lock()   # the shim's shared MultiEngines serialise their callers on it

    def set_dealing_law(self, law):
        code = _law_code(law)
        _call(self._lib.mcq_multi_set_dealing_law, self._m, code)

    def eval_batch(self, queries, seed, first_query_id=0, partition=None):
        """queries: array of QUERY_DTYPE (host) -> array of RESULT_DTYPE; partition 'auto' | 'queries' | 'iterations'."""
        if partition not in _PARTITIONS:
            raise ValueError("partition must be 'auto', 'queries' or 'iterations'")
        q = _queries(queries)
        out = np.zeros(len(q), RESULT_DTYPE)
        _call(self._lib.mcq_multi_eval_batch, self._m, q.ctypes.data, len(q), _u64(seed), _u64(first_query_id),
              _PARTITIONS[partition], out.ctypes.data)
        return out

    def eval_batch_device(self, d_queries, n, seed, d_results, first_query_id=0, partition="auto"):
        """Queries and results resident in HBM: d_queries / d_results = one raw device pointer (int) per shard, on that
        shard's device -- the shard's block of the n queries (partition "queries") or all of them ("iterations"), and
        room for the complete [n] result matrix, which every shard's buffer holds afterwards.  Blocks until done."""
        k = len(self.devices)
        if len(d_queries) != k or len(d_results) != k:
            raise ValueError("one device pointer pair per shard")
        qp = (C.c_void_p * k)(*[_opt(p) for p in d_queries])
        rp = (C.c_void_p * k)(*[_opt(p) for p in d_results])
        _call(self._lib.mcq_multi_eval_batch_device, self._m, qp, int(n), _u64(seed), _u64(first_query_id),
              _PARTITIONS[partition], rp)

    @property
    def info(self):
        v = np.zeros(4, np.int32)
        _call(self._lib.mcq_multi_info, self._m, v.ctypes.data)
        return {"shards": int(v[0]), "devices": int(v[1]), "rccl_version": int(v[2]),
                "last_partition": {0: "auto", 1: "queries", 2: "iterations"}[int(v[3])]}

    @property
    def last_times_ms(self):
        v = np.zeros(3, np.float32)
        _call(self._lib.mcq_multi_times, self._m, v.ctypes.data)
        return {"kernel_max": float(v[0]), "all_reduce": float(v[1]), "call": float(v[2])}


class Tables(_Handle):
    """mcq_tables: T Hold'em tables advanced in lock-step by the native driver (include/mcq.h, BASELINE configs[4]).

    seats: one entry per seat -- ("equity", min_call_equity, min_bet_equity) or ("random",).
    engine=None gives a driver without GPU: only begin()/resume() work (used to pin the rules on the CPU).
    The tables are independent (own generator each): results do not depend on `threads`."""
    _handle, _destroy = "_t", "mcq_tables_destroy"

    def __init__(self, engine, n_tables, seats, runs=1000, initial_stacks=100, small_blind=1, big_blind=2,
                 max_raises=2, seed=0, threads=0, overlap=True, calculate_equity=False):
        self._lib = load_library()
        self._engine = engine
        cfg = np.zeros(1, TABLES_CONFIG_DTYPE)
        cfg["n_tables"], cfg["n_seats"], cfg["runs"], cfg["max_raises"] = n_tables, len(seats), runs, max_raises
        cfg["initial_stacks"], cfg["small_blind"], cfg["big_blind"] = initial_stacks, small_blind, big_blind
        cfg["seed"] = _u64(seed)
        cfg["reserved"][0, 0] = threads          # host threads stepping the tables; 0 = automatic
        cfg["reserved"][0, 1] = 0 if overlap else 1   # run(): groups of tables on streams of their own (same results either way)
        cfg["reserved"][0, 2] = 1 if calculate_equity else 0   # three more queries per observation (env.py:248-256)
        if len(seats) > 10:
            raise ValueError("at most 10 seats")
        for i, s in enumerate(seats):
            if s[0] == "equity":
                cfg["min_call_equity"][0, i], cfg["min_bet_equity"][0, i] = s[1], s[2]
            elif s[0] == "random":
                cfg["seat_kind"][0, i] = 1
            else:
                raise ValueError("seat kind must be 'equity' or 'random'")
        self.n_tables, self.n_seats = int(n_tables), len(seats)
        self._t = self._lib.mcq_tables_create(engine._ctx if engine is not None else None, cfg.ctypes.data)
        if not self._t:
            raise ValueError(_last_error())

    def begin(self):
        """-> the pending query of every table (QUERY_DTYPE[n_tables])."""
        q = np.zeros(self.n_tables, QUERY_DTYPE)
        self._lib.mcq_tables_begin(self._t, q.ctypes.data)
        return q

    def resume(self, equity):
        e = np.ascontiguousarray(equity, np.float64)
        if e.shape != (self.n_tables,):
            raise ValueError("one equity per table")
        _call(self._lib.mcq_tables_resume, self._t, e.ctypes.data)

    def run(self, lock_steps):
        """lock_steps rounds of (queries of all tables -> ONE GPU batch -> every table acts).  -> stats()."""
        st = np.zeros(3, np.uint64)
        _call(self._lib.mcq_tables_run, self._t, int(lock_steps), st.ctypes.data)
        return {"env_steps": int(st[0]), "queries": int(st[1]), "episodes": int(st[2])}

    def stats(self):
        st = np.zeros(3, np.uint64)
        self._lib.mcq_tables_stats(self._t, st.ctypes.data)
        return {"env_steps": int(st[0]), "queries": int(st[1]), "episodes": int(st[2])}

    def state(self, table):
        stacks = np.zeros(self.n_seats, np.float64)
        info = np.zeros(8, np.int32)
        _call(self._lib.mcq_tables_state, self._t, int(table), stacks.ctypes.data, info.ctypes.data)
        keys = ["stage", "current", "winner", "episodes", "env_steps", "queries", "legal", "phase"]
        d = dict(zip(keys, (int(x) for x in info)))
        d["stacks"] = stacks
        return d


_tls = threading.local()      # .engine: the calling thread's default engine
_default_law = "reference"    # dealing law of the default engines (montecarlo_hip.configure(dealing=...))
_default_engines = []         # weak references to every live default engine, for set_default_dealing_law


def default_engine():
    """The calling THREAD's engine on device $MCQ_DEVICE (else $LOCAL_RANK, else 0), created at the thread's first use.
    A context allows one call in flight (include/mcq.h), and ctypes drops the GIL for the duration of a call, so threads
    must not share one: every thread gets its own (own stream, own staging buffers), freed when the thread ends."""
    eng = getattr(_tls, "engine", None)
    if eng is None:
        dev = int(os.environ.get("MCQ_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        n = load_library().mcq_device_count()
        if n <= 0:
            raise McqError("no HIP device visible: neuron_poker_amd needs an AMD GPU (no CPU fallback). " + _last_error())
        eng = Engine(dev % n)
        import weakref
        with _lock:
            if _default_law != "reference":
                eng.set_dealing_law(_default_law)
            _default_engines[:] = [r for r in _default_engines if r() is not None]
            _default_engines.append(weakref.ref(eng))
        _tls.engine = eng
    return eng


def default_dealing_law():
    return _default_law


def set_default_dealing_law(law):
    """Dealing law of every thread's default engine, present and future.  Call it while no equity call is running on
    them (an engine in the middle of a call answers McqBusyError)."""
    global _default_law
    if law not in ("reference", "uniform"):
        raise ValueError("law must be 'reference' or 'uniform'")
    with _lock:
        _default_law = law
        for r in _default_engines:
            e = r()
            if e is not None and getattr(e, "_ctx", None):
                e.set_dealing_law(law)
