"""The evaluator's whole domain, chunk by chunk: all C(52,7) = 133 784 560 seven-card hands (shared by the host sweep,
the GPU sweep and tests/golden/gen_evaluator_census.py).

A chunk is every hand whose two lowest card ids are (a, b): at most C(50,5) = 2 118 760 hands, so no array of the whole
domain is ever held.  Within a hand the cards ascend; the 21 SPLITS say which two positions are the hole cards.

ClassPairs collects the distinct (oracle score, key) pairs of everything it is fed and decides the whole-domain form of
a total-order check: equal scores have equal keys, and over the distinct pairs both columns increase strictly together.
"""
import itertools
import json
import math
import os

import numpy as np

N_HANDS = math.comb(52, 7)
assert N_HANDS == 133784560
SPLITS = list(itertools.combinations(range(7), 2))      # (0, 1) first: the split hostsim.eval7 takes
assert len(SPLITS) == 21
CENSUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluator_census.json")

_tail = None


def _tails():
    """all 5-subsets of range(50), ordered by their greatest element: the subsets of range(m) are the first C(m, 5) rows"""
    global _tail
    if _tail is None:
        t = np.fromiter(itertools.chain.from_iterable(itertools.combinations(range(50), 5)), np.uint8,
                        count=5 * math.comb(50, 5)).reshape(-1, 5)
        _tail = np.ascontiguousarray(t[np.argsort(t[:, 4], kind="stable")])
    return _tail


def leading_pairs():
    return [(a, b) for a in range(46) for b in range(a + 1, 47)]


def chunk(a, b):
    """every hand whose two lowest cards are a < b -> uint8 [C(51 - b, 5), 7], cards ascending in a row"""
    n = math.comb(51 - b, 5)
    out = np.empty((n, 7), np.uint8)
    out[:, 0] = a
    out[:, 1] = b
    out[:, 2:] = _tails()[:n] + np.uint8(b + 1)
    return out


def chunks(pairs=None):
    for a, b in (leading_pairs() if pairs is None else pairs):
        yield a, b, chunk(a, b)


def resplit(cards, split):
    """the same hands with positions split = (x, y) moved to the front (the hole cards of [n, 7] rows)"""
    x, y = split
    return np.ascontiguousarray(cards[:, [x, y] + [k for k in range(7) if k not in (x, y)]])


def key_type(keys):
    """by_type index of ranking keys (bits 28.. hold a code with a gap at 5)"""
    code = np.asarray(keys, np.uint32) >> 28
    return (code - (code >= 6)).astype(np.uint32)


class ClassPairs:
    """Distinct (score, key) pairs and the census of what was fed.  A pair is held as one uint64: the score (36 bits:
    type, then eight 4-bit fields) above the key's low 28 bits -- the key's top four bits are its type code, which add()
    compares with the score's type first, so nothing of the key is lost."""

    def __init__(self):
        self.pairs = np.zeros(0, np.uint64)
        self.hands = np.zeros(9, np.int64)

    def add(self, scores, keys, cards):
        scores, keys = np.asarray(scores, np.uint64), np.asarray(keys, np.uint32)
        assert len(scores) == len(keys) == len(cards)
        typ = (scores >> np.uint64(32)).astype(np.uint32)
        bad = np.flatnonzero((typ != key_type(keys)) | (typ > 8))
        assert bad.size == 0, "type of hand %s: key 0x%08x, oracle score 0x%09x" % (
            cards[bad[0]].tolist(), int(keys[bad[0]]), int(scores[bad[0]]))
        self.hands += np.bincount(typ, minlength=9)
        c = (scores << np.uint64(28)) | (keys & np.uint32(0x0FFFFFFF)).astype(np.uint64)
        u = np.unique(c)
        s = u >> np.uint64(28)
        dup = np.flatnonzero(s[1:] == s[:-1])
        if dup.size:   # one score, two keys inside this chunk: name two such hands
            i = int(np.flatnonzero(c == u[dup[0]])[0])
            j = int(np.flatnonzero(c == u[dup[0] + 1])[0])
            raise AssertionError("equal oracle score 0x%09x but keys 0x%08x / 0x%08x: hands %s and %s" % (
                int(scores[i]), int(keys[i]), int(keys[j]), cards[i].tolist(), cards[j].tolist()))
        self.pairs = np.union1d(self.pairs, u)

    def n_hands(self):
        return int(self.hands.sum())

    def check_strictly_increasing(self):
        """over everything fed: one key per score, and score order = key order (so as many keys as scores)"""
        p = self.pairs
        s = p >> np.uint64(28)
        typ = (s >> np.uint64(32)).astype(np.uint64)
        code = typ + (typ >= 5).astype(np.uint64)                      # the key's type code: a gap at 5
        k = (code << np.uint64(28)) | (p & np.uint64(0x0FFFFFFF))      # the full key again
        bad = np.flatnonzero(s[1:] <= s[:-1])
        assert bad.size == 0, "oracle score 0x%09x has the keys 0x%08x and 0x%08x" % (
            int(s[bad[0]]), int(k[bad[0]]), int(k[bad[0] + 1]))
        bad = np.flatnonzero(k[1:] <= k[:-1])
        assert bad.size == 0, "scores 0x%09x < 0x%09x but keys 0x%08x >= 0x%08x" % (
            int(s[bad[0]]), int(s[bad[0] + 1]), int(k[bad[0]]), int(k[bad[0] + 1]))
        assert len(np.unique(k)) == len(np.unique(s)) == len(p)

    def census(self, names):
        s = self.pairs >> np.uint64(28)
        classes = np.bincount((s >> np.uint64(32)).astype(np.int64), minlength=9)
        assert len(np.unique(s)) == len(s)
        return {"hands": self.n_hands(), "classes": int(classes.sum()),
                "by_type": {n: {"hands": int(self.hands[i]), "classes": int(classes[i])} for i, n in enumerate(names)}}


def load_census():
    with open(CENSUS) as f:
        return json.load(f)
