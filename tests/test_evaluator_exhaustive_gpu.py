"""The ranking key of seven cards over its WHOLE domain on the GPU: all C(52,7) = 133 784 560 hands, each under all 21
splits into (hole, table), through Engine.showdown(..., want_keys=True) = mcq_showdown_kernel, against the oracle's
batch scores computed on the spot (O.score_batch).  The device's helpers (mcq_perm, mcq_bfi, mcq_max3, mcq_sad_u8,
mcq_bfe) are instructions there and emulations in tests/hostsim, so the host sweep alone does not cover them.

Hands go ten to a table, so 7-byte rows start at every alignment inside the kernel's 16-byte staging loads; a chunk
(the hands sharing their two lowest cards) is whatever size it is -- almost never a multiple of the 256-table tile or
of ten -- and what ten does not divide goes as one more table of fewer players, so the last partial tile and the padded
tails of `tile`, `winner` and `keys` are in play 22 000 times.  Checked, nothing sampled:
  * keys do not depend on the split; type and strict monotonicity against the oracle score as in the host sweep
    (tests/test_evaluator_exhaustive_host.py), census included;
  * per table, winner = first index of the greatest oracle score, winner_type = its type, under every split;
  * keys equal the host build's bit for bit on the hands whose lowest card is 2C (C(51,6) = 18 009 460 hands).
One engine, sequential calls.  Inputs are valid hands only.

Wall time, measured on an MI355X host with 16 CPUs: 22 s (19.7 GB of hands in, 11.2 GB of keys out, the oracle's
scores once per chunk).
"""
import math
import os

import numpy as np
import pytest

import neuron_poker_amd as npa
from oracle import oracle as O
from tests import evaluator_domain as D
from tests import hostsim as H

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
P = 10


def _showdown(e, hands, split):
    """hands [n, 7] under one split, ten to a table and the rest as one smaller table -> (keys [n], winner, winner_type)"""
    h = D.resplit(hands, split)
    n, T = len(h), len(h) // P
    keys = np.zeros(n, np.uint32)
    win, wt = np.zeros(T + (n % P != 0), np.uint8), np.zeros(T + (n % P != 0), np.uint8)
    if T:
        w, t, k = e.showdown(h[:T * P].reshape(T, P, 7), want_keys=True)
        keys[:T * P], win[:T], wt[:T] = k.reshape(-1), w, t
    if n % P:
        w, t, k = e.showdown(h[T * P:].reshape(1, n % P, 7), want_keys=True)
        keys[T * P:], win[T], wt[T] = k.reshape(-1), w[0], t[0]
    return keys, win, wt


def _expected_winners(scores):
    n, T = len(scores), len(scores) // P
    full = scores[:T * P].reshape(T, P)
    win = [np.argmax(full, axis=1)] if T else []       # argmax: the first of equal maxima
    top = [full.max(axis=1)] if T else []
    if n % P:
        win.append(np.array([np.argmax(scores[T * P:])]))
        top.append(np.array([scores[T * P:].max()]))
    return np.concatenate(win).astype(np.uint8), O.score_type(np.concatenate(top)).astype(np.uint8)


def test_every_hand_in_every_split_through_the_showdown_kernel():
    acc = D.ClassPairs()
    e = npa.Engine(0)
    shapes, evaluated = set(), 0
    try:
        for a, b, cards in D.chunks():
            n = len(cards)
            assert n == math.comb(51 - b, 5)
            shapes.add(((n // P) % 256 != 0, n % P != 0))
            scores = O.score_batch(cards, THREADS)
            want_win, want_type = _expected_winners(scores)
            keys = None
            for split in D.SPLITS:
                k, win, wt = _showdown(e, cards, split)
                evaluated += len(k)
                if keys is None:
                    keys = k
                    if a == 0:   # one leading card's worth: the host build's keys, bit for bit
                        assert np.array_equal(keys, H.eval7(cards)), (a, b)
                bad = np.flatnonzero(k != keys)
                assert bad.size == 0, "the key of %s depends on the split: %s 0x%08x, (0, 1) 0x%08x" % (
                    [O.card_str(c) for c in cards[bad[0]]], split, int(k[bad[0]]), int(keys[bad[0]]))
                assert np.array_equal(win, want_win), (a, b, split, int(np.flatnonzero(win != want_win)[0]))
                assert np.array_equal(wt, want_type), (a, b, split, int(np.flatnonzero(wt != want_type)[0]))
            acc.add(scores, keys, cards)
    finally:
        e.close()
    assert (True, True) in shapes                       # partial tiles and tables of fewer than ten did occur
    assert acc.n_hands() == D.N_HANDS == 133784560 and evaluated == 21 * D.N_HANDS
    acc.check_strictly_increasing()
    want = D.load_census()
    assert acc.census(O.TYPES) == want and len(acc.pairs) == want["classes"]
