"""The constructions shared by tests/test_ranges_paths_gpu.py, which runs them on the device, and
tests/test_stage_host.py, which asks the kernels' own staging rule (csrc/mcq_stage.hpp) what each of their blocks does.
A record is (table cards, the seats' table numbers, runs)."""
import numpy as np

from neuron_poker_amd import _lib

BOARD = [10, 17, 34, 3, 21]   # 4H 6D TH 2S 7D: clear of every hand the scan tables name
STREETS = (3, 0, 4, 5)
ONE_HOT = [(0, 1), (4, 5), (8, 9), (12, 13), (16, 18), (20, 22), (24, 25), (28, 29), (32, 33), (36, 37)]
THRESHOLD_SHAPES = ["32 records, 6 tables", "32 records, 7 tables", "33 records, 6 tables",
                    "32 records, 6 tables and 4 known hands", "known hands only"]


def batch(recs):
    """recs: [(table cards, seats' table numbers, runs)] -> (queries, seat_table [n, 10])"""
    q = np.concatenate([_lib.pack_query_one([0, 0], BOARD[:nb], len(st), runs) for nb, st, runs in recs])
    seat_table = np.full((len(recs), 10), 0xFFFFFFFF, np.uint32)   # entries at or above n_players are not read
    for i, (_, st, _) in enumerate(recs):
        seat_table[i, :len(st)] = st
    return q, seat_table


def narrow_tables(n, seed):
    """n distinct tables of about 300 hands, weights 1..9."""
    g = np.random.default_rng(seed)
    t = np.zeros((n, 1326), np.uint16)
    for k in range(n):
        on = g.random(1326) < 0.23
        t[k, on] = g.integers(1, 10, int(on.sum()))
    assert len({x.tobytes() for x in t}) == n
    return t


def one_hot_tables(hands):
    t = np.zeros((len(hands), 1326), np.uint16)
    for k, (a, b) in enumerate(hands):
        assert a not in BOARD and b not in BOARD
        t[k, _lib.hand_index(a, b)] = 1 + 7 * k
    return t


def threshold_records(n, n_tables, known=False):
    """n records of 2 to 6 seats over every street, runs 1 .. 200, seat s of record i on table (i + s) % n_tables; with
    `known`, one seat of every record (two of every third) holds one of the four known hands behind the tables."""
    recs = []
    for i in range(n):
        p = 2 + i % 5
        st = [(i + s) % n_tables for s in range(p)]
        if known:
            st[i % p] = n_tables + i % 4
            if i % 3 == 0:
                st[(i + 1) % p] = n_tables + (i + 1) % 4
        recs.append((STREETS[i % 4], st, (1, 17, 64, 200, 130)[i % 5]))
    return recs


def threshold_shape(shape):
    """One of THRESHOLD_SHAPES -> (records, tables): every table is named by some seat."""
    if shape == "known hands only":
        tables = one_hot_tables(ONE_HOT)
        recs = [(STREETS[i % 4], [(i + 3 * s) % 10 for s in range(2 + i % 3)], (1, 17, 64, 200)[i % 4]) for i in range(32)]
        for _, st, _ in recs:
            assert len(set(st)) == len(st)
    else:
        n, nt = (33 if shape.startswith("33") else 32), (7 if "7 tables" in shape else 6)
        known = "known" in shape
        tables = narrow_tables(nt, 23)
        if known:
            tables = np.concatenate([tables, one_hot_tables(ONE_HOT[:4])])
        recs = threshold_records(n, nt, known)
        named = {t for _, st, _ in recs for t in st}
        assert named == set(range(len(tables)))
    return recs, tables


def full_width_tables():
    """Ten distinct tables with all 1326 entries non-zero (weights 1..7), each with most of its weight on the six pairs of
    one rank that is not on the flop: ten seats then collide seldom, and the host build of the reference stays cheap."""
    g = np.random.default_rng(29)
    t = g.integers(1, 8, (10, 1326)).astype(np.uint16)
    ranks = [r for r in range(13) if r not in {c >> 2 for c in BOARD[:3]}]
    for k in range(10):
        for a in range(4):
            for b in range(a + 1, 4):
                t[k, _lib.hand_index(4 * ranks[k] + a, 4 * ranks[k] + b)] = 60000
    assert (t != 0).all()
    return t


def mixed_batch():
    """(records, tables) of the mixed-blocks test: 24 records on tables 0..5, then 24 that seat ten players on the ten
    full-width tables 6..15."""
    tables = np.concatenate([narrow_tables(6, 31), full_width_tables()])
    recs = [(3, [(i + s) % 6 for s in range(2 + i % 5)], 2500) for i in range(24)]
    recs += [(3, [6 + (i + s) % 10 for s in range(10)], 2500) for i in range(24)]
    return recs, tables
