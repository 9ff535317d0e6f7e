"""The dealing's single-hole step (mcq_hole_pair: a hole alone in its register is one compare of the two draws as they
arrive) without a GPU, on a host build of the lane code (tests/hostsim_dealing).

* The step against the generic path it stands for -- insert at slot 0, byte-SWAR scan, insert at slot 1 -- for every
  (t0, r) in 0..63 x 0..63 at the four places the iteration takes it: opponent draws J = 1, 5, 9 (the second card of pairs
  0, 2, 4, each into a fresh register) and table draw K = 1.  Position count and register, bit for bit.
* Whole iterations against the oracle's CTR mode, all thirteen words of a row, 1 to 9 opponents x 0, 3, 4, 5 table cards,
  the straight-line forms and the general form.  The draws pass through a counting policy, and the cases the step can
  get wrong must each have been reached at every place: r2 == r1 - 1 (the first hole just does not count, f = 0), the
  a == c branch of the pair decode (r1 = dd, the largest value a draw can carry), and r2 == r1 (f = 1).  The reference's
  law never deals r2 == r1 to an opponent -- its decode makes a != c or r1 = dd > c -- so at J = 1, 5, 9 that case comes
  from the same grid under the uniform law (the oracle's CTR mode with the uniform law), which in turn has no a == c
  branch; the table's K = 1 meets r2 == r1 and r2 == r1 - 1 under either law and has no a == c branch at all.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import hostsim_dealing

SEED, FQ = (1 << 40) | 0xDEA1, 11
RUNS = 64 * 16
BOARD = ["4C", "JD", "JS", "8H", "AC"]
HANDS = [["QS", "QD"], ["2C", "7H"], ["AH", "KH"], ["9C", "TC"]]
GRID = [(HANDS[(n_opp + nb) % 4], BOARD[:nb], n_opp + 1) for n_opp in range(1, 10) for nb in (0, 3, 4, 5)]
N_OPP = np.array([p - 1 for _, _, p in GRID])
N_DEAL = np.array([5 - len(b) for _, b, _ in GRID])
LAWS = {"reference": (0, O.MODE_CTR), "uniform": (1, O.MODE_CTR_UNIFORM)}


def pack(cells):
    hole = np.array([[O.card_id(c) for c in h] for h, _, _ in cells], np.uint8)
    board = np.array([[O.card_id(c) for c in b] + [255] * (5 - len(b)) for _, b, _ in cells], np.uint8)
    return O.pack_queries(hole, board, np.array([p for _, _, p in cells]), RUNS)


def host_rows(q, straight, uniform):
    L = hostsim_dealing.lib()
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 16)
    out = np.zeros((len(q), 13), np.uint64)
    hits = np.zeros((len(q), 4, 4), np.uint64)
    for i in range(len(q)):
        rec = q[i].copy()
        assert L.hs_dealing_run(rec.ctypes.data_as(C.c_void_p), SEED, FQ + i, straight, uniform,
                                out[i].ctypes.data_as(C.c_void_p), hits[i].ctypes.data_as(C.c_void_p)) == 0
    return out, hits


@pytest.fixture(scope="module")
def want():
    out = {}
    for law, (_, mode) in LAWS.items():
        out[law] = O.run_batch(mode, pack(GRID), SEED, first_qid=FQ, threads=8)
        out[law].setflags(write=False)
    return out


def test_grid_has_every_cell():
    assert len(GRID) == 36 and len(set(zip(N_OPP.tolist(), N_DEAL.tolist()))) == 36


@pytest.mark.parametrize("site", [1, 5, 9, 0], ids=["J1", "J5", "J9", "K1"])
def test_single_hole_step_is_the_generic_scan_and_inserts(site):
    L = hostsim_dealing.lib()
    out = np.zeros(4, np.uint32)
    flags = set()
    for t0 in range(64):
        for r in range(64):
            assert L.hs_dealing_step(site, t0, r, out.ctypes.data_as(C.c_void_p)) == 0
            assert out[0] == out[2] and out[1] == out[3], (site, t0, r, [hex(int(x)) for x in out])
            assert int(out[0]) == (r | 0x80) + (t0 <= r)
            flags.add((t0 <= r, t0 == r, t0 == r + 1))
    assert {(True, True, False), (False, False, True)} <= flags


@pytest.mark.parametrize("straight", [1, 0], ids=["straight", "general"])
@pytest.mark.parametrize("law", list(LAWS))
def test_iterations_match_the_oracle_and_reach_the_edges(want, law, straight):
    got, hits = host_rows(pack(GRID), straight, LAWS[law][0])
    assert int(got[:, 0].sum()) == 36 * RUNS
    for i, cell in enumerate(GRID):
        assert np.array_equal(got[i], want[law][i]), (cell, got[i], want[law][i])
    # draws seen at each place: pair P = 0, 2, 4 wherever there are more than P opponents, K = 1 wherever two cards come
    for s, p in enumerate((0, 2, 4)):
        assert np.array_equal(hits[:, s, 3], np.where(N_OPP > p, RUNS, 0))
    assert np.array_equal(hits[:, 3, 3], np.where(N_DEAL >= 2, RUNS, 0))
    total = hits.sum(0)
    for s, name in enumerate(("J=1", "J=5", "J=9")):
        assert total[s, 1] > 0, (name, total[s])                       # r2 == r1 - 1
        if law == "reference":
            assert total[s, 2] > 0 and total[s, 0] == 0, (name, total[s])   # a == c; the law never deals r2 == r1
        else:
            assert total[s, 0] > 0 and total[s, 2] == 0, (name, total[s])   # r2 == r1; no a == c branch
    assert total[3, 0] > 0 and total[3, 1] > 0, ("K=1", total[3])
