"""The rank-sum hash of the plain path, without a GPU: the tables mcq_fill_tables builds (tests/hostsim_sum), the
sum-form key beside mcq_eval_key over every 7-card hand, and sum-form iterations against the oracle."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import hostsim as HS
from tests import hostsim_sum as H
from tests import hostsim_ways as HW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sum_hash.json")
LDS_BUDGET = 144 * 1024   # what the evaluation kernel's LDS leaves for hoff + hrank (16-bit entries)


@pytest.fixture(scope="module")
def tab():
    hoff, hrank, tfid, tf = H.tables()
    sums, keys = H.multisets()
    return {"hoff": hoff.astype(np.int64), "hrank": hrank.astype(np.int64), "tfid": tfid, "tf": tf, "sums": sums.astype(np.int64),
            "keys": keys, "info": H.info()}


def slots(tab):
    sh = tab["info"]["shift"]
    return tab["hoff"][tab["sums"] & ((1 << sh) - 1)] + (tab["sums"] >> sh)


def test_every_multiset_has_its_own_slot_and_the_tables_fit(tab):
    i = tab["info"]
    assert len(tab["sums"]) == 49205 and len(np.unique(tab["sums"])) == 49205
    s = slots(tab)
    assert s.max() < i["slots"] and len(np.unique(s)) == 49205
    assert i["fits"] and i["rows"] == 1 << i["shift"]
    assert 2 * (i["rows"] + i["slots"]) <= LDS_BUDGET
    assert i["image_bytes"] == 2 * (i["rows"] + i["slots"]) + 1024 and i["image_bytes"] % 1024 == 0
    # nothing but the multisets' slots is filled, and no id is 0
    assert np.count_nonzero(tab["hrank"]) == 49205 and np.all(tab["hrank"][s] != 0)


def test_ids_are_order_isomorphic_to_the_keys(tab):
    ids = tab["hrank"][slots(tab)]
    fl = tab["tf"] != 0
    assert np.array_equal(tab["tfid"] != 0, fl)
    pairs = np.unique(np.stack([np.concatenate([tab["keys"], tab["tf"][fl]]).astype(np.int64),
                                np.concatenate([ids, tab["tfid"][fl].astype(np.int64)])], 1), axis=0)   # sorted by key
    assert np.all(np.diff(pairs[:, 0]) > 0) and np.all(np.diff(pairs[:, 1]) > 0)
    # the type code rides on top of the id as it does on the key
    assert np.array_equal(pairs[:, 1] >> 12, pairs[:, 0] >> 28)
    g = json.load(open(GOLDEN))
    by_code = [int(np.count_nonzero(pairs[:, 0] >> 28 == c)) for c in range(10)]
    assert by_code == g["ids_by_code"] == tab["info"]["ids_by_code"] and len(pairs) == g["ids"]
    assert max(by_code) < 4096
    assert [int(w) for w in H.weights()] == g["weights"] and g["shift"] == tab["info"]["shift"]
    assert (g["rows"], g["slots"]) == (tab["info"]["rows"], tab["info"]["slots"])


def test_sum_form_key_over_all_seven_card_hands():
    """133 784 560 hands: each id belongs to one key, hero's type is mcq_key_type, and ids rise strictly with keys"""
    n, bad, m = H.sweep(threads=min(16, os.cpu_count() or 1))
    assert n == 133784560 and bad == 0
    keys = m[m != 0].astype(np.int64)   # in id order
    # (fewer than the tables hold: tf[] also has entries for suit masks of eight and more cards)
    assert 4824 <= len(keys) <= json.load(open(GOLDEN))["ids"]   # 4824: the distinct 7-card hand values of plain poker
    assert np.all(np.diff(keys) > 0)


def query(rng, p, nb, runs):
    c = rng.permutation(52)[:2 + nb]
    q = np.zeros(16, np.uint8)
    q[0:2] = c[:2]
    q[2:7] = list(c[2:]) + [255] * (5 - nb)
    q[7], q[8] = nb, p
    q[12:16] = np.frombuffer(np.uint32(runs).tobytes(), np.uint8)
    return q


@pytest.mark.parametrize("general", [False, True])
def test_sum_form_iterations_match_the_oracle(general):
    """mcq_iteration / mcq_iterations (sum form) for 1-10 players x 0/3/4/5 table cards, both accumulators"""
    rng = np.random.default_rng(77)
    seed = (1 << 41) | 12345
    for p in range(1, 11):
        for nb in (0, 3, 4, 5):
            q = query(rng, p, nb, 1040)   # a full task and a partly filled one
            want = O.run_batch(O.MODE_CTR, q.reshape(1, 16), seed, first_qid=p)[0]
            got = HS.run_ctr(q, seed, p, general=general)
            assert np.array_equal(np.asarray(got).view(np.uint64).reshape(-1)[:13], want.view(np.uint64).reshape(-1)), (p, nb)
            ways = HW.run(O.MODE_CTR, q, seed, qid=p, general=general)
            assert np.array_equal(ways[:13], want.view(np.uint64).reshape(-1)) and ways[13:].sum() == ways[3], (p, nb)
