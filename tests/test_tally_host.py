"""The wave tallies on the host (neuron_poker_amd/csrc/mcq_tally.hpp through tests/hostsim_tally): the header's fold of a
lane accumulator against an unpacking written here from the field descriptions in mcq_device.hpp, and the kernels' lane
states and lanes -> row step, run for a simulated wave of 64 lanes, against that fold -- the 10-bit fields of the split-pot
tally, its flush threshold and the two-counters-per-reduction forms included, which otherwise only the GPU tests reach
(test_long_queries_gpu.py, test_ways_gpu.py, test_seats_gpu.py, test_ranges_gpu.py).  No GPU."""
import numpy as np
import pytest

from tests import hostbuild
from tests import hostsim_tally as T

KINDS = (T.PLAIN, T.WAYS, T.SEATS)
WORDS = {T.PLAIN: 13, T.WAYS: 22, T.SEATS: 32}          # include/mcq.h: mcq_result, mcq_result_ways, mcq_result_seats
GAP = 5                                                  # codes leave a gap at 5; by_type index = code - (code >= 6)
SHARE_UNIT, WIN_SHIFT, TIE_SHIFT = 2520, 16, 21          # mcq_seat: share 16 bits, win and tie 5 bits each
M64 = (1 << 64) - 1


def unpack_fold(kind, recs):
    """The row a list of records folds into, by the field descriptions alone (arithmetic modulo 2^64)."""
    row = [0] * T.ROW
    for r in (tuple(int(x) for x in rec) for rec in np.asarray(recs).reshape(-1, T.REC)):
        if kind == T.SEATS:
            row[1] += r[0]
            for s in range(10):
                w = r[1 + s]
                row[2 + 3 * s] += (w >> WIN_SHIFT) & 31
                row[3 + 3 * s] += (w >> TIE_SHIFT) & 31
                row[4 + 3 * s] += w & 0xFFFF
            continue
        types, tie, passes, ways = (r[0], r[1], r[2], 0) if kind == T.PLAIN else (r[0], 0, r[1], r[2])
        wins = 0
        for c in range(10):
            if c != GAP:
                v = (types >> (6 * c)) & 63
                row[4 + c - (c >= 6)] += v
                wins += v
        for e in range(1, 10):                       # field e: hero best together with e opponents; field 0 is not stored
            v = (ways >> (6 * e)) & 63
            row[13 + e - 1] += v
            tie += v
        row[1] += passes
        row[2] += wins - tie
        row[3] += tie
    return np.array([x & M64 for x in row], np.uint64)


def pack6(fields):
    return sum(int(v) << (6 * i) for i, v in enumerate(fields))


def any_records(kind, rng, n):
    """Every field over its full legal range: 0..16 per 6-bit or 5-bit field, a share of up to 16 x 2520."""
    recs = np.zeros((n, T.REC), np.uint64)
    for r in recs:
        if kind == T.SEATS:
            r[0] = rng.integers(0, 1 << 32)
            for s in range(10):
                r[1 + s] = int(rng.integers(0, 16 * SHARE_UNIT + 1)) | int(rng.integers(0, 17)) << WIN_SHIFT | int(rng.integers(0, 17)) << TIE_SHIFT
        elif kind == T.PLAIN:
            r[:3] = pack6(rng.integers(0, 17, 10)), rng.integers(0, 17), rng.integers(0, 1 << 32)
        else:
            r[:3] = pack6(rng.integers(0, 17, 10)), rng.integers(0, 1 << 32), pack6(rng.integers(0, 17, 10))
    return recs


def legal_records(kind, rng, shape):
    """What sixteen iterations of a lane can leave behind: each lost, or won with one code and e opponents sharing the pot;
    per seat: k of the ten seats best."""
    recs = np.zeros(shape + (T.REC,), np.uint64)
    for r in recs.reshape(-1, T.REC):
        if kind == T.SEATS:
            seat = [0] * 10
            for _ in range(16):
                k = int(rng.integers(1, 11))
                for s in rng.choice(10, k, replace=False):
                    seat[s] += SHARE_UNIT // k | 1 << (WIN_SHIFT if k == 1 else TIE_SHIFT)
            r[0], r[1:11] = rng.integers(0, 1000), seat
            continue
        types, ways = [0] * 10, [0] * 10
        for _ in range(16):
            if rng.integers(0, 3):
                types[int(rng.choice([c for c in range(10) if c != GAP]))] += 1
                ways[int(rng.integers(1, 10)) if rng.integers(0, 4) == 0 else 0] += 1
        if kind == T.PLAIN:
            r[:3] = pack6(types), sum(ways[1:]), rng.integers(0, 1000)
        else:
            r[:3] = pack6(types), rng.integers(0, 1000), pack6(ways)
    return recs


def largest_records(kind, tasks):
    """16 in every field of every lane's every task (codes and ways alike: win = 0 for the split-pot kind)."""
    r = np.zeros(T.REC, np.uint64)
    if kind == T.SEATS:
        r[1:11] = 16 * SHARE_UNIT | 16 << WIN_SHIFT | 16 << TIE_SHIFT
    elif kind == T.PLAIN:
        r[:2] = pack6([16] * 10), 16
    else:
        r[0] = r[2] = pack6([16] * 10)
    return np.broadcast_to(r, (tasks, T.WAVE, T.REC)).copy()


def assert_wave_is_fold(kind, recs, packed=False):
    row, words = T.fold(kind, recs), T.wave(kind, recs, packed)
    n = WORDS[kind]
    assert (row == unpack_fold(kind, recs)).all()
    assert (words[:n - 1] == row[1:n]).all(), (words, row)       # lane l holds word l + 1 ...
    assert not words[n - 1:].any() and not row[n:].any() and row[0] == 0   # ... the lanes behind them nothing
    return row


def test_row_sizes_are_the_structs():
    c = T.consts()
    assert [c["plain_words"], c["ways_words"], c["seats_words"]] == [WORDS[k] for k in KINDS]
    assert [c["plain_lanes"], c["ways_lanes"], c["seats_lanes"]] == [WORDS[k] - 1 for k in KINDS]
    assert (c["n_codes"], c["n_ways"], c["max_seats"], c["ways_tally_tasks"], c["direct_tasks_limit"]) == (10, 9, 10, 63, 32)


@pytest.mark.parametrize("kind", KINDS)
def test_fold_against_an_independent_unpacking(kind):
    rng = np.random.default_rng(100 + kind)
    recs = any_records(kind, rng, 400)
    assert (T.fold(kind, recs) == unpack_fold(kind, recs)).all()
    for r in recs[:20]:                                           # and one at a time
        assert (T.fold(kind, r) == unpack_fold(kind, r)).all()
    assert int(recs[:, 0 if kind != T.SEATS else 1].max()) > 0


@pytest.mark.parametrize("kind,packed", [(T.PLAIN, False), (T.PLAIN, True), (T.WAYS, False), (T.WAYS, True), (T.SEATS, False)])
def test_wave_against_fold(kind, packed):
    """64 random lanes, each with its own number of tasks (the lanes of a wave add together: a lane that has run out adds
    empty accumulators), up to the flush threshold -- within MCQ_DIRECT_TASKS_LIMIT for the two-per-reduction form."""
    rng = np.random.default_rng(7 + 2 * kind + packed)
    most = T.consts()["direct_tasks_limit" if packed else "ways_tally_tasks"]
    recs = legal_records(kind, rng, (most, T.WAVE))
    n_tasks = rng.integers(1, most + 1, T.WAVE)
    n_tasks[rng.integers(0, T.WAVE)] = most
    recs[np.arange(most)[:, None] >= n_tasks[None, :]] = 0
    row = assert_wave_is_fold(kind, recs, packed)
    assert row[1] > 0 and row[2] > 0 and row[3] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_every_word_has_one_owner(kind):
    """With every counter of the row non-zero, words 1..kWords-1 sit in lanes 0..kLanes-1, one each."""
    r = np.zeros(T.REC, np.uint64)
    if kind == T.SEATS:
        r[0], r[1:11] = 5, [(100 + s) | (1 + s % 3) << WIN_SHIFT | (2 + s % 5) << TIE_SHIFT for s in range(10)]
    else:
        types = pack6([3 + c for c in range(10)])
        r[:3] = (types, 2, 5) if kind == T.PLAIN else (types, 5, pack6([0] + [1 + e % 2 for e in range(9)]))
    recs = np.broadcast_to(r, (3, T.WAVE, T.REC)).copy()
    for packed in ((False, True) if kind != T.SEATS else (False,)):
        row = assert_wave_is_fold(kind, recs, packed)
        assert row[1:WORDS[kind]].all()


def test_the_ten_bit_bound_is_tight():
    """63 tasks of 16 in every way field are exact in every lane; full() turns true with the 63rd; a 64th without a flush
    would carry into the neighbouring field -- a statement about the packing, which is why the threshold is 63."""
    assert_wave_is_fold(T.WAYS, largest_records(T.WAYS, 63))
    one = largest_records(T.WAYS, 64)[:, 0]
    for tasks in (1, 62, 63):
        way3, n_add, full, way = T.ways_state(one[:tasks])
        assert (n_add, full, way) == (tasks, tasks == 63, [16 * tasks] * 9)
        assert way3 == [16 * tasks * (1 | 1 << 10 | 1 << 20)] * 3
    assert 16 * 63 < 1024 <= 16 * 64
    lone = np.zeros((64, T.REC), np.uint64)
    lone[:, 2] = 16 << 6                                          # field 1 of `ways` = tie_ways[0] alone
    assert T.ways_state(lone[:63])[3] == [1008] + [0] * 8
    assert T.ways_state(lone)[3] == [0, 1] + [0] * 7              # 1024: gone from its field, a 1 in the next


@pytest.mark.parametrize("kind", KINDS)
def test_the_sixteen_bit_pairing_is_safe(kind):
    """64 lanes x MCQ_DIRECT_TASKS_LIMIT tasks x 16 in both halves of every pair: the packed sums are the separate ones."""
    limit = T.consts()["direct_tasks_limit"]
    assert 64 * 16 * limit < 1 << 16 and 64 * 16 * SHARE_UNIT < 1 << 22
    recs = largest_records(kind, limit)
    row = assert_wave_is_fold(kind, recs, packed=kind != T.SEATS)
    if kind == T.SEATS:
        assert list(row[2:5]) == [64 * 16 * limit, 64 * 16 * limit, 64 * 16 * SHARE_UNIT * limit]
    else:
        assert row[4] == 64 * 16 * limit and (kind == T.PLAIN or row[13] == 64 * 16 * limit)
        assert (T.wave(kind, recs, packed=False) == T.wave(kind, recs, packed=True)).all()


def test_flush_semantics():
    """The per-seat flush (the header's own): nothing from a clean wave, one atomic per word that is not zero, every lane
    clear() afterwards and a second flush silent.  The plain and split-pot flush is the kernels' wrapper around row_value:
    here, that clear() leaves a lane whose row step gives zero in every lane -- nothing for a flush to add."""
    rng = np.random.default_rng(5)
    recs = legal_records(T.SEATS, rng, (4, T.WAVE))
    recs[:, :, 5:11] = 0                                          # a five-handed query: seats 4..9 stay zero
    recs[:, :, 0] = 0                                             # (parity mode: no passes)
    row, clean, after, again, cleared = T.seats_flush(recs)
    want = unpack_fold(T.SEATS, recs)
    assert (row == want).all() and not want[14:].any() and want[1] == 0
    assert (clean, after, again, cleared) == (0, int((want != 0).sum()), 0, True) and 0 < after < 31
    for kind in (T.PLAIN, T.WAYS):
        assert T.clear_is_clean(kind, legal_records(kind, rng, (3, T.WAVE)))


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """hs_main.cpp walks the same cases, built with AddressSanitizer and UndefinedBehaviorSanitizer."""
    lines = hostbuild.run_sanitized("hostsim_tally/hs_main.cpp", "-O1", tmp_path)
    assert lines[-1] == "ok: 12" and all(ln.endswith(": holds") for ln in lines[:-1]), lines
