"""The cost axis of the Monte-Carlo kernels without a GPU (csrc/mcq_axis.hpp through tests/hostsim_axis): a task belongs to
the slice its start falls into, so the waves' slices must hand every task of every record out exactly once.

  * partition: exhaustively over small batches -- zero-cost records (equal neighbouring prefixes), mixed weights that put
    the cuts inside tasks, more waves than units;
  * 64-bit range: an axis whose total times the number of waves is beyond 2^32;
  * mirror: the Python copy of the block search that the GPU tests' expectations use (tests/ext_grid.py) == the header."""
import random

from tests import ext_grid as G
from tests import hostsim_axis as A

WEIGHTS = [1, 2, 3, 5, 16]


def test_every_task_is_run_exactly_once():
    # n = 1..4 records x (0..3 tasks x five weights) each x 1..9 waves, counted in the host build itself
    cases, bad, first = A.partition_exhaustive(4, 3, WEIGHTS, 9)
    assert cases == 9 * sum(20 ** n for n in range(1, 5))
    assert bad == 0, first


def test_walk_of_a_slice_by_hand():
    # the same property, counted here, on batches that hold what the exhaustive run is about
    for tasks, weights in [([3, 0, 2, 1], [5, 1, 16, 3]), ([0, 0, 3], [2, 2, 5]), ([1], [16]), ([2, 3, 0, 0], [3, 2, 1, 1]),
                           ([0], [1])]:
        want = sorted((i, t) for i, n in enumerate(tasks) for t in range(n))
        total = sum(t * w for t, w in zip(tasks, weights))
        for n_waves in range(1, 10):
            got = [A.walk(tasks, weights, w, n_waves) for w in range(n_waves)]
            assert sorted(p for g in got for p in g) == want, (tasks, weights, n_waves)
            for w, g in enumerate(got):   # a wave's tasks are consecutive and start inside its slice
                lo, hi = total * w // n_waves, total * (w + 1) // n_waves
                assert g == sorted(g)
                for i, t in g:
                    start = sum(a * b for a, b in zip(tasks[:i], weights[:i])) + t * weights[i]
                    assert lo <= start < hi
            if total < n_waves:
                assert sum(1 for g in got if not g) >= n_waves - total
    # a cut inside a task: two records of one task of weight 16, three waves -> cuts at 10 and 21
    assert [A.walk([1, 1], [16, 16], w, 3) for w in range(3)] == [[(0, 0)], [(1, 0)], []]


def test_slices_tile_an_axis_beyond_32_bits():
    tasks, weight, n_waves = 1 << 31, 16, 4096
    total = tasks * weight
    assert total * n_waves > 1 << 32 and total * n_waves < 1 << 64
    at, n_tasks = 0, 0
    for w in range(n_waves):
        lo, hi = A.slice_of(total, w, n_waves)
        assert lo == at == total * w // n_waves and hi == total * (w + 1) // n_waves and hi > lo
        at = hi
        first = A.first_task(0, lo, weight)
        assert first == -(-lo // weight) and (w == 0 or not A.owns(0, first, weight, lo))
        # the tasks of this wave: [first, the first task of the next slice)
        end = A.first_task(0, hi, weight)
        assert A.owns(0, end - 1, weight, hi) and (end == tasks or not A.owns(0, end, weight, hi))
        n_tasks += end - first
    assert at == total and n_tasks == tasks
    # an odd cut: 3 parts of the same axis, and of one that no part count divides
    assert [A.slice_of(total, i, 3) for i in range(3)] == [(total * i // 3, total * (i + 1) // 3) for i in range(3)]
    odd = (1 << 44) + 12345
    cuts = [A.slice_of(odd, i, 4095) for i in range(4095)]
    assert cuts[0][0] == 0 and cuts[-1][1] == odd and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))


def test_block_search_equals_the_mirror_of_the_gpu_tests():
    rng = random.Random(20261020)
    blocks_seen, empty_seen, equal_seen = 0, 0, 0
    for case in range(300):
        n = rng.randint(1, 64)
        costs = [rng.choice([0, 0, 1, 2, 3]) * rng.choice([1, 2, 3, 5, 16, 400]) for _ in range(n)]
        if case % 7 == 0:
            costs = [c if j == rng.randrange(n) else 0 for j, c in enumerate(costs)]   # nearly everything without cost
        prefix = [0]
        for c in costs:
            prefix.append(prefix[-1] + c)
        equal_seen += any(a == b for a, b in zip(prefix, prefix[1:]))
        grid, wpb = rng.randint(1, 8), rng.randint(4, 16)
        for blk in range(grid):
            want = G.block_records(prefix, n, blk, wpb, grid)
            got = A.block_records(prefix, blk, wpb, grid)
            assert got == (want if want is not None else (0, 0)), (prefix, blk, wpb, grid)
            blocks_seen += want is not None
            empty_seen += want is None
            if want is not None:   # the two searches on their own, at the block's two ends
                total, n_waves = prefix[n], grid * wpb
                blo, bhi = total * (blk * wpb) // n_waves, total * ((blk + 1) * wpb) // n_waves
                assert A.last_le(prefix, blo) == want[0]
                assert A.last_lt(prefix, want[0], bhi) == want[0] + want[1] - 1
                assert prefix[want[0]] <= blo < prefix[want[0] + 1]
    assert blocks_seen > 500 and empty_seen > 20 and equal_seen > 100
