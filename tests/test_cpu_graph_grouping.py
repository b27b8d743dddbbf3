"""Host logic of the multi-step graph grouping (no GPU): which captured graphs a run replays.

GraphPool.walk moves a cursor through the resident pool and replays k-step graphs where the grouping
offset allows, aligned smaller graphs (k/2, ..., 2) and single-step graphs otherwise; GraphPool.align
moves the grouping so that a run of n steps after w others replays its remainder first and then only
k-step graphs. Every training path (FusedTwoTowerStep.run / replay_pool, the sharded steps' run)
delegates to it. Checked here on the product's own GraphPool with a ``capture`` whose graphs record
their replays (the real graphs are HIP graphs: tests/test_gpu_multihot.py, tests/test_gpu_ring.py);
the ring's run() is also driven once on a stand-in ring, through its ring_* views."""
import types

import pytest

from two_tower_recommender_model_amd.fused import FusedTwoTowerStep
from two_tower_recommender_model_amd.graph_pool import GraphPool


class _G:
    def __init__(self, log, name, steps):
        self.log, self.name, self.steps = log, name, steps

    def replay(self):
        self.log.append((self.name, self.steps))


def _pool(n, k, **kw):
    """A GraphPool of n positions whose ``capture`` records its calls (``captured``) and returns
    stand-in graphs that log their replays (``log``)."""
    log, captured = [], []

    def capture(idx):
        captured.append(list(idx))
        return _G(log, f"g{len(idx)}_{idx[0]}", list(idx))

    return GraphPool(n, k, capture, **kw), log, captured


def _steps(log):
    return [s for _, steps in log for s in steps]


@pytest.mark.parametrize("n,k,w,K", [(8, 8, 5, 20), (8, 4, 1, 6), (16, 8, 10, 50), (4, 2, 3, 7), (8, 8, 0, 16)])
def test_pool_run_is_consecutive_and_timed_region_uses_big_graphs(n, k, w, K):
    p, log, _ = _pool(n, k)
    p.align(0, K, after=w)
    cursor = p.walk(0, w)
    warm = list(log)
    log.clear()
    cursor = p.walk(cursor, K)
    timed = list(log)
    # every step exactly once, in pool order, continuing at the cursor
    assert _steps(warm) + _steps(timed) == [i % n for i in range(w + K)]
    assert cursor == (w + K) % n
    # the timed region: the remainder first (no single-step graph when it is a sum of the captured
    # sizes), then only k-step graphs
    sizes = [len(steps) for _, steps in timed]
    rem = K % k
    assert sum(sizes) == K and sizes[len(sizes) - K // k:] == [k] * (K // k)
    head = sizes[:len(sizes) - K // k]
    assert sum(head) == rem and all(s > 1 for s in head) == (rem % 2 == 0 or k == 1)


def test_ring_run_matches_pool_grouping():
    """The single-hot ring's run() follows the same rule (its graphs in ring_graphs / ring_mid /
    ring_small, grouping offset ring_offset)."""
    n, k = 16, 8
    log = []
    o = types.SimpleNamespace(ring_cursor=0, ring_k=k, ring_offset=3)
    span = lambda j, sz: [(3 + j + t) % n for t in range(sz)]  # noqa: E731
    o.ring_small = [_G(log, f"s{i}", [i]) for i in range(n)]
    o.ring_graphs = [_G(log, f"k{j}", span(j, k)) for j in range(0, n, k)]
    o.ring_mid = {sz: [_G(log, f"m{sz}", span(j, sz)) for j in range(0, n, sz)] for sz in (4, 2)}
    FusedTwoTowerStep.run(o, 19)
    assert _steps(log) == [i % n for i in range(19)] and o.ring_cursor == 19 % n
    sizes = [len(s) for _, s in log]
    assert sizes == [1, 2, 8, 8]  # 0 alone, 1-2, then 3.. as k-step graphs


def test_pool_regrouped_from_an_offset():
    """The single-hot ring (n = 16, k = 8) grouped from offset 3: k-step graphs, halves of 4 and 2."""
    n, k = 16, 8
    p, log, _ = _pool(n, k)
    p.regroup(3)
    assert p.offset == 3 and sorted(p.mid) == [2, 4] and len(p.big) == 2 and len(p.small) == n
    assert p.big[0].steps == [3, 4, 5, 6, 7, 8, 9, 10] and p.mid[2][7].steps == [1, 2]
    assert p.walk(0, 19) == 19 % n
    assert _steps(log) == [i % n for i in range(19)]
    sizes = [len(s) for _, s in log]
    assert sizes == [1, 2, 8, 8]  # 0 alone, 1-2, then 3.. as k-step graphs


def test_no_halves_is_the_sharded_rule():
    """halves=False (the sharded step): a k-step graph at a multiple of k, single steps otherwise."""
    p, log, _ = _pool(8, 4, halves=False)
    assert p.mid == {} and p.offset == 0
    assert p.walk(3, 10) == (3 + 10) % 8
    assert _steps(log) == [i % 8 for i in range(3, 13)]
    assert [len(s) for _, s in log] == [1, 4, 4, 1]


def test_single_step_pool_never_regroups():
    p, log, captured = _pool(6, 1)
    assert p.big is p.small and p.mid == {} and len(captured) == 6
    for cursor, n_next, after in [(0, 5, 0), (2, 7, 3), (5, 1, 1)]:
        assert p.align(cursor, n_next, after=after) is False
    assert p.big is p.small and p.offset == 0 and len(captured) == 6
    assert p.walk(4, 5) == 3 and _steps(log) == [4, 5, 0, 1, 2]


def test_k_not_a_power_of_two_has_no_halves():
    p, log, _ = _pool(12, 6)
    assert p.mid == {} and [g.steps for g in p.big] == [list(range(0, 6)), list(range(6, 12))]
    assert p.walk(5, 8) == 1 and [len(s) for _, s in log] == [1, 6, 1]


def test_align_with_unchanged_offset_captures_nothing():
    p, _, captured = _pool(8, 4)
    before = len(captured)
    assert p.align(2, 8, after=2) is True and p.offset == 4  # (2 + 2 + 8 % 4) % 8
    moved = len(captured)
    assert moved > before
    assert p.align(1, 7, after=0) is False and p.offset == 4  # (1 + 0 + 7 % 4) % 8: the same offset
    assert p.align(0, 0, after=4) is False
    assert len(captured) == moved
