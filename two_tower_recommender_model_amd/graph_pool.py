"""Capture, grouping and replay of step graphs over a cyclic pool of resident batches: the host
code every training path shares (fused.py, sharded.py, sharded_kjt.py, dropin.py's slot graphs).

``capture_graph`` is the one place the package records a HIP graph. ``GraphPool`` holds a pool's
graphs — one per position, k-step graphs from a grouping offset and (k a power of two) k/2, ..., 2-step
ones at the same alignment — and walks a caller's cursor through them: a launch costs the host
~35-55 us and the stream idles ~20-40 us between two graphs, which single-step graphs pay every step.
The pool knows nothing of tables, comms or KJTs; the caller keeps the cursor."""
from __future__ import annotations

from typing import Callable, Sequence

import torch

from . import _lib


def capture_graph(device, body: Callable[[], None], *, keep_graph: bool = False,
                  thread_local: bool = False) -> torch.cuda.CUDAGraph:
    """Record ``body()`` into a HIP graph on a side stream forked from the current one.
    keep_graph: leave the graph uninstantiated (its user instantiates it); else it is uploaded here,
    so its first launch does not pay for that. thread_local: only this thread's calls are checked
    against the capture (the sharded paths: the RCCL watchdog thread works beside it; its pending
    works are retired by the caller first)."""
    g = torch.cuda.CUDAGraph(keep_graph=keep_graph)
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local" if thread_local else "global"):
            body()
    torch.cuda.current_stream(device).wait_stream(s)
    if not keep_graph:
        _lib.graph_upload(g, device)
    return g


def prefault_if_due(step) -> None:
    """The first replay after a capture walks the tables' pages right before it (TableSet.prefault;
    r06pf_* profiles). Armed by ``step._prefault_due = True``."""
    if step._prefault_due:
        step._prefault_due = False
        step.tables.prefault()


def walk(cursor: int, n: int, k: int, offset: int, small, big, mid) -> int:
    """The replay rule over a pool's graph lists (GraphPool.walk; FusedTwoTowerStep.run passes its
    ``ring_*`` views): n steps in pool order from ``cursor``; at relative position r = (i - offset) % n
    the k-step graph when r % k == 0 and k steps remain, else the largest ``mid`` size that divides
    r and fits, else small[i]. Returns the new cursor."""
    i, nb, sizes = cursor, len(small), sorted(mid, reverse=True)
    if not nb:
        raise _lib.TTError("no captured graphs to replay (capture first)")
    while n > 0:
        r = (i - offset) % nb  # position relative to the graphs' grouping
        if r % k == 0 and n >= k:
            big[r // k].replay()
            sz = k
        else:
            sz = next((m for m in sizes if r % m == 0 and n >= m), 1)
            (mid[sz][r // sz] if sz > 1 else small[i]).replay()
        i, n = (i + sz) % nb, n - sz
    return i


class GraphPool:
    def __init__(self, n: int, k: int, capture: Callable[[Sequence[int]], object], halves: bool = True):
        """``capture(idx)`` returns a graph (anything with ``replay()``) that runs pool positions
        ``idx`` in order. small[i] runs position i alone; big[j] runs the k positions from
        offset + j*k (``small`` itself when k == 1); mid[sz][j] the sz positions from offset + j*sz
        (halves, k a power of two: sz = k/2, ..., 2)."""
        self.n, self.k, self.capture, self.halves = n, k, capture, halves
        self.small = [capture([i]) for i in range(n)]
        self.regroup(0)

    def regroup(self, offset: int) -> None:
        """(Re)capture the multi-step graphs, grouped from pool position ``offset``."""
        n, k = self.n, self.k
        self.offset, self.big, self.mid = (offset % n if k > 1 else 0), [], {}
        if k == 1:
            self.big = self.small
            return
        span = lambda j, sz: [(offset + j + t) % n for t in range(sz)]  # noqa: E731
        self.big = [self.capture(span(j, k)) for j in range(0, n, k)]
        sz = k // 2 if self.halves and k & (k - 1) == 0 else 0
        while sz >= 2:
            self.mid[sz] = [self.capture(span(j, sz)) for j in range(0, n, sz)]
            sz //= 2

    def align(self, cursor: int, n_next: int, after: int = 0) -> bool:
        """Regroup for a run of ``n_next`` steps that starts ``after`` steps from ``cursor``: that
        run replays its n_next % k remainder first, in aligned smaller graphs (the first launch is
        the cheapest: the GPU starts sooner), then n_next // k full graphs — no single-step graphs
        when the remainder is a sum of the captured sizes. Only how the steps are grouped into
        launches changes. True when it regrouped (k > 1 and the offset moved)."""
        off = (cursor + after + n_next % self.k) % self.n
        if self.k == 1 or off == self.offset:
            return False
        self.regroup(off)
        return True

    def walk(self, cursor: int, n: int) -> int:
        """Replay n steps in pool order from ``cursor`` (``walk`` above); returns the new cursor."""
        return walk(cursor, n, self.k, self.offset, self.small, self.big, self.mid)

    def clear(self) -> None:
        """Drop every graph."""
        self.small, self.big, self.mid = [], [], {}
