"""IVF (inverted-file) approximate top-k retrieval over the exported item embeddings: the
approximate vector index that 04_evaluate_retrieval.py:112-153 queries.

The items are partitioned into ``nlist`` lists by k-means (build_ivf_index); a query scans only the
``nprobe`` lists whose centroids are nearest to it. Both steps run on the library's kernels: the
coarse step is ops.topk_mips with the centroids as items, the fine step ops.ivf_scan
(tt_ivf_scan). A pair's score is the exact kernel's, so a search returns exactly what
ops.topk_mips returns when the query is denied every item outside its probed lists, bit for bit;
with nprobe = nlist it is the exact result.

An item mask (the index's ``filters=`` of 04_evaluate_retrieval.py:97-101) is a view of the index:
IVFIndex.restricted(allow) shares every tensor of the base and adds the mask in list order
(ops.ivf_mask_lists). Its coarse step names only lists that hold an eligible item, its fine step is
tt_ivf_scan_masked: exactly ops.topk_mips(allow=...) over the probed lists' items.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import ops

LIST_ALIGN = 128  # every list begins at a multiple of the scan's largest chunk
MAX_NPROBE = 64   # tt_ivf_scan's limit: one lane of the merge per probed list


def _l2_bias(x: torch.Tensor) -> torch.Tensor:
    from .lifecycle import l2_bias

    return l2_bias(x)


class IVFIndex:
    """One immutable set of device tensors (see include/tt_mi355x.h, tt_ivf_scan):
    ``centroids`` fp32 [L, E], ``centroid_bias`` fp32 [L] = l2_bias(centroids), ``rows`` bf16 [P, E]
    (the item rows in list order, rounded to nearest-even once), ``bias`` fp32 [P] or None (the item
    bias in the same order; for metric "l2" l2_bias(item_emb) permuted), ``labels`` int32 [P] (the
    original item row, -1 on padding rows), ``list_begin`` int64 [L], ``list_len`` int32 [L],
    ``metric`` and ``N``. Every list_begin is a multiple of 128, lists do not overlap, labels ascend
    within a list, every item is in exactly one list.

    A view made by ``restricted(allow)`` also carries ``row_allow`` int32 [ceil(P / 32)] (a bit per
    packed row), ``list_allow`` int32 [ceil(L / 32)] (a bit per list with an eligible row),
    ``list_eligible`` int32 [L] and ``eligible`` (a 0-d int64 tensor: the eligible items, for the
    caller to report); they are None on an unrestricted index."""

    _TENSORS = ("centroids", "centroid_bias", "rows", "bias", "labels", "list_begin", "list_len")

    def __init__(self, centroids, centroid_bias, rows, bias, labels, list_begin, list_len, metric: str, N: int):
        if metric not in ("dot", "l2"):
            raise ValueError("metric must be 'dot' or 'l2'")
        self.centroids, self.centroid_bias = centroids, centroid_bias
        self.rows, self.bias, self.labels = rows, bias, labels
        self.list_begin, self.list_len = list_begin, list_len
        self.metric, self.N = metric, int(N)
        self.row_allow = self.list_allow = self.list_eligible = self.eligible = None

    @property
    def nlist(self) -> int:
        return self.list_begin.numel()

    @classmethod
    def from_assignment(cls, item_emb: torch.Tensor, assign: torch.Tensor, nlist: int, metric: str = "dot",
                        bias: Optional[torch.Tensor] = None, centroids: Optional[torch.Tensor] = None) -> "IVFIndex":
        """Pack an index from any assignment int [N] with values in [0, nlist). A stable sort by
        list id keeps the original rows ascending within a list. ``bias``: the item bias [N] (metric
        "l2": l2_bias(item_emb) when not given). ``centroids``: fp32 [nlist, E]; when not given, the
        lists' means (ops.ivf_segment_mean; an empty list's centroid is 0). On the device, one
        host sync (the size P of the packed tensors)."""
        if metric not in ("dot", "l2"):
            raise ValueError("metric must be 'dot' or 'l2'")
        N, E = item_emb.shape
        dev = item_emb.device
        if assign.numel() != N or assign.dtype.is_floating_point:
            raise ValueError("assign must be an integer tensor [N]")
        assign = assign.to(device=dev, dtype=torch.int64)
        if metric == "l2" and bias is None:
            bias = _l2_bias(item_emb)
        order = torch.sort(assign, stable=True).indices
        counts = torch.bincount(assign, minlength=nlist)
        if counts.numel() != nlist:
            raise ValueError("assign holds a list id outside [0, nlist)")
        padded = (counts + (LIST_ALIGN - 1)) // LIST_ALIGN * LIST_ALIGN
        begin = torch.cumsum(padded, 0) - padded
        P = max(int(padded.sum()), LIST_ALIGN)
        lst = assign.index_select(0, order)
        pos = begin.index_select(0, lst) + (torch.arange(N, device=dev) - (torch.cumsum(counts, 0) - counts).index_select(0, lst))
        rows = torch.zeros(P, E, dtype=torch.bfloat16, device=dev)
        rows[pos] = item_emb.index_select(0, order).to(torch.bfloat16)
        labels = torch.full((P,), -1, dtype=torch.int32, device=dev)
        labels[pos] = order.to(torch.int32)
        pbias = None
        if bias is not None:
            pbias = torch.zeros(P, dtype=torch.float32, device=dev)
            pbias[pos] = bias.to(device=dev, dtype=torch.float32).index_select(0, order)
        if centroids is None:
            centroids = torch.zeros(nlist, E, dtype=torch.float32, device=dev)
            seg = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)])
            ops.ivf_segment_mean(item_emb, order, seg, centroids)
        centroids = centroids.to(device=dev, dtype=torch.float32).contiguous()
        return cls(centroids, _l2_bias(centroids), rows, pbias, labels, begin, counts.to(torch.int32), metric, N)

    def restricted(self, allow: torch.Tensor) -> "IVFIndex":
        """A view of this index restricted to the items ``allow`` admits (bool [N] over the item
        rows, or ops.pack_allow_mask's int32 words). It shares all seven tensors of the base index
        (no row is copied: a mask costs P / 8 + L / 8 bytes) and carries the mask in list order.
        restricted() of a restricted view applies the new mask to the base: masks are not ANDed."""
        if not isinstance(allow, torch.Tensor) or allow.dim() != 1:
            raise ValueError("allow must be bool [N] or ops.pack_allow_mask's int32 words")
        if allow.dtype == torch.bool:
            if allow.numel() != self.N:
                raise ValueError(f"allow must have N = {self.N} entries, not {allow.numel()}")
        elif allow.dtype == torch.int32:
            if allow.numel() != (self.N + 31) // 32:
                raise ValueError(f"allow must have ceil(N / 32) = {(self.N + 31) // 32} words, not {allow.numel()}")
        else:
            raise ValueError("allow must be bool [N] or ops.pack_allow_mask's int32 words")
        allow = allow.to(self.labels.device)
        words = (ops.pack_allow_mask(allow) if allow.dtype == torch.bool else allow).contiguous()
        view = IVFIndex(*(getattr(self, n) for n in self._TENSORS), metric=self.metric, N=self.N)
        view.row_allow, view.list_allow, view.list_eligible = ops.ivf_mask_lists(
            words, self.N, self.labels, self.list_begin, self.list_len)
        view.eligible = view.list_eligible.sum()
        return view

    def state_dict(self) -> Dict[str, object]:
        if self.row_allow is not None:
            raise ValueError("a restricted view is not saved: a mask is per request; save the base index")
        d: Dict[str, object] = {n: getattr(self, n) for n in self._TENSORS}
        d["metric"], d["N"] = self.metric, self.N
        return d

    @classmethod
    def from_state_dict(cls, d: Dict[str, object], device=None) -> "IVFIndex":
        t = {n: (d[n] if d[n] is None or device is None else d[n].to(device)) for n in cls._TENSORS}
        return cls(metric=d["metric"], N=d["N"], **t)

    def probes(self, user_emb: torch.Tensor, nprobe: int) -> torch.Tensor:
        """The coarse step: int32 [M, min(nprobe, 64, L)], each query's nearest centroids (by L2 for
        metric "l2", by inner product for "dot"). ``nprobe`` is clamped to [1, min(64, L)]: 64 is
        the most lists tt_ivf_scan takes per query. On a restricted view only lists that hold an
        eligible item count (the exact filtered kernel with ``list_allow`` as the item mask); where
        fewer than nprobe such lists exist the tail columns are -1, which the scan takes for "no
        probe"."""
        nprobe = max(1, min(int(nprobe), MAX_NPROBE, self.nlist))
        ids, _ = ops.topk_mips(user_emb, self.centroids, nprobe,
                               bias=self.centroid_bias if self.metric == "l2" else None, allow=self.list_allow)
        return ids.to(torch.int32)

    def search(self, user_emb: torch.Tensor, k: int, nprobe: int,
               seen: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               query_chunk: int = 1 << 16) -> Tuple[torch.Tensor, torch.Tensor]:
        """(ids [M, k] int64 item row indices, -1 where fewer than k are left; scores [M, k] fp32):
        the top ``k`` of each query over its ``nprobe`` nearest lists (at most 64, clamped to L).
        ``seen``: (values int32 [S] item rows, ascending per query as ops.sort_exclusions leaves
        them, offsets int64 [M + 1]), never returned to that query. On a restricted view, over the
        eligible items only."""
        M = user_emb.shape[0]
        ids = torch.empty(M, k, dtype=torch.int64, device=user_emb.device)
        scores = torch.empty(M, k, dtype=torch.float32, device=user_emb.device)
        for lo in range(0, M, query_chunk):
            n = min(query_chunk, M - lo)
            q = user_emb[lo:lo + n]
            exclude = None if seen is None else (seen[0], seen[1][lo:lo + n + 1])
            i, s = ops.ivf_scan(q, self.rows, self.labels, self.list_begin, self.list_len, self.probes(q, nprobe), k,
                                bias=self.bias, exclude=exclude, row_allow=self.row_allow)
            ids[lo:lo + n] = i
            scores[lo:lo + n] = s
        return ids, scores


def build_ivf_index(item_emb: torch.Tensor, nlist: int, metric: str = "dot", iters: int = 10,
                    sample: Optional[int] = None, seed: int = 0, init_centroids: Optional[torch.Tensor] = None,
                    chunk: int = 1 << 20) -> IVFIndex:
    """k-means (Lloyd, always by L2, as is usual also for inner-product search) over a seeded sample
    of min(N, 256 * nlist) rows (``sample``: another size), then every row assigned to its nearest
    centroid, ``chunk`` rows per launch, and packed (IVFIndex.from_assignment). The initial centroids
    are the first ``nlist`` sample rows, or ``init_centroids`` (a warm start from the previous
    epoch's index). Assignment is ops.topk_mips(k = 1) with l2_bias(centroids); the update is the
    per-list mean in a fixed summation order (ops.ivf_segment_mean), an empty list keeps its
    centroid: the same inputs and seed give bit-identical index tensors."""
    N, E = item_emb.shape
    dev = item_emb.device
    if not 1 <= nlist <= N:
        raise ValueError("nlist must be in [1, N]")
    ns = min(N, 256 * nlist if sample is None else max(int(sample), nlist))
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    pick = torch.randperm(N, generator=g)[:ns].to(dev)
    pts = item_emb.index_select(0, pick).to(torch.float32)
    if init_centroids is None:
        cent = pts[:nlist].clone()
    else:
        if tuple(init_centroids.shape) != (nlist, E):
            raise ValueError("init_centroids must be [nlist, E]")
        cent = init_centroids.to(device=dev, dtype=torch.float32).clone()
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    for _ in range(iters):
        a = ops.topk_mips(pts, cent, 1, bias=_l2_bias(cent))[0][:, 0]
        order = torch.sort(a, stable=True).indices
        seg = torch.cat([zero, torch.cumsum(torch.bincount(a, minlength=nlist), 0)])
        ops.ivf_segment_mean(pts, order, seg, cent)
    cb = _l2_bias(cent)
    assign = torch.empty(N, dtype=torch.int64, device=dev)
    for lo in range(0, N, chunk):
        assign[lo:lo + chunk] = ops.topk_mips(item_emb[lo:lo + chunk], cent, 1, bias=cb)[0][:, 0]
    return IVFIndex.from_assignment(item_emb, assign, nlist, metric=metric, centroids=cent)
