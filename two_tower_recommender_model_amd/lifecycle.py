"""Checkpoint, evaluation, embedding export and retrieval evaluation around the fused steps
(SURVEY.md section 8(f) rows 2-4), in the reference's formats.

* Checkpoint (03_model_training.py:474-502 writes, :1015-1054 reads): the gathered state dict of
  ``TwoTowerTrainTask`` — keys ``two_tower.ebc.embedding_bags.t_<feature>.weight`` (full tables,
  fp32), ``two_tower.query_proj._mlp.<l>._linear.{weight,bias}`` and ``candidate_proj`` alike —
  which ``get_mlflow_model`` strips of "two_tower." (k[10:]) and loads into TwoTower. The optimizer
  state (row-wise Adagrad sums, Adam moments and step), absent from the reference, is a second dict
  so training can resume bit-exactly.
* Evaluation (03:504-566): forward only over a stream of batches; AUROC of sigmoid(logits)
  (torchmetrics binary AUROC, metrics.py) and the reference's average loss, which divides the SUM
  OF PER-BATCH MEAN LOSSES by the number of samples (03:550-559) — kept as is, with the per-sample
  mean reported beside it.
* Embedding export (03:1056-1122, :1160-1240): every row of a table through its tower (EBC of a
  one-id bag = the row itself, then the MLP with ReLU on every layer); row i is labelled id i + 1
  as the reference does (:1168, :1235), which is NOT the training map id -> id % N (03:361).
* Retrieval evaluation (04_evaluate_retrieval.py:125-153, :202-226): the top k items of every test
  user, exactly (ops.topk_mips instead of a vector index), by the model's dot product or by L2 as
  the reference's index ranks, and recall@k / precision@k / nDCG@k against a jagged ground truth
  (metrics.retrieval_metrics).
"""
from __future__ import annotations

from typing import TYPE_CHECKING, Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from .metrics import AUROC

if TYPE_CHECKING:
    from .ivf import IVFIndex

DEFAULT_FEATURES = ("user_id", "product_id")  # cat_cols of 03_model_training.py:39


def _tower_views(params: torch.Tensor, in_dims: Sequence[int], layer_sizes: Sequence[int]):
    """[(W, b)] per tower from the flat parameter buffer (tt_tower_shape_t layout)."""
    out, o = [], 0
    for t in range(2):
        layers, i = [], in_dims[t]
        for n in layer_sizes:
            w = params[o:o + n * i].view(n, i)
            o += n * i
            b = params[o:o + n]
            o += n
            layers.append((w, b))
            i = n
        out.append(layers)
    return out


def _dense_items(towers, prefix: str):
    items = {}
    for name, layers in zip(("query_proj", "candidate_proj"), towers):
        for l, (w, b) in enumerate(layers):
            items[f"{prefix}{name}._mlp.{l}._linear.weight"] = w
            items[f"{prefix}{name}._mlp.{l}._linear.bias"] = b
    return items


# ---- single-GPU fused step ---------------------------------------------------------------------


def fused_state_dict(step, feature_names: Sequence[str] = DEFAULT_FEATURES,
                     prefix: str = "two_tower.") -> Dict[str, torch.Tensor]:
    """The reference's gathered state dict of the model trained by a FusedTwoTowerStep (one table
    per feature, feature f -> table t_<feature f>). Tensors are copies on the step's device."""
    sd = {}
    for f, name in enumerate(feature_names):
        sd[f"{prefix}ebc.embedding_bags.t_{name}.weight"] = step.tables.table_view(f).clone()
    towers = _tower_views(step.params, [step.in_q, step.in_c], step.layer_sizes)
    sd.update({k: v.clone() for k, v in _dense_items(towers, prefix).items()})
    return sd


def load_fused_state_dict(step, sd: Dict[str, torch.Tensor], feature_names: Sequence[str] = DEFAULT_FEATURES,
                          prefix: str = "two_tower.") -> None:
    """Inverse of fused_state_dict (a reference checkpoint loads as is); refreshes the towers' bf16
    weight copies."""
    with torch.no_grad():
        for f, name in enumerate(feature_names):
            step.tables.table_view(f).copy_(sd[f"{prefix}ebc.embedding_bags.t_{name}.weight"])
        towers = _tower_views(step.params, [step.in_q, step.in_c], step.layer_sizes)
        for k, v in _dense_items(towers, prefix).items():
            v.copy_(sd[k])
    step.sync_weights()


def fused_optimizer_state(step) -> Dict[str, torch.Tensor]:
    """Row-wise Adagrad sums of every table, Adam moments and step counter (resume state)."""
    st = {f"rowwise_adagrad.t{f}.momentum1": step.tables.state_view(f).clone() for f in range(step.F)}
    st.update({"adam.exp_avg": step.exp_avg.clone(), "adam.exp_avg_sq": step.exp_avg_sq.clone(),
               "adam.step": step.adam_state.clone()})
    return st


def load_fused_optimizer_state(step, st: Dict[str, torch.Tensor]) -> None:
    with torch.no_grad():
        for f in range(step.F):
            step.tables.state_view(f).copy_(st[f"rowwise_adagrad.t{f}.momentum1"])
        step.exp_avg.copy_(st["adam.exp_avg"])
        step.exp_avg_sq.copy_(st["adam.exp_avg_sq"])
        step.adam_state.copy_(st["adam.step"])


# ---- evaluation ----------------------------------------------------------------------------------


def evaluate_fused(step, batches: Iterable[Tuple[Sequence[torch.Tensor], torch.Tensor]],
                   limit_batches: Optional[int] = None) -> Dict[str, float]:
    """evaluate() of 03_model_training.py:504-566 on a FusedTwoTowerStep: forward only (no table or
    tower update), AUROC over all batches, and the reference's average loss (sum of batch means
    / samples). Returns {"avg_loss", "auroc", "mean_loss", "batches", "samples"}."""
    auroc = AUROC(task="binary").to(step.device)
    total_loss = torch.zeros((), dtype=torch.float64, device=step.device)
    n_batches = n_samples = 0
    for i, (cols, labels) in enumerate(batches):
        if limit_batches is not None and i >= limit_batches:
            break
        loss, logits = step.eval_step(cols, labels)
        auroc(torch.sigmoid(logits), labels)
        total_loss += loss.to(torch.float64)
        n_batches += 1
        n_samples += labels.numel()
    total = float(total_loss)
    return {"avg_loss": total / n_samples if n_samples else 0.0, "auroc": float(auroc.compute()),
            "mean_loss": total / n_batches if n_batches else 0.0, "batches": n_batches, "samples": n_samples}


# ---- embedding export ----------------------------------------------------------------------------


def _fused_tower_check(table: torch.Tensor, layers, precision: str) -> None:
    if precision != "bf16":
        raise ValueError("fused=True runs the bf16 chain only: precision must be 'bf16'")
    widths = [w.shape[0] for w, _ in layers]
    if not ops.tower_embed_supported(table.shape[1], widths):
        raise ValueError(f"fused=True: ops.tower_embed does not run a tower {table.shape[1]} -> {widths} "
                         "(ops.tower_embed_supported)")


def export_embeddings(table: torch.Tensor, layers: Sequence[Tuple[torch.Tensor, torch.Tensor]],
                      chunk: int = 1 << 20, precision: str = "bf16",
                      out: Optional[torch.Tensor] = None, fused: bool = False,
                      out_dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """process_embeddings (03:1089-1117) for every row of ``table`` ([N, D] fp32, device): the
    tower MLP (Linear + ReLU on every layer) on bf16 MFMA GEMMs (fp32 accumulate; "fp32" for the
    exact path), ``chunk`` rows per launch. Returns (ids = arange(N) + 1 — the reference's labels —,
    embeddings [N, out]).

    ``fused=True``: each chunk is one ops.tower_embed launch over its row range instead of one
    linear_fwd per layer (no hidden activation leaves the chip; the same bits; ``precision`` must be
    "bf16" and the tower a shape ops.tower_embed_supported accepts, else ValueError). Only then may
    ``out_dtype`` be torch.bfloat16: the embeddings rounded once to nearest-even, which is what every
    retrieval kernel makes of fp32 items on load."""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("out_dtype must be torch.float32 or torch.bfloat16")
    if out_dtype != torch.float32 and not fused:
        raise ValueError("out_dtype=torch.bfloat16 needs fused=True (the per-layer path writes fp32)")
    N = table.shape[0]
    width = layers[-1][0].shape[0]
    if fused:
        _fused_tower_check(table, layers, precision)
    if out is None:
        out = torch.empty(N, width, dtype=out_dtype, device=table.device)
    elif out.dtype != out_dtype:
        raise ValueError("out's dtype must be out_dtype")
    for lo in range(0, N, chunk):
        if fused:
            n = min(chunk, N - lo)
            ops.tower_embed(table, layers, first_row=lo, count=n, out=out[lo:lo + n])
            continue
        x = table[lo:lo + chunk]
        for l, (w, b) in enumerate(layers):
            y = out[lo:lo + chunk] if l == len(layers) - 1 else None
            x = ops.linear_fwd([x], [w.contiguous()], [b], relu=True, outs=[y] if y is not None else None,
                               precision=precision)[0]
    ids = torch.arange(1, N + 1, dtype=torch.int64, device=table.device)
    return ids, out


def export_fused(step, tower: str = "candidate", **kw) -> Tuple[torch.Tensor, torch.Tensor]:
    """export_embeddings of a FusedTwoTowerStep's item ("candidate", table 1) or user ("query",
    table 0) tower; ``fused`` and ``out_dtype`` (and the rest) as export_embeddings."""
    t = 1 if tower == "candidate" else 0
    towers = _tower_views(step.params, [step.in_q, step.in_c], step.layer_sizes)
    return export_embeddings(step.tables.table_view(t), towers[t], **kw)


# ---- retrieval evaluation (04_evaluate_retrieval.py) ---------------------------------------------


def l2_bias(item_emb: torch.Tensor, chunk: int = 1 << 20) -> torch.Tensor:
    """bias[n] = -0.5 |c_n|^2 of the bf16-rounded rows (what the kernel multiplies), fp32: with it
    the inner-product order is the ascending-L2 order, |q - c|^2 = |q|^2 - 2 (q.c - 0.5 |c|^2)."""
    out = torch.empty(item_emb.shape[0], dtype=torch.float32, device=item_emb.device)
    for lo in range(0, item_emb.shape[0], chunk):
        c = item_emb[lo:lo + chunk].to(torch.bfloat16).to(torch.float64)
        out[lo:lo + chunk] = (-0.5 * (c * c).sum(1)).to(torch.float32)
    return out


def _retrieval_filters(N: int, M: int, device, allow, seen_values, seen_offsets):
    """(packed allow words or None, (sorted int32 item rows, int64 offsets [M + 1]) or None) of
    retrieve()'s filter arguments, on ``device``."""
    if allow is not None:
        allow = allow.to(device)
        if allow.dtype == torch.bool:
            if allow.numel() != N:
                raise ValueError("allow must be bool [N] over the item rows, or the packed int32 words")
            allow = ops.pack_allow_mask(allow)
    if (seen_values is None) != (seen_offsets is None):
        raise ValueError("seen_values and seen_offsets go together")
    if seen_values is None:
        return allow, None
    if seen_offsets.numel() != M + 1:
        raise ValueError("seen_offsets must have M + 1 entries")
    offsets = seen_offsets.to(device=device, dtype=torch.int64).contiguous()
    # label i + 1 is row i; a label outside 1..N is a row outside [0, N), which sort_exclusions
    # turns into "no item"
    rows = ops.sort_exclusions(seen_values.to(device=device, dtype=torch.int64) - 1, offsets, N)
    return allow, (rows, offsets)


# The workspace one call of the large-k selection (256 < k <= 8192) may take: it holds splits * M pools
# of 2 k + 32 keys, and retrieve()'s default of 65,536 queries per call would be 8.6 GB at k = 8192 with
# one split alone. 4 GiB is 1.4 % of an MI355X's HBM and about the size of the reference-scale item
# embeddings beside it; it still gives every CU a workgroup at k = 8192 (32,700 pools = 255
# workgroups of 128 queries) and near-full residency at the reference's k = 5000 (53,500 pools).
LARGE_K_WORKSPACE_BYTES = 4 << 30


def _check_index_k(k: int, index) -> None:
    if index is not None and k > _lib.TT_TOPK_MAX_K:
        raise ValueError(f"k = {k} with an index: the IVF list scan's limit is k <= {_lib.TT_TOPK_MAX_K} "
                         "(exact retrieval, index=None, goes up to 8192)")


def _large_k_plan(M: int, N: int, k: int, query_chunk: int) -> Tuple[int, Optional[int]]:
    """(queries per call, splits) of the large-k selection under LARGE_K_WORKSPACE_BYTES: the chunk is
    ``query_chunk`` lowered to the pools that fit (whole workgroups of 128 queries where it is cut);
    splits is None (the library's choice) where that fits too, else what is left of the pools."""
    pools = max(1, LARGE_K_WORKSPACE_BYTES // ((2 * k + 32) * 8))
    n = min(query_chunk, M)
    if n > pools:
        n = max(pools // 128 * 128, min(pools, 128))
    auto = ops.topk_mips_large_workspace_bytes(n, N, k)
    if 0 < auto <= LARGE_K_WORKSPACE_BYTES:
        return n, None
    return n, max(1, min(64, pools // n))


def retrieve(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int = 100, metric: str = "dot",
             query_chunk: int = 1 << 16, bias: Optional[torch.Tensor] = None, allow: Optional[torch.Tensor] = None,
             seen_values: Optional[torch.Tensor] = None, seen_offsets: Optional[torch.Tensor] = None,
             index: Optional["IVFIndex"] = None, nprobe: int = 32) -> Tuple[torch.Tensor, torch.Tensor]:
    """The query loop of 04_evaluate_retrieval.py:131-153 without an index: for each row of
    ``user_emb`` the exact top ``k`` rows of ``item_emb`` (ops.topk_mips; ops.topk_mips_large for
    256 < k <= 8192, with ``query_chunk`` lowered so that a call's workspace stays under
    LARGE_K_WORKSPACE_BYTES), ``query_chunk`` queries per launch. ``metric``: "dot" (the model's own score) or "l2" (the order of the reference's vector
    index; ``bias`` = l2_bias(item_emb), computed here when not passed). Returns (ids [M, k] int64
    in the reference's labels — row i is id i + 1, as export_embeddings; 0 past the table —, scores
    [M, k] fp32: q.c, or q.c - 0.5 |c|^2 for "l2").

    Filters (tt_topk_mips_filtered; all None: the unfiltered call): ``allow`` restricts the catalogue
    for every query (bool [N] over the item rows, or ops.pack_allow_mask's words: the index's
    ``filters=`` of 04_evaluate_retrieval.py:100); ``seen_values`` / ``seen_offsets`` [M + 1] are each
    user's already-seen items (jagged, in the reference's labels as ``target_values``; labels outside
    1..N are dropped), never returned to that user. The lists are sorted once; a chunk of queries
    takes a view of the offsets.

    ``index`` (ivf.IVFIndex over the same ``item_emb``, built for the same ``metric``): the
    approximate query instead, each user against its ``nprobe`` nearest lists only
    (IVFIndex.search; ``nprobe`` is clamped to min(nprobe, 64, the index's lists)); ids, scores and the seen lists as above, ``item_emb`` and ``bias`` are not
    read (the index holds its own copy). An item mask goes to the index itself, as the reference's
    ``filters=`` does: pass ``index=index.restricted(allow)`` (the coarse step then counts only lists
    with an eligible item, the fine step is the masked list scan); ``allow=`` beside ``index=`` is
    refused, and so is k > 256 (the IVF list scan's limit)."""
    if metric not in ("dot", "l2"):
        raise ValueError("metric must be 'dot' or 'l2'")
    _check_index_k(k, index)
    if index is not None:
        if allow is not None:
            raise ValueError("allow masks are not supported with an index: pass index=index.restricted(allow) "
                             "(IVFIndex.restricted)")
        if index.metric != metric:
            raise ValueError(f"the index was built for metric {index.metric!r}, not {metric!r}")
        _, seen = _retrieval_filters(index.N, user_emb.shape[0], user_emb.device, None, seen_values, seen_offsets)
        i, s = index.search(user_emb, k, nprobe, seen=seen, query_chunk=query_chunk)
        return i + 1, s
    if metric == "l2" and bias is None:
        bias = l2_bias(item_emb)
    if metric == "dot":
        bias = None
    M = user_emb.shape[0]
    allow, seen = _retrieval_filters(item_emb.shape[0], M, user_emb.device, allow, seen_values, seen_offsets)
    ids = torch.empty(M, k, dtype=torch.int64, device=user_emb.device)
    scores = torch.empty(M, k, dtype=torch.float32, device=user_emb.device)
    large = k > _lib.TT_TOPK_MAX_K  # the pooled selection (ops.topk_mips_large), its workspace bounded
    splits = None
    if large and k <= _lib.TT_TOPK_LARGE_MAX_K and M > 0:
        query_chunk, splits = _large_k_plan(M, item_emb.shape[0], k, query_chunk)
    for lo in range(0, M, query_chunk):
        n = min(query_chunk, M - lo)
        exclude = None if seen is None else (seen[0], seen[1][lo:lo + n + 1])
        if large:
            i, s = ops.topk_mips_large(user_emb[lo:lo + n], item_emb, k, bias=bias, splits=splits, allow=allow,
                                       exclude=exclude)
        else:
            i, s = ops.topk_mips(user_emb[lo:lo + n], item_emb, k, bias=bias, allow=allow, exclude=exclude)
        ids[lo:lo + query_chunk] = i + 1
        scores[lo:lo + query_chunk] = s
    return ids, scores


def _query_embeddings(step, user_rows: torch.Tensor, fused: bool) -> torch.Tensor:
    """Rows ``user_rows`` of the user table through the query tower: a gather and one linear_fwd per
    layer, or (``fused``) one ops.tower_embed launch over the row list."""
    towers = _tower_views(step.params, [step.in_q, step.in_c], step.layer_sizes)
    table = step.tables.table_view(0)
    if fused:
        _fused_tower_check(table, towers[0], "bf16")
        rows = user_rows.to(step.device)
        if rows.dtype not in (torch.int32, torch.int64):
            rows = rows.to(torch.int64)
        return ops.tower_embed(table, towers[0], rows=rows.contiguous())
    x = table[user_rows.to(step.device)]
    for w, b in towers[0]:
        x = ops.linear_fwd([x], [w.contiguous()], [b], relu=True)[0]
    return x


def retrieve_fused(step, user_rows: torch.Tensor, k: int = 100, metric: str = "dot",
                   item_emb: Optional[torch.Tensor] = None, allow: Optional[torch.Tensor] = None,
                   seen_values: Optional[torch.Tensor] = None, seen_offsets: Optional[torch.Tensor] = None,
                   query_chunk: int = 1 << 16, index: Optional["IVFIndex"] = None,
                   nprobe: int = 32, fused: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """retrieve() for a FusedTwoTowerStep: rows ``user_rows`` (int64 row indices) of the user table
    through the query tower (as export does), against the item table through the candidate tower
    (export_fused, unless its embeddings ``item_emb`` are passed in). ``allow``, ``seen_values`` /
    ``seen_offsets``, ``query_chunk``, ``index`` and ``nprobe`` as retrieve() (with an index the
    item tower is not run; an item mask with an index is ``index=index.restricted(allow)``).
    ``fused=True``: the query embeddings are one ops.tower_embed launch over ``user_rows`` in place of
    the gather and the per-layer launches, and the item export, where it is computed here, is the
    fused one; the same bits either way."""
    _check_index_k(k, index)
    x = _query_embeddings(step, user_rows, fused)
    if item_emb is None and index is None:
        item_emb = export_fused(step, "candidate", fused=fused)[1]
    return retrieve(x, item_emb, k=k, metric=metric, query_chunk=query_chunk, allow=allow, seen_values=seen_values,
                    seen_offsets=seen_offsets, index=index, nprobe=nprobe)


def evaluate_retrieval(step, user_rows: torch.Tensor, target_values: torch.Tensor, target_offsets: torch.Tensor,
                       k: int = 100, metric: str = "dot", item_emb: Optional[torch.Tensor] = None,
                       allow: Optional[torch.Tensor] = None, seen_values: Optional[torch.Tensor] = None,
                       seen_offsets: Optional[torch.Tensor] = None, query_chunk: int = 1 << 16,
                       index: Optional["IVFIndex"] = None, nprobe: int = 32, fused: bool = False) -> Dict[str, object]:
    """Retrieval evaluation of 04_evaluate_retrieval.py:202-226 (mlflow.evaluate, model_type
    "retriever"): the top ``k`` item ids of every user row against its jagged ground truth
    (``target_values`` item ids in the reference's labels, ``target_offsets`` [M + 1]);
    metrics.retrieval_metrics' dict. ``allow`` and ``seen_values`` / ``seen_offsets`` as retrieve():
    with each user's training positives as the seen set, the held-out items are ranked among the
    items the user has not seen, which is the usual protocol. ``index`` / ``nprobe`` as retrieve():
    the approximate query (ivf.IVFIndex, or its restricted(allow) view for an item mask) in place of
    the exact one. ``fused`` as retrieve_fused()."""
    from .metrics import retrieval_metrics

    ids, _ = retrieve_fused(step, user_rows, k=k, metric=metric, item_emb=item_emb, allow=allow,
                            seen_values=seen_values, seen_offsets=seen_offsets, query_chunk=query_chunk, index=index,
                            nprobe=nprobe, fused=fused)
    ids = torch.where(ids > 0, ids, torch.full_like(ids, -1))  # padding (label 0) is no id
    return retrieval_metrics(ids, target_values.to(ids.device), target_offsets.to(ids.device), k)


# ---- full-catalogue rank evaluation ---------------------------------------------------------------


def target_ranks(user_emb: torch.Tensor, item_emb: torch.Tensor, target_values: torch.Tensor,
                 target_offsets: torch.Tensor, metric: str = "dot", bias: Optional[torch.Tensor] = None,
                 allow: Optional[torch.Tensor] = None, seen_values: Optional[torch.Tensor] = None,
                 seen_offsets: Optional[torch.Tensor] = None, query_chunk: int = 1 << 16) -> torch.Tensor:
    """Each held-out item's exact rank in its user's order of the whole catalogue (ops.target_ranks):
    what retrieve() would put at column ``rank`` for any k above it, without a list and without a limit
    on k. ``target_values`` are item ids in the reference's labels (label i + 1 is row i, as
    retrieve()'s ids), ``target_offsets`` [M + 1] from 0; ``metric``, ``bias``, ``allow``,
    ``seen_values`` / ``seen_offsets`` and ``query_chunk`` as retrieve(). Returns ranks int64 [T],
    0-based; -1 for a label outside 1..N, an item that ``allow`` denies, or one the user has seen."""
    if metric not in ("dot", "l2"):
        raise ValueError("metric must be 'dot' or 'l2'")
    if metric == "l2" and bias is None:
        bias = l2_bias(item_emb)
    if metric == "dot":
        bias = None
    M, N, dev = user_emb.shape[0], item_emb.shape[0], user_emb.device
    if target_offsets.numel() != M + 1:
        raise ValueError("target_offsets must have M + 1 entries")
    allow, seen = _retrieval_filters(N, M, dev, allow, seen_values, seen_offsets)
    # label -> row; a label outside 1..N becomes row -1, which no item has
    rows = target_values.to(device=dev, dtype=torch.int64) - 1
    rows = torch.where((rows >= 0) & (rows < N), rows, torch.full_like(rows, -1)).to(torch.int32).contiguous()
    offsets = target_offsets.to(device=dev, dtype=torch.int64).contiguous()
    ranks = torch.full((rows.numel(),), -1, dtype=torch.int64, device=dev)
    for lo in range(0, M, query_chunk):
        n = min(query_chunk, M - lo)
        exclude = None if seen is None else (seen[0], seen[1][lo:lo + n + 1])
        ops.target_ranks(user_emb[lo:lo + n], item_emb, rows, offsets[lo:lo + n + 1], bias=bias, allow=allow,
                         exclude=exclude, out=(ranks, None))
    return ranks


def evaluate_ranks(step, user_rows: torch.Tensor, target_values: torch.Tensor, target_offsets: torch.Tensor,
                   ks: Sequence[int] = (1, 10, 100, 1000), metric: str = "dot", item_emb: Optional[torch.Tensor] = None,
                   allow: Optional[torch.Tensor] = None, seen_values: Optional[torch.Tensor] = None,
                   seen_offsets: Optional[torch.Tensor] = None, query_chunk: int = 1 << 16,
                   fused: bool = False) -> Dict[str, object]:
    """evaluate_retrieval() under the full-ranking protocol: every held-out item's exact rank among the
    items its user may be shown (target_ranks above; the query tower as retrieve_fused runs it, the
    item tower by export_fused unless ``item_emb`` is passed), then metrics.rank_metrics' dict:
    recall@k and nDCG@k for every k of ``ks`` from the one pass — equal to evaluate_retrieval's at
    each k —, MRR, the mean and median rank. No k limit and no top-k selection. The exact order only:
    ranks under an IVF index are not defined here. ``fused`` as retrieve_fused()."""
    from .metrics import rank_metrics

    x = _query_embeddings(step, user_rows, fused)
    if item_emb is None:
        item_emb = export_fused(step, "candidate", fused=fused)[1]
    ranks = target_ranks(x, item_emb, target_values, target_offsets, metric=metric, allow=allow, seen_values=seen_values,
                         seen_offsets=seen_offsets, query_chunk=query_chunk)
    return rank_metrics(ranks, target_offsets.to(ranks.device), ks)
