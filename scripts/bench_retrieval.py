"""Exact top-k retrieval (ops.topk_mips: tt_topk_mips, the fused score + select kernel) against the
torch composition on the same GPU: bf16 torch.matmul over item chunks, torch.topk of each score
chunk and a running merge of the best k. Interleaved runs of the two arms after a warm-up, timed with
HIP events; prints one JSON line (medians, the runs, the spread). Inputs are seeded, generated on the
device; nothing is read from outside the tree.

    python scripts/bench_retrieval.py                       # M 4096, N 4,194,304, E 64, k 100
    python scripts/bench_retrieval.py --M 10000 --N 100000000 --items bf16 --no-baseline --runs 1
    python scripts/bench_retrieval.py --no-baseline --filter    # + the filtered arms, --seen 256

At --k > 256 (up to 8192) the ``fused`` arm is ops.topk_mips_large (tt_topk_mips_large: pooled radix
selection); --large adds the arm ``fused_large``, that kernel at any k, with its ratio to ``fused`` and
whether the two results are equal (at k <= 256 this prices the new selection where both exist).

--filter adds two arms of tt_topk_mips_filtered to the interleaved runs: ``filtered_noop`` (an
all-ones item mask and empty exclusion lists: the price of the filtered kernel itself) and
``filtered`` (a seeded mask with ~90 % ones and --seen seeded uniform item ids per query, sorted), and
prints each one's ratio to ``fused`` of the same process.

    python scripts/bench_retrieval.py --no-baseline --clusters 2048 --ivf 2048 --nprobe 1,8,32

--ivf NLIST builds an IVF index (ivf.build_ivf_index) on the bench inputs and adds, per value of
--nprobe, three arms to the interleaved runs: ``ivf_npP`` (IVFIndex.search: coarse step + list scan),
``ivf_npP_coarse`` (the probes alone) and ``ivf_npP_scan`` (ops.ivf_scan on probes computed before);
it prints the build time, each arm's ratio to ``fused`` of the same process and recall@k of the IVF
ids against the exact ids. --clusters C draws items and queries from a seeded mixture of C Gaussians
(centres 0.5 N(0, I), --sigma per coordinate): uniform random vectors have no list structure.

    python scripts/bench_retrieval.py --no-baseline --filter --clusters 2048 --ivf 2048 --nprobe 8,32

--ivf with --filter adds the item mask on the index (IVFIndex.restricted: tt_ivf_mask_lists and
tt_ivf_scan_masked), per value of --nprobe: ``ivf_npP_masked_noop`` (an all-ones mask: the price of
the masked path; ``..._noop_scan`` is its scan alone, on the probes of ``ivf_npP_scan``),
``ivf_npP_masked90`` (the seeded ~90 % mask of the ``filtered`` arm, without its seen lists) and, at a
seeded ~5 % mask, ``ivf_npP_masked5_plain`` (the unrestricted index's probes, masked scan) against
``ivf_npP_masked5_aware`` (the restricted view's search: probes that count only lists with an
eligible item); and the same pair at a "department" mask, the items of every 20th list
(``ivf_npP_maskeddept_plain`` / ``_aware``): a uniform mask leaves an eligible item in every list, a
structured one empties most of a query's nearest lists. Each arm's recall@k is against the exact ops.topk_mips(allow=) ids of its mask; the
time of restricted() itself is printed per mask.

    python scripts/bench_retrieval.py --no-baseline --ranks 1,8,20

--ranks T (or a comma-separated list) adds, per value, the arm ``ranks_tT`` to the interleaved runs:
ops.target_ranks (tt_target_ranks: each target's exact rank in the whole catalogue, no top-k) of T seeded
uniform random targets per query, with its ratio to ``fused`` of the same process, the number of
(query, target) pairs and the mean rank it found (uniform targets: about N / 2).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from two_tower_recommender_model_amd import ops  # noqa: E402


def torch_arm(q16, c16, k, chunk):
    best_s = best_i = None
    for lo in range(0, c16.shape[0], chunk):
        s = q16 @ c16[lo:lo + chunk].T  # [M, chunk] bf16: the score chunk goes through HBM
        v, i = torch.topk(s, min(k, s.shape[1]), dim=1)
        i = i + lo
        if best_s is None:
            best_s, best_i = v, i
        else:
            v, j = torch.topk(torch.cat([best_s, v], 1), k, dim=1)
            best_s, best_i = v, torch.cat([best_i, i], 1).gather(1, j)
    return best_i, best_s


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def recall(got, exact):
    """Share of the exact ids (those >= 0) that `got` holds in the same row."""
    hit = 0
    for lo in range(0, exact.shape[0], 1024):
        e = exact[lo:lo + 1024]
        hit += int(((got[lo:lo + 1024].unsqueeze(2) == e.unsqueeze(1)).any(1) & (e >= 0)).sum())
    return round(hit / max(1, int((exact >= 0).sum())), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--N", type=int, default=4194304)
    ap.add_argument("--E", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--items", choices=["f32", "bf16"], default="f32", help="item dtype of the fused arm")
    ap.add_argument("--chunk", type=int, default=65536, help="items per matmul of the torch arm")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--splits", type=int, default=None)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--filter", action="store_true", help="add the filtered_noop and filtered arms")
    ap.add_argument("--large", action="store_true", help="add the fused_large arm (tt_topk_mips_large at any k)")
    ap.add_argument("--seen", type=int, default=256, help="excluded ids per query of the filtered arm")
    ap.add_argument("--ranks", default="", metavar="T", help="add the ranks_tT arms: T random targets per query (comma-separated)")
    ap.add_argument("--ivf", type=int, default=0, metavar="NLIST", help="add the IVF arms over an index of NLIST lists")
    ap.add_argument("--nprobe", default="1,8,32", help="comma-separated nprobe values of the IVF arms")
    ap.add_argument("--ivf-iters", type=int, default=10, help="k-means iterations of the index build")
    ap.add_argument("--clusters", type=int, default=0, metavar="C", help="inputs from a mixture of C Gaussians")
    ap.add_argument("--sigma", type=float, default=0.15, help="per-coordinate noise of the mixture")
    a = ap.parse_args()

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(a.M, a.E, device=dev, generator=g) * 0.5
    centres = None
    if a.clusters:
        centres = torch.randn(a.clusters, a.E, device=dev, generator=g) * 0.5
        q = centres[torch.randint(0, a.clusters, (a.M,), device=dev, generator=g)] + a.sigma * q / 0.5
    gen_dtype = torch.float32 if a.items == "f32" else torch.bfloat16
    c = torch.empty(a.N, a.E, dtype=gen_dtype, device=dev)
    for lo in range(0, a.N, 1 << 22):  # in pieces: the generator's fp32 temporary stays small
        n = min(1 << 22, a.N - lo)
        x = torch.randn(n, a.E, device=dev, generator=g) * 0.5
        if centres is not None:
            x = centres[torch.randint(0, a.clusters, (n,), device=dev, generator=g)] + a.sigma * x / 0.5
        c[lo:lo + n] = x
    q16 = q.to(torch.bfloat16)
    c16 = c if a.items == "bf16" or a.no_baseline else c.to(torch.bfloat16)  # the torch arm's operands (not timed)

    def fused_large():
        return ops.topk_mips_large(q, c, a.k, splits=a.splits)

    def fused():  # past tt_topk_mips' limit of 256 the exact kernel is the pooled selection
        return ops.topk_mips(q, c, a.k, splits=a.splits) if a.k <= 256 else fused_large()

    def composed():
        return torch_arm(q16, c16, a.k, a.chunk)

    arms = {"fused": fused} if a.no_baseline else {"fused": fused, "torch": composed}
    if a.large:
        arms["fused_large"] = fused_large
    if a.filter:
        ones = ops.pack_allow_mask(torch.ones(a.N, dtype=torch.bool, device=dev))
        empty = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(a.M + 1, dtype=torch.int64, device=dev))
        mask = ops.pack_allow_mask(torch.rand(a.N, device=dev, generator=g) < 0.9)
        offs = torch.arange(a.M + 1, dtype=torch.int64, device=dev) * a.seen
        seen = (ops.sort_exclusions(torch.randint(0, a.N, (a.M * a.seen,), device=dev, generator=g), offs, a.N), offs)
        arms["filtered_noop"] = lambda: ops.topk_mips(q, c, a.k, splits=a.splits, allow=ones, exclude=empty)
        arms["filtered"] = lambda: ops.topk_mips(q, c, a.k, splits=a.splits, allow=mask, exclude=seen)
    rank_ts = [int(x) for x in a.ranks.split(",")] if a.ranks else []
    for T in rank_ts:
        tv = torch.randint(0, a.N, (a.M * T,), device=dev, generator=g).to(torch.int32)
        to = torch.arange(a.M + 1, dtype=torch.int64, device=dev) * T
        arms[f"ranks_t{T}"] = lambda tv=tv, to=to: ops.target_ranks(q, c, tv, to, splits=a.splits)
    nprobes = [int(x) for x in a.nprobe.split(",")] if a.ivf else []
    if a.ivf:
        from two_tower_recommender_model_amd.ivf import build_ivf_index

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = build_ivf_index(c, a.ivf, metric="dot", iters=a.ivf_iters, seed=0)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        for p in nprobes:
            probes = index.probes(q, p)
            arms[f"ivf_np{p}"] = lambda p=p: index.search(q, a.k, p)
            arms[f"ivf_np{p}_coarse"] = lambda p=p: index.probes(q, p)
            arms[f"ivf_np{p}_scan"] = lambda probes=probes: ops.ivf_scan(
                q, index.rows, index.labels, index.list_begin, index.list_len, probes, a.k, bias=index.bias)
        masked_ref, mask_prep_ms = {}, {}
        if a.filter:
            mask5 = ops.pack_allow_mask(torch.rand(a.N, device=dev, generator=g) < 0.05)
            # the items of every 20th list: the row's list from list_begin, the item from its label
            row_list = torch.searchsorted(index.list_begin, torch.arange(index.labels.numel(), device=dev), right=True) - 1
            dept_rows = (row_list % 20 == 0) & (index.labels >= 0)
            dept = torch.zeros(a.N, dtype=torch.bool, device=dev)
            dept[index.labels[dept_rows].long()] = True
            maskdept = ops.pack_allow_mask(dept)
            views = {}
            for name, words in (("noop", ones), ("90", mask), ("5", mask5), ("dept", maskdept)):
                index.restricted(words)  # warm-up
                mask_prep_ms[name], views[name] = timed(lambda words=words: index.restricted(words))
            masked_ref = {"masked_noop": None, "masked90": ops.topk_mips(q, c, a.k, splits=a.splits, allow=mask)[0],
                          "masked5_plain": ops.topk_mips(q, c, a.k, splits=a.splits, allow=mask5)[0]}
            masked_ref["masked5_aware"] = masked_ref["masked5_plain"]
            masked_ref["maskeddept_plain"] = ops.topk_mips(q, c, a.k, splits=a.splits, allow=maskdept)[0]
            masked_ref["maskeddept_aware"] = masked_ref["maskeddept_plain"]
            for p in nprobes:
                probes = index.probes(q, p)
                arms[f"ivf_np{p}_masked_noop"] = lambda p=p: views["noop"].search(q, a.k, p)
                arms[f"ivf_np{p}_masked_noop_scan"] = lambda probes=probes: ops.ivf_scan(
                    q, index.rows, index.labels, index.list_begin, index.list_len, probes, a.k, bias=index.bias,
                    row_allow=views["noop"].row_allow)
                arms[f"ivf_np{p}_masked90"] = lambda p=p: views["90"].search(q, a.k, p)
                arms[f"ivf_np{p}_masked5_plain"] = lambda p=p: ops.ivf_scan(
                    q, index.rows, index.labels, index.list_begin, index.list_len, index.probes(q, p), a.k,
                    bias=index.bias, row_allow=views["5"].row_allow)
                arms[f"ivf_np{p}_masked5_aware"] = lambda p=p: views["5"].search(q, a.k, p)
                arms[f"ivf_np{p}_maskeddept_plain"] = lambda p=p: ops.ivf_scan(
                    q, index.rows, index.labels, index.list_begin, index.list_len, index.probes(q, p), a.k,
                    bias=index.bias, row_allow=views["dept"].row_allow)
                arms[f"ivf_np{p}_maskeddept_aware"] = lambda p=p: views["dept"].search(q, a.k, p)
    for _ in range(a.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in arms}
    outs = {}
    for _ in range(a.runs):
        for n, fn in arms.items():
            t, outs[n] = timed(fn)
            ms[n].append(round(t, 3))
    res = {"bench": "retrieval", "M": a.M, "N": a.N, "E": a.E, "k": a.k, "items": a.items, "runs": a.runs,
           "splits": a.splits, "device": torch.cuda.get_device_name(dev)}
    flop = 2.0 * a.M * a.N * a.E
    for n in arms:
        med = statistics.median(ms[n])
        res[n] = {"median_ms": med, "min_ms": min(ms[n]), "max_ms": max(ms[n]), "runs_ms": ms[n]}
        if not n.startswith("ivf_"):  # an IVF arm does not score every pair
            res[n]["tflops"] = round(flop / med / 1e9, 1)
    res["item_bytes"] = c.numel() * c.element_size()
    res["fused"]["item_stream_tb_s"] = round(res["item_bytes"] / res["fused"]["median_ms"] / 1e9, 3)
    if a.filter:
        res["seen"] = a.seen
        for n in ("filtered_noop", "filtered"):
            res[n]["ratio_to_fused"] = round(res[n]["median_ms"] / res["fused"]["median_ms"], 4)
        res["filtered_noop"]["equals_fused"] = bool(torch.equal(outs["filtered_noop"][0], outs["fused"][0]) and
                                                    torch.equal(outs["filtered_noop"][1], outs["fused"][1]))
    for T in rank_ts:
        n = f"ranks_t{T}"
        res[n]["ratio_to_fused"] = round(res[n]["median_ms"] / res["fused"]["median_ms"], 4)
        res[n]["pairs"] = a.M * T
        res[n]["mean_rank"] = round(float(outs[n].to(torch.float64).mean()), 1)
    if a.large:
        res["fused_large"]["ratio_to_fused"] = round(res["fused_large"]["median_ms"] / res["fused"]["median_ms"], 4)
        res["fused_large"]["equals_fused"] = bool(torch.equal(outs["fused_large"][0], outs["fused"][0]) and
                                                  torch.equal(outs["fused_large"][1], outs["fused"][1]))
    if a.ivf:
        lens = index.list_len.to(torch.float64)
        res["ivf"] = {"nlist": a.ivf, "clusters": a.clusters, "sigma": a.sigma, "iters": a.ivf_iters,
                      "build_s": round(build_s, 3), "rows_padded": index.rows.shape[0],
                      "list_len_mean": round(float(lens.mean()), 1), "list_len_max": int(lens.max()),
                      "empty_lists": int((lens == 0).sum())}
        exact = outs["fused"][0]
        for p in nprobes:
            n = f"ivf_np{p}"
            got = outs[n][0]
            res[n]["recall_at_k"] = recall(got, exact)
            for m in (n, n + "_coarse", n + "_scan"):
                res[m]["ratio_to_fused"] = round(res[m]["median_ms"] / res["fused"]["median_ms"], 4)
            res[n]["scan_equals_search"] = bool(torch.equal(outs[n + "_scan"][0], got))
            for arm, ref in masked_ref.items():
                m = f"{n}_{arm}"
                res[m]["recall_at_k"] = recall(outs[m][0], exact if ref is None else ref)
                res[m]["ratio_to_fused"] = round(res[m]["median_ms"] / res["fused"]["median_ms"], 4)
                res[m]["ratio_to_ivf"] = round(res[m]["median_ms"] / res[n]["median_ms"], 4)
            if masked_ref:
                m = n + "_masked_noop"
                res[m]["equals_ivf"] = bool(torch.equal(outs[m][0], got) and torch.equal(outs[m][1], outs[n][1]))
                res[m + "_scan"]["ratio_to_ivf_scan"] = round(res[m + "_scan"]["median_ms"] / res[n + "_scan"]["median_ms"], 4)
        if masked_ref:
            res["ivf"]["restricted_ms"] = {n: round(t, 3) for n, t in mask_prep_ms.items()}
            res["ivf"]["eligible"] = {n: int(v.eligible) for n, v in views.items()}
    if not a.no_baseline:
        res["speedup_median"] = round(res["torch"]["median_ms"] / res["fused"]["median_ms"], 2)
        # slowest fused run against the fastest torch run: > 1 means faster by more than the spread
        res["speedup_worst_case"] = round(res["torch"]["min_ms"] / res["fused"]["max_ms"], 2)
        # agreement of the two arms' id sets (the torch arm ranks bf16-rounded scores: not exact)
        fi, ti = outs["fused"][0], outs["torch"][0]
        nrows = min(a.M, 256)
        step = max(1, min(nrows, (1 << 28) // (a.k * a.k)))  # rows per comparison: k * k booleans each
        hit = sum(float((fi[lo:min(lo + step, nrows)].unsqueeze(2) == ti[lo:min(lo + step, nrows)].unsqueeze(1))
                        .any(2).float().sum()) for lo in range(0, nrows, step)) / (nrows * a.k)
        res["id_overlap_first_rows"] = round(hit, 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
