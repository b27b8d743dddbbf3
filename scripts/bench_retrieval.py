"""Exact top-k retrieval (ops.topk_mips: tt_topk_mips, the fused score + select kernel) against the
torch composition on the same GPU: bf16 torch.matmul over item chunks, torch.topk of each score
chunk and a running merge of the best k. Interleaved runs of the two arms after a warm-up, timed with
HIP events; prints one JSON line (medians, the runs, the spread). Inputs are seeded, generated on the
device; nothing is read from outside the tree.

    python scripts/bench_retrieval.py                       # M 4096, N 4,194,304, E 64, k 100
    python scripts/bench_retrieval.py --M 10000 --N 100000000 --items bf16 --no-baseline --runs 1
    python scripts/bench_retrieval.py --no-baseline --filter    # + the filtered arms, --seen 256

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
    ap.add_argument("--seen", type=int, default=256, help="excluded ids per query of the filtered arm")
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

    def fused():
        return ops.topk_mips(q, c, a.k, splits=a.splits)

    def composed():
        return torch_arm(q16, c16, a.k, a.chunk)

    arms = {"fused": fused} if a.no_baseline else {"fused": fused, "torch": composed}
    if a.filter:
        ones = ops.pack_allow_mask(torch.ones(a.N, dtype=torch.bool, device=dev))
        empty = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(a.M + 1, dtype=torch.int64, device=dev))
        mask = ops.pack_allow_mask(torch.rand(a.N, device=dev, generator=g) < 0.9)
        offs = torch.arange(a.M + 1, dtype=torch.int64, device=dev) * a.seen
        seen = (ops.sort_exclusions(torch.randint(0, a.N, (a.M * a.seen,), device=dev, generator=g), offs, a.N), offs)
        arms["filtered_noop"] = lambda: ops.topk_mips(q, c, a.k, splits=a.splits, allow=ones, exclude=empty)
        arms["filtered"] = lambda: ops.topk_mips(q, c, a.k, splits=a.splits, allow=mask, exclude=seen)
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
            hit = 0
            for lo in range(0, a.M, 1024):  # recall@k against the exact ids (which are all >= 0)
                hit += int((got[lo:lo + 1024].unsqueeze(2) == exact[lo:lo + 1024].unsqueeze(1)).any(2).sum())
            res[n]["recall_at_k"] = round(hit / exact.numel(), 5)
            for m in (n, n + "_coarse", n + "_scan"):
                res[m]["ratio_to_fused"] = round(res[m]["median_ms"] / res["fused"]["median_ms"], 4)
            res[n]["scan_equals_search"] = bool(torch.equal(outs[n + "_scan"][0], got))
    if not a.no_baseline:
        res["speedup_median"] = round(res["torch"]["median_ms"] / res["fused"]["median_ms"], 2)
        # slowest fused run against the fastest torch run: > 1 means faster by more than the spread
        res["speedup_worst_case"] = round(res["torch"]["min_ms"] / res["fused"]["max_ms"], 2)
        # agreement of the two arms' id sets (the torch arm ranks bf16-rounded scores: not exact)
        fi, ti = outs["fused"][0], outs["torch"][0]
        rows = slice(0, min(a.M, 256))
        hit = (fi[rows].unsqueeze(2) == ti[rows].unsqueeze(1)).any(2).float().mean()
        res["id_overlap_first_rows"] = round(float(hit), 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
