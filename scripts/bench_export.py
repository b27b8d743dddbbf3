"""Tower inference over a table (lifecycle.export_embeddings) and over a row list (the query path of
lifecycle.retrieve_fused): the per-layer tt_linear_fwd launches against the fused tt_tower_embed launch
on the same GPU. The arms alternate inside one process after a warm-up of every shape, each run timed
with HIP events around work that ends in a device synchronise; before any timing the fused results are
compared with the per-layer ones at the timed size (torch.equal). Prints one JSON line. Inputs are
seeded, generated on the device; nothing is read from outside the tree. Needs a GPU: no fallback.

    python scripts/bench_export.py                   # N 4,194,304: D 128 -> [128, 64] and D 64 -> [128, 64]
    python scripts/bench_export.py --N 1000000 --runs 3

Arms, per shape:
  layers         export_embeddings as it stands: one tt_linear_fwd per layer per chunk, fp32 out
  fused_f32      export_embeddings(fused=True): one tt_tower_embed per chunk, fp32 out
  fused_bf16     the same with out_dtype=torch.bfloat16
  gather_layers  --gather random rows: torch advanced-index gather + one tt_linear_fwd per layer
  gather_fused   the same rows as one tt_tower_embed launch over the row list
Per arm: median / min / max ms, rows per second, and the algorithmic bytes per row (in_dim * 4 +
out * element size: the rows in and the result out, nothing else) over the median time as a share of
the HBM peak of 8 TB/s. The share is of the whole call's time, not a kernel's.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from two_tower_recommender_model_amd import lifecycle as lc  # noqa: E402
from two_tower_recommender_model_amd import ops  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, specification


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def make_shape(dev, N, D, widths, gather, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    table = torch.empty(N, D, device=dev)
    for lo in range(0, N, 1 << 22):
        n = min(1 << 22, N - lo)
        table[lo:lo + n] = torch.randn(n, D, device=dev, generator=g)
    layers, k = [], D
    for n in widths:
        layers.append((torch.randn(n, k, device=dev, generator=g) / k ** 0.5, 0.5 * torch.randn(n, device=dev, generator=g)))
        k = n
    rows = torch.randint(0, N, (gather,), device=dev, generator=g)
    return table, layers, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4194304)
    ap.add_argument("--gather", type=int, default=65536, help="rows of the gather arms")
    ap.add_argument("--chunk", type=int, default=1 << 20, help="rows per launch of the export arms")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_export.py needs a GPU (there is no fallback)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)

    shapes = [(128, [128, 64]), (64, [128, 64])]
    res = {"bench": "export", "N": a.N, "gather": a.gather, "chunk": a.chunk, "runs": a.runs,
           "device": torch.cuda.get_device_name(dev), "hbm_peak_tb_s": HBM_PEAK_BYTES_PER_S / 1e12, "shapes": []}
    cases = []
    for s, (D, widths) in enumerate(shapes):
        table, layers, rows = make_shape(dev, a.N, D, widths, a.gather, s)
        out32 = torch.empty(a.N, widths[-1], device=dev)
        out16 = torch.empty(a.N, widths[-1], dtype=torch.bfloat16, device=dev)

        def gather_layers(table=table, layers=layers, rows=rows):
            x = table[rows]
            for w, b in layers:
                x = ops.linear_fwd([x], [w], [b], relu=True)[0]
            return x

        arms = {
            "layers": lambda t=table, l=layers, o=out32: lc.export_embeddings(t, l, chunk=a.chunk, out=o)[1],
            "fused_f32": lambda t=table, l=layers, o=out32: lc.export_embeddings(t, l, chunk=a.chunk, out=o, fused=True)[1],
            "fused_bf16": lambda t=table, l=layers, o=out16: lc.export_embeddings(
                t, l, chunk=a.chunk, out=o, fused=True, out_dtype=torch.bfloat16)[1],
            "gather_layers": gather_layers,
            "gather_fused": lambda t=table, l=layers, r=rows: ops.tower_embed(t, l, rows=r),
        }
        # the results at the timed size, before any timing
        want = arms["layers"]().clone()
        equal = {"fused_f32": bool(torch.equal(arms["fused_f32"](), want))}
        equal["fused_bf16"] = bool(torch.equal(arms["fused_bf16"]().view(torch.int16), want.to(torch.bfloat16).view(torch.int16)))
        equal["gather_fused"] = bool(torch.equal(arms["gather_fused"](), arms["gather_layers"]()))
        del want
        if not all(equal.values()):
            raise SystemExit(f"results differ at D = {D}, widths = {widths}: {equal}")
        cases.append((D, widths, arms, equal))

    for _ in range(a.warmup):  # every shape, every arm
        for _, _, arms, _ in cases:
            for fn in arms.values():
                fn()
    torch.cuda.synchronize()
    ms = [{n: [] for n in arms} for _, _, arms, _ in cases]
    for _ in range(a.runs):  # the arms alternate: a drift of the machine lands on all of them
        for c, (_, _, arms, _) in enumerate(cases):
            for n, fn in arms.items():
                ms[c][n].append(round(timed(fn)[0], 4))
    for c, (D, widths, arms, equal) in enumerate(cases):
        out = {"in_dim": D, "widths": widths, "equal": equal}
        for n in arms:
            med = statistics.median(ms[c][n])
            nrows = a.gather if n.startswith("gather") else a.N
            byts = D * 4 + widths[-1] * (2 if n == "fused_bf16" else 4)
            out[n] = {"median_ms": round(med, 4), "min_ms": min(ms[c][n]), "max_ms": max(ms[c][n]), "runs_ms": ms[c][n],
                      "rows_per_s": round(nrows / med * 1e3), "algorithmic_bytes_per_row": byts,
                      "share_of_hbm_peak": round(nrows * byts / (med * 1e-3) / HBM_PEAK_BYTES_PER_S, 4)}
        for n, base in (("fused_f32", "layers"), ("fused_bf16", "layers"), ("gather_fused", "gather_layers")):
            out[n]["speedup_median"] = round(out[base]["median_ms"] / out[n]["median_ms"], 3)
        res["shapes"].append(out)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
