"""T1's label load, grad_scale and output placement in every T1 kernel family (``-m gpu``).

Every T1 kernel has its own label load and applies grad_scale in its own place; the kernel-level tests
elsewhere pass int32 0 / 1 labels and grad_scale = 1 only. The families, by entry point and shape
(csrc/tower.hip launch_t1):

  pooled-rows     fwd_bwd, [64, 64] -> [128, 64], B = 200        the row-owned kernel on pooled rows
  pooled-l2       fwd_bwd, [96, 32] -> [96, 32], B = 136         the two-layer kernel, run-time shape
  pooled-general  fwd_bwd, [64, 96] -> [128, 64, 32], B = 200    the general kernel
  gather          fwd_bwd_gather, D = 64, int32 ids, B = 200     the row-owned kernel, rows from ids
  kjt             fwd_bwd_kjt, D = 128, B = 200                  the two-layer kernel, sum pool inside
  indexed-f32     fwd_bwd_indexed, fp32 rows, D = 128, B = 136   the two-layer kernel, rows by position
  indexed-bf16    fwd_bwd_indexed, bf16 rows, D = 128, B = 136   the row-owned kernel, rows by position
  indexed-f32-64  fwd_bwd_indexed, fp32 rows, D = 64, B = 136    the two-layer kernel's D = 64 form
  indexed-bf16-l2 fwd_bwd_indexed, bf16 rows, [96, 32] -> [96, 32], B = 136   the two-layer kernel, bf16
                                                                 rows at a run-time shape

With these every tower_l2_kernel instantiation of the library is launched by the suite (the multi-hot
D = 64 one by tests/test_gpu_abi_edges.py). Each run is T1 -> wgrad(loss) -> update(do_adam = False, grads_out = ...). The int32 run of every
family is anchored to the fp64 emulation of the kernels' rounding points (tests/tower_emul.py
emulate_bounds / check_towers; loss rtol 1e-4 as tests/test_gpu_baseline_parity.py); label dtypes
and the power-of-two grad_scale are then compared with that run bit for bit."""
import numpy as np
import pytest
import torch

import edge_cases as ec
from oracle import ref
from tower_emul import check_towers, emulate_bounds, split_params

pytestmark = pytest.mark.gpu

SENT = -77.125  # finite sentinel of every output buffer

FAMILIES = {
    "pooled-rows": ("pooled", 200, [64, 64], [128, 64]),
    "pooled-l2": ("pooled", 136, [96, 32], [96, 32]),
    "pooled-general": ("pooled", 200, [64, 96], [128, 64, 32]),
    "gather": ("gather", 200, [64, 64], [128, 64]),
    "kjt": ("kjt", 200, [128, 128], [128, 64]),
    "indexed-f32": ("indexed", 136, [128, 128], [128, 64]),
    "indexed-bf16": ("indexed-bf16", 136, [128, 128], [128, 64]),
    "indexed-f32-64": ("indexed", 136, [64, 64], [128, 64]),
    "indexed-bf16-l2": ("indexed-bf16", 136, [96, 32], [96, 32]),
}


@pytest.fixture(scope="module")
def ops():
    from two_tower_recommender_model_amd import ops as _ops

    return _ops


class Family:
    """One T1 entry point at one shape with fixed inputs; ``run`` gives everything a step leaves."""

    def __init__(self, ops, device, name):
        self.kind, self.B, self.in_dims, self.widths = FAMILIES[name]
        self.name, self.ops, self.device = name, ops, device
        B, in_dims = self.B, self.in_dims
        g = torch.Generator().manual_seed(len(name) + B)
        self.cols = [16, 16 + in_dims[0]]
        self.ldp = sum(in_dims) + 32
        ps = []
        for t in range(2):
            k = in_dims[t]
            for w in self.widths:
                ps.append(torch.randn(w, k, generator=g) / k ** 0.5)
                ps.append(torch.randn(w, generator=g) * 0.1)
                k = w
        self.flat = torch.cat([p.reshape(-1) for p in ps])
        self.P = self.flat.to(device)
        self.tw = ops.FusedTowers(in_dims, self.widths, self.cols, B, device)
        assert self.tw.num_params == self.flat.numel()
        self.tw.update(self.P, do_adam=False)  # the bf16 weight copies
        self.labels = torch.randint(0, 2, (B,), generator=g).to(torch.int32)
        self.soft = torch.rand(B, generator=g)
        kind = self.kind
        if kind == "pooled":
            self.pooled = torch.full((B, self.ldp), SENT)
            for t in range(2):
                self.pooled[:, self.cols[t]:self.cols[t] + in_dims[t]] = torch.randn(B, in_dims[t], generator=g) * 0.5
            self.x = [self.pooled[:, self.cols[t]:self.cols[t] + in_dims[t]].clone() for t in range(2)]
            self.pooled_d = self.pooled.to(device)
        elif kind == "gather":
            self.N = [300, 500]
            self.tables = [torch.randn(n, d, generator=g) * 0.5 for n, d in zip(self.N, in_dims)]
            self.ids = [torch.randint(-n, 3 * n, (B,), generator=g).to(torch.int32) for n in self.N]
            for c in self.ids:
                c[::17] = 0  # dropped ids: zero rows
            self.x = []
            for c, n, tab in zip(self.ids, self.N, self.tables):
                rows = tab[torch.remainder(c.to(torch.int64), n)]
                self.x.append(torch.where((c != 0)[:, None], rows, torch.zeros(())))
            self.tables_d = [t.to(device) for t in self.tables]
            self.ids_d = [c.to(device) for c in self.ids]
        elif kind == "kjt":
            self.N = [300, 500]
            rng = np.random.default_rng(B)
            lengths = rng.integers(0, 6, 2 * B).astype(np.int32)
            self.offsets = ref.complete_cumsum(lengths)
            self.values = np.concatenate([rng.integers(0, self.N[i // B], lengths[i]) for i in range(2 * B)])
            self.maxlen = int(lengths.max())
            self.tables = [torch.randn(n, d, generator=g) * 0.3 for n, d in zip(self.N, in_dims)]
            self.tables_d = [t.to(device) for t in self.tables]
            self.V, self.O = torch.from_numpy(self.values).to(device), torch.from_numpy(self.offsets).to(device)
            self.x = None  # the pooled rows the kernel materialises (checked against the oracle's)
        else:
            NR = B + 24
            dt = torch.bfloat16 if kind == "indexed-bf16" else torch.float32
            self.rows_in = [(torch.randn(NR, d, generator=g) * 0.5).to(dt) for d in in_dims]
            self.pos = []
            for t in range(2):
                p = torch.randperm(NR, generator=g)[:B].to(torch.int32)  # distinct rows: one writer per row
                p[t::19] = -1                                            # dropped ids: zero rows, no gradient row
                self.pos.append(p)
            self.x = [torch.where((p >= 0)[:, None], r.float()[p.clamp(min=0).to(torch.int64)], torch.zeros(()))
                      for p, r in zip(self.pos, self.rows_in)]
            self.rows_d = [r.to(device) for r in self.rows_in]
            self.pos_d = [p.to(device) for p in self.pos]

    def run(self, labels, grad_scale=1.0):
        """-> dict(logits [B], loss, dx [2 x [B, in]], grads flat, + the raw output buffers), CPU."""
        dev, B, tw = self.device, self.B, self.tw
        logits = torch.full((B,), SENT, device=dev)
        loss = torch.full((), SENT, device=dev)
        grads = torch.full_like(self.P, SENT)
        out = {}
        lab = labels.to(dev) if labels.device.type == "cpu" else labels
        if self.kind in ("pooled", "gather", "kjt"):
            gp = torch.full((B, self.ldp), SENT, device=dev)
            po = torch.full((B, self.ldp), SENT, device=dev)
            if self.kind == "pooled":
                tw.fwd_bwd(self.pooled_d, gp, self.P, lab, logits, grad_scale=grad_scale)
                po = None
            elif self.kind == "gather":
                tw.fwd_bwd_gather(self.ids_d, self.N, self.tables_d, gp, self.P, lab, logits, pooled_out=po,
                                  grad_scale=grad_scale)
            else:
                tw.fwd_bwd_kjt(self.V, self.O, self.tables_d, gp, self.P, lab, logits, pooled_out=po,
                               grad_scale=grad_scale)
            tw.wgrad(loss)
            tw.update(self.P, do_adam=False, grads_out=grads)
            torch.cuda.synchronize()
            out["gpooled"] = gp.cpu()
            out["pooled_out"] = po.cpu() if po is not None else None
            out["dx"] = [out["gpooled"][:, c:c + d].clone() for c, d in zip(self.cols, self.in_dims)]
        else:
            gro = [torch.full((r.shape[0], r.shape[1]), SENT, device=dev) for r in self.rows_in]
            tw.fwd_bwd_indexed(self.pos_d, self.rows_d, gro, self.P, lab, logits, grad_scale=grad_scale)
            tw.wgrad(loss)
            tw.update(self.P, do_adam=False, grads_out=grads)
            torch.cuda.synchronize()
            out["grad_rows"] = [x.cpu() for x in gro]
            # a dropped id has no gradient row: zeros (row 0 may be a row no position names: the sentinel)
            out["dx"] = [torch.where((p >= 0)[:, None], x[p.clamp(min=0).to(torch.int64)], torch.zeros(()))
                         for x, p in zip(out["grad_rows"], self.pos)]
        out.update(logits=logits.cpu(), loss=loss.cpu(), grads=grads.cpu())
        return out

    def emu(self, labels, out):
        x = self.x
        if x is None:  # kjt: the kernel's own pooled rows, themselves within tt_pooled_fwd's tolerance
            x = [out["pooled_out"][:, c:c + d] for c, d in zip(self.cols, self.in_dims)]
            want = ref.pooled_fwd(self.tables, [0, 1], torch.from_numpy(self.values), torch.from_numpy(self.offsets),
                                  self.B)
            ec.assert_pooled_close(torch.cat(x, 1).numpy(), want.numpy(), self.maxlen)
        prm = split_params(self.flat, self.in_dims, self.widths)
        return emulate_bounds(x[0], x[1], prm, self.widths, labels), prm

    def check_emulation(self, labels, out, scale=1.0):
        """check_towers on the run's outputs divided by ``scale`` (a power of two: exact)."""
        emu, prm = self.emu(labels, out)
        dx = [d / scale for d in out["dx"]]
        if self.kind.startswith("indexed"):  # a dropped id has no gradient row: nothing to compare
            dx = [torch.where((p >= 0)[:, None], d, w[0].float()) for d, p, w in zip(dx, self.pos, emu[2])]
        glist = split_params(out["grads"] / scale, self.in_dims, self.widths)
        stats = check_towers(emu, out["logits"], dx, glist, self.name)
        np.testing.assert_allclose(float(out["loss"]), float(emu[1]), rtol=1e-4)
        return stats


_FAMS = {}


@pytest.fixture(params=list(FAMILIES))
def fam(request, ops, device):
    if request.param not in _FAMS:
        _FAMS[request.param] = Family(ops, device, request.param)
    return _FAMS[request.param]


def _baseline(fam):
    if not hasattr(fam, "_base"):
        fam._base = fam.run(fam.labels)
    return fam._base


def _same(a, b, what, keys=("logits", "loss", "grads")):
    for k in keys:
        ec.assert_bitwise(a[k], b[k], f"{what}: {k}")
    for t in range(2):
        ec.assert_bitwise(a["dx"][t], b["dx"][t], f"{what}: dX[{t}]")


def test_int32_labels_match_the_emulation(fam):
    print(fam.name, fam.check_emulation(fam.labels, _baseline(fam)))


def test_label_dtypes_bitwise(fam, device):
    """The same 0 / 1 labels as int32, int64 and float32: every output bitwise identical. The int64
    labels are also given as the first half of a buffer whose second half is all -1 (a kernel that
    read 4-byte elements, or past label B - 1, would see other values)."""
    base = _baseline(fam)
    _same(fam.run(fam.labels.to(torch.int64)), base, "int64 labels")
    _same(fam.run(fam.labels.to(torch.float32)), base, "float32 labels")
    buf = torch.cat([fam.labels.to(torch.int64), torch.full((fam.B,), -1, dtype=torch.int64)]).to(device)
    _same(fam.run(buf[:fam.B]), base, "int64 labels beside -1s")
    # the labels do matter: flipped labels change the gradient (the comparison is not vacuous)
    flipped = fam.run(1 - fam.labels)
    ec.assert_bitwise(flipped["logits"], base["logits"], "flipped labels: logits")
    assert not torch.equal(flipped["grads"], base["grads"]) and float(flipped["loss"]) != float(base["loss"])


def test_soft_labels_match_the_emulation(fam):
    out = fam.run(fam.soft)
    print(fam.name, fam.check_emulation(fam.soft, out))


def test_grad_scale_quarter_is_exact(fam):
    """grad_scale = 0.25: logits and loss as with 1.0, dX and every gradient exactly 0.25 x. Each
    kernel multiplies dlogit by grad_scale (or grad_scale / B) before any rounding, and a power of
    two commutes with the bf16 and fp32 roundings that follow (no value here is near the subnormal
    range: the smallest |dX| is far above 2^-126 x 4)."""
    base = _baseline(fam)
    out = fam.run(fam.labels, grad_scale=0.25)
    ec.assert_bitwise(out["logits"], base["logits"], "logits")
    ec.assert_bitwise(out["loss"], base["loss"], "loss")
    ec.assert_bitwise(out["grads"], base["grads"] * 0.25, "gradients")
    for t in range(2):
        ec.assert_bitwise(out["dx"][t], base["dx"][t] * 0.25, f"dX[{t}]")


def test_outputs_land_only_in_their_columns(fam):
    """gpooled (and pooled_out) hold the sentinel in every column outside the two tower inputs
    (ldp = sum(in_dims) + 32, in_col = [16, 16 + in_dim0]); the indexed form leaves the gradient rows
    no position names untouched."""
    out = _baseline(fam)
    assert SENT not in (float(out["loss"]),) and not bool((out["logits"] == SENT).any())
    assert not bool((out["grads"] == SENT).any())
    if fam.kind.startswith("indexed"):
        for t in range(2):
            used = torch.zeros(out["grad_rows"][t].shape[0], dtype=torch.bool)
            used[fam.pos[t][fam.pos[t] >= 0].to(torch.int64)] = True
            assert bool((out["grad_rows"][t][~used] == SENT).all()), f"tower {t}: an unused gradient row was written"
            assert not bool((out["grad_rows"][t][used] == SENT).any())
        return
    inside = torch.zeros(fam.ldp, dtype=torch.bool)
    for c, d in zip(fam.cols, fam.in_dims):
        inside[c:c + d] = True
    for key in ("gpooled", "pooled_out"):
        buf = out[key]
        if buf is None:
            continue
        assert bool((buf[:, ~inside] == SENT).all()), f"{key}: a column outside the tower inputs was written"
        assert not bool((buf[:, inside] == SENT).any()), f"{key}: a tower-input cell was not written"
    if fam.kind == "gather":  # pooled_out is the gather itself: exact
        for t, (c, d) in enumerate(zip(fam.cols, fam.in_dims)):
            ec.assert_bitwise(out["pooled_out"][:, c:c + d], fam.x[t], f"pooled_out tower {t}")
