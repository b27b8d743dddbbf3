"""The fused tower kernels swept over their declared shape limits (``-m gpu``).

tests/tower_shapes.py holds the cases: each is the smallest shape at which one run-time branch of
csrc/tower*.hip exists (L = 1 and L = 4, the 16-tile boundary of the staged T2, wave predication at
widths 32 / 96 and rising widths, a partial 128-column input chunk, a 32-wide tower on the register
T2, ragged T2 slices, the run-time two-layer kernel away from [96, 32], B = 8, and the indexed
multi-feature T1 at D = 16 / 32 / 128). Every case runs T1 -> wgrad(loss) -> update(do_adam = False,
grads_out = ...) and is checked for

  parity      check_towers against the fp64 emulation of the kernels' rounding points (defaults of
              tests/tower_emul.py), loss at rtol 1e-4, and each dX / gradient tensor's relative
              Frobenius error below 2e-3 (which covers the ambiguous rows in aggregate);
  placement   nothing outside the tower-input columns (or the gradient rows pos_out names) written,
              everything inside written;
  workspace   a second run on the same FusedTowers object reproduces every output bit for bit, the
              X^T operand strip holds exactly the bf16 tower inputs and rows [B, Bp) of every strip
              are still zero;
  Adam        (l1-min, l3-wide, l4-full) one Adam step over the full parameter vector from the
              reduced gradient (tower_emul.check_adam).

tests/test_cpu_tower_shapes.py shows, without a GPU, that a correct fp32 implementation in another
summation order passes these very checks at these very shapes."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_cases as ec
import tower_shapes as ts
from tower_emul import check_adam, split_params

pytestmark = pytest.mark.gpu

SENT = ts.SENT
TT_EINVAL = 1001


@pytest.fixture(scope="module")
def ops():
    from two_tower_recommender_model_amd import ops as _ops

    return _ops


class Runner:
    """One case on the GPU with fixed inputs; ``run`` gives everything a step leaves (CPU tensors)."""

    def __init__(self, ops, device, cid):
        from two_tower_recommender_model_amd import _lib

        self.lib, self._lib = _lib.load(), _lib
        self.c, self.inp = ts.BY_ID[cid], ts.inputs(cid)
        self.ops, self.device = ops, device
        c, inp = self.c, self.inp
        assert ops.FusedTowers.supported(c.in_dims, c.widths, c.cols, c.B)
        self.P = inp.flat.to(device)
        self.tw = ops.FusedTowers(list(c.in_dims), list(c.widths), c.cols, c.B, device, flags=c.flags)
        assert self.tw.num_params == inp.flat.numel()
        self.tw.update(self.P, do_adam=False)  # the bf16 weight copies
        self.labels = inp.labels.to(device)
        if c.D:
            self.rows_d, self.pin_d, self.pout_d = inp.rows_in.to(device), inp.pos_in.to(device), inp.pos_out.to(device)
        else:
            self.pooled_d = inp.pooled.to(device)

    def t1_multi(self, tw, D, gro, logits):
        """tt_tower_fwd_bwd_indexed_multi_bf16 as sharded.py's _t1 calls it; returns the status."""
        from two_tower_recommender_model_amd._lib import TT_I32, ptr, stream_handle

        return self.lib.tt_tower_fwd_bwd_indexed_multi_bf16(
            C.byref(tw.shape), self.c.B, D, ptr(self.pin_d), ptr(self.pout_d), ptr(self.rows_d), ptr(gro),
            ptr(self.P), ptr(self.labels), TT_I32, 1.0, ptr(logits), ptr(tw.ws), tw.nbytes,
            stream_handle(self.device))

    def run(self):
        c, inp, dev, tw = self.c, self.inp, self.device, self.tw
        B = c.B
        logits = torch.full((B,), SENT, device=dev)
        loss = torch.full((), SENT, device=dev)
        grads = torch.full_like(self.P, SENT)
        out = {}
        if c.D:
            gro = torch.full((inp.NR, c.D), SENT, device=dev)
            self._lib.check(self.t1_multi(tw, c.D, gro, logits), "tower_fwd_bwd_indexed_multi")
        else:
            gp = torch.full((B, inp.ldp), SENT, device=dev)
            tw.fwd_bwd(self.pooled_d, gp, self.P, self.labels, logits)
        tw.wgrad(loss)
        tw.update(self.P, do_adam=False, grads_out=grads)
        torch.cuda.synchronize()
        if c.D:
            out["grad_rows"] = gro.cpu()
        else:
            out["gpooled"] = gp.cpu()
            out["dx"] = [out["gpooled"][:, col:col + d].clone() for col, d in zip(c.cols, c.in_dims)]
        lay = c.layout
        strips = tw.ws[:lay.o_dzt + 2 * ts.MAXL * ts.MAXW * lay.Bp * 2].cpu().view(torch.bfloat16)
        nt = lay.Bp // 32  # tile-major strips (strip_at): [block][row tile][feature][row in tile]
        out["xt"] = strips[:2 * lay.in_max * lay.Bp].view(2, nt, lay.in_max, 32)
        out["act"] = strips[lay.o_act // 2:lay.o_act // 2 + 2 * ts.MAXL * ts.MAXW * lay.Bp].view(2, ts.MAXL, nt, ts.MAXW, 32)
        out["dzt"] = strips[lay.o_dzt // 2:].view(2, ts.MAXL, nt, ts.MAXW, 32)
        out.update(logits=logits.cpu(), loss=loss.cpu(), grads=grads.cpu())
        return out

    def base(self):
        if not hasattr(self, "_base"):
            self._base = self.run()
        return self._base

    def dx(self, out, emu):
        if not self.c.D:
            return out["dx"]
        return self.inp.dx_from_rows(out["grad_rows"], [d[0].float() for d in emu[2]])


_RUNNERS = {}


@pytest.fixture(params=[c.id for c in ts.CASES])
def rn(request, ops, device):
    if request.param not in _RUNNERS:
        _RUNNERS[request.param] = Runner(ops, device, request.param)
    return _RUNNERS[request.param]


def test_matches_the_emulation(rn):
    c, emu = rn.c, ts.emulation(rn.c.id)
    cond = ts.check_conditions(c, emu)
    out = rn.base()
    glist = split_params(out["grads"], c.in_dims, c.widths)
    print(c.id, f"loss {float(out['loss']):.9g} want {float(emu[1]):.9g}", cond)
    stats = ts.check_case(c, emu, out["logits"], rn.dx(out, emu), glist)
    print(c.id, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in stats.items()})
    np.testing.assert_allclose(float(out["loss"]), float(emu[1]), rtol=1e-4)


def test_outputs_land_only_where_they_belong(rn):
    c, inp, out = rn.c, rn.inp, rn.base()
    assert float(out["loss"]) != SENT and not bool((out["logits"] == SENT).any())
    assert not bool((out["grads"] == SENT).any())
    if c.D:
        # row pos_out[f * B + m] holds columns [(f - f0) * D, + D) of dX: checked against the emulation
        # by test_matches_the_emulation through dx_from_rows; here: who was written at all
        used = torch.zeros(inp.NR, dtype=torch.bool)
        used[inp.pos_out[inp.pos_out >= 0].long()] = True
        assert int((~used).sum()) >= 24
        assert bool((out["grad_rows"][~used] == SENT).all()), "a gradient row no pos_out names was written"
        assert not bool((out["grad_rows"][used] == SENT).any()), "a named gradient row was not written whole"
        return
    inside = torch.zeros(inp.ldp, dtype=torch.bool)
    for col, d in zip(c.cols, c.in_dims):
        inside[col:col + d] = True
    assert bool((out["gpooled"][:, ~inside] == SENT).all()), "gpooled: a column outside the tower inputs was written"
    assert not bool((out["gpooled"][:, inside] == SENT).any()), "gpooled: a tower-input cell was not written"


def test_second_run_is_bitwise_and_the_workspace_stays_clean(rn):
    c, inp, a = rn.c, rn.inp, rn.base()
    b = rn.run()
    for k in ("logits", "loss", "grads", "grad_rows" if c.D else "gpooled", "xt", "act", "dzt"):
        ec.assert_bitwise(b[k], a[k], f"{c.id} second run: {k}")
    lay, B = c.layout, c.B
    # X^T strips: exactly the bf16 tower inputs in rows [0, B), zero in the padded rows [B, Bp) and in
    # the feature rows past a narrower tower's input
    want = torch.zeros(2, lay.Bp, lay.in_max, dtype=torch.bfloat16)
    for t in range(2):
        want[t, :B, :c.in_dims[t]] = inp.x[t].to(torch.bfloat16)
    got = b["xt"].permute(0, 1, 3, 2).reshape(2, lay.Bp, lay.in_max)  # [block][row][feature]
    ec.assert_bitwise(got, want, f"{c.id}: X^T strips")
    for k in ("act", "dzt"):
        rows = b[k].permute(0, 1, 2, 4, 3).reshape(2, ts.MAXL, lay.Bp, ts.MAXW).float()  # [t][layer][row][feature]
        assert not bool(rows[:, :, B:].any()), f"{c.id}: {k} strips written in the padded rows [B, Bp)"
        assert not bool(rows[:, c.L:].any()), f"{c.id}: {k} strips written past layer L - 1"
        for l in range(c.L):
            assert not bool(rows[:, l, :, c.widths[l]:].any()), f"{c.id}: {k} strip of layer {l} written past its width"
    assert bool(b["dzt"].float().any()) and (c.L == 1 or bool(b["act"].float().any()))


@pytest.mark.parametrize("cid", [c.id for c in ts.CASES if c.adam])
def test_adam_over_the_full_parameter_vector(cid, ops, device):
    """T3's fixed-order reduction over the S slabs + Adam at this case's parameter count: step 4
    from non-zero moments, against the EMULATED gradient and its bound."""
    if cid not in _RUNNERS:
        _RUNNERS[cid] = Runner(ops, device, cid)
    rn = _RUNNERS[cid]
    c, emu = rn.c, ts.emulation(cid)
    rn.base()  # the slabs of this case's T2 are in the workspace
    n, lr = rn.inp.flat.numel(), 0.01
    g = torch.Generator().manual_seed(c.seed + 1)
    m0, v0 = torch.randn(n, generator=g) * 1e-3, torch.rand(n, generator=g) * 1e-6
    P, m, v = rn.inp.flat.to(device), m0.to(device), v0.to(device)
    state = torch.tensor([3, 0], dtype=torch.int64, device=device)
    try:
        rn.tw.update(P, m, v, state, lr=lr, do_adam=True)
        torch.cuda.synchronize()
        assert state.cpu().tolist() == [4, 0]
        want = torch.cat([w.reshape(-1) for w, _ in emu[3]])
        bound = torch.cat([e.reshape(-1) for _, e in emu[3]])
        # the ABI takes the betas as fp32: Adam runs with beta = fl32(0.9), fl32(0.999) throughout (1 - beta2
        # is then 1.3e-5 away from 0.001, which the moment-sized v0 here would show in the step)
        betas = (float(np.float32(0.9)), float(np.float32(0.999)))
        check_adam(rn.inp.flat, m0, v0, 4, want, bound, P.cpu(), m.cpu(), v.cpu(), lr, betas=betas, what=cid)
        assert not torch.equal(P.cpu(), rn.inp.flat)
    finally:
        rn.tw.update(rn.P, do_adam=False)  # back to the case's bf16 weight copies
        torch.cuda.synchronize()


def test_indexed_multi_refusals(ops, device):
    """D = 48 (does not divide the 128-column chunk) and a two-layer shape of at most 128 columns
    without TT_TOWER_GENERAL_T1 are TT_EINVAL before any launch: no output is touched."""
    cid = "idx-d16"
    if cid not in _RUNNERS:
        _RUNNERS[cid] = Runner(ops, device, cid)
    rn = _RUNNERS[cid]
    c, inp = rn.c, rn.inp
    logits = torch.full((c.B,), SENT, device=device)
    gro = torch.full((inp.NR, c.D), SENT, device=device)
    # [96, 96] inputs are whole multiples of 48, so only the chunk rule refuses D = 48
    tw48 = ops.FusedTowers([96, 96], list(c.widths), [0, 96], c.B, device, flags=ts.GENERAL_T1)
    assert rn.t1_multi(tw48, 48, gro, logits) == TT_EINVAL
    plain = ops.FusedTowers(list(c.in_dims), list(c.widths), c.cols, c.B, device, flags=0)
    assert rn.t1_multi(plain, c.D, gro, logits) == TT_EINVAL
    torch.cuda.synchronize()
    assert bool((logits == SENT).all()) and bool((gro == SENT).all())
