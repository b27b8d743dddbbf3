"""T3's segment select and slab reduction against torch in the kernel's own order (``-m gpu``).

update_block (csrc/tower_tail.hip) finds a parameter's segment (W or b of tower t, layer l) by compares
and selects over a table of records held in SGPRs, and issues its slab loads before it knows the
segment: a W element sums the S slabs in the order s = 0, 1, ..., a bias element keeps slab 0's
value. Here the slabs in the workspace are overwritten with random numbers (so a wrong segment, a
wrong slab or a wrong order shows in every element), then one T3 runs and

  the reduced gradient (``grads_out``) is compared bit for bit with the sequential fp32 sum,
  both moments bit for bit with fp32 Adam in t3_apply's operation order (adds and multiplies only),
  the parameters with the same Adam within the rounding of the device's sqrt and two divisions,

over the whole vector, and the bitwise ones once more, named, at the first and last element of every
W and b. The parameter bound: p' = p + u with u = -step m' / (sqrt(v') / c + eps). The device's fp32
division is good to 2.5 ulp and its sqrt to 1 ulp, against torch's correctly rounded ones, so the
denominator differs by at most 1 + 2.5 + 0.5 ulp and u by 2.5 more: 8 ulp of u (2^-23 each) covers
it, and 1 ulp of p' the final add's rounding on either side of a tie.

Cases: S = 1 (B = 8), S = 32 (B = 8192: one full round of slab loads) and S = 33 (B = 8200: a
second round with one live load) at the production shape, and a four-layer shape whose sixteen
segments fill the table (its second half is fetched only above eight segments). Each runs through
``update`` (T3 computes Adam's scalars itself) and through ``wgrad_pre`` + ``update_pre`` (T2 leaves
them in the workspace: the fused step's form), with and without ``grads_out``."""
import numpy as np
import pytest
import torch

import tower_shapes as ts

pytestmark = pytest.mark.gpu

LR, EPS = 0.01, 1e-8
B1, B2 = np.float32(0.9), np.float32(0.999)  # the ABI takes the betas as fp32

# (id, B, in_dims, widths)
SHAPES = [
    ("prod-s1", 8, (128, 128), (128, 64)),
    ("prod-s32", 8192, (128, 128), (128, 64)),
    ("prod-s33", 8200, (128, 128), (128, 64)),
    ("l4-s1", 8, (64, 96), (128, 96, 64, 32)),
    ("l4-s2", 264, (64, 96), (128, 96, 64, 32)),
]
WANT_S = {"prod-s1": 1, "prod-s32": 32, "prod-s33": 33, "l4-s1": 1, "l4-s2": 2}


def segments(in_dims, widths):
    """[(name, first, last, is_w)] of the flat parameter vector: per tower, per layer W [n][k] then b."""
    out, o = [], 0
    for t, k in enumerate(in_dims):
        for l, n in enumerate(widths):
            out.append((f"W[{t}][{l}]", o, o + n * k - 1, True))
            o += n * k
            out.append((f"b[{t}][{l}]", o, o + n - 1, False))
            o += n
            k = n
    return out, o


def slab_offset(B, in_dims, widths):
    """Byte offset of the gradient slabs in the tower workspace (tower_ws_layout's order)."""
    lay = ts.host_layout(B, in_dims, widths)
    strip = ts._align(2 * ts.MAXL * ts.MAXW * lay.Bp * 2)
    nwg = ts._cdiv(B, ts.TR)
    return lay.o_dzt + strip + ts._align(2 * ts.MAXL * nwg * ts.MAXW * 4), lay.S


class Case:
    """One shape: the towers, random slabs in the workspace and the torch reference, made once."""

    def __init__(self, ops, device, cid, B, in_dims, widths):
        self.cid, self.device = cid, device
        self.segs, self.P = segments(in_dims, widths)
        self.tw = ops.FusedTowers(list(in_dims), list(widths), [0, in_dims[0]], B, device)
        assert self.tw.num_params == self.P
        self.o_slab, self.S = slab_offset(B, in_dims, widths)
        assert self.S == WANT_S[cid]
        g = torch.Generator().manual_seed(1000 + B + len(widths))
        self.slab = torch.randn(self.S, self.P, generator=g) * 1e-2
        self.p0 = torch.randn(self.P, generator=g) * 0.1
        self.m0 = torch.randn(self.P, generator=g) * 1e-3
        self.v0 = torch.rand(self.P, generator=g) * 1e-6
        is_w = torch.zeros(self.P, dtype=torch.bool)
        for _, a, b, w in self.segs:
            is_w[a:b + 1] = w
        gsum = torch.zeros(self.P)
        for s in range(self.S):  # the kernel's order: s = 0, 1, ...
            gsum = gsum + self.slab[s]
        self.grad = torch.where(is_w, gsum, self.slab[0])
        self.edges = sorted({i for _, a, b, _ in self.segs for i in (a, b)})

    def put_slabs(self):
        n = self.S * self.P * 4
        self.tw.ws[self.o_slab:self.o_slab + n] = self.slab.reshape(-1).view(torch.uint8).to(self.device)

    def adam(self, step):
        """t3_apply in fp32, operation by operation (no contraction), at Adam step `step`."""
        f32 = np.float32
        bc1 = 1.0 - float(B1) ** step
        bc2 = 1.0 - float(B2) ** step
        step_size, bc2_sqrt = f32(float(f32(LR)) / bc1), f32(np.sqrt(bc2))
        g, one = self.grad, f32(1)
        m = self.m0 + float(one - B1) * (g - self.m0)
        v = self.v0 * float(B2) + float(one - B2) * g * g
        denom = v.sqrt() / float(bc2_sqrt) + float(f32(EPS))
        u = float(-step_size) * m / denom
        return self.p0 + u, m, v, u

    def name(self, i):
        for n, a, b, _ in self.segs:
            if a <= i <= b:
                return f"{n}[{i - a}]"
        return str(i)

    def check(self, what, got, want):
        got = got.cpu()
        gi, wi = got.view(torch.int32), want.view(torch.int32)
        for i in self.edges:  # the segment edges by name, then everything
            assert int(gi[i]) == int(wi[i]), \
                f"{self.cid} {what} at {self.name(i)} (index {i}): got {float(got[i]):.9g} want {float(want[i]):.9g}"
        bad = torch.nonzero(gi != wi).flatten()
        assert bad.numel() == 0, f"{self.cid} {what}: {bad.numel()} of {self.P} differ, first at {self.name(int(bad[0]))}"


    def check_close(self, what, got, want, lim):
        err = (got.cpu().double() - want.double()).abs()
        bad = torch.nonzero(~(err <= lim.double())).flatten()
        assert bad.numel() == 0, (f"{self.cid} {what}: {bad.numel()} of {self.P} outside the bound, first at "
                                  f"{self.name(int(bad[0]))}: err {float(err[bad[0]]):.3g} lim {float(lim[bad[0]]):.3g}")


_CASES = {}


@pytest.fixture(params=[s[0] for s in SHAPES])
def case(request, device):
    from two_tower_recommender_model_amd import ops

    if request.param not in _CASES:
        _CASES[request.param] = Case(ops, device, *next(s for s in SHAPES if s[0] == request.param))
    return _CASES[request.param]


@pytest.mark.parametrize("with_grads_out", [True, False], ids=["grads_out", "no_grads_out"])
@pytest.mark.parametrize("form", ["update", "update_pre"])
def test_t3_matches_torch_in_the_kernels_order(case, form, with_grads_out):
    c, dev = case, case.device
    P, m, v = c.p0.to(dev), c.m0.to(dev), c.v0.to(dev)
    gout = torch.full((c.P,), ts.SENT, device=dev) if with_grads_out else None
    state = torch.tensor([3, 0], dtype=torch.int64, device=dev)
    if form == "update":
        c.put_slabs()
        c.tw.update(P, m, v, state, lr=LR, do_adam=True, grads_out=gout)
    else:
        loss = torch.zeros((), device=dev)
        c.tw.wgrad_pre(loss, state, adam_lr=LR)  # advances the step, leaves Adam's scalars (and zero slabs)
        c.put_slabs()
        c.tw.update_pre(P, m, v, grads_out=gout)
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [4, 0]
    if with_grads_out:
        c.check("gradient", gout, c.grad)
    wp, wm, wv, wu = c.adam(4)
    c.check("exp_avg", m, wm)
    c.check("exp_avg_sq", v, wv)
    c.check_close("param", P, wp, 2.0 ** -23 * wp.abs() + 8 * 2.0 ** -23 * wu.abs())


def test_t3_gradient_only(case):
    """do_adam = 0 (the form the shape sweep reads gradients with): no moments, nothing but
    ``grads_out`` and the bf16 weight copies written."""
    c, dev = case, case.device
    P = c.p0.to(dev)
    gout = torch.full((c.P,), ts.SENT, device=dev)
    c.put_slabs()
    c.tw.update(P, do_adam=False, grads_out=gout)
    torch.cuda.synchronize()
    c.check("gradient", gout, c.grad)
    c.check("param", P, c.p0)
