"""The fused tower kernels' shape sweep: the case table and its oracle (test infrastructure).

tt_tower_shape_t admits 1..4 layers, widths that are multiples of 32 in [32, 128], tower inputs that
are multiples of 32 in [32, 1024] and any B % 8 == 0. Each case below is the smallest shape at which
one run-time branch of csrc/tower*.hip exists (the `branch` column). The table is shared by
tests/test_gpu_tower_shapes.py (the kernels against the fp64 emulation of tests/tower_emul.py) and
tests/test_cpu_tower_shapes.py (the emulation and its thresholds checked without a GPU).

`host_layout` recomputes, from the shape alone, what tower_layout / launch_t1 decide on the host:
the T1 kernel, the T2 path (staged through LDS when every K <= 128, else the register path), the
slice count S and the rows per slice. Every case states what it expects of them and the module
asserts it on import, so a later change to the slicing cannot quietly make a case stop covering the
branch it is here for (update the formulas here with tower_layout, then re-pick the shapes).

Measured on the CPU (tests/test_cpu_tower_shapes.py prints them): `amb` is the share of rows with a
ReLU unit within its error bound of 0 (check_towers leaves those out of its tight row statistics;
deep towers have many), and the floors are the fp32 replay's worst statistics against the
thresholds of check_towers. Every case runs with check_towers' default thresholds: none needed
the 4 x noise-floor rule.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from tower_emul import GRAD_RTOL, LOGIT_RTOL, ROW_RTOL, check_towers, emulate_bounds, rel_err, split_params

SENT = -77.125     # finite sentinel of every output buffer
FROB_RTOL = 2e-3   # relative Frobenius error of a whole dX / gradient tensor (test_gpu_ops' number)
GENERAL_T1 = 1     # TT_TOWER_GENERAL_T1

# csrc/tower_common.h constants the layout depends on
TR, MAXW, MAXL, XCH = 32, 128, 4, 128
T2_NT, T2_PASS = 64, 256


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _align(n: int, a: int = 256) -> int:
    return _cdiv(n, a) * a


@dataclass(frozen=True)
class Layout:
    t1: str          # "rows" | "l2-runtime" | "general"
    t2: str          # "staged" | "register"
    S: int           # T2 slices = slab depth T3 reduces over
    mslice: int      # rows per slice
    last: int        # rows of the last slice
    ntiles: int      # T2 tiles per slice
    Bp: int          # strip rows (B rounded up to 32)
    o_xt: int        # byte offsets of the T1 -> T2 operand strips in the workspace
    o_act: int
    o_dzt: int
    in_max: int


def host_layout(B: int, in_dims: Sequence[int], widths: Sequence[int], flags: int = 0, multi: bool = False) -> Layout:
    """tower_layout's slicing and launch_t1's kernel choice for the pooled entry point (multi: the
    indexed multi-feature entry point, always the general kernel)."""
    L, in_max = len(widths), max(in_dims)
    Ks = [[d] + list(widths[:-1]) for d in in_dims]
    if in_max <= MAXW:
        t2 = "staged"
        ntiles = 2 * sum(_cdiv(w, T2_NT) for w in widths)
        s0 = min(64, _cdiv(B, T2_PASS))
        mslice = _cdiv(_cdiv(B, s0), T2_PASS) * T2_PASS
        S = _cdiv(B, mslice)
    else:
        t2 = "register"
        ntiles = sum((w // 32) * (k // 32) for t in range(2) for w, k in zip(widths, Ks[t]))
        S = max(1, 400 // max(1, ntiles))
        S = min(S, max(1, _cdiv(B, 512)), 64)
        mslice = _cdiv(_cdiv(B, S), 128) * 128
    two = L == 2 and in_max <= 128
    prod = two and list(widths) == [128, 64] and in_dims[0] == in_dims[1] and in_dims[0] in (64, 128)
    if multi or not two:
        t1 = "general"
    elif prod and not flags & GENERAL_T1:
        t1 = "rows"
    else:
        t1 = "l2-runtime"
    Bp = _cdiv(B, 32) * 32
    o_act = _align(2 * in_max * Bp * 2)
    o_dzt = o_act + _align(2 * MAXL * MAXW * Bp * 2)
    return Layout(t1, t2, S, mslice, B - (S - 1) * mslice, ntiles, Bp, 0, o_act, o_dzt, in_max)


@dataclass(frozen=True)
class Case:
    id: str
    B: int
    in_dims: tuple
    widths: tuple
    branch: str          # what the case exists for
    t1: str              # expected dispatch (asserted below against host_layout)
    t2: str
    S: int
    mslice: int
    last: int
    amb: float           # measured share of ambiguous rows (fp64 emulation, this seed)
    floor: str = ""      # measured fp32-replay floors (worst over 8 summation orders)
    D: int = 0           # > 0: the indexed multi-feature T1 with D-wide features (flags = GENERAL_T1)
    adam: bool = False   # also one Adam step over the full parameter vector
    seed_add: int = 0    # seed = B + L + seed_add, chosen so the emulation meets `check_conditions`
    row_rtol: float = ROW_RTOL
    logit_rtol: float = LOGIT_RTOL
    grad_rtol: float = GRAD_RTOL

    @property
    def L(self) -> int:
        return len(self.widths)

    @property
    def seed(self) -> int:
        return self.B + self.L + self.seed_add

    @property
    def flags(self) -> int:
        return GENERAL_T1 if self.D else 0

    @property
    def cols(self) -> List[int]:
        return [0, self.in_dims[0]] if self.D else [16, 16 + self.in_dims[0]]

    @property
    def layout(self) -> Layout:
        return host_layout(self.B, self.in_dims, self.widths, self.flags, multi=self.D > 0)


CASES = [
    Case("l1-min", 8, (32, 32), (32,), "L = 1, smallest everything, one 8-row workgroup",
         "general", "staged", 1, 256, 8, amb=0.0,
         floor="row 2.8e-8, logit 1.1e-7, grad 1.4e-7, frob 9.1e-8", adam=True),
    Case("l1-w128", 40, (64, 96), (128,), "L = 1 full width, second workgroup holds 8 rows",
         "general", "staged", 1, 256, 40, amb=0.0,
         floor="row 1.7e-3, logit 1.7e-7, grad 1.1e-6, frob 3.1e-7"),
    Case("l1-wide-ragged", 1032, (160, 32), (32,),
         "partial 128-column chunk, narrow tower on the register T2, S = 3 with a 264-row last slice",
         "general", "register", 3, 384, 264, amb=0.001,
         floor="row 5.6e-4, logit 4.4e-7, grad 5.5e-5, frob 1.9e-5"),
    Case("l2-grow", 200, (128, 128), (64, 128), "run-time two-layer kernel, w1 > w0",
         "l2-runtime", "staged", 1, 256, 200, amb=0.02,
         floor="row 2.6e-3, logit 3.2e-4, grad 1.1e-5, frob 3.9e-6"),
    Case("l2-w32", 200, (32, 128), (32, 32), "run-time two-layer kernel, width 32 twice, unequal inputs",
         "l2-runtime", "staged", 1, 256, 200, amb=0.0,
         floor="row 5.7e-5, logit 1.9e-7, grad 1.4e-5, frob 5.4e-6"),
    Case("l2-uneven-rk", 200, (128, 64), (128, 64), "production widths with unequal inputs: not the row-owned kernel",
         "l2-runtime", "staged", 1, 256, 200, amb=0.015,
         floor="row 4.0e-3, logit 1.0e-3, grad 2.4e-4, frob 1.5e-4"),
    Case("l3-96", 264, (96, 96), (128, 96, 64), "N = 96 as a hidden layer of the general kernel; staged T2 with S = 2",
         "general", "staged", 2, 256, 8, amb=0.102,
         floor="row 2.3e-3, logit 7.2e-4, grad 1.9e-4, frob 1.1e-4"),
    Case("l3-wide", 200, (1024, 32), (128, 64, 32), "maximum input beside minimum input, L = 3 on the register T2",
         "general", "register", 1, 256, 200, amb=0.08,
         floor="row 2.8e-3, logit 1.9e-3, grad 3.2e-4, frob 3.0e-4", adam=True),
    Case("l4-grow", 520, (64, 96), (32, 64, 96, 128), "L = 4, widths rising, staged T2 with S = 3 (last slice 8 rows)",
         "general", "staged", 3, 256, 8, amb=0.206,
         floor="row 2.8e-3, logit 4.0e-5, grad 9.4e-5, frob 5.1e-5"),
    Case("l4-full", 200, (128, 128), (128, 128, 128, 128), "16 staged T2 tiles: the t2_code boundary",
         "general", "staged", 1, 256, 200, amb=0.545,
         floor="row 1.2e-3, logit 1.9e-7, grad 9.2e-4, frob 4.3e-4", adam=True),
    Case("l4-wide", 136, (160, 1024), (64, 96, 128, 32), "L = 4 on the register T2, partial chunk beside the maximum input",
         "general", "register", 1, 256, 136, amb=0.382,
         floor="row 2.3e-5, logit 1.8e-7, grad 3.2e-5, frob 5.8e-6"),
    # the indexed multi-feature T1 (tt_tower_fwd_bwd_indexed_multi_bf16), D-wide features
    Case("idx-d16", 200, (64, 64), (128, 64), "D = 16; only TT_TOWER_GENERAL_T1 keeps T3 off the row-owned weight image",
         "general", "staged", 1, 256, 200, amb=0.01,
         floor="row 3.1e-3, logit 5.5e-4, grad 1.7e-4, frob 7.9e-5", D=16),
    Case("idx-d128", 136, (256, 128), (96, 64, 32), "D = 128: a feature is a whole 128-column chunk",
         "general", "register", 1, 256, 136, amb=0.066,
         floor="row 6.4e-8, logit 2.0e-7, grad 2.5e-7, frob 1.5e-7", D=128,
         # seed B + L itself: 3 of 8 replay orders flip one ambiguous ReLU unit whose row carries up to
         # 3.7 % of a gradient's largest element at B = 136, so the reference alone broke GRAD_RTOL
         seed_add=1),
    Case("idx-d32", 40, (160, 32), (64,), "D = 32, L = 1, partial chunk: 5 query features + 1 candidate feature",
         "general", "register", 1, 128, 40, amb=0.0,
         floor="row 4.5e-8, logit 1.8e-7, grad 1.7e-7, frob 9.0e-8", D=32),
]
BY_ID = {c.id: c for c in CASES}
POOLED = [c.id for c in CASES if not c.D]
INDEXED = [c.id for c in CASES if c.D]


def check_dispatch(c: Case) -> None:
    """The case still reaches the branch it is in the table for (host arithmetic only)."""
    lay = c.layout
    got = (lay.t1, lay.t2, lay.S, lay.mslice, lay.last)
    assert got == (c.t1, c.t2, c.S, c.mslice, c.last), (c.id, got)
    assert (lay.t2 == "staged") == (max(c.in_dims) <= MAXW), c.id
    assert 0 < lay.last <= lay.mslice and (lay.S - 1) * lay.mslice < c.B, c.id
    if lay.t2 == "staged":
        assert lay.ntiles <= 16, c.id  # TowerLayout::t2_code[16]
    assert c.B % 8 == 0 and 1 <= c.L <= MAXL, c.id
    assert all(w % 32 == 0 and 32 <= w <= MAXW for w in c.widths), c.id
    assert all(d % 32 == 0 and 32 <= d <= 1024 for d in c.in_dims), c.id
    if c.D:
        assert XCH % c.D == 0 and all(d % c.D == 0 for d in c.in_dims), c.id


for _c in CASES:
    check_dispatch(_c)
# what the table is for, stated on the cases themselves
assert BY_ID["l4-full"].layout.ntiles == 16
assert BY_ID["l1-wide-ragged"].last % 128 and BY_ID["l1-wide-ragged"].in_dims[0] % XCH
assert BY_ID["l4-grow"].S == 3 and BY_ID["l4-grow"].last == 8
assert all(BY_ID[i].t1 == "l2-runtime" for i in ("l2-grow", "l2-w32", "l2-uneven-rk"))
assert host_layout(200, (64, 64), (128, 64)).t1 == "rows"  # idx-d16's shape without the flag


# ---- inputs ------------------------------------------------------------------------------------

class Inputs:
    """A case's fixed inputs (CPU tensors), drawn as tests/test_gpu_tower_edges.Family draws them:
    weights randn / sqrt(K), biases randn * 0.1, int32 0 / 1 labels, tower inputs randn * 0.5."""

    def __init__(self, c: Case):
        self.case = c
        B, in_dims = c.B, c.in_dims
        g = torch.Generator().manual_seed(c.seed)
        ps = []
        for t in range(2):
            k = in_dims[t]
            for w in c.widths:
                ps.append(torch.randn(w, k, generator=g) / k ** 0.5)
                ps.append(torch.randn(w, generator=g) * 0.1)
                k = w
        self.flat = torch.cat([p.reshape(-1) for p in ps])
        self.params = split_params(self.flat, in_dims, c.widths)
        self.labels = torch.randint(0, 2, (B,), generator=g).to(torch.int32)
        self.cols = c.cols
        if not c.D:
            self.ldp = sum(in_dims) + 32
            self.pooled = torch.full((B, self.ldp), SENT)
            for t in range(2):
                self.pooled[:, self.cols[t]:self.cols[t] + in_dims[t]] = torch.randn(B, in_dims[t], generator=g) * 0.5
            self.x = [self.pooled[:, self.cols[t]:self.cols[t] + in_dims[t]].clone() for t in range(2)]
            return
        # indexed: one bf16 buffer of F * B + 24 rows of D; lookup j = f * B + m reads row pos_in[j] and
        # its gradient goes to row pos_out[j] (two DIFFERENT permutations); every 19th lookup is dropped
        D = c.D
        self.F = sum(in_dims) // D
        self.feat0 = [0, in_dims[0] // D]
        n = self.F * B
        self.NR = n + 24
        self.rows_in = (torch.randn(self.NR, D, generator=g) * 0.5).to(torch.bfloat16)
        self.pos_in = torch.randperm(self.NR, generator=g)[:n].to(torch.int32)
        self.pos_out = torch.randperm(self.NR, generator=g)[:n].to(torch.int32)
        assert not torch.equal(self.pos_in, self.pos_out)
        self.pos_in[::19] = -1
        self.pos_out[::19] = -1
        rows = torch.where((self.pos_in >= 0)[:, None], self.rows_in.float()[self.pos_in.clamp(min=0).long()],
                           torch.zeros(()))  # [F * B, D]
        per_f = rows.view(self.F, B, D)
        self.x = [torch.cat(list(per_f[self.feat0[t]:self.feat0[t] + in_dims[t] // D]), 1) for t in range(2)]

    def dx_from_rows(self, grad_rows: torch.Tensor, fill: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """Indexed: dX [B, in] per tower from the gradient-row buffer; a dropped lookup has no
        gradient row, its columns are taken from ``fill`` (nothing to compare)."""
        c, B, D = self.case, self.case.B, self.case.D
        po = self.pos_out.view(self.F, B)
        out = []
        for t in range(2):
            parts = []
            for k in range(c.in_dims[t] // D):
                p = po[self.feat0[t] + k]
                got = grad_rows[p.clamp(min=0).long()]
                parts.append(torch.where((p >= 0)[:, None], got, fill[t][:, k * D:(k + 1) * D].to(got.dtype)))
            out.append(torch.cat(parts, 1))
        return out


@functools.lru_cache(maxsize=None)
def inputs(case_id: str) -> Inputs:
    return Inputs(BY_ID[case_id])


@functools.lru_cache(maxsize=None)
def emulation(case_id: str):
    """emulate_bounds of the case's inputs, computed once per process and never modified."""
    inp = inputs(case_id)
    return emulate_bounds(inp.x[0], inp.x[1], inp.params, BY_ID[case_id].widths, inp.labels)


# ---- checks shared by the GPU sweep and the CPU check of the oracle --------------------------------

def check_conditions(c: Case, emu) -> dict:
    """What keeps check_towers from being vacuous on this case's emulation: at most two thirds of
    the rows ambiguous, at least 4 unambiguous rows in the last workgroup, an unambiguous row of
    every residue mod 8 (T1 stores strips in runs of 8 rows), no all-zero dX row, a logit > 0.5."""
    (lg, _), _, dxs, _, amb = emu
    B = c.B
    ok = ~amb
    share = float(amb.sum()) / B
    assert share <= 2 / 3, (c.id, "ambiguous share", share)
    last0 = 32 * ((B - 1) // 32)
    n_last = int(ok[last0:].sum())
    assert n_last >= 4, (c.id, "unambiguous rows in the last workgroup", n_last)
    res = sorted(set((ok.nonzero().flatten() % 8).tolist()))
    assert res == list(range(8)), (c.id, "row residues mod 8 with an unambiguous row", res)
    for t in range(2):
        assert bool((dxs[t][0].abs().amax(1) > 0).all()), (c.id, f"an all-zero emulated dX[{t}] row")
    assert float(lg.abs().max()) > 0.5, (c.id, "flat logits")
    return {"amb": share, "last_wg_ok": n_last, "max_logit": float(lg.abs().max())}


def check_frobenius(emu, dx, grads, what: str = "") -> float:
    """Relative Frobenius error of each dX and each gradient tensor against the emulation below
    FROB_RTOL: in aggregate this covers the rows check_towers sets aside as ambiguous."""
    _, _, dxs, gw, _ = emu
    worst = 0.0
    for t in range(2):
        e = rel_err(dx[t], dxs[t][0])
        assert e < FROB_RTOL, (what, f"dX[{t}] relative Frobenius error", e)
        worst = max(worst, e)
    for j, (want, _) in enumerate(gw):
        e = rel_err(grads[j], want)
        assert e < FROB_RTOL, (what, f"grad[{j}] relative Frobenius error", e)
        worst = max(worst, e)
    return worst


def check_case(c: Case, emu, logits, dx, grads, what: Optional[str] = None) -> dict:
    """check_towers at the case's thresholds (the defaults unless the table says otherwise) + the
    whole-tensor check."""
    stats = check_towers(emu, logits, dx, grads, what or c.id, row_rtol=c.row_rtol, logit_rtol=c.logit_rtol,
                         grad_rtol=c.grad_rtol)
    stats["frobenius_max"] = check_frobenius(emu, dx, grads, what or c.id)
    return stats


# ---- the fp32 replay: a correct implementation in another summation order -----------------------

def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.float().to(torch.bfloat16).float()


def _mm(a: torch.Tensor, b: torch.Tensor, g: torch.Generator) -> torch.Tensor:
    """a [M, K] @ b [K, N] in fp32 with the K axis permuted and split into partial sums (2..5 of
    unequal length, added in sequence)."""
    K = a.shape[1]
    perm = torch.randperm(K, generator=g)
    n = min(K, 2 + int(torch.randint(0, 4, (1,), generator=g)))
    cuts = sorted(set([0, K] + torch.randint(1, K, (n - 1,), generator=g).tolist()))
    out = None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        idx = perm[lo:hi]
        part = a[:, idx].contiguous() @ b[idx].contiguous()
        out = part if out is None else out + part
    return out


def fp32_replay(x: Sequence[torch.Tensor], params: Sequence[torch.Tensor], widths: Sequence[int],
                labels: torch.Tensor, order_seed: int):
    """The towers with the kernels' rounding points (bf16 X, W, hidden activations and dZ; fp32
    accumulation; fp32 last-layer outputs; bias gradients from the unrounded dZ) in fp32 torch
    arithmetic, every sum in an order drawn from ``order_seed``. -> logits, [dXq, dXc], grads."""
    g = torch.Generator().manual_seed(order_seed)
    B, L = x[0].shape[0], len(widths)
    ones = torch.ones(1, B)
    Ws = [_bf(p) if p.dim() == 2 else p.float() for p in params]
    acts, outs, i = [], [], 0
    for xt in x:
        h = _bf(xt)
        a_t = [h]
        for li in range(L):
            z = torch.relu(_mm(h, Ws[i].T, g) + Ws[i + 1])
            i += 2
            h = z if li == L - 1 else _bf(z)
            a_t.append(h)
        acts.append(a_t)
        outs.append(h)
    logits = _mm(outs[0] * outs[1], torch.ones(widths[-1], 1), g)[:, 0]
    dl = (torch.sigmoid(logits) - labels.float()) / B
    grads, dxs = [], []
    for t in range(2):
        dz = dl[:, None] * outs[1 - t] * (outs[t] > 0)
        g_t = [None] * (2 * L)
        for li in reversed(range(L)):
            g_t[2 * li] = _mm(_bf(dz).T, acts[t][li], g)
            g_t[2 * li + 1] = _mm(ones, dz, g)[0]
            dA = _mm(_bf(dz), Ws[t * 2 * L + 2 * li], g)
            dz = dA * (acts[t][li] > 0) if li > 0 else dA
        dxs.append(dz)
        grads += g_t
    return logits, dxs, grads
