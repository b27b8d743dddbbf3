"""The shape sweep's oracle checked without a GPU (tests/tower_shapes.py is the case table).

For every case of the sweep, the indexed ones included:

(1) the reference alone is inside the thresholds: an fp32 replay of the kernels' rounding points,
    with every sum's K axis permuted and split into partial sums (8 different orders per case),
    passes the very same check_towers + whole-tensor Frobenius checks the GPU sweep applies to the
    kernels. A correct fp32 implementation in another summation order is therefore not rejected at
    these shapes; the GPU's MFMA order is one more draw from the same distribution;
(2) the conditions that keep the GPU check from being vacuous hold for the emulation itself (deep
    towers flag many rows as ambiguous, which check_towers leaves out of its row statistics): at
    most two thirds of the rows ambiguous, >= 4 unambiguous rows in the last workgroup, an
    unambiguous row of every residue mod 8, no all-zero dX row, max |logit| > 0.5; and the ambiguous
    share is the one written in the table;
(3) the checker bites at each shape: one unambiguous row of the last workgroup 2 % off fails;
(4) each case still reaches the branch it exists for (tower_shapes.check_dispatch, host only)."""
import pytest
import torch

import tower_shapes as ts
from tower_emul import GRAD_RTOL, LOGIT_RTOL, ROW_RTOL

ALL = [c.id for c in ts.CASES]


@pytest.mark.parametrize("cid", ALL)
def test_case_reaches_its_branch(cid):
    c = ts.BY_ID[cid]
    ts.check_dispatch(c)
    lay = c.layout
    print(f"{cid}: T1 {lay.t1}, T2 {lay.t2}, S {lay.S}, mslice {lay.mslice}, last slice {lay.last} rows, "
          f"{lay.ntiles} tiles")
    # no case's thresholds sit below the defaults, and a raised one is recorded with its floor
    assert c.row_rtol >= ROW_RTOL and c.logit_rtol >= LOGIT_RTOL and c.grad_rtol >= GRAD_RTOL
    assert c.floor


def test_the_table_covers_what_it_claims():
    by = ts.BY_ID
    assert {by[i].L for i in ts.POOLED} == {1, 2, 3, 4}
    assert by["l1-min"].B == 8 and by["l1-min"].layout.Bp == 32
    assert by["l4-full"].layout.ntiles == 16 and by["l4-full"].t2 == "staged"
    assert any(w1 > w0 for w0, w1 in zip(by["l4-grow"].widths, by["l4-grow"].widths[1:]))
    assert by["l2-grow"].widths[1] > by["l2-grow"].widths[0]
    assert 96 in by["l3-96"].widths[1:-1]
    for i in ("l1-wide-ragged", "l4-wide", "idx-d32"):  # a partial last 128-column chunk
        assert any(d > ts.XCH and d % ts.XCH for d in by[i].in_dims)
    for i in ("l1-wide-ragged", "l3-wide"):  # a 32-wide tower on the register-path T2
        assert by[i].t2 == "register" and min(by[i].in_dims) == 32
    assert by["l1-wide-ragged"].S == 3 and by["l1-wide-ragged"].last == 264
    assert sorted(by[i].D for i in ts.INDEXED) == [16, 32, 128]
    assert [i for i in ts.POOLED if by[i].adam] == ["l1-min", "l3-wide", "l4-full"]


@pytest.mark.parametrize("cid", ALL)
def test_emulation_is_not_vacuous(cid):
    c = ts.BY_ID[cid]
    cond = ts.check_conditions(c, ts.emulation(cid))
    print(cid, cond)
    assert abs(cond["amb"] - c.amb) <= 0.03, (cid, "ambiguous share differs from the table's", cond["amb"], c.amb)


@pytest.mark.parametrize("cid", ALL)
def test_fp32_replay_within_thresholds(cid):
    c, inp, emu = ts.BY_ID[cid], ts.inputs(cid), ts.emulation(cid)
    worst = {}
    for order in range(8):
        lg, dx, gr = ts.fp32_replay(inp.x, inp.params, c.widths, inp.labels, 1000 + order)
        st = ts.check_case(c, emu, lg, dx, gr, f"{cid} order {order}")
        for k, v in st.items():
            worst[k] = max(worst.get(k, 0), v)
    print(cid, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in worst.items()})


@pytest.mark.parametrize("cid", ALL)
def test_checker_bites_at_this_shape(cid):
    c, inp, emu = ts.BY_ID[cid], ts.inputs(cid), ts.emulation(cid)
    lg, dx, gr = ts.fp32_replay(inp.x, inp.params, c.widths, inp.labels, 7)
    ok = (~emu[4]).nonzero().flatten()
    row = int(ok[-1])  # an unambiguous row of the last workgroup
    assert row >= 32 * ((c.B - 1) // 32)
    for t in range(2):
        bad = [d.clone() for d in dx]
        bad[t][row] *= 1.02
        with pytest.raises(AssertionError, match="dX"):
            ts.check_case(c, emu, lg, bad, gr)
    # the last 32 input columns of the wider tower (a partial chunk where there is one) off by 1 %
    t = 0 if c.in_dims[0] >= c.in_dims[1] else 1
    bad = [d.clone() for d in dx]
    bad[t][:, -32:] *= 1.01
    with pytest.raises(AssertionError, match="dX"):
        ts.check_case(c, emu, lg, bad, gr)
    for j in (0, len(gr) - 2):  # one element of the first and of the last weight gradient
        bad = [g.clone() for g in gr]
        bad[j].view(-1)[-1] += 0.01 * float(bad[j].abs().max())
        with pytest.raises(AssertionError):
            ts.check_case(c, emu, lg, dx, bad)


@pytest.mark.parametrize("cid", ts.INDEXED)
def test_indexed_inputs_are_what_the_header_says(cid):
    """Column k of tower t's row m is column k % D of rows_in[pos_in[(feat0[t] + k / D) * B + m]]
    (zeros for -1), and dx_from_rows inverts the scatter of dX column blocks to rows pos_out."""
    c, inp = ts.BY_ID[cid], ts.inputs(cid)
    B, D = c.B, c.D
    assert inp.rows_in.shape == (inp.F * B + 24, D) and inp.rows_in.dtype == torch.bfloat16
    live_in, live_out = inp.pos_in[inp.pos_in >= 0], inp.pos_out[inp.pos_out >= 0]
    assert live_in.unique().numel() == live_in.numel() and live_out.unique().numel() == live_out.numel()
    assert bool(((inp.pos_in < 0) == (inp.pos_out < 0)).all()) and int((inp.pos_in < 0).sum()) == -(-inp.F * B // 19)
    assert not torch.equal(inp.pos_in, inp.pos_out)
    g = torch.Generator().manual_seed(1)
    for t in range(2):
        for _ in range(20):
            m, k = int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(0, c.in_dims[t], (1,), generator=g))
            p = int(inp.pos_in[(inp.feat0[t] + k // D) * B + m])
            want = float(inp.rows_in[p, k % D]) if p >= 0 else 0.0
            assert float(inp.x[t][m, k]) == want
    dxs = [d[0].float() for d in ts.emulation(cid)[2]]
    rows = torch.full((inp.NR, D), ts.SENT)
    po = inp.pos_out.view(inp.F, B)
    for t in range(2):
        for k in range(c.in_dims[t] // D):
            p = po[inp.feat0[t] + k]
            rows[p[p >= 0].long()] = dxs[t][:, k * D:(k + 1) * D][p >= 0]
    back = inp.dx_from_rows(rows, dxs)
    for t in range(2):
        assert torch.equal(back[t], dxs[t])
    used = torch.zeros(inp.NR, dtype=torch.bool)
    used[live_out.long()] = True
    assert int((~used).sum()) >= 24 and bool((rows[~used] == ts.SENT).all())
