"""Branches of the C ABI (include/tt_mi355x.h) that the workload-path tests never take (``-m gpu``).

1. bounds_check = 1 of tt_pooled_fwd (its three pooling paths), tt_bwd_prepare (+ the direct update's
   own clamp) and tt_pooled_bwd_dense, and tt_tower_fwd_bwd_kjt's "an id >= num_rows reads row 0".
   The oracle of every check is the oracle of the same op with the out-of-range ids replaced by 0.
   The ids are WINDOWED (tests/edge_cases.py): the tables under test are tables 1 and 3 of a
   five-table allocation and an out-of-range id lies within one table's length of its table, so an
   access that a broken check lets through lands in a pad table of the same allocation — and the
   pad tables are asserted bitwise unchanged. Also tt_pooled_fwd's output placement (out_row != 0,
   ldo > out_dim, gapped out_offset): the cells no bag owns keep a sentinel.
2. The KJT glue kernels tt_kjt_single_hot_cols and tt_kjt_admit against their restatements
   (oracle/ref.py), bit-exact, and tt_kjt_permute / tt_block_bucketize beyond one workgroup and
   beyond one grid (grid-stride), with int32 ids and without weights.
5. Dense options: tt_linear_* with relu = 0, no bias, no Y, strided X / Y / dX; tt_dot_bce_fwd_bwd
   with grad_scale, forward only, soft labels and saturated logits; every Adam form with
   weight_decay, betas and eps off their defaults against torch.optim.Adam.

Tolerances are the project's existing ones for each op (tests/test_gpu_ops.py), none wider."""
import numpy as np
import pytest
import torch

import edge_cases as ec
from oracle import ref
from test_gpu_ops import _bf16_gemm_check

pytestmark = pytest.mark.gpu

R = 200        # rows per table of the windowed TableSet (a multiple of 4)
PAD_W = 7.5    # the pad tables' weights
PAD_S = 3.25   # and row-wise state


@pytest.fixture(scope="module")
def ops():
    from two_tower_recommender_model_amd import ops as _ops

    return _ops


def _window(ops, device, D, seed=5):
    """(src, win): five [R, D] tables, pads (0, 2, 4) constant, and the view of tables 1 and 3."""
    src = ops.TableSet([R] * 5, [D] * 5, list(range(5)), device)
    src.weights.fill_(PAD_W)
    src.state.fill_(PAD_S)
    g = torch.Generator(device=device).manual_seed(seed)
    for t in ec.WINDOW_TABLES:
        src.table_view(t).uniform_(-(1.0 / R) ** 0.5, (1.0 / R) ** 0.5, generator=g)
        src.state_view(t).zero_()
    win = ops.TableSet.view_of(src, list(ec.WINDOW_TABLES), [D, D], device)
    spec = ec.WindowSpec(R, D)
    assert src.weight_offsets == spec.weight_offsets and src.total_weights == spec.total_weights
    assert win.weights.data_ptr() == src.weights.data_ptr() and win.state.data_ptr() == src.state.data_ptr()
    return src, win


def _assert_pads_untouched(src):
    for t in (0, 2, 4):
        w, s = src.table_view(t), src.state_view(t)
        assert bool((w == PAD_W).all()), f"pad table {t} was written"
        assert bool((s == PAD_S).all()), f"pad state {t} was written"


# ---- 1. bounds-check mode ---------------------------------------------------------------------------


@pytest.mark.parametrize("D", [128, 512, 10], ids=["d128-row4", "d512-cols4", "d10-cols1"])
@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("pooling", ["sum", "mean"])
def test_pooled_fwd_bounds_check(ops, device, D, dtype, pooling):
    """Out-of-range ids read row 0 and are counted exactly (err_count is cumulative)."""
    spec = ec.WindowSpec(R, D)
    wb = ec.windowed_batch(spec, seed=D, dtype=dtype)
    assert ec.window_in_allocation(spec, wb)
    B = wb.lengths.size // 2
    src, win = _window(ops, device, D)
    tabs = [win.table_view(t).cpu().clone() for t in range(2)]
    V, O = torch.from_numpy(wb.values).to(device), torch.from_numpy(wb.offsets).to(device)
    win.err_count.zero_()
    out = win.pooled_fwd(V, O, B, pooling=1 if pooling == "mean" else 0, bounds_check=True)
    torch.cuda.synchronize()
    want = ref.pooled_fwd(tabs, [0, 1], torch.from_numpy(wb.clamped), torch.from_numpy(wb.offsets), B, pooling)
    ec.assert_pooled_close(out.cpu().numpy(), want.numpy(), wb.maxlen)
    assert int(win.err_count[0]) == wb.n_oob
    out2 = win.pooled_fwd(V, O, B, pooling=1 if pooling == "mean" else 0, bounds_check=True)
    torch.cuda.synchronize()
    assert int(win.err_count[0]) == 2 * wb.n_oob
    ec.assert_bitwise(out2, out, "second call")
    _assert_pads_untouched(src)


@pytest.mark.parametrize("pooling", ["sum", "mean"])
@pytest.mark.parametrize("dims", [[16, 32], [6, 10]], ids=["vec4", "scalar"])
def test_pooled_fwd_out_row_ldo_and_gapped_offsets(ops, device, dims, pooling):
    """What the sharded lookup uses: out_row != 0 (features stacked as row blocks), a row stride above
    out_dim and gaps between the features' columns; every cell no bag owns keeps its sentinel."""
    rng = np.random.default_rng(sum(dims))
    B, rows, ft = 37, [50, 80], [0, 1, 0]
    out_offsets, out_rows, ldo = [8, 40, 84], [0, B, 3], 128
    lengths = rng.integers(0, 6, 3 * B).astype(np.int32)
    offsets = ref.complete_cumsum(lengths)
    values = np.concatenate([rng.integers(0, rows[ft[i // B]], lengths[i]) for i in range(3 * B)])
    ts = ops.TableSet(rows, dims, ft, device, out_offsets=out_offsets, out_rows=out_rows)
    ts.init_uniform_(torch.Generator(device=device).manual_seed(1))
    assert ts.out_dim < ldo
    out = torch.full((2 * B + 5, ldo), SENT, device=device)
    ts.pooled_fwd(torch.from_numpy(values).to(device), torch.from_numpy(offsets).to(device), B,
                  pooling=1 if pooling == "mean" else 0, out=out)
    torch.cuda.synchronize()
    want = ref.pooled_fwd([ts.table_view(t).cpu() for t in range(2)], ft, torch.from_numpy(values),
                          torch.from_numpy(offsets), B, pooling)
    got, owned, c = out.cpu(), torch.zeros(2 * B + 5, ldo, dtype=torch.bool), 0
    for f, t in enumerate(ft):
        r0, c0, d = out_rows[f], out_offsets[f], dims[t]
        ec.assert_pooled_close(got[r0:r0 + B, c0:c0 + d].numpy(), want[:, c:c + d].numpy(), int(lengths.max()))
        assert not bool(owned[r0:r0 + B, c0:c0 + d].any())  # the layout itself does not overlap
        owned[r0:r0 + B, c0:c0 + d] = True
        c += d
    assert bool((got[~owned] == SENT).all()), "a cell outside every feature's block was written"


@pytest.mark.parametrize("D,parts", [(128, (0,)), (128, (1, 2)), (256, (0,))], ids=["d128", "d128-parts", "d256"])
@pytest.mark.parametrize("lone", [False, True], ids=["mixed", "lone-row0"])
@pytest.mark.parametrize("pooling", ["sum", "mean"])
def test_bwd_prepare_bounds_check_rowwise_adagrad(ops, device, D, parts, lone, pooling):
    """tt_bwd_prepare(bounds_check = 1) + tt_bwd_rowwise_adagrad, two steps: out-of-range ids update
    row 0. D = 128 takes the direct kernel for rows looked up once (which re-reads the ids and clamps
    them itself: with ``lone`` the only lookup of feature 1's row 0 is ONE out-of-range id, so the
    grouping files it under row 0 with count 1 and the direct kernel must reach the same row);
    D = 256 the generic path. Parts 1 + 2 give part 0's bits."""
    spec = ec.WindowSpec(R, D)
    wb = ec.windowed_batch(spec, seed=D + 1, dtype=np.int32 if lone else np.int64, lone_row0=lone)
    assert ec.window_in_allocation(spec, wb)
    B = wb.lengths.size // 2
    pool = 1 if pooling == "mean" else 0
    lr, eps = 0.05, 1e-10
    V, O = torch.from_numpy(wb.values).to(device), torch.from_numpy(wb.offsets).to(device)
    gouts = [torch.randn(B, 2 * D, generator=torch.Generator().manual_seed(step)) for step in range(2)]

    def run(parts_):
        src, win = _window(ops, device, D)
        tabs = [win.table_view(t).cpu().clone() for t in range(2)]
        for gout in gouts:
            win.bwd_prepare(V, O, B, max_lookups=wb.values.size, bounds_check=True)
            for p in parts_:
                win.bwd_rowwise_adagrad(gout.to(device), O, B, lr, eps, pooling=pool, part=p)
        torch.cuda.synchronize()
        return src, win, tabs

    src, win, tabs = run(parts)
    states = [torch.zeros(R) for _ in range(2)]
    cl, off = torch.from_numpy(wb.clamped), torch.from_numpy(wb.offsets)
    for gout in gouts:
        grads = ref.pooled_bwd_dense(tabs, [0, 1], cl, off, B, gout, pooling)
        for t in range(2):
            ref.rowwise_adagrad(tabs[t], states[t], grads[t], lr, eps)
    for t in range(2):
        ec.assert_adagrad_close(win.table_view(t).cpu().numpy(), win.state_view(t).cpu().numpy(), tabs[t].numpy(),
                                states[t].numpy())
    if lone:  # the handoff row did move: feature 1's row 0 has exactly one (out-of-range) lookup
        assert float(states[1][0]) > 0 and float(win.state_view(1)[0]) > 0
    _assert_pads_untouched(src)
    if parts != (0,):
        src0, win0, _ = run((0,))
        ec.assert_bitwise(win.weights, win0.weights, "parts 1 + 2 vs part 0: weights")
        ec.assert_bitwise(win.state, win0.state, "parts 1 + 2 vs part 0: state")


@pytest.mark.parametrize("pooling", ["sum", "mean"])
@pytest.mark.parametrize("D", [128, 10])
def test_pooled_bwd_dense_bounds_check(ops, device, D, pooling):
    spec = ec.WindowSpec(R, D)
    wb = ec.windowed_batch(spec, seed=D + 2)
    assert ec.window_in_allocation(spec, wb)
    B = wb.lengths.size // 2
    src, win = _window(ops, device, D)
    gout = torch.randn(B, 2 * D, generator=torch.Generator().manual_seed(1))
    gw = torch.zeros_like(src.weights)
    win.bwd_dense(gout.to(device), torch.from_numpy(wb.values).to(device), torch.from_numpy(wb.offsets).to(device), B,
                  gw, pooling=1 if pooling == "mean" else 0, bounds_check=True)
    torch.cuda.synchronize()
    want = ref.pooled_bwd_dense([win.table_view(t).cpu() for t in range(2)], [0, 1], torch.from_numpy(wb.clamped),
                                torch.from_numpy(wb.offsets), B, gout, pooling)
    for i, t in enumerate(ec.WINDOW_TABLES):
        o = src.weight_offsets[t]
        got = gw[o:o + R * D].view(R, D).cpu()
        np.testing.assert_allclose(got.numpy(), want[i].numpy(), rtol=1e-5, atol=1e-5)
    for t in (0, 2, 4):
        o = src.weight_offsets[t]
        assert int(torch.count_nonzero(gw[o:o + R * D])) == 0, f"gradient written into pad table {t}"
    _assert_pads_untouched(src)


def _tower_params(in_dims, widths, g):
    ps = []
    for t in range(2):
        k = in_dims[t]
        for w in widths:
            ps.append(torch.randn(w, k, generator=g) / k ** 0.5)
            ps.append(torch.randn(w, generator=g) * 0.1)
            k = w
    return torch.cat([p.reshape(-1) for p in ps])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_tower_fwd_bwd_kjt_out_of_range_ids_read_row0(ops, device, D, dtype):
    """tt_tower_fwd_bwd_kjt with ids in [num_rows, 2 num_rows): pooled rows, logits and dX bitwise
    equal to tt_pooled_fwd(bounds_check = 1) + tt_tower_fwd_bwd. The tables are the first half of
    [2 num_rows, D] allocations, so an unclamped read stays inside them."""
    rng = np.random.default_rng(D)
    B, NR = 200, 300
    lengths = rng.integers(0, 10, 2 * B).astype(np.int32)
    offsets = ref.complete_cumsum(lengths)
    n = int(offsets[-1])
    values = rng.integers(0, NR, n)
    oob = rng.random(n) < 0.15
    values = np.where(oob, rng.integers(NR, 2 * NR, n), values)
    values[offsets[3]:offsets[4]] = rng.integers(NR, 2 * NR, lengths[3])  # a bag entirely out of range
    assert ((values >= NR).sum() > 20) and values.max() < 2 * NR and values.min() >= 0
    g = torch.Generator().manual_seed(2)
    big = [torch.empty(2 * NR, D).uniform_(-0.1, 0.1, generator=g).to(device) for _ in range(2)]
    table_rows = [b[:NR] for b in big]
    ts = ops.TableSet([NR, NR], [D, D], [0, 1], device)
    for t in range(2):
        ts.table_view(t).copy_(table_rows[t])
    V, O = torch.from_numpy(values).to(dtype).to(device), torch.from_numpy(offsets).to(device)
    labels = torch.randint(0, 2, (B,), generator=g).to(torch.int32).to(device)
    P = _tower_params([D, D], [128, 64], g).to(device)
    outs = []
    for fused in (False, True):
        tw = ops.FusedTowers([D, D], [128, 64], [0, D], B, device)
        tw.update(P, do_adam=False)
        gp = torch.zeros(B, 2 * D, device=device)
        logits = torch.empty(B, device=device)
        if fused:
            pooled = torch.empty(B, 2 * D, device=device)
            tw.fwd_bwd_kjt(V, O, table_rows, gp, P, labels, logits, pooled_out=pooled)
        else:
            ts.err_count.zero_()
            pooled = ts.pooled_fwd(V, O, B, bounds_check=True)
            tw.fwd_bwd(pooled, gp, P, labels, logits)
        torch.cuda.synchronize()
        outs.append((pooled, logits, gp))
    assert int(ts.err_count[0]) == int((values >= NR).sum())
    for name, a, b in zip(("pooled", "logits", "dX"), outs[1], outs[0]):
        ec.assert_bitwise(a, b, name)
    # and the reference side is the clamped oracle (so both are right, not merely equal)
    want = ref.pooled_fwd([t.cpu() for t in table_rows], [0, 1], torch.from_numpy(np.where(values >= NR, 0, values)),
                          torch.from_numpy(offsets), B)
    ec.assert_pooled_close(outs[1][0].cpu().numpy(), want.numpy(), int(lengths.max()))


# ---- 2. KJT glue kernels ----------------------------------------------------------------------------

BIG_N = {np.int64: 2 ** 31 + 11, np.int32: 2 ** 31 - 1}


def _tdt(dtype):
    return torch.int64 if dtype == np.int64 else torch.int32


def _run_single_hot(ops, device, values, offsets, F_, B, N, dtype, err=None, labels=None, want_labels=True):
    cols = [torch.full((B,), -7, dtype=_tdt(dtype), device=device) for _ in range(F_)]
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=device)
    lab_out = torch.full((B,), -7, dtype=torch.int32, device=device) if labels is not None and want_labels else None
    ops.kjt_single_hot_cols(torch.from_numpy(values).to(device), torch.from_numpy(offsets).to(device), B, N, cols, err,
                            labels=labels, labels_out=lab_out)
    torch.cuda.synchronize()
    return cols, err, lab_out


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
def test_kjt_single_hot_cols(ops, device, dtype):
    rng = np.random.default_rng(1)
    F_, B = 3, 1000
    N = [7, 1000, BIG_N[dtype]]
    values, offsets = ec.single_hot_kjt(rng, F_, B, N, dtype)
    assert int((np.diff(offsets) == 0).sum()) > 200 and (values == 0).sum() >= 3
    want, want_err = ref.kjt_single_hot_cols(values, offsets, F_, B, N)
    assert want_err == 0
    for ldt in (torch.int64, torch.int32):
        labels = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(3)).to(ldt)
        if ldt == torch.int64:
            labels[5] = -1  # a negative int64 label is copied by value, not by its low word alone
        cols, err, lab = _run_single_hot(ops, device, values, offsets, F_, B, N, dtype, labels=labels.to(device))
        ec.assert_ints_equal(torch.stack(cols).cpu().numpy(), want.astype(dtype), "columns")
        assert int(err[0]) == 0
        assert lab.dtype == torch.int32
        ec.assert_ints_equal(lab.cpu().numpy(), labels.numpy().astype(np.int32), "labels")
    cols, err, lab = _run_single_hot(ops, device, values, offsets, F_, B, N, dtype)  # labels_out = None
    assert lab is None and int(err[0]) == 0
    ec.assert_ints_equal(torch.stack(cols).cpu().numpy(), want.astype(dtype), "columns (no labels)")
    # the inverse: the builder gives the KJT back
    v2, _, o2, _ = ops.kjt_build_mod_dropzero(cols, N)
    torch.cuda.synchronize()
    ec.assert_ints_equal(o2.cpu().numpy(), offsets, "round trip offsets")
    ec.assert_ints_equal(v2[:values.size].cpu().numpy(), values, "round trip values")


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
def test_kjt_single_hot_cols_error_bits(ops, device, dtype):
    rng = np.random.default_rng(2)
    F_, B = 3, 1000
    N = [7, 1000, BIG_N[dtype]]
    lengths = (rng.random(F_ * B) >= 0.1).astype(np.int32)
    lengths[[B + 17, 2 * B + 3, 2 * B + 4]] = 1

    def make(multi, bad):
        ln = lengths.copy()
        if multi:
            ln[40] = 2
        off = ref.complete_cumsum(ln)
        v = np.concatenate([rng.integers(0, N[f], int(ln[f * B:(f + 1) * B].sum()), dtype=np.int64)
                            for f in range(F_)])
        if bad:
            v[off[B + 17]] = N[1]   # the value N
            v[off[2 * B + 3]] = -1  # and -1
            if dtype == np.int64:
                v[off[2 * B + 4]] = N[2]  # a value N above 2^31 (the int32 case's N is the largest int32)
        return v.astype(dtype), off

    err = None
    for multi, bad, bits in ((True, False, 1), (False, True, 2), (True, True, 3)):
        v, off = make(multi, bad)
        want, want_err = ref.kjt_single_hot_cols(v, off, F_, B, N)
        assert want_err == bits
        cols, err, _ = _run_single_hot(ops, device, v, off, F_, B, N, dtype)
        assert int(err[0]) == bits
        got = torch.stack(cols).cpu().numpy()
        ec.assert_ints_equal(got, want.astype(dtype), f"columns, err bits {bits}")
        if multi:
            assert got[0, 40] == 0
        if bad:
            assert got[1, 17] == 0 and got[2, 3] == 0 and (dtype == np.int32 or got[2, 4] == 0)
    # sticky: a clean call leaves the bits of the last (3) call
    v, off = make(False, False)
    _, err, _ = _run_single_hot(ops, device, v, off, F_, B, N, dtype, err=err)
    assert int(err[0]) == 3


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
def test_kjt_single_hot_cols_all_empty(ops, device, dtype):
    F_, B = 3, 1000
    cols, err, _ = _run_single_hot(ops, device, np.zeros(0, dtype), np.zeros(F_ * B + 1, np.int32), F_, B,
                                   [7, 1000, BIG_N[dtype]], dtype)
    assert int(err[0]) == 0 and int(torch.stack(cols).abs().sum()) == 0


def _admit_case(rng, dtype, variant):
    F_, B = 3, 5000
    N = [7, 1000, BIG_N[dtype]]
    lengths = (rng.random(F_ * B) >= 0.1).astype(np.int32)
    lengths[B:2 * B] = 0  # the middle feature is entirely empty
    if variant == "empty":
        lengths[:] = 0
    if variant == "multi":
        lengths[2 * B + 123] = 3
    offsets = ref.complete_cumsum(lengths)
    values = np.concatenate([rng.integers(0, N[f], int(lengths[f * B:(f + 1) * B].sum()), dtype=np.int64)
                             for f in range(F_)])
    if variant == "bad":
        values[11] = -1
        values[offsets[2 * B] + 2500] = N[2] if dtype == np.int64 else -2 ** 31
        values[100] = N[0]
    return F_, B, N, values.astype(dtype), offsets


@pytest.mark.parametrize("W", [1, 3, 16])
@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("variant", ["clean", "multi", "bad", "empty"])
def test_kjt_admit(ops, device, W, dtype, variant):
    """Feature 0 table-wise (owner W - 1), features 1 (empty) and 2 row-wise (block = ceil(N / W));
    15 000 bags and ~9 000 values: several workgroups of each kind; out comes back bit-exact over
    the garbage it held."""
    rng = np.random.default_rng(W)
    F_, B, N, values, offsets = _admit_case(rng, dtype, variant)
    bs = [0, (N[1] + W - 1) // W, (N[2] + W - 1) // W]
    owners = [W - 1, 0, 0]
    want = ref.kjt_admit(values, offsets, F_, B, N, bs, owners, W)
    assert want[0] == (1 if variant == "multi" else 0) and want[1] == (2 if variant == "bad" else 0)
    assert int(want[2:].sum()) == values.size - (3 if variant == "bad" else 0)
    if variant in ("clean", "multi"):
        assert values.size > 2048 and F_ * B > 2048
        assert int(want[2 + (W - 1) * F_]) == int(offsets[B])  # the table-wise feature sits at its owner
    out = torch.full((2 + W * F_,), 0x5A5A5A5A, dtype=torch.int32, device=device)
    V = torch.from_numpy(values).to(device) if values.size else torch.empty(0, dtype=_tdt(dtype))
    got = ops.kjt_admit(V, torch.from_numpy(offsets).to(device), F_, B, N, bs, owners, W, out=out)
    torch.cuda.synchronize()
    ec.assert_ints_equal(got.cpu().numpy(), want, "admission counts")


def test_kjt_permute_int32_no_weights(ops, device):
    rng = np.random.default_rng(4)
    F_, B = 3, 700
    for perm in ([2, 0, 1], [1, 1, 0, 2]):
        lengths = rng.integers(0, 5, F_ * B).astype(np.int32)
        values = rng.integers(0, 10 ** 6, int(lengths.sum())).astype(np.int32)
        L = torch.from_numpy(lengths).to(device)
        ol, oo, ov, ow = ops.kjt_permute(L, ops.complete_cumsum(L), torch.from_numpy(values).to(device), F_, B, perm)
        rl, rv, _ = ref.kjt_permute(lengths, values, F_, B, perm)
        assert ow is None and ov.dtype == torch.int32
        ec.assert_ints_equal(ol.cpu().numpy(), rl)
        ec.assert_ints_equal(oo.cpu().numpy(), ref.complete_cumsum(rl))
        ec.assert_ints_equal(ov.cpu().numpy(), rv)


def test_kjt_permute_grid_stride(ops, device):
    """F_out * B = 560 000 bags > 2048 workgroups x 256 threads: the grid-stride loops take a second
    round (bags and values)."""
    rng = np.random.default_rng(5)
    F_, B, perm = 3, 140_000, [1, 1, 0, 2]
    assert len(perm) * B > 2048 * 256
    lengths = rng.integers(0, 3, F_ * B).astype(np.int32)
    values = rng.integers(0, 2 ** 31 - 1, int(lengths.sum())).astype(np.int32)
    L = torch.from_numpy(lengths).to(device)
    ol, oo, ov, _ = ops.kjt_permute(L, ops.complete_cumsum(L), torch.from_numpy(values).to(device), F_, B, perm)
    rl, rv, _ = ref.kjt_permute(lengths, values, F_, B, perm)
    assert rv.size > 2048 * 256
    ec.assert_ints_equal(ol.cpu().numpy(), rl)
    ec.assert_ints_equal(oo.cpu().numpy(), ref.complete_cumsum(rl))
    ec.assert_ints_equal(ov.cpu().numpy(), rv)


def _bucketize_case(rng, F_, B, N, maxlen, dtype):
    lengths = rng.integers(0, maxlen + 1, F_ * B).astype(np.int32)
    per = np.repeat(np.repeat(np.asarray(N, np.int64), B), lengths)
    values = (rng.random(per.size) * (per + 3)).astype(np.int64)  # ids in [0, N + 3): the id >= bs * W branch too
    return lengths, values.astype(dtype)


def test_block_bucketize_int32(ops, device):
    rng = np.random.default_rng(6)
    F_, B, W, N = 3, 700, 4, [100, 1000, 7]
    lengths, values = _bucketize_case(rng, F_, B, N, 5, np.int32)
    bs = [(n + W - 1) // W for n in N]
    L = torch.from_numpy(lengths).to(device)
    nl, no, nv = ops.block_bucketize(L, ops.complete_cumsum(L), torch.from_numpy(values).to(device), F_, B, bs, W)
    rl, rv = ref.block_bucketize(lengths, values, F_, B, bs, W)
    assert nv.dtype == torch.int32
    ec.assert_ints_equal(nl.cpu().numpy(), rl)
    ec.assert_ints_equal(no.cpu().numpy(), ref.complete_cumsum(rl))
    ec.assert_ints_equal(nv.cpu().numpy(), rv)


def test_block_bucketize_grid_stride(ops, device):
    """F * B = 1 060 000 bags > 4096 workgroups x 256 threads."""
    rng = np.random.default_rng(7)
    F_, B, W, N = 2, 530_000, 2, [1000, 77]
    assert F_ * B > 4096 * 256
    lengths, values = _bucketize_case(rng, F_, B, N, 2, np.int64)
    bs = [(n + W - 1) // W for n in N]
    L = torch.from_numpy(lengths).to(device)
    nl, no, nv = ops.block_bucketize(L, ops.complete_cumsum(L), torch.from_numpy(values).to(device), F_, B, bs, W)
    rl, rv = ref.block_bucketize_fast(lengths, values, F_, B, bs, W)
    ec.assert_ints_equal(nl.cpu().numpy(), rl)
    ec.assert_ints_equal(no.cpu().numpy(), ref.complete_cumsum(rl))
    ec.assert_ints_equal(nv.cpu().numpy(), rv)


# ---- 5. dense op options ----------------------------------------------------------------------------

SENT = -123.25  # what the cells outside a strided slice hold


@pytest.mark.parametrize("groups", [1, 2])
def test_linear_no_relu_no_bias_strided(ops, device, groups):
    """relu = 0, bias NULL, Y NULL in the backward calls; X a column slice of a wider buffer, Y and dX
    column slices of wider buffers whose other cells must not change."""
    M, N, K = 77, 64, 96
    g = torch.Generator().manual_seed(11 + groups)
    bigs = [torch.full((M, K + 40), SENT) for _ in range(groups)]
    for b in bigs:
        b[:, 16:16 + K] = torch.randn(M, K, generator=g)
    ws = [torch.randn(N, K, generator=g) / K ** 0.5 for _ in range(groups)]
    dys = [torch.randn(M, N, generator=g) for _ in range(groups)]
    bigd = [b.to(device) for b in bigs]
    xs = [b[:, 16:16 + K] for b in bigd]
    assert xs[0].stride(0) == K + 40
    wd = [w.to(device) for w in ws]
    ybig = [torch.full((M, N + 24), SENT, device=device) for _ in range(groups)]
    ys = ops.linear_fwd(xs, wd, [None] * groups, relu=False, outs=[y[:, 8:8 + N] for y in ybig])
    dxbig = [torch.full((M, K + 12), SENT, device=device) for _ in range(groups)]
    dxs = ops.linear_bwd_data([d.to(device) for d in dys], [None] * groups, wd, relu=False,
                              outs=[d[:, 4:4 + K] for d in dxbig])
    dws, dbs = ops.linear_bwd_weight([d.to(device) for d in dys], [None] * groups, xs, relu=False)
    torch.cuda.synchronize()
    for i in range(groups):
        x = bigs[i][:, 16:16 + K]
        _bf16_gemm_check(ys[i].cpu(), x, ws[i].T.contiguous())  # no bias, negative outputs kept
        assert bool((ys[i] < 0).any())
        _bf16_gemm_check(dxs[i].cpu(), dys[i], ws[i])
        _bf16_gemm_check(dws[i].cpu(), dys[i].T.contiguous(), x)
        np.testing.assert_allclose(dbs[i].cpu().numpy(), dys[i].sum(0).numpy(), rtol=1e-4, atol=1e-3)
        ec.assert_bitwise(bigd[i], bigs[i], "X buffer")  # read only
        for buf, lo, w in ((ybig[i], 8, N), (dxbig[i], 4, K)):
            outside = torch.ones_like(buf, dtype=torch.bool)
            outside[:, lo:lo + w] = False
            assert bool((buf[outside] == SENT).all()), "cells outside the strided output were written"


def _bce_inputs(B, dim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, dim, generator=g) - 0.3, torch.rand(B, dim, generator=g) - 0.3, g


def _bce_torch(q, c, y):
    qq, cc = q.clone().requires_grad_(True), c.clone().requires_grad_(True)
    logits = (qq * cc).sum(1)
    loss = torch.nn.BCEWithLogitsLoss()(logits, y.float())
    loss.backward()
    return logits.detach(), loss.detach(), qq.grad, cc.grad


@pytest.mark.parametrize("ldt", [torch.int32, torch.int64, torch.float32])
def test_dot_bce_grad_scale_and_forward_only(ops, device, ldt):
    B, dim = 1000, 33
    q, c, g = _bce_inputs(B, dim, 3)
    y = torch.rand(B, generator=g) if ldt == torch.float32 else torch.randint(0, 2, (B,), generator=g).to(ldt)
    logits, loss, gq, gc = _bce_torch(q, c, y)
    k = ops.DotBCE(device, B)
    dq, dc = torch.empty(B, dim, device=device), torch.empty(B, dim, device=device)
    lg, ls = k(q.to(device), c.to(device), y.to(device), dq=dq, dc=dc, grad_scale=3.0)
    lg, ls = lg.clone(), ls.clone()
    lg0, ls0 = k(q.to(device), c.to(device), y.to(device))  # forward only
    torch.cuda.synchronize()
    np.testing.assert_allclose(lg.cpu().numpy(), logits.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(float(ls), float(loss), rtol=1e-5)
    np.testing.assert_allclose(dq.cpu().numpy(), 3.0 * gq.numpy(), rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(dc.cpu().numpy(), 3.0 * gc.numpy(), rtol=1e-4, atol=1e-8)
    ec.assert_bitwise(lg0, lg, "forward-only logits")
    ec.assert_bitwise(ls0, ls, "forward-only loss")


def test_dot_bce_saturated_logits(ops, device):
    """Logits of +-60 with either label: the loss stays finite and equals torch's."""
    B, dim = 64, 8
    g = torch.Generator().manual_seed(9)
    c = torch.rand(B, dim, generator=g) + 0.5
    sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)
    q = c * (sign * 60.0 / (c * c).sum(1))[:, None]
    y = (torch.arange(B) % 4 < 2).to(torch.int32)  # every (sign, label) pair
    logits, loss, gq, gc = _bce_torch(q, c, y)
    assert float(logits.abs().min()) > 59.9 and torch.isfinite(loss)
    k = ops.DotBCE(device, B)
    dq, dc = torch.empty(B, dim, device=device), torch.empty(B, dim, device=device)
    lg, ls = k(q.to(device), c.to(device), y.to(device), dq=dq, dc=dc)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ls)) and bool(torch.isfinite(dq).all()) and bool(torch.isfinite(dc).all())
    np.testing.assert_allclose(lg.cpu().numpy(), logits.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(float(ls), float(loss), rtol=1e-5)
    np.testing.assert_allclose(dq.cpu().numpy(), gq.numpy(), rtol=1e-4, atol=1e-8)


ADAM = dict(lr=3e-3, beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=0.01)


class _TorchAdam:
    """torch.optim.Adam on the CPU with the options under test, fed explicit gradients."""

    def __init__(self, p0):
        self.p = torch.nn.Parameter(p0.clone())
        self.opt = torch.optim.Adam([self.p], lr=ADAM["lr"], betas=(ADAM["beta1"], ADAM["beta2"]), eps=ADAM["eps"],
                                    weight_decay=ADAM["weight_decay"])

    def step(self, grad):
        self.p.grad = grad.clone()
        self.opt.step()

    def check(self, got):
        np.testing.assert_allclose(got.cpu().numpy(), self.p.detach().numpy(), rtol=1e-5, atol=1e-6)


def test_adam_step_options(ops, device):
    g = torch.Generator().manual_seed(0)
    p = torch.randn(49536, generator=g)
    want = _TorchAdam(p)
    pd, md, vd = p.to(device), torch.zeros_like(p).to(device), torch.zeros_like(p).to(device)
    st = torch.zeros(2, dtype=torch.int64, device=device)
    for _ in range(3):
        grad = torch.randn(49536, generator=g)
        want.step(grad)
        ops.adam_step(pd, grad.to(device), md, vd, st, **ADAM)
    want.check(pd)
    assert int(st[0]) == 3 and int(st[1]) == 0


@pytest.mark.parametrize("form", ["update", "adam_grads", "pre"])
def test_tower_adam_options(ops, device, form):
    """Every Adam form of the fused towers ([64, 64] -> [128, 64], B = 200), 3 steps with lr, betas,
    eps and weight_decay off their defaults, against torch.optim.Adam fed the gradients the kernels
    report (grads_out) or were given (adam_grads)."""
    B, in_dims, widths = 200, [64, 64], [128, 64]
    g = torch.Generator().manual_seed(21)
    pooled = (torch.randn(B, 128, generator=g) * 0.5).to(device)
    labels = torch.randint(0, 2, (B,), generator=g).to(torch.int32).to(device)
    flat = _tower_params(in_dims, widths, g)
    want = _TorchAdam(flat)
    tw = ops.FusedTowers(in_dims, widths, [0, 64], B, device)
    P = flat.to(device)
    tw.update(P, do_adam=False)
    m, v = torch.zeros_like(P), torch.zeros_like(P)
    st = torch.zeros(2, dtype=torch.int64, device=device)
    gp, logits, loss = torch.zeros(B, 128, device=device), torch.empty(B, device=device), torch.empty((), device=device)
    grads = torch.zeros_like(P)
    a = ADAM
    for _ in range(3):
        if form == "adam_grads":
            grads = (torch.randn(flat.numel(), generator=g) * 0.01).to(device)
            tw.adam_grads(P, grads, m, v, st, **a)
        else:
            tw.fwd_bwd(pooled, gp, P, labels, logits)
            if form == "update":
                tw.wgrad(loss)
                tw.update(P, m, v, st, do_adam=True, grads_out=grads, **a)
            else:
                tw.wgrad_pre(loss, st, adam_lr=a["lr"], adam_beta1=a["beta1"], adam_beta2=a["beta2"])
                tw.update_pre(P, m, v, beta1=a["beta1"], beta2=a["beta2"], eps=a["eps"],
                              weight_decay=a["weight_decay"], grads_out=grads)
        torch.cuda.synchronize()
        assert float(grads.abs().max()) > 0
        want.step(grads.cpu())
    want.check(P)
    assert int(st[0]) == 3
