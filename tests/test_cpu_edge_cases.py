"""The edge-case tests' own tools, checked on the CPU: the oracle additions against their slow or
torch counterparts, the generators' stated properties, and a bite check per comparison routine (fed
a deliberately wrong expected value, it must raise)."""
import numpy as np
import pytest
import torch

import edge_cases as ec
from oracle import ref


@pytest.mark.parametrize("W", [2, 8])
@pytest.mark.parametrize("dtype", [np.int64, np.int32])
def test_block_bucketize_fast_equals_loop(W, dtype):
    rng = np.random.default_rng(W)
    F_, B = 3, 40
    N = [100, 1000, 7]
    lengths = rng.integers(0, 6, F_ * B).astype(np.int32)
    vals = []
    for i in range(F_ * B):
        vals.extend(rng.integers(0, N[i // B] + 3, lengths[i]).tolist())
    values = np.asarray(vals, dtype)
    bs = [(n + W - 1) // W for n in N]
    rl, rv = ref.block_bucketize(lengths, values, F_, B, bs, W)
    fl, fv = ref.block_bucketize_fast(lengths, values, F_, B, bs, W)
    np.testing.assert_array_equal(fl, rl)
    np.testing.assert_array_equal(fv, rv)
    assert fv.dtype == rv.dtype


def test_block_bucketize_fast_empty():
    fl, fv = ref.block_bucketize_fast(np.zeros(6, np.int32), np.zeros(0, np.int64), 2, 3, [4, 4], 2)
    assert fl.tolist() == [0] * 12 and fv.size == 0


def test_ref_adam_with_options_equals_torch():
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(777, generator=g)
    grads = [torch.randn(777, generator=g) for _ in range(3)]
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.01)
    for grad in grads:
        q.grad = grad.clone()
        opt.step()

    def restated(weight_decay):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for step, grad in enumerate(grads, 1):
            ref.adam([p], [grad], [m], [v], step, lr=3e-3, beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=weight_decay)
        return p

    np.testing.assert_allclose(restated(0.01).numpy(), q.detach().numpy(), rtol=1e-6, atol=1e-7)
    # the option matters at this size: without it the GPU tests' tolerance rejects the result
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(restated(0.0).numpy(), q.detach().numpy(), rtol=1e-5, atol=1e-6)


def test_ladder_histogram_and_thresholds():
    assert sum(ec.LADDER) == ec.LADDER_LOOKUPS == 7103 and ec.LADDER_B == 7168
    N = [1000, 1500]
    cols = ec.ladder_cols(N, seed=0)
    assert 2 * ec.LADDER_B > 8192  # HOT_WIN: the step's lookups exceed one window
    for t, (c, n) in enumerate(zip(cols, N)):
        assert c.numel() == ec.LADDER_B and int((c == 0).sum()) == ec.LADDER_B - ec.LADDER_LOOKUPS
        h = ec.ladder_histogram(c, n)
        rows = ec.ladder_rows(n, t)
        np.testing.assert_array_equal(h[rows], ec.LADDER)       # row k: exactly m_k lookups
        assert int((h > 0).sum()) == len(ec.LADDER) and h[0] > 0  # no other row; row 0 is looked up
        present = set(h[h > 0].tolist())
        for thr in ec.LADDER_THRESHOLDS:
            assert {thr - 1, thr, thr + 1} <= present, thr
        assert max(present) > 4096  # DD_HOT_CH: one row needs more than one chunk
        cn = c.numpy()
        assert (cn < 0).any() and (cn >= n).any()  # the floor-mod is needed
    assert not torch.equal(cols[0], ec.ladder_cols(N, seed=1)[0])
    assert torch.equal(cols[0], ec.ladder_cols(N, seed=0)[0])


def test_ladder_kjt_is_the_same_lookups():
    N, B = [1000, 1500], 2048
    cols = ec.ladder_cols(N, seed=0)
    values, lengths = ec.ladder_kjt(N, B, seed=0)
    offs = ref.complete_cumsum(lengths)
    assert lengths.size == 2 * B and values.size == 2 * ec.LADDER_LOOKUPS
    for t, n in enumerate(N):
        v = values[offs[t * B]:offs[(t + 1) * B]]
        np.testing.assert_array_equal(np.bincount(v, minlength=n), ec.ladder_histogram(cols[t], n))
        ln = lengths[t * B:(t + 1) * B]
        assert ln.max() == 40 and int((ln == 40).sum()) == 1 and (ln == 0).any()
        assert set(ln[ln != 40].tolist()) <= set(range(9))
        b40 = int(np.argmax(ln))
        bag = v[offs[t * B + b40] - offs[t * B]:offs[t * B + b40 + 1] - offs[t * B]]
        assert np.unique(bag).size == 1


@pytest.mark.parametrize("D", [128, 512, 10])
@pytest.mark.parametrize("dtype", [np.int64, np.int32])
@pytest.mark.parametrize("lone", [False, True])
def test_windowed_ids_stay_inside_the_allocation(D, dtype, lone):
    spec = ec.WindowSpec(R=200, D=D)
    wb = ec.windowed_batch(spec, seed=3, dtype=dtype, lone_row0=lone)
    B = wb.lengths.size // 2
    assert ec.window_in_allocation(spec, wb)
    ids = wb.values.astype(np.int64)
    oob = (ids < 0) | (ids >= spec.R)
    assert wb.n_oob == int(oob.sum()) > 0
    assert ((ids >= -spec.R) & (ids < 2 * spec.R)).all()
    np.testing.assert_array_equal(wb.clamped, np.where(oob, 0, ids))
    o = wb.offsets
    assert oob[o[0]:o[1]].all() and o[1] > o[0]                     # a bag entirely out of range
    b1 = ids[o[1]:o[2]]
    assert (b1 == 0).any() and ((b1 < 0) | (b1 >= spec.R)).any()    # row 0 beside out-of-range ids
    if lone:
        f1 = ids[o[B]:]
        assert int(((f1 < 0) | (f1 >= spec.R)).sum()) == 1 and not (f1 == 0).any()
    else:
        assert 0.08 < oob.mean() < 0.25
    # an id outside the window's reach would break the property (the check itself bites)
    bad = ec.WindowBatch(wb.lengths, wb.offsets, np.where(oob, 3 * spec.R, ids), wb.clamped, wb.n_oob, wb.maxlen)
    assert not ec.window_in_allocation(spec, bad)


# ---- bite checks ----------------------------------------------------------------------------------


def _ladder_expected(cols, N, D, drop=None):
    """fp64 oracle of one ladder step over tables of dim D, cast to fp32; ``drop`` = (table, row):
    one lookup of that row is left out."""
    g = torch.Generator().manual_seed(5)
    tabs = [torch.empty(n, D, dtype=torch.float64).uniform_(-0.03, 0.03, generator=g) for n in N]
    sts = [torch.zeros(n, dtype=torch.float64) for n in N]
    gout = torch.randn(ec.LADDER_B, 2 * D, generator=g)
    rows, grads = ec.cols_lookups(cols, N, gout, [D, D])
    if drop is not None:
        t, r = drop
        j = int(torch.nonzero(rows[t] == r)[0])
        keep = torch.arange(rows[t].numel()) != j
        rows[t], grads[t] = rows[t][keep], grads[t][keep]
    ec.adagrad_lookups_fp64(tabs, sts, rows, grads, 0.05, 1e-10)
    return [t.float() for t in tabs], [s.float() for s in sts]


@pytest.mark.parametrize("count", [4097, 31])
def test_bite_ladder_oracle_one_lookup_removed(count):
    N = [1000, 1500]
    cols = ec.ladder_cols(N, seed=0)
    w, s = _ladder_expected(cols, N, 64)
    for t in range(2):  # the routine accepts the right answer ...
        ec.assert_adagrad_close(w[t], s[t], w[t], s[t], w_rtol=1e-4, s_rtol=1e-4)
    row = int(ec.ladder_rows(N[1], 1)[ec.LADDER.index(count)])
    w2, s2 = _ladder_expected(cols, N, 64, drop=(1, row))
    with pytest.raises(AssertionError):  # ... and rejects the oracle with one lookup fewer: state
        np.testing.assert_allclose(s[1].numpy(), s2[1].numpy(), rtol=1e-4, atol=1e-9)
    with pytest.raises(AssertionError):  # and weights, at the ladder's own tolerances
        np.testing.assert_allclose(w[1].numpy(), w2[1].numpy(), rtol=1e-4, atol=1e-6)
    with pytest.raises(AssertionError):
        ec.assert_adagrad_close(w[1], s[1], w2[1], s2[1], w_rtol=1e-4, s_rtol=1e-4)


@pytest.mark.parametrize("pooling", ["sum", "mean"])
def test_bite_bounds_oracle_wrong_row(pooling):
    spec = ec.WindowSpec(R=200, D=128)
    wb = ec.windowed_batch(spec, seed=3)
    B = wb.lengths.size // 2
    g = torch.Generator().manual_seed(1)
    tabs = [torch.empty(spec.R, spec.D).uniform_(-0.07, 0.07, generator=g) for _ in range(2)]
    O = torch.from_numpy(wb.offsets)
    want = ref.pooled_fwd(tabs, [0, 1], torch.from_numpy(wb.clamped), O, B, pooling)
    ec.assert_pooled_close(want, want, wb.maxlen)
    ids = wb.values.astype(np.int64)
    j = int(np.nonzero((ids < 0) | (ids >= spec.R))[0][-1])
    wrong = wb.clamped.copy()
    wrong[j] = 1  # one out-of-range id mapped to row 1 instead of row 0
    bad = ref.pooled_fwd(tabs, [0, 1], torch.from_numpy(wrong), O, B, pooling)
    with pytest.raises(AssertionError):
        ec.assert_pooled_close(want, bad, wb.maxlen)


def test_bite_admit_restatement_count_moved():
    rng = np.random.default_rng(0)
    F_, B, W = 3, 500, 3
    N = [7, 1000, 50]
    values, offsets = ec.single_hot_kjt(rng, F_, B, N)
    bs = [3, 0, 17]
    want = ref.kjt_admit(values, offsets, F_, B, N, bs, [0, 2, 0], W)
    assert want[0] == 0 and want[1] == 0 and int(want[2:].sum()) == values.size
    assert int(want[2 + 2 * F_ + 1]) == int(offsets[2 * B] - offsets[B])  # table-wise feature: all at owner 2
    ec.assert_ints_equal(want, want)
    wrong = want.copy()
    wrong[2 + 0 * F_ + 0] -= 1
    wrong[2 + 1 * F_ + 0] += 1  # one id of feature 0 counted at the neighbouring owner
    with pytest.raises(AssertionError):
        ec.assert_ints_equal(want, wrong)


def test_kjt_restatements_flag_bad_batches():
    N = [7, 10]
    values = np.asarray([3, 0, 6, 9], np.int64)
    offsets = np.asarray([0, 1, 2, 2, 3, 4, 4], np.int32)  # F = 2, B = 3
    cols, err = ref.kjt_single_hot_cols(values, offsets, 2, 3, N)
    assert err == 0 and cols.tolist() == [[3, 7, 0], [6, 9, 0]]
    _, err = ref.kjt_single_hot_cols(np.asarray([3, 7, 6, -1], np.int64), offsets, 2, 3, N)
    assert err == 2
    cols, err = ref.kjt_single_hot_cols(values, np.asarray([0, 2, 2, 2, 3, 4, 4], np.int32), 2, 3, N)
    assert err == 1 and cols[0].tolist() == [0, 0, 0]
    out = ref.kjt_admit(np.asarray([3, 7, 6, -1], np.int64), offsets, 2, 3, N, [4, 0], [0, 1], 2)
    assert out.tolist() == [0, 2, 1, 0, 0, 1]  # the values 7 and -1 are counted nowhere


def test_bite_bitwise_one_ulp():
    a = torch.randn(200, generator=torch.Generator().manual_seed(0))
    ec.assert_bitwise(a, a.clone())
    b = a.clone()
    b.view(torch.int32)[17] += 1  # one ulp
    with pytest.raises(AssertionError):
        ec.assert_bitwise(a, b)
    ec.assert_bitwise(torch.tensor(0.5), torch.tensor(0.5))  # 0-d (a loss)
    with pytest.raises(AssertionError):
        ec.assert_bitwise(torch.tensor(0.5), torch.tensor(0.5000001))
    z = torch.zeros(4)
    with pytest.raises(AssertionError):  # the sign of zero is a bit too
        ec.assert_bitwise(z, -z)
    with pytest.raises(AssertionError):
        ec.assert_bitwise(a, a.double())
