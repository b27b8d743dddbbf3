"""The multiplicity ladder (tests/edge_cases.py) through every fused row-wise Adagrad path (``-m gpu``).

The update kernels change algorithm at fixed lookup counts per row (dedup.h DD_INL = 30 and
DD_HOT_CH = 4096; embedding.hip HOT_MIN = 33, HOT_NR_MAX = 64, HOT_SPLIT = 512, HOT_WIN = 8192; the
"<= 14 lookups: ascending order" rule). The ladder gives row k of each table EXACTLY m_k lookups with
m around each of those counts (test_cpu_edge_cases.py asserts the histogram), so every branch runs on
every path, and each path is compared with the oracle (oracle.ref.rowwise_adagrad_from_lookups)
computed in fp64 and cast — not merely with a second run of itself.

Tolerances are the project's (tests/test_gpu_dedup.py, test_gpu_ops.py::test_fused_adagrad_hot_rows):
weights rtol 1e-4 / atol 1e-6 (atol 1e-5 for D = 256), state rtol 1e-4 / atol 1e-9."""
import numpy as np
import pytest
import torch

import edge_cases as ec
from oracle import ref

pytestmark = pytest.mark.gpu

N = [1000, 1500]
LR, EPS, STEPS = 0.05, 1e-10, 2
KJT_B = 2048


@pytest.fixture(scope="module")
def ops():
    from two_tower_recommender_model_amd import ops as _ops

    return _ops


def _init_tables(D):
    g = torch.Generator().manual_seed(100 + D)
    return [torch.empty(n, D).uniform_(-(1.0 / n) ** 0.5, (1.0 / n) ** 0.5, generator=g) for n in N]


def _gout(B, D, step):
    return torch.randn(B, 2 * D, generator=torch.Generator().manual_seed(50 + step))


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _oracle_cols(D):
    def make():
        cols = ec.ladder_cols(N, seed=0)
        tabs = [t.double() for t in _init_tables(D)]
        sts = [torch.zeros(n, dtype=torch.float64) for n in N]
        for step in range(STEPS):
            rows, grads = ec.cols_lookups(cols, N, _gout(ec.LADDER_B, D, step), [D, D])
            ec.adagrad_lookups_fp64(tabs, sts, rows, grads, LR, EPS)
        return [t.float() for t in tabs], [s.float() for s in sts]

    return _cached(("oracle-cols", D), make)


def _oracle_kjt(D, pooling):
    def make():
        values, lengths = ec.ladder_kjt(N, KJT_B, seed=0)
        tabs = [t.double() for t in _init_tables(D)]
        sts = [torch.zeros(n, dtype=torch.float64) for n in N]
        for step in range(STEPS):
            rows, grads = ec.kjt_lookups(values, lengths, KJT_B, _gout(KJT_B, D, step), [D, D], pooling == "mean")
            ec.adagrad_lookups_fp64(tabs, sts, rows, grads, LR, EPS)
        return [t.float() for t in tabs], [s.float() for s in sts]

    return _cached(("oracle-kjt", D, pooling), make)


def _table_set(ops, device, D):
    ts = ops.TableSet(N, [D, D], [0, 1], device)
    for t, w in enumerate(_init_tables(D)):
        ts.table_view(t).copy_(w)
    return ts


def _run_cols(ops, device, path, D):
    """Two steps of the ladder's columns through ``path`` on fresh tables -> (weights, state), CPU."""
    cols = [c.to(device) for c in ec.ladder_cols(N, seed=0)]
    ts = _table_set(ops, device, D)
    for step in range(STEPS):
        gout = _gout(ec.LADDER_B, D, step).to(device)
        if path == "dedup":
            ts.dedup_insert_cols(cols, N)
            ts.dedup_rowwise_adagrad(gout, ec.LADDER_B, LR, EPS)
        else:
            ts.bwd_prepare_cols(cols, N)
            ts.bwd_rowwise_adagrad(gout, None, ec.LADDER_B, LR, EPS)
    torch.cuda.synchronize()
    if path == "dedup":
        ec.assert_clean(ts)
    return [ts.table_view(t).cpu().clone() for t in range(2)], [ts.state_view(t).cpu().clone() for t in range(2)]


def _check(got, want, D):
    (gw, gs), (ww, ws) = got, want
    for t in range(2):
        ec.assert_adagrad_close(gw[t].numpy(), gs[t].numpy(), ww[t].numpy(), ws[t].numpy(), w_rtol=1e-4,
                                w_atol=1e-5 if D == 256 else 1e-6, s_rtol=1e-4, s_atol=1e-9)
        # every ladder row moved, nothing else did
        hist = ec.ladder_histogram(ec.ladder_cols(N, seed=0)[t], N[t])
        moved = (gs[t] != 0).numpy()
        np.testing.assert_array_equal(moved, hist > 0)


@pytest.mark.parametrize("D", [64, 128])
def test_ladder_dedup_path_vs_oracle(ops, device, D):
    """tt_dedup_insert_cols + tt_dedup_rowwise_adagrad; a second identical run is bitwise equal and
    the workspace is clean after each."""
    first = _cached(("dedup", D), lambda: _run_cols(ops, device, "dedup", D))
    _check(first, _oracle_cols(D), D)
    again = _run_cols(ops, device, "dedup", D)
    for a, b in zip(first[0] + first[1], again[0] + again[1]):
        ec.assert_bitwise(a, b, "second run")


@pytest.mark.parametrize("D", [64, 128, 256])
def test_ladder_cols_path_vs_oracle(ops, device, D):
    """tt_bwd_prepare_cols + tt_bwd_rowwise_adagrad (narrow kernels for D <= 128, generic for 256)."""
    first = _cached(("cols", D), lambda: _run_cols(ops, device, "cols", D))
    _check(first, _oracle_cols(D), D)
    again = _run_cols(ops, device, "cols", D)
    for a, b in zip(first[0] + first[1], again[0] + again[1]):
        ec.assert_bitwise(a, b, "second run")


@pytest.mark.parametrize("D", [64, 128])
def test_ladder_rows_up_to_14_lookups_bitwise_between_paths(ops, device, D):
    """Rows of <= 14 lookups are summed in ascending lookup order by both the dedup path and the
    column form of the KJT path: bitwise equal (the hotter rows of the same step beside them)."""
    a = _cached(("dedup", D), lambda: _run_cols(ops, device, "dedup", D))
    b = _cached(("cols", D), lambda: _run_cols(ops, device, "cols", D))
    cols = ec.ladder_cols(N, seed=0)
    for t in range(2):
        hist = ec.ladder_histogram(cols[t], N[t])
        cool = torch.from_numpy(hist <= 14)
        assert int((hist[hist > 0] <= 14).sum()) == 5 and int((hist > 14).sum()) == 16
        ec.assert_bitwise(a[0][t][cool], b[0][t][cool], f"table {t} rows of <= 14 lookups")
        ec.assert_bitwise(a[1][t][cool], b[1][t][cool], f"table {t} state of rows of <= 14 lookups")


def _run_kjt(ops, device, D, pooling, parts):
    values, lengths = ec.ladder_kjt(N, KJT_B, seed=0)
    V = torch.from_numpy(values).to(device)
    O = torch.from_numpy(ref.complete_cumsum(lengths)).to(device)
    ts = _table_set(ops, device, D)
    for step in range(STEPS):
        gout = _gout(KJT_B, D, step).to(device)
        ts.bwd_prepare(V, O, KJT_B, values.size)
        for p in parts:
            ts.bwd_rowwise_adagrad(gout, O, KJT_B, LR, EPS, pooling=1 if pooling == "mean" else 0, part=p)
    torch.cuda.synchronize()
    return [ts.table_view(t).cpu().clone() for t in range(2)], [ts.state_view(t).cpu().clone() for t in range(2)]


@pytest.mark.parametrize("D,parts", [(64, (0,)), (64, (1, 2)), (128, (0,)), (128, (1, 2)), (256, (0,))],
                         ids=["d64", "d64-parts", "d128", "d128-parts", "d256"])
@pytest.mark.parametrize("pooling", ["sum", "mean"])
def test_ladder_kjt_path_vs_oracle(ops, device, D, parts, pooling):
    """tt_bwd_prepare + tt_bwd_rowwise_adagrad on the same lookups as multi-hot bags of 1..8 ids (one
    bag holds one id 40 times: the repeated-bag-id pass), SUM and MEAN, as one launch and as parts
    1 + 2."""
    first = _run_kjt(ops, device, D, pooling, parts)
    _check(first, _oracle_kjt(D, pooling), D)
    again = _run_kjt(ops, device, D, pooling, parts)
    for a, b in zip(first[0] + first[1], again[0] + again[1]):
        ec.assert_bitwise(a, b, "second run")
