"""The IVF entry points without a GPU: every limit of tt_ivf_scan and tt_ivf_segment_mean comes back
as a status code before any launch, the workspace query, the Python layer's refusals (allow with an
index, a metric other than the index's) and the state_dict round trip on CPU tensors."""
import pytest
import torch

FAKE = 1 << 20  # never dereferenced: every call here must return before any launch
F32, BF16 = 2, 3


@pytest.fixture(scope="module")
def lib():
    from two_tower_recommender_model_amd import _lib
    from two_tower_recommender_model_amd.build import build

    build()
    return _lib.load()


def _scan(lib, M=8, E=64, P=1024, L=4, nprobe=2, k=10, q_dtype=F32, ldq=None, queries=FAKE, rows=FAKE, bias=None,
          labels=FAKE, list_begin=FAKE, list_len=FAKE, probes=FAKE, values=None, offsets=None, ids=FAKE, scores=FAKE,
          ws=FAKE, ws_bytes=1 << 40):
    rc = lib.tt_ivf_scan(queries, q_dtype, E if ldq is None else ldq, M, E, rows, bias, labels, P, list_begin, list_len,
                         L, probes, nprobe, values, offsets, k, ids, scores, ws, ws_bytes, None)
    return rc, lib.tt_last_error_string().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(E=0), "E must"), (dict(E=16), "E must"), (dict(E=48), "E must"), (dict(E=160), "E must"), (dict(E=-32), "E must"),
    (dict(k=0), "k must"), (dict(k=257), "k must"), (dict(k=-1), "k must"),
    (dict(nprobe=0), "nprobe must"), (dict(nprobe=65), "nprobe must"), (dict(nprobe=-1), "nprobe must"),
    (dict(L=0), "L must"), (dict(L=(1 << 20) + 1), "L must"), (dict(L=-1), "L must"),
    (dict(M=0), "M must"), (dict(M=-5), "M must"),
    (dict(M=1 << 25, nprobe=64), "M * nprobe"), (dict(M=1 << 31, nprobe=1), "M * nprobe"),
    (dict(P=0), "P must"), (dict(P=1 << 31), "P must"), (dict(P=-1), "P must"),
    (dict(q_dtype=0), "q_dtype"), (dict(ldq=63), "ldq"),
    (dict(queries=None), "null"), (dict(rows=None), "null"), (dict(labels=None), "null"),
    (dict(list_begin=None), "null"), (dict(list_len=None), "null"), (dict(probes=None), "null"),
    (dict(ids=None), "null"), (dict(scores=None), "null"), (dict(ws=None), "null"),
    (dict(values=FAKE), "excl_values"), (dict(offsets=FAKE), "excl_offsets"),
    (dict(rows=FAKE + 8), "16-byte"),
    (dict(ws_bytes=8 * 2 * 10 * 8), "ws_bytes"),
])
def test_scan_limits_are_status_codes(lib, kw, word):
    rc, msg = _scan(lib, **kw)
    assert rc == 1001, (kw, rc)
    assert msg.startswith("tt_ivf_scan:") and word in msg, (kw, msg)


def _mean(lib, dtype=F32, ld=None, n=100, E=64, L=4, rows=FAKE, order=FAKE, seg=FAKE, out=FAKE):
    rc = lib.tt_ivf_segment_mean(rows, dtype, E if ld is None else ld, n, E, order, seg, L, out, None)
    return rc, lib.tt_last_error_string().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(dtype=0), "dtype"), (dict(dtype=1), "dtype"),
    (dict(E=0), "E must"), (dict(E=4097), "E must"), (dict(ld=63), "ld must"),
    (dict(n=0), "n must"), (dict(n=-1), "n must"),
    (dict(L=0), "L must"), (dict(L=(1 << 20) + 1), "L must"),
    (dict(rows=None), "null"), (dict(order=None), "null"), (dict(seg=None), "null"), (dict(out=None), "null"),
])
def test_segment_mean_limits_are_status_codes(lib, kw, word):
    rc, msg = _mean(lib, **kw)
    assert rc == 1001, (kw, rc)
    assert msg.startswith("tt_ivf_segment_mean:") and word in msg, (kw, msg)


def test_workspace_bytes(lib):
    f = lib.tt_ivf_scan_workspace_bytes
    base = f(100, 8, 10, 64)
    # the partial lists and the two per-pair tables at least
    assert base >= 100 * 8 * 10 * 8 + 2 * 100 * 8 * 4
    for bad in [(0, 8, 10, 64), (-1, 8, 10, 64), (100, 0, 10, 64), (100, 65, 10, 64), (100, 8, 0, 64),
                (100, 8, 257, 64), (100, 8, 10, 0), (100, 8, 10, (1 << 20) + 1), (1 << 25, 64, 10, 64)]:
        assert f(*bad) == 0, bad
    # monotone in M, nprobe and k (and never smaller for more lists)
    prev = 0
    for M in (1, 2, 100, 101, 4096, 1 << 20):
        assert f(M, 8, 10, 64) > prev
        prev = f(M, 8, 10, 64)
    prev = 0
    for nprobe in range(1, 65):
        assert f(100, nprobe, 10, 64) > prev
        prev = f(100, nprobe, 10, 64)
    prev = 0
    for k in (1, 2, 10, 100, 255, 256):
        assert f(100, 8, k, 64) > prev
        prev = f(100, 8, k, 64)
    assert f(100, 8, 10, 1 << 20) > f(100, 8, 10, 64)
    # what the call accepts is what the query reports
    assert _scan(lib, M=100, nprobe=8, k=10, L=64, ws_bytes=base - 1)[0] == 1001


def test_symbols_are_bound(lib):
    from two_tower_recommender_model_amd import _lib

    for name in _lib.IVF_ENTRY_POINTS + ["tt_ivf_scan_workspace_bytes"]:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.tt_abi_version() == 4


def _cpu_index(metric="dot"):
    from two_tower_recommender_model_amd.ivf import IVFIndex

    g = torch.Generator().manual_seed(5)
    L, E, P = 3, 32, 384
    labels = torch.full((P,), -1, dtype=torch.int32)
    labels[0:5] = torch.arange(0, 5, dtype=torch.int32)
    labels[128:130] = torch.tensor([5, 6], dtype=torch.int32)
    return IVFIndex(centroids=torch.randn(L, E, generator=g), centroid_bias=torch.randn(L, generator=g),
                    rows=torch.randn(P, E, generator=g).to(torch.bfloat16),
                    bias=torch.randn(P, generator=g) if metric == "l2" else None, labels=labels,
                    list_begin=torch.tensor([0, 128, 256], dtype=torch.int64),
                    list_len=torch.tensor([5, 2, 0], dtype=torch.int32), metric=metric, N=7)


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_state_dict_round_trip(metric, tmp_path):
    from two_tower_recommender_model_amd.ivf import IVFIndex

    idx = _cpu_index(metric)
    sd = idx.state_dict()
    assert set(sd) == {"centroids", "centroid_bias", "rows", "bias", "labels", "list_begin", "list_len", "metric", "N"}
    torch.save(sd, tmp_path / "index.pt")
    back = IVFIndex.from_state_dict(torch.load(tmp_path / "index.pt"))
    assert back.metric == metric and back.N == 7 and back.nlist == 3
    for n in IVFIndex._TENSORS:
        a, b = getattr(idx, n), getattr(back, n)
        if a is None:
            assert b is None
        else:
            assert a.dtype == b.dtype and torch.equal(a, b), n
    with pytest.raises(ValueError):
        IVFIndex.from_state_dict({**sd, "metric": "cosine"})


def test_allow_with_an_index_raises():
    from two_tower_recommender_model_amd import lifecycle as lc

    idx = _cpu_index("dot")
    q = torch.zeros(4, 32)
    with pytest.raises(ValueError, match="allow"):
        lc.retrieve(q, None, k=3, index=idx, allow=torch.ones(7, dtype=torch.bool))


def test_metric_mismatch_raises():
    from two_tower_recommender_model_amd import lifecycle as lc

    q = torch.zeros(4, 32)
    with pytest.raises(ValueError, match="metric"):
        lc.retrieve(q, None, k=3, metric="l2", index=_cpu_index("dot"))
    with pytest.raises(ValueError, match="metric"):
        lc.retrieve(q, None, k=3, metric="dot", index=_cpu_index("l2"))


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_mixture_case_has_recall_one_by_construction(metric):
    """What the GPU end-to-end case relies on, in float64 on the bf16-rounded rows: every query's
    exact top 10 lies in its own cluster, with a margin far beyond the fp32 score error."""
    import ivf_cases as ic

    items, cluster, queries, qcluster, init = ic.mixture()
    assert cluster[init].tolist() == list(range(ic.MIX_C))
    q, c = queries.to(torch.bfloat16).double(), items.to(torch.bfloat16).double()
    s = q @ c.T - (0.5 * (c * c).sum(1) if metric == "l2" else 0.0)
    own = cluster.unsqueeze(0) == qcluster.unsqueeze(1)
    assert (own.sum(1) == ic.MIX_PER).all()
    worst_own = torch.where(own, s, torch.full_like(s, float("inf"))).min(1).values
    best_other = torch.where(~own, s, torch.full_like(s, float("-inf"))).max(1).values
    assert float((worst_own - best_other).min()) > 10.0


def test_exclusion_helper_hand_worked():
    import ivf_cases as ic

    assign = torch.tensor([0, 1, 1, 2, 0, 2])
    probes = torch.tensor([[1, -1], [0, 2], [7, 3]], dtype=torch.int32)
    elig = ic.eligibility_for_probes(assign, probes, 3)
    assert elig.tolist() == [[False, True, True, False, False, False], [True, False, False, True, True, True],
                             [False] * 6]
    xv, xo = ic.exclusion_from_eligibility(elig, seen=[[2, 9], [], [1]])
    assert xo.tolist() == [0, 5, 7, 13] and xv.tolist() == [0, 2, 3, 4, 5, 1, 2, 0, 1, 2, 3, 4, 5]
    assert ic.eligibility_for_probes(assign, probes, 3, dead_lists=(2,))[1].tolist() == [True, False, False, False, True, False]


def test_no_cpu_fallback():
    """A CPU tensor is refused by the wrappers: there is no eager path behind them."""
    from two_tower_recommender_model_amd import _lib, ops

    idx = _cpu_index("dot")
    with pytest.raises(_lib.TTError):
        idx.search(torch.zeros(4, 32), 3, 2)
    with pytest.raises(_lib.TTError):
        ops.ivf_segment_mean(torch.zeros(4, 32), torch.arange(4), torch.tensor([0, 4]), torch.zeros(1, 32))
