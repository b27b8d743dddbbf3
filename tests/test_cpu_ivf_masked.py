"""The masked IVF entry points without a GPU: tt_ivf_mask_lists and tt_ivf_scan_masked are bound and
counted as the IVF entries are, every limit and NULL pointer comes back as a status code before any
launch, and IVFIndex.restricted refuses a wrong mask before any device work."""
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


def test_symbols_are_bound_and_counted(lib):
    from two_tower_recommender_model_amd import _lib

    for name in ("tt_ivf_mask_lists", "tt_ivf_scan_masked"):
        assert name in _lib.IVF_ENTRY_POINTS and name in _lib.SIGNATURES and hasattr(lib, name)
        assert name not in _lib.COMPUTE_ENTRY_POINTS
    assert lib.tt_num_entry_points() == len(_lib.COMPUTE_ENTRY_POINTS) == 55
    assert lib.tt_abi_version() == 4


def _scan(lib, M=8, E=64, P=1024, L=4, nprobe=2, k=10, q_dtype=F32, ldq=None, queries=FAKE, rows=FAKE, bias=None,
          labels=FAKE, list_begin=FAKE, list_len=FAKE, probes=FAKE, values=None, offsets=None, row_allow=FAKE,
          ids=FAKE, scores=FAKE, ws=FAKE, ws_bytes=1 << 40):
    rc = lib.tt_ivf_scan_masked(queries, q_dtype, E if ldq is None else ldq, M, E, rows, bias, labels, P, list_begin,
                                list_len, L, probes, nprobe, values, offsets, row_allow, k, ids, scores, ws, ws_bytes,
                                None)
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
    (dict(row_allow=None), "null row_allow"),
    (dict(values=FAKE), "excl_values"), (dict(offsets=FAKE), "excl_offsets"),
    (dict(rows=FAKE + 8), "16-byte"),
    (dict(ws_bytes=8 * 2 * 10 * 8), "ws_bytes"),
])
def test_scan_masked_limits_are_status_codes(lib, kw, word):
    rc, msg = _scan(lib, **kw)
    assert rc == 1001, (kw, rc)
    assert msg.startswith("tt_ivf_scan_masked:") and word in msg, (kw, msg)


def test_scan_masked_shares_the_workspace_query(lib):
    need = lib.tt_ivf_scan_workspace_bytes(100, 8, 10, 64)
    assert need > 0
    rc, msg = _scan(lib, M=100, nprobe=8, k=10, L=64, ws_bytes=need - 1)
    assert rc == 1001 and "ws_bytes" in msg


def test_unmasked_entry_still_names_itself(lib):
    """tt_ivf_scan shares its body with the masked entry; its messages stay its own."""
    rc = lib.tt_ivf_scan(FAKE, F32, 64, 8, 64, FAKE, None, FAKE, 1024, FAKE, FAKE, 4, FAKE, 2, None, None, 0, FAKE, FAKE,
                         FAKE, 1 << 40, None)
    assert rc == 1001 and lib.tt_last_error_string().decode().startswith("tt_ivf_scan: k must")


def _mask_lists(lib, allow=FAKE, N=1000, labels=FAKE, P=1024, list_begin=FAKE, list_len=FAKE, L=4, row_allow=FAKE,
                list_allow=FAKE, list_eligible=FAKE):
    rc = lib.tt_ivf_mask_lists(allow, N, labels, P, list_begin, list_len, L, row_allow, list_allow, list_eligible, None)
    return rc, lib.tt_last_error_string().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(N=0), "N must"), (dict(N=-1), "N must"), (dict(N=1 << 31), "N must"),
    (dict(P=0), "P must"), (dict(P=-1), "P must"), (dict(P=1 << 31), "P must"),
    (dict(L=0), "L must"), (dict(L=-1), "L must"), (dict(L=(1 << 20) + 1), "L must"),
    (dict(allow=None), "null"), (dict(labels=None), "null"), (dict(list_begin=None), "null"),
    (dict(list_len=None), "null"), (dict(row_allow=None), "null"), (dict(list_allow=None), "null"),
    (dict(list_eligible=None), "null"),
])
def test_mask_lists_limits_are_status_codes(lib, kw, word):
    rc, msg = _mask_lists(lib, **kw)
    assert rc == 1001, (kw, rc)
    assert msg.startswith("tt_ivf_mask_lists:") and word in msg, (kw, msg)


def _cpu_index():
    from two_tower_recommender_model_amd.ivf import IVFIndex

    g = torch.Generator().manual_seed(5)
    L, E, P = 3, 32, 384
    labels = torch.full((P,), -1, dtype=torch.int32)
    labels[0:5] = torch.arange(0, 5, dtype=torch.int32)
    labels[128:130] = torch.tensor([5, 6], dtype=torch.int32)
    return IVFIndex(centroids=torch.randn(L, E, generator=g), centroid_bias=torch.randn(L, generator=g),
                    rows=torch.randn(P, E, generator=g).to(torch.bfloat16), bias=None, labels=labels,
                    list_begin=torch.tensor([0, 128, 256], dtype=torch.int64),
                    list_len=torch.tensor([5, 2, 0], dtype=torch.int32), metric="dot", N=7)


@pytest.mark.parametrize("allow", [
    torch.ones(6, dtype=torch.bool), torch.ones(8, dtype=torch.bool), torch.ones(0, dtype=torch.bool),
    torch.ones(7), torch.ones(7, dtype=torch.float64), torch.ones(7, dtype=torch.int64),
    torch.ones(2, dtype=torch.int32), torch.ones(1, 7, dtype=torch.bool),
], ids=["short", "long", "empty", "float", "double", "int64", "two-words", "2d"])
def test_restricted_rejects_a_wrong_mask(allow):
    """ValueError, not the TTError a CPU tensor would meet in the wrappers: raised before them."""
    with pytest.raises(ValueError, match="allow"):
        _cpu_index().restricted(allow)


def test_restricted_has_no_cpu_fallback():
    from two_tower_recommender_model_amd import _lib

    with pytest.raises(_lib.TTError):
        _cpu_index().restricted(torch.ones(7, dtype=torch.bool))


def test_state_dict_of_a_restricted_view_raises():
    """The view is what restricted() returns (made by hand here: the mask kernel needs the GPU)."""
    idx = _cpu_index()
    assert idx.row_allow is None and idx.list_allow is None and idx.list_eligible is None and idx.eligible is None
    assert set(idx.state_dict()) == {*idx._TENSORS, "metric", "N"}
    view = type(idx)(*(getattr(idx, n) for n in idx._TENSORS), metric=idx.metric, N=idx.N)
    view.row_allow = torch.zeros(12, dtype=torch.int32)
    view.list_allow = torch.zeros(1, dtype=torch.int32)
    view.list_eligible = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="restricted"):
        view.state_dict()


def test_allow_beside_an_index_points_to_restricted():
    from two_tower_recommender_model_amd import lifecycle as lc

    with pytest.raises(ValueError, match="IVFIndex.restricted"):
        lc.retrieve(torch.zeros(4, 32), None, k=3, index=_cpu_index(), allow=torch.ones(7, dtype=torch.bool))
