"""tt_topk_mips_large without a GPU: its declared limits come back as status codes before any launch,
the workspace query and its bound, the bindings (the new symbols beside, not among, the counted
entry points; the pinned constants unchanged), and lifecycle's refusal of k > 256 with an index."""
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


def _call(lib, M=8, N=100, E=64, k=300, splits=0, q_dtype=F32, c_dtype=F32, ldq=None, ldc=None, queries=FAKE,
          items=FAKE, ids=FAKE, scores=FAKE, ws=FAKE, ws_bytes=None, allow=None, xv=None, xo=None):
    if ws_bytes is None:
        ws_bytes = 1 << 50
    rc = lib.tt_topk_mips_large(queries, q_dtype, E if ldq is None else ldq, items, c_dtype, E if ldc is None else ldc,
                                None, M, N, E, k, splits, allow, xv, xo, ids, scores, ws, ws_bytes, None)
    return rc, lib.tt_last_error_string().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(E=0), "E must"), (dict(E=16), "E must"), (dict(E=48), "E must"), (dict(E=160), "E must"),
    (dict(k=0), "k must"), (dict(k=-1), "k must"), (dict(k=8193), "k must"),
    (dict(M=0), "M must"), (dict(M=-5), "M must"), (dict(M=(1 << 30) + 1), "M must"),
    (dict(N=0), "N must"), (dict(N=1 << 31), "N must"), (dict(N=-1), "N must"),
    (dict(splits=-1), "splits must"), (dict(splits=65), "splits must"),
    (dict(q_dtype=0), "q_dtype"), (dict(c_dtype=1), "c_dtype"),
    (dict(ldq=63), "ldq"), (dict(ldc=32), "ldc"),
    (dict(queries=None), "null"), (dict(items=None), "null"), (dict(ids=None), "null"), (dict(scores=None), "null"),
    (dict(ws=None), "null"),
    (dict(xv=FAKE), "excl_values"), (dict(xo=FAKE), "excl_values"),
    (dict(ws_bytes=3 * 8 * (2 * 300 + 32) * 8 - 1, splits=3), "ws_bytes"),
])
def test_limits_are_status_codes(lib, kw, word):
    rc, msg = _call(lib, **kw)
    assert rc == 1001, (kw, rc)
    assert msg.startswith("tt_topk_mips_large") and word in msg, (kw, msg)


def test_workspace_query(lib):
    ws = lib.tt_topk_mips_large_workspace_bytes
    assert ws(8, 100000, 257, 0) > 0 and ws(8, 100000, 8192, 0) > 0
    # the header's formula, under the bound S * M * (2 k + 64) keys, and independent of N at fixed S
    for S, M, k in [(1, 1, 1), (2, 40, 257), (7, 40, 1000), (64, 4096, 8192), (3, 129, 5000), (1, 1 << 16, 8192)]:
        got = ws(M, 100000, k, S)
        assert got == S * M * (2 * k + 32) * 8
        assert 0 < got <= S * M * (2 * k + 64) * 8
        assert ws(M, 10 ** 8, k, S) == got
    # splits = 0: between 1 and 64 pools per query; a split holds several times k items, so a small
    # catalogue is one split however few the queries
    per = (2 * 1000 + 32) * 8
    auto = ws(16, 1 << 22, 1000, 0)
    assert auto % (16 * per) == 0 and 1 < auto // (16 * per) <= 64
    assert ws(16, 3000, 1000, 0) == 16 * per
    assert ws(1 << 16, 1 << 22, 1000, 0) == (1 << 16) * per
    for bad in [(0, 100, 300, 1), ((1 << 30) + 1, 100, 300, 1), (8, 0, 300, 1), (8, 1 << 31, 300, 1), (8, 100, 0, 1),
                (8, 100, -1, 1), (8, 100, 8193, 1), (8, 100, 300, 65), (8, 100, 300, -1)]:
        assert ws(*bad) == 0, bad


def test_bindings_and_pinned_constants(lib):
    from two_tower_recommender_model_amd import _lib

    assert _lib.TT_TOPK_LARGE_MAX_K == 8192
    assert _lib.TT_TOPK_MAX_K == 256
    assert lib.tt_abi_version() == 4
    for name in ("tt_topk_mips_large", "tt_topk_mips_large_workspace_bytes"):
        assert name in _lib.SIGNATURES and name in _lib.TOPK_LARGE_ENTRY_POINTS
        assert name not in _lib.COMPUTE_ENTRY_POINTS and name not in _lib.IVF_ENTRY_POINTS
        assert getattr(lib, name).argtypes is not None
    assert lib.tt_num_entry_points() == 55 == len(_lib.COMPUTE_ENTRY_POINTS)


def test_the_small_k_entry_points_keep_their_limit(lib):
    rc = lib.tt_topk_mips(FAKE, F32, 64, FAKE, F32, 64, None, 8, 100, 64, 257, 0, FAKE, FAKE, FAKE, 1 << 40, None)
    assert rc == 1001 and "TT_TOPK_MAX_K = 256" in lib.tt_last_error_string().decode()
    assert lib.tt_topk_mips_workspace_bytes(8, 100, 257, 1) == 0


def test_index_with_large_k_is_refused(lib):
    """IVF at k > 256 is out of scope: a ValueError that names the list scan's limit, before any
    device work (the index here is CPU dummies that no kernel could read)."""
    from two_tower_recommender_model_amd import lifecycle as lc
    from two_tower_recommender_model_amd.ivf import IVFIndex

    z = torch.zeros(4, 64)
    index = IVFIndex(z, torch.zeros(4), z.to(torch.bfloat16), torch.zeros(4), torch.zeros(4, dtype=torch.int32),
                     torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.int32), "dot", 4)
    with pytest.raises(ValueError, match="256"):
        lc.retrieve(torch.zeros(3, 64), z, k=300, index=index)
    with pytest.raises(ValueError, match="256"):
        lc.retrieve_fused(None, torch.zeros(3, dtype=torch.int64), k=300, index=index)


def test_lifecycle_bounds_the_large_k_workspace(lib):
    from two_tower_recommender_model_amd import lifecycle as lc, ops

    N = 1 << 22
    for M, k, chunk in [(1 << 16, 8192, 1 << 16), (1 << 16, 5000, 1 << 16), (4096, 8192, 1 << 16), (300, 1000, 64),
                        (1 << 20, 257, 1 << 16), (100, 8192, 1 << 16)]:
        n, S = lc._large_k_plan(M, N, k, chunk)
        assert 1 <= n <= min(M, chunk)
        assert 0 < ops.topk_mips_large_workspace_bytes(n, N, k, S) <= lc.LARGE_K_WORKSPACE_BYTES, (M, k, n, S)
    # the default chunk at k = 8192 would be 8.6 GB with one split alone
    assert lib.tt_topk_mips_large_workspace_bytes(1 << 16, N, 8192, 1) > 8 * 10 ** 9
    assert lc._large_k_plan(1 << 16, N, 8192, 1 << 16)[0] < 1 << 16
