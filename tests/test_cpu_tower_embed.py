"""tt_tower_embed without a GPU: the bindings (beside, not among, the counted entry points), every
declared limit as a status code before any launch, the shape predicate, and the Python layers' refusals
that need no device."""
import ctypes as C

import pytest
import torch

FAKE = 1 << 20  # never dereferenced: every call here must return before any launch
I32, I64, F32, BF16 = 0, 1, 2, 3
NAMES = ("tt_tower_embed_supported", "tt_tower_embed")


@pytest.fixture(scope="module")
def lib():
    from two_tower_recommender_model_amd import _lib
    from two_tower_recommender_model_amd.build import build

    build()
    return _lib.load()


def test_bindings_and_pinned_constants(lib):
    from two_tower_recommender_model_amd import _lib

    for name in NAMES:
        assert name in _lib.SIGNATURES and name in _lib.EMBED_ENTRY_POINTS
        assert name not in _lib.COMPUTE_ENTRY_POINTS and name not in _lib.RANK_ENTRY_POINTS
        assert getattr(lib, name).argtypes is not None
    assert sorted(_lib.EMBED_ENTRY_POINTS) == sorted(NAMES)
    assert lib.tt_num_entry_points() == 55 == len(_lib.COMPUTE_ENTRY_POINTS)
    assert lib.tt_abi_version() == 4


def _widths(ws):
    return (C.c_int32 * max(len(ws), 1))(*ws)


def _ptrs(ps):
    arr = (C.c_void_p * max(len(ps), 1))()
    for i, p in enumerate(ps):
        arr[i] = p
    return arr


_UNSET = object()


def _call(lib, in_dim=64, widths=(128, 64), L=None, table=FAKE, ld=None, num_rows=1000, rows=None, row_dtype=I64,
          first_row=0, M=100, W=_UNSET, bias=None, out=FAKE, out_dtype=F32, ldo=None, widths_ptr=_UNSET):
    L = len(widths) if L is None else L
    n = max(L, len(widths))
    if W is _UNSET:
        W = [FAKE] * n
    wp = _widths(list(widths) + [0] * (n - len(widths))) if widths_ptr is _UNSET else widths_ptr
    rc = lib.tt_tower_embed(table, in_dim if ld is None else ld, num_rows, in_dim, rows, row_dtype, first_row, M, L, wp,
                            None if W is None else _ptrs(W), None if bias is None else _ptrs(bias), out, out_dtype,
                            (widths[-1] if widths else 64) if ldo is None else ldo, None, None)
    return rc, lib.tt_last_error_string().decode()


@pytest.mark.parametrize("kw", [
    dict(in_dim=48), dict(in_dim=160), dict(in_dim=0), dict(widths=(128, 16)), dict(widths=(160, 64)),
    dict(widths=(48,)),
    dict(L=0, widths=()), dict(L=5, widths=(64, 64, 64, 64, 64)),
    dict(ld=32), dict(ld=66), dict(table=FAKE + 4), dict(ldo=32), dict(ldo=66), dict(out=FAKE + 8),
    dict(out_dtype=BF16, ldo=68),  # bf16 rows of 136 B are not 16-B aligned
    dict(out_dtype=I32), dict(out_dtype=7), dict(rows=FAKE, row_dtype=F32), dict(rows=FAKE, row_dtype=-1),
    dict(first_row=901), dict(first_row=0, M=1001), dict(first_row=-1), dict(first_row=1 << 62, M=1 << 62),
    dict(rows=FAKE, first_row=1),
    dict(W=[FAKE, None]), dict(W=None), dict(table=None), dict(out=None), dict(widths_ptr=None),
    dict(M=-1), dict(num_rows=0, M=0),
])
def test_limits_are_status_codes(lib, kw):
    rc, msg = _call(lib, **kw)
    assert rc == 1001, (kw, rc)
    assert msg.startswith("tt_tower_embed"), (kw, msg)


def test_empty_call_is_ok_without_a_launch(lib):
    assert _call(lib, M=0)[0] == 0
    assert _call(lib, M=0, rows=FAKE, row_dtype=I32, out_dtype=BF16, bias=[None, FAKE])[0] == 0
    assert _call(lib, M=0, first_row=1000)[0] == 0  # the empty range at the table's end
    assert _call(lib, M=0, in_dim=128, widths=(128, 128, 128, 128))[0] == (
        0 if lib.tt_tower_embed_supported(128, 4, _widths([128] * 4)) else 1001)


def test_supported_predicate(lib):
    sup = lib.tt_tower_embed_supported
    for in_dim, ws in [(64, [128, 64]), (128, [128, 64]), (32, [32]), (128, [128, 128, 128])]:
        assert sup(in_dim, len(ws), _widths(ws)) == 1, (in_dim, ws)
    # every in-range shape with L <= 3
    dims = (32, 64, 96, 128)
    for in_dim in dims:
        for a in dims:
            assert sup(in_dim, 1, _widths([a])) == 1
            for b in dims:
                assert sup(in_dim, 2, _widths([a, b])) == 1
                for c in dims:
                    assert sup(in_dim, 3, _widths([a, b, c])) == 1
    assert sup(64, 4, _widths([32, 32, 32, 32])) == 1
    for in_dim, ws, L in [(48, [64], 1), (160, [64], 1), (0, [64], 1), (64, [16], 1), (64, [128, 160], 2), (64, [64, 40], 2),
                          (64, [], 0), (64, [64] * 5, 5), (-32, [64], 1)]:
        assert sup(in_dim, L, _widths(ws)) == 0, (in_dim, ws)
    assert sup(64, 2, None) == 0


def test_python_predicate_asks_the_library(lib):
    from two_tower_recommender_model_amd import ops

    assert ops.tower_embed_supported(64, [128, 64]) is True
    assert ops.tower_embed_supported(128, [128, 128, 128]) is True
    assert ops.tower_embed_supported(48, [64]) is False
    assert ops.tower_embed_supported(64, []) is False
    assert ops.tower_embed_supported(128, [128] * 4) == bool(lib.tt_tower_embed_supported(128, 4, _widths([128] * 4)))


def test_tower_embed_has_no_cpu_fallback(lib):
    from two_tower_recommender_model_amd import _lib, ops

    table = torch.zeros(10, 64)
    layers = [(torch.zeros(128, 64), torch.zeros(128)), (torch.zeros(64, 128), None)]
    with pytest.raises(_lib.TTError):
        ops.tower_embed(table, layers)
    with pytest.raises(_lib.TTError):
        ops.tower_embed(table, layers, rows=torch.arange(4))


def test_export_refusals_before_any_device_work():
    from two_tower_recommender_model_amd import lifecycle as lc

    table = torch.zeros(10, 64)
    layers = [(torch.zeros(128, 64), torch.zeros(128)), (torch.zeros(64, 128), torch.zeros(64))]
    with pytest.raises(ValueError, match="fused=True"):
        lc.export_embeddings(table, layers, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="out_dtype"):
        lc.export_embeddings(table, layers, fused=True, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="precision"):
        lc.export_embeddings(table, layers, fused=True, precision="fp32")
    # an unsupported shape raises (the predicate's word, asked before any launch)
    wide = [(torch.zeros(48, 64), torch.zeros(48))]
    with pytest.raises(ValueError, match="tower_embed_supported"):
        lc.export_embeddings(table, wide, fused=True)
