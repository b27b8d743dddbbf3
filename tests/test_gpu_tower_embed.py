"""tt_tower_embed on the GPU (ops.tower_embed, lifecycle's fused=True paths): bit-identity with the
per-layer tt_linear_fwd chain that export_embeddings(precision="bf16") runs, the bf16 result, row
lists, the store guards, the oracle, and the lifecycle entry points that take the flag."""
import pytest
import torch

from oracle import ref

pytestmark = pytest.mark.gpu


def _case(device, in_dim, widths, M, seed=0, no_bias=(), ld=None):
    """Seeded table and tower. Rows ~ N(0, 1), W ~ N(0, 1 / K), bias ~ N(0, 1 / 4): pre-activations of
    about unit spread around zero at every layer, so roughly half the ReLUs fire and half do not."""
    g = torch.Generator(device=device).manual_seed(1000 + seed)
    if ld is None:
        table = torch.randn(M, in_dim, generator=g, device=device)
    else:
        table = torch.randn(M, ld, generator=g, device=device)[:, :in_dim]
    layers, k = [], in_dim
    for l, n in enumerate(widths):
        w = torch.randn(n, k, generator=g, device=device) / k ** 0.5
        b = None if l in no_bias else 0.5 * torch.randn(n, generator=g, device=device)
        layers.append((w, b))
        k = n
    return table, layers


def _per_layer(table, layers):
    """The path the fused kernel must reproduce bit for bit: one tt_linear_fwd per layer."""
    from two_tower_recommender_model_amd import lifecycle as lc

    return lc.export_embeddings(table, layers, precision="bf16")[1]


def _relu_share(emb):
    return float((emb > 0).float().mean())


BIT_CASES = [
    (64, [128, 64], 1000),
    (128, [128, 64], 40001),   # many tiles and a ragged tail
    (32, [32], 1),
    (96, [64, 96, 32], 63),
    (96, [64, 96, 32], 65),
    (128, [128, 128, 128], 777),
    # more 32-row tiles than the persistent grid has waves (256 CUs x 8): waves stride over 2 and 3
    # tiles with the next tile's rows prefetched, and the last tile is ragged
    (128, [128, 64], 150001),
    (64, [128, 64], 70003),
]


@pytest.mark.parametrize("in_dim, widths, M", BIT_CASES)
def test_bit_identical_to_the_per_layer_path(device, in_dim, widths, M):
    from two_tower_recommender_model_amd import ops

    assert ops.tower_embed_supported(in_dim, widths)
    table, layers = _case(device, in_dim, widths, M, seed=len(widths) + in_dim)
    want = _per_layer(table, layers)
    got = ops.tower_embed(table, layers)
    assert got.shape == (M, widths[-1]) and got.dtype == torch.float32
    if M >= 63:
        assert 0.2 < _relu_share(want) < 0.8  # a good share of ReLUs fire, a good share do not
    assert torch.equal(got, want)


def test_four_layers_of_128_run_or_are_refused_cleanly(device):
    from two_tower_recommender_model_amd import _lib, ops

    in_dim, widths, M = 128, [128, 128, 128, 128], 300
    table, layers = _case(device, in_dim, widths, M, seed=44)
    if ops.tower_embed_supported(in_dim, widths):
        assert torch.equal(ops.tower_embed(table, layers), _per_layer(table, layers))
        got = ops.tower_embed(table, layers, out_dtype=torch.bfloat16)
        assert torch.equal(got.view(torch.int16), _per_layer(table, layers).to(torch.bfloat16).view(torch.int16))
    else:
        with pytest.raises(_lib.TTError, match="tt_tower_embed"):
            ops.tower_embed(table, layers)


@pytest.mark.parametrize("no_bias", [(0,), (1,), (0, 1)])
def test_a_layer_without_bias(device, no_bias):
    from two_tower_recommender_model_amd import ops

    table, layers = _case(device, 64, [128, 64], 500, seed=7, no_bias=no_bias)
    assert any(b is None for _, b in layers)
    assert torch.equal(ops.tower_embed(table, layers), _per_layer(table, layers))


def test_strided_table(device):
    from two_tower_recommender_model_amd import ops

    for in_dim, widths in ((64, [128, 64]), (96, [64, 32])):
        table, layers = _case(device, in_dim, widths, 333, seed=9, ld=2 * in_dim)
        assert table.stride(0) == 2 * in_dim and not table.is_contiguous()
        want = _per_layer(table, layers)
        assert torch.equal(ops.tower_embed(table, layers), want)
        assert torch.equal(ops.tower_embed(table.contiguous(), layers), want)


@pytest.mark.parametrize("in_dim, widths, M", [(64, [128, 64], 1000), (128, [128, 64], 4097), (96, [64, 96, 32], 65),
                                               (32, [32], 1), (128, [64, 128], 130)])
def test_bf16_output_is_the_fp32_output_rounded_once(device, in_dim, widths, M):
    from two_tower_recommender_model_amd import ops

    table, layers = _case(device, in_dim, widths, M, seed=21)
    f32 = ops.tower_embed(table, layers)
    b16 = ops.tower_embed(table, layers, out_dtype=torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and b16.shape == f32.shape
    assert torch.equal(b16.view(torch.int16), f32.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(f32, _per_layer(table, layers))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("in_dim, widths", [(64, [128, 64]), (96, [64, 96, 32])])
def test_row_lists(device, dtype, in_dim, widths):
    from two_tower_recommender_model_amd import ops

    N = 5000
    table, layers = _case(device, in_dim, widths, N, seed=31)
    full = _per_layer(table, layers)
    zero = _per_layer(torch.zeros(1, in_dim, device=device), layers)[0]  # the tower on an empty bag's zero row
    g = torch.Generator().manual_seed(5)
    rows = torch.cat([torch.randperm(N, generator=g)[:1500],          # shuffled
                      torch.randint(0, N, (700,), generator=g),       # duplicates
                      torch.tensor([0, N - 1, N - 1, 0, 17, 17, 17])])
    bad = torch.tensor([-1, N, N + 1, -N, 2 ** 31 - 1, -(2 ** 31)] + ([2 ** 40, -(2 ** 40)] if dtype == torch.int64 else []))
    rows = torch.cat([rows, bad])[torch.randperm(rows.numel() + bad.numel(), generator=g)]
    ok = (rows >= 0) & (rows < N)
    n_bad = int((~ok).sum())
    assert n_bad == bad.numel() and rows.numel() % 32 != 0
    rows_d = rows.to(device=device, dtype=dtype)
    for out_dtype in (torch.float32, torch.bfloat16):
        count = torch.zeros(1, dtype=torch.int32, device=device)
        got = ops.tower_embed(table, layers, rows=rows_d, out_dtype=out_dtype, bad_rows=count)
        want = torch.where(ok.to(device)[:, None], full[rows.clamp(0, N - 1).to(device)], zero[None, :]).to(out_dtype)
        assert torch.equal(got.view(torch.int16) if out_dtype == torch.bfloat16 else got,
                           want.view(torch.int16) if out_dtype == torch.bfloat16 else want)
        assert int(count) == n_bad
        ops.tower_embed(table, layers, rows=rows_d, out_dtype=out_dtype, bad_rows=count)  # a count: it adds
        assert int(count) == 2 * n_bad
    # without the counter the bad rows are still zero rows, the others the rows they name
    got = ops.tower_embed(table, layers, rows=rows_d)
    assert torch.equal(got[ok.to(device)], full[rows[ok].to(device)])
    assert torch.equal(got[~ok.to(device)], zero[None, :].expand(n_bad, -1))


def test_range_mode_with_a_first_row(device):
    from two_tower_recommender_model_amd import _lib, ops

    N = 5000
    table, layers = _case(device, 64, [128, 64], N, seed=33)
    full = _per_layer(table, layers)
    assert torch.equal(ops.tower_embed(table, layers, first_row=1234), full[1234:])
    assert torch.equal(ops.tower_embed(table, layers, first_row=1234, count=777), full[1234:1234 + 777])
    assert torch.equal(ops.tower_embed(table, layers, first_row=N - 1, count=1), full[N - 1:])
    assert ops.tower_embed(table, layers, first_row=N, count=0).shape == (0, 64)
    with pytest.raises(_lib.TTError, match="tt_tower_embed"):
        ops.tower_embed(table, layers, first_row=1234, count=N - 1233)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("in_dim, widths, M", [(64, [128, 64], 1000), (128, [96], 33)])
def test_nothing_is_written_outside_the_result(device, out_dtype, in_dim, widths, M):
    from two_tower_recommender_model_amd import ops

    table, layers = _case(device, in_dim, widths, M, seed=41)
    width, ldo, before, after = widths[-1], widths[-1] + 24, 40, 40
    sentinel = -7.0  # no ReLU output is negative
    buf = torch.full((before + M + after, ldo), sentinel, dtype=out_dtype, device=device)
    view = buf[before:before + M, :width]
    assert view.stride(0) == ldo
    got = ops.tower_embed(table, layers, out=view)
    assert got.data_ptr() == view.data_ptr()
    want = _per_layer(table, layers).to(out_dtype)
    assert torch.equal(view.float(), want.float())
    assert bool((buf[:before] == sentinel).all()) and bool((buf[before + M:] == sentinel).all())
    assert bool((buf[:, width:] == sentinel).all())


def test_against_the_oracle(device):
    from two_tower_recommender_model_amd import ops

    for in_dim, widths, M in ((64, [128, 64], 3000), (128, [128, 64], 2000), (96, [64, 96, 32], 500)):
        table, layers = _case(device, in_dim, widths, M, seed=51)
        want = ref.mlp_fwd(table.cpu(), [(w.cpu(), b.cpu()) for w, b in layers])
        for out_dtype in (torch.float32, torch.bfloat16):
            got = ops.tower_embed(table, layers, out_dtype=out_dtype).float().cpu()
            err = (got - want).abs().max() / want.abs().max()
            print(in_dim, widths, out_dtype, float(err))
            assert float(err) < 2e-2, float(err)


def test_chunked_fill_of_one_output(device):
    from two_tower_recommender_model_amd import ops

    table, layers = _case(device, 128, [128, 64], 3001, seed=61)
    for out_dtype in (torch.float32, torch.bfloat16):
        one = ops.tower_embed(table, layers, out_dtype=out_dtype)
        out = torch.full((3001, 64), -7.0, dtype=out_dtype, device=device)
        ops.tower_embed(table, layers, first_row=0, count=1777, out=out[:1777])
        ops.tower_embed(table, layers, first_row=1777, out=out[1777:])
        assert torch.equal(out.float(), one.float())


# ---- lifecycle -------------------------------------------------------------------------------------

N = [3000, 5000]
D, B, LAYERS = 64, 512, [128, 64]


@pytest.fixture(scope="module")
def trained(device):
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    st = FusedTwoTowerStep(N, [D, D], [0], [1], LAYERS, B, device, seed=5)
    g = torch.Generator().manual_seed(3)
    cols = [torch.randint(0, 2 * x, (B,), generator=g) for x in N]
    st.load_batch([c.to(device) for c in cols], torch.randint(0, 2, (B,), generator=g).to(torch.int32).to(device))
    st.step()
    users = torch.randint(0, N[0], (300,), generator=g)
    return st, users


def test_export_fused_flag(device, trained):
    from two_tower_recommender_model_amd import lifecycle as lc

    st, _ = trained
    for tower, t in (("candidate", 1), ("query", 0)):
        ids0, emb0 = lc.export_fused(st, tower=tower)
        ids1, emb1 = lc.export_fused(st, tower=tower, fused=True, chunk=1000)
        assert torch.equal(ids0, ids1) and torch.equal(emb0, emb1) and emb1.shape == (N[t], LAYERS[-1])
        _, emb2 = lc.export_fused(st, tower=tower, fused=True, chunk=1000, out_dtype=torch.bfloat16)
        assert emb2.dtype == torch.bfloat16
        assert torch.equal(emb2.view(torch.int16), emb0.to(torch.bfloat16).view(torch.int16))
    with pytest.raises(ValueError):
        lc.export_fused(st, out_dtype=torch.bfloat16)


def test_retrieve_fused_flag(device, trained):
    from two_tower_recommender_model_amd import lifecycle as lc

    st, users = trained
    items16 = lc.export_fused(st, "candidate", fused=True, out_dtype=torch.bfloat16)[1]
    for metric in ("dot", "l2"):
        ids0, sc0 = lc.retrieve_fused(st, users, k=10, metric=metric)
        ids1, sc1 = lc.retrieve_fused(st, users, k=10, metric=metric, fused=True)
        assert torch.equal(ids0, ids1) and torch.equal(sc0, sc1)
        # the retrieval kernels round fp32 items to bf16 on load: bf16 items give the same bits
        ids2, sc2 = lc.retrieve_fused(st, users, k=10, metric=metric, fused=True, item_emb=items16)
        assert torch.equal(ids0, ids2) and torch.equal(sc0, sc2)
    # an int32 row list too
    ids3, sc3 = lc.retrieve_fused(st, users.to(torch.int32), k=10, fused=True)
    ids0, sc0 = lc.retrieve_fused(st, users, k=10)
    assert torch.equal(ids0, ids3) and torch.equal(sc0, sc3)


def test_evaluate_flags(device, trained):
    from two_tower_recommender_model_amd import lifecycle as lc

    st, users = trained
    g = torch.Generator().manual_seed(8)
    lens = torch.randint(0, 5, (users.numel(),), generator=g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    targets = torch.randint(1, N[1] + 1, (int(offsets[-1]),), generator=g)
    r0 = lc.evaluate_ranks(st, users, targets, offsets, ks=(1, 10, 100))
    r1 = lc.evaluate_ranks(st, users, targets, offsets, ks=(1, 10, 100), fused=True)
    for key in ("recall_at_k", "ndcg_at_k", "mrr", "mean_rank", "median_rank", "queries"):
        assert r0[key] == r1[key], key
    e0 = lc.evaluate_retrieval(st, users, targets, offsets, k=10)
    e1 = lc.evaluate_retrieval(st, users, targets, offsets, k=10, fused=True)
    for key in ("recall_at_k", "ndcg_at_k", "queries"):
        assert e0[key] == e1[key], key
