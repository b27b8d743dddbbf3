"""The row-owned T1 (tower_rows_kernel) with its image wave: a fifth wave copies the 96 KB weight
image into LDS by LDS-DMA while the four compute waves fetch ids and rows. A wrong or late image
shows as wrong products, so every instantiation is compared bit for bit (torch.equal) with a path
that does not use the image:

* single-hot columns (row-owned T1, classic step) against the same batch given as bags of one id
  (multi-hot form: tower_l2_kernel, which reads the fragment-order weight copies);
* the ring (UPD instantiation) against the classic step over 3 steps, repeated ids in the batch;
* the pooled-input instantiation against the sum pool inside tower_l2_kernel;
* the IDX instantiation is covered by the sharded world-1 tests.

Tower weights come from the seeded uniform init, so every image element differs from its neighbours.

Batch sizes: the tower ABI takes multiples of 8 only (tower_layout: "B must be a positive multiple of
8", and ops.FusedTowers.supported says the same), so the shapes are the smallest such
sizes with the wanted tile pictures (32-row tiles): 8 and 24 = a ragged single tile, 40 = a ragged
second tile, 264 = 9 tiles, the last ragged, so xcd_remap places tiles on more than 8 block ids."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = [3000, 5000]


def _unique_cols(B, seed, device):
    """Ids in [1, N) (kept by the single-hot transform as they are), distinct per column except one
    repeated item row: the row updates then do not depend on a summation order."""
    g = torch.Generator().manual_seed(seed)
    cols = [torch.randperm(n - 1, generator=g)[:B] + 1 for n in N]
    cols[1][1] = cols[1][0]
    labels = torch.randint(0, 2, (B,), generator=g).to(torch.int32)
    return [c.to(device) for c in cols], labels.to(device)


@pytest.mark.parametrize("B", [8, 24, 40, 264])
@pytest.mark.parametrize("D", [64, 128])
def test_single_hot_step_equals_bags_of_one_id(device, D, B):
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    cols, labels = _unique_cols(B, 100 * D + B, device)
    a = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.01, seed=7)
    b = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.01, seed=7,
                          max_lookups=2 * B)
    assert a.gather and a.dedup_single and a.ring_supported()  # T1 = tower_rows_kernel
    assert b.gather_kjt                                        # T1 = tower_l2_kernel, multi-hot form
    assert torch.equal(a.params, b.params) and torch.equal(a.tables.weights, b.tables.weights)
    a.load_batch(cols, labels)
    a.step()
    b.load_kjt(torch.cat(cols), torch.arange(2 * B + 1, dtype=torch.int32, device=device), labels)
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.logits, b.logits)
    assert float(a.loss) == float(b.loss)
    assert torch.equal(a.gpooled, b.gpooled)
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert torch.equal(a.tables.weights, b.tables.weights)  # the touched rows, and nothing else moved
    assert torch.equal(a.tables.state, b.tables.state)


def _ring_batches(B, n, seed, device):
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(n):
        cols = [torch.randint(0, 2 * x, (B,), generator=g) for x in N]
        cols[0][3] = 0                   # a dropped id
        cols[1][:5] = 17 + s % 2         # a row repeated 5 times
        cols[0][6:8] = cols[0][5]        # a repeated user row
        if B >= 128:
            cols[1][100:160] = 2_345     # a hot row (60 lookups)
        out.append(([c.to(device) for c in cols], torch.randint(0, 2, (B,), generator=g).to(torch.int32).to(device)))
    return out


@pytest.mark.parametrize("B", [40, 264])
def test_ring_three_steps_equal_classic_steps(device, B):
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    batches = _ring_batches(B, 4, seed=B, device=device)
    a = FusedTwoTowerStep(N, [128, 128], [0], [1], [128, 64], B, device, seed=2)
    b = FusedTwoTowerStep(N, [128, 128], [0], [1], [128, 64], B, device, seed=2)
    assert a.ring_supported()
    a.capture_ring(batches, steps_per_graph=1)
    a.run(3)
    for cols, lab in batches[:3]:
        b.load_batch(cols, lab)
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.tables.weights, b.tables.weights) and torch.equal(a.tables.state, b.tables.state)
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert float(a.loss) == float(b.loss)
    assert torch.equal(a.logits, b.logits)


@pytest.mark.parametrize("D", [64, 128])
def test_pooled_input_equals_pool_inside_t1(device, D):
    """fuse_gather=False: tt_pooled_fwd, then the row-owned T1 on the pooled rows (POOL
    instantiation); fuse_gather=True: the sum pool inside tower_l2_kernel. B = 40, bags of 0..5."""
    import numpy as np

    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    B = 40
    rng = np.random.default_rng(50 + D)
    lengths = rng.integers(0, 6, 2 * B).astype(np.int32)
    vals = np.concatenate([rng.integers(0, N[i // B], lengths[i]) for i in range(2 * B)]).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    labels = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(D)).to(torch.int32).to(device)
    outs = []
    for fuse in (False, True):
        st = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.01, seed=6,
                               max_lookups=max(1, vals.size), fuse_gather=fuse, materialize_pooled=True)
        assert st.gather_kjt == fuse and st.towers is not None
        for _ in range(2):
            st.load_kjt(torch.from_numpy(vals).to(device), torch.from_numpy(offs).to(device), labels)
            st.step()
        torch.cuda.synchronize()
        outs.append([x.cpu().clone() for x in (st.pooled, st.logits, st.gpooled, st.loss, st.params, st.exp_avg,
                                               st.exp_avg_sq, st.tables.weights, st.tables.state)])
    for x, y in zip(*outs):
        assert torch.equal(x, y)

