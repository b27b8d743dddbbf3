"""The row-owned T1's product chain (tower_rows_kernel behind barrier 1): one weight-fragment
pipeline runs through the four products (each product issues the next one's first fragments), the
wave's rows are read back and packed in front of barrier 1, the bias column sums run under the
backward products and row half 1's partials are written long before barrier 3, and the tile's loss
partial is read as one batch. What can go wrong is a fragment read of the PREVIOUS launch's weight
image (the LDS keeps it: the previous step's weights), a row read before the wave's DMAs landed, a
bias or loss partial left over from an earlier launch, and a dead wave's partials that are not exact
zeros. Every comparison is torch.equal against a path that does not run tower_rows_body:

* one classic step on float32 soft labels (row losses and dlogit vary per row) against the same
  batch as bags of one id (tower_l2_kernel), over ragged batches (B = 8 and 16: row half 1 of the
  tile is a dead wave; 24: a ragged half; 40: a ragged second tile; 264: 9 tiles), three steps with
  a different batch in the middle, so that what one launch leaves in the LDS meets the next; the
  biases' gradients and moments carry the column sums;
* the ring (UPD instantiation) over 4 steps against 4 classic steps with a dense learning rate at
  which most bf16 weights change every step (checked from the parameters) and different ids in
  every batch;
* the pooled-input (POOL) and indexed (IDX, sharded world 1) instantiations at B = 40, the smallest
  batch with a ragged second tile, against the paths through tower_l2_kernel.

Tables of 3,000 and 5,000 rows (unequal: a pointer from the other tower's record shows)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = [3000, 5000]


def _distinct_cols(B, nb, seed, device):
    """nb batches of ids in [1, N), no id twice in a column over all the batches (the row updates
    then do not depend on a summation order, and no batch reads a row another one wrote), float32
    soft labels."""
    g = torch.Generator().manual_seed(seed)
    perms = [torch.randperm(n - 1, generator=g)[:nb * B] + 1 for n in N]
    out = []
    for s in range(nb):
        cols = [p[s * B:(s + 1) * B].clone().to(device) for p in perms]
        out.append((cols, torch.rand(B, generator=g).to(device)))
    return out


def _equal_steps(a, b, what):
    for name in ("logits", "gpooled", "params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{what}: {name}"
    # the raw tower gradients where both paths write them out (not every update kernel does: the
    # first moments above carry them in any case)
    if bool(a.grads.any()) and bool(b.grads.any()):
        assert torch.equal(a.grads, b.grads), f"{what}: grads"
    assert float(a.loss) == float(b.loss), what
    assert torch.equal(a.tables.weights, b.tables.weights), what
    assert torch.equal(a.tables.state, b.tables.state), what


@pytest.mark.parametrize("B", [8, 16, 24, 40, 264])
@pytest.mark.parametrize("D", [64, 128])
def test_bias_and_loss_partials_over_ragged_tiles(device, D, B):
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    x, y = _distinct_cols(B, 2, 1000 * D + B, device)
    a = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.01, seed=7)
    b = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.01, seed=7,
                          max_lookups=2 * B)
    assert a.gather and a.dedup_single and a.ring_supported()  # T1 = tower_rows_kernel
    assert b.gather_kjt                                        # T1 = tower_l2_kernel, multi-hot form
    a.labels = torch.empty(B, dtype=torch.float32, device=device)
    b.labels = torch.empty(B, dtype=torch.float32, device=device)
    offs = torch.arange(2 * B + 1, dtype=torch.int32, device=device)
    # the batch, another one, the first again (its rows and the weights have moved: not the same step)
    for k, (cols, labels) in enumerate((x, y, x)):
        a.load_batch(cols, labels)
        a.step()
        b.load_kjt(torch.cat(cols), offs, labels)
        b.step()
        torch.cuda.synchronize()
        assert a.labels.dtype == torch.float32
        # every bias's first moment has non-zero entries: the column sums are compared
        for bias in (*a.qb, *a.cb):
            o = (bias.data_ptr() - a.params.data_ptr()) // 4
            assert bool(a.exp_avg[o:o + bias.numel()].any())
        _equal_steps(a, b, f"step {k}")


def _w0_images(st):
    """bf16 images of both towers' first-layer weights, from the parameters."""
    return torch.cat([st.qW[0].detach().flatten(), st.cW[0].detach().flatten()]).to(torch.bfloat16).cpu()


@pytest.mark.parametrize("B", [40, 264])
@pytest.mark.parametrize("D", [64, 128])
def test_ring_reads_this_steps_image_and_rows(device, D, B):
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    g = torch.Generator().manual_seed(77 * D + B)
    batches = []
    perms = [torch.randperm(n - 1, generator=g)[:4 * B] + 1 for n in N]
    for s in range(4):
        cols = [p[s * B:(s + 1) * B].clone() for p in perms]
        cols[0][3] = 0                 # a dropped id
        cols[1][1] = cols[1][0]        # a row looked up twice (the tail's list role)
        cols[0][5] += N[0]             # the modulo path
        batches.append(([c.to(device) for c in cols], torch.randint(0, 2, (B,), generator=g).to(torch.int32).to(device)))
    kw = dict(lr_emb=0.02, lr_dense=0.05, seed=2)
    a = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, **kw)
    b = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, **kw)
    assert a.ring_supported()
    a.capture_ring(batches, steps_per_graph=1)
    a.run(4)
    images = [_w0_images(b)]
    for cols, lab in batches:
        b.load_batch(cols, lab)
        b.step()
        torch.cuda.synchronize()
        images.append(_w0_images(b))
    # the image a launch finds in the LDS (the previous step's) differs from the one it must read
    for s in range(4):
        changed = float((images[s] != images[s + 1]).float().mean())
        print(f"step {s}: {changed:.3f} of W0's bf16 image changed")
        assert changed >= 0.5
    assert torch.equal(a.tables.weights, b.tables.weights) and torch.equal(a.tables.state, b.tables.state)
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert float(a.loss) == float(b.loss)
    assert torch.equal(a.logits, b.logits)


@pytest.mark.parametrize("D", [64, 128])
def test_pooled_input_chain_equals_pool_inside_t1(device, D):
    """fuse_gather=False: tt_pooled_fwd, then the row-owned T1 on the pooled rows (POOL
    instantiation); fuse_gather=True: the sum pool inside tower_l2_kernel. B = 40, bags of 0..5, two
    steps (the second launch finds the first one's image and partials)."""
    import numpy as np

    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    B = 40
    rng = np.random.default_rng(90 + D)
    lengths = rng.integers(0, 6, 2 * B).astype(np.int32)
    vals = np.concatenate([rng.integers(0, N[i // B], lengths[i]) for i in range(2 * B)]).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    labels = torch.rand(B, generator=torch.Generator().manual_seed(D)).to(device)
    outs = []
    for fuse in (False, True):
        st = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.05, seed=6,
                               max_lookups=max(1, vals.size), fuse_gather=fuse, materialize_pooled=True)
        assert st.gather_kjt == fuse and st.towers is not None
        st.labels = torch.empty(B, dtype=torch.float32, device=device)
        for _ in range(2):
            st.load_kjt(torch.from_numpy(vals).to(device), torch.from_numpy(offs).to(device), labels)
            st.step()
        torch.cuda.synchronize()
        outs.append([x.cpu().clone() for x in (st.pooled, st.logits, st.gpooled, st.loss, st.grads, st.params,
                                               st.exp_avg, st.exp_avg_sq, st.tables.weights, st.tables.state)])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("D", [64, 128])
def test_sharded_world1_chain_equals_bags_of_one_id(device, D):
    """The sharded step at W = 1 (IDX instantiation: bf16 rows by position) against the single-GPU
    step on bags of one id (tower_l2_kernel), 3 steps at B = 40."""
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep
    from two_tower_recommender_model_amd.sharded import FusedShardedTwoTowerStep, ThreadComm

    B = 40
    ref_step = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, seed=6, max_lookups=2 * B)
    assert ref_step.gather_kjt
    full = [ref_step.tables.table_view(f).cpu().clone() for f in range(2)]
    sh = FusedShardedTwoTowerStep(ThreadComm.group(1)[0], N, D, [128, 64], B, device, full_tables=full, seed=6)
    sh.params.copy_(ref_step.params)
    sh.towers.update(sh.params, do_adam=False)
    g = torch.Generator().manual_seed(20 + D)
    offs = torch.arange(2 * B + 1, dtype=torch.int32, device=device)
    for s in range(3):
        cols = [torch.randperm(n - 1, generator=g)[:B] + 1 for n in N]
        cols[1][1] = cols[1][0]  # one repeated item row
        lab = torch.randint(0, 2, (B,), generator=g).to(torch.int32)
        cols = [c.to(device) for c in cols]
        sh.load_batch(cols, lab.to(device))
        sh.step()
        ref_step.load_kjt(torch.cat(cols), offs, lab.to(device))
        ref_step.step()
    torch.cuda.synchronize()
    sh.check()
    for f in range(2):
        assert torch.equal(sh.tables.table_view(f), ref_step.tables.table_view(f))
        assert torch.equal(sh.tables.state_view(f), ref_step.tables.state_view(f))
    assert torch.equal(sh.params, ref_step.params)
    assert torch.equal(sh.logits, ref_step.logits)
    assert float(sh.loss) == float(ref_step.loss)
