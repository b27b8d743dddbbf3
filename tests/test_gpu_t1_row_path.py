"""The row-owned T1's row path (tower_rows_kernel): its kernel arguments come from a host-built
front (one common record, one record per tower, fetched in a few batches), the 16 row DMAs of a wave
are issued behind one batch of row-index shuffles, and the updated rows go back to the tables as one
batch (all shuffles and LDS reads, one wait, then the predicated stores). A swapped per-tower record,
a store to a wrong row or a missed row changes a table, so every comparison is torch.equal against a
path that does not share the code:

* the ring (UPD instantiation: in-place update of the rows looked up once) against classic steps
  over 3 steps, whole tables and states compared, with the kinds of row mixed inside one store
  instruction's row group;
* the single-hot classic step against the same batch as bags of one id (tower_l2_kernel), over the
  id and label dtypes of the ABI;
* the POOL and IDX instantiations are covered by the pooled (test_gpu_t1_image_wave) and sharded
  world-1 tests.

The tables have 3,000 and 5,000 rows: unequal, so that a modulus, a table or a state pointer taken
from the other tower's record shows. Batch sizes are multiples of 8 (the tower ABI): 8 and 24 = a
ragged single tile, 40 = a ragged second tile, 264 = 9 tiles, the last ragged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = [3000, 5000]


def _mixed_cols(B, step, seed):
    """One batch whose rows alternate in kind along the batch, so that the rows one store
    instruction writes back (rows 2i, 2i + 1 of a wave's 16 at D = 128, four consecutive rows at
    D = 64) are of different kinds. Per block of 8 rows (tower 1: one row earlier):
    row + 2 is the dropped id 0, row + 3 an id >= N (the modulo path, a row of its own), the others
    rows looked up once, except the rows below that share an id: looked up 2 times (block 0), 3 times
    (block 1, one of them through the modulo path), 5 times (blocks 2 and 3; 4 times when B = 24).
    The dead rows of the ragged last tile follow the batch's last rows in their wave."""
    g = torch.Generator().manual_seed(seed)
    cols = []
    for t, n in enumerate(N):
        ids = torch.randperm(n - 1, generator=g)[:B + 3] + 1  # distinct rows; the last 3: the shared ids
        c = ids[:B].clone()
        multi = ids[B:]
        if step % 2:
            multi[0] = 17 + t  # the same row in every other step: updated again from its new value
        pos = (torch.arange(B) - t) % B  # tower 1: every kind one row earlier
        kinds = {2: [], 3: []}
        for i in range(B):
            if i % 8 in kinds:
                kinds[i % 8].append(i)
        c[pos[kinds[2]]] = 0
        c[pos[kinds[3]]] += n
        for k, rows in enumerate(([1, 4], [9, 12, 14], [17, 20, 22, 23, 31])):
            rows = [r for r in rows if r < B]
            if rows:
                c[pos[rows]] = multi[k]
        if B > 12:
            c[pos[12]] += n  # one lookup of the row looked up 3 times comes through the modulo
        if t == 1 and B >= 264:
            c[100:160] = 2_345  # a hot row: 60 lookups
        cols.append(c)
    labels = torch.randint(0, 2, (B,), generator=g).to(torch.int32)
    return cols, labels


@pytest.mark.parametrize("B", [8, 24, 40, 264])
@pytest.mark.parametrize("D", [64, 128])
def test_ring_three_steps_equal_classic_steps_mixed_row_groups(device, D, B):
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    batches = []
    for s in range(4):
        cols, lab = _mixed_cols(B, s, seed=1000 * D + 10 * B + s)
        batches.append(([c.to(device) for c in cols], lab.to(device)))
    a = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.01, seed=2)
    b = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.01, seed=2)
    assert a.ring_supported()
    assert torch.equal(a.tables.weights, b.tables.weights)
    a.capture_ring(batches, steps_per_graph=1)
    a.run(3)
    for cols, lab in batches[:3]:
        b.load_batch(cols, lab)
        b.step()
    torch.cuda.synchronize()
    # whole tables and states: a store to a wrong row or a missed row shows
    assert torch.equal(a.tables.weights, b.tables.weights)
    assert torch.equal(a.tables.state, b.tables.state)
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert float(a.loss) == float(b.loss)
    assert torch.equal(a.logits, b.logits)


@pytest.mark.parametrize("label_dtype", [torch.int32, torch.int64, torch.float32])
@pytest.mark.parametrize("id_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("B", [24, 40])
@pytest.mark.parametrize("D", [64, 128])
def test_single_hot_step_equals_bags_of_one_id_over_dtypes(device, D, B, id_dtype, label_dtype):
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    g = torch.Generator().manual_seed(100 * D + B)
    cols = [(torch.randperm(n - 1, generator=g)[:B] + 1).to(id_dtype) for n in N]
    cols[1][1] = cols[1][0]  # one repeated item row
    if label_dtype == torch.float32:
        labels = torch.rand(B, generator=g)  # soft labels
    else:
        labels = torch.randint(0, 2, (B,), generator=g).to(label_dtype)
    cols, labels = [c.to(device) for c in cols], labels.to(device)
    a = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.01, seed=7,
                          id_dtype=id_dtype)
    b = FusedTwoTowerStep(N, [D, D], [0], [1], [128, 64], B, device, lr_emb=0.02, lr_dense=0.01, seed=7,
                          id_dtype=id_dtype, max_lookups=2 * B)
    assert a.gather and a.dedup_single and a.ring_supported()  # T1 = tower_rows_kernel
    assert b.gather_kjt                                        # T1 = tower_l2_kernel, multi-hot form
    # the step passes its label buffer on with the buffer's dtype
    a.labels = torch.empty(B, dtype=label_dtype, device=device)
    b.labels = torch.empty(B, dtype=label_dtype, device=device)
    a.load_batch(cols, labels)
    a.step()
    b.load_kjt(torch.cat(cols), torch.arange(2 * B + 1, dtype=torch.int32, device=device), labels)
    b.step()
    torch.cuda.synchronize()
    assert a.labels.dtype == label_dtype and torch.equal(a.labels, labels)
    assert torch.equal(a.logits, b.logits)
    assert float(a.loss) == float(b.loss)
    assert torch.equal(a.gpooled, b.gpooled)
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert torch.equal(a.tables.weights, b.tables.weights)
    assert torch.equal(a.tables.state, b.tables.state)
