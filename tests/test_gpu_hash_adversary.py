"""The grouping hash tables under forced collisions and wrap-around (tests/hash_adversary.py: row ids
derived from a restatement of the kernels' hash, pinned to csrc/ by tests/test_cpu_hash_adversary.py).

Every table use — the dedup global table (column and segment inserts, the deferred insert of the
classic fused step and its resolver, the ring's LDS-merged insert, the sharded owner's insert inside
the gather) and the KJT-form tables (chunk LDS table, batched global insert, column form) — gets
batches whose keys share one home slot (P1), fill a cluster through cap - 1 -> 0 (P2), mix lookup
counts around the inline / hot thresholds inside one cluster (P3), chain in the LDS table only (P4)
and load the KJT-form table to its designed maximum of 1/2 (P5). Three oracles, no new tolerance:

 (a) twin, bitwise: the same op on the batch with its distinct rows relabelled onto rows 1..U (the
     twin's table rows are copies of the adversarial rows). A row's update sums its lookups in
     ascending lookup / bag order (hot rows: fixed ranges of that order), which depends on neither
     the row id nor the slot, so weights, state, logits, loss, tower parameters and Adam moments
     must agree bit for bit;
 (b) the oracle (oracle/ref.py pooled_bwd_dense + rowwise_adagrad) on the touched rows, with the
     tolerances of test_dedup_cols_vs_oracle / test_dedup_segments_vs_oracle (dedup),
     test_pooled_fwd_and_fused_rowwise_adagrad (KJT form) and test_fused_adagrad_hot_rows (its hot rows);
 (c) nothing else moved: every untouched row of weights and state bitwise unchanged (compared on
     the device), the dedup workspace clean after every update.

The tables themselves are read between the launches: the filled slots must be the set linear
probing gives for the batch's keys (order-independent), every key once, in its cluster at or after
its home slot; the run reports the cluster through slot 0 and the displaced hot keys it found."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import hash_adversary as ha
from edge_cases import assert_bitwise, assert_clean
from oracle import ref

pytestmark = pytest.mark.gpu

N = [ha.N_ROWS, ha.N_ROWS]
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
LR, EPS = 0.05, 1e-10


@pytest.fixture(scope="module")
def ops():
    from two_tower_recommender_model_amd import ops as _ops

    return _ops


def _al(x):
    return (x + 255) // 256 * 256


def _t(a, device, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(device)


def _copy_twin_rows(adv, tw, maps):
    """Twin row j + 1 of table t = adversarial row maps[t][j] (every other twin row: zero)."""
    tw.weights.zero_()
    for t, m in enumerate(maps):
        idx = torch.from_numpy(m).to(adv.device)
        tw.table_view(t)[1:m.size + 1] = adv.table_view(t)[idx]
        tw.state_view(t)[1:m.size + 1] = adv.state_view(t)[idx]


def _assert_twin_rows(adv, tw, maps, what):
    for t, m in enumerate(maps):
        idx = torch.from_numpy(m).to(adv.device)
        assert_bitwise(adv.table_view(t)[idx], tw.table_view(t)[1:m.size + 1], f"{what}: weights of table {t} vs twin")
        assert_bitwise(adv.state_view(t)[idx], tw.state_view(t)[1:m.size + 1], f"{what}: state of table {t} vs twin")


def _assert_untouched(ts, w0, maps, what):
    """(c): every row no lookup named keeps its bits (state: still zero); on the device."""
    for t, m in enumerate(maps):
        keep = torch.ones(ts.rows[t], dtype=torch.bool, device=ts.device)
        keep[torch.from_numpy(m).to(ts.device)] = False
        o = ts.weight_offsets[t]
        before = w0[o:o + ts.rows[t] * ts.dims[t]].view(ts.rows[t], ts.dims[t])
        same = (ts.table_view(t).view(torch.int32) == before.view(torch.int32)).all(dim=1)
        assert bool(same[keep].all()), f"{what}: an untouched row of table {t} changed"
        assert bool((ts.state_view(t).view(torch.int32)[keep] == 0).all()), f"{what}: state of an untouched row of table {t}"
        assert int(keep.sum()) == ts.rows[t] - m.size


def _assert_touched_moved(ts, maps, what, frac=1.0):
    """The comparisons above are not vacuous: the touched rows were updated (row state > 0 unless
    every gradient row of the row is exactly zero)."""
    for t, m in enumerate(maps):
        moved = int((ts.state_view(t)[torch.from_numpy(m).to(ts.device)] > 0).sum()) / m.size
        assert moved >= frac, f"{what}: only {moved:.3f} of the touched rows of table {t} have state > 0"


# ---- reading the dedup table (csrc/dedup.hip dedup_layout, as edge_cases.assert_clean restates it) ----


def _read_dedup(ws: torch.Tensor, L: int):
    cap = ha.dedup_cap(L)
    raw = ws[:cap * 128].cpu()
    words = raw.view(torch.int64).view(cap, 16)[:, 0].numpy().view(np.uint64)
    items = raw.view(torch.int32).view(cap, 32)[:, 2:2 + ha.DD_INL].numpy()
    lkey = ws[cap * 128:cap * 128 + 8 * L].view(torch.int64).cpu().numpy().view(np.uint64)
    o = cap * 128 + _al(8 * L) + _al(4 * (L // (ha.DD_INL + 1) + 1))
    ctr = ws[o:o + 16].view(torch.int32).cpu().tolist()
    claim = ws[o + 256:o + 256 + 4 * L].view(torch.int32).cpu().numpy()
    return cap, words, items, lkey, ctr, claim


def _inspect_dedup(ws, L, want_keys, what):
    """After an insert, before the update. want_keys: uint64 [n] key per lookup (EMPTY: dropped)."""
    cap, words, items, lkey, ctr, claim = _read_dedup(ws, L)
    n = want_keys.size
    assert np.array_equal(lkey[:n], want_keys), f"{what}: per-lookup keys"
    live = want_keys != EMPTY
    uk, cnt = np.unique(want_keys[live], return_counts=True)
    full = np.nonzero(words != EMPTY)[0]
    slot_key = {int(s): int(words[s] >> np.uint64(ha.DD_CNT_BITS)) for s in full}
    chk = ha.check_placement(slot_key, uk, cap)
    got = sorted((int(words[s] >> np.uint64(ha.DD_CNT_BITS)), int(words[s] & np.uint64(0x3FFFF))) for s in full)
    assert got == sorted(zip(uk.tolist(), cnt.tolist())), f"{what}: (key, count) pairs of the filled slots"
    hot = {int(k) for k, c in zip(uk.tolist(), cnt.tolist()) if c > ha.DD_INL}
    assert ctr[0] == len(hot), f"{what}: hot counter {ctr[0]}, {len(hot)} keys with more than {ha.DD_INL} lookups"
    pos_of = {int(k): np.nonzero(want_keys == k)[0] for k in uk}
    for s, k in slot_key.items():  # the inline lookup indices: distinct lookups of this very key
        p = pos_of[k]
        it = items[s][:min(p.size, ha.DD_INL)]
        assert np.unique(it).size == it.size and np.isin(it, p).all(), f"{what}: inline lookups of slot {s}"
        assert claim[it[0]] == s, f"{what}: the lookup at position 0 of slot {s} did not record its claim"
    assert int((claim[:n] >= 0).sum()) == uk.size, f"{what}: one claiming lookup per key"
    hot_displaced = sorted(hot & set(chk.displaced_keys))
    print(f"{what}: cap {cap}, {uk.size} keys, {chk.displaced} displaced, longest probe {chk.longest}, "
          f"cluster through slot 0: {chk.wraps}, displaced hot keys: {len(hot_displaced)}")
    return chk, hot_displaced


def _oracle_cols(otab, ost, tcols, gout, dims):
    """One oracle step over the twin's small tables (rows 0..U): dense index_add gradient + row-wise Adagrad."""
    Ns = [t.shape[0] for t in otab]
    B = tcols[0].size
    v, _, o = ref.kjt_build([c.astype(np.int64) for c in tcols], Ns)
    grads = ref.pooled_bwd_dense(otab, list(range(len(Ns))), torch.from_numpy(v).to(torch.int64), torch.from_numpy(o), B, gout)
    for t in range(len(Ns)):
        touched = torch.unique(torch.from_numpy(v[o[t * B]:o[(t + 1) * B]]).to(torch.int64))
        ref.rowwise_adagrad_sparse(otab[t], ost[t], touched, grads[t][touched], LR, EPS)


def _assert_dedup_vs_oracle(tw, otab, ost, maps):
    """Tolerances of test_dedup_cols_vs_oracle / test_dedup_segments_vs_oracle."""
    for t, m in enumerate(maps):
        U = m.size
        np.testing.assert_allclose(tw.state_view(t)[:U + 1].cpu().numpy(), ost[t].numpy(), rtol=1e-4, atol=1e-9)
        np.testing.assert_allclose(tw.table_view(t)[:U + 1].cpu().numpy(), otab[t].numpy(), rtol=1e-4, atol=1e-6)


# ---- 1. tt_dedup_insert_cols -> inspect -> tt_dedup_rowwise_adagrad ----------------------------------------


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_dedup_cols_collisions(ops, device, dtype):
    B, dims = 256, [8, 8]
    adv = ops.TableSet(N, dims, [0, 1], device)
    adv.init_uniform_(torch.Generator(device=device).manual_seed(1))
    w0 = adv.weights.clone()
    tw = ops.TableSet(N, dims, [0, 1], device)
    adv.ensure_dedup_workspace(2 * B)
    cap = ha.dedup_cap(adv._dd_cap)
    assert cap == 8192
    pats = ha.dedup_patterns(N, cap)
    steps = [ha.cols_batch(B, N, pats, seed) for seed in (1, 2)]
    tws, maps = ha.twin([np.concatenate([s[t] for s in steps]) for t in range(2)], N)
    tsteps = [[tws[t][i * B:(i + 1) * B] for t in range(2)] for i in range(2)]
    _copy_twin_rows(adv, tw, maps)
    otab = [tw.table_view(t)[:maps[t].size + 1].cpu().clone() for t in range(2)]
    ost = [torch.zeros(maps[t].size + 1) for t in range(2)]
    for i, (cols, tcols) in enumerate(zip(steps, tsteps)):
        gout = torch.randn(B, sum(dims), generator=torch.Generator().manual_seed(i))
        adv.dedup_insert_cols([_t(c, device, dtype) for c in cols], N)
        torch.cuda.synchronize()
        chk, hot_displaced = _inspect_dedup(adv._dd_ws, adv._dd_cap, np.concatenate(ha.packed_keys(cols, N, ha.dd_key)),
                                            f"dedup cols step {i}")
        assert chk.wraps, "P2: no cluster runs through slot 0"
        assert chk.longest >= 47, "P1: 48 keys of one home slot give a probe of 47"
        assert len(hot_displaced) >= 2, "P3: fewer than two hot keys were displaced"
        adv.dedup_rowwise_adagrad(gout.to(device), B, LR, EPS)
        assert_clean(adv)
        tw.dedup_insert_cols([_t(c, device, dtype) for c in tcols], N)
        tw.dedup_rowwise_adagrad(gout.to(device), B, LR, EPS)
        assert_clean(tw)
        _oracle_cols(otab, ost, tcols, gout, dims)
    torch.cuda.synchronize()
    _assert_twin_rows(adv, tw, maps, "dedup cols")
    _assert_dedup_vs_oracle(tw, otab, ost, maps)
    _assert_untouched(adv, w0, maps, "dedup cols")
    _assert_touched_moved(adv, maps, "dedup cols")


# ---- 2. tt_dedup_insert_segments ------------------------------------------------------------------------------


def test_dedup_segments_collisions(ops, device):
    """The same families as int64 keys in two segments (segment t: table t's kept lookups, counts <
    seg_capacity, the rest of a segment holds -1), flat gradient rows."""
    C, D = 256, 8
    adv = ops.TableSet(N, [D, D], [0, 1], device)
    adv.init_uniform_(torch.Generator(device=device).manual_seed(2))
    tw = ops.TableSet(N, [D, D], [0, 1], device)
    adv.ensure_dedup_workspace(2 * C)
    cap = ha.dedup_cap(adv._dd_cap)
    cols = ha.cols_batch(C, N, ha.dedup_patterns(N, cap), seed=5)
    tcols, maps = ha.twin(cols, N)
    _copy_twin_rows(adv, tw, maps)

    def segments(cc):
        keys = np.full(2 * C, -1, np.int64)
        counts = np.zeros(2, np.int32)
        for t in range(2):
            r = np.mod(cc[t][cc[t] != 0].astype(np.int64), N[t])
            counts[t] = r.size
            keys[t * C:t * C + r.size] = ha.dd_key(t, r).view(np.int64)
        return keys, counts

    keys, counts = segments(cols)
    tkeys, tcounts = segments(tcols)
    assert np.array_equal(counts, tcounts) and counts.max() < C
    otab = [tw.table_view(t)[:maps[t].size + 1].cpu().clone() for t in range(2)]
    ost = [torch.zeros(maps[t].size + 1) for t in range(2)]
    want = keys.view(np.uint64).copy()
    for t in range(2):
        want[t * C + counts[t]:(t + 1) * C] = EMPTY
    for i in range(2):
        grad = torch.randn(2 * C, D, generator=torch.Generator().manual_seed(10 + i))
        adv.dedup_insert_segments(_t(keys, device), _t(counts, device), C)
        torch.cuda.synchronize()
        chk, hot_displaced = _inspect_dedup(adv._dd_ws, adv._dd_cap, want, f"dedup segments step {i}")
        assert chk.wraps and len(hot_displaced) >= 2
        adv.dedup_rowwise_adagrad(grad.to(device), 2 * C, LR, EPS, flat=True)
        assert_clean(adv)
        tw.dedup_insert_segments(_t(tkeys, device), _t(tcounts, device), C)
        tw.dedup_rowwise_adagrad(grad.to(device), 2 * C, LR, EPS, flat=True)
        for t in range(2):  # the oracle of test_dedup_segments_vs_oracle, on the twin's small tables
            gd = torch.zeros(maps[t].size + 1, D)
            k = torch.from_numpy(tkeys[t * C:t * C + counts[t]])
            gd.index_add_(0, k & ((1 << 40) - 1), grad[t * C:t * C + counts[t]])
            touched = torch.unique(k & ((1 << 40) - 1))
            ref.rowwise_adagrad_sparse(otab[t], ost[t], touched, gd[touched], LR, EPS)
    torch.cuda.synchronize()
    _assert_twin_rows(adv, tw, maps, "dedup segments")
    _assert_dedup_vs_oracle(tw, otab, ost, maps)
    _assert_touched_moved(adv, maps, "dedup segments")


# ---- 3 / 4 / 6. the fused steps --------------------------------------------------------------------------------

FB, FD, FSTEPS, FSEED = 512, 64, 4, 2


@lru_cache(maxsize=None)
def _fused_batches():
    """4 batches of B = 512 (1024 lookups: dedup cap 16384) that reuse the colliding rows, their
    twins and the twin maps."""
    cap = ha.dedup_cap(2 * FB)
    pats = ha.fused_patterns(N, cap)
    steps = [ha.cols_batch(FB, N, pats, 20 + s) for s in range(FSTEPS)]
    tws, maps = ha.twin([np.concatenate([s[t] for s in steps]) for t in range(2)], N)
    tsteps = [[tws[t][i * FB:(i + 1) * FB] for t in range(2)] for i in range(FSTEPS)]
    labels = [np.random.default_rng(s).integers(0, 2, FB).astype(np.int32) for s in range(FSTEPS)]
    return cap, steps, tsteps, maps, labels


def _new_step(device, **kw):
    from two_tower_recommender_model_amd.fused import FusedTwoTowerStep

    return FusedTwoTowerStep(N, [FD, FD], [0], [1], [128, 64], FB, device, seed=FSEED, **kw)


def _dev_batches(steps, labels, device):
    return [([_t(c, device) for c in cols], _t(lab, device)) for cols, lab in zip(steps, labels)]


@pytest.fixture(scope="module")
def classic(device):
    """The classic fused step (insert deferred inside T1, resolved by the following launch) over the
    adversarial batches: the reference of the ring and sharded cases, computed once."""
    cap, steps, _, _, labels = _fused_batches()
    st = _new_step(device)
    assert st.gather and st.dedup_single and st.combined_bwd
    assert ha.dedup_cap(st.tables._dd_cap) == cap == 16384
    w0, p0 = st.tables.weights.clone(), st.params.clone()
    for cols, lab in _dev_batches(steps, labels, device):
        st.load_batch(cols, lab)
        st.step()
        assert_clean(st.tables)
    torch.cuda.synchronize()
    return {"step": st, "w0": w0, "p0": p0}


def test_classic_step_collisions_vs_twin(device, classic):
    """Oracle (a) and (c) for the deferred insert + resolver: P1-P4 over 4 steps, state accumulating."""
    _, steps, tsteps, maps, labels = _fused_batches()
    a = classic["step"]
    b = _new_step(device)
    assert_bitwise(b.tables.weights, classic["w0"], "same seed, same initial tables")
    for t, m in enumerate(maps):  # the twin's rows 1..U = the adversarial rows' initial values
        o = b.tables.weight_offsets[t]
        init = classic["w0"][o:o + N[t] * FD].view(N[t], FD)
        b.tables.table_view(t)[1:m.size + 1] = init[torch.from_numpy(m).to(device)]
    for cols, lab in _dev_batches(tsteps, labels, device):
        b.load_batch(cols, lab)
        b.step()
    torch.cuda.synchronize()
    _assert_twin_rows(a.tables, b.tables, maps, "classic step")
    for name in ("params", "exp_avg", "exp_avg_sq", "logits", "loss"):
        assert_bitwise(getattr(a, name), getattr(b, name), f"classic step vs twin: {name}")
    _assert_untouched(a.tables, classic["w0"], maps, "classic step")
    # (a row's dX rows are all exactly zero only when every hidden unit of its samples is inactive)
    _assert_touched_moved(a.tables, maps, "classic step", frac=0.5)


def _assert_equals_classic(x, classic, what):
    a = classic["step"]
    assert torch.equal(x.tables.weights, a.tables.weights), f"{what}: weights"
    assert torch.equal(x.tables.state, a.tables.state), f"{what}: state"
    assert torch.equal(x.params, a.params) and torch.equal(x.exp_avg, a.exp_avg), f"{what}: towers"
    assert float(x.loss) == float(a.loss), f"{what}: loss"
    assert torch.equal(x.logits, a.logits), f"{what}: logits"


@pytest.mark.parametrize("ring_tail", [True, False], ids=["tail", "two_launch_tail"])
def test_ring_collisions_equal_classic_step(device, classic, ring_tail):
    """The ring (ring_tail: the next batch's insert merged in LDS per workgroup of 256 lookups — P4
    chains in that INS_HS-slot table only — then one atomic per key into the global table; else the
    deferred insert + resolver), 2 steps per graph, 4 steps: each of the two alternating workspaces
    receives the families twice. Bit for bit the classic step (test_ring_equals_classic_step)."""
    _, steps, _, _, labels = _fused_batches()
    r = _new_step(device)
    assert r.ring_supported()
    r.ring_tail = ring_tail
    r.capture_ring(_dev_batches(steps, labels, device), steps_per_graph=2)
    r.run(FSTEPS)
    torch.cuda.synchronize()
    _assert_equals_classic(r, classic, f"ring (ring_tail={ring_tail})")


def test_sharded_w1_collisions_equal_classic_step(device, classic):
    """The owner-side insert inside the gather (tt_shard_gather_segs_bf16 with a dedup workspace) at
    world size 1, on the same batches: bit for bit the fused single-GPU step
    (test_sharded_w1_equals_fused_single_gpu_step)."""
    from two_tower_recommender_model_amd.sharded import FusedShardedTwoTowerStep, ThreadComm

    cap, steps, _, _, labels = _fused_batches()
    a, w0 = classic["step"], classic["w0"]
    full = [w0[a.tables.weight_offsets[f]:a.tables.weight_offsets[f] + N[f] * FD].view(N[f], FD) for f in range(2)]
    sh = FusedShardedTwoTowerStep(ThreadComm.group(1)[0], N, FD, [128, 64], FB, device, full_tables=full, seed=FSEED)
    assert ha.dedup_cap(sh.max_lookups) == cap
    sh.params.copy_(classic["p0"])
    sh.towers.update(sh.params, do_adam=False)
    for cols, lab in _dev_batches(steps, labels, device):
        sh.load_batch(cols, lab)
        sh.step()
    torch.cuda.synchronize()
    sh.check()
    for f in range(2):
        assert torch.equal(sh.tables.table_view(f), a.tables.table_view(f)), f"sharded W=1: weights of table {f}"
        assert torch.equal(sh.tables.state_view(f), a.tables.state_view(f)), f"sharded W=1: state of table {f}"
    assert torch.equal(sh.params, a.params) and torch.equal(sh.logits, a.logits)
    assert float(sh.loss) == float(a.loss)


# ---- 5. KJT form ---------------------------------------------------------------------------------------------------


def _bwd_offsets(L: int):
    """csrc/embedding.hip bwd_layout up to ent_h: keys, cnt, cur [cap]; slot_of, perm [L]; urec [L] x 16 B;
    lk, ent_h [L]; every array padded to 256 B."""
    cap = ha.bwd_cap(L)
    o, out = 0, {}
    for name, nbytes in (("keys", 8 * cap), ("cnt", 4 * cap), ("cur", 4 * cap), ("slot_of", 4 * L), ("perm", 4 * L),
                         ("urec", 16 * L), ("lk", 4 * L), ("ent_h", 4 * L)):
        out[name] = (o, nbytes)
        o += _al(nbytes)
    return cap, out


def _bwd_read(ts, name, dtype):
    cap, lay = _bwd_offsets(ts._bwd_cap)
    o, nbytes = lay[name]
    return ts._bwd_ws[o:o + nbytes].view(dtype).cpu().numpy()


def _inspect_bwd(ts, slot_of_lookup, keys, what):
    """After tt_bwd_prepare[_cols]: the key table is clean again; the slot recorded for every lookup
    names one slot per key, the slots are linear probing's set, every key in its cluster; the
    per-slot lookup count (written by the scan) is the key's."""
    cap, _ = _bwd_offsets(ts._bwd_cap)
    assert bool((_bwd_read(ts, "keys", torch.int64) == -1).all()), f"{what}: key table not clean after prepare"
    live = keys != EMPTY
    assert np.array_equal(slot_of_lookup >= 0, live), f"{what}: dropped lookups"
    slot_key = {}
    for s, k in zip(slot_of_lookup[live].tolist(), keys[live].tolist()):
        assert slot_key.setdefault(s, k) == k, f"{what}: slot {s} holds two keys"
    uk, cnt = np.unique(keys[live], return_counts=True)
    chk = ha.check_placement(slot_key, uk, cap)
    c = _bwd_read(ts, "cnt", torch.int32)
    key_slot = {k: s for s, k in slot_key.items()}
    assert [int(c[key_slot[k]]) for k in uk.tolist()] == cnt.tolist(), f"{what}: lookup counts per slot"
    print(f"{what}: cap {cap}, {uk.size} keys (load {uk.size / cap:.3f}), {chk.displaced} displaced, longest probe "
          f"{chk.longest}, cluster through slot 0: {chk.wraps}")
    return chk


def _kjt_slots(ts, lengths):
    """Global slot of every lookup of the tiled form: lookup i of a chunk starting at j0 belongs to
    chunk entry d = lk[j0 + i] & 0xffff, whose slot is ent_h[j0 + d]."""
    lk = _bwd_read(ts, "lk", torch.int32)
    ent_h = _bwd_read(ts, "ent_h", torch.int32)
    n = int(lengths.sum())
    out = np.full(n, -1, np.int64)
    for j0, m in ha.kjt_chunks(lengths):
        out[j0:j0 + m] = ent_h[j0 + (lk[j0:j0 + m] & 0xFFFF)]
    return out


def _kjt_oracle_check(ts_tw, otab, ost, tper, maps):
    """Rows below HOT_MIN lookups: the tolerances of test_pooled_fwd_and_fused_rowwise_adagrad; hot
    rows: those of test_fused_adagrad_hot_rows."""
    for t, m in enumerate(maps):
        U = m.size
        hot = torch.from_numpy(np.bincount(tper[t], minlength=U + 1) >= ha.HOT_MIN)
        gw, gs = ts_tw.table_view(t)[:U + 1].cpu(), ts_tw.state_view(t)[:U + 1].cpu()
        np.testing.assert_allclose(gw[~hot].numpy(), otab[t][~hot].numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(gs[~hot].numpy(), ost[t][~hot].numpy(), rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(gw[hot].numpy(), otab[t][hot].numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(gs[hot].numpy(), ost[t][hot].numpy(), rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("parts", [(0,), (1, 2)], ids=["whole", "parts"])
@pytest.mark.parametrize("pooling", ["sum", "mean"])
@pytest.mark.parametrize("batch", ["p1_p4", "p5_full_load"])
def test_kjt_form_collisions(ops, device, batch, pooling, parts):
    B, dims, L = ha.KJT_B, [8, 8], ha.KJT_TOTAL
    adv = ops.TableSet(N, dims, [0, 1], device)
    adv.init_uniform_(torch.Generator(device=device).manual_seed(3))
    w0 = adv.weights.clone()
    tw = ops.TableSet(N, dims, [0, 1], device)
    adv.ensure_bwd_workspace(L)
    cap = ha.bwd_cap(adv._bwd_cap)
    assert cap == 4096 and adv._bwd_cap == L == cap // 2
    values, lengths, pats = (ha.kjt_adversarial if batch == "p1_p4" else ha.kjt_full_load)(N, cap, seed=7)
    assert values.size <= adv._bwd_cap
    per = ha.kjt_split(values, lengths, B, 2)
    tper, maps = ha.twin(per, N, drop_zero=False)
    tvalues = np.concatenate(tper)
    offsets = ref.complete_cumsum(lengths)
    _copy_twin_rows(adv, tw, maps)
    otab = [tw.table_view(t)[:maps[t].size + 1].cpu().clone() for t in range(2)]
    ost = [torch.zeros(maps[t].size + 1) for t in range(2)]
    keys = np.concatenate(ha.packed_keys(per, N, ha.pk_key, drop_zero=False))
    V, TV, O = _t(values, device), _t(tvalues, device), _t(offsets, device)
    pool = 1 if pooling == "mean" else 0
    for i in range(2):
        gout = torch.randn(B, sum(dims), generator=torch.Generator().manual_seed(30 + i))
        adv.bwd_prepare(V, O, B, max_lookups=L)
        torch.cuda.synchronize()
        chk = _inspect_bwd(adv, _kjt_slots(adv, lengths), keys, f"KJT form {batch} step {i}")
        assert chk.wraps and chk.longest >= (95 if batch == "p1_p4" else 47)  # P2's cluster through slot 0, P1's chain
        if batch == "p5_full_load":
            assert np.unique(keys).size == cap // 2
        tw.bwd_prepare(TV, O, B, max_lookups=L)
        for p in parts:
            adv.bwd_rowwise_adagrad(gout.to(device), O, B, LR, EPS, pooling=pool, part=p)
            tw.bwd_rowwise_adagrad(gout.to(device), O, B, LR, EPS, pooling=pool, part=p)
        grads = ref.pooled_bwd_dense(otab, [0, 1], torch.from_numpy(tvalues), torch.from_numpy(offsets), B, gout, pooling)
        for t in range(2):
            ref.rowwise_adagrad(otab[t], ost[t], grads[t], LR, EPS)
    torch.cuda.synchronize()
    _assert_twin_rows(adv, tw, maps, f"KJT form {batch}")
    _kjt_oracle_check(tw, otab, ost, tper, maps)
    _assert_untouched(adv, w0, maps, f"KJT form {batch}")
    _assert_touched_moved(adv, maps, f"KJT form {batch}")


def test_kjt_cols_form_collisions(ops, device):
    """tt_bwd_prepare_cols (hash_insert, one probing insert per lookup) with P1-P3 under the KJT-form
    packing; the slot of every lookup is slot_of."""
    B, dims = 1024, [8, 8]
    adv = ops.TableSet(N, dims, [0, 1], device)
    adv.init_uniform_(torch.Generator(device=device).manual_seed(4))
    w0 = adv.weights.clone()
    tw = ops.TableSet(N, dims, [0, 1], device)
    adv.ensure_bwd_workspace(2 * B)
    cap = ha.bwd_cap(adv._bwd_cap)
    assert cap == 4096
    cols = ha.cols_batch(B, N, ha.dedup_patterns(N, cap, ha.pk_key, ha.PK_P3_COUNTS), seed=9)
    tcols, maps = ha.twin(cols, N)
    _copy_twin_rows(adv, tw, maps)
    otab = [tw.table_view(t)[:maps[t].size + 1].cpu().clone() for t in range(2)]
    ost = [torch.zeros(maps[t].size + 1) for t in range(2)]
    keys = np.concatenate(ha.packed_keys(cols, N, ha.pk_key))
    for i in range(2):
        gout = torch.randn(B, sum(dims), generator=torch.Generator().manual_seed(40 + i))
        adv.bwd_prepare_cols([_t(c, device) for c in cols], N)
        torch.cuda.synchronize()
        chk = _inspect_bwd(adv, _bwd_read(adv, "slot_of", torch.int32)[:2 * B].astype(np.int64), keys,
                           f"KJT column form step {i}")
        assert chk.wraps and chk.longest >= 47
        adv.bwd_rowwise_adagrad(gout.to(device), None, B, LR, EPS)
        tw.bwd_prepare_cols([_t(c, device) for c in tcols], N)
        tw.bwd_rowwise_adagrad(gout.to(device), None, B, LR, EPS)
        _oracle_cols(otab, ost, tcols, gout, dims)
    torch.cuda.synchronize()
    _assert_twin_rows(adv, tw, maps, "KJT column form")
    tper = [c[c != 0] for c in tcols]
    _kjt_oracle_check(tw, otab, ost, tper, maps)
    _assert_untouched(adv, w0, maps, "KJT column form")
    _assert_touched_moved(adv, maps, "KJT column form")
