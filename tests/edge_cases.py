"""Generators and comparison routines of the edge-case tests (test infrastructure; CPU only, no
GPU call in this module — the GPU tests feed what the kernels gave into the routines below, and
tests/test_cpu_edge_cases.py checks on the CPU that every routine rejects a wrong value).

Windowed ids (bounds-check mode). ``WindowSpec`` describes a TableSet of five equal tables of which a
window TableSet sees tables 1 and 3; an id outside [0, R) of a window table is drawn from [-R, 0) or
[R, 2R), so a read or write that a broken check lets through lands in a neighbouring pad table of the
SAME allocation instead of outside it.

Multiplicity ladder. ``LADDER`` holds the lookup counts per row around every point where the update
kernels change algorithm (dedup.h DD_INL = 30; embedding.hip HOT_MIN = 33, HOT_NR_MAX = 64,
HOT_SPLIT = 512; the "<= 14 ascending" rule; one row above DD_HOT_CH = 4096; two tables of 7168
lookups exceed HOT_WIN = 8192)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch

from oracle import ref

# ---- windowed ids ---------------------------------------------------------------------------------

WINDOW_TABLES = (1, 3)
NUM_SRC_TABLES = 5


@dataclass
class WindowSpec:
    R: int
    D: int
    align: int = 4

    def __post_init__(self):
        assert self.R % 4 == 0, "R a multiple of 4: every weight offset is exact for odd D too"

    @property
    def weight_offsets(self) -> List[int]:
        per = (self.R * self.D + self.align - 1) // self.align * self.align
        return [t * per for t in range(NUM_SRC_TABLES)]

    @property
    def total_weights(self) -> int:
        per = (self.R * self.D + self.align - 1) // self.align * self.align
        return NUM_SRC_TABLES * per


@dataclass
class WindowBatch:
    lengths: np.ndarray   # int32 [2 * B]
    offsets: np.ndarray   # int32 [2 * B + 1]
    values: np.ndarray    # ids of the window's two features (key-major), out-of-range ones included
    clamped: np.ndarray   # the same with every out-of-range id replaced by 0
    n_oob: int
    maxlen: int


def windowed_batch(spec: WindowSpec, B: int = 96, maxlen: int = 9, oob_frac: float = 0.15, seed: int = 0,
                   dtype=np.int64, lone_row0: bool = False) -> WindowBatch:
    """A 2-feature KJT over the window's tables: bags of 0..maxlen ids, ~oob_frac of them outside
    [0, R). Feature 0: bag 0 is entirely out of range, bag 1 holds in-range row 0 beside out-of-range
    ids. ``lone_row0``: feature 1 never looks row 0 up in range and holds exactly ONE out-of-range id,
    so the only lookup of its row 0 is that id (the grouping hash files it under row 0 with count 1
    and the direct once-looked-up update must clamp it to the same row)."""
    rng = np.random.default_rng(seed)
    R = spec.R
    lengths = rng.integers(0, maxlen + 1, 2 * B).astype(np.int32)
    lengths[0], lengths[1] = 3, 4
    if lone_row0:
        lengths[B + 2] = max(2, lengths[B + 2])
    offsets = ref.complete_cumsum(lengths)
    n = int(offsets[-1])
    values = rng.integers(0, R, n).astype(np.int64)
    oob = rng.random(n) < oob_frac
    far = np.where(rng.random(n) < 0.5, rng.integers(-R, 0, n), rng.integers(R, 2 * R, n))
    f1 = np.arange(n) >= offsets[B]
    if lone_row0:
        values[f1] = rng.integers(1, R, int(f1.sum()))
        oob[f1] = False
        oob[offsets[B + 2] + 1] = True
    values = np.where(oob, far, values)
    # feature 0, bag 0: every id out of range (one below 0, the largest and the smallest above)
    values[offsets[0]:offsets[1]] = [-1, 2 * R - 1, R]
    # feature 0, bag 1: in-range row 0 beside out-of-range ids
    values[offsets[1]:offsets[2]] = [0, -R, 5 % R, R + 1]
    is_oob = (values < 0) | (values >= R)
    return WindowBatch(lengths, offsets, values.astype(dtype), np.where(is_oob, 0, values).astype(dtype),
                       int(is_oob.sum()), int(lengths.max()))


def window_in_allocation(spec: WindowSpec, batch: WindowBatch) -> bool:
    """Every id of the batch, taken UNCHECKED, still addresses a whole row inside the source
    TableSet's weight buffer."""
    B = batch.lengths.size // 2
    feat = np.repeat(np.arange(2 * B) // B, batch.lengths)
    woff = np.asarray(spec.weight_offsets, np.int64)[np.asarray(WINDOW_TABLES)[feat]]
    ids = batch.values.astype(np.int64)
    lo = woff + ids * spec.D
    hi = woff + (ids + 1) * spec.D
    return bool((lo >= 0).all() and (hi <= spec.total_weights).all())


def assert_pooled_close(got, want, maxlen: int) -> None:
    """tt_pooled_fwd's tolerance (tests/test_gpu_ops.py): rtol 1e-5, atol 1e-6 x the longest bag."""
    np.testing.assert_allclose(np.asarray(got), np.asarray(want), rtol=1e-5, atol=1e-6 * max(1, maxlen))


def assert_adagrad_close(got_w, got_s, want_w, want_s, w_rtol=1e-5, w_atol=1e-6, s_rtol=1e-5, s_atol=1e-9) -> None:
    """The fused row-wise Adagrad tolerances of tests/test_gpu_ops.py (defaults) / test_gpu_dedup.py."""
    np.testing.assert_allclose(np.asarray(got_s), np.asarray(want_s), rtol=s_rtol, atol=s_atol)
    np.testing.assert_allclose(np.asarray(got_w), np.asarray(want_w), rtol=w_rtol, atol=w_atol)


def assert_bitwise(got: torch.Tensor, want: torch.Tensor, what: str = "") -> None:
    """Same dtype, shape and bits (NaN payloads and the sign of zero included)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a = got.detach().cpu().contiguous().reshape(-1).view(torch.uint8)
    b = want.detach().cpu().contiguous().reshape(-1).view(torch.uint8)
    if not torch.equal(a, b):
        n = int((got.detach().cpu() != want.detach().cpu()).sum())
        raise AssertionError(f"{what}: not bitwise equal ({n} elements differ in value)")


def assert_ints_equal(got, want, what: str = "") -> None:
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg=what)


# ---- multiplicity ladder --------------------------------------------------------------------------

LADDER = (1, 2, 3, 13, 14, 15, 16, 29, 30, 31, 32, 33, 34, 63, 64, 65, 511, 512, 513, 1025, 4097)
LADDER_LOOKUPS = 7103
LADDER_B = 7168
# every fixed lookup count at which an update kernel changes algorithm and that the ladder brackets
# with t - 1, t, t + 1: the "<= 14 ascending" rule, DD_INL, HOT_MIN, HOT_NR_MAX, HOT_SPLIT
LADDER_THRESHOLDS = (14, 30, 33, 64, 512)


def ladder_rows(N: int, seed: int) -> np.ndarray:
    """The 21 distinct rows of a table of N rows that carry the ladder's counts; row 0 is one."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(np.arange(1, N), size=len(LADDER) - 1, replace=False)
    rows = np.concatenate([[0], rows])
    return rows[rng.permutation(len(LADDER))].astype(np.int64)


def ladder_cols(N: Sequence[int], seed: int = 0, dtype=torch.int64) -> List[torch.Tensor]:
    """One [LADDER_B] single-hot id column per table: row ladder_rows(n)[k] is looked up exactly
    LADDER[k] times, ids 0 (dropped) pad the column, the order is a seeded permutation and every id
    is moved by a multiple of n (negative ones too), so the row is id floor-mod n."""
    cols = []
    for t, n in enumerate(N):
        rng = np.random.default_rng(1000 * seed + t)
        rows = np.repeat(ladder_rows(n, 1000 * seed + t), LADDER)
        shift = rng.integers(-2, 3, rows.size)
        ids = rows + shift * n
        ids = np.where(ids == 0, n, ids)  # row 0 unshifted would be the dropped id
        col = np.zeros(LADDER_B, np.int64)
        col[:ids.size] = ids
        cols.append(torch.from_numpy(col[rng.permutation(LADDER_B)]).to(dtype))
    return cols


def ladder_histogram(col: torch.Tensor, n: int) -> np.ndarray:
    """Lookups per row of one column (id 0 dropped, id floor-mod n)."""
    c = col.numpy().astype(np.int64)
    return np.bincount(np.mod(c[c != 0], n), minlength=n)


def ladder_kjt(N: Sequence[int], B: int = 2048, seed: int = 0):
    """The ladder's lookups as multi-hot bags: per feature, the column's kept lookups (rows, in the
    column's order) cut into bags of 1..8 ids, 40 of the hottest row's lookups in ONE bag, empty
    bags up to B, the bag order a seeded permutation. Returns (values int64, lengths int32 [2 * B])."""
    cols = ladder_cols(N, seed)
    vals, lens = [], []
    for t, n in enumerate(N):
        rng = np.random.default_rng(7000 + 1000 * seed + t)
        c = cols[t].numpy()
        rows = np.mod(c[c != 0], n)
        hot = int(np.argmax(np.bincount(rows, minlength=n)))
        idx = np.nonzero(rows == hot)[0][:40]
        rest = np.delete(rows, idx)
        bags, i = [], 0
        while i < rest.size:
            k = int(rng.integers(1, 9))
            bags.append(rest[i:i + k])
            i += k
        bags.append(np.full(40, hot, np.int64))
        assert len(bags) <= B
        bags += [np.zeros(0, np.int64)] * (B - len(bags))
        order = rng.permutation(B)
        bags = [bags[j] for j in order]
        lens.append(np.asarray([b.size for b in bags], np.int32))
        vals.append(np.concatenate(bags))
    return np.concatenate(vals).astype(np.int64), np.concatenate(lens)


def adagrad_lookups_fp64(tables: Sequence[torch.Tensor], states: Sequence[torch.Tensor], rows: Sequence[torch.Tensor],
                         grad_rows: Sequence[torch.Tensor], lr: float, eps: float) -> None:
    """One fused row-wise Adagrad step of the oracle in fp64, in place on fp64 tables / states:
    lookup j of table t adds grad_rows[t][j] to row rows[t][j]."""
    for t in range(len(tables)):
        ref.rowwise_adagrad_from_lookups(tables[t], states[t], rows[t], grad_rows[t].double(), lr, eps)


def cols_lookups(cols: Sequence[torch.Tensor], N: Sequence[int], gout: torch.Tensor, dims: Sequence[int]):
    """(rows, gradient rows) per table of single-hot columns: feature t -> table t, lookup b reads
    gout[b, columns of feature t]."""
    rows, grads, o = [], [], 0
    for c, n, d in zip(cols, N, dims):
        c = c.to(torch.int64)
        keep = c != 0
        rows.append(torch.remainder(c[keep], n))
        grads.append(gout[keep, o:o + d])
        o += d
    return rows, grads


def kjt_lookups(values: np.ndarray, lengths: np.ndarray, B: int, gout: torch.Tensor, dims: Sequence[int],
                mean: bool):
    """(rows, gradient rows) per feature of a key-major KJT: a lookup of bag b reads gout[b, columns
    of the feature], divided by the bag's length for MEAN pooling."""
    offs = ref.complete_cumsum(lengths).astype(np.int64)
    rows, grads, o = [], [], 0
    for f, d in enumerate(dims):
        ln = torch.from_numpy(lengths[f * B:(f + 1) * B].astype(np.int64))
        bag = torch.repeat_interleave(torch.arange(B), ln)
        g = gout[bag, o:o + d].double()
        if mean:
            g = g / ln[bag].clamp(min=1).unsqueeze(1).double()
        rows.append(torch.from_numpy(values[offs[f * B]:offs[(f + 1) * B]].astype(np.int64)))
        grads.append(g)
        o += d
    return rows, grads


# ---- the dedup workspace is clean between steps ----------------------------------------------------


def assert_clean(ts) -> None:
    """After every update the workspace is clean: every slot free, hot-row counters zero, no
    deferred insert pending (dedup.hip dedup_layout: slots, keys, hot list, counters, claims,
    overflow entries)."""
    L = ts._dd_cap
    cap = 1024
    while cap < 16 * L:
        cap <<= 1
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    sl = ts._dd_ws[:cap * 128].view(torch.int64).view(cap, 16).cpu()  # 128-B slots
    assert bool((sl[:, 0] == -1).all())
    o = cap * 128 + al(8 * L) + al(4 * (L // 31 + 1))
    assert ts._dd_ws[o:o + 16].view(torch.int32).cpu().tolist() == [0, 0, 0, 0]
    o_ovf = o + 256 + al(4 * L)
    G = (L + 63) // 64
    ovf = ts._dd_ws[o_ovf:o_ovf + 16 * 64 * G].view(torch.int64).view(G * 64, 2).cpu()
    assert bool((ovf[:, 0] == -1).all())


# ---- KJT glue batches -----------------------------------------------------------------------------


def single_hot_kjt(rng, F: int, B: int, N: Sequence[int], dtype=np.int64, empty_frac: float = 0.1):
    """Bags of 0 or 1 ids (~empty_frac empty), values in [0, N_f) with 0 and N_f - 1 present in every
    feature. Returns (values, offsets int32 [F*B + 1])."""
    lengths = (rng.random(F * B) >= empty_frac).astype(np.int32)
    vals = []
    for f in range(F):
        k = int(lengths[f * B:(f + 1) * B].sum())
        v = rng.integers(0, N[f], k, dtype=np.int64)
        v[0], v[1] = 0, N[f] - 1
        vals.append(v)
    return np.concatenate(vals).astype(dtype), ref.complete_cumsum(lengths)
