"""tests/hash_adversary.py without a GPU: the families really collide under the restated hash, the
batches keep inside the bounds the workspaces were sized for, the twin keeps the lookup -> group
partition, the placement check rejects a wrong table — and every restated constant is pinned to the
csrc/ text, so a change of the kernels' hash fails HERE (the families must then be re-derived)
instead of quietly turning tests/test_gpu_hash_adversary.py into a test of random ids."""
import re
from pathlib import Path

import numpy as np
import pytest

import hash_adversary as ha

CSRC = Path(__file__).resolve().parents[1] / "two_tower_recommender_model_amd" / "csrc"
N = [ha.N_ROWS, ha.N_ROWS]
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
REDERIVE = "csrc/ no longer matches tests/hash_adversary.py: restate it there and re-derive the families"


def _live(keys):
    k = np.concatenate(keys)
    return k[k != EMPTY]


def _mix_py(x: int) -> int:
    m = (1 << 64) - 1
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & m
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & m
    x ^= x >> 33
    return x


def test_mixer_wraps_like_uint64():
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.integers(0, 1 << 63, 200, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                         np.asarray([0, 1, (1 << 64) - 2, (3 << 40) | 12345], np.uint64)])
    assert ha.mix64(xs).tolist() == [_mix_py(int(x)) for x in xs.tolist()]
    assert int(ha.dd_key(3, 5)[0]) == (3 << 40) | 5 and int(ha.pk_key(3, 5)[0]) == (3 << 34) | 5
    assert [ha.dedup_cap(x) for x in (1, 64, 65, 512, 1024)] == [1024, 1024, 2048, 8192, 16384]
    assert [ha.bwd_cap(x) for x in (1, 2048, 2049)] == [4096, 4096, 8192]


@pytest.mark.parametrize("pack,cap", [(ha.dd_key, 8192), (ha.dd_key, 16384), (ha.pk_key, 4096)])
def test_families_collide(pack, cap):
    p3c = ha.DD_P3_COUNTS if pack is ha.dd_key else ha.PK_P3_COUNTS
    p1, p2, p3 = ha.dedup_patterns(N, cap, pack, p3c)
    assert p1.rows.size >= 48 and np.unique(p1.rows).size == p1.rows.size and p1.rows.min() >= 1
    assert set(ha.home(pack(0, p1.rows), cap).tolist()) == {100}
    h2 = ha.home(pack(0, p2.rows), cap)
    assert sorted(set(h2.tolist())) == [cap - 2, cap - 1] and min(np.bincount(h2)[[cap - 2, cap - 1]]) >= 8
    occ = ha.occupied_slots(pack(0, p2.rows), cap)
    assert cap - 1 in occ and 0 in occ and occ == {(cap - 2 + j) % cap for j in range(p2.rows.size)}
    assert set(ha.home(pack(1, p3.rows), cap).tolist()) == {cap // 2 + 9}
    hot = p3.counts > ha.DD_INL if pack is ha.dd_key else p3.counts >= ha.HOT_MIN
    assert hot.sum() - 1 >= 2 or pack is ha.pk_key  # all but the home's winner are displaced
    if pack is ha.pk_key:
        assert tuple(p3.counts) == (1, 2, 32, 33, 600) and hot.sum() == 2 and p3.counts.max() > ha.HOT_SPLIT
    else:
        assert tuple(p3.counts) == (1, 2, 30, 31, 32, 40) and hot.sum() == 3


def test_family_request_that_cannot_be_met_asserts():
    with pytest.raises(AssertionError, match="at most"):
        ha.family(0, ha.N_ROWS, 8192, 5, ha.MAX_FAMILY + 1)
    with pytest.raises(AssertionError, match="have home slot"):
        ha.family(0, 5000, 8192, 5, 40)


@pytest.mark.parametrize("pack,cap,hs,spans", [(ha.dd_key, 8192, ha.INS_HS, 8), (ha.dd_key, 16384, ha.INS_HS, 16),
                                               (ha.pk_key, 4096, ha.TILE_HS, 2)])
def test_lds_only_family(pack, cap, hs, spans):
    rows = ha.lds_only_family(0, ha.N_ROWS, cap, hs, 7, 128, pack)
    k = pack(0, rows)
    assert np.unique(rows).size == 128 and set(ha.home(k, hs).tolist()) == {7}
    g = np.bincount(ha.home(k, cap), minlength=cap)
    assert (g > 0).sum() == spans >= 2 and g.max() == 128 // spans
    # the LDS chain is 128 long, the global chains 128 / spans
    assert len(ha.occupied_slots(k, hs)) == 128


def test_fused_batches():
    cap = ha.dedup_cap(1024)
    pats = ha.fused_patterns(N, cap)
    for seed in range(4):
        cols = ha.cols_batch(512, N, pats, seed)
        assert all(c.size == 512 for c in cols)
        for p in pats:
            pos = np.nonzero(np.isin(np.mod(cols[p.table], N[p.table]), p.rows) & (cols[p.table] != 0))[0]
            assert pos.size == p.counts.sum(), p.name
            if p.window is not None:  # P4: one ring insert workgroup
                assert pos.min() >= p.window[0] and pos.max() < p.window[1] and p.window == (0, ha.INS_GROUP)
                grp = np.mod(cols[0][:ha.INS_GROUP], N[0])
                assert np.unique(grp).size <= ha.INS_HS // 2
            else:  # strided: several waves and, for table 1, both insert workgroups
                assert np.unique(pos // 64).size >= 4, p.name
                if p.table == 1:
                    assert np.unique(pos // ha.INS_GROUP).size == 2
        assert all(int((c == 0).sum()) >= 4 for c in cols)
        assert all((c < 0).any() and (c >= n).any() for c, n in zip(cols, N))  # ids that need the floor-mod
        assert all(np.abs(c).max() < 2 ** 31 for c in cols)                     # and fit int32
        occ = ha.occupied_slots(_live(ha.packed_keys(cols, N, ha.dd_key)), cap)
        assert cap - 1 in occ and 0 in occ


def test_dedup_batch_and_placement_check():
    cap = ha.dedup_cap(512)
    assert cap == 8192
    pats = ha.dedup_patterns(N, cap)
    cols = ha.cols_batch(256, N, pats, seed=1)
    keys = _live(ha.packed_keys(cols, N, ha.dd_key))
    assert keys.size + sum(int((c == 0).sum()) for c in cols) == 512
    uk = np.unique(keys)
    rng = np.random.default_rng(3)
    tabs = []
    for _ in range(3):  # sequential inserts in three orders: one slot set, different placements
        slot_key = {}
        for k in uk[rng.permutation(uk.size)].tolist():
            h = int(ha.home([k], cap)[0])
            while h in slot_key:
                h = (h + 1) % cap
            slot_key[h] = k
        chk = ha.check_placement(slot_key, keys, cap)
        assert chk.wraps and chk.longest >= 47 and chk.displaced >= 47 + 14 + 5
        tabs.append(slot_key)
    assert set(tabs[0]) == set(tabs[1]) == set(tabs[2]) and tabs[0] != tabs[1]
    # a key moved in front of its home, a key lost, a key filed twice: each is rejected
    bad = dict(tabs[0])
    k = bad.pop(cap - 1)
    bad[cap - 3] = k
    with pytest.raises(AssertionError):
        ha.check_placement(bad, keys, cap)
    bad = dict(tabs[0])
    s_p1 = [s for s, k in bad.items() if s in range(100, 148)]
    bad[s_p1[0]] = bad[s_p1[1]]
    with pytest.raises(AssertionError, match="missing from the table or sits in two"):
        ha.check_placement(bad, keys, cap)
    bad = dict(tabs[0])
    last = max(s for s in bad if 100 <= s < 400 and all(j in bad for j in range(100, s + 1)))
    bad[last + 2] = bad.pop(last)  # split cluster: its probe path crosses a free slot
    with pytest.raises(AssertionError):
        ha.check_placement(bad, keys, cap)


def test_kjt_batches():
    cap = ha.bwd_cap(ha.KJT_TOTAL)
    assert cap == 4096 and ha.KJT_TOTAL == cap // 2
    for seed in (0, 1):
        values, lengths, pats = ha.kjt_adversarial(N, cap, seed)
        assert values.size == lengths.sum() == ha.KJT_TOTAL and lengths.min() == 0
        tile = np.zeros(lengths.size, bool)
        tile[ha.KJT_P4_TILE * 16:(ha.KJT_P4_TILE + 1) * 16] = True
        assert (lengths[tile] == 64).all() and 10 <= lengths[~tile].max() <= 20
        per = ha.kjt_split(values, lengths, ha.KJT_B, 2)
        keys = np.concatenate(ha.packed_keys(per, N, ha.pk_key, drop_zero=False))
        chunks = ha.kjt_chunks(lengths)
        for j0, n in chunks:
            assert n <= ha.TILE_CH and np.unique(keys[j0:j0 + n]).size <= ha.TILE_HS // 2
        p4, p1b, p1, p2, p3 = pats
        lo, hi = p4.window
        assert (lo, hi - lo) in chunks and hi - lo == ha.TILE_CH  # the tile is exactly one full chunk
        inside = per[0][lo:hi]
        assert np.isin(p4.rows, inside).all() and np.isin(p1b.rows, inside).all() and not np.isin(p4.rows, per[1]).any()
        assert np.unique(inside).size > 768  # every thread of the workgroup holds 3 or 4 chunk entries
        k4 = ha.pk_key(0, p4.rows)
        assert set(ha.home(k4, ha.TILE_HS).tolist()) == {11} and np.unique(ha.home(k4, cap)).size == 2
        both = np.concatenate([p1.rows, p1b.rows])
        assert np.unique(both).size == 96 and set(ha.home(ha.pk_key(0, both), cap).tolist()) == {100}
        pos = np.nonzero(np.isin(per[0], p1.rows))[0]
        assert ((pos < lo) | (pos >= hi)).sum() >= 24  # the second family comes from other workgroups
        assert [int((per[1] == r).sum()) for r in p3.rows] == list(ha.PK_P3_COUNTS)
        occ = ha.occupied_slots(keys, cap)
        assert cap - 1 in occ and 0 in occ and all((100 + j) in occ for j in range(96))


def test_kjt_full_load():
    cap = ha.bwd_cap(2048)
    values, lengths, pats = ha.kjt_full_load(N, cap, seed=4)
    per = ha.kjt_split(values, lengths, ha.KJT_B, 2)
    keys = np.concatenate(ha.packed_keys(per, N, ha.pk_key, drop_zero=False))
    assert keys.size == cap // 2 and np.unique(keys).size == cap // 2  # the designed maximum load, all distinct
    for p in pats:
        assert np.isin(p.rows, per[p.table]).all()
    occ = ha.occupied_slots(keys, cap)
    assert len(occ) == cap // 2 and cap - 1 in occ and 0 in occ


def test_twin_preserves_partition():
    cap = ha.dedup_cap(1024)
    pats = ha.fused_patterns(N, cap)
    steps = [ha.cols_batch(512, N, pats, seed) for seed in range(3)]
    cat = [np.concatenate([s[t] for s in steps]) for t in range(2)]
    tw, maps = ha.twin(cat, N)
    for t in range(2):
        f0, c0 = ha.partition(cat[t], N[t])
        f1, c1 = ha.partition(tw[t], N[t])
        assert np.array_equal(f0, f1) and np.array_equal(c0, c1)          # same groups: first positions and sizes
        assert np.array_equal((cat[t] == 0), (tw[t] == 0))                # dropped stays dropped, kept never becomes 0
        U = maps[t].size
        assert np.unique(maps[t]).size == U == np.unique(tw[t][tw[t] != 0]).size  # no two families merged
        assert tw[t][tw[t] != 0].min() == 1 and tw[t].max() == U
        kept = cat[t] != 0
        assert np.array_equal(maps[t][tw[t][kept] - 1], np.mod(cat[t][kept], N[t]))
    # KJT form: id 0 is row 0, a kept lookup
    values, lengths, _ = ha.kjt_adversarial(N, 4096, 0)
    per = ha.kjt_split(values, lengths, ha.KJT_B, 2)
    tw, maps = ha.twin(per, N, drop_zero=False)
    for t in range(2):
        assert (per[t] == 0).any() and tw[t].min() == 1
        f0, c0 = ha.partition(per[t], N[t], drop_zero=False)
        f1, c1 = ha.partition(tw[t], N[t], drop_zero=False)
        assert np.array_equal(f0, f1) and np.array_equal(c0, c1)
        assert np.array_equal(maps[t][tw[t] - 1], per[t])


# ---- the restatements against the source text ---------------------------------------------------------


def _src(name: str) -> str:
    return (CSRC / name).read_text()


def _const(text: str, name: str) -> int:
    m = re.search(r"constexpr int %s = (\d+);" % name, text)
    assert m, f"{name}: {REDERIVE}"
    return int(m.group(1))


@pytest.mark.parametrize("fname,func", [("dedup.h", "dd_mix64"), ("embedding.hip", "mix64")])
def test_mixer_pinned_to_source(fname, func):
    m = re.search(r"uint64_t %s\(uint64_t x\) \{(.*?)\n\}" % func, _src(fname), re.S)
    assert m, REDERIVE
    body = [ln.strip() for ln in m.group(1).strip().splitlines()]
    assert body == ["x ^= x >> %d;" % ha.MIX_SHIFT, "x *= 0x%xull;" % ha.MIX_MUL1, "x ^= x >> %d;" % ha.MIX_SHIFT,
                    "x *= 0x%xull;" % ha.MIX_MUL2, "x ^= x >> %d;" % ha.MIX_SHIFT, "return x;"], REDERIVE
    assert ha.MIX_SHIFT == 33 and ha.MIX_MUL1 == 0xFF51AFD7ED558CCD and ha.MIX_MUL2 == 0xC4CEB9FE1A85EC53


def test_constants_pinned_to_source():
    dh, dc, eh, th = _src("dedup.h"), _src("dedup.hip"), _src("embedding.hip"), _src("tower_tail.hip")
    for text, names in ((dh, ("DD_TABLE_SHIFT", "DD_CNT_BITS", "DD_INL")),
                        (eh, ("PK_ROW_BITS", "PK_CNT_BITS", "HOT_MIN", "HOT_SPLIT", "TILE_BAGS", "TILE_CH", "TILE_HS")),
                        (th, ("INS_HS",))):
        for name in names:
            assert _const(text, name) == getattr(ha, name), f"{name}: {REDERIVE}"
    assert (ha.DD_TABLE_SHIFT, ha.PK_ROW_BITS, ha.DD_CNT_BITS, ha.PK_CNT_BITS) == (40, 34, 18, 24)
    assert (ha.DD_INL, ha.HOT_MIN, ha.INS_HS, ha.TILE_HS, ha.TILE_CH) == (30, 33, 1024, 2048, 1024)
    # one lookup per thread of a 256-thread insert workgroup
    assert re.search(r"#define TT_INS_PT 1\b", th) and ha.INS_GROUP == 256, REDERIVE
    # key packings
    assert "<< DD_TABLE_SHIFT) | (uint64_t)py_mod64(id, ca.num_emb[f])" in dc, REDERIVE
    assert "return ((uint64_t)t << PK_ROW_BITS) | row;" in eh, REDERIVE
    # home slots: hash & (slots - 1), linear probing with wrap
    for text, needles in ((dh, ("dd_mix64(key) & ((uint64_t)ws.cap - 1)", "h = (h + 1) & mask;")),
                          (th, ("dd_mix64(key[u]) & (INS_HS - 1)", "h = (h + 1) & (INS_HS - 1);",
                                "dd_mix64(key[u]) & mask", "g = (g + 1) & mask;")),
                          (eh, ("mix64(pk) & mask", "mix64(key) & (TILE_HS - 1)", "h = (h + 1) & (TILE_HS - 1);",
                                "mix64(ekey[q]) & gmask", "(eh[q] + 1) & gmask"))):
        for s in needles:
            assert s in text, f"{s!r}: {REDERIVE}"
    # capacity rules: minimum and factor
    m = re.search(r"static int64_t dedup_cap\(int64_t L\) \{\s*int64_t c = (\d+);\s*while \(c < (\d+) \* L\) c <<= 1;", dc)
    assert m and (int(m.group(1)), int(m.group(2))) == (ha.DEDUP_CAP_MIN, ha.DEDUP_CAP_FACTOR) == (1024, 16), REDERIVE
    m = re.search(r"static int64_t bwd_cap\(int64_t L\) \{\s*int64_t c = SCAN_TILE;\s*while \(c < (\d+) \* L\) c <<= 1;", eh)
    assert m and (_const(eh, "SCAN_TILE"), int(m.group(1))) == (ha.BWD_CAP_MIN, ha.BWD_CAP_FACTOR) == (4096, 2), REDERIVE
