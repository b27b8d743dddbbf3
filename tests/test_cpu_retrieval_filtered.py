"""tt_topk_mips_filtered without a GPU: its limits come back as status codes before any launch, the
entry-point bookkeeping, ops.pack_allow_mask and ops.sort_exclusions on hand-worked inputs, and the
conditions under which the GPU cases (tests/retrieval_filter_oracle.py) mean something: on fp64
scores nearly every query's filtered list differs from its unfiltered one, and the exact rule rejects
the wrong answers a filter can give."""
import pytest
import torch

import retrieval_filter_oracle as fo
import retrieval_oracle as ro

FAKE = 1 << 20  # never dereferenced: every call here must return before any launch
F32, BF16 = 2, 3


@pytest.fixture(scope="module")
def lib():
    from two_tower_recommender_model_amd import _lib
    from two_tower_recommender_model_amd.build import build

    build()
    return _lib.load()


def _call(lib, M=8, N=100, E=64, k=10, splits=0, q_dtype=F32, c_dtype=F32, ldq=None, ldc=None, queries=FAKE,
          items=FAKE, ids=FAKE, scores=FAKE, ws=FAKE, ws_bytes=None, allow=FAKE, values=FAKE, offsets=FAKE):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    rc = lib.tt_topk_mips_filtered(queries, q_dtype, E if ldq is None else ldq, items, c_dtype, E if ldc is None else ldc,
                                   None, M, N, E, k, splits, allow, values, offsets, ids, scores, ws, ws_bytes, None)
    return rc, lib.tt_last_error_string().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(E=0), "E must"), (dict(E=16), "E must"), (dict(E=48), "E must"), (dict(E=160), "E must"), (dict(E=-32), "E must"),
    (dict(k=0), "k must"), (dict(k=257), "k must"), (dict(k=-1), "k must"),
    (dict(M=0), "M must"), (dict(M=-5), "M must"),
    (dict(N=0), "N must"), (dict(N=1 << 31), "N must"), (dict(N=-1), "N must"),
    (dict(splits=-1), "splits must"), (dict(splits=65), "splits must"),
    (dict(q_dtype=0), "q_dtype"), (dict(c_dtype=1), "c_dtype"),
    (dict(ldq=63), "ldq"), (dict(ldc=32), "ldc"),
    (dict(queries=None), "null"), (dict(items=None), "null"), (dict(ids=None), "null"), (dict(scores=None), "null"),
    (dict(ws=None), "null"), (dict(ws_bytes=8 * 10 * 8 - 1, splits=1), "ws_bytes"),
    (dict(values=None), "excl_values"), (dict(offsets=None), "excl_offsets"),
    (dict(values=None, allow=None), "excl_values"), (dict(offsets=None, allow=None), "excl_offsets"),
])
def test_limits_are_status_codes(lib, kw, word):
    rc, msg = _call(lib, **kw)
    assert rc == 1001, (kw, rc)
    assert msg.startswith("tt_topk_mips_filtered:") and word in msg, (kw, msg)


def test_entry_point_is_counted(lib):
    from two_tower_recommender_model_amd import _lib

    assert "tt_topk_mips_filtered" in _lib.COMPUTE_ENTRY_POINTS and "tt_topk_mips_filtered" in _lib.SIGNATURES
    assert lib.tt_num_entry_points() == len(_lib.COMPUTE_ENTRY_POINTS) == 55
    assert lib.tt_abi_version() == 4


# ---- ops.pack_allow_mask / ops.sort_exclusions ----------------------------------------------------


def _u32(words):
    return [int(w) & 0xFFFFFFFF for w in words.tolist()]


def test_pack_allow_mask_hand_worked():
    from two_tower_recommender_model_amd.ops import pack_allow_mask

    t = torch.tensor
    assert _u32(pack_allow_mask(t([True]))) == [1] and _u32(pack_allow_mask(t([False]))) == [0]
    assert _u32(pack_allow_mask(torch.ones(31, dtype=torch.bool))) == [0x7FFFFFFF]
    assert _u32(pack_allow_mask(torch.ones(32, dtype=torch.bool))) == [0xFFFFFFFF]
    assert _u32(pack_allow_mask(torch.ones(33, dtype=torch.bool))) == [0xFFFFFFFF, 1]
    m = torch.zeros(33, dtype=torch.bool)
    m[[0, 5, 31, 32]] = True
    assert _u32(pack_allow_mask(m)) == [0x80000021, 1]
    m = torch.zeros(32, dtype=torch.bool)
    m[31] = True
    w = pack_allow_mask(m)
    assert w.dtype == torch.int32 and w.tolist() == [-(1 << 31)]


@pytest.mark.parametrize("N", [1, 31, 32, 33, 1037])
def test_pack_allow_mask_bit_by_bit(N):
    from two_tower_recommender_model_amd.ops import pack_allow_mask

    mask = torch.rand(N, generator=torch.Generator().manual_seed(N)) < 0.5
    mask[N - 1] = True
    w = pack_allow_mask(mask)
    assert w.dtype == torch.int32 and w.shape == ((N + 31) // 32,) and w.is_contiguous()
    u = _u32(w)
    for n in range(((N + 31) // 32) * 32):
        assert (u[n >> 5] >> (n & 31)) & 1 == (int(mask[n]) if n < N else 0), n
    with pytest.raises(Exception):
        pack_allow_mask(mask.to(torch.int32))


def test_sort_exclusions_hand_worked():
    from two_tower_recommender_model_amd.ops import sort_exclusions

    N = 10
    # segments [5, 1, 5, 3] | [] | [9, 0] | [] | [2]; duplicates stay, empty segments stay empty
    vals = torch.tensor([5, 1, 5, 3, 9, 0, 2], dtype=torch.int64)
    offs = torch.tensor([0, 4, 4, 6, 6, 7], dtype=torch.int64)
    out = sort_exclusions(vals, offs, N)
    assert out.dtype == torch.int32 and out.tolist() == [1, 3, 5, 5, 0, 9, 2]
    # values outside [0, N) become N (no item) and sort last in their segment
    out = sort_exclusions(torch.tensor([11, 4, -1, 10, 0, 2 ** 31 - 1, 3]), torch.tensor([0, 5, 7]), N)
    assert out.tolist() == [0, 4, 10, 10, 10, 3, 10]
    # offsets that do not start at 0 (and do not end at the end): the same offsets serve the output,
    # positions outside every segment stay outside
    vals = torch.tensor([8, 2, 7, 6, 1, 3, 0, 9, 4], dtype=torch.int32)
    offs = torch.tensor([2, 5, 5, 7], dtype=torch.int64)
    out = sort_exclusions(vals, offs, N).tolist()
    assert out[2:5] == [1, 6, 7] and out[5:7] == [0, 3]
    assert sorted(out[:2]) == [2, 8] and sorted(out[7:]) == [4, 9]
    # no values at all
    assert sort_exclusions(torch.zeros(0, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), N).numel() == 0


@pytest.mark.parametrize("N", [1, 31, 32, 33, 1037])
def test_sort_exclusions_against_python(N):
    from two_tower_recommender_model_amd.ops import sort_exclusions

    g = torch.Generator().manual_seed(N)
    lens = torch.randint(0, 9, (20,), generator=g).tolist()
    lens[3] = lens[4] = 0
    lists = [torch.randint(-2, N + 2, (n,), generator=g).tolist() for n in lens]
    vals, offs = fo.csr(lists, lead=3)
    out = sort_exclusions(vals, offs, N).tolist()
    for m, l in enumerate(lists):
        want = sorted(x if 0 <= x < N else N for x in l)
        assert out[int(offs[m]):int(offs[m + 1])] == want, m


def test_topk_mips_rejects_cpu_filters():
    from two_tower_recommender_model_amd import _lib, ops

    with pytest.raises(_lib.TTError):
        ops.topk_mips(torch.zeros(4, 32), torch.zeros(8, 32), 2, allow=torch.zeros(1, dtype=torch.int32))


# ---- the oracle's own conditions ----------------------------------------------------------------


@pytest.mark.parametrize("name", list(fo.CASES))
def test_filtered_cases_are_not_vacuous(name):
    """On the fp64 scores at least 75 % of a case's queries have a filtered expected list that differs
    from their unfiltered one, and the exact answer passes its own rule."""
    c = fo.CASES[name]()
    s, _ = ro.exact_scores(c["Q"], c["Cm"])
    M, N = s.shape
    elig = fo.eligibility(M, N, c["allow"], c["lists"])
    frac = fo.differs_fraction(s, elig, c["k"])
    print(f"{name}: {frac:.3f} of the queries differ")
    assert frac >= 0.75, frac
    s32 = s.to(torch.float32)
    ids, sc = fo.expected_filtered(s32, elig, c["k"])
    fo.check_exact(ids, sc, s32, elig, c["k"])
    if c["lists"] is not None and not name.startswith("monotone_reverse"):
        top = fo.top_half(c["Q"], c["Cm"], c["k"])
        assert all(set(l) & set(t) for l, t in zip(c["lists"], top) if l), "a list misses its query's top k / 2"


def test_list_shapes_case_has_every_shape():
    c = fo.case_list_shapes()
    N, k = c["Cm"].shape[0], c["k"]
    lens = [len(l) for l in c["lists"]]
    assert 0 in lens and 1 in lens and N in lens and max(lens) == N
    assert any(len(set(l)) < len(l) for l in c["lists"])  # duplicates
    assert any(min(l) < 0 and max(l) >= N for l in c["lists"] if l)  # out of range, both sides
    assert any({fo.SPLIT2_BOUNDARY - 1, fo.SPLIT2_BOUNDARY} <= set(l) for l in c["lists"] if len(l) < N // 2)
    left = fo.eligibility(len(lens), N, None, c["lists"]).sum(1)
    assert (left == 0).any() and ((left > 0) & (left < k)).any()


def test_exact_rule_rejects_wrong_answers():
    c = fo.case_list_shapes()
    k = c["k"]
    s = ro.exact_scores(c["Q"], c["Cm"])[0].to(torch.float32)
    M, N = s.shape
    elig = fo.eligibility(M, N, None, c["lists"])
    ids, sc = fo.expected_filtered(s, elig, k)
    fo.check_exact(ids, sc, s, elig, k)
    m = 2  # a query with a long list and more than k items left
    denied = int((~elig[m]).nonzero()[0])
    with pytest.raises(AssertionError, match="denied item was returned"):
        bad_i, bad_s = ids.clone(), sc.clone()
        bad_i[m, 0], bad_s[m, 0] = denied, s[m, denied]
        fo.check_exact(bad_i, bad_s, s, elig, k)
    with pytest.raises(AssertionError, match="displaced"):
        # what a post-filter of the unfiltered top k gives: the denied ones' places are lost, the
        # list is the eligible part of the unfiltered list followed by worse items than it should hold
        un_i = ro.expected_topk(s, k)[0][m]
        kept = un_i[elig[m, un_i]]
        worse = torch.sort(torch.where(elig[m], s[m], torch.full_like(s[m], fo.NEG_INF)), descending=True).indices[k + 50:]
        bad_i, bad_s = ids.clone(), sc.clone()
        bad_i[m] = torch.cat([kept, worse[:k - kept.numel()]])
        bad_s[m] = s[m, bad_i[m]]
        assert kept.numel() < k
        fo.check_exact(bad_i, bad_s, s, elig, k)
    m = 6  # fewer than k eligible
    n_left = int(elig[m].sum())
    assert 0 < n_left < k
    with pytest.raises(AssertionError, match="tail"):
        bad_i, bad_s = ids.clone(), sc.clone()
        bad_i[m, n_left:], bad_s[m, n_left:] = ids[m, 0], sc[m, 0]  # padded with an eligible item instead of -1
        fo.check_exact(bad_i, bad_s, s, elig, k)
    with pytest.raises(AssertionError, match="score bits"):
        fo.check_exact(ids, torch.where(ids >= 0, sc + 1e-3, sc), s, elig, k)
