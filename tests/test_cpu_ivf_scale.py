"""The IVF scale cases without a GPU: importing tests/ivf_scale_cases.py runs its assertions (every case
still reaches the branch of csrc/ivf.hip it is in the table for), the [M, L] eligibility helper equals
the [M, N, nprobe] one, and the host restatements agree with a direct count."""
import torch

import ivf_cases as ic
import ivf_scale_cases as sc


def test_table_is_imported_and_consistent():
    assert [c.id for c in sc.CASES] == ["many-lists", "l-1024", "l-1025", "l-max"]
    for c in sc.CASES:
        sc.check_case(c)
        assert sc.assignment(c.id).shape == (c.N,) and sc.assignment(c.id).dtype == torch.int64
    # the restated constants carry the cases: with a scan width of 2048, l-1025 would not reach per = 2
    assert sc.IVF_SCAN_THREADS == 1024 and sc.TK_QB == 128 and sc.IVF_MASK_LISTS_PER_WG == 32
    assert sc.grid_bound(300, 64, 2500) == 150 + 2500 and sc.grid_bound(2, 3, 2500) == 1 + 6


def test_eligibility_by_list_equals_the_pairwise_helper():
    """On test_gpu_ivf's probe-edge case (nlist 8, junk probe values, dead lists)."""
    M, N, nlist, nprobe = 37, 3000, 8, 4
    assign = torch.randint(0, nlist, (N,), generator=torch.Generator().manual_seed(62))
    probes = ic.distinct_probes(M, nlist, nprobe, 63)
    probes[0] = torch.tensor([-1, 3, nlist, 2 ** 31 - 1])
    probes[1] = -1
    probes[2] = torch.tensor([5, -1, -1, -(2 ** 31)])
    probes[3] = torch.tensor([nlist, nlist + 1, 1 << 20, 7])
    for dead in ((), (2, 4, 6)):
        want = ic.eligibility_for_probes(assign, probes, nlist, dead)
        got = sc.eligibility_by_list(assign, probes, nlist, dead)
        assert got.dtype == torch.bool and torch.equal(got, want), dead
    assert not sc.eligibility_by_list(assign, probes, nlist)[1].any()


def test_eligibility_by_list_hand_worked():
    assign = torch.tensor([0, 1, 1, 2, 0, 2])
    probes = torch.tensor([[1, -1], [0, 2], [7, 3]], dtype=torch.int32)
    assert sc.eligibility_by_list(assign, probes, 3).tolist() == [
        [False, True, True, False, False, False], [True, False, False, True, True, True], [False] * 6]


def test_host_offsets_against_a_loop():
    cnt = torch.tensor([0, 1, 128, 129, 0, 0, 300])
    list_off, tile_off = sc.host_offsets(cnt)
    assert list_off.tolist() == [0, 0, 1, 129, 258, 258, 258, 558]
    assert tile_off.tolist() == [0, 0, 1, 2, 4, 4, 4, 7]
    lo, hi = sc.offsets_ranges(2500)
    assert lo[833].item() == 2499 and hi[833].item() == 2500 and lo[834].item() == 2500 == hi[834].item()
    assert sc.mask_word_passes(0, 2048) == 1 and sc.mask_word_passes(1, 2048) == 2 and sc.mask_word_passes(37, 0) == 0


def test_masks_are_what_they_say():
    for cid in ("many-lists", "l-1025"):
        c, assign = sc.BY_ID[cid], sc.assignment(cid)
        m = sc.mask(cid, "focus-last")
        inside = (assign == c.focus).nonzero().flatten()
        assert int(m[inside].sum()) == 1 and bool(m[inside[-1]]) and m[assign != c.focus].all()
        m = sc.mask(cid, "live-40")
        assert torch.unique(assign[m]).tolist() == sc.live_lists(cid).tolist() and sc.live_lists(cid).numel() == 40
        h = sc.mask(cid, "half")
        assert 0.45 < float(h.float().mean()) < 0.55
