"""Host-side pieces of bench.py (no GPU): the multi-hot KJT synthesiser, the PMC-summary lookup, the
--full / --dump-outputs options and the output writer."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_synth_kjt_batches_shapes_and_ranges():
    B, maxlen = 64, 7
    for ids in ("uniform", "zipf"):
        batches = bench.synth_kjt_batches(300, 500, B, maxlen, 2, torch.device("cpu"), ids, seed=1)
        for values, offsets, labels in batches:
            assert offsets.dtype == torch.int32 and offsets.numel() == 2 * B + 1 and int(offsets[0]) == 0
            lengths = offsets[1:] - offsets[:-1]
            assert int(lengths.min()) >= 1 and int(lengths.max()) <= maxlen
            assert values.numel() == int(offsets[-1])
            nb = int(offsets[B])
            assert int(values[:nb].max()) < 300 and int(values[nb:].max()) < 500 and int(values.min()) >= 0
            assert labels.numel() == B and set(labels.unique().tolist()) <= {0, 1}


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float32_npy_of_the_steps_outputs(tmp_path):
    import numpy as np

    class Tables:  # what dump_outputs reads of an ops.TableSet
        rows, device = [50, 70], torch.device("cpu")
        w = [torch.arange(50 * 4, dtype=torch.float32).view(50, 4), torch.arange(70 * 4, dtype=torch.float32).view(70, 4)]
        s = [torch.arange(50, dtype=torch.float32), torch.arange(70, dtype=torch.float32)]

        def table_view(self, t):
            return self.w[t]

        def state_view(self, t):
            return self.s[t]

    class Step:
        loss = torch.tensor(0.5)
        logits = torch.arange(8, dtype=torch.float32)
        params = torch.ones(5)
        tables = Tables()

    ids = [torch.tensor([3, 49, 120]), torch.tensor([0, 69, 71])]  # ids past the table wrap (id mod N)
    for _ in range(2):  # the same files, bit for bit, from the same arguments
        bench.dump_outputs(str(tmp_path), Step(), ids)
        got = {p.name: np.load(p) for p in tmp_path.iterdir()}
        assert all(v.dtype == np.float32 for v in got.values())
        assert sum(v.nbytes for v in got.values()) < 64 << 20
        np.testing.assert_array_equal(got["loss.npy"], [0.5])
        np.testing.assert_array_equal(got["logits.npy"], Step.logits.numpy())
        np.testing.assert_array_equal(got["table0_batch0_state.npy"], [3, 49, 20])
        np.testing.assert_array_equal(got["table1_batch0_rows.npy"], Tables.w[1][[0, 69, 1]].numpy())
        assert got["table1_seeded_rows.npy"].shape == (bench.DUMP_ROWS, 4)
        if _ == 0:
            first = got
    assert first.keys() == got.keys() and all(np.array_equal(first[k], got[k]) for k in got)


def test_pmc_traffic_uses_the_benchmarked_workload():
    t, src = bench.pmc_traffic("tower_l2_kernel")
    assert src is None or ("config5" not in src and "zipf" not in src)
    t5, src5 = bench.pmc_traffic("bwd_adagrad_direct_kernel", "config5")
    assert src5 is None or "config5" in src5
    assert bench.pmc_traffic("tower_l2_kernel", "northstar_zipf") == (None, None)
