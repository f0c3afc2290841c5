"""bench.py --dump-outputs without a GPU: dump_outputs on stand-in batches (the download / samples_tensor
surface of api.Batch, host tensors) writes float64 .npy files within 64 MB, cuts tables too large for it
to a seeded row sample whose indices it writes beside them, and writes the same bytes every time."""
import os

import numpy as np
import pytest
import torch

import bench
from gp_dla_detection_amd.api import Batch


class StandInBatch:
    def __init__(self, nq, S, seed):
        rng = np.random.default_rng(seed)
        self.num_quasars, self.num_samples = nq, S
        self.samples = torch.as_tensor(rng.standard_normal((nq, S)))
        self.results = {k: rng.standard_normal(v.shape).astype(v.dtype)
                        for k, v in Batch.empty_results(nq, S, False).items()}

    def download(self, with_samples=True):
        assert not with_samples
        return {k: v.copy() for k, v in self.results.items()}

    def samples_tensor(self):
        return self.samples


def dump(directory, cuts, S):
    batches = [StandInBatch(b1 - b0, S, i) for i, (b0, b1) in enumerate(cuts)]
    table = torch.as_tensor(np.random.default_rng(9).standard_normal((cuts[-1][1], 15)))
    bench.dump_outputs(str(directory), cuts, batches, table)
    out = {f[:-4]: np.load(os.path.join(directory, f)) for f in sorted(os.listdir(directory))}
    assert sum(os.path.getsize(os.path.join(directory, f)) for f in os.listdir(directory)) <= 64e6
    assert all(a.dtype == np.float64 for a in out.values())
    return batches, table.numpy(), out


@pytest.mark.parametrize("cuts,S", [([(0, 1000)], 10000),                                 # the headline shape
                                    ([(0, 32768), (32768, 65536), (65536, 162861)], 64)])  # shard batches
def test_dump_is_the_batches_rows_within_the_budget(tmp_path, cuts, S):
    batches, table, out = dump(tmp_path, cuts, S)
    samples = torch.cat([b.samples for b in batches]).numpy()
    rows = out["sample_rows"].astype(np.int64)
    assert rows.size and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(out["sample_log_likelihoods_dla"], samples[rows])
    q = out["quasar_rows"].astype(np.int64)
    for name in ("p_dlas", "log_likelihoods_dla", "model_posteriors", "status"):
        np.testing.assert_array_equal(out[name], np.concatenate([b.results[name] for b in batches])[q])
    np.testing.assert_array_equal(out["summary_table"], table[out["table_rows"].astype(np.int64)])


def test_dump_is_the_same_every_time(tmp_path):
    dump(tmp_path / "a", [(0, 1000)], 10000)
    dump(tmp_path / "b", [(0, 1000)], 10000)
    for f in os.listdir(tmp_path / "a"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
