"""data.negative_sampler drop-in: the reference's NegativeSampler class over the device walk sampler.

  * sample_random_negatives: the reference's indices and numpy stream state (tests/golden/reference_golden_loss.npz, N1);
  * sample_batch_negatives: the reference's epoch schedule;
  * sample_hard_negatives through the class reproduces golden G7 (tests/golden/reference_golden_r2.npz), as
    test_hard_negatives_match_the_reference does through the function (GPU).
"""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_golden_loss.npz"))


class _Dataset:
    def __init__(self, n):
        self.movie_id_to_idx = {1000 + 3 * i: i for i in range(n)}


def test_random_negatives_match_the_reference(gold):
    from data.negative_sampler import NegativeSampler
    s = NegativeSampler(_Dataset(int(gold["n1_num_movies"])))
    assert s.num_negative_samples == int(gold["n1_default_num"]) and s.random_walk_sampler is None
    assert s.all_movie_indices == list(range(int(gold["n1_num_movies"])))
    np.random.seed(77)
    out = s.sample_random_negatives(512, "cpu")
    assert str(out.dtype) == str(gold["n1_dtype"]) and np.array_equal(out.numpy(), gold["n1_indices"])
    st = np.random.get_state()
    assert np.array_equal(st[1], gold["n1_state_key"]) and int(st[2]) == int(gold["n1_state_pos"])
    assert np.random.random_sample() == float(gold["n1_tail"])


def test_batch_negatives_follow_the_epoch_schedule():
    from data.negative_sampler import NegativeSampler
    q = torch.arange(8)
    s = NegativeSampler(_Dataset(100), num_negative_samples=20)
    for epoch in (0, 3):                                    # no walk sampler: never hard negatives
        rnd, hard = s.sample_batch_negatives(q, "cpu", epoch=epoch)
        assert hard is None and rnd.shape == (20,) and rnd.unique().numel() == 20
    with pytest.raises(ValueError):
        s.sample_hard_negatives(q)

    calls = []

    class _Spy(NegativeSampler):
        def sample_hard_negatives(self, query_indices, num_hard_samples=5, max_rank=5000, min_rank=2000):
            calls.append(num_hard_samples)
            return torch.zeros(len(query_indices), num_hard_samples, dtype=torch.int64)

    spy = _Spy(_Dataset(100), random_walk_sampler=object(), num_negative_samples=20)
    assert spy.sample_batch_negatives(q, "cpu", epoch=0)[1] is None and calls == []
    for epoch, want in ((1, 1), (4, 4), (6, 6), (9, 6)):
        rnd, hard = spy.sample_batch_negatives(q, "cpu", epoch=epoch)
        assert hard.shape == (8, want) and calls[-1] == want


@pytest.mark.gpu
def test_hard_negatives_through_the_class_match_the_reference(golden2):
    from data.negative_sampler import NegativeSampler
    from utils.random_walk import RandomWalkSampler
    g = golden2
    walker = RandomWalkSampler(torch.from_numpy(g["g7_edge_index"]), torch.from_numpy(g["g7_edge_weights"]),
                               walk_length=2, num_walks=100)
    s = NegativeSampler(_Dataset(int(g["g7_num_movies"])), random_walk_sampler=walker)
    q = torch.from_numpy(g["g7_queries"])
    for tag in ("window", "short", "default"):
        nh, mx, mn = [int(v) for v in g[f"g7_{tag}_args"]]
        np.random.seed(31)
        out = s.sample_hard_negatives(q, num_hard_samples=nh, max_rank=mx, min_rank=mn)
        assert out.dtype == torch.int64 and np.array_equal(out.numpy(), g[f"g7_{tag}_out"]), tag
        assert np.random.random_sample() == float(g[f"g7_{tag}_tail"]), tag
