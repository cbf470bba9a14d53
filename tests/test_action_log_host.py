"""The action log's host side without a device: metrics.action_means / action_args on hand-made histograms."""
import importlib
import statistics
from fractions import Fraction

import numpy as np


def _mx():
    return importlib.import_module("marl-scheduling_amd.metrics")


def test_action_means_empty_single_and_mixed_bins(ms):
    mx = _mx()
    hist = np.array([[0, 0, 0, 0],    # an empty bin
                     [0, 0, 7, 0],    # a single action
                     [1, 2, 0, 1],    # (0 + 2 + 3) / 4
                     [2 ** 40, 0, 0, 2 ** 40 + 1]], dtype=np.int64)  # exact where a float sum would round
    m = mx.action_means(hist)
    assert m.shape == (4,) and m[0] is None
    assert m[1] == Fraction(2) and m[2] == Fraction(5, 4)
    assert m[3] == Fraction(3 * (2 ** 40 + 1), 2 ** 41 + 1)
    m3 = mx.action_means(hist.reshape(2, 2, 4))
    assert m3.shape == (2, 2) and m3[0, 0] is None and m3[1, 0] == Fraction(5, 4)


def test_action_args_gives_experiment3_keys(ms):
    mx = _mx()
    N, L, A = 2, 3, 4
    rng = np.random.default_rng(0)
    log, picks = [], []
    for ep in range(3):
        acts = rng.integers(0, A, (5, N, L))  # 5 rounds of one replica
        if ep == 1:
            acts[:, 0, 2] = 3  # a slot that always takes one action: a whole mean
        off = np.zeros((N, L, A), dtype=np.int64)
        for t in range(5):
            for a in range(N):
                for s in range(L):
                    off[a, s, acts[t, a, s]] += 1
        log.append(dict(offer=off, price=None, acceptor=np.zeros((N, 2, 7), dtype=np.int64), rounds=5, n_envs=1))
        picks.append(acts)
    for agent in (0, 1):
        d = mx.action_args(log, agent=agent)
        assert sorted(d) == ["0", "1", "2"]
        for s in range(L):
            want = [statistics.mean(int(x) for x in p[:, agent, s]) for p in picks]
            assert d[str(s)] == want and [type(x) for x in d[str(s)]] == [type(x) for x in want]
    assert mx.action_args(log)["2"][1] == 3
    empty = dict(log[0], offer=np.zeros((N, L, A), dtype=np.int64))
    assert mx.action_args([empty])["0"] == [None]
    assert mx.action_args([]) == {} and mx.action_args([], collection_length=2) == {"0": [], "1": []}
