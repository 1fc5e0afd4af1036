"""CPU: the host side of tools/train_pipes_ab.py: the split over pipes and MPLight's pair lookup."""
import numpy as np
import pytest
import torch

from conftest import load_scenario
from resco_amd.sim import maxwave_tables
from tools.train_pipes_ab import pair_of_action, pipe_sizes


def test_pipe_sizes():
    assert pipe_sizes(16, 2) == [8, 8] and pipe_sizes(16, 3) == [6, 5, 5] and pipe_sizes(5, 1) == [5] and pipe_sizes(3, 3) == [1, 1, 1]
    for bad in ((2, 3), (4, 0)):
        with pytest.raises(ValueError):
            pipe_sizes(*bad)


@pytest.mark.parametrize('map_name', ['cologne1', 'ingolstadt21'])
def test_pair_of_action_inverts_the_valid_table(map_name):
    """valid[s][g] = the local action of pair g; the lookup gives back g for every valid (signal, pair)"""
    sc = load_scenario(map_name)
    _, valid, order = maxwave_tables(sc)
    S, P = valid.shape
    n_max = max(int((valid[s] >= 0).sum()) for s in range(S))
    actions, want = np.zeros((n_max, S), np.int32), np.zeros((n_max, S), np.int32)
    for s in range(S):
        gs = [g for g in range(P) if valid[s, g] >= 0]
        for j in range(n_max):                  # every valid pair of the signal at least once
            g = gs[j % len(gs)]
            actions[j, s], want[j, s] = valid[s, g], g
    got = pair_of_action(torch.as_tensor(order, dtype=torch.long), torch.as_tensor(actions))
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
