"""Policy files (mlp.save_policy / load_policy's format), the league's save helper and the evaluation's slot placement - no GPU needed."""
import json
import os
import types

import numpy as np
import pytest
import torch

from gym_continuousdoubleauction_amd import mlp
from gym_continuousdoubleauction_amd.evaluate import slot_modules
from gym_continuousdoubleauction_amd.league_train import save_league


def _theta(n_hist, hidden, head, seed=0):
    return mlp.init_theta(42 * n_hist, generator=torch.Generator().manual_seed(seed), state_dependent_log_std=head, hidden=hidden)


@pytest.mark.parametrize("n_hist", [1, 4, 8])
@pytest.mark.parametrize("hidden", [(256, 256), (64, 128)])
@pytest.mark.parametrize("head", [False, True])
def test_round_trip_is_bit_exact_and_keeps_the_metadata(tmp_path, n_hist, hidden, head):
    th = _theta(n_hist, hidden, head)
    path = str(tmp_path / "p.pt")
    mlp.save_policy(path, th)
    rec = torch.load(path, weights_only=True)
    assert rec["format"] == "cda-mlp-policy" and rec["version"] == 1
    assert rec["n_hist"] == n_hist and list(rec["hidden"]) == list(hidden) and rec["state_dependent_log_std"] is head
    back = mlp.read_policy(path)
    assert back.dtype == torch.float32 and back.device.type == "cpu"
    assert torch.equal(back.view(torch.int32), th.view(torch.int32))


def _write(path, **over):
    rec = mlp.policy_record(_theta(4, (64, 128), True))
    rec.update(over)
    torch.save(rec, path)


@pytest.mark.parametrize("over", [{"n_hist": 8}, {"hidden": [256, 256]}, {"state_dependent_log_std": False}, {"format": "something-else"}, {"version": 2},
                                  {"theta": torch.zeros(12345)}, {"theta": torch.zeros(mlp.PARAMS, dtype=torch.float64)}])
def test_mismatched_or_unknown_files_are_refused(tmp_path, over):
    path = str(tmp_path / "bad.pt")
    _write(path, **over)
    with pytest.raises(ValueError):
        mlp.read_policy(path)


def test_a_bank_row_needs_its_row():
    with pytest.raises(ValueError):
        mlp.policy_record(mlp.PolicyBank.__new__(mlp.PolicyBank), row=None)


def test_league_json_names_files_that_load(tmp_path):
    rows = [_theta(4, (256, 256), False, seed=s) for s in range(5)]
    bank = types.SimpleNamespace(theta=torch.stack(rows), n_trainable=2)
    league = types.SimpleNamespace(net_of={"champion_0": 2, "champion_3": 4},
                                   history=[{"id": "champion_0", "iteration": 3, "return": 1.5, "source": "policy_0"},
                                            {"id": "champion_3", "iteration": 9, "return": 2.5, "source": "policy_1"}])
    out = save_league(str(tmp_path), bank, league)
    with open(tmp_path / "league.json") as fh:
        disk = json.load(fh)
    assert disk == out and disk["format"] == "cda-league"
    assert [t["row"] for t in disk["trainable"]] == [0, 1]
    assert [(c["module"], c["row"], c["promoted_iteration"]) for c in disk["champions"]] == [("champion_0", 2, 3), ("champion_3", 4, 9)]
    for entry in disk["trainable"] + disk["champions"]:
        th = mlp.read_policy(os.path.join(str(tmp_path), entry["file"]))
        assert torch.equal(th, rows[entry["row"]])


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 2])
def test_the_placement_is_the_documented_slot_map(P, k):
    N, A = 7, 4
    m = slot_modules(N, A, k, P)
    assert m.shape == (N, A) and m.dtype == np.int32
    for market in range(N):
        for slot in range(A):
            assert m[market, slot] == (0 if slot < k else 1 + market % P)
    assert (slot_modules(N, A, A, 0) == 0).all()
    with pytest.raises(ValueError):
        slot_modules(N, A, 0, P)
    with pytest.raises(ValueError):
        slot_modules(N, A, A + 1, P)
