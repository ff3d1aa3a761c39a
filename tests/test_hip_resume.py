"""GPU: a checkpointed ppo.train_fused run resumes exactly (checkpoint.py, CDAVecEnv.snapshot / restore).

Run A trains 3 iterations and checkpoints every 2; run B builds everything afresh, restores iter_2 and runs iteration 3.  B's rollout must be A's
third rollout bit for bit.  The update sums advantage and loss statistics with double-precision atomics, so the parameters after it are compared
against the spread of two updates from the same restored state: bit-equal when those two are bit-equal, within their spread otherwise."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 48, "is_render": False, "auto_reset": True}
KW = dict(horizon=32, minibatch=256 * 32 * 4 // 2, chains=2)


def _env():
    from gym_continuousdoubleauction_amd import CDAVecEnv
    return CDAVecEnv(CFG, n_markets=256, with_info=False)


def _resume(ck_dir, restore=True, iters=3):
    from gym_continuousdoubleauction_amd import ppo
    keep = {}
    pol, hist = ppo.train_fused(_env(), iters=iters, log=lambda *_: None, keep=keep, checkpoint_dir=ck_dir, restore=restore, **KW)
    return pol, hist, keep


def _bufs(keep):
    b = keep["buffers"]
    return {k: b[k].clone() for k in ("obs", "category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp", "value", "reward", "record")}


def test_ppo_resume_is_exact(tmp_path):
    from gym_continuousdoubleauction_amd import checkpoint as CK, ppo
    a_dir = str(tmp_path / "a")
    keep_a = {}
    pol_a, hist_a = ppo.train_fused(_env(), iters=3, log=lambda *_: None, keep=keep_a, checkpoint_dir=a_dir, chkpt_freq=2, **KW)
    bufs_a, theta_a = _bufs(keep_a), pol_a.theta.clone()
    assert [n for n, _ in CK.list_checkpoints(a_dir)] == [2, 3]
    # B: restore iter_2 (a copy of the directory, so that B's final save does not touch A's), target 3 -> runs iteration 3 (index 2)
    import shutil
    b_dir = str(tmp_path / "b")
    shutil.copytree(os.path.join(a_dir, "iter_2"), os.path.join(b_dir, "iter_2"))
    pol_b, hist_b, keep_b = _resume(b_dir)
    assert [h["iter"] for h in hist_b] == [2]
    bufs_b = _bufs(keep_b)
    for k in bufs_a:
        assert torch.equal(bufs_a[k].view(torch.uint8), bufs_b[k].view(torch.uint8)), k
    # the update: two updates from the same restored state first
    c_dir = str(tmp_path / "c")
    shutil.copytree(os.path.join(a_dir, "iter_2"), os.path.join(c_dir, "iter_2"))
    pol_c, _, _ = _resume(c_dir)
    spread = (pol_b.theta - pol_c.theta).abs().max().item()
    diff = (pol_b.theta - theta_a).abs().max().item()
    print(f"\nRESUME-THETA: two restored updates {'bit-equal' if spread == 0.0 else f'differ by up to {spread:.3e}'}; resumed vs uninterrupted max |dtheta| = {diff:.3e}")
    if spread == 0.0:
        assert torch.equal(pol_b.theta.view(torch.int32), theta_a.view(torch.int32))
    else:
        assert diff <= spread
    # a restore at the target runs nothing
    pol_d, hist_d, _ = _resume(a_dir, restore=os.path.join(a_dir, "iter_3"))
    assert hist_d == []
    assert torch.equal(pol_d.theta.view(torch.int32), theta_a.view(torch.int32))


def test_ppo_resume_checks_the_run_arguments(tmp_path):
    from gym_continuousdoubleauction_amd import ppo, CDAVecEnv
    d = str(tmp_path / "r")
    ppo.train_fused(_env(), iters=1, log=lambda *_: None, checkpoint_dir=d, **KW)
    with pytest.raises(ValueError, match="horizon"):
        ppo.train_fused(_env(), iters=2, log=lambda *_: None, checkpoint_dir=d, restore=True, horizon=16, minibatch=KW["minibatch"], chains=2)
    with pytest.raises(ValueError, match="markets"):
        env = CDAVecEnv(CFG, n_markets=128, with_info=False)
        ppo.train_fused(env, iters=2, log=lambda *_: None, checkpoint_dir=d, restore=True, **KW)
    with pytest.raises(ValueError, match="world"):
        ppo.train_fused(_env(), iters=2, log=lambda *_: None, checkpoint_dir=d, world=2, allreduce=lambda t: t, **KW)


LCFG = {"num_of_agents": 4, "init_cash": 1000000, "max_step": 64, "is_render": False, "auto_reset": True}
LKW = dict(horizon=32, num_trainable=2, chains=2, minibatch=256 * 32 // 2, std_dev_multiplier=-10.0, min_iterations_between_champions=1)


def _league(ck_dir, iters, **kw):
    from gym_continuousdoubleauction_amd import CDAVecEnv
    from gym_continuousdoubleauction_amd.league_train import train_league_fused
    keep = {}
    env = CDAVecEnv(LCFG, n_markets=256, with_info=False)
    bank, league, hist = train_league_fused(env, iters=iters, log=lambda *_: None, keep=keep, checkpoint_dir=ck_dir, **dict(LKW, **kw))
    return bank, league, hist, keep


def test_league_resume_is_exact(tmp_path):
    """max_step 64, horizon 32: two rollouts per episode.  A runs 5 iterations with a checkpoint every episode (iter_2, iter_4); B restores iter_4 and runs
    iteration 5 (a new episode: fresh opponents drawn from the restored pool).  The promotion threshold is forced low so that champions exist."""
    import shutil
    from gym_continuousdoubleauction_amd import checkpoint as CK
    a_dir = str(tmp_path / "a")
    bank_a, league_a, hist_a, keep_a = _league(a_dir, 5, chkpt_freq=2)
    assert [n for n, _ in CK.list_checkpoints(a_dir)] == [2, 4]        # the final save is skipped: iteration 5 ends mid-episode
    assert league_a.history, "no champion was promoted before the checkpoint"
    b_dir = str(tmp_path / "b")
    shutil.copytree(os.path.join(a_dir, "iter_4"), os.path.join(b_dir, "iter_4"))
    bank_b, league_b, hist_b, keep_b = _league(b_dir, 5, restore=True)
    assert [h["iter"] for h in hist_b] == [4]
    assert league_b.mapper.available_modules == league_a.mapper.available_modules and league_b.mapper.pool() == league_a.mapper.pool()
    assert league_b.net_of == league_a.net_of and [c["id"] for c in league_b.history] == [c["id"] for c in league_a.history]
    assert league_b.mapper.champion_id_counter == league_a.mapper.champion_id_counter and bank_b.n_frozen == bank_a.n_frozen
    assert torch.equal(keep_b["slot_pool"], keep_a["slot_pool"])
    for row in range(bank_a.n_trainable, bank_a.n_trainable + bank_a.n_frozen):     # the champions' rows (never trained after their promotion)
        assert torch.equal(bank_b.theta[row].view(torch.int32), bank_a.theta[row].view(torch.int32))
        assert torch.equal(bank_b.wb[row].view(torch.int16), bank_a.wb[row].view(torch.int16))
    for key in ("obs", "category", "size_mean", "size_sigma", "price", "price_offset", "a_cont", "logp", "value", "reward", "record"):
        assert torch.equal(keep_a["buffers"][key].view(torch.uint8), keep_b["buffers"][key].view(torch.uint8)), key


def test_league_refuses_a_checkpoint_off_the_episode_boundary(tmp_path):
    with pytest.raises(ValueError, match="episode boundar"):
        _league(str(tmp_path / "x"), 2, chkpt_freq=1)
    with pytest.raises(ValueError, match="checkpoint_dir"):
        _league(None, 2, chkpt_freq=2)
