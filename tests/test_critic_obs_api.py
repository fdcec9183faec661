"""Privileged critic observations above the kernel, without a GPU: the cfg flag and its CLI switch, the
runner's observation-group helpers, the torch PPO path with a critic wider than the actor's input, and
the C ABI's new symbols (declared in include/zbot_critic_obs.h, exported by libzbot.so)."""
from __future__ import annotations

import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_TASKS = ["zbot-6b-walking-v2", "zbot-6b-standup-v0", "zbot-6b-walking-v4", "zbot-6b-walking-m-v0",
             "zbot-6b-walking-m-play-v0"]


@pytest.mark.parametrize("task", ENV_TASKS)
def test_cfg_flag_defaults_off(task):
    import zbot_lab_amd
    assert zbot_lab_amd.tasks.load_cfg(task).critic_observations is False


def test_cli_switch_sets_the_cfg_flag(monkeypatch):
    """--critic_obs reaches the env cfg that scripts/train.py hands to make() (stopped there: no GPU here)."""
    import zbot_lab_amd
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import train
    finally:
        sys.path.pop(0)
    assert train.build_parser().parse_args([]).critic_obs is False
    assert train.build_parser().parse_args(["--critic_obs"]).critic_obs is True
    seen = {}

    class Stop(Exception):
        pass

    def fake_make(task, cfg=None, **kw):
        seen[task] = cfg.critic_observations
        raise Stop

    monkeypatch.setattr(zbot_lab_amd, "make", fake_make)
    for argv, want in ((["--device", "cpu"], False), (["--device", "cpu", "--critic_obs"], True)):
        with pytest.raises(Stop):
            train.main(["--task", "zbot-6b-walking-v4", "--log_root", os.devnull] + argv)
        assert seen["zbot-6b-walking-v4"] is want


def test_observation_group_helpers():
    from zbot_lab_amd.rl.runner import _critic_obs, _policy_obs
    p, c = torch.zeros(4, 23), torch.ones(4, 30)
    assert _policy_obs({"policy": p, "critic": c}) is p and _critic_obs({"policy": p, "critic": c}) is c
    assert _policy_obs({"policy": p}) is p and _critic_obs({"policy": p}) is None
    assert _policy_obs(p) is p and _critic_obs(p) is None


def test_torch_ppo_with_a_wider_critic_updates_on_cpu():
    from zbot_lab_amd.rl import PPO, ActorCritic
    torch.manual_seed(0)
    n, t, od, cd, na = 16, 4, 23, 30, 6
    pol = ActorCritic(od, cd, na, actor_hidden_dims=[32, 32], critic_hidden_dims=[32, 32], critic_obs_normalization=True)
    alg = PPO(pol, device="cpu", num_learning_epochs=2, num_mini_batches=2)
    alg.init_storage(n, t, od, cd, na)
    assert alg.storage.observations.shape == (t, n, od) and alg.storage.critic_observations.shape == (t, n, cd)
    before = [p.detach().clone() for p in pol.critic.parameters()]
    seen = []
    for _ in range(t):
        obs, cobs = torch.randn(n, od), torch.randn(n, cd)
        seen.append(cobs)
        a = alg.act(obs, cobs)
        assert a.shape == (n, na)
        alg.process_env_step(torch.randn(n), torch.zeros(n, dtype=torch.long), {})
        pol.update_normalization(obs, cobs)
    assert torch.equal(alg.storage.critic_observations, torch.stack(seen))
    assert int(pol.critic_obs_normalizer.count) == t * n and pol.critic_obs_normalizer._mean.shape[-1] == cd
    alg.compute_returns(torch.randn(n, cd))
    losses = alg.update()
    assert all(torch.isfinite(torch.tensor(v)) for v in losses.values())
    assert any(not torch.equal(b, p.detach()) for b, p in zip(before, pol.critic.parameters()))
    with pytest.raises(RuntimeError):  # the critic takes the critic rows only
        pol.evaluate(torch.randn(n, od))


def test_library_exports_the_critic_entry_points():
    from zbot_lab_amd import _native, build
    text = open(os.path.join(ROOT, "include", "zbot_critic_obs.h")).read()
    declared = set(re.findall(r"^\s*int\s+(zb_\w+)\s*\(", text, re.M))
    assert declared == set(_native.EXPORTED_CRITIC_OBS) and len(declared) == 3
    assert '#include "zbot_critic_obs.h"' in open(os.path.join(ROOT, "include", "zbot.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    assert declared <= set(re.findall(r"\bT (zb_\w+)", out))
    L = _native.lib()
    assert L.zb_critic_obs_dim(None) < 0  # (invalid handle: reported, not crashed on)
    assert L.zb_set_critic_obs_buffer(None, None) < 0 and b"zb_set_critic_obs_buffer" in L.zb_last_error()
    assert L.zb_observe_critic(None, None, None) < 0
