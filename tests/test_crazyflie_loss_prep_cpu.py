"""CPU guard for the CrazyFlie loss-prologue hook: without a GPU the hook
declines and ``GCBFPlus._loss`` runs its composed (eager) branch."""
import numpy as np
import torch

from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.env import make_env
from gcbfplus_amd.env.crazyflie import CrazyFlie
from gcbfplus_amd.trainer.data import FlatBatch


def _setup(n=3, batch=4, seed=7):
    torch.manual_seed(seed)
    env = make_env("CrazyFlie", num_agents=n, area_size=2.0, max_step=8, device="cpu")
    algo = make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim, n_agents=n,
                     gnn_layers=1, batch_size=batch, buffer_size=8, horizon=4,
                     inner_epoch=1, seed=0)
    g = env.reset(batch, np.random.default_rng(seed))
    safe = torch.rand(batch, n) < 0.5
    unsafe = ~safe & (torch.rand(batch, n) < 0.5)
    mb = FlatBatch(g.states, g.mask, safe, unsafe, torch.randn(batch, n, 4))
    return env, algo, g, mb


def test_loss_prep_declines_on_cpu():
    env, _, g, _ = _setup()
    assert type(env) is CrazyFlie
    raw = torch.randn(g.batch_size, env.num_agents, 4)
    assert env.loss_prep(g, raw) is None


def test_loss_takes_the_eager_branch_on_cpu(monkeypatch):
    env, algo, _, mb = _setup()
    calls = []
    orig = CrazyFlie.forward_graph

    def spy(self, graph, action):
        calls.append(1)
        return orig(self, graph, action)

    monkeypatch.setattr(CrazyFlie, "forward_graph", spy)
    total, info = algo._loss(mb, want_info=True)
    assert calls, "eager prologue not taken"
    assert torch.isfinite(total) and all(np.isfinite(v) for v in info.values())
    total.backward()
    grads = [p.grad for p in algo.actor.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads)
    assert any(bool((x != 0).any()) for x in grads)
