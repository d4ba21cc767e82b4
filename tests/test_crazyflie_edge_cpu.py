"""CPU tests of the CrazyFlie layer-0 GNN input, ``ops.edge_msg_in(mode=2)``:
the composed torch path equals ``CrazyFlie.edge_feats`` plus the two one-hots
bit for bit, its gradient equals autograd through ``edge_feats`` in float64,
and a CPU env never routes to the fused input."""
import math

import numpy as np
import torch

from gcbfplus_amd import ops
from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.env import make_env
from gcbfplus_amd.utils.graph import GraphBatch

B, N = 2, 3


def _env():
    return make_env("CrazyFlie", num_agents=N, area_size=2.0, max_step=4, device="cpu")


def _states(env, seed=0):
    """Every node fully random: positions over 1.5 comm so slots fall on both
    sides of the clip, |psi| up to 10, theta/phi, uvw and rates at their limits."""
    rng = np.random.default_rng(seed)
    comm, R = env.params["comm_radius"], env.n_rays
    V = 2 * N + N * R
    assert (V, N + 1 + R) == (54, 20)
    st = np.concatenate([
        rng.uniform(0, 1.5 * comm, (B, V, 3)), rng.uniform(-10, 10, (B, V, 1)),
        rng.uniform(-math.pi / 4, math.pi / 4, (B, V, 2)), rng.uniform(-0.3, 0.3, (B, V, 3)),
        rng.uniform(-10, 10, (B, V, 3))], -1)
    return torch.from_numpy(st.astype(np.float32))


def _graph(env, st):
    mask = torch.ones(st.shape[0], N, N + 1 + env.n_rays, dtype=torch.bool)
    return GraphBatch(states=st, mask=mask, n_agents=N, n_rays=env.n_rays)


def _compose(env, st):
    """cat([edge_feats, sender one-hot, recv one-hot, zero pad]) from the env."""
    e = env.edge_feats(_graph(env, st), st)
    D = e.shape[2]
    oh = torch.zeros(N, D, 6, dtype=st.dtype)
    oh[:, :N, 2] = 1.0
    oh[:, N, 1] = 1.0
    oh[:, N + 1:, 0] = 1.0
    oh[:, :, 5] = 1.0
    pad = torch.zeros(st.shape[0], N, D, 32 - 18, dtype=st.dtype)
    return torch.cat([e, oh[None].expand(st.shape[0], N, D, 6), pad], dim=-1)


def test_mode2_equals_edge_feats_compose():
    env = _env()
    st = _states(env)
    comm = env.params["comm_radius"]
    out = ops.edge_msg_in(st, N, env.n_rays, 3, comm, mode=2)
    ref = _compose(env, st)
    assert out.shape == (B, N, 20, 32) and out.dtype == torch.float32
    assert torch.equal(out, ref)
    # the inputs exercise the transform and both clip branches
    nrm = ref[..., :3].norm(dim=-1)
    clipped = (nrm > comm * (1 - 1e-6)).float().mean()
    assert 0.1 < clipped < 0.9, clipped
    assert not torch.equal(out, ops.edge_msg_in(st, N, env.n_rays, 3, comm, mode=0))


def test_mode2_gradient_matches_edge_feats_autograd_f64():
    env = _env()
    st = _states(env, seed=1).double()
    comm = env.params["comm_radius"]
    g = torch.from_numpy(np.random.default_rng(2).standard_normal((B, N, 20, 32)))
    a = st.clone().requires_grad_(True)
    (ops.edge_msg_in(a, N, env.n_rays, 3, comm, mode=2) * g).sum().backward()
    b = st.clone().requires_grad_(True)
    (_compose(env, b) * g).sum().backward()
    assert a.grad.abs().max() > 1.0
    rel = (a.grad - b.grad).abs().max() / b.grad.abs().max()
    assert rel <= 1e-10, rel


def test_cpu_env_keeps_edge_feats_path():
    env = _env()
    assert env.fused_edge is False
    algo = make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim, n_agents=N,
                     gnn_layers=1, batch_size=4, buffer_size=4, horizon=2, seed=0)
    g = env.reset(B, np.random.default_rng(3))
    e, mi = algo._net_inputs(g)
    assert mi is None and e.shape == (B, N, 20, 12)
    assert torch.equal(e, env.edge_feats(g))
