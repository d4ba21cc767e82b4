"""CPU tests of the deep fused GNN path (``gnn_layers >= 2`` from the fused
layer-0 input alone) and of ``ops.node_msg_in``'s composed torch path.

Fold equivalence: goal and lidar-hit nodes never receive a message, so the
deep path carries them as two constant rows and updates agent rows only. It
must compute what ``GNN.forward`` computes from edge features over all V
nodes. Both are f32 evaluations of the same formulae in another association
order: forward within 1e-5 absolute, every parameter gradient within
1e-5 * max(1, max|g_ref|) (measured: forward 1.3e-6 to 1.9e-6, gradients
5.5e-7 to 8.9e-7 of the scale).
"""
import numpy as np
import pytest
import torch

from gcbfplus_amd import ops
from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.env import make_env
from gcbfplus_amd.nn.gnn import GNN

B = 2


def _random_biases(net, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.3)


@pytest.mark.parametrize("env_id,n,layers", [("DoubleIntegrator", 3, 2), ("DubinsCar", 3, 2),
                                             ("LinearDrone", 2, 3)])
def test_fold_equivalence(env_id, n, layers):
    env = make_env(env_id, num_agents=n, area_size=2.0, max_step=4, device="cpu")
    g = env.reset(B, np.random.default_rng(5))
    torch.manual_seed(6)
    gnn = GNN(env.node_dim, env.edge_dim, n_layers=layers)
    _random_biases(gnn, 7)
    w = torch.randn(B, n, gnn.out_dim, generator=torch.Generator().manual_seed(8))

    ref = gnn(g, env.edge_feats(g))
    gnn.zero_grad()
    (ref * w).sum().backward()
    g_ref = {k: p.grad.clone() for k, p in gnn.named_parameters()}

    out = gnn(g, None, msg_in0=env.edge_msg_in(g))
    gnn.zero_grad()
    (out * w).sum().backward()

    assert out.shape == ref.shape == (B, n, gnn.out_dim)
    err = float((out - ref).detach().abs().max())
    print(f"\n[{env_id} L={layers}] forward max err {err:.3e}")
    assert err <= 1e-5, err
    # the constants are not trivial: goal / hit rows differ and are non-zero
    c = gnn.layers[0].const_node_update(torch.tensor([[0., 1., 0.], [1., 0., 0.]]))
    c = c.detach()
    assert float(c.abs().max()) > 0.1 and not torch.allclose(c[0], c[1])
    worst = 0.0
    for k, p in gnn.named_parameters():
        assert p.grad is not None, k
        scale = max(1.0, float(g_ref[k].abs().max()))
        d = float((p.grad - g_ref[k]).abs().max())
        worst = max(worst, d / scale)
        assert d <= 1e-5 * scale, (k, d, scale)
    # every layer's parameters take part (the last layer's too)
    for l in range(layers):
        assert float(g_ref[f"layers.{l}.msg_mlp.layers.0.kernel"].abs().max()) > 0
        assert float(g_ref[f"layers.{l}.update_out.bias"].abs().max()) > 0
    print(f"[{env_id} L={layers}] worst gradient err / scale {worst:.3e}")


def test_deep_path_keeps_row_gate_single_layer():
    env = make_env("DoubleIntegrator", num_agents=3, area_size=2.0, max_step=4, device="cpu")
    g = env.reset(B, np.random.default_rng(5))
    gnn = GNN(env.node_dim, env.edge_dim, n_layers=2)
    gate = torch.ones(B, 3, dtype=torch.bool)
    with pytest.raises(AssertionError, match="row_gate"):
        gnn(g, None, msg_in0=env.edge_msg_in(g), row_gate=gate)


# ---- ops.node_msg_in, composed torch --------------------------------------------------
def _operands(E, KP0, F, N, R, Bn, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    D = N + 1 + R
    X0 = torch.randn(Bn, N, D, KP0, generator=gen).to(dtype)
    xa = torch.randn(Bn, N, F, generator=gen).to(dtype)
    c = torch.randn(2, F, generator=gen).to(dtype)
    return X0, xa, c


def _hand_cat(X0, xa, c, E):
    Bn, N, D, _ = X0.shape
    F = xa.shape[-1]
    KP1 = (E + 2 * F + 31) // 32 * 32
    out = torch.zeros(Bn, N, D, KP1, dtype=X0.dtype)
    for b in range(Bn):
        for i in range(N):
            for d in range(D):
                s = xa[b, d] if d < N else (c[0] if d == N else c[1])
                out[b, i, d, :E + 2 * F] = torch.cat([X0[b, i, d, :E], s, xa[b, i]])
    return out


@pytest.mark.parametrize("E,F,N,R", [(4, 8, 3, 2), (2, 16, 1, 3), (12, 8, 2, 0), (4, 14, 2, 2)])
def test_node_msg_in_cpu_equals_hand_cat(E, F, N, R):
    X0, xa, c = _operands(E, 32, F, N, R, 2, torch.float32, 11)
    out = ops.node_msg_in(X0, xa, c, E)
    ref = _hand_cat(X0, xa, c, E)
    assert out.shape == ref.shape and out.shape[-1] % 32 == 0
    assert torch.equal(out, ref)
    assert torch.equal(out, ops.node_msg_in(X0, xa, c, E, n_rays=R))
    with pytest.raises(ValueError):
        ops.node_msg_in(X0, xa, c, E, n_rays=R + 1)


def test_node_msg_in_cpu_gradients_f64():
    E, F, N, R, Bn = 4, 8, 3, 2, 2
    D = N + 1 + R
    X0, xa, c = _operands(E, 32, F, N, R, Bn, torch.float64, 12)
    X0, xa, c = (t.requires_grad_(True) for t in (X0, xa, c))
    X1 = ops.node_msg_in(X0, xa, c, E)
    g = torch.randn(X1.shape, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    (X1 * g).sum().backward()
    # dX0: the edge columns are copied, the rest is zero
    dX0 = torch.zeros_like(X0)
    dX0[..., :E] = g[..., :E]
    assert torch.equal(X0.grad, dX0)
    # dxa[b,j,f] = sum_i g[b,i,j,E+f] + sum_d g[b,j,d,E+F+f]
    dxa = g[:, :, :N, E:E + F].sum(dim=1) + g[..., E + F:E + 2 * F].sum(dim=2)
    assert torch.allclose(xa.grad, dxa, rtol=0, atol=1e-12)
    # dc: goal slot d == N, hit slots d > N, over all (b, i)
    dc = torch.stack([g[:, :, N, E:E + F].sum(dim=(0, 1)),
                      g[:, :, N + 1:, E:E + F].sum(dim=(0, 1, 2))])
    assert dc.shape == (2, F) and D - N - 1 == R
    assert torch.allclose(c.grad, dc, rtol=0, atol=1e-12)


# ---- dispatch -----------------------------------------------------------------------
def _algo(env, layers):
    return make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim,
                     n_agents=env.num_agents, gnn_layers=layers, batch_size=4,
                     buffer_size=4, horizon=2, seed=0)


@pytest.mark.parametrize("layers", [1, 2])
def test_cpu_gnn_inputs_equal_net_inputs(layers, monkeypatch):
    env = make_env("DoubleIntegrator", num_agents=3, area_size=2.0, max_step=4, device="cpu")
    algo = _algo(env, layers)
    g = env.reset(B, np.random.default_rng(3))
    calls = []
    real = ops.node_msg_in
    monkeypatch.setattr(ops, "node_msg_in", lambda *a, **k: calls.append(1) or real(*a, **k))
    for states in (None, g.states * 0.5):
        a, b = algo._gnn_inputs(g, states), algo._net_inputs(g, states)
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)
    e, mi = algo._net_inputs(g)
    if layers == 2:  # _net_inputs itself is unchanged: torch edge features
        assert mi is None and torch.equal(e, env.edge_feats(g))
    else:
        assert e is None and torch.equal(mi, env.edge_msg_in(g))
    assert torch.isfinite(algo.act(g)).all() and torch.isfinite(algo.get_cbf(g)).all()
    assert not calls  # a CPU algo never takes the deep fused path
