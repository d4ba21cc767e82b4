"""GPU tests of ``ops.node_msg_in`` (the fused input of GNN layer >= 1) and of
the deep fused path built on it (``gnn_layers >= 2`` on the HIP path).

Kernel level: the forward is a gather, so it is compared bit for bit with the
same gather built from torch ops on bf16 tensors; ``dX0`` likewise. ``dxa``
and ``dc`` are f32 sums of bf16 terms in a fixed order: against the f64 sum of
the same terms each entry must lie within ``n_terms * 2^-23 * sum|t|`` (the
recursive-summation bound (n-1) u sum|t| with u = 2^-24, times two).

Network and algorithm level: the deep path and the eager path (torch edge
features, all V nodes) round to bf16 at the same depths, so with the CPU f32
result as the reference

    err_fused <= 4 * max(err_eager, 2^-8 * max|ref|)

(the factor 4 is for the scatter of two such maxima over ~10^3 entries).
Measured on an MI355X (table in PARITY.md): every ratio err_fused / err_eager
over more than one entry lay between 0.65 and 1.35; the loss total, a single
scalar, gave 0.30 (DoubleIntegrator) and 6.86 (CrazyFlie), both errors below
the 2^-8 * max|ref| floor.
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gcbfplus_amd import ops
from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.algo.module.cbf import CBFNet
from gcbfplus_amd.env import make_env
from gcbfplus_amd.env.crazyflie import CrazyFlie
from gcbfplus_amd.trainer.data import FlatBatch

BF = torch.bfloat16
#          E  KP0   F  N   R  B
CASES = [(2, 32, 128, 3, 32, 1),   # SingleIntegrator: features 4 B off the 16 B grid
         (4, 32, 128, 1, 32, 3),   # DoubleIntegrator, no other agent, D = 34
         (4, 32, 64, 3, 32, 2),    # PPO-net width, KP1 = 160
         (6, 32, 128, 2, 16, 3),   # LinearDrone
         (12, 32, 128, 3, 16, 2)]  # CrazyFlie
IDS = [f"E{c[0]}-F{c[2]}-N{c[3]}-R{c[4]}-B{c[5]}" for c in CASES]


def _kp1(E, F):
    return (E + 2 * F + 31) // 32 * 32


def _operands(case, seed=0):
    E, KP0, F, N, R, B = case
    gen = torch.Generator().manual_seed(seed)
    D = N + 1 + R
    X0 = torch.randn(B, N, D, KP0, generator=gen).to(BF).cuda()
    xa = torch.randn(B, N, F, generator=gen).to(BF).cuda()
    c = torch.randn(2, F, generator=gen).cuda()
    return X0, xa, c


def _ref_fwd(X0, xa, c, E, R):
    """the same gather from torch ops on the bf16 tensors"""
    B, N, D, _ = X0.shape
    F = xa.shape[-1]
    cb = c.to(BF)
    sender = torch.cat([xa[:, None].expand(B, N, N, F), cb[0].expand(B, N, 1, F),
                        cb[1].expand(B, N, R, F)], dim=2)
    recv = xa[:, :, None].expand(B, N, D, F)
    pad = torch.zeros(B, N, D, _kp1(E, F) - E - 2 * F, dtype=BF, device=X0.device)
    return torch.cat([X0[..., :E], sender, recv, pad], dim=-1)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_bit_equal(case):
    E, KP0, F, N, R, B = case
    X0, xa, c = _operands(case)
    assert (B * N * (N + 1 + R) * _kp1(E, F) // 8) % 256 != 0  # a ragged last block
    ref = _ref_fwd(X0, xa, c, E, R)
    # the output lands in memory that held NaNs: every column is written
    junk = torch.full(ref.shape, float("nan"), dtype=BF, device="cuda")
    del junk
    out = ops.node_msg_in(X0, xa, c, E)
    assert out.shape == ref.shape and out.dtype == BF and out.is_contiguous()
    assert torch.equal(_bits(out), _bits(ref))
    assert torch.equal(out[..., E + 2 * F:], torch.zeros_like(out[..., E + 2 * F:]))
    # the constants round as Tensor.to(bfloat16) does, and are not bf16 already
    assert not torch.equal(c.to(BF).float(), c)
    assert torch.equal(_bits(out[:, :, N, E:E + F]), _bits(c[0].to(BF).expand(B, N, F)))


def _bwd_ref(dX1, E, F, N, KP0):
    g = dX1.double()
    B, _, D, _ = g.shape
    dX0 = torch.zeros(B, N, D, KP0, dtype=BF, device=dX1.device)
    dX0[..., :E] = dX1[..., :E]
    snd, rcv = g[..., E:E + F], g[..., E + F:E + 2 * F]
    dxa = snd[:, :, :N].sum(dim=1) + rcv.sum(dim=2)
    dxa_abs = snd[:, :, :N].abs().sum(dim=1) + rcv.abs().sum(dim=2)
    dc = torch.stack([snd[:, :, N].sum(dim=(0, 1)), snd[:, :, N + 1:].sum(dim=(0, 1, 2))])
    dc_abs = torch.stack([snd[:, :, N].abs().sum(dim=(0, 1)),
                          snd[:, :, N + 1:].abs().sum(dim=(0, 1, 2))])
    return dX0, dxa, dxa_abs, dc, dc_abs


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward(case):
    from gcbfplus_amd import _C

    E, KP0, F, N, R, B = case
    D = N + 1 + R
    gen = torch.Generator().manual_seed(1)
    dX1 = torch.randn(B, N, D, _kp1(E, F), generator=gen).to(BF).cuda()
    dX0, dxa, dc = _C.node_msg_in_bwd(dX1, E, F, R, KP0)
    r_dX0, r_dxa, a_dxa, r_dc, a_dc = _bwd_ref(dX1, E, F, N, KP0)
    assert dX0.dtype == BF and dxa.dtype == dc.dtype == torch.float32
    assert dxa.shape == (B, N, F) and dc.shape == (2, F)
    assert torch.equal(_bits(dX0), _bits(r_dX0))
    u2 = 2.0 ** -23
    e_xa = (dxa.double() - r_dxa).abs()
    assert bool((e_xa <= (N + D) * u2 * a_dxa).all()), float((e_xa / a_dxa).max())
    n_dc = torch.tensor([[B * N], [B * N * R]], device="cuda", dtype=torch.float64)
    e_c = (dc.double() - r_dc).abs()
    assert bool((e_c <= n_dc * u2 * a_dc).all()), (e_c / a_dc).max(dim=1).values.tolist()
    assert float(r_dxa.abs().max()) > 1 and float(r_dc.abs().max()) > 1
    # deterministic: a second run has the same bits
    again = _C.node_msg_in_bwd(dX1, E, F, R, KP0)
    for a, b in zip((dX0, dxa, dc), again):
        assert torch.equal(a, b)


def test_autograd_function_routes_gradients():
    """ops.node_msg_in under autograd: X0 and xa get bf16 gradients (the
    kernel's f32 dxa rounded once), c its f32 gradient."""
    from gcbfplus_amd import _C

    case = CASES[3]
    E, KP0, F, N, R, B = case
    X0, xa, c = (t.requires_grad_(True) for t in _operands(case, seed=2))
    X1 = ops.node_msg_in(X0, xa, c, E, n_rays=R)
    dX1 = torch.randn(X1.shape, generator=torch.Generator().manual_seed(3)).to(BF).cuda()
    X1.backward(dX1)
    dX0, dxa, dc = _C.node_msg_in_bwd(dX1, E, F, R, KP0)
    assert torch.equal(X0.grad, dX0) and torch.equal(xa.grad, dxa.to(BF))
    assert torch.equal(c.grad, dc)


def test_captured_forward_backward_replays_bit_equal():
    from gcbfplus_amd import _C

    case = CASES[4]
    E, KP0, F, N, R, B = case
    X0, xa, c = _operands(case, seed=4)
    dX1 = torch.randn(B, N, N + 1 + R, _kp1(E, F),
                      generator=torch.Generator().manual_seed(5)).to(BF).cuda()

    def body():
        return (_C.node_msg_in_fwd(X0, xa, c, E, R, _kp1(E, F)),) + tuple(
            _C.node_msg_in_bwd(dX1, E, F, R, KP0))

    eager = [t.clone() for t in body()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = body()
    # new operand values through the same captured launches
    X0n, xan, cn = _operands(case, seed=6)
    for dst, src in zip((X0, xa, c), (X0n, xan, cn)):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0]), _bits(_ref_fwd(X0, xa, c, E, R)))
    for dst, src in zip((X0, xa, c), _operands(case, seed=4)):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
    del graph


def test_host_refusals():
    """each raises before anything is launched"""
    case = (4, 32, 64, 3, 8, 2)
    E, KP0, F, N, R, B = case
    X0, xa, c = _operands(case)
    D = N + 1 + R
    assert ops.node_msg_in(X0, xa, c, E).shape == (B, N, D, 160)
    with pytest.raises(RuntimeError, match="X0"):
        ops.node_msg_in(X0.float(), xa, c, E)
    xa_nc = torch.zeros(B, N, 2 * F, dtype=BF, device="cuda")[..., ::2]
    assert xa_nc.shape == xa.shape and not xa_nc.is_contiguous()
    with pytest.raises(RuntimeError, match="xa"):
        ops.node_msg_in(X0, xa_nc, c, E)
    with pytest.raises(RuntimeError, match="KP1"):
        ops.node_msg_in(X0, xa, c, E, k_pad=192)
    with pytest.raises(RuntimeError, match="KP1"):
        ops.node_msg_in(X0, xa, c, E, k_pad=128)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.node_msg_in(X0, xa[..., :60].contiguous(), c[:, :60].contiguous(), E)
    with pytest.raises(RuntimeError, match=r"N \+ 1 \+ R"):
        ops.node_msg_in(X0, xa, c, E, n_rays=R - 1)
    with pytest.raises(RuntimeError, match="c must be"):
        ops.node_msg_in(X0, xa, c.double(), E)
    from gcbfplus_amd import _C

    dX1 = torch.zeros(B, N, D, 160, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="KP1"):
        _C.node_msg_in_bwd(dX1[..., :128].contiguous(), E, F, R, KP0)
    with pytest.raises(RuntimeError, match="dX1"):
        _C.node_msg_in_bwd(dX1.float(), E, F, R, KP0)
    with pytest.raises(RuntimeError, match="E <= KP0"):
        _C.node_msg_in_bwd(dX1, 40, F, R, KP0)


# ---- network level ----------------------------------------------------------------
def _rule(err_fused, err_eager, ref_max):
    return err_fused <= 4.0 * max(err_eager, 2.0 ** -8 * ref_max)


def _net_run(net, g, e=None, mi=None):
    net.zero_grad(set_to_none=True)
    h = net(g, e, msg_in=mi)
    h.sum().backward()
    return h.detach().float().cpu(), {k: p.grad.detach().float().cpu().clone()
                                      for k, p in net.named_parameters()}


@pytest.mark.parametrize("env_id,n,layers,seed", [("DoubleIntegrator", 8, 2, 67),
                                                  ("LinearDrone", 2, 3, 71)])
def test_cbf_net_deep_vs_eager_vs_cpu(env_id, n, layers, seed):
    torch.manual_seed(seed)
    env_c = make_env(env_id, num_agents=n, area_size=4.0, max_step=4, device="cpu")
    g = env_c.reset(2, np.random.default_rng(seed + 1))
    net = CBFNet(env_c.node_dim, env_c.edge_dim, layers)
    h_c, g_c = _net_run(net, g, env_c.edge_feats(g))

    net_g = CBFNet(env_c.node_dim, env_c.edge_dim, layers)
    net_g.load_state_dict(net.state_dict())
    net_g = net_g.to("cuda")
    g_g = g.to("cuda")
    h_e, g_e = _net_run(net_g, g_g, env_c.edge_feats(g_g))
    mi = env_c.edge_msg_in(g_g)
    assert mi.dtype == BF and mi.is_cuda
    h_f, g_f = _net_run(net_g, g_g, None, mi)

    bad = []
    ef, ee = float((h_f - h_c).abs().max()), float((h_e - h_c).abs().max())
    print(f"\n[{env_id} L={layers}] h: err_fused {ef:.3e} err_eager {ee:.3e} "
          f"ratio {ef / max(ee, 1e-30):.2f}")
    if not _rule(ef, ee, float(h_c.abs().max())):
        bad.append(("h", ef, ee))
    worst = (0.0, "")
    for k, ref in g_c.items():
        ef, ee = float((g_f[k] - ref).abs().mean()), float((g_e[k] - ref).abs().mean())
        if ee > 0:
            worst = max(worst, (ef / ee, k))
        if not _rule(ef, ee, float(ref.abs().max())):
            bad.append((k, ef, ee))
        if float(ref.norm()) >= 1e-7:
            cos = float(torch.nn.functional.cosine_similarity(
                g_f[k].reshape(-1), ref.reshape(-1), dim=0))
            if not cos > 0.95:
                bad.append((k, "cosine", cos))
    print(f"[{env_id} L={layers}] gradients: worst err_fused/err_eager {worst[0]:.2f} ({worst[1]})")
    assert not bad, bad


# ---- algorithm level --------------------------------------------------------------
N_A, B_A = 4, 8


def _make(env_id, device, layers=2, cls=None):
    if cls is None:
        env = make_env(env_id, num_agents=N_A, area_size=2.0, max_step=4, device=device)
    else:
        env = cls(N_A, 2.0, max_step=4, params=dict(CrazyFlie.PARAMS), device=device)
    torch.manual_seed(31)
    algo = make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim, n_agents=N_A,
                     gnn_layers=layers, batch_size=B_A, buffer_size=B_A, horizon=4,
                     inner_epoch=1, seed=3)
    return env, algo


@functools.lru_cache(maxsize=None)
def _pair(env_id):
    """GPU algo, CPU algo with the same weights, one minibatch on each, and
    the CPU loss and gradients (computed once, shared)."""
    env_g, algo_g = _make(env_id, "cuda")
    env_c, algo_c = _make(env_id, "cpu")
    for a, b in ((algo_c.actor, algo_g.actor), (algo_c.cbf, algo_g.cbf)):
        a.load_state_dict({k: v.cpu() for k, v in b.state_dict().items()})
    g = env_c.reset(B_A, np.random.default_rng(32))
    gen = torch.Generator().manual_seed(33)
    st = g.states.clone()
    if env_id == "CrazyFlie":
        st[:, :N_A, 3:] += torch.randn(B_A, N_A, 9, generator=gen) * 0.1  # off hover
    safe = torch.rand(B_A, N_A, generator=gen) < 0.5
    unsafe = ~safe & (torch.rand(B_A, N_A, generator=gen) < 0.5)
    u_qp = torch.randn(B_A, N_A, env_c.action_dim, generator=gen).clamp(-1, 1)
    mb_c = FlatBatch(st, g.mask, safe, unsafe, u_qp)
    mb_g = FlatBatch(*[t.cuda() for t in mb_c])
    return env_g, algo_g, mb_g, _loss_and_grads(algo_c, mb_c)


def _loss_and_grads(algo, mb):
    gbuf = getattr(algo, "dp_gbuf", None)
    if gbuf is not None:
        gbuf.zero_()
    for p in list(algo.cbf.parameters()) + list(algo.actor.parameters()):
        if p.grad is not None:
            p.grad.zero_()
    total, _ = algo._loss(mb, want_info=False)
    total.backward()
    flat = lambda net: torch.cat([p.grad.reshape(-1) for p in net.parameters()])  # noqa: E731
    return tuple(t.detach().float().cpu().clone()
                 for t in (total.reshape(1), flat(algo.actor), flat(algo.cbf)))


@pytest.fixture
def calls(monkeypatch):
    """counts ops.node_msg_in calls (the deep path looks it up on the module)"""
    n = []
    real = ops.node_msg_in
    monkeypatch.setattr(ops, "node_msg_in", lambda *a, **k: n.append(1) or real(*a, **k))
    return n


@pytest.mark.parametrize("env_id", ["DoubleIntegrator", "CrazyFlie"])
def test_loss_default_vs_opt_out(env_id, calls, monkeypatch):
    env_g, algo_g, mb_g, cpu = _pair(env_id)
    assert env_g.fused_edge and not os.environ.get("GCBF_NO_FUSED_DEEP")
    fused = _loss_and_grads(algo_g, mb_g)
    # actor, CBF on [g; next_g], stop-gradient CBF: one call per layer >= 1 each
    assert len(calls) == 3 * (algo_g.gnn_layers - 1), len(calls)
    del calls[:]
    monkeypatch.setenv("GCBF_NO_FUSED_DEEP", "1")
    eager = _loss_and_grads(algo_g, mb_g)
    assert not calls
    bad = []
    for name, f, e, c in zip(("loss total", "actor grad", "cbf grad"), fused, eager, cpu):
        assert torch.isfinite(f).all() and float(c.abs().max()) > 0
        ef, ee = float((f - c).abs().mean()), float((e - c).abs().mean())
        print(f"\n[{env_id} {name}] err_fused {ef:.3e} err_eager {ee:.3e} "
              f"ratio {ef / max(ee, 1e-30):.2f} max|ref| {float(c.abs().max()):.3e}")
        if not _rule(ef, ee, float(c.abs().max())):
            bad.append((name, ef, ee))
    assert not bad, bad


def test_dispatch_call_counts(calls, monkeypatch):
    env, algo = _make("DoubleIntegrator", "cuda")
    g = env.reset(2, np.random.default_rng(34))
    e, mi = algo._gnn_inputs(g)
    assert e is None and mi.dtype == BF and mi.shape == (2, N_A, N_A + 1 + env.n_rays, 32)
    e, mi = algo._net_inputs(g)  # unchanged: torch edge features at gnn_layers = 2
    assert mi is None and e.dtype == torch.float32
    assert torch.isfinite(algo.act(g)).all() and len(calls) == 1
    assert torch.isfinite(algo.get_cbf(g)).all() and len(calls) == 2
    assert torch.isfinite(algo.step(g)[0]).all() and len(calls) == 3
    del calls[:]

    monkeypatch.setenv("GCBF_NO_FUSED_DEEP", "1")
    e, mi = algo._gnn_inputs(g)
    assert mi is None and e.dtype == torch.float32
    algo.act(g), algo.get_cbf(g)
    monkeypatch.delenv("GCBF_NO_FUSED_DEEP")

    env_c, algo_c = _make("DoubleIntegrator", "cpu")
    g_c = env_c.reset(2, np.random.default_rng(34))
    algo_c.act(g_c), algo_c.get_cbf(g_c)

    class SubFlie(CrazyFlie):
        pass

    env_s, algo_s = _make("CrazyFlie", "cuda", cls=SubFlie)
    assert env_s.fused_edge is False
    g_s = env_s.reset(2, np.random.default_rng(34))
    algo_s.act(g_s), algo_s.get_cbf(g_s)

    env_1, algo_1 = _make("DoubleIntegrator", "cuda", layers=1)
    algo_1.act(g), algo_1.get_cbf(g)
    assert not calls

    env_3, algo_3 = _make("LinearDrone", "cuda", layers=3)
    algo_3.act(env_3.reset(2, np.random.default_rng(34)))
    assert len(calls) == 2


def test_update_with_hip_graph_capture(calls):
    from gcbfplus_amd.trainer.utils import collect_rollout

    assert not os.environ.get("GCBF_NO_HIPGRAPH")
    torch.manual_seed(0)
    env = make_env("DoubleIntegrator", num_agents=N_A, area_size=2.0, max_step=8,
                   device="cuda")
    algo = make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim, n_agents=N_A,
                     gnn_layers=2, batch_size=8, buffer_size=16, horizon=4, inner_epoch=1,
                     seed=0)
    rollout = collect_rollout(env, algo.step, env.reset(2, np.random.default_rng(35)))
    n_rollout = len(calls)
    assert n_rollout >= 8
    info = algo.update(rollout, 0)  # 16 samples: one captured minibatch, one eager
    torch.cuda.synchronize()
    assert algo._mb_graph is not None and algo._mb_graph.graph is not None
    assert info and all(np.isfinite(v) for v in info.values()), info
    assert len(calls) > n_rollout
