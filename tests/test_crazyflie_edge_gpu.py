"""GPU tests of the fused CrazyFlie layer-0 GNN input (``ops.edge_msg_in``
mode 2: node pre-pass + slot kernel, atomic-free backward) and of
``ops.crazyflie_edge_jac``.

Inputs are hand-built: positions uniform in a cube of side 1.5 comm (slots
on both sides of the clip, asserted), |psi| <= 10, theta/phi within pi/4,
uvw within 0.3, rates within 10; one variant with goal / hit rows as real
graphs have them (zero beyond the position), one fully random on every node.
No slot norm sits within ``GAP`` of the clip threshold (asserted in float64),
so every evaluation takes the same branch.

Error figures are max errors normalised by max|ref| of the tensor:
``nerr(x, ref) = max|x - ref| / max|ref|``.

Backward and jacobian: the reference is float64 CPU autograd through the
compose (the torch body for the jacobian); the yardstick is the error of the
same computation in float32 on the CPU. The kernel gets

    nerr_gpu <= MARGIN * max(nerr_f32_cpu, 2^-23),   MARGIN = 8

(both are f32 evaluations of the same formulae; accumulation order and FMA
contraction move the rounding by a small multiple, a wrong index, sign or
jacobian entry shows at 1e-2 or worse). See the docstrings for the figures
measured on an MI355X.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gcbfplus_amd import ops
from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.env import make_env
from gcbfplus_amd.env.crazyflie import CrazyFlie
from gcbfplus_amd.trainer.data import FlatBatch
from gcbfplus_amd.utils.graph import GraphBatch

EPS32 = 2.0 ** -23
MARGIN = 8.0
GAP = 1e-5
COMM = CrazyFlie.PARAMS["comm_radius"]
R = 16  # CrazyFlie.n_rays
SHAPES = [(2, 3), (1, 1), (3, 5), (1, 70)]
VARIANTS = ["graph", "random"]


def nerr(x, ref):
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    return float((x - ref).abs().max() / ref.abs().max())


def _states(B, N, variant, seed):
    rng = np.random.default_rng(seed)
    V = 2 * N + N * R
    st = np.concatenate([
        rng.uniform(0, 1.5 * COMM, (B, V, 3)), rng.uniform(-10, 10, (B, V, 1)),
        rng.uniform(-math.pi / 4, math.pi / 4, (B, V, 2)),
        rng.uniform(-0.3, 0.3, (B, V, 3)), rng.uniform(-10, 10, (B, V, 3))], -1)
    if variant == "graph":
        st[:, N:, 3:] = 0.0
    return torch.from_numpy(st.astype(np.float32))


def _slot_norms(st, N):
    """float64 clip norms (B, N, D) of every slot."""
    B = st.shape[0]
    p = st[..., :3].double()
    send = torch.cat([p[:, None, :N].expand(B, N, N, 3), p[:, N:2 * N, None],
                      p[:, 2 * N:].reshape(B, N, R, 3)], dim=2)
    return torch.sqrt(1e-6 + (p[:, :N, None] - send).square().sum(-1))


@functools.lru_cache(maxsize=None)
def _case(B, N, variant):
    """States, bf16 cotangent and the CPU references of one case, computed
    once and shared (callers must not modify them)."""
    seed = 1000 * B + 10 * N + VARIANTS.index(variant)
    st = _states(B, N, variant, seed)
    nrm = _slot_norms(st, N)
    assert float((nrm - COMM).abs().min()) > GAP
    frac = float((nrm > COMM).double().mean())
    assert 0.1 <= frac <= 0.9, frac  # both sides of the clip
    D = N + 1 + R
    g = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((B, N, D, 32))
                         .astype(np.float32)).bfloat16()
    fwd32 = ops.edge_msg_in(st, N, R, 3, COMM, mode=2)
    s64 = st.double().requires_grad_(True)
    (ops.edge_msg_in(s64, N, R, 3, COMM, mode=2) * g.double()).sum().backward()
    s32 = st.clone().requires_grad_(True)
    (ops.edge_msg_in(s32, N, R, 3, COMM, mode=2) * g.float()).sum().backward()
    return dict(st=st, g=g, fwd32=fwd32, grad64=s64.grad, grad32=s32.grad)


def _gpu_backward(c, N):
    st = c["st"].cuda().requires_grad_(True)
    out = ops.edge_msg_in(st, N, R, 3, COMM, mode=2)
    (out * c["g"].cuda()).sum().backward()
    return st.grad


# ---- forward ---------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,N", SHAPES)
def test_forward_matches_cpu_compose(B, N, variant):
    """|gpu - ref| <= 2^-7 |ref| + 1e-5: one bf16 ulp of the stored value plus
    f32 noise on cancelled entries; one-hot and pad columns exactly."""
    c = _case(B, N, variant)
    out = ops.edge_msg_in(c["st"].cuda(), N, R, 3, COMM, mode=2)
    assert out.shape == (B, N, N + 1 + R, 32) and out.dtype == torch.bfloat16
    out, ref = out.float().cpu(), c["fwd32"]
    err = (out[..., :12] - ref[..., :12]).abs()
    bound = 2.0 ** -7 * ref[..., :12].abs() + 1e-5
    print(f"\n[fwd B={B} N={N} {variant}] max err {float(err.max()):.3e} "
          f"max err/bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())
    assert torch.equal(out[..., 12:], ref[..., 12:])


# ---- backward --------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,N", SHAPES)
def test_backward_matches_f64_autograd(B, N, variant):
    """Agent rows and goal/hit rows separately against float64 CPU autograd;
    bound = 8 * max(f32 CPU, 2^-23). Measured on an MI355X over the sixteen
    (case, row group) pairs: kernel nerr 4.3e-8 .. 1.30e-7, f32 CPU compose
    nerr 5.7e-8 .. 1.86e-7, kernel / f32 CPU between 0.23 and 1.68, i.e. the
    kernel is as accurate as the f32 compose and at most 0.14 of its bound."""
    c = _case(B, N, variant)
    grad = _gpu_backward(c, N).cpu()
    for name, sl in (("agent", slice(0, N)), ("goal/hit", slice(N, None))):
        ref = c["grad64"][:, sl]
        e_gpu, e_cpu = nerr(grad[:, sl], ref), nerr(c["grad32"][:, sl], ref)
        bound = MARGIN * max(e_cpu, EPS32)
        print(f"\n[bwd B={B} N={N} {variant} {name}] gpu {e_gpu:.3e} f32-cpu {e_cpu:.3e} "
              f"bound {bound:.3e}")
        assert float(ref.abs().max()) > 0.1
        assert e_gpu <= bound, (name, e_gpu, e_cpu)


def test_backward_is_deterministic():
    c = _case(3, 5, "random")
    assert torch.equal(_gpu_backward(c, 5), _gpu_backward(c, 5))
    c = _case(1, 70, "graph")
    assert torch.equal(_gpu_backward(c, 70), _gpu_backward(c, 70))


# ---- ops.crazyflie_edge_jac --------------------------------------------------------
def _cpu_env(N):
    return make_env("CrazyFlie", num_agents=N, area_size=2.0, max_step=4, device="cpu")


@pytest.mark.parametrize("M,N", [(2, 3), (1, 1), (3, 5)])
def test_edge_jac_matches_f64_torch_body(M, N):
    """Reference: the torch body of edge_grad_to_state_jac in float64 on the
    CPU; yardstick: the same body in float32. bound = 8 * max(f32 CPU, 2^-23).
    Measured on an MI355X at (2,3), (1,1), (3,5): kernel nerr 1.13e-7, 6.6e-8,
    8.2e-8; f32 CPU nerr 1.49e-7, 4.6e-8, 1.01e-7."""
    c = _case(M, N, "random")
    env = _cpu_env(N)
    D = N + 1 + R
    ge = torch.from_numpy(np.random.default_rng(7 + N).standard_normal((M, N, D, 12))
                          .astype(np.float32))
    gr = GraphBatch(states=c["st"], mask=torch.ones(M, N, D, dtype=torch.bool),
                    n_agents=N, n_rays=R)
    ref = env.edge_grad_to_state_jac(gr, c["st"].double(), ge.double())
    cpu32 = env.edge_grad_to_state_jac(gr, c["st"], ge)
    out = ops.crazyflie_edge_jac(c["st"].cuda(), ge.cuda(), N, R, COMM)
    assert out.shape == (M, N, N, 12) and out.dtype == torch.float32
    e_gpu, e_cpu = nerr(out, ref), nerr(cpu32, ref)
    bound = MARGIN * max(e_cpu, EPS32)
    print(f"\n[jac M={M} N={N}] gpu {e_gpu:.3e} f32-cpu {e_cpu:.3e} bound {bound:.3e}")
    assert e_gpu <= bound, (e_gpu, e_cpu)


# ---- algo-level: shared nets on GPU and CPU ----------------------------------------
N_E2E, B_E2E = 4, 8


def _make(device, gnn_layers=1, cls=None):
    if cls is None:
        env = make_env("CrazyFlie", num_agents=N_E2E, area_size=2.0, max_step=4, device=device)
    else:
        env = cls(N_E2E, 2.0, max_step=4, params=dict(CrazyFlie.PARAMS), device=device)
    torch.manual_seed(21)
    algo = make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim, n_agents=N_E2E,
                     gnn_layers=gnn_layers, batch_size=B_E2E, buffer_size=B_E2E, horizon=4,
                     inner_epoch=1, seed=3)
    return env, algo


@functools.lru_cache(maxsize=None)
def _pair():
    """GPU algo, CPU algo with the same weights, and one minibatch on each."""
    env_g, algo_g = _make("cuda")
    env_c, algo_c = _make("cpu")
    for a, b in ((algo_c.actor, algo_g.actor), (algo_c.cbf, algo_g.cbf)):
        a.load_state_dict({k: v.cpu() for k, v in b.state_dict().items()})
    g = env_c.reset(B_E2E, np.random.default_rng(22))
    gen = torch.Generator().manual_seed(23)
    st = g.states.clone()
    st[:, :N_E2E, 3:] += torch.randn(B_E2E, N_E2E, 9, generator=gen) * 0.1  # off hover
    safe = torch.rand(B_E2E, N_E2E, generator=gen) < 0.5
    unsafe = ~safe & (torch.rand(B_E2E, N_E2E, generator=gen) < 0.5)
    u_qp = torch.randn(B_E2E, N_E2E, 4, generator=gen).clamp(-1, 1)
    mb_c = FlatBatch(st, g.mask, safe, unsafe, u_qp)
    mb_g = FlatBatch(*[t.cuda() for t in mb_c])
    return env_g, algo_g, env_c, algo_c, mb_g, mb_c


def _loss_and_grads(algo, mb):
    gbuf = getattr(algo, "dp_gbuf", None)
    if gbuf is not None:
        gbuf.zero_()
    for p in list(algo.cbf.parameters()) + list(algo.actor.parameters()):
        if p.grad is not None:
            p.grad.zero_()
    total, _ = algo._loss(mb, want_info=False)
    total.backward()
    flat = lambda net: torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()  # noqa: E731
    return total.detach().reshape(1).clone(), flat(algo.actor), flat(algo.cbf)


def _all_outputs(env, algo, mb):
    g = mb.graph(env)
    return (algo.act(g).clone(), algo.get_cbf(g).detach().clone()) + _loss_and_grads(algo, mb)


E2E_NAMES = ("act", "get_cbf", "loss total", "actor grad", "cbf grad")


def test_end_to_end_default_vs_opt_out(monkeypatch):
    """algo.act, algo.get_cbf, the _loss total and both gradients, default
    against GCBF_NO_FUSED_EDGE=1. Both arms round the same f32 features to
    bf16 at the same place, so they differ only through isolated one-ulp
    inputs; the yardstick is the unfused GPU against the CPU fp32 result
    (bf16 rounding of EVERY input, weight and activation), margin 1: the
    fused arm may be no farther from the unfused arm than fp32 is. Measured
    on an MI355X: the two arms were bit-equal in all five outputs (nerr 0);
    unfused GPU against CPU fp32: act 2.1e-3, get_cbf 6.5e-3, loss total
    6.7e-4, actor grad 2.5e-2, cbf grad 4.0e-2."""
    env_g, algo_g, env_c, algo_c, mb_g, mb_c = _pair()
    assert env_g.fused_edge
    fused = _all_outputs(env_g, algo_g, mb_g)
    monkeypatch.setenv("GCBF_NO_FUSED_EDGE", "1")
    assert not env_g.fused_edge
    unfused = _all_outputs(env_g, algo_g, mb_g)
    monkeypatch.delenv("GCBF_NO_FUSED_EDGE")
    cpu = _all_outputs(env_c, algo_c, mb_c)
    bad = []
    for name, f, u, c in zip(E2E_NAMES, fused, unfused, cpu):
        d_arm, d_yard = nerr(f, u), nerr(u, c)
        print(f"\n[e2e {name}] fused-vs-unfused {d_arm:.3e}  unfused-vs-cpu-fp32 {d_yard:.3e}")
        assert torch.isfinite(f).all() and float(u.abs().max()) > 0
        if not d_arm <= 1.0 * d_yard:
            bad.append((name, d_arm, d_yard))
    assert not bad, bad


def test_cbf_and_jacobian_default_vs_opt_out(monkeypatch):
    """GCBFPlus.cbf_and_jacobian on CUDA with and without GCBF_NO_FUSED_EDGE.
    Both arms chain the same ge, so they differ by f32 rounding of the chain
    alone; the bound is the distance of the unfused GPU result from the CPU
    fp32 result (bf16 GEMMs against fp32), margin 1. Measured on an MI355X:
    fused against unfused 1.9e-7, unfused GPU against CPU fp32 1.3e-1."""
    env_g, algo_g, env_c, algo_c, mb_g, mb_c = _pair()
    h_f, hx_f = algo_g.cbf_and_jacobian(mb_g.graph(env_g), algo_g.cbf)
    monkeypatch.setenv("GCBF_NO_FUSED_EDGE", "1")
    monkeypatch.setattr(ops, "crazyflie_edge_jac", _boom)
    h_u, hx_u = algo_g.cbf_and_jacobian(mb_g.graph(env_g), algo_g.cbf)
    monkeypatch.undo()
    h_c, hx_c = algo_c.cbf_and_jacobian(mb_c.graph(env_c), algo_c.cbf)
    assert hx_f.shape == (B_E2E, N_E2E, N_E2E, 12)
    assert torch.equal(h_f, h_u)
    d_arm, d_yard = nerr(hx_f, hx_u), nerr(hx_u, hx_c)
    print(f"\n[cbf_and_jacobian] fused-vs-unfused {d_arm:.3e}  unfused-vs-cpu-fp32 {d_yard:.3e}")
    assert float(hx_u.abs().max()) > 0
    assert d_arm <= 1.0 * d_yard, (d_arm, d_yard)


# ---- HIP graph ------------------------------------------------------------------------
def test_graphed_rollout_matches_eager():
    from gcbfplus_amd.trainer.graphing import GraphedRolloutStep
    from gcbfplus_amd.trainer.utils import collect_rollout

    env, algo = _make("cuda")
    assert env.fused_edge
    rng = np.random.default_rng(24)
    g = env.reset(2, rng)
    ro_eager = collect_rollout(env, algo.step, g)
    graphed = GraphedRolloutStep(env, algo.step)
    ro_graph = collect_rollout(env, algo.step, g, graphed)
    assert not graphed.broken and graphed.graph is not None
    assert ro_eager.rewards.shape[1] == 4
    assert torch.allclose(ro_eager.states, ro_graph.states, atol=1e-5)
    assert torch.allclose(ro_eager.rewards, ro_graph.rewards, atol=1e-4)
    assert torch.equal(ro_eager.masks, ro_graph.masks)
    # second rollout with fresh worlds through the SAME captured graph
    g2 = env.reset(2, rng)
    ro_eager2 = collect_rollout(env, algo.step, g2)
    ro_graph2 = collect_rollout(env, algo.step, g2, graphed)
    assert torch.allclose(ro_eager2.states, ro_graph2.states, atol=1e-5)


# ---- dispatch -------------------------------------------------------------------------
def _boom(*args, **kwargs):
    raise AssertionError("path taken")


def test_dispatch_default_takes_fused_input(monkeypatch):
    env, algo = _make("cuda")
    g = env.reset(2, np.random.default_rng(25))
    monkeypatch.setattr(CrazyFlie, "edge_feats", _boom)
    assert not os.environ.get("GCBF_NO_FUSED_EDGE")
    assert env.fused_edge is True
    e, mi = algo._net_inputs(g)
    assert e is None
    assert mi.shape == (2, N_E2E, N_E2E + 1 + R, 32) and mi.dtype == torch.bfloat16
    assert torch.isfinite(algo.act(g)).all() and torch.isfinite(algo.get_cbf(g)).all()


def test_dispatch_opt_outs_take_edge_feats(monkeypatch):
    monkeypatch.setattr(CrazyFlie, "edge_msg_in", _boom)
    env, algo = _make("cuda")
    g = env.reset(2, np.random.default_rng(26))
    with pytest.raises(AssertionError, match="path taken"):
        algo._net_inputs(g)  # the spy is live
    D = N_E2E + 1 + R

    def takes_edge_feats(algo_, g_):
        e, mi = algo_._net_inputs(g_)
        return mi is None and e.shape == (2, N_E2E, D, 12) and e.dtype == torch.float32

    monkeypatch.setenv("GCBF_NO_FUSED_EDGE", "1")
    assert env.fused_edge is False and takes_edge_feats(algo, g)
    monkeypatch.delenv("GCBF_NO_FUSED_EDGE")

    class SubFlie(CrazyFlie):
        pass

    env_s, algo_s = _make("cuda", cls=SubFlie)
    assert env_s.fused_edge is False and takes_edge_feats(algo_s, g)

    env_c, algo_c = _make("cpu")
    g_c = env_c.reset(2, np.random.default_rng(26))
    assert env_c.fused_edge is False and takes_edge_feats(algo_c, g_c)

    env_2, algo_2 = _make("cuda", gnn_layers=2)
    assert env_2.fused_edge is True and takes_edge_feats(algo_2, g)


# ---- host refusals: nothing is launched --------------------------------------------------
def test_host_refusals():
    from gcbfplus_amd import _C

    N = 3
    V, D = 2 * N + N * R, N + 1 + R
    st = torch.zeros(2, V, 12, device="cuda")
    dX = torch.zeros(2, N, D, 32, device="cuda", dtype=torch.bfloat16)
    _C.edge_msg_in_fwd(st, N, R, 3, 32, COMM, 2)  # the accepted call
    _C.edge_msg_in_bwd(st, dX, N, R, 3, COMM, 2)
    bad_fwd = [
        (torch.zeros(2, V, 4, device="cuda"), N, R, 3, 32),    # S = 4
        (st, N, R, 2, 32),                                      # pdim = 2
        (st, N, R, 3, 64),                                      # KP = 64
        (torch.zeros(2, V + 1, 12, device="cuda"), N, R, 3, 32),  # V != 2N + N R
        (torch.zeros(2, V, 24, device="cuda")[..., ::2], N, R, 3, 32),  # non-contiguous
        (st.double(), N, R, 3, 32),                             # f64
    ]
    for s, n, r, pdim, kp in bad_fwd:
        with pytest.raises(RuntimeError):
            _C.edge_msg_in_fwd(s, n, r, pdim, kp, COMM, 2)
    with pytest.raises(RuntimeError, match="unknown mode"):
        _C.edge_msg_in_fwd(st, N, R, 3, 32, COMM, 7)
    with pytest.raises(RuntimeError, match="unknown mode"):
        _C.edge_msg_in_bwd(st, dX, N, R, 3, COMM, 7)
    for bad_dx in (dX.float(), dX[:, :, :-1].contiguous(), dX[..., :16].contiguous()):
        with pytest.raises(RuntimeError):
            _C.edge_msg_in_bwd(st, bad_dx, N, R, 3, COMM, 2)
    with pytest.raises(RuntimeError):
        _C.edge_msg_in_bwd(st, dX, N, R, 2, COMM, 2)
    ge = torch.zeros(2, N, D, 12, device="cuda")
    _C.crazyflie_edge_jac(st, ge, N, R, COMM)
    for s, g_ in ((st.double(), ge), (st, ge.double()), (st, ge[:, :, :-1].contiguous()),
                  (torch.zeros(2, V + 1, 12, device="cuda"), ge)):
        with pytest.raises(RuntimeError):
            _C.crazyflie_edge_jac(s, g_, N, R, COMM)
    torch.cuda.synchronize()
