"""GPU tests for the fused loss prologue of DubinsCar, LinearDrone and
SingleIntegrator (ops.{dubins,drone,si}_loss_prep, env_loss_prep_{fwd,bwd}_kernel
over the env structs of loss_prep_envs.h) and its dispatch through
``env.loss_prep`` / ``GCBFPlus._loss``.

Oracle, input generator and margins: tests/loss_prep_envs_common.py (f64 numpy,
validated against the CPU f32 eager path by tests/test_loss_prep_envs_cpu.py).
Every case's margins, and the main case's branch presence, are asserted on the
CPU before the GPU is used.

Accuracy rule (PARITY.md), per action / state component ``c``:

    err_fused_c <= 8 * max(err_eager_c, 2^-23 * max|ref_c|)

``eager`` is the composed torch prologue on the same GPU (2*raw + env.u_ref,
env.forward_graph, autograd), both arms against the oracle. The fused arm is
always called through the env's ``loss_prep`` hook, so the limits and
parameters the hook passes are under test too.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import loss_prep_envs_common as C
from gcbfplus_amd import ops
from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.env import make_env
from gcbfplus_amd.trainer.data import FlatBatch
from gcbfplus_amd.utils.graph import GraphBatch

MAIN = C.SHAPES[0]
_CASES = {}


def _case(name, B, N, stop=True):
    """(env, graph, raw, oracle, dact, dbig, case) on the GPU for a shape;
    computed once and shared (read-only) by the tests that use it."""
    key = (name, B, N, stop)
    if key not in _CASES:
        env = make_env(name, num_agents=N, area_size=3.0, max_step=8, device="cuda")
        env.enable_stop = stop
        case = C.make_case(env, B, N, C.SEEDS[(name, B, N)])
        C.check_margins(case)
        if (B, N) == MAIN:
            C.check_presence(case)
        orc = C.oracle_of(case, enable_stop=stop)
        mask = torch.zeros(B, N, N + 1 + env.n_rays, dtype=torch.bool, device="cuda")
        g = GraphBatch(case["states"].cuda(), mask, N, env.n_rays)
        _CASES[key] = (env, g, case["raw"].cuda(), orc, case["dact"].cuda(),
                       case["dbig"].cuda(), case)
    return _CASES[key]


def _fused(env, g, raw):
    raw = raw.detach().clone().requires_grad_(True)
    prep = env.loss_prep(g, raw)
    assert prep is not None, "hook declined on the GPU"
    return raw, prep[0], prep[1]


def _grad(raw, action, big, dact, dbig):
    outs, cots = [], []
    if dact is not None:
        outs.append(action), cots.append(dact)
    if dbig is not None:
        outs.append(big), cots.append(dbig)
    (gr,) = torch.autograd.grad(outs, raw, cots, retain_graph=True)
    return gr


def _mask(a, shape):
    return torch.from_numpy(np.ascontiguousarray(a.reshape(shape))).cuda()


def _check_forward(name, B, N, stop=True):
    env, g, raw, orc, _, _, _ = _case(name, B, N, stop)
    sp = C.SPEC[name]
    _, act_f, big_f = _fused(env, g, raw)
    _, act_e, big_e = C.eager_prologue(env, g, raw)
    assert act_f.shape == (B, N, sp["NU"]) and big_f.shape == (2 * B,) + tuple(g.states.shape[1:])
    C.assert_8x(act_f, act_e, orc.action, sp["anames"], f"{name} action B={B} N={N}")
    C.assert_8x(big_f[B:, :N], big_e[B:, :N], orc.nxt, sp["snames"], f"{name} next B={B} N={N}")
    assert torch.equal(big_f[:B], g.states)
    assert torch.equal(big_f[B:, N:], g.states[:, N:])
    return act_f, big_f


def _check_grad(name, B, N, stop=True):
    env, g, raw, orc, dact, dbig, case = _case(name, B, N, stop)
    rf, act_f, big_f = _fused(env, g, raw)
    re, act_e, big_e = C.eager_prologue(env, g, raw)
    ga = _grad(rf, act_f, big_f, dact, None)
    gb = _grad(rf, act_f, big_f, None, dbig)
    gab = _grad(rf, act_f, big_f, dact, dbig)
    ge = _grad(re, act_e, big_e, dact, dbig)
    assert ((gab - (ga + gb)).abs() <= C.EPS32 * (ga.abs() + gb.abs())).all()
    C.assert_8x(gab, ge, C.oracle_draw(case, orc), C.SPEC[name]["anames"],
                f"{name} draw B={B} N={N}")
    return rf, act_f, big_f, gab


# ---- main case: values, gradients, exact properties ---------------------------------
@pytest.mark.parametrize("name", C.ENVS)
def test_forward_values(name):
    B, N = MAIN
    act_f, _ = _check_forward(name, B, N)
    # unclamped: entries beyond the action limit stay there
    assert (act_f.abs() > C.SPEC[name]["alim"]).any()


@pytest.mark.parametrize("name", C.ENVS)
def test_gradients(name):
    B, N = MAIN
    rf, act_f, big_f, gab = _check_grad(name, B, N)
    _, _, _, _, dact, dbig, _ = _case(name, B, N)
    # cotangents on the copied rows never reach raw
    other = dbig.clone()
    other[:B] = torch.randn_like(other[:B]) * 3
    other[B:, N:] = torch.randn_like(other[B:, N:]) * 3
    assert torch.equal(_grad(rf, act_f, big_f, dact, other), gab)


@pytest.mark.parametrize("name", C.ENVS)
def test_clamp_masks_are_exact(name):
    B, N = MAIN
    env, g, raw, orc, dact, dbig, _ = _case(name, B, N)
    sp = C.SPEC[name]
    rf, act_f, big_f = _fused(env, g, raw)
    gab = _grad(rf, act_f, big_f, dact, dbig)
    # a component whose pre-clamp action is outside its limit: exactly 2*daction
    out = _mask(~orc.m_act, (B, N, sp["NU"]))
    assert out.any() and not out.all()
    assert torch.equal(gab[out], (2 * dact)[out])
    moving = out.new_ones(B, N, 1) if name != "DubinsCar" else ~_mask(orc.stop, (B, N, 1))
    live = ~out & moving
    assert live.any() and not torch.equal(gab[live], (2 * dact)[live])
    # a clipped velocity contributes exactly zero
    clipped = _mask(~orc.m_state, (B, N, sp["S"]))
    if np.isfinite(sp["slim"]).any():
        assert clipped.any()
        only = torch.zeros_like(dbig)
        only[B:, :N] = torch.where(clipped, dbig[B:, :N], torch.zeros_like(dbig[B:, :N]))
        assert (_grad(rf, act_f, big_f, None, only) == 0).all()
    else:
        assert not clipped.any()  # SingleIntegrator: no state limit
    if name == "DubinsCar":
        # inside the stop radius: next == current bit for bit, draw == 2*daction
        stop = _mask(orc.stop, (B, N))
        assert stop.any() and not stop.all()
        assert torch.equal(big_f[B:, :N][stop], g.states[:, :N][stop])
        assert torch.equal(gab[stop], (2 * dact)[stop])


# ---- edge shapes -----------------------------------------------------------------------
@pytest.mark.parametrize("name", C.ENVS)
def test_single_agent_single_world(name):
    _check_forward(name, 1, 1)
    _check_grad(name, 1, 1)


@pytest.mark.parametrize("name", C.ENVS)
def test_many_agents_partial_last_block(name):
    """B=2, N=260: 520 backward threads (2 blocks + 8 lanes) and 18720 / 35360
    forward rows; the forward launches one thread per two rows, so every
    thread takes a second trip of the grid-stride loop and the last block's is
    partial."""
    _check_forward(name, 2, 260)
    _check_grad(name, 2, 260)


def test_dubins_without_stop():
    """enable_stop = False: the agents inside the stop radius move."""
    B, N = MAIN
    _, big_f = _check_forward("DubinsCar", B, N, stop=False)
    _check_grad("DubinsCar", B, N, stop=False)
    env, g, _, _, _, _, case = _case("DubinsCar", B, N, stop=False)
    inside = _mask(C.oracle_of(case, enable_stop=True).stop, (B, N))
    assert inside.any()
    assert (big_f[B:, :N][inside] != g.states[:, :N][inside]).any(-1).all()


# ---- capture -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.ENVS)
def test_capture_replays_bit_equal(name):
    B, N = MAIN
    env, g, raw, _, dact, dbig, _ = _case(name, B, N)
    s_raw = raw.detach().clone()

    def body():
        # A fresh leaf per call, and nothing returned that keeps the autograd
        # graph alive: a leaf's gradient accumulator remembers the stream it
        # was created on, and one surviving from the warm-up (default stream)
        # would make autograd order the capture stream against the default
        # stream in the middle of the capture.
        leaf = s_raw.detach().requires_grad_(True)
        action, big = env.loss_prep(g, leaf)
        (gr,) = torch.autograd.grad([action, big], leaf, [dact, dbig])
        return action.detach(), big.detach(), gr

    torch.cuda.synchronize()
    for _ in range(3):  # warm-up on the default stream
        plain = body()
    plain = [t.clone() for t in plain]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = body()
    torch.cuda.synchronize()
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for t, p in zip(outs, plain):
            assert torch.equal(t, p)


# ---- dispatch -------------------------------------------------------------------------------
def _minibatch(name, device, n=3, batch=4, seed=500):
    torch.manual_seed(seed)
    env = make_env(name, num_agents=n, area_size=2.0, max_step=8, device=device)
    algo = make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim, n_agents=n,
                     gnn_layers=1, batch_size=batch, buffer_size=8, horizon=4,
                     inner_epoch=1, seed=0)
    return env, algo


def _loss_and_grads(algo, mb):
    for p in list(algo.cbf.parameters()) + list(algo.actor.parameters()):
        if p.grad is not None:  # views of the optimizer's flat buffer on the GPU
            p.grad.zero_()
    total, _ = algo._loss(mb, want_info=False)
    total.backward()
    flat = lambda net: torch.cat([p.grad.reshape(-1) for p in net.parameters()  # noqa: E731
                                  if p.grad is not None]).detach().double().cpu().numpy()
    return float(total.detach()), flat(algo.actor), flat(algo.cbf)


@pytest.mark.parametrize("name", C.ENVS)
def test_dispatch_loss_prep_hook(name, monkeypatch):
    B, N = MAIN
    env, g, raw, _, _, _, case = _case(name, B, N)
    monkeypatch.delenv("GCBF_NO_FUSED_PREP", raising=False)
    prep = env.loss_prep(g, raw)
    assert isinstance(prep, tuple) and len(prep) == 2
    assert prep[0].shape == raw.shape and prep[1].shape[0] == 2 * B

    cpu = make_env(name, num_agents=N, area_size=3.0, max_step=8, device="cpu")
    g_cpu = GraphBatch(case["states"], g.mask.cpu(), N, env.n_rays)
    assert cpu.loss_prep(g_cpu, raw.cpu()) is None

    class Sub(type(env)):
        pass

    sub = Sub(N, 3.0, max_step=8, params=dict(type(env).PARAMS), device="cuda")
    assert sub.loss_prep(g, raw) is None

    monkeypatch.setenv("GCBF_NO_FUSED_PREP", "1")
    assert env.loss_prep(g, raw) is None


@pytest.mark.parametrize("name", C.ENVS)
def test_loss_runs_on_the_fused_prologue(name, monkeypatch):
    """_loss on a small minibatch (n=3, batch 4) calls the hook and takes its
    pair; loss and flat actor / CBF gradients agree with the
    GCBF_NO_FUSED_PREP=1 run of the same minibatch under the 8x rule, both
    against the CPU f32 run of the same parameters."""
    monkeypatch.delenv("GCBF_NO_FUSED_PREP", raising=False)
    env, algo = _minibatch(name, "cuda")
    n, batch = 3, 4
    g = env.reset(batch, np.random.default_rng(500))
    safe = torch.rand(batch, n, device="cuda") < 0.5
    unsafe = ~safe & (torch.rand(batch, n, device="cuda") < 0.5)
    mb = FlatBatch(g.states, g.mask, safe, unsafe,
                   torch.randn(batch, n, env.action_dim, device="cuda"))

    cls, took = type(env), []
    orig_hook, orig_fg = cls.loss_prep, cls.forward_graph

    def hook(self, graph, raw):
        out = orig_hook(self, graph, raw)
        took.append(out is not None)
        return out

    eager_calls = []

    def fg(self, graph, action):
        eager_calls.append(1)
        return orig_fg(self, graph, action)

    monkeypatch.setattr(cls, "loss_prep", hook)
    monkeypatch.setattr(cls, "forward_graph", fg)
    fused = _loss_and_grads(algo, mb)
    assert took == [True] and not eager_calls
    monkeypatch.setenv("GCBF_NO_FUSED_PREP", "1")
    eager = _loss_and_grads(algo, mb)
    assert took == [True, False] and len(eager_calls) == 1
    monkeypatch.delenv("GCBF_NO_FUSED_PREP")

    _, cpu_algo = _minibatch(name, "cpu")
    cpu_algo.actor.load_state_dict(algo.actor.state_dict())
    cpu_algo.cbf.load_state_dict(algo.cbf.state_dict())
    mb_cpu = FlatBatch(*[t.cpu() for t in mb])
    ref = _loss_and_grads(cpu_algo, mb_cpu)

    for what, f, e, r in zip(("loss", "actor grad", "cbf grad"), fused, eager, ref):
        f, e, r = (np.atleast_1d(np.asarray(x, np.float64)) for x in (f, e, r))
        assert f.shape == r.shape and np.isfinite(f).all()
        ef, ee = np.abs(f - r).max(), np.abs(e - r).max()
        bound = 8 * max(ee, C.EPS32 * np.abs(r).max())
        print(f"\n[{name} _loss {what}] err_eager {ee:.3e} err_fused {ef:.3e} bound {bound:.3e}")
        assert ef <= bound, (name, what, ef, ee, bound)
    assert np.abs(fused[1]).max() > 0


# ---- bad input ---------------------------------------------------------------------------------
def _entry_points(env, name):
    """fwd(states, raw, N, *mats) and bwd(states, action, daction, dbig, N, *mats)
    of the extension with the env's parameters; mats = the gain / A / B."""
    from gcbfplus_amd import _C

    lim = [[float(v) for v in t] for pair in (env.action_lim(), env.state_lim()) for t in pair]
    comm = env._params["comm_radius"]
    if name == "DubinsCar":
        tail = (env.dt, comm, 0.5 * env._params["car_radius"], True, *lim)
        return ((), lambda st, raw, N: _C.dubins_loss_prep_fwd(st, raw, N, *tail),
                lambda st, a, da, db, N: _C.dubins_loss_prep_bwd(st, a, da, db, N, *tail))
    tail = (env.dt, comm, *lim)
    if name == "LinearDrone":
        mats = (env._K.cuda(), env._A_t.cuda(), env._B_t.cuda())
        return (mats, lambda st, raw, N, *m: _C.drone_loss_prep_fwd(st, raw, *m, N, *tail),
                lambda st, a, da, db, N, *m: _C.drone_loss_prep_bwd(st, *m, a, da, db, N, *tail))
    mats = (env._K.cuda(),)
    return (mats, lambda st, raw, N, *m: _C.si_loss_prep_fwd(st, raw, *m, N, *tail),
            lambda st, a, da, db, N, *m: _C.si_loss_prep_bwd(st, *m, a, da, db, N, *tail))


@pytest.mark.parametrize("name", C.ENVS)
def test_binding_refuses_bad_input(name):
    B, N = MAIN
    env, g, raw, _, dact, dbig, _ = _case(name, B, N)
    sp, st = C.SPEC[name], g.states
    mats, fwd, bwd = _entry_points(env, name)
    action, big = fwd(st, raw, N, *mats)
    assert torch.equal(big[:B], st)
    nc = lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)  # noqa: E731
    bad_fwd = [
        (nc(st), raw, N),                                  # non-contiguous
        (st, nc(raw), N),
        (st.double(), raw, N),                             # dtype
        (st, raw.double(), N),
        (st.cpu(), raw, N),                                # device
        (st, raw.cpu(), N),
        (st[..., : sp["S"] - 1].contiguous(), raw, N),     # wrong S
        (st, raw[..., : sp["NU"] - 1].contiguous(), N),    # wrong NU
        (st, raw, N + 1),                                  # raw does not match N
        (st, raw[:, : N - 1].contiguous(), N),
        (st[:, : 2 * N - 1].contiguous(), raw, N),         # V < 2N
    ]
    for args in bad_fwd:
        with pytest.raises(RuntimeError):
            fwd(*args, *mats)
    bad_bwd = [
        (st, action, nc(dact), dbig, N),
        (st, action, dact[..., : sp["NU"] - 1].contiguous(), dbig, N),
        (st, action, dact, dbig[..., : sp["S"] - 1].contiguous(), N),
        (st, action, dact, dbig[:B].contiguous(), N),
        (st, action, dact.double(), dbig, N),
        (st, action.cpu(), dact, dbig, N),
        (st, action, dact, dbig, N - 1),
    ]
    for args in bad_bwd:
        with pytest.raises(RuntimeError):
            bwd(*args, *mats)
    for k in range(len(mats)):  # gain / A / B: shape, device, dtype
        for wrong in (mats[k][:-1].contiguous(), mats[k].cpu(), mats[k].double()):
            m = mats[:k] + (wrong,) + mats[k + 1:]
            with pytest.raises(RuntimeError):
                fwd(st, raw, N, *m)
            with pytest.raises(RuntimeError):
                bwd(st, action, dact, dbig, N, *m)
    torch.cuda.synchronize()
