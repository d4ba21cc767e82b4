"""CPU side of the fused loss prologue of DubinsCar, LinearDrone and
SingleIntegrator: without a GPU the hooks decline, ``GCBFPlus._loss`` runs its
composed (eager) branch and the ops refuse CPU tensors; the input generator's
margin and presence conditions hold for every case of the GPU test; and the
f64 oracle of the GPU test (tests/loss_prep_envs_common.py) is validated
against the CPU f32 eager path on the main case.

That last bound was not fixed in advance: ``MEASURED`` holds the largest
|eager_cpu_f32 - oracle| per component as measured when the test was written
(torch CPU, main case B=3 N=5; all of it fp32 rounding, a few 2^-24 of the
component's magnitude), and the test asserts 4x those figures to cover other
libm / BLAS builds. PARITY.md lists them next to the GPU table.
"""
import numpy as np
import pytest
import torch

import loss_prep_envs_common as C
from gcbfplus_amd import ops
from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.env import make_env
from gcbfplus_amd.trainer.data import FlatBatch
from gcbfplus_amd.utils.graph import GraphBatch

# (env, enable_stop) -> output -> measured max error per component
MEASURED = {
    ("DubinsCar", True): dict(action=(4.68e-07, 3.04e-07),
                              next=(9.13e-08, 1.10e-07, 2.69e-07, 1.20e-08),
                              draw=(1.44e-07, 9.78e-08)),
    ("DubinsCar", False): dict(action=(4.68e-07, 3.04e-07),
                               next=(9.13e-08, 1.10e-07, 2.69e-07, 1.20e-08),
                               draw=(1.44e-07, 9.78e-08)),
    ("LinearDrone", True): dict(action=(5.53e-08, 7.26e-08, 7.97e-08),
                                next=(9.74e-08, 7.14e-08, 7.10e-08, 2.59e-08, 4.07e-08,
                                      2.91e-08),
                                draw=(1.08e-07, 1.67e-07, 7.16e-08)),
    ("SingleIntegrator", True): dict(action=(1.20e-07, 1.20e-07),
                                     next=(5.69e-08, 6.06e-08),
                                     draw=(5.97e-08, 3.58e-08)),
}


def _graph(env, case):
    B, N = case["B"], case["N"]
    mask = torch.zeros(B, N, N + 1 + env.n_rays, dtype=torch.bool)
    return GraphBatch(case["states"], mask, N, env.n_rays)


def _setup(name, n=3, batch=4, seed=7):
    torch.manual_seed(seed)
    env = make_env(name, num_agents=n, area_size=2.0, max_step=8, device="cpu")
    algo = make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim, n_agents=n,
                     gnn_layers=1, batch_size=batch, buffer_size=8, horizon=4,
                     inner_epoch=1, seed=0)
    g = env.reset(batch, np.random.default_rng(seed))
    safe = torch.rand(batch, n) < 0.5
    unsafe = ~safe & (torch.rand(batch, n) < 0.5)
    mb = FlatBatch(g.states, g.mask, safe, unsafe, torch.randn(batch, n, env.action_dim))
    return env, algo, g, mb


@pytest.mark.parametrize("name", C.ENVS)
def test_hook_declines_and_loss_takes_the_eager_branch_on_cpu(name, monkeypatch):
    monkeypatch.delenv("GCBF_NO_FUSED_PREP", raising=False)
    env, algo, g, mb = _setup(name)
    assert type(env).__name__ == name
    raw = torch.randn(g.batch_size, env.num_agents, env.action_dim)
    assert env.loss_prep(g, raw) is None
    calls = []
    orig = type(env).forward_graph

    def spy(self, graph, action):
        calls.append(1)
        return orig(self, graph, action)

    monkeypatch.setattr(type(env), "forward_graph", spy)
    total, info = algo._loss(mb, want_info=True)
    assert calls, "eager prologue not taken"
    assert torch.isfinite(total) and all(np.isfinite(v) for v in info.values())
    total.backward()
    grads = [p.grad for p in algo.actor.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads)
    assert any(bool((x != 0).any()) for x in grads)


def test_ops_refuse_cpu_tensors():
    lim2, lim4, lim6, lim3 = ([(-1.0,) * k, (1.0,) * k] for k in (2, 4, 6, 3))
    with pytest.raises(NotImplementedError):
        ops.dubins_loss_prep(torch.zeros(1, 18, 4), torch.zeros(1, 1, 2), 1, 0.03, 0.5, 0.025,
                             True, lim2, lim4)
    with pytest.raises(NotImplementedError):
        ops.drone_loss_prep(torch.zeros(1, 18, 6), torch.zeros(1, 1, 3), torch.zeros(3, 6),
                            torch.zeros(6, 6), torch.zeros(6, 3), 1, 0.03, 0.5, lim3, lim6)
    with pytest.raises(NotImplementedError):
        ops.si_loss_prep(torch.zeros(1, 34, 2), torch.zeros(1, 1, 2), torch.zeros(2, 2), 1, 0.03,
                         0.5, lim2, lim2)


@pytest.mark.parametrize("name", C.ENVS)
def test_input_margins_and_presence(name):
    for B, N in C.SHAPES:
        env = make_env(name, num_agents=N, area_size=3.0, max_step=8, device="cpu")
        case = C.make_case(env, B, N, C.SEEDS[(name, B, N)])
        C.check_margins(case)
        if (B, N) == C.SHAPES[0]:
            C.check_presence(case)
            if name == "DubinsCar":  # the stop-radius agents move with the stop off
                on, off = C.oracle_of(case), C.oracle_of(case, enable_stop=False)
                assert on.stop.any() and not off.stop.any()
                assert (on.nxt[on.stop] != off.nxt[on.stop]).any(-1).all()


@pytest.mark.parametrize("name,stop", sorted(MEASURED))
def test_oracle_against_cpu_eager(name, stop):
    B, N = C.SHAPES[0]
    env = make_env(name, num_agents=N, area_size=3.0, max_step=8, device="cpu")
    env.enable_stop = stop
    case = C.make_case(env, B, N, C.SEEDS[(name, B, N)])
    orc = C.oracle_of(case, enable_stop=stop)
    raw, action, big = C.eager_prologue(env, _graph(env, case), case["raw"])
    (gr,) = torch.autograd.grad([action, big], raw, [case["dact"], case["dbig"]])
    got = dict(action=C.errors(action, orc.action), next=C.errors(big[B:, :N], orc.nxt),
               draw=C.errors(gr, C.oracle_draw(case, orc)))
    for what, err in got.items():
        bound = 4 * np.asarray(MEASURED[(name, stop)][what])
        print(f"\n[{name} stop={stop} {what}] err {err} bound {bound}")
        assert (err <= bound).all(), (name, stop, what, err, bound)
    # the copied rows of the composed path: what the fused kernel must reproduce
    assert torch.equal(big[:B], case["states"])
    assert torch.equal(big[B:, N:], case["states"][:, N:])
