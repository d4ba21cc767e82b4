"""GPU tests for the fused CrazyFlie step (crazyflie_step_kernel part A +
raytrace_sphere_topk graph-mode part B).

Oracle: an f64 numpy RK4 built from ``env._xdot_hl_np`` plus the f64 state
clip, one agent at a time -- it shares no code with the kernel. The eager
fp32 path (``GCBF_NO_FUSED_ENV``) is evaluated against the same oracle in the
same test, and per state component ``c`` the fused path must satisfy

    err_fused_c <= 8 * max(err_eager_c, 2^-23 * max|ref_c|)

(both are fp32 evaluations of the same formulae; FMA contraction and
summation order move the rounding by a small multiple, while a wrong
constant, index or RK4 stage shows up at 1e-3 or worse). Discrete outputs
(cost, masks) are compared exactly, under the precondition -- asserted on
the oracle -- that no distance sits within 1e-4 of its threshold.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gcbfplus_amd.env import make_env
from gcbfplus_amd.env.crazyflie import CrazyFlie
from gcbfplus_amd.env.obstacle import Sphere
from gcbfplus_amd.env.utils import beam_dirs_3d

EPS32 = 2.0 ** -23
GAP = 1e-4  # no-near-threshold precondition
NAMES = ("x", "y", "z", "psi", "theta", "phi", "u", "v", "w", "r", "q", "p")


# ---- oracle + helpers --------------------------------------------------------
def _oracle_step(env, agent, action):
    """f64 RK4 + clip_state for (..., 12) states / (..., 4) raw actions."""
    lo, hi = (t.double().numpy() for t in env.state_lim())
    dt = env.dt
    f = env._xdot_hl_np  # clips the action itself
    a = np.asarray(agent, np.float64).reshape(-1, 12)
    u = np.asarray(action, np.float64).reshape(-1, 4)
    out = np.empty_like(a)
    for i in range(a.shape[0]):
        x, ui = a[i], u[i]
        k1 = f(x, ui)
        k2 = f(x + 0.5 * dt * k1, ui)
        k3 = f(x + 0.5 * dt * k2, ui)
        k4 = f(x + dt * k3, ui)
        out[i] = np.clip(x + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4), lo, hi)
    return out.reshape(np.shape(agent))


def _comp_err(x, ref):
    x = x.detach().double().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.abs(x - ref).reshape(-1, 12).max(0)


def _assert_8x(fused, eager, ref, what):
    ef, ee = _comp_err(fused, ref), _comp_err(eager, ref)
    floor = EPS32 * np.abs(ref).reshape(-1, 12).max(0)
    bound = 8 * np.maximum(ee, floor)
    print(f"\n[{what}] comp  err_eager   err_fused   bound")
    for c in range(12):
        print(f"  {NAMES[c]:>5} {ee[c]:.3e}  {ef[c]:.3e}  {bound[c]:.3e}")
    bad = [NAMES[c] for c in range(12) if not ef[c] <= bound[c]]
    assert not bad, (what, bad, ef, ee, bound)


def _pair_gap(pos, thr):
    """min | |p_i - p_j| - thr | over distinct pairs, pos (B, N, 3) f64."""
    n = pos.shape[1]
    if n < 2:
        return math.inf
    d = np.linalg.norm(pos[:, :, None] - pos[:, None], axis=-1)
    iu = np.triu_indices(n, 1)
    return float(np.abs(d[:, iu[0], iu[1]] - thr).min())


def _sphere_gap(pos, center, radius, r):
    """min | |p - c| - (radius + r) | over agents x spheres."""
    if center.shape[1] == 0:
        return math.inf
    d = np.linalg.norm(pos[:, :, None] - center[:, None], axis=-1)
    return float(np.abs(d - (radius[:, None] + r)).min())


def _lidar_gap(pos, center, radius, n_rays, comm):
    """f64 distance of every beam outcome from a decision boundary: a grazing
    root (disc = 0), a root at the range end (alpha = 1) or at the origin
    (alpha = 0), and the lidar mask threshold alpha * comm = comm - 0.1."""
    if center.shape[1] == 0:
        return math.inf
    e = beam_dirs_3d(n_rays).double().numpy() * comm  # (R, 3)
    a2 = comm * comm
    s = pos[:, :, None, None, :] - center[:, None, :, None, :]  # (B,N,K,1,3)
    bq = 2.0 * (s * e).sum(-1)  # (B,N,K,R)
    cq = (s * s).sum(-1) - radius[:, None, :, None] ** 2
    disc = (bq * bq - 4 * a2 * cq) / (4 * a2 * a2)  # (half root separation)^2
    mid = -bq / (2 * a2)
    near = (mid > -0.1) & (mid < 1.1)
    gap = float(np.sqrt(np.abs(disc[near])).min()) if near.any() else math.inf
    ok = disc >= 0
    sq = np.sqrt(np.where(ok, disc, 0.0))
    for root in (mid - sq, mid + sq):
        rt = root[ok]
        if rt.size:
            gap = min(gap, float(np.abs(rt).min()), float(np.abs(rt - 1.0).min()),
                      float(np.abs(rt * comm - (comm - 0.1)).min()))
    return gap


def _eager_step(env, g, a):
    os.environ["GCBF_NO_FUSED_ENV"] = "1"
    try:
        return env.step(g, a)
    finally:
        os.environ.pop("GCBF_NO_FUSED_ENV")


def _rand_states(rng, pos):
    """Angles +-0.7 (theta/phi clip at pi/4), body velocities +-0.3 (at the
    clip), body rates +-8 (clip at 10)."""
    B, N, _ = pos.shape
    ang = rng.uniform(-0.7, 0.7, (B, N, 3))
    vel = rng.uniform(-0.3, 0.3, (B, N, 3))
    rate = rng.uniform(-8.0, 8.0, (B, N, 3))
    return np.concatenate([pos, ang, vel, rate], -1)


def _inputs(B, N, n_obs, seed, area=3.0):
    """Randomised single-step inputs with planted near-collision / in-sphere /
    comm-boundary pairs. float32 CPU tensors: agent, goal, action, Sphere."""
    rng = np.random.default_rng(seed)
    r, comm = CrazyFlie.PARAMS["drone_radius"], CrazyFlie.PARAMS["comm_radius"]
    pos = rng.uniform(0.0, area, (B, N, 3))
    if N >= 5:
        pos[0, 1] = pos[0, 0] + 1.5 * r * np.array([0.6, 0.0, 0.8])  # colliding pair
        pos[1, 1] = pos[1, 0] + np.array([0.95 * comm, 0.0, 0.0])    # just inside comm
        pos[1, 3] = pos[1, 2] + np.array([0.0, 1.05 * comm, 0.0])    # just outside comm
    agent = _rand_states(rng, pos)
    if N >= 5:
        agent[2, 3, 3:6] = (0.3, 0.75, -0.75)   # theta / phi driven into +-pi/4
        agent[2, 3, 9:12] = (0.0, 8.0, -8.0)
        agent[2, 2, 9:12] = (-14.0, 14.0, 14.0)  # rates still beyond +-10 after the step
    goal = np.zeros((B, N, 12))
    goal[..., :3] = rng.uniform(0.0, area, (B, N, 3))
    goal[0, 0, :3] = pos[0, 0] + 0.3  # one goal within comm (coef = 1 branch)
    action = rng.standard_normal((B, N, 4)) * 1.5
    center = np.zeros((B, n_obs, 3))
    radius = np.zeros((B, n_obs))
    if n_obs:
        assert n_obs == 2
        if N >= 5:  # last agent of every world sits inside sphere 0
            center[:, 0] = pos[:, N - 1] + np.array([0.02, 0.0, 0.0])
        else:
            center[:, 0] = pos[:, N - 1] + np.array([-0.6, 0.2, 0.1])
        radius[:, 0] = 0.2
        center[:, 1] = pos[:, 0] + np.array([0.5, 0.1, 0.05])  # in lidar range
        radius[:, 1] = 0.25
    f32 = lambda x: torch.from_numpy(np.asarray(x, np.float32))  # noqa: E731
    return f32(agent), f32(goal), f32(action), Sphere(f32(center), f32(radius))


def _check_single_step(B, N, n_obs, seed):
    env = make_env("CrazyFlie", num_agents=N, area_size=3.0, max_step=8,
                   num_obs=n_obs, device="cuda")
    assert env.params["n_obs"] == n_obs
    p = env.params
    r, comm, R = p["drone_radius"], p["comm_radius"], env.n_rays
    agent, goal, action, obs = _inputs(B, N, n_obs, seed)
    g = env.get_graph(agent.cuda(), goal.cuda(), Sphere(*[t.cuda() for t in obs]))
    a = action.cuda()

    # f64 oracle and the no-near-threshold precondition
    ref = _oracle_step(env, agent.double().numpy(), action.double().numpy())
    cur, nxt = agent[..., :3].double().numpy(), ref[..., :3]
    c64, r64 = obs.center.double().numpy(), obs.radius.double().numpy()
    for pos in (cur, nxt):
        assert _pair_gap(pos, 2 * r) > GAP and _pair_gap(pos, comm) > GAP
        assert _sphere_gap(pos, c64, r64, r) > GAP
    if N >= 5:  # every clip group (theta/phi, uvw, rqp) is hit by some agent
        lim = env.state_lim()[1].double().numpy()
        at_clip = (np.abs(ref) == lim).reshape(-1, 12).any(0)
        assert at_clip[4:6].any() and at_clip[6:9].any() and at_clip[9:].any()
    # lidar decisions of the next scan sit >= 1e-3 from every boundary (the
    # fp32 next positions differ from the oracle by ~1e-7)
    assert _sphere_gap(nxt, c64, r64, 0.0) > 1e-3
    assert _lidar_gap(nxt, c64, r64, p["n_rays"], comm) > 1e-3

    res_f = env._step_fused(g, a)
    res_e = _eager_step(env, g, a)
    sf, se = res_f.graph.states, res_e.graph.states
    mf, me = res_f.graph.mask, res_e.graph.mask
    assert sf.shape == se.shape and mf.shape == me.shape

    _assert_8x(sf[:, :N], se[:, :N], ref, f"step B={B} N={N} n_obs={n_obs}")
    assert torch.equal(sf[:, N:2 * N], g.states[:, N:2 * N])  # goal rows bit-equal
    assert torch.equal(res_f.cost, res_e.cost), (res_f.cost, res_e.cost)
    if N >= 5:
        assert float(res_e.cost.max()) > 0  # planted collision (+ in-sphere) counted
    assert torch.equal(mf[:, :, :N + 1], me[:, :, :N + 1])
    if N >= 5:
        assert bool(me[1, 0, 1]) and not bool(me[1, 2, 3])  # planted comm pairs
    rel = ((res_f.reward - res_e.reward).abs() / res_e.reward.abs()).max()
    assert rel <= 1e-5, rel
    assert not res_f.done.any()

    # hit rows: set-compare per agent (relative, the no-hit rows are ~1e6)
    hf = sf[:, 2 * N:].reshape(B * N, R, 12)
    he = se[:, 2 * N:].reshape(B * N, R, 12)
    assert (hf[..., 3:] == 0).all()
    d = torch.cdist(hf[..., :3], he[..., :3])
    scale = he[..., :3].abs().amax(-1).clamp_min(1.0)
    assert (d.min(dim=2).values / scale).max() < 1e-3
    assert (d.min(dim=1).values / scale).max() < 1e-3

    # lidar mask columns
    if n_obs == 0:
        assert not mf[:, :, N + 1:].any()
        assert not me[:, :, N + 1:].any()
    else:
        env_c = make_env("CrazyFlie", num_agents=N, area_size=3.0, max_step=8,
                         num_obs=n_obs, device="cpu")
        res_c = env_c.step(env_c.get_graph(agent, goal, obs), action)
        # precondition: eager GPU and eager CPU agree on every lidar bit
        assert torch.equal(me[:, :, N + 1:].cpu(), res_c.graph.mask[:, :, N + 1:])
        assert me[:, :, N + 1:].any() and not me[:, :, N + 1:].all()
        assert torch.equal(mf[:, :, N + 1:], me[:, :, N + 1:])


# ---- case 1 / 2: single step ---------------------------------------------------
@pytest.mark.parametrize("n_obs", [0, 2])
def test_single_step_matches_oracle_and_eager(n_obs):
    _check_single_step(B=3, N=5, n_obs=n_obs, seed=101)


@pytest.mark.parametrize("n_obs", [0, 2])
def test_single_agent_single_world(n_obs):
    """N = 1, B = 1: no neighbours, degenerate N x N loops."""
    _check_single_step(B=1, N=1, n_obs=n_obs, seed=102)


# ---- case 3: more agents than threads ---------------------------------------
def test_stride_beyond_one_block_of_threads():
    """N = 260 > 256 threads: second trip of every agent-strided loop."""
    B, N = 2, 260
    env = make_env("CrazyFlie", num_agents=N, area_size=6.0, max_step=8, device="cuda")
    p = env.params
    r, comm = p["drone_radius"], p["comm_radius"]
    rng = np.random.default_rng(103)
    # jittered lattice, spacing 0.8 / jitter 0.025: lattice distances 0.8 and
    # 0.8*sqrt(2) stay > 0.1 away from comm = 1 after jitter and one step
    grid = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(6),
                                indexing="ij"), -1).reshape(-1, 3) * 0.8
    pos = np.stack([grid[rng.permutation(len(grid))[:N]] for _ in range(B)])
    pos = pos + rng.uniform(-0.025, 0.025, pos.shape)
    agent = torch.from_numpy(_rand_states(rng, pos).astype(np.float32))
    goal = torch.zeros(B, N, 12)
    goal[..., :3] = torch.from_numpy(rng.uniform(0, 5.6, (B, N, 3)).astype(np.float32))
    action = torch.from_numpy((rng.standard_normal((B, N, 4)) * 1.5).astype(np.float32))
    empty = Sphere(torch.zeros(B, 0, 3), torch.zeros(B, 0))
    g = env.get_graph(agent.cuda(), goal.cuda(), Sphere(*[t.cuda() for t in empty]))
    a = action.cuda()

    ref = _oracle_step(env, agent.double().numpy(), action.double().numpy())
    for pos64 in (agent[..., :3].double().numpy(), ref[..., :3]):
        assert _pair_gap(pos64, 2 * r) > GAP and _pair_gap(pos64, comm) > GAP

    res_f = env.step(g, a)
    res_e = _eager_step(env, g, a)
    _assert_8x(res_f.graph.states[:, :N], res_e.graph.states[:, :N], ref, "N=260")
    assert torch.equal(res_f.graph.states[:, N:2 * N], g.states[:, N:2 * N])
    assert torch.equal(res_f.graph.mask, res_e.graph.mask)
    aa = res_e.graph.mask[:, :, :N]
    assert aa.any() and not aa.all()
    assert torch.equal(res_f.cost, res_e.cost)
    rel = ((res_f.reward - res_e.reward).abs() / res_e.reward.abs()).max()
    assert rel <= 1e-5, rel


# ---- case 4: open-loop rollout ---------------------------------------------------
def test_open_loop_rollout_matches_oracle():
    """Replay the recorded actions of an eager u_ref rollout through the
    fused step, the eager step and the f64 oracle: fixed actions keep the
    closed-loop feedback out of the comparison."""
    B, N, T = 2, 4, 8
    env = make_env("CrazyFlie", num_agents=N, area_size=2.0, max_step=T, device="cuda")
    g0 = env.reset(B, np.random.default_rng(104))

    os.environ["GCBF_NO_FUSED_ENV"] = "1"
    try:
        actions, g = [], g0
        for _ in range(T):
            actions.append(env.u_ref(g))
            g = env.step(g, actions[-1]).graph
        eager_final = g.agent_states.clone()
    finally:
        os.environ.pop("GCBF_NO_FUSED_ENV")

    g = g0
    for act in actions:
        g = env.step(g, act).graph
    fused_final = g.agent_states.clone()

    x = g0.agent_states.double().cpu().numpy()
    for act in actions:
        x = _oracle_step(env, x, act.double().cpu().numpy())
    assert np.abs(x - g0.agent_states.double().cpu().numpy()).max() > 1e-2  # it moved
    _assert_8x(fused_final, eager_final, x, "8-step open loop")


# ---- case 5: dispatch -----------------------------------------------------------
def _small_graph(env, B=2, seed=105):
    g = env.reset(B, np.random.default_rng(seed))
    torch.manual_seed(seed)
    return g, torch.randn(B, env.num_agents, 4, device="cuda")


def _boom(self, graph, action):
    raise AssertionError("fused path taken")


def test_dispatch_step_takes_fused_path():
    env = make_env("CrazyFlie", num_agents=4, area_size=2.0, max_step=8, device="cuda")
    g, a = _small_graph(env)
    assert not os.environ.get("GCBF_NO_FUSED_ENV")
    r1, r2 = env.step(g, a), env._step_fused(g, a)
    assert torch.equal(r1.graph.states, r2.graph.states)
    assert torch.equal(r1.graph.mask, r2.graph.mask)
    assert torch.equal(r1.reward, r2.reward)
    assert torch.equal(r1.cost, r2.cost)
    assert torch.equal(r1.done, r2.done)


def test_dispatch_env_var_and_subclass_stay_eager(monkeypatch):
    monkeypatch.setattr(CrazyFlie, "_step_fused", _boom)
    env = make_env("CrazyFlie", num_agents=4, area_size=2.0, max_step=8, device="cuda")
    g, a = _small_graph(env)
    with pytest.raises(AssertionError, match="fused path taken"):
        env.step(g, a)  # the spy is live
    monkeypatch.setenv("GCBF_NO_FUSED_ENV", "1")
    res = env.step(g, a)
    assert torch.isfinite(res.graph.states[:, :8]).all()
    monkeypatch.delenv("GCBF_NO_FUSED_ENV")

    class SubFlie(CrazyFlie):
        pass

    sub = SubFlie(4, 2.0, max_step=8, params=dict(CrazyFlie.PARAMS), device="cuda")
    res_s = sub.step(g, a)
    assert torch.equal(res_s.graph.states, res.graph.states)


def test_oversized_lds_request_refused_and_falls_back(monkeypatch):
    """Shapes whose LDS request exceeds 64 KiB: the binding refuses, and
    env.step never launches (eager fallback)."""
    from gcbfplus_amd import _C

    N, R = 1200, 16
    assert _C.crazyflie_step_fits(1000, 0) and not _C.crazyflie_step_fits(N, 0)
    env = make_env("CrazyFlie", num_agents=N, area_size=30.0, max_step=8, device="cuda")
    st = torch.zeros(1, 2 * N + N * R, 12, device="cuda")
    act = torch.zeros(1, N, 4, device="cuda")
    c, rad = torch.zeros(1, 0, 3, device="cuda"), torch.zeros(1, 0, device="cuda")
    with pytest.raises(RuntimeError, match="LDS"):
        _C.crazyflie_step(st, act, c, rad, env._fused_consts(st.device), N, R)

    monkeypatch.setattr(CrazyFlie, "_step_fused", _boom)
    rng = np.random.default_rng(106)
    grid = np.stack(np.meshgrid(*[np.arange(11)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = torch.from_numpy((grid[:N] * 1.3).astype(np.float32))[None]
    agent = torch.cat([pos, torch.zeros(1, N, 9)], -1).cuda()
    g = env.get_graph(agent, agent.clone(), Sphere(c, rad))
    res = env.step(g, act)
    assert torch.isfinite(res.graph.states[:, :N]).all()


# ---- case 6: HIP-graph capture -----------------------------------------------------
def test_graphed_rollout_step_equals_uncaptured():
    from gcbfplus_amd.trainer.graphing import GraphedRolloutStep

    B, N, T = 2, 4, 8
    env = make_env("CrazyFlie", num_agents=N, area_size=2.0, max_step=T, device="cuda")
    g0 = env.reset(B, np.random.default_rng(107))

    plain, g = [], g0
    for _ in range(T):
        res = env.step(g, env.u_ref(g))
        g = res.graph
        plain.append((g.states.clone(), g.mask.clone(), res.reward.clone(),
                      res.cost.clone()))

    graphed = GraphedRolloutStep(env, env.u_ref)
    graphed.reset(g0)
    for t in range(T):
        _, gg, reward, cost, _ = graphed.step()
        st, mk, rw, cs = plain[t]
        assert torch.equal(gg.states, st), t
        assert torch.equal(gg.mask, mk), t
        assert torch.equal(reward, rw) and torch.equal(cost, cs), t
        graphed.advance()
