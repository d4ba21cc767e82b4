"""Shared by tests/test_loss_prep_envs_{cpu,gpu}.py: the input generator and
the f64 numpy oracle for the fused loss prologue of DubinsCar, LinearDrone and
SingleIntegrator, and the project's 8x accuracy rule.

Oracle: plain f64 numpy, written from the formulas, sharing no code with the
kernels or with the env classes' torch code. From an env object it takes
data only (dt, comm / car radius, the f32 LQR gain and the drone's A / B);
the action and state limits are written down here.

  u_ref     DubinsCar: PID heading / speed controller; the other two: error
            clipped by |err / ||err|| * comm|, times K^T, clipped to +-1
  action    2*raw + u_ref, unclamped; a_c = clip(action, +-alim)
  pre       pre-clip next state, affine in a_c:
              SingleIntegrator  x + a_c dt
              LinearDrone       x + (A x + B a_c) dt
              DubinsCar         x + [v cos th, v sin th, 20 a_c0, a_c1] (1 - stop) dt
  nxt       clip(pre, state limits)
  jac       d pre / d a_c (exact: pre is affine in a_c)
  draw      2*daction + 2 * m_act * sum_s m_state_s * jac[s, c] * dnext_s
            with the masks from the oracle's own pre-clamp values

Inputs are generated on the host by construction and by per-agent rejection
in this oracle, so that f32 and f64 cannot disagree on a branch. The margins
(``check_margins``, asserted for every case, none skipped):
  * every pre-clamp action component >= 1e-4 from its limit
  * every pre-clip velocity >= 1e-4 from its limit
  * error norm (Dubins: position norm, with and without the 1e-6) >= 1e-3
    from comm
  * Dubins: goal distance >= 1e-3 from 0.5 * car_radius; theta_diff >= 1e-3
    from 0 and +-pi; theta mod 2pi and theta_t >= 1e-3 from 0, pi, 2pi;
    |inner| <= 0.995 (acos amplifies both arms' error near +-1)
For DubinsCar the action / velocity margins hold with enable_stop on and off.
``check_presence`` (main case): both sides of every clamp and branch occur.
"""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -23
GAP = 1e-4        # actions, velocities
GAP_BRANCH = 1e-3  # norms and angles
INNER_MAX = 0.995

ENVS = ("DubinsCar", "LinearDrone", "SingleIntegrator")

# S, NU, action limit, per-state limit (inf: unlimited), component names
SPEC = {
    "DubinsCar": dict(S=4, NU=2, alim=3.0, slim=(math.inf, math.inf, math.inf, 0.8),
                      snames=("x", "y", "theta", "v"), anames=("omega", "acc")),
    "LinearDrone": dict(S=6, NU=3, alim=1.0, slim=(math.inf,) * 3 + (0.5,) * 3,
                        snames=("x", "y", "z", "vx", "vy", "vz"), anames=("ax", "ay", "az")),
    "SingleIntegrator": dict(S=2, NU=2, alim=1.0, slim=(math.inf, math.inf),
                             snames=("x", "y"), anames=("vx", "vy")),
}

# (B, N) of the cases; (3, 5) is the main case
SHAPES = ((3, 5), (1, 1), (2, 260))
# pinned seeds: the first ones, counting up from 100 / 200 / 300, for which the
# main case has every branch present (check_presence); any seed meets the margins
SEEDS = {
    ("DubinsCar", 3, 5): 111, ("DubinsCar", 1, 1): 200, ("DubinsCar", 2, 260): 300,
    ("LinearDrone", 3, 5): 101, ("LinearDrone", 1, 1): 200, ("LinearDrone", 2, 260): 300,
    ("SingleIntegrator", 3, 5): 100, ("SingleIntegrator", 1, 1): 200,
    ("SingleIntegrator", 2, 260): 300,
}


def env_data(env):
    """The numbers the oracle takes from an env object."""
    d = dict(dt=float(env.dt), comm=float(env._params["comm_radius"]))
    name = type(env).__name__
    if name == "DubinsCar":
        d["stop_r"] = 0.5 * float(env._params["car_radius"])
    else:
        d["K"] = np.asarray(env._K_np, np.float64)
    if name == "LinearDrone":
        d["A"] = np.asarray(env._A_np, np.float64)
        d["Bm"] = np.asarray(env._B_np, np.float64)
    return d


class Oracle:
    """f64 reference for flat agents: agent / goal (n, S), raw (n, NU) as f64
    arrays of f32-representable values. Fields: action, m_act, pre, nxt,
    m_state, jac (n, S, NU), err_norm, and for DubinsCar dist, nrm, theta,
    theta_t, theta_diff, inner, stop, branch (0..3, the omega sign branch)."""

    def __init__(self, name, data, agent, goal, raw, enable_stop=True):
        sp = SPEC[name]
        self.name, self.S, self.NU = name, sp["S"], sp["NU"]
        self.alim = sp["alim"]
        self.slim = np.asarray(sp["slim"])
        x, g = np.asarray(agent, np.float64), np.asarray(goal, np.float64)
        raw = np.asarray(raw, np.float64)
        n, dt, comm = x.shape[0], data["dt"], data["comm"]
        self.jac = np.zeros((n, self.S, self.NU))
        if name == "DubinsCar":
            uref = self._dubins_uref(x, g, comm)
            self.stop = (self.dist < data["stop_r"]) & bool(enable_stop)
        else:
            err = g - x
            self.err_norm = np.sqrt((err * err).sum(-1))
            emax = np.abs(err / np.maximum(self.err_norm, 1e-9)[:, None] * comm)
            uref = np.clip(np.clip(err, -emax, emax) @ data["K"].T, -self.alim, self.alim)
        self.action = 2.0 * raw + uref
        self.m_act = (self.action >= -self.alim) & (self.action <= self.alim)
        ac = np.clip(self.action, -self.alim, self.alim)
        if name == "DubinsCar":
            go = 1.0 - self.stop.astype(np.float64)
            xdot = np.stack([x[:, 3] * np.cos(x[:, 2]), x[:, 3] * np.sin(x[:, 2]),
                             20.0 * ac[:, 0], ac[:, 1]], -1)
            self.pre = x + xdot * go[:, None] * dt
            self.jac[:, 2, 0] = 20.0 * go * dt
            self.jac[:, 3, 1] = go * dt
        elif name == "LinearDrone":
            self.pre = x + (x @ data["A"].T + ac @ data["Bm"].T) * dt
            self.jac[:] = data["Bm"] * dt
        else:
            self.pre = x + ac * dt
            self.jac[:, 0, 0] = self.jac[:, 1, 1] = dt
        self.m_state = (self.pre >= -self.slim) & (self.pre <= self.slim)
        self.nxt = np.clip(self.pre, -self.slim, self.slim)

    def _dubins_uref(self, x, g, comm):
        two_pi = 2.0 * math.pi
        pdx, pdy = x[:, 0] - g[:, 0], x[:, 1] - g[:, 1]
        self.dist = np.sqrt(pdx * pdx + pdy * pdy)
        self.theta_t = np.mod(np.arctan2(-pdy, -pdx), two_pi)
        self.theta = np.mod(x[:, 2], two_pi)
        self.theta_diff = self.theta_t - self.theta
        self.inner = (-pdx * np.cos(self.theta) - pdy * np.sin(self.theta)) / (self.dist + 1e-4)
        between = np.arccos(np.clip(self.inner, -1.0, 1.0))
        fwd = (self.theta_diff < math.pi) & (self.theta_diff >= 0)
        bwd = (self.theta_diff > -math.pi) & (self.theta_diff <= 0)
        le_pi = self.theta <= math.pi
        # branch: 0 le_pi & fwd (+), 1 le_pi & ~fwd (-), 2 ~le_pi & bwd (-), 3 ~le_pi & ~bwd (+)
        self.branch = np.where(le_pi, np.where(fwd, 0, 1), np.where(bwd, 2, 3))
        sign = np.where((self.branch == 0) | (self.branch == 3), 1.0, -1.0)
        omega = np.clip(1.0 * sign * between, -5.0, 5.0)
        self.nrm = np.sqrt(1e-6 + self.dist ** 2)
        self.err_norm = self.dist
        coef = np.where(self.nrm > comm, comm / self.nrm, 1.0)
        acc = -2.5 * x[:, 3] + 2.3 * np.sqrt((coef * pdx) ** 2 + (coef * pdy) ** 2)
        return np.stack([omega, acc], -1)

    def draw(self, daction, dnext):
        """f64 gradient w.r.t. raw for cotangents daction (n, NU) on the action
        and dnext (n, S) on the agent rows of the next-state half."""
        g = np.einsum("ns,nsc->nc", dnext * self.m_state, self.jac)
        return 2.0 * daction + 2.0 * self.m_act * g

    # ---- decision surfaces ------------------------------------------------
    def margins_ok(self, data):
        """(n,) bool: every margin of the module docstring holds for the agent."""
        fin = np.isfinite(self.slim)
        ok = (np.abs(np.abs(self.action) - self.alim) >= GAP).all(-1)
        if fin.any():
            ok &= (np.abs(np.abs(self.pre[:, fin]) - self.slim[fin]) >= GAP).all(-1)
        ok &= np.abs(self.err_norm - data["comm"]) >= GAP_BRANCH
        if self.name == "DubinsCar":
            ok &= np.abs(self.nrm - data["comm"]) >= GAP_BRANCH
            ok &= np.abs(self.dist - data["stop_r"]) >= GAP_BRANCH
            d = self.theta_diff
            ok &= np.minimum(np.abs(d), np.minimum(np.abs(d - math.pi), np.abs(d + math.pi))) \
                >= GAP_BRANCH
            for th in (self.theta, self.theta_t):
                for edge in (0.0, math.pi, 2.0 * math.pi):
                    ok &= np.abs(th - edge) >= GAP_BRANCH
            ok &= np.abs(self.inner) <= INNER_MAX
        return ok

    def presence(self, data):
        """name -> bool: both sides of every clamp and branch occur."""
        p = {}
        for c in range(self.NU):
            p[f"action {c} clamped"] = bool((~self.m_act[:, c]).any())
            p[f"action {c} unclamped"] = bool(self.m_act[:, c].any())
        for s in np.flatnonzero(np.isfinite(self.slim)):
            p[f"state {s} clipped"] = bool((~self.m_state[:, s]).any())
            p[f"state {s} unclipped"] = bool(self.m_state[:, s].any())
        far = (self.nrm if self.name == "DubinsCar" else self.err_norm) > data["comm"]
        p["error clip active"], p["error clip inactive"] = bool(far.any()), bool((~far).any())
        if self.name == "DubinsCar":
            inside = self.dist < data["stop_r"]
            p["inside stop radius"], p["outside stop radius"] = \
                bool(inside.any()), bool((~inside).any())
            for k in range(4):
                p[f"omega branch {k}"] = bool((self.branch == k).any())
        return p


def _oracles(name, data, agent, goal, raw):
    """The oracle under every setting the tests run it with."""
    if name == "DubinsCar":
        return [Oracle(name, data, agent, goal, raw, enable_stop=s) for s in (True, False)]
    return [Oracle(name, data, agent, goal, raw)]


def _propose(name, rng, n, near):
    """n candidate agents as f32-rounded f64 arrays. ``near`` (n,) bool marks
    agents planted close to their goal (Dubins: inside the stop radius)."""
    S, NU = SPEC[name]["S"], SPEC[name]["NU"]
    pdim = 3 if name == "LinearDrone" else 2
    agent, goal = np.zeros((n, S)), np.zeros((n, S))
    agent[:, :pdim] = rng.uniform(0.0, 3.0, (n, pdim))
    d = rng.standard_normal((n, pdim))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    r = np.where(near, rng.uniform(0.004, 0.02, n), rng.uniform(0.05, 1.0, n))
    goal[:, :pdim] = agent[:, :pdim] + d * r[:, None]
    if name == "DubinsCar":
        agent[:, 2] = rng.uniform(-4.0, 7.0, n)    # heading, wraps both ways
        agent[:, 3] = rng.uniform(-0.79, 0.79, n)  # speed, next to the +-0.8 clip
        goal[:, 2] = np.arctan2(d[:, 1], d[:, 0])
        raw = rng.standard_normal((n, NU)) * 1.2
    elif name == "LinearDrone":
        agent[:, 3:] = rng.uniform(-0.49, 0.49, (n, 3))  # next to the +-0.5 clip
        raw = rng.standard_normal((n, NU)) * 0.6
    else:
        raw = rng.standard_normal((n, NU)) * 0.6
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    return f32(agent), f32(goal), f32(raw)


def make_case(env, B, N, seed):
    """Inputs of one case for ``env`` (any device): dict with float32 CPU
    tensors agent / goal (B,N,S), raw (B,N,NU), states (B,V,S) (agent, goal
    and random LiDAR hit rows), cotangents dact (B,N,NU), dbig (2B,V,S), and
    the oracle data. Agents failing a margin are redrawn (rejection in the f64
    oracle); the margins are asserted by ``check_margins``."""
    name = type(env).__name__
    data = env_data(env)
    rng = np.random.default_rng(seed)
    n = B * N
    near = np.zeros(n, bool)
    if n >= 5:
        near[[1, n - 2]] = True
    agent, goal, raw = _propose(name, rng, n, near)
    for _ in range(200):
        ok = np.ones(n, bool)
        for orc in _oracles(name, data, agent, goal, raw):
            ok &= orc.margins_ok(data)
        if ok.all():
            break
        bad = np.flatnonzero(~ok)
        a2, g2, r2 = _propose(name, rng, bad.size, near[bad])
        agent[bad], goal[bad], raw[bad] = a2, g2, r2
    S, NU, R = SPEC[name]["S"], SPEC[name]["NU"], env.n_rays
    hits = rng.uniform(-1.0, 4.0, (B, N * R, S))
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    agent_t, goal_t = t32(agent.reshape(B, N, S)), t32(goal.reshape(B, N, S))
    states = torch.cat([agent_t, goal_t, t32(hits)], dim=1)
    return dict(name=name, B=B, N=N, data=data, agent=agent_t, goal=goal_t,
                raw=t32(raw.reshape(B, N, NU)), states=states,
                dact=t32(rng.standard_normal((B, N, NU))),
                dbig=t32(rng.standard_normal((2 * B, states.shape[1], S))))


def oracle_of(case, enable_stop=True):
    f = lambda t: t.double().numpy().reshape(case["B"] * case["N"], -1)  # noqa: E731
    return Oracle(case["name"], case["data"], f(case["agent"]), f(case["goal"]), f(case["raw"]),
                  enable_stop=enable_stop)


def check_margins(case):
    for stop in ((True, False) if case["name"] == "DubinsCar" else (True,)):
        orc = oracle_of(case, enable_stop=stop)
        ok = orc.margins_ok(case["data"])
        assert ok.all(), ("input margin violated", case["name"], case["B"], case["N"],
                          np.flatnonzero(~ok))


def check_presence(case):
    orc = oracle_of(case)
    missing = [k for k, v in orc.presence(case["data"]).items() if not v]
    assert not missing, ("main case lacks", case["name"], missing)


def oracle_draw(case, orc):
    """Oracle gradient for the case's cotangents, (B*N, NU)."""
    B, N = case["B"], case["N"]
    dnext = case["dbig"][B:, :N].double().numpy().reshape(B * N, -1)
    return orc.draw(case["dact"].double().numpy().reshape(B * N, -1), dnext)


def errors(x, ref):
    """Largest |x - ref| per component (last axis), x a tensor, ref f64 numpy."""
    n = ref.shape[-1]
    return np.abs(x.detach().double().cpu().numpy().reshape(-1, n) - ref.reshape(-1, n)).max(0)


def assert_8x(fused, eager, ref, names, what):
    """err_fused_c <= 8 * max(err_eager_c, 2^-23 * max|ref_c|) per component."""
    ef, ee = errors(fused, ref), errors(eager, ref)
    bound = 8 * np.maximum(ee, EPS32 * np.abs(ref.reshape(-1, len(names))).max(0))
    print(f"\n[{what}] comp  err_eager   err_fused   bound")
    for c, nm in enumerate(names):
        print(f"  {nm:>5} {ee[c]:.3e}  {ef[c]:.3e}  {bound[c]:.3e}")
    bad = [names[c] for c in range(len(names)) if not ef[c] <= bound[c]]
    assert not bad, (what, bad, ef, ee, bound)


def eager_prologue(env, g, raw):
    """The composed prologue: the eager branch of GCBFPlus._loss."""
    raw = raw.detach().clone().requires_grad_(True)
    action = 2 * raw + env.u_ref(g)
    next_g = env.forward_graph(g, action)
    return raw, action, torch.cat([g.states, next_g.states])
