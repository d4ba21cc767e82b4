"""Steady-state CrazyFlie swarm rollout rate: the swarm_demo.py CrazyFlie row
(n=256, area 16, 64 steps, one world) measured with a warm-up rollout and
repeated timed rollouts, for the GCBF+ policy (random init) and for the
``u_ref`` policy, which isolates the env step from the policy forward.

Uses only the public env/algo API, so the same file measures any commit:
    python tools/crazyflie_step_bench.py [--label NAME] [--repeats K] [--out FILE]
Prints one JSON line per policy; GCBF_NO_FUSED_ENV=1 selects the eager step.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.env import make_env


def rollout(env, act, g, steps):
    with torch.no_grad():
        for _ in range(steps):
            g = env.step(g, act(g)).graph
    return g


def measure(n, area, steps, use_algo, repeats):
    env = make_env("CrazyFlie", n, area_size=area, max_step=steps, device="cuda")
    if use_algo:
        torch.manual_seed(0)
        algo = make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                         state_dim=env.state_dim, action_dim=env.action_dim, n_agents=n)
        act = algo.act
    else:
        act = env.u_ref
    g0 = env.reset(1, np.random.default_rng(0))
    rollout(env, act, g0, steps)  # warm-up: code objects, caches, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        g = rollout(env, act, g0, steps)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    rates = [steps / t for t in times]
    return {
        "env": "CrazyFlie", "n_agents": n, "area": area, "steps": steps,
        "policy": "gcbf+ (random init)" if use_algo else "u_ref",
        "fused_env": not os.environ.get("GCBF_NO_FUSED_ENV"),
        "env_steps_per_s_median": round(statistics.median(rates), 1),
        "env_steps_per_s_min": round(min(rates), 1),
        "env_steps_per_s_max": round(max(rates), 1),
        "rollout_s": [round(t, 4) for t in times],
        "finite": bool(torch.isfinite(g.states).all()),
        "final_state_checksum": float(g.states[:, :n].double().abs().sum()),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--area", type=float, default=16.0)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    recs = []
    for use_algo in (True, False):
        rec = measure(args.n, args.area, args.steps, use_algo, args.repeats)
        rec["label"] = args.label
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "runs": recs}, f, indent=1)


if __name__ == "__main__":
    main()
