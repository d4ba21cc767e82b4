"""GCBF+ minibatch loss forward+backward time on DubinsCar, LinearDrone or
SingleIntegrator (n=8, batch 256), eager launches (no HIP-graph replay:
GCBF_NO_HIPGRAPH=1 is set here), so the launch count of the loss prologue
shows up in the time. Same protocol as tools/crazyflie_loss_bench.py.

Two arms are timed in ONE process, alternating sample by sample: the default
dispatch (the fused prologue, ``env.loss_prep``) and GCBF_NO_FUSED_PREP=1 (the
composed torch prologue). On a commit without the fused prologue the two arms
run the same code, and their difference is the spread of the method. Uses only
the public env/algo API and ``GCBFPlus._loss``, so the same file measures any
commit:
    python tools/loss_prep_bench.py --env DubinsCar [--label NAME]
                                    [--rounds K] [--out FILE]
Prints one JSON line; kernel launches per minibatch are counted with the
torch profiler in a separate, untimed pass.
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ["GCBF_NO_HIPGRAPH"] = "1"

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.env import make_env
from gcbfplus_amd.trainer.data import FlatBatch

ENVS = ("DubinsCar", "LinearDrone", "SingleIntegrator")
OPT_OUT = "GCBF_NO_FUSED_PREP"
ARMS = ("default", OPT_OUT + "=1")


def set_arm(arm):
    if arm == "default":
        os.environ.pop(OPT_OUT, None)
    else:
        os.environ[OPT_OUT] = "1"


def minibatch(name, n, batch, seed):
    torch.manual_seed(seed)
    env = make_env(name, num_agents=n, area_size=4.0, max_step=8, device="cuda")
    algo = make_algo("gcbf+", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim, n_agents=n,
                     gnn_layers=1, batch_size=batch, buffer_size=batch, horizon=4,
                     inner_epoch=1, seed=0)
    g = env.reset(batch, np.random.default_rng(seed))
    st = g.states.clone()
    pdim = 3 if name == "LinearDrone" else 2
    if env.state_dim > pdim:  # off rest: headings / velocities as in a rollout
        st[:, :n, pdim:] += torch.randn(batch, n, env.state_dim - pdim, device="cuda") * 0.2
    safe = torch.rand(batch, n, device="cuda") < 0.5
    unsafe = ~safe & (torch.rand(batch, n, device="cuda") < 0.5)
    u_qp = torch.randn(batch, n, env.action_dim, device="cuda").clamp(-1, 1)
    return env, algo, FlatBatch(st, g.mask, safe, unsafe, u_qp)


def step(algo, mb):
    gbuf = getattr(algo, "dp_gbuf", None)  # flat gradient buffer of both optimizers
    if gbuf is not None:
        gbuf.zero_()
    else:
        for p in list(algo.cbf.parameters()) + list(algo.actor.parameters()):
            if p.grad is not None:
                p.grad.zero_()
    total, _ = algo._loss(mb, want_info=False)
    total.backward()
    return total


def count_launches(algo, mb):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(algo, mb)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", required=True, choices=ENVS)
    ap.add_argument("--label", default="")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20, help="minibatches per timed sample")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    env, algo, mb = minibatch(args.env, args.n, args.batch, seed=0)

    loss = {}
    for arm in ARMS:  # warm up every arm: code objects, allocator, lazy state
        set_arm(arm)
        for _ in range(args.warmup):
            total = step(algo, mb)
        torch.cuda.synchronize()
        loss[arm] = float(total.detach())
    samples = {arm: [] for arm in ARMS}
    for _ in range(args.rounds):
        for arm in ARMS:
            set_arm(arm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                step(algo, mb)
            torch.cuda.synchronize()
            samples[arm].append((time.perf_counter() - t0) / args.iters * 1e3)
    launches = {}
    for arm in ARMS:
        set_arm(arm)
        try:
            launches[arm] = count_launches(algo, mb)
        except Exception as e:  # profiler not usable: say so, do not guess
            launches[arm] = f"not measured ({type(e).__name__})"
    set_arm("default")

    rec = {"label": args.label, "env": args.env, "n_agents": args.n, "batch": args.batch,
           "device": torch.cuda.get_device_name(0), "iters_per_sample": args.iters,
           "arms": {}}
    for arm in ARMS:
        s = sorted(samples[arm])
        rec["arms"][arm] = {
            "ms_per_minibatch_median": round(statistics.median(s), 4),
            "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4),
            "ms_iqr": round(s[(3 * len(s)) // 4] - s[len(s) // 4], 4),
            "launches_per_minibatch": launches[arm],
            "loss": loss[arm],
            "samples_ms": [round(x, 4) for x in samples[arm]],
        }
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
