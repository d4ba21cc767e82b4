"""Micro-bench of the fused edge_msg_in kernels (dev tool)."""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import time

import torch

from gcbfplus_amd import ops


def bench(fn, iters=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    N, R, S = 8, 32, 4
    V = 2 * N + N * R
    for B in (512, 256, 16):
        states = torch.randn(B, V, S, device="cuda")
        x = ops.edge_msg_in(states, N, R, 2, 0.5)
        ref = ops.edge_msg_in(states.cpu(), N, R, 2, 0.5)
        err = (x.float().cpu() - ref).abs().max().item()
        us = bench(lambda: ops.edge_msg_in(states, N, R, 2, 0.5))
        # backward
        st2 = states.clone().requires_grad_(True)
        g = torch.randn_like(x)

        def fb():
            out = ops.edge_msg_in(st2, N, R, 2, 0.5)
            (out * g).sum().backward()

        us_fb = bench(fb, 50)
        print(f"B={B:4d} fwd {us:7.1f} us  maxerr {err:.4f}  fwd+bwd {us_fb:7.1f} us")
    crazyflie_rows()


def crazyflie_rows():
    """Mode 2 (CrazyFlie) against the torch composition it replaces:
    env.edge_feats on the GPU, and for fwd+bwd autograd through it."""
    import json

    from gcbfplus_amd.env import make_env
    from gcbfplus_amd.utils.graph import GraphBatch

    for N, B in ((8, 256), (256, 1)):
        env = make_env("CrazyFlie", num_agents=N, area_size=4.0, max_step=4, device="cuda")
        R, comm = env.n_rays, env.params["comm_radius"]
        V, D = 2 * N + N * R, N + 1 + R
        states = torch.randn(B, V, 12, device="cuda")
        graph = GraphBatch(states=states, mask=torch.ones(B, N, D, dtype=torch.bool, device="cuda"),
                           n_agents=N, n_rays=R)
        g = torch.randn(B, N, D, 32, device="cuda").bfloat16()
        g12 = g[..., :12].float()
        st2 = states.clone().requires_grad_(True)

        def fused_fb():
            st2.grad = None
            (ops.edge_msg_in(st2, N, R, 3, comm, mode=2) * g).sum().backward()

        def torch_fb():
            st2.grad = None
            (env.edge_feats(graph, st2) * g12).sum().backward()

        rec = {
            "row": "crazyflie mode 2", "N": N, "B": B, "slots": B * N * D,
            "fused_fwd_us": bench(lambda: ops.edge_msg_in(states, N, R, 3, comm, mode=2)),
            "torch_edge_feats_fwd_us": bench(lambda: env.edge_feats(graph, states)),
            "fused_fwd_bwd_us": bench(fused_fb, 50),
            "torch_fwd_bwd_us": bench(torch_fb, 50),
        }
        print(json.dumps({k: round(v, 1) if isinstance(v, float) else v for k, v in rec.items()}),
              flush=True)


if __name__ == "__main__":
    main()
