import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
"""Micro-bench the GEMM paths at the real training shapes."""
import time
import torch
from gcbfplus_amd import _C

def bench(M, K, N, iters=50):
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    w = torch.randn(K, N, device="cuda").to(torch.bfloat16)
    b = torch.randn(N, device="cuda")
    for _ in range(5):
        y = _C.gemm_bias_act(x, w, b, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        y = _C.gemm_bias_act(x, w, b, 1)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    tf = 2 * M * K * N / dt / 1e12
    # correctness spot check
    ref = (x[:256].float() @ w.float() + b).relu()
    err = (y[:256].float() - ref).abs().max().item()
    print(f"M={M:6d} K={K:3d} N={N:3d}: {dt*1e6:7.1f} us  {tf:6.1f} TF  maxerr {err:.3f}")

def _event_us(fn, iters):
    """Median device time of fn() in microseconds (one event pair per call)."""
    for _ in range(5):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2] * 1e3


def _tn_split(M, K, N):
    """Slab count of the dW launcher for the 64x64 kernels (tests/test_gemm_oracle.py)."""
    gk, gn = (K + 63) // 64, (N + 63) // 64
    S = min(128, max(1, 1024 // (gk * gn)))
    S = min(S, max(1, (M + 127) // 128))
    return (S + 7) // 8 * 8 if S >= 8 else S


# dW shapes of one GNNLayer (nn/gnn.py) at M = batch * agents * edge slots, with
# the activation fold of the layer that owns the weight:
#   msg_mlp 32->256 relu, 256->256 linear; msg_out 256->128 linear;
#   attn_mlp 128->128 relu, 128->128 linear; attn_out 128->1 linear
TN_SHAPES = [(32, 256, 1), (256, 256, 0), (256, 128, 0), (128, 128, 1), (128, 128, 0),
             (128, 1, 0)]


def bench_tn(M, K, N, actin, gated, iters=30):
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    dy = torch.randn(M, N, device="cuda").to(torch.bfloat16)
    y = torch.randn(M, N, device="cuda").relu().to(torch.bfloat16)
    gate = (torch.rand(M, device="cuda") < 0.5) if gated else None
    dw = torch.zeros(K, N, device="cuda")
    db = torch.zeros(N, device="cuda")
    us = _event_us(lambda: _C.gemm_tn_acc(x, dy, y if actin else dy, actin, dw, db, gate), iters)
    line = (f"TN M={M:6d} K={K:3d} N={N:3d} actin={actin} gate={'half' if gated else 'none'}: "
            f"{us:7.1f} us  {2 * M * K * N / us / 1e6:6.1f} TF")
    if hasattr(_C, "reduce_dw_db"):
        S = _tn_split(M, K, N)
        pw = torch.randn(S, K, N, device="cuda")
        pb = torch.randn(S, N, device="cuda")
        rus = _event_us(lambda: _C.reduce_dw_db(pw, pb, dw, db, None, True), iters)
        line += f"  | reduce S={S:3d}: {rus:6.1f} us  {S * K * N * 4 / rus / 1e6:5.2f} TB/s"
    dz = dy.float() * (y > 0).float() if actin else dy.float()
    if gated:
        dz = dz * gate[:, None].float()
    dw1, _ = _C.gemm_tn(x, dy, y if actin else dy, actin, gate)
    ref = x.float().t() @ dz.bfloat16().float()
    err = (dw1 - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(line + f"  relerr {err:.1e}")
    # the forward glds kernel on the same (M, K, N): the yardstick for a
    # row-major-staged MFMA loop at this K
    if N > 16 and not gated:
        w = torch.randn(K, N, device="cuda").to(torch.bfloat16)
        b = torch.randn(N, device="cuda")
        fus = _event_us(lambda: _C.gemm_bias_act(x, w, b, 1), iters)
        print(f"   fwd {_C.gemm_path('fwd', M, K, N):5s} same shape: {fus:7.1f} us  "
              f"{2 * M * K * N / fus / 1e6:6.1f} TF")

def bench_gemv(M, K, N, iters=50):
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    w = torch.randn(K, N, device="cuda").to(torch.bfloat16)
    b = torch.randn(N, device="cuda")
    for _ in range(5):
        y = _C.gemm_bias_act(x, w, b, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        y = _C.gemm_bias_act(x, w, b, 0)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    gb = (2.0 * M * K) / dt / 1e9
    ref = x[:256].float() @ w.float() + b
    err = (y[:256].float() - ref).abs().max().item()
    print(f"GEMV M={M:6d} K={K:3d} N={N:2d}: {dt*1e6:7.1f} us  {gb:6.0f} GB/s  maxerr {err:.3f}")

# fwd / dX shapes of the row-panel kernel: the three hot training shapes, a
# single n-tile (N = 64), the K = 384 single-W-buffer regime and the QP-label
# row count
PANEL_SHAPES = [(167936, 256, 256), (167936, 256, 128), (167936, 128, 128), (167936, 128, 64),
                (167936, 64, 64), (167936, 384, 128), (503808, 128, 128), (503808, 256, 256)]


def bench_fwd_bt(M, K, N, iters=50):
    """Device time of Y = relu(X W + b) (K -> N) and of dX = dZ W^T at the same
    layer (dZ is (M, N), W (N_out = K, K_red = N): reduction N, output K)."""
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    w = torch.randn(K, N, device="cuda").to(torch.bfloat16)
    b = torch.randn(N, device="cuda")
    fus = _event_us(lambda: _C.gemm_bias_act(x, w, b, 1), iters)
    line = (f"FWD M={M:6d} K={K:3d} N={N:3d} {_C.gemm_path('fwd', M, K, N):8s}: {fus:7.1f} us "
            f"{2 * M * K * N / fus / 1e6:6.1f} TF")
    # BT with reduction K and output N: the mirror product of the same cost
    dz = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    wt = torch.randn(N, K, device="cuda").to(torch.bfloat16)
    bus = _event_us(lambda: _C.gemm_bt(dz, wt, dz, 0), iters)
    line += (f" | BT {_C.gemm_path('bt', M, K, N, 0):8s}: {bus:7.1f} us "
             f"{2 * M * K * N / bus / 1e6:6.1f} TF")
    print(line, flush=True)


# the six agent-level dW problems of one network's backward: (K, N, actin)
GROUPED_SHAPES = [(128, 256, 1), (256, 256, 0), (256, 128, 0), (128, 256, 1), (256, 256, 0),
                  (256, 1, 0)]


def bench_grouped(M, gated, iters=50):
    """Six immediate gemm_tn_acc calls (a partial and a reduce launch each)
    against six gemm_tn_defer calls plus one dw_flush (grouped launches)."""
    ops = []
    for K, N, actin in GROUPED_SHAPES:
        x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
        dy = torch.randn(M, N, device="cuda").to(torch.bfloat16)
        y = torch.randn(M, N, device="cuda").relu().to(torch.bfloat16)
        gate = (torch.rand(M, device="cuda") < 0.5) if gated else None
        ops.append((x, dy, y if actin else dy, actin, torch.zeros(K, N, device="cuda"),
                    torch.zeros(N, device="cuda"), gate))

    def immediate():
        for x, dy, y, actin, dw, db, gate in ops:
            _C.gemm_tn_acc(x, dy, y, actin, dw, db, gate)

    def deferred():
        for x, dy, y, actin, dw, db, gate in ops:
            _C.gemm_tn_defer(x, dy, y, actin, dw, db, None, gate)
        _C.dw_flush()

    # alternate the two arms so a drifting clock hits both
    imm, dfr = [], []
    for _ in range(3):
        imm.append(_event_us(immediate, iters))
        dfr.append(_event_us(deferred, iters))
    i, d = sorted(imm)[1], sorted(dfr)[1]
    print(f"GROUPED M={M:5d} gate={'half' if gated else 'none'}: 6 immediate {i:6.1f} us "
          f"(12 launches) | 6 deferred + flush {d:6.1f} us (2 launches)  x{i / d:4.2f}",
          flush=True)


def bench_tn_map(M, K, N, actin, density, iters=40):
    """Device time (us) of one dW call (partial + reduce) through a row map of
    M entries with about density * M live rows, compact operands, half gate."""
    g = torch.Generator().manual_seed(M + K + N)
    live = torch.rand(M, generator=g) < density
    count = int(live.sum())
    inv = torch.full((M,), -1, dtype=torch.int32)
    inv[live] = torch.arange(count, dtype=torch.int32)
    inv = inv.cuda()
    cap = max(count, 1)
    x = torch.randn(cap, K, device="cuda").to(torch.bfloat16)
    dy = torch.randn(cap, N, device="cuda").to(torch.bfloat16)
    y = torch.randn(cap, N, device="cuda").relu().to(torch.bfloat16)
    gate = torch.rand(cap, device="cuda") < 0.5
    dw = torch.zeros(K, N, device="cuda")
    db = torch.zeros(N, device="cuda")
    return _event_us(lambda: _C.gemm_tn_acc(x, dy, y if actin else dy, actin, dw, db, gate, None,
                                            inv), iters)


def bench_row_map(density):
    """The six edge-level dW shapes through a row map: this process's kernel
    (tn3map by default) against gemm_tn_partial3_kernel's map path, which a
    child process with GCBF_NO_TN_SPARSE=1 times (the toggle is read once)."""
    import json
    import subprocess
    child = os.environ.get("GEMM_BENCH_ROW_MAP_CHILD") == "1"
    res = {}
    for M in (167936, 83968):
        for K, N, actin in TN_SHAPES:
            res[f"{M},{K},{N},{actin}"] = bench_tn_map(M, K, N, actin, density)
    if child:
        print("ROWMAP " + json.dumps(res), flush=True)
        return
    env = dict(os.environ, GCBF_NO_TN_SPARSE="1", GEMM_BENCH_ROW_MAP_CHILD="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--row-map", str(density)],
                         env=env, check=True, capture_output=True, text=True).stdout
    old = json.loads([l for l in out.splitlines() if l.startswith("ROWMAP ")][-1][7:])
    tot_new = tot_old = 0.0
    for key, us in res.items():
        M, K, N, actin = (int(v) for v in key.split(","))
        print(f"TN row-map d={density} M={M:6d} K={K:3d} N={N:3d} actin={actin}: "
              f"{_C.gemm_tn_map_path(M, K, N, actin, True).split()[0]} {us:6.1f} us | "
              f"GCBF_NO_TN_SPARSE=1 {old[key]:6.1f} us  x{old[key] / us:4.2f}", flush=True)
        tot_new += us
        tot_old += old[key]
    print(f"TN row-map d={density} sum of 12: {tot_new:7.1f} us | {tot_old:7.1f} us  "
          f"x{tot_old / tot_new:4.2f}")


def _parse_shapes(args):
    return [tuple(int(v) for v in a.split(",")) for a in args]


if __name__ == "__main__":
    # `--panel [M,K,N ...]`: forward and dX times only, at the given shapes
    # (default PANEL_SHAPES)
    if len(sys.argv) > 1 and sys.argv[1] == "--panel":
        for shape in _parse_shapes(sys.argv[2:]) or PANEL_SHAPES:
            bench_fwd_bt(*shape)
        sys.exit(0)
    # `--grouped`: the small-M dW group of one network, immediate vs deferred
    if len(sys.argv) > 1 and sys.argv[1] == "--grouped":
        for M in (4096, 2048):
            for gated in (False, True):
                bench_grouped(M, gated)
        sys.exit(0)
    # `--row-map DENSITY`: dW through a row map per layer shape, new kernel
    # against the GCBF_NO_TN_SPARSE=1 arm
    if len(sys.argv) > 2 and sys.argv[1] == "--row-map":
        bench_row_map(float(sys.argv[2]))
        sys.exit(0)
    for shape in [(167936, 256, 256), (167936, 32, 256), (167936, 256, 128),
                  (167936, 128, 128), (4096, 256, 256), (4096, 128, 256)]:
        bench(*shape)
    for K, N, actin in TN_SHAPES:
        for gated in (False, True):
            bench_tn(167936, K, N, actin, gated)
    for shape in [(167936, 128, 1), (335872, 128, 1), (4096, 256, 2), (4096, 256, 1)]:
        bench_gemv(*shape)
