"""Deferred dW (``_C.gemm_tn_defer`` + ``_C.dw_flush``): the grouped partial
and reduce launches must leave every destination bit-equal to the immediate
``gemm_tn_acc`` / ``gemm_tn_acc2`` calls they replace. Same inputs, both
destinations pre-filled with the same non-zero values, ``torch.equal`` on f32.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from gcbfplus_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NONE, RELU, TANH = 0, 1, 2

# (M, K, N, act) and the path `gemm_plan` gives it (unchanged by deferral)
MIXED = [
    ((130, 32, 64, RELU), "tn1 S=2 remap=0"),     # ragged last slab, S = 2
    ((4096, 128, 256, RELU), "tn1 S=32 remap=1"),
    ((2048, 256, 256, NONE), "tn1 S=16 remap=1"),
    ((256, 256, 1, NONE), "tn1 S=2 remap=0"),
    ((192, 64, 20, NONE), "tn1 S=2 remap=0"),     # N % 8 != 0
    ((64, 32, 32, TANH), "tn1 S=1 remap=0"),      # S = 1, no remap
]


def _ext():
    from gcbfplus_amd import _C
    return _C


def _problem(shape, seed, gate=None):
    """Operands of one dW problem; `gate` in (None, 'true', 'false', 'alt')."""
    M, K, N, act = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    dz = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    y = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)  # both signs: relu fold
    rg = None
    if gate == "true":
        rg = torch.ones(M, dtype=torch.bool, device=DEV)
    elif gate == "false":
        rg = torch.zeros(M, dtype=torch.bool, device=DEV)
    elif gate == "alt":
        rg = (torch.arange(M, device=DEV) % 2) == 0
    return dict(x=x, dz=dz, y=y, act=act, rg=rg, K=K, N=N, seed=seed)


def _dests(p, flat_offset=None):
    """(dw, db, db2) pre-filled with seeded non-zero values. With
    `flat_offset` they are views into one flat buffer starting at that
    element offset (an odd one makes dW 4-byte-odd, off the 16-byte grid)."""
    K, N = p["K"], p["N"]
    g = torch.Generator().manual_seed(1000 + p["seed"])
    if flat_offset is None:
        dw = torch.randn(K, N, generator=g).to(DEV) + 3.0
        db = torch.randn(N, generator=g).to(DEV) + 3.0
        db2 = torch.randn(N, generator=g).to(DEV) + 3.0
        return dw, db, db2
    flat = (torch.randn(flat_offset + K * N + 2 * N, generator=g) + 3.0).to(DEV)
    o = flat_offset
    return (flat[o:o + K * N].view(K, N), flat[o + K * N:o + K * N + N],
            flat[o + K * N + N:o + K * N + 2 * N])


def _immediate(p, dw, db, db2=None):
    if db2 is None:
        _ext().gemm_tn_acc(p["x"], p["dz"], p["y"], p["act"], dw, db, p["rg"])
    else:
        _ext().gemm_tn_acc2(p["x"], p["dz"], p["y"], p["act"], dw, db, db2, p["rg"])


def _defer(p, dw, db, db2=None):
    _ext().gemm_tn_defer(p["x"], p["dz"], p["y"], p["act"], dw, db, db2, p["rg"])


def _check_equal(got, want, what):
    torch.cuda.synchronize()
    for name, a, b in zip(("dw", "db", "db2"), got, want):
        assert torch.equal(a, b), f"{what}: {name} differs, max |d| = {(a - b).abs().max().item()}"


@pytest.fixture(autouse=True)
def _clean_queue():
    _ext().dw_discard()
    yield
    _ext().dw_discard()


def test_path_report_unchanged():
    for (M, K, N, act), path in MIXED:
        for gated in (False, True):
            assert _ext().gemm_path("tn", M, K, N, act, gated) == path


def test_mixed_group_one_flush():
    probs = [_problem(s, i) for i, (s, _) in enumerate(MIXED)]
    want = [_dests(p) for p in probs]
    got = [_dests(p) for p in probs]
    for p, d in zip(probs, want):
        _immediate(p, d[0], d[1])
    before = _ext().dw_launch_counts()
    for p, d in zip(probs, got):
        _defer(p, d[0], d[1])
    assert _ext().dw_pending() == len(probs)
    _ext().dw_flush()
    assert _ext().dw_pending() == 0
    after = _ext().dw_launch_counts()
    assert [a - b for a, b in zip(after, before)] == [1, 1]
    for p, g, w in zip(probs, got, want):
        _check_equal(g[:2], w[:2], f"mixed {p['seed']}")
        assert torch.equal(g[2], w[2])  # db2 not passed: untouched


@pytest.mark.parametrize("gate", ["true", "false", "alt"])
def test_row_gate(gate):
    probs = [_problem(MIXED[0][0], 10, gate), _problem(MIXED[1][0], 11, gate)]
    want = [_dests(p) for p in probs]
    got = [_dests(p) for p in probs]
    for p, d in zip(probs, want):
        _immediate(p, d[0], d[1])
    for p, d in zip(probs, got):
        _defer(p, d[0], d[1])
    _ext().dw_flush()
    for p, g, w in zip(probs, got, want):
        _check_equal(g[:2], w[:2], f"gate {gate} {p['seed']}")
    if gate == "false":  # nothing contributed: destinations keep their fill
        for p, g in zip(probs, got):
            fill = _dests(p)
            _check_equal(g[:2], fill[:2], "all-false gate")


def test_acc2_db_lands_in_both_targets():
    probs = [_problem(MIXED[2][0], 20), _problem(MIXED[4][0], 21, "alt")]
    want = [_dests(p) for p in probs]
    got = [_dests(p) for p in probs]
    for p, d in zip(probs, want):
        _immediate(p, *d)
    for p, d in zip(probs, got):
        _defer(p, *d)
    _ext().dw_flush()
    for p, g, w in zip(probs, got, want):
        _check_equal(g, w, f"acc2 {p['seed']}")
        fill = _dests(p)
        assert not torch.equal(g[2], fill[2])  # db2 did receive the sum


def test_unaligned_destinations_share_a_launch():
    """dW at a 4-byte-odd offset takes the scalar reduce variant in the same
    grouped launch as a 16-byte-aligned one."""
    probs = [_problem(MIXED[1][0], 30), _problem(MIXED[2][0], 31),
             _problem(MIXED[4][0], 32)]
    offs = [1, 0, 3]
    want = [_dests(p, o) for p, o in zip(probs, offs)]
    got = [_dests(p, o) for p, o in zip(probs, offs)]
    assert got[0][0].data_ptr() % 16 == 4 and got[1][0].data_ptr() % 16 == 0
    for p, d in zip(probs, want):
        _immediate(p, *d)
    before = _ext().dw_launch_counts()
    for p, d in zip(probs, got):
        _defer(p, *d)
    _ext().dw_flush()
    assert [a - b for a, b in zip(_ext().dw_launch_counts(), before)] == [1, 1]
    for p, g, w in zip(probs, got, want):
        _check_equal(g, w, f"unaligned {p['seed']}")


def test_table_overflow_takes_two_launches():
    probs = [_problem(MIXED[5][0] if i % 2 else MIXED[4][0], 40 + i) for i in range(17)]
    want = [_dests(p) for p in probs]
    got = [_dests(p) for p in probs]
    for p, d in zip(probs, want):
        _immediate(p, d[0], d[1])
    before = _ext().dw_launch_counts()
    for p, d in zip(probs, got):
        _defer(p, d[0], d[1])
    assert _ext().dw_pending() == 17
    _ext().dw_flush()
    assert [a - b for a, b in zip(_ext().dw_launch_counts(), before)] == [2, 2]
    for p, g, w in zip(probs, got, want):
        _check_equal(g[:2], w[:2], f"overflow {p['seed']}")


def test_aliasing_keeps_call_order():
    """Two entries accumulating into one dW: the second flushes the first."""
    shape = MIXED[1][0]
    pa, pb = _problem(shape, 60), _problem(shape, 61)
    want, got = _dests(pa), _dests(pa)
    _immediate(pa, want[0], want[1])
    _immediate(pb, want[0], want[1])
    _defer(pa, got[0], got[1])
    assert _ext().dw_pending() == 1
    _defer(pb, got[0], got[1])
    assert _ext().dw_pending() == 1  # pa ran, pb waits
    _ext().dw_flush()
    _check_equal(got[:2], want[:2], "aliasing")


def test_large_m_plan_runs_at_once():
    """A `tn3` shape through gemm_tn_defer is not queued: partial and reduce
    run immediately, after a flush of a pending entry it aliases."""
    shape = (16384, 64, 64, RELU)
    assert _ext().gemm_path("tn", *shape) == "tn3 S=128 remap=1"
    small, big = _problem((256, 64, 64, RELU), 65), _problem(shape, 66, "alt")
    want, got = _dests(big), _dests(big)
    _immediate(small, want[0], want[1])
    _immediate(big, *want)
    _defer(small, got[0], got[1])
    assert _ext().dw_pending() == 1
    _defer(big, *got)  # same dW: the small entry is flushed first
    assert _ext().dw_pending() == 0
    _check_equal(got, want, "tn3 through defer")


def test_capture_replays_equal_eager():
    probs = [_problem(MIXED[1][0], 70), _problem(MIXED[0][0], 71, "alt"),
             _problem(MIXED[3][0], 72)]
    want = [tuple(torch.zeros_like(t) for t in _dests(p)) for p in probs]
    for p, d in zip(probs, want):
        _immediate(p, *d)
    got = [tuple(torch.zeros_like(t) for t in _dests(p)) for p in probs]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for p, d in zip(probs, got):
            _defer(p, *d)
        _ext().dw_flush()
    assert _ext().dw_pending() == 0
    for rep in range(2):
        for d in got:
            for t in d:
                t.zero_()
        graph.replay()
        for p, g, w in zip(probs, got, want):
            _check_equal(g, w, f"replay {rep} problem {p['seed']}")


def test_flush_on_empty_queue_launches_nothing():
    assert _ext().dw_pending() == 0
    before = _ext().dw_launch_counts()
    _ext().dw_flush()
    assert _ext().dw_launch_counts() == before


def test_exception_in_scope_discards():
    p = _problem(MIXED[2][0], 80)
    d, fill = _dests(p), _dests(p)
    before = _ext().dw_launch_counts()
    with pytest.raises(RuntimeError, match="boom"):
        with ops.deferred_dw(DEV):
            _defer(p, d[0], d[1])
            assert _ext().dw_pending() == 1
            raise RuntimeError("boom")
    assert _ext().dw_pending() == 0
    assert _ext().dw_launch_counts() == before
    _check_equal(d, fill, "discarded")


def test_scope_routes_fused_linear_and_flushes():
    """Inside ops.deferred_dw the direct-accumulate backward queues its dW;
    the exit flushes it; the gradient equals the immediate one."""
    from gcbfplus_amd.ops.optim import FusedAdamW

    def grads(scope):
        torch.manual_seed(3)
        net = torch.nn.ParameterList([
            torch.nn.Parameter(torch.randn(64, 128) * 0.1), torch.nn.Parameter(torch.zeros(128)),
            torch.nn.Parameter(torch.randn(128, 32) * 0.1), torch.nn.Parameter(torch.zeros(32)),
        ]).to(DEV)
        opt = FusedAdamW(net, lr=0.0)
        opt.zero_grad()
        x = torch.randn(512, 64, device=DEV)
        h = ops.fused_linear(x, net[0], net[1], RELU)
        loss = ops.fused_linear(h, net[2], net[3], NONE).float().square().mean()
        if scope:
            with ops.deferred_dw(DEV):
                loss.backward()
                assert _ext().dw_pending() == 2
        else:
            loss.backward()
        assert _ext().dw_pending() == 0
        torch.cuda.synchronize()
        return opt.gflat.clone()

    a, b = grads(True), grads(False)
    assert a.abs().sum() > 0
    assert torch.equal(a, b)


def test_adamw_step_flushes_pending():
    """A forgotten flush: fused_adamw_step runs the queue before it reads g."""
    from gcbfplus_amd.ops.optim import FusedAdamW

    shape = MIXED[2][0]
    p = _problem(shape, 90)

    def run(deferred):
        lin = torch.nn.Linear(shape[1], shape[2]).to(DEV)  # sizes only: a flat f32 span
        opt = FusedAdamW(lin, lr=0.0)
        opt.zero_grad()
        n = shape[1] * shape[2]
        dw, db = opt.gflat[:n].view(shape[1], shape[2]), opt.gflat[n:n + shape[2]]
        if deferred:
            _defer(p, dw, db)
            assert _ext().dw_pending() == 1
        else:
            _immediate(p, dw, db)
        norm = opt.step()
        assert _ext().dw_pending() == 0
        torch.cuda.synchronize()
        return opt.gflat.clone(), norm.clone()

    (ga, na), (gb, nb) = run(True), run(False)
    assert ga.abs().sum() > 0
    assert torch.equal(ga, gb)
    assert torch.equal(na, nb)


_CHILD = r"""
import hashlib, sys
import numpy as np
import torch
from gcbfplus_amd import ops, _C
from gcbfplus_amd.env import make_env
from gcbfplus_amd.algo.module.cbf import CBFNet
from gcbfplus_amd.ops.optim import FusedAdamW

torch.manual_seed(11)
env = make_env("DoubleIntegrator", num_agents=2, area_size=4.0, max_step=4, device="cpu")
g = env.reset(4, np.random.default_rng(3)).to("cuda")
net = CBFNet(env.node_dim, env.edge_dim, 1).to("cuda")
opt = FusedAdamW(net, lr=1e-3)
opt.zero_grad()
h = net(g, env.edge_feats(g))
loss = h.float().square().mean()
with ops.deferred_dw("cuda"):
    loss.backward()
torch.cuda.synchronize()
assert _C.dw_pending() == 0
gf = opt.gflat.cpu().numpy()
assert np.isfinite(gf).all() and np.abs(gf).sum() > 0
print("GFLAT", hashlib.sha256(gf.tobytes()).hexdigest(), _C.dw_launch_counts()[1])
"""


def test_end_to_end_cbfnet_scope_on_and_off():
    """CBFNet backward under FusedAdamW: bit-equal gflat with the scope on
    and with GCBF_NO_DEFER_DW=1, each in a fresh child process."""
    def child(no_defer):
        env = dict(os.environ)
        env.pop("GCBF_NO_DEFER_DW", None)
        if no_defer:
            env["GCBF_NO_DEFER_DW"] = "1"
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        line = [l for l in r.stdout.splitlines() if l.startswith("GFLAT")][-1].split()
        return line[1], int(line[2])

    (h_on, launches_on), (h_off, launches_off) = child(False), child(True)
    assert launches_on >= 1 and launches_off == 0
    assert h_on == h_off
