"""The CBF network with the edge level on active slots only (ops.EdgeCompact)
against the dense path in the same process, with a row gate, eagerly and
through a captured-and-replayed graph whose static buffers see two different
masks (a stale row count would show).

Two shapes: B = 2, N = 3, R = 4 (capacity 128: the small-M kernels) and
B = 26, N = 8, R = 32 (17 056 slot rows, the smallest batch past the small-M
limit; capacity 17 152: row-panel, 128x64 and tn3 kernels).

h and dstates are compared bit for bit: a masked slot has attention exactly 0,
so dropping its row changes no term of any sum. Parameter gradients are
compared bit for bit too: dW/db of the compact layers are summed over the dense
slot rows in the dense call's order (the row map of the dW kernels), where a
masked row adds an exact zero in both paths. Both paths are also held to the
rule of tests/test_gnn_deep_gpu.py against the CPU f32 autograd result,
err <= 4 * max(err_other, 2^-8 * max|ref|) on the mean absolute error."""
import pytest
import torch
from torch.func import functional_call

pytestmark = pytest.mark.gpu

from gcbfplus_amd import ops
from gcbfplus_amd.algo.module.cbf import CBFNet
from gcbfplus_amd.utils.graph import GraphBatch

DEV = "cuda"
SHAPES = [(2, 3, 4), (26, 8, 32)]
COMM = 0.5


def _inputs(B, N, R, seed, density):
    g = torch.Generator().manual_seed(seed)
    V, D = 2 * N + N * R, N + 1 + R
    states = torch.rand(B, V, 4, generator=g) * torch.tensor([2.0, 2.0, 1.0, 1.0])
    mask = torch.rand(B, N, D, generator=g) < density
    mask[0, 0] = False  # a receiver with no active slot
    mask[-1, -1] = True  # and one with every slot active
    gate = torch.rand(B, N, generator=g) < 0.6
    wts = torch.randn(B, N, generator=g)
    return states, mask, gate, wts


def _run(net, states, mask, gate, wts, N, R, compact):
    st = states.clone().requires_grad_(True)
    mi = ops.edge_msg_in(st, N, R, 2, COMM)
    g = GraphBatch(states=st, mask=mask, n_agents=N, n_rays=R)
    kw = {"compact": ops.EdgeCompact.build(mask, row_gate=gate)} if compact else {}
    h = net(g, None, msg_in=mi, row_gate=gate, **kw).squeeze(-1)
    (h * wts).sum().backward()
    return h.detach(), st.grad


def _cpu_oracle(net, states, mask, gate, wts, N, R):
    """f32 autograd; the row gate (no parameter gradient from rows with
    gate == False, dX untouched) as a second evaluation with detached
    parameters."""
    net.zero_grad(set_to_none=True)
    st = states.clone().requires_grad_(True)
    mi = ops.edge_msg_in(st, N, R, 2, COMM)
    g = GraphBatch(states=st, mask=mask, n_agents=N, n_rays=R)
    h_full = net(g, None, msg_in=mi).squeeze(-1)
    det = {k: v.detach() for k, v in net.named_parameters()}
    h_det = functional_call(net, det, (g, None), {"msg_in": mi}).squeeze(-1)
    (torch.where(gate, h_full, h_det) * wts).sum().backward()
    return {k: p.grad.clone() for k, p in net.named_parameters()}


def _rule(err, err_other, ref_max):
    return err <= 4.0 * max(err_other, 2.0 ** -8 * ref_max)


@pytest.mark.parametrize("B,N,R", SHAPES, ids=lambda v: str(v))
def test_cbf_compact_vs_dense_vs_cpu(B, N, R):
    torch.manual_seed(B)
    net_c = CBFNet(3, 4, 1)
    net = CBFNet(3, 4, 1)
    net.load_state_dict(net_c.state_dict())
    net = net.to(DEV)
    states, mask, gate, wts = _inputs(B, N, R, 100 + B, 0.15)
    ref = _cpu_oracle(net_c, states, mask, gate, wts, N, R)
    dev = [t.to(DEV) for t in (states, mask, gate, wts)]
    out = {}
    for compact in (False, True):
        net.zero_grad(set_to_none=True)
        h, ds = _run(net, *dev, N, R, compact)
        out[compact] = (h, ds, {k: p.grad.float().cpu() for k, p in net.named_parameters()})
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])
    for k in ref:  # dW/db are summed in the dense call's order (row map)
        assert torch.equal(out[True][2][k], out[False][2][k]), k
    bad = []
    for k, r in ref.items():
        ed = float((out[False][2][k] - r).abs().mean())
        ec = float((out[True][2][k] - r).abs().mean())
        print(f"[{B},{N},{R}] {k}: err_dense {ed:.3e} err_compact {ec:.3e}")
        rmax = float(r.abs().max())
        if not (_rule(ec, ed, rmax) and _rule(ed, ec, rmax)):
            bad.append((k, ed, ec, rmax))
    assert not bad, bad


@pytest.mark.parametrize("B,N,R", SHAPES, ids=lambda v: str(v))
def test_captured_replay_two_masks(B, N, R):
    """Forward and backward captured once with the compact path, replayed on
    two masks of different density through the same buffers: h and dstates
    bit-equal to the eager dense path, the directly accumulated parameter
    gradients bit-equal to the eager compact path."""
    torch.manual_seed(7 + B)
    net = CBFNet(3, 4, 1).to(DEV)
    a = [t.to(DEV) for t in _inputs(B, N, R, 200 + B, 0.05)]
    b = [t.to(DEV) for t in _inputs(B, N, R, 300 + B, 0.45)]
    buf = [torch.empty_like(t) for t in a]
    params = list(net.parameters())
    grad_bufs = [torch.zeros_like(p) for p in params]

    def static_grads():
        for p, gb in zip(params, grad_bufs):
            p.grad = gb  # live buffers: the direct-accumulate dW path

    static_grads()
    res = {}

    def body():
        for p in params:
            p.grad.zero_()
        st = buf[0].clone().requires_grad_(True)
        mi = ops.edge_msg_in(st, N, R, 2, COMM)
        g = GraphBatch(states=st, mask=buf[1], n_agents=N, n_rays=R)
        ec = ops.EdgeCompact.build(buf[1], row_gate=buf[2])
        h = net(g, None, msg_in=mi, row_gate=buf[2], compact=ec).squeeze(-1)
        with ops.deferred_dw(DEV):
            (h * buf[3]).sum().backward()
        res["h"], res["ds"] = h.detach(), st.grad

    for dst, src in zip(buf, a):
        dst.copy_(src)
    torch.cuda.synchronize()
    for _ in range(2):
        body()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for inp in (b, a, b):
        for dst, src in zip(buf, inp):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = (res["h"].clone(), res["ds"].clone(), [gb.clone() for gb in grad_bufs])
        for p in params:
            p.grad = None
        h_d, ds_d = _run(net, *inp, N, R, compact=False)
        static_grads()
        for gb in grad_bufs:
            gb.zero_()
        h_c, ds_c = _run(net, *inp, N, R, compact=True)  # immediate dW launches
        grads_c = [gb.clone() for gb in grad_bufs]
        assert torch.equal(got[0], h_d) and torch.equal(got[0], h_c)
        assert torch.equal(got[1], ds_d) and torch.equal(got[1], ds_c)
        for gg, gc in zip(got[2], grads_c):
            assert torch.equal(gg, gc)
        static_grads()
