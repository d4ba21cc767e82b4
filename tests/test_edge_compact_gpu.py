"""Edge compaction kernels (ops/hip/edge_compact.hip) against torch and against
the dense softmax-aggregate kernels, B = 3, N = 4, R = 5 (D = 10): random
masks and four fixed ones (nothing active, everything active, one receiver
with every slot masked, one receiver with every slot active). Everything is
compared bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, N, R = 3, 4, 5
D = N + 1 + R
C = 128
M = B * N * D
CAP = (M + 127) // 128 * 128


def _ext():
    from gcbfplus_amd import _C
    return _C


def _masks():
    g = torch.Generator().manual_seed(5)
    out = {}
    for i, p in enumerate((0.1, 0.5, 0.9)):
        out[f"rand{i}"] = torch.rand(B, N, D, generator=g) < p
    out["none"] = torch.zeros(B, N, D, dtype=torch.bool)
    out["all"] = torch.ones(B, N, D, dtype=torch.bool)
    m = torch.rand(B, N, D, generator=g) < 0.5
    m[1, 2] = False
    out["recv_masked"] = m
    m = torch.rand(B, N, D, generator=g) < 0.3
    m[2, 0] = True
    out["recv_full"] = m
    return out


MASKS = _masks()


@pytest.fixture(scope="module", params=sorted(MASKS))
def compact(request):
    mask = MASKS[request.param].to(DEV)
    gate = (torch.arange(B * N, device=DEV) % 3 != 0)
    prefix = 5  # receivers in the prefix count
    rows, inv, off, cnt, gate_c = _ext().edge_compact(mask, 128, prefix, gate)
    torch.cuda.synchronize()
    return dict(mask=mask, gate=gate, prefix=prefix, rows=rows, inv=inv, off=off, cnt=cnt,
                gate_c=gate_c, count=int(mask.sum()))


def test_compaction(compact):
    c = compact
    mask, count = c["mask"], c["count"]
    rows, inv, off, cnt = c["rows"], c["inv"], c["off"], c["cnt"]
    assert rows.dtype == inv.dtype == off.dtype == cnt.dtype == torch.int32
    assert rows.shape == (CAP,) and inv.shape == (M,) and off.shape == (B * N + 1,)
    want_rows = torch.nonzero(mask.reshape(-1)).reshape(-1).to(torch.int32)
    assert torch.equal(rows[:count], want_rows)
    per_recv = mask.reshape(B * N, D).sum(1)
    want_off = torch.cat([per_recv.new_zeros(1), per_recv.cumsum(0)]).to(torch.int32)
    assert torch.equal(off, want_off)
    want_inv = torch.full((M,), -1, dtype=torch.int32, device=DEV)
    want_inv[want_rows.long()] = torch.arange(count, dtype=torch.int32, device=DEV)
    assert torch.equal(inv, want_inv)
    pad = (count + 127) // 128 * 128
    pcount = int(want_off[c["prefix"]])
    assert cnt.tolist() == [count, pad, pcount, (pcount + 127) // 128 * 128]
    assert pad <= CAP
    assert torch.equal(c["gate_c"][:count], c["gate"][(want_rows // D).long()])


def test_gather_and_scatter(compact):
    c = compact
    ext = _ext()
    count, pad = c["cnt"][0].item(), c["cnt"][1].item()
    g = torch.Generator().manual_seed(11)
    X = torch.randn(M, 32, generator=g).to(torch.bfloat16).to(DEV)
    Xc = ext.gather_rows(X, c["rows"], c["cnt"], CAP)
    assert Xc.shape == (CAP, 32)
    assert torch.equal(Xc[:count], X[c["rows"][:count].long()])
    assert torch.equal(Xc[count:pad], torch.zeros_like(Xc[count:pad]))
    dXc = torch.randn(CAP, 32, generator=g).to(torch.bfloat16).to(DEV)
    dX = ext.gather_rows_bwd(dXc, c["inv"], M)
    dense = torch.zeros(M, 32, dtype=torch.bfloat16, device=DEV)
    dense[c["rows"][:count].long()] = dXc[:count]  # the dense gradient, masked rows zero
    assert torch.equal(dX, dense)


def test_compact_softmax_matches_dense(compact):
    c = compact
    ext = _ext()
    mask = c["mask"]
    count, pad = c["cnt"][0].item(), c["cnt"][1].item()
    live = c["rows"][:count].long()
    g = torch.Generator().manual_seed(23)
    gate = (2.0 * torch.randn(B, N, D, generator=g)).to(DEV)
    msg = torch.randn(B, N, D, C, generator=g).to(torch.bfloat16).to(DEV)
    daggr = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(DEV)
    aggr, attn = ext.softmax_aggr_fwd(gate, msg, mask)
    dgate, dmsg = ext.softmax_aggr_bwd(daggr, attn, msg, mask)

    # compact operands; rows past the count hold NaN: nothing may read them
    gate_c = torch.full((CAP,), float("nan"), device=DEV)
    msg_c = torch.full((CAP, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    gate_c[:count] = gate.reshape(-1)[live]
    msg_c[:count] = msg.reshape(M, C)[live]
    aggr_c, attn_c = ext.softmax_aggr_c_fwd(gate_c, msg_c, c["off"], c["inv"], D)
    assert torch.equal(aggr_c, aggr.reshape(B * N, C))
    assert torch.equal(attn_c[:count], attn.reshape(-1)[live])
    empty = ~mask.reshape(B * N, D).any(1)
    assert torch.equal(aggr_c[empty], torch.zeros_like(aggr_c[empty]))

    dgate_c, dmsg_c = ext.softmax_aggr_c_bwd(daggr.reshape(B * N, C), attn_c, msg_c, c["off"],
                                             c["rows"], c["cnt"], D)
    assert torch.equal(dgate_c[:count], dgate.reshape(-1)[live])
    assert torch.equal(dmsg_c[:count], dmsg.reshape(M, C)[live])
    assert torch.equal(dgate_c[count:pad], torch.zeros_like(dgate_c[count:pad]))
    assert torch.equal(dmsg_c[count:pad], torch.zeros_like(dmsg_c[count:pad]))
    # masked slots of the dense kernels carry exact zeros: nothing is lost
    dead = ~mask.reshape(-1)
    assert torch.equal(dgate.reshape(-1)[dead], torch.zeros_like(dgate.reshape(-1)[dead]))
    assert torch.equal(dmsg.reshape(M, C)[dead], torch.zeros_like(dmsg.reshape(M, C)[dead]))


def test_add_rows_matches_torch_add(compact):
    c = compact
    pad = c["cnt"][1].item()
    g = torch.Generator().manual_seed(31)
    a = torch.randn(CAP, C, generator=g).to(torch.bfloat16).to(DEV)
    b = torch.randn(CAP, C, generator=g).to(torch.bfloat16).to(DEV)
    out = _ext().add_rows_bf16(a, b, c["cnt"])
    assert torch.equal(out[:pad], (a + b)[:pad])
