"""reduce_dw_db_kernel through its own binding: the (S, K, N) / (S, N)
partials are summed in one fixed order,

    a_j = sum of src[s] over s = j (mod 4), s < 4*(S//4), increasing s
    a_0 += the remaining s, in order
    r   = (a_0 + a_1) + (a_2 + a_3)
    dst = dst + r if acc else r;  db2 += r for the db part

and the kernel must reproduce a float32 CPU emulation of that order bit for
bit. The partials mix magnitudes over six decades, so the order matters: the
emulation itself is first shown to change bits when the slabs are visited in
another order, else equality would prove nothing."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 12345.0
SHAPES = [(1, 3, 1), (7, 10, 1), (8, 64, 64), (64, 5, 20), (120, 8, 4), (128, 64, 64)]


def _ext():
    from gcbfplus_amd import _C
    return _C


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _mixed(g, shape):
    mag = 10.0 ** torch.randint(-3, 4, shape, generator=g).to(torch.float32)
    return torch.randn(shape, generator=g) * mag


def _ordered_sum(p, order=None):
    """(S, n) float32 -> (n,) in the kernel's order; ``order`` visits the
    slabs in another sequence (used only to show the order matters)."""
    S = p.shape[0]
    if order is not None:
        p = p[order]
    S4 = S // 4 * 4
    a = [torch.zeros(p.shape[1]) for _ in range(4)]
    for s in range(S4):
        a[s % 4] = a[s % 4] + p[s]
    for s in range(S4, S):
        a[0] = a[0] + p[s]
    return (a[0] + a[1]) + (a[2] + a[3])


def _inputs(S, K, N):
    g = _gen("reduce", S, K, N)
    pw, pb = _mixed(g, (S, K, N)), _mixed(g, (S, N))
    dw0, db0, db20 = _mixed(g, (K, N)), _mixed(g, (N,)), _mixed(g, (N,))
    rw, rb = _ordered_sum(pw.view(S, K * N)).view(K, N), _ordered_sum(pb)
    if S > 1:  # the emulation is order-sensitive on these very inputs
        # (a rotation: reversing the slabs only mirrors the four chains)
        rot = torch.arange(1, S + 1) % S
        other = torch.cat([_ordered_sum(pw.view(S, K * N), rot), _ordered_sum(pb, rot)])
        assert not torch.equal(other, torch.cat([rw.flatten(), rb]))
    return pw, pb, dw0, db0, db20, rw, rb


@pytest.mark.parametrize("with_db2", [False, True], ids=["nodb2", "db2"])
@pytest.mark.parametrize("acc", [False, True], ids=["write", "acc"])
@pytest.mark.parametrize("S,K,N", SHAPES, ids=lambda v: str(v))
def test_reduce_order_bit_exact(S, K, N, acc, with_db2):
    pw, pb, dw0, db0, db20, rw, rb = _inputs(S, K, N)
    dw, db, db2 = dw0.to(DEV), db0.to(DEV), db20.to(DEV)
    _ext().reduce_dw_db(pw.to(DEV), pb.to(DEV), dw, db, db2 if with_db2 else None, acc)
    assert torch.equal(dw.cpu(), dw0 + rw if acc else rw)
    assert torch.equal(db.cpu(), db0 + rb if acc else rb)
    assert torch.equal(db2.cpu(), db20 + rb if with_db2 else db20)


@pytest.mark.parametrize("S,K,N", [(8, 64, 64), (7, 10, 1)], ids=lambda v: str(v))
def test_reduce_into_odd_offset_view(S, K, N):
    """dW a view at an odd float offset of a sentinel-filled buffer (no
    16-byte store can be used); the guards stay intact."""
    pw, pb, dw0, db0, _, rw, rb = _inputs(S, K, N)
    lo, n = 1023, K * N
    buf = torch.full((lo + n + 1024,), SENT, device=DEV)
    buf[lo:lo + n] = dw0.flatten().to(DEV)
    dw = buf[lo:lo + n].view(K, N)
    assert dw.data_ptr() % 16 != 0
    db = db0.to(DEV)
    _ext().reduce_dw_db(pw.to(DEV), pb.to(DEV), dw, db, None, True)
    out = buf.cpu()
    assert torch.equal(out[lo:lo + n].view(K, N), dw0 + rw)
    assert torch.equal(db.cpu(), db0 + rb)
    assert torch.equal(out[:lo], torch.full((lo,), SENT))
    assert torch.equal(out[lo + n:], torch.full((1024,), SENT))
