"""The device row count ``m_dev`` of the GEMM family (edge compaction): every
kernel that takes it, at the smallest shape that reaches the kernel, with
counts 0, 128, 1280 and M (a count past M clamps to M).

Forward and dX: rows below the count are bit-equal to the call without m_dev,
rows at or past it keep the sentinel of a pre-filled output, and the input
rows past the count are NaN (nothing may read them). dW/db: operands NaN past
the count, result finite and within the rounding bound of
tests/test_gemm_oracle.py against the float64 product of the live rows. dW/db
through a row map (compact operands, dense summation order): bit-equal to the
dense call."""
import pytest
import torch

import test_gemm_oracle as O
from test_gemm_oracle import BF16, F32, F64

pytestmark = pytest.mark.gpu

DEV = "cuda"
COUNTS = (0, 128, 1280, None)  # None: M
SENTINEL = 7.0
M_BIG = 16512  # first multiple of 128 above the small-M limit of gemm_plan


def _ext():
    from gcbfplus_amd import _C
    return _C


def _mdev(count):
    return torch.tensor([count], dtype=torch.int32, device=DEV)


def _poison(t, live):
    t = t.clone()
    t[live:] = float("nan")
    return t


# (expected path, M, K, N)
FWD = [("glds", M_BIG, 64, 64), ("base", M_BIG, 32, 64), ("sm", 256, 64, 64),
       ("dot", 1536, 64, 1), ("gemv", 1536, 64, 4)]


@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
@pytest.mark.parametrize("path,M,K,N", FWD, ids=lambda v: str(v))
def test_fwd_rows(path, M, K, N, count):
    ext = _ext()
    assert ext.gemm_path("fwd", M, K, N) == path
    count = M if count is None else count
    live = min(count, M)
    c = O.make_fwd(M, K, N, "rand")
    x, w, b = c["x"].to(DEV), c["w"].to(DEV), c["bias"].to(DEV)
    full = ext.gemm_bias_act(x, w, b, O.ACT_RELU)
    out = torch.full_like(full, SENTINEL)
    got = ext.gemm_bias_act(_poison(x, live), w, b, O.ACT_RELU, _mdev(count), out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out[:live], full[:live])
    assert torch.equal(out[live:], torch.full_like(out[live:], SENTINEL))


# (expected path, M, Kred, Nout, actin)
BT = [("glds_bt", M_BIG, 64, 64, 0), ("base_bt", M_BIG, 64, 64, 1), ("sm_bt", 256, 64, 64, 1)]


@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
@pytest.mark.parametrize("path,M,K,N,actin", BT, ids=lambda v: str(v))
def test_bt_rows(path, M, K, N, actin, count):
    ext = _ext()
    assert ext.gemm_path("bt", M, K, N, actin) == path
    count = M if count is None else count
    live = min(count, M)
    c = O.make_bt(M, K, N, actin, "rand")
    dy, y, w = c["dy"].to(DEV), c["y"].to(DEV), c["w"].to(DEV)
    full = ext.gemm_bt(dy, w, y, actin)
    out = torch.full_like(full, SENTINEL)
    ext.gemm_bt(_poison(dy, live), w, _poison(y, live), actin, _mdev(count), out)
    assert torch.equal(out[:live], full[:live])
    assert torch.equal(out[live:], torch.full_like(out[live:], SENTINEL))


# (variant, M, K, N, gate kinds)
TN = [("tn3", M_BIG, 64, 64, ("none", "half")), ("tn1", 256, 64, 64, ("none",))]
TN_PARAMS = [(v, M, K, N, g) for v, M, K, N, gates in TN for g in gates]


@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"count{c}")
@pytest.mark.parametrize("variant,M,K,N,gate", TN_PARAMS, ids=lambda v: str(v))
def test_tn_live_rows(variant, M, K, N, gate, count):
    ext = _ext()
    actin = O.ACT_RELU
    assert ext.gemm_path("tn", M, K, N, actin, gate != "none") == O.tn_path(variant, M, K, N)
    count = M if count is None else count
    live = min(count, M)
    c = O.make_tn(M, K, N, actin, gate, "rand")
    g = None if c["gate"] is None else c["gate"].to(DEV)
    dw, db = ext.gemm_tn(_poison(c["x"], live).to(DEV), _poison(c["dy"], live).to(DEV),
                         _poison(c["y"], live).to(DEV), actin, g, _mdev(count))
    out = torch.cat([dw, db[None]]).cpu()
    assert out.dtype == F32 and torch.isfinite(out).all()
    # float64 product of the live rows; every one of the S slab partials and
    # the reduce add roundings: R = live + S as in the oracle's canon()
    dz = O.fold(c["dy"][:live], c["y"][:live], actin).to(F64)
    if c["gate"] is not None:
        dz = dz * c["gate"][:live].to(F64)[:, None]
    A = torch.cat([c["x"][:live].to(F64).t(), torch.ones(1, live, dtype=F64)])
    S, _ = O.tn_split(M, K, N)
    worst = O.check_bounded(out, A, dz, torch.zeros(N, dtype=F64), O.ACT_NONE, live + S,
                            f"{variant} count={count} gate={gate}")
    print(f"MDEV_RATIO {variant} {M}x{K}x{N} count={count} gate={gate} worst={worst:.3g}")


def test_acc_entry_points_take_m_dev():
    """gemm_tn_acc / gemm_tn_acc2 / gemm_tn_defer with a count: the same bits
    as gemm_tn with that count, added to the destination; a deferred call with
    a count runs at once (the grouped kernels take none)."""
    ext = _ext()
    M, K, N, count = 256, 64, 64, 128
    c = O.make_tn(M, K, N, 0, "none", "rand")
    x, dy = _poison(c["x"], count).to(DEV), _poison(c["dy"], count).to(DEV)
    md = _mdev(count)
    dw, db = ext.gemm_tn(x, dy, dy, 0, None, md)
    for name in ("acc", "acc2", "defer"):
        w = torch.ones(K, N, device=DEV)
        b = torch.ones(N, device=DEV)
        b2 = torch.ones(N, device=DEV)
        if name == "acc":
            ext.gemm_tn_acc(x, dy, dy, 0, w, b, None, md)
        elif name == "acc2":
            ext.gemm_tn_acc2(x, dy, dy, 0, w, b, b2, None, md)
        else:
            ext.gemm_tn_defer(x, dy, dy, 0, w, b, b2, None, md)
            assert ext.dw_pending() == 0
        assert torch.equal(w, 1.0 + dw) and torch.equal(b, 1.0 + db), name
        if name != "acc":
            assert torch.equal(b2, 1.0 + db), name


@pytest.mark.parametrize("variant,M,K,N,gate", TN_PARAMS, ids=lambda v: str(v))
def test_tn_row_map_keeps_dense_bits(variant, M, K, N, gate):
    """dW/db through a row map (compact operands, dense summation order) against
    the dense call on the scattered operands, whose masked rows have dZ == 0
    and arbitrary X: bit for bit. Compact rows past the count hold NaN."""
    ext = _ext()
    actin = O.ACT_RELU
    c = O.make_tn(M, K, N, actin, gate, "rand")
    g = torch.Generator().manual_seed(M + K)
    live = torch.rand(M, generator=g) < 0.1
    rows = live.nonzero().reshape(-1)
    count = rows.numel()
    inv = torch.full((M,), -1, dtype=torch.int32)
    inv[rows] = torch.arange(count, dtype=torch.int32)
    dy_dense = c["dy"].clone()
    dy_dense[~live] = 0
    gd = None if c["gate"] is None else c["gate"].to(DEV)
    dw, db = ext.gemm_tn(c["x"].to(DEV), dy_dense.to(DEV), c["y"].to(DEV), actin, gd)

    def compact(t, fill):
        out = torch.full_like(t, fill)
        out[:count] = t[rows]
        return out.to(DEV)

    gc = None if c["gate"] is None else compact(c["gate"], False)
    dw_c, db_c = ext.gemm_tn(compact(c["x"], float("nan")), compact(c["dy"], float("nan")),
                             compact(c["y"], float("nan")), actin, gc, None, inv.to(DEV))
    assert torch.equal(dw_c, dw) and torch.equal(db_c, db)
