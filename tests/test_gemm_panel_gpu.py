"""Row-panel GEMM kernel (dispatch names ``glds`` / ``glds_bt``) at the
shapes where its code takes another turn: one and several 64-column tiles
(W buffer parity), one and several 64-wide K chunks, an 8-column tail tile,
W rows that are not 16-byte aligned (the register-staged zero-filling
stage), the single-W-buffer regime at K = 384, and K = 512 where the panel
does not fit and the shape goes to the 128x64 kernel. M = 16512 is the
smallest M the path accepts (129 workgroups).

Operands and comparators are those of tests/test_gemm_oracle.py: bit for bit
against the float64 product on small-integer operands, the rounding bound on
random operands where marked. Random-operand results are also compared bit
for bit between two calls and with the 128x64 kernel (GCBF_GEMM_NOGLDS),
which shares the MFMA, the k -> operand-slot map and the epilogue arithmetic.
"""
import pytest
import torch

import test_gemm_oracle as O
from test_gemm_oracle import ACT_NONE, ACT_RELU, ACT_TANH, BF16

pytestmark = pytest.mark.gpu

DEV = "cuda"
M = 16512

# (expected path, K, N, also bounded?)
FWD = [
    ("glds", 64, 64, False),     # one tile, one K chunk
    ("glds", 128, 192, False),   # three tiles: buffer parity
    ("glds", 256, 256, True),    # four tiles, the training shape
    ("glds", 64, 72, False),     # 8-column tail tile
    ("glds", 128, 70, False),    # N % 8 != 0: unaligned rows, ragged tail
    ("glds", 128, 20, False),    # N % 8 != 0: unaligned rows, ragged tail
    ("glds", 384, 128, False),   # single-W-buffer regime, two tiles
    ("base", 512, 64, False),    # panel does not fit
]
# (expected path, Kred, Nout, also bounded?)
BT = [
    ("glds_bt", 128, 128, False),
    ("glds_bt", 256, 128, True),
    ("glds_bt", 64, 100, False),   # ragged Nout on aligned M
    ("glds_bt", 256, 10, False),   # dX of a K = 10 layer
    ("glds_bt", 384, 64, False),
    ("base_bt", 512, 64, False),   # panel does not fit
]


def _ext():
    from gcbfplus_amd import _C
    return _C


def _run_fwd(c, act):
    return _ext().gemm_bias_act(c["x"].to(DEV), c["w"].to(DEV), c["bias"].to(DEV), act)


def _run_bt(c):
    dy = c["dy"].to(DEV)
    return _ext().gemm_bt(dy, c["w"].to(DEV), dy, 0)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_TANH])
@pytest.mark.parametrize("path,K,N,bounded", FWD, ids=[f"{p}-{k}x{n}" for p, k, n, _ in FWD])
def test_panel_fwd(path, K, N, bounded, act):
    assert _ext().gemm_path("fwd", M, K, N) == path
    c = O.fwd_case(M, K, N, act, "int")
    y = _run_fwd(c, act)
    assert y.dtype == BF16
    O.check_exact(y.cpu(), O.reference(c, act), f"fwd {path} {M}x{K}x{N} act{act}")
    if bounded:
        c = O.fwd_case(M, K, N, act, "rand")
        A, B, bias, act_, _, R = O.canon(c, act)
        r = O.check_bounded(_run_fwd(c, act).cpu(), A, B, bias, act_, R)
        print(f"GEMM_RATIO path={path} fwd {M}x{K}x{N} act{act} worst_err_over_limit={r:.3g}")


@pytest.mark.parametrize("path,K,N,bounded", BT, ids=[f"{p}-{k}x{n}" for p, k, n, _ in BT])
def test_panel_bt(path, K, N, bounded):
    assert _ext().gemm_path("bt", M, K, N, 0) == path
    c = O.bt_case(M, K, N, 0, "int")
    dx = _run_bt(c)
    assert dx.dtype == BF16
    O.check_exact(dx.cpu(), O.reference(c), f"bt {path} {M}x{K}x{N}")
    if bounded:
        c = O.bt_case(M, K, N, 0, "rand")
        A, B, bias, act_, _, R = O.canon(c)
        r = O.check_bounded(_run_bt(c).cpu(), A, B, bias, act_, R)
        print(f"GEMM_RATIO path={path} bt {M}x{K}x{N} worst_err_over_limit={r:.3g}")


def test_panel_repeats_and_matches_128x64_kernel(monkeypatch):
    """On random operands two calls give the same bits, and those are the
    bits of the 128x64 kernel, which is not the code under test."""
    ext = _ext()
    cf = O.fwd_case(M, 256, 256, ACT_RELU, "rand")
    cb = O.bt_case(M, 256, 128, 0, "rand")
    assert ext.gemm_path("fwd", M, 256, 256) == "glds"
    assert ext.gemm_path("bt", M, 256, 128, 0) == "glds_bt"
    yf, yb = _run_fwd(cf, ACT_RELU), _run_bt(cb)
    assert torch.equal(yf, _run_fwd(cf, ACT_RELU))
    assert torch.equal(yb, _run_bt(cb))
    monkeypatch.setenv("GCBF_GEMM_NOGLDS", "1")
    assert ext.gemm_path("fwd", M, 256, 256) == "base"
    assert ext.gemm_path("bt", M, 256, 128, 0) == "base_bt"
    assert torch.equal(yf, _run_fwd(cf, ACT_RELU))
    assert torch.equal(yb, _run_bt(cb))
