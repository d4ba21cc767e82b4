"""The row-major-staged dW kernel (gemm_tn_partial3_kernel) at the shapes the
path matrix of test_gemm_paths_gpu.py does not reach: b128 staging on ragged
tiles (K, N multiples of 8 that are no multiples of 64), operands whose base
is not 16-byte aligned (scalar fallback), operands embedded in NaN (nothing
outside them may feed the result), and slabs whose last tile has one live
row. Integer operands compare bit for bit with the float64 reference of
tests/test_gemm_oracle.py; one random case runs its rounding bound."""
import pytest
import torch

import test_gemm_oracle as O
from test_gemm_oracle import BF16, F32

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN_ROWS = 64  # rows of filler on each side of an embedded operand


def _ext():
    from gcbfplus_amd import _C
    return _C


def _cu(t):
    return None if t is None else t.to(DEV)


def _assert_tn3(M, K, N, actin, gate):
    assert M >= 16384
    path = _ext().gemm_path("tn", M, K, N, actin, gate != "none")
    assert path.startswith("tn3") and path == O.tn_path("tn3", M, K, N), path
    return path


def _run(case, x=None, dy=None, y=None):
    x = _cu(case["x"]) if x is None else x
    dy = _cu(case["dy"]) if dy is None else dy
    y = _cu(case["y"]) if y is None else y
    actin = case["actin"]
    dw, db = _ext().gemm_tn(x, dy, y if actin else dy, actin, _cu(case["gate"]))
    assert dw.dtype == F32 and db.dtype == F32
    return torch.cat([dw, db[None]]).cpu()


def _embed(t, shift, fill):
    """A contiguous view equal to ``t`` that starts ``shift`` elements past a
    16-byte boundary, with NAN_ROWS rows' worth of ``fill`` on either side."""
    rows, cols = t.shape
    pad = NAN_ROWS * cols  # a multiple of 8 elements: keeps the boundary
    assert pad % 8 == 0
    buf = torch.full((pad + shift + rows * cols + pad,), fill, dtype=BF16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[pad + shift:pad + shift + rows * cols].view(rows, cols)
    v.copy_(t.to(DEV))
    assert v.is_contiguous() and v.data_ptr() % 16 == (2 * shift) % 16
    return v


# --------------------------------------------------------------------------
# vector staging on ragged tiles
# --------------------------------------------------------------------------
RAGGED = [(16421, 72, 200), (16385, 136, 8), (16384, 8, 72)]


@pytest.mark.parametrize("gate", ["none", "half"])
@pytest.mark.parametrize("actin", [0, 1, 2])
@pytest.mark.parametrize("M,K,N", RAGGED, ids=lambda v: str(v))
def test_ragged_vector_tiles_exact(M, K, N, actin, gate):
    path = _assert_tn3(M, K, N, actin, gate)
    c = O.tn_case(M, K, N, actin, gate, "int")
    O.check_preconditions(c)
    O.check_exact(_run(c), O.reference(c), f"{path} {M}x{K}x{N} actin{actin} gate={gate}")


def test_ragged_vector_tiles_bounded():
    M, K, N, actin, gate = 16421, 72, 200, 2, "half"
    _assert_tn3(M, K, N, actin, gate)
    c = O.tn_case(M, K, N, actin, gate, "rand")
    A, B, bias, act_, _, R = O.canon(c)
    worst = O.check_bounded(_run(c), A, B, bias, act_, R, "tn3 ragged")
    print(f"GEMM_RATIO path=tn3 tn {M}x{K}x{N} worst_err_over_limit={worst:.3g}")
    assert worst <= 1.0


# --------------------------------------------------------------------------
# operand bases off the 16-byte grid, operands embedded in NaN
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def embedded_case():
    M, K, N, actin, gate = 16421, 64, 128, 2, "half"
    c = O.tn_case(M, K, N, actin, gate, "int")
    O.check_preconditions(c)
    return c, O.reference(c)


def test_unaligned_bases_exact(embedded_case):
    c, ref = embedded_case
    _assert_tn3(c["M"], c["K"], c["N"], c["actin"], "half")
    out = _run(c, *(_embed(c[k], 1, 0.0) for k in ("x", "dy", "y")))
    O.check_exact(out, ref, "tn3 bases at 2 bytes past a 16-byte boundary")


@pytest.mark.parametrize("shift", [1, 0], ids=["unaligned", "aligned"])
def test_nan_around_operands_exact(embedded_case, shift):
    """shift 1 walks the scalar fallback, shift 0 the b128 loads, whose rows
    past a slab end and chunks past the last column must not be fetched into
    the result either."""
    c, ref = embedded_case
    out = _run(c, *(_embed(c[k], shift, float("nan")) for k in ("x", "dy", "y")))
    assert torch.isfinite(out).all()
    O.check_exact(out, ref, f"tn3 operands embedded in NaN, shift {shift}")


# --------------------------------------------------------------------------
# slab tails: the last tile of every slab has one live row
# --------------------------------------------------------------------------
@pytest.mark.parametrize("gate", ["none", "half"])
def test_slab_tail_single_row(gate):
    M, K, N, actin = 16385, 64, 64, 1
    _assert_tn3(M, K, N, actin, gate)
    S, remap = O.tn_split(M, K, N)
    assert (S, remap) == (128, True) and (M + S - 1) // S == 129  # 2 tiles + 1 row
    c = O.tn_case(M, K, N, actin, gate, "int")
    O.check_preconditions(c)
    O.check_exact(_run(c), O.reference(c), f"tn3 129-row slabs gate={gate}")
