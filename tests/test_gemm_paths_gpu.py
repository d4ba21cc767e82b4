"""Path-complete tests of the GEMM kernel family on the GPU: every kernel the
launchers in bindings.hip can select by default is run at shapes that reach
it (asserted through ``_C.gemm_path``) and compared with the float64
reference of tests/test_gemm_oracle.py: bit for bit on small-integer
operands, and within the rounding bound on random operands for the cases
the matrix tags. The oracle's CPU self-tests prove the inputs meet the
comparators' preconditions and that the comparators see the defects they
are here to catch."""
import pytest
import torch

import test_gemm_oracle as O
from test_gemm_oracle import ACT_NONE, ACT_RELU, ACT_TANH, BF16, F32, F64

pytestmark = pytest.mark.gpu

from gcbfplus_amd import ops

DEV = "cuda"
SENT = 12345.0   # guard sentinel around accumulate targets
PAD = 1024       # guard elements on each side


def _ext():
    from gcbfplus_amd import _C
    return _C


def _cu(t):
    return None if t is None else t.to(DEV)


def _report(path, what, ratio):
    print(f"GEMM_RATIO path={path} {what} worst_err_over_limit={ratio:.3g}")


# --------------------------------------------------------------------------
# forward: _C.gemm_bias_act
# --------------------------------------------------------------------------
def _run_fwd(case, act):
    return _ext().gemm_bias_act(_cu(case["x"]), _cu(case["w"]), _cu(case["bias"]), act)


def _fwd_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}"


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU])
@pytest.mark.parametrize("case", O.FWD_CASES, ids=_fwd_id)
def test_fwd_exact(case, act):
    path, M, K, N, _ = case
    assert _ext().gemm_path("fwd", M, K, N) == path
    c = O.fwd_case(M, K, N, act, "int")
    y = _run_fwd(c, act)
    assert y.dtype == (F32 if N <= 16 else BF16)
    O.check_exact(y.cpu(), O.reference(c, act), f"fwd {path} {M}x{K}x{N} act{act}")


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_TANH])
@pytest.mark.parametrize("case", [c for c in O.FWD_CASES if c[4]], ids=_fwd_id)
def test_fwd_bounded(case, act):
    path, M, K, N, _ = case
    assert _ext().gemm_path("fwd", M, K, N) == path
    c = O.fwd_case(M, K, N, act, "rand")
    y = _run_fwd(c, act).cpu()
    A, B, bias, act_, out_dtype, R = O.canon(c, act)
    assert y.dtype == out_dtype
    _report(path, f"fwd {M}x{K}x{N} act{act}", O.check_bounded(y, A, B, bias, act_, R))


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU])
def test_fwd_noglds_toggle_takes_base_kernel(monkeypatch, act):
    """The per-call env toggle moves a glds shape to the 128x64 kernel, in
    the launcher and in the query alike."""
    path, M, K, N, _ = O.FWD_NOGLDS_CASE
    assert _ext().gemm_path("fwd", M, K, N) == "glds"
    monkeypatch.setenv("GCBF_GEMM_NOGLDS", "1")
    assert _ext().gemm_path("fwd", M, K, N) == path == "base"
    assert _ext().gemm_path("bt", M, K, N) == "base_bt"
    c = O.fwd_case(M, K, N, act, "int")
    O.check_exact(_run_fwd(c, act).cpu(), O.reference(c, act), "fwd base (NOGLDS)")


# --------------------------------------------------------------------------
# dX: _C.gemm_bt
# --------------------------------------------------------------------------
def _run_bt(case):
    dy, y = _cu(case["dy"]), _cu(case["y"])
    actin = case["actin"]
    return _ext().gemm_bt(dy, _cu(case["w"]), y if actin else dy, actin)


def _bt_params():
    for path, M, K, N, actins, bounded_actin in O.BT_CASES:
        for actin in actins:
            yield pytest.param(path, M, K, N, actin, bounded_actin == actin,
                               id=f"{path}-{M}x{K}x{N}-actin{actin}")


@pytest.mark.parametrize("path,M,K,N,actin,bounded", list(_bt_params()))
def test_bt(path, M, K, N, actin, bounded):
    assert _ext().gemm_path("bt", M, K, N, actin) == path
    c = O.bt_case(M, K, N, actin, "int")
    dx = _run_bt(c)
    assert dx.dtype == BF16
    O.check_exact(dx.cpu(), O.reference(c), f"bt {path} {M}x{K}x{N} actin{actin}")
    if bounded:
        c = O.bt_case(M, K, N, actin, "rand")
        A, B, bias, act_, _, R = O.canon(c)
        _report(path, f"bt {M}x{K}x{N} actin{actin}",
                O.check_bounded(_run_bt(c).cpu(), A, B, bias, act_, R))


# --------------------------------------------------------------------------
# dW/db: _C.gemm_tn, _acc, _acc2
# --------------------------------------------------------------------------
def _tn_args(case):
    dy, y = _cu(case["dy"]), _cu(case["y"])
    actin = case["actin"]
    return _cu(case["x"]), dy, (y if actin else dy), actin


def _run_tn(case):
    dw, db = _ext().gemm_tn(*_tn_args(case), _cu(case["gate"]))
    assert dw.dtype == F32 and db.dtype == F32
    return torch.cat([dw, db[None]]).cpu()


def _old_values(shape, *key):
    """Non-zero integers already in an accumulate target."""
    v = O._ints(O._gen("old", shape, *key), shape, -3, 3, F32)
    return torch.where(v == 0, torch.ones_like(v), v)


def _guarded(old):
    buf = torch.full((PAD + old.numel() + PAD,), SENT, device=DEV)
    buf[PAD:PAD + old.numel()] = old.flatten().to(DEV)
    return buf


def _check_target(buf, old, ref, what):
    n = old.numel()
    buf = buf.cpu()
    O.check_guarded(buf, PAD, PAD + n, SENT, what)
    O.check_exact(buf[PAD:PAD + n].view(old.shape), old.to(F64) + ref, what)


def _tn_params():
    for variant, remap, M, K, N, bounded in O.TN_CASES:
        for actin in (0, 1, 2):
            for gate in O.GATES:
                yield pytest.param(variant, remap, M, K, N, actin, gate,
                                   id=f"{variant}r{remap}-{M}x{K}x{N}-actin{actin}-{gate}")


@pytest.mark.parametrize("variant,remap,M,K,N,actin,gate", list(_tn_params()))
def test_tn_exact(variant, remap, M, K, N, actin, gate):
    """gemm_tn writes dW/db; gemm_tn_acc adds them into slices of larger
    sentinel-filled buffers; gemm_tn_acc2 also adds db into a row of the
    guarded dW buffer, the layout fused_linear_onehot uses."""
    ext = _ext()
    path = ext.gemm_path("tn", M, K, N, actin, gate != "none")
    assert path == O.tn_path(variant, M, K, N) and path.endswith(f"remap={remap}")
    c = O.tn_case(M, K, N, actin, gate, "int")
    ref = O.reference(c)
    what = f"{path} {M}x{K}x{N} actin{actin} gate={gate}"
    O.check_exact(_run_tn(c), ref, "gemm_tn " + what)
    dw_ref, db_ref = ref[:K], ref[K]

    old_w, old_b = _old_values((K, N), "w"), _old_values((N,), "b")
    wbuf, bbuf = _guarded(old_w), _guarded(old_b)
    ext.gemm_tn_acc(*_tn_args(c), wbuf[PAD:PAD + K * N].view(K, N), bbuf[PAD:PAD + N],
                    _cu(c["gate"]))
    _check_target(wbuf, old_w, dw_ref, "gemm_tn_acc dw " + what)
    _check_target(bbuf, old_b, db_ref, "gemm_tn_acc db " + what)

    oh = 3  # rows 0..oh-2 of the grad buffer must stay untouched, row oh-1 += db
    old_g = torch.cat([torch.full((oh - 1, N), SENT), _old_values((1 + K, N), "g")])
    gbuf, bbuf = _guarded(old_g), _guarded(old_b)
    grad = gbuf[PAD:PAD + (oh + K) * N].view(oh + K, N)
    ext.gemm_tn_acc2(*_tn_args(c), grad[oh:], bbuf[PAD:PAD + N], grad[oh - 1], _cu(c["gate"]))
    add = torch.cat([torch.zeros(oh - 1, N, dtype=F64), db_ref[None], dw_ref])
    _check_target(gbuf, old_g, add, "gemm_tn_acc2 dw/db2 " + what)
    _check_target(bbuf, old_b, db_ref, "gemm_tn_acc2 db " + what)


@pytest.mark.parametrize("gate", ["none", "half"])
@pytest.mark.parametrize("actin", [0, 1, 2])
@pytest.mark.parametrize("case", [c for c in O.TN_CASES if c[5]],
                         ids=lambda c: f"{c[0]}-{c[2]}x{c[3]}x{c[4]}")
def test_tn_bounded(case, actin, gate):
    variant, remap, M, K, N, _ = case
    assert _ext().gemm_path("tn", M, K, N, actin, gate != "none") == O.tn_path(variant, M, K, N)
    c = O.tn_case(M, K, N, actin, gate, "rand")
    A, B, bias, act_, _, R = O.canon(c)
    _report(variant, f"tn {M}x{K}x{N} actin{actin} gate={gate}",
            O.check_bounded(_run_tn(c), A, B, bias, act_, R))


@pytest.mark.parametrize("case", [O.TN_CASES[6], O.TN_CASES[11]],
                         ids=lambda c: f"{c[0]}r{c[1]}-{c[2]}x{c[3]}x{c[4]}")
def test_tn_deterministic(case):
    """Two calls are bit-equal (test_tn_exact asserts the values)."""
    _, _, M, K, N, _ = case
    c = O.tn_case(M, K, N, ACT_TANH, "half", "rand")
    assert torch.equal(_run_tn(c), _run_tn(c))


# --------------------------------------------------------------------------
# act_bwd
# --------------------------------------------------------------------------
@pytest.mark.parametrize("act", [ACT_RELU, ACT_TANH])
@pytest.mark.parametrize("M,N", O.ACT_BWD_CASES)
def test_act_bwd_bit_exact(M, N, act):
    c = O.make_act_bwd(M, N, act)
    dz = _ext().act_bwd(_cu(c["dy"]), _cu(c["y"]), act).cpu()
    want = O.fold(c["dy"], c["y"], act)
    assert dz.dtype == BF16 and torch.equal(dz.view(torch.int16), want.view(torch.int16))
    c = O.make_bt(M, N, 1, act, "int")  # the exact-integer fold operands too
    dz = _ext().act_bwd(_cu(c["dy"]), _cu(c["y"]), act).cpu()
    assert torch.equal(dz, O.fold(c["dy"], c["y"], act))


# --------------------------------------------------------------------------
# autograd wiring: ops.fused_linear, ops.fused_linear_onehot
# --------------------------------------------------------------------------
def _linear_inputs(M, K, N, density=1.0):
    g = O._gen("fused_linear", M, K, N)
    x = O._ints(g, (M, K), -1, 1)
    w = O._ints(g, (K, N), -2, 2, F32)
    if density < 1.0:  # few live rows keep z small, so tanh does not saturate
        w = w * (torch.rand((K, 1), generator=g) < density)
    b = O._ints(g, (N,), -2, 2, F32)
    dy = O._ints(g, (M, N), -2, 2, F32)
    return x, w, b, dy


@pytest.mark.parametrize("M,K,N", [(130, 128, 48),   # act_bwd branch, padded-K dX
                                   (100, 10, 256)])  # unpadded K, ragged-Nout dX
def test_fused_linear_relu_exact(M, K, N):
    x, w, b, dy = _linear_inputs(M, K, N)
    xg, wg, bg = (_cu(t).requires_grad_(True) for t in (x, w, b))
    y = ops.fused_linear(xg, wg, bg, ACT_RELU)
    y.backward(_cu(dy).to(y.dtype))
    z = x.to(F64) @ w.to(F64) + b.to(F64)
    O.check_exact(y.detach().cpu(), torch.relu(z), "fused_linear y")
    dz = dy.to(F64) * (z > 0)
    O.check_exact(xg.grad.cpu(), dz @ w.to(F64).t(), "fused_linear dX")
    O.check_exact(wg.grad.cpu(), x.to(F64).t() @ dz, "fused_linear dW")
    O.check_exact(bg.grad.cpu(), dz.sum(0), "fused_linear db")


@pytest.mark.parametrize("N", [1, 2])
def test_fused_linear_tanh_f32_head(N):
    """Small-N heads come out in f32 and tanh(z) is no bf16 number, so the
    backward operand dz = bf16(dy * (1 - y^2)) is not an integer: forward,
    dX, dW and db are held to the rounding bound instead, with dz formed
    from the kernel's own y by the same fp32 ops as the autograd function."""
    M, K = 300, 256
    x, w, b, dy = _linear_inputs(M, K, N, density=4.0 / K)
    xg, wg, bg = (_cu(t).requires_grad_(True) for t in (x, w, b))
    y = ops.fused_linear(xg, wg, bg, ACT_TANH)
    assert y.dtype == F32
    y.backward(_cu(dy))
    yc = y.detach().cpu()
    x64, w64 = x.to(F64), w.to(F64)
    r = [O.check_bounded(yc, x64, w64, b.to(F64), ACT_TANH, K, "y")]
    assert (yc.abs() < 0.999).float().mean() > 0.3, "inputs saturate tanh"
    dz = (dy * (1.0 - yc * yc)).to(BF16).to(F64)
    zero = torch.zeros(1, dtype=F64)
    # dX = dz @ w^T runs the forward kernel on K = N zero-padded to 32
    r.append(O.check_bounded(xg.grad.cpu(), dz, w64.t(), zero, ACT_NONE, 32, "dX"))
    S, _ = O.tn_split(M, K, N)
    A = torch.cat([x64.t(), torch.ones(1, M, dtype=F64)])
    got = torch.cat([wg.grad, bg.grad[None]]).cpu()
    r.append(O.check_bounded(got, A, dz, zero, ACT_NONE, M + S, "dW/db"))
    _report("fused_linear", f"tanh head N={N} y/dX/dW", max(r))


def test_fused_linear_onehot_exact():
    """One-hot fold with direct accumulation into live grad buffers against
    the float64 composed form y = relu(x @ w[3:] + (b + w[2]))."""
    M, C, N, oh = 130, 128, 64, 3
    g = O._gen("onehot", M, C, N)
    x = O._ints(g, (M, C), -1, 1)
    w, b = O._ints(g, (oh + C, N), -2, 2, F32), O._ints(g, (N,), -2, 2, F32)
    dy = O._ints(g, (M, N), -2, 2)
    old_w, old_b = _old_values((oh + C, N), "ohw"), _old_values((N,), "ohb")
    xg, wg, bg = (_cu(t).requires_grad_(True) for t in (x, w, b))
    wg.grad, bg.grad = _cu(old_w).clone(), _cu(old_b).clone()
    y = ops.fused_linear_onehot(xg, wg, bg, ACT_RELU, oh)
    y.backward(_cu(dy))
    w64 = w.to(F64)
    z = x.to(F64) @ w64[oh:] + (b.to(F64) + w64[oh - 1])
    O.check_exact(y.detach().cpu(), torch.relu(z), "onehot y")
    dz = dy.to(F64) * (z > 0)
    O.check_exact(xg.grad.cpu(), dz @ w64[oh:].t(), "onehot dX")
    add = torch.cat([torch.zeros(oh - 1, N, dtype=F64), dz.sum(0)[None], x.to(F64).t() @ dz])
    O.check_exact(wg.grad.cpu(), old_w.to(F64) + add, "onehot dW")
    O.check_exact(bg.grad.cpu(), old_b.to(F64) + dz.sum(0), "onehot db")


# --------------------------------------------------------------------------
# dispatch coverage and the LDS guard
# --------------------------------------------------------------------------
def test_matrix_covers_every_default_path():
    """The matrix reaches exactly the paths a default environment can
    select, and a sweep of the selector finds no path outside that list."""
    ext = _ext()
    declared = set(ext.gemm_default_paths())
    assert O.matrix_path_keys() == declared
    seen = set()
    for M in (1, 100, 4096, 16384, 16385, 16512, 20480, 300000):
        for K in (8, 10, 32, 40, 64, 131, 256, 384):
            for N in (1, 2, 16, 17, 64, 70, 128, 256):
                seen.add(ext.gemm_path("fwd", M, K, N))
                seen.add(O.path_key(ext.gemm_path("tn", M, K, N)))
                seen.add(O.path_key(ext.gemm_path("tn", M, K, N, 2, True)))
                if K % 32 == 0:
                    for actin in (0, 1, 2):
                        seen.add(ext.gemm_path("bt", M, K, N, actin))
    assert seen == declared


def test_oversized_lds_request_is_refused_before_launch():
    """A shape whose B image cannot fit the device's LDS raises an error that
    names LDS; nothing is launched (K is chosen from the queried limit)."""
    ext = _ext()
    limit = ext.gemm_lds_limit()
    print(f"GEMM_LDS_LIMIT bytes={limit}")
    assert limit >= 64 * 1024
    K = (limit // 128 // 32 + 1) * 32   # B image alone: K * 128 bytes > limit
    x = torch.zeros(32, K, device=DEV, dtype=BF16)
    w = torch.zeros(K, 64, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError, match="LDS"):
        ext.gemm_bias_act(x, w, torch.zeros(64, device=DEV), 0)
    with pytest.raises(RuntimeError, match="LDS"):
        ext.gemm_bt(x, w.t().contiguous(), x, 0)
    Kv = limit // 32 + 8                # gemv caches W: K * 16 * 2 bytes > limit
    with pytest.raises(RuntimeError, match="LDS"):
        ext.gemm_bias_act(torch.zeros(4, Kv, device=DEV, dtype=BF16),
                          torch.zeros(Kv, 16, device=DEV, dtype=BF16),
                          torch.zeros(16, device=DEV), 0)
