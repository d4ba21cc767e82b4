"""Oracle for the GEMM kernel family (gcbfplus_amd/ops/hip/gemm.hip) and its
CPU self-tests.

Every op of the family is one canonical product ``out = act(A @ B + bias)``
with A (P, R), B (R, Q) and R the reduction length:

  fwd  gemm_bias_act : A = x (M, K),         B = w (K, N),         R = K
  bt   gemm_bt       : A = fold(dy, y) (M, Kred), B = W^T (Kred, Nout), R = Kred
  tn   gemm_tn*      : A = [x^T; 1] (K+1, M), B = gate * fold(dy, y) (M, N),
                       R = M; rows 0..K-1 of ``out`` are dW, row K is db

``fold`` is the upstream-activation backward the kernels fold into their
operand stage, dz = bf16(float(dy) * act'(float(y))).

Two comparators judge a kernel output against the float64 product:

* ``check_exact``: operands are small integers (x in {-1,0,1}; w, dy, bias in
  {-2..2}; gate in {0,1}; saved activations y in {0, +-0.5, +-0.75}, so
  act'(y) is in {0, 1, 0.75, 0.4375} and dy * act'(y) is exact in bf16).
  Every product and every partial sum, in any order, is then a multiple of
  1/16 below 2^20, hence exact in fp32, and a correct kernel reproduces the
  float64 reference bit for bit.
* ``check_bounded``: random operands; elementwise
  |y - ref| <= 4*(R+2)*2^-24 * (|A|@|B| + |bias|)   (fp32 accumulation, either
  rounding mode), plus 2^-8 * (|ref| + that) for a bf16 store (half an ulp of
  round-to-nearest) and 2^-20 for tanh.

The CPU tests below prove, at every shape and option of the GPU matrix
(tests/test_gemm_paths_gpu.py), that the generated inputs meet the
preconditions, that an fp32-accumulate / bf16-store emulation passes both
comparators, and that emulated kernel defects (a dropped reduction row, a
dropped 8-wide chunk, a zeroed output column, a slab counted twice, an
ignored gate, the wrong activation derivative, a write past the end of dW)
are rejected by both. A GPU failure can then not be blamed on the inputs
or on a comparator that cannot see.
"""
import zlib

import pytest
import torch

ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

# --------------------------------------------------------------------------
# the matrix: (expected gemm_path, M, K, N, bounded?)        [K = reduction for bt]
# --------------------------------------------------------------------------
FWD_CASES = [
    ("dot", 1, 8, 1, False), ("dot", 300, 10, 1, False), ("dot", 4097, 384, 1, True),
    ("gemv", 5, 10, 2, False), ("gemv", 1030, 256, 4, True), ("gemv", 64, 131, 16, False),
    ("sm", 1, 32, 17, False), ("sm", 33, 64, 64, False), ("sm", 517, 384, 256, True),
    ("sm", 16384, 32, 72, False),
    ("pad->sm", 100, 10, 256, False), ("pad->sm", 70, 131, 128, False),
    ("pad->sm", 40, 260, 64, False),
    ("glds", 16512, 64, 64, False), ("glds", 16512, 256, 200, True),
    ("glds", 16512, 384, 64, False),           # 80 KiB dynamic LDS request
    ("base", 16421, 64, 64, False), ("base", 16421, 32, 40, True),
    ("base", 16385, 384, 129, False),
    ("base", 16512, 32, 64, False),            # aligned M, K % 64 != 0
    ("pad->glds", 16512, 40, 64, False), ("pad->base", 16421, 10, 64, False),
    # N % 8 != 0 with N > 16: W rows are not 16-byte aligned
    ("sm", 100, 64, 20, False), ("sm", 517, 32, 70, False),
    ("base", 16421, 32, 20, False), ("base", 16421, 64, 70, False),
]
# a glds shape with GCBF_GEMM_NOGLDS set takes the 128x64 kernel
FWD_NOGLDS_CASE = ("base", 16512, 64, 64, False)

# (path, M, Kred, Nout, actins, actin that also runs the bounded comparator)
BT_CASES = [
    ("sm_bt", 777, 128, 64, (0, 1, 2), None),
    ("sm_bt", 130, 256, 10, (0, 1, 2), None),   # ragged Nout: dX of a K = 10 layer
    ("sm_bt", 16384, 32, 131, (0, 1, 2), None),
    ("glds_bt", 16512, 64, 64, (0,), None),
    ("glds_bt", 16512, 256, 384, (0,), 0),
    ("base_bt", 16512, 128, 64, (1, 2), 1),
    ("base_bt", 16421, 64, 100, (0,), None),
    ("base_bt", 16421, 32, 260, (1,), None),
]

# (variant, remap, M, K, N, bounded?)
TN_CASES = [
    ("tn1", 0, 100, 64, 64, False), ("tn1", 0, 777, 128, 256, True),
    ("tn1", 0, 129, 10, 1, False), ("tn1", 0, 300, 131, 2, False),
    ("tn1", 0, 513, 260, 4, False), ("tn1", 0, 640, 70, 20, False),
    ("tn1", 1, 4096, 64, 128, False), ("tn1", 1, 4099, 10, 256, False),
    ("tn1", 1, 16383, 256, 1, False), ("tn1", 1, 8200, 384, 64, False),
    ("tn3", 1, 16384, 64, 64, False), ("tn3", 1, 16421, 128, 256, True),
    ("tn3", 1, 16421, 10, 256, False), ("tn3", 1, 16385, 256, 1, False),
    ("tn3", 1, 16421, 131, 2, False), ("tn3", 1, 20480, 64, 128, False),
    ("tn3", 1, 16421, 70, 20, False),
]
GATES = ("none", "half", "allfalse", "alltrue")
ACT_BWD_CASES = [(100, 48), (16421, 24)]


def tn_split(M, K, N):
    """Mirror of the dW launcher's split-M geometry for variants 1 and 3
    (64x64 tiles): (S, remap). The GPU tests assert it against gemm_path."""
    gk, gn = (K + 63) // 64, (N + 63) // 64
    S = min(128, max(1, 1024 // (gk * gn)))
    S = min(S, max(1, (M + 127) // 128))
    remap = S >= 8
    if remap:
        S = (S + 7) // 8 * 8
    return S, remap


def tn_path(variant, M, K, N):
    S, remap = tn_split(M, K, N)
    return f"{variant} S={S} remap={int(remap)}"


def path_key(path):
    """gemm_path string with the dW slab count left out."""
    return " ".join(t for t in path.split(" ") if not t.startswith("S="))


def matrix_path_keys():
    keys = {c[0] for c in FWD_CASES} | {c[0] for c in BT_CASES}
    keys |= {path_key(tn_path(v, M, K, N)) for v, _, M, K, N, _ in TN_CASES}
    return keys


# --------------------------------------------------------------------------
# case generation (CPU tensors in the dtypes the kernels take)
# --------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _ints(g, shape, lo, hi, dtype=BF16):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


_YVALS = torch.tensor([0.0, 0.5, -0.5, 0.75, -0.75])


def _operand(g, shape, kind, amp, scale, dtype=BF16):
    if kind == "int":
        return _ints(g, shape, -amp, amp, dtype)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _saved_act(g, shape, kind, actin):
    """A saved activation y for the fold; with actin == 0 the kernels never
    read it (the callers pass dy itself)."""
    if kind == "int":
        return _YVALS[torch.randint(0, 5, shape, generator=g)].to(BF16)
    y = torch.tanh(torch.randn(shape, generator=g))
    if actin == ACT_RELU:
        y = torch.relu(y)
    return y.to(BF16)


def _gate(g, M, gate):
    if gate == "none":
        return None
    if gate == "allfalse":
        return torch.zeros(M, dtype=torch.bool)
    if gate == "alltrue":
        return torch.ones(M, dtype=torch.bool)
    return torch.rand(M, generator=g) < 0.5


def fold(dy, y, actin):
    """dz = bf16(float(dy) * act'(float(y))) in the kernels' own fp32 ops
    (y*y is exact in fp32, so a fused multiply-add changes nothing)."""
    if actin == ACT_NONE:
        return dy
    yf = y.to(F32)
    grad = (yf > 0).to(F32) if actin == ACT_RELU else 1.0 - yf * yf
    return (dy.to(F32) * grad).to(BF16)


def make_fwd(M, K, N, kind, salt=0):
    g = _gen("fwd", M, K, N, kind, salt)
    return dict(op="fwd", kind=kind, M=M, K=K, N=N,
                x=_operand(g, (M, K), kind, 1, 0.5),
                w=_operand(g, (K, N), kind, 2, 0.2),
                bias=_operand(g, (N,), kind, 2, 0.1, F32))


def make_bt(M, Kred, Nout, actin, kind, salt=0):
    g = _gen("bt", M, Kred, Nout, actin, kind, salt)
    return dict(op="bt", kind=kind, M=M, K=Kred, N=Nout, actin=actin,
                dy=_operand(g, (M, Kred), kind, 2, 0.5),
                y=_saved_act(g, (M, Kred), kind, actin),
                w=_operand(g, (Nout, Kred), kind, 2, 0.2))


def make_tn(M, K, N, actin, gate, kind, salt=0):
    g = _gen("tn", M, K, N, actin, gate, kind, salt)
    return dict(op="tn", kind=kind, M=M, K=K, N=N, actin=actin, gate_kind=gate,
                x=_operand(g, (M, K), kind, 1, 0.5),
                dy=_operand(g, (M, N), kind, 2, 0.5),
                y=_saved_act(g, (M, N), kind, actin),
                gate=_gate(g, M, gate))


def make_act_bwd(M, N, act, salt=0):
    g = _gen("act_bwd", M, N, act, salt)
    return dict(dy=_operand(g, (M, N), "rand", 0, 1.0), y=_saved_act(g, (M, N), "rand", act))


# --------------------------------------------------------------------------
# canonical form, references, comparators
# --------------------------------------------------------------------------
def canon(case, act=ACT_NONE, fold_as=None):
    """(A, B, bias, act, out_dtype, R) of ``out = act(A @ B + bias)`` in
    float64. ``fold_as`` overrides the folded activation (mutant use)."""
    op = case["op"]
    if op == "fwd":
        out_dtype = F32 if case["N"] <= 16 else BF16  # small-N heads come out in f32
        return (case["x"].to(F64), case["w"].to(F64), case["bias"].to(F64), act,
                out_dtype, case["K"])
    actin = case["actin"] if fold_as is None else fold_as
    dz = fold(case["dy"], case["y"], actin).to(F64)
    if op == "bt":
        return dz, case["w"].to(F64).t(), torch.zeros(case["N"], dtype=F64), ACT_NONE, BF16, case["K"]
    if case["gate"] is not None:
        dz = dz * case["gate"].to(F64)[:, None]
    A = torch.cat([case["x"].to(F64).t(), torch.ones(1, case["M"], dtype=F64)])
    S, _ = tn_split(case["M"], case["K"], case["N"])
    return A, dz, torch.zeros(case["N"], dtype=F64), ACT_NONE, F32, case["M"] + S


def apply_act(z, act):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_TANH:
        return torch.tanh(z)
    return z


def reference(case, act=ACT_NONE):
    A, B, bias, act, _, _ = canon(case, act)
    return apply_act(A @ B + bias, act)


def check_preconditions(case, act=ACT_NONE):
    """Integer cases: operands are multiples of 1/16 and any partial sum of
    any order stays below 2^20, i.e. below 2^24 in units of 1/16."""
    A, B, bias, _, _, _ = canon(case, act)
    for t in (A, B, bias):
        assert torch.equal(t * 16, (t * 16).round()), "operand is no multiple of 1/16"
    bound = A.shape[1] * A.abs().max() * B.abs().max() + bias.abs().max()
    assert bound < 2 ** 20, f"partial sums may reach {bound}"


def check_exact(out, ref, what=""):
    """Bit-for-bit against the float64 reference cast to the output dtype."""
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    if out.dtype == BF16:  # integers up to 256 are exact in bf16
        assert ref.abs().max() <= 256, f"{what}: |ref| = {ref.abs().max()} > 256"
    # the exact value is an fp32 number, so this cast is the kernel's own
    # single round-to-nearest-even store
    want = ref.to(F32).to(out.dtype)
    if not torch.equal(out, want):
        bad = (out != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {out.numel()} elements differ; first at "
                             f"{i}: got {out[i].item()}, want {want[i].item()}")


def check_bounded(out, A, B, bias, act, R, what=""):
    """Elementwise rounding bound; returns the worst |err| / limit."""
    z = A @ B + bias
    ref = apply_act(z, act)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    S = A.abs() @ B.abs() + bias.abs()
    limit = 4.0 * (R + 2) * 2.0 ** -24 * S
    if out.dtype == BF16:
        limit = limit + 2.0 ** -8 * (ref.abs() + limit)
    if act == ACT_TANH:
        limit = limit + 2.0 ** -20
    err = (out.to(F64) - ref).abs()
    assert torch.isfinite(out.to(F64)).all(), f"{what}: non-finite output"
    ratio = torch.where(limit > 0, err / limit.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    worst = ratio.max().item()
    if worst > 1.0:
        i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
        raise AssertionError(f"{what}: |err|/limit = {worst:.3g} at {i}: got "
                             f"{out[i].item()}, ref {ref[i].item()}, limit {limit[i].item():.3g}")
    return worst


def check_guarded(buf, lo, hi, sentinel, what=""):
    """The regions around buf[lo:hi] still hold the sentinel."""
    for name, g in (("before", buf[:lo]), ("after", buf[hi:])):
        if not torch.equal(g, torch.full_like(g, sentinel)):
            i = (g != sentinel).nonzero()[0].item()
            raise AssertionError(f"{what}: guard {name} the target overwritten at offset {i}")


# --------------------------------------------------------------------------
# fp32-accumulate / bf16-store emulation and its mutants (CPU only)
# --------------------------------------------------------------------------
def _last_contributing(A, B):
    live = (A != 0).any(0) & (B != 0).any(1)
    idx = live.nonzero()
    return None if idx.numel() == 0 else int(idx[-1])


def mutants_for(case, act=ACT_NONE):
    """Names of the defects that change this case's exact result."""
    A, B, *_ = canon(case, act)
    if _last_contributing(A, B) is None:  # e.g. an all-false gate: dW == 0
        names = []
    else:
        names = ["drop_last_row", "drop_last_8", "zero_last_col"]
        if case["op"] == "tn":
            names.append("slab_twice")
    if case["op"] == "tn" and case["gate"] is not None and not case["gate"].all():
        names.append("ignore_gate")
    if case["op"] != "fwd" and case["actin"] == ACT_TANH and names[:1] == ["drop_last_row"]:
        names.append("relu_for_tanh")
    if case["kind"] == "rand":
        R = canon(case, act)[5]
        S, _ = tn_split(case["M"], case["K"], case["N"])
        m_per = (case["M"] + S - 1) // S
        names = [n for n in names if bounded_can_see(n, R, m_per)]
    return names


def bounded_can_see(name, R, m_per=1):
    """Which defects the rounding bound can see at all. A defect that loses
    (or adds) d of R like-sized terms moves a sum by about d/R of
    S = |A|@|B|, and the bound allows 4*(R+2)*2^-24 * S: beyond R ~ 2048 *
    sqrt(d) a d-row defect hides inside the worst-case fp32 allowance (a
    slab of m_per random-sign rows counts as sqrt(m_per)). Only the exact
    comparator sees those, which is why every GPU case runs it; the bounded
    one is asked for the rest (factor 2 of margin)."""
    d = {"drop_last_row": 1, "ignore_gate": 1, "drop_last_8": 8,
         "slab_twice": m_per ** 0.5}.get(name)
    return d is None or d / R > 8.0 * (R + 2) * 2.0 ** -24


def emulate(case, act=ACT_NONE, mutant=None):
    """The kernel's arithmetic on the CPU: fp32 products and sums, act in
    fp32, one rounding to the output dtype. ``mutant`` injects a defect."""
    A, B, bias, act, out_dtype, _ = canon(
        case, act, fold_as=ACT_RELU if mutant == "relu_for_tanh" else None)
    A, B, bias = A.to(F32), B.to(F32), bias.to(F32)
    z = A @ B
    if mutant in ("drop_last_row", "drop_last_8"):
        r = _last_contributing(A, B)
        lo = r if mutant == "drop_last_row" else max(0, r - 7)
        z = z - A[:, lo:r + 1] @ B[lo:r + 1]
    elif mutant == "slab_twice":
        S, _ = tn_split(case["M"], case["K"], case["N"])
        m_per = (case["M"] + S - 1) // S
        s = max(i for i in range(S)  # last slab holding a contributing row
                if i * m_per < case["M"] and _last_contributing(
                    A[:, i * m_per:(i + 1) * m_per], B[i * m_per:(i + 1) * m_per]) is not None)
        z = z + A[:, s * m_per:(s + 1) * m_per] @ B[s * m_per:(s + 1) * m_per]
    elif mutant == "ignore_gate":
        dz = fold(case["dy"], case["y"], case["actin"]).to(F32)
        closed = (~case["gate"]) & (dz != 0).any(1)
        r = int(closed.nonzero()[0])
        z = z + A[:, r:r + 1] @ dz[r:r + 1]
    z = z + bias
    out = apply_act(z, act)
    if mutant == "zero_last_col":
        out = out.clone()
        out[:, -1] = 0
    return out.to(out_dtype)


def _rejected(case, act, name):
    A, B, bias, act_, _, R = canon(case, act)
    try:
        if case["kind"] == "int":
            check_exact(emulate(case, act, name), apply_act(A @ B + bias, act_), name)
        else:
            check_bounded(emulate(case, act, name), A, B, bias, act_, R, name)
    except AssertionError:
        return True
    return False


def settled(make, act=ACT_NONE):
    """``make(salt)`` -> case. A tiny shape can hide a defect by chance (a
    zero product, a relu that clips the one output it touches): take the
    first salt at which the comparator sees every mutant, so that the GPU
    run of the same inputs has the power the self-test claims."""
    for salt in range(64):
        case = make(salt)
        if case["M"] * case["K"] * case["N"] > 1 << 16:
            return case
        if all(_rejected(case, act, name) for name in mutants_for(case, act)):
            return case
    raise AssertionError("no salt makes every mutant visible")


def fwd_case(M, K, N, act, kind):
    return settled(lambda salt: make_fwd(M, K, N, kind, salt), act)


def bt_case(M, Kred, Nout, actin, kind):
    return settled(lambda salt: make_bt(M, Kred, Nout, actin, kind, salt))


def tn_case(M, K, N, actin, gate, kind):
    return settled(lambda salt: make_tn(M, K, N, actin, gate, kind, salt))


# --------------------------------------------------------------------------
# CPU self-tests
# --------------------------------------------------------------------------
def _fwd_params():
    for path, M, K, N, bounded in FWD_CASES:
        for act in (ACT_NONE, ACT_RELU):
            yield pytest.param(M, K, N, act, id=f"{path}-{M}x{K}x{N}-act{act}")


def _fwd_bounded_params():
    for path, M, K, N, bounded in FWD_CASES:
        if bounded:
            for act in (ACT_NONE, ACT_RELU, ACT_TANH):
                yield pytest.param(M, K, N, act, id=f"{path}-{M}x{K}x{N}-act{act}")


def _bt_params():
    for path, M, K, N, actins, _ in BT_CASES:
        for actin in actins:
            yield pytest.param(M, K, N, actin, id=f"{path}-{M}x{K}x{N}-actin{actin}")


def _tn_params():
    for variant, remap, M, K, N, _ in TN_CASES:
        for actin in (0, 1, 2):
            for gate in GATES:
                yield pytest.param(M, K, N, actin, gate,
                                   id=f"{variant}r{remap}-{M}x{K}x{N}-actin{actin}-{gate}")


def _self_test(make, act=ACT_NONE):
    """Preconditions + emulation + mutants for one matrix entry, with the
    integer operands (exact comparator) and the random ones (bounded)."""
    ci, cr = make("int"), make("rand")
    check_preconditions(ci, act)
    ref_i = reference(ci, act)
    check_exact(emulate(ci, act), ref_i, "emulation")
    A, B, bias, act_, _, R = canon(cr, act)
    assert check_bounded(emulate(cr, act), A, B, bias, act_, R, "emulation") <= 1.0
    seen = []
    for name in mutants_for(ci, act):
        with pytest.raises(AssertionError):
            check_exact(emulate(ci, act, name), ref_i, name)
        seen.append(name)
    for name in mutants_for(cr, act):
        with pytest.raises(AssertionError):
            check_bounded(emulate(cr, act, name), A, B, bias, act_, R, name)
    return seen


@pytest.mark.parametrize("M,K,N,act", list(_fwd_params()))
def test_oracle_fwd(M, K, N, act):
    seen = _self_test(lambda kind: fwd_case(M, K, N, act, kind), act)
    assert seen == ["drop_last_row", "drop_last_8", "zero_last_col"]


@pytest.mark.parametrize("M,K,N,act", list(_fwd_bounded_params()))
def test_oracle_fwd_bounded_emulation(M, K, N, act):
    """The random-operand cases the GPU matrix runs, tanh included."""
    cr = fwd_case(M, K, N, act, "rand")
    A, B, bias, act_, _, R = canon(cr, act)
    assert check_bounded(emulate(cr, act), A, B, bias, act_, R) <= 1.0
    for name in mutants_for(cr, act):
        with pytest.raises(AssertionError):
            check_bounded(emulate(cr, act, name), A, B, bias, act_, R, name)


@pytest.mark.parametrize("M,K,N,actin", list(_bt_params()))
def test_oracle_bt(M, K, N, actin):
    seen = _self_test(lambda kind: bt_case(M, K, N, actin, kind))
    assert ("relu_for_tanh" in seen) == (actin == ACT_TANH)
    assert seen[:3] == ["drop_last_row", "drop_last_8", "zero_last_col"]


@pytest.mark.parametrize("M,K,N,actin,gate", list(_tn_params()))
def test_oracle_tn(M, K, N, actin, gate):
    seen = _self_test(lambda kind: tn_case(M, K, N, actin, gate, kind))
    want = [] if gate == "allfalse" else ["drop_last_row", "drop_last_8", "zero_last_col",
                                          "slab_twice"]
    if gate in ("half", "allfalse"):
        want.append("ignore_gate")
    if actin == ACT_TANH and gate != "allfalse":  # all gated out: dW == 0 either way
        want.append("relu_for_tanh")
    assert seen == want


def test_oracle_tn_split_classes():
    """The matrix's split classes: S < 8 without the remap, S >= 8 with it."""
    for variant, remap, M, K, N, _ in TN_CASES:
        S, r = tn_split(M, K, N)
        assert r == bool(remap) and (S >= 8) == bool(remap) and (not r or S % 8 == 0), (M, K, N, S)
        assert (variant == "tn3") == (M >= 16384)


def test_oracle_guard_write_rejected():
    """A write one element past dW's end is rejected whatever the values."""
    case = make_tn(129, 10, 1, 0, "none", "int")
    ref = reference(case)
    pad, n = 16, ref.numel()
    buf = torch.full((pad + n + pad,), 12345.0)
    buf[pad:pad + n] = emulate(case).flatten()
    check_guarded(buf, pad, pad + n, 12345.0)
    check_exact(buf[pad:pad + n].view_as(ref), ref)
    for off in (pad + n, pad - 1, len(buf) - 1, 0):
        bad = buf.clone()
        bad[off] = 0.0
        with pytest.raises(AssertionError):
            check_guarded(bad, pad, pad + n, 12345.0)


def test_oracle_fold_values():
    """The integer fold operands: act'(y) in {0, 1, 0.75, 0.4375} and
    dy * act'(y) exactly representable in bf16."""
    dy = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0]).to(BF16).repeat_interleave(5)
    y = _YVALS.to(BF16).repeat(5)
    for actin in (ACT_RELU, ACT_TANH):
        dz = fold(dy, y, actin).to(F64)
        g = (y.to(F64) > 0).to(F64) if actin == ACT_RELU else 1 - y.to(F64) ** 2
        assert torch.equal(dz, dy.to(F64) * g)
    assert set((1 - _YVALS.double() ** 2).tolist()) == {1.0, 0.75, 0.4375}


def test_oracle_matrix_names_every_family():
    keys = matrix_path_keys()
    for k in ("dot", "gemv", "sm", "pad->sm", "glds", "base", "sm_bt", "glds_bt", "base_bt",
              "tn1 remap=0", "tn1 remap=1", "tn3 remap=1"):
        assert k in keys
