"""Kernel-level op surface for the MI355X build.

Every hot op has two backends:
  - CPU: plain PyTorch (fp32) — the numerics oracle and the no-GPU test path.
  - GPU (gfx950): hand-written HIP/CDNA4 kernels in gcbfplus_amd/ops/hip/,
    loaded as the in-tree extension ``gcbfplus_amd._C``.

On a CUDA/ROCm device these ops REQUIRE the extension: if it is missing we
raise instead of silently falling back to eager (per-project rule: the HIP
path must be the one that runs on GPU).

Op inventory (kernel numbering follows SURVEY.md §2.7):
  fused_linear        K3/K4: MFMA GEMM + bias + activation, with autograd
                      (backward: transposed-B dX, deterministic split-M dW,
                      upstream-activation fold, direct grad accumulation)
  deferred_dw         scope around backward(): the small-M dW/db of fused_linear
                      run as grouped launches at its exit (GCBF_NO_DEFER_DW=1:
                      immediate launches as outside the scope)
  masked_softmax_aggr K3/K4: per-receiver masked softmax + weighted message sum
  EdgeCompact         active edge slots of a mask as device index tensors; with
                      gather_rows / fork_rows / compact_softmax_aggr and the
                      m_dev row count of fused_linear the edge level of the
                      GCBF+ minibatch runs on active slots only
  edge_msg_in         K2/K15: fused layer-0 GNN input build (+ analytic bwd);
                      mode 0 state diff, 1 DubinsCar, 2 CrazyFlie (node pre-pass)
  node_msg_in         fused layer >= 1 GNN input (gnn_layers >= 2): edge columns of
                      the layer-0 input | sender agent / constant row | receiver
  crazyflie_edge_jac  dh/d(edge feats) -> dh_i/dx_j for the CrazyFlie QP labels
  raytrace_rect       K1: 2D LiDAR fan vs rectangle set (no grad)
  gcbf_plus_loss      K10: all GCBF+ hinge losses + metrics in one kernel pair
  di_loss_prep        K10 prologue: u_ref + action clamp + euler + [cur; next]
  crazyflie_loss_prep K10 prologue (CrazyFlie): u_ref + unclamped action + RK4 with
                      the low-level LQR + [cur; next]; dual-number backward
  dubins_loss_prep    K10 prologue (DubinsCar): PID u_ref + unclamped action + stop
                      freeze + euler + [cur; next]
  drone_loss_prep     K10 prologue (LinearDrone): clipped-error LQR u_ref + unclamped
                      action + euler of A x + B a + [cur; next]
  si_loss_prep        K10 prologue (SingleIntegrator): same with xdot = a, no state clip
  proxqp_solve        K11: batched dense QP (labels; no grad)
  (env_step.hip K5-K8 is launched via env._step_fused: di_env_step for
  DoubleIntegrator/DubinsCar, drone3d_step and crazyflie_step as part A with
  raytrace_sphere_graph as part B for LinearDrone/CrazyFlie; optimizer.hip
  K13 via ops.optim.FusedAdamW)
"""
from __future__ import annotations

import contextlib
import os
from typing import Optional

import torch
from torch import Tensor

_EXT = None
_EXT_ERR: Optional[str] = None
_ZBIAS = {}


def _zero_bias(n: int, device) -> "Tensor":
    key = (n, str(device))
    z = _ZBIAS.get(key)
    if z is None:
        z = _ZBIAS[key] = torch.zeros(n, device=device)
    return z

ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        from gcbfplus_amd import _C  # built in-tree by setup.py / __graft_entry__.build()

        _EXT = _C
    except ImportError as e:  # pragma: no cover
        _EXT_ERR = str(e)
    return _EXT


def hip_available() -> bool:
    return _load_ext() is not None


def _require_ext():
    ext = _load_ext()
    if ext is None:
        raise RuntimeError(
            "gcbfplus_amd._C HIP extension is required on GPU but could not be "
            f"imported: {_EXT_ERR}. Build it with `python setup.py build_ext --inplace` "
            "(or __graft_entry__.build())."
        )
    return ext


# Deferred dW (ops.deferred_dw): a plain module flag, not a thread-local,
# because backward of a device tensor runs on the autograd engine's thread.
_DEFER_DW = False


@contextlib.contextmanager
def deferred_dw(device=None):
    """Scope around a backward pass: the direct-accumulate dW/db calls of
    fused_linear / fused_linear_onehot are queued (``_C.gemm_tn_defer``) and
    run on exit as a few grouped launches (``_C.dw_flush``) instead of a
    partial and a reduce launch per layer; every gradient keeps its bits. An
    exception inside the scope discards the queue. No-op without the
    extension, for a CPU ``device``, with GCBF_NO_DEFER_DW set, and when
    nested."""
    global _DEFER_DW
    ext = _load_ext()
    on_cpu = (torch.device(device).type == "cpu" if device is not None
              else not torch.cuda.is_available())
    if ext is None or on_cpu or _DEFER_DW or os.environ.get("GCBF_NO_DEFER_DW"):
        yield
        return
    _DEFER_DW = True
    try:
        yield
    except BaseException:
        ext.dw_discard()
        raise
    else:
        ext.dw_flush()
    finally:
        _DEFER_DW = False


def _apply_act(y: Tensor, act: int) -> Tensor:
    if act == ACT_RELU:
        return torch.relu(y)
    if act == ACT_TANH:
        return torch.tanh(y)
    return y


# --------------------------------------------------------------------------
# fused_linear: y = act(x @ w + b)
# --------------------------------------------------------------------------
class _FusedLinearHIP(torch.autograd.Function):
    """GPU path. x: (M, K) bf16 (or f32, cast), w: (K, N) f32 master, b: (N,) f32.

    Forward runs the hand-written MFMA GEMM (bf16 in, f32 accumulate) with the
    bias+activation fused into the epilogue. Backward reuses the same GEMM for
    dx = dz @ w^T and a deterministic split-M reduction kernel for
    dw = x^T @ dz (+ db = colsum dz).
    """

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, b: Optional[Tensor], act: int,
                row_gate: Optional[Tensor] = None, m_dev: Optional[Tensor] = None,
                row_map: Optional[Tensor] = None):
        ext = _require_ext()
        x_bf = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
        # FusedAdamW maintains a bf16 shadow per param (p._bf, updated inside
        # the optimizer kernel) — skip the per-call cast when present
        w_bf = getattr(w, "_bf", None)
        if w_bf is None:
            w_bf = w.to(torch.bfloat16)
        bias = b if b is not None else _zero_bias(w.shape[1], w.device)
        y = ext.gemm_bias_act(x_bf.contiguous(), w_bf.contiguous(), bias.contiguous(), act,
                              m_dev)
        ctx.save_for_backward(x_bf, w_bf, y)
        ctx.act = act
        ctx.x_dtype = x.dtype
        ctx.has_bias = b is not None
        # device row count (edge compaction): every GEMM of this layer, forward
        # and backward, works on the rows below it only
        ctx.m_dev = m_dev
        # dW/db of an edge-compacted layer: summed over the dense slot rows in
        # the dense call's order (row_map = EdgeCompact.inv), so they keep the
        # dense path's bits; without it the live rows are summed as they lie
        ctx.row_map = row_map
        # direct-accumulate target: when w/b are leaf params whose .grad is a
        # live buffer (FusedAdamW flat-gradient views), backward writes dW/db
        # straight into it (+=) and returns None — skips the AccumulateGrad
        # add_ kernels (~28 per minibatch across the three networks)
        ctx.acc = None
        if (b is not None and w.is_leaf and b.is_leaf
                and w.grad is not None and b.grad is not None
                and w.grad.is_contiguous() and b.grad.is_contiguous()):
            ctx.acc = (w, b)
        # per-row dW/db stop-gradient mask (dX unaffected): GCBF+ unlabeled
        # h_dot rows — rows with gate=False contribute nothing to the params
        ctx.row_gate = row_gate
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        ext = _require_ext()
        x_bf, w_bf, y = ctx.saved_tensors
        if y.dtype == torch.float32:  # small-N f32 head output path
            if ctx.act == ACT_RELU:
                dz_f = dy * (y > 0)
            elif ctx.act == ACT_TANH:
                dz_f = dy * (1.0 - y * y)
            else:
                dz_f = dy
            dz = dz_f.to(torch.bfloat16).contiguous()
            actin, yact = ACT_NONE, dz
        else:
            # activation backward dz = dy * act'(y) is FOLDED into the two
            # consumer GEMMs' operand stages (same f32 math, same bf16
            # rounding as a materialized act_bwd pass)
            dz = dy.contiguous().to(torch.bfloat16)
            actin, yact = ctx.act, y
            if actin != ACT_NONE and dz.shape[1] % 32 != 0:
                dz = ext.act_bwd(dz, y, actin)  # rare: narrow activated layer
                actin, yact = ACT_NONE, dz
        dx = dw = db = None
        md = ctx.m_dev
        if ctx.needs_input_grad[0]:
            if dz.shape[1] % 32 == 0:
                # dx = dz @ w^T via the transposed B-stage kernel: no
                # materialized w^T copy per backward
                dx = ext.gemm_bt(dz, w_bf, yact, actin, md)
            else:
                # small-N heads: pad path with an explicit transpose (pads K
                # by a copy, so it runs over every row whatever m_dev says;
                # rows past the count hold garbage nobody reads)
                wt = w_bf.t().contiguous()
                dx = ext.gemm_bias_act(dz, wt, _zero_bias(wt.shape[1], wt.device), ACT_NONE)
            dx = dx.to(ctx.x_dtype)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            rg = ctx.row_gate
            rm = ctx.row_map
            if rm is not None:
                md = None
            if ctx.acc is not None:
                wp, bp = ctx.acc
                if _DEFER_DW:
                    ext.gemm_tn_defer(x_bf, dz, yact, actin, wp.grad, bp.grad, None, rg, md, rm)
                else:
                    ext.gemm_tn_acc(x_bf, dz, yact, actin, wp.grad, bp.grad, rg, md, rm)
            else:
                dw, db = ext.gemm_tn(x_bf, dz, yact, actin, rg, md, rm)  # f32 (K,N), (N,)
        if not ctx.has_bias:
            db = None
        return dx, dw, db, None, None, None, None


class _FusedLinearOneHotHIP(torch.autograd.Function):
    """y = act(x @ w[oh:] + (b + w[oh-1])) for the agents-only GNN update
    layer whose first `oh` input features are the constant agent one-hot
    [0,0,1]. Replaces the eager `w[3:]` slice + `b + w[2]` add whose autograd
    backward costs ~10 small kernels per call (zeros-pad of the sliced dW,
    scatter, AccumulateGrad adds): here dW accumulates straight into
    w.grad[oh:] and db into BOTH b.grad and w.grad[oh-1] inside the dW
    reduction (gemm_tn_acc2)."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, b: Tensor, act: int, oh: int,
                row_gate: Optional[Tensor] = None):
        ext = _require_ext()
        x_bf = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
        w_bf = getattr(w, "_bf", None)
        if w_bf is None:
            w_bf = w.to(torch.bfloat16)
        w_bf3 = w_bf[oh:].contiguous() if not w_bf[oh:].is_contiguous() else w_bf[oh:]
        bias_eff = b + w[oh - 1]
        y = ext.gemm_bias_act(x_bf.contiguous(), w_bf3, bias_eff.contiguous(), act)
        ctx.save_for_backward(x_bf, w_bf3, y)
        ctx.act = act
        ctx.oh = oh
        ctx.x_dtype = x.dtype
        ctx.direct = (w.is_leaf and b.is_leaf and w.grad is not None
                      and b.grad is not None and w.grad.is_contiguous()
                      and b.grad.is_contiguous())
        ctx.params = (w, b) if ctx.direct else None
        ctx.row_gate = row_gate
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        ext = _require_ext()
        x_bf, w_bf3, y = ctx.saved_tensors
        oh = ctx.oh
        if y.dtype == torch.float32:
            if ctx.act == ACT_RELU:
                dz_f = dy * (y > 0)
            elif ctx.act == ACT_TANH:
                dz_f = dy * (1.0 - y * y)
            else:
                dz_f = dy
            dz = dz_f.to(torch.bfloat16).contiguous()
            actin, yact = ACT_NONE, dz
        else:
            dz = dy.contiguous().to(torch.bfloat16)
            actin, yact = ctx.act, y
            if actin != ACT_NONE and dz.shape[1] % 32 != 0:
                dz = ext.act_bwd(dz, y, actin)
                actin, yact = ACT_NONE, dz
        dx = dw_full = db_out = None
        if ctx.needs_input_grad[0]:
            dx = ext.gemm_bt(dz, w_bf3, yact, actin).to(ctx.x_dtype)
        if ctx.direct:
            w, b = ctx.params
            if _DEFER_DW:
                ext.gemm_tn_defer(x_bf, dz, yact, actin, w.grad[oh:], b.grad,
                                  w.grad[oh - 1], ctx.row_gate)
            else:
                ext.gemm_tn_acc2(x_bf, dz, yact, actin, w.grad[oh:], b.grad,
                                 w.grad[oh - 1], ctx.row_gate)
        else:
            dw, db = ext.gemm_tn(x_bf, dz, yact, actin, ctx.row_gate)
            dw_full = torch.zeros(oh + dw.shape[0], dw.shape[1],
                                  device=dw.device, dtype=dw.dtype)
            dw_full[oh:] = dw
            dw_full[oh - 1] = db
            db_out = db
        return dx, dw_full, db_out, None, None, None


def fused_linear_onehot(x: Tensor, w: Tensor, b: Tensor, act: int, oh: int = 3,
                        row_gate: Optional[Tensor] = None) -> Tensor:
    """GPU-only one-hot fold (see _FusedLinearOneHotHIP). Callers fall back
    to fused_linear(x, w[oh:], b + w[oh-1], act) on CPU."""
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    y = _FusedLinearOneHotHIP.apply(x2, w, b, act, oh, row_gate)
    return y.reshape(*lead, w.shape[1])


def fused_linear(x: Tensor, w: Tensor, b: Optional[Tensor], act: int = ACT_NONE,
                 row_gate: Optional[Tensor] = None, m_dev: Optional[Tensor] = None,
                 row_map: Optional[Tensor] = None) -> Tensor:
    """act(x @ w + b). x: (..., K); w: (K, N) fp32 master weight; b: (N,) fp32.

    GPU: bf16 MFMA kernel. CPU: fp32 torch (autograd oracle).
    row_gate (flat rows,) bool: rows with False contribute nothing to dW/db
    (dX unaffected) — per-sample parameter stop-gradient.
    m_dev: one int32 on the GPU, the live row count of an edge-compacted call
    (``EdgeCompact.m_pad``): rows at or past it are neither computed nor
    written, forward or backward, and take no part in dW/db. GPU only.
    row_map (``EdgeCompact.inv``, with m_dev): dW/db are summed over the dense
    slot rows in the dense call's order, reading row row_map[m] of the compact
    operands (zero where it is -1): the dense path's bits.
    """
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if x2.shape[-1] != w.shape[0]:
        if x2.shape[-1] < w.shape[0]:
            # weight padded at init (Dense pad_to) but input unpadded (eager
            # CPU edge path): the dropped rows are zero, so slicing is exact
            w = w.narrow(0, 0, x2.shape[-1])
        else:
            # zero-padded input (fused edge_msg_in emits K padded to 32): pad
            # W rows to match — zeros x zeros contribute nothing, and autograd
            # slices dW back to the master shape
            w = torch.cat([w, w.new_zeros(x2.shape[-1] - w.shape[0], w.shape[1])], dim=0)
    if x2.is_cuda:
        y = _FusedLinearHIP.apply(x2, w, b, act, row_gate, m_dev, row_map)
    else:
        assert row_gate is None, "row_gate is a GPU-path feature"
        assert m_dev is None, "m_dev is a GPU-path feature"
        y = torch.addmm(b, x2, w) if b is not None else x2 @ w
        y = _apply_act(y, act)
    return y.reshape(*lead, w.shape[1])


# --------------------------------------------------------------------------
# masked_softmax_aggr: attention aggregate over the dense edge-slot axis
# --------------------------------------------------------------------------
class _SoftmaxAggrHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate: Tensor, msg: Tensor, mask: Tensor):
        ext = _require_ext()
        gate_f = gate.to(torch.float32).contiguous()
        msg_bf = msg.to(torch.bfloat16).contiguous()
        aggr, attn = ext.softmax_aggr_fwd(gate_f, msg_bf, mask.contiguous())
        ctx.save_for_backward(attn, msg_bf, mask)
        ctx.gate_dtype = gate.dtype
        ctx.msg_dtype = msg.dtype
        return aggr

    @staticmethod
    def backward(ctx, daggr: Tensor):
        ext = _require_ext()
        attn, msg_bf, mask = ctx.saved_tensors
        dgate, dmsg = ext.softmax_aggr_bwd(
            daggr.to(torch.bfloat16).contiguous(), attn, msg_bf, mask
        )
        return dgate.to(ctx.gate_dtype), dmsg.to(ctx.msg_dtype), None


def masked_softmax_aggr(gate: Tensor, msg: Tensor, mask: Tensor) -> Tensor:
    """Per-receiver attention aggregation (dense replacement for the
    reference's jraph.segment_softmax + segment_sum, nn/gnn.py:65-72).

    gate: (B, N, D) raw attention logits
    msg:  (B, N, D, C) messages
    mask: (B, N, D) bool; masked slots get zero attention.
    Returns aggr: (B, N, C) = sum_d softmax_d(gate | mask) * msg.
    Rows with no active slot return zeros.
    """
    if gate.is_cuda:
        return _SoftmaxAggrHIP.apply(gate, msg, mask)
    neg = torch.finfo(gate.dtype).min
    g = torch.where(mask, gate, torch.full_like(gate, neg))
    # numerically-stable masked softmax; all-masked rows -> zeros
    gmax = g.max(dim=-1, keepdim=True).values
    e = torch.exp(g - gmax) * mask.to(gate.dtype)
    denom = e.sum(dim=-1, keepdim=True).clamp_min(1e-20)
    attn = e / denom
    return torch.einsum("bnd,bndc->bnc", attn.to(msg.dtype), msg)


# --------------------------------------------------------------------------
# edge compaction: the edge-level GNN kernels on the active slots only
# --------------------------------------------------------------------------
# slot rows up to this take gemm_plan's small-M kernels, where the dense edge
# level already sits at the launch floor (bindings.hip gemm_plan: M <= 16384)
EDGE_COMPACT_MIN_ROWS = 16384


def edge_compact_wanted(n_slot_rows: int) -> bool:
    """Shape-only default for the compact edge path (GPU, fused single-layer
    GNN input): on above the small-M limit. GCBF_NO_EDGE_COMPACT=1 keeps the
    dense path, GCBF_FORCE_EDGE_COMPACT=1 compacts at any size."""
    if os.environ.get("GCBF_NO_EDGE_COMPACT"):
        return False
    if os.environ.get("GCBF_FORCE_EDGE_COMPACT"):
        return True
    return n_slot_rows > EDGE_COMPACT_MIN_ROWS


class EdgeCompact:
    """Active edge slots of a (B, N, D) bool mask as device index tensors
    (``_C.edge_compact``; nothing is read on the host, so it can be built and
    used inside a stream capture):

      rows (cap,)   flat slot index of compact row j < count, ascending
      inv (B*N*D,)  compact row of a slot, -1 if masked
      off (B*N+1,)  exclusive prefix of the per-receiver active counts
      cnt (2,)      [count, count rounded up to 128]
      gate_c (cap,) row_gate[receiver] per compact row (when a gate is given)

    cap = B*N*D rounded up to 128 is the row capacity of every compact tensor.
    ``m_pad`` (= cnt[1:2]) is the ``m_dev`` of the GEMM family. ``prefix(n)``
    is the view for the first n receivers: the same rows, because they ascend
    (GCBF+ runs the actor on g and the CBF on [g; next_g] with one mask)."""

    def __init__(self, rows, inv, off, cnt, gate_c, n_recv: int, D: int):
        self.rows, self.inv, self.off, self.cnt, self.gate_c = rows, inv, off, cnt, gate_c
        self.n_recv, self.D = n_recv, D
        self.n_slots = n_recv * D
        self.cap = (self.n_slots + 127) // 128 * 128
        self.m_pad = cnt[1:2]
        self._prefix = None

    @classmethod
    def build(cls, mask: Tensor, row_gate: Optional[Tensor] = None,
              prefix_recv: Optional[int] = None) -> "EdgeCompact":
        ext = _require_ext()
        D = mask.shape[-1]
        n_recv = mask.numel() // D
        gate = None if row_gate is None else row_gate.reshape(-1).contiguous()
        out = ext.edge_compact(mask.contiguous(), 128,
                               n_recv if prefix_recv is None else prefix_recv, gate)
        rows, inv, off, cnt4 = out[:4]
        c = cls(rows, inv, off, cnt4[0:2], out[4] if gate is not None else None, n_recv, D)
        if prefix_recv is not None:
            c._prefix = cls(rows, inv[: prefix_recv * D], off[: prefix_recv + 1], cnt4[2:4], None,
                            prefix_recv, D)
        return c

    def prefix(self) -> "EdgeCompact":
        assert self._prefix is not None, "built without prefix_recv"
        return self._prefix


class _GatherRowsHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X: Tensor, ec: EdgeCompact):
        ext = _require_ext()
        ctx.ec = ec
        ctx.M = X.shape[0]
        return ext.gather_rows(X.contiguous(), ec.rows, ec.cnt, ec.cap)

    @staticmethod
    def backward(ctx, dXc: Tensor):
        ext = _require_ext()
        return ext.gather_rows_bwd(dXc.contiguous(), ctx.ec.inv, ctx.M), None


def gather_rows(X: Tensor, ec: EdgeCompact) -> Tensor:
    """(B*N*D, K) dense slot rows -> (cap, K) compact rows: row j < count is
    X[rows[j]] bit for bit, rows [count, count_pad) are zeros, later rows are
    left unwritten. Backward scatters back (zeros in masked slots). GPU only."""
    assert X.dim() == 2 and X.shape[0] == ec.n_slots
    return _GatherRowsHIP.apply(X, ec)


class _ForkAddHIP(torch.autograd.Function):
    """x -> (x, x) for a compact bf16 tensor with two consumers: the backward
    adds the two gradients over the live rows only (``_C.add_rows_bf16``,
    the rounding of the eager add autograd would run over the whole capacity)."""

    @staticmethod
    def forward(ctx, x: Tensor, ec: EdgeCompact):
        ctx.ec = ec
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, d1: Tensor, d2: Tensor):
        ext = _require_ext()
        return ext.add_rows_bf16(d1.contiguous(), d2.contiguous(), ctx.ec.cnt), None


def fork_rows(x: Tensor, ec: EdgeCompact):
    return _ForkAddHIP.apply(x, ec)


class _SoftmaxAggrCompactHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate_c: Tensor, msg_c: Tensor, ec: EdgeCompact):
        ext = _require_ext()
        aggr, attn_c = ext.softmax_aggr_c_fwd(gate_c.contiguous(), msg_c.contiguous(),
                                              ec.off, ec.inv, ec.D)
        ctx.save_for_backward(attn_c, msg_c)
        ctx.ec = ec
        return aggr

    @staticmethod
    def backward(ctx, daggr: Tensor):
        ext = _require_ext()
        attn_c, msg_c = ctx.saved_tensors
        ec = ctx.ec
        dgate_c, dmsg_c = ext.softmax_aggr_c_bwd(
            daggr.to(torch.bfloat16).contiguous(), attn_c, msg_c, ec.off, ec.rows, ec.cnt, ec.D)
        return dgate_c, dmsg_c, None


def compact_softmax_aggr(gate_c: Tensor, msg_c: Tensor, ec: EdgeCompact) -> Tensor:
    """``masked_softmax_aggr`` on compact rows: gate_c (cap,) f32 and msg_c
    (cap, C) bf16 -> aggr (B*N, C), bit-equal to the dense kernel on the
    scattered inputs. The backward zeroes the gradients of the padding rows
    [count, count_pad), which keeps them out of every dW upstream. GPU only."""
    assert gate_c.dtype == torch.float32 and msg_c.dtype == torch.bfloat16
    return _SoftmaxAggrCompactHIP.apply(gate_c, msg_c, ec)


# --------------------------------------------------------------------------
# edge_msg_in: fused first-layer GNN input (K2/K15)
# --------------------------------------------------------------------------
class _EdgeMsgInHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, states: Tensor, n_agents: int, n_rays: int, pos_dim: int,
                k_pad: int, comm: float, mode: int):
        ext = _require_ext()
        st = states.contiguous()
        X = ext.edge_msg_in_fwd(st, n_agents, n_rays, pos_dim, k_pad, comm, mode)
        ctx.save_for_backward(st)
        ctx.meta = (n_agents, n_rays, pos_dim, comm, mode)
        return X

    @staticmethod
    def backward(ctx, dX: Tensor):
        ext = _require_ext()
        (st,) = ctx.saved_tensors
        n, r, pdim, comm, mode = ctx.meta
        dstates = ext.edge_msg_in_bwd(st, dX.contiguous().to(torch.bfloat16), n, r,
                                      pdim, comm, mode)
        return dstates, None, None, None, None, None, None


def crazyflie_rotmat(phi: Tensor, theta: Tensor, psi: Tensor) -> Tensor:
    """(...,) angles -> (..., 3, 3) body->world rotation (reference
    env/crazyflie.py:19-33). Lives here, not in env/crazyflie.py (which
    re-exports it as ``rotmat``), because env imports ops."""
    c_phi, s_phi = torch.cos(phi), torch.sin(phi)
    c_th, s_th = torch.cos(theta), torch.sin(theta)
    c_psi, s_psi = torch.cos(psi), torch.sin(psi)
    rows = [
        torch.stack([c_psi * c_th, c_psi * s_th * s_phi - s_psi * c_phi,
                     c_psi * s_th * c_phi + s_psi * s_phi], dim=-1),
        torch.stack([s_psi * c_th, s_psi * s_th * s_phi + c_psi * c_phi,
                     s_psi * s_th * c_phi - c_psi * s_phi], dim=-1),
        torch.stack([-s_th, c_th * s_phi, c_th * c_phi], dim=-1),
    ]
    return torch.stack(rows, dim=-2)


def crazyflie_edge_states(states: Tensor) -> Tensor:
    """12-dim world-frame edge state [pos, vel_W, z-axis_W, omega_W] of
    (..., 12) states (x,y,z, psi,theta,phi, u,v,w, r,q,p) (reference
    edge_state, env/crazyflie.py:165-182): the torch definition behind
    ``CrazyFlie._edge_states`` and the CPU path of ``edge_msg_in`` mode 2."""
    Rm = crazyflie_rotmat(states[..., 5], states[..., 4], states[..., 3])
    v_W = torch.einsum("...ij,...j->...i", Rm, states[..., 6:9])
    z_W = Rm[..., :, 2]
    omega_W = torch.einsum("...ij,...j->...i", Rm, states[..., 9:12].flip(-1))
    return torch.cat([states[..., :3], v_W, z_W, omega_W], dim=-1)


def edge_msg_in(states: Tensor, n_agents: int, n_rays: int, pos_dim: int,
                comm: float, k_pad: Optional[int] = None, mode: int = 0) -> Tensor:
    """Fused layer-0 GNN input: per edge slot
    [clip(es_recv - es_send) | sender one-hot | recv one-hot | 0 pad],
    (B, N, D, KP), where es is the edge state of a node:

      mode 0  es = state (SI/DI/LinearDrone; reference
              double_integrator.py:275-286 + one-hot node feats :288-295)
      mode 1  DubinsCar [x, y, v cos(theta), v sin(theta)]
      mode 2  CrazyFlie [pos, R uvw, R[:, 2], R pqr] on every node (S = 12,
              pos_dim = 3, KP = 32); the trigonometry runs once per node in a
              pre-pass, forward and backward

    GPU: bf16 kernel pair (the extension refuses any other mode, and shapes
    mode 2 does not cover); CPU: composed fp32 torch, differentiable.
    """
    B, V, S = states.shape
    K = S + 6
    if k_pad is None:
        k_pad = (K + 31) // 32 * 32
    if states.is_cuda:
        return _EdgeMsgInHIP.apply(states, n_agents, n_rays, pos_dim, k_pad, comm, mode)
    if mode not in (0, 1, 2):
        raise ValueError(f"edge_msg_in: unknown mode {mode}")
    # CPU compose (fp32)
    if mode == 1:  # DubinsCar edge-state transform [x, y, v cos, v sin]
        th, v = states[..., 2], states[..., 3]
        states = torch.stack(
            [states[..., 0], states[..., 1], v * torch.cos(th), v * torch.sin(th)], dim=-1
        )
    elif mode == 2:
        if S != 12 or pos_dim != 3:
            raise ValueError("edge_msg_in mode 2 needs S == 12 and pos_dim == 3")
        states = crazyflie_edge_states(states)
    n, r = n_agents, n_rays
    recv = states[:, :n, None, :]
    senders = torch.cat(
        [
            states[:, None, :n].expand(B, n, n, S),
            states[:, n : 2 * n, None, :],
            states[:, 2 * n :].reshape(B, n, r, S),
        ],
        dim=2,
    )
    e = recv - senders
    pos = e[..., :pos_dim]
    nrm = torch.sqrt(1e-6 + (pos * pos).sum(-1, keepdim=True))
    coef = torch.where(nrm > comm, comm / torch.clamp(nrm, min=comm), torch.ones_like(nrm))
    e = torch.cat([pos * coef, e[..., pos_dim:]], dim=-1)
    D = n + 1 + r
    oh = torch.zeros(n, D, 6, dtype=states.dtype, device=states.device)
    oh[:, :n, 2] = 1.0  # agent senders: 001
    oh[:, n, 1] = 1.0  # goal: 010
    oh[:, n + 1 :, 0] = 1.0  # obs: 100
    oh[:, :, 5] = 1.0  # receiver is always an agent: 001
    out = torch.cat([e, oh[None].expand(B, n, D, 6)], dim=-1)
    if k_pad > K:
        out = torch.cat([out, out.new_zeros(B, n, D, k_pad - K)], dim=-1)
    return out


# --------------------------------------------------------------------------
# node_msg_in: fused GNN input of layer >= 1 (deep path, gnn_layers >= 2)
# --------------------------------------------------------------------------
class _NodeMsgInHIP(torch.autograd.Function):
    """Operands go to the extension as they are: it refuses a wrong dtype or
    layout instead of converting it on the quiet."""

    @staticmethod
    def forward(ctx, X0: Tensor, xa: Tensor, c: Tensor, E: int, n_rays: int, k_pad: int):
        ext = _require_ext()
        X1 = ext.node_msg_in_fwd(X0, xa, c, E, n_rays, k_pad)
        ctx.meta = (E, xa.shape[-1], n_rays, X0.shape[-1])
        return X1

    @staticmethod
    def backward(ctx, dX1: Tensor):
        ext = _require_ext()
        E, F, n_rays, kp0 = ctx.meta
        dX0, dxa, dc = ext.node_msg_in_bwd(dX1.contiguous().to(torch.bfloat16), E, F,
                                           n_rays, kp0)
        # xa is bf16: its gradient takes the input's dtype, as autograd requires
        return dX0, dxa.to(torch.bfloat16), dc, None, None, None


def node_msg_in(X0: Tensor, xa: Tensor, c: Tensor, E: int,
                n_rays: Optional[int] = None, k_pad: Optional[int] = None) -> Tensor:
    """Fused input of GNN layer >= 1 on the deep path: per edge slot (b, i, d)
    [X0[b,i,d,:E] | s | xa[b,i] | 0 pad], (B, N, D, KP1), KP1 = ceil32(E + 2F);
    s = xa[b,d] for d < N (sender is agent d), c[0] for d == N (the goal node)
    and c[1] for d > N (a lidar hit node). Goal and hit nodes never receive a
    message, so their features are the two constant rows c (2, F).

    X0 (B, N, D, KP0) is the layer-0 input of ``edge_msg_in`` (its first E
    columns are the edge features in every mode); xa (B, N, F) the previous
    layer's agent features. ``n_rays`` defaults to D - N - 1.

    GPU: bf16 HIP kernel pair, X0/xa bf16 and c f32 (anything else is refused
    before a launch); the backward sums in a fixed order without atomics.
    CPU: composed torch in X0's dtype, differentiable.
    """
    B, N, D, _ = X0.shape
    F = xa.shape[-1]
    if n_rays is None:
        n_rays = D - N - 1
    if k_pad is None:
        k_pad = (E + 2 * F + 31) // 32 * 32
    if X0.is_cuda:
        return _NodeMsgInHIP.apply(X0, xa, c, E, n_rays, k_pad)
    if D != N + 1 + n_rays or n_rays < 0:
        raise ValueError(f"node_msg_in: D = {D} is not N + 1 + R for N = {N}, R = {n_rays}")
    if not E + 2 * F <= k_pad < E + 2 * F + 32:
        raise ValueError(f"node_msg_in: k_pad = {k_pad} does not fit E + 2F = {E + 2 * F}")
    xa = xa.to(X0.dtype)
    c = c.to(X0.dtype)
    sender = torch.cat(
        [
            xa[:, None, :, :].expand(B, N, N, F),
            c[0].expand(B, N, 1, F),
            c[1].expand(B, N, n_rays, F),
        ],
        dim=2,
    )
    recv = xa[:, :, None, :].expand(B, N, D, F)
    parts = [X0[..., :E], sender, recv]
    if k_pad > E + 2 * F:
        parts.append(X0.new_zeros(B, N, D, k_pad - E - 2 * F))
    return torch.cat(parts, dim=-1)


def crazyflie_edge_jac(states: Tensor, ge: Tensor, n_agents: int, n_rays: int,
                       comm: float) -> Tensor:
    """Fused ``CrazyFlie.edge_grad_to_state_jac``: states (M, V, 12) and
    ge (M, N, D, 12) f32 = dh/d(edge feats) -> h_x (M, N, N, 12) = dh_i/dx_j
    (clip vjp per slot, receiver-side sum on the diagonal, transposed
    edge-state jacobian of agent j). GPU only (node pre-pass + one kernel, no
    grad); CPU callers take the torch body in env/crazyflie.py."""
    if not states.is_cuda:
        raise NotImplementedError("CPU path is CrazyFlie.edge_grad_to_state_jac's torch body")
    return _require_ext().crazyflie_edge_jac(
        states.detach().contiguous(), ge.detach().float().contiguous(), n_agents, n_rays, comm)


# --------------------------------------------------------------------------
# raytrace (K1) — no autograd
# --------------------------------------------------------------------------
def raytrace_rect(pos: Tensor, points: Tensor, n_rays: int, sense_range: float) -> Tensor:
    """2D LiDAR fan: pos (B,N,2) origins, points (B,K,4,2) rectangle corners.
    Returns hits (B,N,R,2). GPU: HIP kernel; CPU: composed torch (obstacle.py)."""
    ext = _load_ext()
    if pos.is_cuda:
        _require_ext()
        return _EXT.raytrace_rect(pos.contiguous(), points.contiguous(), n_rays, sense_range)
    raise NotImplementedError("CPU path goes through env.get_lidar composition")


def raytrace_sphere_topk(pos: Tensor, centers: Tensor, radii: Tensor, n_beams: int,
                         topk: int, sense_range: float) -> Tensor:
    """3D LiDAR theta x phi fan + poles vs spheres, fused with stable top-k
    closest-hit selection (reference env/utils.py:49-79 + obstacle.py:237-270
    + the argsort top-k of utils.py:127-131). pos (B,N,3), centers (B,K,3),
    radii (B,K) -> hits (B,N,topk,3). GPU only (no grad)."""
    if pos.is_cuda:
        _require_ext()
        return _EXT.raytrace_sphere_topk(pos.contiguous(), centers.contiguous(),
                                         radii.contiguous(), n_beams, topk, sense_range)
    raise NotImplementedError("CPU path goes through env.get_lidar composition")


# --------------------------------------------------------------------------
# fused GCBF+ loss (K10)
# --------------------------------------------------------------------------
class _GCBFLossHIP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, h_next, h_ng, action, u_qp, safe, unsafe, params):
        ext = _require_ext()
        dt, alpha, eps, c_act, c_unsafe, c_safe, c_hdot = params
        args = [t.contiguous() for t in (h, h_next, h_ng, action, u_qp)]
        out = ext.gcbf_loss_fwd(*args, safe.contiguous(), unsafe.contiguous(),
                                dt, alpha, eps, c_act, c_unsafe, c_safe, c_hdot)
        ctx.save_for_backward(*args, safe, unsafe, out)
        ctx.params = params
        parts = out[1:9]
        ctx.mark_non_differentiable(parts)
        return out[0], parts

    @staticmethod
    def backward(ctx, d_total, _d_parts):
        ext = _require_ext()
        h, h_next, h_ng, action, u_qp, safe, unsafe, out = ctx.saved_tensors
        dt, alpha, eps, c_act, c_unsafe, c_safe, c_hdot = ctx.params
        dh, dh_next, dh_ng, daction = ext.gcbf_loss_bwd(
            h, h_next, h_ng, action, u_qp, safe, unsafe, out,
            d_total.reshape(1).contiguous().float(),
            dt, alpha, eps, c_act, c_unsafe, c_safe, c_hdot,
        )
        return dh, dh_next, dh_ng, daction, None, None, None, None


def gcbf_plus_loss(h, h_next, h_ng, action, u_qp, safe, unsafe, dt, alpha, eps,
                   c_act, c_unsafe, c_safe, c_hdot):
    """Fused GCBF+ loss (reference gcbf_plus.py:364-431). Returns
    (total scalar, parts (8,) detached: [action, unsafe, safe, h_dot losses,
    acc_unsafe, acc_safe, acc_h_dot, unsafe_ratio])."""
    return _GCBFLossHIP.apply(h, h_next, h_ng, action, u_qp, safe, unsafe,
                              (dt, alpha, eps, c_act, c_unsafe, c_safe, c_hdot))


# --------------------------------------------------------------------------
# fused GCBF+ minibatch prologue for the DoubleIntegrator (K16)
# --------------------------------------------------------------------------
class _DILossPrepHIP(torch.autograd.Function):
    """u_ref (clipped-error LQR, reference env/double_integrator.py:332-338)
    -> action = clamp(2*raw + u_ref) -> euler next state (:112-143) ->
    big = [states; next_states]: one kernel instead of ~20 eager launches.
    Gradient flows to ``raw`` only (minibatch states are leaves)."""

    @staticmethod
    def forward(ctx, states, raw, K, n_agents, dt, inv_m, comm, vmax):
        ext = _require_ext()
        action, big = ext.di_loss_prep_fwd(
            states.contiguous(), raw.contiguous(), K.contiguous(),
            n_agents, dt, inv_m, comm, vmax)
        ctx.save_for_backward(states, raw, K, action)
        ctx.meta = (n_agents, dt, inv_m, comm, vmax)
        return action, big

    @staticmethod
    def backward(ctx, daction, dbig):
        ext = _require_ext()
        states, raw, K, action = ctx.saved_tensors
        n_agents, dt, inv_m, comm, vmax = ctx.meta
        if daction is None:
            daction = torch.zeros_like(action)
        if dbig is None:
            B, V, _ = states.shape
            dbig = states.new_zeros(2 * B, V, 4)
        draw = ext.di_loss_prep_bwd(
            states, raw, K, action, daction.contiguous(), dbig.contiguous(),
            n_agents, dt, inv_m, comm, vmax)
        return None, draw, None, None, None, None, None, None


def di_loss_prep(states: Tensor, raw: Tensor, K: Tensor, n_agents: int,
                 dt: float, inv_m: float, comm: float, vmax: float):
    """Returns (action (B,N,2), big_states (2B,V,4)). HIP on GPU; composed
    torch ops (same math, differentiable) on CPU."""
    if states.is_cuda and hip_available():
        return _DILossPrepHIP.apply(states, raw, K, n_agents, dt, inv_m, comm, vmax)
    N = n_agents
    agent = states[:, :N]
    goal = states[:, N:2 * N]
    err = goal - agent
    nrm = torch.linalg.vector_norm(err, dim=-1, keepdim=True).clamp_min(1e-9)
    emax = (err / nrm * comm).abs()
    uref = (torch.clamp(err, -emax, emax) @ K.t()).clamp(-1.0, 1.0)
    action = (2.0 * raw + uref).clamp(-1.0, 1.0)
    vel = (agent[..., 2:] + action * inv_m * dt).clamp(-vmax, vmax)
    pos = agent[..., :2] + agent[..., 2:] * dt
    nxt = torch.cat([torch.cat([pos, vel], -1), states[:, N:]], dim=1)
    return action, torch.cat([states, nxt], dim=0)


# --------------------------------------------------------------------------
# fused GCBF+ minibatch prologue for CrazyFlie
# --------------------------------------------------------------------------
class _CrazyFlieLossPrepHIP(torch.autograd.Function):
    """u_ref (env/crazyflie.py) -> action = 2*raw + u_ref (UNCLAMPED, as the
    action loss takes it) -> next = clip_state(RK4(x, clamp(action) * scale))
    with the low-level LQR per stage -> big = [states; next_states]: one
    kernel each way instead of a few hundred eager launches. The backward
    recomputes the RK4 in dual-number arithmetic, one thread per action
    component. Gradient flows to ``raw`` only (minibatch states are leaves)."""

    @staticmethod
    def forward(ctx, states, raw, consts, n_agents):
        ext = _require_ext()
        states, raw, consts = states.contiguous(), raw.contiguous(), consts.contiguous()
        action, big = ext.crazyflie_loss_prep_fwd(states, raw, consts, n_agents)
        # the unclamped action carries u_ref and both clamp masks: raw is not kept
        ctx.save_for_backward(states, consts, action)
        ctx.n_agents = n_agents
        return action, big

    @staticmethod
    def backward(ctx, daction, dbig):
        ext = _require_ext()
        states, consts, action = ctx.saved_tensors
        if daction is None:
            daction = torch.zeros_like(action)
        if dbig is None:
            B, V, S = states.shape
            dbig = states.new_zeros(2 * B, V, S)
        draw = ext.crazyflie_loss_prep_bwd(
            states, consts, action, daction.contiguous(), dbig.contiguous(),
            ctx.n_agents)
        return None, draw, None, None


def crazyflie_loss_prep(states: Tensor, raw: Tensor, consts: Tensor, n_agents: int):
    """Returns (action (B,N,4) = 2*raw + u_ref unclamped, big_states
    (2B,V,12) = [states; next_states]). states (B,V,12) with agent rows
    [:N] and goal rows [N:2N]; consts is CrazyFlie._fused_consts. GPU only
    (HIP, capture-safe); CPU callers take the composed env path."""
    if not states.is_cuda:
        raise NotImplementedError("CPU path goes through env.u_ref / env.forward_graph")
    return _CrazyFlieLossPrepHIP.apply(states, raw, consts, n_agents)


# --------------------------------------------------------------------------
# fused GCBF+ minibatch prologue for DubinsCar, LinearDrone, SingleIntegrator
# (env_loss_prep_{fwd,bwd}_kernel over the env structs of loss_prep_envs.h)
# --------------------------------------------------------------------------
class _EnvLossPrepHIP(torch.autograd.Function):
    """u_ref -> action = 2*raw + u_ref (UNCLAMPED, as the action loss takes
    it) -> next = clip_state(step(x, clamp(action))) -> big = [states;
    next_states]: one kernel each way instead of a few dozen eager launches.
    ``kind`` names the entry-point pair, ``mats`` the tensors it takes after
    ``states`` (gain, A, B), ``tail`` its trailing scalars and limits.
    Gradient flows to ``raw`` only (minibatch states are leaves)."""

    @staticmethod
    def forward(ctx, kind, states, raw, mats, n_agents, tail):
        ext = _require_ext()
        states, raw = states.contiguous(), raw.contiguous()
        mats = tuple(m.contiguous() for m in mats)
        action, big = getattr(ext, kind + "_loss_prep_fwd")(states, raw, *mats, n_agents, *tail)
        # the unclamped action carries u_ref and the action clamp mask: raw is not kept
        ctx.save_for_backward(states, action, *mats)
        ctx.meta = (kind, n_agents, tail)
        return action, big

    @staticmethod
    def backward(ctx, daction, dbig):
        ext = _require_ext()
        states, action, *mats = ctx.saved_tensors
        kind, n_agents, tail = ctx.meta
        if daction is None:
            daction = torch.zeros_like(action)
        if dbig is None:
            B, V, S = states.shape
            dbig = states.new_zeros(2 * B, V, S)
        draw = getattr(ext, kind + "_loss_prep_bwd")(
            states, *mats, action, daction.contiguous(), dbig.contiguous(), n_agents, *tail)
        return None, None, draw, None, None, None


def _lims(act_lim, state_lim):
    return tuple([float(v) for v in lim] for lim in (*act_lim, *state_lim))


def dubins_loss_prep(states: Tensor, raw: Tensor, n_agents: int, dt: float, comm: float,
                     stop_r: float, enable_stop: bool, act_lim, state_lim):
    """Returns (action (B,N,2) = 2*raw + u_ref unclamped, big_states (2B,V,4)
    = [states; next_states]) for DubinsCar. states (B,V,4) with agent rows
    [:N] and goal rows [N:2N]; act_lim / state_lim are (lo, hi) sequences of
    floats (env.action_lim() / env.state_lim()), stop_r = 0.5 * car_radius.
    GPU only (HIP, capture-safe); CPU callers take the composed env path."""
    if not states.is_cuda:
        raise NotImplementedError("CPU path goes through env.u_ref / env.forward_graph")
    tail = (float(dt), float(comm), float(stop_r), bool(enable_stop), *_lims(act_lim, state_lim))
    return _EnvLossPrepHIP.apply("dubins", states, raw, (), n_agents, tail)


def drone_loss_prep(states: Tensor, raw: Tensor, K: Tensor, A: Tensor, Bm: Tensor,
                    n_agents: int, dt: float, comm: float, act_lim, state_lim):
    """LinearDrone: (action (B,N,3) unclamped, big_states (2B,V,6)). K (3,6)
    LQR gain, A (6,6) and Bm (6,3) of xdot = A x + B a. GPU only."""
    if not states.is_cuda:
        raise NotImplementedError("CPU path goes through env.u_ref / env.forward_graph")
    tail = (float(dt), float(comm), *_lims(act_lim, state_lim))
    return _EnvLossPrepHIP.apply("drone", states, raw, (K, A, Bm), n_agents, tail)


def si_loss_prep(states: Tensor, raw: Tensor, K: Tensor, n_agents: int, dt: float,
                 comm: float, act_lim, state_lim):
    """SingleIntegrator: (action (B,N,2) unclamped, big_states (2B,V,2)). K
    (2,2) LQR gain; state_lim is all infinite (no state clip). GPU only."""
    if not states.is_cuda:
        raise NotImplementedError("CPU path goes through env.u_ref / env.forward_graph")
    tail = (float(dt), float(comm), *_lims(act_lim, state_lim))
    return _EnvLossPrepHIP.apply("si", states, raw, (K,), n_agents, tail)
