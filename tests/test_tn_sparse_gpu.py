"""The sparse-staged dW kernel (gemm_tn_partial3_map_kernel): a ``gemm_tn``
call through a row map at the smallest shapes that reach ``tn3``.

Every comparison is on the BITS of dW and db (so a NaN compares equal to the
same NaN), against two references:

(a) the dense call (``row_map=None``) on the scattered operands, whose masked
    rows have dZ == 0 and arbitrary finite X;
(b) the same mapped call under ``GCBF_NO_TN_SPARSE=1``, i.e. through
    gemm_tn_partial3_kernel's map path. The toggle is read once per process,
    so ONE child process computes (b) for every case of this file and the
    tests share its results.

Compact rows past the count hold NaN; nothing may read them. The path is
asserted from ``_C.gemm_tn_map_path`` in each case.

Run as a script (``python test_tn_sparse_gpu.py OUT``) this file is that child:
it computes the mapped result of every case and saves them to OUT.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 128  # TN3MAP_ROWS of dw_group.h: live rows one chunk holds

M_VALUES = (16384, 16385, 20480, 24999)  # 24999 % S != 0: slabs end mid-tile
SHAPES = ((64, 64), (32, 256), (256, 128), (128, 1), (40, 70), (8, 17))
MAPS = ("all_masked", "all_live", "one_slab", "slab_first", "slab_last", "m_last",
        "out_of_range", "permuted", "nan_negzero")


def _ext():
    from gcbfplus_amd import _C
    return _C


def _cases():
    """name -> spec. Every (K, N) at every M with a random 0.1 map, actin and
    gate cycling so that each of the six combinations meets each shape class;
    every special map at (64,64), M = 24999 (four tiles a slab, mid-tile slab
    ends) and at the scalar-path shape (40,70), M = 16385; base pointers 2
    bytes off; one slab longer than the row table (17 tiles: K = N = 512 has
    S = 16, so M = 16500 gives 1032 rows a slab)."""
    out = {}
    i = 0
    for K, N in SHAPES:
        for M in M_VALUES:
            out[f"rand-{M}-{K}x{N}"] = dict(M=M, K=K, N=N, actin=i % 3, gate=(i // 3) % 2 == 1,
                                            map="random")
            i += 1
    for j, kind in enumerate(MAPS):
        out[f"{kind}-24999-64x64"] = dict(M=24999, K=64, N=64, actin=j % 3, gate=j % 2 == 1,
                                          map=kind)
        out[f"{kind}-16385-40x70"] = dict(M=16385, K=40, N=70, actin=(j + 1) % 3,
                                          gate=j % 2 == 0, map=kind)
    out["xoff-20480-64x64"] = dict(M=20480, K=64, N=64, actin=1, gate=False, map="random", xoff=1)
    out["zoff-20480-64x64"] = dict(M=20480, K=64, N=64, actin=2, gate=True, map="random", zoff=1)
    out["yoff-20480-32x256"] = dict(M=20480, K=32, N=256, actin=2, gate=False, map="random", yoff=1)
    out["long_slab-16500-512x512"] = dict(M=16500, K=512, N=512, actin=1, gate=True, map="random")
    out["long_slab_live-16500-512x512"] = dict(M=16500, K=512, N=512, actin=0, gate=False,
                                               map="all_live")
    return out


CASES = _cases()


def _slabs(spec, path):
    S = int(path.split("S=")[1].split()[0])
    m_per = (spec["M"] + S - 1) // S
    return S, m_per


def _live_mask(spec, g, m_per):
    M, kind = spec["M"], spec["map"]
    live = torch.zeros(M, dtype=torch.bool)
    if kind in ("random", "out_of_range", "permuted", "nan_negzero"):
        live = torch.rand(M, generator=g) < 0.1
    elif kind == "all_live":
        live[:] = True
    elif kind == "one_slab":
        live[3 * m_per:4 * m_per] = True
    elif kind == "slab_first":
        live[5 * m_per] = True
    elif kind == "slab_last":
        live[6 * m_per - 1] = True
    elif kind == "m_last":
        live[M - 1] = True
    else:
        assert kind == "all_masked"
    return live


def _offset(t, off):
    """The same values in a contiguous tensor whose base pointer is `off`
    elements (2 bytes each) past a 16-byte boundary: no b128 loads."""
    if not off:
        return t.to(DEV)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 2 * off
    return v


def build(spec, path):
    """CPU operands of one case, dense and compact, from its own seed."""
    M, K, N = spec["M"], spec["K"], spec["N"]
    S, m_per = _slabs(spec, path)
    assert m_per > ROWS or spec["map"] != "all_live", "all-live slab must exceed one chunk"
    g = torch.Generator().manual_seed(1000 * M + 10 * K + N)
    x = torch.randn(M, K, generator=g).to(BF16)
    dy = torch.randn(M, N, generator=g).to(BF16)
    y = torch.randn(M, N, generator=g).to(BF16)
    gate = (torch.rand(M, generator=g) < 0.5) if spec["gate"] else None
    live = _live_mask(spec, g, m_per)
    rows = live.nonzero().reshape(-1)
    count = rows.numel()
    if spec["map"] == "nan_negzero":
        x[rows[1], 3] = float("nan")  # -> row 3 of dW
        dy[rows[2], 0] = float("nan")  # -> column 0 of dW, db[0]
        dy[rows[3], :] = -0.0
        x[rows[4], :] = -0.0
        if gate is not None:
            gate[rows[1:5]] = True
    cap = count + 3  # rows past the count: NaN
    order = torch.arange(count)
    if spec["map"] == "permuted":
        order = torch.randperm(count, generator=g)  # compact index of live row i
    inv = torch.full((M,), -1, dtype=torch.int32)
    inv[rows] = order.to(torch.int32)
    if spec["map"] == "out_of_range":
        dead = (~live).nonzero().reshape(-1)
        pick = dead[torch.randperm(dead.numel(), generator=g)[:512]]
        inv[pick[:256]] = cap
        inv[pick[256:384]] = cap + 1 + torch.arange(128, dtype=torch.int32)
        inv[pick[384:]] = 2 ** 31 - 1

    def compact(t, fill):
        out = torch.full((cap,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
        out[order] = t[rows]
        return out

    dy_dense = dy.clone()
    dy_dense[~live] = 0
    return dict(x=x, dy_dense=dy_dense, y=y, gate=gate, inv=inv,
                xc=compact(x, float("nan")), dyc=compact(dy, float("nan")),
                yc=compact(y, float("nan")),
                gc=None if gate is None else compact(gate, False))


def run_mapped(ext, spec, c):
    gc = None if c["gc"] is None else c["gc"].to(DEV)
    return ext.gemm_tn(_offset(c["xc"], spec.get("xoff", 0)), _offset(c["dyc"], spec.get("zoff", 0)),
                       _offset(c["yc"], spec.get("yoff", 0)), spec["actin"], gc, None,
                       c["inv"].to(DEV))


def run_dense(ext, spec, c):
    gd = None if c["gate"] is None else c["gate"].to(DEV)
    return ext.gemm_tn(_offset(c["x"], spec.get("xoff", 0)), _offset(c["dy_dense"], spec.get("zoff", 0)),
                       _offset(c["y"], spec.get("yoff", 0)), spec["actin"], gd)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def _path(ext, spec):
    return ext.gemm_tn_map_path(spec["M"], spec["K"], spec["N"], spec["actin"], spec["gate"])


@pytest.fixture(scope="module")
def old_kernel_results(tmp_path_factory):
    """(b): every case through the mapped call with GCBF_NO_TN_SPARSE=1, from
    one fresh child process."""
    out = str(tmp_path_factory.mktemp("tn_sparse") / "old.pt")
    env = dict(os.environ)
    env["GCBF_NO_TN_SPARSE"] = "1"
    env["PYTHONNOUSERSITE"] = "1"
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return torch.load(out)


@pytest.mark.parametrize("name", list(CASES), ids=str)
def test_map_kernel_keeps_bits(name, old_kernel_results):
    ext = _ext()
    spec = CASES[name]
    path = _path(ext, spec)
    assert path.startswith("tn3map S="), path
    assert path.replace("tn3map", "tn3") == ext.gemm_path("tn", spec["M"], spec["K"], spec["N"],
                                                         spec["actin"], spec["gate"])
    c = build(spec, path)
    dw, db = run_mapped(ext, spec, c)
    dw_a, db_a = run_dense(ext, spec, c)
    assert bits_equal(dw, dw_a) and bits_equal(db, db_a), "against the dense call"
    dw_b, db_b = old_kernel_results[name]
    assert bits_equal(dw.cpu(), dw_b) and bits_equal(db.cpu(), db_b), "against GCBF_NO_TN_SPARSE=1"
    if spec["map"] == "all_masked":
        assert not dw.any() and not db.any()
    elif spec["map"] != "nan_negzero":
        assert torch.isfinite(dw).all() and torch.isfinite(db).all()


def test_small_m_stays_on_tn1():
    ext = _ext()
    assert ext.gemm_tn_map_path(4096, 64, 64, 1, False).startswith("tn1 S=")


def test_graph_replay_follows_the_buffers():
    """One captured mapped gemm_tn, replayed on two maps and counts written into
    the same buffers: each replay bit-equal to the eager call on that state."""
    ext = _ext()
    spec = dict(M=20480, K=64, N=64, actin=2, gate=True, map="random")
    path = _path(ext, spec)
    assert path.startswith("tn3map S=")
    M, K, N = spec["M"], spec["K"], spec["N"]
    cap = M // 4
    xc = torch.empty(cap, K, dtype=BF16, device=DEV)
    dyc = torch.empty(cap, N, dtype=BF16, device=DEV)
    yc = torch.empty(cap, N, dtype=BF16, device=DEV)
    gc = torch.empty(cap, dtype=torch.bool, device=DEV)
    inv = torch.empty(M, dtype=torch.int32, device=DEV)

    def fill(seed, density):
        g = torch.Generator().manual_seed(seed)
        live = torch.rand(M, generator=g) < density
        count = int(live.sum())
        assert count < cap
        m = torch.full((M,), -1, dtype=torch.int32)
        m[live] = torch.arange(count, dtype=torch.int32)
        inv.copy_(m)
        for buf, width in ((xc, K), (dyc, N), (yc, N)):
            t = torch.full((cap, width), float("nan"), dtype=BF16)
            t[:count] = torch.randn(count, width, generator=g).to(BF16)
            buf.copy_(t)
        gc.copy_(torch.rand(cap, generator=g) < 0.5)

    fill(1, 0.1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext.gemm_tn(xc, dyc, yc, spec["actin"], gc, None, inv)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dw_g, db_g = ext.gemm_tn(xc, dyc, yc, spec["actin"], gc, None, inv)
    for seed, density in ((2, 0.03), (3, 0.2)):
        fill(seed, density)
        graph.replay()
        dw, db = ext.gemm_tn(xc, dyc, yc, spec["actin"], gc, None, inv)
        assert bits_equal(dw_g, dw) and bits_equal(db_g, db), seed
        assert torch.isfinite(dw).all() and dw.any()


def _child(out):
    ext = _ext()
    res = {}
    for name, spec in CASES.items():
        path = _path(ext, spec)
        assert path.startswith("tn3 S="), path
        dw, db = run_mapped(ext, spec, build(spec, path))
        res[name] = (dw.cpu(), db.cpu())
    torch.save(res, out)


if __name__ == "__main__":
    _child(sys.argv[1])
