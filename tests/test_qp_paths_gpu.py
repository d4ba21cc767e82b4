"""Path-complete tests of the batched QP kernel (K11, proxqp.hip) on the GPU:
every case of tests/test_qp_oracle.py is asserted to take the dispatch path
it names (``_C.proxqp_path``), solved on the device at the case's iteration
count and judged by ``check_qp`` against the certified float64 reference,
which is computed on the host. The oracle's CPU self-tests prove that every
reference solution certifies, that the float32 CPU path of the same
algorithm meets a five times tighter bound on the same inputs, and that the
comparator rejects the defects it is here to catch; a failure here can then
not be blamed on the inputs or on the reference."""
import numpy as np
import pytest
import torch

import test_qp_oracle as O

pytestmark = pytest.mark.gpu

from gcbfplus_amd.ops.qp import kernel_path, proxqp_solve

DEV = "cuda"


def _ext():
    from gcbfplus_amd import _C
    return _C


def _solve(problem, iters):
    return proxqp_solve(*O.to_torch(problem, DEV), iters=iters)


@pytest.mark.parametrize("case", O.CASES, ids=O.case_id)
def test_case_matches_certified_optimum(case):
    assert _ext().proxqp_path(case.nv, case.k) == case.path
    assert kernel_path(case.nv, case.k) == case.path
    problem, x_ref, _ = O.reference(case)
    x = _solve(problem, case.iters)
    assert x.dtype == torch.float32 and x.shape == (O.M_PER_CASE, case.nv)
    x = x.cpu().numpy()
    err = np.abs(x - x_ref) / np.maximum(1.0, np.abs(x_ref))
    if case.layout == "dec":
        err = err[:, :O.n_u(case)]
    print(f"QP_GPU case={case.name} path={case.path} iters={case.iters} "
          f"worst_err={err.max():.3g} worst_viol={O.primal_violation(problem, x).max():.3g}")
    O.check_qp(problem, x, x_ref, case.layout, f"{case.name} gpu")


def _limit(path, probe):
    """Largest n for which probe(n) still names ``path``."""
    ext = _ext()
    n = 1
    while ext.proxqp_path(*probe(n + 1)) == path:
        n += 1
        assert n < 4096
    return n


def test_matrix_covers_every_path_and_threshold():
    """Both instantiations and the fallback are reached, and every threshold
    of the dispatch function has a case that fits it exactly and a case just
    past it: a later change of threshold must move a case, not drop a path."""
    ext = _ext()
    reached = {c.path for c in O.CASES}
    print(f"QP_PATHS reached={sorted(reached)}")
    assert reached == {"w32x16", "w64x32", "none"}
    nv_small = _limit("w32x16", lambda n: (n, 1))
    k_small = _limit("w32x16", lambda n: (nv_small, n))
    nv_big = nv_small + _limit("w64x32", lambda n: (nv_small + n, 1))
    k_big = k_small + _limit("w64x32", lambda n: (nv_big, k_small + n))
    print(f"QP_LIMITS w32x16 nv<={nv_small} k<={k_small}; w64x32 nv<={nv_big} k<={k_big}")
    assert ext.proxqp_path(nv_big + 1, 1) == "none"
    assert ext.proxqp_path(nv_big, k_big + 1) == "none"
    shapes = {(c.nv, c.k): c.path for c in O.CASES}
    # exact fit of each limit alone and of both at once
    assert any(nv == nv_small and k < k_small for nv, k in shapes)
    assert shapes.get((nv_small, k_small)) == "w32x16"
    assert any(nv == nv_big and k < k_big for nv, k in shapes)
    assert shapes.get((nv_big, k_big)) == "w64x32"
    # first shape past each limit of the small kernel lands in the big one
    assert any(nv == nv_small + 1 and k <= k_small and p == "w64x32"
               for (nv, k), p in shapes.items())
    assert any(k == k_small + 1 and p == "w64x32" for (nv, k), p in shapes.items())
    # past the big kernel: the torch fallback, within a few variables of the limit
    assert any(nv_big < nv <= nv_big + 2 and p == "none" for (nv, k), p in shapes.items())
    # every class is judged on both kernels
    for path in ("w32x16", "w64x32"):
        assert {c.cls for c in O.CASES if c.path == path} == set(O._CLASSES)


def _case(name):
    return next(c for c in O.CASES if c.name == name)


@pytest.mark.parametrize("M", [1, 37])
@pytest.mark.parametrize("name", ["N16nu1-box", "N32nu1-box", "dec-nu2k3-relax"])
def test_slots_are_independent(name, M):
    """A problem's answer depends on nothing but the problem: the permuted
    batch gives the permuted result bit for bit, and a batch of one gives the
    first row."""
    case = _case(name)
    assert case.path != "none"
    problem = O.make_problem(case, M=37)
    ts = O.to_torch(problem, DEV)
    x = proxqp_solve(*ts, iters=O.TRAIN_ITERS)
    assert torch.isfinite(x).all()
    if M == 1:
        x1 = proxqp_solve(*[t[5:6].contiguous() for t in ts], iters=O.TRAIN_ITERS)
        assert torch.equal(x1, x[5:6])
        return
    perm = torch.from_numpy(np.random.default_rng(3).permutation(M)).to(DEV)
    assert not torch.equal(perm, torch.arange(M, device=DEV))
    xp = proxqp_solve(*[t[perm].contiguous() for t in ts], iters=O.TRAIN_ITERS)
    assert torch.equal(xp, x[perm])
    assert len({tuple(r) for r in x.cpu().numpy().round(6)}) == M   # rows do differ


@pytest.mark.parametrize("name", ["N8nu3-interior", "N16nu3-box"])
def test_deterministic(name):
    case = _case(name)
    problem, _, _ = O.reference(case)
    a = _solve(problem, case.iters)
    b = _solve(problem, case.iters)
    assert torch.equal(a, b)


def test_fallback_runs_float64_on_device_and_float32_on_host():
    """The torch path serves what the kernel cannot: ADMM in float64 on the
    device, float32 on the host, float32 out on both."""
    case = _case("N22nu2-interior")
    assert case.path == "none"
    problem, x_ref, _ = O.reference(case)
    seen = []
    orig = torch.linalg.cholesky

    def spy(K, *a, **kw):
        seen.append((K.device.type, K.dtype))
        return orig(K, *a, **kw)

    torch.linalg.cholesky = spy
    try:
        xg = _solve(problem, case.iters)
        xc = proxqp_solve(*O.to_torch(problem), iters=case.iters)
    finally:
        torch.linalg.cholesky = orig
    assert ("cuda", torch.float64) in seen and ("cpu", torch.float32) in seen
    assert ("cuda", torch.float32) not in seen
    assert xg.dtype == torch.float32 and xc.dtype == torch.float32
    O.check_qp(problem, xg.cpu().numpy(), x_ref, case.layout, "fallback gpu")


# Graph of the route test. The QPs DecShareCBF builds carry rows of norm ~30
# and the solver is only just converging on them at the controller's 150
# iterations: on most draws single problems are off by O(1) at some count
# between 100 and 150 on the float32 CPU path too (profiles/qp_accuracy.md).
# This draw is the first of seeds 1..12 on which the CPU path is within the
# selection tolerance from 120 iterations on, which the test checks.
ROUTE_SEED = 9


def _dec_share_qp(device, seed):
    """(problem, x) of DecShareCBF.get_qp_action on a 4-agent DoubleIntegrator
    graph: the QP it builds, rebuilt here from the same tensors, and its answer."""
    from gcbfplus_amd.algo import make_algo
    from gcbfplus_amd.algo.pwise import pwise_cbf
    from gcbfplus_amd.env import make_env

    torch.manual_seed(seed)
    env = make_env("DoubleIntegrator", num_agents=4, area_size=2.0, max_step=8, device=device)
    algo = make_algo("dec_share_cbf", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                     state_dim=env.state_dim, action_dim=env.action_dim, n_agents=4)
    assert algo.qp_iters == O.TRAIN_ITERS
    graph = env.reset(4, np.random.default_rng(seed))
    with torch.no_grad():
        u_qp, r_qp = algo.get_qp_action(graph)
        B, N, k, nu = graph.batch_size, 4, algo.k, env.action_dim
        h, h_x, isobs = pwise_cbf(env, graph, k)
        f, gdyn = env.control_affine_dyn(graph.agent_states)
        Lf_h = torch.einsum("bikjs,bjs->bik", h_x, f)
        idx = torch.arange(N, device=device)
        Lg = torch.einsum("biks,bisu->biku", h_x[:, idx, :, idx, :].permute(1, 0, 2, 3), gdyn)
        u_ref = env.u_ref(graph)
        bvec = torch.where(isobs, 1.0, 0.5) * (Lf_h + algo.cbf_alpha * h)
        lb, ub = env.action_lim()
    M, nv = B * N, nu + k
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    H = np.tile(np.eye(nv), (M, 1, 1))
    H[:, nu:, nu:] = 10.0
    problem = dict(
        H=H,
        g=np.concatenate([-f64(u_ref).reshape(M, nu), 1e3 * np.ones((M, k))], axis=1),
        C=-np.concatenate([f64(Lg).reshape(M, k, nu), np.tile(np.eye(k), (M, 1, 1))], axis=2),
        b=f64(bvec).reshape(M, k),
        l=np.tile(np.concatenate([f64(lb), np.zeros(k)]), (M, 1)),
        u=np.tile(np.concatenate([f64(ub), np.full(k, np.inf)]), (M, 1)))
    x = np.concatenate([f64(u_qp).reshape(M, nu), f64(r_qp).reshape(M, k)], axis=1)
    return problem, x


def test_dec_share_route():
    """DecShareCBF.get_qp_action on the device against the reference solve of
    the very QP it builds. The graph meets the oracle's selection condition
    around the controller's own iteration count: the float32 CPU path is
    within 2e-5 of the certified optimum at 120, 150 and 300 iterations."""
    problem, x = _dec_share_qp(DEV, ROUTE_SEED)
    M, nv = problem["g"].shape
    k = problem["b"].shape[1]
    nu = nv - k
    assert _ext().proxqp_path(nv, k) == "w32x16"
    x_ref, ys = O.solve_reference(problem)
    cert = np.array([O.kkt_certificate(O._slice(problem, q), x_ref[q], ys[q]) for q in range(M)])
    assert (cert <= O.CERT_TOL).all(), cert.max(axis=0)
    for iters in (O.TRAIN_ITERS * 4 // 5, O.TRAIN_ITERS, 2 * O.TRAIN_ITERS):
        xc = O.solve_under_test(problem, iters)
        assert np.abs(xc - x_ref)[:, :nu].max() <= O.SELECT_TOL, iters
    ratio, viol = O.check_qp(problem, x, x_ref, "dec", "dec-share route")
    print(f"QP_DEC_ROUTE problems={M} worst_err_over_bound={ratio:.3g} worst_viol={viol:.3g}")


def test_accuracy_record_gpu():
    rows = O.accuracy_record(DEV)
    assert len(rows) == len(O.CASES) + len(O.LEFT_OUT_CASES)
