"""Behavioral parity anchor: load the REFERENCE's own pretrained pickles
(<Env>/gcbf+/models/1000/{actor,cbf}.pkl as written by reference
gcbf.py:344-349, stored byte-for-byte under tests/golden/reference_pretrained)
into this framework's nets and check the
policy actually works — this exercises the jax-free unpickler, the flax-tree
layout mapping, and the full forward stack (edges, GNN, u_ref, dynamics,
masks) end-to-end against weights trained in the reference implementation.
"""
import os

import numpy as np
import pytest
import torch

from gcbfplus_amd.algo import make_algo
from gcbfplus_amd.algo.utils import load_flax_pickle
from gcbfplus_amd.env import make_env
from gcbfplus_amd.trainer.utils import collect_rollout

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "reference_pretrained")


@pytest.fixture(scope="module")
def ref_dir(tmp_path_factory):
    """The checkpoints in the reference's directory layout. Each ~1.4 MB
    pickle is stored as two halves (.part0 + .part1) to keep every committed
    file under 1 MiB; joining them restores the original bytes."""
    root = tmp_path_factory.mktemp("reference_pretrained")
    for env_id in sorted(os.listdir(GOLDEN)):
        out = root / env_id / "gcbf+" / "models" / "1000"
        out.mkdir(parents=True)
        for net in ("actor", "cbf"):
            with open(out / f"{net}.pkl", "wb") as f:
                for part in ("part0", "part1"):
                    with open(os.path.join(GOLDEN, env_id, f"{net}.pkl.{part}"), "rb") as g:
                        f.write(g.read())
    return str(root)


def _algo_with_ref_weights(ref_dir, env_id, n_agents, area_size, device="cpu", **env_kw):
    env = make_env(env_id, n_agents, area_size=area_size, device=device, **env_kw)
    algo = make_algo(algo="gcbf+", env=env, node_dim=env.node_dim,
                     edge_dim=env.edge_dim, state_dim=env.state_dim,
                     action_dim=env.action_dim, n_agents=n_agents)
    algo.load(os.path.join(ref_dir, env_id, "gcbf+", "models"), 1000)
    return env, algo


def test_load_flax_pickle_no_jax(ref_dir):
    tree = load_flax_pickle(os.path.join(ref_dir, "DoubleIntegrator/gcbf+/models/1000/cbf.pkl"))
    p = tree["params"]
    assert set(p) == {"GNN_0", "CBFHead", "Dense_0"}
    k = p["GNN_0"]["GNNLayer_0"]["msg"]["Dense_0"]["kernel"]
    assert isinstance(k, np.ndarray) and k.dtype == np.float32 and k.ndim == 2


def test_reference_di_weights_drive_safely(ref_dir):
    """Reference DI checkpoint in this framework: zero collisions and most
    agents reach goals within one episode (reference claims high safe/reach
    at n=8; measured here 100%/94% over 4 epi — see BASELINE.md)."""
    env, algo = _algo_with_ref_weights(ref_dir, "DoubleIntegrator", 8, 4.0)
    rng = np.random.default_rng(1234)
    g = env.reset(1, rng)
    ro = collect_rollout(env, algo.act, g)
    gall = ro.graph_Tp1(env)
    T = ro.time_horizon + 1
    coll = env.collision_mask(gall).reshape(1, T, -1)
    fin = env.finish_mask(gall).reshape(1, T, -1)
    safe = 1.0 - coll.amax(dim=1).float()
    finish = fin.amax(dim=1).float()
    assert safe.mean().item() == 1.0, "reference weights should be collision-free"
    assert finish.mean().item() >= 0.5, "most agents should reach their goals"


def test_reference_weights_h_sign_sanity(ref_dir):
    """h from the reference CBF weights: positive at a spread-out reset,
    negative when two agents are forced into collision."""
    env, algo = _algo_with_ref_weights(ref_dir, "DoubleIntegrator", 8, 4.0)
    rng = np.random.default_rng(7)
    g = env.reset(1, rng)
    h0 = algo.get_cbf(g)
    assert torch.isfinite(h0).all()
    assert (h0 > 0).float().mean().item() > 0.9
    # drive agents 0 and 1 to the same point -> h must flag danger
    states = g.states.clone()
    states[0, 1, :2] = states[0, 0, :2] + 0.01
    g2 = env.get_graph(states[:, : env.num_agents, :],
                       states[:, env.num_agents : 2 * env.num_agents, :],
                       g.env_states)
    h2 = algo.get_cbf(g2)
    assert (h2[0, :2] < 0).any(), "colliding pair should get negative h"


@pytest.mark.parametrize("env_id,n,area", [
    ("SingleIntegrator", 8, 4.0),
    ("DubinsCar", 8, 4.0),
    ("LinearDrone", 8, 4.0),
    ("CrazyFlie", 8, 4.0),
])
def test_reference_weights_load_all_envs(ref_dir, env_id, n, area):
    """Every reference pretrained checkpoint loads and produces finite,
    sane outputs through this framework's forward stack (full behavioral
    evals recorded in profiles/ref_*_eval*.log / BASELINE.md)."""
    env, algo = _algo_with_ref_weights(ref_dir, env_id, n, area)
    rng = np.random.default_rng(5)
    g = env.reset(1, rng)
    h = algo.get_cbf(g)
    a = algo.act(g)
    assert torch.isfinite(h).all() and torch.isfinite(a).all()
    r = env.step(g, a if not isinstance(a, tuple) else a[0])
    assert torch.isfinite(r.graph.states).all()


def test_load_flax_pickle_rejects_arbitrary_globals(tmp_path):
    """The checkpoint unpickler must refuse non-allowlisted globals instead
    of executing them."""
    import pickle

    class Evil:
        def __reduce__(self):
            return (print, ("pwned",))

    p = tmp_path / "evil.pkl"
    with open(p, "wb") as f:
        pickle.dump({"params": Evil()}, f)
    with pytest.raises(Exception):
        load_flax_pickle(str(p))
