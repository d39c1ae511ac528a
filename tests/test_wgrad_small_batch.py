"""The collector of small narrow weight gradients (ops._WgradBatch): K fused MLPs leave as one dW1 grid, one dW2 grid and one
reduction instead of three launches each.  Per member nothing changes, so a trainer step gives the same bits whatever K is --
eager with side streams, captured as one graph with forks, captured as segments; over a rollout (the same MLP arrives once per
AR step: flush on repeat) and over an accumulation window."""
import pytest
import torch

from neural_lam_amd import _lib as L

CAP = L.NLAM_MAX_GROUP


# ---- the policy: pure Python on shapes, no device ---------------------------------------------------------------------------
def test_what_is_small_and_when_the_collector_flushes():
    from neural_lam_amd import ops

    small, policy = ops.wgrad_is_small, ops.wgrad_batch_policy
    # at most two 32-row chunks per workgroup
    assert small(6561, 1, 128, 2)          # 206 chunks on 128 workgroups: the mesh-node MLPs of cfg2
    assert not small(57616, 1, 226, 2)     # 1 801 chunks on 226
    assert small(256 * 32, 1, 128, 2) and not small(256 * 32 + 1, 1, 128, 2)
    assert small(40, 2, 4, 2) and small(1, 1, 1, 2)
    assert small(33, 128, 128, 2) and not small(33, 129, 128, 2)   # chunks are counted per batch item: 33 rows are two
    assert not small(1, 1, 1, 0)           # the override for measuring: nothing is small
    assert small(6561, 1, 128, None) == (ops.WGRAD_BATCH_CHUNKS >= 2)
    # (flush before adding, flush after adding)
    assert policy(set(), 0, 7, 6, 5, CAP, 40) == (False, False)
    assert policy({1, 2, 3}, 18, 7, 6, 5, CAP, 40) == (False, False)
    assert policy({1, 2, 3, 4}, 24, 7, 6, 5, CAP, 40) == (False, True)        # K members wait
    assert policy({1, 2}, 12, 2, 6, 5, CAP, 40) == (True, False)              # the owner is already waiting
    assert policy({1}, 6, 1, 6, 1, CAP, 40) == (True, True)                   # ... and K = 1: alone again, and out
    assert policy({1, 2, 3, 4, 5, 6}, 36, 7, 6, 100, CAP, 40) == (True, False)   # 42 jobs would not fit one reduction launch
    assert policy({1, 2, 3, 4, 5, 6}, 34, 7, 6, 100, CAP, 40) == (False, False)
    assert policy(set(range(CAP)), 16, 99, 2, 100, CAP, 40) == (True, False)  # the entry point's member cap
    assert policy(set(range(CAP - 1)), 14, 99, 2, 100, CAP, 40) == (False, True)   # K is clipped to the cap
    assert policy(set(), 0, 7, 6, 0, CAP, 40) == (False, True)                # (K < 1 reads as 1; the collector is off then anyway)
    assert policy({1}, 6, 7, 6, 2) == (False, True)                           # caps default to the library's
    # driving the policy over a rollout: five MLPs per AR step, two AR steps, K = 3 -> the flushes and their members
    pending, flushed = [], []
    for owner in [1, 2, 3, 4, 5, 1, 2, 3, 4, 5]:
        before, after = policy(set(pending), 6 * len(pending), owner, 6, 3, CAP, 40)
        if before:
            flushed.append(pending)
            pending = []
        pending = pending + [owner]
        if after:
            flushed.append(pending)
            pending = []
    assert flushed == [[1, 2, 3], [4, 5, 1], [2, 3, 4]] and pending == [5]
    for f in flushed:
        assert len(set(f)) == len(f)


# ---- trainer steps ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _trainer(tmp_path, dev, **kw):
    from neural_lam_amd import graph as G
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore
    from neural_lam_amd.trainer import Trainer

    ds = SyntheticDatastore(60, 54, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)
    ext = ds.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state")), max(ext[1] - ext[0], ext[3] - ext[2]))
    torch.manual_seed(1)
    fc = hm.ARForecaster(hm.GraphLAM(ds, graph=graph, hidden_dim=64, processor_layers=2), ds)
    return ds, Trainer(hm.ForecasterStep(fc, ds).to(dev), lr=1e-3, **kw)


def _run(tmp_path, dev, monkeypatch, K, T, nsteps, **kw):
    """``nsteps`` trainer steps with the collector at K -> (losses, flat gradient, flat parameters, sizes of the flushes)."""
    from neural_lam_amd import ops

    monkeypatch.setattr(ops, "WGRAD_BATCH_K", K)
    sizes = []
    launch = ops._wgrad_batch_launch
    monkeypatch.setattr(ops, "_wgrad_batch_launch", lambda members: (sizes.append(len(members)), launch(members))[1])
    ds, tr = _trainer(tmp_path, dev, **kw)
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(0)
    losses = []
    for _ in range(nsteps):
        batch = [torch.randn(1, 2, N, 5, generator=g).to(dev), torch.randn(1, T, N, 5, generator=g).to(dev),
                 torch.randn(1, T, N, 6, generator=g).to(dev)]
        losses.append(float(tr.step(*batch)))
    torch.cuda.synchronize()
    return losses, tr.fp.grad.clone(), tr.fp.flat.clone(), sizes


MODES = {"eager": dict(use_graph=False), "forks": dict(use_graph=True, executor="forks"),
         "segments": dict(use_graph=True, executor="segments")}


@pytest.mark.gpu
@pytest.mark.parametrize("mode,T,accum", [("eager", 1, 1), ("forks", 1, 1), ("segments", 1, 1), ("eager", 2, 1), ("segments", 2, 1),
                                          ("forks", 2, 1), ("forks", 1, 2), ("segments", 1, 2)])
def test_step_has_the_same_bits_for_every_batch_size(dev, tmp_path, monkeypatch, mode, T, accum):
    kw = dict(MODES[mode])
    if accum > 1:
        kw["accumulate_grad_batches"] = accum
    nsteps = 2 * accum
    off = _run(tmp_path, dev, monkeypatch, 0, T, nsteps, **kw)
    assert off[3] == []
    for K in (2, CAP):
        on = _run(tmp_path, dev, monkeypatch, K, T, nsteps, **kw)
        assert on[3] and 2 <= max(on[3]) <= K, on[3]   # the collector was in use, and grouped
        assert on[0] == off[0], (mode, K)
        assert torch.equal(on[1], off[1]), (mode, K, "flat gradient")
        assert torch.equal(on[2], off[2]), (mode, K, "parameters")
