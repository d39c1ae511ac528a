"""Optimizer controls decided on the device: gradient clipping by global norm, closed-form learning-rate schedules and the
non-finite-step guard (``ops.LRSchedule``, ``ops.global_grad_norm``, ``ops.AdamWFlat`` / ``Trainer`` with ``max_grad_norm``,
``lr_schedule``, ``skip_nonfinite``; ``nlam_grad_sumsq`` and ``nlam_adamw_step_controlled`` underneath)."""
import ctypes as C
import math
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, rel_err
from neural_lam_amd import _lib as L

TOL = 1e-4           # relative bar of the existing trainer trajectory tests (losses)
WEIGHT_BAR = 2e-4    # their absolute bar on the final weights
NEW_EXPORTS = ["nlam_grad_sumsq_workspace_doubles", "nlam_grad_sumsq", "nlam_adamw_step_controlled"]
FAKE = 0x1000        # a non-null, aligned address for the argument checks where there is no GPU (nothing can launch there)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
SCHEDULES = [
    ("warm-up only", dict(kind="constant", warmup_steps=5)),
    ("cosine", dict(kind="warmup_cosine", warmup_steps=3, total_steps=12, min_ratio=0.1)),
    ("linear", dict(kind="warmup_linear", warmup_steps=4, total_steps=10, min_ratio=0.25)),
    ("total reached and passed", dict(kind="warmup_cosine", warmup_steps=2, total_steps=6, min_ratio=0.05)),
    ("no warm-up", dict(kind="warmup_linear", warmup_steps=0, total_steps=8)),
    ("no warm-up, constant", dict(kind="constant", warmup_steps=0)),
    ("total inside the warm-up", dict(kind="warmup_cosine", warmup_steps=6, total_steps=4, min_ratio=0.5)),
]


def _formula(s, kind, warmup_steps=0, total_steps=None, min_ratio=0.0):
    """The schedule as the issue states it, written out independently of ops.LRSchedule."""
    W, T, r = warmup_steps, total_steps, min_ratio
    if s < W:
        return (s + 1) / W
    if kind == "constant":
        return 1.0
    p = min(1.0, (s - W) / max(1, T - W))
    if kind == "warmup_cosine":
        return r + (1 - r) * 0.5 * (1 + math.cos(math.pi * p))
    return r + (1 - r) * (1 - p)


@pytest.mark.parametrize("name,kw", SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_lr_schedule_factor_equals_lambda_lr(name, kw):
    from neural_lam_amd import ops

    sch = ops.LRSchedule(**kw)
    w = torch.nn.Parameter(torch.ones(3))
    opt = torch.optim.AdamW([w], lr=2e-3, betas=(0.9, 0.95))
    lam = torch.optim.lr_scheduler.LambdaLR(opt, sch.factor)
    for s in range(16):   # update s + 1 uses what the scheduler left after s steps
        assert opt.param_groups[0]["lr"] == 2e-3 * sch.factor(s), (name, s)
        assert sch.factor(s) == pytest.approx(_formula(s, **kw), rel=1e-15, abs=0.0), (name, s)
        w.grad = torch.ones(3)
        opt.step()
        lam.step()
    if kw["warmup_steps"]:
        assert sch.factor(0) == 1 / kw["warmup_steps"] and sch.factor(kw["warmup_steps"] - 1) == 1.0
    if kw["kind"] != "constant":
        assert sch.factor(kw["total_steps"] + 7) == pytest.approx(kw.get("min_ratio", 0.0), abs=1e-15)
    assert ops.LRSchedule(**sch.state_dict()).state_dict() == sch.state_dict()


def test_lr_schedule_rejects_bad_arguments():
    from neural_lam_amd import ops

    for bad in (dict(kind="step"), dict(kind="warmup_cosine"), dict(kind="constant", warmup_steps=-1),
                dict(kind="warmup_linear", total_steps=5, min_ratio=1.5), dict(kind="constant", warmup_steps=2.5)):
        with pytest.raises(ValueError):
            ops.LRSchedule(**bad)


def test_optctl_struct_matches_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(nlam_optctl_t), offsetof(nlam_optctl_t, control),'
        " offsetof(nlam_optctl_t, n), offsetof(nlam_optctl_t, lr), offsetof(nlam_optctl_t, max_grad_norm),"
        " offsetof(nlam_optctl_t, schedule), offsetof(nlam_optctl_t, skip_nonfinite), NLAM_OPTCTL_WORDS, NLAM_SCHED_NONE,"
        " NLAM_SCHED_CONSTANT, NLAM_SCHED_WARMUP_COSINE, NLAM_SCHED_WARMUP_LINEAR); return 0;}\n"
    )
    exe = tmp_path / "sz"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [
        C.sizeof(L.OptCtl), L.OptCtl.control.offset, L.OptCtl.n.offset, L.OptCtl.lr.offset, L.OptCtl.max_grad_norm.offset,
        L.OptCtl.schedule.offset, L.OptCtl.skip_nonfinite.offset, L.OPTCTL_WORDS, L.SCHED_NONE,
        L.SCHED_KINDS["constant"], L.SCHED_KINDS["warmup_cosine"], L.SCHED_KINDS["warmup_linear"],
    ]


def _address():
    """Where the rejected calls point.  Every one of them must return before a launch; with a GPU present the address is
    still that of a real buffer as large as the largest ``n`` asked for, so a validation that let one through would write
    into this test's own memory and fail the assertion, not launch on a wild pointer."""
    if not torch.cuda.is_available():
        return None, FAKE
    buf = torch.zeros(5_000_000, device="cuda", dtype=torch.float32)
    return buf, buf.data_ptr()


def _ctl(addr, **kw):
    p = L.OptCtl()
    for k in ("param", "grad", "exp_avg", "exp_avg_sq", "step_count_dev", "bias_corr_dev", "partials", "control"):
        setattr(p, k, addr)
    p.n, p.partials_doubles = 1000, 256
    p.lr, p.beta1, p.beta2, p.eps, p.weight_decay, p.grad_scale = 1e-3, 0.9, 0.95, 1e-8, 1e-2, 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_entry_points_are_declared_exported_and_reject_bad_arguments_without_a_gpu():
    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.nlam_abi_version() == L.ABI_VERSION == 8
    # at most nlam_num_blocks(n) workgroups, one fp64 partial each
    for n in (0, 1, 255, 4096, 4097, 100_003, 5_000_000, 10**9):
        nws = lib.nlam_grad_sumsq_workspace_doubles(n)
        assert 1 <= nws <= max(1, lib.nlam_num_blocks(n)) and nws <= 256, n
    assert lib.nlam_grad_sumsq_workspace_doubles(-1) == -1
    keep, addr = _address()   # ``keep`` holds the buffer for the calls below
    assert lib.nlam_grad_sumsq(None, 10, addr, 1, 1.0, None, None) == -1
    assert lib.nlam_grad_sumsq(addr, 10, None, 1, 1.0, None, None) == -1
    assert lib.nlam_grad_sumsq(addr, -1, addr, 1, 1.0, None, None) == -1
    assert lib.nlam_grad_sumsq(addr, 10, addr, 0, 1.0, None, None) == -1            # workspace too small
    assert lib.nlam_grad_sumsq(addr, 5_000_000, addr, 255, 1.0, None, None) == -1
    assert lib.nlam_grad_sumsq(addr + 2, 10, addr, 1, 1.0, None, None) == -1        # not a float address
    assert lib.nlam_adamw_step_controlled(None, None) == -1
    for bad in (dict(param=None), dict(grad=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(step_count_dev=None),
                dict(bias_corr_dev=None), dict(partials=None), dict(control=None), dict(n=-1), dict(partials_doubles=0),
                dict(schedule=4), dict(schedule=-1), dict(schedule=1, warmup_steps=-1), dict(schedule=2, total_steps=-1),
                dict(schedule=0, warmup_steps=3), dict(min_ratio=1.5), dict(min_ratio=-0.1), dict(max_grad_norm=float("nan"))):
        assert lib.nlam_adamw_step_controlled(C.byref(_ctl(addr, **bad)), None) == -1, bad


def test_trainer_refuses_controls_for_a_foreign_optimizer():
    from neural_lam_amd import ops
    from neural_lam_amd.trainer import Trainer

    class Sgd:
        def __init__(self, p, g):
            self.p, self.g = p, g

        def step(self, scale):
            self.p.sub_(self.g * scale)

    for kw in (dict(max_grad_norm=1.0), dict(lr_schedule=ops.LRSchedule("constant", 3)), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="AdamWFlat"):
            Trainer(torch.nn.Linear(3, 2), optimizer_factory=Sgd, **kw)


def test_controls_are_fixed_at_construction():
    """They are constants of a captured control launch: an assignment a replay would ignore must not be accepted silently."""
    from neural_lam_amd import ops

    sch = ops.LRSchedule("warmup_cosine", warmup_steps=2, total_steps=9, min_ratio=0.1)
    for k, v in (("kind", "constant"), ("warmup_steps", 5), ("total_steps", 20), ("min_ratio", 0.5)):
        with pytest.raises(AttributeError):
            setattr(sch, k, v)
    assert sch.state_dict() == dict(kind="warmup_cosine", warmup_steps=2, total_steps=9, min_ratio=0.1)
    p, g = torch.zeros(8), torch.zeros(8)
    opt = ops.AdamWFlat(p, g, max_grad_norm=2.0, lr_schedule=sch, skip_nonfinite=True)
    assert (opt.max_grad_norm, opt.lr_schedule, opt.skip_nonfinite, opt.controlled) == (2.0, sch, True, True)
    plain = ops.AdamWFlat(p, g)
    assert (plain.max_grad_norm, plain.lr_schedule, plain.skip_nonfinite, plain.controlled) == (None, None, False, False)
    for o in (opt, plain):
        for k, v in (("max_grad_norm", 1.0), ("lr_schedule", None), ("skip_nonfinite", False), ("controlled", False)):
            with pytest.raises(AttributeError):
                setattr(o, k, v)
    opt.lr = 5e-4   # the hand-set rate stays assignable (Trainer watches it)
    assert opt.lr == 5e-4


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _ulps(got, want):
    """|got - want| in units of fp32 spacing at ``want``."""
    got, want = np.float32(got), np.float32(want)
    return float(abs(np.float64(got) - np.float64(want)) / np.float64(np.spacing(np.abs(want))))


def _wide_range(n, seed):
    """Gradients spanning ten orders of magnitude."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 10.0 - 6.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 100_003, 4_194_304, 5_000_001])
def test_grad_norm_matches_float64(dev, n):
    from neural_lam_amd import ops

    x = _wide_range(n + 1, seed=n)
    xd = x.to(dev)
    for lo, scale in ((0, 1.0), (1, 0.5)):   # lo = 1: a view that does not start on a 16-byte boundary
        view_h, view_d = x[lo : lo + n], xd[lo : lo + n]
        want = np.float32(scale * math.sqrt(float(view_h.double().square().sum())))
        a = ops.global_grad_norm(view_d, scale)
        b = ops.global_grad_norm(view_d, scale)
        assert a.shape == () and a.dtype == torch.float32 and a.device.type == "cuda"
        u = _ulps(a.item(), want)
        print(f"n = {n}, offset {lo}: norm {a.item():.9g}, float64 {want:.9g}, {u:.2f} ulp")
        assert u <= 1.0, (n, lo, a.item(), want)
        assert torch.equal(a, b)   # fixed-order fp64 sums: the same bits on every run


@pytest.mark.gpu
def test_grad_norm_of_nonfinite_buffers_is_nonfinite(dev):
    from neural_lam_amd import ops

    for bad in (float("inf"), float("-inf"), float("nan")):
        for n, where in ((7, 6), (100_003, 50_001), (100_003, 100_002)):
            x = torch.randn(n)
            x[where] = bad
            assert not math.isfinite(ops.global_grad_norm(x.to(dev)).item()), (bad, n, where)
    assert ops.global_grad_norm(torch.zeros(1000, device=dev)).item() == 0.0


def _grads(n, steps, dev, seed=0, spread=True):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g) * (10.0 ** (k % 3 - 1) if spread else 1.0)).to(dev) for k in range(steps)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [10_001, 4096, 3])
def test_controlled_update_with_unit_coefficient_equals_resident_update_bit_for_bit(dev, n):
    """max_grad_norm so large that the coefficient is 1, a constant schedule: x * 1.0f is exact, so parameters and both
    moments carry the bits of nlam_adamw_step_resident after every one of five steps."""
    from neural_lam_amd import ops

    torch.manual_seed(1)
    p0 = torch.randn(n, device=dev)
    pa, pb = p0.clone(), p0.clone()
    ga, gb = torch.zeros_like(pa), torch.zeros_like(pb)
    plain = ops.AdamWFlat(pa, ga, lr=1e-3)
    ctl = ops.AdamWFlat(pb, gb, lr=1e-3, max_grad_norm=1e30, lr_schedule=ops.LRSchedule("constant"), skip_nonfinite=True)
    for k, grad in enumerate(_grads(n, 5, dev)):
        ga.copy_(grad)
        gb.copy_(grad)
        plain.step(0.5)
        ctl.step(0.5)
        assert torch.equal(pa, pb) and torch.equal(plain.m, ctl.m) and torch.equal(plain.v, ctl.v), k
        assert torch.equal(plain.t_dev, ctl.t_dev) and torch.equal(plain.bc_dev, ctl.bc_dev), k
        assert ctl.clip_coef.item() == 1.0 and ctl.last_lr.item() == float(np.float32(1e-3))
    assert ctl.skipped_steps == 0 and ctl.step_count() == 5


@pytest.mark.gpu
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clipped_scheduled_update_matches_torch(dev, grad_scale):
    """clip_grad_norm_ + torch.optim.AdamW + LambdaLR on the averaged gradient, at test_fused_adamw_matches_torch's bar; the
    coefficient and lr_t read back from the device against the host formulas (1 ulp of fp32)."""
    from neural_lam_amd import ops

    n, lr, max_norm = 10_001, 1e-3, 40.0
    sch = ops.LRSchedule("warmup_cosine", warmup_steps=3, total_steps=7, min_ratio=0.1)
    torch.manual_seed(0)
    p = torch.randn(n, device=dev)
    ref_p = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([ref_p], lr=lr, betas=(0.9, 0.95))
    lam = torch.optim.lr_scheduler.LambdaLR(opt, sch.factor)
    g = torch.zeros_like(p)
    mine = ops.AdamWFlat(p, g, lr=lr, max_grad_norm=max_norm, lr_schedule=sch)
    coefs = []
    for s, grad in enumerate(_grads(n, 9, dev, seed=3)):   # norms ~ 10 / scale, 100 / scale, 1000 / scale in turn
        g.copy_(grad)
        ref_p.grad = grad.clone() * grad_scale
        ref_norm = torch.nn.utils.clip_grad_norm_([ref_p], max_norm)
        opt.step()
        lam.step()
        mine.step(grad_scale)
        norm, coef, lr_t = mine.grad_norm.item(), mine.clip_coef.item(), mine.last_lr.item()
        want_norm = np.float32(grad_scale * math.sqrt(float(grad.double().square().sum())))
        want_coef = min(np.float32(1.0), np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6)))
        want_lr = np.float32(float(np.float32(lr)) * sch.factor(s))
        print(f"step {s}: norm {norm:.9g} ({_ulps(norm, want_norm):.2f} ulp), coefficient {coef:.9g} ({_ulps(coef, want_coef):.2f} ulp), "
              f"lr_t {lr_t:.9g} ({_ulps(lr_t, want_lr):.2f} ulp)")
        assert _ulps(norm, want_norm) <= 1.0 and _ulps(coef, want_coef) <= 1.0 and _ulps(lr_t, want_lr) <= 1.0, s
        assert abs(norm - float(ref_norm)) <= 1e-5 * float(ref_norm)
        coefs.append(coef)
    assert min(coefs) < 0.5 and max(coefs) == 1.0   # clipping was active on some steps and idle on others
    assert rel_err(p.cpu(), ref_p.detach().cpu()) < 1e-5


# ---- Trainer: the small golden-size GraphLAM against the oracle ----
def _datastore(tmp_path):
    from neural_lam_amd.datastore import SyntheticDatastore

    return SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)


def _graph(ds):
    from neural_lam_amd import graph as G

    ext = ds.get_xy_extent("state")
    return G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state")), max(ext[1] - ext[0], ext[3] - ext[2]))


def _oracle_fc(ds, graph, seed=7):
    from oracle import models as om

    torch.manual_seed(seed)
    return om.ARForecaster(om.GraphLAM(ds, graph, hidden_dim=16, processor_layers=2), ds)


def _hip_step(ds, graph, o_fc):
    from neural_lam_amd import models as hm

    h_fc = hm.ARForecaster(hm.GraphLAM(ds, graph=graph, hidden_dim=16, processor_layers=2), ds)
    h_fc.load_state_dict(o_fc.state_dict())
    return h_fc, hm.ForecasterStep(h_fc, ds)


STEPS, MAX_NORM, LR = 6, 10.0, 1e-3
OFFSET = 10.0   # added to every other batch's target: a coherent error, whose gradient norm lies far above MAX_NORM (a target
                # merely scaled up adds incoherently and hardly moves the norm); the other batches' norms lie below it


def _schedule():
    from neural_lam_amd import ops

    return ops.LRSchedule("warmup_cosine", warmup_steps=3, total_steps=STEPS, min_ratio=0.1)


def _traj_batches(ds, n=STEPS, T=2, seed=8):
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        init, target, forcing = (torch.randn(1, 2, N, 5, generator=g), torch.randn(1, T, N, 5, generator=g),
                                 torch.randn(1, T, N, 6, generator=g))
        out.append((init, target + (OFFSET if k % 2 else 0.0), forcing))
    return out


def _oracle_run(ds, graph, batches, controls, clip=True):
    """The oracle model under torch: clip_grad_norm_ + AdamW + LambdaLR (``controls``; ``clip=False``: the norm is only
    measured) or plain AdamW."""
    from oracle import models as om

    o_fc = _oracle_fc(ds, graph)
    pvs, mask = om.per_var_std_uniform(ds), om.interior_mask_bool(ds)
    opt = torch.optim.AdamW(o_fc.parameters(), lr=LR, betas=(0.9, 0.95))
    lam = torch.optim.lr_scheduler.LambdaLR(opt, _schedule().factor) if controls else None
    losses, norms = [], []
    for b in batches:
        opt.zero_grad(set_to_none=True)
        _, loss = om.training_loss(o_fc, b, pvs, mask)
        loss.backward()
        if controls:
            norms.append(float(torch.nn.utils.clip_grad_norm_(o_fc.parameters(), MAX_NORM if clip else float("inf"))))
        opt.step()
        if controls:
            lam.step()
        losses.append(float(loss.detach()))
    return o_fc, losses, norms


def test_oracle_trajectory_depends_on_clipping_and_schedule(tmp_path):
    """CPU: the batches of the trajectory test make the controls matter.  The norms alternate below and far above
    MAX_NORM, and the clipped-and-scheduled weights differ from plain AdamW's by at least ten times the bar the GPU test
    holds the product to -- a product that ignored the options could not pass it."""
    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = _traj_batches(ds)
    with_c, _, norms = _oracle_run(ds, graph, batches, True)
    plain, _, _ = _oracle_run(ds, graph, batches, False)
    print("oracle gradient norms:", [f"{x:.4g}" for x in norms])
    assert all(x < 0.8 * MAX_NORM for x in norms[0::2]) and all(x > 5 * MAX_NORM for x in norms[1::2]), norms
    a, b = with_c.state_dict(), plain.state_dict()
    worst = max(float((a[k] - b[k]).abs().max()) for k in a if a[k].numel())
    print(f"clipped + scheduled against plain AdamW: largest weight difference {worst:.3e}")
    assert worst >= 10 * WEIGHT_BAR
    # and the clipping on its own (Adam ignores a constant gradient scale, not an alternating one)
    unclipped, _, _ = _oracle_run(ds, graph, batches, True, clip=False)
    c = unclipped.state_dict()
    worst_clip = max(float((a[k] - c[k]).abs().max()) for k in a if a[k].numel())
    print(f"clipped + scheduled against scheduled only: largest weight difference {worst_clip:.3e}")
    assert worst_clip >= 10 * WEIGHT_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("executor", ["forks", "segments"])
def test_trainer_trajectory_with_clipping_and_schedule_matches_oracle(dev, tmp_path, executor):
    from neural_lam_amd.trainer import Trainer

    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = _traj_batches(ds)
    o_fc, o_losses, o_norms = _oracle_run(ds, graph, batches, True)
    plain, _, _ = _oracle_run(ds, graph, batches, False)
    a, b = o_fc.state_dict(), plain.state_dict()
    assert max(float((a[k] - b[k]).abs().max()) for k in a if a[k].numel()) >= 10 * WEIGHT_BAR
    assert min(o_norms) < MAX_NORM < max(o_norms)

    h_fc, step = _hip_step(ds, graph, _oracle_fc(ds, graph))
    tr = Trainer(step.to(dev), lr=LR, use_graph=True, executor=executor, max_grad_norm=MAX_NORM, lr_schedule=_schedule())
    graphs = []
    for it, bt in enumerate(batches):
        loss = float(tr.step(*(t.to(dev) for t in bt)))
        norm, lr_t = float(tr.grad_norm), float(tr.last_lr)
        print(f"step {it}: loss {loss:.7g} (oracle {o_losses[it]:.7g}), grad norm {norm:.7g} (oracle {o_norms[it]:.7g}), lr {lr_t:.4g}")
        assert abs(loss - o_losses[it]) < TOL * abs(o_losses[it]), it
        assert abs(norm - o_norms[it]) < TOL * abs(o_norms[it]), it
        assert _ulps(lr_t, np.float32(float(np.float32(LR)) * _schedule().factor(it))) <= 1.0, it
        graphs.append((tr._graph, tr._tail_graph, getattr(tr._graph, "tail", None)))
    # the optimizer never left the captured step and nothing was recorded a second time
    assert tr._graph is not None and not tr._opt_eager and tr._opt_changes == 0
    assert tr._opt_in_graph or tr._tail_graph is not None
    if executor == "segments":
        assert tr._graph.tail is not None
    assert all(g[0] is graphs[0][0] and g[1] is graphs[0][1] and g[2] is graphs[0][2] for g in graphs)
    assert tr.global_step == STEPS and tr.skipped_steps == 0
    o_sd = o_fc.state_dict()
    for k, v in h_fc.state_dict().items():
        if v.numel():
            assert float((v.cpu() - o_sd[k]).abs().max()) < WEIGHT_BAR, k


def _small_trainer(ds, graph, dev, mode, **kw):
    from neural_lam_amd.trainer import Trainer

    modes = {"eager": dict(use_graph=False), "forks": dict(use_graph=True, executor="forks"),
             "segments": dict(use_graph=True, executor="segments")}
    _, step = _hip_step(ds, graph, _oracle_fc(ds, graph))
    return Trainer(step.to(dev), lr=LR, **modes[mode], **kw)


def _state(tr):
    o = tr.opt
    return {k: v.clone() for k, v in dict(flat=tr.fp.flat, m=o.m, v=o.v, t=o.t_dev, bc=o.bc_dev).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "forks", "segments"])
def test_nonfinite_step_is_skipped_and_leaves_no_trace(dev, tmp_path, mode):
    """One inf in a target makes the loss and every gradient non-finite (plain arithmetic, nothing else): parameters, both
    moments, the step count and the bias corrections keep their bits, the counter says 1, and the next clean step equals the
    step of a twin that never saw the bad batch."""
    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = [tuple(t.to(dev) for t in b) for b in _traj_batches(ds, n=4)]
    kw = dict(skip_nonfinite=True, max_grad_norm=MAX_NORM, lr_schedule=_schedule())
    a, twin = _small_trainer(ds, graph, dev, mode, **kw), _small_trainer(ds, graph, dev, mode, **kw)
    for b in batches[:2]:
        assert float(a.step(*b)) == float(twin.step(*b))
    before = _state(a)
    bad = [t.clone() for t in batches[2]]
    interior = int(np.flatnonzero(1.0 - np.asarray(ds.boundary_mask.values).reshape(-1))[0])   # a node the loss counts
    bad[1][0, 1, interior, 2] = float("inf")
    loss = a.step(*bad)
    assert not math.isfinite(float(loss)) and not math.isfinite(float(a.grad_norm))
    after = _state(a)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert a.skipped_steps == 1 and a.global_step == 2 and float(a.opt.clip_coef) == 0.0
    la, lt = float(a.step(*batches[3])), float(twin.step(*batches[3]))
    assert la == lt and math.isfinite(la)
    sa, st = _state(a), _state(twin)
    for k in sa:
        assert torch.equal(sa[k], st[k]), k
    assert bool(torch.isfinite(a.fp.flat).all()) and a.skipped_steps == 1 and twin.skipped_steps == 0 and a.global_step == 3
    assert torch.equal(a.last_lr, twin.last_lr)
    if mode != "eager":
        assert a._graph is not None and not a._opt_eager and a._opt_changes == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "forks", "segments"])
def test_resume_mid_warmup_is_bit_identical(dev, tmp_path, mode):
    """A: 5 steps.  B: 2 steps (inside the 3-step warm-up), saved.  C: a fresh trainer loading B's file, 3 steps.  C's
    losses, weights, moments and step count equal A's bit for bit; the file holds the scheduled lr, the base lr, the
    schedule and the skipped-steps count."""
    from neural_lam_amd import checkpoint as ck

    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = [tuple(t.to(dev) for t in b) for b in _traj_batches(ds, n=5)]
    kw = dict(skip_nonfinite=True, max_grad_norm=MAX_NORM, lr_schedule=_schedule())
    a = _small_trainer(ds, graph, dev, mode, **kw)
    la = [float(a.step(*b)) for b in batches]
    b_ = _small_trainer(ds, graph, dev, mode, **kw)
    lb = [float(b_.step(*b)) for b in batches[:2]]
    assert lb == la[:2]
    path = tmp_path / "b.ckpt"
    made = ck.save_checkpoint(path, b_, epoch=0, global_step=b_.global_step)
    group = made["optimizer_states"][0]["param_groups"][0]
    assert made["global_step"] == 2
    assert group["lr"] == LR * _schedule().factor(2) and group["initial_lr"] == LR
    controls = made["neural_lam_amd"]["optimizer_controls"]
    assert controls == dict(base_lr=LR, lr_schedule=_schedule().state_dict(), max_grad_norm=MAX_NORM, skip_nonfinite=True,
                            skipped_steps=0)
    c = _small_trainer(ds, graph, dev, mode, **kw)
    with torch.no_grad():
        c.fp.flat.mul_(1.5)
    ck.load_checkpoint(path, c)
    assert c.opt.lr == LR and c.global_step == 2
    lc = [float(c.step(*b)) for b in batches[2:]]
    assert lc == la[2:]
    sa, sc = _state(a), _state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert torch.equal(a.last_lr, c.last_lr) and a.global_step == c.global_step == 5
    if mode != "eager":
        assert c._graph is not None and not c._opt_eager and c._opt_changes == 0


@pytest.mark.gpu
def test_checkpoint_without_controls_loads_into_a_controlled_trainer(dev, tmp_path):
    """A checkpoint written by a trainer without the options loads as before: step count, moments and the group's lr."""
    from neural_lam_amd import checkpoint as ck

    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = [tuple(t.to(dev) for t in b) for b in _traj_batches(ds, n=2)]
    old = _small_trainer(ds, graph, dev, "eager")
    for b in batches:
        old.step(*b)
    made = ck.save_checkpoint(None, old, epoch=0, global_step=2)
    assert "optimizer_controls" not in made["neural_lam_amd"] and "initial_lr" not in made["optimizer_states"][0]["param_groups"][0]
    new = _small_trainer(ds, graph, dev, "eager", max_grad_norm=MAX_NORM, skip_nonfinite=True)
    ck.load_checkpoint(made, new)
    assert new.global_step == 2 and new.opt.lr == LR and new.skipped_steps == 0
    assert torch.equal(new.fp.flat, old.fp.flat) and torch.equal(new.opt.m, old.opt.m) and torch.equal(new.opt.v, old.opt.v)


# ---- a one-rank process group gives the bits of no group ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _group_run(dev):
    from neural_lam_amd import gnn_layers as hl
    from neural_lam_amd import ops
    from neural_lam_amd.trainer import Trainer

    torch.manual_seed(0)
    ei = torch.stack([torch.randint(0, 60, (900,)), torch.randint(0, 50, (900,))])
    ei[1, -1] = 49

    class Step(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net = hl.InteractionNet(ei, 64)

        def forward(self, send, rec, edge):
            r, e = self.net(send, rec, edge)
            return (r.square().mean() + e.square().mean(),)

    trainer = Trainer(Step().to(dev), lr=1e-2, use_graph=True, max_grad_norm=0.5, skip_nonfinite=True,
                      lr_schedule=ops.LRSchedule("warmup_linear", warmup_steps=2, total_steps=4, min_ratio=0.2))
    batch = tuple(torch.randn(1, n, 64, device=dev) for n in (60, 50, 900))
    losses, norms = [], []
    for _ in range(4):
        losses.append(float(trainer.step(*batch)))
        norms.append(float(trainer.grad_norm))
    torch.cuda.synchronize()
    return {"losses": losses, "norms": norms, "flat": trainer.fp.flat.cpu(), "m": trainer.opt.m.cpu(), "v": trainer.opt.v.cpu(),
            "t": trainer.global_step, "graph": trainer._graph is not None, "world": trainer.world}


def _rccl_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)   # "nccl" is RCCL on ROCm
    warm = torch.ones(8, device=dev)
    dist.all_reduce(warm)   # communicator + watchdog thread are live before the capture
    torch.save(_group_run(dev), f"{out_dir}/group.pt")
    dist.destroy_process_group()


@pytest.mark.gpu
def test_one_rank_process_group_gives_the_bits_of_no_group(dev, tmp_path):
    mp.spawn(_rccl_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    grouped = torch.load(tmp_path / "group.pt", weights_only=False)
    alone = _group_run(dev)
    assert grouped["graph"] and alone["graph"] and grouped["world"] == alone["world"] == 1
    assert grouped["losses"] == alone["losses"] and grouped["norms"] == alone["norms"] and grouped["t"] == alone["t"] == 4
    assert max(alone["norms"]) > 0.5   # clipping was active
    for k in ("flat", "m", "v"):
        assert torch.equal(grouped[k], alone[k]), k
