"""An exponential moving average of the weights kept by the AdamW update launch inside the captured step
(``Trainer(ema_decay=...)``, ``ops.AdamWFlat(ema_decay=...)``; ``nlam_adamw_step_resident_ema``,
``nlam_adamw_step_controlled_ema`` and ``nlam_flat_swap`` underneath): Lightning's ``EMAWeightAveraging`` over
``torch.optim.swa_utils.AveragedModel`` -- untouched by a skipped step and by the micro-batches inside a window, evaluated
under ``ema_weights()``, carried by the checkpoint."""
import ctypes as C
import math
import os
import re
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from neural_lam_amd import _lib as L

TOL = 1e-4           # the bars of tests/test_grad_accumulation.py and tests/test_optimizer_controls.py: losses, relative ...
WEIGHT_BAR = 2e-4    # ... and final weights, absolute
NEW_EXPORTS = ["nlam_adamw_step_resident_ema", "nlam_adamw_step_controlled_ema", "nlam_flat_swap"]
FAKE = 0x1000        # a non-null, aligned address for the argument checks where there is no GPU (nothing can launch there)

K, UPDATES, MAX_NORM, LR = 2, 6, 10.0, 1e-3
OFFSET = 10.0
OFFSET_ON = [0, 0, 1, 1, 0, 0, 1, 1]   # both micro-batches of every second window carry the coherent error
DECAY = 0.9
W32 = float(np.float32(1.0) - np.float32(DECAY))   # the weight the kernels use: 1.0f - decay, rounded once
EPS24 = 2.0 ** -24
SIZES = [1, 3, 4096, 10_001]   # no quad at all, a tail only, whole quads exactly, quads and a tail


def _bound(u, p, ema):
    """Three fp32 roundings per averaged update (subtract, multiply, add) on values of the size of max(|p|, |ema|), each
    damped by ``decay`` afterwards: 4 u 2^-24 max(|p|, |ema|) after u updates (float64 tensors in, float64 out)."""
    return 4.0 * u * EPS24 * torch.maximum(p.abs(), ema.abs())


def _ema64(avg, p, u, start, lerp_first=False):
    """One step of the float64 recurrence: ``avg`` (float64) behind applied update ``u`` that left the parameters ``p``."""
    p = p.double()
    if u < start:
        return avg
    if u == start and not lerp_first:
        return p.clone()
    return avg + W32 * (p - avg)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_ema_struct_matches_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
        'int main(){printf("%zu %zu %zu %zu %d\\n", sizeof(nlam_ema_t), offsetof(nlam_ema_t, ema),'
        " offsetof(nlam_ema_t, decay), offsetof(nlam_ema_t, start_step), NLAM_ABI_VERSION); return 0;}\n"
    )
    exe = tmp_path / "sz"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(L.Ema), L.Ema.ema.offset, L.Ema.decay.offset, L.Ema.start_step.offset, L.ABI_VERSION]


def _address():
    """Where the rejected calls point: with a GPU present a real buffer, so that a validation that let one through would
    write into this test's own memory, not launch on a wild pointer."""
    if not torch.cuda.is_available():
        return None, FAKE
    buf = torch.zeros(4096, device="cuda", dtype=torch.float32)
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


def _acc(addr, steps=2, loss=None):
    a = L.Accum()
    a.accum, a.loss, a.steps = addr, loss, steps
    return a


def _ema(addr, decay=DECAY, start=1):
    e = L.Ema()
    e.ema, e.decay, e.start_step = addr, decay, start
    return e


BAD_EMA = [dict(addr=None), dict(off=2), dict(decay=1.0), dict(decay=-0.1), dict(decay=1.5), dict(decay=float("nan")),
           dict(start=0), dict(start=-2)]


def test_entry_points_are_declared_exported_and_reject_bad_arguments_without_a_gpu():
    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.nlam_abi_version() == L.ABI_VERSION == 8
    keep, addr = _address()   # ``keep`` holds the buffer for the calls below
    good = _ctl(addr)

    def resident(e, **kw):
        a = dict(param=addr, grad=addr, m=addr, v=addr, n=1000, t=addr, bc=addr)
        a.update(kw)
        return lib.nlam_adamw_step_resident_ema(a["param"], a["grad"], a["m"], a["v"], a["n"], 1e-3, 0.9, 0.95, 1e-8, 1e-2, a["t"],
                                                a["bc"], 1.0, None, e)

    assert resident(None) == -1
    assert lib.nlam_adamw_step_controlled_ema(C.byref(good), None, None, None) == -1
    assert lib.nlam_adamw_step_controlled_ema(C.byref(good), C.byref(_acc(addr)), None, None) == -1
    for bad in BAD_EMA:
        where = None if "addr" in bad else addr + bad.get("off", 0)
        e = _ema(where, decay=bad.get("decay", DECAY), start=bad.get("start", 1))
        assert resident(C.byref(e)) == -1, bad
        assert lib.nlam_adamw_step_controlled_ema(C.byref(good), None, C.byref(e), None) == -1, bad
        assert lib.nlam_adamw_step_controlled_ema(C.byref(good), C.byref(_acc(addr)), C.byref(e), None) == -1, bad
    ok = _ema(addr)
    # whatever the entries without `_ema` reject
    for bad in (dict(param=None), dict(grad=None), dict(m=None), dict(v=None), dict(t=None), dict(bc=None), dict(n=-1)):
        assert resident(C.byref(ok), **bad) == -1, bad
    assert lib.nlam_adamw_step_controlled_ema(None, None, C.byref(ok), None) == -1
    for bad in (dict(param=None), dict(grad=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(step_count_dev=None),
                dict(bias_corr_dev=None), dict(partials=None), dict(control=None), dict(n=-1), dict(partials_doubles=0),
                dict(schedule=4), dict(schedule=0, warmup_steps=3), dict(min_ratio=1.5), dict(max_grad_norm=float("nan"))):
        assert lib.nlam_adamw_step_controlled_ema(C.byref(_ctl(addr, **bad)), None, C.byref(ok), None) == -1, bad
        assert lib.nlam_adamw_step_controlled_ema(C.byref(_ctl(addr, **bad)), C.byref(_acc(addr)), C.byref(ok), None) == -1, bad
    for bad in (_acc(None), _acc(addr, steps=0), _acc(addr + 2), _acc(addr, loss=addr + 1)):
        assert lib.nlam_adamw_step_controlled_ema(C.byref(good), C.byref(bad), C.byref(ok), None) == -1
    other = addr + 2048
    assert lib.nlam_flat_swap(None, other, 10, None) == -1
    assert lib.nlam_flat_swap(addr, None, 10, None) == -1
    assert lib.nlam_flat_swap(addr, other, -1, None) == -1
    assert lib.nlam_flat_swap(addr + 2, other, 10, None) == -1   # not a float address
    assert lib.nlam_flat_swap(addr, other + 1, 10, None) == -1
    assert lib.nlam_flat_swap(addr, other, 0, None) == 0         # nothing to exchange: no launch
    del keep


class _Sgd:
    def __init__(self, p, g):
        self.p, self.g = p, g

    def step(self, scale):
        self.p.sub_(self.g * scale)


def test_optimizer_and_trainer_argument_errors():
    from neural_lam_amd import ops
    from neural_lam_amd.trainer import Trainer

    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            ops.AdamWFlat(torch.zeros(8), torch.zeros(8), ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            Trainer(torch.nn.Linear(3, 2), ema_decay=bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="ema_start_step"):
            ops.AdamWFlat(torch.zeros(8), torch.zeros(8), ema_decay=DECAY, ema_start_step=bad)
        with pytest.raises(ValueError, match="ema_start_step"):
            Trainer(torch.nn.Linear(3, 2), ema_decay=DECAY, ema_start_step=bad)
    p = torch.arange(8.0)
    opt = ops.AdamWFlat(p, torch.zeros(8), ema_decay=DECAY, ema_start_step=3)
    assert opt.ema_decay == DECAY and opt.ema_start_step == 3 and not opt.controlled   # EMA alone keeps the resident path
    assert torch.equal(opt.ema, p) and opt.ema.data_ptr() != p.data_ptr()
    for name in ("ema_decay", "ema_start_step"):
        with pytest.raises(AttributeError):
            setattr(opt, name, 2)
    plain = ops.AdamWFlat(torch.zeros(8), torch.zeros(8))
    assert plain.ema is None and plain.ema_decay is None and plain.ema_start_step == 1
    assert ops.AdamWFlat(torch.zeros(8), torch.zeros(8), ema_decay=0.0).ema_decay == 0.0
    tr = Trainer(torch.nn.Linear(3, 2))
    for call in (tr.ema_state_dict, lambda: tr.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()


def test_trainer_refuses_weight_averaging_with_an_optimizer_factory():
    from neural_lam_amd.trainer import Trainer

    with pytest.raises(ValueError, match="options of the built-in AdamWFlat"):
        Trainer(torch.nn.Linear(3, 2), optimizer_factory=_Sgd, ema_decay=DECAY)
    tr = Trainer(torch.nn.Linear(3, 2), optimizer_factory=_Sgd)   # (ema_start_step alone asks for nothing)
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr.ema_state_dict()


# ---- the small golden-size GraphLAM against the oracle (the helpers of tests/test_grad_accumulation.py, restated) ----
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


def _schedule():
    from neural_lam_amd import ops

    return ops.LRSchedule("warmup_cosine", warmup_steps=2, total_steps=UPDATES, min_ratio=0.1)


def _micro_batches(ds, n=K * UPDATES, T=2, seed=8):
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        init, target, forcing = (torch.randn(1, 2, N, 5, generator=g), torch.randn(1, T, N, 5, generator=g),
                                 torch.randn(1, T, N, 6, generator=g))
        out.append((init, target + (OFFSET if OFFSET_ON[k % len(OFFSET_ON)] else 0.0), forcing))
    return out


def _named(fc):
    return {n: p.detach().clone() for n, p in fc.named_parameters()}


def _oracle_run(ds, graph, batches, skip_window=None):
    """The oracle GraphLAM under torch.optim.AdamW with clip_grad_norm_ and LambdaLR, K micro-batches per update with
    ``loss / K`` per backward, and ``AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(DECAY))`` updated behind every applied
    optimizer step (fp32, torch's own).  ``skip_window``: the window whose update is refused, as a non-finite norm refuses it
    (no optimizer step, no scheduler step, no averaging).  Returns the model, the averaged model, the losses and, per CALL,
    ``(closing, applied, parameters)`` -- the trajectory every EMA variant below is a function of."""
    from oracle import models as om
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    o_fc = _oracle_fc(ds, graph)
    pvs, mask = om.per_var_std_uniform(ds), om.interior_mask_bool(ds)
    opt = torch.optim.AdamW(o_fc.parameters(), lr=LR, betas=(0.9, 0.95))
    lam = torch.optim.lr_scheduler.LambdaLR(opt, _schedule().factor)
    avg = AveragedModel(o_fc, multi_avg_fn=get_ema_multi_avg_fn(DECAY))
    start = _named(o_fc)
    losses, calls = [], []
    opt.zero_grad(set_to_none=True)
    for it, b in enumerate(batches):
        _, loss = om.training_loss(o_fc, b, pvs, mask)
        (loss / K).backward()
        losses.append(float(loss.detach()))
        closing = it % K == K - 1
        applied = closing and it // K != skip_window
        if applied:
            torch.nn.utils.clip_grad_norm_(o_fc.parameters(), MAX_NORM)
            opt.step()
            lam.step()
            avg.update_parameters(o_fc)
        if closing:
            opt.zero_grad(set_to_none=True)
        calls.append((closing, applied, _named(o_fc)))
    return dict(fc=o_fc, avg=avg, start=start, losses=losses, calls=calls)


def _ema_of(run, variant="right", start=1):
    """The average in float64 along a recorded trajectory.  ``right``: behind every applied update.  Wrong on purpose:
    ``skipped`` (also behind a refused update), ``micro`` (behind every micro-batch), ``lerp`` (averaged, not copied, at the
    first averaged update).  Returns ``({name: float64 average}, count of applied updates)``."""
    avg = {n: p.double() for n, p in run["start"].items()}
    u = events = 0
    for closing, applied, params in run["calls"]:
        u += int(applied)
        if not {"right": applied, "lerp": applied, "skipped": closing, "micro": True}[variant]:
            continue
        events += 1
        count = u if variant in ("right", "lerp") else events   # (the wrong ones count what they average behind)
        for n, p in params.items():
            avg[n] = _ema64(avg[n], p, count, start, lerp_first=variant == "lerp")
    return avg, u


def _separation(right, wrong, params, u):
    """The largest difference of two averages in units of the bound the GPU tests hold the kernels to."""
    return max(float(((right[n] - wrong[n]).abs() / _bound(u, params[n].double(), right[n]).clamp_min(1e-300)).max()) for n in right)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """The oracle trajectory, computed once and shared (nothing changes it)."""
    ds = _datastore(tmp_path_factory.mktemp("oracle"))
    graph = _graph(ds)
    batches = _micro_batches(ds)
    run = _oracle_run(ds, graph, batches)
    return dict(ds=ds, graph=graph, batches=batches, **run)


def test_oracle_recipe_tells_the_right_average_from_three_wrong_ones(oracle):
    """CPU: torch's own fp32 ``AveragedModel`` agrees with the float64 restatement inside the kernels' bound, and the inputs of
    the GPU trajectory test tell the right average from three wrong ones.  Measured with exactly these inputs (largest
    difference over all parameters, in units of the bound 4 u 2^-24 max(|p|, |ema|)): torch's fp32 average against float64
    0.206; an average that also moves on a refused update 7.99e+04; one that moves on every micro-batch 7.72e+05; one that
    averages instead of copying at the first update 1.01e+06 -- each far above the 100 asked for."""
    ds, graph, batches = oracle["ds"], oracle["graph"], oracle["batches"]
    right, u = _ema_of(oracle)
    assert u == UPDATES
    final = oracle["calls"][-1][2]
    torch_avg = dict(oracle["avg"].module.named_parameters())
    own = max(float(((torch_avg[n].detach().double() - right[n]).abs() / _bound(u, final[n].double(), right[n]).clamp_min(1e-300)).max())
              for n in right)
    print(f"torch's fp32 AveragedModel against the float64 recurrence: {own:.3g} of the bound")
    assert own <= 1.0
    assert int(oracle["avg"].n_averaged) == UPDATES
    for variant in ("micro", "lerp"):
        sep = _separation(right, _ema_of(oracle, variant)[0], final, u)
        print(f"right average against '{variant}': {sep:.3g} of the bound")
        assert sep > 100.0, variant
    refused = _oracle_run(ds, graph, batches, skip_window=2)
    right_r, u_r = _ema_of(refused)
    assert u_r == UPDATES - 1 and int(refused["avg"].n_averaged) == UPDATES - 1
    sep = _separation(right_r, _ema_of(refused, "skipped")[0], refused["calls"][-1][2], u_r)
    print(f"right average against 'skipped': {sep:.3g} of the bound")
    assert sep > 100.0
    # a later start: untouched before it, a copy at it
    late, _ = _ema_of(oracle, start=3)
    third = oracle["calls"][K * 3 - 1][2]
    assert all(torch.equal(_ema_of(dict(oracle, calls=oracle["calls"][: K * 3]), start=3)[0][n], third[n].double()) for n in late)
    assert all(torch.equal(_ema_of(dict(oracle, calls=oracle["calls"][: K * 2]), start=3)[0][n], oracle["start"][n].double()) for n in late)


# ---------------------------------------------------------------------------
# GPU: the kernels
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_flat_swap_exchanges_exactly_and_twice_is_the_identity(dev, n):
    """From 16-byte aligned bases, from views one float into both buffers (a head in front of the quads) and from bases at
    different offsets within 16 bytes (no common quad: single elements only); the guards around the views keep their bits."""
    lib = L.load()
    g = torch.Generator().manual_seed(n)
    ha, hb = torch.randn(n + 8, generator=g), torch.randn(n + 8, generator=g)
    for la, lb in ((4, 4), (1, 1), (4, 1), (2, 3)):
        a, b = ha.to(dev), hb.to(dev)
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        va, vb = a[la : la + n], b[lb : lb + n]
        L.check(lib.nlam_flat_swap(va.data_ptr(), vb.data_ptr(), n, _stream()), "nlam_flat_swap")
        ga, gb = a.cpu(), b.cpu()
        assert torch.equal(ga[la : la + n], hb[lb : lb + n]) and torch.equal(gb[lb : lb + n], ha[la : la + n]), (n, la, lb)
        assert torch.equal(ga[:la], ha[:la]) and torch.equal(ga[la + n :], ha[la + n :]), (n, la, lb)
        assert torch.equal(gb[:lb], hb[:lb]) and torch.equal(gb[lb + n :], hb[lb + n :]), (n, la, lb)
        L.check(lib.nlam_flat_swap(va.data_ptr(), vb.data_ptr(), n, _stream()), "nlam_flat_swap")
        assert torch.equal(a.cpu(), ha) and torch.equal(b.cpu(), hb), (n, la, lb)


def _grads(n, count, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g) * 10.0 ** (k % 3 - 1)).to(dev) for k in range(count)]


PATHS = ["resident", "controlled", "accum2", "accum1"]


def _drive(path, n, dev, ema, start=1, bad_call=None, updates=6):
    """``updates`` updates of seeded gradients through one of the paths, from the same start whatever ``ema``: the state
    behind every CALL (a window of ``accum2`` is two calls).  ``accum1``: ``nlam_adamw_step_accum`` / ``_controlled_ema``
    with a window of one, called directly.  ``bad_call``: the call whose gradient holds an inf."""
    from neural_lam_amd import ops

    lib = L.load()
    torch.manual_seed(3)
    p, g = torch.randn(n, device=dev), torch.zeros(n, device=dev)
    kw = dict(lr=1e-2)
    if path != "resident":
        kw.update(max_grad_norm=2.0 * math.sqrt(n), lr_schedule=ops.LRSchedule("warmup_cosine", 2, 6, 0.1), skip_nonfinite=True)
    k_ = 2 if path == "accum2" else 1
    if ema:
        kw.update(ema_decay=DECAY, ema_start_step=start)
    opt = ops.AdamWFlat(p, g, accumulate=k_, **kw)
    assert opt.controlled == (path != "resident")
    words = torch.zeros(L.ACCUM_WORDS, device=dev, dtype=torch.int32)
    one = L.Accum()
    one.accum, one.steps = words.data_ptr(), 1
    out = [dict(p=p.clone(), ema=opt.ema.clone() if ema else None)]
    for it, grad in enumerate(_grads(n, updates * k_, dev, seed=n)):
        if it == bad_call:
            grad = grad.clone()
            grad[n // 2] = float("inf")
        if path == "accum1":
            g.copy_(grad)
            if ema:
                rc = lib.nlam_adamw_step_controlled_ema(C.byref(opt._optctl(0.5)), C.byref(one), C.byref(opt._ema_arg()), _stream())
            else:
                rc = lib.nlam_adamw_step_accum(C.byref(opt._optctl(0.5)), C.byref(one), _stream())
            L.check(rc, "nlam_adamw_step_accum / nlam_adamw_step_controlled_ema")
        elif path == "accum2":
            opt.begin()
            g.add_(grad)
            opt.step(0.5 / k_)
        else:
            g.copy_(grad)
            opt.step(0.5)
        st = dict(p=p.clone(), m=opt.m.clone(), v=opt.v.clone(), t=opt.t_dev.clone(), bc=opt.bc_dev.clone(),
                  ema=opt.ema.clone() if ema else None)
        if path != "resident":
            st["ctl"] = opt.ctl.clone()
        out.append(st)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("path", PATHS)
def test_update_bits_do_not_depend_on_the_average_and_the_average_follows_the_float64_recurrence(dev, path, n):
    on, off = _drive(path, n, dev, True), _drive(path, n, dev, False)
    k_ = 2 if path == "accum2" else 1
    avg = on[0]["p"].double()
    assert torch.equal(on[0]["ema"], on[0]["p"])
    worst = 0.0
    for call in range(1, len(on)):
        a, b = on[call], off[call]
        for name in b:
            if name != "ema":
                assert torch.equal(a[name], b[name]), (call, name)
        u = int(a["t"].item())
        if call % k_ != 0:   # a micro-batch inside a window: nothing moved
            assert torch.equal(a["ema"], on[call - 1]["ema"]) and torch.equal(a["p"], on[call - 1]["p"]), call
            continue
        assert u == call // k_
        avg = _ema64(avg, a["p"], u, 1)
        err, bound = (a["ema"].double() - avg).abs(), _bound(u, a["p"].double(), avg)
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (call, float((err / bound.clamp_min(1e-300)).max()))
        if u == 1:
            assert torch.equal(a["ema"], a["p"])   # the first averaged update copies
    print(f"{path}, n = {n}: the average is within {worst:.3g} of its bound")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("path", PATHS)
def test_average_starts_at_the_chosen_update(dev, path, n):
    k_ = 2 if path == "accum2" else 1
    run = _drive(path, n, dev, True, start=3)
    closed = run[::k_]   # the state at the start and behind every update
    for u in (1, 2):
        assert torch.equal(closed[u]["ema"], run[0]["p"]) and not torch.equal(closed[u]["p"], run[0]["p"]), u
    assert torch.equal(closed[3]["ema"], closed[3]["p"])
    avg = closed[3]["p"].double()
    for u in (4, 5, 6):
        avg = _ema64(avg, closed[u]["p"], u, 3)
        err, bound = (closed[u]["ema"].double() - avg).abs(), _bound(u, closed[u]["p"].double(), avg)
        assert bool((err <= bound).all()), u
        assert not torch.equal(closed[u]["ema"], closed[u]["p"]), u


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("start", [1, 3])
def test_refused_update_leaves_the_average_alone_and_is_not_counted(dev, n, start):
    """An inf in the gradient of the third call: nothing moves, and the FOURTH call is applied update 3 -- with
    ``ema_start_step=3`` it is the one that copies."""
    run = _drive("controlled", n, dev, True, start=start, bad_call=2)
    before, refused = run[2], run[3]
    for name in ("p", "m", "v", "t", "bc", "ema"):
        assert torch.equal(before[name], refused[name]), name
    assert int(refused["ctl"][L.OPTCTL_SKIPPED]) == 1 and int(refused["t"]) == 2
    avg = run[0]["p"].double()
    applied = [c for c in (1, 2, 4, 5, 6)]
    for u, call in enumerate(applied, start=1):
        assert int(run[call]["t"]) == u
        avg = _ema64(avg, run[call]["p"], u, start)
        if u < start:
            assert torch.equal(run[call]["ema"], run[0]["p"]), call
        elif u == start:
            assert torch.equal(run[call]["ema"], run[call]["p"]), call
        else:
            err, bound = (run[call]["ema"].double() - avg).abs(), _bound(u, run[call]["p"].double(), avg)
            assert bool((err <= bound).all()), call
            assert not torch.equal(run[call]["ema"], run[call]["p"]), call


# ---------------------------------------------------------------------------
# GPU: the trainer
# ---------------------------------------------------------------------------
MODES = ["eager", "forks", "segments"]
_RUNS = {}


def _small_trainer(ds, graph, dev, mode, **kw):
    from neural_lam_amd.trainer import Trainer

    modes = {"eager": dict(use_graph=False), "forks": dict(use_graph=True, executor="forks"),
             "segments": dict(use_graph=True, executor="segments")}
    h_fc, step = _hip_step(ds, graph, _oracle_fc(ds, graph))
    tr = Trainer(step.to(dev), lr=LR, **modes[mode], **kw)
    tr.forecaster = h_fc
    return tr


def _state(tr):
    o = tr.opt
    out = dict(flat=tr.fp.flat, m=o.m, v=o.v, t=o.t_dev, bc=o.bc_dev, grad=tr.fp.grad)
    if getattr(o, "ema", None) is not None:
        out["ema"] = o.ema
    return {k: v.clone() for k, v in out.items()}


def _controls():
    return dict(max_grad_norm=MAX_NORM, lr_schedule=_schedule(), accumulate_grad_batches=K)


def _on_device(batches, dev):
    return [tuple(t.to(dev) for t in b) for b in batches]


def _trajectory(oracle, dev, mode, ema):
    """The run of the trajectory test in one mode, with or without the average, made once."""
    if (mode, ema) not in _RUNS:
        kw = dict(ema_decay=DECAY) if ema else {}
        tr = _small_trainer(oracle["ds"], oracle["graph"], dev, mode, **_controls(), **kw)
        losses, graphs = [], []
        for bt in _on_device(oracle["batches"], dev):
            losses.append(float(tr.step(*bt)))
            graphs.append((tr._graph, tr._tail_graph, getattr(tr._graph, "tail", None)))
        _RUNS[(mode, ema)] = dict(tr=tr, losses=losses, graphs=graphs, state=_state(tr))
    return _RUNS[(mode, ema)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_trainer_average_matches_oracle_and_leaves_the_training_bits_alone(dev, oracle, mode):
    run, plain = _trajectory(oracle, dev, mode, True), _trajectory(oracle, dev, mode, False)
    tr = run["tr"]
    assert tr.global_step == UPDATES and tr.micro_step == 0 and tr.opt.controlled
    for it, loss in enumerate(run["losses"]):
        assert abs(loss - oracle["losses"][it]) < TOL * abs(oracle["losses"][it]), it
    # the raw training run does not know about the average
    assert run["losses"] == plain["losses"]
    for k, v in plain["state"].items():
        assert torch.equal(v, run["state"][k]), k
    if mode != "eager":
        # the optimizer never left the captured step and nothing was recorded a second time
        assert tr._graph is not None and not tr._opt_eager and tr._opt_changes == 0 and tr._opt_in_graph
        if mode == "segments":
            assert tr._graph.tail is not None
        first = run["graphs"][0]
        assert all(g[0] is first[0] and g[1] is first[1] and g[2] is first[2] for g in run["graphs"])
    want, u = _ema_of(oracle)
    final = oracle["calls"][-1][2]
    got, raw = tr.ema_state_dict(), tr.forecaster.state_dict()
    o_sd = oracle["fc"].state_dict()
    prefix = "forecaster."
    worst = 0.0
    for name, avg in want.items():
        assert float((raw[name].cpu() - o_sd[name]).abs().max()) < WEIGHT_BAR, name
        err = (got[prefix + name].double() - avg).abs()
        bar = _bound(u, final[name].double(), avg) + WEIGHT_BAR
        worst = max(worst, float((err / bar).max()))
        assert got[prefix + name].device.type == "cpu" and bool((err < bar).all()), name
    print(f"{mode}: the trainer's average is within {worst:.3g} of its bar")
    assert set(got) == set(tr.module.state_dict())
    for k, v in tr.module.state_dict().items():   # buffers as they are
        if k[len(prefix):] not in want:
            assert torch.equal(got[k], v.cpu()), k


@pytest.mark.gpu
def test_executors_agree_on_the_average_bit_for_bit(dev, oracle):
    runs = {mode: _trajectory(oracle, dev, mode, True) for mode in MODES}
    for mode in MODES[1:]:
        for k, v in runs["eager"]["state"].items():
            assert torch.equal(v, runs[mode]["state"][k]), (mode, k)


def _eval_tensors(res):
    return {k: getattr(res, k).clone() for k in ("prediction", "time_step_loss", "mean_loss", "entry_mse")}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_evaluation_under_the_averaged_weights(dev, oracle, mode):
    from neural_lam_amd.trainer import graphed_eval_step

    ds, graph = oracle["ds"], oracle["graph"]
    batches = _on_device(oracle["batches"][:5], dev)
    tr, twin = (_small_trainer(ds, graph, dev, mode, ema_decay=DECAY) for _ in range(2))   # (EMA alone: the resident path)
    assert not tr.opt.controlled
    for b in batches[:3]:
        assert float(tr.step(*b)) == float(twin.step(*b))
    held = batches[3]
    val_step = graphed_eval_step(tr.module, *held, phase="val")   # captured BEFORE the block
    out0, cap0 = _eval_tensors(tr.module.evaluate(*held)), _eval_tensors(val_step(*held))
    assert _same(out0, cap0)
    flat_ptr, ema_ptr = tr.fp.flat.data_ptr(), tr.opt.ema.data_ptr()
    raw, avg = tr.fp.flat.clone(), tr.opt.ema.clone()
    assert not torch.equal(raw, avg)
    ema_sd = tr.ema_state_dict()
    with tr.ema_weights():
        assert torch.equal(tr.fp.flat, avg) and torch.equal(tr.opt.ema, raw)
        assert (tr.fp.flat.data_ptr(), tr.opt.ema.data_ptr()) == (flat_ptr, ema_ptr)   # nothing was rebound
        inside, cap_in = _eval_tensors(tr.module.evaluate(*held)), _eval_tensors(val_step(*held))
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.step(*held)
        with pytest.raises(RuntimeError, match="ema_weights"):
            with tr.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.state_dict()
    _, fresh = _hip_step(ds, graph, _oracle_fc(ds, graph))
    fresh = fresh.to(dev)
    fresh.load_state_dict(ema_sd)
    want = _eval_tensors(fresh.evaluate(*held))
    assert _same(inside, want) and _same(cap_in, want)
    assert not torch.equal(inside["prediction"], out0["prediction"])
    out1, cap1 = _eval_tensors(tr.module.evaluate(*held)), _eval_tensors(val_step(*held))
    assert _same(out0, out1) and _same(cap0, cap1)
    assert torch.equal(tr.fp.flat, raw) and torch.equal(tr.opt.ema, avg)
    with pytest.raises(KeyError):   # an exception inside the block: the weights come back all the same
        with tr.ema_weights():
            raise KeyError("x")
    assert torch.equal(tr.fp.flat, raw) and torch.equal(tr.opt.ema, avg) and not tr._ema_swapped
    for b in batches[3:]:
        assert float(tr.step(*b)) == float(twin.step(*b))
    sa, sb = _state(tr), _state(twin)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    if mode != "eager":
        assert tr._graph is not None and tr._opt_in_graph and tr._opt_changes == 0


@pytest.mark.gpu
def test_entering_the_block_inside_an_accumulation_window_raises(dev, oracle):
    tr = _small_trainer(oracle["ds"], oracle["graph"], dev, "eager", ema_decay=DECAY, **_controls())
    tr.step(*_on_device(oracle["batches"][:1], dev)[0])
    before = _state(tr)
    with pytest.raises(RuntimeError, match="window"):
        with tr.ema_weights():
            pass
    after = _state(tr)
    assert all(torch.equal(before[k], after[k]) for k in before) and not tr._ema_swapped


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_checkpoint_carries_the_average_and_resumes_bit_identically(dev, oracle, tmp_path, mode):
    from neural_lam_amd import checkpoint as ck

    ds, graph = oracle["ds"], oracle["graph"]
    batches = _on_device(oracle["batches"], dev)
    kw = dict(skip_nonfinite=True, ema_decay=DECAY, ema_start_step=2, **_controls())
    a = _small_trainer(ds, graph, dev, mode, **kw)
    la = [float(a.step(*b)) for b in batches]
    b_ = _small_trainer(ds, graph, dev, mode, **kw)
    assert [float(b_.step(*b)) for b in batches[: 3 * K]] == la[: 3 * K]
    path = tmp_path / "b.ckpt"
    made = ck.save_checkpoint(path, b_, epoch=0, global_step=b_.global_step)
    entry = made["neural_lam_amd"]["ema"]
    assert made["global_step"] == 3 and entry["decay"] == DECAY and entry["start_step"] == 2
    names = [n for n, p in b_.module.named_parameters() if p.requires_grad]
    assert list(entry["state_dict"]) == names and all(t.device.type == "cpu" for t in entry["state_dict"].values())
    assert all(torch.equal(entry["state_dict"][n], b_.ema_state_dict()[n]) for n in names)
    plain = _small_trainer(ds, graph, dev, mode, skip_nonfinite=True, **_controls())
    assert set(made) == set(ck.save_checkpoint(None, plain, epoch=0, global_step=0))   # the reference-layout parts are the same
    c = _small_trainer(ds, graph, dev, mode, **kw)
    c.step(*batches[0])
    c.step(*batches[1])   # the fresh trainer has an average of its own when the checkpoint arrives
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ck.load_checkpoint(path, c)
    assert torch.equal(c.opt.ema, b_.opt.ema) and torch.equal(c.fp.flat, b_.fp.flat)
    assert [float(c.step(*b)) for b in batches[3 * K :]] == la[3 * K :]
    sa, sc = _state(a), _state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert a.global_step == c.global_step == UPDATES
    if mode != "forks":
        return
    # a checkpoint without an average into a trainer with one: the warning, and the average starts at the weights
    bare = tmp_path / "bare.ckpt"
    ck.save_checkpoint(bare, plain, epoch=0, global_step=0)
    d = _small_trainer(ds, graph, dev, mode, **kw)
    for b in batches[: 3 * K]:   # (one update behind the copy at ema_start_step = 2)
        d.step(*b)
    assert not torch.equal(d.opt.ema, d.fp.flat)
    with pytest.warns(UserWarning, match="no weight average"):
        ck.load_checkpoint(bare, d)
    assert torch.equal(d.opt.ema, d.fp.flat) and torch.equal(d.fp.flat, plain.fp.flat)
    # restore_opt=False: weights only, the average starts at them
    ck.load_checkpoint(path, d, restore_opt=False)
    assert torch.equal(d.opt.ema, d.fp.flat) and torch.equal(d.fp.flat, b_.fp.flat) and d.global_step == 0
    # other constants: the warning, this trainer's go on holding
    other = _small_trainer(ds, graph, dev, mode, skip_nonfinite=True, ema_decay=0.5, ema_start_step=2, **_controls())
    with pytest.warns(UserWarning, match="weight average"):
        ck.load_checkpoint(path, other)
    assert torch.equal(other.opt.ema, b_.opt.ema) and other.opt.ema_decay == 0.5
    # a checkpoint with an average into a trainer without one: ignored
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ck.load_checkpoint(path, plain)
    assert torch.equal(plain.fp.flat, b_.fp.flat) and plain.opt.ema is None and plain.global_step == 3


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

    trainer = Trainer(Step().to(dev), lr=1e-2, use_graph=True, max_grad_norm=0.5, skip_nonfinite=True, accumulate_grad_batches=2,
                      lr_schedule=ops.LRSchedule("warmup_linear", warmup_steps=2, total_steps=4, min_ratio=0.2), ema_decay=DECAY)
    pair = [tuple(torch.randn(1, n, 64, device=dev) for n in (60, 50, 900)) for _ in range(2)]
    losses = [float(trainer.step(*pair[it % 2])) for it in range(6)]
    torch.cuda.synchronize()
    return {"losses": losses, "flat": trainer.fp.flat.cpu(), "m": trainer.opt.m.cpu(), "v": trainer.opt.v.cpu(),
            "ema": trainer.opt.ema.cpu(), "t": trainer.global_step, "graph": trainer._graph is not None, "world": trainer.world}


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
    assert grouped["losses"] == alone["losses"] and grouped["t"] == alone["t"] == 3
    assert not torch.equal(alone["ema"], alone["flat"])
    for k in ("flat", "m", "v", "ema"):
        assert torch.equal(grouped[k], alone[k]), k
