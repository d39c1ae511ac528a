"""Gradient accumulation over micro-batches inside the captured step (``Trainer(accumulate_grad_batches=K)``,
``ops.AdamWFlat(accumulate=K)``; ``nlam_accum_begin`` and ``nlam_adamw_step_accum`` underneath): the head and the tail of the
step decide on the device whether a call opens or closes a window, so one recorded step serves every micro-step."""
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

from conftest import ROOT
from neural_lam_amd import _lib as L

TOL = 1e-4           # the bars of tests/test_optimizer_controls.py: losses and norms, relative ...
WEIGHT_BAR = 2e-4    # ... and final weights, absolute
NEW_EXPORTS = ["nlam_accum_begin", "nlam_adamw_step_accum"]
FAKE = 0x1000        # a non-null, aligned address for the argument checks where there is no GPU (nothing can launch there)

K, WINDOWS, MAX_NORM, LR = 2, 4, 10.0, 1e-3
OFFSET = 10.0
OFFSET_ON = [0, 0, 1, 1, 0, 0, 1, 1]   # both micro-batches of every second window carry the coherent error


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_accum_struct_matches_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
        'int main(){printf("%zu %zu %zu %zu %d\\n", sizeof(nlam_accum_t), offsetof(nlam_accum_t, accum),'
        " offsetof(nlam_accum_t, loss), offsetof(nlam_accum_t, steps), NLAM_ACCUM_WORDS); return 0;}\n"
    )
    exe = tmp_path / "sz"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(L.Accum), L.Accum.accum.offset, L.Accum.loss.offset, L.Accum.steps.offset, L.ACCUM_WORDS]
    assert (L.ACCUM_INDEX, L.ACCUM_HOLD, L.ACCUM_LOSS_SUM, L.ACCUM_WINDOW_LOSS) == (0, 1, 2, 3) and L.ACCUM_WORDS == 4


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


def test_entry_points_are_declared_exported_and_reject_bad_arguments_without_a_gpu():
    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.nlam_abi_version() == L.ABI_VERSION == 8
    keep, addr = _address()   # ``keep`` holds the buffer for the calls below
    assert lib.nlam_accum_begin(None, 10, addr, None) == -1
    assert lib.nlam_accum_begin(addr, 10, None, None) == -1
    assert lib.nlam_accum_begin(addr, -1, addr, None) == -1
    assert lib.nlam_accum_begin(addr + 2, 10, addr, None) == -1      # not a float address
    assert lib.nlam_accum_begin(addr, 10, addr + 2, None) == -1      # not a word address
    good = _ctl(addr)
    assert lib.nlam_adamw_step_accum(None, C.byref(_acc(addr)), None) == -1
    assert lib.nlam_adamw_step_accum(C.byref(good), None, None) == -1
    assert lib.nlam_adamw_step_accum(C.byref(good), C.byref(_acc(None)), None) == -1
    assert lib.nlam_adamw_step_accum(C.byref(good), C.byref(_acc(addr, steps=0)), None) == -1
    assert lib.nlam_adamw_step_accum(C.byref(good), C.byref(_acc(addr, steps=-3)), None) == -1
    assert lib.nlam_adamw_step_accum(C.byref(good), C.byref(_acc(addr + 2)), None) == -1
    assert lib.nlam_adamw_step_accum(C.byref(good), C.byref(_acc(addr, loss=addr + 1)), None) == -1
    # everything nlam_adamw_step_controlled rejects
    for bad in (dict(param=None), dict(grad=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(step_count_dev=None),
                dict(bias_corr_dev=None), dict(partials=None), dict(control=None), dict(n=-1), dict(partials_doubles=0),
                dict(schedule=4), dict(schedule=-1), dict(schedule=1, warmup_steps=-1), dict(schedule=2, total_steps=-1),
                dict(schedule=0, warmup_steps=3), dict(min_ratio=1.5), dict(min_ratio=-0.1), dict(max_grad_norm=float("nan"))):
        assert lib.nlam_adamw_step_accum(C.byref(_ctl(addr, **bad)), C.byref(_acc(addr)), None) == -1, bad


class _Sgd:
    def __init__(self, p, g):
        self.p, self.g = p, g

    def step(self, scale):
        self.p.sub_(self.g * scale)


def test_trainer_rejects_bad_window_lengths_and_a_captured_foreign_optimizer():
    from neural_lam_amd import ops
    from neural_lam_amd.trainer import Trainer

    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            Trainer(torch.nn.Linear(3, 2), optimizer_factory=_Sgd, accumulate_grad_batches=bad)
        with pytest.raises(ValueError, match="accumulate"):
            ops.AdamWFlat(torch.zeros(8), torch.zeros(8), accumulate=bad)
    with pytest.raises(ValueError, match="use_graph=False"):
        Trainer(torch.nn.Linear(3, 2), optimizer_factory=_Sgd, accumulate_grad_batches=2, use_graph=True)
    tr = Trainer(torch.nn.Linear(3, 2), optimizer_factory=_Sgd, accumulate_grad_batches=2)   # the host decides
    assert tr.accumulate_grad_batches == 2 and tr.micro_step == 0
    opt = ops.AdamWFlat(torch.zeros(8), torch.zeros(8), accumulate=3)
    assert opt.accumulate == 3 and opt.controlled and opt.micro_step == 0
    with pytest.raises(AttributeError):
        opt.accumulate = 2
    assert ops.AdamWFlat(torch.zeros(8), torch.zeros(8)).accumulate == 1


# ---- the small golden-size GraphLAM against the oracle (the inputs of tests/test_optimizer_controls.py) ----
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

    return ops.LRSchedule("warmup_cosine", warmup_steps=2, total_steps=WINDOWS, min_ratio=0.1)


def _micro_batches(ds, n=K * WINDOWS, T=2, seed=8, B=None):
    """``B``: batch size per micro-batch (default 1 everywhere)."""
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        b = 1 if B is None else B[k]
        init, target, forcing = (torch.randn(b, 2, N, 5, generator=g), torch.randn(b, T, N, 5, generator=g),
                                 torch.randn(b, T, N, 6, generator=g))
        out.append((init, target + (OFFSET if OFFSET_ON[k % len(OFFSET_ON)] else 0.0), forcing))
    return out


def _oracle_run(ds, graph, batches, variant="right"):
    """The oracle model under torch.optim.AdamW with clip_grad_norm_ and LambdaLR, K micro-batches per update with
    ``loss / K`` per backward -- or one of three wrong implementations: ``summed`` (gradients not averaged), ``every`` (an
    update per micro-batch), ``last`` (the gradient zeroed on every call: only the last micro-batch of a window counts)."""
    from oracle import models as om

    o_fc = _oracle_fc(ds, graph)
    pvs, mask = om.per_var_std_uniform(ds), om.interior_mask_bool(ds)
    opt = torch.optim.AdamW(o_fc.parameters(), lr=LR, betas=(0.9, 0.95))
    lam = torch.optim.lr_scheduler.LambdaLR(opt, _schedule().factor)
    losses, norms = [], []
    opt.zero_grad(set_to_none=True)
    for it, b in enumerate(batches):
        if variant == "last":
            opt.zero_grad(set_to_none=True)
        _, loss = om.training_loss(o_fc, b, pvs, mask)
        (loss if variant == "summed" else loss / K).backward()
        losses.append(float(loss.detach()))
        if variant == "every" or it % K == K - 1:
            norms.append(float(torch.nn.utils.clip_grad_norm_(o_fc.parameters(), MAX_NORM)))
            opt.step()
            lam.step()
            opt.zero_grad(set_to_none=True)
    return o_fc, losses, norms


def _worst(a, b):
    a, b = a.state_dict(), b.state_dict()
    return max(float((a[k] - b[k]).abs().max()) for k in a if a[k].numel())


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """The oracle trajectory, computed once and shared (nothing changes it)."""
    ds = _datastore(tmp_path_factory.mktemp("oracle"))
    graph = _graph(ds)
    batches = _micro_batches(ds)
    o_fc, losses, norms = _oracle_run(ds, graph, batches)
    return dict(ds=ds, graph=graph, batches=batches, fc=o_fc, losses=losses, norms=norms)


def test_oracle_trajectory_depends_on_how_the_window_is_accumulated(oracle):
    """CPU: the inputs of the GPU trajectory test tell a right accumulation from three wrong ones.  Measured with exactly
    these inputs: window norms 4.75 / 115.8 / 4.32 / 92.4; largest weight difference 1.9e-3 (summed), 5.5e-3 (an update per
    micro-batch), 3.3e-3 (last micro-batch only) -- the first is 9.5 x WEIGHT_BAR, hence 5 x and not 10 x."""
    ds, graph, batches, norms = oracle["ds"], oracle["graph"], oracle["batches"], oracle["norms"]
    print("oracle window norms:", [f"{x:.4g}" for x in norms])
    assert len(norms) == WINDOWS
    assert all(x < MAX_NORM for x in norms[0::2]) and all(x > MAX_NORM for x in norms[1::2]), norms
    for variant in ("summed", "every", "last"):
        wrong, _, _ = _oracle_run(ds, graph, batches, variant)
        worst = _worst(oracle["fc"], wrong)
        print(f"right accumulation against '{variant}': largest weight difference {worst:.3e}")
        assert worst >= 5 * WEIGHT_BAR, variant


# ---- two gloo ranks on the CPU ----
class _TorchAdamW:
    def __init__(self, flat_param, flat_grad, lr=1e-2):
        self.g = flat_grad
        self.p = torch.nn.Parameter(flat_param)  # shares storage with the flat buffer
        self.p.data = flat_param
        self.opt = torch.optim.AdamW([self.p], lr=lr, betas=(0.9, 0.95))

    def step(self, grad_scale):
        self.p.grad = self.g * grad_scale
        self.opt.step()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_edges():
    torch.manual_seed(0)  # identical replicas
    ei = torch.stack([torch.randint(0, 6, (20,)), torch.randint(0, 5, (20,))])
    ei[1, -1] = 4
    return ei


def _gloo_sample(rank, call):
    g = torch.Generator().manual_seed(100 + 10 * rank + call)   # a different sample per rank and micro-batch
    return (torch.randn(6, 8, generator=g), torch.randn(5, 8, generator=g), torch.randn(20, 8, generator=g))


def _gloo_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from neural_lam_amd.trainer import Trainer
    from oracle import gnn_layers as og

    ei = _gloo_edges()

    class Step(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net = og.InteractionNet(ei, 8)
            self.unused = torch.nn.Linear(3, 3)  # never gets a gradient: finish_step must still reduce it

        def forward(self, send, rec, edge):
            r, e = self.net(send, rec, edge)
            return (r.square().mean() + e.square().mean(),)

    trainer = Trainer(Step(), optimizer_factory=lambda p, g: _TorchAdamW(p, g), bucket_bytes=1024, accumulate_grad_batches=2)
    issued = []
    reduce_slice = trainer.buckets._reduce_slice

    def counting(s, e):
        issued.append((s, e))
        reduce_slice(s, e)

    trainer.buckets._reduce_slice = counting
    steps, micro = [], []
    for call in range(4):   # two windows of two micro-batches
        micro.append(trainer.micro_step)
        trainer.step(*_gloo_sample(rank, call))
        steps.append(trainer.opt.opt.state[trainer.opt.p]["step"].item() if trainer.opt.opt.state else 0)
    torch.save({"flat": trainer.fp.flat.clone(), "grad": trainer.fp.grad.clone(), "issued": issued, "steps": steps, "micro": micro,
                "nbuckets": len(trainer.buckets.bounds)}, f"{out_dir}/rank{rank}.pt")
    dist.destroy_process_group()


def test_two_rank_gloo_accumulation_matches_single_process_mean(tmp_path):
    world = 2
    mp.spawn(_gloo_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=False)
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["grad"], r1["grad"])   # replicas stay bit-identical
    assert r0["nbuckets"] > 1
    for r in (r0, r1):
        assert len(r["issued"]) == r["nbuckets"] * 2          # collectives per window, not per call
        assert r["steps"] == [0, 1, 1, 2] and r["micro"] == [0, 1, 0, 1]

    # single process: steps on the mean of the four losses of a window
    from neural_lam_amd.trainer import Trainer
    from oracle import gnn_layers as og

    ei = _gloo_edges()

    class Four(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net = og.InteractionNet(ei, 8)
            self.unused = torch.nn.Linear(3, 3)

        def forward(self, *samples):
            tot = 0.0
            for send, rec, edge in samples:
                r, e = self.net(send, rec, edge)
                tot = tot + r.square().mean() + e.square().mean()
            return (tot / len(samples),)

    ref = Trainer(Four(), optimizer_factory=lambda p, g: _TorchAdamW(p, g))
    for w in range(2):
        ref.step(*[_gloo_sample(rank, 2 * w + k) for rank in range(2) for k in range(2)])
    assert torch.allclose(ref.fp.flat, r0["flat"], rtol=1e-5, atol=1e-6)


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
    got, want = np.float32(got), np.float32(want)
    return float(abs(np.float64(got) - np.float64(want)) / np.float64(np.spacing(np.abs(want))))


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 4096, 10_001, 5_000_001])
def test_gated_zero(dev, n):
    """Word 0 == 0: the n elements become 0 and the guards around them keep their bits.  Word 0 == 1: nothing changes.
    From a 16-byte aligned base and from a view one element into a buffer (5 000 001 exceeds one sweep of the capped grid)."""
    lib = L.load()
    g = torch.Generator().manual_seed(n)
    host = torch.rand(n + 8, generator=g) + 0.5   # no zeros, no NaNs
    acc = torch.zeros(L.ACCUM_WORDS, device=dev, dtype=torch.int32)
    for lo in (4, 1):   # float offsets into a fresh allocation: 4 = a 16-byte boundary, 1 = not one
        for word0 in (1, 0):
            buf = host.to(dev)
            assert buf.data_ptr() % 16 == 0
            view = buf[lo : lo + n]
            acc[L.ACCUM_INDEX] = word0
            L.check(lib.nlam_accum_begin(view.data_ptr(), n, acc.data_ptr(), _stream()), "nlam_accum_begin")
            got = buf.cpu()
            if word0:
                assert torch.equal(got, host), (n, lo)
            else:
                assert not bool(got[lo : lo + n].any()), (n, lo)
                assert torch.equal(got[:lo], host[:lo]) and torch.equal(got[lo + n :], host[lo + n :]), (n, lo)
    assert acc.cpu().tolist() == [0, 0, 0, 0]   # the launch only reads the block


def _grads(n, steps, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g) * 10.0 ** (k % 3 - 1)).to(dev) for k in range(steps)]


def _opt_state(o):
    return {k: v.clone() for k, v in dict(p=o.p, m=o.m, v=o.v, t=o.t_dev, bc=o.bc_dev, ctl=o.ctl).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 4096, 10_001])
def test_accumulated_update_equals_one_update_on_the_summed_gradient_bit_for_bit(dev, n):
    from neural_lam_amd import ops

    k_, windows = 3, 3
    torch.manual_seed(1)
    p0 = torch.randn(n, device=dev)
    pa, pb = p0.clone(), p0.clone()
    ga, gb = torch.full_like(pa, 7.0), torch.zeros_like(pb)   # (the first gated zero has something to clear)
    # every window sums gradients of scale 0.1, 1 and 10: a norm near 10 sqrt(n) / 3 behind the 1 / K
    kw = dict(lr=1e-3, max_grad_norm=2.0 * math.sqrt(n), lr_schedule=ops.LRSchedule("warmup_linear", 2, 3, 0.1), skip_nonfinite=True)
    acc = ops.AdamWFlat(pa, ga, accumulate=k_, **kw)
    ref = ops.AdamWFlat(pb, gb, **kw)
    grads = _grads(n, k_ * windows, dev)
    losses = torch.rand(k_ * windows, generator=torch.Generator().manual_seed(5)).mul(3.0).to(dev)
    coefs = []
    for w in range(windows):
        gb.zero_()
        run = np.float32(0.0)
        for k in range(k_):
            it = w * k_ + k
            before = _opt_state(acc)
            assert acc.micro_step == k and acc.t == w
            acc.begin()
            ga.add_(grads[it])
            acc.step(1.0 / k_, loss=losses[it])
            gb.add_(grads[it])   # ((0 + g_1) + g_2) + g_3
            run = np.float32(run + np.float32(losses[it].item()))
            words = acc.acc.cpu().tolist()
            if k < k_ - 1:
                after = _opt_state(acc)
                for name in before:
                    assert torch.equal(before[name], after[name]), (w, k, name)
                assert words[L.ACCUM_INDEX] == k + 1 and words[L.ACCUM_HOLD] == 1
        ref.step(1.0 / k_)
        assert torch.equal(ga, gb), w
        a, b = _opt_state(acc), _opt_state(ref)
        for name in a:
            assert torch.equal(a[name], b[name]), (w, name)
        assert words[L.ACCUM_INDEX] == 0 and words[L.ACCUM_HOLD] == 0
        assert acc.micro_step == 0 and acc.t == w + 1 == acc.step_count()
        want = np.float32(run / np.float32(k_))
        assert np.float32(acc.window_loss.item()) == want, (w, acc.window_loss.item(), want)
        coefs.append(acc.clip_coef.item())
    if n > 3:
        assert max(coefs) < 1.0   # clipping was active


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 4096, 10_001])
def test_window_of_one_equals_the_controlled_update_bit_for_bit(dev, n):
    """steps == 1: nlam_adamw_step_accum is nlam_adamw_step_controlled."""
    from neural_lam_amd import ops

    lib = L.load()
    torch.manual_seed(2)
    p0 = torch.randn(n, device=dev)
    pa, pb = p0.clone(), p0.clone()
    ga, gb = torch.zeros_like(pa), torch.zeros_like(pb)
    kw = dict(lr=1e-3, max_grad_norm=4.0 * math.sqrt(n), lr_schedule=ops.LRSchedule("warmup_cosine", 2, 5, 0.1), skip_nonfinite=True)
    one, ref = ops.AdamWFlat(pa, ga, **kw), ops.AdamWFlat(pb, gb, **kw)
    words = torch.zeros(L.ACCUM_WORDS, device=dev, dtype=torch.int32)
    loss = torch.tensor(1.25, device=dev)
    a = L.Accum()
    a.accum, a.loss, a.steps = words.data_ptr(), loss.data_ptr(), 1
    for it, grad in enumerate(_grads(n, 5, dev, seed=4)):
        ga.copy_(grad)
        gb.copy_(grad)
        L.check(lib.nlam_adamw_step_accum(C.byref(one._optctl(0.5)), C.byref(a), _stream()), "nlam_adamw_step_accum")
        ref.step(0.5)
        sa, sb = _opt_state(one), _opt_state(ref)
        for name in sa:
            assert torch.equal(sa[name], sb[name]), (it, name)
        w = words.cpu()
        assert w[:2].tolist() == [0, 0] and w.view(torch.float32)[2:].tolist() == [1.25, 1.25]


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
    return {k: v.clone() for k, v in dict(flat=tr.fp.flat, m=o.m, v=o.v, t=o.t_dev, bc=o.bc_dev, grad=tr.fp.grad).items()}


def _controls():
    return dict(max_grad_norm=MAX_NORM, lr_schedule=_schedule(), accumulate_grad_batches=K)


MODES = ["eager", "forks", "segments"]
_RUNS = {}


def _trajectory(oracle, dev, mode):
    """The run of the trajectory test in one mode, made once: what every call returned and left behind."""
    if mode not in _RUNS:
        tr = _small_trainer(oracle["ds"], oracle["graph"], dev, mode, **_controls())
        calls = []
        for bt in oracle["batches"]:
            micro = tr.micro_step
            loss = float(tr.step(*(t.to(dev) for t in bt)))
            calls.append(dict(micro=micro, loss=loss, norm=float(tr.grad_norm), lr=float(tr.last_lr), t=tr.global_step,
                              graphs=(tr._graph, tr._tail_graph, getattr(tr._graph, "tail", None))))
        _RUNS[mode] = dict(tr=tr, calls=calls, state=_state(tr), window_loss=float(tr.window_loss))
    return _RUNS[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_trainer_trajectory_with_accumulation_matches_oracle(dev, oracle, mode):
    run = _trajectory(oracle, dev, mode)
    tr, calls = run["tr"], run["calls"]
    for it, c in enumerate(calls):
        w, closing = it // K, it % K == K - 1
        print(f"call {it}: loss {c['loss']:.7g} (oracle {oracle['losses'][it]:.7g}), grad norm {c['norm']:.7g}, lr {c['lr']:.4g}, "
              f"updates {c['t']}")
        assert c["micro"] == it % K
        assert abs(c["loss"] - oracle["losses"][it]) < TOL * abs(oracle["losses"][it]), it
        assert c["t"] == (w + 1 if closing else w), it
        if closing:
            assert abs(c["norm"] - oracle["norms"][w]) < TOL * abs(oracle["norms"][w]), it
            assert _ulps(c["lr"], np.float32(float(np.float32(LR)) * _schedule().factor(w))) <= 1.0, it
        elif w > 0:   # a holding call leaves the last closed window's values
            assert c["norm"] == calls[it - 1]["norm"] and c["lr"] == calls[it - 1]["lr"], it
    assert tr.global_step == WINDOWS and tr.skipped_steps == 0 and tr.micro_step == 0
    want = np.float32(np.float32(np.float32(calls[-2]["loss"]) + np.float32(calls[-1]["loss"])) / np.float32(K))
    assert np.float32(run["window_loss"]) == want
    if mode != "eager":
        # the optimizer never left the captured step and nothing was recorded a second time
        assert tr._graph is not None and not tr._opt_eager and tr._opt_changes == 0 and tr._opt_in_graph
        if mode == "segments":
            assert tr._graph.tail is not None
        first = calls[0]["graphs"]
        assert all(c["graphs"][0] is first[0] and c["graphs"][1] is first[1] and c["graphs"][2] is first[2] for c in calls)
    o_sd = oracle["fc"].state_dict()
    for k, v in tr.forecaster.state_dict().items():
        if v.numel():
            assert float((v.cpu() - o_sd[k]).abs().max()) < WEIGHT_BAR, k


@pytest.mark.gpu
def test_executors_agree_bit_for_bit(dev, oracle):
    runs = {mode: _trajectory(oracle, dev, mode) for mode in MODES}
    for mode in MODES[1:]:
        for k, v in runs["eager"]["state"].items():
            assert torch.equal(v, runs[mode]["state"][k]), (mode, k)
        assert [c["loss"] for c in runs[mode]["calls"]] == [c["loss"] for c in runs["eager"]["calls"]], mode


@pytest.mark.gpu
def test_eager_and_replayed_micro_steps_mix_inside_a_window(dev, oracle):
    """The second micro-batch of every window has another shape (B = 2) and takes the eager fallback of the captured step:
    the device carries the window across, so the run equals an all-eager trainer's bit for bit."""
    ds, graph = oracle["ds"], oracle["graph"]
    batches = [tuple(t.to(dev) for t in b) for b in _micro_batches(ds, n=6, B=[1, 2, 1, 2, 1, 2])]
    mixed, eager = _small_trainer(ds, graph, dev, "forks", **_controls()), _small_trainer(ds, graph, dev, "eager", **_controls())
    for it, b in enumerate(batches):
        assert float(mixed.step(*b)) == float(eager.step(*b)), it
        assert mixed.micro_step == eager.micro_step == (it + 1) % K and mixed.global_step == eager.global_step == (it + 1) // K
    assert mixed._graph is not None and mixed.use_graph and mixed._opt_in_graph and mixed._opt_changes == 0
    sm, se = _state(mixed), _state(eager)
    for k in sm:
        assert torch.equal(sm[k], se[k]), k
    assert torch.equal(mixed.grad_norm, eager.grad_norm) and torch.equal(mixed.window_loss, eager.window_loss)


@pytest.mark.gpu
def test_step_recorded_again_inside_a_window_keeps_the_accumulated_gradient(dev, oracle):
    """opt.lr assigned after the first micro-batch of the second window: the one-graph executor records the step again,
    warm-up passes included, in the middle of a window -- and the weights equal an eager trainer's given the same assignment."""
    ds, graph = oracle["ds"], oracle["graph"]
    batches = [tuple(t.to(dev) for t in b) for b in _micro_batches(ds, n=6)]
    graphed, eager = _small_trainer(ds, graph, dev, "forks", **_controls()), _small_trainer(ds, graph, dev, "eager", **_controls())
    first = None
    for it, b in enumerate(batches):
        if it == K + 1:
            first = graphed._graph
            held = graphed.fp.grad.clone()
            graphed.opt.lr = eager.opt.lr = 4e-4
        assert float(graphed.step(*b)) == float(eager.step(*b)), it
    assert first is not None and graphed._graph is not first and graphed._opt_changes == 1 and graphed._opt_in_graph
    assert bool(held.any())   # there was something to keep
    sg, se = _state(graphed), _state(eager)
    for k in sg:
        assert torch.equal(sg[k], se[k]), k
    assert graphed.global_step == 3 and float(graphed.last_lr) == float(eager.last_lr) < LR * 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_nonfinite_window_is_skipped_and_cleared(dev, oracle, mode):
    """An inf in the target of the first micro-batch of window 2 of 3: the window closes without an update, and window 3
    gives the weights of a run that never saw window 2 -- the gated zero cleared the poisoned gradient."""
    ds, graph = oracle["ds"], oracle["graph"]
    batches = [tuple(t.to(dev) for t in b) for b in _micro_batches(ds, n=6)]
    kw = dict(skip_nonfinite=True, **_controls())
    a, twin = _small_trainer(ds, graph, dev, mode, **kw), _small_trainer(ds, graph, dev, mode, **kw)
    for b in batches[:K]:
        assert float(a.step(*b)) == float(twin.step(*b))
    before = _state(a)
    bad = [t.clone() for t in batches[K]]
    interior = int(np.flatnonzero(1.0 - np.asarray(ds.boundary_mask.values).reshape(-1))[0])   # a node the loss counts
    bad[1][0, 1, interior, 2] = float("inf")
    assert not math.isfinite(float(a.step(*bad)))
    assert math.isfinite(float(a.step(*batches[K + 1])))
    assert not math.isfinite(float(a.grad_norm)) and float(a.opt.clip_coef) == 0.0
    after = _state(a)
    for k in ("flat", "m", "v", "t", "bc"):
        assert torch.equal(before[k], after[k]), k
    assert a.skipped_steps == 1 and a.global_step == 1 and a.micro_step == 0
    assert not bool(torch.isfinite(after["grad"]).all())   # the poison is still in the buffer
    for b in batches[2 * K :]:
        la, lt = float(a.step(*b)), float(twin.step(*b))
        assert la == lt and math.isfinite(la)
    sa, st = _state(a), _state(twin)
    for k in sa:
        assert torch.equal(sa[k], st[k]), k
    assert bool(torch.isfinite(a.fp.flat).all()) and a.skipped_steps == 1 and twin.skipped_steps == 0 and a.global_step == 2
    if mode != "eager":
        assert a._graph is not None and not a._opt_eager and a._opt_changes == 0


@pytest.mark.gpu
def test_checkpoint_at_a_window_boundary_resumes_bit_identically(dev, oracle, tmp_path):
    from neural_lam_amd import checkpoint as ck

    ds, graph = oracle["ds"], oracle["graph"]
    batches = [tuple(t.to(dev) for t in b) for b in _micro_batches(ds, n=6)]
    kw = dict(skip_nonfinite=True, **_controls())
    a = _small_trainer(ds, graph, dev, "forks", **kw)
    la = [float(a.step(*b)) for b in batches]
    b_ = _small_trainer(ds, graph, dev, "forks", **kw)
    lb = [float(b_.step(*b)) for b in batches[:K]]
    assert lb == la[:K]
    path = tmp_path / "b.ckpt"
    made = ck.save_checkpoint(path, b_, epoch=0, global_step=b_.global_step)
    assert made["global_step"] == 1
    assert made["neural_lam_amd"]["optimizer_controls"]["accumulate_grad_batches"] == K
    b_.step(*batches[K])
    with pytest.raises(RuntimeError, match="window"):
        b_.state_dict()
    c = _small_trainer(ds, graph, dev, "forks", **kw)
    c.step(*batches[0])   # the fresh trainer is inside a window when the checkpoint arrives: loading puts it at a boundary
    ck.load_checkpoint(path, c)
    assert c.global_step == 1 and c.micro_step == 0
    lc = [float(c.step(*b)) for b in batches[K:]]
    assert lc == la[K:]
    sa, sc = _state(a), _state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert torch.equal(a.last_lr, c.last_lr) and a.global_step == c.global_step == 3
    other = _small_trainer(ds, graph, dev, "eager", skip_nonfinite=True, max_grad_norm=MAX_NORM, lr_schedule=_schedule(),
                           accumulate_grad_batches=3)
    with pytest.warns(UserWarning, match="accumulate_grad_batches"):
        ck.load_checkpoint(path, other)


# ---- a one-rank process group gives the bits of no group ----
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
                      lr_schedule=ops.LRSchedule("warmup_linear", warmup_steps=2, total_steps=4, min_ratio=0.2))
    pair = [tuple(torch.randn(1, n, 64, device=dev) for n in (60, 50, 900)) for _ in range(2)]
    losses, norms = [], []
    for it in range(6):
        losses.append(float(trainer.step(*pair[it % 2])))
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
    assert grouped["losses"] == alone["losses"] and grouped["norms"] == alone["norms"] and grouped["t"] == alone["t"] == 3
    assert max(alone["norms"]) > 0.5   # clipping was active
    for k in ("flat", "m", "v"):
        assert torch.equal(grouped[k], alone[k]), k
