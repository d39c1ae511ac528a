"""Output clamping and the predicted std inside the step-tail pass (nlam_step_tail_ext_fwd / _bwd, ops.StepTailExtFunction):
the C-ABI without a GPU, and on the GPU the kernels against the float64 formula, the degenerate case against
nlam_step_tail_loss_*, the reference golden through the new route, the new route against the torch-op route
(models.FUSED_CLAMPED_TAIL off), HIP-graph capture against eager, the untouched plain model, and bf16 autocast."""
import ctypes as C
import math
import re
import subprocess

import pytest
import torch

from conftest import ROOT, graph_from_case, load_golden, rel_err
from neural_lam_amd import _lib as L

KINDS = ["mse", "mae", "wmse", "wmae", "nll", "crps_gauss"]
NEW_EXPORTS = ["nlam_step_tail_ext_fwd", "nlam_step_tail_ext_bwd"]
FIELDS = [name for name, _ in L.StepTail._fields_]


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    """Every test here starts on the new route, whatever NLAM_FUSED_CLAMPED_TAIL says; the comparisons switch it themselves."""
    from neural_lam_amd import models as hm

    monkeypatch.setattr(hm, "FUSED_CLAMPED_TAIL", True)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_ext_entry_points_are_declared_and_exported_with_abi_8():
    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert declared == set(L.EXPORTS)
    assert L.ABI_VERSION == 8 and lib.nlam_abi_version() == 8 and re.search(r"#define NLAM_ABI_VERSION 8\b", header)
    assert (L.CLAMP_NONE, L.CLAMP_BOTH, L.CLAMP_LOWER, L.CLAMP_UPPER) == (0, 1, 2, 3)


def test_step_tail_struct_matches_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    offsets = "".join(f' printf(" %zu", offsetof(nlam_step_tail_t, {f}));' for f in FIELDS)
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
        'int main(){printf("%zu", sizeof(nlam_step_tail_t));' + offsets +
        ' printf(" %d %d %d %d\\n", NLAM_CLAMP_NONE, NLAM_CLAMP_BOTH, NLAM_CLAMP_LOWER, NLAM_CLAMP_UPPER); return 0;}\n'
    )
    exe = tmp_path / "sz"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(L.StepTail)] + [getattr(L.StepTail, f).offset for f in FIELDS] + [0, 1, 2, 3]
    assert got == want
    assert len(FIELDS) == 27 and C.sizeof(L.StepTail) == 192


def test_ext_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    F = 3
    good_modes = (C.c_int32 * F)(0, 1, 3)

    def args(std=False, **kw):
        p = L.StepTail()
        for f in FIELDS[:20]:
            setattr(p, f, fake)
        p.clamp_mode_host = C.addressof(good_modes)
        p.pred_std = fake if std else None
        p.g_std = fake if std else None
        p.rows, p.nodes, p.nvars, p.delta_ld, p.kind, p.nparts, p.scale = 8, 4, F, (2 * F if std else F), L.LOSS_NLL, 1, 1.0
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    fwd, bwd = lib.nlam_step_tail_ext_fwd, lib.nlam_step_tail_ext_bwd
    for fn in (fwd, bwd):
        assert fn(None, None) == -1
        for std in (False, True):
            for bad in (dict(kind=0), dict(kind=7), dict(delta=None), dict(prev=None), dict(bmask=None), dict(rows=0), dict(rows=7),
                        dict(nodes=0), dict(nvars=0), dict(delta_ld=F + 1), dict(delta_ld=3 * F), dict(row_weight=None),
                        dict(pred=None), dict(clamp_lo=None), dict(clamp_hi=None)):
                assert fn(args(std, **bad), None) == -1, (fn, std, bad)
        # nvars above the LDS tables (the modes are then never read)
        assert fn(args(nvars=L.LOSS_MAX_VARS + 1, delta_ld=L.LOSS_MAX_VARS + 1, rows=4, nodes=4, clamp_mode_host=None), None) == -2
        # delta_ld and pred_std must agree
        assert fn(args(False, pred_std=fake), None) == -1 and fn(args(True, pred_std=None), None) == -1
        assert fn(args(False, delta_ld=2 * F), None) == -1 and fn(args(True, delta_ld=F), None) == -1
        # a kind that reads a std needs the per-variable one when none is predicted; mse / mae and a predicted std do not
        assert fn(args(False, consts=None), None) == -1
        # clamp modes outside 0..3 (host memory, checked before any launch)
        for bad_mode in (4, -1, 1 << 16):
            modes = (C.c_int32 * F)(0, bad_mode, 2)
            assert fn(args(clamp_mode_host=C.addressof(modes)), None) == -1, bad_mode
    assert fwd(args(truth=None), None) == -1 and fwd(args(partials=None), None) == -1 and fwd(args(nparts=0), None) == -1
    assert fwd(args(target=None), None) == -1   # partials without a target
    assert bwd(args(d_delta=None), None) == -1 and bwd(args(gloss=None), None) == -1
    assert bwd(args(False, g_std=fake), None) == -1   # a std gradient needs a std head


def test_clamp_tables_of_the_variants_golden(tmp_path):
    """The per-variable (mode, lo, hi) table from the golden's kwargs: state_var_0 lower, state_var_2 both, state_var_3
    upper, the rest none; the limits are the standardised ones prepare_clamping_params registers."""
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    base = load_golden("graphlam_30x27_variants")
    ds = SyntheticDatastore(root_path=tmp_path, **base["ds_kwargs"])
    model = hm.GraphLAM(ds, graph=(base["ref_hierarchical"], graph_from_case(base)), **base["model_kwargs"])
    t = model.clamp_tables()
    assert t.modes == (L.CLAMP_LOWER, L.CLAMP_NONE, L.CLAMP_BOTH, L.CLAMP_UPPER, L.CLAMP_NONE)
    assert list(t.mode) == list(t.modes)
    mean, std = base["ds_kwargs"]["state_stats"]["state_mean"], base["ds_kwargs"]["state_stats"]["state_std"]
    lower, upper = base["model_kwargs"]["output_clamping_lower"], base["model_kwargs"]["output_clamping_upper"]
    want_lo = [(lower.get(f"state_var_{i}", mean[i]) - mean[i]) / std[i] for i in range(5)]
    want_hi = [(upper.get(f"state_var_{i}", mean[i]) - mean[i]) / std[i] for i in range(5)]
    assert torch.allclose(t.lo, torch.tensor(want_lo), rtol=1e-6, atol=0) and torch.allclose(t.hi, torch.tensor(want_hi), rtol=1e-6, atol=0)
    assert torch.equal(t.lo[[2]], model.sigmoid_lower_lims) and torch.equal(t.hi[[2]], model.sigmoid_upper_lims)
    assert torch.equal(t.lo[[0]], model.softplus_lower_lims) and torch.equal(t.hi[[3]], model.softplus_upper_lims)
    assert model.clamp_tables() is t   # built once
    assert model.can_fuse_ext_tail() and not model.can_return_raw_delta()
    plain = hm.GraphLAM(ds, graph=(base["ref_hierarchical"], graph_from_case(base)), hidden_dim=8, processor_layers=1)
    assert plain.clamp_tables() is None and not plain.can_fuse_ext_tail() and plain.can_return_raw_delta()


def test_clamp_tables_follow_their_buffers_without_a_call(tmp_path):
    """The tables exist after construction and are rebuilt by load_state_dict, .to() / .double(), copy.deepcopy and unpickling themselves, so the
    call inside a captured step finds them built (building copies the index buffers to the host); they pickle with the module."""
    import copy
    import pickle

    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    base = load_golden("graphlam_30x27_variants")
    ds = SyntheticDatastore(root_path=tmp_path, **base["ds_kwargs"])
    model = hm.GraphLAM(ds, graph=(base["ref_hierarchical"], graph_from_case(base)), **base["model_kwargs"])
    built = model._clamp_tables[1]
    assert model.clamp_tables() is built
    sd = model.state_dict()
    sd["sigmoid_lower_lims"] = sd["sigmoid_lower_lims"] - 0.25
    sd["softplus_upper_lims"] = sd["softplus_upper_lims"] + 0.5
    model.load_state_dict(sd)
    loaded = model._clamp_tables[1]
    assert loaded is not built and loaded.modes == built.modes
    assert torch.equal(loaded.lo[[2]], sd["sigmoid_lower_lims"]) and torch.equal(loaded.hi[[3]], sd["softplus_upper_lims"])
    assert model.clamp_tables() is loaded
    model.double()
    moved = model._clamp_tables[1]
    assert moved is not loaded and model.clamp_tables() is moved and moved.lo.dtype == torch.float32
    for clone in (copy.deepcopy(model), pickle.loads(pickle.dumps(model))):   # __setstate__ builds the copy's own tables
        own = clone._clamp_tables[1]
        assert own is not moved and own.lo is not moved.lo and torch.equal(own.lo, moved.lo) and torch.equal(own.hi, moved.hi)
        assert clone.clamp_tables() is own and own.modes == built.modes and list(own.mode) == list(built.modes)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _misaligned(t):
    """The same values at a 4-byte offset: a contiguous view whose data pointer is not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


TAIL_SCALE, TAIL_GLOSS = 0.25, 1.7
ISP_LOW = float(torch.log(torch.tensor(1e-6 + 1)))   # inverse_softplus' lower clamp as torch evaluates it in fp32
SHAPES = {"scalar": (2, 7, 5), "quads": (2, 8, 5), "f4": (1, 6, 4), "f17": (1, 8, 17), "blocks": (1, 810, 5)}
MODE_SETS = ("mix", "both", "none")


def _modes(which, F):
    if which == "mix":
        return [(1, 2, 3, 0)[f % 4] for f in range(F)]
    return [1 if which == "both" else 0] * F


def _tail_case(shape, which, seed):
    """fp32 inputs that keep the fp32 and the float64 formula on the same branch (checked below in float64): clamped columns
    inside their limits with a margin, about 1 % of the rows (at least one) outside a limit by >= 0.2, a few rows above the
    softplus threshold, raw std ~ N(0, 1) with one element at 25, ~30 % boundary nodes of weight 0."""
    B, N, F = shape
    g = torch.Generator().manual_seed(seed)
    R = B * N
    modes = _modes(which, F)
    lo = torch.tensor([-1.0 + 0.1 * f for f in range(F)])
    hi = lo + 3.0
    prev = torch.randn(R, F, generator=g)
    rows = torch.arange(R)
    outside, above = rows % 97 == 3, rows % 89 == 5
    for f, m in enumerate(modes):
        u, a = torch.rand(R, generator=g), torch.randn(R, generator=g).abs()
        if m == 1:
            col = lo[f] + 0.03 + u * (3.0 - 0.06)
            col[outside] = torch.where(u[outside] < 0.5, lo[f] - 0.2 - u[outside], hi[f] + 0.2 + u[outside])
        elif m == 2:
            col = lo[f] + 0.03 + 1.5 * a
            col[outside] = lo[f] - 0.2 - u[outside]
            col[above] = lo[f] + 23.0 + u[above]
        elif m == 3:
            col = hi[f] - 0.03 - 1.5 * a
            col[outside] = hi[f] + 0.2 + u[outside]
            col[above] = hi[f] - 23.0 - u[above]
        else:
            continue
        prev[:, f] = col
    bmask = (torch.rand(N, generator=g) < 0.3).float()
    bmask[0], bmask[-1] = 0.0, 1.0
    interior = 1.0 - bmask
    d = {"prev": prev.view(B, N, F), "delta2": torch.randn(B, N, 2 * F, generator=g), "truth": torch.randn(B, N, F, generator=g),
         "target": torch.randn(B, N, F, generator=g), "g_pred": torch.randn(B, N, F, generator=g),
         "g_std": torch.randn(B, N, F, generator=g), "dstd": torch.rand(F, generator=g) + 0.5, "dmean": 0.1 * torch.randn(F, generator=g),
         "var_std": torch.rand(F, generator=g) + 0.5, "bmask": bmask, "row_weight": interior / interior.sum(), "lo": lo, "hi": hi}
    d["delta2"][0, 1, F + 1] = 25.0   # the raw std of one interior-or-not element on softplus' linear branch
    d["modes"] = modes
    # nothing within 1e-3 of a clamp bound or a threshold
    p64, r64 = prev.double(), (d["delta2"][..., :F].double() * d["dstd"].double() + d["dmean"].double()).view(R, F)
    for f, m in enumerate(modes):
        if m == 1:
            x = (p64[:, f] - lo[f].double()) / 3.0
            assert float(torch.minimum((x - 1e-6).abs(), (x - (1 - 1e-6)).abs()).min()) > 1e-3
        elif m in (2, 3):
            y = p64[:, f] - lo[f].double() if m == 2 else hi[f].double() - p64[:, f]
            assert float(torch.minimum((y - ISP_LOW).abs(), (y - 20).abs()).min()) > 1e-3
            inv = torch.where(y <= 20, torch.log(torch.expm1(y.clamp(ISP_LOW, 20))), y)
            q = inv + r64[:, f] if m == 2 else inv - r64[:, f]
            assert float((q - 20).abs().min()) > 1e-3
    assert float((d["delta2"][..., F:].double() - 20).abs().min()) > 1e-3
    return d


def _inverse_softplus(y):
    yc = torch.clamp(y, min=ISP_LOW, max=20.0)
    return torch.where(y <= 20.0, torch.log(torch.expm1(yc)), y)


def _entry(kind, diff, s):
    if kind == "mse":
        return diff**2
    if kind == "mae":
        return diff.abs()
    if kind == "wmse":
        return diff**2 / s**2
    if kind == "wmae":
        return diff.abs() / s
    if kind == "nll":
        return 0.5 * diff**2 / s**2 + torch.log(s) + 0.5 * math.log(2 * math.pi)
    z = -diff / s
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    return s * (z * (2 * cdf - 1) + 2 * pdf - 1 / math.sqrt(math.pi))


def _formula(d, kind, has_std, with_g, with_loss, dtype):
    """The reference's formulation (get_clamped_new_state, softplus, the boundary overwrite, metrics.<kind> on the interior
    weights) with torch ops in ``dtype`` on the CPU; the gradients of delta and prev by autograd."""
    sp = torch.nn.functional.softplus
    t = {k: v.to(dtype) for k, v in d.items() if isinstance(v, torch.Tensor)}
    F = t["prev"].shape[-1]
    delta = (t["delta2"] if has_std else t["delta2"][..., :F].contiguous()).clone().requires_grad_()
    prev = t["prev"].clone().requires_grad_()
    r = delta[..., :F] * t["dstd"] + t["dmean"]
    cols = []
    for f, m in enumerate(d["modes"]):
        p, rf, lo, hi = prev[..., f], r[..., f], t["lo"][f], t["hi"][f]
        if m == 0:
            cols.append(p + rf)
        elif m == 1:
            u = torch.clamp((p - lo) / (hi - lo), min=1e-6, max=1 - 1e-6)
            cols.append(lo + (hi - lo) * torch.sigmoid(torch.log(u / (1 - u)) + rf))
        elif m == 2:
            cols.append(lo + sp(_inverse_softplus(p - lo) + rf))
        else:
            cols.append(hi - sp(-(-_inverse_softplus(hi - p) + rf)))
    new = torch.stack(cols, dim=-1)
    bm = t["bmask"][:, None]
    pred = bm * t["truth"] + (1 - bm) * new
    std = sp(delta[..., F:]) if has_std else None
    total = torch.zeros((), dtype=dtype)
    loss = None
    if with_loss:
        s = std if has_std else t["var_std"]
        loss = TAIL_SCALE * (t["row_weight"][:, None] * _entry(kind, pred - t["target"], s)).sum()
        total = total + TAIL_GLOSS * loss
    if with_g:
        total = total + (pred * t["g_pred"]).sum() + ((std * t["g_std"]).sum() if has_std else 0.0)
    d_delta, d_prev = torch.autograd.grad(total, (delta, prev), allow_unused=True)
    d_delta = torch.zeros_like(delta) if d_delta is None else d_delta
    out = {"pred": pred.detach(), "d_delta_mean": d_delta[..., :F], "d_prev": d_prev}
    if has_std:
        out["pred_std"], out["d_delta_std"] = std.detach(), d_delta[..., F:]
    if with_loss:
        out["loss"] = loss.detach()
    return out


def _ext_run(lib, dev, d, kind, has_std, with_g, with_loss, misalign=False, clamp=True):
    put = (lambda t: _misaligned(t.to(dev))) if misalign else (lambda t: t.to(dev).contiguous())
    B, N, F = d["prev"].shape
    ld = 2 * F if has_std else F
    t = {k: put(v) for k, v in d.items() if isinstance(v, torch.Tensor) and k != "delta2"}
    t["delta"] = put(d["delta2"] if has_std else d["delta2"][..., :F].contiguous())
    nan = lambda *shape: put(torch.full(shape, float("nan")))  # noqa: E731
    out = {"pred": nan(B, N, F), "d_delta": nan(B, N, ld), "d_prev": nan(B, N, F)}
    if has_std:
        out["pred_std"] = nan(B, N, F)
    modes = (C.c_int32 * F)(*d["modes"])
    nparts = 512
    partials, loss, gloss = torch.zeros(nparts, device=dev), torch.zeros((), device=dev), torch.tensor(TAIL_GLOSS, device=dev)
    p = L.StepTail()
    p.delta, p.prev, p.truth, p.dstd, p.dmean = (t[k].data_ptr() for k in ("delta", "prev", "truth", "dstd", "dmean"))
    p.bmask, p.row_weight = t["bmask"].data_ptr(), t["row_weight"].data_ptr()
    if clamp:
        p.clamp_mode_host, p.clamp_lo, p.clamp_hi = C.addressof(modes), t["lo"].data_ptr(), t["hi"].data_ptr()
    p.pred = out["pred"].data_ptr()
    if has_std:
        p.pred_std = out["pred_std"].data_ptr()
    else:
        p.consts = t["var_std"].data_ptr()
    if with_loss:
        p.target, p.partials, p.nparts, p.gloss = t["target"].data_ptr(), partials.data_ptr(), nparts, gloss.data_ptr()
    p.rows, p.nodes, p.nvars, p.delta_ld, p.kind, p.scale = B * N, N, F, ld, L.LOSS_KINDS[kind], TAIL_SCALE
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.nlam_step_tail_ext_fwd(C.byref(p), stream), "nlam_step_tail_ext_fwd")
    if with_loss:
        L.check(lib.nlam_reduce_partials(partials.data_ptr(), nparts, 1, 1, loss.data_ptr(), 0, stream), "nlam_reduce_partials")
        out["loss"] = loss
    if with_g:
        p.g_pred = t["g_pred"].data_ptr()
        if has_std:
            p.g_std = t["g_std"].data_ptr()
    p.d_delta, p.d_prev = out["d_delta"].data_ptr(), out["d_prev"].data_ptr()
    L.check(lib.nlam_step_tail_ext_bwd(C.byref(p), stream), "nlam_step_tail_ext_bwd")
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    d_delta = res.pop("d_delta")
    res["d_delta_mean"] = d_delta[..., :F]
    if has_std:
        res["d_delta_std"] = d_delta[..., F:]
    return res


def _err(x, x64):
    return rel_err(x.double().reshape(-1), x64.double().reshape(-1))


@pytest.fixture(scope="module")
def tail_cases():
    return {(name, which): _tail_case(shape, which, seed=11 + 7 * i + j)
            for i, (name, shape) in enumerate(SHAPES.items()) for j, which in enumerate(MODE_SETS)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_ext_step_tail_kernels_match_float64_formula(dev, tail_cases, kind):
    """step_tail_ext_fwd_kernel / _bwd_kernel through the C entry points against the float64 formula: per-variable and predicted
    std, with and without g_pred / g_std, the scalar loop, the 16-byte loop (quads across rows and the node wrap, delta rows
    twice as long as pred rows), F = 4 and 17, more than one workgroup, every operand misaligned, the mode mixes, and the
    forward / backward without a loss term.  Per output tensor err = max|X - X64| / max|X64| <= 2 err_ref + 1e-6, err_ref the
    same formula in fp32 on the CPU, and never above 1e-4.  The measured err / err_ref per kind are recorded in profiles/clamped_tail/README.md."""
    lib = L.load()
    worst = {}
    for (name, which), d in tail_cases.items():
        boundary = d["bmask"] == 1
        for has_std in (False, True):
            for with_g, with_loss in ((True, True), (False, True), (True, False)):
                if not with_loss and (kind != "nll" or name == "blocks"):
                    continue   # without a loss term the kind plays no part: once
                what = (kind, name, which, "std" if has_std else "var", with_g, with_loss)
                ref64 = _formula(d, kind, has_std, with_g, with_loss, torch.float64)
                ref32 = _formula(d, kind, has_std, with_g, with_loss, torch.float32)
                runs = [_ext_run(lib, dev, d, kind, has_std, with_g, with_loss)]
                if name == "quads":
                    runs.append(_ext_run(lib, dev, d, kind, has_std, with_g, with_loss, misalign=True))
                for got in runs:
                    assert set(got) == set(ref64), what
                    for k, x64 in ref64.items():
                        assert bool(torch.isfinite(got[k]).all()) and bool(torch.isfinite(ref32[k]).all()), (what, k)
                        err, err_ref = _err(got[k], x64), _err(ref32[k], x64)
                        print(what, k, f"err {err:.2e} err_ref {err_ref:.2e}")
                        worst[k] = max(worst.get(k, (0.0, 0.0)), (err, err_ref))
                        assert err <= 2 * err_ref + 1e-6 and err <= 1e-4, (what, k, err, err_ref)
                    for k in ("d_delta_mean", "d_prev") + (("d_delta_std",) if has_std and not with_g else ()):
                        assert bool((got[k][:, boundary] == 0).all()), (what, k)
                if len(runs) == 2:   # the 16-byte loop and the scalar loop: the same elementwise bits
                    for k in runs[0]:
                        if k != "loss":
                            assert torch.equal(runs[0][k], runs[1][k]), (what, k)
    print(kind, "worst (err, err_ref):", {k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in worst.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_ext_entries_without_options_give_the_bits_of_the_loss_pair(dev, tail_cases, kind):
    """clamp_mode_host = NULL (or all NLAM_CLAMP_NONE) and no std head: pred, loss, d_delta and d_prev are those of
    nlam_step_tail_loss_fwd / _bwd on the same inputs, bit for bit."""
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name in ("scalar", "quads", "blocks"):
        d = tail_cases[(name, "none")]
        B, N, F = d["prev"].shape
        t = {k: v.to(dev).contiguous() for k, v in d.items() if isinstance(v, torch.Tensor)}
        delta = t["delta2"][..., :F].contiguous()
        pred, d_delta, d_prev = (torch.full((B, N, F), float("nan"), device=dev) for _ in range(3))
        partials, loss, gloss = torch.zeros(512, device=dev), torch.zeros((), device=dev), torch.tensor(TAIL_GLOSS, device=dev)
        ptr = lambda x: x.data_ptr()  # noqa: E731
        k = L.LOSS_KINDS[kind]
        L.check(lib.nlam_step_tail_loss_fwd(k, ptr(delta), ptr(t["prev"]), ptr(t["truth"]), ptr(t["target"]), ptr(t["dstd"]),
                                            ptr(t["dmean"]), ptr(t["bmask"]), ptr(t["var_std"]), ptr(t["row_weight"]), TAIL_SCALE,
                                            ptr(pred), ptr(partials), 512, B * N, N, F, stream), "nlam_step_tail_loss_fwd")
        L.check(lib.nlam_reduce_partials(ptr(partials), 512, 1, 1, ptr(loss), 0, stream), "nlam_reduce_partials")
        L.check(lib.nlam_step_tail_loss_bwd(k, ptr(t["g_pred"]), ptr(gloss), ptr(pred), ptr(t["target"]), ptr(t["dstd"]), ptr(t["bmask"]),
                                            ptr(t["var_std"]), ptr(t["row_weight"]), TAIL_SCALE, ptr(d_delta), ptr(d_prev), B * N, N, F,
                                            stream), "nlam_step_tail_loss_bwd")
        torch.cuda.synchronize()
        for clamp in (False, True):   # NULL, and a table of NLAM_CLAMP_NONE
            got = _ext_run(lib, dev, d, kind, False, True, True, clamp=clamp)
            assert torch.equal(got["pred"], pred.cpu()) and torch.equal(got["loss"], loss.cpu()), (kind, name, clamp)
            assert torch.equal(got["d_delta_mean"], d_delta.cpu()) and torch.equal(got["d_prev"], d_prev.cpu()), (kind, name, clamp)


def _variants_model(tmp_path, dev, loss="wmse", weights=True, **overrides):
    """GraphLAM on the datastore, graph and batch (T = 3) of graphlam_30x27_variants: its kwargs (std + three clamp modes) with
    ``overrides``; the golden's weights, or seeded ones where the overrides change a shape."""
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    base = load_golden("graphlam_30x27_variants")
    ds = SyntheticDatastore(root_path=tmp_path, **base["ds_kwargs"])
    kw = dict(base["model_kwargs"], **overrides)
    torch.manual_seed(3)
    fc = hm.ARForecaster(hm.GraphLAM(ds, graph=(base["ref_hierarchical"], graph_from_case(base)), **kw), ds)
    if weights:
        fc.load_state_dict(base["state_dict"], strict=True)
    step = hm.ForecasterStep(fc, ds, loss=loss).to(dev)
    return base, fc, step, [base[k].contiguous().to(dev) for k in ("init", "target", "forcing")]


class _Counter:
    """Counts the calls of the routes' Functions and of get_clamped_new_state while it is active."""

    def __init__(self, monkeypatch):
        from neural_lam_amd import models as hm
        from neural_lam_amd import ops

        self.calls = {"ext": 0, "loss": 0, "tail": 0, "clamp": 0}
        for cls, key in ((ops.StepTailExtFunction, "ext"), (ops.LossFunction, "loss"), (ops.WmseLossFunction, "loss"),
                         (ops.StepTailFunction, "tail")):
            def counted(*a, _orig=cls.apply, _key=key):
                self.calls[_key] += 1
                return _orig(*a)

            monkeypatch.setattr(cls, "apply", counted)

        def clamped(model, *a, _orig=hm.StepPredictor.get_clamped_new_state):
            self.calls["clamp"] += 1
            return _orig(model, *a)

        monkeypatch.setattr(hm.StepPredictor, "get_clamped_new_state", clamped)


@pytest.mark.gpu
def test_reference_golden_through_the_ext_route(dev, tmp_path, monkeypatch):
    """graphlam_30x27_variants (output_std + lower / both / upper clamps, T = 3) via ForecasterStep: prediction, loss and every
    parameter gradient at the norms of test_hip_parity's model test, on T applications of ops.StepTailExtFunction and nothing
    else; evaluate() and the plain rollout on the same route against the golden's prediction, ref_one_step and ref_one_std."""
    case, fc, step, (init, target, forcing) = _variants_model(tmp_path, dev)
    T = target.shape[1]
    counter = _Counter(monkeypatch)
    pred, loss = step(init, target, forcing)
    loss.backward()
    assert counter.calls == {"ext": T, "loss": 0, "tail": 0, "clamp": 0}
    assert rel_err(pred.cpu(), case["ref_prediction"]) < 1e-4
    assert abs(float(loss.detach()) - float(case["ref_loss"])) < 1e-4 * abs(float(case["ref_loss"]))
    for k, p in fc.named_parameters():
        assert p.grad is not None, k
        ref_g = case["ref_grads"][k]
        assert float((p.grad.cpu() - ref_g).abs().max()) < 1e-4 * max(float(ref_g.abs().max()), 1e-3), k
    r = step.evaluate(init, target, forcing, phase="test", steps_to_log=(1, 3))
    assert counter.calls == {"ext": 2 * T, "loss": 0, "tail": 0, "clamp": 0}
    assert rel_err(r.prediction.cpu(), case["ref_prediction"]) < 1e-4
    assert abs(float(r.mean_loss) - float(case["ref_loss"])) < 1e-4 * abs(float(case["ref_loss"]))
    with torch.no_grad():
        one, one_std = fc(init, forcing[:, :1], target[:, :1])
    assert counter.calls["ext"] == 2 * T + 1 and counter.calls["clamp"] == 0
    interior = fc.boundary_mask.reshape(-1).cpu() == 0
    assert rel_err(one[0, 0].cpu()[interior], case["ref_one_step"][0][interior]) < 1e-4
    assert rel_err(one_std[:, 0].cpu(), case["ref_one_std"]) < 1e-4


@pytest.mark.gpu
def test_evaluate_of_a_predicted_std_model_matches_reference_golden_on_the_ext_route(dev, tmp_path, monkeypatch):
    """tests/golden/eval_metrics.pt's output_std model (the variants golden without its clamps): evaluate(phase="test") on the
    new route against the reference's test_step tensors."""
    golden = load_golden("eval_metrics")
    case = golden["models"]["std"]
    base, fc, step, batch = _variants_model(tmp_path, dev, loss=case["kind"], weights=False, **{
        k: case["model_kwargs"].get(k) for k in ("output_clamping_lower", "output_clamping_upper")})
    sd = fc.state_dict()
    sd.update({k: base["state_dict"][k] for k in case["param_names"]})
    fc.load_state_dict(sd, strict=True)
    counter = _Counter(monkeypatch)
    r = step.evaluate(*batch, phase="test", steps_to_log=golden["models"]["steps_to_log"])
    assert counter.calls == {"ext": golden["models"]["T"], "loss": 0, "tail": 0, "clamp": 0}
    assert rel_err(r.prediction.cpu(), case["ref_prediction"]) < 1e-4
    assert rel_err(r.time_step_loss.cpu(), case["ref_time_step_loss"]) < 1e-4
    assert rel_err(r.entry_mse.cpu(), case["ref_entry_mse"]) < 1e-4 and rel_err(r.entry_mae.cpu(), case["ref_entry_mae"]) < 1e-4
    assert rel_err(r.output_std.cpu(), case["ref_output_std"]) < 1e-4


def _both_routes(monkeypatch, step, fc, batch, autocast=False):
    """(prediction, pred_std, loss, gradients, call counts) of one training step with the switch on, then off."""
    from neural_lam_amd import models as hm

    out = []
    for fused in (True, False):
        with monkeypatch.context() as m:
            m.setattr(hm, "FUSED_CLAMPED_TAIL", fused)
            counter = _Counter(m)
            fc.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                pred, loss = step(*batch)
                with torch.no_grad():
                    _, pred_std = fc(batch[0], batch[2], batch[1])
            loss.float().backward()
            grads = {k: (p.grad.clone() if p.grad is not None else None) for k, p in fc.named_parameters()}
            out.append((pred.detach().float(), None if pred_std is None else pred_std.float(), loss.detach().float(), grads,
                        counter.calls))
    return out


def _assert_routes_agree(new, old, T, old_loss_calls=1):
    (p1, s1, l1, g1, c1), (p0, s0, l0, g0, c0) = new, old
    assert c1 == {"ext": 2 * T, "loss": 0, "tail": 0, "clamp": 0}, c1
    assert c0["ext"] == 0 and c0["tail"] == 0 and c0["loss"] == old_loss_calls, c0
    assert rel_err(p1.cpu(), p0.cpu()) < 1e-5
    assert (s1 is None) == (s0 is None)
    if s1 is not None:
        assert rel_err(s1.cpu(), s0.cpu()) < 1e-5
    assert abs(float(l1) - float(l0)) < 1e-5 * abs(float(l0))
    for k in g0:
        a = g1[k] if g1[k] is not None else torch.zeros_like(g0[k])
        assert bool(torch.isfinite(a).all()), k
        assert float((a - g0[k]).abs().max()) < 1e-5 * max(float(g0[k].abs().max()), 1e-3), k


NO_CLAMPS = dict(output_clamping_lower=None, output_clamping_upper=None)
ROUTE_CASES = [("wmse", {}), ("nll", {}), ("crps_gauss", {}), ("mae", dict(output_std=False)), ("wmse", dict(output_std=False)),
               ("mse", NO_CLAMPS)]


@pytest.mark.gpu
@pytest.mark.parametrize("loss,overrides", ROUTE_CASES, ids=[f"{k}-{'-'.join(o) or 'std+clamps'}" for k, o in ROUTE_CASES])
def test_ext_route_matches_the_torch_op_route(dev, tmp_path, monkeypatch, loss, overrides):
    """The same model and T = 3 batch with models.FUSED_CLAMPED_TAIL on, then off (get_clamped_new_state, softplus, the loss pass
    over the rollout): prediction, pred_std, loss and every gradient within 1e-5.  std + clamps with wmse / nll / crps_gauss,
    clamps only with mae / wmse, std only with mse (the std half of the output gradient is all zeros, and written)."""
    _, fc, step, batch = _variants_model(tmp_path, dev, loss=loss, weights=not overrides, **overrides)
    new, old = _both_routes(monkeypatch, step, fc, batch)
    std = overrides.get("output_std", True)
    # the old route of a predicted-std wmse is the torch formula: no loss Function at all
    _assert_routes_agree(new, old, T=3, old_loss_calls=0 if (loss == "wmse" and std) else 1)
    if loss == "mse":
        w = new[3]["predictor.output_map.2.weight"]
        assert w.shape[0] == 10 and bool((w[5:] == 0).all()) and bool((new[3]["predictor.output_map.2.bias"][5:] == 0).all())
        assert bool((w[:5] != 0).any())


@pytest.mark.gpu
def test_ext_route_matches_the_torch_op_route_on_a_small_hilam(dev, tmp_path, monkeypatch):
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    case = load_golden("hilam_81x30")
    ds = SyntheticDatastore(root_path=tmp_path, **case["ds_kwargs"])
    names = ds.get_vars_names("state")
    kw = dict(case["model_kwargs"], output_clamping_lower={names[0]: -0.5, names[1]: -1.0},
              output_clamping_upper={names[1]: 1.5, names[-1]: 2.0})
    fc = hm.ARForecaster(hm.HiLAM(ds, graph=(case["ref_hierarchical"], graph_from_case(case)), **kw), ds)
    sd = fc.state_dict()
    sd.update({k: v for k, v in case["state_dict"].items() if k in dict(fc.named_parameters())})
    fc.load_state_dict(sd, strict=True)
    step = hm.ForecasterStep(fc, ds).to(dev)
    assert fc.predictor.clamp_tables().modes[:2] == (L.CLAMP_LOWER, L.CLAMP_BOTH) and fc.predictor.clamp_tables().modes[-1] == L.CLAMP_UPPER
    batch = [case[k].contiguous().to(dev) for k in ("init", "target", "forcing")]
    new, old = _both_routes(monkeypatch, step, fc, batch)
    _assert_routes_agree(new, old, T=batch[1].shape[1])


def _small_clamped_std_step(tmp_path, dev, loss="nll"):
    from neural_lam_amd import graph as G
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)
    ext = ds.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state")), max(ext[1] - ext[0], ext[3] - ext[2]))
    names = ds.get_vars_names("state")
    torch.manual_seed(1)
    model = hm.GraphLAM(ds, graph=graph, hidden_dim=16, processor_layers=2, output_std=True,
                        output_clamping_lower={names[0]: -1.0, names[2]: -2.0}, output_clamping_upper={names[2]: 2.0, names[3]: 1.5})
    return ds, hm.ForecasterStep(hm.ARForecaster(model, ds), ds, loss=loss).to(dev)


def _batches(ds, dev, n, seed=0):
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(1, 2, N, 5, generator=g).to(dev), torch.randn(1, 2, N, 5, generator=g).to(dev),
             torch.randn(1, 2, N, 6, generator=g).to(dev)] for _ in range(n)]


@pytest.mark.gpu
def test_hip_graph_trainer_equals_eager_trainer_on_the_ext_route(dev, tmp_path, monkeypatch):
    """Trainer(use_graph=True) against the eager Trainer: three AdamW steps of a clamped output_std model with nll, bit for bit."""
    from neural_lam_amd.trainer import Trainer

    ds, s_e = _small_clamped_std_step(tmp_path, dev)
    _, s_g = _small_clamped_std_step(tmp_path, dev)
    t_eager, t_graph = Trainer(s_e, lr=1e-3, use_graph=False), Trainer(s_g, lr=1e-3, use_graph=True)
    counter = _Counter(monkeypatch)
    for batch in _batches(ds, dev, 3):
        le, lg = float(t_eager.step(*batch)), float(t_graph.step(*batch))
        assert le == lg and math.isfinite(le)
        assert torch.equal(t_eager.fp.flat, t_graph.fp.flat) and torch.equal(t_eager.fp.grad, t_graph.fp.grad)
    assert t_graph._graph is not None
    assert counter.calls["ext"] >= 2 * 3 + 2 and counter.calls["loss"] == 0 and counter.calls["clamp"] == 0


@pytest.mark.gpu
def test_graphed_flat_step_equals_eager_module_on_the_ext_route(dev, tmp_path):
    """graphed_training_step(flat=True) of the same model against the eager module: loss, prediction, every gradient and the
    weights after three AdamW steps, bit for bit."""
    from neural_lam_amd.trainer import graphed_training_step

    ds, s_e = _small_clamped_std_step(tmp_path, dev)
    _, s_g = _small_clamped_std_step(tmp_path, dev)
    batches = _batches(ds, dev, 4)
    graphed = graphed_training_step(s_g, *batches[0], flat=True)
    leaf = graphed.flat_parameter
    o_e = torch.optim.AdamW(s_e.parameters(), lr=1e-3, betas=(0.9, 0.95))
    o_g = torch.optim.AdamW([leaf], lr=1e-3, betas=(0.9, 0.95))
    for b in batches[1:]:
        o_e.zero_grad(set_to_none=True)
        pred_e, loss_e = s_e(*b)
        loss_e.backward()
        o_g.zero_grad(set_to_none=True)
        pred_g, loss_g = graphed(*b)
        loss_g.backward()
        assert float(loss_e) == float(loss_g) and torch.equal(pred_e, pred_g)
        for p, o in zip(s_e.parameters(), graphed.goffs):
            assert torch.equal(p.grad.reshape(-1), leaf.grad[o : o + p.numel()])
        o_e.step()
        o_g.step()
        for a, c in zip(s_e.parameters(), s_g.parameters()):
            assert torch.equal(a, c)


@pytest.mark.gpu
def test_plain_model_is_untouched_by_the_switch(dev, tmp_path, monkeypatch):
    """A model with neither option: loss, prediction and gradients bit for bit with the switch on and off, on ops.StepTailFunction
    both times; ops.StepTailExtFunction is never applied."""
    _, fc, step, batch = _variants_model(tmp_path, dev, weights=False, output_std=False, **NO_CLAMPS)
    (p1, s1, l1, g1, c1), (p0, s0, l0, g0, c0) = _both_routes(monkeypatch, step, fc, batch)
    assert c1 == c0 and c1["ext"] == 0 and c1["tail"] == 3 and c1["loss"] == 0 and s1 is None and s0 is None
    assert torch.equal(p1, p0) and torch.equal(l1, l0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


@pytest.mark.gpu
def test_ext_route_under_bf16_autocast_matches_the_torch_op_route(dev, tmp_path, monkeypatch):
    """Under torch.autocast(bfloat16) the route is taken and agrees with the torch-op route at 1e-5: both see the same
    output_map bits."""
    _, fc, step, batch = _variants_model(tmp_path, dev, loss="nll")
    new, old = _both_routes(monkeypatch, step, fc, batch, autocast=True)
    _assert_routes_agree(new, old, T=3)


@pytest.mark.gpu
def test_four_entry_loss_spec_runs_as_wmse_on_the_ext_route(dev, tmp_path):
    """ARForecaster.forward's documented wmse form (target, inv_var, row_weight, scale) on a clamped model is the five-entry
    spec with NLAM_LOSS_WMSE and var_std = inv_var ** -0.5 (1e-6: the rsqrt's rounding); on a predicted-std model the
    predicted std is the std of the loss and inv_var is not read (the same bits)."""
    for overrides in (dict(output_std=False), {}):
        _, fc, step, (init, target, forcing) = _variants_model(tmp_path, dev, weights=not overrides, **overrides)
        scale = 1.0 / (target.shape[0] * target.shape[1])
        var_std = step.per_var_std if overrides else None
        inv_var = step.inv_var if overrides else torch.ones(5, device=dev)
        with torch.no_grad():
            p4, s4, l4 = fc(init, forcing, target, loss_spec=(target, inv_var, step.interior_weight, scale))
            p5, s5, l5 = fc(init, forcing, target, loss_spec=(target, var_std, step.interior_weight, scale, L.LOSS_WMSE))
        assert l4 is not None and torch.equal(p4, p5) and (s4 is None) == bool(overrides)
        assert abs(float(l4) - float(l5)) <= (1e-6 if overrides else 0.0) * abs(float(l5))
