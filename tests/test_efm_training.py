"""Training Graph-EFM with the variational objective (models.EFMForecaster / EFMForecasterStep, ops.LatentKLFunction,
nlam_latent_kl_fwd / nlam_latent_kl_bwd).  Without a GPU: the C-ABI (exports, layout, argument checks, workspace query), the
float64 reference of elbo_ref.py against torch.distributions and float64 autograd, and the step's host logic.  On the GPU: the
kernels against that float64 math element by element, the objective and every parameter gradient against the same modules
composed from torch ops, the step inside Trainer (replays, reseeding, annealing, accumulation), resume, and the hand-off of the
trained predictor to EnsembleForecast.

The budgets of the kernel test, in u = 2^-24 (first order; an ulp is at most 2 u of the value).  Error figures of the device
functions as test_ensemble_forecast.py takes them (the OpenCL ULP table the ROCm device library is built to): expf 3 ulp, logf
3 ulp, log1pf 2 ulp; division, sqrt and the arithmetic correctly rounded, 1 u.
  softplus(x) = log1pf(expf(x)): 6 u from expf (the condition number e / ((1 + e) log1p(e)) of log1p is at most 1) + 4 u = 10 u;
    s = 1e-4 + softplus: S = 11 u.  softplus'(x) = 1 / (1 + expf(-x)): 6 u e / (1 + e) + 1 u for the sum + 1 u for the
    division: G = 8 u.
  z = mu_q + s_q eps: the product (S + 1) u |s_q eps|, the sum u (|mu_q| + |s_q eps|):          13 u (|mu_q| + |s_q eps|)
  KL element = 1/2 (r^2 + n^2) - 1/2 - logf(r), r = s_q / s_p ((2 S + 1) u = 23 u), n = (mu_q - mu_p) / s_p ((S + 2) u = 13 u):
    r^2 / 2 carries 2 * 23 + 1 u and three more roundings (the sum, - 1/2, - log): 50 u; n^2 / 2: 2 * 13 + 1 + 3 = 30 u; logf: 6 u
    + 1 u of |log r|, and 23 u ABSOLUTE from the error of r, which the constant 1/2 of the magnitudes covers (46 u of it, + 2):
                                                                                       50 u (|log r| + r^2 / 2 + n^2 / 2 + 1 / 2)
  kl[b]: the elements' budgets plus the additions on the longest path of the reduction the kernel documents -- 4 elements per
    quad over ceil(quads / (blocks * 256)) grid-stride passes in one thread, 6 levels of the wave tree, 2 for the four waves,
    blocks - 1 for the partials in block order -- each u of the running sum, itself at most the sum of the magnitudes:
                                                                                       (50 + depth) u sum_e magnitudes
  kl_term: ceil(B / 256) items per thread, 8 levels for the 256 threads, 1 for the weight: (50 + depth + ceil(B / 256) + 9) u
  backward, w = g_kl_term * kl_weight (1 u), 1 / s_p: S + 1 = 12 u:
    d mu: w dlt / s_p^2 = 1 + 1 + 24 + 3 products = 29 u, + 1 u for g + .:                              30 u (|g| + |w dlt / s_p^2|)
    d raw_q: s_q / s_p^2 37 u, 1 / s_q 12 u, their difference 1 u, w 2 u, + g eps 1 u, softplus' G + 1 = 9 u:          50 u
    d raw_p: s_q^2 + dlt^2 24 u, / s_p^3 39 u, the product 1 u, the difference 1 u, w 2 u, softplus' 9 u:             80 u
    each of the sum of the magnitudes of the pieces (elbo_ref.backward returns them).
The sums are compared against sum |pieces|, not against |KL|, which cancels (q == p gives exactly 0: checked on its own)."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import elbo_ref as E
from conftest import ROOT, graph_from_case, load_golden, rel_err
from neural_lam_amd import _lib as L
from test_ensemble_forecast import EPS32, NORMAL_ULPS, _c_layout

U = 2.0 ** -24
TOL = 1e-4   # the project's parity bound (test_graph_efm.py)
C_Z, C_TERM, C_GMU, C_GRAW_Q, C_GRAW_P = 13, 50, 30, 50, 80
SLACK = 1 + 1e-3   # second-order terms of the first-order budgets
NEW_EXPORTS = ["nlam_latent_kl_fwd", "nlam_latent_kl_bwd", "nlam_latent_kl_workspace_floats"]
EFM_CASES = ["efm_hi_81x30", "efm_ms_30x27", "efm_hi_constprior_81x30"]
# the launcher's cap (csrc/nlam_latent_kl.inc: kLatentKlMaxBlocks workgroups of 256 threads, a quad of 4 elements per thread):
# one pass of the capped grid covers 64 * 256 * 4 elements of an item
MAX_BLOCKS = 64
PASS_ELEMENTS = MAX_BLOCKS * 256 * 4
SHAPES = [(1, 5, 3), (3, 7, 8), (2, 1, 64), (2, 1031, 65), (1, 1100, 64)]   # the last two wrap: scalar and 16-byte parameter rows


def _blocks(per):
    return min(MAX_BLOCKS, ((per + 3) // 4 + 255) // 256)


def _depth(per):
    nblk = _blocks(per)
    return 4 * math.ceil(((per + 3) // 4) / (nblk * 256)) + 6 + 2 + (nblk - 1)


# ---------------------------------------------------------------------------
# CPU: the C-ABI
# ---------------------------------------------------------------------------
def test_latent_kl_symbols_are_exported_and_the_struct_matches_c_layout(tmp_path):
    import re

    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.nlam_abi_version() == 8 == L.ABI_VERSION
    _c_layout(tmp_path, L.LatentKl, "nlam_latent_kl_t")


def test_latent_kl_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    B, R, D = 3, 9, 8
    nws = lib.nlam_latent_kl_workspace_floats(B, R, D)
    assert nws == B * _blocks(R * D)
    for bad in ((0, R, D), (B, 0, D), (B, R, 0), (-1, R, D)):
        assert lib.nlam_latent_kl_workspace_floats(*bad) == -1, bad
    sizes = [lib.nlam_latent_kl_workspace_floats(B, r, D) for r in (1, 100, 1000, 10000, 100000)]
    assert sizes == sorted(sizes) and sizes[-1] == B * MAX_BLOCKS   # monotone, capped
    assert lib.nlam_latent_kl_workspace_floats(2 * B, R, D) == 2 * nws

    def args(**kw):
        p = L.LatentKl()
        for name in ("pq", "pp", "noise_in", "kl_weight", "seed", "draw", "eps", "latent", "kl", "kl_term", "workspace", "g_latent",
                     "g_kl_term", "g_pq", "g_pp"):
            setattr(p, name, fake)
        p.workspace_floats, p.batch, p.rows, p.latent_dim, p.diagonal, p.t = nws, B, R, D, 1, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    for entry in (lib.nlam_latent_kl_fwd, lib.nlam_latent_kl_bwd):
        assert entry(None, None) == -1
        for kw in (dict(pq=None), dict(pp=None), dict(eps=None), dict(kl_weight=None), dict(batch=0), dict(rows=0), dict(latent_dim=0),
                   dict(diagonal=2), dict(diagonal=-1), dict(t=-1)):
            assert entry(args(**kw), None) == -1, kw
        assert entry(args(batch=65536, workspace_floats=1 << 40), None) == -2
        assert entry(args(rows=1 << 16, latent_dim=1 << 15, workspace_floats=1 << 40), None) == -2
    for kw in (dict(latent=None), dict(kl=None), dict(kl_term=None), dict(workspace=None), dict(workspace_floats=nws - 1),
               dict(noise_in=None, seed=None), dict(noise_in=None, draw=None)):
        assert lib.nlam_latent_kl_fwd(args(**kw), None) == -1, kw
    for kw in (dict(g_kl_term=None), dict(g_pq=None)):
        assert lib.nlam_latent_kl_bwd(args(**kw), None) == -1, kw


# ---------------------------------------------------------------------------
# CPU: the float64 reference
# ---------------------------------------------------------------------------
def _problem(B, R, D, diagonal, seed=0, same=False):
    """Parameters with raw stds on both sides of softplus' threshold (20) and far below 0, in fp32 values."""
    g = torch.Generator().manual_seed(1000 * B + 10 * R + D + (500 if diagonal else 0) + seed)
    pq = torch.randn(B, R, 2 * D, generator=g) * 1.5
    pp = torch.randn(B, R, 2 * D if diagonal else D, generator=g) * 1.5
    flat_q, flat_p = pq.view(-1, 2 * D), pp.view(-1, pp.shape[-1])
    flat_q[0, D] = 25.0
    flat_q[-1, 2 * D - 1] = -30.0
    if R * B > 1:
        flat_q[1, D] = 19.5
    if diagonal:
        flat_p[0, D] = 21.0
        flat_p[-1, 2 * D - 1] = -12.0
    if same:
        pp = pq.clone() if diagonal else torch.cat((pq[..., :D], torch.zeros(B, R, 0)), -1)
    eps = torch.randn(B, R, D, generator=g)
    g_z = torch.randn(B, R, D, generator=g)
    return pq, pp, eps, g_z


@pytest.mark.parametrize("diagonal", [False, True])
def test_reference_kl_is_torch_distributions_and_its_gradients_are_autograd(diagonal):
    from torch.distributions import Normal, kl_divergence

    for same in (False, True):
        pq, pp, eps, g_z = _problem(2, 7, 5, diagonal, same=same and diagonal)
        if same and not diagonal:   # q == p against the unit prior: raw_q with 1e-4 + softplus(raw) = 1
            pq[..., 5:] = math.log(math.expm1(1 - 1e-4))
            pp = pq[..., :5].clone()
        pq64, pp64 = pq.double().requires_grad_(), pp.double().requires_grad_()
        mu_q, raw_q, mu_p, raw_p = E.split(pq64, pp64)
        s_q, s_p = E.stds(raw_q, raw_p)
        want = kl_divergence(Normal(mu_q, s_q), Normal(mu_p, s_p)).sum((1, 2))
        got = E.kl_per_item(pq, pp)
        scale = float(E.forward(pq, pp, eps)[2].sum())
        assert float((got - want.detach()).abs().max()) <= 1e-12 * scale
        if same:
            assert float(got.abs().max()) <= 1e-9 and float(want.detach().abs().max()) <= 1e-9   # 0 by cancellation
        w = 0.37
        z = mu_q + s_q * eps.double()
        ((z * g_z.double()).sum() + w * want.sum()).backward()
        g_pq, g_pp, mag_pq, mag_pp = E.backward(pq, pp, eps, g_z, w)
        assert float((g_pq - pq64.grad).abs().max()) <= 1e-12 * float(mag_pq.max())
        assert float((g_pp - pp64.grad).abs().max()) <= 1e-12 * max(float(mag_pp.max()), 1e-30)
        assert float((E.forward(pq, pp, eps)[0] - z.detach()).abs().max()) == 0.0
        g0 = E.backward(pq, pp, eps, None, w)[0]
        assert torch.equal(g0, E.backward(pq, pp, eps, torch.zeros_like(g_z), w)[0])


# ---------------------------------------------------------------------------
# CPU: host logic of the step
# ---------------------------------------------------------------------------
def _cpu_world(tmp_path, name="efm_hi_81x30"):
    from neural_lam_amd import graph as G
    from neural_lam_amd import graph_efm
    from neural_lam_amd.datastore import SyntheticDatastore

    case = load_golden(name)
    ds = SyntheticDatastore(root_path=tmp_path, **case["ds_kwargs"])
    G.save_graph(tmp_path / "graph" / "g", graph_from_case(case, "ref_graph_raw"))
    model = getattr(graph_efm, case["cls"])(ds, graph_name="g", **case["model_kwargs"])
    model.load_state_dict(case["state_dict"], strict=True)
    return case, ds, model


def test_step_host_logic(tmp_path):
    from neural_lam_amd import models as hm

    case, ds, model = _cpu_world(tmp_path)
    with pytest.raises(ValueError):
        hm.EFMForecasterStep(hm.EFMForecaster(model, ds), ds, loss="huber")
    with pytest.raises(ValueError):
        hm.EFMForecasterStep(hm.ARForecaster(model, ds), ds)
    (tmp_path / "lam").mkdir()
    from neural_lam_amd.datastore import SyntheticDatastore

    ds2 = SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path / "lam", boundary="random", seed=1)
    from neural_lam_amd import graph as G

    G.save_graph(tmp_path / "lam" / "graph" / "multiscale", G.create_regular_grid_graph(ds2.get_xy("state")))
    lam = hm.GraphLAM(ds2, hidden_dim=8)
    with pytest.raises(ValueError):
        hm.EFMForecasterStep(hm.EFMForecaster(lam, ds2), ds2)
    step = hm.EFMForecasterStep(hm.EFMForecaster(model, ds), ds, kl_beta=0.25, seed=(1 << 63) + 5, rank=0)
    assert step.loss_name == "nll" and isinstance(step, hm.ForecasterStep) and isinstance(step.forecaster, hm.ARForecaster)
    n_int = int((1 - torch.tensor(ds.boundary_mask.values)).sum())
    assert step.n_interior == n_int and step.kl_weight_value(3, 4) == 0.25 / (n_int * 3 * 4)
    word = step.kl_weight_word(3, 4)
    assert float(word) == np.float32(0.25 / (n_int * 12)) and step.kl_weight_word(3, 4) is word
    other_shape = step.kl_weight_word(1, 2)   # one word per batch shape: a call at another shape leaves this one alone
    assert other_shape is not word and float(other_shape) == np.float32(0.25 / (n_int * 2)) and float(word) == np.float32(0.25 / (n_int * 12))
    step.set_kl_beta(0.5)                     # ... and annealing reaches every one of them, in place
    assert step.kl_weight_word(3, 4) is word and float(word) == np.float32(0.5 / (n_int * 12))
    assert float(other_shape) == np.float32(0.5 / (n_int * 2))
    assert int(step.seed) & 0xFFFFFFFFFFFFFFFF == (1 << 63) + 5   # rank 0: the seed itself, all 64 bits
    # the state round-trips, draw included
    step.reseed(77, draw=9)
    st = step.draw_state()
    assert st == {"seed": 77, "draw": 9, "kl_beta": 0.5}
    other = hm.EFMForecasterStep(hm.EFMForecaster(model, ds), ds, rank=0)
    other.load_draw_state(st)
    assert other.draw_state() == st and torch.equal(other.seed, step.seed) and torch.equal(other.draw, step.draw)
    assert torch.equal(other.kl_weight_word(3, 4), step.kl_weight_word(3, 4))
    # ranks do not share a key
    keys = {hm.EFMForecasterStep.noise_key(77, r) for r in range(64)}
    assert len(keys) == 64 and hm.EFMForecasterStep.noise_key(77, 0) == 77
    r1 = hm.EFMForecasterStep(hm.EFMForecaster(model, ds), ds, seed=77, rank=1)
    r1.kl_weight_word(3, 4)
    assert not torch.equal(r1.seed, step.seed) and r1.draw_state()["seed"] == 77
    assert "seed" not in step.state_dict() and "draw" not in step.state_dict()   # the words travel in the checkpoint's extra
    # no CPU fallback
    N = ds.num_grid_points
    with pytest.raises(RuntimeError):
        step(torch.zeros(1, 2, N, 5), torch.zeros(1, 1, N, 5), torch.zeros(1, 1, N, 6))


# ---------------------------------------------------------------------------
# GPU: the kernels against float64 math
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


GUARD = 8


class _Buf:
    """A tensor between NaN guard floats, 16-byte aligned or one float off."""

    def __init__(self, dev, shape, misalign, value=None):
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
        self.first = GUARD + (1 if misalign else 0)
        self.t = self.raw[self.first:self.first + n].view(shape)
        if value is not None:
            self.t.copy_(value)

    def guards_intact(self):
        n = self.t.numel()
        return bool(torch.isnan(self.raw[:self.first]).all()) and bool(torch.isnan(self.raw[self.first + n:]).all())


def _run_kernels(dev, B, R, D, diagonal, misalign, given, seed=0x1234ABCD9876, draw=(7 << 32) + 5, t=3, w=0.013, g_term=1.7,
                 with_g_pp=True, with_g_z=True, problem=None):
    lib = L.load()
    pq, pp, eps_in, g_z = problem if problem is not None else _problem(B, R, D, diagonal)
    P = pp.shape[-1]
    mk = lambda shape, value=None: _Buf(dev, shape, misalign, value)   # noqa: E731
    b = types.SimpleNamespace(pq=mk((B, R, 2 * D), pq), pp=mk((B, R, P), pp), noise=mk((B, R, D), eps_in) if given else None,
                              eps=mk((B, R, D)), z=mk((B, R, D)), kl=mk((B,)), term=mk((1,)), g_z=mk((B, R, D), g_z) if with_g_z else None,
                              g_pq=mk((B, R, 2 * D)), g_pp=mk((B, R, P)))
    nws = lib.nlam_latent_kl_workspace_floats(B, R, D)
    ws = torch.full((nws,), float("nan"), device=dev)
    klw = torch.tensor([w], device=dev)
    gt = torch.tensor([g_term], device=dev)
    seed_t = torch.tensor([seed], dtype=torch.int64, device=dev)
    draw_t = torch.tensor([draw], dtype=torch.int64, device=dev)
    p = L.LatentKl()
    p.pq, p.pp, p.noise_in, p.kl_weight = _ptr(b.pq.t), _ptr(b.pp.t), _ptr(b.noise.t) if given else None, _ptr(klw)
    if not given:
        p.seed, p.draw = _ptr(seed_t), _ptr(draw_t)
    p.eps, p.latent, p.kl, p.kl_term, p.workspace, p.workspace_floats = _ptr(b.eps.t), _ptr(b.z.t), _ptr(b.kl.t), _ptr(b.term.t), _ptr(ws), nws
    p.batch, p.rows, p.latent_dim, p.diagonal, p.t = B, R, D, int(diagonal), t
    L.check(lib.nlam_latent_kl_fwd(C.byref(p), _stream()), "nlam_latent_kl_fwd")
    p.g_latent, p.g_kl_term, p.g_pq, p.g_pp = _ptr(b.g_z.t) if with_g_z else None, _ptr(gt), _ptr(b.g_pq.t), _ptr(b.g_pp.t) if with_g_pp else None
    L.check(lib.nlam_latent_kl_bwd(C.byref(p), _stream()), "nlam_latent_kl_bwd")
    torch.cuda.synchronize()
    assert int(draw_t) == draw and int(seed_t) == seed   # only read
    for name, buf in vars(b).items():
        assert buf is None or buf.guards_intact(), name
    return b, (pq, pp, eps_in, g_z)


@pytest.mark.gpu
@pytest.mark.parametrize("given", [True, False], ids=["given", "drawn"])
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "off_by_one_float"])
@pytest.mark.parametrize("diagonal", [False, True], ids=["isotropic", "diagonal"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_against_float64_math(dev, shape, diagonal, misalign, given):
    """Budgets: the module docstring.  (2, 1031, 65) and (1, 1100, 64) hold more than PASS_ELEMENTS = 65536 elements per item: the
    capped grid of 64 workgroups strides a second time and every item leaves 64 partials."""
    B, R, D = shape
    per = R * D
    if R > 1000:
        assert per > PASS_ELEMENTS and _blocks(per) == MAX_BLOCKS
    SEED, DRAW, T, W, GT = 0x1234ABCD9876, (7 << 32) + 5, 3, 0.013, 1.7
    b, (pq, pp, eps_in, g_z) = _run_kernels(dev, B, R, D, diagonal, misalign, given, SEED, DRAW, T, W, GT)
    eps = b.eps.t.cpu()
    if given:
        assert torch.equal(_bits(eps), _bits(eps_in))
    else:   # the generator's numbers for counter (quad, t, b, low word of draw)
        want = E.noise(SEED, DRAW, T, B, per)
        ratio = np.abs(eps.double().numpy().reshape(B, -1) - want) / (EPS32 * np.abs(want))
        print(f"noise {shape}: worst {ratio.max():.3f} ulp-units, bar {NORMAL_ULPS}")
        assert bool((ratio <= NORMAL_ULPS * (1 + 1e-3)).all())
        for i in range(B):   # and the bits of the fill entry point on the same counter
            flat = torch.empty(per, device=dev)
            L.check(L.load().nlam_philox_normal_fill(_ptr(flat), per, SEED, T, i, DRAW & 0xFFFFFFFF, _stream()), "nlam_philox_normal_fill")
            assert torch.equal(_bits(flat.cpu()), _bits(eps[i].reshape(-1))), i
    z64, term, mag = E.forward(pq, pp, eps)
    mu_q, raw_q, _, _ = E.split(pq, pp)
    s_q, _ = E.stds(raw_q, None)
    worst = {}
    z_budget = C_Z * U * (mu_q.abs() + (s_q * eps.double()).abs())
    worst["z"] = float(((b.z.t.cpu().double() - z64).abs() / z_budget).max())
    depth = _depth(per)
    kl_budget = (C_TERM + depth) * U * mag.sum((1, 2))
    worst["kl"] = float(((b.kl.t.cpu().double() - term.sum((1, 2))).abs() / kl_budget).max())
    w32, gt32 = float(np.float32(W)), float(np.float32(GT))
    term_budget = abs(w32) * (C_TERM + depth + math.ceil(B / 256) + 9) * U * float(mag.sum())
    worst["kl_term"] = abs(float(b.term.t.cpu().double()) - w32 * float(term.sum())) / term_budget
    g_pq, g_pp, mag_pq, mag_pp = E.backward(pq, pp, eps, g_z, gt32 * w32)
    c_pq = torch.cat((torch.full((D,), float(C_GMU)), torch.full((D,), float(C_GRAW_Q)))).double()
    worst["g_pq"] = float(((b.g_pq.t.cpu().double() - g_pq).abs() / (c_pq * U * mag_pq)).max())
    c_pp = torch.cat((torch.full((D,), float(C_GMU)), torch.full((D,), float(C_GRAW_P))))[:pp.shape[-1]].double()
    pp_budget = c_pp * U * mag_pp
    diff_pp = (b.g_pp.t.cpu().double() - g_pp).abs()
    worst["g_pp"] = float(torch.where(pp_budget > 0, diff_pp / pp_budget.clamp(min=1e-300), diff_pp * 1e300).max())
    print(f"{shape} diagonal {diagonal} misaligned {misalign} given {given}: error / budget " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= SLACK, (k, v)
    assert bool(torch.isfinite(b.kl.t).all()) and float(b.kl.t.min()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("diagonal", [False, True], ids=["isotropic", "diagonal"])
def test_kernel_null_pointers_reruns_and_q_equal_p(dev, diagonal):
    B, R, D = 3, 7, 8
    prob = _problem(B, R, D, diagonal)
    a, _ = _run_kernels(dev, B, R, D, diagonal, False, False, problem=prob)
    again, _ = _run_kernels(dev, B, R, D, diagonal, False, False, problem=prob)
    for name in ("eps", "z", "kl", "term", "g_pq", "g_pp"):   # two runs, equal bits
        assert torch.equal(_bits(getattr(a, name).t), _bits(getattr(again, name).t)), name
    # g_pp == NULL: the prior's gradient is not written, everything else keeps its bits
    no_pp, _ = _run_kernels(dev, B, R, D, diagonal, False, False, problem=prob, with_g_pp=False)
    assert bool(torch.isnan(no_pp.g_pp.t).all()) and torch.equal(_bits(no_pp.g_pq.t), _bits(a.g_pq.t))
    # g_latent == NULL is a zero cotangent
    zero = (prob[0], prob[1], prob[2], torch.zeros_like(prob[3]))
    z0, _ = _run_kernels(dev, B, R, D, diagonal, False, False, problem=zero)
    null, _ = _run_kernels(dev, B, R, D, diagonal, False, False, problem=prob, with_g_z=False)
    assert torch.equal(_bits(null.g_pq.t), _bits(z0.g_pq.t)) and torch.equal(_bits(null.g_pp.t), _bits(z0.g_pp.t))
    # another draw, another AR step, another seed: other noise
    for kw in (dict(draw=(7 << 32) + 6), dict(t=4), dict(seed=0x1234ABCD9877)):
        other, _ = _run_kernels(dev, B, R, D, diagonal, False, False, problem=prob, **kw)
        assert float((_bits(other.eps.t) == _bits(a.eps.t)).float().mean()) < 1e-2, kw
    high, _ = _run_kernels(dev, B, R, D, diagonal, False, False, problem=prob, draw=5)   # the low word of draw counts
    assert torch.equal(_bits(high.eps.t), _bits(a.eps.t))
    # q == p: every element's term is exactly 0
    pq = prob[0].clone()
    if diagonal:
        pp = pq.clone()
    else:
        pq[..., D:] = math.log(math.expm1(1 - 1e-4))
        pp = pq[..., :D].clone()
    same, _ = _run_kernels(dev, B, R, D, diagonal, False, False, problem=(pq, pp, prob[2], prob[3]))
    if diagonal:
        assert float(same.kl.t.abs().max()) == 0.0 and float(same.term.t) == 0.0
    else:   # s_q = 1e-4 + softplus(raw) is 1 within a few ulp: r^2 / 2 - 1 / 2 - log r is second order in r - 1
        assert float(same.kl.t.abs().max()) <= R * D * (16 * U) and float(same.term.t.abs()) <= B * R * D * 16 * U


# ---------------------------------------------------------------------------
# GPU: the objective against the torch composition
# ---------------------------------------------------------------------------
def _world(name, dev, root, B, T, loss="nll", kl_beta=1.0, seed=3):
    from neural_lam_amd import models as hm

    case, ds, model = _cpu_world(root, name)
    step = hm.EFMForecasterStep(hm.EFMForecaster(model, ds), ds, loss=loss, kl_beta=kl_beta, seed=seed, rank=0).to(dev)
    g = torch.Generator().manual_seed(23)
    N = ds.num_grid_points
    w = types.SimpleNamespace(case=case, ds=ds, step=step, model=model, N=N, B=B, T=T)
    w.init = (torch.randn(B, 2, N, 5, generator=g) * 0.5).to(dev)
    w.target = (torch.randn(B, T, N, 5, generator=g) * 0.5).to(dev)
    w.forcing = torch.randn(B, T, N, 6, generator=g).to(dev)
    return w


def _fused_noise(step, B, T):
    """The noise the step's NEXT forward draws, read back from the fused path: nlam_latent_kl_fwd on zero parameters under the
    step's own seed word and draw + 1 (the draw does not depend on the parameters)."""
    lib = L.load()
    model = step.forecaster.predictor
    R, D = int(model.latent_spatial_dim), int(model.latent_dim)
    dev = step.seed.device
    klw = step.kl_weight_word(B, T)
    nxt = step.draw + 1
    out = torch.empty((B, T, R, D), device=dev)
    zeros = torch.zeros((B, R, 2 * D), device=dev)
    for t in range(T):
        eps, z, kl, term = torch.empty((B, R, D), device=dev), torch.empty((B, R, D), device=dev), torch.empty(B, device=dev), torch.empty(1, device=dev)
        nws = lib.nlam_latent_kl_workspace_floats(B, R, D)
        ws = torch.empty(nws, device=dev)
        p = L.LatentKl()
        p.pq, p.pp, p.kl_weight, p.seed, p.draw = _ptr(zeros), _ptr(zeros), _ptr(klw), _ptr(step.seed), _ptr(nxt)
        p.eps, p.latent, p.kl, p.kl_term, p.workspace, p.workspace_floats = _ptr(eps), _ptr(z), _ptr(kl), _ptr(term), _ptr(ws), nws
        p.batch, p.rows, p.latent_dim, p.diagonal, p.t = B, R, D, 1, t
        L.check(lib.nlam_latent_kl_fwd(C.byref(p), _stream()), "nlam_latent_kl_fwd")
        out[:, t] = eps
    return out


def _torch_elbo(w, noise, kl_beta, loss_name):
    """The same modules composed from torch ops: torch.distributions for the posterior, the prior and their KL, the predictor's
    own unfused tail (rescale, get_clamped_new_state, softplus), the boundary mix and models.<loss> on the interior."""
    from torch.distributions import kl_divergence

    from neural_lam_amd import models as hm

    step, fc, model = w.step, w.step.forecaster, w.model
    metric = hm.get_metric(loss_name)
    prev_prev, prev = w.init[:, 0], w.init[:, 1]
    liks, kls, preds = [], [], []
    with model.static_cache():
        for t in range(w.T):
            forcing, target = w.forcing[:, t], w.target[:, t]
            grid_prev_emb, graph_emb = model.embedd_grid_and_graph(prev, prev_prev, forcing)
            prior = model.prior_model(grid_prev_emb, graph_emb=graph_emb)
            post = model.encoder(model.embedd_grid_with_target(prev, prev_prev, forcing, target), graph_emb=graph_emb)
            z = post.mean + post.stddev * noise[:, t]
            kls.append(kl_divergence(post, prior).sum((1, 2)))
            pred_state, pred_std = model(prev, prev_prev, forcing, latent=z)
            new = fc.boundary_mask * target + fc.interior_mask * pred_state
            std = pred_std if pred_std is not None else step.per_var_std
            liks.append(metric(new, target, std, mask=step.interior_index))
            preds.append(new)
            prev_prev, prev = prev, new
    lik = torch.stack(liks).mean()
    kl = kl_beta / step.n_interior * torch.stack(kls).mean()
    return torch.stack(preds, dim=1), lik, kl


@pytest.mark.gpu
@pytest.mark.parametrize("loss,kl_beta", [("nll", 1.0), ("nll", 0.0), ("wmse", 0.5)])
@pytest.mark.parametrize("name", EFM_CASES)
def test_objective_and_gradients_match_the_torch_composition(dev, tmp_path, monkeypatch, name, loss, kl_beta):
    from neural_lam_amd import models as hm

    B = load_golden(name)["prev"].shape[0]
    w = _world(name, dev, tmp_path, B, 2, loss=loss, kl_beta=kl_beta)
    step, model = w.step, w.model
    noise = _fused_noise(step, B, 2)
    assert bool(torch.isfinite(noise).all()) and float(noise.std()) > 0.5
    pred, total = step(w.init, w.target, w.forcing)          # draws (seed, draw 1) itself
    lik, kl = (t.clone() for t in step.last_terms)
    assert step.draw_state()["draw"] == 1
    total.backward()
    fused = {k: (None if p.grad is None else p.grad.clone()) for k, p in step.named_parameters()}
    step.zero_grad(set_to_none=True)
    # the same call on the noise read back: the same bits, and the draw count does not move
    pred_n, total_n = step(w.init, w.target, w.forcing, latent_noise=noise)
    assert torch.equal(_bits(pred_n), _bits(pred)) and torch.equal(_bits(total_n), _bits(total)) and step.draw_state()["draw"] == 1
    step.zero_grad(set_to_none=True)
    monkeypatch.setattr(hm, "FUSED_STATE_UPDATE", False)
    ref_pred, ref_lik, ref_kl = _torch_elbo(w, noise, kl_beta, loss)
    (ref_lik + ref_kl).backward()
    print(f"{name} {loss} beta {kl_beta}: loss {float(total.detach()):.6f} / {float((ref_lik + ref_kl).detach()):.6f}, likelihood {float(lik):.6f} / "
          f"{float(ref_lik.detach()):.6f}, kl {float(kl):.6g} / {float(ref_kl.detach()):.6g}")
    assert rel_err(pred, ref_pred) < TOL
    assert rel_err(lik, ref_lik) < TOL and rel_err(total, ref_lik + ref_kl) < TOL
    if kl_beta == 0.0:
        assert float(kl) == 0.0 and float(ref_kl.detach()) == 0.0
    else:
        assert rel_err(kl, ref_kl) < TOL and float(kl) > 0
    learn_prior = w.case["model_kwargs"].get("learn_prior", True)
    names = [k for k, _ in step.named_parameters()]
    assert any(".encoder." in k for k in names) and any("grid_current_embedder" in k for k in names)
    assert any(".prior_model." in k for k in names) == learn_prior
    worst = ("", 0.0)
    for k, p in step.named_parameters():
        got, ref = fused[k], p.grad
        if learn_prior:
            assert got is not None and ref is not None, k   # what the feature exists for: no parameter is left without a gradient
        if ref is None or float(ref.abs().max()) == 0.0:
            assert got is None or float(got.abs().max()) == 0.0, k
            continue
        assert got is not None, k
        err = rel_err(got, ref)
        worst = max(worst, (k, err), key=lambda kv: kv[1])
        assert err < TOL, (k, err)
    print(f"  worst gradient: {worst[0]} {worst[1]:.3g}")
    # FUSED_STATE_UPDATE is still off: the forecaster's fall-back (the unfused tail and one ops.LossFunction pass over the rollout)
    off = step.evaluate(w.init, w.target, w.forcing, latent_noise=noise)
    assert rel_err(off.loss, total) < TOL and rel_err(off.prediction, pred) < TOL and rel_err(off.likelihood, lik) < TOL
    monkeypatch.setattr(hm, "FUSED_STATE_UPDATE", True)
    # evaluate: the launches of forward without a graph, on its own draw counter
    ev = step.evaluate(w.init, w.target, w.forcing, latent_noise=noise)
    assert torch.equal(_bits(ev.loss), _bits(total)) and torch.equal(_bits(ev.prediction), _bits(pred)) and not ev.loss.requires_grad
    assert ev.kl_per_item.shape == (2, B) and step.draw_state()["draw"] == 1
    ev2 = step.evaluate(w.init, w.target, w.forcing, phase="test", steps_to_log=(1, 2, 5))
    assert step.draw_state()["draw"] == 1 and int(step.eval_draw) == (1 << 31) + 1 and bool(torch.isfinite(ev2.loss))
    # it is ForecasterStep.evaluate's EvalResult too: the metric pass on the rollout's predictions
    assert isinstance(ev2, hm.EvalResult) and ev2.phase == "test" and ev2.map_steps == (1, 2) and ev2.batch_size == B
    assert ev2.time_step_loss.shape == (2,) and ev2.entry_mse.shape == (B, 2, 5) and ev2.entry_mae.shape == (B, 2, 5)
    assert ev2.spatial_loss.shape == (B, 2, w.N) and rel_err(ev2.mean_loss, ev2.likelihood) < 1e-5   # the same loss on the same rollout
    assert ev.phase == "val" and ev.entry_mae is None and rel_err(ev.mean_loss, lik) < 1e-5
    with pytest.raises(ValueError):
        step.evaluate(w.init, w.target, w.forcing, phase="train")


@pytest.mark.gpu
def test_operator_refuses_cpu_tensors_and_marks_kl_per_item(dev):
    from neural_lam_amd.ops import LatentKLFunction

    pq, pp, eps, _ = _problem(2, 7, 8, True)
    klw = torch.tensor([0.1], device=dev)
    seed, draw = torch.tensor([5], dtype=torch.int64, device=dev), torch.tensor([1], dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError):
        LatentKLFunction.apply(pq, pp, klw, seed, draw, 0, None)
    pq_d, pp_d = pq.to(dev).requires_grad_(), pp.to(dev)   # a prior without a gradient (the constant prior)
    z, term, kl = LatentKLFunction.apply(pq_d, pp_d, klw, seed, draw, 0, eps.to(dev))
    assert z.requires_grad and term.requires_grad and not kl.requires_grad
    (z.sum() + term).backward()
    assert pq_d.grad is not None and pp_d.grad is None
    ref = E.backward(pq, pp, eps, torch.ones_like(eps), float(np.float32(0.1)))[0]
    assert rel_err(pq_d.grad.cpu().double(), ref) < 1e-5


# ---------------------------------------------------------------------------
# GPU: inside the Trainer
# ---------------------------------------------------------------------------
def _trainer_world(dev, root, use_graph=True, seed=3, **kw):
    from neural_lam_amd.trainer import Trainer

    w = _world("efm_hi_81x30", dev, root, 2, 2, seed=seed)
    w.tr = Trainer(w.step, lr=1e-3, use_graph=use_graph, **kw)
    return w


def _encoder_weights(w):
    return torch.cat([p.detach().reshape(-1) for k, p in w.step.named_parameters() if ".encoder." in k]).clone()


def _all_weights(w):
    return torch.cat([p.detach().reshape(-1) for p in w.step.parameters()]).clone()


@pytest.mark.gpu
def test_step_inside_the_trainer(dev, tmp_path):
    a = _trainer_world(dev, tmp_path / "a")
    enc0 = _encoder_weights(a)
    losses_a = [a.tr.step(a.init, a.target, a.forcing).clone() for _ in range(3)]
    assert a.tr.use_graph and a.tr._graph is not None   # the recording did not fall back to eager launches
    vals = [float(x) for x in losses_a]
    assert len(set(vals)) == 3 and all(math.isfinite(v) for v in vals), vals
    assert not torch.equal(_encoder_weights(a), enc0)
    assert a.step.draw_state()["draw"] == 3   # the warm-up passes of the recording are not counted
    # a fresh trainer from the same weights, reseeded: the same three losses and weights, bit for bit
    b = _trainer_world(dev, tmp_path / "b", seed=99)
    b.step.reseed(3, 0)
    losses_b = [b.tr.step(b.init, b.target, b.forcing).clone() for _ in range(3)]
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(losses_a, losses_b))
    assert torch.equal(_bits(_all_weights(a)), _bits(_all_weights(b)))
    # without the graph: the same bits as the replays
    c = _trainer_world(dev, tmp_path / "c", use_graph=False)
    losses_c = [c.tr.step(c.init, c.target, c.forcing).clone() for _ in range(3)]
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(losses_a, losses_c)), (vals, [float(x) for x in losses_c])
    assert torch.equal(_bits(_all_weights(a)), _bits(_all_weights(c)))
    # annealing: a new kl_beta changes the loss of the next replay and records nothing
    graph = a.tr._graph
    a.step.set_kl_beta(0.0)
    loss0 = a.tr.step(a.init, a.target, a.forcing)
    lik, kl = a.step.last_terms
    assert a.tr._graph is graph and float(kl) == 0.0 and torch.equal(_bits(loss0), _bits(lik.reshape(())))
    a.step.set_kl_beta(5.0)
    a.tr.step(a.init, a.target, a.forcing)
    assert a.tr._graph is graph and float(a.step.last_terms[1]) > 0


@pytest.mark.gpu
def test_micro_batches_of_an_accumulation_window_draw_different_noise(dev, tmp_path):
    a = _trainer_world(dev, tmp_path, accumulate_grad_batches=2)
    before = _all_weights(a)
    first = a.tr.step(a.init, a.target, a.forcing).clone()
    assert torch.equal(_bits(_all_weights(a)), _bits(before))   # the window is open: same weights, same batch ...
    second = a.tr.step(a.init, a.target, a.forcing).clone()
    assert float(first) != float(second)                         # ... other noise
    assert not torch.equal(_all_weights(a), before) and a.step.draw_state()["draw"] == 2


@pytest.mark.gpu
def test_calls_at_another_batch_shape_do_not_change_what_the_recorded_step_reads(dev, tmp_path):
    """kl_weight holds 1 / (B T): a recorded step must keep the word of ITS shape while ``evaluate`` on a validation batch of
    another size and rollout length, or the eager step Trainer makes of a last partial batch, run between its replays.  The run
    with those calls gives the bits of the run without them."""
    a, b = _trainer_world(dev, tmp_path / "a"), _trainer_world(dev, tmp_path / "b")
    small = (a.init[:1], a.target[:1, :1], a.forcing[:1, :1])   # (B, T) = (1, 1) against the recording's (2, 2)
    la, lb = [], []
    for w, out in ((a, la), (b, lb)):
        out.append(w.tr.step(w.init, w.target, w.forcing).clone())
    ev = a.step.evaluate(*small)
    assert ev.prediction.shape[:2] == (1, 1) and bool(torch.isfinite(ev.loss))
    for w, out in ((a, la), (b, lb)):
        out.append(w.tr.step(w.init, w.target, w.forcing).clone())
    for w in (a, b):
        w.step.set_kl_beta(0.3)
    a.step.evaluate(*small)
    with torch.no_grad():
        a.step(*small, latent_noise=torch.zeros(1, 1, int(a.model.latent_spatial_dim), int(a.model.latent_dim), device=dev))
    for w, out in ((a, la), (b, lb)):
        out.append(w.tr.step(w.init, w.target, w.forcing).clone())
    assert a.tr._graph is not None and float(a.step.last_terms[1]) > 0
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(la, lb)), ([float(x) for x in la], [float(x) for x in lb])
    assert torch.equal(_bits(_all_weights(a)), _bits(_all_weights(b)))
    # the words: one per shape, each with its own 1 / (B T), both annealed
    n = a.step.n_interior
    assert float(a.step.kl_weight_word(2, 2)) == np.float32(0.3 / (n * 4)) and float(a.step.kl_weight_word(1, 1)) == np.float32(0.3 / n)
    # a last partial batch through the trainer (an eager step: it trains, so only its own sanity and the word are checked)
    part = a.tr.step(a.init[:1], a.target[:1], a.forcing[:1])
    assert bool(torch.isfinite(part)) and float(a.step.kl_weight_word(2, 2)) == np.float32(0.3 / (n * 4))
    again = a.tr.step(a.init, a.target, a.forcing)
    assert a.tr.use_graph and bool(torch.isfinite(again))


@pytest.mark.gpu
def test_evaluate_is_served_by_the_graphed_eval_step_and_the_forecaster_by_a_plain_step(dev, tmp_path):
    from neural_lam_amd import models as hm
    from neural_lam_amd.trainer import graphed_eval_step

    w = _world("efm_ms_30x27", dev, tmp_path, 2, 2)
    val = graphed_eval_step(w.step, w.init, w.target, w.forcing, phase="val")
    first = val(w.init, w.target, w.forcing)
    loss1, draw1 = first.loss.clone(), int(w.step.eval_draw)
    second = val(w.init, w.target, w.forcing)
    assert isinstance(second, hm.EFMEvalResult) and int(w.step.eval_draw) == draw1 + 1 and w.step.draw_state()["draw"] == 0
    assert float(second.loss) != float(loss1) and bool(torch.isfinite(second.mean_loss))   # a replay draws new noise
    # EFMForecaster without the objective's arguments is ARForecaster: a plain ForecasterStep over it rolls out prior samples
    plain = hm.ForecasterStep(w.step.forecaster, w.ds, loss="nll").to(dev)
    with torch.no_grad():
        pred, loss = plain(w.init, w.target, w.forcing)
    assert pred.shape == w.target.shape and bool(torch.isfinite(loss))
    res = plain.evaluate(w.init, w.target, w.forcing, phase="test", steps_to_log=(1,))
    assert type(res) is hm.EvalResult and bool(torch.isfinite(res.mean_loss))


@pytest.mark.gpu
def test_resume_continues_the_noise_sequence(dev, tmp_path):
    from neural_lam_amd.checkpoint import load_checkpoint, save_checkpoint

    a = _trainer_world(dev, tmp_path / "a")
    for _ in range(2):
        a.tr.step(a.init, a.target, a.forcing)
    path = tmp_path / "efm.ckpt"
    save_checkpoint(path, a.tr, epoch=0, global_step=2, extra=a.step.draw_state())
    want = [a.tr.step(a.init, a.target, a.forcing).clone() for _ in range(2)]
    b = _trainer_world(dev, tmp_path / "b", seed=1234)
    with torch.no_grad():
        for p in b.step.parameters():
            p.mul_(0.5)   # not the saved weights
    ckpt = load_checkpoint(path, b.tr)
    extra = ckpt["neural_lam_amd"]["extra"]
    assert extra == {"seed": 3, "draw": 2, "kl_beta": 1.0}
    b.step.load_draw_state(extra)
    got = [b.tr.step(b.init, b.target, b.forcing).clone() for _ in range(2)]
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(want, got)), ([float(x) for x in want], [float(x) for x in got])
    assert torch.equal(_bits(_all_weights(a)), _bits(_all_weights(b)))


@pytest.mark.gpu
def test_trained_predictor_runs_in_the_ensemble_forecast(dev, tmp_path):
    from neural_lam_amd.data import DeviceWeatherDataset
    from neural_lam_amd.forecast import EnsembleForecast

    a = _trainer_world(dev, tmp_path)
    for _ in range(2):
        a.tr.step(a.init, a.target, a.forcing)
    step = a.step
    g = torch.Generator().manual_seed(17)
    times_n = 12
    state = (torch.randn(times_n, a.N, 5, generator=g) * 0.5).to(dev) * step.state_std + step.state_mean
    forcing = torch.randn(times_n, a.N, 2, generator=g).to(dev)
    times = (torch.arange(times_n, dtype=torch.int64) * 10 + 1000).to(dev)
    data = DeviceWeatherDataset(state, forcing, times, ar_steps=1, standardization=step.standardization_stats())
    ens = EnsembleForecast(step, data, 2, members=3, n_starts=1, seed=11)   # the step as it is: no re-wrapping
    res = ens.run([1])
    assert res.members.shape == (1, 3, 2, a.N, 5) and bool(torch.isfinite(res.members).all())
    assert bool(torch.isfinite(res.spread).all()) and float(res.spread.max()) > 0
