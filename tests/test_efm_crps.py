"""The ensemble CRPS fine-tuning term of Graph-EFM training (models.EFMForecasterStep(crps_members=M), ops.LatentDrawFunction,
ops.CrpsEnsFunction, nlam_latent_draw_fwd / _bwd, nlam_crps_ens_fwd / _bwd).  Without a GPU: the C-ABI (exports, layouts, argument
checks, workspace query), the float64 reference of crps_ref.py against a brute-force double loop, float64 autograd and the
closed-form Gaussian CRPS, and the step's host logic.  On the GPU: the kernels against that float64 math element by element (ties
included), the objective and every parameter gradient against the torch-op route on the same member states, the step inside
Trainer (replays, the weight word, resume), and evaluate.

The budgets of the kernel tests, in u = 2^-24 (first order), counted on the operations the kernels document:
  CRPS element  wc (sa / M - sp / (M (M - 1))), mag = |wc| (sa / M + sp / (M (M - 1))):
    sa = sum_m |x_m - y|: 1 u per difference + M - 1 additions, times 1 / M (1 u) and the product (1 u): (M + 2) u
    sp = sum_{i<j} |x_i - x_j| over P = M (M - 1) / 2 pairs, the same way: (P + 2) u
    the difference 1 u, wc = w_n c_f 1 u, the last product 1 u:                    C_EL = max(M, P) + 5 u of mag
  crps[b]: plus the additions on the longest path of the fixed-order reduction -- 4 elements per quad over
    ceil(quads / (blocks * 256)) grid-stride passes in one thread, 6 levels of the wave tree, 2 for the four waves, blocks - 1
    for the partials in block order (the scheme test_efm_training.py counts for the KL):   (C_EL + depth) u sum mag
  term: ceil(B / 256) items per thread, 8 levels for the 256 threads, 1 for the weight:   (C_EL + depth + ceil(B / 256) + 9) u
  g_pred = (gw wc) (sgn / M - pairs / (M (M - 1))), gw = g_term * weight: gw 1 u, wc 1 u, their product 1 u, 1 / M and
    1 / (M (M - 1)) 1 u each with the (exact integer) sign sums' products 1 u, the difference 1 u, the last product 1 u:  C_G = 8 u
    of |gw wc| (|sgn| / M + |pairs| / (M (M - 1))); where that is 0 (ties) the gradient is exactly 0.
  draw: z = mean + std eps: C_Z = 13 u (|mean| + |std eps|) as for the posterior draw; g_params[.., :D] = g exactly;
    g_params[.., D:] = g eps softplus'(raw): two products and softplus' (G = 8 u): C_GRAW = 11 u."""
import ctypes as C
import math
import re
import types

import numpy as np
import pytest
import torch

import crps_ref as R
import elbo_ref as E
from conftest import ROOT, load_golden, rel_err
from neural_lam_amd import _lib as L
from test_efm_training import (EFM_CASES, EPS32, MAX_BLOCKS, NORMAL_ULPS, PASS_ELEMENTS, SLACK, TOL, U, _all_weights, _bits, _blocks, _Buf,
                               _c_layout, _cpu_world, _depth, _ptr, _stream)

NEW_EXPORTS = ["nlam_latent_draw_fwd", "nlam_latent_draw_bwd", "nlam_crps_ens_fwd", "nlam_crps_ens_bwd", "nlam_crps_ens_workspace_floats"]
C_Z, C_GRAW, C_G = 13, 11, 8
# the launcher's cap is the KL's (csrc/nlam_crps_ens.inc launches latent_kl_blocks(nodes * nvars) workgroups per item): MAX_BLOCKS = 64
# workgroups of 256 threads, a quad of 4 elements per thread -- one pass of the capped grid covers PASS_ELEMENTS = 65536 elements
CRPS_SHAPES = [(1, 2, 5, 3), (3, 3, 7, 8), (2, 4, 1, 17), (2, 8, 33, 5), (1, 5, 9, 4), (1, 16, 9, 4), (2, 2, 3900, 17), (1, 2, 4100, 16)]
# 66 300 elements per item, past the 64-block cap, for the instantiations M = 3, 4, 8 and the generic one (M = 5, 16)
CRPS_SHAPES += [(1, M, 3900, 17) for M in (3, 4, 8, 5, 16)]
DRAW_SHAPES = [(1, 5, 3), (3, 7, 8), (2, 1031, 65), (1, 1100, 64)]


def _c_el(M):
    return max(M, M * (M - 1) // 2) + 5


# ---------------------------------------------------------------------------
# CPU: the C-ABI
# ---------------------------------------------------------------------------
def test_crps_symbols_are_exported_and_the_structs_match_c_layout(tmp_path):
    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.nlam_abi_version() == 8 == L.ABI_VERSION
    _c_layout(tmp_path, L.LatentDraw, "nlam_latent_draw_t")
    _c_layout(tmp_path, L.CrpsEns, "nlam_crps_ens_t")
    assert re.search(r"#define NLAM_CRPS_MAX_MEMBERS 16\b", header) and L.CRPS_MAX_MEMBERS == 16


def test_crps_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    B, M, N, F = 3, 4, 9, 8
    nws = lib.nlam_crps_ens_workspace_floats(B, M, N, F)
    assert nws == B * _blocks(N * F)
    for bad in ((0, M, N, F), (B, 1, N, F), (B, 0, N, F), (B, M, 0, F), (B, M, N, 0), (-1, M, N, F)):
        assert lib.nlam_crps_ens_workspace_floats(*bad) == -1, bad
    for bad in ((B, 17, N, F), (B, M, N, 4097), (B, M, 1 << 20, 1 << 11)):
        assert lib.nlam_crps_ens_workspace_floats(*bad) == -2, bad
    sizes = [lib.nlam_crps_ens_workspace_floats(B, M, n, F) for n in (1, 100, 1000, 10000, 100000)]
    assert sizes == sorted(sizes) and sizes[-1] == B * MAX_BLOCKS   # monotone, capped
    assert lib.nlam_crps_ens_workspace_floats(2 * B, M, N, F) == 2 * nws   # linear in batch
    assert lib.nlam_crps_ens_workspace_floats(B, 2, N, F) == nws == lib.nlam_crps_ens_workspace_floats(B, 16, N, F)

    def args(**kw):
        p = L.CrpsEns()
        for name in ("pred", "target", "row_weight", "var_weight", "weight", "crps", "term", "workspace", "g_term", "g_pred"):
            setattr(p, name, fake)
        p.workspace_floats, p.batch, p.members, p.nodes, p.nvars = nws, B, M, N, F
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    for entry in (lib.nlam_crps_ens_fwd, lib.nlam_crps_ens_bwd):
        assert entry(None, None) == -1
        for kw in (dict(pred=None), dict(target=None), dict(row_weight=None), dict(weight=None), dict(batch=0), dict(members=1),
                   dict(members=0), dict(members=-3), dict(nodes=0), dict(nvars=0)):
            assert entry(args(**kw), None) == -1, kw
        for kw in (dict(members=17), dict(batch=65536, workspace_floats=1 << 40), dict(nvars=4097),
                   dict(nodes=1 << 20, nvars=1 << 11, workspace_floats=1 << 40)):
            assert entry(args(**kw), None) == -2, kw
    for kw in (dict(crps=None), dict(term=None), dict(workspace=None), dict(workspace_floats=nws - 1)):
        assert lib.nlam_crps_ens_fwd(args(**kw), None) == -1, kw
    for kw in (dict(g_term=None), dict(g_pred=None)):
        assert lib.nlam_crps_ens_bwd(args(**kw), None) == -1, kw

    def dargs(**kw):
        p = L.LatentDraw()
        for name in ("params", "noise_in", "seed", "draw", "eps", "latent", "g_latent", "g_params"):
            setattr(p, name, fake)
        p.batch, p.rows, p.latent_dim, p.diagonal, p.t = B, N, F, 1, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    for entry in (lib.nlam_latent_draw_fwd, lib.nlam_latent_draw_bwd):
        assert entry(None, None) == -1
        for kw in (dict(params=None), dict(eps=None), dict(batch=0), dict(rows=0), dict(latent_dim=0), dict(diagonal=2), dict(diagonal=-1),
                   dict(t=-1)):
            assert entry(dargs(**kw), None) == -1, kw
        assert entry(dargs(batch=65536), None) == -2
        assert entry(dargs(rows=1 << 16, latent_dim=1 << 15), None) == -2
    for kw in (dict(latent=None), dict(noise_in=None, seed=None), dict(noise_in=None, draw=None)):
        assert lib.nlam_latent_draw_fwd(dargs(**kw), None) == -1, kw
    assert lib.nlam_latent_draw_bwd(dargs(g_latent=None), None) == -1
    assert lib.nlam_latent_draw_bwd(dargs(g_params=None), None) == 0   # a constant prior: checked, nothing launched


# ---------------------------------------------------------------------------
# CPU: the float64 reference
# ---------------------------------------------------------------------------
def _crps_problem(B, M, N, F, seed=0):
    """fp32 members, target and weights with ties built in: element i (flat over B, N, F) has members 0 and 1 bit-equal where
    i % 7 == 0 and the last member bit-equal to the target where i % 13 == 0; every third row weight is 0."""
    g = torch.Generator().manual_seed(10000 * B + 1000 * M + 10 * N + F + seed)
    x = torch.randn(B, M, N, F, generator=g)
    y = torch.randn(B, N, F, generator=g)
    i = torch.arange(B * N * F).reshape(B, N, F)
    x[:, 1] = torch.where(i % 7 == 0, x[:, 0], x[:, 1])
    y = torch.where(i % 13 == 0, x[:, M - 1], y)
    w = torch.rand(N, generator=g) + 0.1
    w[::3] = 0.0
    if N == 1:
        w[:] = 0.7
    c = torch.rand(F, generator=g) + 0.5
    assert float((x[:, 0] == x[:, 1]).float().mean()) >= 0.1 and float((x[:, M - 1] == y).float().mean()) >= 0.05
    return x, y, w, c


def test_reference_crps_is_the_double_loop_and_its_gradient_is_autograd():
    for B, M, N, F in ((2, 2, 5, 3), (1, 3, 4, 7), (2, 5, 3, 2)):
        x, y, w, c = _crps_problem(B, M, N, F)
        v, mag = R.bracket(x, y)
        brute = torch.zeros(B, N, F, dtype=torch.float64)
        for b in range(B):
            for n in range(N):
                for f in range(F):
                    xs, t = [float(x[b, m, n, f]) for m in range(M)], float(y[b, n, f])
                    skill = sum(abs(a - t) for a in xs) / M
                    pair = sum(abs(xs[i] - xs[j]) for i in range(M) for j in range(i + 1, M)) / (M * (M - 1))
                    brute[b, n, f] = skill - pair
        assert float((v - brute).abs().max()) <= 1e-14 * float(mag.max())
        if M == 2:
            x64, y64 = x.double(), y.double()
            two = ((x64[:, 0] - y64).abs() + (x64[:, 1] - y64).abs()) / 2 - (x64[:, 0] - x64[:, 1]).abs() / 2
            assert float((v - two).abs().max()) <= 1e-15 * float(mag.max())
        # the closed-form gradient against float64 autograd of the torch.abs composition: ties included (abs' is 0 at 0)
        x64 = x.double().requires_grad_()
        skill = (x64 - y.double()[:, None]).abs().sum(1) / M
        pair = (x64[:, :, None] - x64[:, None]).abs().sum((1, 2)) / (2 * M * (M - 1))
        wc = R.weights(w, c, F)
        total = 0.37 * ((skill - pair) * wc).sum()
        crps, term, _ = R.forward(x, y, w, c, 0.37)
        assert abs(float(total.detach()) - term) <= 1e-13 * abs(term) and abs(float(crps.sum()) * 0.37 - term) <= 1e-13 * abs(term)
        total.backward()
        g, gmag = R.backward(x, y, w, c, 0.37)
        assert float((g - x64.grad).abs().max()) <= 1e-14 * float(gmag.max())
        tie = (x[:, 0] == x[:, 1]) & (x[:, 0] == y) if M == 2 else None
        if tie is not None and bool(tie.any()):
            assert float(g[:, 0][tie].abs().max()) == 0.0
        assert torch.equal(R.backward(x, y, w, None, 0.37)[0], R.backward(x, y, w, torch.ones(F), 0.37)[0])


def test_reference_bracket_is_unbiased_for_the_gaussian_crps():
    """Members x_m ~ N(mu, sigma^2) i.i.d.: the mean of the bracket over K draws estimates CRPS(N(mu, sigma^2), y) without bias for
    every M >= 2.  The bound: 5 standard errors of that mean, from the sample variance of the K brackets themselves (a 5-sigma
    miss of a true estimator has probability < 1e-6); K = 200000 makes the standard error about 1e-3 of sigma."""
    K, mu, sigma, y = 200000, 0.3, 1.7, 1.1
    want = R.gaussian_crps(mu, sigma, y)
    for M in (2, 3, 5):
        g = torch.Generator().manual_seed(100 + M)
        x = mu + sigma * torch.randn(K, M, 1, 1, generator=g, dtype=torch.float64)
        v, _ = R.bracket(x, torch.full((K, 1, 1), y, dtype=torch.float64))
        v = v.reshape(-1)
        se = float(v.std(unbiased=True)) / math.sqrt(K)
        print(f"M {M}: mean bracket {float(v.mean()):.6f}, closed form {want:.6f}, standard error {se:.2e}")
        assert abs(float(v.mean()) - want) <= 5 * se and se < 5e-3 * sigma
    # the biased estimator (pairs over M^2) is what the test would catch: its expectation is off by E|x - x'| / (2 M) = sigma / (sqrt(pi) M)
    assert sigma / (math.sqrt(math.pi) * 5) > 5 * 5e-3 * sigma   # at M = 5, the largest count above


# ---------------------------------------------------------------------------
# CPU: host logic of the step
# ---------------------------------------------------------------------------
def test_step_host_logic_of_the_crps_stage(tmp_path):
    from neural_lam_amd import models as hm

    case, ds, model = _cpu_world(tmp_path)
    mk = lambda **kw: hm.EFMForecasterStep(hm.EFMForecaster(model, ds), ds, rank=0, **kw)   # noqa: E731
    for bad in (1, -1, -2, 17, 64):
        with pytest.raises(ValueError):
            mk(crps_members=bad)
    with pytest.raises(ValueError):
        mk(crps_weight=0.5)
    with pytest.raises(ValueError):
        mk(crps_members=0, crps_weight=-1.0)
    plain = mk(seed=77)
    assert plain.crps_members == 0 and plain.last_crps is None and len(plain.last_terms) == 2
    plain.reseed(77, draw=9)
    assert plain.draw_state() == {"seed": 77, "draw": 9, "kl_beta": 1.0}   # as it was
    assert "member_seed" not in dict(plain.named_buffers())
    with pytest.raises(ValueError):
        plain.set_crps_weight(1.0)
    step = mk(crps_members=2, crps_weight=0.5, seed=77)
    assert step.crps_members == 2 and mk(crps_members=16).crps_members == 16 and mk(crps_members=2).crps_weight == 0.0
    # the second key: the first plus the constant mod 2^64, never the first, never another rank's first
    off = 0xD1B54A32D192ED03
    first = [hm.EFMForecasterStep.noise_key(77, r) for r in range(8)]
    second = [hm.EFMForecasterStep.member_key(77, r) for r in range(8)]
    assert second == [(k + off) & 0xFFFFFFFFFFFFFFFF for k in first] == [R.member_key(77, r) for r in range(8)]
    assert len(set(first) | set(second)) == 16
    assert hm.EFMForecasterStep.member_key((1 << 64) - 1, 0) == off - 1   # wraps
    step.crps_weight_word(3, 4)
    assert int(step.member_seed) & 0xFFFFFFFFFFFFFFFF == second[0] and int(step.seed) & 0xFFFFFFFFFFFFFFFF == first[0]
    r1 = mk(crps_members=2, seed=77)
    r1.rank = 1
    r1.reseed(77)
    assert int(r1.member_seed) & 0xFFFFFFFFFFFFFFFF == second[1]
    # one word per batch shape, rewritten in place
    word, other = step.crps_weight_word(3, 4), step.crps_weight_word(1, 2)
    assert float(word) == np.float32(0.5 / 12) and float(other) == np.float32(0.5 / 2) and step.crps_weight_word(3, 4) is word
    assert step.crps_weight_value(3, 4) == 0.5 / 12
    step.set_crps_weight(2.0)
    assert step.crps_weight_word(3, 4) is word and float(word) == np.float32(2.0 / 12) and float(other) == np.float32(1.0)
    step.set_kl_beta(0.25)   # the KL words are their own
    assert float(word) == np.float32(2.0 / 12) and float(step.kl_weight_word(3, 4)) == np.float32(0.25 / (step.n_interior * 12))
    # the state round-trips
    step.reseed(77, draw=9)
    st = step.draw_state()
    assert st == {"seed": 77, "draw": 9, "kl_beta": 0.25, "crps_weight": 2.0}
    twin = mk(crps_members=2)
    twin.crps_weight_word(3, 4)
    twin.load_draw_state(st)
    assert twin.draw_state() == st and torch.equal(twin.member_seed, step.member_seed) and torch.equal(twin.seed, step.seed)
    assert torch.equal(twin.crps_weight_word(3, 4), word)
    twin.load_draw_state({"seed": 5, "draw": 1, "kl_beta": 1.0})   # a checkpoint of the ELBO stage: the weight stays
    assert twin.crps_weight == 2.0
    plain.load_draw_state(st)   # and a step without members ignores the key
    assert plain.draw_state() == {"seed": 77, "draw": 9, "kl_beta": 0.25}
    assert "member_seed" not in step.state_dict() and float(step.last_crps) == 0.0
    assert step.per_var_std is None and step.crps_var_weight is None   # a predicted std: c_f = 1
    case2, ds2, model2 = _cpu_world(tmp_path / "ms", "efm_ms_30x27")
    assert not model2.output_std
    fixed = hm.EFMForecasterStep(hm.EFMForecaster(model2, ds2), ds2, rank=0, crps_members=3)
    assert torch.equal(fixed.crps_var_weight, 1.0 / fixed.per_var_std) and fixed.crps_var_weight.shape == (5,)
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


def _run_crps(dev, prob, M, misalign, with_c=True, weight=0.013, g_term=1.7):
    lib = L.load()
    x, y, w, c = prob
    B, _, N, F = x.shape
    mk = lambda shape, value=None: _Buf(dev, shape, misalign, value)   # noqa: E731
    b = types.SimpleNamespace(x=mk((B * M, N, F), x.reshape(B * M, N, F)), y=mk((B, N, F), y), crps=mk((B,)), term=mk((1,)),
                              g=mk((B * M, N, F)))
    nws = lib.nlam_crps_ens_workspace_floats(B, M, N, F)
    ws = torch.full((nws,), float("nan"), device=dev)
    wt, gt, wd, cd = torch.tensor([weight], device=dev), torch.tensor([g_term], device=dev), w.to(dev), c.to(dev)
    p = L.CrpsEns()
    p.pred, p.target, p.row_weight, p.var_weight, p.weight = _ptr(b.x.t), _ptr(b.y.t), _ptr(wd), _ptr(cd) if with_c else None, _ptr(wt)
    p.crps, p.term, p.workspace, p.workspace_floats = _ptr(b.crps.t), _ptr(b.term.t), _ptr(ws), nws
    p.batch, p.members, p.nodes, p.nvars = B, M, N, F
    L.check(lib.nlam_crps_ens_fwd(C.byref(p), _stream()), "nlam_crps_ens_fwd")
    p.g_term, p.g_pred = _ptr(gt), _ptr(b.g.t)
    L.check(lib.nlam_crps_ens_bwd(C.byref(p), _stream()), "nlam_crps_ens_bwd")
    torch.cuda.synchronize()
    for name, buf in vars(b).items():
        assert buf.guards_intact(), name
    assert torch.equal(_bits(b.x.t.cpu()), _bits(x.reshape(B * M, N, F))) and torch.equal(_bits(b.y.t.cpu()), _bits(y))   # only read
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("with_c", [True, False], ids=["var_weight", "null_var_weight"])
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "off_by_one_float"])
@pytest.mark.parametrize("shape", CRPS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_crps_kernels_against_float64_math(dev, shape, misalign, with_c):
    """Budgets: the module docstring.  (2, 2, 3900, 17) and (1, 2, 4100, 16) hold more than PASS_ELEMENTS = 65536 elements per item:
    the capped grid of 64 workgroups strides a second time; the first has rows of 17 floats (a quad crosses rows), the second
    rows of 16.  M = 5 and 16 run the generic instantiation.  Every element is compared, ties included."""
    B, M, N, F = shape
    per = N * F
    if N > 1000:
        assert per > PASS_ELEMENTS and _blocks(per) == MAX_BLOCKS
    W, GT = 0.013, 1.7
    prob = _crps_problem(B, M, N, F)
    x, y, w, c = prob
    b = _run_crps(dev, prob, M, misalign, with_c, W, GT)
    cc = c if with_c else None
    w32, gt32 = float(np.float32(W)), float(np.float32(GT))
    crps, term, mag = R.forward(x, y, w, cc, w32)
    depth, worst = _depth(per), {}
    worst["crps"] = float(((b.crps.t.cpu().double() - crps).abs() / ((_c_el(M) + depth) * U * mag)).max())
    term_budget = abs(w32) * (_c_el(M) + depth + math.ceil(B / 256) + 9) * U * float(mag.sum())
    worst["term"] = abs(float(b.term.t.cpu().double()) - term) / term_budget
    gw = float(np.float32(gt32 * w32))   # the kernel's own first product, so that its rounding is not counted twice
    g, gmag = R.backward(x, y, w, cc, gw)
    got = b.g.t.cpu().double().reshape(B, M, N, F)
    diff, budget = (got - g).abs(), C_G * U * gmag
    assert float(got[gmag == 0].abs().sum()) == 0.0   # ties and zero weights: exactly 0
    worst["g_pred"] = float((diff[budget > 0] / budget[budget > 0]).max())
    print(f"{shape} misaligned {misalign} var_weight {with_c}: error / budget " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= SLACK, (k, v)
    again = _run_crps(dev, prob, M, misalign, with_c, W, GT)
    for name in ("crps", "term", "g"):   # two runs, equal bits
        assert torch.equal(_bits(getattr(b, name).t), _bits(getattr(again, name).t)), name


def _draw_problem(B, Rr, D, diagonal):
    g = torch.Generator().manual_seed(1000 * B + 10 * Rr + D + (500 if diagonal else 0))
    params = torch.randn(B, Rr, 2 * D if diagonal else D, generator=g) * 1.5
    if diagonal:   # raw stds on both sides of softplus' threshold and far below 0
        flat = params.view(-1, 2 * D)
        flat[0, D], flat[-1, 2 * D - 1] = 25.0, -30.0
        if B * Rr > 1:
            flat[1, D] = 19.5
    return params, torch.randn(B, Rr, D, generator=g), torch.randn(B, Rr, D, generator=g)


def _run_draw(dev, prob, D, misalign, given, seed=0x1234ABCD9876, draw=(7 << 32) + 5, t=3, with_g_params=True):
    lib = L.load()
    params, eps_in, g_z = prob
    B, Rr, P = params.shape
    mk = lambda shape, value=None: _Buf(dev, shape, misalign, value)   # noqa: E731
    b = types.SimpleNamespace(params=mk((B, Rr, P), params), noise=mk((B, Rr, D), eps_in) if given else None, eps=mk((B, Rr, D)),
                              z=mk((B, Rr, D)), g_z=mk((B, Rr, D), g_z), g_params=mk((B, Rr, P)))
    seed_t = torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64, device=dev)   # the 64 bits, signed
    draw_t = torch.tensor([draw], dtype=torch.int64, device=dev)
    p = L.LatentDraw()
    p.params, p.noise_in, p.eps, p.latent = _ptr(b.params.t), _ptr(b.noise.t) if given else None, _ptr(b.eps.t), _ptr(b.z.t)
    if not given:
        p.seed, p.draw = _ptr(seed_t), _ptr(draw_t)
    p.batch, p.rows, p.latent_dim, p.diagonal, p.t = B, Rr, D, int(P == 2 * D), t
    L.check(lib.nlam_latent_draw_fwd(C.byref(p), _stream()), "nlam_latent_draw_fwd")
    p.g_latent, p.g_params = _ptr(b.g_z.t), _ptr(b.g_params.t) if with_g_params else None
    L.check(lib.nlam_latent_draw_bwd(C.byref(p), _stream()), "nlam_latent_draw_bwd")
    torch.cuda.synchronize()
    assert int(draw_t) == draw and int(seed_t) & 0xFFFFFFFFFFFFFFFF == seed   # only read
    for name, buf in vars(b).items():
        assert buf is None or buf.guards_intact(), name
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("given", [True, False], ids=["given", "drawn"])
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "off_by_one_float"])
@pytest.mark.parametrize("diagonal", [False, True], ids=["isotropic", "diagonal"])
@pytest.mark.parametrize("shape", DRAW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_draw_kernels_against_float64_math(dev, shape, diagonal, misalign, given):
    B, Rr, D = shape
    per = Rr * D
    if Rr > 1000:
        assert per > PASS_ELEMENTS
    SEED, DRAW, T = 0x1234ABCD9876, (7 << 32) + 5, 3
    prob = _draw_problem(B, Rr, D, diagonal)
    params, eps_in, g_z = prob
    b = _run_draw(dev, prob, D, misalign, given, SEED, DRAW, T)
    eps = b.eps.t.cpu()
    if given:
        assert torch.equal(_bits(eps), _bits(eps_in))
    else:   # the generator's numbers for counter (quad, t, b, low word of draw)
        want = E.noise(SEED, DRAW, T, B, per)
        ratio = np.abs(eps.double().numpy().reshape(B, -1) - want) / (EPS32 * np.abs(want))
        print(f"noise {shape}: worst {ratio.max():.3f} ulp-units, bar {NORMAL_ULPS}")
        assert bool((ratio <= NORMAL_ULPS * (1 + 1e-3)).all())
    z64, zmag = R.draw(params, eps, D)
    worst = {"z": float(((b.z.t.cpu().double() - z64).abs() / (C_Z * U * zmag)).max())}
    got = b.g_params.t.cpu()
    assert torch.equal(_bits(got[..., :D]), _bits(g_z))   # the mean's gradient is the cotangent itself
    if diagonal:
        g64 = R.draw_backward(params, eps, g_z, D)[..., D:]
        worst["g_raw"] = float(((got[..., D:].double() - g64).abs() / (C_GRAW * U * g64.abs()).clamp(min=1e-300)).max())
    print(f"{shape} diagonal {diagonal} misaligned {misalign} given {given}: error / budget " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= SLACK, (k, v)
    if misalign and not given:   # g_params == NULL: nothing is written; two runs, equal bits; another key, other noise
        null = _run_draw(dev, prob, D, misalign, given, SEED, DRAW, T, with_g_params=False)
        assert bool(torch.isnan(null.g_params.t).all()) and bool(torch.isnan(null.g_params.raw).all())
        assert torch.equal(_bits(null.eps.t), _bits(b.eps.t)) and torch.equal(_bits(null.z.t), _bits(b.z.t))
        other = _run_draw(dev, prob, D, misalign, given, R.member_key(SEED, 0), DRAW, T)
        assert float((_bits(other.eps.t) == _bits(b.eps.t)).float().mean()) < 1e-2


@pytest.mark.gpu
def test_operators_refuse_cpu_tensors_and_mark_what_is_not_differentiable(dev):
    from neural_lam_amd.ops import CrpsEnsFunction, LatentDrawFunction, crps_ens_torch

    x, y, w, c = _crps_problem(2, 3, 7, 8)
    wt = torch.tensor([0.1], device=dev)
    with pytest.raises(RuntimeError):
        CrpsEnsFunction.apply(x.reshape(6, 7, 8), y, w, c, wt, 3)
    with pytest.raises(ValueError):
        CrpsEnsFunction.apply(x.reshape(6, 7, 8).to(dev), y.to(dev), w.to(dev), c.to(dev), wt, 4)
    xd = x.reshape(6, 7, 8).to(dev).requires_grad_()
    term, crps = CrpsEnsFunction.apply(xd, y.to(dev), w.to(dev), c.to(dev), wt, 3)
    assert term.requires_grad and not crps.requires_grad and crps.shape == (2,)
    term.backward()
    ref_g, ref_mag = R.backward(x, y, w, c, float(np.float32(0.1)))
    assert float((xd.grad.cpu().double().reshape(2, 3, 7, 8) - ref_g).abs().max()) <= 1e-5 * float(ref_mag.max())
    # the torch-op route on the same states: the same term and gradient within the parity bound
    xt = x.reshape(6, 7, 8).to(dev).requires_grad_()
    term_t, crps_t = crps_ens_torch(xt, y.to(dev), w.to(dev), c.to(dev), wt, 3)
    term_t.backward()
    assert rel_err(term, term_t) < TOL and rel_err(crps, crps_t) < TOL and rel_err(xd.grad, xt.grad) < TOL
    params, eps, _ = _draw_problem(2, 7, 8, True)
    seed, draw = torch.tensor([5], dtype=torch.int64, device=dev), torch.tensor([1], dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError):
        LatentDrawFunction.apply(params, 8, seed, draw, 0, None)
    z = LatentDrawFunction.apply(params.to(dev), 8, seed, draw, 0, eps.to(dev))   # a prior without a gradient (the constant prior)
    assert not z.requires_grad
    pd = params.to(dev).requires_grad_()
    z = LatentDrawFunction.apply(pd, 8, seed, draw, 0, eps.to(dev))
    z.sum().backward()
    ref = R.draw_backward(params, eps, torch.ones_like(eps), 8)
    assert rel_err(pd.grad.cpu().double(), ref) < 1e-5


# ---------------------------------------------------------------------------
# GPU: the objective
# ---------------------------------------------------------------------------
def _world(name, dev, root, B, T, seed=3, **kw):
    from neural_lam_amd import models as hm

    case, ds, model = _cpu_world(root, name)
    step = hm.EFMForecasterStep(hm.EFMForecaster(model, ds), ds, seed=seed, rank=0, **kw).to(dev)
    g = torch.Generator().manual_seed(23)
    N = ds.num_grid_points
    w = types.SimpleNamespace(case=case, ds=ds, step=step, model=model, N=N, B=B, T=T)
    w.init = (torch.randn(B, 2, N, 5, generator=g) * 0.5).to(dev)
    w.target = (torch.randn(B, T, N, 5, generator=g) * 0.5).to(dev)
    w.forcing = torch.randn(B, T, N, 6, generator=g).to(dev)
    return w


def _grads(step):
    return {k: (None if p.grad is None else p.grad.clone()) for k, p in step.named_parameters()}


def _noise(w, M, seed):
    g = torch.Generator().manual_seed(seed)
    Rr, D = int(w.model.latent_spatial_dim), int(w.model.latent_dim)
    dev = w.init.device
    return torch.randn(w.B, w.T, Rr, D, generator=g).to(dev), torch.randn(w.B * M, w.T, Rr, D, generator=g).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name,M", [(n, 2) for n in EFM_CASES] + [("efm_ms_30x27", 3)])
def test_objective_and_gradients_match_the_torch_op_route_on_the_same_member_states(dev, tmp_path, monkeypatch, name, M):
    """The comparison swaps only the term (models.FUSED_CRPS) and keeps the rollout's launches, so the member states of the two routes
    carry the same bits in the forward: |.| has a kink, and a rollout that differs by rounding could flip a sign at a near-tie."""
    from neural_lam_amd import models as hm

    B, T = 2, 2
    w = _world(name, dev, tmp_path, B, T, crps_members=M, crps_weight=0.7)
    step = w.step
    pred, total = step(w.init, w.target, w.forcing)          # draws (seed, draw 1) itself, posterior and members
    lik, kl = (t.clone() for t in step.last_terms)
    crps = step.last_crps.clone()
    assert step.draw_state()["draw"] == 1 and float(crps) > 0 and bool(torch.isfinite(total))
    assert torch.equal(_bits(total.detach().reshape(())), _bits(((lik + kl) + crps).reshape(())))
    total.backward()
    fused = _grads(step)
    step.zero_grad(set_to_none=True)
    step.reseed(3, 0)                                          # the same draws again
    monkeypatch.setattr(hm, "FUSED_CRPS", False)
    pred_t, total_t = step(w.init, w.target, w.forcing)
    crps_t = step.last_crps.clone()
    total_t.backward()
    monkeypatch.setattr(hm, "FUSED_CRPS", True)
    print(f"{name} M {M}: loss {float(total.detach()):.6f} / {float(total_t.detach()):.6f}, crps {float(crps):.6f} / {float(crps_t):.6f}, "
          f"likelihood {float(lik):.6f}, kl {float(kl):.6g}")
    assert torch.equal(_bits(pred), _bits(pred_t)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip((lik, kl), step.last_terms))
    assert rel_err(crps, crps_t) < TOL and rel_err(total, total_t) < TOL
    learn_prior = w.case["model_kwargs"].get("learn_prior", True)
    names = [k for k, _ in step.named_parameters()]
    assert any(".prior_model." in k for k in names) == learn_prior and any(".decoder." in k for k in names)
    worst = ("", 0.0)
    for k, p in step.named_parameters():
        got, ref = fused[k], p.grad
        if learn_prior:
            assert got is not None and ref is not None, k
        if ref is None or float(ref.abs().max()) == 0.0:
            assert got is None or float(got.abs().max()) == 0.0, k
            continue
        assert got is not None, k
        err = rel_err(got, ref)
        worst = max(worst, (k, err), key=lambda kv: kv[1])
        assert err < TOL, (k, err)
    print(f"  worst gradient: {worst[0]} {worst[1]:.3g}")
    # given noise for both rollouts: the draw count does not move, and the call is repeatable bit for bit
    zq, zm = _noise(w, M, 5)
    step.zero_grad(set_to_none=True)
    _, a = step(w.init, w.target, w.forcing, latent_noise=zq, member_noise=zm)
    _, b = step(w.init, w.target, w.forcing, latent_noise=zq, member_noise=zm)
    assert torch.equal(_bits(a), _bits(b)) and step.draw_state()["draw"] == 1
    with pytest.raises(ValueError):
        step(w.init, w.target, w.forcing, latent_noise=zq, member_noise=zm[:, :, :-1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["efm_hi_81x30", "efm_hi_constprior_81x30"])
def test_zero_weight_is_the_step_without_members_and_the_term_reaches_the_decoder(dev, tmp_path, name):
    B, T, M = 2, 2, 2
    base = _world(name, dev, tmp_path / "a", B, T)
    w = _world(name, dev, tmp_path / "b", B, T, crps_members=M, crps_weight=0.0)
    zq, zm = _noise(w, M, 7)
    _, loss0 = base.step(base.init, base.target, base.forcing, latent_noise=zq)
    loss0.backward()
    g0 = _grads(base.step)
    _, loss1 = w.step(w.init, w.target, w.forcing, latent_noise=zq, member_noise=zm)
    assert float(w.step.last_crps) == 0.0 and rel_err(loss1, loss0) < TOL
    loss1.backward()
    g1 = _grads(w.step)
    for k, ref in g0.items():
        if ref is None or float(ref.abs().max()) == 0.0:
            assert g1[k] is None or float(g1[k].abs().max()) == 0.0, k
        else:
            assert g1[k] is not None and rel_err(g1[k], ref) < TOL, k
    # with a weight the decoder's gradient moves; a constant prior has no parameters to move, a learnt one moves too
    w.step.zero_grad(set_to_none=True)
    w.step.set_crps_weight(0.7)
    _, loss2 = w.step(w.init, w.target, w.forcing, latent_noise=zq, member_noise=zm)
    assert float(w.step.last_crps) > 0
    loss2.backward()
    g2 = _grads(w.step)
    moved = {k for k in g2 if g2[k] is not None and g1[k] is not None and rel_err(g2[k], g1[k]) > 1e-3}
    assert any(".decoder." in k for k in moved), sorted(moved)
    learn_prior = w.case["model_kwargs"].get("learn_prior", True)
    assert any(".prior_model." in k for k in g2) == learn_prior
    if learn_prior:
        assert any(".prior_model." in k for k in moved)
    assert not any(".encoder." in k for k in moved)   # the members never see the posterior


# ---------------------------------------------------------------------------
# GPU: inside the Trainer
# ---------------------------------------------------------------------------
def _trainer_world(dev, root, use_graph=True, seed=3, lr=1e-3, members=2, weight=0.7, **kw):
    from neural_lam_amd.trainer import Trainer

    w = _world("efm_hi_81x30", dev, root, 2, 2, seed=seed, crps_members=members, crps_weight=weight)
    w.tr = Trainer(w.step, lr=lr, use_graph=use_graph, **kw)
    return w


def _run(w, n=3):
    out = []
    for _ in range(n):
        loss = w.tr.step(w.init, w.target, w.forcing).clone()
        out.append((loss, w.step.last_crps.clone()))
    return out


@pytest.mark.gpu
def test_step_with_members_inside_the_trainer(dev, tmp_path):
    a = _trainer_world(dev, tmp_path / "a")
    ra = _run(a)
    assert a.tr.use_graph and a.tr._graph is not None   # the recording did not fall back to eager launches
    crps_vals = [float(c) for _, c in ra]
    assert len(set(crps_vals)) == 3 and all(math.isfinite(v) and v > 0 for v in crps_vals), crps_vals   # each replay: new member noise
    assert a.step.draw_state()["draw"] == 3
    c = _trainer_world(dev, tmp_path / "c", use_graph=False)
    rc = _run(c)
    for (la, ca), (lc, cc) in zip(ra, rc):   # the eager trainer: the same bits
        assert torch.equal(_bits(la), _bits(lc)) and torch.equal(_bits(ca), _bits(cc)), (float(la), float(lc), float(ca), float(cc))
    assert torch.equal(_bits(_all_weights(a)), _bits(_all_weights(c)))


@pytest.mark.gpu
def test_weight_word_between_replays_and_calls_at_another_shape(dev, tmp_path):
    """lr = 0 and weight_decay = 0 keep the weights where they are, ``reseed`` puts the draw count back in place: two replays then
    see the same noise, and the only thing that differs is the word ``set_crps_weight`` rewrote.  crps_weight / (B T) = 1 / 4 and
    2 / 4 are powers of two, so the term scales exactly."""
    a = _trainer_world(dev, tmp_path, lr=0.0, weight=1.0, weight_decay=0.0)
    a.tr.step(a.init, a.target, a.forcing)
    graph, before = a.tr._graph, _all_weights(a)
    a.step.reseed(3, 10)
    a.tr.step(a.init, a.target, a.forcing)
    one, terms_one = a.step.last_crps.clone(), [t.clone() for t in a.step.last_terms]
    a.step.set_crps_weight(2.0)
    a.step.reseed(3, 10)
    # a call at another batch shape in between: its own words, and the draw count put back behind it
    small = (a.init[:1], a.target[:1, :1], a.forcing[:1, :1])
    ev = a.step.evaluate(*small)
    assert ev.crps is not None and float(a.step.crps_weight_word(1, 1)) == 2.0 and float(a.step.crps_weight_word(2, 2)) == 0.5
    with torch.no_grad():
        a.step(*small)
    a.step.reseed(3, 10)
    a.tr.step(a.init, a.target, a.forcing)
    two = a.step.last_crps.clone()
    assert a.tr._graph is graph and torch.equal(_bits(_all_weights(a)), _bits(before))
    assert float(one) > 0 and torch.equal(_bits(two), _bits(2.0 * one)), (float(one), float(two))
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(terms_one, a.step.last_terms))
    a.step.set_crps_weight(0.0)   # a weight of 0 still runs the members
    a.tr.step(a.init, a.target, a.forcing)
    assert a.tr._graph is graph and float(a.step.last_crps) == 0.0


@pytest.mark.gpu
def test_resume_continues_the_member_noise_sequence(dev, tmp_path):
    from neural_lam_amd.checkpoint import load_checkpoint, save_checkpoint

    a = _trainer_world(dev, tmp_path / "a")
    for _ in range(2):
        a.tr.step(a.init, a.target, a.forcing)
    path = tmp_path / "efm.ckpt"
    save_checkpoint(path, a.tr, epoch=0, global_step=2, extra=a.step.draw_state())
    want = _run(a, 2)
    b = _trainer_world(dev, tmp_path / "b", seed=1234, weight=0.1)
    with torch.no_grad():
        for p in b.step.parameters():
            p.mul_(0.5)   # not the saved weights
    ckpt = load_checkpoint(path, b.tr)
    extra = ckpt["neural_lam_amd"]["extra"]
    assert extra == {"seed": 3, "draw": 2, "kl_beta": 1.0, "crps_weight": 0.7}
    b.step.load_draw_state(extra)
    got = _run(b, 2)
    for (lw, cw), (lg, cg) in zip(want, got):
        assert torch.equal(_bits(lw), _bits(lg)) and torch.equal(_bits(cw), _bits(cg)), (float(lw), float(lg), float(cw), float(cg))


# ---------------------------------------------------------------------------
# GPU: crps_members = 0 is the step as it was; evaluate
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_without_members_the_step_is_the_step_as_it_was(dev, tmp_path):
    """No launch counter exists in this suite, so the check is on bits: the loss, both terms and every gradient."""
    from neural_lam_amd import models as hm

    a = _world("efm_hi_81x30", dev, tmp_path / "a", 2, 2)
    case, ds, model = _cpu_world(tmp_path / "b", "efm_hi_81x30")
    plain = hm.EFMForecasterStep(hm.EFMForecaster(model, ds), ds, seed=3, rank=0, crps_members=0, crps_weight=0.0).to(dev)
    _, la = a.step(a.init, a.target, a.forcing)
    _, lb = plain(a.init, a.target, a.forcing)
    la.backward()
    lb.backward()
    assert torch.equal(_bits(la.detach()), _bits(lb.detach())) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a.step.last_terms, plain.last_terms))
    ga, gb = _grads(a.step), _grads(plain)
    assert all(torch.equal(_bits(ga[k]), _bits(gb[k])) for k in ga)
    assert plain.last_crps is None and set(plain.draw_state()) == {"seed", "draw", "kl_beta"}
    assert plain.evaluate(a.init, a.target, a.forcing).crps is None
    assert {k for k, _ in plain.named_buffers()} == {k for k, _ in a.step.named_buffers()}


@pytest.mark.gpu
def test_evaluate_with_members(dev, tmp_path):
    from neural_lam_amd import models as hm
    from neural_lam_amd.trainer import graphed_eval_step

    w = _world("efm_ms_30x27", dev, tmp_path, 2, 2, crps_members=2, crps_weight=0.7)
    ev = w.step.evaluate(w.init, w.target, w.forcing)
    assert isinstance(ev, hm.EFMEvalResult) and ev.crps is not None and float(ev.crps) > 0 and not ev.loss.requires_grad
    assert torch.equal(_bits(ev.loss), _bits((ev.likelihood + ev.kl) + ev.crps))
    assert w.step.draw_state()["draw"] == 0 and int(w.step.eval_draw) == (1 << 31) + 1   # the training draw stays where it was
    # the same noise through forward: the same terms
    zq, zm = _noise(w, 2, 11)
    ev_n = w.step.evaluate(w.init, w.target, w.forcing, latent_noise=zq, member_noise=zm)
    with torch.no_grad():
        _, loss = w.step(w.init, w.target, w.forcing, latent_noise=zq, member_noise=zm)
    assert torch.equal(_bits(ev_n.loss), _bits(loss)) and torch.equal(_bits(ev_n.crps.reshape(())), _bits(w.step.last_crps))
    val = graphed_eval_step(w.step, w.init, w.target, w.forcing, phase="val")   # its warm-up is the eager call of this shape
    first = val(w.init, w.target, w.forcing)
    crps1, draw1 = first.crps.clone(), int(w.step.eval_draw)
    second = val(w.init, w.target, w.forcing)
    assert int(w.step.eval_draw) == draw1 + 1 and w.step.draw_state()["draw"] == 0
    assert float(second.crps) != float(crps1) and bool(torch.isfinite(second.loss))   # a replay draws new member noise
    assert torch.equal(_bits(second.loss), _bits((second.likelihood + second.kl) + second.crps))
