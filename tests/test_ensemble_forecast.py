"""Sampled ensembles (neural_lam_amd.forecast.EnsembleForecast; nlam_philox_normal_fill, nlam_latent_sample, nlam_ens_scores).
Without a GPU: the reference generator against the Random123 known answers, the C-ABI (exports, layouts, argument checks), the
float64 score math against hand-computed cases, and the predictors' raw_delta / latent arguments.  On the GPU: the generator
against float64 Box-Muller of the reference integers and against its sampling bounds, the draw and the scores against float64
math (an exact tier on integers, a budget tier on random states), and the engine on the Graph-EFM golden cases' graphs and weights
against a python loop over the same module, the reference's own draw, the score math, itself, and a deterministic predictor."""
import ctypes as C
import math
import subprocess
import types

import numpy as np
import pytest
import torch

import philox_ref as P
from conftest import ROOT, graph_from_case, load_golden, rel_err
from neural_lam_amd import _lib as L

U = 2.0 ** -24   # fp32 unit roundoff
EPS32 = 2.0 ** -23
NEW_EXPORTS = ["nlam_philox_normal_fill", "nlam_latent_sample", "nlam_ens_scores", "nlam_ens_scores_workspace_floats"]
EFM_CASES = ["efm_hi_81x30", "efm_ms_30x27", "efm_hi_constprior_81x30"]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_reference_philox_reproduces_the_random123_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        assert " ".join(f"{w:08x}" for w in P.philox4x32_10(counter, key)) == want
    # the vectorised form used on the GPU side of this file is the same function
    seed = 0x299F31D0A4093822
    blocks = P.philox_blocks([0x243F6A88, 0, 7], 0x85A308D3, 0x13198A2E, 0x03707344, seed)
    for row, q in zip(blocks, (0x243F6A88, 0, 7)):
        assert tuple(int(w) for w in row) == P.philox4x32_10((q, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    u = P.uniforms(np.array([0, 0xFFFFFFFF, 1 << 9]))
    assert u.tolist() == [2.0 ** -24, 1.0 - 2.0 ** -24, 1.5 * 2.0 ** -23]
    assert all(float(np.float32(v)) == v for v in u)   # exact in fp32, never 0 or 1


def _c_layout(tmp_path, ctype, cstruct):
    fields = [name for name, _ in ctype._fields_]
    src = tmp_path / f"{cstruct}.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
                   f'int main(){{printf("%zu", sizeof({cstruct}));\n'
                   + "".join(f'printf(" %zu", offsetof({cstruct}, {f}));\n' for f in fields)
                   + 'printf(" %d %d\\n", NLAM_ABI_VERSION, NLAM_ENS_MAX_MEMBERS); return 0;}\n')
    exe = tmp_path / cstruct
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] + [8, L.ENS_MAX_MEMBERS]


def test_ensemble_symbols_are_exported_and_the_structs_match_c_layout(tmp_path):
    import re

    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.nlam_abi_version() == 8 == L.ABI_VERSION
    _c_layout(tmp_path, L.LatentSample, "nlam_latent_sample_t")
    _c_layout(tmp_path, L.EnsScores, "nlam_ens_scores_t")


def test_ensemble_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    S, M, N, F, LEAD = 2, 3, 37, 5, 4
    nws = lib.nlam_ens_scores_workspace_floats(S, M, N, F)
    assert nws >= S * F * (M + 5)
    for bad in ((0, M, N, F), (S, 0, N, F), (S, M, 0, F), (S, M, N, 0)):
        assert lib.nlam_ens_scores_workspace_floats(*bad) == -1, bad
    assert lib.nlam_ens_scores_workspace_floats(S, 65, N, F) == -2 and lib.nlam_ens_scores_workspace_floats(S, M, N, 257) == -2
    assert lib.nlam_ens_scores_workspace_floats(S, 64, N, 256) > 0

    def scores(**kw):
        p = L.EnsScores()
        for name in ("prev", "truth", "row_weight", "state_mean", "state_std", "lead", "ens_sq", "ens_var", "ens_abs", "ens_pair",
                     "rank_hist", "out_mean", "out_spread", "workspace"):
            setattr(p, name, fake)
        p.workspace_floats, p.starts, p.members, p.nodes, p.d_state, p.max_lead = nws, S, M, N, F, LEAD
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    assert lib.nlam_ens_scores(None, None) == -1
    nulls = [{name: None} for name in ("prev", "truth", "row_weight", "state_mean", "state_std", "lead", "ens_sq", "ens_var", "ens_abs",
                                       "ens_pair", "rank_hist", "out_mean", "out_spread", "workspace")]
    for kw in nulls + [dict(starts=0), dict(members=0), dict(nodes=0), dict(d_state=0), dict(max_lead=0), dict(workspace_floats=nws - 1)]:
        assert lib.nlam_ens_scores(scores(**kw), None) == -1, kw
    for kw in (dict(members=65), dict(d_state=257), dict(starts=65536)):
        assert lib.nlam_ens_scores(scores(workspace_floats=1 << 40, **kw), None) == -2, kw

    def sample(**kw):
        p = L.LatentSample()
        for name in ("params", "noise_in", "noise_out", "latent", "start", "lead", "seed"):
            setattr(p, name, fake)
        p.batch, p.members, p.rows, p.latent_dim, p.diagonal, p.max_lead = S * M, M, 9, 8, 1, LEAD
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    assert lib.nlam_latent_sample(None, None) == -1
    for kw in (dict(params=None), dict(latent=None), dict(start=None), dict(lead=None), dict(noise_in=None, seed=None), dict(batch=0),
               dict(members=0), dict(rows=0), dict(latent_dim=0), dict(max_lead=0), dict(diagonal=2), dict(batch=S * M + 1)):
        assert lib.nlam_latent_sample(sample(**kw), None) == -1, kw
    assert lib.nlam_latent_sample(sample(batch=65536 * M, members=M), None) == -2
    assert lib.nlam_latent_sample(sample(rows=1 << 16, latent_dim=1 << 15), None) == -2
    assert lib.nlam_philox_normal_fill(None, 4, 0, 0, 0, 0, None) == -1
    assert lib.nlam_philox_normal_fill(fake, -1, 0, 0, 0, 0, None) == -1
    assert lib.nlam_philox_normal_fill(fake, (1 << 34) + 1, 0, 0, 0, 0, None) == -2
    assert lib.nlam_philox_normal_fill(fake, 0, 0, 0, 0, 0, None) == 0   # nothing to do, nothing launched


def test_score_reference_against_hand_computed_cases():
    t = lambda v: torch.tensor(v, dtype=torch.float64)   # noqa: E731
    # M = 2, one node, one variable: members 1 and 4, truth 2, weight 0.5
    r = P.ens_scores(t([1.0, 4.0]).view(1, 2, 1, 1), t([2.0]).view(1, 1, 1), t([0.5]), t([10.0]), t([2.0]))
    assert r["ens_sq"].item() == 0.5 * 0.25          # xbar 2.5
    assert r["ens_var"].item() == 0.5 * 4.5          # ((1.5)^2 + (1.5)^2) / 1
    assert r["ens_abs"].item() == 0.5 * 1.5          # (1 + 2) / 2
    assert r["ens_pair"].item() == 0.5 * 1.5         # |1 - 4| / (2 * 1)
    assert r["rank_hist"].view(-1).tolist() == [0, 1, 0]
    assert r["mean"].item() == 2.5 * 2.0 + 10.0 and r["spread"].item() == math.sqrt(4.5) * 2.0
    # a member equal to the truth is not below it: members (2, 2, 5), truth 2 -> rank 0; truth 5 -> rank 2; weight 0 is not counted
    x = t([[2.0, 2.0, 5.0], [2.0, 2.0, 5.0], [2.0, 2.0, 5.0]]).t().reshape(1, 3, 3, 1)
    r = P.ens_scores(x, t([2.0, 5.0, 9.0]).view(1, 3, 1), t([1.0, 1.0, 0.0]))
    assert r["rank_hist"].view(-1).tolist() == [1, 0, 1, 0]
    # M = 1
    r = P.ens_scores(t([3.0, -1.0]).view(1, 1, 2, 1), t([1.0, 1.0]).view(1, 2, 1), t([0.25, 0.75]))
    assert r["ens_var"].item() == 0.0 and r["ens_pair"].item() == 0.0 and float(r["spread"].abs().max()) == 0.0
    assert r["ens_sq"].item() == 0.25 * 4 + 0.75 * 4 and r["ens_abs"].item() == 0.25 * 2 + 0.75 * 2
    assert r["rank_hist"].view(-1).tolist() == [1, 1]


def test_efm_raw_delta_and_latent_arguments_reproduce_forward_through_a_python_tail(tmp_path, monkeypatch):
    """BaseGraphEFM.forward(latent=, raw_delta=True) and BaseGraphLatentDecoder.forward(raw=True) on the CPU: the HIP MLPs of the
    decoder are replaced by torch Linears (the library does not run on the CPU), forward's own code runs.  The python tail
    (rescale, get_clamped_new_state, softplus) on the raw output reproduces the default result: rel_err <= 1e-6, the bar of
    test_restatement_equals_the_oracle_rollout_on_the_cpu."""
    from neural_lam_amd import graph as G
    from neural_lam_amd import graph_efm
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)
    G.save_graph(tmp_path / "graph" / "multiscale", G.create_regular_grid_graph(ds.get_xy("state")))
    names = ds.get_vars_names("state")
    g = torch.Generator().manual_seed(4)
    for kw in ({}, dict(output_std=True, output_clamping_lower={names[0]: -3.0, names[2]: -4.0},
                        output_clamping_upper={names[2]: 4.0, names[4]: 3.0})):
        m = graph_efm.GraphEFMMultiScale(ds, hidden_dim=8, latent_dim=4, learn_prior=False, prior_m2m_layers=1, encoder_m2m_layers=1,
                                         decoder_m2m_layers=1, **kw)
        N, F, B = ds.num_grid_points, 5, 2
        dec = m.decoder
        dec.latent_embedder = torch.nn.Linear(4, 8)
        dec.grid_update_mlp = torch.nn.Linear(8, 8)
        dec.grid_update_mlp.fully_fused = False
        dec.param_map = torch.nn.Linear(8, m.grid_output_dim)
        dec.combine_with_latent = lambda grid, lat, resid, emb: resid + lat.mean(dim=1, keepdim=True)
        grid_emb = torch.randn(B, N, 8, generator=g)
        m.embedd_grid_and_graph = lambda *a: (grid_emb, {})
        prev, latent = torch.randn(B, N, F, generator=g) * 0.5, torch.randn(B, m.latent_spatial_dim, 4, generator=g)
        with torch.no_grad():
            want, want_std = m(prev, prev, None, latent=latent)
            raw, none = m(prev, prev, None, latent=latent, raw_delta=True)
            assert none is None and raw.shape == (B, N, m.grid_output_dim)
            assert torch.equal(raw, dec(grid_emb, latent, {}, raw=True))
            mean_delta = raw[..., :F]
            got = m.get_clamped_new_state(mean_delta * m.diff_std + m.diff_mean, prev)
            assert rel_err(got, want) <= 1e-6
            if kw:
                assert rel_err(torch.nn.functional.softplus(raw[..., F:]), want_std) <= 1e-6
            else:
                assert want_std is None
            # latent = the sample: with the prior's own draw handed over as noise the default path gives the same state
            noise = torch.randn(B, m.latent_spatial_dim, 4, generator=g)
            assert torch.equal(m(prev, prev, None, latent_noise=noise)[0], m(prev, prev, None, latent=noise)[0])   # N(0, 1) prior
            assert m.prior_params(grid_emb, {}).shape == (B, m.latent_spatial_dim, 4)
        assert m.can_return_raw_delta() and m.draws_latent
        monkeypatch.setattr(hm, "FUSED_CLAMPED_TAIL", False)
        assert m.can_return_raw_delta() == (not kw)
        monkeypatch.undo()
        m.diff_std = m.diff_std.reshape(1, -1)
        assert not m.can_return_raw_delta()


def test_engines_refuse_what_they_do_not_serve(tmp_path):
    from neural_lam_amd import graph as G
    from neural_lam_amd import graph_efm
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore
    from neural_lam_amd.forecast import EnsembleForecast, Forecast

    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)
    G.save_graph(tmp_path / "graph" / "multiscale", G.create_regular_grid_graph(ds.get_xy("state")))
    m = graph_efm.GraphEFMMultiScale(ds, hidden_dim=8, prior_m2m_layers=1, encoder_m2m_layers=1, decoder_m2m_layers=1)
    step = hm.ForecasterStep(hm.ARForecaster(m, ds), ds)
    plain = types.SimpleNamespace(kernel="nlam_window_batch", device=torch.device("cpu"))
    with pytest.raises(ValueError, match="Graph-EFM is not served"):   # the deterministic engine keeps its refusal
        Forecast(step, plain, 4)
    for members in (0, 65):
        with pytest.raises(ValueError, match="members"):
            EnsembleForecast(step, plain, 4, members=members)
    with pytest.raises(ValueError, match="ensemble"):
        EnsembleForecast(step, types.SimpleNamespace(kernel="nlam_window_batch_ens"), 4, members=2)
    with pytest.raises(RuntimeError, match="GPU"):
        EnsembleForecast(step, plain, 4, members=2)


# ---------------------------------------------------------------------------
# GPU: the generator
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _misaligned(t):
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


def _fill(dev, n, seed, c1=0, c2=0, c3=0, misalign=False):
    """n normals into a poisoned buffer, 16-byte aligned or 4 bytes off; nothing outside [0, n) is written."""
    buf = torch.full((n + 8,), float("nan"), device=dev)
    first = 1 if misalign else 4
    out = buf[first:first + n]
    L.check(L.load().nlam_philox_normal_fill(_ptr(out), n, seed, c1, c2, c3, _stream()), "nlam_philox_normal_fill")
    assert bool(torch.isnan(buf[:first]).all()) and bool(torch.isnan(buf[first + n:]).all())
    return out


# The first-order bound of one Box-Muller normal z = sqrtf(-2 logf(u)) * cospif / sinpif (2 v), u and 2 v exact in fp32, -2 * exact:
#   logf within 3 ulp, sinpi / cospi / sincospi within 4 ulp: the ULP table of the OpenCL C specification ("Relative Error as ULPs"),
#   the accuracy the ROCm device library (OCML) these HIP functions compile to is built to;
#   sqrtf correctly rounded, 0.5 ulp (IEEE 754; hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt); the product 0.5 ulp.
# A relative error e of the logarithm becomes e / 2 behind the square root; an ulp is at most 2^-23 of the value.
NORMAL_ULPS = 3 / 2 + 0.5 + 4 + 0.5
_WORST = {"normal": 0.0}


@pytest.mark.gpu
def test_generator_matches_float64_box_muller_of_the_reference_integers(dev):
    for seed in (0, 0x9E3779B97F4A7C15):
        for n in (1, 3, 4, 5, 4099):
            for misalign in (False, True):
                c = (5, 2, 0xFFFFFFF0) if misalign else (0, 0, 0)
                got = _fill(dev, n, seed, *c, misalign=misalign).cpu().double().numpy()
                want = P.normals(n, seed, *c)
                ratio = np.abs(got - want) / (EPS32 * np.abs(want))
                _WORST["normal"] = max(_WORST["normal"], float(ratio.max()))
                print(f"normals seed {seed:#x} n {n} misaligned {misalign}: worst error {ratio.max():.3f} ulp-units, bar {NORMAL_ULPS}")
                assert bool((ratio <= NORMAL_ULPS * (1 + 1e-3)).all()), (seed, n, misalign, float(ratio.max()))


@pytest.mark.gpu
def test_generator_moments_and_stream_independence(dev):
    n = 1 << 20
    seed = 1234567
    base = _fill(dev, n, seed, 3, 1, 77).double()
    assert abs(float(base.mean())) <= 5 / math.sqrt(n)
    assert abs(float(base.var()) - 1.0) <= 5 * math.sqrt(2 / n)
    others = {"lead": _fill(dev, n, seed, 4, 1, 77), "member": _fill(dev, n, seed, 3, 2, 77), "t0": _fill(dev, n, seed, 3, 1, 78),
              "seed": _fill(dev, n, seed + 1, 3, 1, 77)}
    for what, other in others.items():
        assert float((_bits(other) == _bits(base.float())).float().mean()) < 1e-3, what   # different bits, element by element
        if what in ("lead", "member"):
            corr = float(torch.corrcoef(torch.stack([base, other.double()]))[0, 1])
            assert abs(corr) <= 5 / math.sqrt(n), (what, corr)
    assert torch.equal(_bits(_fill(dev, n, seed, 3, 1, 77)), _bits(base.float()))


# ---------------------------------------------------------------------------
# GPU: nlam_latent_sample
# ---------------------------------------------------------------------------
def _sample_args(params, latent, start, lead, seed, members, rows, dim, diagonal, max_lead, noise_in=None, noise_out=None):
    p = L.LatentSample()
    p.params, p.latent, p.start, p.lead, p.seed = _ptr(params), _ptr(latent), _ptr(start), _ptr(lead), _ptr(seed)
    p.noise_in, p.noise_out = _ptr(noise_in), _ptr(noise_out)
    p.batch, p.members, p.rows, p.latent_dim, p.diagonal, p.max_lead = params.shape[0], members, rows, dim, int(diagonal), max_lead
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows,dim", [(1, 1), (7, 3), (30, 8)])
@pytest.mark.parametrize("diagonal", [False, True])
def test_latent_sample_draws_and_reparameterises(dev, diagonal, rows, dim, misalign):
    lib = L.load()
    put = _misaligned if misalign else (lambda t: t)
    S, M, LEAD, K, SEED = 2, 3, 4, 2, 0xDEADBEEF12345
    B = S * M
    g = torch.Generator().manual_seed(rows * 10 + dim)
    params = put((torch.randn(B, rows, dim * (2 if diagonal else 1), generator=g) * 1.5).to(dev))
    if diagonal:
        params[0, 0, dim] = 25.0   # softplus' linear branch
    t0 = [5, 5, 5, (1 << 32) + 9, (1 << 32) + 9, (1 << 32) + 9]   # the low word of the start time counts
    start = torch.tensor(t0, dtype=torch.int64, device=dev)
    lead = torch.full((1,), K, dtype=torch.int32, device=dev)
    seed = torch.tensor([SEED], dtype=torch.int64, device=dev)
    nan = lambda *shape: put(torch.full(shape, float("nan"), device=dev))   # noqa: E731
    latent, noise = nan(B, rows, dim), nan(LEAD, B, rows, dim)
    p = _sample_args(params, latent, start, lead, seed, M, rows, dim, diagonal, LEAD, noise_out=noise)
    L.check(lib.nlam_latent_sample(C.byref(p), _stream()), "nlam_latent_sample")
    assert int(lead) == K
    others = [k for k in range(LEAD) if k != K]
    assert bool(torch.isnan(noise[others]).all()) and bool(torch.isfinite(noise[K]).all())
    # the noise is the generator's: counter (quad, lead, member, low word of t0)
    want = P.latent_noise(K, M, t0, rows * dim, SEED)
    ratio = np.abs(noise[K].cpu().double().numpy().reshape(B, -1) - want) / (EPS32 * np.abs(want))
    assert bool((ratio <= NORMAL_ULPS * (1 + 1e-3)).all())
    flat = lambda v: _fill(dev, rows * dim, SEED, K, v[0], v[1])   # noqa: E731
    for b in range(B):
        assert torch.equal(_bits(noise[K, b].reshape(-1)), _bits(flat((b % M, t0[b] & 0xFFFFFFFF)))), b
    # given-noise mode on the drawn noise: the same bits; against float64: the softplus budget of test_clamped_tail.py
    # (err <= 2 err_ref + 1e-6, err_ref the same formula in fp32 on the CPU) plus one rounding each for the product and the sum
    latent2 = nan(B, rows, dim)
    p2 = _sample_args(params, latent2, start, lead, None, M, rows, dim, diagonal, LEAD, noise_in=noise)
    L.check(lib.nlam_latent_sample(C.byref(p2), _stream()), "nlam_latent_sample")
    assert torch.equal(_bits(latent2), _bits(latent))
    ref64 = P.latent_sample(params.cpu(), noise[K].cpu(), diagonal)
    ref32 = P.latent_sample(params.cpu(), noise[K].cpu(), diagonal, torch.float32)
    err, err_ref = rel_err(latent.cpu().double(), ref64), rel_err(ref32.double(), ref64)
    assert err <= 2 * err_ref + 1e-6 + 2 * EPS32, (err, err_ref)
    # the same (t0, member) in another position of another batch gets the same noise: item 4 here = (t0 2^32 + 9, member 1)
    start2 = torch.tensor([(1 << 32) + 9] * 3 + [77] * 3, dtype=torch.int64, device=dev)
    noise2 = nan(LEAD, B, rows, dim)
    p3 = _sample_args(params, nan(B, rows, dim), start2, lead, seed, M, rows, dim, diagonal, LEAD, noise_out=noise2)
    L.check(lib.nlam_latent_sample(C.byref(p3), _stream()), "nlam_latent_sample")
    assert torch.equal(_bits(noise2[K, 1]), _bits(noise[K, 4])) and not torch.equal(_bits(noise2[K, 4]), _bits(noise[K, 4]))
    # *lead = max_lead: nothing is written
    lead.fill_(LEAD)
    poisoned_latent, poisoned_noise = nan(B, rows, dim), nan(LEAD + 1, B, rows, dim)
    p4 = _sample_args(params, poisoned_latent, start, lead, seed, M, rows, dim, diagonal, LEAD, noise_out=poisoned_noise)
    L.check(lib.nlam_latent_sample(C.byref(p4), _stream()), "nlam_latent_sample")
    assert bool(torch.isnan(poisoned_latent).all()) and bool(torch.isnan(poisoned_noise).all()) and int(lead) == LEAD


# ---------------------------------------------------------------------------
# GPU: nlam_ens_scores
# ---------------------------------------------------------------------------
def _chunk_nodes(F, M):
    """Nodes per workgroup: from the workspace size (one row of F (M + 5) words per chunk)."""
    lib = L.load()
    n = 1
    while lib.nlam_ens_scores_workspace_floats(1, M, n + 1, F) == F * (M + 5):
        n += 1
    return n


def _scores_run(dev, x, y, w, mean, std, misalign, K=1, LEAD=3):
    """One nlam_ens_scores launch at lead K on x (S, M, N, F), y (S, N, F): outputs with every other slot poisoned."""
    lib = L.load()
    put = _misaligned if misalign else (lambda t: t)
    S, M, N, F = x.shape
    prev = put(x.reshape(S * M, N, F).float().to(dev))
    truth = torch.full((S, M, N, F), float("nan"))
    truth[:, 0] = y.float()   # the truth of member 0 is used
    truth = put(truth.reshape(S * M, N, F).to(dev))
    nan = lambda *shape: put(torch.full(shape, float("nan"), device=dev))   # noqa: E731
    o = types.SimpleNamespace(ens_sq=nan(S, LEAD, F), ens_var=nan(S, LEAD, F), ens_abs=nan(S, LEAD, F), ens_pair=nan(S, LEAD, F),
                              mean=nan(S, LEAD, N, F), spread=nan(S, LEAD, N, F),
                              rank_hist=torch.full((S, LEAD, F, M + 1), -7, dtype=torch.int32, device=dev))
    nws = int(lib.nlam_ens_scores_workspace_floats(S, M, N, F))
    ws = torch.full((nws,), float("nan"), device=dev)
    lead = torch.full((1,), K, dtype=torch.int32, device=dev)
    keep = [t.float().to(dev) for t in (w, mean, std)]
    p = L.EnsScores()
    p.prev, p.truth, p.row_weight, p.state_mean, p.state_std, p.lead = _ptr(prev), _ptr(truth), *(_ptr(t) for t in keep), _ptr(lead)
    p.ens_sq, p.ens_var, p.ens_abs, p.ens_pair = _ptr(o.ens_sq), _ptr(o.ens_var), _ptr(o.ens_abs), _ptr(o.ens_pair)
    p.rank_hist, p.out_mean, p.out_spread, p.workspace, p.workspace_floats = _ptr(o.rank_hist), _ptr(o.mean), _ptr(o.spread), _ptr(ws), nws
    p.starts, p.members, p.nodes, p.d_state, p.max_lead = S, M, N, F, LEAD
    L.check(lib.nlam_ens_scores(C.byref(p), _stream()), "nlam_ens_scores")
    torch.cuda.synchronize()
    assert int(lead) == K   # only read
    others = [k for k in range(LEAD) if k != K]
    got = {}
    for name, t in vars(o).items():
        assert bool(torch.isnan(t[:, others]).all()) if t.dtype == torch.float32 else bool((t[:, others] == -7).all()), name
        got[name] = t[:, K].cpu().clone()
    return got


def _score_shapes(M):
    for F in (1, 5, 17):
        cn = _chunk_nodes(F, M)
        for N in sorted({1, 5, cn - 1, cn, cn + 1} - {0}):
            for S, misalign in ((1, False), (3, True)) if N > 5 else ((1, False), (1, True), (3, False), (3, True)):
                yield F, N, S, misalign


MEMBERS = [1, 2, 3, 20, 64]


@pytest.mark.gpu
@pytest.mark.parametrize("M", MEMBERS)
def test_ens_scores_exact_on_integers(dev, M):
    """Tier (a).  Members M (a + t [m == j]) with integers a, t and one marked member j per element, truth M b, weights in
    {0, 1/2, 1, 2}, statistics (integer mean, power-of-two std): the member sum is M (M a + t), the squared deviations add up to
    M (M - 1) t^2, the pair sum to (M - 1) M |t| -- every quotient is an integer and every partial sum a multiple of 1/2 below
    2^23 (asserted on the float64 totals: the terms are non-negative), so every output is exact in any order: bit for bit, the
    histogram included; b == a, the usual case, puts members on the truth."""
    g = torch.Generator().manual_seed(M)
    seen_below = seen_tie = False
    for F, N, S, misalign in _score_shapes(M):
        a = torch.randint(-1, 2, (S, 1, N, F), generator=g)
        t = torch.randint(-2, 3, (S, 1, N, F), generator=g)
        j = torch.randint(0, M, (S, 1, N, F), generator=g)
        x = (M * (a + t * (torch.arange(M).view(1, M, 1, 1) == j))).double()
        off = torch.randint(-1, 2, (S, N, F), generator=g) * (torch.rand(S, N, F, generator=g) < 0.125)   # the truth M off away, rarely
        y = (M * (a[:, 0] + off)).double()
        w = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N,), generator=g)].double()
        mean, std = torch.randint(-3, 4, (F,), generator=g).double(), 2.0 ** torch.randint(-2, 3, (F,), generator=g).double()
        want = P.ens_scores(x, y, w, mean, std)
        assert all(2 * float(want[k].max()) < 2 ** 24 for k in ("ens_sq", "ens_var", "ens_abs", "ens_pair"))   # halves, non-negative terms
        seen_below |= bool((x < y[:, None]).any())
        seen_tie |= bool((x == y[:, None]).any())
        got = _scores_run(dev, x, y, w, mean, std, misalign)
        what = (M, F, N, S, misalign)
        for k in ("ens_sq", "ens_var", "ens_abs", "ens_pair", "mean"):
            assert torch.equal(got[k].double(), want[k]), (what, k)
        var = ((x - x.mean(1, keepdim=True)) ** 2).sum(1) / max(M - 1, 1)
        assert torch.equal(got["spread"], torch.sqrt(var.float()) * std.float()), what   # one correctly rounded square root
        assert torch.equal(got["rank_hist"], want["rank_hist"]), what
        again = _scores_run(dev, x, y, w, mean, std, misalign)
        assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got), what
    assert seen_below and seen_tie   # members below the truth, and members on it


def _score_bounds(x, y, w, mean, std, want):
    """The budget of test_ens_scores_within_the_rounding_budget's docstring for float64 x (S, M, N, F), y (S, N, F)."""
    S, M, N, F = x.shape
    cn = _chunk_nodes(F, M)
    tau = U * (min(cn, N) + -(-N // cn) + 24)
    wn = w.view(1, N, 1)
    xbar = x.mean(1)
    e_mean = U * ((M + 1) * (x - x[:, :1]).abs().mean(1) + xbar.abs())
    dev_sum = (2 * (x - xbar[:, None]).abs() * e_mean[:, None] + e_mean[:, None] ** 2).sum(1) / max(M - 1, 1)
    a = (x - y[:, None]).abs()
    e_abs = U * ((M + 1) * (a - a[:, :1]).abs().mean(1) + 3 * a.mean(1))
    b = {"ens_sq": (wn * (2 * (xbar - y).abs() * e_mean + e_mean ** 2)).sum(1) + (tau + 4 * U) * want["ens_sq"],
         "ens_var": (wn * dev_sum).sum(1) + (tau + U * (M + 8)) * want["ens_var"],
         "ens_abs": (wn * e_abs).sum(1) + (tau + U) * want["ens_abs"],
         "ens_pair": (tau + U * (M * (M - 1) / 2 + 4)) * want["ens_pair"],
         "mean": e_mean * std + 2 * U * ((xbar * std).abs() + mean.abs())}
    if M > 1:
        sd = want["spread"] / std
        var_err = dev_sum + U * (M + 8) * sd ** 2
        b["spread"] = (var_err / (2 * sd) + 2 * U * sd) * std
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("M", MEMBERS)
def test_ens_scores_within_the_rounding_budget(dev, M):
    """Tier (b): random states with per-variable scales against the float64 math, first order.  The kernel's mean of v_0 .. v_{M-1}
    is v_0 + (sum_m (v_m - v_0)) / M: M - 1 differences, M - 2 additions, a division and an addition, so its error is at most
    e(v) = U ((M + 1) mean_m |v_m - v_0| + |mean|).  With e = e(x) for the member mean and a_m = |x_m - y|:
      ens_sq    sum_n w (2 |xbar - y| e + e^2)                          + (tau + 4 U) ens_sq      (subtraction, square, weight)
      ens_var   sum_n w / (M - 1) sum_m (2 |x_m - xbar| e + e^2)        + (tau + U (M + 8)) ens_var
      ens_abs   sum_n w (e(a) + 2 U mean_m a_m)                         + (tau + U) ens_abs       (the a_m carry a rounding each)
      ens_pair                                                            (tau + U (M (M - 1) / 2 + 4)) ens_pair
    tau = U (chunk nodes + chunks + 24): the additions of one output, in a chunk, across a wave's chunks and across the waves.
    The fields: e times the std plus two roundings; the spread's from the variance's through the root."""
    g = torch.Generator().manual_seed(100 + M)
    for F, N, S, misalign in _score_shapes(M):
        scale = torch.logspace(-1, 1, F).double()
        x = (torch.randn(S, M, N, F, generator=g).float().double() * scale + 0.3 * scale)
        y = (torch.randn(S, N, F, generator=g).float().double() * scale)
        x, y = x.float().double(), y.float().double()
        assert not bool((x == y[:, None]).any())   # no ties: the histogram is exact
        w = torch.rand(N, generator=g).float().double() * (torch.rand(N, generator=g) > 0.3)
        if N > 1:
            w[0] = 0.0
        mean, std = torch.randn(F, generator=g).float().double(), (torch.rand(F, generator=g) + 0.5).float().double()
        want = P.ens_scores(x, y, w, mean, std)
        got = _scores_run(dev, x, y, w, mean, std, misalign)
        what = (M, F, N, S, misalign)
        for k, bound in _score_bounds(x, y, w, mean, std, want).items():
            err = (got[k].double() - want[k]).abs()
            assert bool((err <= bound * (1 + 1e-3)).all()), (what, k, float((err / bound.clamp_min(1e-300)).max()))
        if M == 1:
            assert float(got["spread"].abs().max()) == 0.0
            assert float(got["ens_var"].abs().max()) == 0.0 and float(got["ens_pair"].abs().max()) == 0.0
        assert torch.equal(got["rank_hist"], want["rank_hist"]), what
        assert int(got["rank_hist"].sum()) == S * F * int((w != 0).sum())
        again = _scores_run(dev, x, y, w, mean, std, misalign)
        assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got), what


# ---------------------------------------------------------------------------
# GPU: the engine on the golden cases' graphs and weights
# ---------------------------------------------------------------------------
E_TIMES, E_LEAD = 14, 3


def _efm_world(name, dev, root):
    from neural_lam_amd import graph as G
    from neural_lam_amd import graph_efm
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    case = load_golden(name)
    ds = SyntheticDatastore(root_path=root, **case["ds_kwargs"])
    G.save_graph(root / "graph" / "g", graph_from_case(case, "ref_graph_raw"))
    model = getattr(graph_efm, case["cls"])(ds, graph_name="g", **case["model_kwargs"])
    r = model.load_state_dict(case["state_dict"], strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    step = hm.ForecasterStep(hm.ARForecaster(model, ds), ds).to(dev)
    g = torch.Generator().manual_seed(17)
    N = ds.num_grid_points
    w = types.SimpleNamespace(case=case, ds=ds, step=step, model=model, N=N)
    w.state = (torch.randn(E_TIMES, N, 5, generator=g) * 0.5).to(dev) * step.state_std + step.state_mean
    w.forcing = torch.randn(E_TIMES, N, 2, generator=g).to(dev)
    w.times = (torch.arange(E_TIMES, dtype=torch.int64) * 10 + 1000).to(dev)
    return w


def _dataset(w, state=None, forcing=None, times=None):
    from neural_lam_amd.data import DeviceWeatherDataset

    return DeviceWeatherDataset(w.state if state is None else state, w.forcing if forcing is None else forcing,
                                w.times if times is None else times, ar_steps=1, standardization=w.step.standardization_stats())


@pytest.fixture(scope="module", params=EFM_CASES)
def efm(request, dev, tmp_path_factory):
    return _efm_world(request.param, dev, tmp_path_factory.mktemp(request.param))


def _snap(res):
    return {k: v.clone() for k, v in res._asdict().items() if torch.is_tensor(v)}


def _same(a, b, keys=None):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in (keys or a))


@pytest.mark.gpu
def test_engine_trajectory_scores_and_reproducibility(dev, efm):
    from neural_lam_amd.forecast import EnsembleForecast, plan_forecast

    w, step = efm, efm.step
    S, M, starts = 2, 3, [1, 4]
    data = _dataset(w)
    ens = EnsembleForecast(step, data, E_LEAD, members=M, n_starts=S, seed=11, record_noise=True)
    res = ens.run(starts)
    first = _snap(res)
    assert res.members.shape == (S, M, E_LEAD, w.N, 5) and res.mean.shape == (S, E_LEAD, w.N, 5) == res.spread.shape
    assert res.rank_hist.shape == (S, E_LEAD, 5, M + 1) and res.member_sq.shape == (S, M, E_LEAD, 5) and res.ens_sq.shape == (S, E_LEAD, 5)
    assert (res.std is not None) == bool(w.model.output_std) and ens.launches_per_lead > 6
    off, _ = plan_forecast(E_TIMES, 1, 1, E_LEAD)
    t0 = torch.tensor(starts) + off - 1
    assert torch.equal(res.valid_times.cpu(), w.times.cpu()[t0[:, None] + 1 + torch.arange(E_LEAD)])
    # 1. the trajectory: a python loop over the same module with the recorded noise, the boundary overwrite of
    #    test_graph_efm_rolls_out_inside_the_forecaster, de-standardised: 1e-4, the bar of test_engine_matches_the_existing_rollout_and_evaluate
    fc = step.forecaster
    std_state = (w.state - step.state_mean) / step.state_std
    fstats = step.standardization_stats()
    fstd = (w.forcing - fstats["forcing_mean"]) / fstats["forcing_std"]
    tb = t0.repeat_interleave(M).to(dev)
    with torch.no_grad():
        prev_prev, prev = std_state[tb - 1], std_state[tb]
        for k in range(E_LEAD):
            tv = tb + k + 1
            window = torch.stack([fstd[tv - 1], fstd[tv], fstd[tv + 1]], dim=-1).reshape(S * M, w.N, 6)   # feature-major, window-minor
            p, p_std = w.model(prev, prev_prev, window, latent_noise=res.noise[k])
            new = fc.boundary_mask * std_state[tv] + fc.interior_mask * p
            assert rel_err(res.state[:, k], new * step.state_std + step.state_mean) <= 1e-4, k
            if p_std is not None:
                assert rel_err(res.out_std[:, k], p_std * step.state_std) <= 1e-4, k
            prev_prev, prev = prev, new
    # 3. the scores against the float64 math on the engine's own members and the analysis, inside the kernel test's budget
    wgt = step.interior_weight.cpu().double()
    smean, sstd = step.state_mean.cpu().double(), step.state_std.cpu().double()
    for k in range(E_LEAD):   # after k + 1 leads the engine's prev is the standardised state the launch of lead k read
        r = ens.run(starts, leads=k + 1)
        x = ens.prev.view(S, M, w.N, 5).cpu().double()
        y = std_state[t0.to(dev) + k + 1].cpu().double()
        want = P.ens_scores(x, y, wgt, smean, sstd)
        got = {name: getattr(r, name)[:, k].cpu() for name in ("ens_sq", "ens_var", "ens_abs", "ens_pair", "mean", "spread", "rank_hist")}
        for name, bound in _score_bounds(x, y, wgt, smean, sstd, want).items():
            err = (got[name].double() - want[name]).abs()
            assert bool((err <= bound * (1 + 1e-3)).all()), (name, k, float((err / bound.clamp_min(1e-300)).max()))
        live = (wgt != 0).view(1, 1, -1, 1)
        assert not bool(((x == y[:, None]) & live).any())
        assert torch.equal(got["rank_hist"], want["rank_hist"]), k
        for name in ("ens_sq", "ens_var", "ens_abs", "ens_pair", "rank_hist", "mean", "spread", "state"):
            assert torch.equal(_bits(getattr(r, name)), _bits(first[name][:, :k + 1])), (name, k)   # a shorter run is a prefix
        sq = (wgt.view(1, 1, -1, 1) * (x - y[:, None]) ** 2).sum(2)   # Forecast(verify=True)'s formula per member
        ab = (wgt.view(1, 1, -1, 1) * (x - y[:, None]).abs()).sum(2)
        tol = (w.N + 8) * EPS32   # the bar test_forecast.py sets for these two sums
        assert bool(((r.member_sq[:, :, k].cpu().double() - sq).abs() <= tol * sq).all())
        assert bool(((r.member_ab[:, :, k].cpu().double() - ab).abs() <= tol * ab).all())
    res = ens.run(starts)
    assert torch.allclose(res.rmse(step.state_std), torch.sqrt(res.ens_sq.mean(0)) * step.state_std)
    assert torch.allclose(res.crps(step.state_std), (res.ens_abs - res.ens_pair).mean(0) * step.state_std)
    assert torch.allclose(res.spread_skill(), torch.sqrt((M + 1) / M * res.ens_var.mean(0)) / torch.sqrt(res.ens_sq.mean(0)))
    # 4. the same bits eagerly, on a second run, and for a start whatever shares its batch; another seed changes the members only
    eager = EnsembleForecast(step, data, E_LEAD, members=M, n_starts=S, seed=11, record_noise=True, use_graph=False)
    assert _same(first, _snap(eager.run(starts))) and eager.launches_per_lead is None
    other = _snap(ens.run(starts, seed=12))
    assert not torch.equal(other["state"], first["state"]) and not torch.equal(other["noise"], first["noise"])
    assert torch.equal(ens.seed.cpu(), torch.tensor([12]))
    assert _same(first, _snap(ens.run(starts, seed=11)))
    mixed = _snap(ens.run([1, 7]))
    per = lambda d, k, s: d[k][s * M:(s + 1) * M] if d[k].shape[0] == S * M else d[k][s]   # noqa: E731
    for k in ("state", "sq", "ab", "mean", "spread", "ens_sq", "ens_var", "ens_abs", "ens_pair", "rank_hist", "times"):
        assert torch.equal(_bits(per(mixed, k, 0)), _bits(per(first, k, 0))), k
        assert not torch.equal(_bits(per(mixed, "state", 1)), _bits(per(first, "state", 1)))
    assert torch.equal(_bits(mixed["noise"][:, :M]), _bits(first["noise"][:, :M]))
    # given noise reproduces the drawn run; a wrong shape is refused
    given = _snap(ens.run(starts, latent_noise=first["noise"]))
    assert _same(first, given)
    with pytest.raises(ValueError, match="latent_noise"):
        ens.run(starts, latent_noise=first["noise"][:, :1])
    assert _same(first, _snap(ens.run(starts)))   # and back on the generator
    # 6. a replay too many writes nothing
    short = _snap(ens.run(starts, leads=2))
    assert short["state"].shape[1] == 2 and torch.equal(_bits(short["state"]), _bits(first["state"][:, :2]))
    ens.run(starts)
    before = {k: getattr(ens, k).clone() for k in ("out_state", "prev", "prev_prev", "mean", "spread", "ens_sq", "rank_hist", "noise", "latent", "sq")}
    ens._graph.replay()
    torch.cuda.synchronize()
    assert int(ens.lead) == E_LEAD
    for k, v in before.items():
        assert torch.equal(_bits(getattr(ens, k)), _bits(v)), k
    # 7. weights changed in place are honoured
    g = torch.Generator().manual_seed(2)
    saved = [p.detach().clone() for p in step.parameters()]
    with torch.no_grad():
        for p in step.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(dev))
    changed = _snap(ens.run(starts))
    assert not torch.equal(changed["state"], first["state"])
    assert _same(changed, _snap(EnsembleForecast(step, data, E_LEAD, members=M, n_starts=S, seed=11, record_noise=True).run(starts)))
    with torch.no_grad():
        for p, s in zip(step.parameters(), saved):
            p.copy_(s)
    assert _same(first, _snap(ens.run(starts)))


@pytest.mark.gpu
def test_engine_reproduces_the_reference_draw(dev, efm):
    """latent_noise = the golden case's noise, M = 1, one lead from the golden inputs laid out as a series: the standardised new
    state is the reference's pred_mean on interior nodes (TOL = 1e-4 of tests/test_graph_efm.py)."""
    from neural_lam_amd.forecast import EnsembleForecast

    w, step, case = efm, efm.step, efm.case
    B = case["prev"].shape[0]
    T = 4 * B + 1
    stats = step.standardization_stats()
    state = torch.zeros(T, w.N, 5, device=dev)
    forcing = torch.zeros(T, w.N, 2, device=dev)
    for b in range(B):   # item b: t0 = 4 b + 1; its window (past 1, future 1) reads times t0 .. t0 + 2
        t0 = 4 * b + 1
        state[t0 - 1] = case["prev_prev"][b].to(dev) * step.state_std + step.state_mean
        state[t0] = case["prev"][b].to(dev) * step.state_std + step.state_mean
        win = case["forcing"][b].to(dev).view(w.N, 2, 3)
        for s in range(3):
            forcing[t0 + s] = win[:, :, s] * stats["forcing_std"] + stats["forcing_mean"]
    data = _dataset(w, state, forcing, torch.arange(T, dtype=torch.int64, device=dev))
    ens = EnsembleForecast(step, data, 1, members=1, n_starts=B)
    res = ens.run([4 * b for b in range(B)], latent_noise=case["noise"].to(dev)[None])
    interior = step.forecaster.interior_mask.reshape(-1).bool().cpu()
    got = ((res.members[:, 0, 0] - step.state_mean) / step.state_std).cpu()
    assert rel_err(got[:, interior], case["ref_pred_mean"][:, interior]) <= 1e-4
    assert rel_err(ens.prev.cpu()[:, interior], case["ref_pred_mean"][:, interior]) <= 1e-4
    assert rel_err(ens.latent.cpu(), case["ref_latent"]) <= 1e-4
    if case["ref_pred_std"] is not None:
        assert rel_err((res.std[:, 0, 0] / step.state_std).cpu(), case["ref_pred_std"]) <= 1e-4


def _graph_lam_step(dev, root):
    """The GraphLAM predictor and series test_forecast.py builds."""
    from neural_lam_amd import graph as G
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=root, boundary="random", seed=1)
    ext = ds.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state")), max(ext[1] - ext[0], ext[3] - ext[2]))
    torch.manual_seed(1)
    predictor = hm.MODELS["graph_lam"](ds, graph=graph, hidden_dim=16, processor_layers=2)
    step = hm.ForecasterStep(hm.ARForecaster(predictor, ds), ds).to(dev)
    g = torch.Generator().manual_seed(11)
    w = types.SimpleNamespace(ds=ds, step=step, N=ds.num_grid_points)
    w.state, w.forcing = torch.randn(20, w.N, 5, generator=g).to(dev), torch.randn(20, w.N, 2, generator=g).to(dev)
    w.times = (torch.arange(20, dtype=torch.int64) * 10 + 1000).to(dev)
    return w


@pytest.mark.gpu
def test_a_deterministic_predictor_gives_identical_members(dev, tmp_path):
    from neural_lam_amd.forecast import EnsembleForecast, Forecast

    w = _graph_lam_step(dev, tmp_path)
    data = _dataset(w)
    S, M, LEADS = 2, 3, 4
    ens = EnsembleForecast(w.step, data, LEADS, members=M, n_starts=S)
    res = ens.run([1, 5])
    assert res.noise is None and not ens.samples
    single = Forecast(w.step, data, LEADS, batch_size=1, verify=True)
    # the scores and their finishing pass on top of the deterministic engine at the same batch
    assert ens.launches_per_lead == Forecast(w.step, data, LEADS, batch_size=S * M, verify=True).launches_per_lead + 2
    for s, start in enumerate([1, 5]):
        one = single.run([start])
        for m in range(M):
            assert torch.equal(_bits(res.members[s, m]), _bits(one.state[0])), (s, m)
            assert torch.equal(_bits(res.member_sq[s, m]), _bits(one.sq[0])) and torch.equal(_bits(res.member_ab[s, m]), _bits(one.ab[0]))
    assert float(res.ens_var.abs().max()) == 0.0 and float(res.ens_pair.abs().max()) == 0.0 and float(res.spread.abs().max()) == 0.0
    assert torch.equal(_bits(res.ens_abs), _bits(res.member_ab[:, 0])) and torch.equal(_bits(res.ens_sq), _bits(res.member_sq[:, 0]))
    interior = int((w.step.interior_weight != 0).sum())
    assert bool((res.rank_hist.sum(-1) == interior).all()) and int(res.rank_hist[..., 1:M].sum()) == 0   # bins 0 and M only
    # without verification: the same fields, no sums
    mean, members = res.mean.clone(), res.members.clone()
    bare = EnsembleForecast(w.step, data, LEADS, members=M, n_starts=S, verify=False).run([1, 5])
    assert bare.ens_sq is None and bare.rank_hist is None and bare.member_sq is None
    assert torch.equal(_bits(bare.mean), _bits(mean)) and torch.equal(_bits(bare.members), _bits(members))
    with pytest.raises(ValueError, match="verify"):
        bare.rmse(w.step.state_std)
    with pytest.raises(ValueError, match="latent_noise"):
        ens.run([1, 5], latent_noise=torch.zeros(LEADS, S * M, 1, 1, device=dev))
    with pytest.raises(ValueError):
        ens.run([1])
    with pytest.raises(IndexError):
        ens.run([0, ens.n_starts])


@pytest.mark.gpu
def test_engine_inside_ema_weights(dev, tmp_path):
    from neural_lam_amd.forecast import EnsembleForecast
    from neural_lam_amd.trainer import Trainer

    w = _graph_lam_step(dev, tmp_path)
    data2 = __import__("neural_lam_amd.data", fromlist=["DeviceWeatherDataset"]).DeviceWeatherDataset(
        w.state, w.forcing, w.times, ar_steps=2, standardization=w.step.standardization_stats())
    tr = Trainer(w.step, lr=1e-2, use_graph=False, ema_decay=0.5)
    for i in (0, 3):
        init, target, forcing, _ = data2.batch([i, i + 1], standardize=True)
        tr.step(init, target, forcing)
    ens = EnsembleForecast(w.step, _dataset(w), 3, members=2, n_starts=1)
    raw = _snap(ens.run([2]))
    with tr.ema_weights():
        inside = _snap(ens.run([2]))
    assert not _same(raw, inside, ["state"]) and _same(raw, _snap(ens.run([2])))
