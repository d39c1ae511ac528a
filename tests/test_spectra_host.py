"""DCT variance spectra without a GPU: the basis and the bins of neural_lam_amd.forecast against scipy and a double loop in Python
integers, Parseval on the float64 reference, every ValueError of parse_spectra and of the engines' constructors, the C layout of
nlam_dct_spectra_t and the argument checks of both entry points (every check comes before any launch, so they run here)."""
import ctypes as C
import re
import subprocess
import types

import numpy as np
import pytest
import scipy.fft
import torch

import spectra_ref as R
from conftest import ROOT
from neural_lam_amd import _lib as L
from neural_lam_amd.forecast import dct_basis, dct_bins, parse_spectra

NEW_EXPORTS = ["nlam_dct_spectra", "nlam_dct_spectra_workspace_floats"]
BIN_SHAPES = [(2, 2), (5, 9), (9, 5), (37, 29), (268, 238)]


@pytest.mark.parametrize("n", [1, 2, 3, 8, 29, 67, 238, 268])
def test_dct_basis_is_scipys_orthonormal_dct2(n):
    c = dct_basis(n)
    assert c.dtype == torch.float64 and tuple(c.shape) == (n, n)
    c = c.numpy()
    assert np.abs(c - scipy.fft.dct(np.eye(n), type=2, norm="ortho", axis=0)).max() <= 1e-14
    assert np.abs(c @ c.T - np.eye(n)).max() <= 1e-13   # the rows are orthonormal: n products of entries known to 1e-16
    x = np.random.default_rng(n).standard_normal(n)
    assert np.abs(c @ x - scipy.fft.dct(x, type=2, norm="ortho")).max() <= 1e-13


@pytest.mark.parametrize("cx,cy", BIN_SHAPES)
def test_dct_bins_equal_the_double_loop_in_integers(cx, cy):
    bin_of, bin_ptr, bin_idx, nb = dct_bins(cx, cy)
    assert nb == min(cx, cy) and bin_of.dtype == bin_ptr.dtype == bin_idx.dtype == torch.int32
    want = R.bins_ref(cx, cy)
    assert np.array_equal(bin_of.numpy().reshape(cx, cy), want)
    # every coefficient but (0, 0) is in exactly one bin, and the CSR list says the same as the table
    assert int(bin_of[0]) == -1 and int((bin_of < 0).sum()) == 1 and int(bin_of.max()) <= nb - 1
    ptr, idx = bin_ptr.tolist(), bin_idx.tolist()
    assert len(ptr) == nb + 1 and ptr[0] == 0 and ptr[-1] == len(idx) == cx * cy - 1
    assert sorted(idx) == list(range(1, cx * cy))
    for b in range(nb):
        mine = idx[ptr[b]:ptr[b + 1]]
        assert mine == sorted(mine) and all(int(bin_of[i]) == b for i in mine), b   # ascending inside the bin
    counts = np.diff(np.array(ptr))
    if (cx, cy) == (2, 2):
        # Nmin = 2: all three coefficients have k = 1 <= Nmin - 1, so the corner bin of the definition is empty at this one shape
        assert counts.tolist() == [3, 0]
    else:
        assert counts.min() >= 1, counts
    # the bin of a coefficient on an axis is its own index scaled to Nmin: (m, 0) -> floor(Nmin m / cx)
    for m in range(1, cx):
        k = min(cx, cy) * m // cx
        assert want[m, 0] == (max(k, 1) - 1 if k <= nb - 1 else nb - 1)


def test_dct_bins_and_basis_reject_bad_sizes():
    for bad in ((1, 5), (5, 1), (0, 0), (-2, 4)):
        with pytest.raises(ValueError, match="dct_bins"):
            dct_bins(*bad)
    with pytest.raises(ValueError, match="dct_basis"):
        dct_basis(0)


@pytest.mark.parametrize("cx,cy", [(2, 2), (5, 9), (33, 25), (37, 29), (70, 45), (131, 67)])
def test_reference_bins_add_up_to_the_variance(cx, cy):
    rng = np.random.default_rng(cx * 1000 + cy)
    bins = R.bins_ref(cx, cy)
    for g in (rng.standard_normal((cx, cy)) * 3.0 + 11.0, R.white_field(rng, (cx, cy)).astype(np.float64),
              R.red_field(rng, cx, cy).astype(np.float64)):
        spec, budget = R.spectra_ref(g, bins, min(cx, cy), scale=2.5)
        assert abs(spec.sum() - 2.5 * g.var()) <= 1e-12 * 2.5 * g.var()   # Parseval
        assert budget.shape == spec.shape and bool((budget >= 0).all())
    # a custom table: dropped coefficients and an empty bin
    table = np.where(bins >= 0, 1, -1)
    table[1:, 1:] = -1
    spec, budget = R.spectra_ref(g, table, 2)
    G = scipy.fft.dctn(g, norm="ortho")
    assert spec[0] == 0.0 and budget[0] == 0.0
    assert abs(spec[1] - ((G[0, 1:] ** 2).sum() + (G[1:, 0] ** 2).sum()) / (cx * cy)) <= 1e-12 * spec[1]


def test_parse_spectra_accepts_and_rejects():
    names = ["t2m", "u10", "v10", "q"]
    assert parse_spectra(None, None, None, names, 4) == ([], None, None)
    assert parse_spectra(["u10", 3], (5, 6), None, names, 4, 30) == ([1, 3], (5, 6), (0, 5, 0, 6))
    assert parse_spectra([np.int64(2), 0.0], [5, 6], (1, 4, np.int64(2), 6.0), None, 4) == ([2, 0], (5, 6), (1, 4, 2, 6))
    assert parse_spectra("q", (5, 6), [3, 5, 0, 2], names, 4) == ([3], (5, 6), (3, 5, 0, 2))
    ok = dict(spectra=["t2m"], grid_shape=(5, 6), window=None, var_names=names, n_vars=4, nodes=30)
    bad = [dict(spectra=["rain"]), dict(spectra=["t2m"], var_names=None),            # an unknown name, a name without names
           dict(spectra=[4]), dict(spectra=[-1]), dict(spectra=[1.5]), dict(spectra=[True]), dict(spectra=[None]),
           dict(spectra=["t2m", 0]), dict(spectra=[2, 2]),                           # duplicates, by name and by index
           dict(spectra=[]),
           dict(grid_shape=None), dict(grid_shape=(30,)), dict(grid_shape=(5, 7)), dict(grid_shape=(0, 30)), dict(grid_shape=(-5, -6)),
           dict(grid_shape="ab"),
           dict(window=(0, 5, 0)), dict(window=(0, 5, 0, 6, 1)), dict(window=(0.5, 5, 0, 6)), dict(window=("a", 5, 0, 6)),
           dict(window=(True, 5, 0, 6)), dict(window=7),
           dict(window=(-1, 5, 0, 6)), dict(window=(0, 6, 0, 6)), dict(window=(0, 5, 0, 7)), dict(window=(0, 5, -1, 6)),
           dict(window=(3, 3, 0, 6)), dict(window=(4, 2, 0, 6)), dict(window=(0, 5, 4, 4)),
           dict(window=(0, 1, 0, 6)), dict(window=(0, 5, 5, 6))]                     # one cell along a side
    for kw in bad:
        with pytest.raises(ValueError, match="Forecast"):
            parse_spectra(**{**ok, **kw})


def test_engines_validate_spectra_on_the_host():
    from neural_lam_amd.forecast import EnsembleForecast, Forecast, Spectra

    step = types.SimpleNamespace(state_var_names=["t2m", "u10", "v10"], state_mean=torch.zeros(3), interior_weight=torch.ones(12))
    bad = [dict(spectra=["rain"], grid_shape=(3, 4)), dict(spectra=[0, 0], grid_shape=(3, 4)), dict(spectra=[], grid_shape=(3, 4)),
           dict(spectra=[0]), dict(spectra=[0], grid_shape=(3, 5)), dict(spectra=[0], grid_shape=(3, 4), spectra_window=(0, 1, 0, 4))]
    for kw in bad:   # the checks come before anything else is read
        with pytest.raises(ValueError, match="Forecast: "):
            Forecast(step, None, 3, **kw)
        with pytest.raises(ValueError, match="Forecast: "):
            EnsembleForecast(step, None, 3, members=2, **kw)
    with pytest.raises(ValueError, match="Forecast needs"):   # valid arguments pass on to the next check
        Forecast(step, None, 3, spectra=["u10"], grid_shape=(3, 4), spectra_window=(0, 3, 1, 4))
    with pytest.raises(ValueError, match="Forecast needs"):
        Forecast(step, None, 3)
    # a trailing field with a default: positional construction elsewhere keeps working
    from neural_lam_amd.forecast import EnsembleResult, ForecastResult

    assert ForecastResult._fields[-1] == "spectra" == EnsembleResult._fields[-1]
    assert ForecastResult(1, 2, 3, 4, 5).spectra is None and EnsembleResult(*range(15)).spectra is None
    sp = Spectra(None, None, None, (0,), torch.tensor([0.25, 0.5, 0.75, float("nan")], dtype=torch.float64), (0, 4, 0, 4))
    wl = sp.wavelength(2.5)
    assert wl[:2].tolist() == [20.0, 10.0] and abs(float(wl[2]) - 20.0 / 3) < 1e-14 and bool(torch.isnan(wl[3]))


def test_spectra_symbols_are_exported_and_the_structs_match_c_layout(tmp_path):
    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    fields = [name for name, _ in L.DctSpectra._fields_]
    sub = [name for name, _ in L.DctSpectraSrc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
                   'int main(){printf("%zu %zu", sizeof(nlam_dct_spectra_t), sizeof(nlam_dct_spectra_src_t));\n'
                   + "".join(f'printf(" %zu", offsetof(nlam_dct_spectra_t, {f}));\n' for f in fields)
                   + "".join(f'printf(" %zu", offsetof(nlam_dct_spectra_src_t, {f}));\n' for f in sub)
                   + 'printf(" %d %d\\n", NLAM_SPEC_MAX_SOURCES, NLAM_EVAL_MAX_VARS); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == ([C.sizeof(L.DctSpectra), C.sizeof(L.DctSpectraSrc)] + [getattr(L.DctSpectra, f).offset for f in fields]
                   + [getattr(L.DctSpectraSrc, f).offset for f in sub] + [L.SPEC_MAX_SOURCES, L.EVAL_MAX_VARS])
    # the header declares the fields in the binding's order (the offsets above ascend, so equal offsets mean equal order)
    offs = [getattr(L.DctSpectra, f).offset for f in fields]
    assert offs == sorted(offs) and len(set(offs)) == len(offs) and L.SPEC_MAX_SOURCES == 3


POINTERS = ("origin", "basis_x", "basis_y", "var", "bin_ptr", "bin_idx", "state_std", "lead", "workspace")


def test_spectra_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    ws = lib.nlam_dct_spectra_workspace_floats
    assert ws(5, 33, 25, 3) == 2 * 5 * 33 * 25 * 3 and ws(1, 2, 2, 1) == 8
    assert ws(3 * 65535, 268, 238, 17) == 2 * 3 * 65535 * 268 * 238 * 17
    for bad in ((0, 5, 5, 1), (1, 1, 5, 1), (1, 5, 1, 1), (1, 5, 5, 0), (-1, 5, 5, 1), (1, -5, 5, 1)):
        assert ws(*bad) == -1, bad
    for bad in ((3 * 65535 + 1, 5, 5, 1), (1, 5, 5, 257), (1, 1 << 16, 1 << 15, 1), (1, 1 << 15, 1 << 15, 2)):
        assert ws(*bad) == -2, bad
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    NX, NY, F, V, CX, CY, NB, LEAD = 37, 29, 5, 3, 33, 25, 25, 4
    batches = (3, 2, 1)
    nws = ws(sum(batches), CX, CY, V)

    def args(src=None, **kw):
        p = L.DctSpectra()
        for name in POINTERS:
            setattr(p, name, fake)
        for k, b in enumerate(batches):
            p.src[k].x, p.src[k].spec, p.src[k].batch, p.src[k].batch_stride = fake, fake, b, NX * NY * F
        p.workspace_floats, p.sources, p.nx, p.ny, p.d_state, p.vars, p.bins, p.bin_entries = nws, 3, NX, NY, F, V, NB, CX * CY - 1
        p.max_lead, p.cx, p.cy = LEAD, CX, CY
        for k, v in kw.items():
            setattr(p, k, v)
        for (k, name), v in (src or {}).items():
            setattr(p.src[k], name, v)
        return C.byref(p)

    call = lib.nlam_dct_spectra
    assert call(None, None) == -1
    einval = [{name: None} for name in POINTERS]
    einval += [dict(sources=0), dict(sources=4), dict(sources=-1), dict(nx=0), dict(ny=0), dict(d_state=0), dict(vars=0), dict(bins=0),
               dict(max_lead=0), dict(cx=1), dict(cy=1), dict(cx=0), dict(cx=NX + 1), dict(cy=NY + 1), dict(bin_entries=-1),
               dict(bin_entries=CX * CY + 1), dict(workspace_floats=nws - 1)]
    for kw in einval:
        assert call(args(**kw), None) == -1, kw
    for k in range(3):
        for src in ({(k, "x"): None}, {(k, "spec"): None}, {(k, "batch"): 0}, {(k, "batch_stride"): -1}, {(k, "lead_stride"): -1}):
            assert call(args(src=src), None) == -1, src
    big = 1 << 50
    for kw in (dict(d_state=257), dict(vars=F + 1), dict(nx=1 << 16, ny=1 << 15), dict(nx=1 << 14, ny=1 << 14, d_state=8, vars=8)):
        assert call(args(workspace_floats=big, **kw), None) == -2, kw
    assert call(args(src={(1, "batch"): 65536}, workspace_floats=big), None) == -2
    # sources beyond `sources` are not looked at: a batch of 0 there would be NLAM_EINVAL, which comes first
    assert call(args(src={(2, "x"): None, (2, "batch"): 0}, sources=2, d_state=257, workspace_floats=big), None) == -2
    assert call(args(src={(2, "batch"): 0}, d_state=257, workspace_floats=big), None) == -1
