"""nlam_dct_spectra at the C-ABI against the float64 reference of spectra_ref.py (scipy.fft.dctn of the fp32 inputs and the same bins;
no basis is shared with the code under test), within the rounding budget derived there.  Before anything is compared the test
asserts, from the reference alone, that the budget is at most 5 % of the bin's power in every bin, so the budget cannot hide a
failure.  Windows cx x cy, each the smallest where something new can break: 2 x 2 and 5 x 9 (below one MFMA tile both ways),
33 x 25 (one past a tile in M and K, cut as the window (3, 36, 2, 27) of a 37 x 29 grid: offsets, and a row stride that is not
cy), 37 x 29 whole, 70 x 45, 131 x 67 (more than two K tiles of 32, ragged M, N and K at once)."""
import ctypes as C

import numpy as np
import pytest
import torch

import spectra_ref as R
from neural_lam_amd import _lib as L
from neural_lam_amd.forecast import dct_basis, dct_bins

POISON = -7.0   # no output is negative
SHAPES = {"2x2": (2, 2, None), "5x9": (5, 9, None), "33x25": (37, 29, (3, 36, 2, 27)), "37x29": (37, 29, None), "70x45": (70, 45, None),
          "131x67": (131, 67, None)}
RED = ("2x2", "5x9", "33x25", "37x29", "70x45")   # the precondition holds for a red spectrum up to 70 x 45 (spectra_ref.py)
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Src:
    """One source: ``x`` (batch, nx * ny, F) fp32 numpy.  ``layout``: "plain", "stride2" (``batch_stride`` twice the row block, NaN
    between the items) or "slots" (a (batch, max_lead, N, F) buffer with ``lead_stride``; every other lead's slot is NaN)."""

    def __init__(self, x, layout="plain", physical=False):
        self.x, self.layout, self.physical = x, layout, physical


class Call:
    """The device tables, buffers and argument struct of one nlam_dct_spectra call."""

    def __init__(self, dev, nx, ny, F, var, window, sources, lead=0, max_lead=1, std=None, table=None):
        i0, i1, j0, j1 = window or (0, nx, 0, ny)
        cx, cy, N = i1 - i0, j1 - j0, nx * ny
        if table is None:
            _, bin_ptr, bin_idx, nb = dct_bins(cx, cy)
            self.bin_of = R.bins_ref(cx, cy)
        else:   # a custom table (cx, cy) -> bin or -1
            self.bin_of, nb = np.asarray(table), int(np.max(table)) + 2   # one more bin than the table uses: it stays empty
            lists = [np.flatnonzero(self.bin_of.reshape(-1) == b) for b in range(nb)]
            bin_ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(v) for v in lists])]), dtype=torch.int32)
            bin_idx = torch.tensor(np.concatenate(lists), dtype=torch.int32)
        self.geom = (nx, ny, F, list(var), (i0, i1, j0, j1), nb, lead, max_lead)
        self.sources = sources
        self.std = np.ones(F, dtype=np.float32) if std is None else std
        f32 = dict(device=dev, dtype=torch.float32)
        self.keep = [dct_basis(cx).to(**f32), dct_basis(cy).to(**f32), bin_ptr.to(dev), bin_idx.to(dev),
                     torch.tensor(list(var), device=dev, dtype=torch.int32), torch.tensor([i0, j0], device=dev, dtype=torch.int32),
                     torch.tensor(self.std, **f32), torch.tensor([lead], device=dev, dtype=torch.int32)]
        bx, by, bp, bi, vr, org, sd, ld = self.keep
        items = sum(s.x.shape[0] for s in sources)
        nws = int(L.load().nlam_dct_spectra_workspace_floats(items, cx, cy, len(var)))
        assert nws == 2 * items * cx * cy * len(var)
        self.workspace = torch.full((nws + 64,), float("nan"), **f32)
        p = L.DctSpectra()
        self.bufs, self.outs = [], []
        for k, s in enumerate(sources):
            B = s.x.shape[0]
            x = torch.tensor(s.x, **f32)
            if s.layout == "plain":
                buf, bstride, lstride = x.clone(), N * F, 0
            elif s.layout == "stride2":
                buf = torch.full((B, 2, N, F), float("nan"), **f32)
                buf[:, 0] = x
                bstride, lstride = 2 * N * F, 0
            else:
                buf = torch.full((B, max_lead, N, F), float("nan"), **f32)
                buf[:, min(lead, max_lead - 1)] = x
                bstride, lstride = max_lead * N * F, N * F
            out = torch.full((B, max_lead, len(var), nb), POISON, **f32)
            self.bufs.append(buf)
            self.outs.append(out)
            q = p.src[k]
            q.x, q.spec, q.batch_stride, q.lead_stride, q.batch, q.physical = buf.data_ptr(), out.data_ptr(), bstride, lstride, B, int(s.physical)
        p.origin, p.basis_x, p.basis_y, p.var, p.bin_ptr, p.bin_idx = (_ptr(t) for t in (org, bx, by, vr, bp, bi))
        p.state_std, p.lead, p.workspace, p.workspace_floats = _ptr(sd), _ptr(ld), _ptr(self.workspace), nws
        p.sources, p.nx, p.ny, p.d_state, p.vars, p.bins, p.bin_entries, p.max_lead = len(sources), nx, ny, F, len(var), nb, int(bi.numel()), max_lead
        p.cx, p.cy = cx, cy
        self.p, self.nws = p, nws

    def run(self):
        rc = L.load().nlam_dct_spectra(C.byref(self.p), _stream())
        torch.cuda.synchronize()
        return rc

    def reference(self):
        """Per source ``(spec, budget)``, each (batch, V, nb) float64, after the precondition on every bin that holds anything."""
        nx, ny, F, var, (i0, i1, j0, j1), nb, _, _ = self.geom
        res = []
        for s in self.sources:
            spec = np.zeros((s.x.shape[0], len(var), nb))
            budget = np.zeros_like(spec)
            for b in range(s.x.shape[0]):
                for v, f in enumerate(var):
                    g = s.x[b].reshape(nx, ny, F)[i0:i1, j0:j1, f]
                    scale = 1.0 if s.physical else float(np.float64(self.std[f]) ** 2)
                    spec[b, v], budget[b, v] = R.spectra_ref(g, self.bin_of, nb, scale)
            assert bool((budget <= 0.05 * spec).all()), float((budget / np.maximum(spec, 1e-300)).max())   # the precondition
            res.append((spec, budget))
        return res

    def check(self, what):
        """The lead's slot within the budget; every other slot and the words behind the workspace untouched."""
        _, _, _, _, _, _, lead, max_lead = self.geom
        for k, (spec, budget) in enumerate(self.reference()):
            got = self.outs[k].cpu().double().numpy()
            for other in range(max_lead):
                if other != lead:
                    assert bool((got[:, other] == POISON).all()), (what, k, other)
            err = np.abs(got[:, lead] - spec)
            ratio = float(np.max(err / np.where(budget > 0, budget, 1.0) * (budget > 0)))
            WORST["ratio"] = max(WORST["ratio"], ratio)
            print(f"spectra {what} source {k}: worst error / budget {ratio:.3e} (all tests so far {WORST['ratio']:.3e})")
            assert bool((err <= budget).all()), (what, k, ratio)
            assert bool((got[:, lead][budget == 0] == 0).all()), (what, k)   # an empty bin is exactly 0
        assert bool(torch.isnan(self.workspace[self.nws:]).all()), what


def _fields(rng, name, batch, F, red=False):
    nx, ny, win = SHAPES[name]
    i0, i1, j0, j1 = win or (0, nx, 0, ny)
    x = R.white_field(rng, (batch, nx, ny, F))
    if red and name in RED:   # a red window inside the white grid
        for b in range(batch):
            for f in range(F):
                x[b, i0:i1, j0:j1, f] = R.red_field(rng, i1 - i0, j1 - j0)
    return x.reshape(batch, nx * ny, F)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_variable_of_five(dev, name):
    """d_state = 5, vars = [3]: one source, batch 1; a red spectrum where its precondition holds."""
    nx, ny, win = SHAPES[name]
    rng = np.random.default_rng(1)
    for red in (False, True):
        call = Call(dev, nx, ny, 5, [3], win, [Src(_fields(rng, name, 1, 5, red))], std=np.array([1, 2, 3, 0.5, 7], dtype=np.float32))
        assert call.run() == 0
        call.check((name, "one of five", red))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_three_variables_out_of_memory_order_two_sources(dev, name):
    """d_state = 5, vars = [4, 0, 2]; batch 3 and a second source of batch 1 whose batch stride is twice its row block."""
    nx, ny, win = SHAPES[name]
    rng = np.random.default_rng(2)
    std = np.array([0.25, 1, 3, 1, 11], dtype=np.float32)
    call = Call(dev, nx, ny, 5, [4, 0, 2], win, [Src(_fields(rng, name, 3, 5)), Src(_fields(rng, name, 1, 5), "stride2")], std=std)
    assert call.run() == 0
    call.check((name, "three of five"))
    two = Call(dev, nx, ny, 5, [4, 0, 2], win, [Src(_fields(rng, name, 2, 5, True), "stride2")], std=std)
    assert two.run() == 0
    two.check((name, "stride2 batch 2"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["5x9", "33x25", "131x67"])
def test_a_variable_listed_twice(dev, name):
    """The C-ABI takes any ``var`` table (the engine rejects duplicates; the launch does not): vars = [2, 2, 0] gives the spectrum
    of variable 2 twice, with equal bits, and that of variable 0."""
    nx, ny, win = SHAPES[name]
    rng = np.random.default_rng(9)
    call = Call(dev, nx, ny, 5, [2, 2, 0], win, [Src(_fields(rng, name, 2, 5)), Src(_fields(rng, name, 1, 5), "stride2")],
                std=np.array([3, 1, 0.5, 1, 1], dtype=np.float32))
    assert call.run() == 0
    call.check((name, "listed twice"))
    assert all(torch.equal(_bits(o[:, :, 0]), _bits(o[:, :, 1])) for o in call.outs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("lead", [0, 2])
def test_all_four_variables_three_sources_and_lead_slots(dev, name, lead):
    """d_state = 4 with all four (aligned rows); three sources: batch 3, batch 1, and a physical one read through its lead
    stride at lead 0 and at lead 2 of max_lead = 3.  Two runs give equal bits."""
    nx, ny, win = SHAPES[name]
    rng = np.random.default_rng(3 + lead)
    srcs = [Src(_fields(rng, name, 3, 4)), Src(_fields(rng, name, 1, 4)), Src(_fields(rng, name, 3, 4) * np.float32(3.0), "slots", physical=True)]
    call = Call(dev, nx, ny, 4, [0, 1, 2, 3], win, srcs, lead=lead, max_lead=3, std=np.array([2, 0.5, 1, 5], dtype=np.float32))
    assert call.run() == 0
    call.check((name, "four of four", lead))
    first = [o.clone() for o in call.outs]
    call.workspace.fill_(float("nan"))
    for o in call.outs:
        o.fill_(POISON)
    assert call.run() == 0
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, call.outs))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["5x9", "33x25", "131x67"])
def test_a_lead_past_the_end_writes_nothing(dev, name):
    nx, ny, win = SHAPES[name]
    rng = np.random.default_rng(5)
    for lead in (3, 4, 2 ** 31 - 1):
        call = Call(dev, nx, ny, 4, [1, 3], win, [Src(_fields(rng, name, 2, 4)), Src(_fields(rng, name, 1, 4), "slots", True)], lead=lead, max_lead=3)
        assert call.run() == 0
        assert all(bool((o == POISON).all()) for o in call.outs) and bool(torch.isnan(call.workspace).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_a_custom_bin_table_with_dropped_coefficients_and_an_empty_bin(dev, name):
    """Two bins that hold something -- the first row and the first column of the coefficients; the rest, and (0, 0), dropped --
    and a third that holds nothing: the reference's sums, and exactly 0."""
    nx, ny, win = SHAPES[name]
    i0, i1, j0, j1 = win or (0, nx, 0, ny)
    table = np.full((i1 - i0, j1 - j0), -1)
    table[0, 1:], table[1:, 0] = 0, 1
    rng = np.random.default_rng(6)
    call = Call(dev, nx, ny, 5, [2, 1], win, [Src(_fields(rng, name, 2, 5))], table=table)
    assert call.geom[5] == 3 and call.run() == 0
    call.check((name, "custom table"))
    assert bool((call.outs[0][:, 0, :, 2] == 0).all()) and bool((call.outs[0][:, 0, :, :2] > 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_default_bins_add_up_to_the_variance_of_the_window(dev, name):
    nx, ny, win = SHAPES[name]
    i0, i1, j0, j1 = win or (0, nx, 0, ny)
    rng = np.random.default_rng(7)
    x = _fields(rng, name, 2, 3) * np.float32(2.0) + np.float32(0.5)
    std = np.array([3, 1, 0.125], dtype=np.float32)
    call = Call(dev, nx, ny, 3, [0, 1, 2], win, [Src(x)], std=std)
    assert call.run() == 0
    (spec, budget), = call.reference()
    got = call.outs[0][:, 0].cpu().double().numpy().sum(-1)
    var = x.astype(np.float64).reshape(2, nx, ny, 3)[:, i0:i1, j0:j1].var(axis=(1, 2)) * std.astype(np.float64) ** 2
    assert bool((np.abs(got - var) <= budget.sum(-1) + 1e-12 * var).all()), (got, var)


@pytest.mark.gpu
def test_bad_arguments_return_before_any_launch(dev):
    nx, ny, win = SHAPES["33x25"]
    rng = np.random.default_rng(8)

    def fresh():
        return Call(dev, nx, ny, 5, [4, 0], win, [Src(_fields(rng, "33x25", 2, 5)), Src(_fields(rng, "33x25", 1, 5), physical=True)], max_lead=2)

    def untouched(call):
        torch.cuda.synchronize()
        return all(bool((o == POISON).all()) for o in call.outs) and bool(torch.isnan(call.workspace).all())

    einval = [{name: None} for name in ("origin", "basis_x", "basis_y", "var", "bin_ptr", "bin_idx", "state_std", "lead", "workspace")]
    einval += [dict(sources=0), dict(sources=4), dict(nx=0), dict(ny=0), dict(d_state=0), dict(vars=0), dict(bins=0), dict(max_lead=0), dict(cx=1),
               dict(cy=1), dict(cx=nx + 1), dict(cy=ny + 1), dict(bin_entries=-1), dict(bin_entries=33 * 25 + 1)]
    eunsup = [dict(d_state=257), dict(vars=6), dict(nx=1 << 16, ny=1 << 15)]
    for kw, want in [(kw, -1) for kw in einval] + [(kw, -2) for kw in eunsup]:
        call = fresh()
        for k, v in kw.items():
            setattr(call.p, k, v)
        assert call.run() == want and untouched(call), kw
    call = fresh()
    call.p.workspace_floats = call.nws - 1
    assert call.run() == -1 and untouched(call)
    for k, (name, value, want) in [(k, c) for k in range(2) for c in (("x", None, -1), ("spec", None, -1), ("batch", 0, -1), ("batch_stride", -1, -1),
                                                                      ("lead_stride", -1, -1), ("batch", 65536, -2))]:
        call = fresh()
        setattr(call.p.src[k], name, value)
        call.p.workspace_floats = 1 << 50
        assert call.run() == want and untouched(call), (k, name)
    # a call whose sources are all physical needs no state_std; the origin is clamped into the grid
    call = Call(dev, nx, ny, 5, [4, 0], win, [Src(_fields(rng, "33x25", 2, 5), physical=True)])
    call.p.state_std = None
    assert call.run() == 0
    call.check("physical only")
    edge = Call(dev, nx, ny, 5, [4, 0], (4, 37, 4, 29), [Src(call.sources[0].x, physical=True)])
    edge.keep[5].copy_(torch.tensor([1000, -5], dtype=torch.int32))   # clamped to (nx - cx, 0) = (4, 0)
    want = Call(dev, nx, ny, 5, [4, 0], (4, 37, 0, 25), [Src(call.sources[0].x, physical=True)])
    assert edge.run() == 0 and want.run() == 0
    assert torch.equal(_bits(edge.outs[0]), _bits(want.outs[0]))
    want.check("clamped origin")
