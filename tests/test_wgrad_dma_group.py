"""nlam_wgrad_dma_group: several narrow weight gradients of ONE kernel shape in one grid.

Every member must come out exactly as from a launch of its own (nlam_wgrad at the same nparts): the grouped kernel runs the
body of wgrad_dma_kernel on the member's own range of workgroups.  So the check is torch.equal on the PARTIALS, member by
member, for every group size and member order -- and, through the same reduction, the float64 bound of test_wgrad_kernels.
Partials are allocated NaN-poisoned: a workgroup that writes nothing, or into a neighbour's buffer, shows.

One geometry cannot be built for the grouped entry point: "nparts larger than the chunk count".  The entry point
refuses any member whose nparts is not nlam_wgrad_nparts(member), and that never exceeds the member's chunk count.  The body
is shared with the plain kernel, which takes any nparts: test_empty_sequences_write_zero_partials checks it there."""
import ctypes as C
from dataclasses import replace

import pytest
import torch

from neural_lam_amd import _lib as L
from test_wgrad_kernels import C_, MM3, describe, launch, make_operands, reduce_sum, reference, tau

pytestmark = pytest.mark.gpu

CAP = L.NLAM_MAX_GROUP
EINVAL, EUNSUP = -1, -2

# the four instantiated shapes (+ m = 32, where waves 1 .. 3 own no output block): (m, widths, SiLU)
SHAPES = {
    "dw2": (64, (64,), False),
    "dw2_silu": (64, (64,), True),
    "dw1_2src": (64, (64, 64), False),
    "dw1_3src": (64, (64, 64, 64), False),
    "dw2_m32": (32, (32,), False),
}


def members_of(shape):
    """Eight members of one shape, the smallest geometries that can go wrong: one row; one row short of a chunk; exactly one; one
    over; two chunks and a row; two batch items of 40 rows (chunks of 32, 8, 32, 8 rows: a short chunk in the middle) with a
    batch-shared source; 131 chunks on 128 workgroups (three workgroups sum two chunks); gathered and plain sources mixed."""
    m, widths, silu = SHAPES[shape]
    last = len(widths) - 1
    geo = [dict(rows=1), dict(rows=31, gather=(0,)), dict(rows=32), dict(rows=33, gather=(last,)), dict(rows=65),
           dict(rows=40, batch=2, broadcast=(0,)), dict(rows=131 * 32 - 5, gather=(0,)), dict(rows=40, batch=2, gather=tuple(range(len(widths))))]
    return [C_(f"{shape}_{k}", L.WGP_DMA, m, widths, silu=silu, **g) for k, g in enumerate(geo)]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_SINGLE = {}   # shape -> [(case, A, Ad, srcs, partials of its own launch, nparts)]: computed once, shared, never written again


def singles(lib, shape):
    if shape not in _SINGLE:
        out = []
        for k, case in enumerate(members_of(shape)):
            A, Ad, srcs = make_operands(case, torch.Generator().manual_seed(100 + k), False)
            partials, _, nparts = launch(lib, case, Ad, srcs)
            out.append((case, A, Ad, srcs, partials, nparts))
        _SINGLE[shape] = out
    return _SINGLE[shape]


def poisoned(nparts, m, n):
    return torch.full((nparts, m, n), float("nan"), device="cuda", dtype=torch.float32)


def group_launch(lib, picked):
    """One grouped launch of the members ``picked`` (entries of singles()) -> (return code, their NaN-poisoned partials)."""
    qs, parts = [], []
    for case, _A, Ad, srcs, _p, nparts in picked:
        q = describe(lib, case, Ad, srcs)
        assert q.nparts == nparts and lib.nlam_wgrad_dma_group_supported(C.byref(q)) == 1
        buf = poisoned(nparts, case.m, q.n)
        q.partials = buf.data_ptr()
        qs.append(q)
        parts.append(buf)
    arr = (L.Wgrad * len(qs))(*qs)
    rc = lib.nlam_wgrad_dma_group(arr, len(qs), _stream())
    torch.cuda.synchronize()
    return rc, parts


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("size", [1, 2, CAP])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_members_equal_their_own_launch(lib, shape, size, order):
    one = singles(lib, shape)
    picked = {1: one[4:5], 2: one[4:6], CAP: one[:CAP]}[size]
    if order == "reversed":
        picked = picked[::-1]
    rc, parts = group_launch(lib, picked)
    assert rc == 0
    for (case, A, _Ad, srcs, own, nparts), got in zip(picked, parts):
        assert torch.isfinite(got).all(), f"{case}: unwritten partials"
        assert torch.equal(got, own), f"{case}: grouped partials differ from the member's own launch"
        if size == CAP and order == "forward":
            out = reduce_sum(lib, got, nparts, case.m, got.shape[2])
            torch.cuda.synchronize()
            R, scale, tie = reference(case, A, srcs)
            err = (out.double().cpu() - R).abs()
            bound = tau(case, nparts) * scale + 2.0 ** -7 * tie
            ratio = float((err / scale.clamp_min(1e-300)).max())
            print(f"{case}: worst err/scale {ratio:.3e}, tau {tau(case, nparts):.3e}")
            assert not (err > bound).any(), f"{case}: over the float64 bound; worst err/scale {ratio:.3e}"


@pytest.mark.parametrize("shape", ["dw2_silu", "dw1_2src"])
def test_empty_sequences_write_zero_partials(lib, shape):
    """More workgroups than chunks (the shared body, through the plain kernel -- see the module docstring): the workgroups
    without a chunk write zeros, the others what they write at the natural nparts."""
    case, _A, Ad, srcs, own, nparts = singles(lib, shape)[4]   # 65 rows: three chunks
    assert nparts == 3
    q = describe(lib, case, Ad, srcs)
    buf = poisoned(nparts + 4, case.m, q.n)
    q.partials, q.nparts = buf.data_ptr(), nparts + 4
    assert lib.nlam_wgrad(C.byref(q), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(buf).all()
    live = buf.abs().sum((1, 2)) > 0
    assert int(live.sum()) == 3 and torch.equal(buf[~live], torch.zeros_like(buf[~live]))
    assert torch.equal(buf.double().sum(0), buf[live].double().sum(0))


def _pair(lib, shape="dw2"):
    one = singles(lib, shape)
    return [one[3], one[4]]


def _refused(lib, qs, bufs, n, want):
    arr = (L.Wgrad * max(len(qs), 1))(*qs)
    rc = lib.nlam_wgrad_dma_group(arr, n, _stream())
    torch.cuda.synchronize()
    assert rc == want, (rc, want)
    for b in bufs:
        assert torch.isnan(b).all(), "a refused group wrote partials"


def _described(lib, entries, extra_parts=0):
    qs, bufs = [], []
    for case, _A, Ad, srcs, _p, _np in entries:
        q = describe(lib, case, Ad, srcs)
        buf = poisoned(q.nparts + extra_parts, case.m, q.n)
        q.partials = buf.data_ptr()
        qs.append(q)
        bufs.append(buf)
    return qs, bufs


def _fresh(lib, case, seed=7):
    A, Ad, srcs = make_operands(case, torch.Generator().manual_seed(seed), False)
    return (case, A, Ad, srcs, None, None)


def test_refusals_launch_nothing(lib):
    base = _pair(lib)
    qs, bufs = _described(lib, base)
    _refused(lib, qs, bufs, 0, EINVAL)
    assert lib.nlam_wgrad_dma_group(None, 2, _stream()) == EINVAL
    # cap + 1 members
    many = singles(lib, "dw2")[:CAP] + [singles(lib, "dw2")[0]]
    qs9, bufs9 = _described(lib, many)
    _refused(lib, qs9, bufs9, CAP + 1, EINVAL)
    # a member of another width / another flag: each fine alone, not together
    other_w = _fresh(lib, C_("w32", L.WGP_DMA, 64, (32,), 33))
    qs, bufs = _described(lib, [base[0], other_w])
    assert lib.nlam_wgrad_dma_group_supported(C.byref(qs[1])) == 1
    _refused(lib, qs, bufs, 2, EUNSUP)
    other_f = singles(lib, "dw2_silu")[3]
    qs, bufs = _described(lib, [base[0], other_f])
    _refused(lib, qs, bufs, 2, EUNSUP)
    # a (blocks per wave, sources) pair without an instantiation: two 32-column sources on m = 32 are two blocks on four waves
    odd = [_fresh(lib, C_("odd_a", L.WGP_DMA, 32, (32, 32), 33)), _fresh(lib, C_("odd_b", L.WGP_DMA, 32, (32, 32), 65), seed=8)]
    qs, bufs = _described(lib, odd)
    assert lib.nlam_wgrad_plan(C.byref(qs[0])) == L.WGP_DMA and lib.nlam_wgrad_dma_group_supported(C.byref(qs[0])) == 0
    _refused(lib, qs, bufs, 2, EUNSUP)
    # a member of the split-bf16 wide family
    wide = [_fresh(lib, C_("wide_a", L.WGP_WBF, 128, (128,), 100, mm=MM3)), _fresh(lib, C_("wide_b", L.WGP_WBF, 128, (128,), 70, mm=MM3), seed=8)]
    qs, bufs = _described(lib, wide)
    assert lib.nlam_wgrad_plan(C.byref(qs[0])) == L.WGP_WBF and lib.nlam_wgrad_dma_group_supported(C.byref(qs[0])) == 0
    _refused(lib, qs, bufs, 2, EUNSUP)
    qs, bufs = _described(lib, [base[0], wide[0]])
    _refused(lib, qs, bufs, 2, EUNSUP)
    # nparts off by one (the buffers have room for it)
    for delta in (1, -1):
        qs, bufs = _described(lib, base, extra_parts=1)
        qs[1].nparts += delta
        _refused(lib, qs, bufs, 2, EINVAL)


def test_supported_is_a_question_about_the_shape(lib):
    """No pointer is read: a description without operands answers like one with them."""
    for shape, (m, widths, silu) in SHAPES.items():
        q = L.Wgrad()
        q.m, q.batch, q.rows, q.nsrc, q.n = m, 1, 6561, len(widths), sum(widths)
        q.flags = MM3 | (L.F_SILU_B if silu else 0)
        for k, w in enumerate(widths):
            q.src[k].width = w
        assert lib.nlam_wgrad_dma_group_supported(C.byref(q)) == 1, shape
        q.flags |= L.F_A_BF16
        assert lib.nlam_wgrad_dma_group_supported(C.byref(q)) == 0, shape
    assert lib.nlam_wgrad_dma_group_supported(None) == 0
    silu3 = replace(members_of("dw1_3src")[0], silu=True)
    A, Ad, srcs = make_operands(silu3, torch.Generator().manual_seed(3), False)
    assert lib.nlam_wgrad_dma_group_supported(C.byref(describe(lib, silu3, Ad, srcs))) == 0   # SiLU comes with one source only
