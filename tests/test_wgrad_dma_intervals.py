"""wgrad_dma_kernel with R = 1, 2, 4 chunks of 32 rows per barrier interval (NLAM_TUNE_WGRAD_DMA_R), against float64 math.

R changes how many chunks a workgroup requests behind one barrier, never which chunks it sums or in which order: the partials
must be the same bits for every R.  Every case passes nparts itself, so the workgroups' chunk sequences have the lengths that
matter to the interval loop: 1 and 2 (shorter than an interval), 3 and 5 (a short last interval), 4 and 12 (whole intervals).
Each (case, nparts) runs the two tiers of tests/test_wgrad_kernels.py -- (a) small-integer operands come out exactly, partial
slices included; (b) random operands with a scale per column stay within its tau bound -- for every R, and the partials of the
three R are compared with torch.equal.  A value of R the LDS does not hold for the case's source count is clamped by the
library (4 -> 2 with two or three sources); it is launched all the same."""
import pytest
import torch

from neural_lam_amd import _lib as L
from test_wgrad_kernels import C_, launch, make_operands, reference, tau

pytestmark = pytest.mark.gpu

RS = (1, 2, 4)
DMA = L.WGP_DMA
CASES = [
    # (case, nparts values); chunk sequences per workgroup in the comments
    # three sources of full width: three output blocks per wave.  357 rows = 12 chunks, the last of 5 rows: 12 | 4 4 4 | 3 3 2 2 2 |
    # 2 2 2 2 2 1 1 | 1 x 12
    (C_("w64x3_r357", DMA, 64, [64, 64, 64], 357), (1, 3, 5, 7, 12)),
    # 3 x 70 rows: 9 chunks, every third one a 6-row tail in the middle of a sequence; source 1 shared by the batch, 0 and 2
    # gathered (unsorted, repeated rows): 9 | 5 4 | 3 2 2 2
    (C_("w60_60_12_b3", DMA, 64, [60, 60, 12], 70, batch=3, broadcast=(1,), gather=(0, 2)), (1, 2, 4)),
    # one un-gathered source with SiLU (the dW2 launch): one block per wave.  12 | 3 3 2 2 2
    (C_("w64_silu_r357", DMA, 64, [64], 357, silu=True), (1, 5)),
    # two sources: two blocks per wave.  200 rows = 7 chunks: 7 | 3 2 2
    (C_("w64x2_r200", DMA, 64, [64, 64], 200), (1, 3)),
    # one 32 x 32 output block: three of the four waves have none.  165 rows = 6 chunks: 6 | 3 3
    (C_("w32_r165", DMA, 32, [32], 165), (1, 2)),
    # the width of the smallest configuration: 2 x 40 rows = 4 chunks, two of them of 8 rows
    (C_("w16_b2_r40", DMA, 16, [16], 40, batch=2), (1,)),
    # (blocks per wave, sources) pairs without an instantiation of their own -- the run-time source count, one chunk per
    # interval whatever R says
    (C_("w16x3_b2_r40", DMA, 16, [16, 16, 16], 40, batch=2, gather=(1,)), (1, 3)),
    (C_("w32x2_r165", DMA, 32, [32, 32], 165, gather=(0,)), (2,)),
]
PARAMS = [pytest.param(case, nparts, id=f"{case.name}-np{nparts}") for case, parts in CASES for nparts in parts]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib = L.load()
    yield lib
    lib.nlam_set_tuning(L.TUNE_WGRAD_DMA_R, 0)


def _for_every_r(lib, case, nparts, integer, seed):
    """The case's partials and reduced dW for every R, from one set of operands."""
    gen = torch.Generator().manual_seed(seed)
    A, Ad, srcs = make_operands(case, gen, integer)
    runs = {}
    try:
        for r in RS:
            assert lib.nlam_set_tuning(L.TUNE_WGRAD_DMA_R, r) == 0
            partials, out, np_ = launch(lib, case, Ad, srcs, nparts)   # asserts the plan: WGP_DMA
            assert np_ == nparts
            runs[r] = (partials, out)
    finally:
        lib.nlam_set_tuning(L.TUNE_WGRAD_DMA_R, 0)
    return A, srcs, runs


@pytest.mark.parametrize("case,nparts", PARAMS)
def test_intervals_exact_and_bit_identical(lib, case, nparts):
    if not case.silu:   # tier (a)
        A, srcs, runs = _for_every_r(lib, case, nparts, True, 21)
        R, _, _ = reference(case, A, srcs)
        for r, (partials, out) in runs.items():
            assert torch.isfinite(partials).all(), f"{case} R={r}: unwritten partials"
            assert torch.equal(partials.double().sum(0).cpu(), R), f"{case} R={r}: partials do not sum to the exact product"
            assert torch.equal(out.double().cpu(), R), f"{case} R={r}: reduced dW is not the exact product"
    # tier (b), and the same bits for every R
    A, srcs, runs = _for_every_r(lib, case, nparts, False, 22)
    R, scale, tie = reference(case, A, srcs)
    bound = tau(case, nparts) * scale + 2.0 ** -7 * tie
    for r, (partials, out) in runs.items():
        err = (out.double().cpu() - R).abs()
        ratio = float((err / scale.clamp_min(1e-300)).max())
        assert not (err > bound).any(), f"{case} R={r}: worst err/scale {ratio:.3e}, tau {tau(case, nparts):.3e}"
        assert torch.equal(partials, runs[RS[0]][0]), f"{case}: partials of R={r} differ from R={RS[0]}"
        assert torch.equal(out, runs[RS[0]][1]), f"{case}: reduced dW of R={r} differs from R={RS[0]}"


def test_tuning_key_values(lib):
    """0 (the built-in choice), 1, 2 and 4 are accepted, everything else refused."""
    try:
        for v in (1, 2, 4, 0):
            assert lib.nlam_set_tuning(L.TUNE_WGRAD_DMA_R, v) == 0
        for v in (-1, 3, 5, 8):
            assert lib.nlam_set_tuning(L.TUNE_WGRAD_DMA_R, v) == -1
    finally:
        lib.nlam_set_tuning(L.TUNE_WGRAD_DMA_R, 0)
