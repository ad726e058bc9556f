"""The exact-integer method of tests/test_conv_exact_gpu.py has teeth, shown without a GPU:

* the fp64 reference of EVERY case of the GPU file stays exactly representable in both 16-bit formats (the condition under which
  "any correct kernel gives the same values" holds);
* slips a kernel could commit -- a boundary column of one weight-gradient tap dropped (everywhere, or in one row of tiles), one
  (tap, 8-channel group) operand load skipped on the ragged right edge of the forward, one tile of the weight gradient reduced
  twice -- each break equality by at least one unit in every touched element.  For the SAME slips the "max error as a fraction
  of the largest magnitude" of the tolerance tests (tests/test_conv_igemm_gpu.py: 6e-3 forward, 1.5e-2 gradients) is measured
  with that test's random-normal operands on its own geometry: printed (pytest -s) and recorded in DESIGN.md "Exact-integer
  parity" -- most come out 2 - 3 x over the bar, the one-tile-row column under it."""
import pytest
import torch

from tests import exact_ops as ex
from tests import test_conv_exact_gpu as gpu_cases
from tests.exact_ops import ConvCase

FWD_BAR, GRAD_BAR = 6e-3, 1.5e-2            # tests/test_conv_igemm_gpu.py

DEEP = gpu_cases.PRODUCT[0]                 # 1056 -> 256, 3 x 3, nearest-2x, 4 x 13: the longest reduction (K = 9504)
WIDE = gpu_cases.PRODUCT[14]                # 17 -> 16, 3 x 3: the full-resolution layer, shrunk to 25 x 49
# the geometry the tolerance tests run these two layers at (batch 2)
DEEP_FULL = ConvCase(1056, 256, 3, 1, 4, 13, "nearest")
WIDE_FULL = ConvCase(17, 16, 3, 1, 128, 416)


@pytest.mark.parametrize("case", gpu_cases.ALL_CONV_CASES, ids=str)
def test_conv_reference_is_exact_in_both_16_bit_formats(case):
    ref = ex.conv_reference(case)
    for dtype in ex.FORMATS:
        ex.check_conv_reference(case, ref, dtype)
    # not vacuous: the operands are live and most outputs are non-zero on both sides of the activation's kink
    assert float((ref["y"] != 0).double().mean()) > 0.5 and bool((ref["y"] < 0).any()) and bool((ref["y"] > 0).any())
    assert float(ref["dw"].abs().max()) >= 4 and float(ref["dx"].abs().max()) >= 4
    if case.ups == "bilinear":
        assert bool((ref["xu"] % 16 != 0).any()), "the interpolated operand never mixes two pixels"


def test_sink_cases_are_covered_by_the_exactness_check():
    assert set(gpu_cases.SINK) <= set(gpu_cases.ALL_CONV_CASES)


@pytest.mark.parametrize("C,H,W", gpu_cases.HEADS)
def test_head_reference_is_exact(C, H, W):
    ref = ex.head_reference(C, H, W)
    for dtype in ex.FORMATS:
        ex.require_fits({"x": ref["x"], "dx": ref["dx"]}, dtype, f"head {C}")


@pytest.mark.parametrize("shape", gpu_cases.DW_SHAPES)
@pytest.mark.parametrize("k,stride", [(3, 1), (5, 1), (7, 1), (3, 2), (5, 2), (7, 2)])
@pytest.mark.parametrize("relu_in", [False, True])
def test_depthwise_reference_is_exact(k, stride, shape, relu_in):
    ref = ex.depthwise_reference(k, stride, shape, relu_in)                 # (asserts both formats itself)
    assert float(ref["y"].abs().max()) >= 3 and float(ref["dw"].abs().max()) >= 3


def test_fits_and_tri():
    gen = torch.Generator().manual_seed(1)
    t = ex.tri((64, 64), 0.25, gen, 16)
    assert set(t.unique().tolist()) == {-16.0, 0.0, 16.0} and 0.15 < float((t != 0).double().mean()) < 0.35
    assert ex.fits(torch.tensor([256.0, 127.5, -0.0]), torch.bfloat16) and not ex.fits(torch.tensor([257.0]), torch.bfloat16)
    assert ex.fits(torch.tensor([2047.0]), torch.float16) and not ex.fits(torch.tensor([2049.0, 1e5]), torch.float16)
    n, first = ex.mismatches(torch.tensor([0.0, 1.0, 2.0]), torch.tensor([-0.0, 1.0, 3.0]))
    assert n == 1 and first == [((2,), 2.0, 3.0)]
    got, want = torch.zeros(2, 2, 1, 1), torch.zeros(2, 2, 1, 1)
    got[1, 0, 0, 0], want[1, 0, 0, 0] = 5.0, 4.0
    with pytest.raises(AssertionError, match=r"1 of 4 elements differ -- \(cout=1, cin=0, kh=0, kw=0\): got 5, want 4"):
        ex.assert_equal(got, want, "dW", ex.DW_AXES)


# ------------------------------------------------------------------------------------------------ corruptions
def _corruptions(ref, case):
    """name -> (which result, the corrupted value): centre tap / first channel group, so that every dropped term is in range."""
    return {
        "dW boundary column dropped": ("dw", ex.drop_dw_boundary_column(ref, case, 1, 1)),
        "dW boundary column dropped in one row of tiles": ("dw", ex.drop_dw_boundary_column(ref, case, 1, 1, rows=8)),
        "y tap x 8-channel group dropped at the ragged edge": ("y", ex.drop_y_tap_group(ref, case, 1, 1, 8)),
        "dW tile reduced twice": ("dw", ex.duplicate_dw_tile(ref, case)),
    }


@pytest.fixture(scope="module")
def floors():
    """The tolerance metric of each corruption on the tolerance tests' own operands and geometry (computed once)."""
    out = {}
    for name, full in (("deep", DEEP_FULL), ("wide", WIDE_FULL)):
        case, ref = ex.normal_recipe(full)
        for what, (key, bad) in _corruptions(ref, case).items():
            out[name, what] = (key, ex.largest_magnitude_error(bad, ref[key]))
    return out


@pytest.mark.parametrize("name,case", [("deep", DEEP), ("wide", WIDE)])
def test_exact_comparison_catches_what_the_tolerance_metric_cannot(floors, name, case):
    ref = ex.conv_reference(case)
    for what, (key, bad) in _corruptions(ref, case).items():
        n, _ = ex.mismatches(bad, ref[key])
        assert n > 0, f"{case}: {what}: the corruption is a no-op on the exact operands"
        with pytest.raises(AssertionError, match="elements differ"):
            ex.assert_equal(bad, ref[key], what, ex.DW_AXES if key == "dw" else ex.MAP_AXES)
        # every wrong element is off by at least one unit of the integer grid (1/2 below the kink of slope 0.5)
        step = float((bad - ref[key]).abs()[bad != ref[key]].min())
        assert step >= (0.5 if key == "y" else 1.0)
        _, floor = floors[name, what]
        bar = FWD_BAR if key == "y" else GRAD_BAR
        print(f"[floor] {name:4s} {what:52s}: {n:6d} elements differ exactly; tolerance metric {floor:.2e} (bar {bar:.1e}) "
              f"-> {'UNDER the bar: invisible' if floor < bar else 'over the bar'}")


def test_where_the_tolerance_metric_stops_seeing_a_dropped_weight_gradient_column(floors):
    """At the tolerance tests' full-resolution shape (2 x 128 x 416, 106 496 terms per dW element) the metric takes the LARGEST
    error over the 272 elements of the tap, about three standard deviations: a whole dropped boundary column (256 terms) measures
    4.0e-2, over the 1.5e-2 bar -- the tolerance tests do see that one, by a factor of 2.7.  The same slip confined to one row of
    8 x 16 tiles (16 terms: what a ragged-tile bug in one tile row commits) measures 1.1e-2: invisible.  Exact comparison fails
    on both (test above)."""
    key, column = floors["wide", "dW boundary column dropped"]
    _, tile_row = floors["wide", "dW boundary column dropped in one row of tiles"]
    print(f"[floor] whole column {column:.2e}, one row of tiles {tile_row:.2e} (bar {GRAD_BAR:.1e})")
    assert key == "dw" and 0 < tile_row < GRAD_BAR < column, (tile_row, column)
