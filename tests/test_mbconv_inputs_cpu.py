"""The inputs tests/test_mbconv_gpu.py draws, checked without a GPU from their fp64 reference: y has sizeable shares at 0, inside
(0, 6) and at 6, both clamps of act_in act on x, and the share of dy that is zeroed near the kinks (where a 16-bit store of y may
land on the other side of the mask) stays at or below 5 %."""
import pytest

from tests.test_mbconv_gpu import FORMATS, SHAPES, case


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("act_in", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_input_distribution_exercises_every_branch_and_zeroes_at_most_5_percent(shape, act_in, fmt):
    c = case(shape, act_in, fmt)
    print(f"{shape} act_in={act_in} {fmt}: shares {c['shares']}, zeroed {c['zeroed']:.4f}")
    assert min(c["shares"]) >= 0.05, c["shares"]
    assert c["zeroed"] <= 0.05, c["zeroed"]
    assert abs(sum(c["shares"]) - 1.0) < 1e-12
    if act_in:
        assert float((c["x"] < 0).double().mean()) > 0.1 and float((c["x"] > 6).double().mean()) > 0.05
    assert float((c["dy"] == 0).double().mean()) >= c["zeroed"]
