"""The plan-forcing fixture of the dense-convolution tests (tests/test_conv_igemm_gpu.py, tests/test_conv_exact_gpu.py): a plain
module both import, so the fixture is visible in each without a conftest entry."""
import pytest

# 0: automatic choice; 901 / 902: the LDS-staged kernel (32 / 64 output channels per workgroup) forced on EVERY layer
# shape (ragged tiles, residue classes, quad fold, 8-channel inputs); 110: the direct 32 x 32 kernel forced likewise;
# 911 / 912: the halo-tile kernel (32 / 64 output channels per workgroup) on every stride-1 layer, forward and data gradient
# 5001 / 5002 / 5008 / 5016: the split-K tile kernels (1 / 2 / 8 / 16 slices of the reduction axis) on every stride-1 layer
# 6001 / 6003 / 6102: the persistent weight-stationary kernels, 1 / 3 workgroups per CU (6102: generic kernel only, 2 per CU), on
# every 3 x 3 stride-1 layer that fits
PLANS = [0, 901, 902, 110, 911, 912, 5001, 5002, 5008, 5016, 5104, 6001, 6003, 6102, 7002]


@pytest.fixture
def conv_plan():
    """Forces one kernel instantiation for forward + data gradient (xpt_conv2d_tune), restores the automatic choice."""
    from xpt_mde_2021_amd.hip import lib as _lib
    lib = _lib.load()

    def set_plan(plan):
        # xpt_conv2d_bwd_weight_tune(-1000, n): the specialised persistent weight-gradient kernel (conv_wgrad_fast_kernel) serves the
        # 3 x 3 (stride 1 / 2, nearest-2x) and 5 x 5 stride-2 layers from n tiles on.  Every plan: from 1 tile on, the product's
        # setting; 7002: as plan 0 with n = 2 (one-tile layers take the general kernel)
        _lib.check(lib.xpt_conv2d_bwd_weight_tune(-1000, 2 if plan == 7002 else 1), "wgrad tune")
        if plan == 7002:
            plan = 0
        if plan == 0:             # the product's automatic choice among ALL kernel families
            _lib.check(lib.xpt_conv2d_tune(0), "tune")
            _lib.check(lib.xpt_conv2d_splitk_tune(1, 0, 1024, 8192), "splitk tune")
            _lib.check(lib.xpt_conv2d_stream_tune(1, 512, 3, 80), "stream tune")
        elif plan >= 6000:        # 6000 + w: the persistent weight-stationary kernels (csrc/xpt_conv_stream.hip), w workgroups per CU,
            _lib.check(lib.xpt_conv2d_tune(0), "tune")                      # on EVERY 3 x 3 stride-1 layer they can hold
            _lib.check(lib.xpt_conv2d_splitk_tune(0, 0, 0, 0), "splitk tune")
            # (6100 + w: the generic kernel for every shape; 6000 + w: the specialised instantiations where they exist)
            _lib.check(lib.xpt_conv2d_stream_tune(2 if plan >= 6100 else 1, 1, plan % 100, 150), "stream tune")
        elif plan >= 5000:        # 5000 + n: the split-K kernels (csrc/xpt_conv_splitk.hip) with n slices on EVERY stride-1 layer
            _lib.check(lib.xpt_conv2d_tune(0), "tune")
            _lib.check(lib.xpt_conv2d_stream_tune(0, 0, 0, 0), "stream tune")
            # (5100 + n: four waves per workgroup instead of eight on the 128-channel tile)
            _lib.check(lib.xpt_conv2d_splitk_tune(4 if plan >= 5100 else 8, plan % 100, 1, 1 << 30), "splitk tune")
        else:                     # the kernels of csrc/xpt_conv.hip, one instantiation forced
            _lib.check(lib.xpt_conv2d_splitk_tune(0, 0, 0, 0), "splitk tune")
            _lib.check(lib.xpt_conv2d_stream_tune(0, 0, 0, 0), "stream tune")
            _lib.check(lib.xpt_conv2d_tune(plan), "tune")

    yield set_plan
    lib.xpt_conv2d_bwd_weight_tune(-1000, 1)
    lib.xpt_conv2d_tune(0)
    lib.xpt_conv2d_splitk_tune(8, 0, 1024, 8192)
    lib.xpt_conv2d_stream_tune(1, 512, 3, 80)
