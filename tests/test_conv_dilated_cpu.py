"""Dilated 3 x 3 convolutions (csrc/xpt_conv_dilated.hip) without a GPU: the four C entry points refuse bad arguments before any
launch, through both builds of the library, and the shape half of hip/conv.py usable() admits exactly the dilated layers the
kernels serve."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (cin, cout, d, H, W): the shapes of tests/test_conv_dilated_gpu.py
SHAPES = [(32, 128, 2, 16, 24), (128, 128, 4, 16, 24), (128, 96, 8, 16, 24), (96, 64, 16, 16, 24), (128, 128, 2, 13, 21),
          (20, 8, 4, 9, 11), (64, 64, 16, 40, 8)]


def test_dilated_entry_points_reject_bad_arguments_before_any_launch_through_both_libraries():
    import __graft_entry__ as ge
    from xpt_mde_2021_amd.hip import lib as xl
    if not (os.path.isfile(xl.LIB_PATH) and os.path.isfile(xl.LIB_PATH_F16)):
        ge.build()
    p = ctypes.c_void_p(4096)                                    # never dereferenced: the argument check fails first
    ARG = -3                                                     # XPT_ERR_ARG
    big = 10 ** 9
    for path in (xl.LIB_PATH, xl.LIB_PATH_F16):
        lib = ctypes.CDLL(path)
        fn = {}
        for name in ("xpt_conv2d_dilated_fwd", "xpt_conv2d_dilated_bwd_data", "xpt_conv2d_dilated_bwd_weight_splits",
                     "xpt_conv2d_dilated_bwd_weight_partials"):
            fn[name] = getattr(lib, name)
            fn[name].restype, fn[name].argtypes = xl.SIGNATURES[name]

        def fwd(x=p, w=p, y=p, C=16, N=16, KH=3, KW=3, stride=1, d=2):
            return fn["xpt_conv2d_dilated_fwd"](x, w, p, y, 2, 8, 12, C, C, N, KH, KW, stride, d, N, 0.1, None)

        def dgrad(g=p, w=p, dx=p, C=16, Np=16, KH=3, KW=3, stride=1, d=2):
            return fn["xpt_conv2d_dilated_bwd_data"](g, w, dx, 2, 8, 12, Np, Np, C, KH, KW, stride, d, C, None)

        def splits(C=16, N=16, KH=3, KW=3, stride=1, d=2, B=2, H=8, W=12):
            return fn["xpt_conv2d_dilated_bwd_weight_splits"](B, C, N, KH, KW, stride, d, H, W)

        def wgrad(g=p, x=p, part=p, floats=big, C=16, N=16, KH=3, KW=3, stride=1, d=2):
            return fn["xpt_conv2d_dilated_bwd_weight_partials"](g, x, part, floats, 2, 8, 12, C, C, C, N, N, KH, KW, stride, d, None)

        for call in (fwd, dgrad, splits, wgrad):
            bad = {"dilation 0": call(d=0), "dilation -1": call(d=-1), "5 x 5": call(KH=5, KW=5), "3 x 1": call(KW=1),
                   "1 x 3": call(KH=1), "stride 2": call(stride=2), "stride 0": call(stride=0), "C % 8": call(C=12)}
            assert set(bad.values()) == {ARG}, (path, call.__name__, bad)
        assert fwd(N=12) == ARG and splits(N=12) == ARG and wgrad(N=12) == ARG and dgrad(Np=12) == ARG
        nulls = [fwd(x=None), fwd(w=None), fwd(y=None), dgrad(g=None), dgrad(w=None), dgrad(dx=None), wgrad(g=None),
                 wgrad(x=None), wgrad(part=None)]
        assert set(nulls) == {ARG}, (path, nulls)
        ns = splits()
        assert ns >= 1
        assert wgrad(floats=ns * 16 * 9 * 16 - 1) == ARG, "a partials buffer one float short must be refused"
        for cin, cout, d, H, W in SHAPES:
            cp = (cin + 7) // 8 * 8
            assert splits(C=cp, N=cout, d=d, B=2, H=H, W=W) >= 1, (cin, cout, d, H, W)


def test_usable_geometry_truth_table():
    from xpt_mde_2021_amd.hip import conv as xc
    assert xc.geometry_usable((3, 3), (1, 1), (2, 2), 1, 128) is True
    assert xc.geometry_usable((5, 5), (1, 1), (2, 2), 1, 128) is False
    assert xc.geometry_usable((3, 3), (2, 2), (2, 2), 1, 128) is False
    assert xc.geometry_usable((3, 3), (1, 1), (2, 4), 1, 128) is False       # unequal dilation
    assert xc.geometry_usable((3, 3), (1, 1), (2, 2), 1, 2) is False         # the 2-channel flow head stays on the library
    assert xc.geometry_usable((3, 3), (1, 1), (2, 2), 2, 128) is False       # grouped
    # undilated: as before
    assert xc.geometry_usable((3, 3), (2, 2), (1, 1), 1, 64) and xc.geometry_usable((7, 7), (1, 1), (1, 1), 1, 8)
    assert not xc.geometry_usable((4, 4), (1, 1), (1, 1), 1, 64) and not xc.geometry_usable((3, 3), (1, 1), (1, 1), 1, 196)


def test_library_dilated_switch_restores_the_library_path():
    """XPT_DEBUG_LIBRARY_DILATED=1 is read at import: a fresh child process."""
    code = ("from xpt_mde_2021_amd.hip import conv as xc\n"
            "print(int(xc.geometry_usable((3, 3), (1, 1), (2, 2), 1, 128)), int(xc.geometry_usable((3, 3), (1, 1), (1, 1), 1, 128)))\n")
    for flag, want in (("1", "0 1"), ("0", "1 1")):
        env = dict(os.environ, XPT_DEBUG_LIBRARY_DILATED=flag, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.split("\n")[-2].strip() == want, (flag, out.stdout, out.stderr)
