"""Host-side pieces of the fp32 training mode on the matrix cores (`fp32_train_conv`): flag validation, bindings, and the K-split
plan of the weight gradient (a pure host function).  No GPU needed."""
import ctypes

import pytest


def test_fp32_train_conv_flag_is_validated():
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    from upflow_pytorch_amd.model import pwc_modules
    conf = UPFlow_net.config()
    assert conf.fp32_train_conv == 'miopen'              # the default keeps today's behaviour
    conf.update({'fp32_train_conv': 'hip_x3'}, verbose=False)
    assert conf().conf.fp32_train_conv == 'hip_x3'
    conf.update({'fp32_train_conv': 'cudnn'}, verbose=False)
    with pytest.raises(ValueError):
        conf()
    with pytest.raises(ValueError):
        pwc_modules.fp32_train_conv_mode('hip_x4')
    assert pwc_modules.FP32_TRAIN_CONV[0] == 'miopen'
    with pwc_modules.fp32_train_conv_mode('hip_x3'):
        assert pwc_modules.FP32_TRAIN_CONV[0] == 'hip_x3'
    assert pwc_modules.FP32_TRAIN_CONV[0] == 'miopen'


def test_x3_train_entries_are_bound_and_exported():
    from upflow_pytorch_amd import _lib, ops
    names = ('upf_act_grad_x3', 'upf_conv_x3_pack_weights_dgrad', 'upf_conv_x3_dgrad', 'upf_conv_x3_wgrad', 'upf_conv_x3_wgrad_workspace_bytes')
    for n in names:
        assert n in _lib.SIGNATURES
        assert getattr(_lib.lib(), n) is not None
    header = open(__import__('os').path.join(__import__('os').path.dirname(_lib._PKG), 'include', 'upflow_hip.h')).read()
    for n in names:
        assert n + '(' in header
    assert hasattr(ops, 'ConvX3TrainFunction') and callable(ops.conv_x3_train)


def test_x3_wgrad_workspace_query():
    """Partial blocks: at most 64 MB, at least one slice per level, an error for what the kernel does not take; tiny levels are accepted
    (no W >= 8 or even-size restriction)."""
    from upflow_pytorch_amd import _lib
    L = _lib.lib()

    def levels(*shapes):
        arr = (_lib.WgradLevel * len(shapes))()
        for a, (B, H, W) in zip(arr, shapes):
            a.x, a.grad_pre, a.B, a.H, a.W = 16, 16, B, H, W         # (never dereferenced by the query)
        return arr

    def query(arr, n, Cin, Cout, k, d, s):
        out = ctypes.c_longlong(-1)
        rc = L.upf_conv_x3_wgrad_workspace_bytes(arr, n, Cin, Cout, k, d, s, ctypes.byref(out))
        return out.value if rc == 0 else -1
    one = query(levels((8, 64, 208)), 1, 565, 128, 3, 1, 1)
    per_slice = 565 * 128 * 9 * 4
    assert one > 0 and one % per_slice == 0 and one <= (64 << 20) + per_slice
    tiny = query(levels((2, 2, 7), (2, 4, 13), (2, 1, 1)), 3, 35, 2, 3, 1, 1)
    assert tiny == 3 * 35 * 2 * 9 * 4                     # one slice per level
    assert query(levels((1, 13, 27)), 1, 32, 64, 3, 1, 2) > 0       # stride 2, odd sizes
    assert query(levels((1, 13, 27)), 1, 32, 64, 3, 2, 2) == -1     # stride 2 with dilation
    assert query(levels((1, 13, 27)), 1, 32, 64, 5, 1, 1) == -1
    assert query(levels(*[(1, 4, 4)] * 7), 7, 32, 64, 3, 1, 1) == -1
    assert query(None, 1, 32, 64, 3, 1, 1) == -1
    assert ctypes.sizeof(_lib.WgradLevel) == 48
