"""CPU tests that go with tests/test_gpu_sk_and_small_kernels.py: the reference the SK kernel checks differentiate is the oracle's own
code, and the argument checks of the small launchers answer before anything is launched."""
import ctypes

import pytest
import torch

from simclr_amd import _lib


@pytest.mark.parametrize('strides', [1, 2])
def test_factored_sk_functions_reproduce_sk_conv2d_bitwise(strides):
    """oracle/model_torch.py sk_split / sk_pooled / sk_mix_weights / sk_mix, fed with the intermediate tensors of a full
    Builder.sk_conv2d call (captured at the layers around them), give its pooled feature and its output bit for bit."""
    from oracle.model_torch import Builder, Config, sk_mix, sk_mix_weights, sk_pooled, sk_split
    f = 64
    for dtype in (torch.float32, torch.float64):
        b = Builder(Config(sk_ratio=0.0625), seed=3, randomize_bn=True, dtype=dtype)
        bn_out, conv_in, conv_out = [], [], []
        bn, conv = b.batch_norm_relu, b.plain_conv1x1

        def rec_bn(x, *a, **k):
            y = bn(x, *a, **k)
            bn_out.append(y)
            return y

        def rec_conv(x, filters):
            y = conv(x, filters)
            conv_in.append(x)
            conv_out.append(y)
            return y
        b.batch_norm_relu, b.plain_conv1x1 = rec_bn, rec_conv
        x = torch.randn(3, 64, 9, 9, generator=torch.Generator().manual_seed(5), dtype=dtype)
        out = b.sk_conv2d(x, f, strides)
        assert len(bn_out) == 2 and len(conv_in) == 2
        a, g, logits = bn_out[0], conv_in[0], conv_out[1]
        oh = (9 + strides - 1) // strides
        assert tuple(a.shape) == (3, 2 * f, oh, oh) and tuple(logits.shape) == (3, 2 * f, 1, 1)
        streams = sk_split(a, f)
        assert torch.equal(streams[0], a[:, :f]) and torch.equal(streams[1], a[:, f:])
        assert torch.equal(sk_pooled(streams), g)
        mix = sk_mix_weights(logits, f)
        assert torch.equal(sk_mix(streams, mix), out)


def test_small_launchers_check_their_arguments():
    """simclr_colsum, simclr_cast, simclr_axpy_f32 and simclr_l2_loss_f32: an empty tensor is a successful no-op, bad arguments return
    status 1 with a message -- decided on the host, before any launch (so this runs without a GPU)."""
    L = _lib.lib()
    dll = L._dll
    one = ctypes.c_void_p(16)          # never dereferenced: every call below returns before it launches
    assert L.cast(None, None, 0, _lib.DT_F32, _lib.DT_BF16, None) == 0
    assert L.axpy_f32(1.0, None, None, 0, None) == 0
    assert L.l2_loss_f32(None, 0, None, None) == 0
    for rows, C, cvalid in [(0, 16, 10), (-1, 16, 10), (4, 16, 0), (4, 16, 17)]:
        assert dll.simclr_colsum(one, rows, C, cvalid, one, 0, _lib.DT_F32, None) == 1
        assert 'colsum: bad shape' in L.last_error() and 'cvalid=%d' % cvalid in L.last_error()
    with pytest.raises(_lib.SimclrHipError, match='colsum: null argument'):
        L.colsum(None, 4, 16, 10, None, 0, _lib.DT_F32, None)
    with pytest.raises(_lib.SimclrHipError, match='cast: n=-1 must not be negative'):
        L.cast(one, one, -1, _lib.DT_F32, _lib.DT_BF16, None)
    with pytest.raises(_lib.SimclrHipError, match='cast: dtypes must be f32 / bf16'):
        L.cast(one, one, 4, _lib.DT_F32, 7, None)
    with pytest.raises(_lib.SimclrHipError, match='cast: null argument'):
        L.cast(None, one, 4, _lib.DT_F32, _lib.DT_BF16, None)
    with pytest.raises(_lib.SimclrHipError, match='axpy_f32: n=-5 must not be negative'):
        L.axpy_f32(1.0, one, one, -5, None)
    with pytest.raises(_lib.SimclrHipError, match='axpy_f32: null argument'):
        L.axpy_f32(1.0, None, one, 4, None)
    with pytest.raises(_lib.SimclrHipError, match='l2_loss_f32: n=-1 must not be negative'):
        L.l2_loss_f32(one, -1, one, None)
    with pytest.raises(_lib.SimclrHipError, match='l2_loss_f32: null argument'):
        L.l2_loss_f32(one, 4, None, None)
