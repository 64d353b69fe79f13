"""``fv3hip_cyclegan_conv_context`` on its own: the convolution with context channels, bit for bit against torch's ``conv2d`` on
the padded channel-wise concatenation ``[T(src) | ctx_cell | ctx_uniform]``.

As in ``test_gpu_cyclegan_layers.py`` the data is exact: inputs, context values and biases are small integers, weights in
{-1, 0, 1}, ``rstd`` a power of two, so every partial sum is an integer below 2**24 and the float32 result does not depend on
the order of the sum.  Sizes: faces of 3 (the halo as wide as the face allows for k = 3), 6 and, for k = 7, 8 cells; one sample
(6 * 36 = 216 rows end inside the second 128-row block) and three; ``c_in`` 16 and 32 (the vector loader, one and two chunks),
20 and 3 (the scalar loader); context rows 27, 18 and 45 for k = 3, 125 for k = 5 and 147 for k = 7, all ending inside a
16-row chunk; ``c_out`` 8, 40 (two MFMA tiles, the second partial) and 72 (two channel groups).
"""
import numpy as np
import pytest
import torch

import cyclegan_cases as cc
import fmr_cases as fc

pytestmark = pytest.mark.gpu

CONTEXTS = ((3, 0), (0, 2), (3, 2))
C_IN, C_OUT = (16, 32, 20, 3), (8, 40, 72)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def exact_case(rng, S, n, k, c_in, c_cell, c_uni, c_out):
    x = rng.integers(-4, 5, (S, 6, n, n, c_in)).astype(np.float32)
    w = rng.integers(-1, 2, (c_out, c_in, k, k)).astype(np.float32)
    w_ctx = rng.integers(-1, 2, (c_out, c_cell + c_uni, k, k)).astype(np.float32) if c_cell + c_uni else None
    bias = rng.integers(-3, 4, c_out).astype(np.float32)
    cell = rng.integers(-4, 5, (6, n, n, c_cell)).astype(np.float32) if c_cell else None
    uni = rng.integers(-4, 5, c_uni).astype(np.float32) if c_uni else None
    return x, w, w_ctx, bias, cell, uni


@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
@pytest.mark.parametrize("k,n", [(3, 3), (3, 6), (5, 6), (7, 8)], ids=["k3-n3", "k3-n6", "k5-n6", "k7-n8"])
def test_context_convolution_is_exact(device, k, n, halo):
    """Every (c_in, context, c_out) triple; one sample where the three indices sum to an even number, three where to an odd one."""
    rng = np.random.default_rng(100 * n + k)
    for i, c_in in enumerate(C_IN):
        for j, (c_cell, c_uni) in enumerate(CONTEXTS):
            for l, c_out in enumerate(C_OUT):
                S = 3 if (i + j + l) % 2 else 1
                x, w, w_ctx, bias, cell, uni = exact_case(rng, S, n, k, c_in, c_cell, c_uni, c_out)
                want = fc.torch_context_layer(k, halo, x, w, w_ctx, bias, cell, uni)
                got = fc.device_context_layer(device, k, halo, x, w, w_ctx, bias, cell, uni)
                assert got.shape == want.shape
                assert np.array_equal(bits(got), bits(want)), (k, n, S, c_in, c_cell, c_uni, c_out, int(np.sum(got != want)))


@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
def test_the_loader_transform_leaves_the_context_alone(device, halo):
    """A pending ``relu((v - mean) * rstd + bias)`` on the source: the context values -- negative ones among them -- go in as
    they are.  Through the vector loader at channel offset 4 and the scalar loader at offset 2 and with 20 channels."""
    rng = np.random.default_rng(5)
    S, n, k, c_out = 3, 6, 3, 40
    for c_in, src_off in ((16, 0), (16, 4), (16, 2), (20, 0)):
        x, w, w_ctx, bias, cell, uni = exact_case(rng, S, n, k, c_in, 3, 2, c_out)
        cell[0, 0, 0, :], uni[:] = -4, (-3, 2)
        mean = rng.integers(-3, 4, (S, 6, c_in)).astype(np.float32)
        rstd = (2.0 ** rng.integers(-1, 3, (S, 6, c_in))).astype(np.float32)
        cell_bias = rng.integers(-2, 3, (6, n, n, c_in)).astype(np.float32)
        for transform in ((mean, rstd, cell_bias, True), (mean, rstd, None, False)):
            want = fc.torch_context_layer(k, halo, x, w, w_ctx, bias, cell, uni, transform=transform)
            got = fc.device_context_layer(device, k, halo, x, w, w_ctx, bias, cell, uni, transform=transform, src_off=src_off,
                                          src_width=c_in + 8)
            assert np.array_equal(bits(got), bits(want)), (c_in, src_off, transform[3], int(np.sum(got != want)))
        relu_on_all = fc.torch_context_layer(k, halo, np.concatenate([x, np.broadcast_to(cell, (S,) + cell.shape),
                                                                      np.broadcast_to(uni, (S, 6, n, n, 2))], axis=-1),
                                             np.concatenate([w, w_ctx], axis=1), None, bias,
                                             transform=(np.zeros((S, 6, c_in + 5), np.float32), np.ones((S, 6, c_in + 5), np.float32), None, True))
        plain = fc.device_context_layer(device, k, halo, x, w, w_ctx, bias, cell, uni, transform=(np.zeros_like(mean), np.ones_like(rstd), None, True))
        assert not np.array_equal(plain, relu_on_all), "the case cannot tell a ReLU on the context from none"


def test_no_context_is_the_plain_convolution(device):
    """``c_cell = c_uni = 0``: the same bits as ``fv3hip_cyclegan_conv`` on data that is not exact."""
    rng = np.random.default_rng(6)
    for k, n, c_in, c_out in ((3, 6, 16, 40), (7, 8, 3, 8), (5, 6, 20, 72)):
        x = rng.normal(0, 1, (3, 6, n, n, c_in)).astype(np.float32)
        w = rng.normal(0, 0.2, (c_out, c_in, k, k)).astype(np.float32)
        bias = rng.normal(0, 1, c_out).astype(np.float32)
        for halo in (True, False):
            got = fc.device_context_layer(device, k, halo, x, w, None, bias)
            assert np.array_equal(bits(got), bits(cc.device_layer(device, "regular", k, halo, x, w, bias))), (k, n, c_in, c_out, halo)


def test_a_uniform_context_differs_from_a_bias_exactly_at_the_corner_windows(device):
    """With cube halos the uniform value is present on every halo cell but the corners, which are zero: folding it into the
    bias is wrong at the cells whose window touches a corner -- for k = 3 the four corner cells of every face -- and only there.
    With zero padding every border cell differs."""
    rng = np.random.default_rng(7)
    S, n, k, c_in, c_out = 1, 6, 3, 3, 8
    x, w, _, bias, _, _ = exact_case(rng, S, n, k, c_in, 0, 2, c_out)
    uni, w_ctx = np.array([2, 3], np.float32), np.ones((c_out, 2, k, k), np.float32)
    folded = bias + np.einsum("c,ocxy->o", uni, w_ctx)
    corner, border = np.zeros((n, n), bool), np.ones((n, n), bool)
    corner[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    border[1:-1, 1:-1] = False
    for halo, where in ((True, corner), (False, border)):
        got = fc.device_context_layer(device, k, halo, x, w, w_ctx, bias, None, uni)
        assert np.array_equal(bits(got), bits(fc.torch_context_layer(k, halo, x, w, w_ctx, bias, None, uni)))
        as_bias = cc.device_layer(device, "regular", k, halo, x, w, folded)
        differs = np.any(got != as_bias, axis=-1)
        assert np.array_equal(differs, np.broadcast_to(where, differs.shape)), halo
        if halo:     # one tap of the nine is missing at a corner cell: 2 + 3 less in every channel
            assert np.all((as_bias - got)[differs] == 5.0)


def test_refusals(device):
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)
    src, dst, half, double = z(1, 6, 4, 4, 4), z(1, 6, 4, 4, 4), z(1, 6, 2, 2, 4), z(1, 6, 8, 8, 4)
    w, w_ctx, cell, uni = z(4, 4, 4, 4), z(4, 4, 5, 4), z(6, 4, 4, 3), z(2)

    def conv(kind=_lib.CYCLEGAN_CONV_REGULAR, k=3, out=dst, ctx_cell=cell, c_cell=3, ctx_uniform=uni, c_uni=2, weights=w_ctx):
        p = lambda t: None if t is None else t.data_ptr()
        _lib.call_on(device, "fv3hip_cyclegan_conv_context", src.data_ptr(), 4, 0, 0, None, None, None, 0, w.data_ptr(), None, None,
                     out.data_ptr(), 4, 0, 0, 1, 4, 4, 4, kind, k, _lib.CYCLEGAN_HALO_CUBE, p(ctx_cell), c_cell, p(ctx_uniform), c_uni,
                     p(weights), _stream(device))

    conv()
    for kind, out in ((_lib.CYCLEGAN_CONV_STRIDED, half), (_lib.CYCLEGAN_CONV_TRANSPOSED, double)):
        with pytest.raises(_lib.Fv3HipError, match="context channels are built for the regular convolution") as e:
            conv(kind, 4, out)
        assert e.value.code == _lib.EUNSUPPORTED
        conv(kind, 4, out, None, 0, None, 0, None)                       # without a context they are the plain layers
    for kwargs, match in ((dict(ctx_cell=None), "ctx_cell is null with c_cell = 3"), (dict(c_cell=0), "ctx_cell is given with c_cell = 0"),
                          (dict(ctx_uniform=None), "ctx_uniform is null with c_uni = 2"), (dict(c_uni=0), "ctx_uniform is given with c_uni = 0"),
                          (dict(weights=None), "w_ctx is null with 5 context channels"), (dict(c_cell=-1), "c_cell and c_uni must be in"),
                          (dict(ctx_cell=None, c_cell=0, ctx_uniform=None, c_uni=0), "w_ctx is given with 0 context channels"),
                          (dict(k=4), "k = 4")):
        with pytest.raises(_lib.Fv3HipError, match=match):
            conv(**kwargs)
    torch.cuda.synchronize(device)
