"""The one seam rule of the kernels (csrc/cube.h) through its three callers, on the field of ``seam_cases``: one sample, one
channel, faces of 2, 3 and 5 cells -- the smallest at which a wrong neighbour, axis, reversal or line shows on each of the
6 x 4 sides -- and a halo as wide as the face (k = 7 at n = 3).

A convolution with the one-hot weight of one tap gives the shifted field itself: every product is by 1.0 or 0.0 and every sum
is with zeros, all values are integers below 2**24, so the result equals the numpy padding of test_host_cube_seams.py bit for
bit.  The SAGE layer with ``W_self = 0`` and ``W_neigh = 1`` gives ``mean5``: a sum of five integers, exact, and one division
by 5, correctly rounded to float32 by the kernel; ``graph_np.sage`` rounds the same quotient to float64 first, which cannot
change the float32 result (53 >= 2 * 24 + 2 bits: double rounding of a quotient is innocuous)."""
import numpy as np
import pytest

import conv_cases
import cyclegan_cases
import graph_cases
import graph_np
import seam_cases

pytestmark = pytest.mark.gpu


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _one_hot(k, taps):
    """torch's ``Conv2d`` weight ``[len(taps), 1, k, k]``: output channel i reads tap ``taps[i]`` = dx * k + dy alone."""
    w = np.zeros((len(taps), 1, k, k), np.float32)
    for i, tap in enumerate(taps):
        w[i, 0, tap // k, tap % k] = 1
    return w


@pytest.mark.parametrize("n", seam_cases.FACES)
def test_cyclegan_conv_reads_the_shifted_field(device, n):
    x, want = seam_cases.field(n).reshape(1, 6, n, n, 1), seam_cases.shifted(n, 3)
    for tap in range(9):
        got = cyclegan_cases.device_layer(device, "regular", 3, True, x, _one_hot(3, [tap]), None)
        assert _same_bits(got[0, ..., 0], want[..., tap]), f"tap ({tap // 3}, {tap % 3})"


def test_cyclegan_conv_with_a_halo_as_wide_as_the_face(device):
    n, k = seam_cases.WIDE[0], 2 * seam_cases.WIDE[1] + 1
    x = seam_cases.field(n).reshape(1, 6, n, n, 1)
    got = cyclegan_cases.device_layer(device, "regular", k, True, x, _one_hot(k, range(k * k)), None)
    assert _same_bits(got[0], seam_cases.shifted(n, k))


@pytest.mark.parametrize("n", seam_cases.FACES)
def test_conv_model_reads_the_shifted_field(device, n):
    """One 3 x 3 layer of nine filters, filter i the one-hot weight of tap i, and the identity as the head."""
    import torch

    from fv3net_amd.conv import ConvModel

    spec = conv_cases.make_spec(np.random.default_rng(0), {"field": 1}, 9, 2, 3, {"taps": 9}, activation="linear", bias=False,
                                unit_inputs=True)
    spec.hidden_kernels[0] = np.ascontiguousarray(_one_hot(3, range(9)).transpose(2, 3, 1, 0))   # [k, k, 1, 9]
    head = spec.outputs[0]
    head.kernel, head.bias = np.eye(9, dtype=np.float32), np.zeros(9, np.float32)
    head.scale, head.center = np.ones(9, np.float32), np.zeros(9, np.float32)
    spec.validate()
    src = torch.from_numpy(seam_cases.field(n).reshape(6, n, n, 1)).to(device)
    got = ConvModel(spec, device).predict({"field": src}, halo="cube", channels_last=True)["taps"].cpu().numpy()
    assert _same_bits(got, seam_cases.shifted(n, 3))


@pytest.mark.parametrize("n", seam_cases.FACES)
def test_graph_sage_means_the_five_cells(device, n):
    from fv3net_amd.graph import SageLayer

    h = seam_cases.field(n).reshape(1, 6, n, n, 1)
    layer = SageLayer(np.zeros((1, 1), np.float32), np.ones((1, 1), np.float32), np.zeros(1, np.float32))
    got = graph_cases.device_layer(device, "sage", h, layer).cpu().numpy()
    assert _same_bits(got, graph_np.sage(h, layer.w_self, layer.w_neigh, layer.bias).astype(np.float32))
