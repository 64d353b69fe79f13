"""The layer kernels of the graph autoregressor (``fv3hip_graph_sage`` / ``_pool2`` / ``_up2``) at their edges, against the
float64 oracle ``graph_np`` with the project's per-level gate (``tolerances.assert_close_per_level``, rel 1e-5, ``cpu32`` = the
plain-torch twin in float32 on the CPU).

The kernel's borders: the spatial tile is 16 x 16 cells (n = 15, 16, 17 and 34: below, at and above one tile, above two), a K
chunk is 8 source channels for SAGE and 16 for the transposed convolution (c_in = 8, 9 / 16, 17), an N tile is 32 channels and
a block holds two (c_out = 31, 32, 33, 64, 65).

Float32 twin against the float64 oracle, worst per-level ratio, measured on the CPU before the cases were fixed (the gate is
1e-5, cases were to be kept up to 5e-6): SAGE, all 42 (c_in, c_out) pairs at n = 6: 7.4e-8 ... 4.9e-7; SAGE 9 -> 33 at the
tile borders 1.8e-7 ... 2.4e-7; the SAGE slice cases 2.1e-7 ... 3.8e-7; pool2 5.3e-8 ... 1.1e-7; up2 4.0e-8 ... 3.3e-7.  No case
had to be dropped.
"""
import numpy as np
import pytest
import torch

import graph_cases
import graph_np
import tolerances

pytestmark = pytest.mark.gpu

C_IN = (1, 3, 8, 9, 33, 65)
C_OUT = (1, 4, 31, 32, 33, 64, 65)


def _flat(a):
    return np.asarray(a).reshape(-1, a.shape[-1])


def _gate(got, truth, cpu32, name):
    return tolerances.assert_close_per_level(_flat(got), _flat(truth), cpu32=_flat(cpu32), name=name, rel=1e-5)


@pytest.mark.parametrize("nx", [2, 3, 15, 16, 17, 34])
def test_seam_map_is_exact(device, nx):
    """W_self = 0, W_neigh = 5 I: every output is the exact sum of the cell's id and its four neighbours' ids."""
    from fv3net_amd.graph import SageLayer

    ids = np.arange(6 * nx * nx, dtype=np.float32).reshape(1, 6, nx, nx, 1)
    assert ids.max() < 2 ** 22
    h = np.concatenate([ids, ids[:, ::-1] + 1], axis=-1)   # a second channel with other ids
    layer = SageLayer(np.zeros((2, 2), np.float32), 5 * np.eye(2, dtype=np.float32), np.zeros(2, np.float32))
    got = graph_cases.device_layer(device, "sage", h, layer).cpu().numpy()
    want = graph_np.gather5(h.astype(np.float64)).sum(axis=-2)
    assert np.array_equal(graph_np.sage(h, layer.w_self, layer.w_neigh, layer.bias), want)   # (x / 5) * 5 is exact in float64
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("c_in", C_IN)
def test_sage_channel_borders(device, c_in):
    rng = np.random.default_rng(c_in)
    for k, c_out in enumerate(C_OUT):
        S, act = (1, 3)[k % 2], ("relu", "tanh", "linear")[k % 3]
        layer = graph_cases.sage_layer(rng, c_in, c_out)
        h = graph_cases.make_state(rng, S, 6, c_in)
        got = graph_cases.device_layer(device, "sage", h, layer, act).cpu().numpy()
        _gate(got, graph_np.sage(h, layer.w_self, layer.w_neigh, layer.bias, act), graph_cases.twin_sage(layer, h, act),
              f"sage {c_in}->{c_out} S={S} {act}")


@pytest.mark.parametrize("nx", [2, 15, 16, 17, 34])
def test_sage_tile_borders(device, nx):
    rng = np.random.default_rng(nx)
    layer = graph_cases.sage_layer(rng, 9, 33)
    h = graph_cases.make_state(rng, 3 if nx < 34 else 1, nx, 9)
    got = graph_cases.device_layer(device, "sage", h, layer, "relu").cpu().numpy()
    _gate(got, graph_np.sage(h, layer.w_self, layer.w_neigh, layer.bias, "relu"), graph_cases.twin_sage(layer, h, "relu"), f"sage n={nx}")


def test_sage_without_bias(device):
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    rng = np.random.default_rng(8)
    layer = graph_cases.sage_layer(rng, 5, 7, bias=False)
    h = graph_cases.make_state(rng, 2, 4, 5)
    src, dst = torch.from_numpy(h).to(device), torch.empty((2, 6, 4, 4, 7), dtype=torch.float32, device=device)
    ws, wn = torch.from_numpy(layer.w_self).to(device), torch.from_numpy(layer.w_neigh).to(device)
    _lib.call_on(device, "fv3hip_graph_sage", src.data_ptr(), 5, 0, 0, ws.data_ptr(), wn.data_ptr(), None, dst.data_ptr(), 7, 0, 0, 2, 4, 5,
                 7, _lib.ACT_LINEAR, _stream(device))
    _gate(dst.cpu().numpy(), graph_np.sage(h, layer.w_self, layer.w_neigh, None), graph_cases.twin_sage(layer, h), "sage, null bias")


@pytest.mark.parametrize("kind, c_in, c_out, src_off, dst_off", [("sage", 9, 33, 0, 5), ("sage", 8, 4, 3, 0), ("sage", 33, 65, 7, 31),
                                                                  ("pool2", 6, 6, 2, 3), ("up2", 17, 9, 1, 9)])
def test_channel_slices_of_wider_buffers(device, kind, c_in, c_out, src_off, dst_off):
    """The source is a channel slice of a NaN-filled buffer, the destination a slice of a sentinel-filled one, two channels
    wider on the right: what lies outside the destination slice is bit-unchanged, and no NaN from outside the source slice
    is read."""
    rng = np.random.default_rng(c_in + c_out)
    n, S = 6, 2
    h = graph_cases.make_state(rng, S, n, c_in)
    n_out = {"sage": n, "pool2": n // 2, "up2": 2 * n}[kind]
    ld = dst_off + c_out + 2
    sentinel = rng.normal(0, 1, (S, 6, n_out, n_out, ld)).astype(np.float32)
    dst = torch.from_numpy(sentinel).to(device)
    if kind == "sage":
        layer = graph_cases.sage_layer(rng, c_in, c_out)
        truth, cpu32 = graph_np.sage(h, layer.w_self, layer.w_neigh, layer.bias, "tanh"), graph_cases.twin_sage(layer, h, "tanh")
    elif kind == "pool2":
        layer, truth = None, graph_np.pool2(h)
        cpu32 = h.reshape(S, 6, n // 2, 2, n // 2, 2, c_in).mean(axis=(3, 5), dtype=np.float32)
    else:
        layer = graph_cases.up_layer(rng, c_in, c_out)
        truth, cpu32 = graph_np.up2(h, layer.weight, layer.bias), graph_cases.twin_up2(layer, h)
    graph_cases.device_layer(device, kind, h, layer, "tanh", c_out=c_out, dst=dst, dst_off=dst_off, src_off=src_off,
                             src_width=src_off + c_in + 3)
    got = dst.cpu().numpy()
    outside = np.ones(ld, bool)
    outside[dst_off:dst_off + c_out] = False
    assert np.array_equal(got[..., outside].view(np.uint32), sentinel[..., outside].view(np.uint32))
    _gate(got[..., dst_off:dst_off + c_out], truth, cpu32, f"{kind} slice")


def test_overlapping_slices_are_refused(device):
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    buf = torch.zeros((1, 6, 4, 4, 12), dtype=torch.float32, device=device)
    w = torch.zeros((4, 4), dtype=torch.float32, device=device)
    for src_off, dst_off in ((0, 3), (4, 4), (5, 2)):
        with pytest.raises(_lib.Fv3HipError, match="overlap"):
            _lib.call_on(device, "fv3hip_graph_sage", buf.data_ptr(), 12, src_off, 0, w.data_ptr(), w.data_ptr(), None, buf.data_ptr(), 12,
                         dst_off, 0, 1, 4, 4, 4, _lib.ACT_LINEAR, _stream(device))
    with pytest.raises(_lib.Fv3HipError, match="do not fit"):
        _lib.call_on(device, "fv3hip_graph_sage", buf.data_ptr(), 12, 9, 0, w.data_ptr(), w.data_ptr(), None, buf.data_ptr(), 12, 0, 0, 1,
                     4, 4, 4, _lib.ACT_LINEAR, _stream(device))
    with pytest.raises(_lib.Fv3HipError, match="even"):
        _lib.call_on(device, "fv3hip_graph_pool2", buf.data_ptr(), 12, 0, buf.data_ptr(), 12, 6, 1, 3, 4, _stream(device))
    with pytest.raises(_lib.Fv3HipError) as err:
        _lib.call_on(device, "fv3hip_graph_sage", buf.data_ptr(), 12, 0, 0, w.data_ptr(), w.data_ptr(), None, buf.data_ptr(), 12, 6, 0, 1, 4,
                     4, 4, 7, _stream(device))
    assert err.value.code == _lib.EUNSUPPORTED


@pytest.mark.parametrize("nx", [2, 16, 18])
def test_pool2(device, nx):
    rng = np.random.default_rng(nx)
    for S, c in ((1, 1), (3, 5), (2, 64)):
        h = graph_cases.make_state(rng, S, nx, c)
        got = graph_cases.device_layer(device, "pool2", h).cpu().numpy()
        # the kernel's own order in float32: ((a00 + a01) + a10) + a11, times 0.25 -- bit for bit
        want32 = (((h[:, :, 0::2, 0::2] + h[:, :, 0::2, 1::2]) + h[:, :, 1::2, 0::2]) + h[:, :, 1::2, 1::2]) * np.float32(0.25)
        assert np.array_equal(got, want32)
        _gate(got, graph_np.pool2(h), want32, f"pool2 n={nx} c={c}")


@pytest.mark.parametrize("nx", [2, 16, 18])
def test_up2(device, nx):
    rng = np.random.default_rng(nx)
    for S, c_in, c_out in ((1, 1, 1), (3, 16, 8), (2, 17, 33), (1, 65, 5)):
        layer = graph_cases.up_layer(rng, c_in, c_out)
        h = graph_cases.make_state(rng, S, nx, c_in)
        got = graph_cases.device_layer(device, "up2", h, layer).cpu().numpy()
        _gate(got, graph_np.up2(h, layer.weight, layer.bias), graph_cases.twin_up2(layer, h), f"up2 n={nx} {c_in}->{c_out}")


def _class_map(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN."""
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("nx, cell", [(17, (0, 0, 5)), (17, (2, 16, 16)), (17, (4, 8, 8)), (2, (5, 1, 0)), (34, (3, 33, 15))])
def test_a_non_finite_cell_reaches_itself_and_its_four_neighbours(device, value, nx, cell):
    rng = np.random.default_rng(nx)
    layer = graph_cases.sage_layer(rng, 9, 33)
    h = graph_cases.make_state(rng, 2, nx, 9)
    clean = graph_cases.device_layer(device, "sage", h, layer, "relu").cpu().numpy()
    bad = h.copy()
    t, x, y = cell
    bad[1, t, x, y, 4] = value
    got = graph_cases.device_layer(device, "sage", bad, layer, "relu").cpu().numpy()
    truth = graph_np.sage(bad, layer.w_self, layer.w_neigh, layer.bias, "relu")
    touched = np.zeros((2, 6 * nx * nx), bool)
    touched[1, graph_np.neighbour_table(nx)[(t * nx + x) * nx + y]] = True
    touched = touched.reshape(2, 6, nx, nx)
    assert touched.sum() == 5
    assert np.array_equal(_class_map(got), _class_map(truth))
    assert (~np.isfinite(got[touched])).any(axis=-1).all() and np.isfinite(got[~touched]).all()   # (ReLU turns -Inf into 0)
    assert np.array_equal(got[~touched].view(np.uint32), clean[~touched].view(np.uint32))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_non_finite_cell_in_pool2_and_up2(device, value):
    rng = np.random.default_rng(3)
    h = graph_cases.make_state(rng, 2, 18, 17)
    bad = h.copy()
    bad[1, 2, 17, 0, 3] = value
    layer = graph_cases.up_layer(rng, 17, 9)
    for kind, lay, oracle, cells in (("pool2", None, graph_np.pool2, [(8, 0)]),
                                     ("up2", layer, lambda a: graph_np.up2(a, layer.weight, layer.bias), [(34, 0), (34, 1), (35, 0), (35, 1)])):
        clean = graph_cases.device_layer(device, kind, h, lay).cpu().numpy()
        got = graph_cases.device_layer(device, kind, bad, lay).cpu().numpy()
        touched = np.zeros(got.shape, bool)
        for x, y in cells:
            touched[1, 2, x, y, 3 if kind == "pool2" else slice(None)] = True
        assert np.array_equal(_class_map(got), _class_map(oracle(bad)))
        assert not np.isfinite(got[touched]).any() and np.isfinite(got[~touched]).all()
        assert np.array_equal(got[~touched].view(np.uint32), clean[~touched].view(np.uint32))
