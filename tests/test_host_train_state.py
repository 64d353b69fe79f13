"""What the trainers and the ``train_*`` functions share (``fv3net_amd.train_state``, ``fv3net_amd.fit.training``), on the host:
nothing here launches a kernel."""
import numpy as np
import pytest
import torch

from fv3net_amd.fit.training import epoch_minibatches, linear_arrays, resolve_backend
from fv3net_amd.train_state import FlatParameters, split_heads

SHAPES = {"k0": (3, 2), "b0": (2,), "conv": (1, 1, 2, 3), "b1": (3,)}


def _arrays():
    rng = np.random.default_rng(0)
    return [(key, rng.normal(0, 1, shape).astype(np.float32)) for key, shape in SHAPES.items()]


def test_flat_parameters_lay_the_arrays_out_in_order():
    arrays = _arrays()
    flat = FlatParameters(arrays, "cpu")
    sizes = [a.size for _, a in arrays]
    assert flat.size == sum(sizes) == 17
    for buffer in (flat.params, flat.grads, flat.m, flat.v):
        assert buffer.dtype == torch.float32 and tuple(buffer.shape) == (17,) and buffer.device.type == "cpu"
    assert all(not bool(b.any()) for b in (flat.grads, flat.m, flat.v))
    assert flat.step_count.dtype == torch.int64 and flat.step_count.tolist() == [0]

    host = flat.to_host(flat.params)
    assert list(host) == [key for key, _ in arrays]
    for key, a in arrays:
        assert host[key].dtype == np.float32 and host[key].shape == a.shape and host[key].tobytes() == a.tobytes()
    assert flat.params.numpy().tobytes() == b"".join(a.tobytes() for _, a in arrays)   # one after the other, nothing between


def test_flat_parameter_views_alias_their_buffer_at_one_offset():
    arrays = _arrays()
    flat = FlatParameters(arrays, "cpu")
    p, g = flat.views(flat.params), flat.views(flat.grads)
    offsets = np.cumsum([0] + [a.size for _, a in arrays])
    for (key, a), off in zip(arrays, offsets):
        assert tuple(p[key].shape) == tuple(g[key].shape) == a.shape
        assert p[key].storage_offset() == g[key].storage_offset() == off
        assert p[key].data_ptr() == flat.params.data_ptr() + 4 * off and g[key].data_ptr() == flat.grads.data_ptr() + 4 * off
    p["conv"][0, 0, 1, 2] = 7.5
    g["b0"].fill_(-2.0)
    assert flat.params[offsets[2] + 5] == 7.5 and flat.grads[offsets[1]:offsets[2]].tolist() == [-2.0, -2.0]
    assert flat.to_host(flat.params)["conv"][0, 0, 1, 2] == 7.5 and flat.to_host(flat.grads)["b0"].tolist() == [-2.0, -2.0]
    copy = flat.to_host(flat.params)
    copy["k0"][:] = 0                                         # a copy: the buffer does not see it
    assert flat.params[:6].numpy().tobytes() == arrays[0][1].tobytes()
    with pytest.raises(ValueError, match="given twice"):
        FlatParameters(arrays + arrays[:1], "cpu")


def test_split_heads_cuts_columns_and_biases_alike():
    rng = np.random.default_rng(1)
    kernels = [rng.normal(0, 1, (4, 5)).astype(np.float32), rng.normal(0, 1, (5, 6)).astype(np.float32)]
    biases = [rng.normal(0, 1, 5).astype(np.float32), rng.normal(0, 1, 6).astype(np.float32)]
    hidden_k, hidden_b, out_k, out_b = split_heads(kernels, biases, 6, None)
    assert len(hidden_k) == len(hidden_b) == 1 and np.array_equal(hidden_k[0], kernels[0]) and np.array_equal(hidden_b[0], biases[0])
    assert len(out_k) == len(out_b) == 1 and np.array_equal(out_k[0], kernels[1]) and np.array_equal(out_b[0], biases[1])
    _, _, out_k, out_b = split_heads(kernels, biases, 6, [2, 1, 3])
    for k, b, (lo, hi) in zip(out_k, out_b, [(0, 2), (2, 3), (3, 6)]):
        assert np.array_equal(k, kernels[1][:, lo:hi]) and np.array_equal(b, biases[1][lo:hi])
        assert k.flags.c_contiguous and k.base is None and b.base is None   # copies
    assert len(out_k) == len(out_b) == 3
    with pytest.raises(ValueError, match=r"head sizes \[2, 1, 2\] do not add up to 6 output features"):
        split_heads(kernels, biases, 6, [2, 1, 2])


def test_epoch_minibatches_are_the_loop_they_replace():
    g = torch.Generator().manual_seed(5)
    want = []
    for _ in range(2):
        perm = torch.randperm(7, generator=g)
        want.append([perm[0:3], perm[3:6], perm[6:7]])
    got = list(epoch_minibatches(7, 3, 2, 5, "cpu"))
    assert len(got) == 2
    for got_epoch, want_epoch in zip(got, want):
        assert [len(b) for b in got_epoch] == [3, 3, 1]
        assert all(a.dtype == torch.int64 and torch.equal(a, b) for a, b in zip(got_epoch, want_epoch))
    assert not torch.equal(torch.cat(got[0]), torch.cat(got[1]))   # one generator: the second epoch goes on where the first ended
    assert list(epoch_minibatches(7, 3, 0, 5, "cpu")) == []


def test_resolve_backend():
    assert resolve_backend(None, "cpu") == ("torch", torch.device("cpu"))
    assert resolve_backend("torch", "cpu") == ("torch", torch.device("cpu"))
    backend, dev = resolve_backend(None, None)
    assert backend == "torch" and dev.type == ("cuda" if torch.cuda.is_available() else "cpu")
    with pytest.raises(ValueError, match="backend must be None, 'torch' or 'hip', got 'bogus'"):
        resolve_backend("bogus", "cpu")
    with pytest.raises(ValueError, match="backend must be None, 'torch', got 'hip'"):
        resolve_backend("hip", "cpu", allow=("torch",))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resolve_backend("hip", "cpu")


def test_linear_arrays_are_fresh_keras_layout_copies():
    torch.manual_seed(0)
    layer = torch.nn.Linear(3, 2)
    weight, bias = layer.weight.detach().clone(), layer.bias.detach().clone()
    kernels, biases = linear_arrays([layer])
    assert len(kernels) == len(biases) == 1
    assert kernels[0].shape == (3, 2) and kernels[0].flags.c_contiguous and np.array_equal(kernels[0], weight.numpy().T)
    assert biases[0].shape == (2,) and np.array_equal(biases[0], bias.numpy())
    kernels[0][:] = 9.0
    biases[0][:] = 9.0
    assert torch.equal(layer.weight.detach(), weight) and torch.equal(layer.bias.detach(), bias)
