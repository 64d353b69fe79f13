"""The MLP create paths on the host: fv3hip_mlp_create and fv3hip_mlp3_create share one check of the descriptor, so a
malformed one is FV3HIP_EINVAL in both, with the same message, before any device call and without a handle left behind."""
import ctypes

import numpy as np
import pytest

from fv3net_amd import _lib

PF = ctypes.POINTER(ctypes.c_float)


def _desc(keep, **over):
    """A valid descriptor: one source of 4 features, one hidden layer of width 256, one output of 3 features and one
    residual output.  ``over`` sets scalar fields or element 0 of an int array."""
    K, W, F = 4, 256, 3
    rng = np.random.RandomState(0)
    ints = {"in_source": [0], "in_feat_start": [0], "in_nfeat": [K], "in_transform": [_lib.TRANSFORM_NONE],
            "out_nfeat": [F], "res_source": [0], "res_output": [0]}
    floats = {"in_eps": np.zeros(1), "in_center": np.zeros(K), "in_scale": np.ones(K), "out_kernel": rng.randn(W, F),
              "out_bias": rng.randn(F), "out_scale": np.ones(F), "out_center": np.zeros(F)}
    d = _lib.MlpDesc()
    d.n_sources, d.n_inputs, d.n_hidden, d.width, d.n_outputs, d.n_residual = 1, 1, 1, W, 1, 1
    d.hidden_activation = _lib.ACT_RELU
    for k, v in ints.items():
        a = np.array([over.pop(k)] if k in over else v, np.intc)
        keep.append(a)
        setattr(d, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    for k, v in floats.items():
        a = np.ascontiguousarray(v, np.float32)
        keep.append(a)
        setattr(d, k, a.ctypes.data_as(PF))
    hk, hb = np.ascontiguousarray(rng.randn(K, W), np.float32), np.zeros(W, np.float32)
    ptrs = ((PF * 1)(hk.ctypes.data_as(PF)), (PF * 1)(hb.ctypes.data_as(PF)))
    keep.extend([hk, hb, ptrs])
    d.hidden_kernels = ctypes.cast(ptrs[0], ctypes.POINTER(PF))
    d.hidden_biases = ctypes.cast(ptrs[1], ctypes.POINTER(PF))
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("entry", ["fv3hip_mlp_create", "fv3hip_mlp3_create"])
@pytest.mark.parametrize("change, message", [
    (dict(n_sources=0), b"n_sources must be in [1, 16], got 0"),
    (dict(n_sources=17), b"n_sources must be in [1, 16], got 17"),
    (dict(in_source=1), b"in_source[0] out of range"),
    (dict(in_nfeat=0), b"bad feature range for input 0"),
    (dict(in_feat_start=-1), b"bad feature range for input 0"),
    (dict(out_nfeat=0), b"bad out_nfeat[0]"),
    (dict(res_source=5), b"res_source[0] out of range"),
    (dict(res_output=1), b"res_output[0] out of range"),
    (dict(n_residual=32), b"n_outputs + n_residual (+ the hidden output) must be <= 32"),
    (dict(width=0), b"width must be >= 1"),
    (dict(hidden_activation=9), b"unknown activation 9"),
    (None, b"null pointer"),
], ids=["n_sources=0", "n_sources=17", "in_source", "in_nfeat", "in_feat_start", "out_nfeat", "res_source", "res_output",
        "33-outputs", "width=0", "activation", "null-desc"])
def test_create_refuses_malformed_descriptors(entry, change, message):
    lib = _lib.load()
    keep = []
    d = None if change is None else _desc(keep, **change)
    h = ctypes.c_void_p()
    assert getattr(lib, entry)(None if d is None else ctypes.byref(d), ctypes.byref(h)) == _lib.EINVAL
    assert message in lib.fv3hip_last_error(), lib.fv3hip_last_error()
    assert not h.value
