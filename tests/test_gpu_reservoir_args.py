"""The C-side argument checks of the reservoir and codec entry points that take the caller's (x, y, z) arrays: a null entry
in a pointer table, a dtype code that is neither F32 nor F64, and a null table are refused with EINVAL and their message
before anything is launched -- the state, the latent and the outputs are read back unchanged.

The entry points are called through ``_lib`` directly: the Python layer builds these tables itself and cannot get them wrong.
"""
import ctypes

import numpy as np
import pytest
import torch

from fv3net_amd import _lib

import codec_cases as CC
import reservoir_cases as RC

pytestmark = pytest.mark.gpu

N_T = 2
NULL_ENTRY, BAD_DTYPE, NULL_TABLE = "source 0 is null", "source 0: dtype must be F32 or F64", "null source pointer"


def _call(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.fv3hip_last_error().decode()


def _tables(tensors, ndim):
    n = len(tensors)
    return [(ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]),
            (ctypes.c_int * n)(*[_lib.F64 if t.dtype == torch.float64 else _lib.F32 for t in tensors]),
            (ctypes.c_int64 * (ndim * n))(*[s for t in tensors for s in t.stride()])]


def _bad_sources(tensors, ndim):
    """(pointer table, dtype codes, strides, expected message) of each bad form of the sources."""
    null_entry, bad_dtype = _tables(tensors, ndim), _tables(tensors, ndim)
    null_entry[0][0] = None
    bad_dtype[1][0] = 7
    yield (*null_entry, NULL_ENTRY)
    yield (*bad_dtype, BAD_DTYPE)
    yield (None, *_tables(tensors, ndim)[1:], NULL_TABLE)


def _out_tables(tensors):
    n = len(tensors)
    return [(ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]), (ctypes.c_int64 * (3 * n))(*[s for t in tensors for s in t.stride()])]


def _bad_outputs(tensors):
    null_entry = _out_tables(tensors)
    null_entry[0][0] = None
    yield (*null_entry, "output 0 is null")
    yield (None, _out_tables(tensors)[1], "null output pointer")


@pytest.fixture(scope="module")
def model():
    """Layout (1, 2), 2 x 2 cells per subdomain, overlap 1, state 3, one hybrid variable; a state that is not zero."""
    rng = np.random.RandomState(RC._seed("args"))
    m = RC.make_model(rng, (1, 2), (2, 2), overlap=1, state_size=3, in_sizes=(1,), out_sizes=(1,), hybrid_sizes=(1,))
    handle = RC.package_model(m, state=rng.uniform(-1, 1, (2, 3)))._model()
    z = lambda *shape: torch.full(shape, 0.5, dtype=torch.float64, device=handle.device)  # noqa: E731
    return handle, dict(x=[z(4, 6, 1)], h=[z(2, 4, 1)], out=[z(2, 4, 1)], xs=[z(N_T, 4, 6, 1)], hs=[z(N_T, 2, 4, 1)],
                        ys=[z(N_T, 2, 4, 1)], X=z(N_T, 2, 3 + 4), Y=z(N_T, 2, 4))


def test_reservoir_entry_points_refuse_bad_sources_before_any_launch(model):
    handle, a = model
    h, st = handle._handle, None
    before = handle.get_state().cpu().numpy()
    assert np.abs(before).min() > 0
    good_x, good_h, good_xs, good_hs = _tables(a["x"], 3), _tables(a["h"], 3), _tables(a["xs"], 4), _tables(a["hs"], 4)
    outs = _out_tables(a["out"])
    X, Y = a["X"].data_ptr(), a["Y"].data_ptr()
    calls = []
    for *bad, text in _bad_sources(a["x"], 3):
        calls.append((text, "fv3hip_reservoir_increment", (h, *bad, st)))
    for *bad, text in _bad_sources(a["h"], 3):
        calls.append((text, "fv3hip_reservoir_predict", (h, *bad, *outs, st)))
    for *bad, text in _bad_outputs(a["out"]):
        calls.append((text, "fv3hip_reservoir_predict", (h, *good_h, *bad, st)))
    for *bad, text in _bad_sources(a["xs"], 4):
        calls.append((text, "fv3hip_reservoir_train_series", (h, *bad, None, *good_hs, N_T, 0, X, st)))
    for *bad, text in _bad_sources(a["ys"], 4):
        calls.append((text, "fv3hip_reservoir_encode_targets", (h, *bad, N_T, Y, st)))
    with torch.cuda.device(handle.device):
        for text, name, args in calls:
            rc, message = _call(name, *args)
            assert rc == _lib.EINVAL and message == text, (name, text, rc, message)
        torch.cuda.synchronize()
    assert np.array_equal(handle.get_state().cpu().numpy(), before), "a refused call changed the state"
    for name in ("out", "X", "Y"):
        t = a[name][0] if isinstance(a[name], list) else a[name]
        assert bool((t == 0.5).all()), f"a refused call wrote {name}"
    # the good tables are good: the same calls go through
    with torch.cuda.device(handle.device):
        assert _call("fv3hip_reservoir_increment", h, *good_x, st)[0] == _lib.OK
        assert _call("fv3hip_reservoir_predict", h, *good_h, *outs, st)[0] == _lib.OK
        assert _call("fv3hip_reservoir_train_series", h, *good_xs, None, *good_hs, N_T, 0, X, st)[0] == _lib.OK
        assert _call("fv3hip_reservoir_encode_targets", h, *_tables(a["ys"], 4), N_T, Y, st)[0] == _lib.OK
        torch.cuda.synchronize()
    assert not np.array_equal(handle.get_state().cpu().numpy(), before)


def test_codec_entry_points_refuse_bad_tables_before_any_launch():
    """A dense codec of two variables (z sizes 2 and 1) with a latent of 2."""
    rng = np.random.RandomState(RC._seed("args-codec"))
    codec = CC.dense_codec(CC.dense_spec(rng, (2, 1), (), 2))
    dev = torch.device("cuda", torch.cuda.current_device())
    h, st, nx, ny = codec._handle_on(dev), None, 2, 3
    z = lambda *shape: torch.full(shape, 0.5, dtype=torch.float32, device=dev)  # noqa: E731
    x, outs, latent = [z(nx, ny, 2), z(nx, ny, 1)], [z(nx, ny, 2), z(nx, ny, 1)], z(nx, ny, 2)
    with torch.cuda.device(dev):
        for *bad, text in _bad_sources(x, 3):
            rc, message = _call("fv3hip_codec_encode", h, *bad, nx, ny, latent.data_ptr(), st)
            assert rc == _lib.EINVAL and message == text, (text, rc, message)
        for *bad, text in _bad_outputs(outs):
            rc, message = _call("fv3hip_codec_decode", h, latent.data_ptr(), _lib.F32, nx, ny, *bad, st)
            assert rc == _lib.EINVAL and message == text, (text, rc, message)
        rc, message = _call("fv3hip_codec_decode", h, latent.data_ptr(), 7, nx, ny, *_out_tables(outs), st)
        assert rc == _lib.EINVAL and message == "latent dtype must be F32 or F64", (rc, message)
        torch.cuda.synchronize()
        for t in (latent, *outs):
            assert bool((t == 0.5).all()), "a refused call wrote its output"
        assert _call("fv3hip_codec_encode", h, *_tables(x, 3), nx, ny, latent.data_ptr(), st)[0] == _lib.OK
        assert _call("fv3hip_codec_decode", h, latent.data_ptr(), _lib.F32, nx, ny, *_out_tables(outs), st)[0] == _lib.OK
        torch.cuda.synchronize()
