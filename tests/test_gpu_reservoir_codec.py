"""Reservoir models whose transformers are column codecs, on the MI355X.

Composition, bit for bit: a model whose input / output / hybrid transformer is a codec equals -- in state bits and output
bits -- the same model with do-nothing transformers of the latent sizes, fed ``codec.encode(inputs)`` and decoded by
``codec.decode(...)``.  The reservoir kernels themselves are gated by tests/test_gpu_reservoir*.py and the codecs by
tests/test_gpu_codec.py; what is new here is the wiring, which adds no arithmetic of its own.
"""
import zlib

import numpy as np
import pytest
import torch

from fv3net_amd import fit
from fv3net_amd.fit.reservoir import (HybridReservoirComputingModel, HybridReservoirDatasetAdapter, ReservoirComputingModel,
                                      ReservoirDatasetAdapter, TransformerGroup)
from fv3net_amd.graphs import GraphedCall
from fv3net_amd.xr_compat import DataArray, Dataset

import codec_cases as C
import reservoir_cases as RC

pytestmark = pytest.mark.gpu

IN_SIZES, OUT_SIZES, HYB_SIZES = (3, 2), (2, 1), (1, 2)
L_IN, L_OUT, L_HYB = 4, 3, 2


def _codec(kind, rng, sizes, n_latent):
    if kind == "dense":
        return C.dense_codec(C.dense_spec(rng, sizes, (20,), n_latent))
    return C.affine_codec(C.affine_spec(rng, sizes, n_latent, whiten=True, with_mean=True, with_std=True, positive=False))


def _case(kinds, hybrid, layout, overlap, mask, out_scale_spatial=False, seed=0, sizes=None):
    """(coded model, plain model with do-nothing transformers of the latent sizes, the codecs (input, output or None,
    hybrid or None), the restatement model).  ``kinds``: the codec kind of the (input, output, hybrid) side; ``sizes``:
    the z sizes of the variables of each side (default ``IN_SIZES``, ``OUT_SIZES``, ``HYB_SIZES``)."""
    in_sizes, out_sizes, hyb_sizes = sizes or (IN_SIZES, OUT_SIZES, HYB_SIZES)
    rng = np.random.RandomState(zlib.crc32(repr((kinds, hybrid, layout, overlap, str(mask), out_scale_spatial, seed)).encode())
                                % (2 ** 31))
    m = RC.make_model(rng, layout, (2, 3), overlap=overlap, state_size=41, in_sizes=(L_IN,),
                      out_sizes=(2, 2) if out_scale_spatial else (L_OUT,),
                      out_kind="scale-spatial" if out_scale_spatial else "do-nothing",
                      out_tf_mask=np.float64 if out_scale_spatial else None, hybrid_sizes=(L_HYB,) if hybrid else None,
                      input_mask=mask, hybrid_mask=mask if hybrid else None, square=True)
    ns = layout[0] * layout[1]
    state = rng.uniform(-1, 1, (ns, 41))
    plain = RC.package_model(m, state=state)
    tf_in = _codec(kinds[0], rng, in_sizes, L_IN)
    tf_out = None if out_scale_spatial else _codec(kinds[1], rng, out_sizes, L_OUT)
    tf_hyb = _codec(kinds[2], rng, hyb_sizes, L_HYB) if hybrid else None
    group = TransformerGroup(tf_in, tf_out or plain.transformers.output, tf_hyb or tf_in)
    names = lambda p, n: [f"{p}{v}" for v in range(n)]  # noqa: E731
    n_out = 2
    parts = (plain.reservoir, plain.readout, plain.rank_divider, group)
    if hybrid:
        coded = HybridReservoirComputingModel(names("i", 2), names("h", 2), names("o", n_out), *parts,
                                              square_half_hidden_state=True, hybrid_input_mask=m["hybrid_mask"])
    else:
        coded = ReservoirComputingModel(names("i", 2), names("o", n_out), *parts, square_half_hidden_state=True)
    return coded, plain, (tf_in, tf_out, tf_hyb), m, rng


def _inputs(rng, sizes, extent, dtypes=(np.float64, np.float32)):
    return [torch.from_numpy(a).cuda() for a in RC.make_arrays(rng, sizes, extent, list(dtypes))]


def _step_both(coded, plain, codecs, x, h):
    """One increment and one predict of both models; asserts equal bits; returns the coded model's outputs."""
    tf_in, tf_out, tf_hyb = codecs
    coded.increment_state(x)
    plain.increment_state([tf_in.encode_unstacked_xyz(x)])
    assert np.array_equal(coded.get_state().view(np.uint8), plain.get_state().view(np.uint8)), "state bits"
    if tf_hyb is not None:
        got = coded.predict(h)
        raw = plain.predict([tf_hyb.encode_unstacked_xyz(h)])
    else:
        got = coded.predict(device_output=True)
        raw = plain.predict(device_output=True)
    want = tf_out.decode_unstacked_xyz(raw[0]) if tf_out is not None else raw
    assert len(got) == len(want)
    for v, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and torch.equal(g.view(torch.uint8), w.view(torch.uint8)), f"output {v} bits"
    return got


CASES = {
    "pure-dense-22-ov1-f64": (("dense", "dense", None), False, (2, 2), 1, np.float64),
    "pure-dense-32-ov0-f32": (("dense", "dense", None), False, (3, 2), 0, np.float32),
    "pure-affine-32-ov1-f32": (("affine", "affine", None), False, (3, 2), 1, np.float32),
    "pure-affine-22-ov0-f64": (("affine", "affine", None), False, (2, 2), 0, np.float64),
    "hybrid-dense-32-ov1-f32": (("dense", "dense", "dense"), True, (3, 2), 1, np.float32),
    "hybrid-affine-22-ov1-f64": (("affine", "affine", "affine"), True, (2, 2), 1, np.float64),
    "hybrid-mixed-22-ov0-f32": (("dense", "affine", "affine"), True, (2, 2), 0, np.float32),
    "hybrid-mixed-32-ov1-f64": (("affine", "dense", "dense"), True, (3, 2), 1, np.float64),
}


@pytest.mark.parametrize("name", list(CASES))
def test_codec_model_equals_do_nothing_model_around_the_codec(name):
    kinds, hybrid, layout, overlap, mask = CASES[name]
    coded, plain, codecs, m, rng = _case(kinds, hybrid, layout, overlap, mask)
    for _ in range(2):
        x = _inputs(rng, IN_SIZES, RC.ov_extent(m))
        h = _inputs(rng, HYB_SIZES, m["rank"]) if hybrid else None
        outs = _step_both(coded, plain, codecs, x, h)
    assert [tuple(o.shape) for o in outs] == [(*m["rank"], nz) for nz in OUT_SIZES]
    # numpy in, numpy out
    if not hybrid:
        host = coded.predict()
        assert all(isinstance(a, np.ndarray) and np.array_equal(a, o.cpu().numpy(), equal_nan=True) for a, o in zip(host, outs))


@pytest.mark.parametrize("hybrid", [False, True], ids=["pure", "hybrid"])
def test_codec_input_with_scale_spatial_output(hybrid):
    coded, plain, codecs, m, rng = _case(("dense", None, "affine"), hybrid, (2, 2), 1, np.float64, out_scale_spatial=True)
    x = _inputs(rng, IN_SIZES, RC.ov_extent(m))
    h = _inputs(rng, HYB_SIZES, m["rank"]) if hybrid else None
    outs = _step_both(coded, plain, codecs, x, h)
    assert all(o.dtype == torch.float32 for o in outs)


@pytest.mark.parametrize("hybrid", [False, True], ids=["pure", "hybrid"])
def test_get_model_from_subdomain(hybrid):
    coded, plain, codecs, m, rng = _case(("dense", "affine", "dense"), hybrid, (3, 2), 1, np.float64)
    x = _inputs(rng, IN_SIZES, RC.ov_extent(m))
    h = _inputs(rng, HYB_SIZES, m["rank"]) if hybrid else None
    _step_both(coded, plain, codecs, x, h)
    sub_c, sub_p = coded.get_model_from_subdomain(4), plain.get_model_from_subdomain(4)
    assert sub_c.transformers.input is coded.transformers.input
    xs = _inputs(rng, IN_SIZES, (2 + 2, 3 + 2))
    hs = _inputs(rng, HYB_SIZES, (2, 3)) if hybrid else None
    outs = _step_both(sub_c, sub_p, codecs, xs, hs)
    assert [tuple(o.shape) for o in outs] == [(2, 3, nz) for nz in OUT_SIZES]


@pytest.mark.parametrize("hybrid", [False, True], ids=["pure", "hybrid"])
def test_dataset_adapters_and_dump_load(hybrid, tmp_path):
    same_z = ((2, 2), (2, 2), (2, 2))  # the variables of a dataset share one z
    coded, plain, codecs, m, rng = _case(("affine", "dense", "affine"), hybrid, (2, 2), 1, np.float32, sizes=same_z)
    adapter = (HybridReservoirDatasetAdapter if hybrid else ReservoirDatasetAdapter)(coded)
    fit.dump(adapter, str(tmp_path / "adapter"))
    loaded = fit.load(str(tmp_path / "adapter"))
    assert type(loaded) is type(adapter)
    assert type(loaded.model.transformers.input) is type(codecs[0])
    assert type(loaded.model.transformers.output) is type(codecs[1])
    x = RC.make_arrays(rng, (2, 2), RC.ov_extent(m))
    h = RC.make_arrays(rng, (2, 2), m["rank"])
    ds_in = Dataset({f"i{v}": DataArray(torch.from_numpy(a).cuda(), dims=["x", "y", "z"]) for v, a in enumerate(x)})
    ds_h = Dataset({f"h{v}": DataArray(torch.from_numpy(np.ascontiguousarray(a.transpose(1, 0, 2))).cuda(), dims=["y", "x", "z"])
                    for v, a in enumerate(h)})
    results = []
    for ad in (adapter, loaded):
        ad.increment_state(ds_in)
        out = ad.predict(ds_h)
        results.append((ad.model.get_state(), [out[f"o{v}"] for v in range(2)]))
    assert np.array_equal(results[0][0].view(np.uint8), results[1][0].view(np.uint8)), "state bits after dump and load"
    for a, b in zip(results[0][1], results[1][1]):
        assert a.dims == b.dims and torch.equal(a.data.contiguous().view(torch.uint8), b.data.contiguous().view(torch.uint8)), \
            "output bits after dump and load"
    # the adapter against the models underneath
    _, plain2, codecs2, _, _ = _case(("affine", "dense", "affine"), hybrid, (2, 2), 1, np.float32, sizes=same_z)
    xd = [torch.from_numpy(a).cuda() for a in x]
    hd = [torch.from_numpy(a).cuda() for a in h]
    plain2.increment_state([codecs2[0].encode_unstacked_xyz(xd)])
    raw = plain2.predict([codecs2[2].encode_unstacked_xyz(hd)]) if hybrid else plain2.predict(device_output=True)
    want = codecs2[1].decode_unstacked_xyz(raw[0])
    for v, w in enumerate(want):
        da = results[0][1][v]
        got = da.data.permute(*[da.dims.index(d) for d in ("x", "y", "z") if d in da.dims])  # the inputs came as (y, x, z)
        w = w[:, :, 0] if w.shape[-1] == 1 else w
        assert torch.equal(got.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), f"adapter output {v}"


@pytest.mark.parametrize("name", ["pure-reservoir", "hybrid-reservoir"])
def test_model_dump_load_same_bits(name, tmp_path):
    hybrid = name == "hybrid-reservoir"
    coded, plain, codecs, m, rng = _case(("dense", "affine", "dense"), hybrid, (3, 2), 1, np.float64)
    fit.dump(coded, str(tmp_path / "m"))
    with open(tmp_path / "m" / "name") as f:
        assert f.read() == name
    loaded = fit.load(str(tmp_path / "m"))
    x = _inputs(rng, IN_SIZES, RC.ov_extent(m))
    h = _inputs(rng, HYB_SIZES, m["rank"]) if hybrid else None
    outs = _step_both(coded, plain, codecs, x, h)
    loaded.increment_state(x)
    assert np.array_equal(loaded.get_state().view(np.uint8), coded.get_state().view(np.uint8))
    again = loaded.predict(h) if hybrid else loaded.predict(device_output=True)
    for a, b in zip(again, outs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("hybrid", [False, True], ids=["pure", "hybrid"])
def test_graph_replay_steps_like_eager(hybrid):
    """One increment + predict with codecs on every side, captured by ``GraphedCall`` and replayed three times on new data,
    is bit-identical to eager steps."""
    kinds = ("dense", "affine", "dense")
    graphed, _, _, m, rng = _case(kinds, hybrid, (3, 2), 1, np.float64)
    eager, _, _, _, _ = _case(kinds, hybrid, (3, 2), 1, np.float64)
    state0 = graphed.reservoir.state
    series = [(_inputs(rng, IN_SIZES, RC.ov_extent(m)), _inputs(rng, HYB_SIZES, m["rank"]) if hybrid else None)
              for _ in range(4)]
    x = [t.clone() for t in series[0][0]]
    h = [t.clone() for t in series[0][1]] if hybrid else None

    def step():
        graphed.increment_state(x)
        return graphed.predict(h) if hybrid else graphed.predict(device_output=True)

    call = GraphedCall(step, warmup=2)
    graphed.set_state(state0)  # the warm-up steps and the capture moved it
    eager.set_state(state0)
    for t in range(1, 4):
        for held, new in zip(x + (h or []), series[t][0] + (series[t][1] or [])):
            held.copy_(new)
        outs = call.replay()
        eager.increment_state(series[t][0])
        expect = eager.predict(series[t][1]) if hybrid else eager.predict(device_output=True)
        assert np.array_equal(graphed.get_state().view(np.uint8), eager.get_state().view(np.uint8)), f"state after replay {t}"
        for o, e in zip(outs, expect):
            assert torch.equal(o.view(torch.uint8), e.view(torch.uint8)), f"outputs after replay {t}"
