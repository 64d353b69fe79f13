"""The column codecs without a GPU: the restatement (tests/codec_np.py) against torch-CPU layers and against sklearn's own
scaler and PCA, the artifacts, their recognition by ``load_transformer`` and ``fit.load``, the refusals, and the offline
training function."""
import os

import numpy as np
import pytest
import torch

from fv3net_amd import fit
from fv3net_amd.fit.reservoir import (HybridReservoirComputingModel, HybridReservoirDatasetAdapter, ReservoirComputingModel,
                                      ReservoirDatasetAdapter, TransformerGroup)
from fv3net_amd.reservoir import DenseAutoencoder, DoNothingTransformer, SkTransformer, load_transformer

import codec_cases as C
import codec_np as N
import reservoir_cases as RC
import tolerances


def _linear(w, b):
    lin = torch.nn.Linear(w.shape[0], w.shape[1])
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w.T))
        lin.bias.copy_(torch.from_numpy(b))
    return lin


@pytest.mark.parametrize("name", ["default", "k7", "k63_three", "k65_none"])
def test_restatement_matches_torch_linear_chains(name):
    """The float32 evaluation by torch's ``nn.Linear`` layers passes the gate the kernels pass, with the numpy float32
    evaluation as its yardstick: the restatement is the graph Keras builds."""
    spec, x, latent = C.cached(C.dense_case, name)
    with torch.no_grad():
        h = torch.from_numpy(N.normalise32(spec, x))
        for w, b in spec["enc"]:
            h = torch.relu(_linear(w, b)(h))
        tolerances.assert_close_per_level(h.numpy(), N.dense_encode(spec, x, np.float64), cpu32=N.dense_encode(spec, x, np.float32),
                                          name=f"encode {name}", rel=1e-5)
        h = torch.from_numpy(latent)
        for w, b in spec["dec"]:
            h = torch.relu(_linear(w, b)(h))
        y = torch.cat([_linear(w, b)(h) for w, b in spec["heads"]], dim=1) * torch.from_numpy(spec["scale"]) + torch.from_numpy(
            spec["center"])
    outs = [N.limit(p, None if lo is None else np.float32(lo), None if hi is None else np.float32(hi))
            for p, lo, hi in zip(N.split(y.numpy(), spec["sizes"]), spec["min"], spec["max"])]
    for v, (g, t, c) in enumerate(zip(outs, N.dense_decode(spec, latent, np.float64), N.dense_decode(spec, latent, np.float32))):
        tolerances.assert_close_per_level(g, t, cpu32=c, name=f"decode {name} variable {v}", rel=1e-5)


def test_limit_semantics():
    y = np.array([-2.0, -1.0, 0.0, 1.0, 2.0, np.nan, np.inf, -np.inf], np.float32)
    got = N.limit(y, np.float32(-1.0), np.float32(1.0))
    np.testing.assert_array_equal(got, np.array([-1, -1, 0, 1, 1, np.nan, 1, -1], np.float32))
    np.testing.assert_array_equal(N.limit(y, None, np.float32(1.0))[[0, 7]], [-2.0, -np.inf])


@pytest.mark.parametrize("whiten", [False, True], ids=["plain", "whiten"])
@pytest.mark.parametrize("with_mean, with_std", [(True, True), (False, True), (True, False)])
def test_restatement_and_from_sklearn_match_sklearn(whiten, with_mean, with_std):
    pytest.importorskip("sklearn")
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler

    rng = np.random.RandomState(3)
    sizes = [5, 1, 6]
    x = rng.randn(400, 12) @ rng.randn(12, 12) + rng.randn(12)
    scaler = StandardScaler(with_mean=with_mean, with_std=with_std).fit(x)
    pca = PCA(n_components=4, whiten=whiten).fit(scaler.transform(x))
    codec = SkTransformer.from_sklearn(pca, scaler, enforce_positive_outputs=True, original_feature_sizes=sizes)
    assert codec.n_latent_dims == 4 and codec.original_feature_sizes == sizes and codec.enforce_positive_outputs
    assert (codec.scaler_mean is None) == (not with_mean) and (codec.scaler_scale is None) == (not with_std)
    assert (codec.explained_variance is None) == (not whiten)
    spec = {"sizes": sizes, "mean": codec.scaler_mean, "std": codec.scaler_scale, "pca_mean": codec.pca_mean,
            "components": codec.components, "ev": codec.explained_variance, "positive": False}
    parts = N.split(x, sizes)
    want = pca.transform(scaler.transform(x))
    RC.check(N.affine_encode(spec, parts), want, C.affine_gate(want), "encode against sklearn")
    z = rng.randn(50, 4)
    back = scaler.inverse_transform(pca.inverse_transform(z))
    RC.check(np.concatenate(N.affine_decode(spec, z), -1), back, C.affine_gate(back), "decode against sklearn")
    spec["positive"] = True
    np.testing.assert_array_equal(np.concatenate(N.affine_decode(spec, z), -1) >= 0, True)


def test_from_sklearn_refusals():
    pytest.importorskip("sklearn")
    from sklearn.decomposition import PCA, TruncatedSVD
    from sklearn.preprocessing import MinMaxScaler, StandardScaler

    x = np.random.RandomState(0).randn(30, 6)
    scaler, pca = StandardScaler().fit(x), PCA(n_components=2).fit(x)
    with pytest.raises(ValueError, match="TruncatedSVD"):
        SkTransformer.from_sklearn(TruncatedSVD(n_components=2).fit(x), scaler, original_feature_sizes=[6])
    with pytest.raises(ValueError, match="MinMaxScaler"):
        SkTransformer.from_sklearn(pca, MinMaxScaler().fit(x), original_feature_sizes=[6])
    with pytest.raises(ValueError, match="PCA"):
        SkTransformer.from_sklearn(PCA(n_components=2), scaler, original_feature_sizes=[6])  # not fitted
    with pytest.raises(ValueError, match="original_feature_sizes is required"):
        SkTransformer.from_sklearn(pca, scaler)


def _same_arrays(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert p.dtype == q.dtype and np.array_equal(p, q)


def test_dense_artifact_round_trip(tmp_path):
    spec, _, _ = C.cached(C.dense_case, "k7")
    codec = C.dense_codec(spec)
    codec.dump(str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == ["dense_autoencoder.yaml", "weights.npz"]
    for back in (DenseAutoencoder.load(str(tmp_path / "d")), load_transformer(str(tmp_path / "d"))):
        assert type(back) is DenseAutoencoder
        assert back.original_feature_sizes == [5, 1, 1] and back.n_latent_dims == 10 and back.n_variables == 3
        _same_arrays([back.center, back.scale], [codec.center, codec.scale])
        for name in ("encoder_kernels", "encoder_biases", "decoder_kernels", "decoder_biases", "head_kernels", "head_biases"):
            _same_arrays(getattr(back, name), getattr(codec, name))
        assert back.output_min == codec.output_min and back.output_max == codec.output_max
        assert back.output_min[1] is None and back.output_min[0] is not None
    scale_only = C.dense_codec(C.cached(C.scale_only_case, "s7")[0])
    scale_only.dump(str(tmp_path / "s"))
    back = load_transformer(str(tmp_path / "s"))
    assert back.n_latent_dims == 7 and not back.encoder_kernels and not back.head_kernels


def test_sk_artifact_round_trip(tmp_path):
    for name in ("whiten40", "k7", "k64"):
        spec = C.cached(C.affine_case, name)[0]
        codec = C.affine_codec(spec)
        path = str(tmp_path / name)
        codec.dump(path)
        assert sorted(os.listdir(path)) == ["arrays.npz", "sk_transformer.yaml"]
        back = load_transformer(path)
        assert type(back) is SkTransformer and back.original_feature_sizes == spec["sizes"]
        assert back.enforce_positive_outputs == spec["positive"] and back.n_latent_dims == spec["components"].shape[0]
        for attr in ("components", "pca_mean", "explained_variance", "scaler_mean", "scaler_scale"):
            a, b = getattr(back, attr), getattr(codec, attr)
            assert (a is None and b is None) or np.array_equal(a, b), attr


def test_registered_names(tmp_path):
    dense = C.dense_codec(C.cached(C.dense_case, "k7")[0])
    sk = C.affine_codec(C.cached(C.affine_case, "k7")[0])
    for codec, name in ((dense, "hip-dense-autoencoder"), (sk, "hip-sk-transformer")):
        path = str(tmp_path / name)
        fit.dump(codec, path)
        with open(os.path.join(path, "name")) as f:
            assert f.read() == name
        assert type(fit.load(path)) is type(codec)
        assert callable(codec.predict)


@pytest.mark.parametrize("leaf, kind", [("encoder.tf", "dense-autoencoder"), ("sk_transformer.pkl", "sk-transformer")])
def test_reference_files_are_still_refused(tmp_path, leaf, kind):
    d = tmp_path / "t"
    os.makedirs(d / leaf) if leaf.endswith(".tf") else (os.makedirs(d), open(d / leaf, "wb").close())
    with pytest.raises(ValueError, match=kind) as err:
        load_transformer(str(d))
    assert "INTEGRATION.md" in str(err.value)


def test_constructor_refusals():
    w = lambda a, b: np.zeros((a, b), np.float32)  # noqa: E731
    b = lambda n: np.zeros(n, np.float32)  # noqa: E731
    with pytest.raises(ValueError, match="center and scale need 3 values"):
        DenseAutoencoder(np.zeros(2), np.ones(3), [2, 1])
    with pytest.raises(ValueError, match="encoder layer 1: kernel"):
        DenseAutoencoder(np.zeros(3), np.ones(3), [2, 1], [w(3, 4), w(5, 2)], [b(4), b(2)], [], [], [w(2, 2), w(2, 1)],
                         [b(2), b(1)])
    with pytest.raises(ValueError, match="one head per variable"):
        DenseAutoencoder(np.zeros(3), np.ones(3), [2, 1], [w(3, 2)], [b(2)], [], [], [w(2, 3)], [b(3)])
    with pytest.raises(ValueError, match="head 1: kernel"):
        DenseAutoencoder(np.zeros(3), np.ones(3), [2, 1], [w(3, 2)], [b(2)], [], [], [w(2, 2), w(2, 2)], [b(2), b(2)])
    with pytest.raises(ValueError, match="no decoder layers or heads"):
        DenseAutoencoder(np.zeros(3), np.ones(3), [2, 1], [], [], [w(3, 2)], [b(2)])
    with pytest.raises(ValueError, match="must be greater than min"):
        DenseAutoencoder(np.zeros(3), np.ones(3), [2, 1], output_min=[1.0, None], output_max=[1.0, None])
    with pytest.raises(ValueError, match="must be finite"):
        DenseAutoencoder(np.zeros(3), np.ones(3), [2, 1], [w(3, 2) * np.nan], [b(2)], [], [], [w(2, 2), w(2, 1)], [b(2), b(1)])
    with pytest.raises(ValueError, match="do not match the 3 features"):
        SkTransformer(np.zeros((2, 4)), np.zeros(3), [2, 1])
    with pytest.raises(ValueError, match="explained_variance needs shape"):
        SkTransformer(np.zeros((2, 3)), np.zeros(3), [2, 1], explained_variance=np.ones(3))
    with pytest.raises(ValueError, match="original_feature_sizes is required"):
        SkTransformer(np.zeros((2, 3)), np.zeros(3), None)
    codec = SkTransformer(np.zeros((2, 3)), np.zeros(3), [2, 1])
    with pytest.raises(ValueError, match="Expected 2 input arrays"):
        codec.check_inputs([(4, 4, 2)])
    with pytest.raises(ValueError, match="feature dimension must be 1"):
        codec.check_inputs([(4, 4, 2), (4, 4, 2)])


@pytest.mark.parametrize("name", ["pure-reservoir", "hybrid-reservoir", "reservoir-adapter", "hybrid-reservoir-adapter"])
def test_fit_load_of_the_four_layouts_with_codec_directories(name, tmp_path):
    """``_model()`` is lazy, so dumping and loading needs no GPU."""
    hybrid = name.startswith("hybrid")
    rng = np.random.RandomState(5)
    m = RC.make_model(rng, (2, 2), (2, 3), overlap=1, state_size=11, in_sizes=(4,), out_sizes=(3,),
                      hybrid_sizes=(2,) if hybrid else None, input_mask=np.float64)
    plain = RC.package_model(m, state=rng.uniform(-1, 1, (4, 11)))
    tf_in = C.dense_codec(C.dense_spec(rng, (3, 2), (20,), 4))
    tf_out = C.affine_codec(C.affine_spec(rng, (2, 1), 3, True, True, True, True))
    tf_hyb = C.dense_codec(C.dense_spec(rng, (1, 2), (), 2)) if hybrid else DoNothingTransformer([4])
    parts = (plain.reservoir, plain.readout, plain.rank_divider, TransformerGroup(tf_in, tf_out, tf_hyb))
    if hybrid:
        model = HybridReservoirComputingModel(["a", "b"], ["c", "d"], ["e", "f"], *parts)
    else:
        model = ReservoirComputingModel(["a", "b"], ["e", "f"], *parts)
    assert model._output_rank_divider.z_feature_size == 3
    obj = model
    if name.endswith("adapter"):
        obj = (HybridReservoirDatasetAdapter if hybrid else ReservoirDatasetAdapter)(model)
    path = str(tmp_path / "m")
    fit.dump(obj, path)
    back = fit.load(path)
    assert type(back) is type(obj)
    back_model = back.model if name.endswith("adapter") else back
    tfs = back_model.transformers
    assert type(tfs.input) is DenseAutoencoder and type(tfs.output) is SkTransformer
    assert type(tfs.hybrid) is (DenseAutoencoder if hybrid else DoNothingTransformer)
    assert tfs.input.n_latent_dims == 4 and tfs.output.n_latent_dims == 3 and tfs.output.enforce_positive_outputs
    _same_arrays(tfs.input.encoder_kernels, tf_in.encoder_kernels)
    assert np.array_equal(tfs.output.components, tf_out.components)
    assert back_model._device_model is None
    held = back_model._device_transformer(tfs.input)
    assert type(held) is DoNothingTransformer and held.original_feature_sizes == [4]
    assert back_model._device_transformer(tfs.hybrid) is tfs.hybrid or hybrid


def test_train_dense_autoencoder_learns_rank_three_columns():
    """Seeded rank-3 columns: after training the standardised reconstruction MSE is below the untrained model's and below
    1, the MSE of predicting the mean."""
    rng = np.random.RandomState(11)
    sizes = [6, 4]
    x = rng.randn(2000, 3) @ rng.randn(3, 10) + 0.01 * rng.randn(2000, 10) + rng.randn(10)
    arrays = N.split(x.astype(np.float32), sizes)

    def mse(codec):
        spec = {"sizes": sizes, "center": codec.center, "scale": codec.scale,
                "enc": list(zip(codec.encoder_kernels, codec.encoder_biases)),
                "dec": list(zip(codec.decoder_kernels, codec.decoder_biases)),
                "heads": list(zip(codec.head_kernels, codec.head_biases))}
        back = np.concatenate(N.dense_decode(spec, N.dense_encode(spec, arrays)), -1)
        return float(np.mean(((back - x) / x.std(axis=0)) ** 2))

    hp = fit.DenseAutoencoderHyperparameters(["a", "b"], latent_dim_size=5, units=16, n_dense_layers=1, epochs=0,
                                             batch_size=100, learning_rate=3e-3, seed=4)
    untrained = fit.train_dense_autoencoder(hp, arrays, device="cpu")
    hp.epochs = 30
    trained = fit.train_dense_autoencoder(hp, arrays, device="cpu")
    assert type(trained) is DenseAutoencoder and trained.original_feature_sizes == sizes and trained.n_latent_dims == 5
    assert len(trained.encoder_kernels) == 2 and len(trained.decoder_kernels) == 1 and len(trained.head_kernels) == 2
    np.testing.assert_allclose(trained.center, x.mean(axis=0), rtol=1e-4, atol=1e-5)
    before, after = mse(untrained), mse(trained)
    print(f"standardised reconstruction MSE: untrained {before:.3f}, trained {after:.3f}")
    assert after < before and after < 1.0
    again = fit.train_dense_autoencoder(hp, arrays, device="cpu")
    _same_arrays(again.encoder_kernels, trained.encoder_kernels)  # seeded
    hp.output_limits = {"b": (0.0, None)}
    limited = fit.train_dense_autoencoder(dataclass_with(hp, epochs=0), arrays, device="cpu")
    assert limited.output_min == [None, 0.0] and limited.output_max == [None, None]


def dataclass_with(hp, **changes):
    import dataclasses

    return dataclasses.replace(hp, **changes)
