"""The CycleGAN training entry points check every argument on the host, before any HIP call: each spoiled argument list returns
``EINVAL`` / ``EUNSUPPORTED`` with a message on a machine without a GPU (the pointers are made-up addresses; the good
arguments themselves are never passed).  Also the workspace queries and the training forward's own refusals; then the
plain-torch side of the trainer against the reference's own run (tests/golden/make_cyclegan_train_golden.py), the image pool,
the configurations, ``train_cyclegan`` with the torch backend and the tile-by-tile halo padding."""
import os
import random

import numpy as np
import pytest
import torch

from cyclegan_train_cases import GOLDEN, fixture_config, training_batches, training_hyperparameters
from fv3net_amd import _lib
from fv3net_amd._lib import EINVAL, EUNSUPPORTED

REGULAR, STRIDED, TRANSPOSED = _lib.CYCLEGAN_CONV_REGULAR, _lib.CYCLEGAN_CONV_STRIDED, _lib.CYCLEGAN_CONV_TRANSPOSED
CUBE, ZEROS = _lib.CYCLEGAN_HALO_CUBE, _lib.CYCLEGAN_HALO_ZEROS
A, B, C, D, E, F, G = (0x10000000 * i for i in range(1, 8))   # far apart: no two buffers overlap

# S = 2 samples of an 8 x 8 face, 3 -> 5 channels, regular 3 x 3, cube halos
GOOD = {
    "fv3hip_cyclegan_train_conv": [
        ("src", A), ("src_ld", 3), ("src_off", 0), ("src_ss", 0), ("w", B), ("bias", C), ("dst", D), ("dst_ld", 5), ("dst_off", 0),
        ("dst_ss", 0), ("n_samples", 2), ("n", 8), ("c_in", 3), ("c_out", 5), ("kind", REGULAR), ("k", 3), ("halo", CUBE), ("stream", None)],
    "fv3hip_cyclegan_train_backward_data": [
        ("dy", A), ("dy_ld", 5), ("dy_off", 0), ("dy_ss", 0), ("w", B), ("dx", D), ("dx_ld", 3), ("dx_off", 0), ("dx_ss", 0),
        ("workspace", E), ("workspace_bytes", 2 * 6 * 10 * 10 * 3 * 4), ("n_samples", 2), ("n", 8), ("c_in", 3), ("c_out", 5),
        ("kind", REGULAR), ("k", 3), ("halo", CUBE), ("stream", None)],
    "fv3hip_cyclegan_train_backward_weight": [
        ("x", A), ("x_ld", 3), ("x_off", 0), ("x_ss", 0), ("dy", B), ("dy_ld", 5), ("dy_off", 0), ("dy_ss", 0), ("dw", C), ("db", D),
        ("workspace", E), ("workspace_bytes", 2 * (9 * 3 + 2) * 5 * 4), ("n_samples", 2), ("n", 8), ("c_in", 3), ("c_out", 5),
        ("kind", REGULAR), ("k", 3), ("halo", CUBE), ("stream", None)],
    "fv3hip_cyclegan_train_norm_backward": [
        ("dy", A), ("dy_ld", 3), ("dy_off", 0), ("dy_ss", 0), ("x", B), ("x_ld", 3), ("x_off", 0), ("x_ss", 0), ("mean", C), ("rstd", D),
        ("bias", None), ("slope", 0.2), ("dx", E), ("dx_ld", 3), ("dx_off", 0), ("dx_ss", 0), ("dbias", None), ("n_samples", 2), ("n", 8),
        ("c", 3), ("stream", None)],
}

GEOMETRY = [   # shared by the three convolution entry points
    ({"kind": REGULAR, "k": 7, "n": 2}, EINVAL),            # a halo of 3 on a face of 2
    ({"kind": REGULAR, "k": 5, "n": 1}, EINVAL),
    ({"kind": REGULAR, "k": 4}, EUNSUPPORTED), ({"kind": REGULAR, "k": 9}, EUNSUPPORTED), ({"kind": REGULAR, "k": 1}, EUNSUPPORTED),
    ({"kind": STRIDED, "k": 5}, EUNSUPPORTED), ({"kind": STRIDED, "k": 2}, EUNSUPPORTED),
    ({"kind": TRANSPOSED, "k": 3}, EUNSUPPORTED), ({"kind": 3}, EUNSUPPORTED), ({"kind": -1}, EUNSUPPORTED),
    ({"kind": STRIDED, "k": 3, "n": 7}, EINVAL), ({"kind": STRIDED, "k": 4, "n": 7}, EINVAL),
    ({"kind": TRANSPOSED, "k": 4, "n": 2049}, EINVAL),
    ({"halo": 2}, EINVAL), ({"n": 0}, EINVAL), ({"n": 4097}, EINVAL), ({"n_samples": -1}, EINVAL),
    ({"c_in": 0}, EINVAL), ({"c_out": 0}, EINVAL), ({"c_in": (1 << 16) + 1}, EINVAL),
]

CASES = {
    "fv3hip_cyclegan_train_conv": GEOMETRY + [
        ({"src": None}, EINVAL), ({"w": None}, EINVAL), ({"dst": None}, EINVAL), ({"src_ld": 2}, EINVAL), ({"dst_off": 1}, EINVAL),
        ({"src_ss": 5}, EINVAL), ({"dst": A, "dst_ld": 3, "c_out": 3}, EINVAL)],
    "fv3hip_cyclegan_train_backward_data": GEOMETRY + [
        ({"dy": None}, EINVAL), ({"w": None}, EINVAL), ({"dx": None}, EINVAL), ({"workspace": None}, EINVAL),
        ({"workspace_bytes": 2 * 6 * 10 * 10 * 3 * 4 - 1}, EINVAL), ({"dy_ld": 4}, EINVAL), ({"dx_off": 1}, EINVAL), ({"dx_ss": 7}, EINVAL),
        ({"dx": A, "dx_ld": 5, "c_in": 5, "workspace_bytes": 1 << 20}, EINVAL),    # dx is dy
        ({"workspace": A}, EINVAL), ({"workspace": D}, EINVAL),                     # the workspace overlaps dy / dx
        ({"kind": REGULAR, "k": 7, "workspace_bytes": 2 * 6 * 14 * 14 * 3 * 4 - 1}, EINVAL)],   # halo 3: 14 x 14 positions
    "fv3hip_cyclegan_train_backward_weight": GEOMETRY + [
        ({"x": None}, EINVAL), ({"dy": None}, EINVAL), ({"dw": None}, EINVAL), ({"workspace": None}, EINVAL),
        ({"workspace_bytes": 2 * (9 * 3 + 2) * 5 * 4 - 1}, EINVAL), ({"n_samples": 0}, EINVAL), ({"x_ld": 2}, EINVAL),
        ({"dw": A}, EINVAL), ({"db": B}, EINVAL), ({"workspace": C}, EINVAL)],
    "fv3hip_cyclegan_train_norm_backward": [
        ({"dy": None}, EINVAL), ({"x": None}, EINVAL), ({"mean": None}, EINVAL), ({"rstd": None}, EINVAL), ({"dx": None}, EINVAL),
        ({"slope": -0.1}, EINVAL), ({"slope": 1.5}, EINVAL), ({"slope": float("nan")}, EINVAL), ({"c": 0}, EINVAL), ({"n": 0}, EINVAL),
        ({"n_samples": -1}, EINVAL), ({"dx": A}, EINVAL), ({"dx": B}, EINVAL), ({"dbias": A}, EINVAL), ({"dbias": E}, EINVAL),
        ({"dy_ld": 2}, EINVAL), ({"x_off": 1}, EINVAL)],
}


def test_the_tables_match_the_signatures():
    for name, good in GOOD.items():
        assert len(good) == len(_lib.SIGNATURES[name][1]), name
        names = [arg for arg, _ in good]
        assert all(k in names for changes, _ in CASES[name] for k in changes), name


@pytest.mark.parametrize("name", sorted(GOOD))
def test_argument_checks(name):
    lib = _lib.load()
    fn, wrong = getattr(lib, name), []
    for changes, expected in CASES[name]:
        rc = fn(*[changes.get(arg, good) for arg, good in GOOD[name]])
        message = lib.fv3hip_last_error()
        if rc != expected or not message:
            wrong.append((changes, rc, expected, message))
    assert not wrong, wrong


def test_refusals_name_the_offending_value():
    lib = _lib.load()
    spoil = lambda name, **changes: getattr(lib, name)(*[changes.get(arg, good) for arg, good in GOOD[name]])   # noqa: E731
    assert spoil("fv3hip_cyclegan_train_backward_data", kind=REGULAR, k=7, n=2) == EINVAL
    assert b"halo (3 cells) is wider than the face (2)" in lib.fv3hip_last_error()
    assert spoil("fv3hip_cyclegan_train_backward_weight", kind=STRIDED, k=5) == EUNSUPPORTED
    assert b"k = 5" in lib.fv3hip_last_error()
    assert spoil("fv3hip_cyclegan_train_conv", kind=STRIDED, k=5) == EUNSUPPORTED
    assert b"k = 5" in lib.fv3hip_last_error()


def test_the_inference_entry_point_still_refuses_the_3x3_strided_convolution():
    """A guard, not a test of the new code: the 3 x 3 strided kind went into the kernel that ``fv3hip_cyclegan_conv`` launches
    too, and that entry point must go on refusing it with the message it had."""
    lib = _lib.load()
    rc = lib.fv3hip_cyclegan_conv(A, 3, 0, 0, None, None, None, 0, B, None, None, D, 5, 0, 0, 2, 8, 3, 5, STRIDED, 3, CUBE, None)
    assert rc == EUNSUPPORTED and b"k = 4, got 3" in lib.fv3hip_last_error()


def test_workspace_queries():
    lib, S, n, ci, co = _lib.load(), 3, 12, 20, 70
    chunk = lib.fv3hip_cyclegan_train_chunk_cells()
    assert chunk == 512
    data = lib.fv3hip_cyclegan_train_backward_data_workspace_bytes
    assert data(S, n, ci, REGULAR, 7, CUBE) == S * 6 * 18 * 18 * ci * 4        # the padded field, halo 3
    assert data(S, n, ci, STRIDED, 3, CUBE) == data(S, n, ci, TRANSPOSED, 4, CUBE) == S * 6 * 14 * 14 * ci * 4
    assert data(S, n, ci, REGULAR, 7, ZEROS) == 0 and data(S, n, ci, REGULAR, 4, CUBE) == 0
    weight = lib.fv3hip_cyclegan_train_backward_weight_workspace_bytes
    chunks = lambda rows: -(-rows // chunk)   # noqa: E731
    assert weight(S, n, ci, co, REGULAR, 3) == chunks(S * 864) * (9 * ci + 2) * co * 4    # per chunk dW and one float64 per channel
    assert weight(S, n, ci, co, STRIDED, 4) == chunks(S * 216) * (16 * ci + 2) * co * 4      # rows: the output cells
    assert weight(S, n, ci, co, TRANSPOSED, 4) == chunks(S * 864) * (16 * ci + 2) * co * 4   # rows: the input cells
    assert weight(S, n, ci, co, STRIDED, 5) == 0


# -- the trainer against the reference's own (tests/golden/make_cyclegan_train_golden.py) ---------------------------------
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_discriminator_twin_reproduces_the_reference(golden):
    from fv3net_amd import fit

    for key in "ab":
        twin = fit.DiscriminatorTwin(3, 12, n_convolutions=2, max_filters=8, strided_kernel_size=3, use_geographic_embedded_bias=True,
                                     lon=golden["lon"], xyz=golden["xyz"])
        prefix = f"state0.discriminator_{key}."
        twin.load_state_dict({k[len(prefix):]: torch.from_numpy(v).float() for k, v in golden.items() if k.startswith(prefix)}, strict=True)
        time, state = torch.from_numpy(golden["disc.time"]), torch.from_numpy(golden["disc.state"])
        truth, want = golden[f"disc.out_{key}"], golden[f"disc.out32_{key}"]
        with torch.no_grad():
            got32 = twin(time.float(), state.float()).numpy()
        # the gate of test_host_cyclegan.py: two float32 evaluations may differ by twice what one differs from float64
        scale = np.max(np.abs(truth))
        own = np.max(np.abs(want.astype(np.float64) - truth)) / scale
        diff = np.max(np.abs(got32 - want)) / scale
        print(f"discriminator_{key}: twin - reference {diff:.2e} of the scale (reference float32 - float64: {own:.2e})")
        assert got32.shape == truth.shape == (2, 6, 1, 3, 3) and diff <= 2 * own
        twin.double()
        twin.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith(prefix)}, strict=True)
        with torch.no_grad():
            got64 = twin(time, state).numpy()
        assert np.max(np.abs(got64 - truth)) <= 1e-12 * scale


def two_reference_steps(golden):
    from fv3net_amd.fit import cyclegan_train as ct

    state0 = {k[len("state0."):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith("state0.")}
    random.seed(0)
    trainer = fixture_config().build(3, 12, 2, golden["lon"], golden["xyz"], backend="torch", dtype=torch.float64, state_dict=state0)
    assert all(torch.equal(v, state0[k]) for k, v in trainer.state_dict().items()) and set(trainer.state_dict()) == set(state0)
    losses = []
    for step in range(2):
        batch = lambda d: (torch.from_numpy(golden[f"time_{d}"][step]), torch.from_numpy(golden[f"real_{d}"][step]))   # noqa: E731
        losses.append(trainer.train_on_batch(batch("a"), batch("b")))
        assert tuple(losses[-1]) == ct.LOSS_KEYS == tuple(golden["loss_keys"])
    return state0, trainer, losses


def test_torch_trainer_reproduces_the_losses_of_two_reference_steps_in_float64(golden):
    state0, _, losses = two_reference_steps(golden)
    for step in range(2):
        for value, want in zip(losses[step].values(), golden["losses"][step]):
            assert abs(value - want) <= 1e-10 * abs(want), (step, losses[step], golden["losses"][step])
    # ConvTranspose2d keeps torch's default initialisation, Conv2d is N(0, 0.02) with zero bias (the embedded biases were drawn)
    up = state0["generator_a_to_b._main.1._up.conv_block.0.1.0._wrapped.weight"]
    down = state0["generator_a_to_b._main.1._down.conv_block.0.1._wrapped.weight"]
    assert 0.015 < float(down.std()) < 0.025 and float(up.abs().max()) > 0.1


def test_torch_trainer_reproduces_every_parameter_after_two_reference_steps_in_float64(golden):
    """Every parameter after step 2 within 1e-9 of its own max-norm -- the 18 ``Conv2d`` biases that feed an instance norm
    and start at zero included (of the 22 biases with a mathematically zero gradient; the four ``ConvTranspose2d`` ones keep
    torch's non-zero default), which hold nothing but amplified rounding noise (max-norms 3e-13 ...
    5e-12).  Those follow the reference only if every gradient does to the last bit, which is what
    ``append_halos_tensor_reference_order`` is for: with the batched ``append_halos_tensor`` in the twins they were off by
    0.2 ... 2.2 of their max-norm (and 5 of 62 tensors bitwise equal after one step); with it a step is bitwise the
    reference's."""
    _, trainer, _ = two_reference_steps(golden)
    worst = {}
    for key, value in trainer.state_dict().items():
        want = golden[f"state2.{key}"]
        worst[key] = float(np.max(np.abs(value.numpy() - want)) / np.max(np.abs(want)))
    missed = {k: v for k, v in worst.items() if v > 1e-9}
    print(f"{len(missed)} of {len(worst)} tensors beyond 1e-9 of their max-norm; the others' worst: "
          f"{max(v for k, v in worst.items() if k not in missed):.1e}")
    assert not missed, missed


def test_validation_pass_changes_nothing(golden):
    state0 = {k[len("state0."):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith("state0.")}
    trainer = fixture_config().build(3, 12, 2, golden["lon"], golden["xyz"], dtype=torch.float64, state_dict=state0)
    batch = lambda d: (torch.from_numpy(golden[f"time_{d}"][0]), torch.from_numpy(golden[f"real_{d}"][0][:1]))   # noqa: E731
    first = (golden["time_a"][0][:1], golden["real_a"][0][:1]), (golden["time_b"][0][:1], golden["real_b"][0][:1])
    losses = trainer.train_on_batch(*first, training=False)    # a batch smaller than samples_per_batch
    assert len(losses) == 9 and all(np.isfinite(v) for v in losses.values())
    assert all(torch.equal(v, state0[k]) for k, v in trainer.state_dict().items())
    assert trainer.fake_a_buffer.num_imgs == 0


def test_both_backends_start_from_the_same_seeded_parameters(golden):
    a = fixture_config().build(3, 12, 2, golden["lon"], golden["xyz"], seed=5).state_dict()
    b = fixture_config().build(3, 12, 2, golden["lon"], golden["xyz"], seed=5).state_dict()
    c = fixture_config().build(3, 12, 2, golden["lon"], golden["xyz"], seed=6).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a) and not all(torch.equal(a[k], c[k]) for k in a)
    assert all(float(v.abs().max()) == 0 for k, v in a.items() if k.endswith("_wrapped.bias") and "_up." not in k)


def test_image_pool():
    from fv3net_amd.fit import cyclegan_train as ct

    pool = ct.ImagePool(50)
    image = lambda i: (torch.tensor([float(i)]), torch.full((1, 6, 1, 2, 2), float(i)))   # noqa: E731
    for i in range(50):    # fewer than 50 queries return the input
        time, img = pool.query(image(i))
        assert float(time) == i and float(img.flatten()[0]) == i
    for seed in (0, 1, 7):
        pool = ct.ImagePool(50)
        for i in range(25):
            pool.query((torch.tensor([2.0 * i, 2.0 * i + 1]), torch.stack([image(2 * i)[1][0], image(2 * i + 1)[1][0]])))
        random.seed(seed)
        got = [pool.query(image(100 + q)) for q in range(10)]           # queries 51 - 60
        random.seed(seed)
        held = list(range(50))                                           # a direct replay of the reference's rule
        for q, (time, img) in enumerate(got):
            if random.uniform(0, 1) > 0.5:
                slot = random.randint(0, 49)
                want, held[slot] = held[slot], 100 + q
            else:
                want = 100 + q
            assert float(time) == want and torch.all(img == want), (seed, q)   # times travel with images


def test_configurations_refuse_what_is_not_built():
    from fv3net_amd import fit
    from fv3net_amd.fit import cyclegan_train as ct

    with pytest.raises(ValueError, match="no fields \\['n_resnets'\\]"):
        fixture_config(generator=dict(n_resnets=2))
    with pytest.raises(ValueError, match="no fields \\['epochs'\\]"):
        ct.CycleGANHyperparameters(["a"], training=dict(epochs=3))
    with pytest.raises(ValueError, match="no fields \\['bogus'\\]"):
        ct.CycleGANHyperparameters(["a"], network=dict(bogus=1))
    with pytest.raises(ValueError, match="loss_type must be 'mse' or 'mae', got 'huber'"):
        fixture_config(gan_loss=dict(loss_type="huber"))
    with pytest.raises(ValueError, match="convolution_type wrapped_conv2d not supported"):
        fixture_config(convolution_type="wrapped_conv2d")
    with pytest.raises(ValueError, match="input edge of 3 cells"):
        fit.DiscriminatorTwin(3, 12, n_convolutions=3, max_filters=8, use_geographic_features=False)
    with pytest.raises(NotImplementedError, match="strided_kernel_size = 5"):
        fit.DiscriminatorTwin(3, 12, n_convolutions=2, max_filters=8, strided_kernel_size=5, use_geographic_features=False)
    with pytest.raises(NotImplementedError, match="kernel_size = 4"):
        fit.DiscriminatorTwin(3, 12, n_convolutions=2, max_filters=8, kernel_size=4, use_geographic_features=False)
    with pytest.raises(ValueError, match="backend must be"):
        fixture_config().build(3, 12, 2, backend="triton", lon=np.zeros((6, 12, 12)), xyz=np.zeros((6, 3, 12, 12)))
    defaults = ct.CycleGANHyperparameters(["a"])
    assert (defaults.normalization_fit_samples, defaults.training.n_epoch, defaults.training.samples_per_batch) == (50_000, 20, 1)
    assert defaults.network.convolution_type == "conv2d" and defaults.network.optimizer.name == "Adam"
    assert defaults.network.discriminator.strided_kernel_size == 3 and defaults.network.generator.strided_kernel_size == 4
    assert defaults.variables == ("a", "time")


def same_files(a, b):
    import filecmp

    return sorted(os.listdir(a)) == sorted(os.listdir(b)) and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False)
                                                                   for f in os.listdir(a))


def test_train_cyclegan_with_the_torch_backend(tmp_path):
    import cyclegan_cases as cc
    from fv3net_amd import fit
    from fv3net_amd.fit import cyclegan_train as ct

    lon, xyz = cc.synthetic_grid(12)
    batches = training_batches()
    random.seed(0)
    model = fit.train_cyclegan(training_hyperparameters(checkpoint_path=str(tmp_path / "checkpoints")), batches, batches[:1], lon=lon, xyz=xyz)
    assert isinstance(model, fit.HipCycleGAN)
    assert set(model.history) == set(ct.LOSS_KEYS) | {f"val_{k}" for k in ct.LOSS_KEYS}
    assert all(len(v) == 1 and np.isfinite(v[0]) for v in model.history.values())
    assert os.listdir(tmp_path / "checkpoints") == ["epoch_000"]
    # the artifact round-trips with its discriminators
    fit.dump(model, str(tmp_path / "a"))
    loaded = fit.load(str(tmp_path / "a"))
    fit.dump(loaded, str(tmp_path / "b"))
    assert same_files(tmp_path / "a", tmp_path / "b") and same_files(tmp_path / "a", tmp_path / "checkpoints" / "epoch_000")
    assert len(loaded.discriminators["state_dict"]) == 18 and loaded.discriminators["config"]["strided_kernel_size"] == 3
    # an artifact without discriminators is written byte for byte as before
    golden_dir = os.path.join(os.path.dirname(GOLDEN), "cyclegan_reference")
    old = fit.load(golden_dir)
    assert old.discriminators is None
    fit.dump(old, str(tmp_path / "old"))
    assert all(filecmp_equal(os.path.join(golden_dir, f), tmp_path / "old" / f) for f in os.listdir(tmp_path / "old"))
    # reload_path resumes from bitwise-equal parameters and the same scalers
    hp = training_hyperparameters()
    hp.training.n_epoch, hp.reload_path = 0, str(tmp_path / "a")
    resumed = fit.train_cyclegan(hp, batches)
    (_, a), (_, b) = model.spec.to_arrays(), resumed.spec.to_arrays()
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(np.array_equal(v, resumed.discriminators["state_dict"][k]) for k, v in model.discriminators["state_dict"].items())
    with pytest.raises(ValueError, match="holds no CycleGAN with its discriminators"):
        hp.reload_path = golden_dir
        fit.train_cyclegan(hp, batches)


def filecmp_equal(a, b):
    import filecmp

    return filecmp.cmp(str(a), str(b), shallow=False)


def test_reference_order_is_a_switch_that_only_the_trainer_turns_on(golden):
    from fv3net_amd import fit
    from fv3net_amd.fit.cyclegan import _AppendHalos, set_reference_order_gradients

    pads = lambda net: [m.reference_order_gradients for m in net.modules() if isinstance(m, _AppendHalos)]   # noqa: E731
    twin = fit.GeneratorTwin(3, 12, 2, 2, max_filters=12, lon=golden["lon"], xyz=golden["xyz"])
    assert len(pads(twin)) == 10 and not any(pads(twin))                       # an existing twin pads as it always did
    on = fixture_config().build(3, 12, 2, golden["lon"], golden["xyz"])
    off = fixture_config().build(3, 12, 2, golden["lon"], golden["xyz"], reference_order_gradients=False)
    assert all(all(pads(t)) for t in on.twins.values()) and not any(any(pads(t)) for t in off.twins.values())
    x, time = torch.from_numpy(golden["real_a"][0][:, 0]).float(), torch.from_numpy(golden["time_a"][0].reshape(-1)).float()
    with torch.no_grad():
        before = twin(time, x)
        assert torch.equal(set_reference_order_gradients(twin)(time, x), before)   # the same values either way


@pytest.mark.parametrize("n,h", [(12, 1), (12, 3), (4, 3), (3, 1), (5, 2)])
def test_reference_order_halos(n, h):
    """The values of ``append_halos_tensor``; the gradient the same sum in another order: equal on integers, within an ulp
    per term otherwise, and -- what the order is for -- handed to the input tile by tile, after whatever else reads it."""
    from fv3net_amd.cubedsphere.halos import append_halos_tensor, append_halos_tensor_reference_order

    rng = np.random.default_rng(n + h)
    for integers in (True, False):
        draw = (lambda *s: rng.integers(-3, 4, s).astype(np.float64)) if integers else (lambda *s: rng.normal(0, 1, s))
        x, d = torch.from_numpy(draw(6, 2, 3, n, n)), torch.from_numpy(draw(6, 2, 3, n + 2 * h, n + 2 * h))
        grads = []
        for pad in (append_halos_tensor, append_halos_tensor_reference_order):
            leaf = x.clone().requires_grad_()
            out = pad(leaf, h)
            out.backward(d)
            grads.append(leaf.grad)
            assert torch.equal(out, append_halos_tensor(x, h))
        if integers:
            assert torch.equal(grads[0], grads[1])
        else:
            assert float((grads[0] - grads[1]).abs().max()) <= 4 * 2.0 ** -52 * float(d.abs().max())
    # tiles along another dimension, as the twins hold them
    leaf = x.movedim(0, 1).clone().requires_grad_()
    out = append_halos_tensor_reference_order(leaf, h, tile_dim=1)
    assert torch.equal(out.movedim(1, 0), append_halos_tensor(x, h))
    out.backward(d.movedim(0, 1))
    assert torch.equal(leaf.grad.movedim(1, 0), grads[1])
    with pytest.raises(ValueError, match="six tiles"):
        append_halos_tensor_reference_order(x[:5], h)
