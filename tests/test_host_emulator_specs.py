"""The emulator's Python layer where it needs no GPU: the saved-model format (tests/golden/emulator_specs/, written once by
tests/golden/make_emulator_specs.py -- files like the ones users have on disk), the defaults filled in for files that lack
an optional key, every ``validate()`` rule of the four spec classes, the source / output name lists, and how ``HipEmulator``
chooses its arithmetic (its model is built lazily)."""
import copy
import os

import numpy as np
import pytest
import yaml

from fv3net_amd.emulation.models import HipEmulator, HipLocalEmulator, load_emulator
from fv3net_amd.local_mlp import ConditionalScale, HybridRnnSpec, LocalInput, LocalMlpSpec, LocalOutput, RnnLayer, RnnSpec
from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec, ResidualSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emulator_specs")
NAMES = {"dense": MlpSpec, "dense_local": LocalMlpSpec, "rnn_v1": RnnSpec, "hybrid_rnn": HybridRnnSpec}


def _files(path):
    with open(os.path.join(path, "spec.yaml")) as f:
        meta = yaml.safe_load(f)
    with np.load(os.path.join(path, "weights.npz"), allow_pickle=False) as z:
        return meta, {k: z[k] for k in z.files}


def _same_arrays(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape, k
        assert g.tobytes() == w.tobytes(), k


def _golden(name):
    return load_emulator(os.path.join(GOLDEN, name)).spec


# -- a. the format ------------------------------------------------------------------------------------------------------------

def test_the_goldens_hold_what_they_are_meant_to_cover():
    metas = {name: _files(os.path.join(GOLDEN, name)) for name in NAMES}
    assert "architecture" not in metas["dense"][0]
    assert [metas[n][0]["architecture"] for n in ("dense_local", "rnn_v1", "hybrid_rnn")] == ["dense-local", "rnn-v1-shared-weights", "rnn"]
    meta, arrays = metas["dense_local"]
    # centre and scale, centre only, scale only, neither; scalar ([1]) and per-level ([3]) tables
    have = [(f"in{n}_center" in arrays, f"in{n}_scale" in arrays) for n in range(4)]
    assert have == [(True, True), (True, False), (False, True), (False, False)]
    assert {arrays[k].shape for k in ("in0_center", "in0_scale", "in1_center", "in2_scale")} == {(1,), (3,)}
    assert meta["inputs"][1]["transform"] == "log" and meta["inputs"][1]["eps"] == 1e-8
    out = meta["outputs"][0]
    assert out["conditional"] == {"name": "dq", "on": "T", "min_scale": 0.1} and (out["after"], out["before"]) == ("q_after", "q")
    assert out["value_limit"] == [None, 0.0] and out["after_limit"] == [0.0, None]
    assert meta["outputs"][1]["channels"] == 3
    assert [o["single_level"] for o in metas["rnn_v1"][0]["outputs"]] == [True, False] and metas["rnn_v1"][0]["n_rnn"] == 2
    meta = metas["hybrid_rnn"][0]
    assert meta["go_backwards"] is False and meta["head"]["n_hidden"] == 0 and len(meta["head"]["residuals"]) == 1
    meta, arrays = metas["dense"]
    assert meta["hidden_output"] == "hidden" and meta["inputs"][1]["start"] == 1 and arrays["in2_scale"].shape == ()
    assert meta["outputs"] == [{"name": "dQ1", "nfeat": 3, "min": -1.0, "max": 2.0}, {"name": "rain", "nfeat": 1, "min": None, "max": None}]
    assert "out0_mask" in arrays and not any(k.startswith("out1_") for k in arrays)


@pytest.mark.parametrize("name", NAMES)
def test_saved_format_is_pinned(name, tmp_path):
    """What the loaded spec serialises to is the file: the parsed yaml, and the npz's keys, dtypes, shapes and bits; a dump of
    it loads to the same again."""
    path = os.path.join(GOLDEN, name)
    meta, arrays = _files(path)
    emulator = load_emulator(path)
    assert type(emulator) is (HipEmulator if name == "dense" else HipLocalEmulator) and type(emulator.spec) is NAMES[name]
    emulator.spec.validate()
    got_meta, got_arrays = emulator.spec.to_arrays()
    assert got_meta == meta
    _same_arrays(got_arrays, arrays)
    emulator.dump(str(tmp_path / "again"))
    assert sorted(os.listdir(tmp_path / "again")) == ["spec.yaml", "weights.npz"]
    meta2, arrays2 = _files(str(tmp_path / "again"))
    assert meta2 == meta
    _same_arrays(arrays2, arrays)
    got_meta, got_arrays = load_emulator(str(tmp_path / "again")).spec.to_arrays()
    assert got_meta == meta
    _same_arrays(got_arrays, arrays)
    assert type(emulator).load(path).spec.to_arrays()[0] == meta


# -- b. files written before a key existed ---------------------------------------------------------------------------------------

# optional key -> what a file without it serialises to after loading
DEFAULTS = {"transform": "none", "eps": 0.0, "start": 0, "channels": 1, "value_limit": [None, None], "after_limit": [None, None],
            "single_level": False, "go_backwards": True, "residuals": [], "activation": "relu", "hidden_output": None}


def _paths(node, here=()):
    """Every (path to a dict, optional key in it) of a meta."""
    if isinstance(node, dict):
        for k, v in node.items():
            if k in DEFAULTS or k == "architecture":
                yield here, k
            yield from _paths(v, here + (k,))
    elif isinstance(node, list):
        for n, v in enumerate(node):
            yield from _paths(v, here + (n,))


def _at(node, path):
    for p in path:
        node = node[p]
    return node


def test_missing_optional_keys_get_the_defaults():
    seen = set()
    for name, cls in NAMES.items():
        meta, arrays = _files(os.path.join(GOLDEN, name))
        for path, key in _paths(meta):
            old = copy.deepcopy(meta)
            del _at(old, path)[key]
            want = copy.deepcopy(meta)
            if key != "architecture":  # (a spec class writes its own; which class reads a file is load_emulator's choice, below)
                _at(want, path)[key] = DEFAULTS[key]
            spec = cls.from_arrays(old, arrays)
            assert spec.to_arrays()[0] == want, (name, path, key)
            seen.add(key)
    assert seen == set(DEFAULTS) | {"architecture"}
    # the defaults as the spec objects hold them
    meta, arrays = _files(os.path.join(GOLDEN, "dense_local"))
    for m in meta["inputs"] + meta["outputs"]:
        for key in ("transform", "eps", "channels", "value_limit", "after_limit", "single_level"):
            m.pop(key, None)
    spec = LocalMlpSpec.from_arrays(meta, arrays)
    assert [(i.transform, i.eps) for i in spec.inputs] == [("none", 0.0)] * 4
    assert [(o.channels, o.value_limit, o.after_limit, o.single_level) for o in spec.outputs] == [(1, (None, None), (None, None), False)] * 2
    meta, arrays = _files(os.path.join(GOLDEN, "hybrid_rnn"))
    del meta["go_backwards"], meta["head"]["residuals"], meta["head"]["activation"], meta["head"]["hidden_output"], meta["head"]["inputs"][0]["start"]
    spec = HybridRnnSpec.from_arrays(meta, arrays)
    assert spec.go_backwards is True and spec.head.residuals == [] and spec.head.activation == "relu"
    assert spec.head.hidden_output is None and spec.head.inputs[0].start == 0


def test_a_file_without_architecture_is_a_dense_emulator(tmp_path):
    meta, _ = _files(os.path.join(GOLDEN, "dense"))
    assert "architecture" not in meta
    emulator = load_emulator(os.path.join(GOLDEN, "dense"))
    assert type(emulator) is HipEmulator
    for arch in ("dense", "linear"):
        emulator.dump(str(tmp_path / arch))
        with open(tmp_path / arch / "spec.yaml", "w") as f:
            yaml.safe_dump({**meta, "architecture": arch}, f)
        again = load_emulator(str(tmp_path / arch))
        assert type(again) is HipEmulator and again.spec.to_arrays()[0] == meta
    # "rnn-v1" reads as "rnn-v1-shared-weights" does
    rnn = load_emulator(os.path.join(GOLDEN, "rnn_v1"))
    rnn.dump(str(tmp_path / "rnn"))
    rnn_meta, rnn_arrays = _files(str(tmp_path / "rnn"))
    with open(tmp_path / "rnn" / "spec.yaml", "w") as f:
        yaml.safe_dump({**rnn_meta, "architecture": "rnn-v1"}, f)
    again = load_emulator(str(tmp_path / "rnn"))
    assert type(again.spec) is RnnSpec and again.spec.to_arrays()[0] == rnn_meta
    _same_arrays(again.spec.to_arrays()[1], rnn_arrays)


# -- c. validate(): one row per raise ----------------------------------------------------------------------------------------------

def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


def _swap_inputs(s):
    s.inputs[0], s.inputs[1] = s.inputs[1], s.inputs[0]


Z = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731

VALIDATE = [
    # MlpSpec (9 network inputs, two hidden layers of 6, 4 output features)
    ("dense", lambda s: s.hidden_biases.pop(), "hidden_kernels and hidden_biases differ in length"),
    ("dense", lambda s: _set(s, activation="tanh"), "activation must be 'relu' or 'linear', got 'tanh'"),
    ("dense", lambda s: _set(s, hidden_kernels=[], hidden_biases=[]), "hidden_output needs a hidden layer"),
    ("dense", lambda s: s.hidden_kernels.__setitem__(0, Z(8, 6)), "first kernel has shape (8, 6), expected (9, 6)"),
    ("dense", lambda s: s.hidden_biases.__setitem__(0, Z(5)), "first bias has shape (5,), expected (6,)"),
    ("dense", lambda s: s.hidden_kernels.__setitem__(1, Z(6, 5)), "hidden layers must all have the same width"),
    ("dense", lambda s: s.hidden_biases.__setitem__(1, Z(5)), "hidden layers must all have the same width"),
    ("dense", lambda s: _set(s, out_kernel=Z(6, 3)), "output kernel has shape (6, 3), expected (6, 4)"),
    ("dense", lambda s: _set(s, out_bias=Z(3)), "output kernel has shape (6, 4), expected (6, 4)"),
    ("dense", lambda s: _set(s.residuals[0], output="nope"), "residual 'T_after' refers to unknown output 'nope'"),
    # LocalMlpSpec (4 inputs, one hidden layer of 6, 1 + 3 channels)
    ("dense_local", _swap_inputs, "inputs must be listed sorted by their network name (combine_sequence_inputs)"),
    ("dense_local", lambda s: _set(s, hidden_kernels=[], hidden_biases=[]), "at least one hidden layer, one bias per kernel"),
    ("dense_local", lambda s: s.hidden_biases.append(Z(6)), "at least one hidden layer, one bias per kernel"),
    ("dense_local", lambda s: s.hidden_kernels.__setitem__(0, Z(5, 6)), "first kernel has 5 rows, the model has 4 inputs"),
    ("dense_local", lambda s: _set(s, out_kernel=Z(6, 5)), "output kernel has shape (6, 5), expected (6, 4)"),
    ("dense_local", lambda s: _set(s, out_bias=Z(5)), "output kernel has shape (6, 4), expected (6, 4)"),
    ("dense_local", lambda s: _set(s.outputs[1], scale=np.float32(2)), "multi-channel output 'classes' must be unscaled"),
    ("dense_local", lambda s: _set(s.outputs[1], conditional=s.outputs[0].conditional), "multi-channel output 'classes' must be unscaled"),
    ("dense_local", lambda s: _set(s.outputs[1], after="a", before="T"), "multi-channel output 'classes' must be unscaled"),
    ("dense_local", lambda s: _set(s.outputs[0], before=None), "output 'dq_tscaled': 'after' and 'before' go together"),
    ("dense_local", lambda s: _set(s.outputs[0], after=None), "output 'dq_tscaled': 'after' and 'before' go together"),
    # RnnSpec (3 inputs, two layers of 4 channels, 2 outputs)
    ("rnn_v1", _swap_inputs, "inputs must be listed sorted by their network name (combine_sequence_inputs)"),
    ("rnn_v1", lambda s: _set(s, layers=[]), "at least one recurrent layer"),
    ("rnn_v1", lambda s: _set(s.layers[0], kernel=Z(2, 4)),
     "recurrent layer 0: kernel (2, 4), recurrent kernel (4, 4), bias (4,) do not fit 3 inputs"),
    ("rnn_v1", lambda s: _set(s.layers[1], recurrent_kernel=Z(4, 5)),
     "recurrent layer 1: kernel (4, 4), recurrent kernel (4, 5), bias (4,) do not fit 4 inputs"),
    ("rnn_v1", lambda s: _set(s.layers[1], bias=Z(5)), "recurrent layer 1: kernel (4, 4), recurrent kernel (4, 4), bias (5,) do not fit 4 inputs"),
    ("rnn_v1", lambda s: _set(s.layers[1], kernel=Z(4, 5), recurrent_kernel=Z(5, 5), bias=Z(5)), "output kernel has shape (4, 2), expected (5, 2)"),
    ("rnn_v1", lambda s: _set(s, out_bias=Z(3)), "output kernel has shape (4, 2), expected (4, 2)"),
    ("rnn_v1", lambda s: (_set(s.outputs[0], channels=2), _set(s, out_kernel=Z(4, 3), out_bias=Z(3))), "multi-channel outputs are not supported by the RNN architectures here"),
    ("rnn_v1", lambda s: _set(s.outputs[1], before=None), "output 'cloud_difference': 'after' and 'before' go together"),
    ("rnn_v1", lambda s: _set(s.outputs[0], after="a", before="c"), "single-level output 'total_precipitation' cannot carry level-wise transforms"),
    ("rnn_v1", lambda s: _set(s.outputs[0], conditional=ConditionalScale("u", "T", Z(2), Z(2), Z(2))),
     "single-level output 'total_precipitation' cannot carry level-wise transforms"),
    # HybridRnnSpec (2 inputs, 5 channels, a head without hidden layers)
    ("hybrid_rnn", _swap_inputs, "inputs must be listed sorted by their network name (combine_sequence_inputs)"),
    ("hybrid_rnn", lambda s: _set(s.rnn, kernel=Z(3, 5)), "recurrent layer: kernel (3, 5), recurrent kernel (5, 5), bias (5,) do not fit 2 inputs"),
    ("hybrid_rnn", lambda s: _set(s.rnn, recurrent_kernel=Z(5, 4)), "recurrent layer: kernel (2, 5), recurrent kernel (5, 4), bias (5,) do not fit 2 inputs"),
    ("hybrid_rnn", lambda s: _set(s.rnn, bias=Z(4)), "recurrent layer: kernel (2, 5), recurrent kernel (5, 5), bias (4,) do not fit 2 inputs"),
    ("hybrid_rnn", lambda s: _set(s.head.inputs[0], source="T"), "the head's only input must be the 5 features of 'rnn_state'"),
    ("hybrid_rnn", lambda s: _set(s.head.inputs[0], start=1), "the head's only input must be the 5 features of 'rnn_state'"),
    ("hybrid_rnn", lambda s: s.head.inputs.append(InputSpec("T", 3)), "the head's only input must be the 5 features of 'rnn_state'"),
    ("hybrid_rnn", lambda s: _set(s.head, hidden_output="h"), "the head returns outputs, not its hidden layer"),
    ("hybrid_rnn", lambda s: _set(s.head.residuals[0], source="rnn_state"), "a residual cannot be added to the recurrent state"),
    ("hybrid_rnn", lambda s: _set(s.head, out_bias=Z(3)), "output kernel has shape (5, 4), expected (5, 4)"),  # (the head's own rules)
]


@pytest.mark.parametrize("name,mutate,message", VALIDATE, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(VALIDATE)])
def test_validate_refuses(name, mutate, message):
    spec = _golden(name)
    spec.validate()
    mutate(spec)
    with pytest.raises(ValueError) as info:
        spec.validate()
    assert message in str(info.value)


# -- d. sources and output names -----------------------------------------------------------------------------------------------------

def test_sources_and_output_names_keep_first_seen_order_without_duplicates():
    spec = _golden("dense")  # T twice as an input and as a residual's source
    assert spec.sources == ["T", "q", "p"] and spec.output_names == ["dQ1", "rain", "T_after", "hidden"]
    assert spec.source_nfeat() == {"T": 3, "q": 3, "p": 1}
    spec.residuals.append(ResidualSpec("r", "extra", "rain"))
    assert spec.sources == ["T", "q", "p", "extra"] and spec.source_nfeat()["extra"] == 1
    spec = _golden("dense_local")  # T: two inputs and the conditional's `on`; q: an input and `before`
    assert spec.sources == ["T", "q", "p"] and spec.output_names == ["dq_tscaled", "dq", "q_after", "classes"]
    assert spec.n_channels == 4
    spec.outputs[0].conditional.on, spec.outputs[0].before = "on", "base"
    assert spec.sources == ["T", "q", "p", "on", "base"]
    spec = _golden("rnn_v1")  # c: an input and `before`
    assert spec.sources == ["c", "q", "T"] and spec.output_names == ["total_precipitation", "cloud_difference", "cloud_after"]
    assert spec.n_channels == 2
    spec = _golden("hybrid_rnn")  # T: an input and the head's residual source; the state is no source of the call
    assert spec.sources == ["q", "T"] and spec.output_names == ["dT", "total_precipitation", "T_after"]
    spec.head.residuals += [ResidualSpec("p2", "extra", "total_precipitation"), ResidualSpec("p3", "q", "total_precipitation")]
    assert spec.sources == ["q", "T", "extra"] and spec.output_names[-2:] == ["p2", "p3"]
    emulator = HipLocalEmulator(spec)
    assert emulator.input_variables == spec.sources and emulator.output_variables == spec.output_names


# -- e. the emulator objects ---------------------------------------------------------------------------------------------------------

def test_hip_emulator_arithmetic_choice(monkeypatch):
    spec = _golden("dense")
    monkeypatch.delenv(HipEmulator.ARITHMETIC_ENV, raising=False)
    assert HipEmulator.ARITHMETIC_ENV == "FV3NET_AMD_EMULATOR_ARITHMETIC"
    assert HipEmulator(spec).arithmetic == "fp32"
    assert HipEmulator(spec, arithmetic="split-bf16").arithmetic == "split-bf16"
    monkeypatch.setenv(HipEmulator.ARITHMETIC_ENV, "split-bf16")
    assert HipEmulator(spec).arithmetic == "split-bf16"
    assert HipEmulator(spec, arithmetic="fp32").arithmetic == "fp32"
    with pytest.raises(ValueError) as info:
        HipEmulator(spec, arithmetic="bf16")
    assert str(info.value) == "arithmetic must be 'fp32' or 'split-bf16', got 'bf16'"
    monkeypatch.setenv(HipEmulator.ARITHMETIC_ENV, "fp16")
    with pytest.raises(ValueError) as info:
        HipEmulator(spec)
    assert str(info.value) == "arithmetic must be 'fp32' or 'split-bf16', got 'fp16'"
    assert HipEmulator(spec, arithmetic="fp32").arithmetic == "fp32"  # (the argument is looked at first)
    emulator = HipEmulator(spec, inputs_to_ignore=["rank"], arithmetic="fp32")
    assert emulator.inputs_to_ignore == ("rank",) and emulator.device_resident
    assert emulator.input_variables == ["T", "q", "p"] and emulator.output_variables == ["dQ1", "rain", "T_after", "hidden"]


def test_load_emulator_refusals(tmp_path):
    load_emulator(os.path.join(GOLDEN, "dense")).dump(str(tmp_path / "m"))
    meta, _ = _files(str(tmp_path / "m"))
    with open(tmp_path / "m" / "spec.yaml", "w") as f:
        yaml.safe_dump({**meta, "architecture": "transformer"}, f)
    with pytest.raises(NotImplementedError) as info:
        load_emulator(str(tmp_path / "m"))
    assert str(info.value) == ("architecture 'transformer' is not implemented on the device "
                               "(dense, linear, dense-local, rnn, rnn-v1, rnn-v1-shared-weights are)")
    path = os.path.join(GOLDEN, "dense")
    with pytest.raises(TypeError) as info:
        load_emulator(path, expect=HipLocalEmulator)
    assert str(info.value) == f"{path} holds a HipEmulator, not a HipLocalEmulator"
    with pytest.raises(TypeError):
        HipLocalEmulator.load(path)
    path = os.path.join(GOLDEN, "rnn_v1")
    with pytest.raises(TypeError) as info:
        load_emulator(path, expect=HipEmulator)
    assert str(info.value) == f"{path} holds a HipLocalEmulator, not a HipEmulator"
    assert type(load_emulator(path, expect=HipLocalEmulator)) is HipLocalEmulator
    assert type(HipLocalEmulator.load(path).spec) is RnnSpec


def test_the_spec_classes_name_their_architecture():
    assert (LocalMlpSpec.architecture, RnnSpec.architecture, HybridRnnSpec.architecture) == ("dense-local", "rnn-v1-shared-weights", "rnn")
    assert HybridRnnSpec.STATE == "rnn_state"
    # the dataclasses' field orders are part of the interface: the test cases build them positionally
    layer = RnnLayer(np.zeros((2, 3)), np.zeros((3, 3)), np.zeros(3))
    assert layer.kernel.shape == (2, 3) and layer.recurrent_kernel.shape == (3, 3) and layer.bias.shape == (3,)
    assert LocalInput("n", "s").transform == "none" and LocalOutput("o").channels == 1 and OutputSpec("o", 2).mask is None
