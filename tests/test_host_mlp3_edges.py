"""What tests/test_gpu_mlp3_edges.py relies on, proved without a GPU: the catalogue of tests/mlp3_cases.py selects all 16
rows of ``kMlp3Table`` (csrc/mlp_bf16x3.hip) and every run-time path inside them, its cases are conditioned for float32,
the restated dispatch refuses what the library refuses, and the tracer models of the arithmetic test tell a kernel that
keeps all six cross products from one that drops any one of them in any layer type."""
import numpy as np
import pytest

import mlp3_cases as m3
from oracle import mlp_np


def _variants():
    return {c.name: m3.variant_of(c) for c in m3.CATALOGUE}


def test_catalogue_selects_all_sixteen_rows_and_every_run_time_path():
    variants = _variants()
    assert len(m3.ALL_ROWS) == 16 and len(set(m3.ALL_ROWS)) == 16
    assert len(variants) == len(m3.CATALOGUE)  # (names are unique)
    assert {m3.row(v) for v in variants.values()} == set(m3.ALL_ROWS)
    f = {name: dict(m3.facts(v), row=m3.row(v), fast=m3.row(v).endswith(",true>"), res=",true," in m3.row(v))
         for name, v in variants.items()}
    have = lambda **kw: any(all(x[k] == v for k, v in kw.items()) for x in f.values())
    # the output paths: the vector-ALU layer with 1..4 outputs, the matrix cores, none
    assert {x["out"] for x in f.values()} == {"mfma", "none", "valu1", "valu2", "valu3", "valu4"}
    for out in ("valu4", "valu3"):
        assert have(out=out, hout="1"), out
    # no output layer and a hidden output beside an MFMA output layer (with and without residuals): both epilogues
    for fast in (True, False):
        assert have(out="none", hout="1", fast=fast)
        assert have(out="mfma", hout="1", fast=fast, res=False) and have(out="mfma", hout="1", fast=fast, res=True)
    # depth, and the two ways layer 1 requests its chunks (builtin: one hidden layer in front of an MFMA output layer only)
    assert {x["hidden"] for x in f.values()} == {"1", "2", "3"}
    assert have(layer1="builtin", hidden="1", out="mfma") and have(layer1="block", hidden="1", out="none")
    assert all((x["layer1"] == "builtin") == (x["hidden"] == "1" and x["out"] == "mfma") for x in f.values())
    ks1 = {int(x["ks1"].split("/")[0]) for x in f.values()}
    assert {1, 2, 3, 4, 64} <= ks1
    for lay in ("block", "builtin"):   # odd (the tail step) and even k-step counts on both
        got = {int(x["ks1"].split("/")[0]) % 2 for x in f.values() if x["layer1"] == lay}
        assert got == {0, 1}, lay
    assert variants["mlp3-cell-G2"].endswith("out=none hout=1 layer1=block ks1=2/0 hidden=1 xwrap=0")
    # log k-steps: none, all, some
    logs = {(int(a), int(b)) for a, b in (x["ks1"].split("/") for x in f.values())}
    assert any(b == 0 for a, b in logs) and any(a == b for a, b in logs) and any(0 < b < a for a, b in logs)
    # every sample count is small, and both a partial tile and more than one tile are there
    assert all(0 < c.n <= 700 for c in m3.CATALOGUE)


def test_catalogue_reaches_both_ends_of_every_tile_count_and_the_input_edges():
    got = {}
    for c in m3.CATALOGUE:
        g = m3.geometry3(m3.build_spec(c))
        if g["has_out"]:
            got.setdefault((g["n_ot"], bool(g["n_res"])), set()).add(g["F"])
    for key, ends in {(1, False): (5, 32), (1, True): (1, 32), (3, False): (65, 96), (3, True): (65, 96), (5, False): (129, 160),
                      (5, True): (129, 160), (13, False): (385, 416), (13, True): (385, 416)}.items():
        assert set(ends) <= got[key], (key, got[key])
    nfeat = {i[2] for c in m3.CATALOGUE for i in c.base.inputs}
    assert {1, 15, 16, 17} <= nfeat
    eps = {i[4] for c in m3.CATALOGUE for i in c.base.inputs if i[4] is not None}
    assert m3.FLT_MIN in eps and 1e-8 in eps
    # a log input listed after a plain one is moved to the front: slot 0 belongs to a later input
    spec = m3.build_spec(m3.by_name("t1-F5"))
    g = m3.geometry3(spec)
    assert spec.inputs[0].transform == "none" and spec.inputs[g["slots"][0][0]].transform == "log"
    assert g["ks_rows"] == [16, 1, 7, 3, 1] and g["n_log_ks"] == 2 and g["slots"][17:32] == [None] * 15
    # ... and the ranges of the shared source start past 0 and leave features nobody reads between them
    read = sorted(f for i in spec.inputs if i.source == "s" for f in range(i.start, i.start + i.nfeat))
    assert read[0] == 3 and 10 not in read and 11 not in read and read[-1] == 31
    # the 13-tile residual cases: the residual rows span more than 5 tiles and start in a tile other than 0
    for name in ("t13r-F385", "t13r-F416-ressrc"):
        spec = m3.build_spec(m3.by_name(name))
        f0 = sum(o.nfeat for o in spec.outputs[:[o.name for o in spec.outputs].index("y")])
        nf = next(o.nfeat for o in spec.outputs if o.name == "y")
        tiles = set(range(f0 // 32, (f0 + nf - 1) // 32 + 1))
        assert len(tiles) > 5 and 0 not in tiles, (name, tiles)


def test_each_condition_of_the_sixteen_byte_epilogue_is_broken_on_its_own():
    broken = {}
    for c in m3.CATALOGUE:
        cond = m3.fast_conditions(m3.build_spec(c), c.n, c.layout)
        bad = [k for k, v in cond.items() if not v]
        assert len(bad) <= 1, (c.name, bad)   # one at a time: the case shows that condition and no other
        if bad:
            broken.setdefault(bad[0], []).append(c.name)
            assert m3.row(m3.variant_of(c)).endswith(",false>")
    assert set(broken) == set(m3.fast_conditions(m3.build_spec(m3.CATALOGUE[0]), 4, m3.Layout())), broken
    assert {c.misalign for c in m3.CATALOGUE} == set(m3.MISALIGN)
    # the LDS budget: 13 tiles and 64 k-steps take exactly 160 KiB with one hidden layer and 1 KiB more with two
    g1 = m3.geometry3(m3.build_spec(m3.by_name("ks64-t13-exactly-160KiB")))
    g2 = m3.geometry3(m3.build_spec(m3.by_name("ks64-t13-lds-forced")))
    assert g1["lds_fast"] == m3.LDS_MAX and g2["lds_fast"] == m3.LDS_MAX + 1024 and g2["lds_bytes"] <= m3.LDS_MAX
    assert broken["LDS of the 16-byte layout <= 160 KiB"] == ["mlp3-ks64-t13-lds-forced"]
    # `fast` flips with n % 4 on an aligned call
    spec = m3.build_spec(m3.by_name("t13r-F385"))
    assert [m3.row(m3.expected_variant3(spec, n)).endswith(",true>") for n in (1, 3, 4, 5, 128, 129, 132)] == \
        [False, False, True, False, True, False, True]


def test_refusals_restated():
    for kind, specs in m3.REFUSALS.items():
        for kw in specs:
            with pytest.raises(m3.VariantRefused, match=m3.REFUSAL_MESSAGES[kind]):
                m3.geometry3(m3.refusal_spec(**kw))
    for kw in m3.ACCEPTED:
        m3.geometry3(m3.refusal_spec(**kw))
    # the smallest model whose tables exceed the LDS, from the formula: 13 tiles and 64 k-steps leave room for 20 hidden layers
    assert m3.smallest_refused_depth() == 21
    g = m3.geometry3(m3.refusal_spec(F=385, n_in=(1024,), n_hidden=20))
    assert m3.LDS_MAX - 1024 < g["lds_bytes"] <= m3.LDS_MAX


@pytest.mark.parametrize("case", m3.CATALOGUE + m3.poison_cases(), ids=lambda c: c.name)
def test_cases_are_conditioned_for_float32(case):
    """As tests/test_host_mlp_edges.py holds the fp32 kernels' cases: the float32 evaluation of the oracle is within a
    quarter of the device gate (1e-5 of a level's maximum) of the float64 one at every level."""
    spec = m3.build_spec(case)
    src = m3.make_sources(case)
    o64, o32 = mlp_np.forward(spec, src, dtype=np.float64), mlp_np.forward(spec, src, dtype=np.float32)
    assert set(o64) == set(spec.output_names)
    for name in o64:
        scale = np.max(np.abs(o64[name]), axis=0)
        err = np.max(np.abs(o32[name].astype(np.float64) - o64[name]), axis=0)
        worst = int(np.argmax(err / np.where(scale == 0, 1, scale)))
        assert np.all(err <= 2.5e-6 * scale), (case.name, name, worst, err[worst], scale[worst])


@pytest.mark.parametrize("case", m3.poison_cases(), ids=lambda c: c.name)
def test_poisoned_cases_in_the_oracle(case):
    """What section f of the device test compares with: NaN-poisoned samples are NaN in every oracle output, the
    +-inf-poisoned ones are not finite somewhere, floored log inputs change their sample and stay finite."""
    spec = m3.build_spec(case)
    clean, bad, classes = m3.poisoned_sources(case)
    with np.errstate(invalid="ignore", over="ignore"):
        o64 = mlp_np.forward(spec, bad, dtype=np.float64)
        c64 = mlp_np.forward(spec, clean, dtype=np.float64)
    all64 = np.concatenate([o64[k] for k in spec.output_names], axis=1)
    clean64 = np.concatenate([c64[k] for k in spec.output_names], axis=1)
    nan_s = [s for s, c in classes.items() if c == "nan"]
    inf_s = [s for s, c in classes.items() if c == "inf"]
    floor_s = [s for s, c in classes.items() if c == "floor"]
    rest = np.array([s for s in range(case.n) if classes.get(s) not in ("nan", "inf")])
    assert {0, 31, 32, 63, 127, 128, case.n - 4, case.n - 1} <= set(classes)
    assert np.isnan(all64[nan_s]).all()  # (the hidden output too: numpy's maximum(NaN, 0) is NaN)
    assert not np.isfinite(all64[inf_s]).all(axis=1).any()
    assert np.isfinite(all64[rest]).all()
    assert (all64[floor_s] != clean64[floor_s]).any(axis=1).all()


# ---------------------------------------------------------------------------------------------------------------------
# the tracer inputs of the arithmetic test discriminate
# ---------------------------------------------------------------------------------------------------------------------
def test_bf16_pieces_are_exact_and_round_to_nearest_even():
    rng = np.random.default_rng(0)
    x = np.concatenate([m3._mantissas(rng, 4096), np.float32([1.0, 1.00390625, 1.01171875, 3.0e-5, 7.0e8])])
    p = m3.bf16_pieces(x)
    assert np.array_equal(p["hi"].astype(np.float64) + p["mid"].astype(np.float64) + p["lo"].astype(np.float64), x.astype(np.float64))
    for piece in p.values():
        assert not (piece.view(np.uint32) & 0xFFFF).any()
    # ties to even: 1 + 2^-8 is half way between 1 and 1 + 2^-7 -> 1; 1 + 3 x 2^-8 -> 1 + 2^-6
    assert p["hi"][-4] == 1.0 and p["hi"][-3] == np.float32(1.015625)
    assert np.all(np.abs(x - p["hi"]) <= 2.0 ** -8 * np.abs(x)) and np.all(np.abs(p["lo"]) <= 2.0 ** -16 * np.abs(x))


@pytest.mark.parametrize("kind", m3.TRACER_KINDS)
def test_tracer_inputs_discriminate(kind):
    """The emulation of the kernel's product with all six terms passes the derived bound on the tracer model; with any
    one term removed in any one split layer type of the model it fails -- so the device test's bound can tell."""
    tr = m3.tracer(kind)
    g = m3.geometry3(tr.spec)
    truth = mlp_np.forward(tr.spec, tr.sources, dtype=np.float64)
    # every weight matrix is a scaled (partial) permutation of full-mantissa numbers; the oracle's chain is exact
    for w in list(tr.spec.hidden_kernels) + [tr.spec.out_kernel]:
        assert ((w != 0).sum(axis=0) == 1).all() and ((w != 0).sum(axis=1) <= 1).all()
        assert (w[w != 0].view(np.uint32) & 1).all() and (w[w != 0] > 0).all()
    assert (tr.sources["a"].view(np.uint32) & 1).all()
    assert all(i.center is None and i.scale is None for i in tr.spec.inputs) and not any(b.any() for b in tr.spec.hidden_biases)
    assert (truth["y"] > 0).all() and (truth["h"] > 0).all()
    full = m3.tracer_excess(tr, m3.emulate_tracer(tr), truth)
    assert full <= 1.0, (kind, full)
    expected_types = {"layer1": {"layer1"}, "hidden": {"layer1", "hidden"}, "mfma-out": {"layer1", "output"}, "valu-out": {"layer1"}}[kind]
    assert set(tr.layer_types) == expected_types and (("output" in tr.layer_types) == bool(g["has_out"]))
    for layer_type in tr.layer_types:
        for term in m3.TERMS:
            dropped = m3.tracer_excess(tr, m3.emulate_tracer(tr, drop=(layer_type, term)), truth)
            assert dropped > 1.0, (kind, layer_type, term, dropped)


def test_tracers_cover_every_split_layer_type_and_the_valu_layer():
    types = set()
    outs = set()
    for kind in m3.TRACER_KINDS:
        tr = m3.tracer(kind)
        types |= set(tr.layer_types)
        outs.add(m3.facts(m3.expected_variant3(tr.spec, 132))["out"])
    assert types == set(m3.LAYER_TYPES) and outs == {"mfma", "valu4"}
