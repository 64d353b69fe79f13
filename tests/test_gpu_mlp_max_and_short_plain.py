"""The one-instruction maximum and the short first plain chunk of the fast-I/O fused MLP kernels.

ReLU and the floor of the fast logarithm are `max_keep_nan` (v_maximum3_f32) in mlp_fused_kernel: a NaN stays a NaN, every
other value is what the compare-and-select gave, except that ReLU of -0 is +0 -- equal by value.  The ReLU cases use
weights of +-1 and small integer biases on inputs that are multiples of 0.5, so every finite sum is exact in float32 in
any order and the float32 restatement is the expected value, not an approximation of it.

Where the plain inputs do not fill their last 32-row chunk, the host makes the partial chunk the plain block's first and
the kernel runs 13 of its 16 k-pair slots (MlpLaunch::l1_short_plain).  A dropped slot would add +-0 to every accumulator,
so the results must EQUAL those of a model whose zero rows are real rows of zero weight, which runs every chunk in full.
The host does so where the partial chunk holds at most 26 real rows, another plain chunk follows, and the chunk ahead of
the plain block is none or the 8-slot last log chunk.  Behind a log block that leaves 17 to 26 real rows as candidates:
the table has fewer than 32 zero rows in all, 16 or more of them pad the log block, 6 or more the plain one.
"""
import numpy as np
import pytest
import torch

from oracle import mlp_np

from tolerances import assert_close_per_level, decades

pytestmark = pytest.mark.gpu


def _to_device(src_sf, device):
    """[sample, feature] host arrays as [feature, sample] contiguous device arrays (a fresh copy: the transpose of a
    one-feature array already counts as contiguous and would keep a feature stride of 1, which is no fast-I/O layout)."""
    return {k: torch.from_numpy(np.array(v.T, order="C", copy=True)).to(device) for k, v in src_sf.items()}


def _predict(spec, src_sf, device, kernel=",false,true,"):
    from fv3net_amd.mlp import MlpModel

    model = MlpModel(spec, device=device, small_limit=0)
    names = set(spec.sources)
    out = model.predict(_to_device({k: v for k, v in src_sf.items() if k in names}, device))
    v = model.last_variant
    assert v.startswith("mlp_fused_kernel<") and kernel in v, v
    return {k: t.cpu().numpy().T for k, t in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# ReLU values
# ---------------------------------------------------------------------------------------------------------------------
CLASSES = np.array([2.5, -2.5, 0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], np.float32)


def _signs(rng, shape):
    return rng.choice(np.array([-1.0, 1.0], np.float32), size=shape)


@pytest.mark.parametrize("n_hidden", [1, 2])
@pytest.mark.parametrize("width", [32, 256])
def test_relu_values(device, width, n_hidden):
    from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec

    rng = np.random.default_rng(width + n_hidden)
    n, nf_out = 256, 8
    hk = [_signs(rng, (1, width))] + [_signs(rng, (width, width)) for _ in range(n_hidden - 1)]
    hb = [rng.integers(-3, 4, width).astype(np.float32) for _ in range(n_hidden)]
    wo, bo = _signs(rng, (width, nf_out)), rng.integers(-3, 4, nf_out).astype(np.float32)
    spec = MlpSpec(inputs=[InputSpec(source="x", nfeat=1)], hidden_kernels=hk, hidden_biases=hb,
                   outputs=[OutputSpec(name="y", nfeat=nf_out)], out_kernel=wo, out_bias=bo, hidden_output="h")
    x = CLASSES[np.arange(n) % len(CLASSES)].reshape(n, 1)
    got = _predict(spec, {"x": x}, device, kernel=",false,true,true,")

    with np.errstate(invalid="ignore"):
        act = x  # float32 restatement; float64 sums of these values are exact, so the cast back is too
        for w, b in zip(hk, hb):
            pre = (act.astype(np.float64) @ w.astype(np.float64) + b).astype(np.float32)
            act = np.maximum(pre, np.float32(0))
        y = (act.astype(np.float64) @ wo.astype(np.float64) + bo).astype(np.float32)
    # (the expected activations hold what the classes are there for: zeros and positive values, infinities, NaNs)
    assert np.isfinite(act[:4]).all() and (act[:4] == 0).any() and (act[0] > 0).any() and (act[1] > 0).any()
    assert not np.isfinite(act[4]).any() or n_hidden == 1
    assert np.isinf(act[4]).any() or n_hidden > 1
    assert np.isnan(act[6]).all() and np.isnan(act[7]).all()
    assert got["h"].shape == act.shape and got["y"].shape == y.shape
    assert np.array_equal(got["h"], act, equal_nan=True)
    assert np.array_equal(got["y"], y, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
# the floor of the fast logarithm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 256])
def test_log_floor_on_the_fast_path(device, width):
    from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec

    rng = np.random.default_rng(7 + width)
    n, nlog, nf_out = 128, 32, 40
    eps = np.float32(1e-8)
    spec = MlpSpec(
        inputs=[InputSpec(source="q", nfeat=nlog, transform="log", eps=float(eps), center=rng.normal(-12, 1, nlog).astype(np.float32),
                          scale=rng.uniform(0.5, 2, nlog).astype(np.float32)),
                InputSpec(source="p", nfeat=1, center=np.zeros(1, np.float32), scale=np.ones(1, np.float32))],
        hidden_kernels=[(rng.normal(0, 1, (nlog + 1, width)) / np.sqrt(nlog + 1)).astype(np.float32),
                        (rng.normal(0, 1, (width, width)) / np.sqrt(width)).astype(np.float32)],
        hidden_biases=[rng.normal(0, 0.1, width).astype(np.float32) for _ in range(2)],
        outputs=[OutputSpec(name="y", nfeat=nf_out)],
        out_kernel=(rng.normal(0, 1, (width, nf_out)) / np.sqrt(width)).astype(np.float32), out_bias=rng.normal(0, 0.1, nf_out).astype(np.float32))
    clean = {"q": (10 ** rng.uniform(-8, -2, (n, nlog))).astype(np.float32), "p": rng.uniform(0.3, 1.5, (n, 1)).astype(np.float32)}
    floor_values = np.array([0.0, -0.0, -1.0, -np.inf, eps / np.float32(2)], np.float32)
    first = 40  # samples first .. first + 5: at and below the floor; first + 5: exactly eps; first + 6: NaN
    probe = {k: v.copy() for k, v in clean.items()}
    for i, v in enumerate(floor_values):
        probe["q"][first + i] = v
    probe["q"][first + len(floor_values)] = eps
    probe["q"][first + len(floor_values) + 1] = np.nan
    special = np.arange(first, first + len(floor_values) + 2)
    probe["p"][special] = probe["p"][first]

    y_clean = _predict(spec, clean, device)["y"]
    y = _predict(spec, probe, device)["y"]
    at_eps = y[first + len(floor_values)]
    assert np.isfinite(at_eps).all()
    for i in range(len(floor_values)):
        assert np.array_equal(y[first + i].view(np.int32), at_eps.view(np.int32)), float(floor_values[i])
    assert np.isnan(y[first + len(floor_values) + 1]).all()
    others = np.setdiff1d(np.arange(n), special)
    assert np.isfinite(y_clean).all()
    assert np.array_equal(y[others], y_clean[others])
    # and the samples that were left alone meet the oracle
    truth = mlp_np.forward(spec, {k: v[others] for k, v in probe.items()}, dtype=np.float64)["y"]
    cpu32 = mlp_np.forward(spec, {k: v[others] for k, v in probe.items()}, dtype=np.float32)["y"]
    assert_close_per_level(y[others], truth, cpu32, "log floor model")


# ---------------------------------------------------------------------------------------------------------------------
# the short first plain chunk
# ---------------------------------------------------------------------------------------------------------------------
N = 256


def _plain_pair(seed, rows, n_log, width, short, n_full=1, residual=True):
    """Model A: n_log log features and 32 * n_full + rows plain ones, whose partial chunk holds `rows` real rows.  Model B:
    A with 32 - rows further plain features of zero layer-1 weight, which read finite data, where A's table has its zero
    rows: behind the first `rows` plain features if A's partial chunk is the block's first (`short`), behind all of them
    if not.  (n_log + rows must leave room to pad the log block, or A has one chunk that mixes both kinds and B has not.)"""
    from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec, ResidualSpec

    rng = np.random.default_rng(seed)
    n_plain, extra = 32 * n_full + rows, 32 - rows

    def inp(source, nf, start=0, log=False):
        return InputSpec(source=source, nfeat=nf, start=start, transform="log" if log else "none", eps=1e-8 if log else 0.0,
                         center=rng.normal(0, 1, nf).astype(np.float32), scale=rng.uniform(0.5, 2, nf).astype(np.float32))

    lg = [inp("q", n_log, log=True)] if n_log else []
    first = rows if short else n_plain  # plain features ahead of A's zero rows
    head, tail, fill = inp("p", first), (inp("p", n_plain - first, start=first) if first < n_plain else None), inp("p2", extra)
    fan = n_log + n_plain
    hk = [(rng.normal(0, 1, (fan, width)) / np.sqrt(fan)).astype(np.float32), (rng.normal(0, 1, (width, width)) / np.sqrt(width)).astype(np.float32)]
    hb = [rng.normal(0, 0.1, width).astype(np.float32) for _ in range(2)]
    outs = {"dp": n_plain, "z": 1}
    outputs = [OutputSpec(name=k, nfeat=nf, scale=decades(rng, nf), center=rng.normal(0, 1, nf).astype(np.float32) * decades(rng, nf, top=0.5))
               for k, nf in outs.items()]
    F = sum(outs.values())
    common = dict(hidden_biases=hb, outputs=outputs, out_kernel=(rng.normal(0, 1, (width, F)) / np.sqrt(width)).astype(np.float32),
                  out_bias=rng.normal(0, 0.1, F).astype(np.float32))
    res = [ResidualSpec(name="p_after", source="p", output="dp")] if residual else []
    a = MlpSpec(inputs=lg + [head] + ([tail] if tail else []), hidden_kernels=hk, residuals=list(res), **common)
    w1b = np.concatenate([hk[0][:n_log + first], np.zeros((extra, width), np.float32), hk[0][n_log + first:]], axis=0)
    b = MlpSpec(inputs=lg + [head, fill] + ([tail] if tail else []), hidden_kernels=[w1b, hk[1]], residuals=list(res), **common)
    return a, b


def _plain_sources(seed, rows, n_log, n, n_full=1):
    rng = np.random.default_rng(2000 + seed)
    src = {"p": rng.uniform(0.3, 1.5, (n, 32 * n_full + rows)).astype(np.float32), "p2": rng.uniform(0.3, 1.5, (n, 32 - rows)).astype(np.float32)}
    if n_log:
        src["q"] = np.where(rng.random((n, n_log)) < 0.3, 0.0, 10 ** rng.uniform(-8, -2, (n, n_log))).astype(np.float32)
    return src


def _oracle_check(spec, src_sf, out, what):
    src = {k: v for k, v in src_sf.items() if k in set(spec.sources)}
    truth = mlp_np.forward(spec, src, dtype=np.float64)
    cpu32 = mlp_np.forward(spec, src, dtype=np.float32)
    assert set(out) == set(truth)
    for name, t in truth.items():
        assert_close_per_level(out[name], t, cpu32[name], f"{name} ({what})")


@pytest.mark.parametrize("width", [32, 256])
@pytest.mark.parametrize("rows,n_log,short", [(1, 0, True), (13, 0, True), (26, 0, True), (31, 0, False),
                                              (1, 32, False), (13, 20, False), (26, 13, True), (26, 20, False), (31, 13, False)])
def test_short_plain_chunk_equals_the_full_chunks(device, rows, n_log, short, width):
    """rows = 1, 13, 26 behind no log block, and 26 behind one whose last chunk runs 8 slots (13 log features), turn the
    short chunk on in model A.  31 rows need all 16 slots; behind 32 or 20 log features a full 16-slot log chunk would
    have to run ahead of the short one (1 and 13 rows leave no room for a log block that is padded by 16 rows or more):
    those models keep every chunk at 16 slots and their zero rows at the end, and still agree."""
    a, b = _plain_pair(rows * 100 + n_log, rows, n_log, width, short)
    src = _plain_sources(rows + n_log, rows, n_log, N)
    out_a = _predict(a, src, device)
    out_b = _predict(b, src, device)
    assert set(out_a) == set(out_b) == {"dp", "z", "p_after"}
    for name in out_a:
        assert np.isfinite(out_a[name]).all(), name
        assert np.array_equal(out_a[name], out_b[name]), name  # (by value: -0.0 == 0.0)
    _oracle_check(a, src, out_a, f"rows={rows} n_log={n_log} width={width}")


def test_short_plain_chunk_with_two_full_chunks_at_384_samples(device):
    a, b = _plain_pair(5, 26, 13, 256, True, n_full=2, residual=False)
    src = _plain_sources(6, 26, 13, 384, n_full=2)
    out_a = _predict(a, src, device)
    out_b = _predict(b, src, device)
    for name in out_a:
        assert np.array_equal(out_a[name], out_b[name]), name
    _oracle_check(a, src, out_a, "384 samples")


def test_short_plain_chunk_in_the_persistent_loop(device):
    """More tiles than workgroups: the chunk stream wraps from a tile's last chunk to chunk 0 of the next -- the short
    chunk itself where the model has no log block.  The last columns of the big call must equal those columns run alone."""
    from fv3net_amd import ops
    from fv3net_amd.mlp import MlpModel

    for n_log in (0, 13):
        a, _ = _plain_pair(9 + n_log, 26, n_log, 32, True)
        n_big = 128 * (int(ops.device_info()["compute_units"]) + 2) + 32
        model = MlpModel(a, device=device, small_limit=0)
        small = _to_device({k: v for k, v in _plain_sources(4, 26, n_log, N).items() if k in set(a.sources)}, device)
        g = torch.Generator(device=device).manual_seed(5)
        big = {"p": 0.3 + 1.2 * torch.rand((58, n_big), device=device, generator=g)}
        if n_log:
            big["q"] = 10 ** (-8 + 6 * torch.rand((n_log, n_big), device=device, generator=g))
        for k in big:
            big[k][:, -N:] = small[k]
        alone = model.predict(small)
        full = model.predict(big)
        assert model.last_variant.startswith("mlp_fused_kernel<") and ",false,true," in model.last_variant, model.last_variant
        for name in alone:
            assert full[name].shape[1] == n_big
            assert torch.equal(full[name][:, -N:], alone[name]), (n_log, name)


@pytest.mark.parametrize("n_log,n_plain", [(45, 0), (0, 26), (13, 26)])
def test_models_that_keep_sixteen_slots(device, n_log, n_plain):
    """An all-log model and models with a single plain chunk (alone, and behind a log block): nothing to move."""
    from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec

    rng = np.random.default_rng(30 + n_log + n_plain)
    width, nf_out, inputs, src = 32, 40, [], {}
    for source, nf, log in (("q", n_log, True), ("p", n_plain, False)):
        if nf:
            inputs.append(InputSpec(source=source, nfeat=nf, transform="log" if log else "none", eps=1e-8 if log else 0.0,
                                    center=rng.normal(0, 1, nf).astype(np.float32), scale=rng.uniform(0.5, 2, nf).astype(np.float32)))
            src[source] = (np.where(rng.random((N, nf)) < 0.3, 0.0, 10 ** rng.uniform(-8, -2, (N, nf))) if log
                           else rng.uniform(0.3, 1.5, (N, nf))).astype(np.float32)
    fan = n_log + n_plain
    spec = MlpSpec(
        inputs=inputs,
        hidden_kernels=[(rng.normal(0, 1, (fan, width)) / np.sqrt(fan)).astype(np.float32), (rng.normal(0, 1, (width, width)) / np.sqrt(width)).astype(np.float32)],
        hidden_biases=[rng.normal(0, 0.1, width).astype(np.float32) for _ in range(2)],
        outputs=[OutputSpec(name="y", nfeat=nf_out, scale=decades(rng, nf_out), center=rng.normal(0, 1, nf_out).astype(np.float32) * decades(rng, nf_out, top=0.5))],
        out_kernel=(rng.normal(0, 1, (width, nf_out)) / np.sqrt(width)).astype(np.float32), out_bias=rng.normal(0, 0.1, nf_out).astype(np.float32))
    _oracle_check(spec, src, _predict(spec, src, device), f"n_log={n_log} n_plain={n_plain}")
