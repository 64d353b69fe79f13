"""The 8-slot last log chunk of the fast-I/O fused MLP kernels.

When the log-transformed inputs fill at most half of their last 32-row chunk (the host pads the rest with zero weight rows)
and plain chunks follow, the kernel runs that chunk with 8 of its 16 k-pair slots.  A dropped slot would add +-0 to every
accumulator, so the results must EQUAL those of a model whose log block fills the chunk with real rows of zero weights,
which takes the 16-slot body; and they must still meet the float64 oracle at the per-level tolerance.
"""
import numpy as np
import pytest
import torch

from oracle import mlp_np

from tolerances import assert_close_per_level, decades

pytestmark = pytest.mark.gpu

N = 288  # two full 128-sample tiles plus one wave; a multiple of 32, so the fast-I/O kernel is the one launched


def _model_pair(seed, r, n_plain, width, residual=True, n_hidden=2, eps=1e-8):
    """Model A (r log features + n_plain plain ones) and model B (A with 32 - r further log features whose layer-1
    weight rows are zero).  Output `dp` has n_plain rows, so that `p_after = p + dp` is a residual output."""
    from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec, ResidualSpec

    rng = np.random.default_rng(seed)
    extra = 32 - r

    def inp(source, nf, log):
        return InputSpec(source=source, nfeat=nf, start=0, transform="log" if log else "none", eps=eps if log else 0.0,
                         center=rng.normal(0, 1, nf).astype(np.float32), scale=rng.uniform(0.5, 2, nf).astype(np.float32))

    lg, pl, lg2 = inp("q", r, True), inp("p", n_plain, False), inp("q2", extra, True)
    hk, hb = [], []
    fan = r + n_plain
    for _ in range(n_hidden):
        hk.append((rng.normal(0, 1, (fan, width)) / np.sqrt(fan)).astype(np.float32))
        hb.append(rng.normal(0, 0.1, width).astype(np.float32))
        fan = width
    outs = {"dp": n_plain, "z": 1}
    outputs = [OutputSpec(name=k, nfeat=nf, scale=decades(rng, nf), center=rng.normal(0, 1, nf).astype(np.float32) * decades(rng, nf, top=0.5))
               for k, nf in outs.items()]
    F = sum(outs.values())
    out_kernel = (rng.normal(0, 1, (width, F)) / np.sqrt(width)).astype(np.float32)
    out_bias = rng.normal(0, 0.1, F).astype(np.float32)
    residuals = [ResidualSpec(name="p_after", source="p", output="dp")] if residual else []
    a = MlpSpec(inputs=[lg, pl], hidden_kernels=hk, hidden_biases=hb, outputs=outputs, out_kernel=out_kernel, out_bias=out_bias,
                residuals=list(residuals))
    w1b = np.concatenate([hk[0][:r], np.zeros((extra, width), np.float32), hk[0][r:]], axis=0)
    b = MlpSpec(inputs=[lg, lg2, pl], hidden_kernels=[w1b] + hk[1:], hidden_biases=hb, outputs=outputs, out_kernel=out_kernel,
                out_bias=out_bias, residuals=list(residuals))
    return a, b


def _sources(seed, r, n_plain, n):
    """[sample, feature] float32 arrays: positive values over six decades with some zeros (the eps floor) for the logs."""
    rng = np.random.default_rng(1000 + seed)

    def logsrc(nf):
        return np.where(rng.random((n, nf)) < 0.3, 0.0, 10 ** rng.uniform(-8, -2, (n, nf))).astype(np.float32)

    return {"q": logsrc(r), "q2": logsrc(32 - r), "p": rng.uniform(0.3, 1.5, (n, n_plain)).astype(np.float32)}


def _to_device(src_sf, names, device):
    """[feature, sample] contiguous device arrays.  (A fresh copy: the transpose of a one-feature array already counts as
    contiguous and would keep a feature stride of 1, which is not a fast-I/O layout.)"""
    return {k: torch.from_numpy(np.array(v.T, order="C", copy=True)).to(device) for k, v in src_sf.items() if k in names}


def _predict(spec, src_sf, device):
    from fv3net_amd.mlp import MlpModel

    model = MlpModel(spec, device=device, small_limit=0)
    dev = _to_device(src_sf, {i.source for i in spec.inputs}, device)
    out = model.predict(dev)
    v = model.last_variant
    assert v.startswith("mlp_fused_kernel<") and ",false,true," in v, v
    return out


def _oracle_check(spec, src_sf, out, what):
    names = {i.source for i in spec.inputs}
    src = {k: v for k, v in src_sf.items() if k in names}
    truth = mlp_np.forward(spec, src, dtype=np.float64)
    cpu32 = mlp_np.forward(spec, src, dtype=np.float32)
    assert set(out) == set(truth)
    for name, t in truth.items():
        assert_close_per_level(out[name].cpu().numpy().T, t, cpu32[name], f"{name} ({what})")


@pytest.mark.parametrize("width", [32, 256])
@pytest.mark.parametrize("r,n_plain", [(r, p) for r in (1, 13, 16, 17) for p in (26, 32)] + [(1, 31)])
def test_short_log_chunk_equals_the_full_chunk(device, r, n_plain, width):
    """r = 1, 13, 16 turn the 8-slot chunk on in model A; with r = 17 both models run the 16-slot path and still agree.

    One case cannot be an equality: r = 1 with 26 plain features is 27 inputs, which the host packs into ONE chunk that
    mixes both kinds (there is no room to pad the log block), while model B has two chunks -- other k-pairs and the other
    log flavour, on any version of the kernel.  That case checks both models against the oracle instead; (1, 31) is
    there so that r = 1 meets an odd number of plain features with the 8-slot chunk on."""
    a, b = _model_pair(r * 100 + n_plain, r, n_plain, width)
    src = _sources(r, r, n_plain, N)
    out_a = _predict(a, src, device)
    out_b = _predict(b, src, device)
    assert set(out_a) == set(out_b) == {"dp", "z", "p_after"}
    if r + n_plain <= 32:
        _oracle_check(a, src, out_a, "A, one mixed chunk")
        _oracle_check(b, src, out_b, "B")
        return
    for name in out_a:
        assert torch.equal(out_a[name], out_b[name]), name  # (by value: -0.0 == 0.0)


def test_short_log_chunk_with_a_denormal_log_floor(device):
    """eps below FLT_MIN: the log chunks take the libm flavour, and the 8-slot chunk sits behind that loop instead."""
    a, b = _model_pair(11, 13, 26, 256, eps=1e-40)
    src = _sources(12, 13, 26, N)
    out_a = _predict(a, src, device)
    out_b = _predict(b, src, device)
    for name in out_a:
        assert torch.equal(out_a[name], out_b[name]), name
    _oracle_check(a, src, out_a, "eps=1e-40")


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("width", [32, 256])
@pytest.mark.parametrize("r,n_plain", [(1, 32), (13, 26), (16, 26), (16, 32)])
def test_short_log_chunk_against_oracle(device, r, n_plain, width, residual):
    a, _ = _model_pair(7 + r, r, n_plain, width, residual=residual)
    src = _sources(50 + r, r, n_plain, N)
    _oracle_check(a, src, _predict(a, src, device), f"r={r} width={width}")


def test_short_log_chunk_in_the_persistent_loop(device):
    """More tiles than workgroups: the chunk stream wraps from a tile's last chunk to chunk 0 of the next with the short
    chunk in the middle.  The last 288 columns of the big call must equal the same columns run alone."""
    from fv3net_amd import ops
    from fv3net_amd.mlp import MlpModel

    r, n_plain = 13, 26
    a, _ = _model_pair(3, r, n_plain, 32)
    n_big = 128 * (int(ops.device_info()["compute_units"]) + 2) + 32
    model = MlpModel(a, device=device, small_limit=0)
    small = _to_device(_sources(4, r, n_plain, N), {"q", "p"}, device)
    g = torch.Generator(device=device).manual_seed(5)
    big = {"q": 10 ** (-8 + 6 * torch.rand((r, n_big), device=device, generator=g)),
           "p": 0.3 + 1.2 * torch.rand((n_plain, n_big), device=device, generator=g)}
    for k in big:
        big[k][:, -N:] = small[k]
    alone = model.predict(small)
    full = model.predict(big)
    assert model.last_variant.startswith("mlp_fused_kernel<") and ",false,true," in model.last_variant, model.last_variant
    for name in alone:
        assert full[name].shape[1] == n_big
        assert torch.equal(full[name][:, -N:], alone[name]), name


@pytest.mark.parametrize("n_log", [0, 13, 45])
def test_models_without_a_short_chunk_are_unchanged(device, n_log):
    """No log inputs, and all-log models (one chunk; two chunks, the second less than half full): no plain chunk follows
    the log block, so every chunk keeps its 16 slots."""
    from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec

    rng = np.random.default_rng(20 + n_log)
    log = n_log > 0
    nf = n_log if log else 39
    width = 32
    spec = MlpSpec(
        inputs=[InputSpec(source="q" if log else "p", nfeat=nf, start=0, transform="log" if log else "none", eps=1e-8 if log else 0.0,
                          center=rng.normal(0, 1, nf).astype(np.float32), scale=rng.uniform(0.5, 2, nf).astype(np.float32))],
        hidden_kernels=[(rng.normal(0, 1, (nf, width)) / np.sqrt(nf)).astype(np.float32),
                        (rng.normal(0, 1, (width, width)) / np.sqrt(width)).astype(np.float32)],
        hidden_biases=[rng.normal(0, 0.1, width).astype(np.float32) for _ in range(2)],
        outputs=[OutputSpec(name="y", nfeat=40, scale=decades(rng, 40), center=rng.normal(0, 1, 40).astype(np.float32) * decades(rng, 40, top=0.5))],
        out_kernel=(rng.normal(0, 1, (width, 40)) / np.sqrt(width)).astype(np.float32), out_bias=rng.normal(0, 0.1, 40).astype(np.float32))
    if log:
        src = {"q": np.where(rng.random((N, nf)) < 0.3, 0.0, 10 ** rng.uniform(-8, -2, (N, nf))).astype(np.float32)}
    else:
        src = {"p": rng.uniform(0.3, 1.5, (N, nf)).astype(np.float32)}
    _oracle_check(spec, src, _predict(spec, src, device), f"n_log={n_log}")
