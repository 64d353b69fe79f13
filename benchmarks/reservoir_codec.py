"""The reservoir models' column codecs (fv3hip_codec_encode / fv3hip_codec_decode), timed with HIP events
after warm-up:

  dense   the reference-default autoencoder (4 x 79 -> 20 -> 20 -> 10 and back), float32 sources
  affine  StandardScaler + PCA 316 -> 40, float64 sources

each on one C48 tile with overlap 4 (56 x 56 columns) and on one C384 tile (384 x 384 columns), next to

  - the streaming rate of a large device copy measured in the same run (read + write, as benchmarks/hbm_bandwidth.py
    measures it): bytes moved / time against it.  The C48 arrays (4-8 MB) stay in the Infinity Cache between calls;
  - a plain-torch twin on the same device (torch.cat, the normalisation, an F.linear chain / torch.matmul);
  - one whole reservoir step of R1's size (benchmarks/reservoir_step.py: one C48 tile, 2 x 2 layout, state 1000) on the
    latent, with and without the dense codec around it, and R1 itself for scale.

One JSON line per measurement.

    python3 benchmarks/reservoir_codec.py [--steps K] [--warmup W]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fv3net_amd import ops  # noqa: E402
from fv3net_amd.reservoir import (DenseAutoencoder, DoNothingTransformer, RankXYDivider, ReservoirModel,  # noqa: E402
                                  SkTransformer, SparseMatrix)

import reservoir_step  # noqa: E402

SIZES = (79, 79, 79, 79)
K = sum(SIZES)
EXTENTS = {"C48+4": (56, 56), "C384": (384, 384)}


def timed(fn, steps, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = ops.HipTimer()
    t.start(dev)
    for _ in range(steps):
        fn()
    t.stop(dev)
    return t.elapsed_ms() * 1e3 / steps  # us


def stream_rate(dev, steps, warmup):
    src = torch.rand((3, 79, 1536, 1536), device=dev)  # 2.2 GB read + 2.2 GB written: past the Infinity Cache
    dst = torch.empty_like(src)
    us = timed(lambda: dst.copy_(src), steps, warmup, dev)
    return 2 * src.numel() * 4 / (us * 1e-6) / 1e12


def dense_codec(rng):
    def layer(a, b):
        return (rng.standard_normal((a, b)) * np.sqrt(2.0 / a)).astype(np.float32), (0.1 * rng.standard_normal(b)).astype(np.float32)

    enc = [layer(K, 20), layer(20, 20), layer(20, 10)]
    dec = [layer(10, 20), layer(20, 20)]
    heads = [layer(20, nz) for nz in SIZES]
    u = lambda ls, i: [x[i] for x in ls]  # noqa: E731
    return DenseAutoencoder(rng.standard_normal(K), rng.uniform(0.5, 2, K), SIZES, u(enc, 0), u(enc, 1), u(dec, 0), u(dec, 1),
                            u(heads, 0), u(heads, 1))


def affine_codec(rng):
    q, _ = np.linalg.qr(rng.standard_normal((K, 40)))
    return SkTransformer(q.T, 0.1 * rng.standard_normal(K), SIZES, scaler_mean=rng.standard_normal(K),
                         scaler_scale=rng.uniform(0.5, 2, K))


def dense_twin(codec, dev):
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    c, s = t(codec.center), t(codec.scale)
    enc = [(t(w.T.copy()), t(b)) for w, b in zip(codec.encoder_kernels, codec.encoder_biases)]
    dec = [(t(w.T.copy()), t(b)) for w, b in zip(codec.decoder_kernels, codec.decoder_biases)]
    head_w = t(np.concatenate(codec.head_kernels, axis=1).T.copy())
    head_b = t(np.concatenate(codec.head_biases))

    def encode(xs):
        h = (torch.cat(xs, dim=-1).reshape(-1, K) - c) / (s + 1e-7)
        for w, b in enc:
            h = torch.relu(F.linear(h, w, b))
        return h

    def decode(z):
        h = z.reshape(-1, z.shape[-1])
        for w, b in dec:
            h = torch.relu(F.linear(h, w, b))
        y = F.linear(h, head_w, head_b) * s + c
        return [p.contiguous() for p in torch.split(y, SIZES, dim=1)]

    return encode, decode


def affine_twin(codec, dev):
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    mean, std, pm, comp = t(codec.scaler_mean), t(codec.scaler_scale), t(codec.pca_mean), t(codec.components)

    def encode(xs):
        return torch.matmul((torch.cat(xs, dim=-1).reshape(-1, K) - mean) / std - pm, comp.T)

    def decode(z):
        y = (torch.matmul(z.reshape(-1, z.shape[-1]), comp) + pm) * std + mean
        return [p.contiguous() for p in torch.split(y, SIZES, dim=1)]

    return encode, decode


def codec_lines(name, codec, twin, src_dtype, stream, args, dev):
    for extent_name, (nx, ny) in EXTENTS.items():
        xs = [torch.randn((nx, ny, nz), dtype=src_dtype, device=dev) for nz in SIZES]
        latent = codec.encode_device(xs)
        outs = codec.decode_device(latent)
        n = nx * ny
        src_b, lat_b, out_b = xs[0].element_size(), latent.element_size(), outs[0].element_size()
        enc_bytes = n * (K * src_b + codec.n_latent_dims * lat_b)
        dec_bytes = n * (K * out_b + codec.n_latent_dims * lat_b)
        t_enc = timed(lambda: codec.encode_device(xs, out=latent), args.steps, args.warmup, dev)
        t_dec = timed(lambda: codec.decode_device(latent, outs), args.steps, args.warmup, dev)
        t_enc_twin = timed(lambda: twin[0](xs), args.steps, args.warmup, dev)
        t_dec_twin = timed(lambda: twin[1](latent), args.steps, args.warmup, dev)
        enc_tbs, dec_tbs = enc_bytes / (t_enc * 1e-6) / 1e12, dec_bytes / (t_dec * 1e-6) / 1e12
        print(json.dumps({
            "codec": name, "extent": extent_name, "columns": n, "features": K, "n_latent": codec.n_latent_dims,
            "encode_us": round(t_enc, 2), "decode_us": round(t_dec, 2), "encode_bytes": enc_bytes, "decode_bytes": dec_bytes,
            "encode_tbs": round(enc_tbs, 3), "decode_tbs": round(dec_tbs, 3), "copy_stream_tbs": round(stream, 3),
            "encode_frac_stream": round(enc_tbs / stream, 3), "decode_frac_stream": round(dec_tbs / stream, 3),
            "torch_encode_us": round(t_enc_twin, 2), "torch_decode_us": round(t_dec_twin, 2),
            "encode_speedup_vs_torch": round(t_enc_twin / t_enc, 2), "decode_speedup_vs_torch": round(t_dec_twin / t_dec, 2),
        }), flush=True)


def step_lines(codec, args, dev):
    """R1's reservoir (one C48 tile, 2 x 2 layout, overlap 0, state 1000) on the codec's latent: 10 latent levels in and
    out, stepped from the latent alone and with encode before / decode after."""
    rng = np.random.default_rng(1)
    tile, lx, S, L = 48, 2, 1000, codec.n_latent_dims
    sub = tile // lx
    n_in = n_out = sub * sub * L
    divider = RankXYDivider((lx, lx), 0, rank_extent=(tile, tile), z_feature_size=L)
    w_in = reservoir_step.random_csr(rng, S, n_in, 1.0 - reservoir_step.W_IN_SPARSITY, -0.1, 0.1)
    w_res = reservoir_step.random_csr(rng, S, S, 1.0 - reservoir_step.W_RES_SPARSITY, 0.0, 1.0)
    w_res = (w_res[0], w_res[1], w_res[2] * (0.99 / max(1.0, S * (1.0 - reservoir_step.W_RES_SPARSITY) * 0.5)))
    model = ReservoirModel(divider, DoNothingTransformer([L]), DoNothingTransformer([L]), SparseMatrix.from_csr(*w_in, (S, n_in)),
                           SparseMatrix.from_csr(*w_res, (S, S)), rng.standard_normal((lx * lx, S, n_out)) / np.sqrt(S),
                           rng.standard_normal((lx * lx, n_out)))
    xs = [torch.randn((tile, tile, nz), dtype=torch.float32, device=dev) for nz in SIZES]
    lat_in = codec.encode_device(xs)
    lat_out = torch.empty((tile, tile, L), dtype=torch.float64, device=dev)
    outs = codec.decode_device(lat_out.zero_())

    def plain():
        model.increment([lat_in])
        model.predict(outs=[lat_out])

    def coded():
        codec.encode_device(xs, out=lat_in)
        model.increment([lat_in])
        model.predict(outs=[lat_out])
        codec.decode_device(lat_out, outs)

    t_plain = timed(plain, args.steps, args.warmup, dev)
    t_coded = timed(coded, args.steps, args.warmup, dev)
    r1 = reservoir_step.build("R1", np.random.default_rng(0))
    t_r1 = timed(lambda: (r1["model"].increment(r1["inputs"]), r1["model"].predict()), args.steps, args.warmup, dev)
    print(json.dumps({"step": "R1-sized reservoir on the dense codec's latent", "state_size": S, "input_size": n_in,
                      "step_without_codec_us": round(t_plain, 2), "step_with_codec_us": round(t_coded, 2),
                      "codec_share": round(1 - t_plain / t_coded, 3), "r1_step_us": round(t_r1, 2)}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path to time")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    stream = stream_rate(dev, max(5, args.steps // 5), 2)
    dense, affine = dense_codec(rng), affine_codec(rng)
    codec_lines("dense 316-20-20-10", dense, dense_twin(dense, dev), torch.float32, stream, args, dev)
    codec_lines("affine 316-40 f64", affine, affine_twin(affine, dev), torch.float64, stream, args, dev)
    step_lines(dense, args, dev)


if __name__ == "__main__":
    main()
