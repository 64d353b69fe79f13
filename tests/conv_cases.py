"""Shared builders of the convolution tests: random networks, inputs of the kind real fields have, and the
``torch.nn.functional.conv2d`` chain on the CPU (float64: a second opinion on ``conv_np``; float32: the reference arithmetic
the GPU result is compared with)."""
import numpy as np
import torch

import tolerances
from fv3net_amd.conv import ConvInput, ConvOutput, ConvSpec


def make_spec(rng, channels, filters, depth, k, heads, activation="relu", bias=True, unit_inputs=False):
    """``channels`` / ``heads``: name -> channel count.  Weights N(0, 1 / sqrt(fan_in)); output scales fall over decades."""
    inputs = []
    for name, nf in channels.items():
        center = np.zeros(nf, np.float32) if unit_inputs else rng.normal(0, 1, nf).astype(np.float32) * 10
        scale = np.ones(nf, np.float32) if unit_inputs else rng.uniform(0.5, 2, nf).astype(np.float32)
        inputs.append(ConvInput(name, nf, center, scale))
    c_in = sum(channels.values())
    kernels, biases = [], []
    for _ in range(depth - 1):
        kernels.append((rng.normal(0, 1, (k, k, c_in, filters)) / np.sqrt(k * k * c_in)).astype(np.float32))
        biases.append(rng.normal(0, 0.1, filters).astype(np.float32))
        c_in = filters
    outputs = []
    for name, nf in heads.items():
        outputs.append(ConvOutput(name, nf, (rng.normal(0, 1, (filters, nf)) / np.sqrt(filters)).astype(np.float32),
                                  rng.normal(0, 0.1, nf).astype(np.float32), tolerances.decades(rng, nf),
                                  (rng.normal(0, 1, nf) * tolerances.decades(rng, nf)).astype(np.float32)))
    return ConvSpec(inputs, kernels, biases if bias else None, outputs, activation=activation)


def make_inputs(rng, spec, lead, nx, ny, dtype=np.float32):
    """name -> ``lead + (x, y, z)``: standard normal scaled and shifted per channel to the variable's own mean and spread."""
    out = {}
    for i in spec.inputs:
        a = rng.normal(0, 1, tuple(lead) + (nx, ny, i.nfeat))
        out[i.source] = (a * np.asarray(i.scale, np.float64) + np.asarray(i.center, np.float64)).astype(dtype)
    return out


def torch_chain(spec, inputs, dtype=torch.float32):
    """``inputs``: name -> [sample, x, y, z] with the halo.  The same graph through ``conv2d`` on the CPU in ``dtype``."""
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype)
    cols = [(tt(inputs[i.source]) - tt(i.center)) / tt(i.scale) for i in spec.inputs]
    x = torch.cat(cols, dim=-1).permute(0, 3, 1, 2)  # [s, c, x, y]
    act = {"relu": torch.relu, "tanh": torch.tanh, "linear": lambda v: v}[spec.activation]
    for l, w in enumerate(spec.hidden_kernels):
        b = None if spec.hidden_biases is None else tt(spec.hidden_biases[l])
        x = act(torch.nn.functional.conv2d(x, tt(w).permute(3, 2, 0, 1), b))
    out = {}
    for o in spec.outputs:
        y = torch.nn.functional.conv2d(x, tt(o.kernel).t()[:, :, None, None], tt(o.bias))
        y = y.permute(0, 2, 3, 1) * tt(o.scale) + tt(o.center)
        out[o.name] = y.numpy()
    return out
