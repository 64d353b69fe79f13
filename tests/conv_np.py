"""Float64 numpy restatement of fv3fit's convolutional network and of ``append_halos`` -- the oracle of the convolution tests.

Network (external/fv3fit/fv3fit/keras/_models/convolutional.py:153-210, shared/convolutional_network.py:136-195): per input
variable ``(x - mean) / scale`` per channel, the variables concatenated along the channel axis; ``depth - 1`` hidden layers of
``Conv2D(filters, k, padding="valid", activation)`` -- kernel ``[k, k, c_in, filters]``, first kernel axis along ``x``, second
along ``y``, cross-correlation -- each shrinking ``x`` and ``y`` by ``k - 1``; one linear 1 x 1 head per output on the last
hidden layer, then ``y * scale + center``.  Arrays are ``[sample, x, y, channel]``.

Halos (_shared/halos.py:135-160): see ``append_halos`` below.  Nothing here imports ``fv3net_amd``: the spec is read by
attribute only.
"""
import numpy as np

# tile -> axis -> ((low neighbour, the axis it is joined through), (high neighbour, its axis))
CONNECTIONS = {
    0: {"x": ((4, "y"), (1, "x")), "y": ((5, "y"), (2, "x"))},
    1: {"x": ((0, "x"), (3, "y")), "y": ((5, "x"), (2, "y"))},
    2: {"x": ((0, "y"), (3, "x")), "y": ((1, "y"), (4, "x"))},
    3: {"x": ((2, "x"), (5, "y")), "y": ((1, "x"), (4, "y"))},
    4: {"x": ((2, "y"), (5, "x")), "y": ((3, "y"), (0, "x"))},
    5: {"x": ((4, "x"), (1, "y")), "y": ((3, "x"), (0, "y"))},
}

ACTIVATIONS = {"linear": lambda v: v, "relu": lambda v: np.maximum(v, 0), "tanh": np.tanh}


def append_halos(field, n_halo):
    """``[6, ..., x, y]`` -> ``[6, ..., x + 2 n_halo, y + 2 n_halo]``: line ``d`` outward of a tile's low (high) edge along an
    axis is the low (high) neighbour's line ``d`` inward from its last (first) line along the axis it is joined through,
    reversed along the edge when that is its other axis; corners zero."""
    field = np.asarray(field)
    if field.shape[0] != 6:
        raise ValueError("six tiles")
    if n_halo == 0:
        return field
    n, h = field.shape[-1], n_halo
    out = np.zeros(field.shape[:-2] + (n + 2 * h, n + 2 * h), field.dtype)
    out[..., h:h + n, h:h + n] = field
    for t in range(6):
        dst = np.moveaxis(out[t], (-2, -1), (0, 1))  # a view [x, y, ...]
        for axis in "xy":
            for high in (0, 1):
                nbr, nbr_axis = CONNECTIONS[t][axis][high]
                src = np.moveaxis(field[nbr], (-2, -1), (0, 1))
                if nbr_axis == "y":
                    src = src.swapaxes(0, 1)  # [along the joining axis, along the edge, ...]
                for d in range(h):
                    line = src[d] if high else src[n - 1 - d]
                    if nbr_axis != axis:
                        line = line[::-1]
                    pos = h + n + d if high else h - 1 - d
                    if axis == "x":
                        dst[pos, h:h + n] = line
                    else:
                        dst[h:h + n, pos] = line
    return out


def conv2d_valid(x, w):
    """``x`` [s, X, Y, c], ``w`` [k, k, c, f] -> [s, X - k + 1, Y - k + 1, f]: out[x, y] = sum w[i, j] . in[x + i, y + j]."""
    k = w.shape[0]
    nx, ny = x.shape[1] - k + 1, x.shape[2] - k + 1
    out = np.zeros((x.shape[0], nx, ny, w.shape[3]), x.dtype)
    for i in range(k):
        for j in range(k):
            out += x[:, i:i + nx, j:j + ny, :] @ w[i, j]
    return out


def forward(spec, inputs, dtype=np.float64):
    """``inputs``: name -> [sample, x, y, channel] carrying the halo (single-channel variables with a channel axis of 1).
    Returns name -> [sample, x - 2 h, y - 2 h, channel]."""
    cols = []
    for i in spec.inputs:
        a = np.asarray(inputs[i.source], dtype)
        cols.append((a - np.asarray(i.center, dtype)) / np.asarray(i.scale, dtype))
    x = np.concatenate(cols, axis=-1)
    act = ACTIVATIONS[spec.activation]
    for l, w in enumerate(spec.hidden_kernels):
        x = conv2d_valid(x, np.asarray(w, dtype))
        if spec.hidden_biases is not None:
            x = x + np.asarray(spec.hidden_biases[l], dtype)
        x = act(x)
    out = {}
    for o in spec.outputs:
        y = x @ np.asarray(o.kernel, dtype) + np.asarray(o.bias, dtype)
        out[o.name] = y * np.asarray(o.scale, dtype) + np.asarray(o.center, dtype)
    return out


def halos_required(kernel_size, depth):
    return (kernel_size - 1) // 2 * (depth - 1)
