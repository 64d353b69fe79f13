"""The field and the expected values of the cube-seam tests (test_host_cube_seams.py, test_gpu_cube_seams.py).

The field holds ``1 + flat cell index``, so every cell of the cube is told from every other and from the zero of a corner; all
values are integers far below 2**24, exact in float32.  The faces are the smallest at which a wrong neighbour, axis, reversal
or line shows on each of the 6 x 4 sides: n = 2, 3 and 5 with a halo of one cell, and n = 3 with a halo of three -- as wide as
the face itself."""
import numpy as np

import conv_np

SIDES = ("x-low", "x-high", "y-low", "y-high")
FACES = (2, 3, 5)        # halo 1
WIDE = (3, 3)            # (n, halo): the halo is the neighbour's whole face


def field(n):
    """``[6, n, n]`` float32."""
    return (1 + np.arange(6 * n * n, dtype=np.float32)).reshape(6, n, n)


def halo_lines(padded, n, h):
    """``[6, n + 2 h, n + 2 h]`` -> ``[6, 4, h, n]``: per tile and side the halo lines, depth 0 next to the tile, each along
    the edge in the tile's own direction."""
    p = np.asarray(padded)
    return np.stack([p[:, :h, h:h + n][:, ::-1], p[:, h + n:, h:h + n],
                     p[:, h:h + n, :h][:, :, ::-1].swapaxes(1, 2), p[:, h:h + n, h + n:].swapaxes(1, 2)], axis=1)


def corners(padded, n, h):
    """The four h x h corners ``[6, 4, h, h]``."""
    p = np.asarray(padded)
    return np.stack([p[:, :h, :h], p[:, :h, h + n:], p[:, h + n:, :h], p[:, h + n:, h + n:]], axis=1)


def shifted(n, k):
    """``[6, n, n, k * k]``: what a k x k convolution over the cube halo with the one-hot weight of tap (dx, dy) gives, tap
    ``dx * k + dy`` last -- the padded field itself, read at (x + dx, y + dy)."""
    p = conv_np.append_halos(field(n), (k - 1) // 2)
    return np.stack([p[:, dx:dx + n, dy:dy + n] for dx in range(k) for dy in range(k)], axis=-1)
