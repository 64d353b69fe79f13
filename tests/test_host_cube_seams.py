"""The three numpy / torch restatements of the cube's seams that the tests use as oracles agree on every seam:
``conv_np.append_halos`` (the convolution tests), ``graph_np.neighbour_table`` (the graph tests; one step outside only) and
``cyclegan_cases.pad`` with the cube halo (the CycleGAN and FMR tests).  The kernels' one seam rule (csrc/cube.h) is tested
against the first of them in test_gpu_cube_seams.py."""
import numpy as np
import pytest
import torch

import conv_np
import cyclegan_cases
import graph_np
import seam_cases

CASES = [(n, 1) for n in seam_cases.FACES] + [seam_cases.WIDE]


def _pad_torch(f, h):
    n = f.shape[-1]
    return cyclegan_cases.pad(torch.from_numpy(f).reshape(1, 6, 1, n, n), h, True).reshape(6, n + 2 * h, n + 2 * h).numpy()


@pytest.mark.parametrize("n,h", CASES)
def test_the_padded_fields_agree(n, h):
    f = seam_cases.field(n)
    a, c = conv_np.append_halos(f, h), _pad_torch(f, h)
    assert a.shape == c.shape == (6, n + 2 * h, n + 2 * h)
    assert np.array_equal(a[:, h:h + n, h:h + n], f) and np.array_equal(c[:, h:h + n, h:h + n], f)
    la, lc = seam_cases.halo_lines(a, n, h), seam_cases.halo_lines(c, n, h)
    assert la.shape == (6, 4, h, n) and np.all(la >= 1)      # every halo cell shows a cell of the cube
    for t in range(6):
        for s, side in enumerate(seam_cases.SIDES):
            assert np.array_equal(la[t, s], lc[t, s]), f"tile {t}, side {side}: {la[t, s]} and {lc[t, s]}"
    assert not seam_cases.corners(a, n, h).any() and not seam_cases.corners(c, n, h).any()


@pytest.mark.parametrize("n", seam_cases.FACES)
def test_the_neighbour_table_agrees(n):
    f = seam_cases.field(n)
    flat, table = f.reshape(-1), graph_np.neighbour_table(n).reshape(6, n, n, 5)
    assert np.array_equal(flat[table[..., 0]], f)
    # the halo line of a side: the neighbour in that direction of the tile's cells along that edge
    lines = np.stack([flat[table[:, 0, :, 1]], flat[table[:, n - 1, :, 2]], flat[table[:, :, 0, 3]], flat[table[:, :, n - 1, 4]]], axis=1)
    want = seam_cases.halo_lines(conv_np.append_halos(f, 1), n, 1)[:, :, 0]
    torch_lines = seam_cases.halo_lines(_pad_torch(f, 1), n, 1)[:, :, 0]
    for t in range(6):
        for s, side in enumerate(seam_cases.SIDES):
            assert np.array_equal(lines[t, s], want[t, s]) and np.array_equal(lines[t, s], torch_lines[t, s]), f"tile {t}, side {side}"
    # away from the edges a neighbour is the next cell of the same tile
    assert np.array_equal(flat[table[:, 1:, :, 1]], f[:, :-1]) and np.array_equal(flat[table[:, :-1, :, 2]], f[:, 1:])
    assert np.array_equal(flat[table[:, :, 1:, 3]], f[:, :, :-1]) and np.array_equal(flat[table[:, :, :-1, 4]], f[:, :, 1:])


def test_every_side_is_told_apart():
    """The field and the faces are fine enough: the 24 halo lines of a cube differ from each other and from their reverses
    (n >= 2), so a wrong neighbour, axis or reversal cannot go unseen."""
    for n in seam_cases.FACES:
        lines = seam_cases.halo_lines(conv_np.append_halos(seam_cases.field(n), 1), n, 1).reshape(24, n)
        seen = {tuple(l) for l in lines} | {tuple(l[::-1]) for l in lines}
        assert len(seen) == 48
