"""Writes ``append_halos_reference.npz``: the reference's torch-only halo fill, ``AppendHalos.forward``
(external/fv3fit/fv3fit/pytorch/cyclegan/modules.py:425-543, tensors ``[batch, tile, channel, x, y]``), run on the CPU on a
six-tile cube of unique cell ids.  The reference's own test holds it equal to the ``pace.util`` exchange that
``fv3fit._shared.halos.append_halos`` performs (tests/pytorch/test_append_halos.py:32-57), so the file pins the orientation of
an n-cell halo strip on every cube edge.

    python tests/golden/make_append_halos_golden.py <path of the reference checkout>

The module is loaded from the checkout by path; the two imports it cannot satisfy without the rest of the reference's stack
(``vcm.grid``, ``fv3fit.pytorch.system``) are stubbed, neither is used by ``AppendHalos``.  Only data goes into the fixture.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

N, CHANNELS, HALOS = 8, 2, (1, 3)


def load_modules(reference: str):
    for name, attrs in (("vcm", {}), ("vcm.grid", {"get_grid_xyz": None, "get_grid": None}), ("fv3fit", {}),
                        ("fv3fit.pytorch", {}), ("fv3fit.pytorch.system", {"DEVICE": torch.device("cpu")})):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        mod.__path__ = []  # (a package, so that the dotted names below it import)
        sys.modules.setdefault(name, mod)
    path = os.path.join(reference, "external", "fv3fit", "fv3fit", "pytorch", "cyclegan", "modules.py")
    spec = importlib.util.spec_from_file_location("_reference_cyclegan_modules", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main(reference: str):
    modules = load_modules(reference)
    # unique ids: tile, channel, x, y all recoverable from the value
    ids = np.arange(6 * CHANNELS * N * N, dtype=np.float64).reshape(1, 6, CHANNELS, N, N) + 1.0
    out = {"input": ids[0]}  # [tile, channel, x, y]
    for h in HALOS:
        padded = modules.AppendHalos(n_halo=h)(torch.from_numpy(ids))
        out[f"padded_{h}"] = padded.numpy()[0]
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "append_halos_reference.npz"), "wb") as f:
        np.savez(f, **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
