"""The configurations on which the GPU random-forest trainer is compared with sklearn and with ``forest_train_np``; shared by
``test_gpu_forest_train.py`` and, for the CPU check that no decision in them hangs on the order of a sum (the restatement's
pairwise twin partitions alike), ``test_host_forest_train.py``.

Sizes are the smallest at which the kernels can go wrong: the scan works in chunks of 256 list positions and LDS tiles of 32,
one thread per output column in blocks of 256; a bootstrap of n leaves about 0.63 n samples in bag.
"""
import dataclasses
from typing import Optional, Union

import numpy as np


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    n: int
    F: int
    O: int
    max_depth: Optional[int] = None
    min_samples_leaf: int = 1
    min_samples_split: int = 2
    bootstrap: bool = True
    max_samples: Union[int, float, None] = None
    grid: Optional[float] = None      # feature values rounded to multiples of it: heavy duplicates
    seed: int = 0
    n_trees: int = 2

    def params(self):
        return dict(max_depth=self.max_depth, min_samples_leaf=self.min_samples_leaf, min_samples_split=self.min_samples_split,
                    bootstrap=self.bootstrap, max_samples=self.max_samples)


CASES = [
    Case("one_sample", 1, 1, 1),
    Case("two_samples", 2, 5, 1, bootstrap=False),
    Case("n31_o64_depth6", 31, 5, 64, max_depth=6, seed=1),
    Case("n33_o65_to_single_samples", 33, 5, 65, bootstrap=False, seed=2),
    Case("n33_leaf17_binds", 33, 1, 1, min_samples_leaf=17, bootstrap=False, seed=3),
    Case("n300_leaf17", 300, 5, 1, min_samples_leaf=17, seed=4),
    Case("n300_stump", 300, 5, 1, max_depth=1, seed=5),
    Case("n300_f160_o158_depth6", 300, 160, 158, max_depth=6, seed=6, n_trees=1),
    Case("n1000_unlimited_leaf3", 1000, 5, 3, min_samples_leaf=3, seed=7),
    Case("n1000_o65_split10_half", 1000, 5, 65, max_depth=6, min_samples_split=10, max_samples=0.5, seed=8),
    Case("n1000_grid_no_bootstrap", 1000, 5, 2, bootstrap=False, grid=0.125, seed=9),
    Case("n100_o300_short_tile", 100, 3, 300, max_depth=5, seed=10),   # 302 columns: two per thread, an LDS tile of 24 rows
    # a level of more than 1024 open nodes (asserted in test_host_forest_train_levels.py): ft_children_kernel scans in rounds of
    # 1024 and carries the counts across them
    Case("n4096_over_1024_open_nodes", 4096, 2, 1, bootstrap=False, seed=24, n_trees=1),
    Case("n40_f300", 40, 300, 1, seed=12),   # more features than the 256 of one ft_count_carry_kernel block
]


def data(case: Case):
    rng = np.random.default_rng(1000 + case.seed)
    X = rng.normal(size=(case.n, case.F)).astype(np.float32)
    if case.grid:
        X = (np.round(X / case.grid) * case.grid).astype(np.float32)
    w = rng.normal(size=(case.F, case.O))
    y = np.tanh(X.astype(np.float64) @ w / np.sqrt(case.F)) + 0.1 * rng.normal(size=(case.n, case.O))
    return X, y
