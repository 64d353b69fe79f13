"""The kernels of csrc/forest_train.hip one level at a time on the MI355X, through ``fv3hip_forest_train_begin`` / ``_level`` on a
workspace this file allocates itself, against ``forest_level_np`` (plain numpy and Python integers).

Every buffer has exactly the size the header states and lies between two guard bands of 64 elements inside the same allocation;
before each call every output and scratch buffer is filled with poison (NaN for doubles, 0x7f bytes for integers), so a level
that read what it had not been given, or wrote past what it owns, shows.  The cases (``forest_level_cases``) have whole-number
targets and weights with every sum below 2^53 (asserted on the CPU in ``test_host_forest_train_levels.py``): the device's sums
are exact whatever their order and **every output is compared bit for bit** -- node statistics, all m x F proxies, the best
position per (node, feature), the split records, the children, the partitioned lists -- except the impurity, which is allowed
``(3 O + 2) 2^-53 Q / (W O)`` (three roundings per output plus two, each of at most Q / W; exactly 0 for a pure node).  One case
with real-valued targets checks the sums against ``np.longdouble`` within ``4 n 2^-53 max|w y|`` and the proxies through the
splits they decide, which that case's seed makes unambiguous."""
import ctypes
import math

import numpy as np
import pytest
import torch

import forest_level_cases as LC
import forest_level_np as L
from fv3net_amd import _lib
from fv3net_amd.ops import _stream

pytestmark = pytest.mark.gpu

GUARD = 64            # elements on either side of every buffer
SENTINEL = 0xA5       # the guard bands' bytes
POISON = 0x7F         # the bytes of a poisoned integer buffer

_TORCH = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i64": torch.int64, "u8": torch.uint8}
_POISON_INT = {torch.int32: 0x7F7F7F7F, torch.int64: 0x7F7F7F7F7F7F7F7F, torch.uint8: 0x7F}
INPUTS = ("xt", "y", "ysq", "order", "weight")
TREE = ("left", "right", "feature", "threshold", "missing_left", "value", "impurity", "weighted_n", "n_samples")


class Buffer:
    """``shape`` elements of ``dtype`` between two guard bands, all in one allocation."""

    def __init__(self, shape, dtype, device):
        self.dtype, self.shape = dtype, tuple(int(v) for v in shape)
        size = torch.empty(0, dtype=dtype).element_size()
        count = math.prod(self.shape)
        assert count >= 1
        self.raw = torch.full(((count + 2 * GUARD) * size,), SENTINEL, dtype=torch.uint8, device=device)
        self.body = self.raw[GUARD * size:(GUARD + count) * size]
        self.t = self.body.view(dtype).view(self.shape)
        self.band = GUARD * size

    def poison(self):
        if self.dtype.is_floating_point:
            self.t.fill_(float("nan"))
        else:
            self.body.fill_(POISON)

    def set(self, array):
        """``array`` into the leading entries (of the flattened rows for a 2-d buffer: [:, :array.shape[1]])."""
        a = torch.from_numpy(np.ascontiguousarray(array)).to(self.t.dtype)
        if a.ndim == 2:
            self.t[:a.shape[0], :a.shape[1]] = a.to(self.t.device)
        else:
            self.t[:a.shape[0]] = a.to(self.t.device)

    def get(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        return bool((self.raw[:self.band] == SENTINEL).all() and (self.raw[-self.band:] == SENTINEL).all())


def poisoned(values):
    """Elementwise: does the entry still hold the poison."""
    values = np.asarray(values)
    if values.dtype.kind == "f":
        return np.isnan(values)
    return values == _POISON_INT[getattr(torch, values.dtype.name)]


class Workspace:
    """``fv3hip_forest_train_t`` with every buffer at the size the header states."""

    def __init__(self, n, F, O, k_cap, node_cap, device):
        self.n, self.F, self.O, self.k_cap, self.node_cap, self.device = n, F, O, k_cap, node_cap, device
        chunk = int(_lib.load().fv3hip_forest_train_chunk())
        assert chunk == LC.C
        chunks = -(-n // chunk)
        sizes = {
            "xt": ((F, n), "f32"), "y": ((n, O), "f64"), "ysq": ((n,), "f64"), "order": ((F, n), "i32"), "weight": ((n,), "i32"),
            "list_a": ((F, n), "i32"), "list_b": ((F, n), "i32"), "side": ((n,), "u8"), "pos_node": ((n,), "i32"),
            "seg_a": ((k_cap + 1,), "i64"), "seg_b": ((k_cap + 1,), "i64"), "node_a": ((k_cap,), "i32"), "node_b": ((k_cap,), "i32"),
            "stats": ((k_cap, O + 2), "f64"), "carry": ((F, chunks, O + 2), "f64"), "count": ((F, chunks), "i32"),
            "proxy": ((F, n), "f64"), "best_proxy": ((k_cap, F), "f64"), "best_pos": ((k_cap, F), "i64"),
            "n_left": ((k_cap,), "i64"), "dst_left": ((k_cap,), "i64"), "dst_right": ((k_cap,), "i64"),
            "left": ((node_cap,), "i32"), "right": ((node_cap,), "i32"), "feature": ((node_cap,), "i32"),
            "threshold": ((node_cap,), "f64"), "missing_left": ((node_cap,), "u8"), "value": ((node_cap, O), "f64"),
            "impurity": ((node_cap,), "f64"), "weighted_n": ((node_cap,), "f64"), "n_samples": ((node_cap,), "i32"),
            "level": ((4,), "i64"),
        }
        self.b = {name: Buffer(shape, _TORCH[kind], device) for name, (shape, kind) in sizes.items()}
        self.ws = _lib.ForestTrain()
        self.ws.n, self.ws.F, self.ws.O, self.ws.k_cap, self.ws.node_cap = n, F, O, k_cap, node_cap
        for name, buf in self.b.items():
            setattr(self.ws, name, buf.t.data_ptr())
        for name in self.b:
            if name not in INPUTS:
                self.b[name].poison()

    def load(self, X, y, weight):
        xt = np.ascontiguousarray(np.asarray(X, np.float32).T)
        self.b["xt"].set(xt)
        self.b["y"].set(y)
        self.b["ysq"].set(np.cumsum(y * y, axis=1)[:, -1].copy())
        self.b["order"].set(np.argsort(xt, axis=1, kind="stable").astype(np.int32))
        self.b["weight"].set(np.asarray(weight, np.int32))

    def poison_for_level(self, parity):
        """Everything a level writes or uses as scratch; the tree arrays keep the records of the nodes that exist."""
        nxt = "a" if parity else "b"
        for name in ("list_" + nxt, "seg_" + nxt, "node_" + nxt, "side", "pos_node", "stats", "carry", "count", "proxy", "best_proxy",
                     "best_pos", "n_left", "dst_left", "dst_right", "level"):
            self.b[name].poison()

    def begin(self, n_inbag):
        with torch.cuda.device(self.device):
            _lib.call("fv3hip_forest_train_begin", ctypes.byref(self.ws), n_inbag, _stream(self.device))
            torch.cuda.synchronize()

    def level(self, parity, n_open, n_positions, n_nodes, depth, max_depth, min_split, min_leaf, phases=(_lib.FOREST_TRAIN_ALL,)):
        with torch.cuda.device(self.device):
            for flags in phases:
                _lib.call("fv3hip_forest_train_level", ctypes.byref(self.ws), parity, n_open, n_positions, n_nodes, depth, max_depth,
                          min_split, min_leaf, flags, _stream(self.device))
            torch.cuda.synchronize()

    def assert_guards(self):
        broken = [name for name, buf in self.b.items() if not buf.guards_intact()]
        assert not broken, f"guard bands overwritten around {broken}"


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(np.asarray(want).astype(got.dtype))
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=f"{what} (compared as bytes)")


def _check_level(w, case, step, written):
    """The buffers after one level against the reference's result ``step``."""
    r, parity = step["result"], step["parity"]
    nxt = "a" if parity else "b"
    node = step["node"].astype(np.int64)
    K, m, O = node.shape[0], int(step["seg"][-1]), w.O
    got = {name: buf.get() for name, buf in w.b.items()}
    w.assert_guards()
    n_next, m_next = int(r["level"][0]), int(r["level"][1])

    _same_bits(got["level"], r["level"], "level")
    if case.exact:
        _same_bits(got["stats"][:K], r["stats"], "stats")
        _same_bits(got["value"][node], r["value"], "value")
        tolerance = (3 * O + 2) * 2.0 ** -53 * r["impurity_scale"]
        error = np.abs(got["impurity"][node] - r["impurity"])
        worst = int(np.argmax(error - tolerance))
        print(f"{case.name}: impurity error {error[worst]:.3e} at node {node[worst]}, allowed {tolerance[worst]:.3e}")
        assert (error <= tolerance).all()
        ids0 = step["list"][0]
        for k in range(K):
            rows = case.y[ids0[step["seg"][k]:step["seg"][k + 1]]]
            if (rows == rows[0]).all():
                assert got["impurity"][node[k]] == 0.0 and r["impurity"][k] == 0.0, f"pure node {node[k]}"
    else:
        bound = 4 * case.X.shape[0] * 2.0 ** -53 * np.abs(case.weight[:, None] * case.y).max()
        errors = [np.abs(got["stats"][:K] - r["stats"]).max(), np.abs(got["value"][node] - r["value"]).max(),
                  np.abs(got["impurity"][node] - r["impurity"]).max()]
        print(f"{case.name}: stats, value, impurity errors {errors[0]:.3e}, {errors[1]:.3e}, {errors[2]:.3e}; bound {bound:.3e}")
        assert max(errors) <= bound
        _same_bits(got["stats"][:K, O], r["stats"][:, O], "weights")
    assert poisoned(got["stats"][K:]).all()
    _same_bits(got["weighted_n"][node], r["weighted_n"], "weighted_n")
    _same_bits(got["n_samples"][node], r["n_samples"], "n_samples")

    if r["proxy"] is None:   # a final level searches nothing
        for name in ("proxy", "best_proxy", "best_pos", "list_" + nxt):
            assert poisoned(got[name]).all(), f"{name} written at the final depth"
    else:
        if case.exact:
            _same_bits(got["proxy"][:, :m], r["proxy"], "proxy")
            _same_bits(got["best_proxy"][:K], r["best_proxy"], "best_proxy")
            _same_bits(got["best_pos"][:K], r["best_pos"], "best_pos")
        else:
            np.testing.assert_array_equal(np.isfinite(got["proxy"][:, :m]), np.isfinite(r["proxy"]))
        assert poisoned(got["proxy"][:, m:]).all() and poisoned(got["best_proxy"][K:]).all() and poisoned(got["best_pos"][K:]).all()

    for name in ("feature", "threshold", "missing_left", "left", "right"):
        _same_bits(got[name][node], r[name], name)
    _same_bits(got["n_left"][:K], r["n_left"], "n_left")
    assert poisoned(got["n_left"][K:]).all()
    written |= set(node.tolist())
    untouched = np.setdiff1d(np.arange(w.node_cap), np.fromiter(written, np.int64))
    for name in TREE:
        assert poisoned(got[name][untouched]).all(), f"{name} written outside the level's nodes"

    _same_bits(got["seg_" + nxt][:n_next + 1], r["seg_next"], "seg_next")
    _same_bits(got["node_" + nxt][:n_next], r["node_next"], "node_next")
    assert poisoned(got["seg_" + nxt][n_next + 1:]).all() and poisoned(got["node_" + nxt][n_next:]).all()
    if r["proxy"] is not None:
        _same_bits(got["list_" + nxt][:, :m_next], r["list_next"], "list_next")
        assert poisoned(got["list_" + nxt][:, m_next:]).all()
    # what the level was given is as it was
    cur = "b" if parity else "a"
    _same_bits(got["list_" + cur][:, :m], step["list"], "the level's own lists")
    _same_bits(got["seg_" + cur][:K + 1], step["seg"], "the level's own segments")


def _run_case(device, case, phases=(_lib.FOREST_TRAIN_ALL,)):
    ref = LC.reference(case.name)
    steps = ref["steps"]
    if case.exact:   # in Python integers: no sum or sum of squares reaches 2^53, so the device's are exact in any order
        assert max(s["result"]["max_int"] for s in steps) < L.EXACT_LIMIT
    n, F = case.X.shape
    k_cap, node_cap = LC.caps(case.name)
    w = Workspace(n, F, case.y.shape[1], k_cap, node_cap, device)
    w.load(case.X, case.y, case.weight)
    first = steps[0]
    if ref["begin"] is not None:
        m = int(ref["begin"]["level"][1])
        w.begin(m)
        w.assert_guards()
        got = {name: w.b[name].get() for name in ("list_a", "seg_a", "node_a", "level")}
        _same_bits(got["list_a"][:, :m], ref["begin"]["list"], "list_a after begin")
        _same_bits(got["list_a"][:, :m], np.stack([row[case.weight[row] > 0] for row in ref["order"]]), "order filtered by weight > 0")
        assert poisoned(got["list_a"][:, m:]).all()
        _same_bits(got["seg_a"][:2], [0, m], "seg_a after begin")
        _same_bits(got["node_a"][:1], [0], "node_a after begin")
        _same_bits(got["level"], [1, m, 1, 0], "level after begin")
        for name in TREE + ("list_b", "node_b", "stats", "proxy", "best_proxy", "best_pos", "n_left"):
            assert poisoned(w.b[name].get()).all(), f"begin wrote {name}"
    else:
        cur = "b" if first["parity"] else "a"
        w.b["list_" + cur].set(first["list"])
        w.b["seg_" + cur].set(first["seg"])
        w.b["node_" + cur].set(first["node"])
    written = set()
    for step in steps:
        w.poison_for_level(step["parity"])
        w.level(step["parity"], len(step["node"]), int(step["seg"][-1]), step["n_nodes"], step["depth"], case.max_depth,
                case.min_samples_split, case.min_samples_leaf, phases)
        _check_level(w, case, step, written)


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_level_against_the_reference(device, case):
    _run_case(device, case)


@pytest.mark.parametrize("name", ["heads_at_chunk_and_tile_edges", "segment_over_four_chunks_final_depth", "open_nodes_1025",
                                  "begin_n257_alternating"])
def test_the_three_phases_in_three_calls_give_the_same(device, name):
    """FV3HIP_FOREST_TRAIN_SUMS, _SCAN and _SPLIT one call each, as benchmarks/forest_train.py times them."""
    _run_case(device, LC.BY_NAME[name], (_lib.FOREST_TRAIN_SUMS, _lib.FOREST_TRAIN_SCAN, _lib.FOREST_TRAIN_SPLIT))


@pytest.mark.parametrize("O", [3822, 4096])
def test_more_outputs_than_the_tile_holds_are_refused_by_both_entry_points(device, O):
    """One row of the scan's LDS tile holds at most 3821 outputs; ``begin`` must refuse what ``level`` cannot run, before any
    launch."""
    n = 8
    X, y, weight = LC.int_data(n, 1, O, 5)
    w = Workspace(n, 1, O, 1, 1, device)
    w.load(X, y, weight)
    outputs = [name for name in w.b if name not in INPUTS]
    with pytest.raises(_lib.Fv3HipError, match=r"output count must be in \[1, 3821\]"):
        w.begin(n)
    with pytest.raises(_lib.Fv3HipError, match=r"output count must be in \[1, 3821\]"):
        w.level(0, 1, n, 1, 0, -1, 2, 1)
    for name in outputs:
        assert poisoned(w.b[name].get()).all(), f"{name} written by a refused call"
    w.assert_guards()
