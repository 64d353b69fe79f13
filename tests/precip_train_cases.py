"""Inputs shared by tests/test_host_precip_train.py and the two GPU files of the precipitative training step (DESIGN.md section
25): synthetic training columns, and the arguments of one ``fv3hip_train_precip_loss_grad`` launch."""
import functools

import numpy as np

from fv3net_amd.xr_compat import DataArray, Dataset

T_NAME, Q_NAME, DELP, PP = "air_temperature", "specific_humidity", "pressure_thickness_of_atmospheric_layer", "physics_precip"
INPUTS = [T_NAME, Q_NAME, DELP, PP]
OUTPUTS = ["dQ1", "dQ2", "total_precipitation_rate"]


@functools.lru_cache(maxsize=None)
def batches(nz=79, ny=32, nx=64, seed=2025):
    """``ny * nx`` columns: T, q, delp on ``nz`` levels and physics_precip in; the targets a fixed smooth (random two-layer
    tanh) function of the inputs at the scales of the real ones (dQ1 ~ 1e-4 K/s, dQ2 ~ 1e-7 kg/kg/s, precipitation ~ 1e-4)."""
    rng = np.random.default_rng(seed)
    t = (250 + 30 * rng.normal(0, 1, (nz, ny, nx))).astype(np.float32)
    q = np.abs(1e-3 * rng.normal(0, 1, (nz, ny, nx))).astype(np.float32)
    delp = rng.uniform(300, 1500, (nz, ny, nx)).astype(np.float32)
    pp = rng.uniform(0, 1e-4, (ny, nx)).astype(np.float32)
    x = np.concatenate([(t - 250) / 30, q / 1e-3 - 0.8, (delp - 900) / 350, pp[None] / 1e-4 - 0.5]).reshape(3 * nz + 1, -1).T
    w1, w2 = rng.normal(0, 1, (3 * nz + 1, 6)) / np.sqrt(3 * nz + 1), rng.normal(0, 1, (6, 2 * nz + 1))
    y = (np.tanh(x @ w1) @ w2).T.reshape(2 * nz + 1, ny, nx)
    dims = ["z", "y", "x"]
    ds = Dataset({T_NAME: DataArray(t, dims=dims), Q_NAME: DataArray(q, dims=dims), DELP: DataArray(delp, dims=dims),
                  PP: DataArray(pp, dims=["y", "x"]),
                  "dQ1": DataArray((1e-4 * y[:nz]).astype(np.float32), dims=dims),
                  "dQ2": DataArray((1e-7 * y[nz:2 * nz]).astype(np.float32), dims=dims),
                  "total_precipitation_rate": DataArray((pp + 2e-5 * y[2 * nz]).astype(np.float32), dims=["y", "x"])})
    return (ds,)


def columns(name, **kw):
    """``[sample, feature]`` of one variable of ``batches(**kw)``."""
    v = batches(**kw)[0][name].values
    return v.reshape(v.shape[0], -1).T if v.ndim == 3 else v.reshape(-1, 1)


def launch_inputs(n, nz, has_dead=False, rows=None, seed=0):
    """The arrays of one launch, float32, at the scales of a freshly initialised network on real data: raw heads of order one,
    de-normalisation over two decades, thicknesses of hundreds of Pa.  ``rows`` resident rows (default ``n``)."""
    rng = np.random.default_rng([seed, n, nz, int(has_dead)])
    rows = n if rows is None else rows
    f32 = np.float32
    a = dict(
        yhat=rng.normal(0, 1, (n, 3 * nz + int(has_dead))).astype(f32),
        scale1=(1e-4 * 10.0 ** rng.uniform(-1, 1, nz)).astype(f32), center1=rng.normal(0, 1e-4, nz).astype(f32),
        scale2=(1e-7 * 10.0 ** rng.uniform(-1, 1, nz)).astype(f32), center2=rng.normal(0, 1e-7, nz).astype(f32),
        delp=rng.uniform(300, 1500, (rows, nz)).astype(f32), pp=rng.uniform(0, 1e-4, rows).astype(f32),
        t1=rng.normal(0, 1e-4, (rows, nz)).astype(f32), t2=rng.normal(0, 1e-7, (rows, nz)).astype(f32),
        t3=rng.uniform(0, 2e-4, rows).astype(f32))
    a["inv1"] = (1.0 / a["scale1"].astype(np.float64) ** 2).astype(f32)
    a["inv2"] = (1.0 / a["scale2"].astype(np.float64) ** 2).astype(f32)
    a["inv3"] = float(f32(1.0 / 3e-5 ** 2))
    return a


def reference_args(a):
    """``a`` in the positional order of ``precip_train_np.loss_grad``."""
    return [a[k] for k in ("yhat", "scale1", "center1", "scale2", "center2", "inv1", "inv2", "inv3", "delp", "pp", "t1", "t2", "t3")]
