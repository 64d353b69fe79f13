"""TEST INFRASTRUCTURE ONLY: the inputs of the emulator-training tests: head tables for
``fv3hip_train_emulator_loss_grad`` and its restatement, and the two end-to-end configurations with their synthetic data."""
import numpy as np

from fv3net_amd.ops import EmulatorHead


def make_heads(rng, rows, levels, layout, pad=0):
    """``(heads, F)``.  ``layout``: per head ``(kind, ncol, options)`` with the options ``scaled`` (bool), ``direct`` / ``after``
    (None, or ``("loss" | "metric", weight)``) and ``single_level``.  Slots are numbered in order of appearance.  The resident
    arrays are views with ``pad`` spare values per row.  ``before`` is temperature-like (~250) and the ``after`` target is
    ``before`` plus a difference of order one, so that the rounding of ``before + p`` is part of what is tested."""
    f32 = np.float32

    def resident(a):
        if not pad:
            return np.ascontiguousarray(a, f32)
        flat = a.reshape(a.shape[0], -1)
        full = np.full((flat.shape[0], flat.shape[1] + pad), 7.5, f32)
        full[:, :flat.shape[1]] = flat
        return full[:, :flat.shape[1]].reshape(a.shape)

    heads, col0, slot = [], 0, 0
    for kind, ncol, opt in layout:
        single = bool(opt.get("single_level", False))
        nt = ncol if kind == "mse" else levels
        inner = (levels, ncol) if kind == "xent" else (1,) if single else (nt,)
        h = EmulatorHead(kind=kind, col0=col0, ncol=ncol, single_level=single)
        if opt.get("scaled", False):
            h.scale, h.center = rng.uniform(0.5, 2.0, nt).astype(f32), rng.normal(0, 1, nt).astype(f32)
        if opt.get("direct") is not None:
            role, weight = opt["direct"]
            h.slot, h.weight, h.is_loss = slot, float(weight), role == "loss"
            slot += 1
            if kind == "xent":
                t = rng.uniform(0, 1, (rows,) + inner).astype(f32)
                hot = np.eye(ncol, dtype=f32)[rng.integers(0, ncol, (rows, levels))]
                t = np.where(rng.uniform(size=(rows, levels, 1)) < 0.6, hot, t)
                h.target = resident(t)
            else:
                h.target = resident(rng.normal(0, 2, (rows,) + inner).astype(f32))
                h.inv = rng.uniform(0.2, 3.0, nt).astype(f32)
        if opt.get("after") is not None:
            role, weight = opt["after"]
            h.slot_after, h.weight_after, h.is_loss_after = slot, float(weight), role == "loss"
            slot += 1
            before = rng.normal(250, 10, (rows,) + inner).astype(f32)
            h.before = resident(before)
            h.target_after = resident((before + rng.normal(0, 2, before.shape).astype(f32)).astype(f32))
            h.inv_after = rng.uniform(0.2, 3.0, nt).astype(f32)
        heads.append(h)
        col0 += ncol
    return heads, col0


def dense_loss_case(rng, rows=5, nfeat=3):
    """Direct + after terms on one head, both weighted; a metric-only after term; an unscaled output; a head in no loss term; a
    metric-only head."""
    layout = [("mse", nfeat, dict(scaled=True, direct=("loss", 2.0), after=("loss", 0.5))),
              ("mse", nfeat, dict(scaled=True, direct=("loss", 1.0), after=("metric", 1.0))),
              ("mse", 1, dict(scaled=False, direct=("loss", 3.0))),
              ("mse", nfeat, dict(scaled=True)),
              ("mse", 2, dict(scaled=True, direct=("metric", 1.0)))]
    return make_heads(rng, rows, 1, layout)


def local_loss_case(rng, rows=3, levels=4):
    """A two-term local head, a single-level head and a 4-channel cross-entropy head whose first three truth rows are one-hot,
    soft and all zero."""
    layout = [("mse_local", 1, dict(scaled=True, direct=("loss", 1.5), after=("metric", 1.0))),
              ("mse_local", 1, dict(scaled=True, direct=("loss", 0.7), single_level=True)),
              ("xent", 4, dict(direct=("loss", 2.0)))]
    heads, f = make_heads(rng, rows, levels, layout)
    t = heads[2].target
    t[0] = np.eye(4, dtype=np.float32)[np.arange(levels) % 4]
    t[1] = rng.dirichlet(np.ones(4), levels).astype(np.float32)
    t[2] = 0.0
    return heads, f


# ---- the end-to-end configurations ------------------------------------------------------------------------------------------------
def dense_config(batch_size=256, epochs=3, seed=0, width=8):
    """4 sources + 2 log inputs -> 8 -> 8 -> 4 heads; two Differences, the temperature one trained on its ``after`` field."""
    return {
        "batch_size": batch_size, "epochs": epochs, "valid_freq": 2, "seed": seed, "use_wandb": False,
        "tensor_transform": [
            {"to": "log_cloud_input", "source": "cloud_water_mixing_ratio_input", "transform": {"epsilon": 1e-10}},
            {"to": "log_humidity_input", "source": "specific_humidity_input", "transform": {"epsilon": 1e-8}},
            {"to": "temperature_gscond_difference", "before": "air_temperature_input", "after": "air_temperature_after_gscond"},
            {"to": "humidity_gscond_difference", "before": "specific_humidity_input", "after": "specific_humidity_after_gscond"},
        ],
        "loss": {
            "optimizer": {"name": "Adam", "kwargs": {"learning_rate": 0.01}},
            "loss_variables": ["air_temperature_after_gscond", "humidity_gscond_difference", "total_precipitation", "cloud_flag"],
            "metric_variables": ["specific_humidity_after_gscond", "temperature_gscond_difference"],
            "weights": {"air_temperature_after_gscond": 2.0, "cloud_flag": 0.5},
            "normalization_map": {"total_precipitation": {"scale": "per_feature", "center": "none", "epsilon": 1e-9}},
        },
        "model": {
            "architecture": {"name": "dense", "kwargs": {"width": width, "depth": 2}},
            "input_variables": ["air_temperature_input", "specific_humidity_input", "cloud_water_mixing_ratio_input", "log_cloud_input",
                                "log_humidity_input", "pressure_thickness_of_atmospheric_layer"],
            "direct_out_variables": ["temperature_gscond_difference", "humidity_gscond_difference", "total_precipitation"],
            "unscaled_outputs": ["cloud_flag"],
            "normalize_default": {"center": "per_feature", "scale": "all"},
            "normalize_map": {"pressure_thickness_of_atmospheric_layer": {"center": "all", "scale": "all_center_all"}},
        },
    }


def local_config(batch_size=128, epochs=3, seed=0, width=8):
    """6 inputs -> 8 -> 8 -> one regression head + one 4-channel logit head."""
    return {
        "batch_size": batch_size, "epochs": epochs, "valid_freq": 2, "seed": seed, "use_wandb": False,
        "tensor_transform": [
            {"to": "log_cloud_input", "source": "cloud_water_mixing_ratio_input", "transform": {"epsilon": 1e-10}},
            {"to": "log_humidity_input", "source": "specific_humidity_input", "transform": {"epsilon": 1e-8}},
            {"to": "humidity_gscond_difference", "before": "specific_humidity_input", "after": "specific_humidity_after_gscond"},
        ],
        "loss": {
            "optimizer": {"name": "Adam", "kwargs": {"learning_rate": 0.01}},
            "loss_variables": ["humidity_gscond_difference"],
            "metric_variables": ["specific_humidity_after_gscond"],
            "logit_variables": ["gscond_classes"],
            "weights": {"gscond_classes": 1.0},
        },
        "model": {
            "architecture": {"name": "dense-local", "kwargs": {"width": width, "depth": 2}, "output_channels": {"gscond_classes": 4}},
            "input_variables": ["air_temperature_input", "specific_humidity_input", "cloud_water_mixing_ratio_input", "log_cloud_input",
                                "log_humidity_input", "surface_air_pressure"],
            "direct_out_variables": ["humidity_gscond_difference"],
            "unscaled_outputs": ["gscond_classes"],
            "normalize_default": {"center": "per_feature", "scale": "all"},
        },
    }


def state(rows, nz=5, seed=0):
    """A synthetic microphysics state and its targets: smooth functions of the inputs plus noise, so that training has something
    to learn.  Every field the two configurations name."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    z = np.linspace(0.0, 1.0, nz)
    t = (220 + 70 * z + rng.normal(0, 5, (rows, nz))).astype(f32)
    q = (1e-3 * np.exp(3 * z) * rng.uniform(0.2, 1.5, (rows, nz))).astype(f32)
    qc = np.where(rng.uniform(size=(rows, nz)) < 0.4, 0.0, 1e-4 * rng.uniform(0, 1, (rows, nz))).astype(f32)
    delp = (1000 + 200 * rng.uniform(-1, 1, (rows, nz))).astype(f32)
    ps = (1e5 + 2e3 * rng.normal(0, 1, rows)).astype(f32)
    signal = np.tanh((t - 255) / 20) * (q / q.mean())
    dq = (-2e-4 * signal * (qc > 0) + 2e-5 * rng.normal(0, 1, (rows, nz))).astype(f32)
    dt = (-2500.0 * dq + 0.05 * rng.normal(0, 1, (rows, nz))).astype(f32)
    precip = (np.maximum(-dq, 0).sum(axis=1) * 10 + 1e-5 * rng.uniform(0, 1, rows)).astype(f32)
    klass = np.where(qc == 0, 0, np.where(dq > 2e-5, 1, np.where(dq < -2e-5, 2, 3)))
    return {
        "air_temperature_input": t, "specific_humidity_input": q, "cloud_water_mixing_ratio_input": qc,
        "pressure_thickness_of_atmospheric_layer": delp, "surface_air_pressure": ps,
        "air_temperature_after_gscond": (t + dt).astype(f32), "specific_humidity_after_gscond": (q + dq).astype(f32),
        "total_precipitation": precip, "cloud_flag": (qc > 0).mean(axis=1, keepdims=True).astype(f32),
        "gscond_classes": np.eye(4, dtype=f32)[klass],
    }


def batches(rows, nz=5, seed=0, n_batches=2):
    """``state`` cut into ``n_batches`` mappings, the shape ``train_batches`` has."""
    s = state(rows, nz, seed)
    cuts = np.linspace(0, rows, n_batches + 1).astype(int)
    return [{k: v[a:b] for k, v in s.items()} for a, b in zip(cuts[:-1], cuts[1:])]
