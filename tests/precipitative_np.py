"""numpy restatement of fv3fit's precipitative predict graph -- TEST INFRASTRUCTURE ONLY.

Follows (paths relative to the reference checkout) external/fv3fit/fv3fit/keras/_models/precipitative.py:
  :192-238  the network: clipped, normalised inputs -> Dense(relu) x (depth-1) -> linear heads, denormalised; the
            column-precipitation head with dQ2's mean and std (evaluated by ``oracle.mlp_np.forward`` on the spec)
  :35-66    IntegratePrecipLayer (-1/g * reduce_sum(cp * delp)), CondensationalHeatingLayer (-LV/CPD * cp)
  :239-253  the closure: the two Adds under couple_precip_to_dQ1_dQ2, physics_precip + the integral of the RAW delp

The graph's constants are float32 (``tf.constant(..., dtype=dQ2.dtype)``).  TensorFlow leaves the order of ``reduce_sum``
open; the project fixes it -- float32 products, each rounded, added into a float32 accumulator from +0 over ascending
levels -- and ``closure32`` is that order, so the kernel is compared with it bit for bit.  In float64 the same expression
(float32 constants and inputs, float64 arithmetic, numpy's float64 sum) is the truth the float32 paths are measured against.
"""
import numpy as np

from oracle import mlp_np

LV, CPD, GRAVITY = 2.5e6, 1004.6, 9.80665   # precipitative.py:21-24
C_HEAT = np.float32(-LV / CPD)
C_G = np.float32(-1.0 / GRAVITY)

DELP, PHYS_PRECIP = "pressure_thickness_of_atmospheric_layer", "physics_precip"
T_RES, Q_RES, COL_PRECIP, PRECIP = "dQ1", "dQ2", "q_tendency_due_to_precip", "total_precipitation_rate"


def closure32(t_res, q_res, cp, delp, pp, couple):
    """The closure on ``[nz, n]`` float32 heads, ``delp`` ``[nz, n]`` and ``pp`` ``[n]`` (float32 or float64: cast to float32
    first, as Keras casts its inputs): (dQ1, dQ2, precip), every operation rounded to float32, the integral a sequential
    loop over the levels.  Without ``couple`` the residual heads come back as they are (they may be None)."""
    cp = np.asarray(cp, np.float32)
    d = np.asarray(delp).astype(np.float32)
    acc = np.zeros(cp.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for k in range(cp.shape[0]):
            acc = acc + cp[k] * d[k]
        precip = np.asarray(pp).astype(np.float32) + C_G * acc
        if not couple:
            return t_res, q_res, precip
        dq1 = np.asarray(t_res, np.float32) + C_HEAT * cp
        dq2 = np.asarray(q_res, np.float32) + cp
    assert dq1.dtype == dq2.dtype == precip.dtype == np.float32
    return dq1, dq2, precip


def closure64(t_res, q_res, cp, delp, pp, couple):
    """The same expression in float64 on ``[nz, n]`` arrays: float32 constants, ``delp`` and ``pp`` cast to float32 first."""
    cp = np.asarray(cp, np.float64)
    d = np.asarray(delp).astype(np.float32).astype(np.float64)
    precip = np.asarray(pp).astype(np.float32).astype(np.float64) + np.float64(C_G) * np.sum(cp * d, axis=0)
    if not couple:
        return t_res, q_res, precip
    return np.asarray(t_res, np.float64) + np.float64(C_HEAT) * cp, np.asarray(q_res, np.float64) + cp, precip


def forward(spec, couple, sources, dtype=np.float32):
    """The whole predict graph.  ``sources``: name -> ``[sample, feature]`` (or ``[sample]``) arrays as for
    ``mlp_np.forward``.  Returns ``dQ1``, ``dQ2`` ``[sample, nz]``, ``total_precipitation_rate`` ``[sample]`` and the
    column-precipitation head ``q_tendency_due_to_precip`` ``[sample, nz]`` (the gates scale with it).  float64: the truth;
    float32: the bit pattern the device computes from the same heads."""
    heads = mlp_np.forward(spec, sources, dtype=dtype)
    delp = np.asarray(sources[DELP])                      # raw: every level, whatever the network's clip
    pp = np.asarray(sources[PHYS_PRECIP]).reshape(delp.shape[0])
    close = closure32 if np.dtype(dtype) == np.float32 else closure64
    dq1, dq2, precip = close(heads[T_RES].T, heads[Q_RES].T, heads[COL_PRECIP].T, delp.T, pp, couple)
    return {T_RES: dq1.T, Q_RES: dq2.T, PRECIP: precip, COL_PRECIP: heads[COL_PRECIP]}
