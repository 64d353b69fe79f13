"""A float64 numpy restatement of fv3fit's reservoir training (readout.py:19-70, utils.py:40-96, train.py:165-396), the
checker of the device path.  Built on ``reservoir_np``'s ``increment`` and ``encode``: a model is the
same dictionary, of which training reads the divider, the transformers, the masks, ``w_in`` and ``w_res``.

  - BatchLinearRegressor: A += X1.T X1, B += X1.T y with X1 = [X, 1] when the bias is added; W = solve(A + l2 I, B) or
    lstsq; coefficients = W[:-1], intercepts = W[-1];
  - SynchronizationTracker: complete only once MORE than n_synchronize steps are counted; the trim keeps
    arr[-steps_past_sync:] (all of arr when that is longer than arr);
  - per batch: the state series of one increment per time step (noise, when given, is added to the encoded input before the
    input mask), X = states[:-1] with even ELEMENTS squared (axis -1) when asked, then hybrid[:-1]; Y = targets[1:], the
    output transformer's encoding of the outputs without their halo; both trimmed, then one update per subdomain.
"""
import numpy as np

import reservoir_np as R


class NotFittedError(Exception):
    pass


class BatchLinearRegressor:
    def __init__(self, l2, add_bias_term=True, use_least_squares_solve=False):
        self.l2, self.add_bias_term, self.use_least_squares_solve = l2, add_bias_term, use_least_squares_solve
        self.A = self.B = None

    def batch_update(self, X, y):
        X, y = np.asarray(X, np.float64), np.asarray(y, np.float64)
        if self.add_bias_term:
            X = np.concatenate([X, np.ones((X.shape[0], 1))], axis=1)
        elif not np.allclose(np.unique(X[:, -1]), np.array([1.0])):
            raise ValueError("Last column of X array must all be ones if add_bias_term is False.")
        if self.A is None:
            self.A = np.zeros((X.shape[1], X.shape[1]))
            self.B = np.zeros((X.shape[1], y.shape[1]))
        self.A = self.A + X.T @ X
        self.B = self.B + X.T @ y

    def get_weights(self):
        if self.A is None:
            raise NotFittedError("At least one call of batch_update on data must be done before solving for weights.")
        lhs = self.A + self.l2 * np.identity(self.A.shape[1])
        W = np.linalg.lstsq(lhs, self.B, rcond=None)[0] if self.use_least_squares_solve else np.linalg.solve(lhs, self.B)
        return W[:-1, :], W[-1, :]


class SynchronizationTracker:
    def __init__(self, n_synchronize):
        self.n_synchronize, self.n_steps_synchronized = n_synchronize, 0

    @property
    def completed_synchronization(self):
        return self.n_steps_synchronized > self.n_synchronize

    def count_synchronization_steps(self, n_samples):
        self.n_steps_synchronized += n_samples

    def trim_synchronization_samples_if_needed(self, arr):
        if not self.completed_synchronization:
            return np.array([])
        steps_past_sync = self.n_steps_synchronized - self.n_synchronize
        return arr if steps_past_sync > len(arr) else arr[-steps_past_sync:]


def construct_readout_inputs_outputs(states, targets, square_even_inputs, hybrid=None):
    """[time, subdomain, feature] series to (X, Y) (train.py:379-396)."""
    X = states[:-1]
    if square_even_inputs:
        X = R.square_even_terms(X, axis=-1)
    if hybrid is not None:
        X = np.concatenate((X, hybrid[:-1]), axis=-1)
    return X, targets[1:]


def trim_halo(arr, overlap):
    """[t, x, y, z] without its halo."""
    return arr[:, overlap:arr.shape[1] - overlap, overlap:arr.shape[2] - overlap] if overlap else arr


def increment(m, state, arrays, noise=None):
    """``reservoir_np.increment``, with ``noise`` [subdomain, input] added to the encoded input before the input mask
    (train.py:373-374, reservoir.py:74-80)."""
    if noise is None:
        return R.increment(m, state, arrays)
    u = R.blocks(R.encode(m["input"], arrays), m["layout"], m["overlap"]) + noise
    if m.get("input_mask") is not None:
        u = u * m["input_mask"]
    return np.tanh(R._matmul_t(u, m["w_in"]) + R._matmul_t(state, m["w_res"]))


def state_series(m, state, inputs, noise=None):
    """One increment per time step of the [t, x, y, z] arrays: ([t, subdomain, state], the last state)."""
    out = []
    for t in range(inputs[0].shape[0]):
        state = increment(m, state, [a[t] for a in inputs], None if noise is None else noise[t])
        out.append(state)
    return np.array(out), state


def encoded_series(m, tf, arrays, mask=None):
    """The encoding of [t, x, y, z] arrays over the rank extent without overlap: [t, subdomain, feature]."""
    out = np.array([R.blocks(R.encode(tf, [a[t] for a in arrays]), m["layout"], 0) for t in range(arrays[0].shape[0])])
    return out if mask is None else out * mask


def train(m, sequences, input_variables, output_variables, n_synchronize, l2, hybrid_variables=None, square=False,
          noises=None):
    """The training loop over ``sequences`` (a list of lists of batches, each a dict of [t, x, y, z] arrays with overlap).
    ``noises``: one [t, subdomain, input] array per batch, in the order the batches are visited, or None.  Returns a dict
    with the per-subdomain regressors, ``coefficients`` [subdomain, feature, out], ``intercepts`` [subdomain, out], the
    last ``state``, and the samples that entered the regression, ``X`` and ``Y`` [sample, subdomain, feature]."""
    ns = m["layout"][0] * m["layout"][1]
    regressors = [BatchLinearRegressor(l2) for _ in range(ns)]
    noises = iter(noises) if noises is not None else None
    state, samples = None, []
    for batches in sequences:
        tracker = SynchronizationTracker(n_synchronize)
        for b, batch in enumerate(batches):
            if b == 0:
                state = np.zeros((ns, m["w_res"][3][0]))
            noise = next(noises) if noises is not None else None
            states, state = state_series(m, state, [batch[v] for v in input_variables], noise)
            targets = encoded_series(m, m["output"], [trim_halo(batch[v], m["overlap"]) for v in output_variables])
            tracker.count_synchronization_steps(len(states))
            hybrid = None
            if hybrid_variables is not None:
                hybrid = encoded_series(m, m["hybrid"], [trim_halo(batch[v], m["overlap"]) for v in hybrid_variables],
                                        m.get("hybrid_mask"))
            X, Y = construct_readout_inputs_outputs(states, targets, square, hybrid)
            if tracker.completed_synchronization:
                X = tracker.trim_synchronization_samples_if_needed(X)
                Y = tracker.trim_synchronization_samples_if_needed(Y)
                samples.append((X, Y))
                for s, regressor in enumerate(regressors):
                    regressor.batch_update(X[:, s], Y[:, s])
    weights = [r.get_weights() for r in regressors]
    return {"regressors": regressors, "coefficients": np.stack([w[0] for w in weights]),
            "intercepts": np.stack([w[1] for w in weights]), "state": state,
            "X": np.concatenate([x for x, _ in samples]), "Y": np.concatenate([y for _, y in samples])}
