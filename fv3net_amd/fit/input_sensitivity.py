"""What ``Predictor.input_sensitivity`` returns (external/fv3fit/fv3fit/_shared/input_sensitivity.py): per-output Jacobians for
the differentiable models, feature importances for the random forests."""
import dataclasses
from typing import Mapping, Optional, Sequence

import numpy as np

# {output name: {input name: d output / d input, [nfeat_out, nfeat_in]}}
JacobianInputSensitivity = Mapping[str, Mapping[str, np.ndarray]]


@dataclasses.dataclass
class RandomForestInputSensitivity:
    """Importances of one input variable over the ensemble's trees: their mean and standard deviation per feature, and
    ``indices``, the position of each along the feature dimension (one NaN for a scalar input)."""

    mean_importances: Sequence[float]
    std_importances: Sequence[float]
    indices: Sequence[int]


RandomForestInputSensitivities = Mapping[str, RandomForestInputSensitivity]


@dataclasses.dataclass
class InputSensitivity:
    """One of the two is set, by the kind of model."""

    rf_feature_importances: Optional[RandomForestInputSensitivities] = None
    jacobians: Optional[JacobianInputSensitivity] = None


def nondimensionalize_jacobians(jacobians: JacobianInputSensitivity, std_factors: Mapping[str, np.ndarray]):
    """Every ``jacobians[out][in]`` times ``std_factors[in]`` along its columns and divided by ``std_factors[out]`` along its
    rows (numpy semantics: a zero output std gives inf / nan); an output without a factor raises ``KeyError``."""
    scaled = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for out_name, per_input in jacobians.items():
            inv = 1.0 / np.asarray(std_factors[out_name]).reshape(-1, 1)
            scaled[out_name] = {in_name: np.multiply(np.multiply(j, np.asarray(std_factors[in_name]).reshape(1, -1)), inv)
                                for in_name, j in per_input.items()}
    return scaled
