"""Diagnostics computed where the predictions are: on the device."""
from .offline import DIAGNOSTIC_NAMES, DOMAIN_CLASSES, OfflineDiagnostics, output_name, region_mask  # noqa: F401
