"""The value checks the fitted models' `validate_*_conf` functions share.  Each raises ValueError naming the key and the
value it refused, and returns the value in the type the model keeps."""
import math

import numpy as np


def require(conf: dict, who: str, *keys):
    for key in keys:
        if key not in conf:
            raise ValueError(f'{who} conf needs {key}')


def number(key: str, v) -> float:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f'{key} = {v!r} must be a number')
    return float(v)


def positive(key: str, v) -> float:
    if not (math.isfinite(number(key, v)) and v > 0):
        raise ValueError(f'{key} = {v!r} must be finite and > 0')
    return float(v)


def integer(key: str, v, lo: int, hi=None) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f'{key} = {v!r} must be an integer')
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f'{key} = {v!r} must be ' + (f'>= {lo}' if hi is None else f'in [{lo}, {hi}]'))
    return int(v)
