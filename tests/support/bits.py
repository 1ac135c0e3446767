"""Comparisons of floating-point arrays whose names state their strength."""
import numpy as np


def bitwise(a, b):
    """Equal bit for bit as float64: signed zeros distinguished, every NaN
    equal to every NaN (payloads canonicalised), shapes equal."""
    a = np.where(np.isnan(a), np.nan, np.asarray(a, np.float64))
    b = np.where(np.isnan(b), np.nan, np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def equal_nan(a, b):
    """Equal values, NaN equal to NaN, shapes equal: +0 equals -0."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def ulps(a, b):
    """Distance in units of the last place of max(|a|, |b|) (NaN == NaN -> 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    a, b = np.nan_to_num(a), np.nan_to_num(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
    d[a == b] = 0
    return d
