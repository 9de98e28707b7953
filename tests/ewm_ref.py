"""The reference's ewm_mean loop restated in Python, for the ewm tests.

`ewm_mean_ref` is a literal reading of EwmMeanState::update_iter
(polars-compute/src/ewm/mean.rs:52), applied per segment, in any float type:
  float             the reference's f64 arithmetic, operation for operation (r64)
  numpy.float32     its Float32 path
  numpy.longdouble  the yardstick (r80; a 64-bit significand on x86-64)
`errors` measures a result against the yardstick in the units the tolerance
of DESIGN.md "Float tolerance against the reference" is stated in."""

import math

import numpy as np


def prepare_alpha(com=None, span=None, half_life=None, alpha=None):
    """The conversions of py-polars' _prepare_alpha (expr.py:11710)."""
    if com is not None:
        return 1.0 / (1.0 + com)
    if span is not None:
        return 2.0 / (span + 1.0)
    if half_life is not None:
        return 1.0 - math.exp(-math.log(2.0) / half_life)
    return alpha


def _bounds(n, starts):
    if starts is None or n == 0:
        return [0, n]
    st = np.asarray(starts, bool).copy()
    st[0] = True
    return np.flatnonzero(st).tolist() + [n]


def ewm_mean_ref(values, valid, alpha, adjust=True, min_samples=1, ignore_nulls=False, starts=None, ftype=float):
    """(values, validity) of ewm_mean; the state restarts at every set row of
    `starts`.  `values` are converted to `ftype` first (exact for the inputs
    the tests use: float64 into float / longdouble, float32 into any)."""
    n = len(valid)
    np_t = np.float64 if ftype is float else ftype
    xs = np.asarray(values).astype(np_t)
    xs = xs.tolist() if ftype is float else list(xs)
    ok_in = np.asarray(valid, bool).tolist()
    one, zero = ftype(1), ftype(0)
    alpha = ftype(alpha)
    new_value_weight = one if adjust else alpha
    min_periods = max(int(min_samples), 1)
    out = np.zeros(n, np_t)
    ok = np.zeros(n, bool)
    bd = _bounds(n, starts)
    with np.errstate(all="ignore"):
        for a, b in zip(bd[:-1], bd[1:]):
            mean, weight, count = zero, zero, 0
            for i in range(a, b):
                v = xs[i] if ok_in[i] else None
                if count == 0 and v is not None:
                    count = 1
                    mean = v
                    weight = one
                else:
                    if v is not None or not ignore_nulls:
                        weight = weight * (one - alpha)
                    if v is not None:
                        new_weight = weight + new_value_weight
                        mean = mean + (v - mean) * (new_value_weight / new_weight)
                        weight = weight + one if adjust else one
                        count += 1
                if v is not None and count >= min_periods:
                    out[i] = mean
                    ok[i] = True
    return out, ok


class Yardstick:
    """r80 of x and of |x| for one (values, validity, parameters, segments)."""

    def __init__(self, values, valid, alpha, adjust, ignore_nulls, starts=None, min_samples=1):
        kw = dict(alpha=alpha, adjust=adjust, min_samples=min_samples, ignore_nulls=ignore_nulls, starts=starts,
                  ftype=np.longdouble)
        self.r80, self.ok = ewm_mean_ref(values, valid, **kw)
        v = np.asarray(values)
        if (v[np.asarray(valid, bool)] >= 0).all():
            self.scale = self.r80  # |x| is x
        else:
            self.scale, _ = ewm_mean_ref(np.abs(v), valid, **kw)

    def error(self, got, unit=2.0 ** -53):
        """max over the finite non-null rows of |got - r80| / (unit * A_t)."""
        rows = self.ok & np.isfinite(self.r80)
        if not rows.any():
            return 0.0
        d = np.abs(np.asarray(got)[rows].astype(np.longdouble) - self.r80[rows])
        a = self.scale[rows] * np.longdouble(unit)
        with np.errstate(all="ignore"):
            e = np.where(d == 0, np.longdouble(0), d / a)
        return float(e.max())
