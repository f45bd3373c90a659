"""Analytic acquisition functions of a Gaussian posterior, as value AND gradient with respect to ``(mu, sigma^2)``: what a
gradient-based search needs to chain with ``Engine.predict_with_grad``'s ``d mu / d x*`` and ``d sigma^2 / d x*``.  Pure numpy and
scipy; standardized units; computed on the noise-free posterior.

* :func:`expected_improvement` -- ``EI = s [z Phi(z) + phi(z)]`` with ``z = +-(mu - best) / s``, returned in its LOG form
  ``log EI = log s + log h(z)`` so that flat regions (EI underflowing to 0) keep a gradient.  ``log h`` switches to the
  asymptotic series of the Mills ratio below ``z = -30`` (the direct form loses ``z^2 eps`` to cancellation and underflows
  near ``z = -38``; at -30 the two agree to ~1e-12).
* :func:`upper_confidence_bound` -- ``mu + sqrt(beta) s`` (``beta = 2`` by default); minimising uses ``-(mu - sqrt(beta) s)``,
  so the returned value is always to be MAXIMISED.

Every function returns ``(value, d value / d mu, d value / d sigma^2)`` elementwise; larger is better for both settings of
``maximize``.
"""
import numpy as np
from scipy.special import log_ndtr, ndtr

_LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)
_VAR_FLOOR = 1e-300


def _log_h(z):
    """``log h(z)`` and ``h'(z) / h(z)`` for ``h(z) = z Phi(z) + phi(z)`` (``h' = Phi``)."""
    z = np.asarray(z, float)
    log_h = np.empty_like(z)
    ratio = np.empty_like(z)
    far = z < -30.0
    zn = z[~far]
    phi = np.exp(-0.5 * zn * zn - _LOG_SQRT_2PI)
    Phi = ndtr(zn)
    h = zn * Phi + phi
    log_h[~far] = np.log(h)
    ratio[~far] = Phi / h
    # z -> -inf: Phi(z) = phi(z) / |z| (1 - 1/z^2 + 3/z^4 - 15/z^6 + 105/z^8 - ...), so
    # h = phi(z) (1/z^2 - 3/z^4 + 15/z^6 - 105/z^8 + ...): the leading terms cancel analytically, not numerically
    # (first term dropped: 2027025 u^7 < 5e-15 for |z| > 30)
    zf = z[far]
    u = 1.0 / (zf * zf)
    series = u * (1.0 - u * (3.0 - u * (15.0 - u * (105.0 - u * (945.0 - u * (10395.0 - u * 135135.0))))))
    log_h[far] = -0.5 * zf * zf - _LOG_SQRT_2PI + np.log(series)
    ratio[far] = np.exp(log_ndtr(zf) - log_h[far])
    return log_h, ratio


def expected_improvement(mu, var, best, maximize=True):
    """``(log EI, d log EI / d mu, d log EI / d sigma^2)`` of improving on ``best`` (the best observed value)."""
    mu, var = np.asarray(mu, float), np.maximum(np.asarray(var, float), _VAR_FLOOR)
    sign = 1.0 if maximize else -1.0
    s = np.sqrt(var)
    z = sign * (mu - best) / s
    log_h, ratio = _log_h(z)
    value = np.log(s) + log_h
    d_mu = ratio * sign / s                       # d z / d mu = sign / s
    d_var = 0.5 / var - ratio * z * 0.5 / var     # d log s / d var = 1 / (2 var);  d z / d var = -z / (2 var)
    return value, d_mu, d_var


def upper_confidence_bound(mu, var, beta=2.0, maximize=True):
    """``(UCB, d UCB / d mu, d UCB / d sigma^2)``: ``mu + sqrt(beta) s``, or ``-(mu - sqrt(beta) s)`` when minimising."""
    mu, var = np.asarray(mu, float), np.maximum(np.asarray(var, float), _VAR_FLOOR)
    sign = 1.0 if maximize else -1.0
    s = np.sqrt(var)
    rb = np.sqrt(float(beta))
    return sign * mu + rb * s, np.full_like(mu, sign), 0.5 * rb / s


def get(name, **kwargs):
    """The acquisition ``f(mu, var, maximize) -> (value, d/d mu, d/d var)`` named ``"EI"`` (needs ``best=``) or ``"UCB"``
    (optional ``beta=``)."""
    if name == "EI":
        best = float(kwargs["best"])
        return lambda mu, var, maximize=True: expected_improvement(mu, var, best, maximize=maximize)
    if name == "UCB":
        beta = float(kwargs.get("beta", 2.0))
        return lambda mu, var, maximize=True: upper_confidence_bound(mu, var, beta=beta, maximize=maximize)
    raise ValueError(f'acquisition must be "EI" or "UCB", got {name!r}')
