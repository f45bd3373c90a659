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

Batches of q points, optimised as a whole (the reference's ``propose(q=.., mc_samples=256)``, botorch/GP.py:652):

* :func:`batch_expected_improvement` -- reparameterised Monte-Carlo q-EI of the joint posterior ``N(mean, cov)`` of a batch, in its
  LOG form, on fixed base samples (:func:`sobol_normals`), as value and adjoints with respect to ``mean`` and ``cov`` -- what chains
  with ``Engine.predict_batches``'s ``dmean`` and ``dcov``.  The adjoint goes through the Cholesky factor in closed form
  (:func:`cholesky_adjoint`).
"""
import warnings

import numpy as np
from scipy.special import log_ndtr, ndtr, ndtri

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


#: Temperature of the smoothed maximum over the q points of a batch, ``tau log sum_j exp(y_j / tau)``, in standardized units of the
#: output.  It exceeds the true maximum by at most ``tau log q`` (2.8e-3 at q = 16, 0 at q = 1): below the Monte-Carlo error of 256
#: samples wherever the improvement matters, and large enough that every point of a batch near the maximum keeps a gradient.
TAU_MAX = 1e-3
#: Temperature of the smoothed ReLU ``tau softplus(x / tau)`` of the improvement.  Its bias in the expectation is O(tau^2 p(0)) --
#: 1e-6 times the improvement's density at 0 -- and in a flat region, where every sample lies below the incumbent, the log of the
#: sample mean falls off linearly with slope 1 / tau = 1e3 per standardized unit: finite, with a gradient an optimiser can follow
#: (a smaller tau makes that slope dominate the summed objective of restarts run in lock step).
TAU_RELU = 1e-3


def sobol_normals(S, q, seed=None):
    """``(S, q)`` standard-normal base samples: scrambled Sobol points through the normal quantile.  Fixed for a whole
    optimisation, so the Monte-Carlo acquisition is a deterministic, differentiable function of the batch."""
    from scipy.stats import qmc

    S, q = int(S), int(q)
    if S < 1 or q < 1:
        raise ValueError(f"sobol_normals: S = {S} samples of q = {q} dimensions")
    engine = qmc.Sobol(d=q, scramble=True, seed=seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (a sample count that is no power of 2 loses the balance property only)
        u = engine.random(S)
    tiny = np.finfo(float).eps
    return ndtri(np.clip(u, tiny, 1.0 - tiny))


def cholesky_adjoint(L, L_bar):
    """The adjoint of ``cov`` given that of its lower Cholesky factor: with ``cov = L L^T`` and ``d value = sum L_bar * d L`` over
    the lower triangle, the SYMMETRIC ``cov_bar`` with ``d value = sum cov_bar * d cov`` for symmetric ``d cov``:
    ``cov_bar = sym(L^-T Phi(L^T L_bar) L^-1)``, ``Phi`` = the lower triangle with its diagonal halved (Murray 2016,
    "Differentiation of the Cholesky decomposition").  Works on stacks ``(..., q, q)``."""
    L = np.asarray(L, float)
    P = np.tril(np.swapaxes(L, -1, -2) @ np.tril(np.asarray(L_bar, float)))
    idx = np.arange(L.shape[-1])
    P[..., idx, idx] *= 0.5
    Lt = np.swapaxes(L, -1, -2)
    S = np.linalg.solve(Lt, P)                                        # L^-T P
    S = np.swapaxes(np.linalg.solve(Lt, np.swapaxes(S, -1, -2)), -1, -2)  # ... L^-1
    return 0.5 * (S + np.swapaxes(S, -1, -2))


def _log_softplus(x):
    """``log softplus(x)`` and its derivative ``sigmoid(x) / softplus(x)``; below x = -30 softplus is exp(x) to 1e-13 relative."""
    x = np.asarray(x, float)
    value = np.array(x, copy=True)
    slope = np.ones_like(x)
    near = x >= -30.0
    xn = x[near]
    sp = np.where(xn > 0.0, xn + np.log1p(np.exp(-np.abs(xn))), np.log1p(np.exp(-np.abs(xn))))
    value[near] = np.log(sp)
    slope[near] = 1.0 / (1.0 + np.exp(-xn)) / sp
    return value, slope


def batch_expected_improvement(mean, cov, Z, best, maximize=True):
    """Monte-Carlo log q-EI of ``B`` batches: ``(value (B,), d value / d mean (B, q), d value / d cov (B, q, q) symmetric)``.

    Per batch, with ``L = chol(cov)`` and the base samples ``Z`` (S, q): ``Y = mean + Z L^T`` (S joint draws of the q points); the
    improvement of a draw is a smoothed maximum over the q points (temperature :data:`TAU_MAX`) of ``+-(Y - best)`` through a
    smoothed ReLU (:data:`TAU_RELU`); the value is the LOG of the sample mean, evaluated in log space throughout (log-softplus,
    log-sum-exp over the samples), so a batch whose every draw lies far below the incumbent has a finite value and a non-zero
    gradient where the plain sample mean underflows.  ``d value / d cov`` is the symmetric adjoint: ``d value = sum(it * d cov)``
    for symmetric ``d cov``.  ``LinAlgError`` for a covariance that is not positive definite."""
    from scipy.special import logsumexp

    mean = np.asarray(mean, float)
    cov = np.asarray(cov, float)
    Z = np.asarray(Z, float)
    B, q = mean.shape
    if cov.shape != (B, q, q) or Z.ndim != 2 or Z.shape[1] != q:
        raise ValueError(f"batch_expected_improvement: mean {mean.shape}, cov {cov.shape}, Z {Z.shape} do not fit together")
    sign = 1.0 if maximize else -1.0
    L = np.linalg.cholesky(cov)                                       # (B, q, q)
    Y = mean[:, None, :] + np.einsum("sk,bjk->bsj", Z, L)             # (B, S, q)
    obj = sign * (Y - best)
    top = TAU_MAX * logsumexp(obj / TAU_MAX, axis=2)                  # (B, S): the smoothed maximum
    pick = np.exp((obj - top[:, :, None]) / TAU_MAX)                  # d top / d obj: softmax over the q points
    lsp, slope = _log_softplus(top / TAU_RELU)
    log_imp = np.log(TAU_RELU) + lsp                                  # log of the smoothed improvement of every draw
    value = logsumexp(log_imp, axis=1) - np.log(Z.shape[0])
    weight = np.exp(log_imp - (value[:, None] + np.log(Z.shape[0])))  # d value / d log_imp: softmax over the draws
    g_Y = sign * (weight * slope / TAU_RELU)[:, :, None] * pick       # d value / d Y
    d_mean = g_Y.sum(axis=1)
    L_bar = np.tril(np.einsum("bsj,sk->bjk", g_Y, Z))
    return value, d_mean, cholesky_adjoint(L, L_bar)


def get(name, **kwargs):
    """The acquisition ``f(mu, var, maximize) -> (value, d/d mu, d/d var)`` named ``"EI"`` (needs ``best=``) or ``"UCB"``
    (optional ``beta=``), or the batch form ``f(mean, cov, Z, maximize) -> (value, d/d mean, d/d cov)`` named ``"qEI"`` (needs
    ``best=``)."""
    if name == "qEI":
        best = float(kwargs["best"])
        return lambda mean, cov, Z, maximize=True: batch_expected_improvement(mean, cov, Z, best, maximize=maximize)
    if name == "EI":
        best = float(kwargs["best"])
        return lambda mu, var, maximize=True: expected_improvement(mu, var, best, maximize=maximize)
    if name == "UCB":
        beta = float(kwargs.get("beta", 2.0))
        return lambda mu, var, maximize=True: upper_confidence_bound(mu, var, beta=beta, maximize=maximize)
    raise ValueError(f'acquisition must be "EI" or "UCB", got {name!r}')
