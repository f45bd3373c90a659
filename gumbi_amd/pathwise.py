"""Host side of the pathwise posterior draws (``csrc/pathwise.hpp``): the random numbers of a set of draws.

numpy only -- no engine import: the normals stay the caller's, so a set of draws is reproducible from a numpy seed.

For draw ``s`` the engine evaluates, in its prepared coordinates ``u = x / ls``,

    f_s(x) = phi(x)^T w_s + k(x, X) a_s,    phi_f(x) = eta sqrt(2 / F) cos(omega_f^T u + b_f),

with ``a_s = Sigma^-1 (y - Phi(X) w_s - d o eps_s)``.  ``eta`` and ``ls`` come from theta on the engine's side, so the frequencies
drawn here do not depend on theta: they are draws from the spectral density of the UNIT kernel (Bochner's theorem), whose feature
products ``phi(x)^T phi(x')`` average to ``k(x, x')``.
"""

from __future__ import annotations

import numpy as np

#: kernel kind (name or the engine's number) -> Matern smoothness nu (None: ExpQuad) and the scale of the distance
_KINDS = {
    "ExpQuad": (None, 1.0), "Matern52": (2.5, 1.0), "Matern32": (1.5, 1.0), "Matern12": (0.5, 1.0), "Exponential": (0.5, 0.5),
    0: (None, 1.0), 1: (2.5, 1.0), 2: (1.5, 1.0), 3: (0.5, 1.0), 4: (0.5, 0.5),
}


def spectral_frequencies(kind, F, Dc, rng):
    """``(F, Dc)`` frequencies of the unit kernel of ``kind`` (a name or the engine's kind number) in the prepared coordinates:

    * ``ExpQuad`` (``exp(-r^2 / 2)``): ``omega ~ N(0, I)``;
    * Matern-nu: ``omega = z / sqrt(g)`` with ``z ~ N(0, I)`` and ``g ~ Gamma(shape nu, rate nu)`` -- a multivariate Student-t with
      ``2 nu`` degrees of freedom, the spectral density of the Matern kernel; nu = 5/2, 3/2, 1/2;
    * ``Exponential`` (``exp(-r / 2)``): the ``Matern12`` draw times 1/2.
    """
    if kind not in _KINDS:
        raise ValueError(f"unknown kernel kind {kind!r}")
    nu, scale = _KINDS[kind]
    F, Dc = int(F), int(Dc)
    z = rng.standard_normal((F, Dc))
    if nu is None:
        return z
    g = rng.gamma(shape=nu, scale=1.0 / nu, size=(F, 1))
    return scale * z / np.sqrt(g)


def path_inputs(kind, S, F, Dc, N, seed, antithetic=False):
    """``(omega (F, Dc), phase (F,), w (S, F), eps (S, N))`` of ``S`` draws: frequencies (:func:`spectral_frequencies`), phases
    uniform in [0, 2 pi), and standard normals for the feature weights and the noise of the conditioning.  With
    ``antithetic=True`` draws ``2 i`` and ``2 i + 1`` carry ``(w, eps)`` and ``(-w, -eps)`` (the last draw of an odd ``S`` stands
    alone): the mean of such a pair is exactly the posterior mean ``k(x, X) Sigma^-1 y``."""
    S, F, Dc, N = int(S), int(F), int(Dc), int(N)
    if S < 1 or F < 1 or Dc < 1 or N < 1:
        raise ValueError(f"path_inputs: S = {S}, F = {F}, Dc = {Dc}, N = {N} must all be positive")
    rng = np.random.default_rng(seed)
    omega = spectral_frequencies(kind, F, Dc, rng)
    phase = rng.uniform(0.0, 2.0 * np.pi, F)
    n_own = (S + 1) // 2 if antithetic else S
    w = rng.standard_normal((n_own, F))
    eps = rng.standard_normal((n_own, N))
    if antithetic:
        w = np.stack([w, -w], axis=1).reshape(2 * n_own, F)[:S]
        eps = np.stack([eps, -eps], axis=1).reshape(2 * n_own, N)[:S]
    return omega, phase, np.ascontiguousarray(w), np.ascontiguousarray(eps)
