"""``GPC``: Gaussian-process classification by the Laplace approximation, on the HIP engine.

The reference's second model (``gumbi.regression.GPC``: a latent GP with a logit link and a Bernoulli likelihood, sampled by
NUTS) as a class of its own: :class:`HipGPC` reuses :class:`HipGP`'s model declaration, lengthscale priors, transforms and
optimiser loop with ``Engine.laplace_evaluate`` (``gmb_laplace_evaluate``: Rasmussen & Williams' Algorithms 3.1 and 5.1, a short
Newton loop of N x N Cholesky factorisations, no sampling) as the objective and ``Engine.laplace_predict`` (Algorithm 3.2) behind
``predict``.

* The output column holds the labels: exactly 0 and 1 in natural space.  They go to the engine as they are -- the output's
  standardizer entry is the identity -- so ``predict_points`` / ``predict_grid`` return the LATENT logit ``f`` as an uncertain
  array, and ``predict_proba`` / ``predict_points_proba`` / ``predict_grid_proba`` the averaged probability
  ``E[sigmoid(f)]`` in (0, 1).
* There is no observation noise: sigma is held at 0 (Sigma = K + 1e-6 I, ``pm.gp.Latent``'s prior with its default jitter), is
  not optimised and carries no prior.
* Scope: one output; continuous dimensions of the five stationary kinds, ARD or shared; linear dimensions; categorical
  dimensions other than the output.  Additive, periodic, distributed, Kronecker and sparse models, ``cross_validate`` and every
  query that reads the exact factor raise ``NotImplementedError``.
"""

from __future__ import annotations

import numpy as np

from ..aggregation import Standardizer
from ..engine import LaplaceConvergenceError
from .hip_gp import HipGP
from .sparse_gp import HipSparseGP

__all__ = ["HipGPC", "averaged_sigmoid"]


def averaged_sigmoid(mean, var, block=4096):
    """``E[sigmoid(f)]`` for ``f ~ N(mean, var)``, elementwise, to about 1e-11.

    The trapezoid rule in ``z = (f - mean) / sqrt(var)`` on [-9, 9]: for an integrand analytic in a strip it converges like
    ``exp(-2 pi d / h)``, ``d`` the strip's half-width -- here ``pi / sqrt(var)``, the logistic's nearest poles -- so the step
    ``h = min(0.4, 0.7 / sqrt(max var))`` leaves ``e^-28``.  (Gauss-Hermite quadrature with a fixed 32 nodes does not: the same
    poles lie ``pi / sqrt(2 var)`` from its axis, and at ``var = 100`` its error is 1e-2.)  O(M sqrt(max var)) on the host."""
    mean, var = np.broadcast_arrays(np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64))
    shape = mean.shape
    mean, var = mean.ravel(), np.maximum(var.ravel(), 0.0)
    out = np.empty(mean.size)
    if mean.size == 0:
        return out.reshape(shape)
    vmax = float(var.max())
    h = min(0.4, 0.7 / np.sqrt(vmax)) if vmax > 0 else 0.4
    n = int(np.ceil(9.0 / h))
    z = h * np.arange(-n, n + 1)
    w = h * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
    sd = np.sqrt(var)
    for i in range(0, mean.size, block):
        f = mean[i:i + block, None] + sd[i:i + block, None] * z[None, :]
        e = np.exp(-np.abs(f))
        out[i:i + block] = np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e)) @ w
    return out.reshape(shape)


class _LaplaceEngine:
    """What ``HipGP.find_MAP`` and ``HipGP.predict`` ask of an engine, answered by the Laplace calls of the engine it wraps.
    ``i_sigma``: sigma's place in theta -- passed on as 0, its gradient entry 0."""

    def __init__(self, engine, i_sigma):
        self.exact = engine
        self.host_blas_free = getattr(engine, "host_blas_free", True)
        self.i_sigma = i_sigma
        self._theta = None
        self._current = False

    def _noise_free(self, theta):
        theta = np.array(theta, dtype=float)
        theta[self.i_sigma] = 0.0
        return theta

    def evaluate(self, theta, grad=True):
        self._current = False
        try:
            out = self.exact.laplace_evaluate(self._noise_free(theta), grad=grad)
        except LaplaceConvergenceError as err:  # a rejected step of the optimiser, as a covariance that is not positive definite
            raise np.linalg.LinAlgError(str(err)) from err
        self._theta = np.array(theta, dtype=float)
        self._current = True
        if grad:
            out[1][self.i_sigma] = 0.0
        return out

    def set_theta(self, theta):
        self._theta = np.array(theta, dtype=float)
        self._current = False

    def factorize(self):
        self.evaluate(self._theta, grad=False)

    def factor_is_current(self):
        return self._current

    def predict(self, Xs, with_noise=True):
        return self.exact.laplace_predict(Xs)  # (the latent function: there is no noise to add)

    def laplace_info(self):
        return self.exact.laplace_info()

    def close(self):
        self.exact.close()


def _not_built(name):
    def method(self, *args, **kwargs):
        raise NotImplementedError(f"{name} is not built for GP classification")

    method.__name__ = name
    method.__doc__ = f"Not part of ``GPC``: ``{name}`` needs the exact (Gaussian-noise) factor."
    return method


class HipGPC(HipGP):
    """Gaussian-process classification (Laplace approximation, logit link) on an MI355X; ``gumbi_amd.GPC``.  See the module
    docstring."""

    #: the queries of :class:`HipGP` that read the exact factor, and the hold-out loop that refits
    NOT_BUILT = HipSparseGP.NOT_BUILT + ("cross_validate",)

    def __init__(self, dataset, outputs=None, seed=2021, device=0, distributed=None, kronecker=False):
        if distributed:
            raise NotImplementedError("distributed=True is not built for GP classification")
        if kronecker not in (False, None, "auto"):
            raise NotImplementedError("the Kronecker form is not built for GP classification (one output only)")
        super().__init__(dataset, outputs=outputs, seed=seed, device=device, distributed=None, kronecker=False)
        if len(self.outputs) != 1:
            raise NotImplementedError(f"GP classification is built for one output, got {self.outputs}")
        self._check_labels()
        # the labels are not standardized: the output's entry is the identity, so the model's "standardized" output IS the latent logit
        stdzr = Standardizer(**{**self.stdzr, **{out: {"μ": 0.0, "σ2": 1.0} for out in self.outputs}})
        self.stdzr._clone_kinds_into(stdzr)
        stdzr.transforms = {name: tr for name, tr in stdzr.transforms.items() if name not in self.outputs}
        self.stdzr = stdzr
        self.latent = True

    def _check_labels(self):
        tidy = self.data.tidy
        vcol = self.data.values_column if self.data.values_column in tidy.columns else "Value"
        for out in self.outputs:
            vals = np.asarray(tidy.loc[tidy[self.out_col] == out, vcol], dtype=float)
            vals = vals[~np.isnan(vals)]
            bad = vals[(vals != 0.0) & (vals != 1.0)]
            if bad.size:
                raise ValueError(f"GPC: the output {out!r} must hold only the labels 0 and 1, found {np.unique(bad)[:5]}")

    def specify_model(self, *args, **kwargs):
        super().specify_model(*args, **kwargs)
        if self.additive:
            raise NotImplementedError("additive models are not built for GP classification")
        if self.out_col in self.categorical_dims:
            raise NotImplementedError("several outputs are not built for GP classification (one output only)")
        return self

    def build_model(self, seed=None, continuous_kernel="ExpQuad", period=None, heteroskedastic_inputs=False,
                    heteroskedastic_outputs=True, sparse=False, n_u=100, ARD=True, ls_bounds=None, mass=0.98):
        """Declare the latent GP (reference :759-797) and move the inputs and the labels into HBM."""
        if sparse:
            raise NotImplementedError("the sparse approximation is not built for GP classification")
        if period is not None or "Periodic" in str(continuous_kernel):
            raise NotImplementedError("periodic kernels (period=...) are not built for GP classification")
        if self.additive:
            raise NotImplementedError("additive models are not built for GP classification")
        super().build_model(seed=seed, continuous_kernel=continuous_kernel, period=None, heteroskedastic_inputs=heteroskedastic_inputs,
                            heteroskedastic_outputs=heteroskedastic_outputs, sparse=False, n_u=n_u, ARD=ARD, ls_bounds=ls_bounds, mass=mass)
        y = self.model.y
        if not np.all((y == 0.0) | (y == 1.0)):
            raise ValueError("GPC: the labels must be exactly 0 or 1")
        (sl,) = [sl for name, _kind, _shape, sl in self.model.blocks if name == "σ"]
        self.engine = _LaplaceEngine(self.engine, sl.start)
        self.gp_dict = dict.fromkeys(self.additive_levels, self.engine)
        self.latent = True
        return self

    def _sigma_slice(self):
        return next(sl for name, _kind, _shape, sl in self.model.blocks if name == "σ")

    def _log_prior(self, theta):
        """``HipGP``'s priors without sigma's: the model has no noise parameter."""
        sl = self._sigma_slice()
        val, grad = super()._log_prior(theta)
        val += float(np.sum(theta[sl]))  # (Exponential(1): log p = -sigma, taken back)
        grad[sl] = 0.0
        return val, grad

    def find_MAP(self, *args, **kwargs):
        """As ``HipGP.find_MAP`` over every parameter but sigma, which is 0: the objective is ``-log q(y | theta)`` of the Laplace
        approximation minus the log-prior.  Leaves the mode resident for the predictions."""
        super().find_MAP(*args, **kwargs)
        sl = self._sigma_slice()
        self._theta_fitted[sl] = 0.0
        with np.errstate(divide="ignore"):
            self.MAP = self._theta_to_dict(self._theta_fitted)
        self.MAP.pop("σ_log__", None)  # (log 0)
        return self.MAP

    @property
    def laplace_info(self):
        """The Newton iteration of the engine's last Laplace evaluation: ``iterations``, ``halvings``, ``psi``, ``step``."""
        if self.engine is None:
            raise ValueError("The model must be built (build_model) first")
        return self.engine.laplace_info()

    # -- probabilities -----------------------------------------------------------------------------------------------------------
    def predict_proba(self, points_array):
        """``E[sigmoid(f)]`` at standardized points ``(M, len(dims))``: the latent mean and variance of :meth:`predict`, averaged
        over the link on the host (:func:`averaged_sigmoid`)."""
        mean, var = self.predict(points_array)
        return averaged_sigmoid(mean, var)

    def _proba_of(self, latent):
        p = averaged_sigmoid(np.asarray(latent.μ, dtype=float), np.asarray(latent.σ2, dtype=float))
        return self.parray(**{latent.name: p}, stdzd=False)

    def predict_points_proba(self, points):
        """Averaged probabilities at a 1-D parray of points, as a parray named after the output."""
        return self._proba_of(self.predict_points(points))

    def predict_grid_proba(self, categorical_levels=None):
        """Averaged probabilities on the grid ``prepare_grid`` left behind, in the grid's shape."""
        return self._proba_of(self.predict_grid(categorical_levels=categorical_levels))


for _name in HipGPC.NOT_BUILT:
    setattr(HipGPC, _name, _not_built(_name))
del _name
