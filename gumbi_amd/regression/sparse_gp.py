"""``SparseGP``: the FITC approximation on inducing points, on the HIP engine.

The reference's ``fit(sparse=True, n_u=...)`` builds PyMC's ``MarginalSparse(approx="FITC")`` on k-means inducing points
(``gumbi/regression/pymc/GP.py:571-591``).  Here the same model is a class of its own: :class:`HipGP` keeps refusing
``sparse=True``, and ``SparseGP`` reuses its model declaration, priors, transforms and optimiser loop with
``Engine.fitc_evaluate`` (``gmb_fitc_evaluate``: O(N m^2) per evaluation, nothing of N x N elements) as the objective and
``Engine.fitc_predict`` behind ``predict``.  ``predict_points``, ``predict_grid``, ``get_conditional_prediction`` and
``cross_validate`` work through the ``Regressor`` seam unchanged.

Scope: one output, continuous dimensions only (no categorical or linear dimensions, not additive, not periodic), scalar noise --
the reference itself falls back to scalar noise for sparse models.  The inducing locations are fixed (k-means, or given); they are
not optimised.  Every posterior query other than mean and variance raises ``NotImplementedError``.
"""

from __future__ import annotations

import numpy as np

from .hip_gp import HipGP

__all__ = ["HipSparseGP", "kmeans_inducing_points"]

#: rows of the table k-means sees per inducing point asked for (at most; all rows of a smaller table)
KMEANS_ROWS_PER_CENTRE = 64


def kmeans_inducing_points(X, n_u, seed):
    """``n_u`` inducing points by k-means on the whitened rows of ``X`` (what ``pm.gp.util.kmeans_inducing_points`` does: every
    column divided by its standard deviation, ``scipy.cluster.vq.kmeans``, scaled back), seeded, on at most ``64 n_u`` rows drawn
    with that seed.  k-means may return fewer centres than asked for: the caller reads the count off the result."""
    from scipy.cluster.vq import kmeans

    X = np.asarray(X, dtype=np.float64)
    n_u = int(n_u)
    if X.ndim != 2 or n_u < 1:
        raise ValueError(f"kmeans_inducing_points: X must be (N, D) and n_u >= 1, got {X.shape} and {n_u}")
    rng = np.random.default_rng(seed)
    if len(X) > KMEANS_ROWS_PER_CENTRE * n_u:
        X = X[np.sort(rng.choice(len(X), size=KMEANS_ROWS_PER_CENTRE * n_u, replace=False))]
    scaling = np.std(X, axis=0)
    scaling[scaling <= 1e-6] = 1.0
    centres, _ = kmeans(X / scaling, min(n_u, len(X)), seed=rng)
    return np.ascontiguousarray(centres * scaling)


class _FitcEngine:
    """What ``HipGP.find_MAP`` and ``HipGP.predict`` ask of an engine, answered by the sparse calls of the engine it wraps."""

    host_blas_free = True

    def __init__(self, engine, Z):
        self.exact = engine
        self.host_blas_free = getattr(engine, "host_blas_free", True)
        engine.set_inducing(Z)
        self._theta = None
        self._current = False

    def evaluate(self, theta, grad=True):
        self._current = False
        out = self.exact.fitc_evaluate(theta, grad=grad)
        self._theta = np.array(theta, dtype=float)
        self._current = True
        return out

    def set_theta(self, theta):
        self._theta = np.array(theta, dtype=float)
        self._current = False

    def factorize(self):
        self.evaluate(self._theta, grad=False)

    def factor_is_current(self):
        return self._current

    def predict(self, Xs, with_noise=True):
        return self.exact.fitc_predict(Xs, with_noise=with_noise)

    def close(self):
        self.exact.close()


def _not_built(name):
    def method(self, *args, **kwargs):
        raise NotImplementedError(f"{name} is not built for the sparse approximation")

    method.__name__ = name
    method.__doc__ = f"Not part of ``SparseGP``: ``{name}`` needs the exact factor."
    return method


class HipSparseGP(HipGP):
    """Sparse Gaussian-process regression (FITC) on an MI355X; ``gumbi_amd.SparseGP``.  See the module docstring."""

    #: the queries of :class:`HipGP` that read the exact factor
    NOT_BUILT = ("predict_grad", "predict_points_grad", "predict_grid_grad", "predict_slope", "predict_points_slope",
                 "predict_grid_slope", "acquisition_with_grad", "propose_continuous", "condition_on", "predict_joint",
                 "draw_point_samples", "draw_grid_samples", "decompose_points", "decompose_grid", "leave_one_out", "leave_group_out",
                 "predict_groups", "predict_average", "marginal_design", "predict_marginal", "compare_levels", "design_batch",
                 "variance_reduction", "batch_acquisition_with_grad", "propose_batch", "draw_paths", "propose_thompson")

    def __init__(self, dataset, outputs=None, seed=2021, device=0, distributed=None, kronecker=False):
        if distributed:
            raise NotImplementedError("distributed=True is not built for the sparse approximation")
        super().__init__(dataset, outputs=outputs, seed=seed, device=device, distributed=None, kronecker=False)
        self.sparse = True
        self.model_specs["sparse"] = True
        #: the inducing points Z in the model's standardized input space, ``(n_u, D)`` (``build_model``)
        self.inducing_points = None

    def fit(self, outputs=None, linear_dims=None, continuous_dims=None, continuous_levels=None, continuous_coords=None,
            categorical_dims=None, categorical_levels=None, additive=False, seed=None, continuous_kernel="ExpQuad", period=None,
            heteroskedastic_inputs=False, heteroskedastic_outputs=True, sparse=True, n_u=100, ARD=True, ls_bounds=None, mass=0.98,
            spec_kwargs=None, build_kwargs=None, MAP_kwargs=None, inducing_points=None):
        """``specify_model`` -> ``build_model`` -> ``find_MAP``, as ``GP.fit``; ``inducing_points`` (a parray with one layer per
        model dimension) replaces the k-means default."""
        build_kwargs = dict(build_kwargs or {})
        if inducing_points is not None:
            build_kwargs["inducing_points"] = inducing_points
        return super().fit(outputs=outputs, linear_dims=linear_dims, continuous_dims=continuous_dims, continuous_levels=continuous_levels,
                           continuous_coords=continuous_coords, categorical_dims=categorical_dims, categorical_levels=categorical_levels,
                           additive=additive, seed=seed, continuous_kernel=continuous_kernel, period=period,
                           heteroskedastic_inputs=heteroskedastic_inputs, heteroskedastic_outputs=heteroskedastic_outputs,
                           sparse=sparse, n_u=n_u, ARD=ARD, ls_bounds=ls_bounds, mass=mass, spec_kwargs=spec_kwargs,
                           build_kwargs=build_kwargs, MAP_kwargs=MAP_kwargs)

    def _check_scope(self, continuous_kernel, period):
        if self.out_col in self.categorical_dims:
            raise NotImplementedError("several outputs are not built for the sparse approximation (one output only)")
        if self.categorical_dims:
            raise NotImplementedError(f"categorical dimensions {self.categorical_dims} are not built for the sparse approximation")
        if self.linear_dims:
            raise NotImplementedError("linear_dims are not built for the sparse approximation")
        if self.additive:
            raise NotImplementedError("additive models are not built for the sparse approximation")
        if period is not None or "Periodic" in str(continuous_kernel):
            raise NotImplementedError("periodic kernels (period=...) are not built for the sparse approximation")

    def _inducing_array(self, inducing_points):
        """a parray of inducing points -> ``(m, D)`` standardized rows in the order of ``self.dims``"""
        points = np.atleast_1d(inducing_points)
        if points.ndim != 1:
            raise ValueError(f"inducing_points must be a 1-D parray of points, got shape {points.shape}")
        if set(points.names) != set(self.dims):
            raise ValueError(f"inducing_points must have one layer per model dimension {self.dims}, got {points.names}")
        tz = points[:, None].z
        Z = np.hstack([np.asarray(tz[dim + "_z"].values(), dtype=np.float64) for dim in self.dims])
        if not np.all(np.isfinite(Z)):
            raise ValueError("inducing_points must be finite")
        return np.ascontiguousarray(Z)

    def build_model(self, seed=None, continuous_kernel="ExpQuad", period=None, heteroskedastic_inputs=False,
                    heteroskedastic_outputs=True, sparse=True, n_u=100, ARD=True, ls_bounds=None, mass=0.98, inducing_points=None):
        """Declare the sparse marginal GP (reference :571-591) and move the data and the inducing points into HBM.

        ``n_u`` inducing points come from seeded k-means of the shaped inputs (:func:`kmeans_inducing_points`) unless
        ``inducing_points`` gives them; afterwards ``self.inducing_points`` holds Z and ``self.n_u`` the real count (k-means may
        return fewer centres than asked for)."""
        if not sparse:
            raise ValueError("SparseGP is the sparse approximation: sparse=False is gumbi_amd.GP")
        self._check_scope(continuous_kernel, period)
        seed = self.seed if seed is None else seed
        X, _ = self.get_shaped_data("mean")
        if inducing_points is not None:
            Z = self._inducing_array(inducing_points)
        else:
            if int(n_u) < 1:
                raise ValueError(f"n_u must be at least 1, got {n_u}")
            Z = kmeans_inducing_points(X, n_u, seed)
        super().build_model(seed=seed, continuous_kernel=continuous_kernel, period=None, heteroskedastic_inputs=heteroskedastic_inputs,
                            heteroskedastic_outputs=heteroskedastic_outputs, sparse=False, n_u=n_u, ARD=ARD, ls_bounds=ls_bounds,
                            mass=mass)
        self.engine = _FitcEngine(self.engine, Z)
        self.gp_dict = dict.fromkeys(self.additive_levels, self.engine)
        self.inducing_points = Z
        self.sparse, self.n_u = True, len(Z)
        self.model_specs.update(sparse=True, n_u=n_u)
        if inducing_points is not None:
            self.model_specs["inducing_points"] = inducing_points  # (cross_validate rebuilds with build_model(**model_specs))
        return self


for _name in HipSparseGP.NOT_BUILT:
    setattr(HipSparseGP, _name, _not_built(_name))
del _name
