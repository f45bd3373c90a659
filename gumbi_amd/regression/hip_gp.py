"""``GP``: the MI355X-native exact-GP backend behind Gumbi's ``Regressor`` seam.

Same class surface as the reference's default backend ``PymcGP`` (``gumbi/regression/pymc/GP.py``:
``__init__`` :227-249, ``fit`` :255-387, ``build_model`` :468-583, ``find_MAP`` :799-813,
``predict`` :837-849; attributes ``model``, ``gp_dict``, ``MAP``, ``model_specs``), but every
covariance build, Cholesky factorisation, triangular solve and gradient runs in
``libgumbi_hip.so`` (HIP, gfx950) through :mod:`gumbi_amd.engine`.  This module holds only what
PyMC's *model declaration* held: which column feeds which kernel, the priors, the
unconstrained parametrisation and the optimiser loop.  There is no CPU implementation of the
numerics here and no fallback.

Model (non-additive, reference docstring :61-71 and code :711-729, :560-569)::

    K     = (eta^2 k(r; ls) [+ tau Linear(c)]) * prod_dims Coregion(W_dim, kappa_dim) * Coregion_out
    noise = WhiteNoise(sigma) [* Coregion("Output_noise")]
    y ~ N(0, K + noise + 1e-6 I)

Priors (:407, :409, :451-452, :460-461, :560): ls ~ InverseGamma(alpha, beta) from the pairwise
distance rule; eta ~ Gamma(2,1); sigma ~ Exponential(1); c ~ N(0,10); tau ~ HalfNormal(10);
W ~ N(0,3) with seeded initial value; kappa ~ Gamma(1.5,1).  ``find_MAP`` minimises, like
``pm.find_MAP`` of PyMC >= 4, ``-(log-lik + log-priors)`` over the log of the positive parameters
with L-BFGS-B (scipy -- the optimiser PyMC itself calls).  The log-Jacobians of the log transforms
are NOT part of that objective (``model.compile_logp(jacobian=False)`` in pymc/tuning/starting.py;
confirmed against the predictions printed in the reference's Multioutput_Regression notebook, see
``HipGP.map_includes_jacobian``).
"""

from __future__ import annotations

import warnings
from math import lgamma

import numpy as np
import pandas as pd

from ..aggregation import DataSet
from ..arrays import ParameterArray as parray
from ..arrays import UncertainArray
from ..engine import KERNEL_KINDS, MAX_PERIODIC_DIMS, Engine, KernelSpec, resolve_kernel_name
from . import icm
from ..utils.gp_utils import get_ls_prior
from ..utils.misc import assert_in
from .base import Regressor

__all__ = ["HipGP"]

_REJECTED = 1e100  # objective value of a rejected step (non-PD covariance); far above any real NLML


class HipModel:
    """What ``gp.model`` exposes: the declared structure (kernel spec, priors, parameter
    layout).  Plays the descriptive role of the ``pm.Model`` the reference stores."""

    def __init__(self, spec: KernelSpec, ls_params: dict, blocks: list, X, y):
        self.spec = spec
        self.ls_params = ls_params
        self.blocks = blocks  # [(name, kind, shape, slice)], kind in {"pos", "real"}
        self.X = X
        self.y = y

    @property
    def named_vars(self):
        return [b[0] for b in self.blocks]

    def __repr__(self):
        names = ", ".join(f"{n}{shape}" for n, _, shape, _ in self.blocks)
        return f"HipModel(kernel={self.spec.kind}, N={len(self.y)}, D={self.X.shape[1]}, params=[{names}])"


_BLAS_CONTROLLER = None
_BLAS_LIBS_SEEN = -1


class UnknownAdditiveLevel(ValueError, NotImplementedError):
    """``additive_level`` names a level the model does not have.  A ``ValueError`` -- the argument is wrong, and the message
    lists the levels there are -- that is also a ``NotImplementedError``: the reference raises that for every level but
    "total", and a non-additive model still has no other level to offer callers written against it."""


def _single_threaded_host_blas(engine):
    """Context for the optimiser's loop when the evaluations run on the GPU: scipy's L-BFGS-B factors its m x m (m <= 10)
    matrices with LAPACK, and a many-threaded OpenBLAS spends 0.1 - 20 ms per iteration waking its pool for them -- more than a
    whole MAP evaluation at Gumbi's usual sizes (N = 392: 0.27 ms).  One thread inside ``minimize`` only, and only for engines
    whose arithmetic is not the host's BLAS (``host_blas_free``).

    The limit is PROCESS-GLOBAL while the context is open (that is how threadpoolctl works): another thread doing host BLAS work
    during ``find_MAP`` is throttled too.  ``GUMBI_HOST_BLAS_LIMIT=0`` switches it off.  The library scan is cached and redone
    when the number of shared objects in the process changed -- a BLAS loaded after the first fit (torch's bundled copy, a
    second numpy / scipy one) is then covered as well; counting the objects costs ~20 us, a scan ~2 ms."""
    import contextlib
    import os

    if not getattr(engine, "host_blas_free", False) or os.environ.get("GUMBI_HOST_BLAS_LIMIT", "1") == "0":
        return contextlib.nullcontext()
    global _BLAS_CONTROLLER, _BLAS_LIBS_SEEN
    try:
        n_libs = _loaded_shared_objects()
        if _BLAS_CONTROLLER is None or n_libs != _BLAS_LIBS_SEEN:
            from threadpoolctl import ThreadpoolController

            _BLAS_CONTROLLER = ThreadpoolController()
            _BLAS_LIBS_SEEN = n_libs
        return _BLAS_CONTROLLER.limit(limits=1, user_api="blas")
    except Exception:  # noqa: BLE001 -- no threadpoolctl, or a BLAS it cannot steer: the fit is merely slower
        return contextlib.nullcontext()


def _loaded_shared_objects() -> int:
    """How many shared objects the process has mapped (dl_iterate_phdr): changes when a library -- e.g. another BLAS -- is loaded."""
    import ctypes

    global _PHDR_COUNTER
    try:
        if _PHDR_COUNTER is None:
            cb_t = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)
            count = [0]

            def _cb(_info, _size, _data):
                count[0] += 1
                return 0

            libc = ctypes.CDLL(None)
            libc.dl_iterate_phdr.argtypes = [cb_t, ctypes.c_void_p]
            _PHDR_COUNTER = (libc, cb_t(_cb), count)
        libc, cb, count = _PHDR_COUNTER
        count[0] = 0
        libc.dl_iterate_phdr(cb, None)
        return count[0]
    except Exception:  # noqa: BLE001 -- no dl_iterate_phdr: behave as before (one scan per process)
        return 0


_PHDR_COUNTER = None


class PosteriorPaths:
    """A set of posterior function draws (:meth:`HipGP.draw_paths`): functions of the model's inputs that can be evaluated at any
    points after the fact.  The state lives on the GP's engine, which holds ONE set: another ``draw_paths`` or
    ``propose_thompson`` replaces it, and a refit or new data invalidate it -- this object's methods then raise ``ValueError``
    rather than evaluate another set's draws."""

    def __init__(self, gp, outputs, cont, cols, full, n_draws, generation):
        self.gp, self.outputs, self.continuous_dims, self.n_draws = gp, outputs, cont, n_draws
        self._cols, self._full = cols, full
        self._engine, self._generation = gp.engine, generation  # the engine holds ONE set: this one while its generation stands

    def _own_engine(self):
        """The engine, if the set it holds is still this one: another ``draw_paths`` / ``propose_thompson``, a cleared set or a
        rebuilt engine is a ``ValueError`` here (changed data, theta or factor are the engine's own to refuse)."""
        eng = self.gp.engine
        if eng is not self._engine or eng.paths_generation != self._generation:
            raise ValueError("these posterior paths are stale: the GP has drawn another set (draw_paths, propose_thompson), cleared "
                             "them or rebuilt its engine since; draw them again")
        return eng

    def at_points(self, points):
        """All draws at a 1-D parray of ``points``: a parray of shape ``(n_draws, M)`` in standardized units, like
        :meth:`HipGP.draw_point_samples`; also left in the GP's :attr:`predictions` / :attr:`predictions_X`."""
        gp = self.gp
        eng = self._own_engine()
        points_array, _, _ = gp._prepare_points_for_prediction(points, output=self.outputs)
        samples = eng.paths_eval(np.asarray(points_array, dtype=np.float64))
        gp.predictions = gp.parray(**{self.outputs[0]: samples}, stdzd=True)
        gp.predictions_X = points
        return gp.predictions

    def on_grid(self):
        """All draws at the points :meth:`prepare_grid` defined, at any grid size: a parray of shape ``(n_draws, *grid shape)``."""
        gp = self.gp
        self._own_engine()
        if gp.grid_points is None:
            raise ValueError("Grid must first be specified with `prepare_grid`")
        samples = self.at_points(gp.grid_points)
        gp.predictions = samples.reshape(-1, *gp.grid_parray.shape)
        gp.predictions_X = gp.predictions_X.reshape(gp.grid_parray.shape)
        return gp.predictions

    def value_and_grad(self, points_z, draw, grad=True):
        """Point ``m`` of ``points_z`` -- ``(M, n_cont)`` STANDARDIZED continuous coordinates in ``continuous_dims`` order -- on
        draw ``draw[m]`` only: ``(value (M,), gradient (M, n_cont))`` in standardized units (the gradient ``None`` with
        ``grad=False``).  ONE ``engine.paths_eval_own`` call: the objective of a Thompson search."""
        Z = np.asarray(points_z, float).reshape(-1, len(self.continuous_dims))
        val, g = self._own_engine().paths_eval_own(self._full(Z), draw, grad=grad)
        return val, (g[:, self._cols] if grad else None)


class HipGP(Regressor):
    """Gaussian-process regression on an MI355X.  Drop-in for ``gumbi.GP`` on the
    ``fit() / prepare_grid() / predict_grid()`` path; see the module docstring."""

    def __init__(self, dataset: DataSet, outputs=None, seed=2021, device=0, distributed=None, kronecker="auto"):
        """``distributed``: ``True`` (default process group) or a ``torch.distributed`` group -- ONE GP
        spread over the group's GPUs (:class:`gumbi_amd.distributed.DistributedEngine`: block-cyclic
        Cholesky, sharded gradient and prediction).  Every rank constructs the same GP on the same data
        and makes the same calls; all ranks obtain identical MAP estimates and predictions."""
        super().__init__(dataset, outputs, seed)
        self.device = device
        self.distributed = distributed
        #: "auto": multi-output tables that repeat the same inputs for every output are evaluated in
        #: Kronecker form (:mod:`gumbi_amd.regression.icm`: P systems of size N instead of one of size
        #: PN); False: always the stacked system, as the reference builds it
        self.kronecker = kronecker
        self.model = None
        self.gp_dict = None
        self.additive_levels = None  # {level: the engine's term selection} (build_model)
        self.component_cov = self.component_levels = None  # decompose_points: covariance between the components, and its axes
        self.marginal_points = self.marginal_cov = self.average_labels = None  # predict_marginal's grid and joint covariance; predict_average's labels
        self.slope_cov = None  # predict_points_slope(joint=True): {output: (points, n_cont, n_cont)} covariance of the partial slopes
        self.MAP = None
        self.trace = None
        self.engine = None

        self.continuous_kernel = "ExpQuad"
        self.heteroskedastic_inputs = False
        self.heteroskedastic_outputs = True
        self.sparse = False
        self.latent = False
        self.n_u = 100
        self.model_specs = {
            "seed": self.seed,
            "continuous_kernel": self.continuous_kernel,
            "heteroskedastic_inputs": self.heteroskedastic_inputs,
            "heteroskedastic_outputs": self.heteroskedastic_outputs,
            "sparse": self.sparse,
            "n_u": self.n_u,
        }
        self.nlml_trace = []
        self._rejected = 0
        self._last_eval_theta = None
        self.n_refactor = 0
        self._theta_fitted = None
        self._draw_rng = None  # generator of the posterior draws' normals (draw_point_samples), seeded on first use

    # ------------------------------------------------------------------------------------------
    def fit(self, outputs=None, linear_dims=None, continuous_dims=None, continuous_levels=None,
            continuous_coords=None, categorical_dims=None, categorical_levels=None, additive=False,
            seed=None, continuous_kernel="ExpQuad", period=None, heteroskedastic_inputs=False,
            heteroskedastic_outputs=True, sparse=False, n_u=100, ARD=True, ls_bounds=None, mass=0.98,
            spec_kwargs=None, build_kwargs=None, MAP_kwargs=None):
        """``specify_model`` -> ``build_model`` -> ``find_MAP`` (reference :255-387)."""
        self.specify_model(outputs=outputs, linear_dims=linear_dims, continuous_dims=continuous_dims,
                           continuous_levels=continuous_levels, continuous_coords=continuous_coords,
                           categorical_dims=categorical_dims, categorical_levels=categorical_levels,
                           additive=additive, **(spec_kwargs or {}))
        self.build_model(seed=seed, continuous_kernel=continuous_kernel, period=period,
                         heteroskedastic_inputs=heteroskedastic_inputs,
                         heteroskedastic_outputs=heteroskedastic_outputs, sparse=sparse, n_u=n_u, ARD=ARD,
                         ls_bounds=ls_bounds, mass=mass, **(build_kwargs or {}))
        self.find_MAP(**(MAP_kwargs or {}))
        return self

    # -- helpers ---------------------------------------------------------------------------------------
    def _get_dim_indexes(self):
        dims = self.dims
        return {
            "l": [dims.index(d) for d in self.linear_dims],
            "s": [dims.index(d) for d in self.continuous_dims],
            "c": [dims.index(d) for d in self.categorical_dims],
            "p": dims.index(self.out_col) if self.out_col in dims else None,
        }

    def _prepare_lengthscales(self, X, *, ARD, ls_bounds=None, mass=0.98):
        X_s = X[:, self._get_dim_indexes()["s"]]
        lower = upper = None
        if ls_bounds is not None:
            zb = []
            for dim in self.continuous_dims:
                if dim in ls_bounds.names:
                    vals = np.atleast_1d(ls_bounds[dim].z.values().squeeze())
                    zb.append([None if np.isnan(b) else float(b) for b in vals])
            lower, upper = (list(t) for t in zip(*zb))
            if not ARD and (len(lower) != 1 or len(upper) != 1):
                raise ValueError("Bounds must be specified for only a single dimension if ARD is False")
        return get_ls_prior(X_s, ARD=ARD, lower=lower, upper=upper, mass=mass, device=self.device)

    # -- model declaration ---------------------------------------------------------------------------------
    def build_model(self, seed=None, continuous_kernel="ExpQuad", period=None, heteroskedastic_inputs=False,
                    heteroskedastic_outputs=True, sparse=False, n_u=100, ARD=True, ls_bounds=None, mass=0.98):
        """Declare the marginal GP (reference :468-583) and move the data into HBM.

        ``continuous_kernel``: one of the five stationary kinds, ``"Periodic"`` (``pm.gp.cov.Periodic``:
        ``eta^2 exp(-1/2 sum_d sin^2(pi (x_d - x'_d) / T_d) / ls_d^2)``) or ``"<kind>+Periodic"`` (the stationary kind on the inputs
        warped by ``u(x) = (sin(2 pi x / T), cos(2 pi x / T))``: ``r^2 = sum_d 4 sin^2(pi (x_d - x'_d) / T_d) / ls_d^2``).  All
        six periodic forms need ``period``: a parray with one layer per continuous dimension, read as the reference reads it
        (``period.z[dim + "_z"]``, reference :403, :431).  Build it with :func:`gumbi_amd.array_utils.make_deltas_parray`
        (``make_deltas_parray(stdzr=..., scale="natural", X=[T])``), as ``ls_bounds`` is built, so that ``.z`` is the period as a
        standardized STEP ``T / sigma`` rather than a standardized position.  Periods are data, not parameters: they are never
        optimised.  At most 8 continuous dimensions.

        ``"<kind>+Periodic"`` with several continuous dimensions is NOT what the reference evaluates: its inner kernel is
        declared with ``input_dim=2, active_dims=None`` (:427-429), so it reads only the first two warped columns -- the sines
        of the first two dimensions -- and is well-formed for one continuous dimension only.  Here every dimension contributes
        its own (sin, cos) pair with its own lengthscale, the form the construction intends; the two agree for one dimension.
        The lengthscale prior comes from the unwarped inputs, as in the reference."""
        if heteroskedastic_inputs:
            raise NotImplementedError("Heteroskedasticity over inputs is not yet implemented.")
        if sparse:
            raise NotImplementedError("The sparse (FITC) approximation is not part of the HIP backend.")
        periodic = [k + "+Periodic" for k in KERNEL_KINDS] + ["Periodic"]
        assert_in("Continuous kernel", continuous_kernel, list(KERNEL_KINDS) + periodic)
        kind, periodic_mode = resolve_kernel_name(continuous_kernel)
        periods = []
        if periodic_mode:
            if period is None:
                raise ValueError("Period must be specified for periodic kernel")
            if self.distributed:
                raise NotImplementedError("Periodic kernels with distributed=True: the multi-GPU driver does not carry the periods")
            if len(self.continuous_dims) > MAX_PERIODIC_DIMS:
                raise ValueError(f"a periodic kernel supports at most {MAX_PERIODIC_DIMS} continuous dimensions, "
                                 f"got {len(self.continuous_dims)}")
            missing = [dim for dim in self.continuous_dims if dim not in period.names]
            if missing:
                raise ValueError(f"period has no entry for the continuous dimension(s) {missing}")
            for dim in self.continuous_dims:
                zp = np.asarray(period.z[dim + "_z"].values(), dtype=float).ravel()
                if zp.size != 1 or not np.isfinite(zp[0]) or zp[0] <= 0:
                    raise ValueError(f"period of {dim!r} must be one finite positive number on the standardized scale, got {zp}")
                periods.append(float(zp[0]))

        X, y = self.get_shaped_data("mean")
        D_in = len(self.dims)
        assert X.shape[1] == D_in
        if not self.continuous_dims:
            raise ValueError("At least one continuous dimension is required")

        seed = self.seed if seed is None else seed
        self.seed = seed
        self.continuous_kernel = continuous_kernel
        self.heteroskedastic_inputs = heteroskedastic_inputs
        self.heteroskedastic_outputs = heteroskedastic_outputs
        self.sparse, self.n_u, self.latent = sparse, n_u, False
        self.model_specs = {"seed": seed, "continuous_kernel": continuous_kernel,
                            "heteroskedastic_inputs": heteroskedastic_inputs,
                            "heteroskedastic_outputs": heteroskedastic_outputs, "sparse": sparse, "n_u": n_u}
        if periodic_mode:
            # a periodic model cannot be rebuilt from its kernel's name alone: cross_validate rebuilds the training model
            # with build_model(**model_specs)
            self.model_specs["period"] = period
        self._ARD = ARD

        idx = self._get_dim_indexes()
        multi = self.out_col in self.categorical_dims
        coreg = [(i, len(self.categorical_levels[d])) for d, i in zip(self.categorical_dims, idx["c"])
                 if d != self.out_col]
        spec = KernelSpec(D=D_in, idx_cont=idx["s"], kind=kind, ard=ARD, idx_lin=idx["l"],
                          coreg=coreg, out_col=idx["p"] if multi else -1,
                          n_out=len(self.categorical_levels[self.out_col]) if multi else 0,
                          hetero_noise=bool(heteroskedastic_outputs), jitter=1e-6,
                          additive=bool(self.additive and coreg), periodic=periodic_mode, periods=periods)
        ls_params = self._prepare_lengthscales(X, ARD=ARD, ls_bounds=ls_bounds, mass=mass)

        # parameter blocks in the packing order of include/gumbi_hip.h
        blocks, k = [], 0

        def add(name, kind, shape):
            nonlocal k
            n = int(np.prod(shape)) if shape else 1
            blocks.append((name, kind, shape, slice(k, k + n)))
            k += n

        n_ls = len(idx["s"]) if ARD else 1
        add("ls_total", "pos", (n_ls,))
        add("η_total", "pos", ())
        add("σ", "pos", ())
        if idx["l"]:
            add("c_total", "real", (len(idx["l"]),))
            add("τ_total", "pos", ())
        for d, (_, L) in zip([d for d in self.categorical_dims if d != self.out_col], coreg):
            add(f"W_{d}", "real", (L, 2))
            add(f"κ_{d}", "pos", (L,))
        if multi:
            P = spec.n_out
            add(f"W_{self.out_col}", "real", (P, 2))
            add(f"κ_{self.out_col}", "pos", (P,))
            if spec.hetero_noise:
                add("W_Output_noise", "real", (P, 2))
                add("κ_Output_noise", "pos", (P,))
        if spec.additive:
            # one more continuous (+ linear) kernel per categorical dimension (reference :732-754),
            # appended in the order of include/gumbi_hip.h
            for d in [d for d in self.categorical_dims if d != self.out_col]:
                add(f"ls_{d}", "pos", (n_ls,))
                add(f"η_{d}", "pos", ())
                if idx["l"]:
                    add(f"c_{d}", "real", (len(idx["l"]),))
                    add(f"τ_{d}", "pos", ())
        assert k == spec.theta_size()

        self.model = HipModel(spec, ls_params, blocks, X, y)
        if self.engine is not None:
            self.engine.close()
        if self.distributed:
            from ..distributed import DistributedEngine

            self.engine = DistributedEngine(self.device, None if self.distributed is True else self.distributed)
        elif self.kronecker and spec.out_col >= 0 and not spec.additive and icm.aligned_outputs(X, spec):
            self.engine = icm.IcmEngine(device=self.device)
        else:
            self.engine = Engine(device=self.device)
        self.engine.set_data(X, y)
        self.engine.set_kernel(spec)
        # The levels of an additive model as term selections of the engine (bit 0: the global kernel, bit 1 + j: the kernel of
        # the j-th categorical dimension other than the output column); every other model has "total" alone.
        n_terms = 1 + len(coreg) if spec.additive else 1
        self.additive_levels = {"total": (1 << n_terms) - 1}
        if spec.additive:
            self.additive_levels["global"] = 1
            for j, d in enumerate(d for d in self.categorical_dims if d != self.out_col):
                self.additive_levels[d] = 1 << (1 + j)
        self.gp_dict = dict.fromkeys(self.additive_levels, self.engine)
        self.component_cov = self.component_levels = None
        self.MAP = None
        self._theta_fitted = None
        return self

    # -- priors, transforms ------------------------------------------------------------------------------------------
    def _initial_theta(self):
        """PyMC's default starting point: the moment of each prior, and the seeded draw for W
        (``initval`` at reference :459-460)."""
        m = self.model
        theta = np.zeros(m.spec.theta_size())
        for name, _kind, shape, sl in m.blocks:
            if name.startswith("ls_"):
                a, b = np.asarray(m.ls_params["alpha"]), np.asarray(m.ls_params["beta"])
                theta[sl] = np.where(a > 1, b / np.maximum(a - 1, 1e-300), b / (a + 1))
            elif name.startswith("η_"):
                theta[sl] = 2.0
            elif name == "σ":
                theta[sl] = 1.0
            elif name.startswith("c_"):
                theta[sl] = 0.0
            elif name.startswith("τ_"):
                theta[sl] = 10.0
            elif name.startswith("W_"):
                theta[sl] = np.random.default_rng(self.seed).standard_normal(size=shape).ravel()
            elif name.startswith("κ_"):
                theta[sl] = 1.5
        return theta

    def _log_prior(self, theta):
        """(value, d/dtheta) of the sum of log-prior densities on the natural scale."""
        m = self.model
        val, grad = 0.0, np.zeros_like(theta)
        for name, _kind, _shape, sl in m.blocks:
            x = theta[sl]
            if name.startswith("ls_"):
                a, b = np.asarray(m.ls_params["alpha"], float), np.asarray(m.ls_params["beta"], float)
                val += np.sum(a * np.log(b) - np.array([lgamma(v) for v in a]) - (a + 1) * np.log(x) - b / x)
                grad[sl] = -(a + 1) / x + b / x**2
            elif name.startswith("η_"):  # Gamma(2, 1)
                val += np.sum(np.log(x) - x)
                grad[sl] = 1.0 / x - 1.0
            elif name == "σ":  # Exponential(1)
                val += np.sum(-x)
                grad[sl] = -1.0
            elif name.startswith("c_"):  # Normal(0, 10)
                val += np.sum(-0.5 * np.log(2 * np.pi) - np.log(10.0) - 0.5 * (x / 10.0) ** 2)
                grad[sl] = -x / 100.0
            elif name.startswith("τ_"):  # HalfNormal(10)
                val += np.sum(0.5 * np.log(2 / np.pi) - np.log(10.0) - 0.5 * (x / 10.0) ** 2)
                grad[sl] = -x / 100.0
            elif name.startswith("W_"):  # Normal(0, 3)
                val += np.sum(-0.5 * np.log(2 * np.pi) - np.log(3.0) - 0.5 * (x / 3.0) ** 2)
                grad[sl] = -x / 9.0
            elif name.startswith("κ_"):  # Gamma(1.5, 1)
                val += np.sum(-lgamma(1.5) + 0.5 * np.log(x) - x)
                grad[sl] = 0.5 / x - 1.0
        return float(val), grad

    def _positive_mask(self):
        mask = np.zeros(self.model.spec.theta_size(), dtype=bool)
        for _name, kind, _shape, sl in self.model.blocks:
            if kind == "pos":
                mask[sl] = True
        return mask

    #: PyMC >= 4's ``find_MAP`` compiles ``model.logp(jacobian=False)`` (pymc/tuning/starting.py): the
    #: log-Jacobians of the log transforms are NOT in the objective.  True restates PyMC3.
    map_includes_jacobian = False

    def _objective(self, u, pos):
        """-(log-lik + log-prior [+ log|d theta/du|, see ``map_includes_jacobian``]) and its gradient
        w.r.t. the unconstrained u (u = log theta for the positive parameters)."""
        theta = np.where(pos, np.exp(np.clip(u, -700, 700)), u)
        eng = self.engine
        # from here on the engine's factor belongs to THIS theta (or to none): an evaluation that is rejected further
        # down must not leave `_last_eval_theta` pointing at an earlier point whose factor is gone
        self._last_eval_theta = None
        try:
            fused = getattr(eng, "evaluate", None)  # the single-GPU engine: one C call, no host round trip in between
            if fused is not None:
                nlml, g_nlml = fused(theta)
            else:
                eng.set_theta(theta)
                eng.factorize()
                nlml, g_nlml = eng.nlml(grad=True)
        except np.linalg.LinAlgError:  # covariance not positive definite at this theta: reject the step
            self._rejected += 1
            return _REJECTED, np.zeros_like(u)
        except ValueError as err:
            # parameters the engine refuses on their VALUE (a length scale or kappa that underflowed to zero,
            # an overflow to inf) are rejected steps as well; anything else -- call order, packing, shapes --
            # is a bug and must surface
            if "must be positive" in str(err) or "not finite" in str(err):
                self._rejected += 1
                return _REJECTED, np.zeros_like(u)
            raise
        lp, g_lp = self._log_prior(theta)
        J = 1.0 if self.map_includes_jacobian else 0.0
        f = nlml - lp - J * np.sum(u[pos])
        g = g_nlml - g_lp
        g = np.where(pos, g * theta - J, g)
        if not np.isfinite(f):
            self._rejected += 1
            return _REJECTED, np.zeros_like(u)
        self.nlml_trace.append(float(nlml))
        self._last_eval_theta = theta.copy()
        return float(f), g

    # -- fitting -----------------------------------------------------------------------------------------------------------
    def find_MAP(self, *args, start=None, theta=None, maxeval=5000, method="L-BFGS-B", progressbar=False,
                 **kwargs):
        """Maximum a posteriori hyper-parameters (reference :799-813, ``pm.find_MAP``).

        ``theta`` (natural-scale vector in ``include/gumbi_hip.h`` order, or a dict keyed by the
        MAP names) skips the optimisation and just installs the given hyper-parameters.
        ``start`` is a dict of natural-scale starting values keyed by MAP names."""
        assert self.model is not None, "build_model must be called before find_MAP"
        from scipy.optimize import minimize

        pos = self._positive_mask()
        theta0 = self._initial_theta()
        if start is not None:
            theta0 = self._theta_from_dict(start, theta0)
        self.nlml_trace = []
        self._rejected = 0
        self._last_eval_theta = None
        if theta is not None:
            th = self._theta_from_dict(theta, theta0) if isinstance(theta, dict) else np.asarray(theta, float)
            self.n_eval = 0
        else:
            u0 = theta0.copy()
            u0[pos] = np.log(theta0[pos])
            with _single_threaded_host_blas(self.engine):
                res = minimize(self._objective, u0, args=(pos,), jac=True, method=method,
                               options={"maxfun": int(maxeval), **kwargs.pop("options", {})}, **kwargs)
            th = np.where(pos, np.exp(res.x), res.x)
            self.n_eval = int(res.nfev)
            self.opt_result = res
            # pm.find_MAP reports what the optimiser did; a fit that never left the rejection plateau (every
            # evaluation non-PD: L-BFGS-B sees a zero gradient and "converges" at the start) or that scipy
            # flags as failed must not pass silently
            if res.fun >= _REJECTED or not self.nlml_trace:
                warnings.warn("find_MAP: no admissible evaluation -- the covariance was not positive definite at "
                              f"every one of the {self.n_eval} points tried; MAP is the starting point",
                              RuntimeWarning, stacklevel=2)
            elif not res.success and res.status != 1:  # status 1 = evaluation budget (maxeval) reached
                warnings.warn(f"find_MAP: L-BFGS-B stopped without converging ({res.message})", RuntimeWarning,
                              stacklevel=2)
        # leave the engine factorised at the MAP so predict() reuses the resident factor.  When the optimiser's
        # last evaluation was AT the MAP (the usual L-BFGS-B ending) that factorisation is still resident -- the
        # gradient puts the factor back together -- and nothing is recomputed (the reference factorises again
        # in every predict call, pymc/GP.py:845-847)
        current = getattr(self.engine, "factor_is_current", lambda: False)
        if self._last_eval_theta is not None and np.array_equal(th, self._last_eval_theta) and current():
            self.n_refactor = 0
        else:
            self.engine.set_theta(th)
            self.engine.factorize()
            self.n_refactor = 1
        self._theta_fitted = th
        self.MAP = self._theta_to_dict(th)
        return self.MAP

    def _theta_to_dict(self, theta):
        out = {}
        for name, kind, shape, sl in self.model.blocks:
            val = np.array(theta[sl]).reshape(shape) if shape else np.array(theta[sl][0])
            out[name] = val
            if kind == "pos":
                out[name + "_log__"] = np.log(val)
        return out

    def _theta_from_dict(self, dct, base):
        theta = np.array(base, dtype=float)
        for name, _kind, _shape, sl in self.model.blocks:
            if name in dct:
                theta[sl] = np.asarray(dct[name], dtype=float).ravel()
            elif name + "_log__" in dct:
                theta[sl] = np.exp(np.asarray(dct[name + "_log__"], dtype=float).ravel())
        return theta

    def sample(self, *args, **kwargs):
        raise NotImplementedError("NUTS sampling of hyper-parameters is not part of the HIP backend.")

    # -- prediction ------------------------------------------------------------------------------------------------------------
    def predict(self, points_array, with_noise=True, additive_level="total", **kwargs):
        """Posterior mean / variance at standardized points (reference :837-849): one call into
        ``gmb_predict`` against the factor left resident by :meth:`find_MAP`."""
        terms = self._level_terms(additive_level)
        if self.MAP is None or self.engine is None:
            raise ValueError("The model must be fit (find_MAP) before predicting")
        return self.engine.predict(np.asarray(points_array, dtype=np.float64), with_noise=with_noise, **terms)

    def _level_terms(self, additive_level):
        """The engine's term selection for ``additive_level`` as keyword arguments of its prediction calls: none for ``"total"``
        (the call without a selection, on any engine), ``terms=`` the level's mask otherwise (the reference raises for every
        level but "total", pymc/GP.py:839-841)."""
        levels = self.additive_levels if self.additive_levels is not None else {"total": 1}
        if additive_level not in levels:
            raise UnknownAdditiveLevel(f"Unknown additive_level {additive_level!r}: this model has the levels {list(levels)}")
        return {} if additive_level == "total" else {"terms": levels[additive_level]}

    # -- slope of the fitted surface --------------------------------------------------------------------------------------------
    def predict_grad(self, points_array, additive_level="total"):
        """Gradient of the posterior mean with respect to the standardized points, ``(M, D)`` with one column per model
        dimension in ``dims`` order (categorical columns and the output index: 0) -- the reference's autograd pass
        (botorch/GP.py:535-576) in closed form: one call into ``gmb_predict_grad`` against the factor left resident by
        :meth:`find_MAP`."""
        terms = self._level_terms(additive_level)
        if self.MAP is None or self.engine is None:
            raise ValueError("The model must be fit (find_MAP) before predicting")
        return self.engine.predict_grad(np.asarray(points_array, dtype=np.float64), **terms)

    def predict_points_grad(self, points, output=None, norm=True, additive_level="total"):
        """Slope of the fitted surface at a 1-D parray of points (reference botorch/GP.py:579-622): a parray with one layer
        ``δ[{y}]/δ[{x}]`` per output and continuous dimension, or, with ``norm=True``, one layer ``|∇|{y}`` per output (the
        Euclidean norm over the continuous dimensions).

        The slope is taken in the TRANSFORMED space: the standardized gradient times ``σ_y / σ_x`` of the standardizer.  As
        in the reference, log (or logit) transforms of inputs or outputs are NOT unwound -- for a log-transformed variable
        the layer is the slope with respect to (or of) its logarithm."""
        output = self._parse_prediction_output(output)
        points_array, tall, param_coords = self._prepare_points_for_prediction(points, output=output)
        grad_z = self.predict_grad(points_array, additive_level=additive_level)
        task = tall[self.out_col].values().squeeze() if param_coords is not None else None
        partials = {}
        for i, y_var in enumerate(output):
            rows = grad_z if task is None else grad_z[np.atleast_1d(task == param_coords[i])]
            σy = np.sqrt(self.stdzr[y_var]["σ2"])
            for x_var in self.continuous_dims:
                σx = np.sqrt(self.stdzr[x_var]["σ2"])
                partials[f"δ[{y_var}]/δ[{x_var}]"] = rows[:, self.dims.index(x_var)] * σy / σx
        grad = self.parray(**partials)
        return self._get_pgrad_norm(grad) if norm else grad

    def predict_grid_grad(self, output=None, categorical_levels=None, norm=True, additive_level="total"):
        """:meth:`predict_points_grad` on the grid :meth:`prepare_grid` left behind, in the grid's shape (reference
        botorch/GP.py:625-633)."""
        if self.grid_points is None:
            raise ValueError("Grid must first be specified with `prepare_grid`")
        points = self.grid_points
        if self.categorical_dims:
            points = self.append_categorical_points(points, categorical_levels=categorical_levels)
        return self.predict_points_grad(points, output=output, norm=norm, additive_level=additive_level).reshape(self.grid_parray.shape)

    # -- slope with uncertainty: the posterior of the derivative ----------------------------------------------------------------
    def predict_slope(self, points_array, additive_level="total", cov=False):
        """The posterior of the slope ``d f / d x`` of the latent function at standardized points: ``(dmean, dvar)``, ``(M, D)``
        each with one column per model dimension in ``dims`` order (categorical columns and the output index: 0), or
        ``(dmean, dvar, dcov)`` with ``cov=True``, ``dcov`` ``(M, D, D)`` the joint covariance of the partial derivatives at
        each point -- one call into ``gmb_predict_slope`` against the factor left resident by :meth:`find_MAP`.  ``dmean`` is
        :meth:`predict_grad`'s quantity; ``dvar`` is the variance OF the slope (the derivative of a GP is a GP), not the slope
        of the variance.  Matern-1/2 and Exponential kernels have no mean-square derivative: ``ValueError``."""
        terms = self._level_terms(additive_level)
        if self.MAP is None or self.engine is None:
            raise ValueError("The model must be fit (find_MAP) before predicting")
        kind, _ = resolve_kernel_name(self.continuous_kernel)
        if kind in ("Matern12", "Exponential"):
            raise ValueError(f"predict_slope: a GP with the {self.continuous_kernel} kernel is not mean-square differentiable -- "
                             "the process has no derivative (use ExpQuad, Matern52 or Matern32)")
        return self.engine.predict_slope(np.asarray(points_array, dtype=np.float64), cov=cov, **terms)

    def predict_points_slope(self, points, output=None, additive_level="total", joint=False):
        """Slope of the fitted surface WITH its uncertainty at a 1-D parray of points: a dict with one ``UncertainArray``
        ``δ[{y}]/δ[{x}]`` per output and continuous dimension (the layer names of :meth:`predict_points_grad`).  ``μ`` is the
        standardized slope times ``σ_y / σ_x`` of the standardizer, ``σ2`` its standardized variance times ``(σ_y / σ_x)^2``:
        is the effect of x different from zero here, where is the surface flat, which input matters most.  With
        ``joint=True``, :attr:`slope_cov` is set too: ``{output: (points, n_cont, n_cont)}``, the covariance between the
        partial slopes at each point in the same units, continuous dimensions in ``continuous_dims`` order.

        As in :meth:`predict_points_grad`, everything is in the TRANSFORMED space: log (or logit) transforms of inputs or
        outputs are NOT unwound.  The norm ``|∇|y`` gets no uncertainty here: the norm of a Gaussian vector is not Gaussian."""
        output = self._parse_prediction_output(output)
        points_array, tall, param_coords = self._prepare_points_for_prediction(points, output=output)
        res = self.predict_slope(points_array, additive_level=additive_level, cov=joint)
        task = tall[self.out_col].values().squeeze() if param_coords is not None else None
        cols = [self.dims.index(x_var) for x_var in self.continuous_dims]
        σx = np.array([np.sqrt(self.stdzr[x_var]["σ2"]) for x_var in self.continuous_dims])
        slopes, covs = {}, {}
        for i, y_var in enumerate(output):
            rows = slice(None) if task is None else np.atleast_1d(task == param_coords[i])
            σy = np.sqrt(self.stdzr[y_var]["σ2"])
            for k, x_var in enumerate(self.continuous_dims):
                name = f"δ[{y_var}]/δ[{x_var}]"
                slopes[name] = UncertainArray(name, res[0][rows][:, cols[k]] * σy / σx[k], res[1][rows][:, cols[k]] * (σy / σx[k]) ** 2,
                                              stdzr=self.stdzr)
            if joint:
                covs[y_var] = res[2][rows][:, cols][:, :, cols] * (σy**2 / np.outer(σx, σx))
        self.slope_cov = covs if joint else None
        return slopes

    def predict_grid_slope(self, output=None, categorical_levels=None, additive_level="total", joint=False):
        """:meth:`predict_points_slope` on the grid :meth:`prepare_grid` left behind, every array in the grid's shape
        (:attr:`slope_cov`: the grid's shape, then ``(n_cont, n_cont)``)."""
        if self.grid_points is None:
            raise ValueError("Grid must first be specified with `prepare_grid`")
        points = self.grid_points
        if self.categorical_dims:
            points = self.append_categorical_points(points, categorical_levels=categorical_levels)
        slopes = self.predict_points_slope(points, output=output, additive_level=additive_level, joint=joint)
        shape = self.grid_parray.shape
        if joint:
            self.slope_cov = {y: c.reshape(*shape, *c.shape[1:]) for y, c in self.slope_cov.items()}
        return {name: ua.reshape(shape) for name, ua in slopes.items()}

    @staticmethod
    def _get_pgrad_norm(pgrad):
        """``|∇|{y}`` per output from the layers ``δ[{y}]/δ[{x}]`` of ``pgrad``."""
        by_output = {}
        for name in pgrad.names:
            by_output.setdefault(name.split("/")[0].removeprefix("δ[").removesuffix("]"), []).append(name)
        norms = {f"|∇|{y}": np.sqrt(sum(np.square(pgrad[name].values()) for name in names)) for y, names in by_output.items()}
        return parray(**norms, stdzr=pgrad.stdzr)

    # -- gradient-based proposal over the continuous inputs ---------------------------------------------------------------------
    def _acquisition_problem(self, output, acquisition, maximize, categorical_levels, beta):
        """What :meth:`acquisition_with_grad` and :meth:`propose_continuous` share: the acquisition ``f(mu, var, maximize)``,
        the continuous dims with their columns of a model point, and ``full(Z)``, which completes (M, n_cont) standardized
        continuous coordinates to (M, D) points with the fixed columns (categories, the output index)."""
        from .. import acquisition as acq

        if self.distributed:
            raise NotImplementedError("the acquisition's gradient is not built for distributed GPs (the factor is spread over ranks)")
        if self.MAP is None or self.engine is None:
            raise ValueError("The model must be fit (find_MAP) before proposing")
        outputs = self._parse_prediction_output(output)
        if len(outputs) != 1:
            raise ValueError(f"an acquisition is optimised for ONE output: pass output= one of {outputs}")
        cont = list(self.continuous_dims)
        cols = [self.dims.index(d) for d in cont]
        template = self.parray(**{d: np.array([0.0]) for d in cont}, stdzd=True)
        if set(self.categorical_dims) - {self.out_col}:
            if categorical_levels is None:
                raise AttributeError("Must specify level for every categorical dimension")
            template = self.append_categorical_points(template, categorical_levels)
        row, _, _ = self._prepare_points_for_prediction(template, output=outputs)
        row = np.asarray(row, float)[0]

        def full(Z):
            P = np.tile(row, (len(Z), 1))
            P[:, cols] = Z
            return P

        kwargs = {}
        if acquisition in ("EI", "qEI"):  # the incumbent: the best observed standardized value of this output
            y = np.asarray(self.model.y, float)
            if self.out_col in self.categorical_dims:
                oc = self.dims.index(self.out_col)
                y = y[np.asarray(self.model.X, float)[:, oc] == row[oc]]
            kwargs["best"] = float(np.max(y) if maximize else np.min(y))
        elif beta is not None:
            kwargs["beta"] = beta
        return acq.get(acquisition, **kwargs), cont, cols, full

    def acquisition_with_grad(self, points_z, output=None, acquisition="EI", maximize=True, categorical_levels=None, beta=None,
                              _problem=None):
        """Acquisition value (M,) and its gradient (M, n_cont) with respect to the STANDARDIZED continuous coordinates
        ``points_z`` (M, n_cont, in ``continuous_dims`` order), on the noise-free posterior: ONE ``engine.predict_with_grad``
        call, chained with the acquisition's gradient in (mu, sigma^2).  Larger is better for both settings of ``maximize``
        (``"EI"`` is log-EI).  This is the objective :meth:`propose_continuous` optimises."""
        f, cont, cols, full = _problem or self._acquisition_problem(output, acquisition, maximize, categorical_levels, beta)
        Z = np.asarray(points_z, float).reshape(-1, len(cont))
        mu, var, dmu, dvar = self.engine.predict_with_grad(full(Z), with_noise=False)
        value, d_mu, d_var = f(mu, var, maximize)
        return value, d_mu[:, None] * dmu[:, cols] + d_var[:, None] * dvar[:, cols]

    def propose_continuous(self, output=None, acquisition="EI", maximize=True, bounds=None, categorical_levels=None,
                           num_restarts=10, raw_samples=512, seed=None, q=1, sequential=False, fantasy="mean", **optim_kwargs):
        """Next point to measure by optimising an acquisition function over the CONTINUOUS inputs (the reference's
        ``BotorchGP.propose``, botorch/GP.py, whose keywords this follows): multi-start L-BFGS-B on analytic ``"EI"`` (in its log
        form) or ``"UCB"`` (``beta=`` in ``optim_kwargs``, default 2) of the noise-free posterior, in standardized units.

        ``raw_samples`` seeded uniform points inside ``bounds`` are scored in one ``predict`` call and the best
        ``num_restarts`` become the starts; the restarts are then optimised in lock step -- one ``scipy.optimize.minimize``
        over their concatenated coordinates with the summed negative acquisition -- and every objective evaluation is ONE
        ``engine.predict_with_grad`` call at ``M = num_restarts`` (:meth:`acquisition_with_grad`) against the factor
        :meth:`find_MAP` left resident.

        ``bounds``: a parray with two entries (lower, upper) per continuous dimension; default: the range of the training data.
        Categorical coordinates are fixed through ``categorical_levels`` (as in :meth:`append_categorical_points`); with
        several outputs ``output`` names the one to optimise.  The incumbent of EI is the best observed standardized value of
        that output.  Returns the best candidate -- of the optimised restarts and their starts -- as a parray in natural units
        and sets :attr:`proposal`, :attr:`proposal_acquisition` (its acquisition value) and :attr:`optimization_bounds`
        (standardized ``(lower, upper)`` in ``continuous_dims`` order); for diagnosis also :attr:`proposal_result` (scipy's
        result of the lock-step run) and :attr:`proposal_raw_acquisition` (the raw samples' scores).  Remaining
        ``optim_kwargs`` go to L-BFGS-B's ``options``.

        ``q > 1`` needs ``sequential=True`` (the reference's keyword): a greedy batch.  Each of the ``q`` picks is the single-point
        search above; the pick is then appended to the resident factor (``engine.append``: a bordered update, no
        re-factorisation) with its noise-free posterior mean as the observation -- ``fantasy="mean"``, the Kriging believer; for EI
        the fantasy enters the incumbent when it is better -- so that the next search sees the posterior conditioned on it.
        After the last pick (which needs no fantasy: ``q - 1`` appends) the engine is truncated back to the real observations,
        whatever happened in between.  Returns a parray of ``q`` points; :attr:`proposal_acquisition` is then the list of the
        ``q`` acquisition values, each under the posterior its search saw (a fantasy at the mean of a model WITH observation noise
        shrinks the variance s^2 at its pick to s^2 sigma^2 / (s^2 + sigma^2) and leaves the mean: where the data have settled the
        surface the picks of a batch can lie close together), :attr:`proposal_result` and
        :attr:`proposal_raw_acquisition` those of the last search.  Not for the Kronecker path (pass ``kronecker=False``)."""
        q = int(q)
        if q != 1 and not sequential:
            raise NotImplementedError("propose_continuous: q > 1 needs a Monte-Carlo batch acquisition, which is not built "
                                      "(sequential=True proposes a greedy batch)")
        if q < 1:
            raise ValueError(f"q must be >= 1, got {q}")
        if q > 1 and fantasy != "mean":
            raise NotImplementedError(f"propose_continuous: fantasy={fantasy!r}; only 'mean' (the Kriging believer) is built")
        if q > 1 and self.distributed:
            raise NotImplementedError("propose_continuous(sequential=True): the factor of a distributed GP is spread over the ranks; "
                                      "the fantasies' bordered update works on one device's complete factor")
        if q > 1 and isinstance(self.engine, icm.IcmEngine):
            raise NotImplementedError("propose_continuous(sequential=True): the Kronecker path holds P systems over the SAME inputs; "
                                      "a fantasy of one output would break that alignment (pass kronecker=False)")
        beta = optim_kwargs.pop("beta", None)
        problem = self._acquisition_problem(output, acquisition, maximize, categorical_levels, beta)
        f, cont, cols, full = problem
        num_restarts, raw_samples = int(num_restarts), max(int(raw_samples), int(num_restarts))

        # standardized bounds, one entry per continuous dim
        if bounds is None:
            Xc = np.asarray(self.model.X, float)[:, cols]
            lo, hi = Xc.min(axis=0), Xc.max(axis=0)
        else:
            bz = bounds.z
            both = np.array([np.asarray(bz[d + "_z"].values(), float).ravel() for d in cont])
            if both.shape != (len(cont), 2):
                raise ValueError("bounds must hold two entries (lower, upper) per continuous dimension")
            lo, hi = both.min(axis=1), both.max(axis=1)
        self.optimization_bounds = (lo.copy(), hi.copy())

        rng = np.random.default_rng(self.seed if seed is None else seed)
        options = {"maxiter": 200, **optim_kwargs.pop("options", {}), **optim_kwargs}
        if q == 1:
            z, value = self._propose_one(problem, lo, hi, rng, num_restarts, raw_samples, maximize, options)
            self.proposal_acquisition = value
            self.proposal = self.parray(**{d: np.array([z[k]]) for k, d in enumerate(cont)}, stdzd=True)
            return self.proposal

        # greedy batch: condition the resident factor on each pick's posterior mean before the next search
        n_real, X_real, y_real = len(self.model.y), self.model.X, self.model.y
        picks, values, grown = [], [], False
        try:
            for i in range(q):
                if i > 0:  # (the incumbent of EI follows the fantasies)
                    problem = self._acquisition_problem(output, acquisition, maximize, categorical_levels, beta)
                    full = problem[3]
                z, value = self._propose_one(problem, lo, hi, rng, num_restarts, raw_samples, maximize, options)
                picks.append(z)
                values.append(value)
                if i + 1 < q:
                    point = full(z[None, :])
                    mean, _ = self.engine.predict(point, with_noise=False)
                    grown = True  # (also when the append fails half-way: the engine's data may have the new size)
                    self.engine.append(point, mean)
                    self.model.X = np.vstack([self.model.X, point])
                    self.model.y = np.concatenate([self.model.y, np.asarray(mean, float)])
        except BaseException:
            # the search's (or a fantasy's) error is the one to report: the clean-up below must not replace it
            self.model.X, self.model.y = X_real, y_real
            if grown:
                try:
                    self._drop_fantasies(n_real)
                except Exception as err:  # noqa: BLE001
                    warnings.warn(f"propose_continuous: restoring the engine to its {n_real} observations failed ({err}); "
                                  "call build_model / find_MAP again", RuntimeWarning, stacklevel=2)
            raise
        self.model.X, self.model.y = X_real, y_real
        if grown:
            self._drop_fantasies(n_real)
        picks = np.array(picks)
        self.proposal_acquisition = values
        self.proposal = self.parray(**{d: picks[:, k] for k, d in enumerate(cont)}, stdzd=True)
        return self.proposal

    def _drop_fantasies(self, n_real):
        """Back to the ``n_real`` real observations with a valid factor: a truncation of the resident factor, or -- behind a
        fantasy whose append was not positive definite, which leaves no factor -- the cut data factorised again (as
        :meth:`condition_on` does)."""
        self.engine.truncate(n_real)
        if not self.engine.factor_is_current():
            self.engine.factorize()

    def _propose_one(self, problem, lo, hi, rng, num_restarts, raw_samples, maximize, options):
        """One single-point search of :meth:`propose_continuous` against the engine's present posterior: the best candidate's
        standardized continuous coordinates and its acquisition value."""
        from scipy.optimize import minimize

        f, cont, cols, full = problem
        raw = lo + (hi - lo) * rng.random((raw_samples, len(cont)))
        mu, var = self.engine.predict(full(raw), with_noise=False)
        raw_value = f(mu, var, maximize)[0]
        starts = raw[np.argsort(-raw_value, kind="stable")[:num_restarts]]

        def objective(z):
            value, grad = self.acquisition_with_grad(z.reshape(num_restarts, len(cont)), maximize=maximize, _problem=problem)
            return -float(np.sum(value)), -grad.ravel()

        res = minimize(objective, starts.ravel(), jac=True, method="L-BFGS-B",
                       bounds=list(zip(np.tile(lo, num_restarts), np.tile(hi, num_restarts))), options=options)
        cand = np.clip(np.vstack([res.x.reshape(num_restarts, len(cont)), starts]), lo, hi)
        mu, var = self.engine.predict(full(cand), with_noise=False)
        value = f(mu, var, maximize)[0]
        best = int(np.argmax(value))
        self.proposal_result = res
        self.proposal_raw_acquisition = raw_value
        return cand[best], float(value[best])

    # -- joint batch proposals: Monte-Carlo q-EI on per-batch joint posteriors -----------------------------------------------------
    def batch_acquisition_with_grad(self, batches_z, output=None, acquisition="qEI", maximize=True, categorical_levels=None,
                                    mc_samples=256, seed=None, jitter=1e-6, _problem=None, _base=None):
        """Batch acquisition value (B,) and its gradient (B, q, n_cont) with respect to the STANDARDIZED continuous coordinates
        ``batches_z`` (B, q, n_cont, in ``continuous_dims`` order) of B batches of q points, on the noise-free joint posterior of
        each batch: ONE ``engine.predict_batches`` call, chained with the acquisition's adjoints in (mean, cov)

            grad_j = mean_bar_j dmean_j + cov_bar_jj dcov[j, j] + 2 sum_{l != j} cov_bar_jl dcov[j, l]

        ``"qEI"`` is the log of the Monte-Carlo expected improvement of the batch as a whole on ``mc_samples`` fixed base samples
        (:func:`gumbi_amd.acquisition.batch_expected_improvement`; scrambled Sobol points under ``seed``); larger is better for
        both settings of ``maximize``.  This is the objective :meth:`propose_batch` optimises -- the analogue of
        :meth:`acquisition_with_grad`."""
        from .. import acquisition as acq

        f, cont, cols, full = _problem or self._acquisition_problem(output, acquisition, maximize, categorical_levels, None)
        Z = np.asarray(batches_z, float)
        if Z.ndim != 3 or Z.shape[2] != len(cont):
            raise ValueError(f"batches_z must be (B, q, {len(cont)}), got {Z.shape}")
        B, q, nc = Z.shape
        base = acq.sobol_normals(mc_samples, q, seed=self.seed if seed is None else seed) if _base is None else _base
        mean, cov, dmean, dcov = self.engine.predict_batches(full(Z.reshape(B * q, nc)), q, jitter=jitter, grad=True)
        value, mean_bar, cov_bar = f(mean, cov, base, maximize)
        weight = 2.0 * cov_bar
        idx = np.arange(q)
        weight[:, idx, idx] = cov_bar[:, idx, idx]
        grad = mean_bar[:, :, None] * dmean[:, :, cols] + np.einsum("bjl,bjld->bjd", weight, dcov[:, :, :, cols])
        return value, grad

    def propose_batch(self, q, output=None, acquisition="qEI", maximize=True, bounds=None, categorical_levels=None, num_restarts=10,
                      raw_samples=512, mc_samples=256, seed=None, **optim_kwargs):
        """A batch of ``q`` points to measure next, optimised AS A WHOLE against the correlation between its own points (the
        reference's ``BotorchGP.propose(q=.., mc_samples=256, sequential=False)``, botorch/GP.py:652): multi-start L-BFGS-B on the
        Monte-Carlo log q-EI of the batch's joint noise-free posterior, in standardized units.  The greedy batch of
        :meth:`propose_continuous` (``sequential=True``) conditions on one pick at a time; this one moves all q points together.

        ``raw_samples`` seeded uniform batches inside ``bounds`` are scored in ONE values-only ``engine.predict_batches`` call and
        the best ``num_restarts`` become the starts; the restarts are optimised in lock step -- one ``scipy.optimize.minimize``
        over their ``num_restarts x q x n_cont`` coordinates with the summed negative acquisition -- and every objective
        evaluation is ONE ``engine.predict_batches`` call at ``B = num_restarts`` (:meth:`batch_acquisition_with_grad`) against
        the factor :meth:`find_MAP` left resident.  The ``mc_samples`` base samples are drawn once (scrambled Sobol under the
        seed) and stay fixed, so the objective is deterministic.

        Bounds, the incumbent and the choice of ``output`` follow :meth:`propose_continuous`.  Returns the best batch -- of the
        optimised restarts and their starts -- as a parray of ``q`` points in natural units and sets :attr:`proposal`,
        :attr:`proposal_acquisition` (its acquisition value), :attr:`optimization_bounds`, :attr:`proposal_result` and
        :attr:`proposal_raw_acquisition` (the raw batches' scores).  Remaining ``optim_kwargs`` go to L-BFGS-B's ``options``.
        ``1 <= q <= 16``.  Not for the Kronecker path (pass ``kronecker=False``) or distributed GPs."""
        from scipy.optimize import minimize

        from .. import acquisition as acq

        q = int(q)
        if q < 1 or q > 16:
            raise ValueError(f"propose_batch: q must be 1 .. 16, got {q}")
        if acquisition != "qEI":
            raise ValueError(f'propose_batch: acquisition must be "qEI", got {acquisition!r}')
        if isinstance(self.engine, icm.IcmEngine):
            raise NotImplementedError("propose_batch: the joint posteriors of batches are not built for the Kronecker engine "
                                      "(pass kronecker=False)")
        problem = self._acquisition_problem(output, acquisition, maximize, categorical_levels, None)
        f, cont, cols, full = problem
        nc = len(cont)
        num_restarts, raw_samples = int(num_restarts), max(int(raw_samples), int(num_restarts))

        # standardized bounds, one entry per continuous dim (as propose_continuous)
        if bounds is None:
            Xc = np.asarray(self.model.X, float)[:, cols]
            lo, hi = Xc.min(axis=0), Xc.max(axis=0)
        else:
            bz = bounds.z
            both = np.array([np.asarray(bz[d + "_z"].values(), float).ravel() for d in cont])
            if both.shape != (nc, 2):
                raise ValueError("bounds must hold two entries (lower, upper) per continuous dimension")
            lo, hi = both.min(axis=1), both.max(axis=1)
        self.optimization_bounds = (lo.copy(), hi.copy())

        rng = np.random.default_rng(self.seed if seed is None else seed)
        options = {"maxiter": 200, **optim_kwargs.pop("options", {}), **optim_kwargs}
        base = acq.sobol_normals(mc_samples, q, seed=int(rng.integers(2**31 - 1)))

        def score(batches):  # values only: (B, q, nc) -> (B,)
            mean, cov = self.engine.predict_batches(full(batches.reshape(-1, nc)), q, grad=False)
            return f(mean, cov, base, maximize)[0]

        raw = lo + (hi - lo) * rng.random((raw_samples, q, nc))
        raw_value = score(raw)
        starts = raw[np.argsort(-raw_value, kind="stable")[:num_restarts]]

        def objective(z):
            value, grad = self.batch_acquisition_with_grad(z.reshape(num_restarts, q, nc), maximize=maximize, _problem=problem, _base=base)
            return -float(np.sum(value)), -grad.ravel()

        res = minimize(objective, starts.ravel(), jac=True, method="L-BFGS-B",
                       bounds=list(zip(np.tile(lo, num_restarts * q), np.tile(hi, num_restarts * q))), options=options)
        cand = np.clip(np.concatenate([res.x.reshape(num_restarts, q, nc), starts]), lo, hi)
        value = score(cand)
        best = int(np.argmax(value))
        self.proposal_result = res
        self.proposal_raw_acquisition = raw_value
        self.proposal_acquisition = float(value[best])
        self.proposal = self.parray(**{d: cand[best][:, k] for k, d in enumerate(cont)}, stdzd=True)
        return self.proposal

    # -- pathwise posterior draws: function samples and Thompson batches -----------------------------------------------------------
    def _paths_problem(self, output, what):
        """What :meth:`draw_paths` and :meth:`propose_thompson` share: the one output, the continuous dims with their columns
        of a model point, and ``full(Z)`` as :meth:`_acquisition_problem` makes it (no categorical level to fix: models with
        categorical dimensions are outside the pathwise draws' scope)."""
        if self.distributed:
            raise NotImplementedError(f"{what}: pathwise posterior draws are not built for distributed GPs (the factor is spread over ranks)")
        if isinstance(self.engine, icm.IcmEngine):
            raise NotImplementedError(f"{what}: pathwise posterior draws are not built for the Kronecker path (pass kronecker=False)")
        if self.MAP is None or self.engine is None:
            raise ValueError(f"The model must be fit (find_MAP) before {what}")
        outputs = self._parse_prediction_output(output)
        if len(outputs) != 1:
            raise ValueError(f"{what} works on ONE output: pass output= one of {outputs}")
        cont = list(self.continuous_dims)
        cols = [self.dims.index(d) for d in cont]
        template = self.parray(**{d: np.array([0.0]) for d in cont}, stdzd=True)
        row, _, _ = self._prepare_points_for_prediction(template, output=outputs)
        row = np.asarray(row, float)[0]

        def full(Z):
            P = np.tile(row, (len(Z), 1))
            P[:, cols] = Z
            return P

        return outputs, cont, cols, full

    def draw_paths(self, n_draws=16, n_features=2048, seed=None, antithetic=False, output=None):
        """``n_draws`` posterior FUNCTION draws (:class:`PosteriorPaths`) by pathwise conditioning (Matheron's rule; DESIGN
        §3.20): a prior draw from ``n_features`` random Fourier features plus an exact-kernel update against the data, prepared
        by one solve with ``n_draws`` right-hand sides against the factor :meth:`find_MAP` left resident.  Afterwards a draw is
        a function: it can be evaluated at any points, any number of times, at O(N + n_features) per point and draw -- on a
        whole :meth:`prepare_grid` grid, where :meth:`draw_grid_samples` needs the grid's joint covariance.  The draws are of
        the latent function (no observation noise).  The random-feature prior is an approximation (error O(1 / sqrt(n_features))
        in the prior covariance); the data term uses the exact kernel.  Reproducible from ``seed`` (default: the GP's);
        ``antithetic=True`` draws in pairs that mirror each other around the posterior mean.

        The paths live on the engine until the model is refit, conditioned on new data or another set is drawn: one set at a
        time.  One stationary kernel over the continuous dimensions only (no linear or categorical dimensions, one output, not
        additive, not periodic): anything else is refused."""
        from .. import pathwise

        outputs, cont, cols, full = self._paths_problem(output, "draw_paths")
        spec = self.model.spec
        omega, phase, w, eps = pathwise.path_inputs(spec.kind, int(n_draws), int(n_features), len(spec.idx_cont), len(self.model.y),
                                                    self.seed if seed is None else seed, antithetic=antithetic)
        generation = self.engine.paths_prepare(omega, phase, w, eps)
        return PosteriorPaths(self, outputs, cont, cols, full, int(n_draws), generation)

    def propose_thompson(self, q, output=None, maximize=True, bounds=None, num_restarts=10, raw_samples=512, n_features=2048, seed=None,
                         **optim_kwargs):
        """A batch of ``q`` points by Thompson sampling: ``q`` posterior function draws (:meth:`draw_paths`), each maximised (or
        minimised) over the continuous inputs inside ``bounds`` -- a plate-sized batch at the cost of ONE solve, where
        :meth:`propose_batch` stops at 16 points and the greedy batch of :meth:`propose_continuous` pays a bordered update and a
        search per pick.

        ONE ``engine.paths_eval`` call scores ``raw_samples`` seeded uniform points under all ``q`` draws; the best
        ``num_restarts`` of each draw become its starts; all ``q x num_restarts`` starts are optimised in lock step by one
        L-BFGS-B run over their coordinates, every objective evaluation ONE ``engine.paths_eval_own`` call.  Per draw the best
        of its optimised points and its starts is returned: a parray of ``q`` points in natural units, also in
        :attr:`proposal`; :attr:`proposal_acquisition` holds each point's value under its own draw (standardized units),
        :attr:`proposal_raw_acquisition` the raw samples' ``(q, raw_samples)`` values, :attr:`proposal_result` scipy's result.
        Bounds and the choice of ``output`` follow :meth:`propose_continuous`; remaining ``optim_kwargs`` go to L-BFGS-B's
        ``options``."""
        from scipy.optimize import minimize

        q = int(q)
        if q < 1 or q > 512:
            raise ValueError(f"propose_thompson: q must be 1 .. 512, got {q}")
        rng = np.random.default_rng(self.seed if seed is None else seed)
        paths = self.draw_paths(q, n_features=n_features, seed=int(rng.integers(2**31 - 1)), output=output)
        cont, cols, full = paths.continuous_dims, paths._cols, paths._full
        nc = len(cont)
        num_restarts, raw_samples = int(num_restarts), max(int(raw_samples), int(num_restarts))
        if bounds is None:
            Xc = np.asarray(self.model.X, float)[:, cols]
            lo, hi = Xc.min(axis=0), Xc.max(axis=0)
        else:
            bz = bounds.z
            both = np.array([np.asarray(bz[d + "_z"].values(), float).ravel() for d in cont])
            if both.shape != (nc, 2):
                raise ValueError("bounds must hold two entries (lower, upper) per continuous dimension")
            lo, hi = both.min(axis=1), both.max(axis=1)
        self.optimization_bounds = (lo.copy(), hi.copy())
        options = {"maxiter": 200, **optim_kwargs.pop("options", {}), **optim_kwargs}
        sign = 1.0 if maximize else -1.0

        raw = lo + (hi - lo) * rng.random((raw_samples, nc))
        raw_value = paths._own_engine().paths_eval(full(raw))  # (q, raw_samples)
        order = np.argsort(-sign * raw_value, axis=1, kind="stable")[:, :num_restarts]
        starts = raw[order]  # (q, num_restarts, nc)
        draw = np.repeat(np.arange(q, dtype=np.int32), num_restarts)

        def objective(z):
            value, grad = paths.value_and_grad(z.reshape(q * num_restarts, nc), draw)
            return -sign * float(np.sum(value)), -sign * grad.ravel()

        res = minimize(objective, starts.ravel(), jac=True, method="L-BFGS-B",
                       bounds=list(zip(np.tile(lo, q * num_restarts), np.tile(hi, q * num_restarts))), options=options)
        cand = np.clip(np.concatenate([res.x.reshape(q, num_restarts, nc), starts], axis=1), lo, hi)  # (q, 2 num_restarts, nc)
        value, _ = paths.value_and_grad(cand.reshape(-1, nc), np.repeat(np.arange(q, dtype=np.int32), 2 * num_restarts), grad=False)
        value = value.reshape(q, 2 * num_restarts)
        best = np.argmax(sign * value, axis=1)
        picks = cand[np.arange(q), best]
        self.proposal_result = res
        self.proposal_raw_acquisition = raw_value
        self.proposal_acquisition = value[np.arange(q), best]
        self.proposal_paths = paths
        self.proposal = self.parray(**{d: picks[:, k] for k, d in enumerate(cont)}, stdzd=True)
        return self.proposal

    def _shaped_rows(self):
        """:meth:`get_shaped_data` for a table of ANY number of rows: ``(K, D)`` and ``(K,)`` -- the base method squeezes a
        one-row table of a single-output model to a 0-d y (and masks X with it into three dimensions)."""
        self.X, self.y = self.get_structured_data("mean")
        if self.out_col in self.dims:
            return self.get_shaped_data("mean")  # (stacked with hstack / vstack: already 1-D and 2-D)
        y = np.atleast_1d(np.asarray(self.y.z.values(), dtype=np.float64).squeeze())
        xz = self.X.z
        X = np.column_stack([np.atleast_1d(np.asarray(xz[dim + "_z"].values(), dtype=np.float64).squeeze()) for dim in self.dims])
        X = X.reshape(-1, len(self.dims))
        keep = ~np.isnan(y)
        return np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep])

    # -- new observations under the fitted hyper-parameters ---------------------------------------------------------------------
    def condition_on(self, new_data, refit=False):
        """Absorb further measurements into the fitted GP WITHOUT re-factorising: the rows of ``new_data`` -- a wide-form DataFrame,
        or a DataSet, with the columns of ``gp.data`` -- are appended to the resident Cholesky factor (``engine.append``: a bordered
        update, O(N^2 K) instead of O(N^3)) under the hyper-parameters :attr:`MAP`, which stay as they are.

        The rows are standardized with the EXISTING standardizer and coded with the fitted model's own levels and coordinates
        (a categorical level, or a filter value, the model has not seen is a ``ValueError``; new values of a numeric continuous
        dimension join its levels).  ``self.data`` becomes the merged DataSet with the same standardizer and specs; ``model.X``
        and ``model.y`` gain the rows in the engine's order (behind the old ones).  Cached predictions, the grid and the
        structured-data cache are dropped.  The lengthscale prior keeps the pairwise-distance limits of the data the model was
        built on.  ``refit=True`` then runs ``find_MAP(start=self.MAP)`` on the merged data.  Returns ``self``.

        Kronecker and distributed GPs raise ``NotImplementedError`` (build with ``kronecker=False``)."""
        import pandas as pd

        if self.distributed:
            raise NotImplementedError("condition_on: the factor of a distributed GP is spread over the ranks; the bordered update "
                                      "works on one device's complete factor")
        if isinstance(self.engine, icm.IcmEngine):
            raise NotImplementedError("condition_on: the Kronecker path holds P systems over the SAME inputs; new observations "
                                      "would break that alignment (pass kronecker=False)")
        if self.model is None or self.MAP is None or self.engine is None:
            raise ValueError("The model must be fit (find_MAP) before it can be conditioned on new data")
        wide = pd.DataFrame(new_data.data if isinstance(new_data, DataSet) else new_data)
        columns = list(self.data.data.columns)
        missing = [c for c in columns if c not in wide.columns]
        if missing:
            raise ValueError(f"new_data lacks the column(s) {missing} of the GP's data")
        wide = wide[columns].reset_index(drop=True)
        if len(wide) == 0:
            return self

        # the fitted model's levels: categorical and filter values must be known, numeric continuous values join their levels
        levels, coords = dict(self.continuous_levels), dict(self.continuous_coords)
        for dim, known in self.filter_dims.items():
            if dim != self.out_col and not wide[dim].isin(known).all():
                raise ValueError(f"new_data[{dim!r}] holds values other than {known}, which the model was filtered to")
        for dim in self.categorical_dims:
            if dim == self.out_col:
                continue
            unseen = sorted(set(wide[dim].unique().tolist()) - set(self.categorical_levels[dim]))
            if unseen:
                raise ValueError(f"new_data[{dim!r}] holds level(s) {unseen} the fitted model has not seen "
                                 f"(its levels: {self.categorical_levels[dim]})")
        for dim in self.continuous_dims:
            fresh = [v for v in wide[dim].unique().tolist() if v not in coords[dim]]
            if not fresh:
                continue
            if not all(k is v or k == v for k, v in coords[dim].items()) or wide[dim].dtype.kind not in "fiu":
                raise ValueError(f"new_data[{dim!r}] holds level(s) {fresh} without coordinates in the fitted model")
            levels[dim] = list(levels[dim]) + fresh
            coords[dim] = {**coords[dim], **{v: v for v in fresh}}

        # the new rows as the engine takes them: shaped by the model's own plumbing on a DataSet that shares the standardizer
        old = (self.data, self.continuous_levels, self.continuous_coords, self._structured_cache, self.X, self.y)
        try:
            self.data = DataSet(wide, **self.data.specs)
            self.continuous_levels, self.continuous_coords, self._structured_cache = levels, coords, None
            X_new, y_new = self._shaped_rows()
        finally:
            self.data, self.continuous_levels, self.continuous_coords, self._structured_cache, self.X, self.y = old
        if len(y_new) == 0:
            return self
        n_old = len(self.model.y)
        try:
            self.engine.append(X_new, y_new)
        except np.linalg.LinAlgError:
            # the grown covariance is not positive definite at the MAP: back to the fitted state, and say so
            self.engine.truncate(n_old)
            self.engine.factorize()
            raise
        self.model.X = np.vstack([self.model.X, X_new])
        self.model.y = np.concatenate([self.model.y, y_new])
        self.data = DataSet(pd.concat([pd.DataFrame(self.data.data), wide], ignore_index=True), **self.data.specs)
        self.continuous_levels, self.continuous_coords = levels, coords
        self._structured_cache = None
        for slot in ("grid_vectors", "grid_parray", "grid_points", "ticks", "predictions", "predictions_X"):
            setattr(self, slot, None)
        self.X, self.y = self.get_structured_data("mean")
        if refit:
            self.find_MAP(start=self.MAP)
        return self

    # -- joint posterior: covariance and draws ---------------------------------------------------------------------------------
    def _joint_engine(self, additive_level, what):
        """The engine of a joint-posterior call and the term selection of ``additive_level`` (:meth:`_level_terms`)."""
        terms = self._level_terms(additive_level)
        if self.MAP is None or self.engine is None:
            raise ValueError("The model must be fit (find_MAP) before predicting")
        if self.distributed:
            raise NotImplementedError(f"{what}: the joint posterior is not built for distributed GPs (the factor is spread over ranks)")
        if isinstance(self.engine, icm.IcmEngine):
            raise NotImplementedError(f"{what}: the joint posterior is not built for the Kronecker path (pass kronecker=False)")
        return self.engine, terms

    def predict_joint(self, points_array, with_noise=True, additive_level="total"):
        """Posterior mean (M) and full M x M covariance at standardized points, in standardized units
        (``pm.gp.Marginal._build_conditional(..., diag=False)``): one call into ``gmb_predict_joint`` against the factor
        left resident by :meth:`find_MAP`.  No jitter is added; the diagonal is :meth:`predict`'s variance."""
        engine, terms = self._joint_engine(additive_level, "predict_joint")
        return engine.predict_joint(np.asarray(points_array, dtype=np.float64), with_noise=with_noise, jitter=0.0, **terms)

    def draw_point_samples(self, points, *args, source=None, output=None, var_name="posterior_samples", additive_level="total",
                           increment_var=True, n_draws=1, with_noise=False, rng=None, z=None, **kwargs):
        """Draw ``n_draws`` correlated samples of the fitted posterior at ``points`` (reference :861-922): a parray of shape
        ``(n_draws, M)`` in standardized units, also left in :attr:`predictions` (with ``points`` in :attr:`predictions_X`).

        The normals behind the draws are ``z`` (``(n_draws, M)``) if given, else drawn from ``rng``, else from a
        ``np.random.default_rng(self.seed)`` generator kept on the GP: successive calls differ, a fresh GP with the same seed
        repeats them.  A draw is ``mean + L* z`` with ``L*`` the Cholesky factor of the joint posterior covariance
        (``gmb_draw_joint``), so it is reproducible from ``z`` alone.

        Jitter convention implemented: the reference calls ``conditional(var_name, points_array)`` with PyMC's defaults,
        i.e. noise-free draws whose covariance PyMC 5 stabilises with its default jitter -- the model's ``jitter`` (1e-6) is
        added for ``with_noise=False``; with ``with_noise=True`` (``pred_noise=True``) PyMC adds none and neither do we.

        ``source`` / ``var_name`` / ``increment_var`` exist for signature compatibility: draws come from the stored MAP, and
        any other ``source`` raises."""
        output = self._parse_prediction_output(output)
        if len(output) > 1:
            raise NotImplementedError("Drawing correlated samples of multiple outputs is not yet implemented.")
        if args or kwargs:
            raise TypeError(f"draw_point_samples: unsupported arguments {args} {sorted(kwargs)} (PyMC sampling options have no meaning here)")
        points_array, tall_points, param_coords = self._prepare_points_for_prediction(points, output=output)
        if self.MAP is None or self.engine is None:
            raise ValueError('"Source" of predictions must be supplied if GP object has no trace or MAP stored.')
        if not (source is None or source is self.MAP or
                (isinstance(source, (list, tuple)) and len(source) == 1 and source[0] is self.MAP)):
            raise NotImplementedError("draw_point_samples draws from the stored MAP only; `source` must be None or that MAP")
        engine, terms = self._joint_engine(additive_level, "draw_point_samples")

        M = points_array.shape[0]
        if z is None:
            if rng is None:
                if self._draw_rng is None:
                    self._draw_rng = np.random.default_rng(self.seed)
                rng = self._draw_rng
            z = rng.standard_normal((int(n_draws), M))
        else:
            z = np.asarray(z, dtype=np.float64)
            if z.shape != (int(n_draws), M):
                raise ValueError(f"z must have shape (n_draws, M) = ({int(n_draws)}, {M}), got {z.shape}")
        jitter = 0.0 if with_noise else float(self.model.spec.jitter)
        samples = engine.draw_joint(points_array, z, with_noise=with_noise, jitter=jitter, **terms)

        self.predictions = self.parray(**{output[0]: samples}, stdzd=True)
        self.predictions_X = points
        return self.predictions

    # -- the components of an additive model ------------------------------------------------------------------------------------
    def decompose_points(self, points, output=None):
        """Every additive level at a 1-D parray of points, from ONE pass of the engine (``gmb_predict_decompose``):
        ``{level: uparray}`` for ``"total"`` and each level of :attr:`additive_levels`, for one output.  The values are the
        LATENT components (no noise): level t has mean ``mu_t`` and variance ``cov_tt``; ``"total"`` is their sum,
        ``sum_t mu_t`` and ``sum_tu cov_tu`` -- :meth:`predict_points` with ``with_noise=False``.  The standardized pointwise
        covariance BETWEEN the components, ``(T, T, M)``, stays in :attr:`component_cov` with :attr:`component_levels` naming
        its axes: a strongly negative off-diagonal says the data cannot tell two components apart."""
        output = self._parse_prediction_output(output)
        if len(output) > 1:
            raise NotImplementedError("Decomposing multiple outputs at once is not yet implemented.")
        points_array, _, _ = self._prepare_points_for_prediction(points, output=output)
        engine, _ = self._joint_engine("total", "decompose_points")
        means, cov, _ = engine.predict_decompose(points_array)
        by_bit = {mask: level for level, mask in self.additive_levels.items() if level != "total" or len(self.additive_levels) == 1}
        self.component_levels = [by_bit[1 << t] for t in range(means.shape[0])]
        self.component_cov = cov
        parts = {"total": self.uparray(output[0], means.sum(axis=0), cov.sum(axis=(0, 1)), stdzd=True)}
        if len(self.additive_levels) > 1:
            for t, level in enumerate(self.component_levels):
                parts[level] = self.uparray(output[0], means[t], cov[t, t], stdzd=True)
        self.predictions_X = points
        return parts

    # -- leave-one-out and leave-group-out predictions of the training rows -----------------------------------------------------
    def _leave_out_engine(self, what):
        if self.MAP is None or self.engine is None:
            raise ValueError(f"{what}: the model must be fit (find_MAP) first")
        if self.distributed:
            raise NotImplementedError(f"{what}: leave-out predictions are not built for distributed GPs (the factor is spread over ranks)")
        if isinstance(self.engine, icm.IcmEngine):
            raise NotImplementedError(f"{what}: leave-out predictions are not built for the Kronecker path (pass kronecker=False)")
        return self.engine

    def _output_rows(self):
        """``{output name: engine rows}``: the rows of ``model.X`` / ``model.y`` that belong to each output."""
        n = len(self.model.y)
        if self.out_col not in self.dims:
            return {self.outputs[0]: np.arange(n)}
        oc = self.dims.index(self.out_col)
        col = np.asarray(self.model.X, float)[:, oc]
        ordered = [name for name, _ in sorted(self.coords[self.out_col].items(), key=lambda kv: kv[1])]
        coords = np.unique(col)
        if len(coords) != len(ordered):
            raise ValueError(f"the output column holds {len(coords)} levels, the model has {len(ordered)} outputs")
        return {name: np.flatnonzero(col == c) for name, c in zip(ordered, coords)}

    def _unit_rows(self, unit):
        """The value of column ``unit`` of the table at every engine row (the order of :meth:`_shaped_rows`: a stacked table's
        outputs one after the other, rows without an observation dropped)."""
        df = self.get_filtered_data(standardized=False, metric="mean")
        if unit not in df.columns:
            raise ValueError(f'leave_group_out: "{unit}" is not a column of the data')
        names = df[self.out_col].to_numpy()
        values = df[self.data.values_column if self.data.values_column in df.columns else "Value"].to_numpy()
        if self.out_col in self.dims:
            ordered = [name for name, _ in sorted(self.coords[self.out_col].items(), key=lambda kv: kv[1])]
        else:
            ordered = [self.outputs[0]]
        col = df[unit].to_numpy()
        labels = np.concatenate([col[names == out] for out in ordered])
        seen = np.concatenate([np.asarray(values[names == out], dtype=np.float64) for out in ordered])
        labels = labels[~np.isnan(seen)]
        _, y_table = self._shaped_rows()
        if len(labels) != len(self.model.y) or not np.array_equal(y_table, np.asarray(self.model.y, float)):
            raise ValueError("leave_group_out(unit=...): the engine's rows are no longer in the table's order (observations were "
                             "appended to a stacked table); fit again, or name the rows with `groups`")
        return labels

    @staticmethod
    def _gaussian_nlpd(resid, var):
        return 0.5 * (np.log(2.0 * np.pi * var) + resid ** 2 / var)

    def leave_one_out(self, with_noise=True):
        """What the fitted model predicts for each observation from all the OTHERS, at the fitted hyper-parameters and without a
        refit (``gmb_loo``; Rasmussen & Williams 5.4.2): a dict, everything standardized and in the engine's row order
        (``model.X`` / ``model.y``) --

        ``"mean"``, ``"var"`` (N each); ``"z_score"`` ``(y - mean) / sqrt(var)``; ``"nlpd"`` the Gaussian negative log predictive
        density of each held-out observation; ``"predictions"`` ``{output name: uparray}`` of that output's rows.

        With ``with_noise=True`` (the default, what a held-out MEASUREMENT is judged against) the variances are those of
        :meth:`predict` with noise on the data without the row; ``with_noise=False`` gives the latent function's.  Behind
        :meth:`find_MAP` this is one pass over the inverse factor the fit left on the device."""
        engine = self._leave_out_engine("leave_one_out")
        mean, var = engine.loo(with_noise=with_noise)
        y = np.asarray(self.model.y, dtype=np.float64)
        resid = y - mean
        return {
            "mean": mean,
            "var": var,
            "z_score": resid / np.sqrt(var),
            "nlpd": self._gaussian_nlpd(resid, var),
            "predictions": {name: self.uparray(name, mean[rows], var[rows], stdzd=True) for name, rows in self._output_rows().items()},
        }

    def leave_group_out(self, unit=None, groups=None, n_folds=None, seed=None, with_noise=True, joint=False):
        """The JOINT prediction of each group of observations from all the others, at the fitted hyper-parameters and without a
        refit (``gmb_leave_out``, one engine call per group).  Exactly one of

        * ``unit``: a column of ``gp.data.wide`` -- rows sharing a value leave together, every output of a stacked table included
          (the meaning of ``cross_validate(unit=...)``);
        * ``groups``: a list of index arrays into the engine's rows (``model.X`` / ``model.y``);
        * ``n_folds``: a random partition from ``np.random.default_rng(seed or self.seed)``.

        Returns a list of dicts, one per group, standardized: ``"rows"``, ``"mean"``, ``"var"``, ``"nlpd"`` (per row), for ``unit``
        also ``"unit"``; with ``joint=True`` also ``"cov"`` (m x m) and ``"nlpd"`` is the joint Gaussian negative log density of
        the group's observations."""
        engine = self._leave_out_engine("leave_group_out")
        if sum(a is not None for a in (unit, groups, n_folds)) != 1:
            raise ValueError("leave_group_out: give exactly one of `unit`, `groups` and `n_folds`")
        n = len(self.model.y)
        labels = None
        if unit is not None:
            if not isinstance(unit, str):
                raise TypeError('Keyword "unit" must be a single string.')
            col = self._unit_rows(unit)
            labels = list(pd.unique(col))
            parts = [np.flatnonzero(col == value) for value in labels]
        elif groups is not None:
            parts = [np.asarray(g, dtype=np.int64).ravel() for g in groups]
        else:
            n_folds = int(n_folds)
            if not 1 <= n_folds <= n:
                raise ValueError(f"leave_group_out: n_folds must be in [1, {n}], got {n_folds}")
            perm = np.random.default_rng(seed or self.seed).permutation(n)
            parts = [np.sort(part) for part in np.array_split(perm, n_folds)]
        y = np.asarray(self.model.y, dtype=np.float64)
        out = []
        for k, rows in enumerate(parts):
            res = engine.leave_out(rows, with_noise=with_noise, cov=joint)
            mean, var = res[0], res[1]
            resid = y[rows] - mean
            entry = {"rows": rows, "mean": mean, "var": var}
            if joint:
                cov = res[2]
                chol = np.linalg.cholesky(cov)
                white = np.linalg.solve(chol, resid)
                entry["cov"] = cov
                entry["nlpd"] = float(0.5 * (white @ white) + np.log(np.diag(chol)).sum() + 0.5 * len(rows) * np.log(2.0 * np.pi))
            else:
                entry["nlpd"] = self._gaussian_nlpd(resid, var)
            if labels is not None:
                entry["unit"] = labels[k]
            out.append(entry)
        return out

    # -- averages of the posterior over groups of points: marginal effects and contrasts ------------------------------------------
    def predict_groups(self, points_array, offsets, weights=None, cov=False, additive_level="total"):
        """Weighted averages of the LATENT posterior over groups of standardized points, in standardized units: ``(mean, var)``,
        or ``(mean, var, cov)`` with ``cov=True`` -- one call into ``gmb_predict_groups`` against the factor left resident by
        :meth:`find_MAP`.  Group g is the rows ``offsets[g]:offsets[g + 1]`` of ``points_array``; ``weights`` of any sign, ``None``
        for the plain mean of each group.  The variance of an average is ``w^T C w`` with C the joint posterior covariance of the
        group's points, NOT the mean of their variances; nothing of size M x M is formed to get it.

        Averages are taken on the model's own standardized, transformed scale, like everything the GP computes: for a
        log-normal output the natural-scale reading of an average is therefore a GEOMETRIC mean."""
        terms = self._level_terms(additive_level)
        if self.MAP is None or self.engine is None:
            raise ValueError("The model must be fit (find_MAP) before predicting")
        if self.distributed:
            raise NotImplementedError("predict_groups: group averages are not built for distributed GPs (the factor is spread over ranks)")
        if isinstance(self.engine, icm.IcmEngine):
            raise NotImplementedError("predict_groups: group averages are not built for the Kronecker path (pass kronecker=False)")
        return self.engine.predict_groups(np.asarray(points_array, dtype=np.float64), offsets, weights=weights, cov=cov, **terms)

    def _one_output(self, output, what):
        outputs = self._parse_prediction_output(output)
        if len(outputs) != 1:
            raise ValueError(f"{what} averages ONE output: pass output= one of {outputs}")
        return outputs

    def predict_average(self, points, groups=None, weights=None, output=None, joint=False, additive_level="total"):
        """The posterior of the weighted mean of the latent function over groups of ``points`` (a 1-D parray): a uparray of
        length G, one entry per distinct label of ``groups`` (an integer per point; ``None``: all points are one group) in
        ascending label order; with ``joint=True`` ``(uparray, cov)``, ``cov`` the standardized G x G covariance between the
        averages.  ``weights`` (one per point, any sign) default to ``1 / |g|``.  The points are sorted stably by label, so
        points of one label keep their order.

        Averages are taken on the model's standardized, transformed scale: for a log-normal output the natural-scale value
        of the returned uparray is a geometric mean."""
        self._level_terms(additive_level)
        outputs = self._one_output(output, "predict_average")
        points_array, _, _ = self._prepare_points_for_prediction(points, output=outputs)
        M = points_array.shape[0]
        labels = np.zeros(M, dtype=np.int64) if groups is None else np.asarray(groups).ravel()
        if labels.shape[0] != M or not np.issubdtype(labels.dtype, np.integer):
            raise ValueError(f"predict_average: `groups` must hold one integer label per point ({M}), got {labels.shape[0]} of dtype {labels.dtype}")
        order = np.argsort(labels, kind="stable")
        uniq, counts = np.unique(labels, return_counts=True)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        w = None
        if weights is not None:
            w = np.asarray(weights, dtype=np.float64).ravel()
            if w.shape[0] != M:
                raise ValueError(f"predict_average: {w.shape[0]} weights for {M} points")
            w = w[order]
        res = self.predict_groups(points_array[order], offsets, weights=w, cov=joint, additive_level=additive_level)
        self.average_labels = uniq
        avg = self.uparray(outputs[0], res[0], res[1], stdzd=True)
        return (avg, res[2]) if joint else avg

    def _background_rows(self, what, over, outputs, n_background, seed, categorical_levels, overwritten):
        """``(B, D)`` standardized model rows to average over: the fitted table's rows of the output (``over="data"``), a seeded
        random subset of ``n_background`` of them, or the points of a parray.  ``overwritten``: dims the caller sets afterwards
        (a parray need not carry them)."""
        if isinstance(over, str):
            if over != "data":
                raise ValueError(f'{what}: `over` must be "data" or a parray of background points, got {over!r}')
            rows = np.asarray(self.model.X, dtype=np.float64)[self._output_rows()[outputs[0]]].copy()
            for dim, level in (categorical_levels or {}).items():
                if dim not in self.categorical_dims or dim == self.out_col:
                    raise ValueError(f'{what}: "{dim}" is not a categorical dimension of the model')
                rows[:, self.dims.index(dim)] = self.stdzr.stdz(dim, float(self.categorical_coords[dim][level]))
        else:
            pts = np.atleast_1d(over)
            fill = {dim: np.zeros(pts.shape) for dim in overwritten if dim not in pts.names}
            if fill:
                pts = pts.add_layers(stdzd=True, **fill)
            if set(self.categorical_dims) - {self.out_col} - set(pts.names):
                if categorical_levels is None:
                    raise AttributeError("Must specify level for every categorical dimension")
                pts = self.append_categorical_points(pts, {d: l for d, l in categorical_levels.items() if d not in pts.names})
            rows, _, _ = self._prepare_points_for_prediction(pts, output=outputs)
            rows = np.asarray(rows, dtype=np.float64)
        if n_background is not None:
            n_background = int(n_background)
            if not 1 <= n_background <= len(rows):
                raise ValueError(f"{what}: n_background must be in [1, {len(rows)}], got {n_background}")
            rng = np.random.default_rng(self.seed if seed is None else seed)
            rows = rows[np.sort(rng.choice(len(rows), n_background, replace=False))]
        return rows

    def marginal_design(self, dims, limits=None, resolution=50, over="data", n_background=None, seed=None, categorical_levels=None,
                        output=None):
        """What :meth:`predict_marginal` averages: a dict with ``"grid"`` (the parray of grid values, shaped like the grid),
        ``"points_array"`` (G B standardized model rows: for every grid value, in the grid's row-major order, the B background
        rows with ``dims`` overwritten), ``"offsets"`` (group g = grid value g) and ``"weights"`` (1 / B)."""
        what = "predict_marginal"
        dims = [dims] if isinstance(dims, str) else list(dims)
        if not 1 <= len(dims) <= 2 or len(set(dims)) != len(dims) or any(d not in self.continuous_dims for d in dims):
            raise ValueError(f"{what}: `dims` must be one or two of the continuous dimensions {list(self.continuous_dims)}, got {dims}")
        outputs = self._one_output(output, what)
        back = self._background_rows(what, over, outputs, n_background, seed, categorical_levels, dims)
        defaults = self._default_grid_limits(set(dims))
        if limits is None:
            limits = defaults
        else:
            missing = set(dims) - set(limits.names)
            if missing:
                limits = limits.add_layers(**defaults[list(missing)].as_dict())
        per_dim = self._grid_resolution(resolution)
        order = [d for d in self.dims if d in dims]  # grid axes follow the model's dimension order
        lz = limits.z
        axes = [np.linspace(*lz[d + "_z"].values(), per_dim[d]) for d in order]
        mesh = np.meshgrid(*axes, indexing="ij")
        grid = self.parray(**{d: m for d, m in zip(order, mesh)}, stdzd=True)
        G, B = mesh[0].size, back.shape[0]
        points_array = np.tile(back, (G, 1))
        for d, m in zip(order, mesh):
            points_array[:, self.dims.index(d)] = np.repeat(m.ravel(), B)
        return {"grid": grid, "points_array": points_array, "offsets": np.arange(G + 1, dtype=np.int64) * B,
                "weights": np.full(G * B, 1.0 / B), "output": outputs[0]}

    def predict_marginal(self, dims, limits=None, resolution=50, over="data", n_background=None, seed=None, categorical_levels=None,
                         output=None, joint=False, additive_level="total"):
        """The marginal effect of one or two continuous dimensions: for every value (or pair) of a regular grid over ``dims``,
        the posterior of the latent function AVERAGED over a background of points -- the background's other coordinates with
        ``dims`` overwritten, every background row weighing ``1 / B``.  Returns a uparray shaped like the grid.

        ``over``: ``"data"`` (the fitted table's rows of the output, with their own categorical coordinates unless
        ``categorical_levels`` pins some), or a 1-D parray of background points; ``n_background`` + ``seed`` take a seeded random
        subset of the background.  ``limits`` (a parray with two values per dim) default to those :meth:`prepare_grid` would
        take; ``resolution`` an int or a dict per dim.  The grid is left in :attr:`marginal_points`; with ``joint=True`` the
        standardized G x G covariance between the grid values' averages (row-major over the grid) is left in
        :attr:`marginal_cov`.  The variance of each average is that of the MEAN of the latent function over the background
        (``w^T C w``), which is not the mean of the pointwise variances.

        Averages are taken on the model's standardized, transformed scale: for a log-normal output the natural-scale reading
        of a marginal effect is a geometric mean over the background."""
        self._level_terms(additive_level)
        design = self.marginal_design(dims, limits=limits, resolution=resolution, over=over, n_background=n_background, seed=seed,
                                      categorical_levels=categorical_levels, output=output)
        res = self.predict_groups(design["points_array"], design["offsets"], weights=design["weights"], cov=joint,
                                  additive_level=additive_level)
        shape = design["grid"].shape
        self.marginal_points = design["grid"]
        self.marginal_cov = res[2] if joint else None
        return self.uparray(design["output"], res[0].reshape(shape), res[1].reshape(shape), stdzd=True)

    def compare_levels(self, dim, a, b, over="data", n_background=None, seed=None, categorical_levels=None, output=None,
                       additive_level="total"):
        """Is level ``a`` of the categorical dimension ``dim`` different from level ``b``, averaged over a background?  ONE group
        of 2 B points -- the background at level ``a`` with weights ``+1 / B``, at level ``b`` with ``-1 / B`` -- so the variance
        holds the posterior covariance BETWEEN the two levels' averages.  Returns a dict, standardized: ``"mean"`` (the
        difference a - b of the averages), ``"var"``, ``"z_score"`` ``= mean / sqrt(var)``, ``"levels"`` ``(a, b)`` and
        ``"n_background"``.  ``over`` / ``n_background`` / ``seed`` / ``categorical_levels`` as :meth:`predict_marginal`.

        The difference is taken on the model's standardized, transformed scale: for a log-normal output it is a log RATIO of
        geometric means, in units of the output's standard deviation."""
        what = "compare_levels"
        self._level_terms(additive_level)
        if dim not in self.categorical_dims or dim == self.out_col:
            raise ValueError(f'{what}: "{dim}" is not a categorical dimension of the model')
        for level in (a, b):
            if level not in self.categorical_coords[dim]:
                raise ValueError(f'{what}: "{level}" is not a level of "{dim}" ({list(self.categorical_coords[dim])})')
        outputs = self._one_output(output, what)
        if not isinstance(over, str) and dim not in np.atleast_1d(over).names:
            over = np.atleast_1d(over).fill_with(**{dim: self.categorical_coords[dim][a]})
        back = self._background_rows(what, over, outputs, n_background, seed, categorical_levels, [])
        B, col = back.shape[0], self.dims.index(dim)
        points_array = np.tile(back, (2, 1))
        points_array[:B, col] = self.stdzr.stdz(dim, float(self.categorical_coords[dim][a]))
        points_array[B:, col] = self.stdzr.stdz(dim, float(self.categorical_coords[dim][b]))
        weights = np.concatenate([np.full(B, 1.0 / B), np.full(B, -1.0 / B)])
        mean, var = self.predict_groups(points_array, np.array([0, 2 * B], dtype=np.int64), weights=weights, additive_level=additive_level)
        with np.errstate(invalid="ignore", divide="ignore"):  # (a level against itself: the variance is rounding noise around 0)
            z_score = float(mean[0] / np.sqrt(var[0]))
        return {"mean": float(mean[0]), "var": float(var[0]), "z_score": z_score, "levels": (a, b), "n_background": B}

    # -- a batch of experiments by integrated variance reduction ---------------------------------------------------------------
    def _design_points(self, what, candidates, reference, n_candidates, n_reference, bounds, categorical_levels, output, seed):
        """The standardized continuous coordinates of the candidates and the reference points of :meth:`design_batch`
        (``(M, n_cont)``, ``(R, n_cont)``; each given as a parray or such an array, or drawn: seeded quasi-random points inside
        ``bounds``, default the data's limits), the continuous dims, and ``full(Z)``, which completes them to model points."""
        if self.distributed:
            raise NotImplementedError(f"{what}: the rectangular posterior covariance is built on the single-device engine only "
                                      "(the factor of a distributed GP is spread over ranks)")
        if isinstance(self.engine, icm.IcmEngine):
            raise NotImplementedError(f"{what}: the rectangular posterior covariance is built on the single-device engine only, "
                                      "not for the Kronecker path (pass kronecker=False)")
        _, cont, cols, full = self._acquisition_problem(output, "UCB", True, categorical_levels, None)
        if bounds is None:
            Xd = np.asarray(self.model.X, float)[:, cols]
            lo, hi = Xd.min(axis=0), Xd.max(axis=0)
        else:
            both = np.array([np.asarray(bounds.z[d + "_z"].values(), float).ravel() for d in cont])
            if both.shape != (len(cont), 2):
                raise ValueError("bounds must hold two entries (lower, upper) per continuous dimension")
            lo, hi = both.min(axis=1), both.max(axis=1)
        seed = self.seed if seed is None else seed

        def drawn(n, stream):
            try:
                from scipy.stats import qmc

                with warnings.catch_warnings():  # (a Sobol' sample whose size is no power of two: still a fine design)
                    warnings.simplefilter("ignore", UserWarning)
                    u = qmc.Sobol(len(cont), seed=np.random.default_rng([seed, stream])).random(int(n))
            except ImportError:
                u = np.random.default_rng([seed, stream]).uniform(size=(int(n), len(cont)))
            return lo + (hi - lo) * u

        def given(points, name):
            if hasattr(points, "z"):
                Z = np.column_stack([np.asarray(points.z[d + "_z"].values(), float).ravel() for d in cont])
            else:
                Z = np.asarray(points, float).reshape(-1, len(cont))
            if len(Z) < 1:
                raise ValueError(f"{what}: {name} holds no point")
            return Z

        Zc = drawn(n_candidates, 0) if candidates is None else given(candidates, "candidates")
        Zr = drawn(n_reference, 1) if reference is None else given(reference, "reference")
        return Zc, Zr, cont, full

    def design_batch(self, q, candidates=None, reference=None, n_candidates=1024, n_reference=4096, bounds=None,
                     categorical_levels=None, output=None, weights=None, allow_repeats=True, with_noise=True, seed=None):
        """Which ``q`` conditions to run next to learn the surface as a whole: a greedy batch by integrated variance reduction
        (IVR, also called ALC), one call into ``gmb_design_batch`` against the factor :meth:`find_MAP` left resident.

        Measuring at a candidate c lowers the latent variance at every point r by ``cov(c, r)^2 / (var f(c) + noise(c))`` -- in
        closed form, whatever will be observed, so no value is fantasised (unlike ``propose_continuous(sequential=True)``,
        which optimises an acquisition of the mean).  The score of a candidate is that reduction summed over the ``reference``
        points with ``weights`` (default ``1 / R`` each), which stand for the region of interest; each pick conditions the
        posterior before the next.  ``candidates`` and ``reference``: parrays, or ``(n, n_cont)`` arrays of standardized
        continuous coordinates in ``continuous_dims`` order; default ``n_candidates`` / ``n_reference`` seeded quasi-random
        points inside ``bounds`` (a parray with two entries per continuous dimension; default the data's limits).
        Categorical coordinates are fixed through ``categorical_levels`` and ``output`` names the output, as in
        :meth:`propose_continuous`.  With ``with_noise`` (a measurement carries the model's noise) and ``allow_repeats`` a
        candidate may be picked again: a replicate, where it teaches more than a new condition.

        Returns the picked points as a parray in pick order, repeats included (fewer than ``q`` once no candidate lowers the
        variance any further), and sets :attr:`design_picks` (candidate indices), :attr:`design_gains` (the variance each pick
        removes), :attr:`design_ivar0` (the weighted variance over the reference points before any pick: ``gains / ivar0`` are
        fractions), :attr:`design_scores` (the step-0 score of every candidate) and :attr:`design_candidates` (the candidates,
        a parray).  Covers one-term and additive models as a whole; not the Kronecker or distributed paths."""
        q = int(q)
        if q < 0:
            raise ValueError(f"q must be >= 0, got {q}")
        Zc, Zr, cont, full = self._design_points("design_batch", candidates, reference, n_candidates, n_reference, bounds,
                                                 categorical_levels, output, seed)
        picks, gains, scores, ivar0 = self.engine.design_batch(full(Zc), full(Zr), q, weights=weights, with_noise=with_noise,
                                                               allow_repeats=allow_repeats)
        picks = np.asarray(picks, dtype=np.int64)
        self.design_picks, self.design_gains, self.design_ivar0, self.design_scores = picks, np.asarray(gains, float), float(ivar0), scores
        self.design_candidates = self.parray(**{d: Zc[:, k] for k, d in enumerate(cont)}, stdzd=True)
        chosen = Zc[picks[picks >= 0]]
        return self.parray(**{d: chosen[:, k] for k, d in enumerate(cont)}, stdzd=True)

    def variance_reduction(self, candidates, reference, bounds=None, categorical_levels=None, output=None, weights=None,
                           with_noise=True):
        """The integrated variance reduction of every candidate on its own -- :meth:`design_batch`'s step-0 score, its ``q = 0``
        form: how much one measurement there would lower the weighted latent variance over ``reference``.  Returns the scores
        (one per candidate) and sets :attr:`design_ivar0`."""
        Zc, Zr, _, full = self._design_points("variance_reduction", candidates, reference, 0, 0, bounds, categorical_levels, output, None)
        _, _, scores, ivar0 = self.engine.design_batch(full(Zc), full(Zr), 0, weights=weights, with_noise=with_noise, allow_repeats=True)
        self.design_ivar0 = float(ivar0)
        return scores

    def decompose_grid(self, output=None, categorical_levels=None):
        """:meth:`decompose_points` on the grid :meth:`prepare_grid` left behind, every level in the grid's shape."""
        if self.grid_points is None:
            raise ValueError("Grid must first be specified with `prepare_grid`")
        points = self.grid_points
        if self.categorical_dims:
            points = self.append_categorical_points(points, categorical_levels=categorical_levels)
        shape = self.grid_parray.shape
        parts = {level: up.reshape(shape) for level, up in self.decompose_points(points, output=output).items()}
        self.predictions_X = self.predictions_X.reshape(shape)
        return parts

    def draw_grid_samples(self, *args, source=None, output=None, categorical_levels=None, var_name="posterior_samples",
                          additive_level="total", increment_var=True, n_draws=1, with_noise=False, rng=None, z=None, **kwargs):
        """Draw posterior samples at the points :meth:`prepare_grid` defined (reference :924-979): a parray of shape
        ``(n_draws, *grid shape)``; see :meth:`draw_point_samples` for the arguments."""
        if self.grid_points is None:
            raise ValueError("Grid must first be specified with `prepare_grid`")
        points = self.grid_points
        if self.categorical_dims:
            points = self.append_categorical_points(points, categorical_levels=categorical_levels)
        samples = self.draw_point_samples(points, *args, source=source, output=output, var_name=var_name,
                                          additive_level=additive_level, increment_var=increment_var, n_draws=n_draws,
                                          with_noise=with_noise, rng=rng, z=z, **kwargs)
        self.predictions = samples.reshape(-1, *self.grid_parray.shape)
        self.predictions_X = self.predictions_X.reshape(self.grid_parray.shape)
        return self.predictions
