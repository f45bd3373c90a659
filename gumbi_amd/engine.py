"""ctypes binding of ``libgumbi_hip.so`` (C ABI in ``include/gumbi_hip.h``).

This is the only door between the Python front end and the numerics: there is no Python / numpy
implementation of the covariance build, the Cholesky factorisation or the posterior solves in
this package.  If the shared library is missing or no HIP device is present every call raises --
the product path never falls back to the CPU.
"""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

__all__ = ["Engine", "KernelSpec", "GumbiHipError", "library_path", "load_library", "KERNEL_KINDS", "resolve_kernel_name",
           "PERIODIC_OFF", "PERIODIC_WARPED", "PERIODIC_PLAIN", "MAX_PERIODIC_DIMS",
           "ls_limits", "dist_plan", "GmbComm", "DistStep"]

GMB_MAX_DIMS, GMB_MAX_LIN, GMB_MAX_COREG, GMB_MAX_LEVELS = 16, 8, 4, 32
GMB_OK, GMB_EINVAL, GMB_ENOMEM, GMB_EHIP, GMB_ENOTPD, GMB_ENODEVICE, GMB_ENOCONV = 0, -1, -2, -3, -4, -5, -6
GMB_HOST, GMB_DEVICE = 0, 1

# pm.gp.cov names accepted by PymcGP._construct_kernels (gumbi/regression/pymc/GP.py:664-674)
KERNEL_KINDS = {"ExpQuad": 0, "Matern52": 1, "Matern32": 2, "Matern12": 3, "Exponential": 4}


#: ``gmb_set_periodic`` modes
PERIODIC_OFF, PERIODIC_WARPED, PERIODIC_PLAIN = 0, 1, 2
#: largest number of continuous dimensions of a periodic model (two prepared columns each)
MAX_PERIODIC_DIMS = GMB_MAX_DIMS // 2


def resolve_kernel_name(name: str):
    """``continuous_kernel`` of the front end -> ``(stationary kind, periodic mode)``: ``"Matern52"`` -> ``("Matern52", 0)``,
    ``"Matern52+Periodic"`` -> ``("Matern52", 1)``, ``"Periodic"`` -> ``("ExpQuad", 2)`` (pm.gp.cov.Periodic is the
    exponentiated quadratic of the half-scaled warped inputs)."""
    if name == "Periodic":
        return "ExpQuad", PERIODIC_PLAIN
    if isinstance(name, str) and name.endswith("+Periodic") and name[: -len("+Periodic")] in KERNEL_KINDS:
        return name[: -len("+Periodic")], PERIODIC_WARPED
    if name in KERNEL_KINDS:
        return name, PERIODIC_OFF
    raise ValueError(f"Continuous kernel must be one of {list(KERNEL_KINDS)}, optionally with '+Periodic', or 'Periodic'; got {name!r}")


class LaplaceConvergenceError(RuntimeError):
    """``gmb_laplace_evaluate`` hit one of its caps (``GMB_ENOCONV``): 40 Newton iterations, or 20 halvings of one step."""


class GumbiHipError(RuntimeError):
    """A libgumbi_hip call failed (bad HIP state, missing device, out of memory ...)."""


class _Spec(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("ard", C.c_int32),
        ("n_cont", C.c_int32),
        ("idx_cont", C.c_int32 * GMB_MAX_DIMS),
        ("n_lin", C.c_int32),
        ("idx_lin", C.c_int32 * GMB_MAX_LIN),
        ("n_coreg", C.c_int32),
        ("coreg_col", C.c_int32 * GMB_MAX_COREG),
        ("coreg_levels", C.c_int32 * GMB_MAX_COREG),
        ("out_col", C.c_int32),
        ("n_out", C.c_int32),
        ("hetero_noise", C.c_int32),
        ("additive", C.c_int32),
        ("jitter", C.c_double),
    ]


class Timings(C.Structure):
    _fields_ = [
        ("kbuild_ms", C.c_double),
        ("chol_ms", C.c_double),
        ("chol_gemm_ms", C.c_double),
        ("chol_gemm_flops", C.c_double),
        ("chol_gemm_launches", C.c_int64),
        ("chol_leaf_ms", C.c_double),
        ("chol_trsm_ms", C.c_double),
        ("predict_ms", C.c_double),
        ("predict_gemm_ms", C.c_double),
        ("predict_gemm_flops", C.c_double),
        ("predict_gemm_launches", C.c_int64),
        ("grad_ms", C.c_double),
        ("grad_gemm_ms", C.c_double),
        ("grad_gemm_flops", C.c_double),
        ("kbuild_bytes", C.c_double),
        ("total_gemm_ms", C.c_double),
        ("total_gemm_flops", C.c_double),
        ("total_gemm_launches", C.c_int64),
        ("total_kbuild_ms", C.c_double),
        ("total_kbuild_bytes", C.c_double),
        ("total_kbuild_launches", C.c_int64),
        ("masked_gemm_ms", C.c_double),
        ("masked_gemm_flops", C.c_double),
        ("masked_cus", C.c_int64),
        ("total_gemm_wall_ms", C.c_double),
        ("total_chol_gemm_ms", C.c_double),
        ("total_chol_gemm_flops", C.c_double),
        ("total_chol_gemm_launches", C.c_int64),
        ("total_chol_gemm_wall_ms", C.c_double),
        ("total_chol_panel_gemm_ms", C.c_double),
        ("total_chol_panel_gemm_flops", C.c_double),
        # multi-GPU driver: communication probes of the last gmb_dist_factorize / gmb_dist_nlml (this rank)
        ("dist_world", C.c_int64),
        ("dist_chol_collectives", C.c_int64),
        ("dist_chol_comm_bytes", C.c_double),
        ("dist_chol_comm_ms", C.c_double),
        ("dist_chol_comm_exposed_ms", C.c_double),
        ("dist_chol_main_wait_ms", C.c_double),
        ("dist_chol_bulk_wait_ms", C.c_double),
        ("dist_grad_collectives", C.c_int64),
        ("dist_grad_comm_bytes", C.c_double),
        ("dist_grad_comm_ms", C.c_double),
        ("dist_grad_comm_exposed_ms", C.c_double),
        ("dist_lockstep_repairs", C.c_int64),
        ("total_chol_tile_ms", C.c_double),
        ("total_chol_tile_flops", C.c_double),
        ("total_chol_tile_launches", C.c_int64),
        ("total_eval_tile_ms", C.c_double),
        ("total_eval_tile_flops", C.c_double),
        ("total_eval_tile_launches", C.c_int64),
        # ABI 10: every launch issued AS a Cholesky trailing update (the population of ``total_chol_gemm_*`` up to round 4), and
        # which form the last prediction took
        ("total_chol_update_all_ms", C.c_double),
        ("total_chol_update_all_flops", C.c_double),
        ("total_chol_update_all_launches", C.c_int64),
        ("predict_gemm_form", C.c_int64),
        ("total_chol_panel_tile_ms", C.c_double),
        ("total_chol_panel_tile_flops", C.c_double),
        ("total_chol_panel_tile_launches", C.c_int64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


@dataclass
class KernelSpec:
    """Which columns of X feed which covariance term (mirror of ``gmb_kernel_spec``)."""

    D: int
    idx_cont: list
    kind: str | int = "ExpQuad"
    ard: bool = True
    idx_lin: list = field(default_factory=list)
    coreg: list = field(default_factory=list)  # [(column, n_levels), ...]
    out_col: int = -1
    n_out: int = 0
    hetero_noise: bool = True
    jitter: float = 1e-6
    additive: bool = False  # a global kernel + one kernel per coregion dim (specify_model(additive=True))
    #: periodic mode (``gmb_set_periodic``; not part of ``gmb_kernel_spec``): 0 off, 1 ``<kind>+Periodic``, 2 ``Periodic``
    periodic: int = 0
    #: one period per entry of idx_cont, in the units of X.  ``to_c`` checks their number only; that each is finite and
    #: positive is the engine's check (``gmb_set_periodic`` -> ``ValueError`` from ``Engine.set_kernel``)
    periods: list = field(default_factory=list)

    @property
    def kind_id(self) -> int:
        if isinstance(self.kind, str):
            if self.kind not in KERNEL_KINDS:
                raise ValueError(f"Continuous kernel must be one of {list(KERNEL_KINDS)}, got {self.kind!r}")
            return KERNEL_KINDS[self.kind]
        return int(self.kind)

    def as_dict(self) -> dict:
        return dict(D=int(self.D), kind=self.kind_id, ard=bool(self.ard),
                    idx_cont=[int(i) for i in self.idx_cont], idx_lin=[int(i) for i in self.idx_lin],
                    coreg=[(int(c), int(n)) for c, n in self.coreg], out_col=int(self.out_col),
                    n_out=int(self.n_out), hetero_noise=bool(self.hetero_noise), jitter=float(self.jitter),
                    additive=bool(self.additive), periodic=int(self.periodic), periods=[float(t) for t in self.periods])

    def theta_size(self) -> int:
        n = (len(self.idx_cont) if self.ard else 1) + 2
        if self.idx_lin:
            n += len(self.idx_lin) + 1
        n += sum(3 * L for _, L in self.coreg)
        if self.out_col >= 0:
            n += 3 * self.n_out * (2 if self.hetero_noise else 1)
        if self.additive:  # one more [ls | eta | (c, tau)] block per coregion dim
            blk = (len(self.idx_cont) if self.ard else 1) + 1 + ((len(self.idx_lin) + 1) if self.idx_lin else 0)
            n += len(self.coreg) * blk
        return n

    def to_c(self) -> _Spec:
        if not 1 <= len(self.idx_cont) <= GMB_MAX_DIMS:
            raise ValueError(f"between 1 and {GMB_MAX_DIMS} continuous dimensions are supported")
        if len(self.idx_lin) > GMB_MAX_LIN:
            raise ValueError(f"at most {GMB_MAX_LIN} linear dimensions are supported")
        if len(self.coreg) > GMB_MAX_COREG:
            raise ValueError(f"at most {GMB_MAX_COREG} categorical dimensions are supported")
        if self.periodic:  # (travels beside the struct: gmb_set_periodic)
            if self.periodic not in (PERIODIC_WARPED, PERIODIC_PLAIN):
                raise ValueError(f"periodic must be 0, 1 or 2, got {self.periodic!r}")
            if len(self.idx_cont) > MAX_PERIODIC_DIMS:
                raise ValueError(f"a periodic kernel supports at most {MAX_PERIODIC_DIMS} continuous dimensions")
            if len(self.periods) != len(self.idx_cont):
                raise ValueError(f"{len(self.periods)} periods for {len(self.idx_cont)} continuous dimensions")
        s = _Spec()
        s.kind, s.ard = self.kind_id, int(bool(self.ard))
        s.n_cont = len(self.idx_cont)
        for i, v in enumerate(self.idx_cont):
            s.idx_cont[i] = int(v)
        s.n_lin = len(self.idx_lin)
        for i, v in enumerate(self.idx_lin):
            s.idx_lin[i] = int(v)
        s.n_coreg = len(self.coreg)
        for i, (col, lev) in enumerate(self.coreg):
            s.coreg_col[i], s.coreg_levels[i] = int(col), int(lev)
        s.out_col, s.n_out = int(self.out_col), int(self.n_out)
        s.hetero_noise = int(bool(self.hetero_noise))
        s.additive = int(bool(self.additive))
        s.jitter = float(self.jitter)
        return s


# ------------------------------------------------------------------------------------------------
_LIB = None
_DBL_P = C.POINTER(C.c_double)


def library_path() -> Path:
    override = os.environ.get("GUMBI_HIP_LIB")
    if override:
        return Path(override)
    return Path(__file__).resolve().parent / "lib" / "libgumbi_hip.so"


class GmbComm(C.Structure):
    """``gmb_comm``: the one collective the multi-GPU driver needs (include/gumbi_hip.h)."""

    ALL_GATHER = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("ctx", C.c_void_p), ("all_gather", ALL_GATHER)]


class LaplaceStats(C.Structure):
    """``gmb_laplace_stats``: the Newton iteration of the last ``gmb_laplace_evaluate``."""

    _fields_ = [("iterations", C.c_int32), ("halvings", C.c_int32), ("psi", C.c_double), ("step", C.c_double)]


class DistStep(C.Structure):
    """``gmb_dist_step``: one step of a rank's schedule (include/gumbi_hip.h)."""

    _fields_ = [(n, C.c_int32) for n in ("op", "c0", "c1", "lo", "hi", "first", "count", "maxcount", "stream")] + [
        ("elems", C.c_int64)]
    OPS = ("KBUILD", "SQUARE", "PANEL", "UPDATE", "FORK", "JOIN", "SOLVE", "TAIL")

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_}
        d["op"] = self.OPS[d["op"]]
        return d


class GemmDesc(C.Structure):
    """``gmb_gemm_desc`` (ABI 13): one GEMM launch with every descriptor field and every choice of the launcher pinned or left
    (-1) -- the test door :meth:`Engine.blk_gemm_ex`."""

    _fields_ = [(n, C.c_int64) for n in ("ldc", "lda", "ldb", "m", "n", "k")] + [("alpha", C.c_double), ("beta", C.c_double)] + [
        (n, C.c_int32) for n in ("tri", "tri_off", "nblk_stride", "cblk_stride", "klo_m", "klo_n", "khi_n", "krow_off",
                                 "krow_stride", "variant", "staging", "pfc", "order", "strip")]


#: block tile (BM, BN) of each GEMM tile shape (``variant`` of gmb_gemm_desc)
GEMM_TILE_SHAPES = ((128, 128), (64, 64), (128, 64), (128, 32))


_SIGNATURES = {
    "gmb_abi_version": (C.c_int, []),
    "gmb_device_count": (C.c_int, []),
    "gmb_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p]),
    "gmb_create_sibling": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "gmb_destroy": (None, [C.c_void_p]),
    "gmb_last_error": (C.c_char_p, [C.c_void_p]),
    "gmb_stream": (C.c_void_p, [C.c_void_p]),
    "gmb_set_data": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32]),
    "gmb_set_y": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "gmb_set_kernel": (C.c_int, [C.c_void_p, C.POINTER(_Spec)]),
    "gmb_theta_size": (C.c_int, [C.POINTER(_Spec)]),
    "gmb_set_periodic": (C.c_int, [C.c_void_p, C.c_int32, _DBL_P, C.c_int32]),
    "gmb_set_theta": (C.c_int, [C.c_void_p, _DBL_P, C.c_int32]),
    "gmb_factorize": (C.c_int, [C.c_void_p]),
    "gmb_notpd_index": (C.c_int64, [C.c_void_p]),
    "gmb_factor_valid": (C.c_int, [C.c_void_p]),
    "gmb_nlml": (C.c_int, [C.c_void_p, _DBL_P, _DBL_P]),
    "gmb_evaluate": (C.c_int, [C.c_void_p, _DBL_P, C.c_int32, _DBL_P, _DBL_P]),
    "gmb_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                              C.c_void_p, C.c_int32]),
    "gmb_predict_joint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_draw_joint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_int64,
                                 C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]),
    "gmb_predict_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_predict_with_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_ls_limits": (C.c_int, [C.c_int32, _DBL_P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, _DBL_P, _DBL_P]),
    "gmb_mfma_f64_peak": (C.c_int, [C.c_int32, _DBL_P, _DBL_P]),
    "gmb_mfma_f64_sustained": (C.c_int, [C.c_int32, C.c_double, _DBL_P, _DBL_P, _DBL_P, C.POINTER(C.c_int64)]),
    "gmb_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "gmb_timings_get": (C.c_int, [C.c_void_p, C.POINTER(Timings)]),
    "gmb_copy_factor": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _DBL_P]),
    "gmb_copy_v": (C.c_int, [C.c_void_p, _DBL_P]),
    "gmb_blk_potrf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmb_copy_alpha": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "gmb_rccl_unique_id": (C.c_int, [C.c_char_p, C.c_void_p]),
    "gmb_rccl_comm_create": (C.c_int, [C.POINTER(C.POINTER(GmbComm)), C.c_char_p, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_int32]),
    "gmb_rccl_comm_destroy": (None, [C.POINTER(GmbComm)]),
    "gmb_rccl_comm_ranks": (C.c_int, [C.POINTER(GmbComm)]),
    "gmb_rccl_comm_split": (C.c_int, [C.POINTER(GmbComm)]),
    "gmb_rccl_last_error": (C.c_char_p, []),
    "gmb_dist_plan": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DistStep), C.c_int64]),
    "gmb_dist_factorize": (C.c_int, [C.c_void_p, C.POINTER(GmbComm), C.c_int32]),
    "gmb_dist_nlml": (C.c_int, [C.c_void_p, C.POINTER(GmbComm), _DBL_P, _DBL_P]),
    "gmb_dist_predict": (C.c_int, [C.c_void_p, C.POINTER(GmbComm), C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_int32]),
    "gmb_debug_cov_grid": (C.c_int64, [C.c_int32] * 7 + [C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]),
    "gmb_debug_tile_list": (C.c_int64, [C.c_int32] * 12 + [C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int32)]),
    "gmb_debug_chol_task": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gmb_chol_task_trace": (C.c_int64, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    "gmb_set_chol_scheme": (C.c_int, [C.c_void_p, C.c_int32]),
    "gmb_debug_assume_factored": (C.c_int, [C.c_void_p]),
    "gmb_set_eval_pairs": (C.c_int, [C.c_void_p, C.c_int32]),
    "gmb_set_predict_form": (C.c_int, [C.c_void_p, C.c_int32]),
    "gmb_reserve": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    "gmb_set_grad_scheme": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "gmb_dist_set_mode": (C.c_int, [C.c_void_p, C.c_int32]),
    "gmb_resident_bytes": (C.c_int64, [C.c_void_p, C.c_int32]),
    "gmb_debug_eval_tasks": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_int64]),
    "gmb_debug_chol_lose_tickets": (C.c_int, [C.c_void_p, C.c_int32]),
    "gmb_blk_invert": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "gmb_blk_covariance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "gmb_blk_trsm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                               C.c_int32]),
    "gmb_blk_gemm_nt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                  C.c_int32, C.c_int64]),
    "gmb_blk_gemm_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GemmDesc), C.POINTER(C.c_int32)]),
    "gmb_blk_gemm_splitk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                      C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "gmb_append": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32]),
    "gmb_truncate": (C.c_int, [C.c_void_p, C.c_int64]),
    "gmb_num_obs": (C.c_int64, [C.c_void_p]),
    "gmb_num_terms": (C.c_int, [C.c_void_p]),
    "gmb_predict_terms": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_int32]),
    "gmb_predict_grad_terms": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_predict_joint_terms": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_draw_joint_terms": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_void_p,
                                       C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]),
    "gmb_predict_decompose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_int32]),
    "gmb_loo": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]),
    "gmb_leave_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                C.c_int32]),
    "gmb_predict_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_predict_groups_terms": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_debug_group_tasks": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]),
    "gmb_predict_slope": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_int64, C.c_int32]),
    "gmb_predict_slope_terms": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_debug_slope_tile_rows": (C.c_int64, [C.c_int64, C.c_int32]),
    "gmb_design_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "gmb_debug_design_plan": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]),
    "gmb_predict_batches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]),
    "gmb_debug_batch_plan": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64]),
    "gmb_paths_prepare": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmb_paths_eval": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_paths_eval_own": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "gmb_paths_clear": (C.c_int, [C.c_void_p]),
    "gmb_paths_count": (C.c_int32, [C.c_void_p]),
    "gmb_debug_paths_plan": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64]),
    "gmb_fitc_set_inducing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32]),
    "gmb_fitc_evaluate": (C.c_int, [C.c_void_p, _DBL_P, C.c_int32, _DBL_P, _DBL_P]),
    "gmb_fitc_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]),
    "gmb_debug_fitc_plan": (C.c_int64, [C.c_int64, C.c_int64, C.c_void_p, C.c_int64]),
    "gmb_laplace_evaluate": (C.c_int, [C.c_void_p, _DBL_P, C.c_int32, _DBL_P, _DBL_P]),
    "gmb_laplace_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]),
    "gmb_laplace_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmb_laplace_copy_mode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmb_laplace_set_options": (C.c_int, [C.c_void_p, C.c_double, C.c_int32]),
    "gmb_debug_laplace_plan": (C.c_int64, [C.c_int64, C.c_void_p, C.c_int64]),
    "gmb_debug_laplace_symv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}


def exported_symbols() -> list:
    """Every entry point ``include/gumbi_hip.h`` declares."""
    return list(_SIGNATURES)


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so with the
    same SONAME (libamdhip64.so.7) as /opt/rocm's; whichever is mapped first serves every later
    request for that SONAME, but torch asks for its copy by *file name* and would map a second
    runtime if ours came from /opt/rocm first.  Mapping torch's copy up front (when torch is
    installed) makes libgumbi_hip.so, torch and RCCL share one runtime -- and therefore streams,
    events and device pointers -- in either import order."""
    if os.environ.get("GUMBI_HIP_SYSTEM_RUNTIME") == "1":
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
        if cand.exists():
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
    except OSError:
        pass  # fall back to whatever libamdhip64.so.7 the loader finds


#: GMB_ABI_VERSION of include/gumbi_hip.h this binding was written against (the layout of
#: ``gmb_kernel_spec`` changed with version 2: ``additive``; ``gmb_timings`` grew with version 3; version 4 replaced the block-level
#: multi-GPU entry points by the native driver ``gmb_dist_*``; version 5 added ``gmb_blk_covariance``, ``gmb_set_y`` and ``gmb_create_sibling``;
#: version 6 the communication fields of ``gmb_timings`` and ``gmb_rccl_comm_ranks``; version 7 ``gmb_evaluate``, the tile
#: Cholesky's doors ``gmb_set_chol_scheme`` / ``gmb_chol_task_trace`` / ``gmb_debug_chol_*``; version 8 the persistent evaluation
#: launch: ``gmb_set_grad_scheme``, ``gmb_debug_eval_tasks``, ``total_eval_tile_*`` in ``gmb_timings``; version 9 the timing
#: tools' door ``gmb_debug_assume_factored``, the guards between single-engine and capacity-mode factorisations, ``gmb_set_eval_pairs``;
#: version 10 ``gmb_set_predict_form`` (GEMM-form prediction behind a fit), ``total_chol_update_all_*`` / ``predict_gemm_form`` in
#: ``gmb_timings``, ``gmb_debug_assume_factored`` behind GUMBI_HIP_DEBUG_DOORS=1; version 11 the joint posterior:
#: ``gmb_predict_joint`` / ``gmb_draw_joint``; version 12 periodic kernels: ``gmb_set_periodic``; version 13 the GEMM test door
#: ``gmb_blk_gemm_ex`` / ``gmb_gemm_desc``; version 14 the posterior mean's gradient ``gmb_predict_grad``; version 15 mean and
#: variance with both gradients in one call, ``gmb_predict_with_grad``; version 16 ``gmb_append`` / ``gmb_truncate`` -- observations
#: appended to / cut from the resident factor -- and the split-k GEMM's test door ``gmb_blk_gemm_splitk``; added to version 16
#: without a change of layout: the components of an additive model, ``gmb_num_terms``, the ``gmb_*_terms`` forms of the four
#: prediction calls and ``gmb_predict_decompose``; likewise the leave-out predictions of the training rows, ``gmb_loo`` /
#: ``gmb_leave_out``, and the averages of the posterior over groups of points, ``gmb_predict_groups`` / ``gmb_predict_groups_terms``
#: with the host-only ``gmb_debug_group_tasks``, and the posterior of the slope, ``gmb_predict_slope`` / ``gmb_predict_slope_terms``
#: with the host-only ``gmb_debug_slope_tile_rows``, and the batch design by integrated variance reduction, ``gmb_design_batch`` with
#: the host-only ``gmb_debug_design_plan``, and the sparse path ``gmb_fitc_*``, and GP classification by the Laplace approximation,
#: ``gmb_laplace_*`` with the status ``GMB_ENOCONV``, the struct ``gmb_laplace_stats`` and the host-only ``gmb_debug_laplace_plan``,
#: and the joint posteriors of many small batches with their derivatives, ``gmb_predict_batches`` with the host-only
#: ``gmb_debug_batch_plan``, and the pathwise posterior draws, ``gmb_paths_prepare`` / ``gmb_paths_eval`` / ``gmb_paths_eval_own`` /
#: ``gmb_paths_clear`` / ``gmb_paths_count`` with the host-only ``gmb_debug_paths_plan``)
ABI_VERSION = 16

#: points per task of ``gmb_predict_groups`` (csrc/group_tasks.hpp)
GROUP_CHUNK = 512


def load_library():
    """Load libgumbi_hip.so (once) and attach the prototypes.  Raises if it is not built or was
    built from another version of the header."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not path.exists():
        raise GumbiHipError(
            f"{path} not found: the HIP engine is not built (run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or `make -C gumbi_amd/csrc`). gumbi_amd has no CPU fallback."
        )
    _preload_hip_runtime()
    lib = C.CDLL(str(path))
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header / library mismatch
        fn.restype, fn.argtypes = restype, argtypes
    if lib.gmb_abi_version() != ABI_VERSION:
        raise GumbiHipError(f"{path} has ABI version {lib.gmb_abi_version()}, this binding needs {ABI_VERSION}: "
                            f"rebuild it (`python -m gumbi_amd.build`)")
    _LIB = lib
    return lib


def _ptr(arr):
    return arr.ctypes.data_as(C.c_void_p)


def terms_mask(terms) -> int:
    """A term selection as the ``*_terms`` calls take it: an ``int`` is the mask itself (bit t = term t: 0 the global kernel,
    1 + j coregion dimension j), anything else an iterable of term indices.  Whether the model has those terms is the engine's
    to say (``ValueError``)."""
    if isinstance(terms, (int, np.integer)) and not isinstance(terms, bool):
        mask = int(terms)
    else:
        mask = 0
        for t in terms:
            t = int(t)
            if not 0 <= t < 32:
                raise ValueError(f"term index {t} out of range")
            mask |= 1 << t
    if not 0 <= mask < 2 ** 32:
        raise ValueError(f"terms mask {mask} does not fit 32 bits")
    return mask


def _dptr(arr):
    return arr.ctypes.data_as(_DBL_P)


def device_count() -> int:
    n = load_library().gmb_device_count()
    return max(n, 0)


class Engine:
    """One GP resident on one MI355X: data, covariance / factor, predict workspaces."""

    #: the evaluations do not run on the host's BLAS (HipGP.find_MAP keeps OpenBLAS to one thread inside the optimiser's loop)
    host_blas_free = True

    def __init__(self, device: int = 0, stream: int | None = None, sibling_of: "Engine | None" = None):
        self._lib = load_library()
        self._h = C.c_void_p()
        self._peer = sibling_of  # a sibling borrows the peer's HIP streams: the peer must outlive it
        if sibling_of is not None:  # gmb_create_sibling; close the sibling first
            rc = self._lib.gmb_create_sibling(C.byref(self._h), sibling_of._h)
        else:
            rc = self._lib.gmb_create(C.byref(self._h), int(device), C.c_void_p(stream) if stream else None)
        if rc == GMB_ENODEVICE:
            raise GumbiHipError("no HIP device visible: gumbi_amd needs an MI355X (gfx950); there is no CPU fallback")
        if rc != GMB_OK:
            raise GumbiHipError(f"gmb_create failed with status {rc}")
        self.spec = None
        self.N = 0
        self.D = 0
        #: advanced by every :meth:`paths_prepare` and :meth:`paths_clear`: the identity of the ONE set of pathwise draws the engine holds
        self.paths_generation = 0

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.gmb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- error mapping (Regressor error surface: ValueError / LinAlgError) ---------
    def _check(self, rc, what):
        if rc == GMB_OK:
            return
        msg = self._lib.gmb_last_error(self._h)
        msg = msg.decode() if msg else ""
        if rc == GMB_EINVAL:
            raise ValueError(f"{what}: {msg}")
        if rc == GMB_ENOTPD:
            raise np.linalg.LinAlgError(f"{what}: {msg}")
        if rc == GMB_ENOMEM:
            raise MemoryError(f"{what}: {msg}")
        if rc == GMB_ENODEVICE:
            raise GumbiHipError(f"{what}: no HIP device (no CPU fallback exists)")
        if rc == GMB_ENOCONV:
            raise LaplaceConvergenceError(f"{what}: {msg}")
        raise GumbiHipError(f"{what}: status {rc}: {msg}")

    @property
    def stream(self) -> int:
        return int(self._lib.gmb_stream(self._h) or 0)

    # -- model definition -----------------------------------------------------------------------
    def set_data(self, X, y):
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if X.ndim != 2 or y.ndim != 1 or X.shape[0] != y.shape[0]:
            raise ValueError(f"X must be (N, D) and y (N,), got {X.shape} and {y.shape}")
        self._check(self._lib.gmb_set_data(self._h, _ptr(X), X.shape[0], X.shape[1], X.shape[1], _ptr(y), GMB_HOST),
                    "gmb_set_data")
        self.N, self.D = X.shape

    def set_y(self, y):
        """New observations for the same inputs: everything but the factorisation stays."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (self.N,):
            raise ValueError(f"y must be ({self.N},), got {y.shape}")
        self._check(self._lib.gmb_set_y(self._h, _ptr(y), GMB_HOST), "gmb_set_y")

    def append(self, X, y):
        """``K`` further observations for the same kernel and theta (``gmb_append``): with a valid resident factor the factor is
        updated in O(N^2 K) and stays valid (``LinAlgError`` when the grown covariance is not positive definite: the data then has
        the new N, ``truncate`` + ``factorize`` recovers); without one only the data changes.  No ``set_theta`` is needed."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if X.ndim != 2 or y.ndim != 1 or X.shape[0] != y.shape[0] or X.shape[1] != self.D:
            raise ValueError(f"X must be (K, {self.D}) and y (K,), got {X.shape} and {y.shape}")
        try:
            self._check(self._lib.gmb_append(self._h, _ptr(X), X.shape[0], self.D, _ptr(y), GMB_HOST), "gmb_append")
        finally:
            self.N = int(self._lib.gmb_num_obs(self._h))  # (after an error the data may have either size: the engine says which)

    def truncate(self, n: int):
        """Keep the first ``n`` observations (``gmb_truncate``, ``1 <= n <= N``); a valid resident factor is cut along."""
        try:
            self._check(self._lib.gmb_truncate(self._h, int(n)), "gmb_truncate")
        finally:
            self.N = int(self._lib.gmb_num_obs(self._h))

    def set_data_device(self, x_ptr: int, N: int, D: int, ldx: int, y_ptr: int):
        """Inputs already in HBM (e.g. ``torch.Tensor.data_ptr()``)."""
        self._check(self._lib.gmb_set_data(self._h, C.c_void_p(x_ptr), N, D, ldx, C.c_void_p(y_ptr), GMB_DEVICE),
                    "gmb_set_data")
        self.N, self.D = N, D

    def set_kernel(self, spec: KernelSpec):
        cs = spec.to_c()
        self._check(self._lib.gmb_set_kernel(self._h, C.byref(cs)), "gmb_set_kernel")
        if int(getattr(spec, "periodic", 0)) != 0:
            self.set_periodic(spec.periodic, spec.periods)
        self.spec = spec

    def set_periodic(self, mode: int, periods):
        """Periodic continuous kernel (``gmb_set_periodic``): ``mode`` 0 off, 1 ``<kind>+Periodic``, 2 ``Periodic`` (kind ExpQuad);
        ``periods``: one per continuous dimension of the kernel, in the units of ``X``.  Call between ``set_kernel`` (which
        resets the mode) and ``set_theta``; ``ValueError`` for what the engine refuses."""
        periods = np.ascontiguousarray(periods, dtype=np.float64).ravel()
        self._check(self._lib.gmb_set_periodic(self._h, int(mode), _dptr(periods) if periods.size else None, periods.size),
                    "gmb_set_periodic")

    def set_theta(self, theta):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        self._check(self._lib.gmb_set_theta(self._h, _dptr(theta), theta.size), "gmb_set_theta")

    # -- hot path ----------------------------------------------------------------------------------
    def factorize(self):
        self._check(self._lib.gmb_factorize(self._h), "gmb_factorize")

    def notpd_index(self) -> int:
        return int(self._lib.gmb_notpd_index(self._h))

    def factor_is_current(self) -> bool:
        """True while a usable factorisation of the current (data, kernel, theta) is resident -- also after
        ``nlml(grad=True)``: ``predict`` may follow without another ``factorize``."""
        return bool(self._lib.gmb_factor_valid(self._h))

    def nlml(self, grad: bool = False):
        val = C.c_double()
        if not grad:
            self._check(self._lib.gmb_nlml(self._h, C.byref(val), None), "gmb_nlml")
            return val.value
        g = np.empty(self.spec.theta_size(), dtype=np.float64)
        self._check(self._lib.gmb_nlml(self._h, C.byref(val), _dptr(g)), "gmb_nlml")
        return val.value, g

    def evaluate(self, theta, grad: bool = True):
        """``set_theta`` + ``factorize`` + ``nlml`` in one call (no host round trip between the factorisation and the
        gradient): ``(nlml, gradient)`` or ``nlml``."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        val = C.c_double()
        g = np.empty(self.spec.theta_size(), dtype=np.float64) if grad else None
        self._check(self._lib.gmb_evaluate(self._h, _dptr(theta), theta.size, C.byref(val), _dptr(g) if grad else None), "gmb_evaluate")
        return (val.value, g) if grad else val.value

    @property
    def num_terms(self) -> int:
        """Covariance terms of the model (``gmb_num_terms``): 1, or 1 + the coregion dimensions of an additive spec."""
        n = int(self._lib.gmb_num_terms(self._h))
        if n < 0:
            raise ValueError("gmb_num_terms: gmb_set_theta has not been called")
        return n

    def predict(self, Xs, with_noise=True, terms=None):
        """Posterior mean and variance at the rows of ``Xs``.  ``terms`` (a mask or an iterable of term indices,
        :func:`terms_mask`) restricts an additive model to a selection of its terms (``gmb_predict_terms``); ``with_noise`` then
        still adds the model's noise."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        M = Xs.shape[0]
        mean = np.empty(M, dtype=np.float64)
        var = np.empty(M, dtype=np.float64)
        if terms is not None:
            self._check(
                self._lib.gmb_predict_terms(self._h, terms_mask(terms), _ptr(Xs), M, Xs.shape[1], int(bool(with_noise)), _ptr(mean),
                                            _ptr(var), GMB_HOST),
                "gmb_predict_terms",
            )
            return mean, var
        self._check(
            self._lib.gmb_predict(self._h, _ptr(Xs), M, Xs.shape[1], int(bool(with_noise)), _ptr(mean), _ptr(var),
                                  GMB_HOST),
            "gmb_predict",
        )
        return mean, var

    def _joint_points(self, Xs):
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        return Xs

    def predict_joint(self, Xs, with_noise=True, jitter=0.0, terms=None):
        """Posterior mean (M) and the full M x M posterior covariance ``K** - V V^T (+ noise) + jitter I`` at the rows of
        ``Xs`` (``gmb_predict_joint``; ``pm.gp.Marginal._build_conditional(..., diag=False)``).  ``MemoryError`` -- raised
        before anything is computed -- when the device cannot hold the request."""
        Xs = self._joint_points(Xs)
        M = Xs.shape[0]
        mean = np.empty(M, dtype=np.float64)
        cov = np.empty((M, M), dtype=np.float64)
        if terms is not None:  # a selection of an additive model's terms (gmb_predict_joint_terms)
            self._check(
                self._lib.gmb_predict_joint_terms(self._h, terms_mask(terms), _ptr(Xs), M, Xs.shape[1], int(bool(with_noise)),
                                                  float(jitter), _ptr(mean), _ptr(cov), M, GMB_HOST),
                "gmb_predict_joint_terms",
            )
            return mean, cov
        self._check(
            self._lib.gmb_predict_joint(self._h, _ptr(Xs), M, Xs.shape[1], int(bool(with_noise)), float(jitter), _ptr(mean),
                                        _ptr(cov), M, GMB_HOST),
            "gmb_predict_joint",
        )
        return mean, cov

    def draw_joint(self, Xs, Z, with_noise=False, jitter=1e-6, return_mean=False, terms=None):
        """``Y[s] = mean + L* Z[s]`` for the S rows of ``Z`` (S x M standard normals of the caller's), ``L*`` the lower Cholesky
        factor of ``predict_joint``'s covariance (``gmb_draw_joint``): S correlated draws of the posterior at the rows of
        ``Xs``, a deterministic function of (model, theta, Xs, Z).  ``LinAlgError`` when that covariance is not positive
        definite (``notpd_index``: its row).  ``return_mean=True`` returns ``(Y, mean)``."""
        Xs = self._joint_points(Xs)
        M = Xs.shape[0]
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[1] != M:
            raise ValueError(f"Z must be (S, {M}), got {Z.shape}")
        S = Z.shape[0]
        Y = np.empty((S, M), dtype=np.float64)
        mean = np.empty(M, dtype=np.float64)
        if terms is not None:  # a selection of an additive model's terms (gmb_draw_joint_terms)
            self._check(
                self._lib.gmb_draw_joint_terms(self._h, terms_mask(terms), _ptr(Xs), M, Xs.shape[1], int(bool(with_noise)), float(jitter),
                                               _ptr(Z), S, max(M, 1), _ptr(Y), max(M, 1), _ptr(mean), GMB_HOST),
                "gmb_draw_joint_terms",
            )
            return (Y, mean) if return_mean else Y
        self._check(
            self._lib.gmb_draw_joint(self._h, _ptr(Xs), M, Xs.shape[1], int(bool(with_noise)), float(jitter), _ptr(Z), S, max(M, 1),
                                     _ptr(Y), max(M, 1), _ptr(mean), GMB_HOST),
            "gmb_draw_joint",
        )
        return (Y, mean) if return_mean else Y

    def predict_grad(self, Xs, terms=None):
        """Gradient of the posterior mean with respect to the test point at the rows of ``Xs``: ``(M, D)``, one column per
        column of ``X`` -- the kernel's continuous columns carry the derivative, every other column 0 (``gmb_predict_grad``).
        Needs the resident factor as ``predict`` does and leaves it, and everything a fit left beside it, untouched."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        M = Xs.shape[0]
        grad = np.empty((M, self.D), dtype=np.float64)
        if terms is not None:  # a selection of an additive model's terms (gmb_predict_grad_terms)
            self._check(self._lib.gmb_predict_grad_terms(self._h, terms_mask(terms), _ptr(Xs), M, self.D, _ptr(grad), self.D, GMB_HOST),
                        "gmb_predict_grad_terms")
            return grad
        self._check(self._lib.gmb_predict_grad(self._h, _ptr(Xs), M, self.D, _ptr(grad), self.D, GMB_HOST), "gmb_predict_grad")
        return grad

    def predict_decompose(self, Xs):
        """Every component of an additive model at the rows of ``Xs`` from one pass (``gmb_predict_decompose``):
        ``(means, cov, noise)`` -- ``means`` (T, M) the posterior means of the T terms, ``cov`` (T, T, M) the symmetric pointwise
        posterior covariance of the latent components (``cov[t, u, m] = delta_tu k_t(x*, x*) - <V_t, V_u>``: no noise, no jitter),
        ``noise`` (M) the model's noise variance at each point.  ``means.sum(0)`` is ``predict``'s mean and ``cov.sum((0, 1))`` its
        noise-free variance."""
        Xs = self._joint_points(Xs)
        M = Xs.shape[0]
        T = self.num_terms
        means = np.empty((T, M), dtype=np.float64)
        packed = np.empty((T * (T + 1) // 2, M), dtype=np.float64)
        noise = np.empty(M, dtype=np.float64)
        self._check(self._lib.gmb_predict_decompose(self._h, _ptr(Xs), M, Xs.shape[1], _ptr(means), max(M, 1), _ptr(packed), max(M, 1),
                                                    _ptr(noise), GMB_HOST), "gmb_predict_decompose")
        cov = np.empty((T, T, M), dtype=np.float64)
        for t in range(T):
            for u in range(t + 1):
                cov[t, u] = cov[u, t] = packed[t * (t + 1) // 2 + u]
        return means, cov, noise

    def loo(self, rows=None, with_noise=True):
        """Leave-one-out predictions of the training rows from the resident factor (``gmb_loo``): ``(mean, var)`` -- what the
        model, at the resident theta, predicts for observation i from all the others, ``mean_i = y_i - alpha_i / d_i`` and
        ``var_i = 1 / d_i - jitter`` (less the row's noise with ``with_noise=False``), ``d_i = (Sigma^-1)_ii``.  ``rows``:
        ``None`` for every row, or a ``(start, stop)`` pair.  No refit: behind a fit it is one pass over the resident inverse
        factor."""
        start, stop = (0, self.N) if rows is None else (int(rows[0]), int(rows[1]))
        n = stop - start
        mean = np.empty(max(n, 0), dtype=np.float64)
        var = np.empty(max(n, 0), dtype=np.float64)
        self._check(self._lib.gmb_loo(self._h, start, n, int(bool(with_noise)), _ptr(mean), _ptr(var), GMB_HOST), "gmb_loo")
        return mean, var

    def leave_out(self, idx, with_noise=True, cov=False):
        """The joint prediction of the training rows ``idx`` from all the others (``gmb_leave_out``): ``(mean, var)``, or
        ``(mean, var, cov)`` with ``cov=True``, in the order of ``idx``.  ``mean = y_B - C^-1 alpha_B`` and
        ``cov = C^-1 - jitter I`` (less the rows' noise with ``with_noise=False``), ``C = (Sigma^-1)_BB``.  ``ValueError`` for
        duplicate or out-of-range rows, ``LinAlgError`` when C is not positive definite, ``MemoryError`` -- before anything is
        computed -- when the device cannot hold the request."""
        idx = np.ascontiguousarray(np.asarray(idx).ravel(), dtype=np.int64)
        m = idx.shape[0]
        mean = np.empty(m, dtype=np.float64)
        var = np.empty(m, dtype=np.float64)
        full = np.empty((m, m), dtype=np.float64) if cov else None
        self._check(self._lib.gmb_leave_out(self._h, _ptr(idx), m, int(bool(with_noise)), _ptr(mean), _ptr(var),
                                            _ptr(full) if cov else None, max(m, 1), GMB_HOST), "gmb_leave_out")
        return (mean, var, full) if cov else (mean, var)

    def predict_groups(self, Xs, offsets, weights=None, cov=False, terms=None):
        """Weighted averages of the LATENT posterior over groups of the rows of ``Xs`` (``gmb_predict_groups``): ``(mean, var)``,
        or ``(mean, var, cov)`` with ``cov=True`` -- ``mean_g = sum_{m in g} w_m E f(x_m)`` and ``cov = W C W^T`` with C the joint
        posterior covariance of all the points (never formed: nothing of size M x M or M x N exists on the device).  Group g is
        the rows ``offsets[g]:offsets[g + 1]`` (``offsets[0] == 0``, strictly increasing, ``offsets[-1] == len(Xs)``);
        ``weights`` of any sign, ``None`` for a plain mean ``1 / |g|``.  No noise, no jitter, variances not clipped; ``cov`` is
        exactly symmetric and its diagonal is ``var``.  ``terms`` selects terms of an additive model (:func:`terms_mask`).
        ``ValueError`` for malformed offsets or weights that are not finite, ``MemoryError`` -- before anything is computed --
        when the device cannot hold the request."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        offsets = np.ascontiguousarray(np.asarray(offsets).ravel(), dtype=np.int64)
        M, G = Xs.shape[0], offsets.shape[0] - 1
        if weights is not None:
            weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel())
            if weights.shape[0] != M:
                raise ValueError(f"predict_groups: {weights.shape[0]} weights for {M} points")
        mean = np.empty(max(G, 0), dtype=np.float64)
        var = np.empty(max(G, 0), dtype=np.float64)
        full = np.empty((G, G), dtype=np.float64) if cov and G > 0 else None
        tail = (_ptr(Xs), M, Xs.shape[1] if Xs.ndim == 2 else 0, _ptr(offsets), G, _ptr(weights) if weights is not None else None,
                _ptr(mean), _ptr(var), _ptr(full) if full is not None else None, max(G, 1), GMB_HOST)
        if terms is not None:
            self._check(self._lib.gmb_predict_groups_terms(self._h, terms_mask(terms), *tail), "gmb_predict_groups_terms")
        else:
            self._check(self._lib.gmb_predict_groups(self._h, *tail), "gmb_predict_groups")
        return (mean, var, full) if cov else (mean, var)

    def predict_slope(self, Xs, cov=False, terms=None):
        """The posterior of the slope ``d f / d x*`` of the LATENT function at the rows of ``Xs`` (``gmb_predict_slope``):
        ``(dmean, dvar)``, ``(M, D)`` each with the columns of :meth:`predict_grad`, or ``(dmean, dvar, dcov)`` with ``cov=True``,
        ``dcov`` ``(M, D, D)`` the joint covariance of the partial derivatives at each point -- exactly symmetric, its diagonal
        equal to ``dvar``.  ``dmean`` is the quantity :meth:`predict_grad` returns; ``dvar`` is the variance OF the slope, not
        the slope of the variance (:meth:`predict_with_grad`).  Columns that carry no derivative are 0; variances are not
        clipped.  ``terms`` selects terms of an additive model (:func:`terms_mask`).  ``ValueError`` for a Matern-1/2 or
        Exponential kernel, whose process has no derivative.  Leaves the factor and everything a fit left beside it untouched."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        M, D = Xs.shape[0], self.D
        dmean, dvar = np.empty((M, D), dtype=np.float64), np.empty((M, D), dtype=np.float64)
        dcov = np.empty((M, D, D), dtype=np.float64) if cov else None
        tail = (_ptr(Xs), M, D, _ptr(dmean), _ptr(dvar), D, _ptr(dcov) if cov else None, D * D, GMB_HOST)
        if terms is not None:
            self._check(self._lib.gmb_predict_slope_terms(self._h, terms_mask(terms), *tail), "gmb_predict_slope_terms")
        else:
            self._check(self._lib.gmb_predict_slope(self._h, *tail), "gmb_predict_slope")
        return (dmean, dvar, dcov) if cov else (dmean, dvar)

    def design_batch(self, Xc, Xr, q, weights=None, with_noise=True, allow_repeats=True):
        """A batch of ``q`` experiments by greedy integrated variance reduction (``gmb_design_batch``): which rows of the
        candidates ``Xc`` (M x D), measured next, lower the LATENT posterior variance summed over the reference points ``Xr``
        (R x D, ``weights`` >= 0, ``None`` = ``1 / R`` each) the most.  Returns ``(picks, gains, score0, ivar0)``: the picked
        candidate indices in pick order (-1 once no candidate has a positive gain), the variance each pick removes, the step-0
        score of every candidate and ``sum_r w_r var f(x_r)`` before any pick.  ``with_noise``: a measurement carries the
        model's noise; then ``allow_repeats`` lets a candidate be picked again -- a replicate.  ``q = 0`` computes the scores
        alone.  No ``y`` is fantasised: a GP's posterior covariance does not depend on it.  ``ValueError`` for a negative or
        non-finite weight or a NaN coordinate, ``MemoryError`` -- before anything is computed -- when the device cannot hold the
        request.  Leaves the factor and everything a fit left beside it untouched."""
        Xc = np.ascontiguousarray(Xc, dtype=np.float64)
        Xr = np.ascontiguousarray(Xr, dtype=np.float64)
        for name, X in (("Xc", Xc), ("Xr", Xr)):
            if X.ndim != 2 or X.shape[1] != self.D:
                raise ValueError(f"design_batch: {name} must be (n, {self.D}), got {X.shape}")
        M, R, q = Xc.shape[0], Xr.shape[0], int(q)
        if weights is not None:
            weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel())
            if weights.shape[0] != R:
                raise ValueError(f"design_batch: {weights.shape[0]} weights for {R} reference points")
        picks = np.full(max(q, 0), -1, dtype=np.int64)
        gains = np.zeros(max(q, 0), dtype=np.float64)
        score0 = np.zeros(M, dtype=np.float64)
        ivar0 = np.zeros(1, dtype=np.float64)
        self._check(self._lib.gmb_design_batch(self._h, _ptr(Xc), M, self.D, _ptr(Xr), R, self.D,
                                               _ptr(weights) if weights is not None else None, q, int(bool(with_noise)),
                                               int(bool(allow_repeats)), _ptr(picks), _ptr(gains), _ptr(score0), _ptr(ivar0), GMB_HOST),
                    "gmb_design_batch")
        return picks, gains, score0, float(ivar0[0])

    def predict_with_grad(self, Xs, with_noise=True):
        """``(mean, var, dmean, dvar)`` at the rows of ``Xs``: ``predict``'s mean and variance (M each) and their gradients with
        respect to the test point, ``(M, D)`` each with the columns of :meth:`predict_grad` (``gmb_predict_with_grad``) -- one
        engine call per evaluation of an acquisition function and its gradient.  ``with_noise`` changes ``var`` only.  Needs
        the resident factor as ``predict`` does and leaves it, and everything a fit left beside it, untouched."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        M = Xs.shape[0]
        mean, var = np.empty(M, dtype=np.float64), np.empty(M, dtype=np.float64)
        dmean, dvar = np.empty((M, self.D), dtype=np.float64), np.empty((M, self.D), dtype=np.float64)
        self._check(self._lib.gmb_predict_with_grad(self._h, _ptr(Xs), M, self.D, int(bool(with_noise)), _ptr(mean), _ptr(var),
                                                    _ptr(dmean), _ptr(dvar), self.D, GMB_HOST), "gmb_predict_with_grad")
        return mean, var, dmean, dvar

    def predict_batches(self, Xs, q, jitter=1e-6, grad=True):
        """The joint LATENT posterior of every batch of ``q`` consecutive rows of ``Xs`` (``(B q, D)`` or ``(B, q, D)``,
        ``1 <= q <= 16``) and its derivative with respect to the batch's own coordinates (``gmb_predict_batches``):
        ``(mean (B, q), cov (B, q, q), dmean (B, q, D), dcov (B, q, q, D))``, or the first two with ``grad=False`` (the same
        bits; the second triangular pass is skipped).  ``cov[b] = K(P_b, P_b) - V_b V_b^T + jitter I``, exactly symmetric;
        ``dcov[b, j, l] = d cov[b, j, l] / d x_j``, for ``l = j`` the full derivative of the variance, i.e.
        :meth:`predict_with_grad`'s ``dvar``; ``dmean`` is :meth:`predict_grad`'s.  One engine call per evaluation of a
        Monte-Carlo batch acquisition for ``B`` restarts.  Leaves the factor and everything a fit left beside it untouched."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        q = int(q)
        if Xs.ndim == 3 and Xs.shape[1] == q:
            Xs = Xs.reshape(-1, Xs.shape[2])
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"predict_batches: Xs must be (B q, {self.D}) or (B, q, {self.D}), got {Xs.shape}")
        if q < 1 or Xs.shape[0] % q:
            raise ValueError(f"predict_batches: {Xs.shape[0]} points are no whole number of batches of q = {q}")
        B, D = Xs.shape[0] // q, self.D
        mean, cov = np.empty((B, q), dtype=np.float64), np.empty((B, q, q), dtype=np.float64)
        dmean = np.empty((B, q, D), dtype=np.float64) if grad else None
        dcov = np.empty((B, q, q, D), dtype=np.float64) if grad else None
        self._check(self._lib.gmb_predict_batches(self._h, _ptr(Xs), B, q, D, float(jitter), _ptr(mean), _ptr(cov),
                                                  _ptr(dmean) if grad else None, D, _ptr(dcov) if grad else None, GMB_HOST),
                    "gmb_predict_batches")
        return (mean, cov, dmean, dcov) if grad else (mean, cov)

    # -- pathwise posterior draws (csrc/pathwise.hpp) ---------------------------------------------------------------------
    def paths_prepare(self, omega, phase, w, eps):
        """Prepare ``S`` posterior function draws (``gmb_paths_prepare``; the arrays are :func:`gumbi_amd.pathwise.path_inputs`'s):
        ``omega (F, Dc)`` frequencies in the prepared coordinates, ``phase (F,)``, ``w (S, F)`` and ``eps (S, N)`` standard
        normals.  One solve with ``S`` right-hand sides against the resident factor; the state stays on the device until the
        data, theta or the factor change.  ``ValueError`` for a model outside the scope (linear or categorical dimensions,
        several outputs, additive, periodic), ``1 <= S <= 512``, ``1 <= F <= 16384``.  Leaves the factor and everything a fit
        left beside it untouched.

        Returns the set's generation: :attr:`paths_generation`, which every preparation and :meth:`paths_clear` advance -- an
        engine holds ONE set, and whoever keeps a handle on a set (``PosteriorPaths``) compares it to know whether the set is
        still the engine's."""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        if omega.ndim == 1:
            omega = omega[:, None]
        phase = np.ascontiguousarray(phase, dtype=np.float64).ravel()
        w = np.ascontiguousarray(w, dtype=np.float64)
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        if w.ndim != 2 or eps.ndim != 2 or omega.ndim != 2:
            raise ValueError("paths_prepare: omega must be (F, Dc), w (S, F) and eps (S, N)")
        S, F = w.shape
        if omega.shape[0] != F or phase.shape != (F,) or eps.shape != (S, self.N) or omega.shape[1] != len(self.spec.idx_cont):
            raise ValueError(f"paths_prepare: omega {omega.shape}, phase {phase.shape}, w {w.shape}, eps {eps.shape} do not fit "
                             f"(F, {len(self.spec.idx_cont)}), (F,), (S, F), (S, {self.N})")
        self.paths_generation += 1  # (before the call: a preparation that fails half-way has dropped the previous set as well)
        self._check(self._lib.gmb_paths_prepare(self._h, S, F, _ptr(omega), _ptr(phase), _ptr(w), _ptr(eps)), "gmb_paths_prepare")
        return self.paths_generation

    @property
    def n_paths(self) -> int:
        """Draws of the prepared set (``gmb_paths_count``): the rows :meth:`paths_eval` returns; 0 when none are prepared."""
        return int(self._lib.gmb_paths_count(self._h))

    def paths_eval(self, Xs):
        """All prepared draws at the rows of ``Xs``: ``(S, M)`` (``gmb_paths_eval``) -- draws of the LATENT function.  No
        triangular pass and nothing of size M x N: ``M`` may be a whole grid.  ``ValueError`` when no paths are prepared or the
        data, theta or the factor changed since."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        M = Xs.shape[0]
        Y = np.empty((self.n_paths, M), dtype=np.float64)  # (the engine's own count: whoever prepared the set)
        self._check(self._lib.gmb_paths_eval(self._h, _ptr(Xs), M, self.D, _ptr(Y), M, GMB_HOST), "gmb_paths_eval")
        return Y

    def paths_eval_own(self, Xs, draw, grad=True):
        """Row ``m`` of ``Xs`` on draw ``draw[m]`` only (``gmb_paths_eval_own``): ``(val (M,), grad (M, D))`` -- the gradient with
        respect to the point, columns as :meth:`predict_grad` -- or ``(val, None)`` with ``grad=False``.  One call per objective
        evaluation of a Thompson search over many draws and restarts."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        M = Xs.shape[0]
        draw = np.ascontiguousarray(draw, dtype=np.int32).ravel()
        if draw.shape != (M,):
            raise ValueError(f"paths_eval_own: draw must hold one index per point ({M}), got {draw.shape}")
        val = np.empty(M, dtype=np.float64)
        g = np.empty((M, self.D), dtype=np.float64) if grad else None
        self._check(self._lib.gmb_paths_eval_own(self._h, _ptr(Xs), M, self.D, _ptr(draw), _ptr(val), _ptr(g) if grad else None, self.D,
                                                 GMB_HOST), "gmb_paths_eval_own")
        return val, g

    def paths_clear(self):
        """Drop the prepared draws and free their device buffers (``gmb_paths_clear``)."""
        self.paths_generation += 1
        self._check(self._lib.gmb_paths_clear(self._h), "gmb_paths_clear")

    # -- sparse GPs: FITC on inducing points (csrc/fitc.hpp) ---------------------------------------------------------
    def set_inducing(self, Z):
        """The inducing points of the sparse approximation (``gmb_fitc_set_inducing``): ``Z`` is ``(m, D)``, columns as ``X``.
        Needs ``set_data`` and ``set_kernel``; a later ``set_data`` / ``set_kernel`` drops them.  ``ValueError`` for a model
        outside the sparse path's scope (several outputs, categorical or linear dimensions, additive, periodic)."""
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[1] != self.D:
            raise ValueError(f"Z must be (m, {self.D}), got {Z.shape}")
        self._check(self._lib.gmb_fitc_set_inducing(self._h, _ptr(Z), Z.shape[0], Z.shape[1], GMB_HOST), "gmb_fitc_set_inducing")
        self.n_inducing = Z.shape[0]

    def fitc_evaluate(self, theta, grad: bool = True):
        """The FITC negative log marginal likelihood at ``theta`` -- ``(nlml, gradient)`` or ``nlml`` -- in O(N m^2)
        (``gmb_fitc_evaluate``).  Sets theta as ``set_theta`` does (an exact factor on this engine is stale afterwards) and
        leaves the state ``fitc_predict`` needs.  ``LinAlgError`` when one of the two m x m matrices is not positive definite."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        val = C.c_double()
        g = np.empty(self.spec.theta_size(), dtype=np.float64) if grad else None
        self._check(self._lib.gmb_fitc_evaluate(self._h, _dptr(theta), theta.size, C.byref(val), _dptr(g) if grad else None),
                    "gmb_fitc_evaluate")
        return (val.value, g) if grad else val.value

    def fitc_predict(self, Xs, with_noise=True):
        """Mean and variance of the FITC posterior at the rows of ``Xs`` against the state the last ``fitc_evaluate`` left
        (``gmb_fitc_predict``); ``ValueError`` when theta, the data or the inducing points changed since."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        M = Xs.shape[0]
        mean, var = np.empty(M, dtype=np.float64), np.empty(M, dtype=np.float64)
        self._check(self._lib.gmb_fitc_predict(self._h, _ptr(Xs), M, Xs.shape[1], int(bool(with_noise)), _ptr(mean), _ptr(var), GMB_HOST),
                    "gmb_fitc_predict")
        return mean, var

    @staticmethod
    def fitc_plan(N: int, m: int) -> dict:
        """:func:`fitc_plan` (host-only: no device needed)."""
        return fitc_plan(N, m)

    # -- GP classification: the Laplace approximation (csrc/laplace.hpp) --------------------------------------------
    def laplace_evaluate(self, theta, grad: bool = True):
        """``-log q(y | theta)`` of the Laplace approximation for the labels ``set_data`` / ``set_y`` hold (exactly 0 or 1),
        logit link -- ``(nlq, gradient)`` or ``nlq`` (``gmb_laplace_evaluate``); theta and the gradient laid out as ``evaluate``'s.
        The Newton iteration starts at 0 in every call.  Leaves the state ``laplace_predict`` needs and the exact path "not
        factored".  ``ValueError`` for other labels or a model outside the scope (additive, several outputs, periodic),
        ``LinAlgError`` when B is not positive definite, :class:`LaplaceConvergenceError` when the iteration hits a cap."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        val = C.c_double()
        g = np.empty(self.spec.theta_size(), dtype=np.float64) if grad else None
        self._check(self._lib.gmb_laplace_evaluate(self._h, _dptr(theta), theta.size, C.byref(val), _dptr(g) if grad else None),
                    "gmb_laplace_evaluate")
        return (val.value, g) if grad else val.value

    def laplace_predict(self, Xs):
        """Mean and variance of the LATENT function at the rows of ``Xs`` against the state the last ``laplace_evaluate`` left
        (``gmb_laplace_predict``; the variance without noise and jitter); ``ValueError`` when theta, the data, the labels or the
        kernel changed since, or an exact factorisation took the factor buffer."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        M = Xs.shape[0]
        mean, var = np.empty(M, dtype=np.float64), np.empty(M, dtype=np.float64)
        self._check(self._lib.gmb_laplace_predict(self._h, _ptr(Xs), M, Xs.shape[1], _ptr(mean), _ptr(var), GMB_HOST), "gmb_laplace_predict")
        return mean, var

    def laplace_info(self) -> dict:
        """The Newton iteration of the last ``laplace_evaluate``: ``iterations``, ``halvings``, ``psi``, ``step``."""
        st = LaplaceStats()
        self._check(self._lib.gmb_laplace_info(self._h, C.byref(st)), "gmb_laplace_info")
        return {"iterations": int(st.iterations), "halvings": int(st.halvings), "psi": float(st.psi), "step": float(st.step)}

    def laplace_mode(self, padded: bool = False):
        """The resident mode ``(f_hat, a_hat)`` with ``f_hat = Sigma a_hat`` (``gmb_laplace_copy_mode``); ``padded``: all
        ``N`` rounded up to 128 entries the engine keeps (0 beyond ``N``)."""
        Np = (self.N + 127) // 128 * 128
        f, a = np.empty(Np, dtype=np.float64), np.empty(Np, dtype=np.float64)
        self._check(self._lib.gmb_laplace_copy_mode(self._h, _ptr(f), _ptr(a)), "gmb_laplace_copy_mode")
        return (f, a) if padded else (f[:self.N].copy(), a[:self.N].copy())

    def set_laplace_options(self, tol: float = 1e-9, max_iter: int = 40):
        """Stop rule and iteration cap (at most 40) of ``laplace_evaluate``'s Newton iteration."""
        self._check(self._lib.gmb_laplace_set_options(self._h, float(tol), int(max_iter)), "gmb_laplace_set_options")

    def debug_laplace_symv(self, v):
        """Test door: ``Sigma v`` by the symmetric product against the resident Sigma; ``v`` has ``N`` entries, the result all
        ``N`` rounded up to 128 the kernel writes."""
        Np = (self.N + 127) // 128 * 128
        vin = np.zeros(Np, dtype=np.float64)
        vin[:self.N] = np.asarray(v, dtype=np.float64)
        out = np.empty(Np, dtype=np.float64)
        self._check(self._lib.gmb_debug_laplace_symv(self._h, _ptr(vin), _ptr(out)), "gmb_debug_laplace_symv")
        return out

    @staticmethod
    def laplace_plan(N: int) -> dict:
        """:func:`laplace_plan` (host-only: no device needed)."""
        return laplace_plan(N)

    def predict_device(self, xs_ptr: int, M: int, ldxs: int, mean_ptr: int, var_ptr: int, with_noise=True):
        self._check(
            self._lib.gmb_predict(self._h, C.c_void_p(xs_ptr), M, ldxs, int(bool(with_noise)), C.c_void_p(mean_ptr),
                                  C.c_void_p(var_ptr), GMB_DEVICE),
            "gmb_predict",
        )

    # -- introspection -----------------------------------------------------------------------------
    def set_profiling(self, on: bool):
        self._check(self._lib.gmb_set_profiling(self._h, int(bool(on))), "gmb_set_profiling")

    def timings(self) -> dict:
        t = Timings()
        self._check(self._lib.gmb_timings_get(self._h, C.byref(t)), "gmb_timings_get")
        return t.as_dict()

    #: schedules of the Cholesky (``set_chol_scheme``): by size / plain recursion / masked look-ahead / persistent tile kernel
    CHOL_BY_SIZE, CHOL_RECURSION, CHOL_LOOKAHEAD, CHOL_TILES, CHOL_RECURSION_TILE_PANELS = -1, 0, 2, 3, 4

    def set_chol_scheme(self, scheme: int) -> int:
        """Schedule of the following factorisations; returns the previous setting."""
        prev = int(self._lib.gmb_set_chol_scheme(self._h, int(scheme)))  # previous + 1, or a negative status
        if prev < 0:
            self._check(prev, "gmb_set_chol_scheme")
        return prev - 1

    #: schedules of the gradient's inverse / Sigma^-1 (``set_grad_scheme``)
    GRAD_BY_SIZE, GRAD_LAUNCH_TREE, GRAD_TILES, GRAD_FUSED = -1, 0, 1, 2

    def set_grad_scheme(self, scheme: int, lag: int = -1) -> int:
        """Schedule of the gradient's inverse and Sigma^-1 for the following evaluations (``lag``: block columns the inverse
        follows the factorisation by in the fused launch's ticket order); returns the previous setting."""
        prev = int(self._lib.gmb_set_grad_scheme(self._h, int(scheme), int(lag)))
        if prev < 0:
            self._check(prev, "gmb_set_grad_scheme")
        return prev - 1

    def debug_lose_tickets(self, n: int):
        """Fault injection (tests): the next tile factorisation never computes the tiles of tickets 0 .. n-1."""
        self._check(self._lib.gmb_debug_chol_lose_tickets(self._h, int(n)), "gmb_debug_chol_lose_tickets")

    def chol_task_trace(self, enable: int = -1):
        """Per-task stamps of the last persistent tile factorisation: ``(tiles, stamps)`` with ``tiles`` the (I, J) of every
        ticket and ``stamps`` (ntasks, 4) seconds since the first ticket (taken / contraction done / solve input ready /
        published); ``None`` when the last factorisation recorded nothing.  ``enable`` = 1 / 0 switches the stamps of the
        FOLLOWING factorisations on / off."""
        n = int(self._lib.gmb_chol_task_trace(self._h, int(enable), None, 0))
        if n <= 0:
            return None
        raw = np.zeros((n, 4), dtype=np.uint64)
        self._check(min(0, int(self._lib.gmb_chol_task_trace(self._h, -1, _ptr(raw), n))), "gmb_chol_task_trace")
        nct = (self.N + 127) // 128
        nrt = (self.N + 1 + 127) // 128
        tiles = np.array([chol_task(t, nct, nrt) for t in range(n)], dtype=np.int32)
        t0 = raw[raw > 0].min() if (raw > 0).any() else 0
        return tiles, (raw.astype(np.int64) - int(t0)) * 1e-8

    def eval_task_trace(self, with_chol: bool = True, lag: int = -1):
        """Per-task stamps of the last persistent EVALUATION launch (csrc/eval_tiles.hpp; switch them on with
        ``chol_task_trace(1)``): ``(tasks, stamps)`` with ``tasks`` an (ntasks, 3) array of (kind, I, J) in ticket order and
        ``stamps`` as in ``chol_task_trace``; ``None`` when nothing was recorded or the task count does not match."""
        n = int(self._lib.gmb_chol_task_trace(self._h, -1, None, 0))
        if n <= 0:
            return None
        nct = (self.N + 127) // 128
        nrt = (self.N + 1 + 127) // 128
        if lag < 0:
            lag = max(2, min(24, nct // 4))  # the engine's default (csrc/engine.hip: eval_tiles)
        tasks = np.array(eval_task_list(nct, nrt, with_chol, lag), dtype=np.int32)
        if len(tasks) != n:
            return None
        raw = np.zeros((n, 4), dtype=np.uint64)
        self._check(min(0, int(self._lib.gmb_chol_task_trace(self._h, -1, _ptr(raw), n))), "gmb_chol_task_trace")
        t0 = raw[raw > 0].min() if (raw > 0).any() else 0
        return tasks, (raw.astype(np.int64) - int(t0)) * 1e-8

    def copy_factor(self, r0=0, nr=None, c0=0, nc=None):
        nr = self.N if nr is None else nr
        nc = self.N if nc is None else nc
        out = np.empty((nr, nc), dtype=np.float64)
        self._check(self._lib.gmb_copy_factor(self._h, r0, nr, c0, nc, _dptr(out)), "gmb_copy_factor")
        return out

    def copy_v(self):
        out = np.empty(self.N, dtype=np.float64)
        self._check(self._lib.gmb_copy_v(self._h, _dptr(out)), "gmb_copy_v")
        return out

    def copy_alpha(self):
        """alpha = Sigma^-1 y (available after ``nlml(grad=True)``)."""
        out = np.empty(self.N, dtype=np.float64)
        self._check(self._lib.gmb_copy_alpha(self._h, _dptr(out)), "gmb_copy_alpha")
        return out

    # -- ONE GP over several GPUs (native driver, gumbi_amd/csrc/dist_driver.hpp) -----------------------------
    #: how the ranks of ``dist_*`` hold the factor (``set_dist_mode``): every rank all of it / owned block rows + panel buffers
    DIST_REPLICATED, DIST_CAPACITY = 0, 1

    def set_eval_pairs(self, mode: int) -> int:
        """Sigma^-1 tile tasks in pairs (128 x 256): -1 by size, 0 never, 1 always (same bits either way); returns the previous mode."""
        prev = int(self._lib.gmb_set_eval_pairs(self._h, int(mode)))
        if prev < 0:
            self._check(prev, "gmb_set_eval_pairs")
        return prev - 1

    def set_predict_form(self, form: int) -> int:
        """How ``predict`` forms K(X*, X) L^-T: -1 / 1 = one GEMM against the inverse factor whenever the fit's last gradient
        evaluation left it resident (tile path), 0 = always the triangular solve; returns the previous mode."""
        prev = int(self._lib.gmb_set_predict_form(self._h, int(form)))
        if prev < 0:
            self._check(prev, "gmb_set_predict_form")
        return prev - 1

    def reserve(self, gradient: bool = True, M: int = 0):
        """Allocate now what the following factorisation / gradient / prediction of ``M`` points would allocate on first use."""
        self._check(self._lib.gmb_reserve(self._h, int(bool(gradient)), int(M)), "gmb_reserve")

    def debug_assume_factored(self):
        """Timing tools only: the last factorisation counts as valid whatever it produced (``gmb_debug_assume_factored``)."""
        self._check(self._lib.gmb_debug_assume_factored(self._h), "gmb_debug_assume_factored")

    def set_dist_mode(self, mode: int) -> int:
        """Replicated (0) or capacity (1) mode of the multi-GPU driver for the following ``dist_factorize``; returns the previous mode."""
        prev = int(self._lib.gmb_dist_set_mode(self._h, int(mode)))
        if prev < 0:
            self._check(prev, "gmb_dist_set_mode")
        return prev

    def resident_bytes(self, peak: bool = False) -> int:
        """Device bytes the engine holds through its own allocations (``peak``: the largest value so far)."""
        return int(self._lib.gmb_resident_bytes(self._h, int(bool(peak))))

    def dist_factorize(self, comm, panel_blocks: int = 0):
        """Collective: ``gmb_factorize`` over the ranks of ``comm`` (a :class:`gumbi_amd.distributed` comm)."""
        self._check(self._lib.gmb_dist_factorize(self._h, comm.handle, int(panel_blocks)), "gmb_dist_factorize")

    def dist_nlml(self, comm, grad: bool = False):
        val = C.c_double()
        if not grad:
            self._check(self._lib.gmb_dist_nlml(self._h, comm.handle, C.byref(val), None), "gmb_dist_nlml")
            return val.value
        g = np.empty(self.spec.theta_size(), dtype=np.float64)
        self._check(self._lib.gmb_dist_nlml(self._h, comm.handle, C.byref(val), _dptr(g)), "gmb_dist_nlml")
        return val.value, g

    def dist_predict(self, comm, Xs, with_noise=True):
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError(f"points_array must be (M, {self.D}), got {Xs.shape}")
        M = Xs.shape[0]
        mean = np.empty(M, dtype=np.float64)
        var = np.empty(M, dtype=np.float64)
        self._check(self._lib.gmb_dist_predict(self._h, comm.handle, _ptr(Xs), M, Xs.shape[1], int(bool(with_noise)),
                                               _ptr(mean), _ptr(var), GMB_HOST), "gmb_dist_predict")
        return mean, var

    # -- block-level operations (device pointers) --------------------------------------------------------
    def blk_potrf(self, a_ptr, lda, nvalid, dinv16_ptr, logdet_ptr=0, info_ptr=0):
        """Factor a 128 x 128 block in place; ``dinv16_ptr`` (8 x 256 doubles) receives the inverses of
        its 16 x 16 diagonal sub-blocks, the operand of :meth:`blk_trsm` / :meth:`blk_invert`."""
        self._check(self._lib.gmb_blk_potrf(self._h, C.c_void_p(a_ptr), lda, nvalid,
                                            C.c_void_p(dinv16_ptr) if dinv16_ptr else None,
                                            C.c_void_p(logdet_ptr) if logdet_ptr else None,
                                            C.c_void_p(info_ptr) if info_ptr else None), "gmb_blk_potrf")

    def blk_invert(self, l_ptr, lda, nvalid, dinv16_ptr, inv_ptr):
        self._check(self._lib.gmb_blk_invert(self._h, C.c_void_p(l_ptr), lda, nvalid, C.c_void_p(dinv16_ptr),
                                             C.c_void_p(inv_ptr)), "gmb_blk_invert")

    def blk_covariance(self, out_ptr, ldo):
        """The covariance build alone into a caller's device buffer (lower-triangle tiles, y row, padding)."""
        self._check(self._lib.gmb_blk_covariance(self._h, C.c_void_p(out_ptr), ldo), "gmb_blk_covariance")

    def blk_trsm(self, b_ptr, ldb, nrows, l_ptr, ldl, dinv16_ptr, nvalid=128):
        """B <- B inv(L)^T in place on ``nrows`` (multiple of 16) rows."""
        self._check(self._lib.gmb_blk_trsm(self._h, C.c_void_p(b_ptr), ldb, nrows, C.c_void_p(l_ptr), ldl,
                                           C.c_void_p(dinv16_ptr), nvalid), "gmb_blk_trsm")

    def blk_gemm_nt(self, c_ptr, ldc, a_ptr, lda, b_ptr, ldb, m, n, k, alpha, beta, tri=0, tri_shift=0):
        self._check(self._lib.gmb_blk_gemm_nt(self._h, C.c_void_p(c_ptr), ldc, C.c_void_p(a_ptr), lda,
                                              C.c_void_p(b_ptr), ldb, m, n, k, alpha, beta, tri, tri_shift),
                    "gmb_blk_gemm_nt")

    def blk_gemm_ex(self, c_ptr, a_ptr, b_ptr, ldc, lda, ldb, m, n, k, alpha, beta, tri=0, tri_off=0, nblk_stride=1,
                    cblk_stride=0, klo_m=0, klo_n=0, khi_n=0, krow_off=0, krow_stride=0, variant=-1, staging=-1, pfc=-1,
                    order=-1, strip=-1):
        """One GEMM launch with every field of its descriptor given and the launcher's choices pinned (-1 = left to it);
        ``c_ptr == b_ptr`` selects the in-place form.  Returns what ran: ``dict(variant, dma, pfc, in_place, order, strip,
        grid)``; raises ``ValueError`` for a combination the launcher could not produce (nothing is launched)."""
        d = GemmDesc(ldc, lda, ldb, m, n, k, alpha, beta, tri, tri_off, nblk_stride, cblk_stride, klo_m, klo_n, khi_n,
                     krow_off, krow_stride, variant, staging, pfc, order, strip)
        w = C.c_int32(0)
        self._check(self._lib.gmb_blk_gemm_ex(self._h, C.c_void_p(c_ptr), C.c_void_p(a_ptr), C.c_void_p(b_ptr),
                                              C.byref(d), C.byref(w)), "gmb_blk_gemm_ex")
        w = w.value
        return dict(variant=w & 3, dma=(w >> 2) & 1, pfc=(w >> 3) & 1, in_place=(w >> 4) & 1, order=(w >> 5) & 3,
                    strip=(w >> 8) & 0xFF, grid=(w >> 16) & 0x7FFF)

    def blk_gemm_splitk(self, c_ptr, ldc, a_ptr, lda, b_ptr, ldb, m, n, k, alpha, beta, tri=0, slices=-1):
        """The split-k f64 GEMM on device blocks (``gmb_blk_gemm_splitk``; ``slices`` -1 = by the rule, >= 1 = pinned): returns the
        number of slices that ran, also kept in ``splitk_slices_used`` -- 0 after a refusal (``ValueError``, nothing launched:
        bad sizes, or a pinned ``slices`` that leaves a slice empty)."""
        used = C.c_int32(-1)
        rc = self._lib.gmb_blk_gemm_splitk(self._h, C.c_void_p(c_ptr), ldc, C.c_void_p(a_ptr), lda, C.c_void_p(b_ptr), ldb, m, n, k,
                                           float(alpha), float(beta), int(tri), int(slices), C.byref(used))
        self.splitk_slices_used = int(used.value)
        self._check(rc, "gmb_blk_gemm_splitk")
        return self.splitk_slices_used


def chol_task(t: int, nct: int, nrt: int):
    """Ticket ``t`` of the persistent tile Cholesky -> its tile (I, J) (host-side enumeration shared with the kernel)."""
    lib = load_library()
    i, j = C.c_int32(), C.c_int32()
    n = lib.gmb_debug_chol_task(int(t), int(nct), int(nrt), C.byref(i), C.byref(j))
    if n < 0:
        raise ValueError("gmb_debug_chol_task: bad arguments")
    return i.value, j.value


def eval_task_list(nct: int, nrt: int, with_chol: bool = True, lag: int = 1, pairs: bool = False) -> list:
    """[(kind, I, J), ...] of the persistent evaluation launch in ticket order (host-only; kind 0 = Cholesky tile,
    1 = tile of U = L^-T, 2 = tile of Sigma^-1, 3 = alpha (and v) of block row I).  ``pairs``: the Sigma^-1 tasks as the launch
    lists them for large matrices -- ``(2, I, J + 0x4000)`` stands for the two tiles (I, J) and (I, J + 1)."""
    lib = load_library()
    mode = int(bool(with_chol)) | (2 if pairs else 0)
    n = lib.gmb_debug_eval_tasks(int(nct), int(nrt), mode, int(lag), None, 0)
    if n < 0:
        raise ValueError("gmb_debug_eval_tasks: bad arguments")
    buf = (C.c_uint32 * n)()
    lib.gmb_debug_eval_tasks(int(nct), int(nrt), mode, int(lag), buf, n)
    return [(w >> 30, (w >> 15) & 0x7FFF, w & 0x7FFF) for w in buf]


def group_tasks(offsets, chunk=None) -> list:
    """[(group, first point, count), ...]: the tasks ``gmb_predict_groups`` runs over for these offsets (host-only), every count
    at most ``chunk`` (``None``: :data:`GROUP_CHUNK`), in ascending group order, then ascending first point.  ``ValueError`` for
    offsets that do not start at 0 or do not increase strictly."""
    lib = load_library()
    offsets = np.ascontiguousarray(np.asarray(offsets).ravel(), dtype=np.int64)
    G = offsets.shape[0] - 1
    chunk = 0 if chunk is None else int(chunk)
    n = lib.gmb_debug_group_tasks(_ptr(offsets), G, chunk, None, 0) if G >= 1 else GMB_EINVAL
    if n < 0:
        raise ValueError("gmb_debug_group_tasks: offsets must start at 0 and increase strictly (no empty group)")
    buf = np.empty((n, 3), dtype=np.int64)
    lib.gmb_debug_group_tasks(_ptr(offsets), G, chunk, _ptr(buf), n)
    return [tuple(int(v) for v in row) for row in buf]


def slope_tile_rows(Np: int, Dc: int) -> int:
    """Test points per M-tile of ``gmb_predict_slope`` behind ``Np`` padded training points with ``Dc`` differentiable columns
    (host-only)."""
    n = int(load_library().gmb_debug_slope_tile_rows(int(Np), int(Dc)))
    if n < 0:
        raise ValueError(f"gmb_debug_slope_tile_rows: Np = {Np}, Dc = {Dc}")
    return n


def design_plan(Np: int, M: int, R: int) -> dict:
    """The plan of ``gmb_design_batch`` behind ``Np`` padded training points (host-only): the sizes, the point tiles
    ``(first stacked index, count, padded count, first column of D)`` and the step kernel's column chunks ``(first, end)``.
    ``ValueError`` for a request the call refuses."""
    lib = load_library()
    n = int(lib.gmb_debug_design_plan(int(Np), int(M), int(R), None, 0))
    if n < 0:
        raise ValueError(f"gmb_debug_design_plan: Np = {Np}, M = {M}, R = {R} is refused (code {-n})")
    buf = np.empty(n, dtype=np.int64)
    lib.gmb_debug_design_plan(int(Np), int(M), int(R), _ptr(buf), n)
    keys = ("Mc", "ld", "mt_max", "mt", "ntile", "nchunk", "chunk", "rows", "own_bytes")
    plan = {k: int(v) for k, v in zip(keys, buf)}
    h, nt = len(keys), int(buf[4])
    plan["tiles"] = [tuple(int(v) for v in buf[h + 4 * t:h + 4 * t + 4]) for t in range(nt)]
    plan["chunks"] = [tuple(int(v) for v in buf[h + 4 * nt + 2 * c:h + 4 * nt + 2 * c + 2]) for c in range(plan["nchunk"])]
    return plan


def batch_plan(N: int, Np: int, B: int, q: int) -> dict:
    """The plan of ``gmb_predict_batches`` for ``B`` batches of ``q`` points behind ``N`` training points padded to ``Np``
    (host-only): ``bt`` batches per full M-tile, ``ntile``, ``mt`` rows of the prediction workspace, the ``slots`` the partials are
    sized for, the ``unit`` of a chunk's length, and the tiles ``(first batch, batches, points, padded points, chunk length,
    chunks)``.  ``ValueError`` for a request the call refuses."""
    lib = load_library()
    n = int(lib.gmb_debug_batch_plan(int(N), int(Np), int(B), int(q), None, 0))
    if n < 0:
        raise ValueError(f"gmb_debug_batch_plan: N = {N}, Np = {Np}, B = {B}, q = {q} is refused (code {-n})")
    buf = np.empty(n, dtype=np.int64)
    lib.gmb_debug_batch_plan(int(N), int(Np), int(B), int(q), _ptr(buf), n)
    keys = ("bt", "ntile", "mt", "slots", "unit")
    plan = {k: int(v) for k, v in zip(keys, buf)}
    h = len(keys)
    plan["tiles"] = [tuple(int(v) for v in buf[h + 6 * t:h + 6 * t + 6]) for t in range(plan["ntile"])]
    return plan


def paths_plan(N: int, F: int, M: int, S: int, nacc: int = 2) -> dict:
    """The plan of the pathwise calls for ``S`` draws of ``F`` features at ``M`` points behind ``N`` training points (host-only):
    ``Sp`` (S padded to 16), ``draw_blocks`` of 64, ``N4`` / ``F4`` (the two parts of the contraction index, padded to 4), ``mt``
    rows of the largest M-tile, ``ntile``, the doubles of the all-draws partials and of the own-draw partials for ``nacc``
    accumulators, and the tiles ``(first point, points, padded points, point tiles of 16, chunk length, chunks, own-draw chunk
    length, own-draw chunks)``.  ``ValueError`` for a request the calls refuse."""
    lib = load_library()
    n = int(lib.gmb_debug_paths_plan(int(N), int(F), int(M), int(S), int(nacc), None, 0))
    if n < 0:
        raise ValueError(f"gmb_debug_paths_plan: N = {N}, F = {F}, M = {M}, S = {S} is refused (code {-n})")
    buf = np.empty(n, dtype=np.int64)
    lib.gmb_debug_paths_plan(int(N), int(F), int(M), int(S), int(nacc), _ptr(buf), n)
    keys = ("Sp", "draw_blocks", "N4", "F4", "mt", "ntile", "part_doubles", "own_part_doubles")
    plan = {k: int(v) for k, v in zip(keys, buf)}
    h = len(keys)
    plan["tiles"] = [tuple(int(v) for v in buf[h + 8 * t:h + 8 * t + 8]) for t in range(plan["ntile"])]
    return plan


def fitc_plan(N: int, m: int) -> dict:
    """The plan of ``gmb_fitc_evaluate`` for ``N`` observations and ``m`` inducing points (host-only): the padded sizes, the
    column tiles of X ``(first column, count, padded count)`` and the bytes of the call's buffer list for one input column, in
    three parts -- ``bytes_fixed`` (a function of m alone), ``bytes_blocks`` (the m x tile blocks) and ``bytes_columns`` (the
    per-column vectors, O(N)).  ``ValueError`` for a request the call refuses."""
    lib = load_library()
    n = int(lib.gmb_debug_fitc_plan(int(N), int(m), None, 0))
    if n < 0:
        raise ValueError(f"gmb_debug_fitc_plan: N = {N}, m = {m} is refused (code {-n})")
    buf = np.empty(n, dtype=np.int64)
    lib.gmb_debug_fitc_plan(int(N), int(m), _ptr(buf), n)
    keys = ("Np", "mp", "mr", "tile_rows", "tmax", "ntile", "col_blocks", "bytes_fixed", "bytes_blocks", "bytes_columns")
    plan = {k: int(v) for k, v in zip(keys, buf)}
    h = len(keys)
    plan["tiles"] = [tuple(int(v) for v in buf[h + 3 * t:h + 3 * t + 3]) for t in range(plan["ntile"])]
    return plan


def laplace_plan(N: int) -> dict:
    """The plan of ``gmb_laplace_evaluate`` for ``N`` observations (host-only): padded sizes, block rows ``nt``, the workspace
    ``slots`` of the symmetric product, the partial sets of the likelihood pass, ``bytes_state`` of the path's own buffers, and
    per block row the offsets (in doubles) of the ``nt + 1`` parts its sum adds, in order (``row_terms``)."""
    lib = load_library()
    n = int(lib.gmb_debug_laplace_plan(int(N), None, 0))
    if n < 0:
        raise ValueError(f"gmb_debug_laplace_plan: N = {N} is refused (code {-n})")
    buf = np.empty(n, dtype=np.int64)
    lib.gmb_debug_laplace_plan(int(N), _ptr(buf), n)
    keys = ("Np", "Nr", "nt", "slots", "lik_blocks", "slot_doubles", "lik_sums", "bytes_state")
    plan = {k: int(v) for k, v in zip(keys, buf)}
    h, nt = len(keys), plan["nt"]
    plan["row_terms"] = [[int(v) for v in buf[h + R * (nt + 1):h + (R + 1) * (nt + 1)]] for R in range(nt)]
    return plan


def chol_task_count(nct: int, nrt: int) -> int:
    return int(load_library().gmb_debug_chol_task(-1, int(nct), int(nrt), None, None))


def gemm_tile_list(mt, nt, bm=128, bn=128, k=1024, tri=0, tri_off=0, nblk_stride=1, klo_n=0, khi_n=0, order=0, strip=0):
    """(grid, [(block, tm, tn), ...]) of one GEMM launch as the kernel enumerates it (host-only)."""
    lib = load_library()
    args = [int(v) for v in (mt, nt, bm, bn, k, tri, tri_off, nblk_stride, klo_n, khi_n, order, strip)]
    grid = C.c_int32()
    n = lib.gmb_debug_tile_list(*args, None, 0, C.byref(grid))
    if n < 0:
        raise ValueError("gmb_debug_tile_list: bad arguments")
    buf = (C.c_int32 * (3 * n))()
    lib.gmb_debug_tile_list(*args, buf, n, C.byref(grid))
    arr = np.frombuffer(buf, dtype=np.int32).reshape(n, 3)
    return int(grid.value), [tuple(int(v) for v in row) for row in arr]


def cov_grid(ti, tj, strip=1, tri_grid=1, row_first=0, row_stride=0, keep_order=1):
    """(grid, array of (block, tile row, tile column)) of one covariance-build launch as cov_tile_kernel enumerates
    it (host-only)."""
    lib = load_library()
    args = [int(v) for v in (ti, tj, strip, tri_grid, row_first, row_stride, keep_order)]
    grid = C.c_int64()
    n = lib.gmb_debug_cov_grid(*args, None, 0, C.byref(grid))
    if n < 0:
        raise ValueError("gmb_debug_cov_grid: bad arguments")
    buf = (C.c_int32 * max(3 * n, 1))()
    lib.gmb_debug_cov_grid(*args, buf, n, C.byref(grid))
    return int(grid.value), np.frombuffer(buf, dtype=np.int32)[: 3 * n].reshape(n, 3).copy()


def dist_plan(N: int, rank: int, world: int, panel_blocks: int = 0) -> list:
    """The schedule rank ``rank`` of ``world`` executes in ``gmb_dist_factorize`` (host-only; no device needed)."""
    lib = load_library()
    n = lib.gmb_dist_plan(int(N), int(rank), int(world), int(panel_blocks), None, 0)
    if n < 0:
        raise ValueError(f"gmb_dist_plan: bad arguments (N={N}, rank={rank}, world={world})")
    buf = (DistStep * n)()
    lib.gmb_dist_plan(int(N), int(rank), int(world), int(panel_blocks), buf, n)
    return [st.as_dict() for st in buf]


def ls_limits(X, ard: bool, device: int = 0):
    """Minimum non-zero and maximum pairwise distance per group (``gmb_ls_limits``)."""
    lib = load_library()
    X = np.ascontiguousarray(X, dtype=np.float64)
    n_groups = X.shape[1] if ard else 1
    lo = np.empty(n_groups)
    hi = np.empty(n_groups)
    rc = lib.gmb_ls_limits(int(device), _dptr(X), X.shape[0], X.shape[1], X.shape[1], int(bool(ard)), _dptr(lo),
                           _dptr(hi))
    if rc == GMB_ENODEVICE:
        raise GumbiHipError("gmb_ls_limits: no HIP device (no CPU fallback exists)")
    if rc != GMB_OK:
        raise GumbiHipError(f"gmb_ls_limits failed with status {rc}")
    return lo, hi


def mfma_f64_sustained(device: int = 0, seconds: float = 1.0) -> dict:
    """The register-only MFMA loop run back to back for ``seconds``: mean / worst launch rate (TFLOP/s), the
    shader clock it ran at (MHz) and the number of launches (``gmb_mfma_f64_sustained``)."""
    mean, worst, mhz, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
    rc = load_library().gmb_mfma_f64_sustained(int(device), float(seconds), C.byref(mean), C.byref(worst), C.byref(mhz),
                                                C.byref(n))
    if rc != GMB_OK:
        raise GumbiHipError(f"gmb_mfma_f64_sustained failed with status {rc}")
    return {"tflops_mean": mean.value, "tflops_min": worst.value, "shader_mhz": mhz.value, "launches": int(n.value),
            "seconds": float(seconds)}


def mfma_f64_peak(device: int = 0):
    """(TFLOP/s, shader cycles per MFMA as seen by one wave) from ``gmb_mfma_f64_peak``."""
    out, cyc = C.c_double(), C.c_double()
    rc = load_library().gmb_mfma_f64_peak(int(device), C.byref(out), C.byref(cyc))
    if rc != GMB_OK:
        raise GumbiHipError(f"gmb_mfma_f64_peak failed with status {rc}")
    return out.value, cyc.value
