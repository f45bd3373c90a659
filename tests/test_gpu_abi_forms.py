"""The call forms ``include/gumbi_hip.h`` promises on every data-carrying entry point and ``gumbi_amd/engine.py`` never makes:
caller arrays in device memory (``GMB_DEVICE`` -- the form ``bench.py`` times), leading dimensions larger than the row, and
more than one M-tile of ``gmb_predict`` / ``gmb_predict_grad`` / ``gmb_predict_with_grad``.  Needs a GPU (``-m gpu``).

The four forms: packed host (``engine.py``'s own call, the one the rest of the suite pins), strided host, packed device, strided
device -- ``ld = D + 3`` for arrays of width D, ``M + 5`` (``M + 3`` for Z, ``M + 7`` for Y) for arrays of width M.  The C functions
are called through ``eng._lib`` / ``eng._h`` with the buffers of tests/abi_forms.py: input padding is NaN (a read past column D or
row M poisons the result), output padding and at least 64 elements behind every output's last row carry a fixed bit pattern (a
write past column D, or of the padded row count, changes it).

Every form is checked twice:

(a) against the project's float64 references at the bars the project states --
    ``O.predict(direct)``: mean 1e-10 relative, variance 1e-11 absolute (tests/test_gpu_parity.py);
    ``grad_reference.mean_grad`` / ``var_grad_reference.mean_var_grad``: 1e-8 max|G_ref| (tests/test_gpu_predict_grad.py);
    ``JointOracleEngine``: covariance 1e-9 absolute, mean 1e-8 relative, well-conditioned draws 1e-8 max|Y_oracle|
    (tests/test_gpu_joint.py); NLML 1e-10 relative; behind an append L, v, NLML 1e-10, mean 1e-8, variance 1e-9
    (tests/test_gpu_append.py);
(b) bit-identical to the packed host call on the same engine in the same state: all four forms feed the same packed device
    buffers and the same launches, and the header promises "the same bits call after call".

The measured worst errors are printed per test (``ABI-FORMS ...``).
"""
import ctypes as C
import functools
from typing import NamedTuple

import numpy as np
import pytest

import abi_forms as AF
import grad_reference as GR
import var_grad_reference as VR
from oracle import gp_oracle as O
from test_gpu_parity import GOLD, golden_spec, kspec, make_engine, rel
from test_gpu_predict_grad import points, table
from test_gpu_var_grad import M_TILE, case as var_grad_case, oracle_predict

pytestmark = pytest.mark.gpu

NAN = np.nan


# ---- forms and buffers ---------------------------------------------------------------------------------------------------------
class Form(NamedTuple):
    name: str
    device: bool
    strided: bool

    def ld(self, width, pad):
        return width + pad if self.strided else width

    @property
    def memspace(self):
        from gumbi_amd.engine import GMB_DEVICE, GMB_HOST

        return GMB_DEVICE if self.device else GMB_HOST


PACKED_HOST, STRIDED_HOST, PACKED_DEVICE, STRIDED_DEVICE = FORMS = (
    Form("packed host", False, False), Form("strided host", False, True),
    Form("packed device", True, False), Form("strided device", True, True))
STRIDED = (STRIDED_HOST, STRIDED_DEVICE)


def sync():
    """The engine runs on its own stream: torch's writes (copies to the device, fills) are finished before an engine call."""
    import torch

    torch.cuda.synchronize()


class Buf:
    """One caller array (a buffer of tests/abi_forms.py) in host memory or, as a torch tensor, in device memory."""

    def __init__(self, host, device, ld=None):
        self.host, self.ld, self.dev = host, ld, None
        if device:
            import torch

            self.dev = torch.from_numpy(host).to("cuda:0")

    @property
    def ptr(self):
        return C.c_void_p(self.dev.data_ptr() if self.dev is not None else self.host.ctypes.data)

    def fetch(self):
        return self.dev.cpu().numpy() if self.dev is not None else self.host

    def poison(self):
        """Overwrite the caller's array with NaN: what the library does afterwards must not depend on it."""
        if self.dev is not None:
            self.dev.fill_(NAN)
        else:
            self.host[...] = NAN


def mat_in(a, form, pad):
    ld = form.ld(a.shape[1], pad)
    return Buf(AF.embed(a, ld, NAN), form.device, ld)


def vec_in(v, form):
    return Buf(AF.padded(len(v), AF.SPARE, NAN, values=v), form.device)


def mat_out(rows, width, form, pad):
    ld = form.ld(width, pad)
    return Buf(AF.embed(np.full((rows, width), AF.FILL), ld, AF.FILL), form.device, ld)


def vec_out(n, form):
    return Buf(AF.padded(n, AF.SPARE, AF.FILL), form.device)


def take(buf, rows, width, what):
    """The rows x width window of an output matrix; its padding columns and everything behind row ``rows`` untouched, every
    element of the window written."""
    h = buf.fetch()
    assert AF.untouched(h, width, AF.FILL_BITS, rows=rows), f"{what}: written outside its {rows} x {width} window (ld = {buf.ld})"
    out = h[:rows, :width].copy()
    assert not np.any(out.view(np.uint64) == AF.FILL_BITS), f"{what}: elements of the window were not written"
    return out


def take_vec(buf, n, what):
    h = buf.fetch()
    assert AF.untouched(h, n, AF.FILL_BITS), f"{what}: written behind its {n} elements"
    out = h[:n].copy()
    assert not np.any(out.view(np.uint64) == AF.FILL_BITS), f"{what}: elements were not written"
    return out


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    differ = int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
    assert differ == 0, f"{what}: {differ} of {got.size} elements differ from the packed host call (max |diff| {np.nanmax(np.abs(got - want)):.3e})"


# ---- the raw calls ---------------------------------------------------------------------------------------------------------------
def call_set_data(eng, X, y, form):
    N, D = X.shape
    x, yy = mat_in(X, form, 3), vec_in(y, form)
    sync()
    eng._check(eng._lib.gmb_set_data(eng._h, x.ptr, N, D, x.ld, yy.ptr, form.memspace), f"gmb_set_data ({form.name})")
    eng.N, eng.D = N, D
    return x, yy


def call_set_y(eng, y, form):
    yy = vec_in(y, form)
    sync()
    eng._check(eng._lib.gmb_set_y(eng._h, yy.ptr, form.memspace), f"gmb_set_y ({form.name})")
    return (yy,)


def call_append(eng, Xn, yn, form):
    x, yy = mat_in(Xn, form, 3), vec_in(yn, form)
    sync()
    rc = eng._lib.gmb_append(eng._h, x.ptr, Xn.shape[0], x.ld, yy.ptr, form.memspace)
    eng.N = int(eng._lib.gmb_num_obs(eng._h))
    eng._check(rc, f"gmb_append ({form.name})")
    return x, yy


def call_predict(eng, Xs, form, with_noise=True):
    M = Xs.shape[0]
    what = f"gmb_predict ({form.name})"
    x, mean, var = mat_in(Xs, form, 3), vec_out(M, form), vec_out(M, form)
    sync()
    eng._check(eng._lib.gmb_predict(eng._h, x.ptr, M, x.ld, int(with_noise), mean.ptr, var.ptr, form.memspace), what)
    return take_vec(mean, M, what + " mean"), take_vec(var, M, what + " var")


def call_predict_grad(eng, Xs, form, pad_xs=3, pad_g=3):
    M, D = Xs.shape
    what = f"gmb_predict_grad ({form.name}, ldxs = D + {pad_xs}, ldg = D + {pad_g})"
    x, g = mat_in(Xs, form, pad_xs), mat_out(M, D, form, pad_g)
    sync()
    eng._check(eng._lib.gmb_predict_grad(eng._h, x.ptr, M, x.ld, g.ptr, g.ld, form.memspace), what)
    return take(g, M, D, what)


def call_predict_with_grad(eng, Xs, form, pad_xs=3, pad_g=3, with_noise=True):
    M, D = Xs.shape
    what = f"gmb_predict_with_grad ({form.name}, ldxs = D + {pad_xs}, ldg = D + {pad_g})"
    x, mean, var = mat_in(Xs, form, pad_xs), vec_out(M, form), vec_out(M, form)
    dm, dv = mat_out(M, D, form, pad_g), mat_out(M, D, form, pad_g)
    sync()
    eng._check(eng._lib.gmb_predict_with_grad(eng._h, x.ptr, M, x.ld, int(with_noise), mean.ptr, var.ptr, dm.ptr, dv.ptr, dm.ld,
                                              form.memspace), what)
    return (take_vec(mean, M, what + " mean"), take_vec(var, M, what + " var"), take(dm, M, D, what + " dmean"),
            take(dv, M, D, what + " dvar"))


def call_predict_joint(eng, Xs, form, with_noise, jitter):
    M = Xs.shape[0]
    what = f"gmb_predict_joint ({form.name})"
    x, mean, cov = mat_in(Xs, form, 3), vec_out(M, form), mat_out(M, M, form, 5)
    sync()
    eng._check(eng._lib.gmb_predict_joint(eng._h, x.ptr, M, x.ld, int(with_noise), float(jitter), mean.ptr, cov.ptr, cov.ld,
                                          form.memspace), what)
    return take_vec(mean, M, what + " mean"), take(cov, M, M, what + " cov")


def call_draw_joint(eng, Xs, Z, form, with_noise, jitter, want_mean):
    M, S = Xs.shape[0], Z.shape[0]
    what = f"gmb_draw_joint ({form.name}, S = {S}, mean {'requested' if want_mean else 'NULL'})"
    x, z, yy = mat_in(Xs, form, 3), mat_in(Z, form, 3), mat_out(S, M, form, 7)
    mean = vec_out(M, form) if want_mean else None
    sync()
    eng._check(eng._lib.gmb_draw_joint(eng._h, x.ptr, M, x.ld, int(with_noise), float(jitter), z.ptr, S, z.ld, yy.ptr, yy.ld,
                                       mean.ptr if want_mean else None, form.memspace), what)
    return take(yy, S, M, what + " Y"), (take_vec(mean, M, what + " mean") if want_mean else None)


def prepare(eng, theta, fit):
    """The two sources of V and alpha: behind ``factorize`` the triangular solve and back substitution, behind
    ``evaluate(theta)`` the product with the inverse factor and the gradient evaluation's alpha."""
    if fit:
        eng.evaluate(theta, grad=True)
    else:
        eng.factorize()


def grad_err(got, ref):
    return float(np.max(np.abs(got - ref))) / float(np.max(np.abs(ref)))


# ---- 1. data in ------------------------------------------------------------------------------------------------------------------
#: three block columns with a ragged last one; D = 1: the 8-byte-wide 2-D copy
DATA_MODELS = [("Matern52", 300, 3), ("ExpQuad", 300, 1)]


@pytest.mark.parametrize("kind,N,d", DATA_MODELS)
def test_set_data_in_every_form(gpu, kind, N, d):
    from gumbi_amd.engine import Engine

    spec, theta, X, y = table(N, d, kind)
    nlml_o = O.nlml(spec, theta, X, y, dist_mode="direct")
    with make_engine(spec, theta, X, y) as base:
        base.factorize()
        L0, v0, n0 = np.tril(base.copy_factor()), base.copy_v(), base.nlml()
    err = abs(n0 - nlml_o) / abs(nlml_o)
    print(f"ABI-FORMS set_data {kind} N={N} d={d}: nlml vs oracle {err:.2e} (bar 1e-10)")
    assert err <= 1e-10
    for form in FORMS:
        with Engine(0) as eng:
            for buf in call_set_data(eng, X, y, form):
                buf.poison()  # the library never retains a caller pointer
            sync()
            eng.set_kernel(kspec(spec))
            eng.set_theta(theta)
            eng.factorize()
            same_bits(np.tril(eng.copy_factor()), L0, f"set_data ({form.name}): factor")
            same_bits(eng.copy_v(), v0, f"set_data ({form.name}): v")
            same_bits(np.float64(eng.nlml()), np.float64(n0), f"set_data ({form.name}): nlml")
            assert abs(eng.nlml() - nlml_o) <= 1e-10 * abs(nlml_o)


@pytest.mark.parametrize("kind,N,d", DATA_MODELS)
def test_set_y_from_device_memory(gpu, kind, N, d):
    spec, theta, X, y = table(N, d, kind)
    y2 = np.cos(3.0 * y) + 0.1 * y[::-1]
    nlml_o = O.nlml(spec, theta, X, y2, dist_mode="direct")
    with make_engine(spec, theta, X, y) as host, make_engine(spec, theta, X, y) as dev:
        host.factorize()
        dev.factorize()
        host.set_y(y2)
        (buf,) = call_set_y(dev, y2, PACKED_DEVICE)
        assert not dev.factor_is_current()
        buf.poison()
        sync()
        host.factorize()
        dev.factorize()
        same_bits(np.tril(dev.copy_factor()), np.tril(host.copy_factor()), "set_y (device): factor")
        same_bits(dev.copy_v(), host.copy_v(), "set_y (device): v")
        same_bits(np.float64(dev.nlml()), np.float64(host.nlml()), "set_y (device): nlml")
        err = abs(dev.nlml() - nlml_o) / abs(nlml_o)
    print(f"ABI-FORMS set_y {kind} N={N} d={d}: nlml vs oracle {err:.2e} (bar 1e-10)")
    assert err <= 1e-10


@functools.lru_cache(maxsize=None)
def appended(kind, N, d, K):
    """The table of N + K, 77 test points and the oracle at N + K."""
    spec, theta, X, y = table(N + K, d, kind)
    Xs = points(X, 77, list(range(d)), seed=5)
    L, v = O.factorize(spec, theta, X, y, dist_mode="direct")
    return spec, theta, X, y, Xs, L, v, O.nlml(spec, theta, X, y, dist_mode="direct"), O.predict(spec, theta, X, y, Xs, dist_mode="direct")


@pytest.mark.parametrize("K", [20, 100])  # 300 + 20 keeps the padded size (384); 300 + 100 crosses it: the factor is re-laid
@pytest.mark.parametrize("kind,N,d", DATA_MODELS)
def test_append_in_the_strided_forms(gpu, kind, N, d, K):
    spec, theta, X, y, Xs, L_o, v_o, nlml_o, (mu_o, var_o) = appended(kind, N, d, K)
    with make_engine(spec, theta, X[:N], y[:N]) as twin:
        twin.factorize()
        twin.append(X[N:], y[N:])
        L0, v0, n0 = np.tril(twin.copy_factor()), twin.copy_v(), twin.nlml()
        mu0, var0 = twin.predict(Xs)
    for form in STRIDED:
        with make_engine(spec, theta, X[:N], y[:N]) as eng:
            eng.factorize()
            for buf in call_append(eng, X[N:], y[N:], form):
                buf.poison()
            sync()
            assert eng.N == N + K and eng.factor_is_current()
            mu, var = eng.predict(Xs)
            L, v, n = np.tril(eng.copy_factor()), eng.copy_v(), eng.nlml()
        errs = (rel(L, L_o), rel(v, v_o), abs(n - nlml_o) / abs(nlml_o), rel(mu, mu_o), float(np.max(np.abs(var - var_o))))
        print(f"ABI-FORMS append {kind} {N}+{K} d={d} ({form.name}): L {errs[0]:.2e} v {errs[1]:.2e} nlml {errs[2]:.2e} (bars 1e-10) "
              f"mean {errs[3]:.2e} (1e-8) var {errs[4]:.2e} (1e-9)")
        assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-10 and errs[3] <= 1e-8 and errs[4] <= 1e-9
        same_bits(L, L0, f"append ({form.name}): factor")
        same_bits(v, v0, f"append ({form.name}): v")
        same_bits(np.float64(n), np.float64(n0), f"append ({form.name}): nlml")
        same_bits(mu, mu0, f"append ({form.name}): predicted mean")
        same_bits(var, var0, f"append ({form.name}): predicted variance")


# ---- 2. diagonal prediction, one tile ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_tile():
    spec, theta, X, y = table(300, 3, "Matern52")
    return spec, theta, X, y, points(X, 333, [0, 1, 2])


@functools.lru_cache(maxsize=None)
def one_tile_refs():
    spec, theta, X, y, Xs = one_tile()
    mu, var = O.predict(spec, theta, X, y, Xs, with_noise=True, dist_mode="direct")
    return mu, var, GR.mean_grad(spec, theta, X, y, Xs), VR.mean_var_grad(spec, theta, X, y, Xs)


def composite():
    name = "composite_N140"
    spec, theta, X, y = golden_spec(name), GOLD[f"{name}/theta"], GOLD[f"{name}/X"], GOLD[f"{name}/y"]
    return spec, theta, X, y, points(X, 90, spec["idx_cont"], on_train=10)


#: (form, padding of ldxs, padding of ldg): the four forms, and two with different paddings on the two sides
GRAD_FORMS = [(f, 3, 3) for f in FORMS] + [(STRIDED_DEVICE, 3, 5), (STRIDED_HOST, 1, 6)]


@pytest.mark.parametrize("fit", [False, True])
def test_predict_in_every_form(gpu, fit):
    spec, theta, X, y, Xs = one_tile()
    mu_o, var_o = one_tile_refs()[:2]
    with make_engine(spec, theta, X, y) as eng:
        prepare(eng, theta, fit)
        mu0, var0 = eng.predict(Xs)
        assert eng.timings()["predict_gemm_form"] == int(fit)
        e_m, e_v = rel(mu0, mu_o), float(np.max(np.abs(var0 - var_o)))
        print(f"ABI-FORMS predict fit={fit}: mean {e_m:.2e} (bar 1e-10) var {e_v:.2e} (bar 1e-11)")
        assert e_m <= 1e-10 and e_v <= 1e-11
        for form in FORMS:
            mu, var = call_predict(eng, Xs, form)
            assert eng.timings()["predict_gemm_form"] == int(fit)
            assert rel(mu, mu_o) <= 1e-10 and float(np.max(np.abs(var - var_o))) <= 1e-11, form.name
            same_bits(mu, mu0, f"predict fit={fit} ({form.name}): mean")
            same_bits(var, var0, f"predict fit={fit} ({form.name}): var")


@pytest.mark.parametrize("fit", [False, True])
def test_predict_grad_in_every_form(gpu, fit):
    spec, theta, X, y, Xs = one_tile()
    G_ref = one_tile_refs()[2]
    with make_engine(spec, theta, X, y) as eng:
        prepare(eng, theta, fit)
        G0 = eng.predict_grad(Xs)
        print(f"ABI-FORMS predict_grad fit={fit}: max |G - G_ref| / max |G_ref| = {grad_err(G0, G_ref):.2e} (bar 1e-8)")
        assert grad_err(G0, G_ref) <= 1e-8
        for form, pad_xs, pad_g in GRAD_FORMS:
            G = call_predict_grad(eng, Xs, form, pad_xs, pad_g)
            assert grad_err(G, G_ref) <= 1e-8, form.name
            same_bits(G, G0, f"predict_grad fit={fit} ({form.name}, +{pad_xs}, +{pad_g})")


@pytest.mark.parametrize("fit", [False, True])
def test_predict_with_grad_in_every_form(gpu, fit):
    spec, theta, X, y, Xs = one_tile()
    mu_o, var_o, _, (_, _, dm_ref, dv_ref) = one_tile_refs()
    with make_engine(spec, theta, X, y) as eng:
        prepare(eng, theta, fit)
        base = eng.predict_with_grad(Xs)
        errs = (rel(base[0], mu_o), float(np.max(np.abs(base[1] - var_o))), grad_err(base[2], dm_ref), grad_err(base[3], dv_ref))
        print(f"ABI-FORMS predict_with_grad fit={fit}: mean {errs[0]:.2e} (bar 1e-10) var {errs[1]:.2e} (1e-11) "
              f"dmean {errs[2]:.2e} dvar {errs[3]:.2e} (1e-8 max|G_ref|)")
        assert errs[0] <= 1e-10 and errs[1] <= 1e-11 and errs[2] <= 1e-8 and errs[3] <= 1e-8
        for form, pad_xs, pad_g in GRAD_FORMS:
            got = call_predict_with_grad(eng, Xs, form, pad_xs, pad_g)
            assert rel(got[0], mu_o) <= 1e-10 and float(np.max(np.abs(got[1] - var_o))) <= 1e-11, form.name
            assert grad_err(got[2], dm_ref) <= 1e-8 and grad_err(got[3], dv_ref) <= 1e-8, form.name
            for a, b, name in zip(got, base, ("mean", "var", "dmean", "dvar")):
                same_bits(a, b, f"predict_with_grad fit={fit} ({form.name}, +{pad_xs}, +{pad_g}): {name}")


def test_composite_model_gradients_in_every_form(gpu):
    """Linear + coregion + two outputs (the golden composite case, D = 4 with two categorical columns): the columns written as
    zero are exactly 0 in every form, and nothing past column D is written."""
    spec, theta, X, y, Xs = composite()
    G_ref = GR.mean_grad(spec, theta, X, y, Xs)
    _, _, dm_ref, dv_ref = VR.mean_var_grad(spec, theta, X, y, Xs)
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        G0 = eng.predict_grad(Xs)
        base = eng.predict_with_grad(Xs)
        errs = (grad_err(G0, G_ref), grad_err(base[2], dm_ref), grad_err(base[3], dv_ref))
        print(f"ABI-FORMS composite: predict_grad {errs[0]:.2e} dmean {errs[1]:.2e} dvar {errs[2]:.2e} (bar 1e-8 max|G_ref|)")
        assert max(errs) <= 1e-8
        for form, pad_xs, pad_g in GRAD_FORMS:
            G = call_predict_grad(eng, Xs, form, pad_xs, pad_g)
            got = call_predict_with_grad(eng, Xs, form, pad_xs, pad_g)
            for arr in (G, got[2], got[3]):
                assert arr.shape == (90, 4) and not np.any(arr[:, 2:]), form.name  # (0.0 or -0.0, nothing else)
            assert grad_err(G, G_ref) <= 1e-8 and grad_err(got[2], dm_ref) <= 1e-8 and grad_err(got[3], dv_ref) <= 1e-8, form.name
            same_bits(G, G0, f"composite predict_grad ({form.name}, +{pad_xs}, +{pad_g})")
            for a, b, name in zip(got, base, ("mean", "var", "dmean", "dvar")):
                same_bits(a, b, f"composite predict_with_grad ({form.name}, +{pad_xs}, +{pad_g}): {name}")


# ---- 3. more than one M-tile -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [False, True])
def test_m_tiles_of_predict_against_the_oracle_and_in_the_strided_forms(gpu, fit):
    """ExpQuad, N = 300 (Np = 384: tiles of 32768 rows), M = 32768 + 77: the smallest shape at which the tile offsets
    ``Xs + m0 * ldxs``, ``mean + m0`` run at all; with D = 1 and ldxs = 4 a tile offset in units of D reads the wrong rows."""
    spec, theta, X, y, Xs, _, _ = var_grad_case("M-tiles")
    mu_o, var_o = oracle_predict("M-tiles")
    assert Xs.shape == (M_TILE + 77, 1)
    with make_engine(spec, theta, X, y) as eng:
        prepare(eng, theta, fit)
        mu0, var0 = eng.predict(Xs)
        assert eng.timings()["predict_gemm_form"] == int(fit)
        e_m, e_v = rel(mu0, mu_o), float(np.max(np.abs(var0 - var_o)))
        e_m2, e_v2 = rel(mu0[M_TILE:], mu_o[M_TILE:]), float(np.max(np.abs(var0[M_TILE:] - var_o[M_TILE:])))
        print(f"ABI-FORMS M-tiles predict fit={fit}: mean {e_m:.2e} (second tile {e_m2:.2e}; bar 1e-10) "
              f"var {e_v:.2e} (second tile {e_v2:.2e}; bar 1e-11)")
        assert e_m < 1e-10 and e_v < 1e-11 and e_m2 < 1e-10 and e_v2 < 1e-11
        for form in STRIDED:
            mu, var = call_predict(eng, Xs, form)  # ldxs = 4
            same_bits(mu, mu0, f"M-tiles predict fit={fit} ({form.name}): mean")
            same_bits(var, var0, f"M-tiles predict fit={fit} ({form.name}): var")


def test_m_tiles_of_predict_grad_in_the_strided_forms(gpu):
    """``gmb_predict_grad`` tiles M by 16384 rows; the packed call on these points is pinned to the reference by
    tests/test_gpu_predict_grad.py::test_m_tiles_with_a_ragged_tail."""
    spec, theta, X, y = table(300, 1, "ExpQuad")
    Xs = points(X, 16384 + 77, [0])
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        G0 = eng.predict_grad(Xs)
        for form in STRIDED:
            same_bits(call_predict_grad(eng, Xs, form), G0, f"M-tiles predict_grad ({form.name}, ldxs = ldg = 4)")


def test_m_tiles_of_predict_with_grad_in_the_strided_device_form(gpu):
    spec, theta, X, y, Xs, _, _ = var_grad_case("M-tiles")
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        base = eng.predict_with_grad(Xs)
        got = call_predict_with_grad(eng, Xs, STRIDED_DEVICE)
        for a, b, name in zip(got, base, ("mean", "var", "dmean", "dvar")):
            same_bits(a, b, f"M-tiles predict_with_grad (strided device, ldxs = ldg = 4): {name}")


# ---- 4. joint posterior ------------------------------------------------------------------------------------------------------------
#: 77 = 2 x 32 + 13 (edge blocks of the symmetrise kernel partly inside) = 4 x 16 + 13 (the draw kernel's row blocks)
M_JOINT = 77


@functools.lru_cache(maxsize=None)
def joint_problem():
    spec, theta, X, y = table(300, 2, "Matern52")
    return spec, theta, X, y, points(X, M_JOINT, [0, 1])


@functools.lru_cache(maxsize=None)
def joint_oracle(with_noise, jitter):
    from test_joint_cpu import JointOracleEngine

    spec, theta, X, y, Xs = joint_problem()
    ref = JointOracleEngine()
    ref.set_data(X, y)
    ref.spec = spec
    ref.set_theta(theta)
    return ref.predict_joint(Xs, with_noise=with_noise, jitter=jitter)


@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("fit", [False, True])
def test_predict_joint_in_every_form(gpu, fit, with_noise):
    spec, theta, X, y, Xs = joint_problem()
    jitter = 0.0 if with_noise else 1e-6
    mean_r, cov_r = joint_oracle(with_noise, jitter)
    with make_engine(spec, theta, X, y) as eng:
        prepare(eng, theta, fit)
        mean0, cov0 = eng.predict_joint(Xs, with_noise=with_noise, jitter=jitter)
        assert eng.timings()["predict_gemm_form"] == int(fit)
        e_c, e_m = float(np.max(np.abs(cov0 - cov_r))), rel(mean0, mean_r)
        print(f"ABI-FORMS predict_joint fit={fit} noise={int(with_noise)}: max|dC| {e_c:.2e} (bar 1e-9) mean {e_m:.2e} (bar 1e-8)")
        assert e_c <= 1e-9 and e_m <= 1e-8 and np.array_equal(cov0, cov0.T)
        for form in FORMS:  # ldc = M (packed) or M + 5
            mean, cov = call_predict_joint(eng, Xs, form, with_noise, jitter)
            assert eng.timings()["predict_gemm_form"] == int(fit)
            assert float(np.max(np.abs(cov - cov_r))) <= 1e-9 and rel(mean, mean_r) <= 1e-8, form.name
            assert np.array_equal(cov, cov.T), f"{form.name}: not exactly symmetric"
            same_bits(cov, cov0, f"predict_joint fit={fit} noise={int(with_noise)} ({form.name}): cov")
            same_bits(mean, mean0, f"predict_joint fit={fit} noise={int(with_noise)} ({form.name}): mean")


@pytest.mark.parametrize("S", [5, 20, 70])  # launch_draw: S <= 16, <= 32, and above with two blocks along S; each with a ragged tail
def test_draw_joint_in_every_form(gpu, S):
    """``with_noise=True, jitter=0``: the well-conditioned regime of tests/test_gpu_joint.py section 2."""
    spec, theta, X, y, Xs = joint_problem()
    mean_r, cov_r = joint_oracle(True, 0.0)
    Z = np.random.default_rng(S).standard_normal((S, M_JOINT))
    Y_r = mean_r[None, :] + Z @ O.cholesky_lower(cov_r).T
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        Y0, mean0 = eng.draw_joint(Xs, Z, with_noise=True, jitter=0.0, return_mean=True)
        err = float(np.max(np.abs(Y0 - Y_r))) / float(np.max(np.abs(Y_r)))
        print(f"ABI-FORMS draw_joint S={S}: max |Y - Y_oracle| / max |Y_oracle| = {err:.2e} (bar 1e-8)")
        assert err <= 1e-8 and rel(mean0, mean_r) <= 1e-8
        for form in FORMS:  # ldz = M + 3, ldy = M + 7 in the strided forms
            for want_mean in (True, False):
                Y, mean = call_draw_joint(eng, Xs, Z, form, True, 0.0, want_mean)
                assert float(np.max(np.abs(Y - Y_r))) <= 1e-8 * float(np.max(np.abs(Y_r))), form.name
                same_bits(Y, Y0, f"draw_joint S={S} ({form.name}, mean {'requested' if want_mean else 'NULL'}): Y")
                if want_mean:
                    same_bits(mean, mean0, f"draw_joint S={S} ({form.name}): mean")


@pytest.mark.parametrize("fit", [False, True])
def test_device_form_calls_leave_the_engine_as_they_found_it(gpu, fit):
    spec, theta, X, y, Xs = joint_problem()
    Z = np.random.default_rng(3).standard_normal((20, M_JOINT))

    def state(eng):
        mu, var = eng.predict(Xs)
        return mu.tobytes(), var.tobytes(), eng.timings()["predict_gemm_form"], np.float64(eng.nlml()).tobytes(), eng.copy_v().tobytes()

    with make_engine(spec, theta, X, y) as eng:
        prepare(eng, theta, fit)
        before = state(eng)
        for form in (PACKED_DEVICE, STRIDED_DEVICE):
            call_predict(eng, Xs, form)
            call_predict_grad(eng, Xs, form)
            call_predict_with_grad(eng, Xs, form)
            call_predict_joint(eng, Xs, form, True, 0.0)
            call_draw_joint(eng, Xs, Z, form, True, 0.0, True)
            assert eng.factor_is_current()
        assert state(eng) == before and before[2] == int(fit)
