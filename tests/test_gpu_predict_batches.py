"""``gmb_predict_batches`` -- the joint posterior of many small batches of test points with its derivative with respect to the
batch's own coordinates -- on the MI355X against the numpy reference of tests/batch_reference.py (itself pinned to finite
differences of a longdouble joint covariance by tests/test_predict_batches_cpu.py), and ``propose_batch`` on top of it.  Needs a
GPU (``-m gpu``).

Bars, each copied from where the project states it:

* ``dmean`` and ``dcov`` against the reference: ``1e-8 max|ref|`` absolute (tests/test_gpu_predict_grad.py, test_gpu_var_grad.py);
* ``cov`` against the reference: 1e-9 absolute; ``mean``: 1e-8 relative (tests/test_gpu_joint.py);
* against the engine's own ``predict``, ``predict_joint`` and ``predict_with_grad``: 1e-10 relative for mean, blocks and
  gradients, 1e-11 absolute for the diagonal;
* determinism, the values-only form, companions within a tile, state: bit-identical; across a tile seam 1e-12 relative.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import abi_forms as AF
import batch_reference as BR
from oracle import gp_oracle as O
from test_gpu_abi_forms import PACKED_HOST, STRIDED_DEVICE, STRIDED_HOST, mat_in, mat_out, same_bits, sync, take, take_vec, vec_out
from test_gpu_parity import GOLD, golden_spec, make_engine, rel
from test_gpu_predict_grad import DISPATCH_DIMS, frontend_dataset, points, table

pytestmark = pytest.mark.gpu

JITTER = 1e-6
M_TILE = 32768  # gmb_predict's M-tile at these N


def batch_points(X, q, B, cont, on_train=None, twins=True, seed=1):
    """B q points as ``test_gpu_predict_grad.points`` makes them, the first third ON training points (by default), and -- q >= 2 --
    the second point of the last batch a copy of its first."""
    M = q * B
    Xs = points(X, M, cont, seed=seed, on_train=M // 3 if on_train is None else on_train)
    if twins and q >= 2:
        Xs[M - q + 1] = Xs[M - q]
    return Xs


def check_grad(got, ref, what):
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: max |G - G_ref| = {err:.3e}, max |G_ref| = {scale:.3e}, ratio {err / scale:.2e}")
    assert got.shape == ref.shape
    assert err <= 1e-8 * scale


def check_all(got, ref, what):
    mean, cov, dmean, dcov = got
    r_mean, r_cov, r_dmean, r_dcov = ref
    e_cov = float(np.max(np.abs(cov - r_cov)))
    print(f"{what}: mean rel {rel(mean, r_mean):.2e}, cov abs {e_cov:.2e}")
    assert rel(mean, r_mean) <= 1e-8
    assert e_cov <= 1e-9
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2)), f"{what}: cov is not exactly symmetric"
    check_grad(dmean, r_dmean, f"{what} dmean")
    check_grad(dcov, r_dcov, f"{what} dcov")


def run(spec, theta, X, y, Xs, q, what, mode=0, periods=None):
    if mode:
        from test_gpu_periodic import make_engine as periodic_engine

        eng = periodic_engine(spec, mode, periods, theta, X, y)
    else:
        eng = make_engine(spec, theta, X, y)
    with eng:
        eng.factorize()
        got = eng.predict_batches(Xs, q, jitter=JITTER)
    check_all(got, BR.batch_posterior(spec, theta, X, y, Xs, q, jitter=JITTER, periodic=mode, periods=periods), what)
    return got


# ---- 1. against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,B", [(1, 77), (2, 39), (5, 15), (16, 5)])
@pytest.mark.parametrize("kind", O.KINDS)
def test_matches_the_reference(gpu, kind, q, B):
    spec, theta, X, y = table(300, 3, kind)
    got = run(spec, theta, X, y, batch_points(X, q, B, [0, 1, 2]), q, f"{kind} N=300 d=3 q={q} B={B}")
    if q >= 2:  # the coincident pair of the last batch: every derivative finite
        assert np.all(np.isfinite(got[3][-1]))


@pytest.mark.parametrize("d", DISPATCH_DIMS)
@pytest.mark.parametrize("kind", O.KINDS)
def test_every_padded_width(gpu, kind, d):
    spec, theta, X, y = table(200, d, kind)
    run(spec, theta, X, y, batch_points(X, 5, 7, list(range(d))), 5, f"{kind} N=200 d={d} q=5 B=7")


def test_shared_lengthscale(gpu):
    spec, theta, X, y = table(300, 3, "Matern52", ard=False)
    run(spec, theta, X, y, batch_points(X, 5, 15, [0, 1, 2]), 5, "Matern52 shared lengthscale")


def test_eight_block_columns(gpu):
    spec, theta, X, y = table(1000, 3, "Matern32")
    run(spec, theta, X, y, batch_points(X, 16, 21, [0, 1, 2]), 16, "Matern32 N=1000 q=16 B=21")


def test_composite_model_with_batches_that_mix_categories(gpu):
    case = "composite_N140"
    spec, theta, X, y = golden_spec(case), GOLD[f"{case}/theta"], GOLD[f"{case}/X"], GOLD[f"{case}/y"]
    Xs = batch_points(X, 6, 15, spec["idx_cont"], on_train=10)
    cats = Xs[:, 2:].reshape(15, 6, -1)
    assert any(len({tuple(r) for r in b}) > 1 for b in cats), "no batch mixes categories"
    _, _, dmean, dcov = run(spec, theta, X, y, Xs, 6, "composite N=140 q=6 B=15")
    assert not np.any(dmean[:, :, 2:]) and not np.any(dcov[:, :, :, 2:])


def test_additive_model(gpu):
    from test_oracle import additive_problem

    spec, theta, X, y = additive_problem(n=150, two_outputs=True, lin=True, hetero=True)  # N = 300
    Xs = batch_points(X, 5, 13, spec["idx_cont"], on_train=0)
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        got = eng.predict_batches(Xs, 5, jitter=JITTER)
        mu, _ = eng.predict(Xs, with_noise=False)  # term 0's preparation of the training points is back in place
    check_all(got, BR.batch_posterior(spec, theta, X, y, Xs, 5, jitter=JITTER), "additive N=300 q=5 B=13")
    assert rel(mu, O.predict(spec, theta, X, y, Xs, with_noise=False, dist_mode="direct")[0]) < 1e-8


@pytest.mark.parametrize("kind,mode", [("Matern52", 1), ("ExpQuad", 2)])
def test_periodic_models(gpu, kind, mode):
    from test_gpu_periodic import case as periodic_case

    spec, theta, X, y, periods = periodic_case(kind, mode, 300, 2)
    run(spec, theta, X, y, batch_points(X, 4, 12, [0, 1], on_train=16), 4, f"{kind} periodic mode {mode}", mode, periods)


# ---- 2. consistency with the engine's other calls, determinism, state ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small():
    spec, theta, X, y = table(300, 3, "Matern52")
    return spec, theta, X, y, batch_points(X, 8, 10, [0, 1, 2])


def test_agrees_with_predict_joint_and_predict_with_grad(gpu):
    spec, theta, X, y, Xs = small()
    q, B = 8, 10
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        mean, cov, dmean, dcov = eng.predict_batches(Xs, q, jitter=JITTER)
        j_mean, j_cov = eng.predict_joint(Xs, with_noise=False, jitter=JITTER)
        g_mean, g_var, g_dmean, g_dvar = eng.predict_with_grad(Xs, with_noise=False)
        p_mean, p_var = eng.predict(Xs, with_noise=False)
    blocks = np.stack([j_cov[b * q:(b + 1) * q, b * q:(b + 1) * q] for b in range(B)])
    idx = np.arange(q)
    diag = cov[:, idx, idx].ravel()
    print(f"blocks vs predict_joint {rel(cov, blocks):.2e}, diagonal vs predict {np.max(np.abs(diag - JITTER - p_var)):.2e}, "
          f"dcov[j, j] vs dvar {rel(dcov[:, idx, idx].reshape(B * q, -1), g_dvar):.2e}, dmean {rel(dmean.reshape(B * q, -1), g_dmean):.2e}")
    assert rel(cov, blocks) < 1e-10 and rel(mean.ravel(), j_mean) < 1e-10
    assert rel(mean.ravel(), p_mean) < 1e-10 and rel(mean.ravel(), g_mean) < 1e-10
    assert np.max(np.abs(diag - JITTER - p_var)) <= 1e-11 and np.max(np.abs(diag - JITTER - g_var)) <= 1e-11
    assert np.max(np.abs(diag - np.diag(j_cov))) <= 1e-11
    assert rel(dmean.reshape(B * q, -1), g_dmean) < 1e-10
    assert rel(dcov[:, idx, idx].reshape(B * q, -1), g_dvar) < 1e-10


def test_values_only_form_repeats_and_state(gpu):
    spec, theta, X, y, Xs = small()

    def state(eng):
        mu, var = eng.predict(Xs)
        return mu.tobytes(), var.tobytes(), eng.copy_v().tobytes(), eng.factor_is_current()

    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        before = state(eng)
        eng.factorize()
        a = eng.predict_batches(Xs, 8, jitter=JITTER)
        b = eng.predict_batches(Xs, 8, jitter=JITTER)
        v = eng.predict_batches(Xs, 8, jitter=JITTER, grad=False)
        after = state(eng)
    for x, z in zip(a, b):
        assert x.tobytes() == z.tobytes()
    assert len(v) == 2 and v[0].tobytes() == a[0].tobytes() and v[1].tobytes() == a[1].tobytes()
    assert before == after and before[3] is True


def test_a_batch_does_not_depend_on_its_companions(gpu):
    spec, theta, X, y, Xs = small()
    other = batch_points(X, 8, 10, [0, 1, 2], seed=7)
    other[24:32] = Xs[24:32]  # batch 3 of 10 in both
    moved = np.concatenate([other[:8], Xs[24:32], other[8:24], other[32:]])  # ... and as batch 1 among other companions
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        a = eng.predict_batches(Xs, 8, jitter=JITTER)
        b = eng.predict_batches(other, 8, jitter=JITTER)
        c = eng.predict_batches(moved, 8, jitter=JITTER)
    for x, z, w in zip(a, b, c):
        assert x[3].tobytes() == z[3].tobytes() == w[1].tobytes()


def test_tile_seam(gpu):
    """q = 5: a full M-tile holds 6553 batches (32765 points); 6556 batches put three behind the seam."""
    q, bt = 5, M_TILE // 5
    spec, theta, X, y = table(300, 1, "ExpQuad")
    Xs = batch_points(X, q, bt + 3, [0], on_train=0)
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        whole = eng.predict_batches(Xs, q, jitter=JITTER)
        tail = eng.predict_batches(Xs[bt * q:], q, jitter=JITTER)
        head = eng.predict_batches(Xs[:3 * q], q, jitter=JITTER)
    for name, w, t, h in zip(("mean", "cov", "dmean", "dcov"), whole, tail, head):
        print(f"{name}: behind the seam vs alone {rel(w[bt:], t):.2e}, first batches vs alone {rel(w[:3], h):.2e}")
        assert w.shape[0] == bt + 3 and rel(w[bt:], t) <= 1e-12 and rel(w[:3], h) <= 1e-12
    ref = BR.batch_posterior(spec, theta, X, y, Xs[bt * q:], q, jitter=JITTER)
    check_all(tuple(w[bt:] for w in whole), ref, "behind the seam")


# ---- 3. refusals and call forms -------------------------------------------------------------------------------------------------------
def raw_call(eng, Xs, q, form=PACKED_HOST, B=None, grad=True, null=(), pad=3, jitter=JITTER):
    """The C call with guarded buffers: ``(status, outputs or None, clean)`` -- ``clean``: every output buffer still carries its fill."""
    M, D = Xs.shape
    B = M // max(q, 1) if B is None else B
    nb = max(M // max(q, 1), 1)
    qq = max(q, 1) ** 2
    x = mat_in(Xs, form, pad)
    mean, cov = vec_out(M, form), vec_out(nb * qq, form)
    dmean, dcov = mat_out(M, D, form, pad), vec_out(nb * qq * D, form)
    bufs = {"mean": mean, "cov": cov, "dmean": dmean, "dcov": dcov}
    ptr = {k: (None if k in null or (not grad and k in ("dmean", "dcov")) else b.ptr) for k, b in bufs.items()}
    sync()
    rc = eng._lib.gmb_predict_batches(eng._h, None if "Xs" in null else x.ptr, B, q, x.ld, float(jitter), ptr["mean"], ptr["cov"], ptr["dmean"],
                                      dmean.ld, ptr["dcov"], form.memspace)
    fetched = {k: b.fetch() for k, b in bufs.items()}
    clean = all(bool(np.all(np.ascontiguousarray(h).view(np.uint64) == AF.FILL_BITS)) for h in fetched.values())
    if rc != 0 or B == 0:
        return rc, None, clean
    what = f"gmb_predict_batches ({form.name})"
    out = [take_vec(mean, M, what + " mean").reshape(B, q), take_vec(cov, B * q * q, what + " cov").reshape(B, q, q)]
    if grad:
        out += [take(dmean, M, D, what + " dmean").reshape(B, q, D), take_vec(dcov, B * q * q * D, what + " dcov").reshape(B, q, q, D)]
    return rc, out, clean


def test_refusals_write_nothing(gpu):
    from gumbi_amd.engine import GMB_EINVAL

    spec, theta, X, y, Xs = small()
    with make_engine(spec, theta, X, y) as eng:
        def refused(label, *args, **kw):
            rc, _, clean = raw_call(eng, *args, **kw)
            assert rc == GMB_EINVAL, f"{label}: status {rc}"
            assert clean, f"{label}: outputs were written"

        refused("no factor", Xs, 8)
        eng.factorize()
        before = eng.predict(Xs)
        refused("q = 0", Xs, 0, B=10)
        refused("q = 17", Xs[:68], 17)
        refused("B < 0", Xs, 8, B=-1)
        refused("null Xs", Xs, 8, null=("Xs",))
        refused("null mean", Xs, 8, null=("mean",))
        refused("null cov", Xs, 8, null=("cov",))
        refused("dmean without dcov", Xs, 8, null=("dcov",))
        refused("dcov without dmean", Xs, 8, null=("dmean",))
        rc, _, clean = raw_call(eng, Xs, 8, B=0)
        assert rc == 0 and clean, "B == 0 is GMB_OK and writes nothing"
        with pytest.raises(ValueError):
            eng.predict_batches(Xs[:-1], 8)
        eng.set_theta(theta * 1.01)
        refused("after gmb_set_theta", Xs, 8)
        eng.set_theta(theta)
        eng.factorize()
        eng.nlml(grad=True)  # (a single engine holds the CONSUMED state only while a gradient is in flight: current, or refused)
        if eng.factor_is_current():
            assert raw_call(eng, Xs, 8)[0] == 0
        else:
            refused("on a consumed factor", Xs, 8)
        eng.factorize()
        after = eng.predict(Xs)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        eng.set_dist_mode(eng.DIST_CAPACITY)
        refused("capacity mode", Xs, 8)


@pytest.mark.parametrize("form", [STRIDED_HOST, STRIDED_DEVICE], ids=lambda f: f.name)
def test_device_memory_and_strided_forms(gpu, form):
    spec, theta, X, y, Xs = small()
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        want = eng.predict_batches(Xs, 8, jitter=JITTER)
        rc, got, _ = raw_call(eng, Xs, 8, form)
        assert rc == 0
        for g, w, name in zip(got, want, ("mean", "cov", "dmean", "dcov")):
            same_bits(g, w, f"{form.name} {name}")
        rc, vals, _ = raw_call(eng, Xs, 8, form, grad=False)
        assert rc == 0
        same_bits(vals[0], want[0], "values-only mean")
        same_bits(vals[1], want[1], "values-only cov")


# ---- 4. the front end -----------------------------------------------------------------------------------------------------------------
def test_frontend_propose_batch(gpu):
    import gumbi_amd as gmb

    ds = frontend_dataset(300, ["y"])
    gp = gmb.GP(ds, outputs="y")
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 25})
    prop = gp.propose_batch(3, num_restarts=4, raw_samples=64, mc_samples=128, seed=1, maxiter=30)
    assert prop is gp.proposal
    lo, hi = gp.optimization_bounds
    z = np.column_stack([prop[d].z.values().ravel() for d in gp.continuous_dims])
    assert z.shape == (3, 2) and np.all(z >= lo - 1e-12) and np.all(z <= hi + 1e-12)
    for d in ("a", "b"):
        v = prop[d].values().ravel()
        assert np.all(v >= ds.wide[d].min() - 1e-9) and np.all(v <= ds.wide[d].max() + 1e-9)
    raw = gp.proposal_raw_acquisition
    print(f"proposal {z.tolist()}, log qEI {gp.proposal_acquisition:.6f}, best raw batch {float(np.max(raw)):.6f}, "
          f"{gp.proposal_result.nfev} evaluations")
    assert raw.shape == (64,) and gp.proposal_acquisition >= float(np.max(raw))
    value, grad = gp.batch_acquisition_with_grad(z[None], mc_samples=128, seed=1)
    assert value.shape == (1,) and grad.shape == (1, 3, 2) and np.all(np.isfinite(grad))
    again = gp.propose_batch(3, num_restarts=4, raw_samples=64, mc_samples=128, seed=1, maxiter=30)
    z2 = np.column_stack([again[d].z.values().ravel() for d in gp.continuous_dims])
    assert z2.tobytes() == z.tobytes()
    with pytest.raises(NotImplementedError):  # the single-point entry keeps refusing a joint batch
        gp.propose_continuous(q=3)
