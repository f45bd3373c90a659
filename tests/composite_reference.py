"""Independent reference of the composite model's covariance derivatives (TEST INFRASTRUCTURE, CPU, numpy only).

Written from the formulas in the docstring of oracle/gp_oracle.py, not from its gradient code: nothing here calls
``O._kernel_grad_given_M`` or ``O.grad_given_M``.  For every entry of theta, in ABI order, ``dsigma`` yields the N x N matrix
dSigma / dtheta_p in closed form; ``grad_reference`` contracts each with M = (Sigma^-1 - alpha alpha^T) / 2 in longdouble:

    g_p = sum_ij M_ij dSigma_p,ij          A_p = sum_ij |M_ij dSigma_p,ij|

A_p is the size of the sum that component p is the remainder of: a float64 evaluation of g_p in ANY order is off by a few
eps A_p however small g_p itself comes out, so ``4 eps A_p`` is the floor of a per-component bar (a max-norm bar over a
gradient whose components span six orders of magnitude sees only the largest ones).

Model (pymc/GP.py:711-729; additive: :732-754), with a = x[lin] - c, B_t = W_t W_t^T + diag(kappa_t):

    term(ls, eta, c, tau; tables T) = (eta^2 k(r) + tau a.a') * prod_{t in T} B_t[cat_t, cat_t']
    non-additive: Sigma = term(theta's kernel; every table)                      + noise + jitter I
    additive:     Sigma = term(kernel 0; output table) + sum_j term(kernel 1 + j; table j, output table) + noise + jitter I
    noise = sigma^2 I, or sigma^2 diag(B_noise[out, out]) for heteroskedastic multi-output models

    d term / d ls_k   = eta^2 k'(r^2) (-2 (x_k - x'_k)^2 / ls_k^3) prod B     (shared lengthscale: summed over k)
    d term / d eta    = 2 eta k prod B            d term / d tau = a.a' prod B
    d term / d c_k    = -tau (a_k + a'_k) prod B
    d term / d W_t[u, q]  = base prod_{s != t} B_s * ([cat = u] W_t[cat', q] + W_t[cat, q] [cat' = u])
    d term / d kappa_t[u] = base prod_{s != t} B_s * [cat = u] [cat' = u]
    d noise / d sigma = 2 sigma diag(B_noise);  d noise / d W_n[u, q] = 2 sigma^2 W_n[u, q] [out = u];  d / d kappa_n[u] = sigma^2 [out = u]
"""
import numpy as np

from oracle import gp_oracle as O

import precise_reference as PR

LD = np.longdouble
EPS = np.finfo(float).eps


# ------------------------------------------------------------------------------------------------------------------------
# the structures of tests/test_gpu_composite_limits.py: the smallest shapes at which each path of the gradient is reached
# ------------------------------------------------------------------------------------------------------------------------
CASES = {
    #               d  n_lin  levels          n_out hetero kind          additive  N
    "big9":         (3, 1, (9,),              0, False, "Matern52",    False, 300),
    "edge8_9":      (2, 0, (8, 9),            2, True,  "ExpQuad",     False, 300),
    "big32":        (5, 2, (32, 3),           2, True,  "Matern32",    False, 300),
    "out32":        (4, 0, (),               32, True,  "Matern12",    False, 300),
    "lin8":         (8, 8, (),                0, False, "Exponential", False, 300),
    "max":          (16, 8, (32, 9, 8, 2),   32, True,  "Matern52",    False, 384),
    "additive_big": (3, 1, (12, 3),           2, True,  "ExpQuad",     True,  300),
    "one_tile":     (2, 1, (9,),              2, True,  "Matern52",    False, 100),
}


def case_problem(name):
    d, n_lin, levels, n_out, hetero, kind, additive, N = CASES[name]
    seed = 1000 + sorted(CASES).index(name)
    return problem(d, n_lin=n_lin, levels=levels, n_out=n_out, hetero=hetero, kind=kind, additive=additive, N=N, seed=seed)


def _deal(rng, n, L, tile=128):
    """n categories of L levels: every level occurs (a shuffled round-robin deal, so the counts differ by at most one), and
    neither the table's first tile nor any other holds one level only."""
    c = np.arange(n) % L
    while True:
        c = rng.permutation(c)
        if L == 1 or all(len(np.unique(c[s:s + tile])) > 1 for s in range(0, n, tile) if n - s > 1):
            return c.astype(float)


def problem(d, n_lin=0, levels=(), n_out=0, hetero=False, kind="Matern52", additive=False, N=300, M=64, seed=0, ard=True):
    """``(spec, theta, X, y, Xs)`` of one structure from a seed.  Columns of X: d continuous (the first n_lin of them also
    linear), one per categorical dim, the output column last.  Every level of every table occurs among the N training rows
    and among the M test rows; unequal levels meet inside one 128-row tile and across tiles (checked by
    tests/test_composite_reference_cpu.py).  Lengthscales ~ 1.5 sqrt(d) on standard-normal inputs and noise 0.3 keep
    cond(Sigma) near 1e3."""
    rng = np.random.default_rng(seed)
    levels = tuple(int(L) for L in levels)
    D = d + len(levels) + (1 if n_out else 0)
    M = max(M, max(levels + (n_out, 1)))

    def table(n):
        cols = [rng.standard_normal((n, d))]
        cols += [_deal(rng, n, L)[:, None] for L in levels]
        if n_out:
            cols.append(_deal(rng, n, n_out)[:, None])
        return np.column_stack(cols)

    X, Xs = table(N), table(M)
    spec = O.make_spec(D, range(d), kind=kind, ard=ard, idx_lin=range(n_lin), coreg=[(d + j, L) for j, L in enumerate(levels)],
                       out_col=D - 1 if n_out else -1, n_out=n_out, hetero_noise=hetero, additive=additive)

    def kernel_block():
        ls = 1.5 * np.sqrt(d) * rng.uniform(0.8, 1.25, d if ard else 1)
        part = [ls, [rng.uniform(0.9, 1.3)]]
        return part, ([rng.normal(0.0, 0.3, n_lin), [rng.uniform(0.2, 0.6) / n_lin]] if n_lin else [])

    def coreg_block(L):
        return [rng.normal(0.0, 0.5, 2 * L), rng.uniform(0.6, 1.4, L)]

    head, lin = kernel_block()
    parts = head + [[0.3]] + lin
    for L in levels:
        parts += coreg_block(L)
    if n_out:
        parts += coreg_block(n_out)
        if hetero:
            parts += coreg_block(n_out)
    if additive:
        for _ in levels:
            head, lin = kernel_block()
            parts += head + lin
    theta = np.concatenate([np.asarray(p, float).ravel() for p in parts])
    assert theta.size == O.theta_size(spec)
    f = np.sin(X[:, :d].sum(axis=1) / np.sqrt(d)) + 0.2 * X[:, :n_lin].sum(axis=1)
    for j in range(d, D):
        f = f + 0.3 * np.cos(1.7 * X[:, j] + j)
    y = f + 0.3 * rng.standard_normal(N)
    y = (y - y.mean()) / y.std(ddof=1)
    return spec, theta, X, y, Xs


# ------------------------------------------------------------------------------------------------------------------------
# theta's layout
# ------------------------------------------------------------------------------------------------------------------------
def layout(spec):
    """``(blocks, terms, tables)``: ``blocks`` -- ``[(name, start, stop)]`` over theta in ABI order (ls, eta, sigma, c, tau,
    W<j> / kappa<j> per categorical dim, W_out / kappa_out, W_noise / kappa_noise; additive models: t<1+j>.ls ... per further
    kernel); ``terms`` -- per covariance term the dict of its kernel's slices and the list of its tables; ``tables`` -- per
    table ``(column, levels, W slice start, kappa slice start)``, the output table last."""
    n_ls = len(spec["idx_cont"]) if spec["ard"] else 1
    n_lin = len(spec["idx_lin"])
    blocks, k = [], 0

    def take(name, n):
        nonlocal k
        blocks.append((name, k, k + n))
        k += n
        return k - n

    def kernel(prefix, with_sigma):
        kr = {"ls": take(prefix + "ls", n_ls), "eta": take(prefix + "eta", 1)}
        if with_sigma:
            take("sigma", 1)
        if n_lin:
            kr["c"] = take(prefix + "c", n_lin)
            kr["tau"] = take(prefix + "tau", 1)
        return kr

    kernels = [kernel("", True)]
    tables = []
    for j, (col, L) in enumerate(spec["coreg"]):
        tables.append((col, L, take(f"W{j}", 2 * L), take(f"kappa{j}", L)))
    n_cat = len(tables)
    if spec["out_col"] >= 0:
        P = spec["n_out"]
        tables.append((spec["out_col"], P, take("W_out", 2 * P), take("kappa_out", P)))
        if spec["hetero_noise"]:
            take("W_noise", 2 * P)
            take("kappa_noise", P)
    out = list(range(n_cat, len(tables)))
    if spec.get("additive"):
        for j in range(n_cat):
            kernels.append(kernel(f"t{1 + j}.", False))
        terms = [dict(kernels[0], tables=out)] + [dict(kernels[1 + j], tables=[j] + out) for j in range(n_cat)]
    else:
        terms = [dict(kernels[0], tables=list(range(len(tables))))]
    assert k == O.theta_size(spec)
    return blocks, terms, tables


def block_of(spec):
    """name of the block each entry of theta belongs to"""
    blocks, _, _ = layout(spec)
    names = [None] * O.theta_size(spec)
    for name, a, b in blocks:
        names[a:b] = [name] * (b - a)
    return names


def _stationary(kind, r2):
    """k and dk / d r^2 of the five kinds (r = sqrt(r^2 + 1e-12) for all but ExpQuad)"""
    if kind == 0:
        e = np.exp(-r2 / 2)
        return e, -e / 2
    r = np.sqrt(r2 + 1e-12)
    if kind == 1:
        a, e = np.sqrt(5.0) * r, np.exp(-np.sqrt(5.0) * r)
        return (1 + a + a * a / 3) * e, -(5.0 / 6.0) * (1 + a) * e
    if kind == 2:
        a, e = np.sqrt(3.0) * r, np.exp(-np.sqrt(3.0) * r)
        return (1 + a) * e, -1.5 * e
    if kind == 3:
        e = np.exp(-r)
        return e, -e / (2 * r)
    e = np.exp(-r / 2)
    return e, -e / (4 * r)


def dsigma(spec, theta, X):
    """Generator over p = 0 .. theta.size - 1: the N x N matrix dSigma / dtheta_p (float64, closed form)."""
    theta = np.asarray(theta, float)
    X = np.asarray(X, float)
    N = X.shape[0]
    blocks, terms, tables = layout(spec)
    n_ls = len(spec["idx_cont"]) if spec["ard"] else 1
    n_lin = len(spec["idx_lin"])
    # tables: categories, W, the gathered B[cat_i, cat_j]
    tab = []
    for col, L, w0, k0 in tables:
        cat = X[:, col].astype(int)
        W = theta[w0:w0 + 2 * L].reshape(L, 2)
        B = W @ W.T + np.diag(theta[k0:k0 + L])
        tab.append(dict(cat=cat, W=W, L=L, G=B[cat[:, None], cat[None, :]]))
    # terms: kernel value, its r^2-derivative, the linear part, the product of the term's tables (and of all but one)
    tm = []
    for tr in terms:
        ls = theta[tr["ls"]:tr["ls"] + n_ls]
        eta = theta[tr["eta"]]
        Xc = X[:, spec["idx_cont"]]
        sq = [(Xc[:, k][:, None] - Xc[:, k][None, :]) ** 2 for k in range(Xc.shape[1])]
        lsk = ls if spec["ard"] else np.full(Xc.shape[1], ls[0])
        r2 = sum(s / l ** 2 for s, l in zip(sq, lsk))
        kv, dk = _stationary(spec["kind"], r2)
        base = eta ** 2 * kv
        A = lin = None
        tau = 0.0
        if n_lin:
            A = X[:, spec["idx_lin"]] - theta[tr["c"]:tr["c"] + n_lin]
            tau = theta[tr["tau"]]
            lin = A @ A.T
            base = base + tau * lin
        F = np.ones((N, N))
        for t in tr["tables"]:
            F = F * tab[t]["G"]
        others = {}
        for t in tr["tables"]:
            Fo = np.ones((N, N))
            for s in tr["tables"]:
                if s != t:
                    Fo = Fo * tab[s]["G"]
            others[t] = base * Fo
        tm.append(dict(tr=tr, ls=lsk, eta=eta, sq=sq, kv=kv, dk=dk, A=A, lin=lin, tau=tau, F=F, others=others))
    # what multiplies dB_t: summed over the terms that hold table t
    rest = []
    for t in range(len(tab)):
        R = np.zeros((N, N))
        for m in tm:
            if t in m["others"]:
                R = R + m["others"][t]
        rest.append(R)
    hetero = spec["out_col"] >= 0 and spec["hetero_noise"]
    sigma = theta[n_ls + 1]
    if hetero:
        P = spec["n_out"]
        out = X[:, spec["out_col"]].astype(int)
        w0 = [a for name, a, b in blocks if name == "W_noise"][0]
        Wn = theta[w0:w0 + 2 * P].reshape(P, 2)
        bn = np.sum(Wn * Wn, axis=1) + theta[w0 + 2 * P:w0 + 3 * P]

    def kernel_params(m, name, i):
        if name == "ls":
            if spec["ard"]:
                return m["eta"] ** 2 * m["dk"] * (-2.0 * m["sq"][i] / m["ls"][i] ** 3) * m["F"]
            return m["eta"] ** 2 * m["dk"] * (-2.0 * sum(m["sq"]) / m["ls"][0] ** 3) * m["F"]
        if name == "eta":
            return 2.0 * m["eta"] * m["kv"] * m["F"]
        if name == "c":
            a = m["A"][:, i]
            return -m["tau"] * (a[:, None] + a[None, :]) * m["F"]
        assert name == "tau"
        return m["lin"] * m["F"]

    for name, a, b in blocks:
        for i in range(b - a):
            short = name.split(".")[-1]
            if short in ("ls", "eta", "c", "tau"):
                m = tm[int(name[1:].split(".")[0]) if "." in name else 0]
                yield kernel_params(m, short, i)
            elif name == "sigma":
                yield np.diag(2.0 * sigma * bn[out]) if hetero else 2.0 * sigma * np.eye(N)
            elif name == "W_noise":
                u, q = divmod(i, 2)
                yield np.diag(2.0 * sigma ** 2 * Wn[u, q] * (out == u))
            elif name == "kappa_noise":
                yield np.diag(sigma ** 2 * (out == i).astype(float))
            else:
                t = len(tab) - 1 if name.endswith("_out") else int(name.lstrip("Wkapa"))
                tb = tab[t]
                if name.startswith("W"):
                    u, q = divmod(i, 2)
                    is_u, wq = (tb["cat"] == u).astype(float), tb["W"][tb["cat"], q]
                    yield rest[t] * (is_u[:, None] * wq[None, :] + wq[:, None] * is_u[None, :])
                else:
                    is_u = (tb["cat"] == i).astype(float)
                    yield rest[t] * (is_u[:, None] * is_u[None, :])


def contract(spec, theta, X, M):
    """``(g, A)`` with g_p = sum_ij M_ij dSigma_p,ij and A_p = sum_ij |M_ij dSigma_p,ij|, accumulated in M's dtype
    (longdouble M: longdouble sums)."""
    g, A = [], []
    for dS in dsigma(spec, theta, X):
        T = M * dS
        g.append(T.sum())
        A.append(np.abs(T).sum())
    return np.array(g, dtype=M.dtype), np.array(A, dtype=M.dtype)


def grad_reference(spec, theta, X, y, post=None):
    """``(g, A)`` in longdouble from M = (Sigma^-1 - alpha alpha^T) / 2 of ``precise_reference.posterior`` (``post``: that
    call's result with ``grad=True``, if the caller has it)."""
    if post is None:
        post = PR.posterior(spec, theta, X, y, grad=True)
    M = (post["Sinv"] - np.outer(post["alpha"], post["alpha"])) / 2
    assert M.dtype == LD
    return contract(spec, theta, X, M)


def float64_bar(spec, theta, X, M):
    """Per-component bound on the difference of two backward-stable float64 evaluations of the gradient, for the tests whose
    reference is the float64 oracle (``M``: its dNLML / dSigma): each evaluation sums g_p to ~4 eps A_p, and contracts an M
    whose Sigma^-1 and alpha carry the solve's relative error ~cond(Sigma) eps, so

        |g_p - g'_p| <= 2 (4 + cond(Sigma)) eps A_p.

    (On the structures above the float64 host path measures at most 0.08 cond eps A_p against the longdouble reference, and
    only in the blocks whose dSigma is diagonal: sigma and the noise table.)  Returns ``(bar, A)``."""
    S = O.sigma_matrix(spec, theta, X, dist_mode="direct")
    w = np.linalg.eigvalsh(S)
    _, A = contract(spec, theta, X, np.asarray(M, float))
    return 2.0 * (4.0 + w[-1] / w[0]) * EPS * A, A


def oracle_m(spec, theta, X, y):
    """M = dNLML / dSigma = (Sigma^-1 - alpha alpha^T) / 2 as the float64 oracle forms it (``O.nlml_and_grad``: L^-1 by a triangular
    solve of the identity, direct distances)."""
    X, y = np.asarray(X, float), np.asarray(y, float)
    L = O.cholesky_lower(O.sigma_matrix(spec, theta, X, dist_mode="direct"))
    Linv = O.solve_lower(L, np.eye(len(y)))
    alpha = Linv.T @ (Linv @ y)
    return 0.5 * (Linv.T @ Linv - np.outer(alpha, alpha))


def worst_by_block(spec, ratio):
    """``{block: max of ratio over the block's entries}`` in theta's order"""
    out = {}
    for name, r in zip(block_of(spec), np.asarray(ratio, float)):
        out[name] = max(out.get(name, 0.0), float(r))
    return out


def gradient_floor(spec, A, e64):
    """The floor of the per-component bar K max(e64_p, floor_p):

        floor_p = max(4 eps, max over the components q of p's block of e64_q / A_q) * A_p.

    4 eps A_p is what any float64 summation of g_p may be off by.  It covers the host path in every kernel and table block
    (e64_p <= 3.9 eps A_p on all structures), but not in the sigma and noise-table blocks: their dSigma is diagonal, so they read
    diag(Sigma^-1) and alpha^2 with the solve's own relative error ~cond(Sigma) eps in full (e64_p up to 98 eps A_p at cond
    1.3e3; tests/test_composite_reference_cpu.py prints the figures), where the smooth kernel derivatives average it out.
    There e64_p sets the bar, and a component whose e64_p came out small by chance would be held to far less than the host's
    typical error on its neighbours.  So the floor of a component is never below the host's worst RELATIVE error in its block:
    all the noise-table components are held to the same multiple of their own A_p.  In a block of one component (sigma) and
    wherever the host stays below 4 eps A_p this is the plain max(e64_p, 4 eps A_p)."""
    rel = worst_by_block(spec, e64 / A)
    return np.array([max(4 * EPS, rel[b]) for b in block_of(spec)]) * A


_REFERENCE = {}


def reference(name):
    """Everything the tests need of case ``name``, computed once per process and shared (arrays read-only): the problem, the
    longdouble results of precise_reference.posterior (nlml, mean, var, var_noise, its float64-chain-rule ``post_grad``),
    ``g`` / ``A`` of grad_reference rounded to float64, the float64 host path's gradient ``host_grad`` and its error
    ``e64 = |host_grad - g|`` per component and the bar's ``floor`` (gradient_floor)."""
    if name in _REFERENCE:
        return _REFERENCE[name]
    spec, theta, X, y, Xs = case_problem(name)
    post = PR.posterior(spec, theta, X, y, Xs=Xs, grad=True)
    g, A = grad_reference(spec, theta, X, y, post)
    host = PR.host_float64(spec, theta, X, y, grad=True)["grad"]
    ref = dict(theta=theta, X=X, y=y, Xs=Xs, g=g.astype(float), A=A.astype(float), host_grad=host,
               e64=np.abs(host.astype(LD) - g).astype(float), post_grad=post["grad"], nlml=float(post["nlml"]),
               floor=gradient_floor(spec, A.astype(float), np.abs(host.astype(LD) - g).astype(float)),
               mean=post["mean"].astype(float), var=post["var"].astype(float), var_noise=post["var_noise"].astype(float))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    ref["spec"] = spec
    _REFERENCE[name] = ref
    return ref


# ------------------------------------------------------------------------------------------------------------------------
# the launch shapes of grad_tile_kernel no small table reaches (tests/golden/make_composite_limits_goldens.py stores the
# float64 oracle's NLML and gradient of each; the problems themselves come back from their seeds)
# ------------------------------------------------------------------------------------------------------------------------
LARGE_CASES = ("table9_n4224", "matern12_d2_n4224", "matern12_d1_n7040")


def large_problem(name):
    """``(spec, theta, X, y)``.  N = 4224: 561 lower-triangle tiles, more than the 512 up to which a direct-loop launch shares
    every tile among four workgroups; N = 7040: 1540 tiles, more than the 1536 workgroups of one resident round, so every
    workgroup walks two tiles and the runs cross block rows."""
    if name == "table9_n4224":
        spec, theta, X, y, _ = problem(2, n_lin=1, levels=(9,), kind="Matern52", N=4224, seed=4224)
        return spec, theta, X, y
    N, d = (4224, 2) if name == "matern12_d2_n4224" else (7040, 1)
    X, y, ls = O.synthetic_table(N, d, seed=N + d)
    spec = O.make_spec(d, range(d), kind="Matern12")
    return spec, O.pack_theta(spec, ls, 1.2, 0.3), X, y
