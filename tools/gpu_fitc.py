"""Timing of the sparse (FITC) path: one ``fitc_evaluate`` with gradient and one ``fitc_predict`` of M = 10^4 points.

    python tools/gpu_fitc.py          N = 100,000, d = 4, Matern-5/2 ARD, m = 512 and m = 1024 inducing points (k-means centres)

Whole-call times are wall-clock times around the call (both calls end in a synchronise), medians of ``REPEATS`` calls after a
warm-up, profiling off.  From one further call with profiling on (``gmb_set_profiling`` + ``GMB_TRACE_FILE``) the launches' own
times are summed into

* cross-covariance  kind 21, flags 0: K(tile, Z) of every tile of both passes;
* solves            the blocked triangular solves: strip solves (kind 6), their update products (kind 2), the passes V L^-1
                    (kind 21, flags 1);
* GEMMs             the products that add B and P (kind 4);
* reductions        the column / row / adjoint / transpose passes and the derivative and prediction reductions (kind 21, flags 2, 3);
* Cholesky          every launch of the two m x m factorisations (kinds 0, 1, 5, 7, 8, 10).

The sum of the parts is less than the call: host work between the launches, the synchronises behind the two factorisations and
the copies are in the call's time only.  Beside them: one exact ``evaluate`` with gradient at N = 10,000 on the same table's first
rows.  No pass / fail threshold: the numbers are for DESIGN 3.17.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``TC_TIMEOUT`` seconds,
default 480), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, M = 100_000, 4, 10_000
N_EXACT = 10_000
MS = (512, 1024)
REPEATS = 3
PARTS = ("cross-covariance", "solves", "GEMMs", "reductions", "Cholesky")


def part_of(kind, flags):
    if kind == 21:
        return ("cross-covariance", "solves", "reductions", "reductions")[flags]
    if kind in (2, 6):
        return "solves"
    if kind == 4:
        return "GEMMs"
    if kind in (0, 1, 5, 7, 8, 10):
        return "Cholesky"
    return None


def child():
    sys.path.insert(0, ROOT)
    import numpy as np

    from gumbi_amd.engine import Engine, KernelSpec, fitc_plan
    from scipy.cluster.vq import kmeans
    from oracle import gp_oracle as O

    trace = os.environ["GMB_TRACE_FILE"]
    X, y, ls = O.synthetic_table(N, D)
    spec = O.make_spec(D, range(D), kind="Matern52")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    Xs = np.random.default_rng(0).standard_normal((M, D))
    ks = KernelSpec(D=D, idx_cont=list(range(D)), kind=spec["kind"], ard=True, jitter=spec["jitter"])

    def split():  # {part: ms} of the launches logged since the last call
        out = dict.fromkeys(PARTS, 0.0)
        with open(trace) as fh:
            for line in fh:
                f = line.split()
                part = part_of(int(f[0]), int(f[4]))
                if part:
                    out[part] += float(f[5])
        open(trace, "w").close()
        return out

    def timed(call):
        call()  # allocations, code objects
        ts = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            call()
            ts.append(1e3 * (time.perf_counter() - t0))
        return np.median(ts), min(ts), max(ts)

    def report(what, t, parts):
        print(f"  {what}: {t[0]:9.2f} ms (min {t[1]:.2f}, max {t[2]:.2f}); while profiling: "
              + ", ".join(f"{p} {parts[p]:.2f}" for p in PARTS) + f" ms (sum {sum(parts.values()):.2f})", flush=True)

    print(f"N={N} d={D} Matern-5/2 ARD, M={M} test points; medians of {REPEATS} calls after a warm-up", flush=True)
    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(ks)
        for m in MS:
            t0 = time.perf_counter()
            # (SparseGP's default runs scipy's k-means 20 times on 64 m rows -- two minutes on the host at m = 1024; the timings
            # below do not depend on where the centres lie, so two runs on 16 m rows serve here)
            rows = np.sort(np.random.default_rng(1).choice(N, size=16 * m, replace=False))
            Z = np.ascontiguousarray(kmeans(X[rows], m, iter=2, seed=1)[0])
            plan = fitc_plan(N, len(Z))
            print(f" m = {len(Z)} (k-means on the host: {time.perf_counter() - t0:.1f} s); {plan['ntile']} tiles of {plan['tile_rows']} columns, "
                  f"buffers {(plan['bytes_fixed'] + plan['bytes_blocks'] + plan['bytes_columns']) / 2**20:.0f} MiB", flush=True)
            eng.set_inducing(Z)
            t_eval = timed(lambda: eng.fitc_evaluate(theta, grad=True))
            t_nlml = timed(lambda: eng.fitc_evaluate(theta, grad=False))
            t_pred = timed(lambda: eng.fitc_predict(Xs))
            eng.set_profiling(True)
            split()
            val, grad = eng.fitc_evaluate(theta, grad=True)
            p_eval = split()
            eng.fitc_predict(Xs)
            p_pred = split()
            eng.set_profiling(False)
            report("fitc_evaluate with gradient", t_eval, p_eval)
            print(f"  fitc_evaluate, NLML only:    {t_nlml[0]:9.2f} ms (min {t_nlml[1]:.2f}, max {t_nlml[2]:.2f})", flush=True)
            report(f"fitc_predict of {M} points ", t_pred, p_pred)
            print(f"  NLML {val:.6f}, |grad| {np.linalg.norm(grad):.4e}, resident peak {eng.resident_bytes(peak=True) / 2**20:.0f} MiB", flush=True)
    with Engine(0) as eng:
        eng.set_data(X[:N_EXACT], y[:N_EXACT])
        eng.set_kernel(ks)
        t = timed(lambda: eng.evaluate(theta, grad=True))
        print(f" exact evaluate with gradient at N = {N_EXACT}: {t[0]:.2f} ms (min {t[1]:.2f}, max {t[2]:.2f}), "
              f"resident peak {eng.resident_bytes(peak=True) / 2**20:.0f} MiB", flush=True)


def main():
    limit = os.environ.get("TC_TIMEOUT", "480")
    with tempfile.NamedTemporaryFile(prefix="tc_trace_", suffix=".txt") as tf:
        env = dict(os.environ, GMB_TRACE_FILE=tf.name)
        rc = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode
    if rc != 0:
        print(f"the child ended with status {rc}; nothing further is started")
    return rc


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        child()
    else:
        sys.exit(main())
