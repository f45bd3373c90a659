"""Timing of ``gmb_predict_decompose`` against its yardstick on the same commit: the same components from separate calls, i.e. T
calls of ``gmb_predict_terms`` (one term each) plus one ``gmb_predict`` for the total -- T + 1 cross-covariances and triangular
solves against the decomposition's T stacked blocks in ONE solve.

    python tools/gpu_components.py          three-term additive model, N = 10,000, M = 10,000

Behind ``factorize`` (both sides on the triangular solve).  Whole-call times are the HIP-event time of each call on the engine's
stream (``predict_ms`` of ``gmb_timings``), medians of ``REPEATS`` calls after a warm-up of each, the two sides alternating, with
profiling off.  The reduction's time comes from one further call with profiling on (``gmb_set_profiling`` + ``GMB_TRACE_FILE``:
launch kind 17 = ``term_gram_partial_kernel`` + ``term_gram_final_kernel`` of one M-tile); its traffic is what the pass must read,
the stacked V once: T x (M padded) x N x 8 bytes, computed here from the shapes.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``TC_TIMEOUT`` seconds,
default 300), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PER_OUTPUT, OUTPUTS, M = 5_000, 2, 10_000
REPEATS = 5


def problem():
    """The three-term model of the tests at N = 10,000: two continuous dimensions (one linear), categorical columns with 3 and 2
    levels, two outputs, hetero noise."""
    import numpy as np

    from oracle import gp_oracle as O

    rng = np.random.default_rng(11)
    n = N_PER_OUTPUT
    X1 = np.column_stack([rng.standard_normal((n, 2)), rng.integers(0, 3, n).astype(float), rng.integers(0, 2, n).astype(float)])
    X = np.vstack([np.column_stack([X1, np.full(n, p)]) for p in range(OUTPUTS)])
    spec = O.make_spec(X.shape[1], [0, 1], idx_lin=[1], coreg=[(2, 3), (3, 2)], out_col=4, n_out=OUTPUTS, hetero_noise=True, additive=True)
    theta = np.abs(rng.normal(1.0, 0.3, O.theta_size(spec))) + 0.2
    y = rng.standard_normal(len(X))
    Xs = X[rng.integers(0, len(X), M)].copy()
    Xs[:, :2] += 0.3 * rng.standard_normal((M, 2))
    return spec, theta, X, y, Xs


def child():
    sys.path.insert(0, ROOT)
    import numpy as np

    from gumbi_amd.engine import Engine, KernelSpec

    trace = os.environ["GMB_TRACE_FILE"]
    spec, theta, X, y, Xs = problem()

    def events():  # {kind: [ms, ...]} logged since the last call
        out = {}
        with open(trace) as fh:
            for line in fh:
                f = line.split()
                out.setdefault(int(f[0]), []).append(float(f[5]))
        open(trace, "w").close()
        return out

    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(KernelSpec(D=spec["D"], idx_cont=spec["idx_cont"], kind=spec["kind"], ard=spec["ard"], idx_lin=spec["idx_lin"],
                                  coreg=spec["coreg"], out_col=spec["out_col"], n_out=spec["n_out"], hetero_noise=spec["hetero_noise"],
                                  jitter=spec["jitter"], additive=True))
        eng.set_theta(theta)
        eng.factorize()
        T, N = eng.num_terms, len(y)

        def separate():
            ms, parts = 0.0, []
            for t in range(T):
                parts.append(eng.predict(Xs, with_noise=False, terms=1 << t))
                ms += eng.timings()["predict_ms"]
            total = eng.predict(Xs, with_noise=False)
            return ms + eng.timings()["predict_ms"], parts, total

        def stacked():
            out = eng.predict_decompose(Xs)
            return eng.timings()["predict_ms"], out

        separate(), stacked()  # allocations, code objects
        t_sep, t_dec = [], []
        for _ in range(REPEATS):
            ms, parts, total = separate()
            t_sep.append(ms)
            ms, (means, cov, noise) = stacked()
            t_dec.append(ms)
        eng.set_profiling(True)
        events()
        again = eng.predict_decompose(Xs)
        ev = events()
        eng.set_profiling(False)
        red_ms = sum(ev.get(17, []))
        mpad = -(-M // 128) * 128
        v_bytes = 8.0 * T * mpad * N
        sep, dec = float(np.median(t_sep)), float(np.median(t_dec))
        print(f"N={N} M={M} T={T}, behind factorize; medians of {REPEATS} calls, the two sides alternating")
        print(f"  {T} x gmb_predict_terms + gmb_predict: {sep:9.3f} ms  (min {min(t_sep):.3f}, max {max(t_sep):.3f})")
        print(f"  gmb_predict_decompose:              {dec:9.3f} ms  (min {min(t_dec):.3f}, max {max(t_dec):.3f})   ratio {dec / sep:.2f}"
              f"  (solves: {T} against {T + 1} = {T / (T + 1):.2f})")
        print(f"  the reduction (kind 17, {len(ev.get(17, []))} M-tile(s), while profiling): {red_ms:.3f} ms for {v_bytes / 1e9:.3f} GB of stacked V "
              f"= {v_bytes / red_ms / 1e9:.2f} TB/s")
        err_mu = max(float(np.max(np.abs(means[t] - parts[t][0]))) for t in range(T))
        err_var = max(float(np.max(np.abs(cov[t, t] - parts[t][1]))) for t in range(T))
        print(f"  against the separate calls: max |mu_t| difference {err_mu:.2e}, max |var_t| difference {err_var:.2e}; "
              f"sum of means against gmb_predict {float(np.max(np.abs(means.sum(0) - total[0]))):.2e}")
        print(f"  same bits call after call: {all(a.tobytes() == b.tobytes() for a, b in zip(again, (means, cov, noise)))}", flush=True)


def main():
    limit = os.environ.get("TC_TIMEOUT", "300")
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
