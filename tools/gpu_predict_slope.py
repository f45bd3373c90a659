"""Timing of ``gmb_predict_slope`` behind ``factorize``, beside a solve-form prediction of as many solved rows.

    python tools/gpu_predict_slope.py          the benchmark's N = 10,000 table (d = 4, ExpQuad-ARD: bench.py's C2)

Behind ``gmb_factorize`` (no resident U: ``gmb_predict`` takes the solve form, the form ``gmb_predict_slope`` always takes).
Whole-call times are the HIP-event time of the call on the engine's stream (``predict_ms`` of ``gmb_timings``), medians of
``REPEATS`` calls after a warm-up of each, profiling off.  Timed, at M = N / Dc (Dc M = 10^4 solved rows) and at M = 1024:

* ``gmb_predict_slope`` without and with ``dcov``;
* ``gmb_predict`` at Dc M points: the same number of rows through the same triangular solve, on the same commit;
* from one further call of each with profiling on (``gmb_set_profiling`` + ``GMB_TRACE_FILE``): the pair rate of
  ``slope_cross_cov_kernel`` (launch kind 19: mt x nt tiles of 128 x 128 pairs, Dc doubles written per pair) against the
  cross-covariance launch's of a prediction (kind 11: one double written per pair).

No pass / fail threshold: the numbers are for DESIGN 3.15.  The expectation they confirm or refute: the call costs about what a
solve-form prediction of Dc M rows costs.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``TC_TIMEOUT`` seconds,
default 300), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 10_000, 4
REPEATS = 5


def child():
    sys.path.insert(0, ROOT)
    import numpy as np

    from gumbi_amd.engine import Engine, KernelSpec
    from oracle import gp_oracle as O

    trace = os.environ["GMB_TRACE_FILE"]
    X, y, ls = O.synthetic_table(N, D)
    spec = O.make_spec(D, range(D), kind="ExpQuad")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    rng = np.random.default_rng(0)
    Dc = D

    def events():  # [(kind, mt, nt, k, ms)] logged since the last call
        out = []
        with open(trace) as fh:
            for line in fh:
                f = line.split()
                out.append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), float(f[5])))
        open(trace, "w").close()
        return out

    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(KernelSpec(D=D, idx_cont=list(range(D)), kind=spec["kind"], ard=True, jitter=spec["jitter"]))
        eng.set_theta(theta)
        eng.factorize()

        def timed(call):
            call()  # allocations, code objects
            ms = []
            for _ in range(REPEATS):
                call()
                ms.append(eng.timings()["predict_ms"])
            return float(np.median(ms)), min(ms), max(ms)

        def line(label, t, extra=""):
            print(f"  {label:<62s} {t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}){extra}", flush=True)

        print(f"N={N} d={D} (Dc = {Dc}) ExpQuad-ARD, behind factorize; medians of {REPEATS} calls after a warm-up")
        for M in (N // Dc, 1024):
            Xs = X[rng.choice(N, M, replace=False)] + 0.1 * rng.standard_normal((M, D))
            Xp = X[rng.choice(N, Dc * M, replace=Dc * M > N)] + 0.1 * rng.standard_normal((Dc * M, D))
            plain = timed(lambda: eng.predict_slope(Xs))
            full = timed(lambda: eng.predict_slope(Xs, cov=True))
            pred = timed(lambda: eng.predict(Xp, with_noise=False))
            assert eng.timings()["predict_gemm_form"] == 0
            line(f"gmb_predict_slope, M = {M} ({Dc * M} solved rows)", plain, f"   = {plain[0] / pred[0]:.2f} x the prediction")
            line(f"gmb_predict_slope, M = {M}, with dcov", full, f"   = {full[0] / pred[0]:.2f} x the prediction")
            line(f"gmb_predict (solve form), M = {Dc * M}", pred)
            # pair rates, from one call of each with profiling on
            eng.set_profiling(True)
            events()
            eng.predict_slope(Xs, cov=True)
            ev_slope = events()
            eng.predict(Xp, with_noise=False)
            ev_pred = events()
            eng.set_profiling(False)
            for kind, evs, what in ((19, ev_slope, f"slope_cross_cov_kernel (kind 19), M = {M}: {Dc} doubles per pair"),
                                    (11, ev_pred, f"cross-covariance launch of gmb_predict (kind 11), M = {Dc * M}: 1 double per pair")):
                sel = [e for e in evs if e[0] == kind]
                ms = sum(e[4] for e in sel)
                pairs = sum(16384.0 * e[1] * e[2] for e in sel)
                written = pairs * (Dc if kind == 19 else 1) * 8.0
                print(f"    {what:<84s} {len(sel)} launch(es), {ms:8.3f} ms while profiling, {pairs:.3e} pairs = "
                      f"{pairs / ms / 1e6:6.1f} G pairs/s, {written / ms / 1e6:7.1f} GB/s written", flush=True)
            solve = sum(e[4] for e in ev_slope if e[0] in (3, 6)), sum(e[4] for e in ev_pred if e[0] in (3, 6))
            print(f"    the triangular solve's launches (kinds 3, 6) while profiling: {solve[0]:.3f} ms in the slope call, {solve[1]:.3f} ms in the prediction")


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
