"""Timing of the pathwise posterior draws (``gmb_paths_prepare`` / ``gmb_paths_eval`` / ``gmb_paths_eval_own``) behind ``factorize``.

    python tools/gpu_pathwise.py          the benchmark's N = 10,000 table (d = 4, ExpQuad-ARD: bench.py's C2)

Whole-call times are the HIP-event time of the call on the engine's stream (``predict_ms`` of ``gmb_timings``), medians of
``REPEATS`` calls after a warm-up, profiling off.  Reported:

* ``gmb_paths_prepare`` at S = 64, F = 2048 and, from one further call with profiling on (``gmb_set_profiling`` +
  ``GMB_TRACE_FILE``), its parts: the feature pass over the training points (lines of kind 24, flags 0), the two triangular
  passes (kinds 3 and 15) and the rest (uploads, the residual, A's store);
* ``gmb_paths_eval`` at M = 10^6 and M = 10^4: the call, and the all-draws launches alone (kind 24, flags 1) as a pair rate --
  generated (point, index) pairs per second -- and as a share of the FP64 matrix peak (78.6 TF/s); beside it the pair rate of a
  prediction's cross-covariance launch (kind 11) at one M-tile of ``gmb_predict`` (32768 points), which WRITES the M x N block this
  kernel never forms;
* ``gmb_paths_eval_own`` at M = 960 (96 draws x 10 restarts: one objective evaluation of ``propose_thompson`` for a plate) beside
  ``gmb_predict_with_grad`` at the same M.

No pass / fail threshold: the numbers are for DESIGN 3.20.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``TC_TIMEOUT`` seconds,
default 480), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 10_000, 4
S, F = 64, 2048
REPEATS = 5
EV_GEMM, EV_COV, EV_SOLVE_W, EV_PATHS = 3, 11, 15, 24
PEAK = 78.6e12


def child():
    sys.path.insert(0, ROOT)
    import numpy as np

    from gumbi_amd import pathwise
    from gumbi_amd.engine import Engine, KernelSpec
    from oracle import gp_oracle as O

    trace = os.environ["GMB_TRACE_FILE"]
    X, y, ls = O.synthetic_table(N, D)
    spec = O.make_spec(D, range(D), kind="ExpQuad")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    rng = np.random.default_rng(0)
    lo, hi = X.min(axis=0), X.max(axis=0)

    def events():  # [(kind, mt, nt, k, flags, ms)] logged since the last call
        out = []
        with open(trace) as fh:
            for line in fh:
                f = line.split()
                out.append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), float(f[5])))
        open(trace, "w").close()
        return out

    def timed(eng, call):
        call()  # allocations, code objects
        ms = []
        for _ in range(REPEATS):
            call()
            ms.append(eng.timings()["predict_ms"])
        return float(np.median(ms)), min(ms), max(ms)

    def profiled(eng, call):
        eng.set_profiling(True)
        events()
        call()
        ev = events()
        eng.set_profiling(False)
        return ev

    print(f"N={N} d={D} ExpQuad-ARD, behind factorize; medians of {REPEATS} calls after a warm-up (min, max)", flush=True)
    inputs = pathwise.path_inputs("ExpQuad", S, F, D, N, seed=0)
    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(KernelSpec(D=D, idx_cont=list(range(D)), kind=spec["kind"], ard=True, jitter=spec["jitter"]))
        eng.set_theta(theta)
        eng.factorize()
        whole = timed(eng, lambda: eng.paths_prepare(*inputs))
        ev = profiled(eng, lambda: eng.paths_prepare(*inputs))
        feat = sum(e[5] for e in ev if e[0] == EV_PATHS and e[4] == 0)
        pass_v = sum(e[5] for e in ev if e[0] == EV_GEMM)
        pass_w = sum(e[5] for e in ev if e[0] == EV_SOLVE_W)
        print(f"  gmb_paths_prepare S = {S}, F = {F}: {whole[0]:8.3f} ms ({whole[1]:.3f}, {whole[2]:.3f}); while profiling: features at the "
              f"training points {feat:.3f} ms, V = R L^-T {pass_v:.3f} ms, W = V L^-1 {pass_w:.3f} ms (the rest -- uploads of {8 * S * (N + F) / 1e6:.1f} MB, "
              f"residual, store -- is the difference to the call)", flush=True)
        for M in (10**6, 10**4):
            Xs = lo + (hi - lo) * rng.random((M, D))
            call = timed(eng, lambda: eng.paths_eval(Xs))
            ev = [e for e in profiled(eng, lambda: eng.paths_eval(Xs)) if e[0] == EV_PATHS and e[4] == 1]
            ms = sum(e[5] for e in ev)
            pairs = float(M) * (N + F)
            print(f"  gmb_paths_eval M = {M}: {call[0]:9.3f} ms ({call[1]:.3f}, {call[2]:.3f}) with the copies of {8 * M * (D + S) / 1e6:.0f} MB; the all-draws "
                  f"launches alone {ms:.3f} ms in {len(ev)} tile(s) (grid of the first: {ev[0][1]} point tiles x {ev[0][2]} chunks): "
                  f"{pairs / ms / 1e6:.1f} G pairs/s, {2.0 * pairs * S / (ms * 1e-3) / 1e12:.2f} TF/s = {2.0 * pairs * S / (ms * 1e-3) / PEAK:.3f} of the FP64 matrix peak",
                  flush=True)
        Mt = 32768
        Xs = lo + (hi - lo) * rng.random((Mt, D))
        eng.predict(Xs, with_noise=False)
        cov = [e for e in profiled(eng, lambda: eng.predict(Xs, with_noise=False)) if e[0] == EV_COV]
        ms = sum(e[5] for e in cov)
        print(f"  a prediction's cross-covariance launch at M = {Mt}: {ms:.3f} ms for {cov[0][1]} x {cov[0][2]} tiles of 128 x 128 pairs: "
              f"{cov[0][1] * cov[0][2] * 16384 / ms / 1e6:.1f} G pairs/s (it writes {8 * cov[0][1] * cov[0][2] * 16384 / 1e9:.2f} GB)", flush=True)
        M = 960
        Xs = lo + (hi - lo) * rng.random((M, D))
        draw = np.repeat(np.arange(96, dtype=np.int32) % S, 10)
        own = timed(eng, lambda: eng.paths_eval_own(Xs, draw))
        ev = [e for e in profiled(eng, lambda: eng.paths_eval_own(Xs, draw)) if e[0] == EV_PATHS and e[4] == 2]
        old = timed(eng, lambda: eng.predict_with_grad(Xs, with_noise=False))
        print(f"  gmb_paths_eval_own M = {M}: {own[0]:8.3f} ms ({own[1]:.3f}, {own[2]:.3f}), its launches alone {1e3 * sum(e[5] for e in ev):.1f} us "
              f"(grid {ev[0][1]} point blocks x {ev[0][2]} chunks); gmb_predict_with_grad at M = {M} {old[0]:8.3f} ms ({old[1]:.3f}, {old[2]:.3f}); "
              f"ratio {own[0] / old[0]:.3f}", flush=True)


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
