"""Timing of ``gmb_predict_batches`` behind ``factorize``, beside the calls that do the same triangular work at the same M.

    python tools/gpu_predict_batches.py          the benchmark's N = 10,000 table (d = 4, ExpQuad-ARD: bench.py's C2)

Whole-call times are the HIP-event time of the call on the engine's stream (``predict_ms`` of ``gmb_timings``), medians of
``REPEATS`` calls after a warm-up, profiling off.  Reported:

* the call with gradients at B = 10, q = 8 (what one objective evaluation of ``propose_batch`` costs at its defaults) beside
  ``gmb_predict_with_grad`` at M = 80;
* the values-only call at B = 512, q = 8 (the raw batches' scoring) beside ``gmb_predict`` at M = 4096;
* from one further call of each with profiling on (``gmb_set_profiling`` + ``GMB_TRACE_FILE``), the new contraction launches
  alone -- lines of kind 23: flags 0 = the partial + finishing launches of Q = V V^T, 1 = those of the derivative sums -- the
  second triangular pass (kind 15), and beside the derivative sums the vector launches of ``gmb_predict_with_grad`` at the same
  points (kind 14), which form the diagonal pairs alone.

No pass / fail threshold: the numbers are for DESIGN 3.19.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``TC_TIMEOUT`` seconds,
default 480), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 10_000, 4
REPEATS = 5
EV_BATCH, EV_SOLVE_W, EV_VGRAD = 23, 15, 14


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

    print(f"N={N} d={D} ExpQuad-ARD, behind factorize; medians of {REPEATS} calls after a warm-up (min, max)", flush=True)
    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(KernelSpec(D=D, idx_cont=list(range(D)), kind=spec["kind"], ard=True, jitter=spec["jitter"]))
        eng.set_theta(theta)
        eng.factorize()
        for B, q, grad in ((10, 8, True), (512, 8, False)):
            Xs = lo + (hi - lo) * rng.random((B * q, D))
            new = timed(eng, lambda: eng.predict_batches(Xs, q, grad=grad))
            if grad:
                old, name = timed(eng, lambda: eng.predict_with_grad(Xs, with_noise=False)), "gmb_predict_with_grad"
            else:
                old, name = timed(eng, lambda: eng.predict(Xs, with_noise=False)), "gmb_predict"
            eng.set_profiling(True)
            events()
            eng.predict_batches(Xs, q, grad=grad)
            ev = events()
            vector = 0.0
            if grad:  # the vector kernel of gmb_predict_with_grad at the same points: the diagonal pairs (j, j) alone, 1 / q of the pairs
                eng.predict_with_grad(Xs, with_noise=False)
                vector = sum(e[5] for e in events() if e[0] == EV_VGRAD)
            eng.set_profiling(False)
            gram = sum(e[5] for e in ev if e[0] == EV_BATCH and e[4] == 0)
            sums = sum(e[5] for e in ev if e[0] == EV_BATCH and e[4] == 1)
            solve_w = sum(e[5] for e in ev if e[0] == EV_SOLVE_W)
            plan = [e for e in ev if e[0] == EV_BATCH][0]
            print(f"  B = {B}, q = {q}, {'with gradients' if grad else 'values only'}: gmb_predict_batches {new[0]:8.3f} ms ({new[1]:.3f}, {new[2]:.3f}); "
                  f"{name} at M = {B * q} {old[0]:8.3f} ms ({old[1]:.3f}, {old[2]:.3f}); ratio {new[0] / old[0]:.2f}", flush=True)
            print(f"    while profiling: Q = V V^T {1e3 * gram:.1f} us" + (f", derivative sums {1e3 * sums:.1f} us (gmb_predict_with_grad's vector launches for the {B * q} diagonal pairs alone: {1e3 * vector:.1f} us), W = V L^-1 {solve_w:.3f} ms" if grad else "")
                  + f"; grid {plan[1]} batches x {plan[2]} chunks", flush=True)


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
