"""Timing of ``gmb_design_batch`` behind a fit's last evaluation, beside the same picks by ``append`` + ``predict`` rounds.

    python tools/gpu_design_batch.py          the benchmark's N = 10,000 table (d = 4, ExpQuad-ARD: bench.py's C2)

Behind ``evaluate(theta, grad=True)`` (the resident U: V takes the product form).  Cases: M = 1024 candidates, R = 10^5 reference
points, q = 96 picks (a plate), and M = 256, R = 10^4, q = 8.  Whole-call times are the HIP-event time of the call on the engine's
stream (``predict_ms`` of ``gmb_timings``), medians of ``REPEATS`` calls after a warm-up, profiling off.  Reported:

* the call's time and, from one further call with profiling on (``gmb_set_profiling`` + ``GMB_TRACE_FILE``, phase lines of kind 20:
  flags 0 = the solved rows V of a point tile, 1 = its prior + rank-N update, 2 = the greedy loop), its split into V, prior + GEMM
  and loop;
* the loop's time per step against the bytes a step moves, ``2 x 8 x M x (M + R)`` (one read and one write of D), as a rate beside
  the device copy rate the project quotes for its HBM-bound kernels (6.29 TB/s);
* the only way to the same numbers without the call: q rounds of ``append`` of the pick (y = 0) + ``predict`` of the R reference
  points on a second engine -- wall-clock time of the q rounds (both calls synchronise), the engine truncated afterwards -- and
  how far ``ivar0 - sum gains`` lies from that route's last ``sum w var``.  (The rounds are GIVEN the picks: finding them this way
  would cost M such predictions per step on top.)

No pass / fail threshold: the numbers are for DESIGN 3.16.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``TC_TIMEOUT`` seconds,
default 480), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 10_000, 4
REPEATS = 3
COPY_RATE = 6.29e12
CASES = [(1024, 100_000, 96), (256, 10_000, 8)]


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

    def engine():
        eng = Engine(0)
        eng.set_data(X, y)
        eng.set_kernel(KernelSpec(D=D, idx_cont=list(range(D)), kind=spec["kind"], ard=True, jitter=spec["jitter"]))
        return eng

    print(f"N={N} d={D} ExpQuad-ARD, behind evaluate(theta, grad=True); medians of {REPEATS} calls after a warm-up", flush=True)
    with engine() as eng, engine() as grown:
        eng.evaluate(theta, grad=True)
        grown.set_theta(theta)
        grown.factorize()
        for M, R, q in CASES:
            Xc = lo + (hi - lo) * rng.random((M, D))
            Xr = lo + (hi - lo) * rng.random((R, D))
            res = eng.design_batch(Xc, Xr, q)  # allocations, code objects
            assert eng.timings()["predict_gemm_form"] == 1
            ms = []
            for _ in range(REPEATS):
                eng.design_batch(Xc, Xr, q)
                ms.append(eng.timings()["predict_ms"])
            score_ms = []
            for _ in range(REPEATS):
                eng.design_batch(Xc, Xr, 0)
                score_ms.append(eng.timings()["predict_ms"])
            eng.set_profiling(True)
            events()
            eng.design_batch(Xc, Xr, q)
            ev = [e for e in events() if e[0] == 20]
            eng.set_profiling(False)
            split = [sum(e[5] for e in ev if e[4] == f) for f in (0, 1, 2)]
            picks, gains, _, ivar0 = res
            print(f"  M = {M}, R = {R}, q = {q}: gmb_design_batch {np.median(ms):9.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}); "
                  f"q = 0 (scores only) {np.median(score_ms):.3f} ms", flush=True)
            print(f"    while profiling: V {split[0]:.3f} ms in {sum(1 for e in ev if e[4] == 0)} point tile(s), prior + GEMM {split[1]:.3f} ms, "
                  f"loop {split[2]:.3f} ms = {1e3 * split[2] / q:.1f} us per step", flush=True)
            step_bytes = 2.0 * 8.0 * M * (M + R)
            rate = step_bytes / (1e-3 * split[2] / q)
            print(f"    a step moves {step_bytes / 1e9:.3f} GB: {rate / 1e12:.2f} TB/s = {rate / COPY_RATE:.2f} of the {COPY_RATE / 1e12:.2f} TB/s copy rate; "
                  f"gains {gains[0]:.4e} .. {gains[-1]:.4e}, sum = {gains.sum() / ivar0:.3f} of ivar0 = {ivar0:.4e}; "
                  f"{len(set(picks.tolist()))} distinct picks", flush=True)
            # the same numbers by q rounds of append + predict, given the picks
            w = np.full(R, 1.0 / R)
            t0 = time.perf_counter()
            for t in range(q):
                grown.append(Xc[picks[t]][None, :], np.zeros(1))
                _, var = grown.predict(Xr, with_noise=False)
            rounds = time.perf_counter() - t0
            left = ivar0 - gains.sum()
            print(f"    {q} rounds of append + predict of the R points: {1e3 * rounds:.1f} ms wall = {1e3 * rounds / np.median(ms):.0f} x the call; "
                  f"ivar0 - sum gains = {left:.9e}, the rounds' sum w var = {float(w @ var):.9e} (jitter on the appended points: DESIGN 3.16)",
                  flush=True)
            grown.truncate(N)
            if not grown.factor_is_current():
                grown.factorize()


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
