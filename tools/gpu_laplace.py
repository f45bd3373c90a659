"""Timing of GP classification by the Laplace approximation: one ``laplace_evaluate`` with gradient and one ``laplace_predict`` of
M = 10^4 points.

    python tools/gpu_laplace.py          N = 10,000, d = 4, Matern-5/2 ARD, labels drawn from a known latent function

Whole-call times are wall-clock times around the call (both calls end in a synchronise), medians of ``REPEATS`` calls after a
warm-up, profiling off.  From one further call with profiling on (``gmb_set_profiling`` + ``GMB_TRACE_FILE``) the call's phases
(trace lines of kind 22, by their flags) are summed into

* Sigma build   flags 0: the covariance build into the Laplace state's buffer, once per evaluation;
* B builds      flags 1: B = I + (s s^T) o Sigma of every Newton iteration and of the mode, and Z' behind the inverse;
* Choleskys     flags 2: every factorisation of B with its forward row and its back substitution;
* SYMVs         flags 3: the symmetric matrix-vector products (two per iteration, one more per halved step, three in the gradient);
* elementwise   flags 4: the likelihood passes and their folds (the few vector kernels between the phases are not inside one);
* inverse       flags 5: L^-1, L^-T and B^-1 = L^-T L^-1;
* trace pass    flags 6: the exact path's gradient reductions over Z'.

The sum of the parts is less than the call: the host's look at every step (a synchronise and a copy of a few scalars) and the
vector kernels are in the call's time only.  The SYMV's rate is the bytes of the lower triangle (8 N (N + 1) / 2) over the mean
time of a product, beside the 6.29 TB/s copy rate of the box.  Beside them: one exact ``evaluate`` with gradient at the same N and
theta (sigma = 0.2).  No pass / fail threshold: the numbers are for DESIGN 3.18.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``TC_TIMEOUT`` seconds,
default 480), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, M = 10_000, 4, 10_000
REPEATS = 3
COPY_RATE = 6.29e12
PARTS = ("Sigma build", "B builds", "Choleskys", "SYMVs", "elementwise", "inverse", "trace pass")


def child():
    sys.path.insert(0, ROOT)
    import numpy as np

    from gumbi_amd.engine import Engine, KernelSpec, laplace_plan
    from oracle import gp_oracle as O

    trace = os.environ["GMB_TRACE_FILE"]
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, D))
    latent = 2.0 * np.sin(1.5 * X[:, 0]) + X[:, 1] - 0.5 * X[:, 2] * X[:, 3]
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-latent))).astype(float)
    spec = O.make_spec(D, range(D), kind="Matern52")
    theta = O.pack_theta(spec, [1.5, 2.0, 2.5, 2.5], 2.0, 0.0)
    theta_exact = O.pack_theta(spec, [1.5, 2.0, 2.5, 2.5], 2.0, 0.2)
    Xs = rng.standard_normal((M, D))
    ks = KernelSpec(D=D, idx_cont=list(range(D)), kind=spec["kind"], ard=True, jitter=spec["jitter"])

    def split():  # ({part: ms}, {part: count}) of the phases logged since the last call
        ms, cnt = dict.fromkeys(PARTS, 0.0), dict.fromkeys(PARTS, 0)
        with open(trace) as fh:
            for line in fh:
                f = line.split()
                if int(f[0]) == 22:
                    ms[PARTS[int(f[4])]] += float(f[5])
                    cnt[PARTS[int(f[4])]] += 1
        open(trace, "w").close()
        return ms, cnt

    def timed(call):
        call()  # allocations, code objects
        ts = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            call()
            ts.append(1e3 * (time.perf_counter() - t0))
        return np.median(ts), min(ts), max(ts)

    plan = laplace_plan(N)
    print(f"N={N} d={D} Matern-5/2 ARD, {int(y.sum())} labels 1, M={M} test points; medians of {REPEATS} calls after a warm-up; "
          f"{plan['nt']} block rows, {plan['slots']} slots, own buffers {plan['bytes_state'] / 2**20:.0f} MiB", flush=True)
    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(ks)
        t_eval = timed(lambda: eng.laplace_evaluate(theta, grad=True))
        t_nlq = timed(lambda: eng.laplace_evaluate(theta, grad=False))
        t_pred = timed(lambda: eng.laplace_predict(Xs))
        eng.set_profiling(True)
        split()
        val, grad = eng.laplace_evaluate(theta, grad=True)
        ms, cnt = split()
        eng.set_profiling(False)
        info = eng.laplace_info()
        print(f"  laplace_evaluate with gradient: {t_eval[0]:9.2f} ms (min {t_eval[1]:.2f}, max {t_eval[2]:.2f}); {info['iterations']} Newton "
              f"iterations, {info['halvings']} halvings", flush=True)
        print("   while profiling: " + ", ".join(f"{p} {ms[p]:.2f} ms / {cnt[p]}" for p in PARTS) + f" (sum {sum(ms.values()):.2f} ms)", flush=True)
        per = ms["SYMVs"] / max(cnt["SYMVs"], 1)
        rate = 8.0 * N * (N + 1) / 2 / (per * 1e-3)
        print(f"   one SYMV: {per:.3f} ms = {rate / 1e12:.2f} TB/s of the lower triangle, {rate / COPY_RATE:.2f} of the {COPY_RATE / 1e12:.2f} TB/s copy rate;"
              f" one Cholesky of B with its solves: {ms['Choleskys'] / max(cnt['Choleskys'], 1):.2f} ms", flush=True)
        print(f"  laplace_evaluate, objective only: {t_nlq[0]:9.2f} ms (min {t_nlq[1]:.2f}, max {t_nlq[2]:.2f})", flush=True)
        print(f"  laplace_predict of {M} points:   {t_pred[0]:9.2f} ms (min {t_pred[1]:.2f}, max {t_pred[2]:.2f})", flush=True)
        print(f"  -log q {val:.6f}, |grad| {np.linalg.norm(grad):.4e}, resident peak {eng.resident_bytes(peak=True) / 2**20:.0f} MiB", flush=True)
    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(ks)
        t = timed(lambda: eng.evaluate(theta_exact, grad=True))
        print(f" exact evaluate with gradient at N = {N}: {t[0]:.2f} ms (min {t[1]:.2f}, max {t[2]:.2f}), "
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
