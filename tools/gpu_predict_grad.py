"""Timing of ``gmb_predict_grad`` against its yardstick, the cross-covariance launch of a prediction at the same (M, N, d) -- the
same pair arithmetic plus an 8-byte store per pair.

    python tools/gpu_predict_grad.py [c2] [c3]        c2: N = 10,000 d = 4 ExpQuad;  c3: N = 50,000 d = 8 Matern-5/2;  M = 10^4

Per case: ``gmb_predict_grad`` behind ``factorize`` (first call: back substitution for alpha included; second call: alpha
resident) and behind ``evaluate(grad=True)`` (the fit's alpha), and ``gmb_predict``'s cross-covariance launch.  Every figure is a
HIP-event duration of the engine's profiling log (``gmb_set_profiling`` + ``GMB_TRACE_FILE``: launch kinds 11 = the prediction's
cross-covariance launch, 12 = predict_grad's partial + finishing launches, 13 = its back substitution); wall-clock times of the
calls are printed beside them.

The parent process starts no GPU work itself: each case runs in a child under its own time limit (``PG_TIMEOUT`` seconds,
default 420), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"c2": (10_000, 4, "ExpQuad"), "c3": (50_000, 8, "Matern52")}
M = 10_000


def child(name):
    sys.path.insert(0, ROOT)
    import numpy as np

    from gumbi_amd.engine import Engine, KernelSpec
    from oracle import gp_oracle as O

    N, d, kind = CASES[name]
    trace = os.environ["GMB_TRACE_FILE"]
    X, y, ls = O.synthetic_table(N, d)
    Xs = np.random.default_rng(0).standard_normal((M, d))
    spec = O.make_spec(d, range(d), kind=kind)
    theta = O.pack_theta(spec, ls, 1.0, 0.2)

    def events():  # {kind: [ms, ...]} logged since the last call
        out = {}
        with open(trace) as fh:
            for line in fh:
                f = line.split()
                out.setdefault(int(f[0]), []).append(float(f[5]))
        open(trace, "w").close()
        return out

    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return res, 1e3 * (time.perf_counter() - t0)

    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(KernelSpec(D=d, idx_cont=list(range(d)), kind=kind))
        eng.set_theta(theta)
        eng.factorize()
        eng.predict_grad(Xs[:256])  # allocations, code objects
        eng.predict(Xs[:256])
        eng.set_profiling(True)
        eng.factorize()
        events()
        G1, wall1 = timed(lambda: eng.predict_grad(Xs))
        ev1 = events()
        G2, wall2 = timed(lambda: eng.predict_grad(Xs))
        ev2 = events()
        _, wall_p = timed(lambda: eng.predict(Xs))
        cov = sum(events().get(11, []))
        eng.evaluate(theta, grad=True)
        events()
        G3, wall3 = timed(lambda: eng.predict_grad(Xs))
        ev3 = events()
    g1, bs = sum(ev1.get(12, [])), sum(ev1.get(13, []))
    g2, g3 = sum(ev2.get(12, [])), sum(ev3.get(12, []))
    assert not ev2.get(13) and not ev3.get(13), "alpha was solved for twice"
    agree = float(np.max(np.abs(G3 - G1)) / np.max(np.abs(G1)))
    print(f"{name}: N={N} d={d} {kind} M={M}")
    print(f"  cross-covariance launch of gmb_predict (yardstick)      {cov:8.3f} ms   (gmb_predict: {wall_p:.1f} ms wall)")
    print(f"  predict_grad behind factorize: launches                 {g1:8.3f} ms   ratio {g1 / cov:.2f}")
    print(f"                                 + back substitution      {bs:8.3f} ms   ratio {(g1 + bs) / cov:.2f}   ({wall1:.1f} ms wall)")
    print(f"                                 second call (alpha kept) {g2:8.3f} ms   ratio {g2 / cov:.2f}   ({wall2:.1f} ms wall)")
    print(f"  predict_grad behind evaluate(grad=True)                 {g3:8.3f} ms   ratio {g3 / cov:.2f}   ({wall3:.1f} ms wall)")
    print(f"  same bits on the second call: {G1.tobytes() == G2.tobytes()};  the two alphas agree to {agree:.1e}", flush=True)


def main():
    names = [a for a in sys.argv[1:] if a in CASES] or list(CASES)
    limit = os.environ.get("PG_TIMEOUT", "420")
    for name in names:
        with tempfile.NamedTemporaryFile(prefix="pg_trace_", suffix=".txt") as tf:
            env = dict(os.environ, GMB_TRACE_FILE=tf.name)
            rc = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--child", name], env=env).returncode
        if rc != 0:
            print(f"{name}: the child ended with status {rc}; nothing further is started")
            return rc
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main())
