"""Timing of ``gmb_predict_with_grad`` against its yardstick, ``gmb_predict`` at the same (M, N) on the same commit -- the call
runs that prediction (solve form) and adds one more triangular pass, W = V L^-1, and the fused gradient launch.

    python tools/gpu_predict_with_grad.py          N = 10,000 d = 4 ExpQuad;  M = 16 and M = 1024

Per M, behind ``factorize``: the whole call's HIP-event time (``predict_ms`` of ``gmb_timings``) for both calls, their ratio, and
the shares of the backward pass and of the fused launch from the engine's profiling log (``gmb_set_profiling`` +
``GMB_TRACE_FILE``: launch kinds 15 = the backward pass, 14 = the fused partial + finishing launches).  Whole-call times are
taken with profiling off (per-launch events serialise nothing here, but they are not free); the shares with it on.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``PG_TIMEOUT`` seconds,
default 300), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, KIND = 10_000, 4, "ExpQuad"
MS = (16, 1024)
REPEATS = 5


def child():
    sys.path.insert(0, ROOT)
    import numpy as np

    from gumbi_amd.engine import Engine, KernelSpec
    from oracle import gp_oracle as O

    trace = os.environ["GMB_TRACE_FILE"]
    X, y, ls = O.synthetic_table(N, D)
    spec = O.make_spec(D, range(D), kind=KIND)
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    rng = np.random.default_rng(0)

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
        eng.set_kernel(KernelSpec(D=D, idx_cont=list(range(D)), kind=KIND))
        eng.set_theta(theta)
        eng.factorize()
        print(f"N={N} d={D} {KIND}, behind factorize; median of {REPEATS} calls")
        for M in MS:
            Xs = rng.standard_normal((M, D))
            eng.predict_with_grad(Xs)  # allocations, code objects, alpha by back substitution
            eng.predict(Xs)
            t_p, t_g = [], []
            for _ in range(REPEATS):
                eng.predict(Xs)
                t_p.append(eng.timings()["predict_ms"])
                r1 = eng.predict_with_grad(Xs)
                t_g.append(eng.timings()["predict_ms"])
            eng.set_profiling(True)
            events()
            r2 = eng.predict_with_grad(Xs)
            ev = events()
            total = eng.timings()["predict_ms"]
            eng.set_profiling(False)
            back, fused = sum(ev.get(15, [])), sum(ev.get(14, []))
            p, g = float(np.median(t_p)), float(np.median(t_g))
            print(f"  M={M:5d}: gmb_predict {p:8.3f} ms   gmb_predict_with_grad {g:8.3f} ms   ratio {g / p:.2f}")
            print(f"           while profiling ({total:.3f} ms): backward pass {back:8.3f} ms ({back / total:.0%}), "
                  f"fused launch {fused:8.3f} ms ({fused / total:.0%})")
            print(f"           same bits call after call: {all(a.tobytes() == b.tobytes() for a, b in zip(r1, r2))}", flush=True)


def main():
    limit = os.environ.get("PG_TIMEOUT", "300")
    with tempfile.NamedTemporaryFile(prefix="pvg_trace_", suffix=".txt") as tf:
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
