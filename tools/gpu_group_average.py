"""Timing of ``gmb_predict_groups`` behind a fit's last evaluation, and of what a user had to do before it existed.

    python tools/gpu_group_average.py          the benchmark's N = 10,000 table (d = 4, ExpQuad-ARD: bench.py's C2)

Behind ``evaluate(theta, grad=True)`` (the tile path: U = L^-T and alpha resident, so V_A = A L^-T is one product).  Whole-call times
are the HIP-event time of the call on the engine's stream (``predict_ms`` of ``gmb_timings``), medians of ``REPEATS`` calls after a
warm-up of each, profiling off; host-side arithmetic is wall time.  Timed:

* the marginal-effect shape, G = 100 grid values x B = 1000 background rows (M = 10^5 points): ``gmb_predict_groups`` without and
  with ``cov`` -- the joint posterior of these points would need an 80 GB covariance and an 8 GB cross-covariance;
* G = 100 x B = 40 (M = 4000), where the old way still fits: ``gmb_predict_joint`` at the M points plus ``W C W^T`` on the host,
  beside the new call, and the difference of their results;
* from one further call of each with profiling on (``gmb_set_profiling`` + ``GMB_TRACE_FILE``): the pair rate of
  ``group_cov_partial_kernel`` (launch kind 18: flags 0 = the cross part A, M x Np pairs; 1 = the prior part Q, M x Mpad pairs;
  2 = Q's diagonal only) against the cross-covariance launch's of a prediction (kind 11, 128 x 128 pairs per tile).

No pass / fail threshold: the numbers are for DESIGN 3.14.

The parent process starts no GPU work itself: the measurement runs in a child under its own time limit (``TC_TIMEOUT`` seconds,
default 300), and nothing further is started after a child that did not end cleanly.
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 10_000, 4
REPEATS = 5
G = 100
B_LARGE, B_SMALL = 1000, 40


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

    def design(B):  # for every grid value of column 0, B background rows of the table with column 0 overwritten
        back = X[rng.choice(N, B, replace=False)]
        Xs = np.tile(back, (G, 1))
        Xs[:, 0] = np.repeat(np.linspace(X[:, 0].min(), X[:, 0].max(), G), B)
        return Xs, np.arange(G + 1, dtype=np.int64) * B

    def events():  # [(kind, mt, nt, flags, ms)] logged since the last call
        out = []
        with open(trace) as fh:
            for line in fh:
                f = line.split()
                out.append((int(f[0]), int(f[1]), int(f[2]), int(f[4]), float(f[5])))
        open(trace, "w").close()
        return out

    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(KernelSpec(D=D, idx_cont=list(range(D)), kind=spec["kind"], ard=True, jitter=spec["jitter"]))
        eng.evaluate(theta, grad=True)

        def timed(call):
            call()  # allocations, code objects
            ms, out = [], None
            for _ in range(REPEATS):
                out = call()
                ms.append(eng.timings()["predict_ms"])
            return float(np.median(ms)), min(ms), max(ms), out

        def line(label, t, extra=""):
            print(f"  {label:<58s} {t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}){extra}", flush=True)

        print(f"N={N} d={D} ExpQuad-ARD, behind evaluate(theta, grad=True); medians of {REPEATS} calls after a warm-up")
        eng.predict(X[:256])
        assert eng.timings()["predict_gemm_form"] == 1, "U is not resident: the evaluation did not take the tile path"

        Xl, off_l = design(B_LARGE)
        M = len(Xl)
        plain = timed(lambda: eng.predict_groups(Xl, off_l))
        line(f"gmb_predict_groups, G = {G} x B = {B_LARGE} (M = {M})", plain)
        full = timed(lambda: eng.predict_groups(Xl, off_l, cov=True))
        line(f"gmb_predict_groups, G = {G} x B = {B_LARGE} (M = {M}), with cov", full)
        print(f"    the joint posterior of these points: {8.0 * M * M / 1e9:.0f} GB of covariance, {8.0 * M * N / 1e9:.0f} GB of cross-covariance; "
              f"device memory the engine holds now: {eng.resident_bytes() / 1e9:.3f} GB")
        print(f"    var with cov against var without: max |diff| {float(np.max(np.abs(full[3][1] - plain[3][1]))):.2e}; "
              f"cov symmetric: {np.array_equal(full[3][2], full[3][2].T)}; smallest variance {float(plain[3][1].min()):.3e}")

        Xm, off_m = design(B_SMALL)
        Ms = len(Xm)
        small = timed(lambda: eng.predict_groups(Xm, off_m, cov=True))
        line(f"gmb_predict_groups, G = {G} x B = {B_SMALL} (M = {Ms}), with cov", small)
        W = np.zeros((G, Ms))
        for g in range(G):
            W[g, off_m[g]:off_m[g + 1]] = 1.0 / B_SMALL
        host_ms = []

        def old_way():
            mu, C = eng.predict_joint(Xm, with_noise=False, jitter=0.0)
            t0 = time.perf_counter()
            out = W @ mu, W @ C @ W.T
            host_ms.append(1e3 * (time.perf_counter() - t0))
            return out

        old = timed(old_way)
        host = float(np.median(host_ms[1:]))
        line(f"gmb_predict_joint at the M = {Ms} points", old, f"   + W C W^T on the host {host:.3f} ms (wall) = {old[0] + host:.3f} ms")
        print(f"    new call / old way: {small[0] / (old[0] + host):.3f}; results: mean {float(np.max(np.abs(small[3][0] - old[3][0]))):.2e}, "
              f"cov {float(np.max(np.abs(small[3][2] - old[3][1]))):.2e} (max |diff|)")

        # pair rates, from one call of each with profiling on
        eng.set_profiling(True)
        events()
        eng.predict_groups(Xl, off_l, cov=True)
        ev_full = events()
        eng.predict_groups(Xl, off_l)
        ev_diag = events()
        eng.predict(Xl[:16384])
        ev_pred = events()
        eng.set_profiling(False)
        names = {0: "A  (M x Np pairs)", 1: "Q  (M x Mpad pairs)", 2: "Q, diagonal only (sum |g|^2 pairs)"}
        for flags, evs in ((0, ev_full), (1, ev_full), (2, ev_diag)):
            sel = [e for e in evs if e[0] == 18 and e[3] == flags]
            ms = sum(e[4] for e in sel)
            # every launch covers mt column blocks of 64; over a reduction's launches the tasks cover each of the M points once
            pairs = float(G) * B_LARGE * B_LARGE if flags == 2 else 64.0 * sel[0][1] * M
            print(f"  group_cov_partial_kernel, {names[flags]:<36s} {len(sel)} launch(es), {ms:9.3f} ms while profiling, "
                  f"{pairs:.3e} pairs = {pairs / ms / 1e6:.1f} G pairs/s", flush=True)
        sel = [e for e in ev_pred if e[0] == 11]
        ms = sum(e[4] for e in sel)
        pairs = sum(16384.0 * e[1] * e[2] for e in sel)
        print(f"  cross-covariance launch of gmb_predict (kind 11), M = 16384   {len(sel)} launch(es), {ms:9.3f} ms while profiling, "
              f"{pairs:.3e} pairs = {pairs / ms / 1e6:.1f} G pairs/s (it also WRITES its M x Np doubles)", flush=True)


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
